// USLAM::Initializer (include/Initializer.h, src/Initializer.cc) over the C ABI (uvo_initializer_* in uvo/uvo.h), for the two places the
// reference uses it: Tracking::Initialize, src/Tracking.cc:1340, and the recovery path, :1582.
//
//     - mpInitializer = new Initializer(mInitialFrame,1.0,200);
//     + mpInitializer = new USLAM::Initializer(initDevice,mInitialFrame,1.0,200);      // initDevice: a USLAM::InitializerDevice
//       ...
//       if(mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated))   // unchanged
//
// Only the F path exists, which is all the reference's Initialize executes (src/Initializer.cc:110; see uvo/uvo.h): there is no
// FindHomography, ReconstructH or Re_CheckRT here.  The frame type needs mK (3 x 3 CV_32F) and mvKeysUn (cv::KeyPoint layout).  The
// random stream: the reference draws from libc's rand(), never seeded, the stream PnPsolver and Sim3Solver consume too; the device
// object owns the restated generator (srand(1) at construction, or hand it the state the process's other solvers share) and every
// Initialize call advances it by exactly the 8 x iterations draws the reference would have made.  When the call does not initialise,
// R21 and t21 come back empty and vP3D / vbTriangulated are left alone, as in the reference.  Fewer than 8 matches, or no hypothesis
// scoring above 0 (where the reference's behaviour is undefined), return false.  Needs <opencv2/core/core.hpp> for cv::Mat and
// cv::Point3f in the signature; header only, C++11.
#ifndef UVO_COMPAT_INITIALIZER_H_
#define UVO_COMPAT_INITIALIZER_H_
#include <opencv2/core/core.hpp>
#include <vector>

#include "uvo/uvo.h"

namespace USLAM {

// the device object every Initializer of a tracker runs on, and the generator state (the process-wide rand() of the reference)
class InitializerDevice {
 public:
  InitializerDevice(uvo_klt* klt, int max_keys) : h_(0) {
    uvo_initializer_create(klt, max_keys, &h_);
    uvo_glibc_srand(&rng_, 1);
  }
  ~InitializerDevice() { uvo_initializer_destroy(h_); }
  bool ok() const { return h_ != 0; }
  uvo_initializer* handle() { return h_; }
  uvo_glibc_rand* rng() { return &rng_; }

 private:
  InitializerDevice(const InitializerDevice&);
  InitializerDevice& operator=(const InitializerDevice&);
  uvo_initializer* h_;
  uvo_glibc_rand rng_;
};

class Initializer {
 public:
  // Initializer::Initializer(ReferenceFrame, sigma, iterations), :33-42
  template <class Frame>
  Initializer(InitializerDevice& device, const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200)
      : dev_(&device), sigma_(sigma), iterations_(iterations) {
    cam_ = uvo_camera_model();
    cam_.fx = ReferenceFrame.mK.template at<float>(0, 0), cam_.fy = ReferenceFrame.mK.template at<float>(1, 1);
    cam_.cx = ReferenceFrame.mK.template at<float>(0, 2), cam_.cy = ReferenceFrame.mK.template at<float>(1, 2);
    keys(ReferenceFrame, keys1_);
  }

  // Initializer::Initialize, :44-113
  template <class Frame>
  bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                  std::vector<bool>& vbTriangulated) {
    R21 = cv::Mat();
    t21 = cv::Mat();
    if (!dev_->ok() || keys1_.empty()) return false;
    // the object may be shared by several Initializers (the recovery path builds a new one): the reference goes with every call
    if (uvo_initializer_set_reference(dev_->handle(), &keys1_[0], (int)(keys1_.size() / 2), &cam_, sigma_, iterations_) != UVO_OK) return false;
    std::vector<float> keys2;
    keys(CurrentFrame, keys2);
    const int n2 = (int)vMatches12.size();
    if ((size_t)n2 != keys2.size() / 2) return false;  // :51-59: one entry per current key
    std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
    std::vector<uint8_t> tri(n2 > 0 ? n2 : 1);
    std::vector<float> p3d(n2 > 0 ? 3 * (size_t)n2 : 3);
    last_ = uvo_initializer_result();
    last_.p3d = &p3d[0], last_.triangulated = &tri[0];
    const int rc = uvo_initializer_initialize(dev_->handle(), n2 ? &keys2[0] : 0, n2, n2 ? &m12[0] : 0, dev_->rng(), &last_);
    last_.p3d = 0, last_.triangulated = 0;
    if (rc != UVO_OK || !last_.initialized) return false;
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R21.at<float>(r, c) = last_.R21[3 * r + c];
      t21.at<float>(r) = last_.t21[r];
    }
    vP3D.resize(n2);
    vbTriangulated.assign(n2, false);
    for (int i = 0; i < n2; ++i) {
      vP3D[i].x = p3d[3 * i], vP3D[i].y = p3d[3 * i + 1], vP3D[i].z = p3d[3 * i + 2];
      vbTriangulated[i] = tri[i] != 0;
    }
    return true;
  }

  // what the last Initialize call found besides its return value (scores, counts, parallaxes; the buffer pointers are null)
  const uvo_initializer_result& last() const { return last_; }

 private:
  template <class Frame>
  static void keys(const Frame& F, std::vector<float>& out) {
    out.resize(2 * F.mvKeysUn.size());
    for (size_t i = 0; i < F.mvKeysUn.size(); ++i) out[2 * i] = F.mvKeysUn[i].pt.x, out[2 * i + 1] = F.mvKeysUn[i].pt.y;
  }
  InitializerDevice* dev_;
  float sigma_;
  int iterations_;
  uvo_camera_model cam_;
  std::vector<float> keys1_;
  uvo_initializer_result last_;
};

}  // namespace USLAM
#endif  // UVO_COMPAT_INITIALIZER_H_
