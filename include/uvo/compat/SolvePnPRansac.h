// cv::solvePnPRansac(objectPoints, imagePoints, K, distCoeffs, rvec, tvec, useExtrinsicGuess, iterationsCount, reprojectionError,
// confidence, inliers, cv::SOLVEPNP_EPNP) for the call site in Tracking::TrackWithPnP (src/Tracking.cc:1864), over the tracker handle
// the front-end already owns:
//
//     - cv::solvePnPRansac(mappts, pts, mK, mDistCoef, Rvec, Tvec, false, 300, 3, 0.99, mask_pnp, cv::SOLVEPNP_EPNP);
//     + std::vector<int> inl;  float Tcw[16];
//     + bool ok = USLAM::solvePnPRansac(klt, mappts, pts, cam, Rvec, Tvec, false, 300, 3, 0.99, inl, Tcw);
//
// mappts / pts are std::vector<cv::Point3f> / std::vector<cv::Point2f> (any types with that layout); `inl` holds point indices,
// ascending, as OpenCV's inlier output does; Tcw (optional) is the float 4 x 4 that :1874-1878 builds from Rvec / Tvec.  Semantics and
// contract: uvo_klt_solve_pnp_ransac in uvo/uvo.h.  Header only, C++11, no OpenCV.
#ifndef UVO_COMPAT_SOLVEPNPRANSAC_H_
#define UVO_COMPAT_SOLVEPNPRANSAC_H_
#include <vector>

#include "uvo/uvo.h"

namespace USLAM {

template <class Point3, class Point2>
inline bool solvePnPRansac(uvo_klt* klt, const std::vector<Point3>& objectPoints, const std::vector<Point2>& imagePoints, const uvo_camera_model& cam,
                           double* rvec, double* tvec, bool useExtrinsicGuess, int iterationsCount, float reprojectionError, double confidence,
                           std::vector<int>& inliers, float* Tcw = 0) {
  static_assert(sizeof(Point3) == 3 * sizeof(float) && sizeof(Point2) == 2 * sizeof(float), "Point3f / Point2f layout expected");
  inliers.clear();
  if (useExtrinsicGuess || objectPoints.size() != imagePoints.size()) return false;  // EPnP takes no initial guess (the call site passes false)
  const int n = (int)objectPoints.size();
  std::vector<int32_t> idx(n > 0 ? n : 1);
  uvo_pnp_info info;
  const int rc = uvo_klt_solve_pnp_ransac(klt, n ? reinterpret_cast<const float*>(&objectPoints[0]) : 0, n ? reinterpret_cast<const float*>(&imagePoints[0]) : 0,
                                          n, &cam, iterationsCount, (double)reprojectionError, confidence, rvec, tvec, Tcw, &idx[0], &info);
  if (rc != UVO_OK || !info.ok) return false;
  inliers.assign(idx.begin(), idx.begin() + info.inliers);
  return true;
}

}  // namespace USLAM
#endif  // UVO_COMPAT_SOLVEPNPRANSAC_H_
