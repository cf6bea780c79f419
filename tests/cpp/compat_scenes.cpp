// Scene-driven driver of the compat adaptors (include/uvo/compat/): reads a scene written by tests/test_gpu_compat_adaptors.py, runs
// its list of calls through USLAM::ORBmatcher / USLAM::ORBextractor / USLAM::Grider_FAST, and dumps every result and the map state.
// The stand-ins below BEHAVE like the reference's classes where the adaptors can observe it: MapPoint::Replace moves observations
// and recomputes the target's descriptor (src/MapPoint.cc:132-170, :214-260), KeyFrame::GetMapPoints skips NULL and bad slots, ...
//
// Scene file, little-endian, read in this order (i32 = int32, f32 = float, u8 = uint8; "kp" = one 28-byte cv::KeyPoint record):
//   i32 magic 0x43535655 ("UVSC"), i32 version 1
//   i32 nkf, then per key frame:
//     i32 N, nlevels; f32 fx, fy, cx, cy; i32 mnMinX, mnMinY, mnMaxX, mnMaxY; f32 scale[nlevels], sigma2[nlevels];
//     f32 Rcw[9] (row-major), tcw[3], Ow[3]; kp keysUn[N]; u8 desc[N][32]; i32 slot[N] (map-point id or -1); featvec
//   featvec: i32 nnodes, then per node: u32 node id, i32 count, i32 feature[count]
//   i32 nmp, then per map point (id = its index):
//     f32 pos[3], normal[3], mfMinDistance, mfMaxDistance; u8 desc[32]; i32 bad;
//     i32 mbTrackInView, mnTrackScaleLevel; f32 mTrackViewCos, mTrackProjX, mTrackProjY
//   i32 nframes, then per frame:
//     i32 N, nlevels; f32 fx, fy, cx, cy, mnMinX, mnMinY, mnMaxX, mnMaxY; f32 scale[nlevels]; f32 Tcw[16] (row-major 4x4);
//     kp mvKeys[N]; kp mvKeysUn[N]; u8 desc[N][32]; i32 mvpMapPoints[N] (id or -1); u8 mvbOutlier[N]; featvec
//   i32 nimages, then per image: i32 width, height, stride; u8 pixels[height * stride]
//   i32 ncalls, then per call: i32 op; i32 ni, i32 iarg[ni]; i32 nf, f32 farg[nf]; i32 nlists, then per list: i32 len, i32 v[len]
// Observations are derived from the key-frame slots: a slot k of key frame f holding a point that is not bad is the observation (f, k).
//
// Dump (text, one record per line): "call <index> <op> <return value>", then "v <name> <values...>" for every output vector (map
// points as ids, -1 = NULL; key points and descriptors as hex of their raw bytes).  After a call that can change the map:
// "kf <f> <slot ids...>" for every key frame and "mp <id> <bad> <replaced id> <n> <f:k>... <descriptor hex>" for every point.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "uvo/compat/Grider_FAST.h"
#include "uvo/compat/ORBextractor.h"
#include "uvo/compat/ORBmatcher.h"

namespace {

struct Mat {  // cv::Mat CV_32F stand-in (3x1, 3x3, 4x4): at<float>(r, c) and at<float>(r) like a column vector
  int cols = 1;
  std::vector<float> v;
  template <class T>
  T at(int r, int c) const { return v[(size_t)r * cols + c]; }
  template <class T>
  T at(int r) const { return v[(size_t)r * cols]; }
};
Mat make_mat(const float* p, int rows, int cols) {
  Mat m;
  m.cols = cols, m.v.assign(p, p + rows * cols);
  return m;
}
struct DescRow {  // the row a GetDescriptor() returns
  const uint8_t* p;
  const uint8_t* ptr(int) const { return p; }
};
struct DescRows {  // a frame's mDescriptors
  std::vector<uint8_t> d;
  const uint8_t* ptr(int i) const { return &d[(size_t)i * 32]; }
};
struct Point2f {
  float x, y;
};
typedef std::map<unsigned, std::vector<unsigned> > FeatureVector;

struct KeyFrame;
int desc_distance(const uint8_t* a, const uint8_t* b) { return USLAM::ORBmatcher::DescriptorDistance(a, b); }

struct MapPoint {
  long unsigned int mnId = 0;
  float pos[3], normal[3], mfMinDistance = 1.f, mfMaxDistance = 1.f;
  std::vector<uint8_t> desc;
  bool mbBad = false;
  MapPoint* mpReplaced = nullptr;
  std::map<KeyFrame*, size_t> mObservations;
  // the tracking fields SearchByProjection(F, vpMapPoints, th) reads (set by isInFrustum in the reference)
  bool mbTrackInView = false;
  int mnTrackScaleLevel = 0;
  float mTrackViewCos = 0.f, mTrackProjX = 0.f, mTrackProjY = 0.f;

  bool isBad() const { return mbBad; }
  Mat GetWorldPos() const { return make_mat(pos, 3, 1); }
  Mat GetNormal() const { return make_mat(normal, 3, 1); }
  float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
  DescRow GetDescriptor() const { return DescRow{desc.data()}; }
  bool IsInKeyFrame(KeyFrame* pKF) const { return mObservations.count(pKF) != 0; }
  int GetIndexInKeyFrame(KeyFrame* pKF) const {
    auto it = mObservations.find(pKF);
    return it == mObservations.end() ? -1 : (int)it->second;
  }
  void AddObservation(KeyFrame* pKF, size_t idx) {
    if (!mObservations.count(pKF)) mObservations[pKF] = idx;
  }
  void Replace(MapPoint* pMP);               // src/MapPoint.cc:132-170
  void ComputeDistinctiveDescriptors();      // src/MapPoint.cc:214-260
};

struct KeyFrame {
  int N = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
  std::vector<float> scale, sigma2;
  float R[9], t[3], ow[3];
  std::vector<uvo_keypoint> keys;
  std::vector<uint8_t> desc;
  std::vector<MapPoint*> mvpMapPoints;
  FeatureVector featvec;

  bool isBad() const { return false; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
  std::set<MapPoint*> GetMapPoints() const {  // src/KeyFrame.cc: skips NULL and bad slots
    std::set<MapPoint*> s;
    for (MapPoint* p : mvpMapPoints)
      if (p && !p->isBad()) s.insert(p);
    return s;
  }
  MapPoint* GetMapPoint(size_t i) const { return mvpMapPoints[i]; }
  void AddMapPoint(MapPoint* p, size_t i) { mvpMapPoints[i] = p; }
  void ReplaceMapPointMatch(size_t i, MapPoint* p) { mvpMapPoints[i] = p; }
  void EraseMapPointMatch(size_t i) { mvpMapPoints[i] = nullptr; }
  std::vector<uvo_keypoint> GetKeyPointsUn() const { return keys; }
  uvo_keypoint GetKeyPointUn(size_t i) const { return keys[i]; }
  DescRow GetDescriptor(size_t i) const { return DescRow{&desc[i * 32]}; }
  const FeatureVector& GetFeatureVector() const { return featvec; }
  int GetScaleLevels() const { return (int)scale.size(); }
  float GetSigma2(int l) const { return sigma2[l]; }
  std::vector<float> GetScaleFactors() const { return scale; }
  Mat GetRotation() const { return make_mat(R, 3, 3); }
  Mat GetTranslation() const { return make_mat(t, 3, 1); }
  Mat GetCameraCenter() const { return make_mat(ow, 3, 1); }
};

void MapPoint::Replace(MapPoint* pMP) {
  if (pMP->mnId == mnId) return;
  std::map<KeyFrame*, size_t> obs = mObservations;
  mObservations.clear();
  mbBad = true;
  mpReplaced = pMP;
  for (auto& o : obs) {
    KeyFrame* pKF = o.first;
    if (!pMP->IsInKeyFrame(pKF)) {
      pKF->ReplaceMapPointMatch(o.second, pMP);
      pMP->AddObservation(pKF, o.second);
    } else {
      pKF->EraseMapPointMatch(o.second);
    }
  }
  pMP->ComputeDistinctiveDescriptors();
}

void MapPoint::ComputeDistinctiveDescriptors() {
  if (mbBad || mObservations.empty()) return;
  std::vector<const uint8_t*> d;
  for (auto& o : mObservations)
    if (!o.first->isBad()) d.push_back(o.first->GetDescriptor(o.second).ptr(0));
  if (d.empty()) return;
  const size_t n = d.size();
  int best_median = INT_MAX;
  size_t best = 0;
  for (size_t i = 0; i < n; ++i) {
    std::vector<int> row(n);
    for (size_t j = 0; j < n; ++j) row[j] = i == j ? 0 : desc_distance(d[i], d[j]);
    std::sort(row.begin(), row.end());
    const int median = row[(size_t)(0.5 * (n - 1))];
    if (median < best_median) best_median = median, best = i;
  }
  desc.assign(d[best], d[best] + 32);
}

struct Frame {
  std::vector<uvo_keypoint> mvKeys, mvKeysUn;
  DescRows mDescriptors;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<float> mvScaleFactors;
  FeatureVector mFeatVec;
  Mat mTcw;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
};

struct Image {
  int w = 0, h = 0, stride = 0;
  std::vector<uint8_t> px;
};

struct Call {
  int op;
  std::vector<int> i;
  std::vector<float> f;
  std::vector<std::vector<int> > l;
};

// ---- reading ----
struct Reader {
  std::vector<uint8_t> buf;
  size_t at = 0;
  void get(void* p, size_t n) {
    if (at + n > buf.size()) {
      fprintf(stderr, "scene truncated at byte %zu\n", at);
      exit(2);
    }
    memcpy(p, &buf[at], n);
    at += n;
  }
  int i32() {
    int v;
    get(&v, 4);
    return v;
  }
  float f32() {
    float v;
    get(&v, 4);
    return v;
  }
  template <class T>
  void vec(std::vector<T>& v, size_t n) {
    v.resize(n);
    if (n) get(v.data(), n * sizeof(T));
  }
  void featvec(FeatureVector& fv) {
    const int nn = i32();
    for (int k = 0; k < nn; ++k) {
      unsigned id;
      get(&id, 4);
      std::vector<int> f;
      vec(f, i32());
      fv[id].assign(f.begin(), f.end());
    }
  }
};

struct Scene {
  std::vector<KeyFrame> kfs;  // one array: std::map<KeyFrame*, ...> then orders observations by key-frame index
  std::vector<std::unique_ptr<MapPoint> > mps;
  std::vector<Frame> frames;
  std::vector<Image> images;
  std::vector<Call> calls;
  MapPoint* mp(int id) const { return id < 0 ? nullptr : mps[id].get(); }
  int id(const MapPoint* p) const { return p ? (int)p->mnId : -1; }
};

void read_scene(const char* path, Scene& S) {
  Reader r;
  FILE* fp = fopen(path, "rb");
  if (!fp) exit(2);
  fseek(fp, 0, SEEK_END);
  r.buf.resize(ftell(fp));
  fseek(fp, 0, SEEK_SET);
  if (fread(r.buf.data(), 1, r.buf.size(), fp) != r.buf.size()) exit(2);
  fclose(fp);
  if (r.i32() != 0x43535655 || r.i32() != 1) exit(2);
  std::vector<std::vector<int> > slots(r.i32());
  S.kfs.resize(slots.size());
  for (size_t f = 0; f < slots.size(); ++f) {
    KeyFrame& K = S.kfs[f];
    K.N = r.i32();
    const int nl = r.i32();
    K.fx = r.f32(), K.fy = r.f32(), K.cx = r.f32(), K.cy = r.f32();
    K.mnMinX = r.i32(), K.mnMinY = r.i32(), K.mnMaxX = r.i32(), K.mnMaxY = r.i32();
    r.vec(K.scale, nl), r.vec(K.sigma2, nl);
    r.get(K.R, 36), r.get(K.t, 12), r.get(K.ow, 12);
    r.vec(K.keys, K.N), r.vec(K.desc, (size_t)K.N * 32), r.vec(slots[f], K.N);
    r.featvec(K.featvec);
  }
  const int nmp = r.i32();
  for (int i = 0; i < nmp; ++i) {
    S.mps.emplace_back(new MapPoint);
    MapPoint& P = *S.mps.back();
    P.mnId = i;
    r.get(P.pos, 12), r.get(P.normal, 12);
    P.mfMinDistance = r.f32(), P.mfMaxDistance = r.f32();
    r.vec(P.desc, 32);
    P.mbBad = r.i32() != 0;
    P.mbTrackInView = r.i32() != 0, P.mnTrackScaleLevel = r.i32();
    P.mTrackViewCos = r.f32(), P.mTrackProjX = r.f32(), P.mTrackProjY = r.f32();
  }
  for (size_t f = 0; f < slots.size(); ++f) {
    KeyFrame* K = &S.kfs[f];
    K->mvpMapPoints.resize(K->N);
    for (int k = 0; k < K->N; ++k) {
      MapPoint* p = S.mp(slots[f][k]);
      K->mvpMapPoints[k] = p;
      if (p && !p->isBad()) p->AddObservation(K, k);
    }
  }
  S.frames.resize(r.i32());
  for (Frame& F : S.frames) {
    const int n = r.i32(), nl = r.i32();
    F.fx = r.f32(), F.fy = r.f32(), F.cx = r.f32(), F.cy = r.f32();
    F.mnMinX = r.f32(), F.mnMinY = r.f32(), F.mnMaxX = r.f32(), F.mnMaxY = r.f32();
    r.vec(F.mvScaleFactors, nl);
    float T[16];
    r.get(T, 64);
    F.mTcw = make_mat(T, 4, 4);
    r.vec(F.mvKeys, n), r.vec(F.mvKeysUn, n), r.vec(F.mDescriptors.d, (size_t)n * 32);
    std::vector<int> ids;
    std::vector<uint8_t> outl;
    r.vec(ids, n), r.vec(outl, n);
    for (int k = 0; k < n; ++k) F.mvpMapPoints.push_back(S.mp(ids[k])), F.mvbOutlier.push_back(outl[k] != 0);
    r.featvec(F.mFeatVec);
  }
  S.images.resize(r.i32());
  for (Image& I : S.images) {
    I.w = r.i32(), I.h = r.i32(), I.stride = r.i32();
    r.vec(I.px, (size_t)I.h * I.stride);
  }
  S.calls.resize(r.i32());
  for (Call& c : S.calls) {
    c.op = r.i32();
    r.vec(c.i, r.i32());
    r.vec(c.f, r.i32());
    c.l.resize(r.i32());
    for (auto& l : c.l) r.vec(l, r.i32());
  }
  if (r.at != r.buf.size()) {
    fprintf(stderr, "trailing bytes in scene\n");
    exit(2);
  }
}

// ---- dumping ----
FILE* out = nullptr;
void dump_ids(const Scene& S, const char* name, const std::vector<MapPoint*>& v) {
  fprintf(out, "v %s", name);
  for (MapPoint* p : v) fprintf(out, " %d", S.id(p));
  fputc('\n', out);
}
void dump_ints(const char* name, const std::vector<int>& v) {
  fprintf(out, "v %s", name);
  for (int x : v) fprintf(out, " %d", x);
  fputc('\n', out);
}
void dump_hex(const char* name, const void* p, size_t n) {
  fprintf(out, "v %s ", name);
  for (size_t k = 0; k < n; ++k) fprintf(out, "%02x", ((const uint8_t*)p)[k]);
  fputc('\n', out);
}
void dump_map(const Scene& S) {
  for (size_t f = 0; f < S.kfs.size(); ++f) {
    fprintf(out, "kf %zu", f);
    for (MapPoint* p : S.kfs[f].mvpMapPoints) fprintf(out, " %d", S.id(p));
    fputc('\n', out);
  }
  std::map<const KeyFrame*, int> kfi;
  for (size_t f = 0; f < S.kfs.size(); ++f) kfi[&S.kfs[f]] = (int)f;
  for (auto& P : S.mps) {
    std::vector<std::pair<int, int> > obs;
    for (auto& o : P->mObservations) obs.push_back(std::make_pair(kfi[o.first], (int)o.second));
    std::sort(obs.begin(), obs.end());
    fprintf(out, "mp %lu %d %d %zu", P->mnId, (int)P->mbBad, S.id(P->mpReplaced), obs.size());
    for (auto& o : obs) fprintf(out, " %d:%d", o.first, o.second);
    fputc(' ', out);
    for (int k = 0; k < 32; ++k) fprintf(out, "%02x", P->desc[k]);
    fputc('\n', out);
  }
}

enum Op {
  OP_MATCHER = 0,           // f: nnratio; i: checkOri                               -- a new USLAM::ORBmatcher for the calls that follow
  OP_SBP_LOCAL = 1,         // i: frame; f: th; l0: map points                       SearchByProjection(F, vpMapPoints, th)
  OP_SBP_KF = 2,            // i: frame, kf, ORBdist; f: th; l0: sAlreadyFound       SearchByProjection(F, pKF, sAlreadyFound, th, ORBdist)
  OP_BOW_KF_FRAME = 3,      // i: kf, frame                                          SearchByBoW(pKF, F, vpMapPointMatches)
  OP_BOW_KF_KF = 4,         // i: kf1, kf2                                           SearchByBoW(pKF1, pKF2, vpMatches12)
  OP_TRIANG = 5,            // i: kf1, kf2; f: F12[9]                                SearchForTriangulation
  OP_FUSE = 6,              // i: kf; f: th; l0: map points (-1 = NULL)              Fuse(pKF, vpMapPoints, th)
  OP_TRI_BEGIN = 7,         // i: kf1; l0: kf2 list; f: F12[9] per kf2               SearchForTriangulationBegin
  OP_TRI_NEXT = 8,          // i: kf1, kf2, k, create                                SearchForTriangulationNext, then the map-point rule
  OP_FUSE_TARGETS = 9,      // l0: target kfs; l1: map points; f: th                 FuseTargets
  OP_SBP_SCW = 10,          // i: kf, th; f: Scw[16]; l0: points; l1: vpMatched      SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
  OP_FUSE_SCW = 11,         // i: kf; f: Scw[16], th; l0: points                     Fuse(pKF, Scw, vpPoints, th)
  OP_SIM3 = 12,             // i: kf1, kf2; f: s12, R12[9], t12[3], th; l0: vpMatches12   SearchBySim3
  OP_WINDOW = 13,           // i: f1, f2, window, [minLevel, maxLevel]               WindowSearch
  OP_SBP_FRAMES = 14,       // i: f1, f2, window                                     SearchByProjection(F1, F2, windowSize, vpMapPointMatches2)
  OP_INIT = 15,             // i: f1, f2, window; f: vbPrevMatched (x, y) per key point of f1    SearchForInitialization
  OP_SBP_LAST = 16,         // i: current frame, last frame; f: th                   SearchByProjection(CurrentFrame, LastFrame, th)
  OP_EXTRACTOR = 17,        // i: nfeatures, nlevels, fastTh; f: scaleFactor          -- a new USLAM::ORBextractor
  OP_EXTRACT = 18,          // i: image (-1 = empty), width, height, stride, min_px, FullDetect, need, grid rows, grid cols;
                            //    l0: caller key points (7 words each); l1: grid (column-major)
  OP_GRIDER = 19,           // i: image, num_features, grid_x, grid_y, threshold, nms  Grider_FAST::perform_griding (appends to 3 canaries)
};

// the map-point creation rule between two SearchForTriangulationNext calls (stands in for the triangulation of
// src/LocalMapping.cc:1082-1180): every matched pair (i1, i2) with i1 % 3 == 0 gets a new map point observed by key frame 1 at i1
// and key frame 2 at i2; its descriptor is key frame 1's at i1.
void create_points(Scene& S, KeyFrame* K1, KeyFrame* K2, const std::vector<std::pair<size_t, size_t> >& pairs) {
  for (auto& pr : pairs) {
    if (pr.first % 3 != 0) continue;
    S.mps.emplace_back(new MapPoint);
    MapPoint* P = S.mps.back().get();
    P->mnId = S.mps.size() - 1;
    memset(P->pos, 0, 12), memset(P->normal, 0, 12);
    P->desc.assign(K1->desc.begin() + pr.first * 32, K1->desc.begin() + pr.first * 32 + 32);
    P->AddObservation(K1, pr.first), P->AddObservation(K2, pr.second);
    K1->AddMapPoint(P, pr.first), K2->AddMapPoint(P, pr.second);
  }
}

const std::vector<int>& list(const Call& c, size_t k) {  // list k of a call, empty when the call has fewer
  static const std::vector<int> none;
  return k < c.l.size() ? c.l[k] : none;
}
std::vector<MapPoint*> points(const Scene& S, const std::vector<int>& ids) {
  std::vector<MapPoint*> v;
  for (int i : ids) v.push_back(S.mp(i));
  return v;
}
KeyFrame* kf(Scene& S, int i) { return &S.kfs[i]; }
std::vector<KeyFrame*> keyframes(Scene& S, const std::vector<int>& ids) {
  std::vector<KeyFrame*> v;
  for (int i : ids) v.push_back(&S.kfs[i]);
  return v;
}

int run(Scene& S) {
  std::unique_ptr<USLAM::ORBmatcher> m;
  std::unique_ptr<USLAM::ORBextractor> ex;
  for (size_t ci = 0; ci < S.calls.size(); ++ci) {
    const Call& c = S.calls[ci];
    const std::vector<int>& I = c.i;
    int ret = 0;
    bool map_changed = false;
    std::string err;
    const std::string err_before = m ? m->last_error() : std::string();
    fprintf(out, "call %zu %d ", ci, c.op);
    switch (c.op) {
      case OP_MATCHER:
        m.reset(new USLAM::ORBmatcher(c.f[0], I[0] != 0));
        fprintf(out, "0\n");
        continue;
      case OP_SBP_LOCAL: {
        Frame& F = S.frames[I[0]];
        ret = m->SearchByProjection(F, points(S, c.l[0]), c.f[0]);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "frame", F.mvpMapPoints);
        break;
      }
      case OP_SBP_KF: {
        Frame& F = S.frames[I[0]];
        std::vector<MapPoint*> found = points(S, c.l[0]);
        ret = m->SearchByProjection(F, kf(S, I[1]), std::set<MapPoint*>(found.begin(), found.end()), c.f[0], I[2]);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "frame", F.mvpMapPoints);
        break;
      }
      case OP_BOW_KF_FRAME: {
        std::vector<MapPoint*> v(3, S.mp(0));  // stale content: the member must reset it
        ret = m->SearchByBoW(kf(S, I[0]), S.frames[I[1]], v);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "matches", v);
        break;
      }
      case OP_BOW_KF_KF: {
        std::vector<MapPoint*> v(3, S.mp(0));
        ret = m->SearchByBoW(kf(S, I[0]), kf(S, I[1]), v);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "matches", v);
        break;
      }
      case OP_TRIANG: {
        std::vector<uvo_keypoint> k1, k2;
        std::vector<std::pair<size_t, size_t> > pairs;
        ret = m->SearchForTriangulation(kf(S, I[0]), kf(S, I[1]), make_mat(c.f.data(), 3, 3), k1, k2, pairs);
        fprintf(out, "%d\n", ret);
        std::vector<int> p;
        for (auto& x : pairs) p.push_back((int)x.first), p.push_back((int)x.second);
        dump_ints("pairs", p);
        dump_hex("keys1", k1.data(), k1.size() * sizeof(uvo_keypoint));
        dump_hex("keys2", k2.data(), k2.size() * sizeof(uvo_keypoint));
        break;
      }
      case OP_FUSE: {
        std::vector<MapPoint*> v = points(S, c.l[0]);
        ret = m->Fuse(kf(S, I[0]), v, c.f[0]);
        fprintf(out, "%d\n", ret);
        map_changed = true;
        break;
      }
      case OP_TRI_BEGIN: {
        std::vector<Mat> f12;
        for (size_t k = 0; k < c.l[0].size(); ++k) f12.push_back(make_mat(&c.f[9 * k], 3, 3));
        ret = m->SearchForTriangulationBegin(kf(S, I[0]), keyframes(S, c.l[0]), f12);
        fprintf(out, "%d\n", ret);
        break;
      }
      case OP_TRI_NEXT: {
        std::vector<uvo_keypoint> k1, k2;
        std::vector<std::pair<size_t, size_t> > pairs;
        KeyFrame *K1 = kf(S, I[0]), *K2 = kf(S, I[1]);
        ret = m->SearchForTriangulationNext(K1, K2, I[2], k1, k2, pairs);
        fprintf(out, "%d\n", ret);
        std::vector<int> p;
        for (auto& x : pairs) p.push_back((int)x.first), p.push_back((int)x.second);
        dump_ints("pairs", p);
        dump_hex("keys2", k2.data(), k2.size() * sizeof(uvo_keypoint));
        if (I[3]) create_points(S, K1, K2, pairs);
        map_changed = true;
        break;
      }
      case OP_FUSE_TARGETS: {
        std::vector<MapPoint*> v = points(S, c.l[1]);
        ret = m->FuseTargets(keyframes(S, c.l[0]), v, c.f[0]);
        fprintf(out, "%d\n", ret);
        map_changed = true;
        break;
      }
      case OP_SBP_SCW: {
        std::vector<MapPoint*> matched = points(S, c.l[1]);
        ret = m->SearchByProjection(kf(S, I[0]), make_mat(c.f.data(), 4, 4), points(S, c.l[0]), matched, I[1]);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "matched", matched);
        break;
      }
      case OP_FUSE_SCW:
        ret = m->Fuse(kf(S, I[0]), make_mat(c.f.data(), 4, 4), points(S, c.l[0]), c.f[16]);
        fprintf(out, "%d\n", ret);
        map_changed = true;
        break;
      case OP_SIM3: {
        std::vector<MapPoint*> v = points(S, c.l[0]);
        const float s12 = c.f[0];
        ret = m->SearchBySim3(kf(S, I[0]), kf(S, I[1]), v, s12, make_mat(&c.f[1], 3, 3), make_mat(&c.f[10], 3, 1), c.f[13]);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "matches", v);
        break;
      }
      case OP_WINDOW: {
        std::vector<MapPoint*> v;
        if (I.size() > 3)
          ret = m->WindowSearch(S.frames[I[0]], S.frames[I[1]], I[2], v, I[3], I[4]);
        else
          ret = m->WindowSearch(S.frames[I[0]], S.frames[I[1]], I[2], v);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "matches", v);
        break;
      }
      case OP_SBP_FRAMES: {
        std::vector<MapPoint*> v;
        ret = m->SearchByProjection(S.frames[I[0]], S.frames[I[1]], I[2], v);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "matches", v);
        break;
      }
      case OP_INIT: {
        std::vector<Point2f> prev(c.f.size() / 2);
        for (size_t k = 0; k < prev.size(); ++k) prev[k].x = c.f[2 * k], prev[k].y = c.f[2 * k + 1];
        std::vector<int> m12(2, 7);
        ret = m->SearchForInitialization(S.frames[I[0]], S.frames[I[1]], prev, m12, I[2]);
        fprintf(out, "%d\n", ret);
        dump_ints("m12", m12);
        dump_hex("prev", prev.data(), prev.size() * sizeof(Point2f));
        break;
      }
      case OP_SBP_LAST: {
        Frame& F = S.frames[I[0]];
        ret = m->SearchByProjection(F, static_cast<const Frame&>(S.frames[I[1]]), c.f[0]);
        fprintf(out, "%d\n", ret);
        dump_ids(S, "frame", F.mvpMapPoints);
        break;
      }
      case OP_EXTRACTOR:
        ex.reset(new USLAM::ORBextractor(I[0], c.f[0], I[1], USLAM::ORBextractor::HARRIS_SCORE, I[2]));
        fprintf(out, "0\n");
        continue;
      case OP_EXTRACT: {
        const uint8_t* img = I[0] < 0 ? nullptr : S.images[I[0]].px.data();
        std::vector<uvo_keypoint> kps(list(c, 0).size() / 7);
        if (!kps.empty()) memcpy(kps.data(), list(c, 0).data(), kps.size() * sizeof(uvo_keypoint));
        std::vector<uint8_t> desc(5, 0xab);  // stale content
        std::vector<int32_t> grid = list(c, 1);
        ret = ex->extract(img, I[1], I[2], I[3], kps, desc, grid.empty() ? nullptr : grid.data(), I[7], I[8], I[4], I[5] != 0, I[6]);
        fprintf(out, "%d\n", ret);
        dump_hex("kps", kps.data(), kps.size() * sizeof(uvo_keypoint));
        dump_hex("desc", desc.data(), desc.size());
        dump_ints("grid", grid);
        if (ret != UVO_OK) err = ex->last_error();
        break;
      }
      case OP_GRIDER: {
        const Image& im = S.images[I[0]];
        uvo_extractor_cfg cfg;
        cfg.nfeatures = 1000, cfg.scale_factor = 1.2f, cfg.nlevels = 8, cfg.score_type = 0, cfg.fast_th = 20;
        cfg.max_width = im.w, cfg.max_height = im.h, cfg.max_batch = 1, cfg.max_input_keypoints = 0, cfg.device = 0;
        uvo_extractor* h = nullptr;
        ret = uvo_extractor_create(&cfg, &h);
        std::vector<uvo_keypoint> pts(3);
        for (int k = 0; k < 3; ++k) memset(&pts[k], 0, sizeof(uvo_keypoint)), pts[k].class_id = 1000 + k;
        if (ret == UVO_OK)
          ret = USLAM::Grider_FAST::perform_griding(h, im.px.data(), im.w, im.h, im.stride, pts, I[1], I[2], I[3], I[4], I[5] != 0);
        uvo_extractor_destroy(h);
        fprintf(out, "%d\n", ret);
        dump_hex("kps", pts.data(), pts.size() * sizeof(uvo_keypoint));
        break;
      }
      default:
        fprintf(stderr, "unknown op %d\n", c.op);
        return 2;
    }
    if (m && m->last_error() != err_before) err = m->last_error();  // last_error() is never cleared: a change is a new error
    fprintf(out, "v err %s\n", err.empty() ? "-" : "set");
    if (!err.empty()) fprintf(stderr, "call %zu: %s\n", ci, err.c_str());
    if (map_changed) dump_map(S);
    fflush(out);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s scene.bin dump.txt\n", argv[0]);
    return 2;
  }
  Scene S;
  read_scene(argv[1], S);
  out = fopen(argv[2], "w");
  if (!out) return 2;
  const int rc = run(S);
  fclose(out);
  return rc;
}
