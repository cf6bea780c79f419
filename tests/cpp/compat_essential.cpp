// Drives USLAM::Optimizer::OptimizeEssentialGraph (include/uvo/compat/Optimizer.h) the way LoopClosing::CorrectLoop would: key frames,
// map points and the map as stub types, a graph with everything the walk of src/Optimizer.cc:2437-2598 distinguishes (a bad key frame
// that is a parent, a loop edge and a covisible; loop connections below and above the weight rule; a covisible that is the parent, a
// child, a loop edge or an inserted pair; points corrected by the current key frame, a bad point, a point whose reference is bad);
// everything the call gathered and touched is written out for tests/test_gpu_cpp_essential.py.  Built as C++11 with -Wall -Werror, no
// OpenCV.
//
//   compat_essential scene.bin out.bin
// scene.bin: int32 nKF, nMP, loop, current; per key frame: int32 mnId, bad, parent (-1: none); float R[9] t[3]; int32 nloop, loop[nloop];
//            int32 ncov, {int32 kf, weight} [ncov] (in the order GetCovisiblesByWeight returns them); int32 nchild, child[nchild];
//            int32 corrected, double sim[8] if so; int32 noncorrected, double sim[8] if so; int32 nconn, conn[nconn] (its LoopConnections);
//            per map point: int32 bad, ref; float pos[3]; int32 mnCorrectedByKF, mnCorrectedReference
// out.bin:   int32 ret, K, E, P, iterations, trials, blocks; double Scw[K][8], Scw_normal[K][8]; int32 i[E], j[E]; uint8 connection[E];
//            int32 ref[P]; per key frame: int32 poses set; float T[16]; per map point: int32 positions set, normal updates; float pos[3]
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "uvo/compat/Optimizer.h"

namespace {
struct Vec {
  std::vector<float> v;
  float operator[](int i) const { return v[i]; }
};
struct KeyFrame {
  long unsigned int mnId;
  bool bad;
  float T[16];
  int n_set;
  KeyFrame* parent;
  std::set<KeyFrame*> loop, children;
  std::vector<std::pair<KeyFrame*, int> > cov;
  bool isBad() const { return bad; }
  Vec GetRotation() const {
    Vec m;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) m.v.push_back(T[4 * r + c]);
    return m;
  }
  Vec GetTranslation() const {
    Vec m;
    for (int r = 0; r < 3; ++r) m.v.push_back(T[4 * r + 3]);
    return m;
  }
  void SetPose(const float* M) { std::memcpy(T, M, sizeof T), ++n_set; }
  KeyFrame* GetParent() const { return parent; }
  std::set<KeyFrame*> GetLoopEdges() const { return loop; }
  bool hasChild(KeyFrame* p) const { return children.count(p) != 0; }
  int GetWeight(KeyFrame* p) const {
    for (size_t i = 0; i < cov.size(); ++i)
      if (cov[i].first == p) return cov[i].second;
    return 0;
  }
  std::vector<KeyFrame*> GetCovisiblesByWeight(int w) const {
    std::vector<KeyFrame*> out;
    for (size_t i = 0; i < cov.size(); ++i)
      if (cov[i].second >= w) out.push_back(cov[i].first);
    return out;
  }
};
struct MapPoint {
  bool bad;
  float pos[3];
  int n_set, n_updates;
  long unsigned int mnCorrectedByKF, mnCorrectedReference;
  KeyFrame* ref;
  bool isBad() const { return bad; }
  Vec GetWorldPos() const {
    Vec p;
    p.v.assign(pos, pos + 3);
    return p;
  }
  void SetWorldPos(const float* X) { pos[0] = X[0], pos[1] = X[1], pos[2] = X[2], ++n_set; }
  void UpdateNormalAndDepth() { ++n_updates; }
  KeyFrame* GetReferenceKeyFrame() const { return ref; }
};
struct Map {
  std::vector<KeyFrame*> kfs;
  std::vector<MapPoint*> mps;
  std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<MapPoint*> GetAllMapPoints() const { return mps; }
};
bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
void wr(FILE* f, const void* p, size_t n) { std::fwrite(p, 1, n, f); }
void wi(FILE* f, int32_t v) { wr(f, &v, 4); }
bool list(FILE* f, std::vector<int32_t>& v, int per = 1) {
  int32_t n;
  if (!rd(f, &n, 4) || n < 0 || n > 100000) return false;
  v.resize((size_t)n * per);
  return n == 0 || rd(f, &v[0], 4 * v.size());
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[4];
  if (!rd(f, h, sizeof h)) return 2;
  const int nKF = h[0], nMP = h[1];
  std::vector<KeyFrame> kfs(nKF);
  std::vector<MapPoint> mps(nMP);
  std::vector<std::vector<int32_t> > loop(nKF), cov(nKF), child(nKF), conn(nKF);
  std::vector<int32_t> parent(nKF), ref(nMP);
  typedef std::map<KeyFrame*, USLAM::Sim3> KeyFrameAndPose;
  KeyFrameAndPose Corrected, NonCorrected;
  for (int k = 0; k < nKF; ++k) {
    KeyFrame& kf = kfs[k];
    int32_t id[3];
    float R[9], t[3];
    if (!rd(f, id, 12) || !rd(f, R, 36) || !rd(f, t, 12) || !list(f, loop[k]) || !list(f, cov[k], 2) || !list(f, child[k])) return 2;
    kf.mnId = (long unsigned int)id[0], kf.bad = id[1] != 0, parent[k] = id[2], kf.n_set = 0, kf.parent = 0;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) kf.T[4 * r + c] = R[3 * r + c];
      kf.T[4 * r + 3] = t[r];
    }
    kf.T[12] = kf.T[13] = kf.T[14] = 0.f, kf.T[15] = 1.f;
    for (int which = 0; which < 2; ++which) {
      int32_t has;
      double s[8];
      if (!rd(f, &has, 4)) return 2;
      if (!has) continue;
      if (!rd(f, s, sizeof s)) return 2;
      (which == 0 ? Corrected : NonCorrected)[&kfs[k]] = USLAM::Sim3(s, s + 4, s[7]);
    }
    if (!list(f, conn[k])) return 2;
  }
  for (int j = 0; j < nMP; ++j) {
    int32_t br[2], c[2];
    if (!rd(f, br, 8) || !rd(f, mps[j].pos, 12) || !rd(f, c, 8)) return 2;
    mps[j].bad = br[0] != 0, ref[j] = br[1], mps[j].n_set = mps[j].n_updates = 0;
    mps[j].mnCorrectedByKF = (long unsigned int)c[0], mps[j].mnCorrectedReference = (long unsigned int)c[1];
    mps[j].ref = &kfs[ref[j]];
  }
  std::fclose(f);
  std::map<KeyFrame*, std::set<KeyFrame*> > LoopConnections;
  Map map;
  for (int k = 0; k < nKF; ++k) {
    if (parent[k] >= 0) kfs[k].parent = &kfs[parent[k]];
    for (size_t i = 0; i < loop[k].size(); ++i) kfs[k].loop.insert(&kfs[loop[k][i]]);
    for (size_t i = 0; i < child[k].size(); ++i) kfs[k].children.insert(&kfs[child[k][i]]);
    for (size_t i = 0; i + 1 < cov[k].size(); i += 2) kfs[k].cov.push_back(std::make_pair(&kfs[cov[k][i]], (int)cov[k][i + 1]));
    for (size_t i = 0; i < conn[k].size(); ++i) LoopConnections[&kfs[k]].insert(&kfs[conn[k][i]]);
    map.kfs.push_back(&kfs[k]);
  }
  for (int j = 0; j < nMP; ++j) map.mps.push_back(&mps[j]);

  uvo_matcher_cfg cfg = {64, 64, 1, 64, 0};
  uvo_matcher* m = 0;
  if (uvo_matcher_create(&cfg, &m) != UVO_OK) return 3;
  {
    USLAM::EssentialGraphOptimizer graph(m, 64, 512, 2048, 256);
    if (!graph.ok()) return 3;
    const USLAM::Sim3 Scurw;
    const int ret = USLAM::Optimizer::OptimizeEssentialGraph(graph, &map, &kfs[h[2]], &kfs[h[3]], Scurw, NonCorrected, Corrected, LoopConnections);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t K = ret == 0 ? (int32_t)graph.Scw.size() : 0, E = ret == 0 ? (int32_t)graph.edge_i.size() : 0, P = ret == 0 ? (int32_t)graph.point_ref.size() : 0;
    wi(o, ret), wi(o, K), wi(o, E), wi(o, P);
    wi(o, ret == 0 ? graph.result.iterations : 0), wi(o, ret == 0 ? graph.result.n_trials : 0), wi(o, ret == 0 ? graph.result.envelope_blocks : 0);
    if (K) wr(o, &graph.Scw[0], 64 * (size_t)K), wr(o, &graph.Scw_normal[0], 64 * (size_t)K);
    if (E) wr(o, &graph.edge_i[0], 4 * (size_t)E), wr(o, &graph.edge_j[0], 4 * (size_t)E), wr(o, &graph.edge_connection[0], (size_t)E);
    if (P) wr(o, &graph.point_ref[0], 4 * (size_t)P);
    for (int k = 0; k < nKF; ++k) wi(o, kfs[k].n_set), wr(o, kfs[k].T, sizeof kfs[k].T);
    for (int j = 0; j < nMP; ++j) wi(o, mps[j].n_set), wi(o, mps[j].n_updates), wr(o, mps[j].pos, 12);
    std::fclose(o);
  }
  uvo_matcher_destroy(m);
  return 0;
}
