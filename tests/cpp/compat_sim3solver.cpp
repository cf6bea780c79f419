// Drives USLAM::Sim3Solver (include/uvo/compat/Sim3Solver.h) the way LoopClosing::ComputeSim3 would (src/LoopClosing.cc:409-479), on a
// scene written by tests/test_gpu_cpp_sim3solver.py, twice: the reference's loop as it stands (iterate(5) solver by solver), and the
// same loop with its for(i) replaced by USLAM::IterateCandidates (one library call per stretch of candidates).  OptimizeSim3 is stood
// in for by a threshold on nInliers, so that a returned transform can be rejected and the loop goes on behind it.  Each mode on a set
// of its own, so both start from srand(1).
//   compat_sim3solver scene.bin out.bin
// scene.bin: int32 nkeys, C, accept; float sigma2[8]; per candidate: 2 x {float Rcw[9], tcw[3], K[4] (fx fy cx cy)}, then nkeys x
//   {int32 flag (0 no match, 1 good, 2 first point bad, 3 second point bad, 4 first key frame has no point there); float X1[3], X2[3];
//    int32 octave1, octave2}.
// out.bin, per mode: int32 candidate (-1: none), nInliers, rounds, nCandidates left; float T12[16], R[9], t[3], s; nkeys x uint8
// vbInliers (zeros when none); C x uint8 vbDiscarded.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uvo/compat/Sim3Solver.h"

namespace {
struct Vec {
  std::vector<float> v;
  float operator[](int i) const { return v[i]; }
};
struct KeyFrame;
struct MapPoint {
  Vec pos;
  bool bad;
  const KeyFrame* owner;
  int index;
  bool isBad() const { return bad; }
  Vec GetWorldPos() const { return pos; }
  int GetIndexInKeyFrame(const KeyFrame* pKF) const { return pKF == owner ? index : -1; }
};
struct KeyFrame {
  Vec R, t, K;
  std::vector<uvo_keypoint> keys;
  std::vector<MapPoint*> points;
  const float* sigma2;
  std::vector<MapPoint*> GetMapPointMatches() const { return points; }
  Vec GetRotation() const { return R; }
  Vec GetTranslation() const { return t; }
  Vec GetCalibrationMatrix() const { return K; }
  const uvo_keypoint& GetKeyPointUn(int i) const { return keys[i]; }
  float GetSigma2(int octave) const { return sigma2[octave]; }
};
struct Candidate {
  KeyFrame kf1, kf2;
  std::vector<MapPoint> mp1, mp2;
  std::vector<MapPoint*> matched12;
};
struct Outcome {
  int32_t candidate, nInliers, rounds, left;
  float T[29];
  std::vector<uint8_t> inliers, discarded;
};

bool read_kf(FILE* f, KeyFrame& kf, int nkeys, const float* sigma2) {
  float p[16];
  if (std::fread(p, 4, 16, f) != 16) return false;
  kf.R.v.assign(p, p + 9), kf.t.v.assign(p + 9, p + 12);
  const float K[9] = {p[12], 0, p[14], 0, p[13], p[15], 0, 0, 1};
  kf.K.v.assign(K, K + 9);
  kf.keys.assign(nkeys, uvo_keypoint());
  kf.points.assign(nkeys, 0);
  kf.sigma2 = sigma2;
  return true;
}

Outcome compute_sim3(uvo_matcher* matcher, std::vector<Candidate>& cands, int nkeys, int accept, bool one_call) {
  const int nInitialCandidates = (int)cands.size();
  USLAM::Sim3SolverSet solvers(matcher, nInitialCandidates, nkeys);
  std::vector<USLAM::Sim3Solver*> vpSim3Solvers(nInitialCandidates);
  std::vector<bool> vbDiscarded(nInitialCandidates);
  int nCandidates = 0;
  for (int i = 0; i < nInitialCandidates; i++) {
    USLAM::Sim3Solver* pSolver = new USLAM::Sim3Solver(solvers, &cands[i].kf1, &cands[i].kf2, cands[i].matched12);
    pSolver->SetRansacParameters(0.99, 2, 300);
    vpSim3Solvers[i] = pSolver;
    nCandidates++;
  }
  Outcome o;
  o.candidate = -1, o.nInliers = 0, o.rounds = 0;
  for (int k = 0; k < 29; ++k) o.T[k] = 0.f;
  o.inliers.assign(nkeys, 0);
  bool bMatch = false;
  while (nCandidates > 0 && !bMatch && o.rounds < 100) {
    o.rounds++;
    for (int i = 0; i < nInitialCandidates; i++) {
      std::vector<bool> vbInliers;
      int nInliers = 0;
      USLAM::Sim3Solver::T12 Scm;
      if (one_call) {
        i = USLAM::IterateCandidates(solvers, vpSim3Solvers, vbDiscarded, nCandidates, i, 5, Scm, vbInliers, nInliers);
        if (i < 0) break;
      } else {
        if (vbDiscarded[i]) continue;
        bool bNoMore;
        Scm = vpSim3Solvers[i]->iterate(5, bNoMore, vbInliers, nInliers);
        if (bNoMore) {
          vbDiscarded[i] = true;
          nCandidates--;
        }
      }
      if (!Scm.empty() && nInliers >= accept) {  // OptimizeSim3's verdict
        USLAM::Sim3Solver* pSolver = vpSim3Solvers[i];
        bMatch = true;
        o.candidate = i, o.nInliers = nInliers;
        for (int k = 0; k < 16; ++k) o.T[k] = Scm.data()[k];
        for (int k = 0; k < 9; ++k) o.T[16 + k] = pSolver->GetEstimatedRotation().data()[k];
        for (int k = 0; k < 3; ++k) o.T[25 + k] = pSolver->GetEstimatedTranslation().at(k);
        o.T[28] = pSolver->GetEstimatedScale();
        for (size_t j = 0; j < vbInliers.size(); j++) o.inliers[j] = vbInliers[j] ? 1 : 0;
        break;
      }
    }
  }
  o.left = nCandidates;
  for (int i = 0; i < nInitialCandidates; i++) o.discarded.push_back(vbDiscarded[i] ? 1 : 0), delete vpSim3Solvers[i];
  return o;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[3] = {0, 0, 0};
  float sigma2[8];
  bool ok = std::fread(head, 4, 3, f) == 3 && std::fread(sigma2, 4, 8, f) == 8;
  const int nkeys = head[0], C = head[1], accept = head[2];
  if (!ok || nkeys < 1 || C < 1) return 2;
  std::vector<Candidate> cands(C);
  for (int c = 0; ok && c < C; ++c) {
    Candidate& k = cands[c];
    ok = read_kf(f, k.kf1, nkeys, sigma2) && read_kf(f, k.kf2, nkeys, sigma2);
    k.mp1.resize(nkeys), k.mp2.resize(nkeys), k.matched12.assign(nkeys, 0);
    for (int i = 0; ok && i < nkeys; ++i) {
      int32_t flag, oct[2];
      float X[6];
      ok = std::fread(&flag, 4, 1, f) == 1 && std::fread(X, 4, 6, f) == 6 && std::fread(oct, 4, 2, f) == 2;
      k.mp1[i].pos.v.assign(X, X + 3), k.mp2[i].pos.v.assign(X + 3, X + 6);
      k.mp1[i].bad = flag == 2, k.mp2[i].bad = flag == 3;
      k.mp1[i].owner = &k.kf1, k.mp2[i].owner = &k.kf2, k.mp1[i].index = k.mp2[i].index = i;
      k.kf1.keys[i].octave = oct[0], k.kf2.keys[i].octave = oct[1];
      k.kf1.points[i] = flag == 4 ? 0 : &k.mp1[i];
      k.matched12[i] = flag == 0 ? 0 : &k.mp2[i];
    }
  }
  std::fclose(f);
  if (!ok) return 2;
  uvo_matcher_cfg cfg = {64, 64, 1, 64, 0};
  uvo_matcher* matcher = 0;
  if (uvo_matcher_create(&cfg, &matcher) != UVO_OK) {
    std::fprintf(stderr, "%s\n", uvo_last_error());
    return 1;
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  int32_t said[2][3];
  for (int mode = 0; mode < 2; ++mode) {
    const Outcome r = compute_sim3(matcher, cands, nkeys, accept, mode == 1);
    std::fwrite(&r.candidate, 4, 4, o);
    std::fwrite(r.T, 4, 29, o);
    std::fwrite(&r.inliers[0], 1, r.inliers.size(), o);
    std::fwrite(&r.discarded[0], 1, r.discarded.size(), o);
    said[mode][0] = r.candidate, said[mode][1] = r.nInliers, said[mode][2] = r.rounds;
  }
  std::fclose(o);
  uvo_matcher_destroy(matcher);
  std::printf("{\"by_solver\": [%d, %d, %d], \"one_call\": [%d, %d, %d]}\n", said[0][0], said[0][1], said[0][2], said[1][0], said[1][1], said[1][2]);
  return 0;
}
