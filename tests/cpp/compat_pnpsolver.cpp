// Drives USLAM::PnPsolver (include/uvo/compat/PnPsolver.h) the way Tracking::Relocalisation would (src/Tracking.cc:2415-2441), on a
// scene written by tests/test_gpu_cpp_pnpsolver.py, twice: the reference's loop as it stands (iterate(5) solver by solver), and the
// same loop with its inner for(i) replaced by USLAM::IterateCandidates (one library call per round).  Each on a set of its own, so
// both start from srand(1).
//   compat_pnpsolver scene.bin out.bin
// scene.bin: int32 nkeys, C; float fx, fy, cx, cy, sigma2[8]; nkeys x uvo_keypoint; C x nkeys x {int32 flag (0 null, 1 good, 2 bad); float X, Y, Z}.
// out.bin, per mode: int32 candidate (-1: none), nInliers, rounds, nCandidates left; float Tcw[16]; nkeys x uint8 vbInliers (zeros when
// none); C x uint8 vbDiscarded.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uvo/compat/PnPsolver.h"

namespace {
struct Pos {
  float v[3];
  float operator[](int i) const { return v[i]; }
};
struct MapPoint {
  Pos pos;
  bool bad;
  bool isBad() const { return bad; }
  Pos GetWorldPos() const { return pos; }
};
struct Frame {
  std::vector<uvo_keypoint> mvKeysUn;
  std::vector<float> mvLevelSigma2;
  float fx, fy, cx, cy;
};
struct Outcome {
  int32_t candidate, nInliers, rounds, left;
  float Tcw[16];
  std::vector<uint8_t> inliers, discarded;
};

Outcome relocalise(uvo_klt* klt, const Frame& F, std::vector<std::vector<MapPoint*> >& vvpMapPointMatches, bool one_call) {
  const size_t nKFs = vvpMapPointMatches.size();
  USLAM::PnPsolverSet solvers(klt, (int)nKFs, (int)F.mvKeysUn.size());
  std::vector<USLAM::PnPsolver*> vpPnPsolvers(nKFs);
  std::vector<bool> vbDiscarded(nKFs);
  int nCandidates = 0;
  for (size_t i = 0; i < nKFs; i++) {
    USLAM::PnPsolver* pSolver = new USLAM::PnPsolver(solvers, F, vvpMapPointMatches[i]);
    pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    vpPnPsolvers[i] = pSolver;
    nCandidates++;
  }
  Outcome o;
  o.candidate = -1, o.nInliers = 0, o.rounds = 0;
  for (int k = 0; k < 16; ++k) o.Tcw[k] = 0.f;
  o.inliers.assign(F.mvKeysUn.size(), 0);
  bool bMatch = false;
  while (nCandidates > 0 && !bMatch && o.rounds < 100) {
    o.rounds++;
    std::vector<bool> vbInliers;
    int nInliers = 0;
    USLAM::PnPsolver::Tcw Tcw;
    int who = -1;
    if (one_call) {
      who = USLAM::IterateCandidates(solvers, vpPnPsolvers, vbDiscarded, nCandidates, 5, Tcw, vbInliers, nInliers);
    } else {
      for (size_t i = 0; i < nKFs; i++) {
        if (vbDiscarded[i]) continue;
        bool bNoMore;
        Tcw = vpPnPsolvers[i]->iterate(5, bNoMore, vbInliers, nInliers);
        if (bNoMore) {
          vbDiscarded[i] = true;
          nCandidates--;
        }
        if (!Tcw.empty()) {
          who = (int)i;
          break;
        }
      }
    }
    if (who >= 0 && !Tcw.empty()) {
      bMatch = true;
      o.candidate = who, o.nInliers = nInliers;
      for (int k = 0; k < 16; ++k) o.Tcw[k] = Tcw.data()[k];
      for (size_t j = 0; j < vbInliers.size(); j++) o.inliers[j] = vbInliers[j] ? 1 : 0;
    }
  }
  o.left = nCandidates;
  for (size_t i = 0; i < nKFs; i++) o.discarded.push_back(vbDiscarded[i] ? 1 : 0), delete vpPnPsolvers[i];
  return o;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t nkeys = 0, C = 0;
  Frame F;
  F.mvLevelSigma2.resize(8);
  bool ok = std::fread(&nkeys, 4, 1, f) == 1 && std::fread(&C, 4, 1, f) == 1 && std::fread(&F.fx, 4, 1, f) == 1 && std::fread(&F.fy, 4, 1, f) == 1 &&
            std::fread(&F.cx, 4, 1, f) == 1 && std::fread(&F.cy, 4, 1, f) == 1 && std::fread(&F.mvLevelSigma2[0], 4, 8, f) == 8;
  if (!ok || nkeys < 1 || C < 1) return 2;
  F.mvKeysUn.resize(nkeys);
  ok = std::fread(&F.mvKeysUn[0], sizeof(uvo_keypoint), nkeys, f) == (size_t)nkeys;
  std::vector<std::vector<MapPoint> > store(C, std::vector<MapPoint>(nkeys));
  std::vector<std::vector<MapPoint*> > matches(C, std::vector<MapPoint*>(nkeys));
  for (int c = 0; ok && c < C; ++c)
    for (int i = 0; ok && i < nkeys; ++i) {
      int32_t flag;
      ok = std::fread(&flag, 4, 1, f) == 1 && std::fread(store[c][i].pos.v, 4, 3, f) == 3;
      store[c][i].bad = flag == 2;
      matches[c][i] = flag == 0 ? 0 : &store[c][i];
    }
  std::fclose(f);
  if (!ok) return 2;
  uvo_klt_cfg cfg = {64, 64, 3, 21, 21, 16, 2, 0};
  uvo_klt* klt = 0;
  if (uvo_klt_create(&cfg, &klt) != UVO_OK) {
    std::fprintf(stderr, "%s\n", uvo_last_error());
    return 1;
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  int32_t said[2][3];
  for (int mode = 0; mode < 2; ++mode) {
    const Outcome r = relocalise(klt, F, matches, mode == 1);
    std::fwrite(&r.candidate, 4, 4, o);
    std::fwrite(r.Tcw, 4, 16, o);
    std::fwrite(&r.inliers[0], 1, r.inliers.size(), o);
    std::fwrite(&r.discarded[0], 1, r.discarded.size(), o);
    said[mode][0] = r.candidate, said[mode][1] = r.nInliers, said[mode][2] = r.rounds;
  }
  std::fclose(o);
  uvo_klt_destroy(klt);
  std::printf("{\"by_solver\": [%d, %d, %d], \"one_call\": [%d, %d, %d]}\n", said[0][0], said[0][1], said[0][2], said[1][0], said[1][1], said[1][2]);
  return 0;
}
