"""Plain-Python model of the map the compat adaptors mutate (include/uvo/compat/ORBmatcher.h): map points with observations, key frames
with map-point slots, and the reference's loops that change them.  The expected values of tests/test_gpu_compat_adaptors.py are
computed on it; tests/test_matcher_rules.py checks it on a hand-worked example.  Test infrastructure only.

    MapPoint::Replace                      src/MapPoint.cc:132-170
    MapPoint::ComputeDistinctiveDescriptors src/MapPoint.cc:214-260
    ORBmatcher::Fuse(pKF, vpMapPoints, th)  src/ORBmatcher.cc:1016-1134 (mutation :1101-1119)
    ORBmatcher::Fuse(pKF, Scw, vpPoints, th) :1136-1265 (mutation :1241-1258)
    LocalMapping::SearchInNeighbors          src/LocalMapping.cc:1228-1236 (one Fuse per target key frame)
"""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    return int(_POP[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


class MapPoint:
    def __init__(self, pid, desc, bad=False):
        self.id = pid
        self.desc = np.array(desc, np.uint8).reshape(32)
        self.bad = bool(bad)
        self.replaced = -1
        self.obs = {}            # key-frame index -> key-point index (std::map<KeyFrame*, size_t>, key frames in index order)


class KeyFrame:
    def __init__(self, desc, slots):
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.slots = [int(s) for s in slots]   # map-point id per key point, -1 = NULL


class MapModel:
    """counts per fuse form: 'replace', 'add', 'redescribed_searched' = searches of a point whose descriptor a Replace changed (since
    the start of the last fuse_targets), 'redescribed_changed' = those whose result the old descriptor would have changed."""

    def __init__(self, kfs, points):
        self.kfs, self.mps = kfs, points
        for f, kf in enumerate(kfs):                     # observations follow the slots (bad points observe nothing)
            for k, pid in enumerate(kf.slots):
                if pid >= 0 and not self.mps[pid].bad:
                    self.mps[pid].obs.setdefault(f, k)
        self.counts = {}
        self.redescribed = {}

    def count(self, key, n=1):
        self.counts[key] = self.counts.get(key, 0) + n

    def get_map_points(self, f):
        """KeyFrame::GetMapPoints: the non-NULL, non-bad slots"""
        return {p for p in self.kfs[f].slots if p >= 0 and not self.mps[p].bad}

    def add_observation(self, p, f, k):
        if f not in p.obs:
            p.obs[f] = k

    def new_point(self, desc):
        p = MapPoint(len(self.mps), desc)
        self.mps.append(p)
        return p

    def replace(self, p, q):
        """p.Replace(q)"""
        if p.id == q.id:
            return
        obs, p.obs = p.obs, {}
        p.bad, p.replaced = True, q.id
        for f in sorted(obs):
            k = obs[f]
            if f not in q.obs:
                self.kfs[f].slots[k] = q.id
                self.add_observation(q, f, k)
            else:
                self.kfs[f].slots[k] = -1
        self.compute_distinctive(q)

    def compute_distinctive(self, q):
        if q.bad or not q.obs:
            return
        d = [self.kfs[f].desc[q.obs[f]] for f in sorted(q.obs)]
        n = len(d)
        best, best_median = 0, None
        for i in range(n):
            row = sorted(0 if i == j else descriptor_distance(d[i], d[j]) for j in range(n))
            med = row[int(0.5 * (n - 1))]
            if best_median is None or med < best_median:      # strict: the first index wins ties
                best, best_median = i, med
        if not np.array_equal(q.desc, d[best]):
            self.redescribed.setdefault(q.id, q.desc)           # the descriptor before the first change
        q.desc = d[best].copy()

    def fuse(self, f, ids, search, form="fuse"):
        """Fuse(pKF = key frame f, vpMapPoints = ids (-1 = NULL), th); search(f, point) -> best key point or -1 with the point's
        descriptor as it is now.  Returns nFused."""
        n = 0
        for pid in ids:
            if pid < 0:
                continue
            p = self.mps[pid]
            if p.bad or f in p.obs:
                continue
            b = search(f, p)
            if pid in self.redescribed:
                self.count(form + ":redescribed_searched")
                cur, p.desc = p.desc, self.redescribed[pid]
                self.count(form + ":redescribed_changed", int(search(f, p) != b))   # a result the stale descriptor gets wrong
                p.desc = cur
            if b < 0:
                continue
            q = self.kfs[f].slots[b]
            if q >= 0:
                if not self.mps[q].bad:
                    self.replace(p, self.mps[q])
                    self.count(form + ":replace")
            else:
                self.add_observation(p, f, b)
                self.kfs[f].slots[b] = pid
                self.count(form + ":add")
            n += 1
        return n

    def fuse_targets(self, targets, ids, search):
        """the loop of LocalMapping::SearchInNeighbors: one Fuse per target key frame, in order"""
        self.redescribed = {}
        return sum(self.fuse(f, ids, search, "fuse_targets") for f in targets)

    def fuse_scw(self, f, ids, search):
        """Fuse(pKF, Scw, vpPoints, th): spAlreadyFound taken once up front; the key frame's point is replaced by the candidate"""
        already = self.get_map_points(f)
        n = 0
        for pid in ids:
            p = self.mps[pid]
            if p.bad or pid in already:
                continue
            b = search(f, p)
            if b < 0:
                continue
            q = self.kfs[f].slots[b]
            if q >= 0:
                if not self.mps[q].bad:
                    self.replace(self.mps[q], p)
                    self.count("fuse_scw:replace")
            else:
                self.add_observation(p, f, b)
                self.kfs[f].slots[b] = pid
                self.count("fuse_scw:add")
            n += 1
        return n

    def dump(self):
        """the map state in the driver's dump form: ({f: slots}, {id: (bad, replaced, sorted observations, descriptor hex)})"""
        kfs = {f: list(kf.slots) for f, kf in enumerate(self.kfs)}
        mps = {p.id: (int(p.bad), p.replaced, sorted(p.obs.items()), p.desc.tobytes().hex()) for p in self.mps}
        return kfs, mps
