"""Plain numpy model of the 256-bit Hamming operations of csrc/hamming.hip: brute force, no oracle, no library.

A descriptor is 32 bytes = four 64-bit words; a distance is the popcount of the XOR of the words (ORBmatcher::DescriptorDistance,
src/ORBmatcher.cc:1794-1810, counts the same bits 32 at a time).  Conventions are the library's (include/uvo/uvo.h): idx = -1 and
d = 0xFFFF where fewer than one / two train rows are allowed, the lower train index wins a tie."""
import numpy as np

NO_IDX, NO_DIST = -1, 0xFFFF
_CHUNK = 1 << 22   # query x train pairs per block of the distance matrix (32 MiB of uint64 per word)


def _words(d):
    d = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
    return d.view(np.uint64).reshape(len(d), 4)


def distance_matrix(q, t):
    """(nq, nt) int32: popcount(q[i] ^ t[j])."""
    qw, tw = _words(q), _words(t)
    out = np.zeros((len(qw), len(tw)), np.int32)
    if len(qw) == 0 or len(tw) == 0:
        return out
    step = max(1, _CHUNK // len(tw))
    for a in range(0, len(qw), step):
        acc = np.zeros((len(qw[a:a + step]), len(tw)), np.uint8)
        for w in range(4):
            acc += np.bitwise_count(qw[a:a + step, w, None] ^ tw[None, :, w])   # at most 64 per word: no overflow before the last add
            if w == 2:
                acc = acc.astype(np.int32)
        out[a:a + step] = acc
    return out


def knn2(q, t, mask=None):
    """Best and second best train row per query: idx0, d0, idx1, d1 (int32, int32, int32, int32 with -1 / 0xFFFF for "none").
    mask: (nq, nt), non-zero = pair allowed.  The order is that of the key d * 65536 + index, sorted stably: nearest first, the
    lower index among equals."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    assert nt <= 65535
    idx0, idx1 = np.full(nq, NO_IDX, np.int32), np.full(nq, NO_IDX, np.int32)
    d0, d1 = np.full(nq, NO_DIST, np.int32), np.full(nq, NO_DIST, np.int32)
    if nq == 0 or nt == 0:
        return idx0, d0, idx1, d1
    if mask is not None:
        mask = np.asarray(mask).reshape(nq, nt) != 0
    none = np.int64(1) << 40                      # above every real key (256 * 65536 + 65534)
    step = max(1, _CHUNK // nt)
    for a in range(0, nq, step):
        key = distance_matrix(q[a:a + step], t).astype(np.int64) * 65536 + np.arange(nt, dtype=np.int64)[None, :]
        if mask is not None:
            key[~mask[a:a + step]] = none
        if nt > 2:
            two = np.sort(np.partition(key, 1, axis=1)[:, :2], axis=1, kind="stable")   # keys are distinct: the two smallest are unique
        else:
            two = np.sort(key, axis=1, kind="stable")
        k0 = two[:, 0]
        k1 = two[:, 1] if nt > 1 else np.full(len(k0), none)
        for k, idx, d in ((k0, idx0, d0), (k1, idx1, d1)):
            ok = k < none
            idx[a:a + step] = np.where(ok, k & 0xFFFF, NO_IDX)
            d[a:a + step] = np.where(ok, k >> 16, NO_DIST)
    return idx0, d0, idx1, d1


def medoid(desc):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:197-270): the row whose median distance to all rows, itself included,
    is least; median = sorted[int(0.5 * (N - 1))]; the first index wins a tie.  (best_idx, best_median), (-1, -1) for no rows."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    if n == 0:
        return -1, -1
    med = np.sort(distance_matrix(desc, desc), axis=1)[:, int(0.5 * (n - 1))]
    best = int(np.argmin(med))                    # argmin returns the first of equal minima
    return best, int(med[best])


def ratio_matches(q, t, ratio, mask=None):
    """Utils::ratioMatching (include/utils.h:81-111): rows (query, train, distance) of the queries with two neighbours and
    d0 <= d1 * ratio, the product taken in double; nothing for an empty side."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    if len(q) == 0 or len(t) == 0:
        return np.zeros((0, 3), np.int32)
    idx0, d0, idx1, d1 = knn2(q, t, mask)
    ok = (idx1 >= 0) & (d0.astype(np.float64) <= d1.astype(np.float64) * float(ratio))
    qi = np.nonzero(ok)[0]
    return np.stack([qi, idx0[qi], d0[qi]], 1).astype(np.int32)
