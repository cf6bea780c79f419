"""The four kernels of csrc/hamming.hip (k_knn2_mfma, k_knn2, k_matrix, k_medoid) against the brute-force numpy model of
tests/hamming_model.py, at the edges of their launch shapes and of the documented contract (include/uvo/uvo.h).

Every comparison is exact and covers all four outputs (idx0, d0, idx1, d1).  Outputs start from a prefill that no result can equal,
so a row the kernel did not write, or wrote where it must not, is seen.  Train rows a kernel must ignore hold exact copies of the
queries: a lost guard is a wrong answer (distance 0 at a forbidden index), never a read outside a buffer of the test.

The matrix-core kernel's shape, for reference (csrc/hamming.hip): a workgroup owns 128 queries, each of its four wavefronts 32 of
them (the MFMA columns); the train rows come in tiles of 32 (the MFMA rows); lane half h = lane >> 5 holds rows 4h + (0..3) + 8g of
a tile, g = 0..3, and the two halves' best two are merged at the end."""
import numpy as np
import pytest

import hamming_model as hm

pytestmark = pytest.mark.gpu

IDX_FILL, D_FILL = 0x5EADBEEF, 0xABCD   # no train index reaches the first; no distance (<= 256) or "none" (0xFFFF) equals the second
NAMES = ("idx0", "d0", "idx1", "d1")


def _random(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _low_entropy(rng, n):
    """Bytes from {0, 1, 128, 255}, mostly 0: nearly every best and second best is a tie that the lower train index must win."""
    return rng.choice(np.array([0, 1, 128, 255], np.uint8), (n, 32), p=[0.7, 0.1, 0.1, 0.1])


def _flip(d, nbits, salt, lo=0, span=256):
    """d with nbits distinct bits of [lo, lo + span) flipped; salt picks which (span is a power of two, 13 is odd: distinct positions)."""
    d = d.copy()
    for k in range(nbits):
        p = lo + (salt * 7 + k * 13) % span
        d[p >> 3] ^= np.uint8(1 << (p & 7))
    return d


def _planted(rng, q, nt):
    """nt random train rows; every third one a copy of a query with 0, 1 or 2 bits flipped (exact matches, near matches, and for
    nt > 3 * nq equal distances at different indices)."""
    t = _random(rng, nt)
    for j in range(0, nt, 3):
        t[j] = _flip(q[(j // 3) % len(q)], (j // 3 // len(q)) % 3, j)
    return t


def _knn2(uvo, m, q, t, mask=None, pad=5):
    """uvo_hamming_knn2 through the C entry point with prefilled outputs of nq + pad rows: the four results as int32, after checking
    that the pad kept its prefill."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    idx0, idx1 = np.full(nq + pad, IDX_FILL, np.int32), np.full(nq + pad, IDX_FILL, np.int32)
    d0, d1 = np.full(nq + pad, D_FILL, np.uint16), np.full(nq + pad, D_FILL, np.uint16)
    if mask is not None:
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.shape == (nq, nt)
    # an empty array's data pointer is not promised to be non-null: give the library a real address for "no rows"
    spare = np.zeros(32, np.uint8)
    rc = uvo.lib.uvo_hamming_knn2(m._h, (q if nq else spare).ctypes.data, nq, (t if nt else spare).ctypes.data, nt,
                                  None if mask is None else (mask if mask.size else spare).ctypes.data, idx0.ctypes.data, d0.ctypes.data,
                                  idx1.ctypes.data, d1.ctypes.data)
    assert rc == 0, "uvo_hamming_knn2(nq=%d, nt=%d) returned %d: %s" % (nq, nt, rc, uvo.last_error())
    out = [idx0, d0.astype(np.int32), idx1, d1.astype(np.int32)]
    for a, fill, name in zip(out, (IDX_FILL, D_FILL, IDX_FILL, D_FILL), NAMES):
        assert (a[nq:] == fill).all(), "%s written past nq=%d" % (name, nq)
    return [a[:nq] for a in out]


def _same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        np.testing.assert_array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64), err_msg="%s: %s" % (what, name))


def _check(uvo, m, q, t, what, mask=None):
    want = hm.knn2(q, t, mask)
    if len(q):
        _same(_knn2(uvo, m, q, t, mask), want, what)
    else:
        assert all(len(a) == 0 for a in _knn2(uvo, m, q, t, mask))
    return want


# ---- host form, no mask: k_knn2_mfma --------------------------------------------------------------------------------------------

SWEEP_NQ = (1, 31, 32, 33, 127, 128, 129, 257)


@pytest.mark.parametrize("kind", ["low_entropy", "planted"])
def test_knn2_size_sweep(uvo, kind):
    """Every nt from 0 to 130 (every nt mod 32 four times over, the tile count from 0 to 5) against nq on both sides of a wavefront's
    32 columns and a workgroup's 128, on ONE handle: the staging buffers keep the longer train sets of earlier calls behind nt."""
    rng = np.random.default_rng(101 if kind == "low_entropy" else 102)
    m = uvo.ORBmatcher(0.8, max_query=300, max_train=200)
    for nt in range(130, -1, -1):           # descending: whatever follows row nt in the staging buffer is an earlier call's row
        for nq in SWEEP_NQ:
            if kind == "low_entropy":
                q, t = _low_entropy(rng, nq), _low_entropy(rng, nt)
            else:
                q = _random(rng, nq)
                t = _planted(rng, q, nt)
            _check(uvo, m, q, t, "%s nq=%d nt=%d" % (kind, nq, nt))
    m.close()


def _placements(nt):
    """(row, row) pairs for a best and a second best: for every row position p of a 32-row tile, partners in the same lane half, the
    opposite half, other tiles, the last (partial) tile, and at index 0 and nt - 1."""
    last = (nt - 1) // 32 * 32
    tail = nt - last
    assert 32 * 3 <= last and 6 <= tail < 32
    out = []
    for p in range(32):
        a = 32 + p
        out += [(a, 32 + (p ^ 1)), (a, 32 + (p ^ 8)), (a, 32 + (p ^ 16)),      # same half: rows 4h + (0..3) + 8g share bit 2
                (a, 32 + (p ^ 4)), (a, 32 + (p ^ 12)),                          # opposite halves of one tile
                (a, p), (a, 64 + (p ^ 4)), (p, 64 + p),                         # different tiles, same or other half
                (a, last + p % tail), (last + p % tail, last + (p + 5) % tail),  # into and inside the partial tile
                (0, a), (nt - 1, a), (p if p else 64, nt - 1)]
    return out


def test_knn2_planted_placements(uvo):
    """A best and a second best planted at chosen rows, for all 128 query columns of a workgroup at once and a partial second
    workgroup.  Even and odd columns descend from two different base descriptors with different placements, so neighbouring columns
    have different answers.  Every query differs from its base in bits 128..255 only and every planted row in bits 0..127 only, so the
    distance of a planted row is pop(private part) + its flips for every column: (1, 2) flips make the first row of a placement the
    best, (2, 1) the second, (1, 1) a tie that the lower index wins."""
    rng = np.random.default_rng(103)
    nq, nt = 161, 32 * 3 + 13
    m = uvo.ORBmatcher(0.8, max_query=nq, max_train=nt)
    places = _placements(nt)
    n = len(places)
    best_at, second_at = np.zeros((2, 128, 32), bool)
    seen = dict.fromkeys(("same_half", "opposite_halves", "other_tile", "partial_tile", "index_0", "index_last", "tie_across_halves",
                          "tie_across_tiles", "tie_in_half"), 0)
    for i, pl_even in enumerate(places):
        k = i + 37
        while set(places[k % n]) & set(pl_even):
            k += 1
        pl = (pl_even, places[k % n])
        for flips in ((1, 2), (2, 1), (1, 1)):
            base = _random(rng, 2)
            q = base[np.arange(nq) % 2]              # even columns from base 0, odd columns from base 1
            q[:, 16:] ^= _random(rng, nq)[:, 16:]
            t = _random(rng, nt)
            for parity in (0, 1):
                for row, f in zip(pl[parity], flips):
                    t[row] = _flip(base[parity], f, row, 0, 128)
            idx0, d0, idx1, d1 = _check(uvo, m, q, t, "placement %s / %s flips %s" % (pl[0], pl[1], flips))
            # the inputs did what they were built for (a statement about the model's answer, not the kernel's)
            for parity in (0, 1):
                a, b = pl[parity]
                first, second = (a, b) if flips[0] < flips[1] else (b, a) if flips[0] > flips[1] else (min(a, b), max(a, b))
                assert (idx0[parity::2] == first).all() and (idx1[parity::2] == second).all()
            col = np.arange(nq) % 128
            best_at[col, idx0 % 32] = True
            second_at[col, idx1 % 32] = True
            for a, b, tie in zip(idx0, idx1, d0 == d1):
                tile, half = (a // 32, b // 32), ((a >> 2) & 1, (b >> 2) & 1)
                kind = "other_tile" if tile[0] != tile[1] else "same_half" if half[0] == half[1] else "opposite_halves"
                seen[kind] += 1
                seen["partial_tile"] += max(a, b) >= 96
                seen["index_0"] += min(a, b) == 0
                seen["index_last"] += max(a, b) == nt - 1
                if tie:
                    seen["tie_across_tiles" if tile[0] != tile[1] else "tie_in_half" if half[0] == half[1] else "tie_across_halves"] += 1
    m.close()
    assert best_at.all() and second_at.all(), "a query column never saw some row position as best / second best"
    assert all(seen.values()), seen


def test_knn2_key_extremes(uvo):
    """The signed key pop(t) - 2 <q, t> at both ends: -256 (all ones against all ones, distance 0) and +256 (all-zero query against
    all ones, distance 256), with the row order and the tile of the extreme rows varied; a train set of identical rows."""
    rng = np.random.default_rng(104)
    m = uvo.ORBmatcher(0.8, max_query=300, max_train=200)
    ones, zeros = np.full((1, 32), 255, np.uint8), np.zeros((1, 32), np.uint8)
    q = np.concatenate([ones, zeros, _random(rng, 30), _low_entropy(rng, 30), ones, zeros, _random(rng, 70)])
    seen = set()
    for nt in (1, 2, 3, 31, 32, 33, 64, 65, 130):
        for name, t in (("ones", np.repeat(ones, nt, 0)), ("zeros", np.repeat(zeros, nt, 0)),
                        ("ones_then_zeros", np.concatenate([np.repeat(ones, (nt + 1) // 2, 0), np.repeat(zeros, nt // 2, 0)])),
                        ("zeros_then_ones", np.concatenate([np.repeat(zeros, (nt + 1) // 2, 0), np.repeat(ones, nt // 2, 0)])),
                        ("alternating", np.where((np.arange(nt) % 2 == 0)[:, None], ones, zeros).astype(np.uint8)),
                        ("identical_random", np.repeat(_random(rng, 1), nt, 0))):
            for qq in (q, q[:1], q[1:2]):
                idx0, d0, idx1, d1 = _check(uvo, m, qq, t, "%s nt=%d nq=%d" % (name, nt, len(qq)))
                seen.update(d0.tolist()), seen.update(d1.tolist())
                if name == "identical_random" and nt > 1:
                    assert (idx0 == 0).all() and (idx1 == 1).all() and (d0 == d1).all()
    m.close()
    assert {0, 256, 0xFFFF} <= seen


def test_knn2_stale_staging(uvo):
    """The staging buffer keeps what an earlier call uploaded.  After a call whose train set held exact copies of the queries, a
    shorter unrelated train set with the same queries: nothing at or past the new nt may come back, down to nt = 1 and 0."""
    rng = np.random.default_rng(105)
    m = uvo.ORBmatcher(0.8, max_query=200, max_train=400)
    q = _random(rng, 150)
    for nt_short in (37, 33, 32, 31, 2, 1, 0):
        t_long = np.concatenate([_random(rng, nt_short), q, q[:50]])          # copies of the queries from row nt_short on
        idx0, d0, idx1, d1 = _check(uvo, m, q, t_long, "long train set before nt=%d" % nt_short)
        assert (d0 == 0).all() and (idx0 >= nt_short).all()
        got = _knn2(uvo, m, q, _random(rng, nt_short))
        assert (got[0] < nt_short).all() and (got[2] < nt_short).all(), "a train row past nt=%d was returned" % nt_short
        _knn2(uvo, m, q, t_long)
        _check(uvo, m, q, _random(rng, nt_short), "short train set nt=%d after a long one" % nt_short)
    m.close()


def _plant_high(q, t):
    """Best and second best of the first queries at the top of a 65535-row train set and across the index's bit 15."""
    nt = len(t)
    assert nt == 65535 and len(q) >= 8
    t[65534], t[65533] = _flip(q[0], 1, 1), _flip(q[0], 2, 2)                 # query 0: (65534, 65533)
    t[65532], t[65531] = _flip(q[1], 2, 3), _flip(q[1], 1, 4)                 # query 1: (65531, 65532)
    t[32768], t[32767] = _flip(q[2], 1, 5), _flip(q[2], 1, 6)                 # query 2: a tie across bit 15 -> (32767, 32768)
    t[32769], t[65530] = _flip(q[3], 1, 7), _flip(q[3], 1, 8)                 # query 3: a tie -> (32769, 65530)
    for i in range(4, len(q)):
        t[32770 + 500 * (i % 60) + i // 60] = _flip(q[i], 1, i)                # best high, second low
        t[100 + i] = _flip(q[i], 3, i + 1)


def _assert_high(want):
    idx0, d0, idx1, d1 = want
    assert (idx0[0], idx1[0], idx0[1], idx1[1]) == (65534, 65533, 65531, 65532)
    assert (idx0[2], idx1[2], idx0[3], idx1[3]) == (32767, 32768, 32769, 65530)
    assert (idx0[4:] >= 32768).all() and (idx1[4:] < 32768).all()


def test_knn2_capacity_train_65535(uvo):
    """The contract's largest train set: the key packs the train index in 16 bits, 65534 is the last one."""
    rng = np.random.default_rng(106)
    m = uvo.ORBmatcher(0.8, max_query=256, max_train=65535)
    q, t = _random(rng, 256), _random(rng, 65535)
    _plant_high(q, t)
    _assert_high(_check(uvo, m, q, t, "nt=65535"))
    m.close()


def test_knn2_capacity_query_65535(uvo):
    """The contract's largest query set: 512 workgroups, the last one partial."""
    rng = np.random.default_rng(107)
    m = uvo.ORBmatcher(0.8, max_query=65535, max_train=128)
    q = _random(rng, 65535)
    t = _planted(rng, q[-26:], 77)
    want = _check(uvo, m, q, t, "nq=65535")
    assert (want[1][-26:] == 0).all()        # the planted rows are copies of the last queries, in the last workgroup
    q = _low_entropy(rng, 65535)
    _check(uvo, m, q, _low_entropy(rng, 33), "nq=65535 low entropy")
    m.close()


# ---- host form with a mask: k_knn2 ----------------------------------------------------------------------------------------------

def _mask(rng, nq, nt, kind):
    mk = np.zeros((nq, nt), np.uint8)
    if nt == 0:
        return mk
    rows = np.arange(nq)
    if kind == "random":
        mk = (rng.random((nq, nt)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (nq, nt), dtype=np.uint8)   # any non-zero byte allows
        mk[::7] = 0                                     # all-zero rows among them
    elif kind == "one":
        mk[rows, rng.integers(0, nt, nq)] = 1
    elif kind == "two":
        mk[rows, rng.integers(0, nt, nq)] = 1
        mk[rows, rng.integers(0, nt, nq)] = 255           # the same column now and then: one allowed row
    elif kind == "last":
        mk[:, nt - 1] = 1
    elif kind == "none":
        pass
    elif kind == "all":
        mk[:] = 1
    return mk


MASK_KINDS = ("random", "one", "two", "last", "none", "all")


@pytest.mark.parametrize("kind", ["low_entropy", "planted"])
def test_knn2_masked_size_sweep(uvo, kind):
    """k_knn2: 256 queries per workgroup, train tiles of 128.  All four outputs, under masks that leave no, one, two, only the last
    or every train row."""
    rng = np.random.default_rng(111 if kind == "low_entropy" else 112)
    m = uvo.ORBmatcher(0.8, max_query=600, max_train=300)
    for nt in (300, 257, 256, 255, 130, 129, 128, 127, 65, 33, 32, 31, 3, 2, 1, 0):
        for nq in (1, 33, 255, 256, 257, 513):
            if kind == "low_entropy":
                q, t = _low_entropy(rng, nq), _low_entropy(rng, nt)
            else:
                q = _random(rng, nq)
                t = _planted(rng, q, nt)
            for mk in MASK_KINDS:
                _check(uvo, m, q, t, "%s mask=%s nq=%d nt=%d" % (kind, mk, nq, nt), _mask(rng, nq, nt, mk))
    m.close()


def test_knn2_masked_second_best(uvo):
    """A masked-out row that would be the second best (and one that would be the best) must not come back as either."""
    rng = np.random.default_rng(113)
    m = uvo.ORBmatcher(0.8, max_query=300, max_train=800)
    for nq in (60, 257):
        nt = 3 * nq + 17
        q, t = _random(rng, nq), _random(rng, nt)
        plan = rng.permutation(nt)[:3 * nq].reshape(nq, 3)       # three train rows of its own per query, anywhere in the set ...
        for i in range(nq):
            for r, f in zip(plan[i], (0, 2, 4)):                 # ... at distances 0, 2 and 4; every other row is about 128 away
                t[r] = _flip(q[i], f, r)
        for drop in (0, 1, 2):
            mk = np.ones((nq, nt), np.uint8)
            mk[np.arange(nq), plan[:, drop]] = 0
            idx0, d0, idx1, d1 = _check(uvo, m, q, t, "nq=%d, rank %d masked out" % (nq, drop), mk)
            keep = [c for c in (0, 1, 2) if c != drop]
            assert (idx0 == plan[:, keep[0]]).all() and (idx1 == plan[:, keep[1]]).all()
    m.close()


def test_knn2_python_wrapper(uvo):
    """ORBmatcher.knn2, the wrapper the tests above go round to prefill the outputs: masked and unmasked, empty sets included."""
    rng = np.random.default_rng(115)
    m = uvo.ORBmatcher(0.8, max_query=300, max_train=200)
    for nq, nt in ((0, 7), (5, 0), (1, 1), (33, 2), (129, 65), (257, 130)):
        for kind in ("low_entropy", "planted"):
            if kind == "low_entropy" or nq == 0:
                q, t = _low_entropy(rng, nq), _low_entropy(rng, nt)
            else:
                q = _random(rng, nq)
                t = _planted(rng, q, nt)
            for mk in (None, "random", "one", "all"):
                mask = None if mk is None else _mask(rng, nq, nt, mk)
                got = m.knn2(q, t, mask)
                assert got[1].dtype == np.uint16 and got[3].dtype == np.uint16 and all(len(a) == nq for a in got)
                _same(got, hm.knn2(q, t, mask), "wrapper %s mask=%s nq=%d nt=%d" % (kind, mk, nq, nt))
    m.close()


@pytest.mark.parametrize("ratio", [1.0, 0.8, 0.6, 0.0])
def test_ratio_matching_against_the_model(uvo, ratio):
    rng = np.random.default_rng(114)
    m = uvo.ORBmatcher(0.8, max_query=600, max_train=300)
    ties = 0
    for nq, nt in ((0, 5), (5, 0), (1, 1), (1, 2), (257, 130), (513, 33)):
        for kind in ("low_entropy", "planted"):
            if kind == "low_entropy" or nq == 0:
                q, t = _low_entropy(rng, nq), _low_entropy(rng, nt)
            else:
                q = _random(rng, nq)
                t = _planted(rng, q, nt)
            for mk in (None, "random", "one", "two", "all"):
                mask = None if mk is None else _mask(rng, nq, nt, mk)
                got = m.ratio_matching(q, t, ratio, mask)
                want = hm.ratio_matches(q, t, ratio, mask)
                np.testing.assert_array_equal(got, want, err_msg="ratio %g %s mask=%s nq=%d nt=%d" % (ratio, kind, mk, nq, nt))
                if nq and nt:
                    w = hm.knn2(q, t, mask)
                    ties += int(((w[2] >= 0) & (w[1] == w[3])).sum())
    m.close()
    assert ties > 100     # d0 == d1 occurred: accepted at ratio 1.0, and at any ratio when both are 0


# ---- batched, HBM-resident form: uvo_hamming_knn2_batch_device ------------------------------------------------------------------

def _clamp(n, cap):
    return min(max(int(n), 0), cap)


def _batch_buffers(rng, counts_q, counts_t, q_stride, t_stride, head):
    """Query and train buffers of len(counts) + 1 slices (the spare slice keeps a kernel without clamps inside the allocation).
    Train slice p: rows below the count are random with near-copies of the pair's queries planted; rows at and past the count are
    exact copies of the pair's queries; the first `head` rows of every slice carry exact copies of the PREVIOUS pair's queries (all
    of them while they are live rows, every other one where they are dead rows), which is what a count above the stride reaches.
    Query slices are arbitrary past their counts."""
    P = len(counts_q)
    q = _random(rng, (P + 1) * q_stride).reshape(P + 1, q_stride, 32)
    t = _random(rng, (P + 1) * t_stride).reshape(P + 1, t_stride, 32)
    for p in range(P + 1):
        nq = _clamp(counts_q[p], q_stride) if p < P else 0
        nt = _clamp(counts_t[p], t_stride) if p < P else 0
        nq_prev = _clamp(counts_q[p - 1], q_stride) if p > 0 else 0
        for j in range(t_stride):
            from_prev = nq_prev > 0 and j < head and (j < nt or j % 2 == 1)
            if from_prev:
                t[p, j] = q[p - 1, j % nq_prev]
            elif nq > 0 and j >= nt:
                t[p, j] = q[p, (j - nt) % nq]
            elif nq > 0 and j % 3 == 0:
                t[p, j] = _flip(q[p, (j // 3) % nq], 1 + (j // 3 // nq) % 3, j)
    return q, t


def _run_batch(uvo, mt, q, t, counts_q, counts_t, q_stride, t_stride, max_query):
    import torch
    dev = torch.device("cuda", 0)
    P = len(counts_q)
    d_q, d_t = torch.from_numpy(q.reshape(-1, 32)).to(dev), torch.from_numpy(t.reshape(-1, 32)).to(dev)
    d_nq = torch.tensor(counts_q, dtype=torch.int32, device=dev)
    d_nt = torch.tensor(counts_t, dtype=torch.int32, device=dev)
    i0 = torch.full((P + 1, max_query), IDX_FILL, dtype=torch.int32, device=dev)      # one spare row set, as for the inputs
    i1 = torch.full((P + 1, max_query), IDX_FILL, dtype=torch.int32, device=dev)
    d0 = torch.full((P + 1, max_query), D_FILL - 65536, dtype=torch.int16, device=dev)
    d1 = torch.full((P + 1, max_query), D_FILL - 65536, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mt.knn2_batch_device(P, d_q.data_ptr(), d_nq.data_ptr(), q_stride, d_t.data_ptr(), d_nt.data_ptr(), t_stride, i0.data_ptr(), d0.data_ptr(),
                         i1.data_ptr(), d1.data_ptr())
    mt.synchronize()
    u16 = lambda x: x.cpu().numpy().view(np.uint16).astype(np.int32)
    return i0.cpu().numpy(), u16(d0), i1.cpu().numpy(), u16(d1)


def _expect_batch(q, t, counts_q, counts_t, q_stride, t_stride, max_query):
    P = len(counts_q)
    want = [np.full((P + 1, max_query), f, np.int32) for f in (IDX_FILL, D_FILL, IDX_FILL, D_FILL)]
    for p in range(P):
        nq, nt = _clamp(counts_q[p], q_stride), _clamp(counts_t[p], t_stride)
        for w, r in zip(want, hm.knn2(q[p, :nq], t[p, :nt])):
            w[p, :nq] = r
    return want


@pytest.mark.parametrize("max_query,q_stride,t_stride,over", [(96, 80, 50, 5), (300, 200, 77, 13)])
def test_knn2_batch_device_clamps_and_strides(uvo, max_query, q_stride, t_stride, over):
    """Every count of {0, 1, 33, stride - 1, stride, stride + over, negative} for the queries against every one for the train rows, as
    49 pairs of one launch; q_stride < max_query (the output pitch is max_query) and t_stride != q_stride.  Rows past
    min(d_nq[p], q_stride) keep their prefill; train rows past min(d_nt[p], t_stride) are ignored although they would win."""
    rng = np.random.default_rng(121)
    cq = [0, 1, 33, q_stride - 1, q_stride, q_stride + over, -3]
    ct = [0, 1, 33, t_stride - 1, t_stride, t_stride + over, -7]
    counts_q = [a for a in cq for _ in ct]
    counts_t = [b for _ in cq for b in ct]
    P = len(counts_q)
    q, t = _batch_buffers(rng, counts_q, counts_t, q_stride, t_stride, head=over + 3)
    mt = uvo.ORBmatcher(0.8, max_query=max_query, max_train=16, max_batch=P)
    got = _run_batch(uvo, mt, q, t, counts_q, counts_t, q_stride, t_stride, max_query)
    mt.close()
    want = _expect_batch(q, t, counts_q, counts_t, q_stride, t_stride, max_query)
    _same(got, want, "max_query=%d q_stride=%d t_stride=%d" % (max_query, q_stride, t_stride))
    # the inputs did what they were built for: with the dead rows let in, answers change (so a lost clamp or guard cannot pass)
    changed = 0
    for p in range(P):
        nq, nt = _clamp(counts_q[p], q_stride), _clamp(counts_t[p], t_stride)
        if nq and nt < t_stride:
            loose = hm.knn2(q[p, :nq], t[p])
            changed += int((loose[0] != want[0][p, :nq]).any())
        if nq and counts_t[p] > t_stride:
            loose = hm.knn2(q[p, :nq], t[p:p + 2].reshape(-1, 32)[:counts_t[p]])
            changed += int((loose[0] != want[0][p, :nq]).any())
    assert changed == 5 * 5 + 5 * 1     # five live query counts x (five train counts below the stride + the one above it)


def test_knn2_batch_device_full_train_slice(uvo):
    """t_stride = 65535, the largest the contract allows: one pair with exactly 65535 rows, one whose count lies above the stride."""
    rng = np.random.default_rng(122)
    q_stride, t_stride, max_query = 64, 65535, 100
    counts_q, counts_t = [64, 40], [65535, 70000]
    q = _random(rng, 3 * q_stride).reshape(3, q_stride, 32)
    t = _random(rng, 3 * t_stride).reshape(3, t_stride, 32)
    for p in range(2):
        _plant_high(q[p, :counts_q[p]], t[p])
        t[p + 1, :16] = q[p, :16]                     # what a count above the stride would reach: exact copies
    mt = uvo.ORBmatcher(0.8, max_query=max_query, max_train=16, max_batch=2)
    got = _run_batch(uvo, mt, q, t, counts_q, counts_t, q_stride, t_stride, max_query)
    mt.close()
    want = _expect_batch(q, t, counts_q, counts_t, q_stride, t_stride, max_query)
    for p in range(2):
        _assert_high([w[p, :counts_q[p]] for w in want])
    _same(got, want, "t_stride=65535")


def test_knn2_batch_device_bad_arguments(uvo):
    import torch
    dev = torch.device("cuda", 0)
    mt = uvo.ORBmatcher(0.8, max_query=64, max_train=64, max_batch=2)
    buf = torch.zeros(4 * 65536 * 32, dtype=torch.uint8, device=dev)     # large enough for whatever a missing check would launch
    n = torch.zeros(8, dtype=torch.int32, device=dev)
    out = [torch.zeros(8 * 64, dtype=torch.int32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()

    def call(pairs, q_stride, t_stride):
        mt.knn2_batch_device(pairs, buf.data_ptr(), n.data_ptr(), q_stride, buf.data_ptr(), n.data_ptr(), t_stride, out[0].data_ptr(),
                             out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr())

    call(2, 64, 65535)                                                    # the limits themselves are fine
    for pairs, q_stride, t_stride in ((2, 65, 64), (2, 64, 65536), (3, 64, 64), (0, 64, 64), (2, 0, 64), (2, 64, 0)):
        with pytest.raises(uvo.UvoError) as e:
            call(pairs, q_stride, t_stride)
        assert e.value.code == uvo.UVO_E_BADARG, (pairs, q_stride, t_stride)
    mt.synchronize()
    mt.close()


# ---- k_matrix and k_medoid ------------------------------------------------------------------------------------------------------

def test_distance_matrix_against_the_model(uvo):
    """k_matrix: 256 queries per workgroup, 128 train rows per tile; both sides of both."""
    rng = np.random.default_rng(131)
    m = uvo.ORBmatcher(0.8, max_query=600, max_train=300)
    for nq in (1, 255, 256, 257, 513):
        for nt in (1, 127, 128, 129, 257):
            for kind in ("random", "low_entropy"):
                q, t = (_random(rng, nq), _random(rng, nt)) if kind == "random" else (_low_entropy(rng, nq), _low_entropy(rng, nt))
                q[nq - 1], t[nt - 1] = 255, 255                # the last row of each side, in the last (partial) workgroup / tile
                q[0], t[nt // 2] = 0, 0
                if nq > 1:
                    q[nq // 2] = t[0]
                want = hm.distance_matrix(q, t)
                got = m.distance_matrix(q, t)
                assert got.dtype == np.uint16
                np.testing.assert_array_equal(got.astype(np.int32), want, err_msg="%s nq=%d nt=%d" % (kind, nq, nt))
                assert want.min() == 0 and (nq == 1 or nt == 1 or want.max() == 256)
    m.close()


MEDOID_N = list(range(0, 41)) + [255, 256, 257, 511, 1000]


@pytest.mark.parametrize("kind", ["random", "low_entropy", "identical", "clustered"])
def test_medoid_against_the_model(uvo, kind):
    """k_medoid: one workgroup per map point, one thread per row (strided above 256).  Every n from 0 to 40, even and odd (the
    median position int(0.5 * (n - 1)) is the lower median for even n), around 256 and 512; as one batch that mixes empty and
    non-empty points, and point by point."""
    rng = np.random.default_rng(141)
    m = uvo.ORBmatcher(0.8)

    def make(n):
        if kind == "random":
            return _random(rng, n)
        if kind == "low_entropy":
            return _low_entropy(rng, n)              # medians tie: the first index must win
        if kind == "identical":
            return np.repeat(_random(rng, 1), n, 0)
        centre = _random(rng, 1)[0]                  # rows a few bits from a centre, the centre itself somewhere in the middle
        d = np.stack([_flip(centre, 1 + i % 9, i) for i in range(n)]) if n else np.zeros((0, 32), np.uint8)
        if n > 2:
            d[n // 2] = centre
        return d

    lists = [make(n) for n in MEDOID_N] + [np.zeros((0, 32), np.uint8), make(7), np.zeros((0, 32), np.uint8)]
    want = [hm.medoid(d) for d in lists]
    idx, med = m.distinctive_descriptors(lists)
    assert list(zip(idx.tolist(), med.tolist())) == want, kind
    for d, w in zip(lists[:45], want):               # alone: offsets start at 0 for every point
        i1, m1 = m.distinctive_descriptors([d])
        assert (int(i1[0]), int(m1[0])) == w, (kind, len(d))
    m.close()
    assert want[0] == (-1, -1) and want[-1] == (-1, -1)
    if kind == "identical":
        assert all(w == (0, 0) for w, d in zip(want, lists) if len(d))
