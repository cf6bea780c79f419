"""The numpy Hamming model (tests/hamming_model.py) held to hand-computed cases and to the C++ oracle.  No GPU: this ties the two
references of tests/test_gpu_hamming.py together."""
import numpy as np
import pytest

import hamming_model as hm


def _bits(*positions):
    """A descriptor with exactly the given bit positions (0 .. 255) set."""
    d = np.zeros(32, np.uint8)
    for p in positions:
        d[p >> 3] |= 1 << (p & 7)
    return d


def _low_entropy(rng, n):
    return rng.choice(np.array([0, 1, 128, 255], np.uint8), (n, 32), p=[0.7, 0.1, 0.1, 0.1])


def test_distance_by_hand():
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    a = _bits(0, 63, 64, 255)
    dm = hm.distance_matrix(np.stack([z, o, a]), np.stack([z, o, a, _bits(0), _bits(7, 8, 200)]))
    assert dm.dtype == np.int32
    assert dm.tolist() == [[0, 256, 4, 1, 3], [256, 0, 252, 255, 253], [4, 252, 0, 3, 7]]
    assert hm.distance_matrix(np.zeros((0, 32), np.uint8), o[None]).shape == (0, 1)
    assert hm.distance_matrix(o[None], np.zeros((0, 32), np.uint8)).shape == (1, 0)


def test_distance_is_the_bit_count_of_the_xor():
    rng = np.random.default_rng(1)
    q, t = rng.integers(0, 256, (37, 32), dtype=np.uint8), rng.integers(0, 256, (53, 32), dtype=np.uint8)
    ref = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2)
    np.testing.assert_array_equal(hm.distance_matrix(q, t), ref)


def test_knn2_by_hand():
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    # distances 0 and 256, both orders
    i0, d0, i1, d1 = hm.knn2(np.stack([z, o]), np.stack([o, z]))
    assert (i0.tolist(), d0.tolist(), i1.tolist(), d1.tolist()) == ([1, 0], [0, 0], [0, 1], [256, 256])
    # a three-way tie at distance 1 behind nothing nearer: the two lowest indices, in order
    t = np.stack([_bits(5, 6), _bits(1), _bits(2), _bits(3)])
    i0, d0, i1, d1 = hm.knn2(z[None], t)
    assert (i0[0], d0[0], i1[0], d1[0]) == (1, 1, 2, 1)
    # the same tie with a nearer row behind it
    i0, d0, i1, d1 = hm.knn2(z[None], np.concatenate([t, z[None]]))
    assert (i0[0], d0[0], i1[0], d1[0]) == (4, 0, 1, 1)
    # one train row, no train row
    i0, d0, i1, d1 = hm.knn2(z[None], _bits(1, 2, 3)[None])
    assert (i0[0], d0[0], i1[0], d1[0]) == (0, 3, -1, 0xFFFF)
    i0, d0, i1, d1 = hm.knn2(z[None], np.zeros((0, 32), np.uint8))
    assert (i0[0], d0[0], i1[0], d1[0]) == (-1, 0xFFFF, -1, 0xFFFF)
    assert all(len(x) == 0 for x in hm.knn2(np.zeros((0, 32), np.uint8), t))


def test_knn2_masks_by_hand():
    z = np.zeros(32, np.uint8)
    t = np.stack([_bits(5, 6), _bits(1), _bits(2), z])          # distances 2, 1, 1, 0 from z
    q = np.stack([z, z, z, z])
    mask = np.array([[1, 1, 1, 0],     # the nearest masked out: the tie at distance 1, lower index first
                     [0, 0, 1, 0],     # a single allowed row
                     [0, 0, 0, 0],     # none
                     [9, 0, 0, 1]], np.uint8)   # any non-zero byte allows
    i0, d0, i1, d1 = hm.knn2(q, t, mask)
    assert i0.tolist() == [1, 2, -1, 3] and d0.tolist() == [1, 1, 0xFFFF, 0]
    assert i1.tolist() == [2, -1, -1, 0] and d1.tolist() == [1, 0xFFFF, 0xFFFF, 2]


def test_medoid_by_hand():
    assert hm.medoid(np.zeros((0, 32), np.uint8)) == (-1, -1)
    assert hm.medoid(_bits(3)[None]) == (0, 0)
    # two rows: k = int(0.5) = 0, every median is the self-distance 0, the first row wins
    assert hm.medoid(np.stack([_bits(3), _bits(4, 5)])) == (0, 0)
    # three rows on a line, distances 0-1: 2, 1-2: 3, 0-2: 5; k = 1: medians 2, 2, 3 -> first of the tie
    a, b, c = _bits(), _bits(0, 1), _bits(0, 1, 2, 3, 4)
    assert hm.medoid(np.stack([a, b, c])) == (0, 2)
    assert hm.medoid(np.stack([c, b, a])) == (1, 2)   # rows c, b, a: medians 3, 2, 2
    # four rows, k = int(1.5) = 1 (the lower median); d adds the distances a-d: 7, b-d: 5, c-d: 2
    d = _bits(0, 1, 2, 3, 4, 5, 6)
    # sorted rows: a: 0 2 5 7, b: 0 2 3 5, c: 0 2 3 5, d: 0 2 5 7 -> every median is 2, the first row wins
    assert hm.medoid(np.stack([a, b, c, d])) == (0, 2)
    assert hm.medoid(np.stack([b, d, c])) == (1, 2)   # b: 0 3 5 -> 3, d: 0 2 5 -> 2, c: 0 2 3 -> 2
    # five rows, k = 2, an all-ones row in front: o: 0 249 251 254 256 -> 251; a: 0 2 5 7 256 -> 5; b: 0 2 3 5 254 -> 3;
    # c: 0 2 3 5 251 -> 3; d: 0 2 5 7 249 -> 5
    o = np.full(32, 255, np.uint8)
    assert hm.medoid(np.stack([o, a, b, c, d])) == (2, 3)


def test_ratio_matches_by_hand():
    z = np.zeros(32, np.uint8)
    t = np.stack([_bits(0, 1, 2, 3), _bits(4, 5, 6, 7, 8)])          # distances 4 and 5 from z
    q = z[None]
    assert hm.ratio_matches(q, t, 0.8).tolist() == [[0, 0, 4]]       # 4 <= 5 * 0.8 = 4.0 exactly, in double
    assert hm.ratio_matches(q, t, 0.79).tolist() == []
    assert hm.ratio_matches(q, np.stack([t[0], t[0]]), 1.0).tolist() == [[0, 0, 4]]   # d0 == d1 passes at ratio 1
    assert hm.ratio_matches(q, t[:1], 1.0).tolist() == []            # fewer than two neighbours: nothing
    assert hm.ratio_matches(q, t, 1.0, np.array([[0, 1]], np.uint8)).tolist() == []
    assert hm.ratio_matches(np.zeros((0, 32), np.uint8), t, 1.0).shape == (0, 3)
    assert hm.ratio_matches(q, np.zeros((0, 32), np.uint8), 1.0).shape == (0, 3)
    # distance 0 against distance 0 at ratio 0
    assert hm.ratio_matches(q, np.stack([z, z]), 0.0).tolist() == [[0, 0, 0]]


def _oracle_knn2(oracle, q, t, mask=None):
    i0, d0, i1, d1 = oracle.knn2(q, t, mask)
    return i0, np.where(i0 < 0, 0xFFFF, d0), i1, np.where(i1 < 0, 0xFFFF, d1)   # the oracle writes -1 for "no distance"


@pytest.mark.parametrize("kind", ["random", "low_entropy"])
def test_knn2_against_the_oracle(oracle, kind):
    rng = np.random.default_rng(11 if kind == "random" else 12)
    make = (lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)) if kind == "random" else (lambda n: _low_entropy(rng, n))
    for nq, nt in ((1, 1), (1, 2), (3, 0), (0, 3), (17, 1), (64, 33), (33, 64), (130, 300), (300, 129), (257, 31)):
        q, t = make(nq), make(nt)
        if kind == "random" and nt > 4 and nq > 4:
            t[:3] = q[:3]
            t[nt - 1] = q[4]
        for mask in (None, (rng.random((nq, nt)) < 0.3).astype(np.uint8), (rng.random((nq, nt)) < 0.02).astype(np.uint8)):
            got, want = hm.knn2(q, t, mask), _oracle_knn2(oracle, q, t, mask)
            for g, w, name in zip(got, want, ("idx0", "d0", "idx1", "d1")):
                np.testing.assert_array_equal(g, w, err_msg="%s %s nq=%d nt=%d" % (kind, name, nq, nt))


@pytest.mark.parametrize("kind", ["random", "low_entropy", "identical"])
def test_medoid_against_the_oracle(oracle, kind):
    rng = np.random.default_rng(21)
    for n in list(range(0, 41)) + [255, 256, 257]:
        if kind == "random":
            d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        elif kind == "low_entropy":
            d = _low_entropy(rng, n)
        else:
            d = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), n, 0)
        want = oracle.distinctive_descriptor(d) if n else (-1, -1)
        assert hm.medoid(d) == want, (kind, n)


def test_distance_against_the_oracle(oracle):
    rng = np.random.default_rng(31)
    q = np.concatenate([rng.integers(0, 256, (20, 32), dtype=np.uint8), _low_entropy(rng, 20), np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)])
    dm = hm.distance_matrix(q, q)
    assert dm.min() == 0 and dm.max() == 256
    for i in range(len(q)):
        for j in range(len(q)):
            assert dm[i, j] == oracle.descriptor_distance(q[i], q[j])
