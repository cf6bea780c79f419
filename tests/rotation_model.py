"""The rotation-consistency filter of the ORBmatcher search loops in plain Python: the bin of a match (src/ORBmatcher.cc:168,235-240,
float32 throughout), ComputeThreeMaxima (:1748-1789) and the removal of every match outside the three kept bins (:263-284).  Held to
oracle.compute_three_maxima by tests/test_window_model.py, run against k_rot_filter by tests/test_gpu_windows.py.

The reference asserts 0 <= bin < 30 and takes angles in [0, 360), so that a difference lies in [0, 360] and its bin in 0..12.  A
difference that is NaN has no reference behaviour; the library documents that such a match lands in no bin and is dropped, and the
model says the same.  Finite differences beyond 360 are outside what the model states: the cases hold none."""
import numpy as np

f32 = np.float32
HISTO_LENGTH = 30
FACTOR = f32(1.0) / f32(HISTO_LENGTH)                                   # const float factor = 1.0f/HISTO_LENGTH


def rot_of(qa, ta):
    with np.errstate(all="ignore"):
        rot = f32(f32(qa) - f32(ta))
        if float(rot) < 0.0:
            rot = f32(rot + f32(360.0))
    return rot


def bin_of(qa, ta):
    """-> bin 0..29, or -2 for a match that lands in no bin"""
    rot = rot_of(qa, ta)
    if not np.isfinite(rot):
        return -2
    v = float(f32(rot * FACTOR))
    b = int(np.copysign(np.floor(abs(v) + 0.5), v))                     # round(): half away from zero, exact in float64
    if b == HISTO_LENGTH:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else -2


def compute_three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return [ind1, ind2, ind3]


def rot_filter(match, dist, qangle, tangle):
    """match[nq] / dist[nq] before the filter -> (match, dist, n_matches) after it"""
    match, dist = np.array(match, np.int64), np.array(dist, np.int64)
    bins = np.array([bin_of(qangle[i], tangle[t]) if t >= 0 else -1 for i, t in enumerate(match)], np.int64)
    hist = [int((bins == b).sum()) for b in range(HISTO_LENGTH)]
    keep = compute_three_maxima(hist)
    drop = (match >= 0) & ~np.isin(bins, [k for k in keep if k >= 0])
    match[drop], dist[drop] = -1, -1
    return match, dist, int((match >= 0).sum()), hist, keep


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def from_rots(rots):
    """query i matched to target i with rot_i = qa - ta: ta = 0 and qa = rot where rot >= 0; a negative rot from qa = 0, ta = -rot"""
    rots = np.asarray(rots, f32)
    neg = rots < 0
    qa = np.where(neg, f32(0), rots).astype(f32)
    ta = np.where(neg, -rots, f32(0)).astype(f32)
    return qa, ta


def from_hist(counts, rng):
    """counts: {bin: population} -> rots inside the bins (30 * bin +- 10 degrees, kept inside [0, 360)), shuffled.  With
    factor = 1 / 30 differences in [0, 360) reach the bins 0..12 only."""
    rots = []
    for b, c in counts.items():
        assert 0 <= b <= 12
        rots += [float(v) for v in rng.uniform(max(30.0 * b - 10, 0.0), min(30.0 * b + 10, 359.5), c)]
    rots = np.asarray(rots, f32)
    rng.shuffle(rots)
    return rots


def cases():
    """name -> rots[nq] (NaN = a match whose angle difference is NaN); what each is for is in its name"""
    rng = np.random.default_rng(23)
    below = lambda v: float(np.nextafter(f32(v), f32(0)))
    tiny = -float(np.nextafter(f32(0), f32(1)))                         # the smallest negative difference: + 360 gives 360 exactly
    c = {
        # 15 * factor is 0.5 exactly; 45 and 345 land one float above 1.5 and 11.5, their lower neighbours exactly on them
        "ties_15_45_345": [15.0] * 5 + [45.0] * 4 + [345.0] * 3 + [30.0] * 2 + [0.0] + [below(45.0)] * 2 + [below(345.0)] * 2 + [below(15.0)],
        "zero_and_smallest_negative": [0.0] * 3 + [tiny] * 4 + [-30.0] * 2 + [359.9] + [-1e-3] * 2,
        "wrap": [-15.0] * 4 + [-345.0] * 3 + [-0.5] * 2 + [-359.5],
        "three_equal_bins": from_hist({4: 6, 7: 6, 11: 6}, rng),
        "four_equal_bins": from_hist({2: 5, 5: 5, 9: 5, 12: 5}, rng),
        "tie_for_third": from_hist({3: 9, 8: 7, 10: 4, 11: 4}, rng),
        "tie_for_first": from_hist({6: 8, 9: 8, 12: 3}, rng),
        "ten_percent_kept": from_hist({5: 20, 12: 2, 8: 2, 1: 1}, rng),
        "ten_percent_third_dropped": from_hist({5: 20, 12: 2, 8: 1}, rng),
        "ten_percent_second_dropped": from_hist({5: 20, 12: 1, 8: 1}, rng),
        "thirty_and_three": from_hist({0: 30, 12: 3, 6: 3, 7: 2}, rng),
        "one_bin": from_hist({10: 9}, rng),
        "nq_1": [77.0],
        "nan_difference": [float("nan")] * 3 + [40.0] * 4 + [100.0] * 2 + [200.0] + [300.0],
        "nq_1024": from_hist({1: 400, 2: 300, 10: 200, 7: 100, 12: 24}, rng),
        "nq_1025": from_hist({0: 400, 2: 300, 10: 200, 7: 100, 12: 25}, rng),
    }
    return {k: np.asarray(v, f32) for k, v in c.items()}
