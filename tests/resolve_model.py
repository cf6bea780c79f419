"""A sequential model of the order-dependent matcher loops, and constructed scenes whose answers are known.  Test infrastructure only.

resolve() restates the loops of src/ORBmatcher.cc the way the reference runs them -- queries 0..nq-1 visited once, in order, against one
mutable taken[] (SearchForInitialization: matched_distance[] and holder[]) -- for the seven rules of include/uvo/uvo.h.  It is written
from the reference and the rule table, not from the kernels, which solve the same loops as a parallel fixed point (every query chooses,
ownership goes to the lowest query index, repeat until nothing changes).

jacobi_sweeps() simulates that parallel iteration, one numpy step per sweep, and returns how many sweeps it takes.  It exists only to
prove that a scene is adversarial (that its dependency chain is as deep as intended); expected results never come from it.

Scenes (each returns a Scene: descriptors, candidate lists, target levels, and the closed-form answer where there is one):
  domino(N)        query 0 sees t0; query j sees [t(j-1), t(j)] at distances 5 and 20.  Alone every query wants its left target; in
                   sequence query j ends on t(j).  Depth N.
  steal_domino(N)  the same lists, both distances 20.  Alone a query is rejected (20 < 0.9 * 20 fails); in sequence its left target is
                   already matched at 20 and skipped, so it accepts t(j).  Depth N.
  pile(nq, K)      one all-to-all group, target k at distance k from every query.  Under a rule that takes the best free target, query i
                   ends on target i while i <= max_dist, -1 after that.  Depth max_dist + 1 (+ 1 sweep in which the rest let go).
  contention(...)  random short lists over few targets, descriptors from a handful of prototypes so that ties, equal best and second
                   and d == max_dist are common; empty lists in front, between and behind; blocked targets; d = 0 and d = 256 pairs.
"""
import numpy as np

# include/uvo/uvo.h
RULE_BEST_RATIO_SAME_LEVEL, RULE_BEST_ONLY, RULE_BEST_RATIO_LE, RULE_BEST_RATIO_LT, RULE_TRIANGULATION, RULE_BEST_RATIO_LEQ, RULE_INIT_STEAL = range(7)
RULES = tuple(range(7))
RULE_NAMES = ("same_level", "best_only", "ratio_le", "ratio_lt", "triangulation", "ratio_leq", "init_steal")
INT_MAX = 0x7fffffff
f32 = np.float32


class Hamming:
    """D(i, t): the 256-bit Hamming distance of query row i and target row t, by np.unpackbits.  Values are kept, a scene is resolved
    under many rules."""

    def __init__(self, qdesc, tdesc):
        self.q = np.unpackbits(np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32), axis=1)
        self.t = np.unpackbits(np.ascontiguousarray(tdesc, np.uint8).reshape(-1, 32), axis=1)
        self.seen = {}

    def __call__(self, i, t):
        k = (i, t)
        d = self.seen.get(k)
        if d is None:
            d = self.seen[k] = int(np.count_nonzero(self.q[i] != self.t[t]))
        return d


def _accepts(rule, max_dist, ratio, best, best2, level, level2):
    """The acceptance test behind best / second best; ratio is float32 and the products are float32, as `float * int` is."""
    if rule == RULE_BEST_RATIO_SAME_LEVEL:   # :114-117
        return best <= max_dist and not (level == level2 and f32(best) > ratio * f32(best2))
    if rule == RULE_BEST_ONLY:               # :1701, :1101
        return best <= max_dist
    if rule == RULE_BEST_RATIO_LE:           # :216-218
        return best <= max_dist and f32(best) < ratio * f32(best2)
    if rule == RULE_BEST_RATIO_LT:           # :786-788
        return best < max_dist and f32(best) < ratio * f32(best2)
    if rule == RULE_BEST_RATIO_LEQ:          # :476
        return f32(best) <= f32(best2) * ratio and best <= max_dist
    raise ValueError(rule)


def resolve(rule, max_dist, nn_ratio, exclusive, cand_lists, D, tlevel=None, pred=None, blocked=None):
    """-> match[nq] (target or -1), dist[nq] (its distance or -1), nmatches.

    cand_lists[i]: the candidate targets of query i in list order (`d < bestDist` is strict: of equals the earlier entry wins);
    D(i, t): distance; tlevel[t]: octave (SAME_LEVEL); pred(i, t): the epipolar predicate (TRIANGULATION; None = always true);
    blocked[t] != 0: unavailable from the start.  INIT_STEAL has neither exclusivity nor blocked targets: both are ignored."""
    nq = len(cand_lists)
    match, dist = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    ratio = f32(nn_ratio)
    if rule == RULE_INIT_STEAL:              # :598-680
        matched_distance, holder = {}, {}
        for i in range(nq):
            best, best2, best_t = INT_MAX, INT_MAX, -1
            for t in cand_lists[i]:
                t = int(t)
                d = D(i, t)
                if matched_distance.get(t, INT_MAX) <= d:        # :637
                    continue
                if d < best:
                    best2, best, best_t = best, d, t
                elif d < best2:
                    best2 = d
            if best <= max_dist and f32(best) < f32(best2) * ratio:   # :652-654
                if holder.get(best_t, -1) >= 0:                    # :656-660: the holder is displaced
                    match[holder[best_t]] = -1
                    dist[holder[best_t]] = -1
                match[i], dist[i] = best_t, best
                holder[best_t] = i
                matched_distance[best_t] = best
        return match, dist, int((match >= 0).sum())
    taken = set(int(t) for t in np.nonzero(np.asarray(blocked))[0]) if blocked is not None else set()
    none = 256 if rule == RULE_BEST_RATIO_SAME_LEVEL else INT_MAX       # :80-82 against INT_MAX everywhere else
    for i in range(nq):
        choice, cd = -1, -1
        if rule == RULE_TRIANGULATION:       # :902-957
            free = sorted((D(i, int(t)), int(t)) for t in cand_lists[i] if int(t) not in taken and D(i, int(t)) <= max_dist)
            if free:
                dist_th = 2 * free[0][0]
                for d, t in free:
                    if d > dist_th:
                        break
                    if pred is None or pred(i, t):
                        choice, cd = t, d
                        break
        else:
            best, best2, level, level2, best_t = none, none, -1, -1, -1
            for t in cand_lists[i]:
                t = int(t)
                if t in taken:
                    continue
                d = D(i, t)
                lv = int(tlevel[t]) if tlevel is not None else 0
                if d < best:
                    best2, level2 = best, level
                    best, level, best_t = d, lv, t
                elif d < best2:
                    best2, level2 = d, lv
            if best_t >= 0 and _accepts(rule, max_dist, ratio, best, best2, level, level2):
                choice, cd = best_t, best
        if choice >= 0:
            match[i], dist[i] = choice, cd
            if exclusive:
                taken.add(choice)
    return match, dist, int((match >= 0).sum())


# ---- the parallel iteration, for depth only ---------------------------------------------------------------------------------------

def _pad(cand_lists, fill=-1):
    nq = len(cand_lists)
    width = max(1, max((len(c) for c in cand_lists), default=1))
    C = np.full((nq, width), fill, np.int64)
    for i, c in enumerate(cand_lists):
        C[i, :len(c)] = c
    return C


def jacobi_sweeps(rule, max_dist, nn_ratio, exclusive, cand_lists, D, nt, tlevel=None, pred=None, blocked=None, limit=None):
    """How many sweeps of the parallel iteration change a choice: sweep = every query chooses against the ownership the sweep before
    left (owner[t] = lowest query whose choice is t; the steal rule: what the accepts of lower queries left on t).  A sequential loop
    takes one such sweep when no query depends on another."""
    nq = len(cand_lists)
    C = _pad(cand_lists)
    valid = C >= 0
    Cs = np.where(valid, C, 0)
    Dm = np.zeros(C.shape, np.int64)
    P = np.ones(C.shape, bool)
    for i in range(nq):
        for k, t in enumerate(cand_lists[i]):
            Dm[i, k] = D(i, int(t))
            if pred is not None:
                P[i, k] = bool(pred(i, int(t)))
    L = (np.asarray(tlevel, np.int64)[Cs] if tlevel is not None else np.zeros(C.shape, np.int64))
    me = np.arange(nq)[:, None]
    ratio = f32(nn_ratio)
    BIG = 1 << 40
    owner = np.full(nt, BIG, np.int64)
    if blocked is not None and rule != RULE_INIT_STEAL:
        owner[np.asarray(blocked) != 0] = -1
    seen = np.full(C.shape, INT_MAX, np.int64)          # steal: matched distance of every candidate as the query finds it
    choice, cdist = np.full(nq, -2, np.int64), np.full(nq, -2, np.int64)
    sweeps = 0
    for _ in range(limit if limit is not None else nq + 2):
        if rule == RULE_INIT_STEAL:
            avail = valid & ~(seen <= Dm)
        else:
            avail = valid & ~(owner[Cs] < me) if exclusive else valid & ~(owner[Cs] < 0)
        if rule == RULE_TRIANGULATION:
            ok = avail & (Dm <= max_dist)
            best = np.where(ok, Dm, BIG).min(1)
            within = ok & (Dm <= 2 * best[:, None]) & P
            key = np.where(within, Dm * 65536 + Cs, BIG)
            k = key.min(1)
            new = np.where(k < BIG, k % 65536, -1)
            newd = np.where(k < BIG, k // 65536, -1)
        else:
            none = 256 if rule == RULE_BEST_RATIO_SAME_LEVEL else INT_MAX
            best, best2 = np.full(nq, none, np.int64), np.full(nq, none, np.int64)
            lev, lev2, bt = np.full(nq, -1, np.int64), np.full(nq, -1, np.int64), np.full(nq, -1, np.int64)
            for c in range(C.shape[1]):                 # the ordered walk of a list, all queries at once
                d, a = Dm[:, c], avail[:, c]
                first = a & (d < best)
                second = a & ~first & (d < best2)
                best2 = np.where(first, best, np.where(second, d, best2))
                lev2 = np.where(first, lev, np.where(second, L[:, c], lev2))
                best = np.where(first, d, best)
                lev = np.where(first, L[:, c], lev)
                bt = np.where(first, Cs[:, c], bt)
            b32, s32 = best.astype(f32), best2.astype(f32)
            if rule == RULE_BEST_RATIO_SAME_LEVEL:
                ok = (best <= max_dist) & ~((lev == lev2) & (b32 > ratio * s32))
            elif rule == RULE_BEST_ONLY:
                ok = best <= max_dist
            elif rule == RULE_BEST_RATIO_LE:
                ok = (best <= max_dist) & (b32 < ratio * s32)
            elif rule == RULE_BEST_RATIO_LT:
                ok = (best < max_dist) & (b32 < ratio * s32)
            elif rule == RULE_BEST_RATIO_LEQ:
                ok = (b32 <= s32 * ratio) & (best <= max_dist)
            else:                                       # INIT_STEAL :652-654
                ok = (best <= max_dist) & (b32 < s32 * ratio)
            ok &= bt >= 0
            new, newd = np.where(ok, bt, -1), np.where(ok, best, -1)
        if (new == choice).all() and (newd == cdist).all():
            return sweeps
        sweeps += 1
        choice, cdist = new, newd
        acc = np.nonzero(choice >= 0)[0]                # ascending query index
        if rule == RULE_INIT_STEAL:
            # seen[i, c] = min{ dist(j) : j < i accepted C[i, c] }: accepts sorted by (target, query), running minimum inside a target
            seen = np.full(C.shape, INT_MAX, np.int64)
            if len(acc):
                key = choice[acc] * (nq + 1) + acc
                order = np.argsort(key, kind="stable")
                key, tgt, dd = key[order], choice[acc][order], cdist[acc][order]
                seg = np.cumsum(np.r_[0, tgt[1:] != tgt[:-1]])
                run = np.minimum.accumulate(dd - seg * 1024) + seg * 1024      # a later target's values lie below every earlier one's
                pos = np.searchsorted(key, Cs * (nq + 1) + me, side="left") - 1
                hit = valid & (pos >= 0)
                hit &= tgt[np.maximum(pos, 0)] == Cs
                seen = np.where(hit, run[np.maximum(pos, 0)], INT_MAX)
        elif exclusive:
            owner = np.where(owner < 0, -1, BIG)
            np.minimum.at(owner, choice[acc], acc)
    raise AssertionError("the parallel iteration did not settle")


# ---- scenes -----------------------------------------------------------------------------------------------------------------------

class Scene:
    def __init__(self, qdesc, tdesc, cand_lists, tlevel=None, blocked=None, expected=None, name=""):
        self.qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        self.tdesc = np.ascontiguousarray(tdesc, np.uint8).reshape(-1, 32)
        self.cand_lists = [np.asarray(c, np.int32) for c in cand_lists]
        self.nq, self.nt = len(self.cand_lists), len(self.tdesc)
        assert len(self.qdesc) == self.nq
        self.tlevel = np.zeros(self.nt, np.int32) if tlevel is None else np.ascontiguousarray(tlevel, np.int32)
        self.blocked = blocked
        self.expected = expected                 # closed form: (match, dist) or None
        self.name = name
        self.D = Hamming(self.qdesc, self.tdesc)

    def csr(self):
        start = np.zeros(self.nq + 1, np.int32)
        start[1:] = np.cumsum([len(c) for c in self.cand_lists])
        idx = np.concatenate(self.cand_lists).astype(np.int32) if start[-1] else np.zeros(0, np.int32)
        return start, idx


def _bits(positions):
    b = np.zeros(256, np.uint8)
    b[list(positions)] = 1
    return np.packbits(b)


def _domino_descriptors(n):
    """Targets alternate between all zeros (even) and bits 0..24 set (odd).  Query j is its left target t(j-1) with five of the first
    25 bits toggled -- which five depends on j -- so it is 5 from the left target's kind and 20 from t(j)'s."""
    even, odd = _bits([]), _bits(range(25))
    tdesc = np.stack([odd if j & 1 else even for j in range(n)])
    q = []
    for j in range(n):
        flip = [(j * 3 + k * 5) % 25 for k in range(5)]       # 5 is coprime to 25: five distinct positions
        left_is_odd = (j - 1) & 1
        q.append(_bits(set(range(25)) - set(flip)) if left_is_odd else _bits(flip))
    return np.stack(q), tdesc


def domino(n):
    qdesc, tdesc = _domino_descriptors(n)
    lists = [[0]] + [[j - 1, j] for j in range(1, n)]
    exp = (np.arange(n, dtype=np.int32), np.full(n, 20, np.int32))
    return Scene(qdesc, tdesc, lists, expected=exp, name="domino(%d)" % n)


def steal_domino(n):
    """Both distances 20: all targets are the zero descriptor, every query has 20 of the first 25 bits set."""
    tdesc = np.zeros((n, 32), np.uint8)
    qdesc = np.stack([_bits(set(range(25)) - {(j * 3 + k * 5) % 25 for k in range(5)}) for j in range(n)])
    lists = [[0]] + [[j - 1, j] for j in range(1, n)]
    exp = (np.arange(n, dtype=np.int32), np.full(n, 20, np.int32))
    return Scene(qdesc, tdesc, lists, expected=exp, name="steal_domino(%d)" % n)


def pile_descriptors(nq, k):
    """Every query the zero descriptor; target j has its first j bits set: distance j from every query."""
    assert k <= 257
    return np.zeros((nq, 32), np.uint8), np.stack([_bits(range(j)) for j in range(k)])


def pile(nq, k, max_dist):
    """Closed form for a rule that takes the best free target whatever the runner-up is."""
    qdesc, tdesc = pile_descriptors(nq, k)
    lists = [list(range(k))] * nq
    m = np.array([i if i <= max_dist and i < k else -1 for i in range(nq)], np.int32)
    return Scene(qdesc, tdesc, lists, tlevel=np.arange(k) & 1, expected=(m, m.copy()), name="pile(%d,%d)" % (nq, k))


RUN = 16


def contention(nq, nt, seed, hot=None):
    """Random lists of 1..12 candidates over `hot` of the nt targets (default about nq / 3, spread over the whole index range with
    both ends in), about a tenth of the lists empty (the first and the last always, from three queries on), a twentieth of the hot targets
    blocked, descriptors noisy copies of 8 prototypes; planted: identical and complementary pairs, pairs at 50 and 100, and queues of
    RUN queries (see below) that make the scene at least RUN sweeps deep under every rule."""
    rng = np.random.default_rng(seed)
    hot = min(nt, max(1, nq // 3)) if hot is None else min(hot, nt)
    if hot >= nt or nt <= 2:
        hot_t = np.arange(nt, dtype=np.int64)
    else:
        hot_t = np.sort(np.r_[0, nt - 1, 1 + rng.choice(nt - 2, max(hot - 2, 0), replace=False)]).astype(np.int64)
    base = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
    protos = []
    for k in range(8):                      # prototype k: the base with the first 16 bits of its 32-bit block k toggled: 32 apart
        b = base.copy()
        b[32 * k:32 * k + 16] ^= 1
        protos.append(b)

    def noisy(n, plain):
        """Row r of n: the prototype of its stretch of the index range (one in six: any prototype), as it is with probability `plain`,
        else with 5 or 25 bits of the second half of a block toggled: distances take few values (0, 5, 10, 25, 30, 32, 37, 50, 57, ...).
        Queries are mostly plain and targets mostly noisy, so neighbouring queries rank their shared targets alike and queue for them."""
        out = np.zeros((n, 32), np.uint8)
        for r in range(n):
            b = protos[int(rng.integers(0, 8)) if rng.random() < 1 / 6 else (r * 16 // n) % 8].copy()
            kind = 0 if rng.random() < plain else int(rng.integers(2, 4))
            if kind >= 2:
                lo = 32 * int(rng.integers(0, 8)) + 16
                if kind == 2:
                    b[lo:lo + 5] ^= 1
                else:
                    b[lo:lo + 16] ^= 1
                    lo2 = 32 * int(rng.integers(0, 8)) + 16
                    b[lo2 + 7:lo2 + 16] ^= 1           # 16 + 9 = 25 when the blocks differ, 7 when they are the same
            out[r] = np.packbits(b)
        return out
    # only the hot targets are ever candidates; the rest of tdesc keeps copies of queries so that a wrong index shows as distance 0
    qdesc = noisy(nq, 0.7)
    tdesc = qdesc[rng.integers(0, nq, nt)].copy() if nt > len(hot_t) else np.zeros((nt, 32), np.uint8)
    tdesc[hot_t] = noisy(len(hot_t), 0.15)
    lists = []
    for i in range(nq):
        empty = (nq >= 3 and i in (0, nq - 1)) or rng.random() < 0.1
        if empty and nq >= 3:
            lists.append([])
            continue
        # a window of neighbouring hot targets around the query's own position: chains form along the index
        centre = int(i * len(hot_t) / nq)
        k = int(rng.integers(1, 13))
        pick = np.clip(centre + rng.integers(-3, 4, k), 0, len(hot_t) - 1)
        lists.append([int(t) for t in hot_t[pick]])           # repeats allowed: a list may name a target twice
    # planted pairs: identical (d = 0) and complementary (d = 256)
    for i in range(0, nq, 37):
        if len(lists[i]):
            b = np.unpackbits(qdesc[i])
            b[:(0, 256, 50, 100)[(i // 37) & 3]] ^= 1          # identical, complementary, and 50 and 100 away (d == max_dist)
            tdesc[lists[i][0]] = np.packbits(b)
    blocked = np.zeros(nt, np.uint8)
    blocked[hot_t[rng.random(len(hot_t)) < 0.05]] = 1
    tlevel = rng.integers(0, 2, nt).astype(np.int32)
    # planted queues: RUN consecutive queries whose lists are [t(j-1), t(j)] over RUN consecutive hot targets, both at distance 20 (the
    # steal-domino): under every rule query j ends on t(j) only after query j-1 has settled, whatever the random queries around them do
    # to the same targets.  One queue every 256 queries, and one across query 1024, where a thread's second query begins.
    starts = [i0 for i0 in list(range(20, nq, 256)) + [1016] if i0 + RUN < nq - 1 and len(hot_t) >= RUN]
    for i0 in starts:
        p0 = min(int(i0 * len(hot_t) / nq), len(hot_t) - RUN)
        run_t = hot_t[p0:p0 + RUN]
        z = protos[(i0 // 256) % 8]
        tdesc[run_t] = np.packbits(z)
        blocked[run_t] = 0
        for j in range(RUN):
            b = z.copy()
            b[sorted(set(range(25)) - {(j * 3 + k * 5) % 25 for k in range(5)})] ^= 1
            qdesc[i0 + j] = np.packbits(b)
            lists[i0 + j] = [int(run_t[0])] if j == 0 else [int(run_t[j - 1]), int(run_t[j])]
    return Scene(qdesc, tdesc, lists, tlevel=tlevel, blocked=blocked, name="contention(%d,%d,%d)" % (nq, nt, seed))


def epipolar_pred(f12, q_x, q_y, t_x, t_y, sigma2, tlevel):
    """pred(i, t) of ORBmatcher::CheckDistEpipolarLine (:136-153) in float32, expression by expression; the last comparison is double
    (3.84 is a double literal)."""
    f12 = np.asarray(f12, f32).reshape(9)

    def pred(i, t):
        x1, y1, x2, y2 = f32(q_x[i]), f32(q_y[i]), f32(t_x[t]), f32(t_y[t])
        a = x1 * f12[0] + y1 * f12[3] + f12[6]
        b = x1 * f12[1] + y1 * f12[4] + f12[7]
        c = x1 * f12[2] + y1 * f12[5] + f12[8]
        num = a * x2 + b * y2 + c
        den = a * a + b * b
        if den == 0:
            return False
        dsqr = f32(num * num / den)
        return float(dsqr) < 3.84 * float(sigma2[tlevel[t]])
    return pred


SIDEWAYS_F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], f32)     # a translation along x: the epipolar line of (x1, y1) is y = y1


def epipolar_third(scene):
    """An uvo_epipolar whose predicate fails exactly for the targets with t % 3 == 2, and pred(i, t) from the float32 formula.  Queries
    lie on y = 0; targets with t % 3 == 2 on y = 100, the others on y = 3 * level: with sigma2 = (1, 4) a level-1 target is 9 from its
    line, inside 3.84 * 4 but outside 3.84 * 1 -- a predicate that read the wrong level's sigma fails it.
    -> dict(f12, q_x, q_y, t_x, t_y, sigma2), pred"""
    nq, nt = scene.nq, scene.nt
    q_x, q_y = (np.arange(nq) % 7).astype(f32), np.zeros(nq, f32)
    t = np.arange(nt)
    t_x = (t % 5).astype(f32)
    t_y = np.where(t % 3 == 2, 100, 3 * scene.tlevel).astype(f32)
    sigma2 = np.array([1.0, 4.0], f32)
    assert scene.tlevel.max(initial=0) <= 1
    pred = epipolar_pred(SIDEWAYS_F12, q_x, q_y, t_x, t_y, sigma2, scene.tlevel)
    return dict(f12=SIDEWAYS_F12, q_x=q_x, q_y=q_y, t_x=t_x, t_y=t_y, sigma2=sigma2), pred


# ---- the domino as geometry: key points in a row, windows that hold exactly two of them -------------------------------------------

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
ROW_STEP, ROW_X0, ROW_Y, ROW_RADIUS = 6.0, 10.0, 100.0, 4.0


def domino_row(n, steal=False):
    """The domino (or the steal-domino) laid out along x: target key point j at (10 + 6 j, 100) on level 0, query j centred midway
    between key points j - 1 and j, so that a window of radius 4 holds exactly those two (query 0: key point 0 alone).
    -> dict(kp, tdesc, qdesc, qx, qy, bounds = (min_x, min_y, max_x, max_y), scene)"""
    sc = steal_domino(n) if steal else domino(n)
    kp = np.zeros(n, KP)
    kp["x"], kp["y"], kp["size"] = ROW_X0 + ROW_STEP * np.arange(n), ROW_Y, 31.0
    qx = (kp["x"] - f32(ROW_STEP / 2)).astype(f32)
    qy = np.full(n, ROW_Y, f32)
    # the frame grid rounds to the nearest of its 64 columns and drops what rounds to column 64: keep the row clear of the last half column
    bounds = (0, 0, int((ROW_X0 + ROW_STEP * n) * 1.02) + 20, 480)
    return dict(kp=kp, tdesc=sc.tdesc, qdesc=sc.qdesc, qx=qx, qy=qy, bounds=bounds, scene=sc)


def bow_lists(groups1, groups2, skip1):
    """The visiting order of the vocabulary-guided loops (:178-249, :884-973): shared nodes ascending, the features of side 1 in node
    order unless skip1[feature], each with the node's features of side 2 as its list.  -> q_of (feature of every query), cand_lists"""
    q_of, lists = [], []
    for node in sorted(set(groups1) & set(groups2)):
        for f in groups1[node]:
            if not skip1[f]:
                q_of.append(int(f))
                lists.append([int(t) for t in groups2[node]])
    return np.asarray(q_of, np.int64), lists


# ---- what the GPU file runs, and how deep each scene must be (tests/test_resolve_model.py proves it on the CPU) --------------------

DOMINO_N = (64, 1025, 4096, 4097)          # one query per thread; two; the LDS tables' edge; the global tables
ROW_N = (64, 1025, 4097)
GROUP_NQ = (1, 2, 1023, 1024, 1025, 2049)  # one query per thread, the edge, two or more per thread
GROUP_NT = (1, 4096, 4097, 65535)          # the LDS tables, their edge, the global tables, the 16-bit index limit
CONTENTION_SEED = 11                       # every (nq, nt) of the grid with this seed; picked here, fixed
VARIANT_SCENES = ((1025, 4096, 12), (2049, 4097, 13))   # (nq, nt, seed) for the exclusive / blocked / max_dist / epipolar variants
MAX_DISTS = (0, 50, 100, 256)
CONTENTION_DEPTH = 12                      # at least this many sweeps wherever a scene is large enough to hold a planted queue
NN_RATIO = 0.9


def deep_enough(nq, nt):
    """Whether contention(nq, nt, .) can hold a planted queue at all: the launch-edge sizes nq = 1, 2 and nt = 1 cannot."""
    return nq >= 64 and min(nt, max(1, nq // 3)) >= RUN
