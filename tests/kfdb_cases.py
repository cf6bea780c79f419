"""The case table of the keyframe database and the three ways a case is run: through the literal model (kfdb_model.py), through an
object with the device API (u-vip-slam_amd.KeyFrameDatabase), and as a text script a stand-alone program reads (the host build of
kfdb_core.hpp, tests/emu/kfdb_emu.cpp, and the C++ adaptor's driver, tests/cpp/compat_kfdb.cpp).  Every run yields the same plain
structure, floats as their bits, so `==` is the comparison.

A case is (max_keyframes, max_words, hash_len, ops); an op is one of
  ("add", mnId, ids, values, hash | None)    ("erase", slot)    ("clear",)    ("cov", slot, [slot | -1, ...])
  ("reloc", query_id, ids, values)           ("loop", query_id, ids, values, [connected slot, ...], minScore)
  ("haloc", query_id, hash | None, [excluded mnId, ...], maxScore)
"""
import functools

import numpy as np

import kfdb_model as km

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- runners
def run_model(case):
    _, _, _, ops = case
    db = km.KeyFrameDatabase()
    out = []
    for op in ops:
        k = op[0]
        if k == "add":
            out.append(db.add(km.KeyFrame(op[1], op[2], op[3], op[4])))
        elif k == "erase":
            db.erase(db.kfVec[op[1]])
            out.append(None)
        elif k == "clear":
            db.clear()
            out.append(None)
        elif k == "cov":
            db.kfVec[op[1]].best_covisibles = [None if s < 0 else db.kfVec[s] for s in op[2]]
            out.append(None)
        elif k in ("reloc", "loop"):
            if k == "reloc":
                cand = db.DetectRelocalisationCandidates(op[1], (op[2], op[3]))
            else:
                cand = db.DetectLoopCandidates(op[1], (op[2], op[3]), [db.kfVec[s] for s in op[4]], op[5])
            maxc, minc, rows = db.table
            out.append({"cand": [kf.slot for kf in cand], "maxc": maxc, "minc": minc, "rows": rows, "state": db.state()})
        elif k == "haloc":
            cand = db.DetectLoopCandidatesHaloc(op[1], op[2], op[3], op[4])
            out.append({"cand": [kf.slot for kf in cand], "haloc": list(db.haloc), "state": db.state()})
        else:
            raise ValueError(k)
    return out


def _state_rows(st):
    return [(int(r["loop_query"]), int(r["reloc_query"]), int(r["loop_words"]), int(r["reloc_words"]), int(r["loop_score"].view(np.uint32)),
             int(r["reloc_score"].view(np.uint32))) for r in st]


def run_api(case, make_db):
    """make_db(max_keyframes, max_words, hash_len) -> an object with the methods of u-vip-slam_amd.KeyFrameDatabase"""
    mk, mw, hl, ops = case
    db = make_db(mk, mw, hl)
    out = []
    try:
        for op in ops:
            k = op[0]
            if k == "add":
                out.append(db.add(op[1], (op[2], op[3]), op[4]))
            elif k == "erase":
                out.append(db.erase(op[1]))
            elif k == "clear":
                out.append(db.clear())
            elif k == "cov":
                out.append(db.set_covisibles(op[1], op[2]))
            elif k in ("reloc", "loop"):
                cand = db.detect_reloc(op[1], (op[2], op[3])) if k == "reloc" else db.detect_loop(op[1], (op[2], op[3]), op[4], op[5])
                rows, maxc, minc = db.last_query()
                out.append({"cand": [int(c) for c in cand], "maxc": maxc, "minc": minc,
                            "rows": [(int(r["slot"]), int(r["words"]), int(r["flags"]), int(r["best"]), int(r["score"].view(np.uint32)),
                                      int(r["acc"].view(np.uint32))) for r in rows],
                            "state": _state_rows(db.state())})
            elif k == "haloc":
                cand = db.detect_loop_haloc(op[1], op[2], op[3], op[4])
                m, kept = db.last_haloc()
                out.append({"cand": [int(c) for c in cand], "haloc": [(int(a), int(b)) for a, b in zip(m.view(np.uint32), kept)], "state": _state_rows(db.state())})
            else:
                raise ValueError(k)
    finally:
        db.close()
    return out


def _f64bits(v):
    return [str(int(x)) for x in np.ascontiguousarray(v, np.float64).view(np.uint64)]


def _f32bits(v):
    return [str(int(x)) for x in np.ascontiguousarray(v, np.float32).view(np.uint32)]


def to_script(case):
    """The case as whitespace-separated tokens; doubles and floats as the decimal of their bits."""
    mk, mw, hl, ops = case
    t = ["create", str(mk), str(mw), str(hl)]
    for op in ops:
        k = op[0]
        if k == "add":
            t += ["add", str(int(op[1])), str(len(op[2])), "0" if op[4] is None else "1"] + [str(int(i)) for i in op[2]] + _f64bits(op[3])
            if op[4] is not None:
                t += _f32bits(op[4])
        elif k == "erase":
            t += ["erase", str(op[1])]
        elif k == "clear":
            t += ["clear"]
        elif k == "cov":
            t += ["cov", str(op[1]), str(len(op[2]))] + [str(int(s)) for s in op[2]]
        elif k == "reloc":
            t += ["reloc", str(int(op[1])), str(len(op[2]))] + [str(int(i)) for i in op[2]] + _f64bits(op[3])
        elif k == "loop":
            t += ["loop", str(int(op[1])), str(len(op[2]))] + [str(int(i)) for i in op[2]] + _f64bits(op[3]) + [str(len(op[4]))] + [str(int(s)) for s in op[4]]
            t += _f32bits([op[5]])
        elif k == "haloc":
            t += ["haloc", str(int(op[1])), "0" if op[2] is None else "1"] + ([] if op[2] is None else _f32bits(op[2]))
            t += [str(len(op[3]))] + [str(int(x)) for x in op[3]] + _f32bits([op[4]])
        t.append("\n")
    t.append("end\n")
    return " ".join(t)


def parse_output(text):
    """What a script-driven program printed -> the runners' structure.  Lines: `slot K` | `ok` | `cand n s..` | `table maxc minc n` then n
    `row slot words flags best score acc` | `haloc n` then n `h m kept` | `state n` then n `st lq rq lw rw ls rs`."""
    out, cur = [], None
    lines = [ln.split() for ln in text.strip().split("\n") if ln.strip()]
    i = 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        if ln[0] == "slot":
            out.append(int(ln[1]))
        elif ln[0] == "ok":
            out.append(None)
        elif ln[0] == "cand":
            cur = {"cand": [int(x) for x in ln[2:2 + int(ln[1])]]}
            out.append(cur)
        elif ln[0] == "table":
            cur["maxc"], cur["minc"] = int(ln[1]), int(ln[2])
            n = int(ln[3])
            cur["rows"] = [tuple(int(x) for x in r[1:]) for r in lines[i:i + n]]
            i += n
        elif ln[0] == "haloc":
            n = int(ln[1])
            cur["haloc"] = [tuple(int(x) for x in r[1:]) for r in lines[i:i + n]]
            i += n
        elif ln[0] == "state":
            n = int(ln[1])
            cur["state"] = [tuple(int(x) for x in r[1:]) for r in lines[i:i + n]]
            i += n
        else:
            raise ValueError("unexpected line %r" % (ln,))
    return out


def explain(got, want, case):
    """the first op whose answer differs, for the assertion message"""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            keys = [k for k in w if g.get(k) != w[k]] if isinstance(w, dict) and isinstance(g, dict) else []
            return "op %d (%s): %s differ: %s != %s" % (i, case[3][i][0], keys, str({k: g.get(k) for k in keys} or g)[:600], str({k: w[k] for k in keys} or w)[:600])
    return "%d answers, %d expected" % (len(got), len(want))


# ------------------------------------------------------------------------------------------------------------------ cases
def bow(ids, vals):
    order = np.argsort(np.asarray(ids))
    return np.asarray(ids, np.uint32)[order], np.asarray(vals, np.float64)[order]


def rand_bow(rng, n, pool):
    """n distinct words of the pool, ascending, L1-normalised values"""
    ids = np.sort(rng.choice(pool, size=n, replace=False)).astype(np.uint32)
    v = rng.random(n) + 0.05
    return ids, (v / v.sum()).astype(np.float64)


def _covis(rng, n, erased=()):
    k = int(rng.integers(0, 11))
    row = [int(x) for x in rng.integers(0, n, size=k)]
    if k and rng.random() < 0.3:
        row[int(rng.integers(0, k))] = -1
    return row


def sized_case(nkf, length, seed):
    """nkf keyframes of `length` words from a pool in 0..10^6 that makes sharing common; shuffled mnIds; two reloc queries (the second
    reuses state: half the keyframes share few words now), two loop queries with the same id (the second continues the counts), one haloc."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(10 ** 6, size=max(2 * length, 8), replace=False)
    hl = 7
    ids = rng.permutation(nkf) + 1
    ops = []
    for k in range(nkf):
        ln = length if k % 5 else max(1, length // 2)
        ops.append(("add", int(ids[k]), *rand_bow(rng, ln, pool), rng.standard_normal(hl).astype(np.float32) if k % 7 != 3 else None))
    for k in range(nkf):
        ops.append(("cov", k, _covis(rng, nkf)))
    if nkf > 4:
        ops.append(("erase", int(rng.integers(0, nkf))))
    q = rand_bow(rng, length, pool)
    ops.append(("reloc", 1000, *q))
    sub = rand_bow(rng, max(1, length // 3), q[0])
    ops.append(("reloc", 1001, *sub))
    ops.append(("reloc", 1001, *q))                                  # same id again: nobody listed twice, counts go on
    conn = [int(x) for x in rng.choice(nkf, size=min(nkf, 3), replace=False)]
    ops.append(("loop", 2000, *q, conn, F32(0.01)))
    ops.append(("loop", 2000, *sub, [], F32(0.0)))
    ops.append(("loop", 2001, *rand_bow(rng, length, pool), conn[:1], F32(0.05)))
    ops.append(("haloc", int(ids[0]), rng.standard_normal(hl).astype(np.float32), [int(x) for x in ids[1:3]], F32(8.0)))
    return (nkf, max(length, 1), hl, ops)


W = [1000 * (k + 1) + 7 * k for k in range(16)]        # hand-picked words, ascending
Q3 = bow([W[0], W[1], W[2]], [0.5, 0.25, 0.25])


def hand_two_keyframes():
    """Two keyframes, three words: A = the query itself (score 1), B shares w0, w1 with other values.
    B: |0.5-0.25| - 0.5 - 0.25 = -0.5 ; |0.25-0.25| - 0.25 - 0.25 = -0.5 ; sum -1 -> score 0.5.  maxCommonWords 3, minCommonWords 2:
    B (2 words) is listed, not scored."""
    ops = [("add", 10, *Q3, None), ("add", 11, *bow([W[0], W[1], W[5]], [0.25, 0.25, 0.5]), None), ("reloc", 1, *Q3)]
    return (4, 8, 2, ops)


def hand_scores():
    """Exact scores against Q3: A 1.0 (identical), B 0.75, C 0.875, all sharing three words.
    B = {w0: .5, w1: .125, w2: .125, w5: .25}: -1, -.25, -.25 -> 0.75;  C = {w0: .5, w1: .25, w2: .125, w5: .125}: -1, -.5, -.25 -> 0.875."""
    A = ("add", 20, *Q3, None)
    B = ("add", 21, *bow([W[0], W[1], W[2], W[5]], [0.5, 0.125, 0.125, 0.25]), None)
    C = ("add", 22, *bow([W[0], W[1], W[2], W[5]], [0.5, 0.25, 0.125, 0.125]), None)
    return A, B, C


def retention_boundary():
    """acc(B) = 0.75 = 0.75f * bestAcc(1.0): `>` does not retain it; C (0.875) stays.  Then the loop query with minScore = 0.75 = si(B):
    `>=` lets B into the accumulation; and minScore 0.875 as the start of bestAccScore."""
    A, B, C = hand_scores()
    ops = [B, A, C, ("reloc", 5, *Q3), ("loop", 6, *Q3, [], F32(0.75)), ("loop", 7, *Q3, [], F32(0.875)), ("loop", 8, *Q3, [], F32(1.5))]
    return (4, 8, 2, ops)


def stale_score():
    """Query 5: N scores 1.0.  Query 6 is two words of N's five-word neighbour A plus three words only A holds: N is listed (1 word,
    not scored), A scored; A's covisible N has mnRelocQuery == 6 and the mRelocScore query 5 left: it is added and elects N."""
    N = ("add", 30, *Q3, None)
    a_bow = bow([W[2], W[6], W[7], W[8], W[9]], [0.2, 0.2, 0.2, 0.2, 0.2])
    A = ("add", 31, *a_bow, None)
    Z = ("add", 32, *bow([W[12]], [1.0]), None)                      # shares nothing, ever
    q6 = bow(a_bow[0], [0.4, 0.15, 0.15, 0.15, 0.15])              # A scores below 1.0, so N's stale 1.0 is the strictly greater one
    ops = [N, A, Z, ("cov", 1, [0, 2]), ("reloc", 5, *Q3), ("reloc", 6, *q6),
           # the same through the loop query: its neighbour test also asks words > minCommonWords, which N (1 word) fails
           ("loop", 5, *Q3, [], F32(0.1)), ("loop", 6, *q6, [], F32(0.1)),
           # and with a query in which N keeps enough words: {w0, w1, w2, w6}: N 3, A 2 of max 3 -> min 2: A not scored, N scored, stale A
           ("cov", 0, [1]), ("loop", 7, *bow([W[0], W[1], W[2], W[6]], [0.25, 0.25, 0.25, 0.25]), [], F32(0.1))]
    return (4, 8, 2, ops)


def never_scored_neighbour():
    """A fresh database: N is listed with 1 of 5 words and never scored; the scored A adds N's 0.0f."""
    a_bow = bow([W[2], W[6], W[7], W[8], W[9]], [0.2, 0.2, 0.2, 0.2, 0.2])
    ops = [("add", 30, *Q3, None), ("add", 31, *a_bow, None), ("cov", 1, [0]), ("reloc", 6, *a_bow)]
    return (4, 8, 2, ops)


def query_id_zero():
    """mnRelocQuery / mnLoopQuery start at 0: a query with id 0 lists nobody, the counts go on from 0; the next id lists everybody."""
    A, B, C = hand_scores()
    ops = [A, B, ("reloc", 0, *Q3), ("loop", 0, *Q3, [], F32(0.0)), C, ("cov", 2, [0, 1]), ("reloc", 0, *Q3), ("reloc", 1, *Q3), ("loop", 1, *Q3, [1], F32(0.0))]
    return (4, 8, 2, ops)


def dedup_same_best():
    """A, B, C each name D (score 1.0) as a covisible: three list entries elect D, D itself a fourth; one candidate, at the first's place."""
    A, B, C = hand_scores()
    D = ("add", 23, *Q3, None)
    E = ("add", 24, *bow([W[0], W[1], W[2], W[9]], [0.25, 0.25, 0.25, 0.25]), None)
    ops = [B, C, E, D, A, ("cov", 0, [3]), ("cov", 1, [3, 0]), ("cov", 2, [1, 3]), ("cov", 4, [3]), ("reloc", 9, *Q3), ("loop", 9, *Q3, [], F32(0.2))]
    return (8, 8, 2, ops)


def holes_in_neighbour_rows():
    """A neighbour row holding -1 and an erased slot: the erased keyframe keeps the fields an earlier query left and still contributes."""
    A, B, C = hand_scores()
    ops = [A, B, C, ("reloc", 4, *Q3), ("loop", 4, *Q3, [], F32(0.0)), ("erase", 0), ("cov", 1, [-1, 0, 2]), ("cov", 2, [0, -1]),
           ("reloc", 4, *Q3), ("reloc", 5, *Q3), ("loop", 4, *Q3, [], F32(0.0)), ("loop", 5, *Q3, [], F32(0.0))]
    return (4, 8, 2, ops)


def zero_and_one_word():
    """One keyframe shares nothing; then a query of which every keyframe holds exactly one word (maxCommonWords 1, minCommonWords 0)."""
    rng = np.random.default_rng(3)
    ops = []
    for k in range(6):
        ops.append(("add", 50 + k, *bow([W[k], W[10], W[11 + k % 2]], [0.5, 0.25, 0.25]), None))
    ops.append(("add", 60, *bow([W[14], W[15]], [0.5, 0.5]), None))
    for k in range(7):
        ops.append(("cov", k, _covis(rng, 7)))
    q = bow(W[:6], [1 / 6.0] * 6)
    ops += [("reloc", 3, *q), ("loop", 3, *q, [2], F32(0.0)), ("reloc", 4, *bow([W[10], W[3]], [0.5, 0.5]))]
    return (8, 8, 2, ops)


def add_erase_add():
    """The ordering key after erasure: the walk's order is add order with the erased keyframes gone; a keyframe added after an erase comes
    last; clear starts over with slot 0."""
    rng = np.random.default_rng(4)
    pool = rng.choice(10 ** 6, size=24, replace=False)
    ops = [("add", 70 + 3 * ((k * 5) % 7), *rand_bow(rng, 10, pool), None) for k in range(6)]
    q = rand_bow(rng, 12, pool)
    ops += [("cov", 1, [0, 2, 3]), ("cov", 4, [1, 5]), ("reloc", 1, *q), ("erase", 1), ("erase", 3), ("add", 5, *rand_bow(rng, 10, pool), None), ("cov", 6, [1, 0]),
            ("reloc", 2, *q), ("loop", 2, *q, [0], F32(0.01)), ("erase", 0), ("add", 6, *rand_bow(rng, 10, pool), None), ("reloc", 3, *q),
            ("clear",), ("add", 90, *rand_bow(rng, 10, pool), None), ("add", 80, *rand_bow(rng, 10, pool), None), ("cov", 0, [1]), ("reloc", 3, *q),
            ("loop", 3, *q, [], F32(0.0))]
    return (8, 16, 2, ops)


def connected_not_listed():
    """A connected keyframe is never listed, its mnLoopQuery stays, its mnLoopWords end at 1."""
    A, B, C = hand_scores()
    ops = [A, B, C, ("loop", 3, *Q3, [0], F32(0.0)), ("loop", 3, *Q3, [], F32(0.0)), ("loop", 4, *Q3, [1, 2], F32(0.0))]
    return (4, 8, 2, ops)


def _h(*x):
    return np.array(x, np.float32)


def haloc_cases():
    """hash_len 4, distances exact: 2 kept -> none; 3 kept with equal m -> add order; an erased keyframe still returned; empty hashes on
    either side (m = 1); a NaN hash (m = 1); m exactly at maxScore * 0.8 in double (5.0f * 0.8 == 4.0: not kept); an excluded id."""
    q = _h(0, 0, 0, 0)
    adds = [("add", 100, *Q3, _h(1, 0, 0, 0)),            # m 1
            ("add", 101, *Q3, _h(0, 2, 0, 0)),            # m 2
            ("add", 102, *Q3, _h(0, 0, 0, 4)),            # m 4
            ("add", 103, *Q3, _h(0.5, 0.5, 0.5, 0.5)),    # m 2: ties with 101
            ("add", 104, *Q3, None),                      # empty: m 1
            ("add", 105, *Q3, _h(np.nan, 0, 0, 0)),       # NaN: m 1
            ("add", 106, *Q3, _h(1, 1, 1, 0.99999)),      # just under 4
            ("add", 107, *Q3, _h(np.inf, 0, 0, 0))]       # inf: never kept
    ops = adds + [
        ("haloc", 999, q, [], F32(2.0)),                 # kept: m < 1.6: 100, 104, 105 -> three, ties at m = 1 in add order
        ("haloc", 999, q, [104], F32(2.0)),              # an excluded id: two kept -> none
        ("haloc", 100, q, [], F32(2.0)),                 # the query's own id: two kept -> none
        ("erase", 0), ("erase", 5),
        ("haloc", 999, q, [], F32(2.0)),                 # erased keyframes are still in kfVec
        ("haloc", 999, q, [], F32(5.0)),                 # m < 4.0: 102 (m = 4) is out, 106 in
        ("haloc", 999, q, [100, 104, 105], F32(5.0)),    # 101 and 103 tie at 2
        ("haloc", 999, None, [], F32(2.0)),              # empty query hash: every m = 1
        ("haloc", 999, None, [], F32(1.25)),             # 1 < 1.0: nothing
        ("haloc", 999, _h(np.nan, 0, 0, 0), [], F32(2.0)),
        ("haloc", 999, q, [], F32(np.inf)),
        ("clear",), ("add", 1, *Q3, _h(1, 0, 0, 0)), ("haloc", 999, q, [], F32(9.0))]
    return (8, 8, 4, ops)


def haloc_many(n, seed):
    rng = np.random.default_rng(seed)
    hl = 33
    ops = [("add", int(i) + 1, *Q3, (rng.integers(0, 4, size=hl) * 0.25).astype(np.float32) if k % 9 != 4 else None) for k, i in enumerate(rng.permutation(n))]
    q = (rng.integers(0, 4, size=hl) * 0.25).astype(np.float32)
    ops += [("haloc", 10 ** 6, q, [2, 5], F32(t)) for t in (4.0, 12.0, 14.0, 40.0)]
    return (n, 4, hl, ops)


def beyond_the_lds_sort(nkf=4100):
    """More slots than the epilogue orders in LDS (4096): short vectors over a dozen words, so the list is long and full of equal first words."""
    rng = np.random.default_rng(41)
    pool = rng.choice(10 ** 6, size=12, replace=False)
    ops = [("add", int(i) + 1, *rand_bow(rng, 3, pool), None) for i in rng.permutation(nkf)]
    for k in range(0, nkf, 3):
        ops.append(("cov", k, [int(x) for x in rng.integers(0, nkf, size=10)]))
    ops += [("erase", 5), ("erase", 4097), ("reloc", 1, *rand_bow(rng, 5, pool)), ("loop", 1, *rand_bow(rng, 6, pool), [0, 4099, 77], F32(0.05)),
            ("reloc", 1, *rand_bow(rng, 4, pool))]
    return (nkf, 8, 2, ops)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Keyframe counts straddle the wavefront and workgroup edges, BoW lengths the 64-lane stride."""
    c = {}
    for nkf in (1, 2, 63, 64, 65, 257):
        for length in (1, 63, 64, 65, 200):
            c["sized_%d_%d" % (nkf, length)] = sized_case(nkf, length, 1000 * nkf + length)
    c["hand_two_keyframes"] = hand_two_keyframes()
    c["retention_boundary"] = retention_boundary()
    c["stale_score"] = stale_score()
    c["never_scored_neighbour"] = never_scored_neighbour()
    c["query_id_zero"] = query_id_zero()
    c["dedup_same_best"] = dedup_same_best()
    c["holes_in_neighbour_rows"] = holes_in_neighbour_rows()
    c["zero_and_one_word"] = zero_and_one_word()
    c["add_erase_add"] = add_erase_add()
    c["connected_not_listed"] = connected_not_listed()
    c["haloc"] = haloc_cases()
    for n in (1, 2, 63, 64, 65, 257):
        c["haloc_many_%d" % n] = haloc_many(n, n)
    c["beyond_the_lds_sort"] = beyond_the_lds_sort()
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's answer, computed once per case and shared by the tests; callers must not change it"""
    return run_model(cases()[name])
