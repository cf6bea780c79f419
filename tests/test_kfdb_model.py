"""The literal model of KeyFrameDatabase (tests/kfdb_model.py) pinned on cases derivable by hand, without a GPU: what the device database
and its host build are compared with has to be right by itself first."""
import numpy as np

import kfdb_cases as kc
import kfdb_model as km

F32 = np.float32
ONE, HALF = km.bits32(1.0), km.bits32(0.5)
ALL = km.LISTED | km.SCORED | km.ENTERED | km.RETAINED


def test_two_keyframes_three_words_by_hand():
    """A is the query itself: three terms -1, -.5, -.5 -> 1.0.  B shares w0, w1: -.5, -.5 -> 0.5, but with 2 of max 3 words
    (minCommonWords = (int)(3 * 0.8f) = 2) it is listed and not scored: its score field keeps the 0.0f of its add."""
    case = kc.hand_two_keyframes()
    assert float(km.l1_score(list(zip(*kc.Q3)), list(zip(*case[3][1][2:4])))) == 0.5
    res = kc.run_model(case)[-1]
    assert res["cand"] == [0] and (res["maxc"], res["minc"]) == (3, 2)
    assert res["rows"] == [(0, 3, ALL, 0, ONE, ONE), (1, 2, km.LISTED, -1, 0, 0)]
    assert res["state"] == [(0, 1, 0, 3, 0, ONE), (0, 1, 0, 2, 0, 0)]


def test_score_of_nothing_in_common_is_minus_zero():
    assert km.bits32(F32(km.l1_score([(1, 0.5)], [(2, 0.5)]))) == 0x80000000        # -0.0 / 2.0


def test_truncation_of_the_float_product():
    """(int)(5 * 0.8f) == 4 although 5 * 0.8 is 4.000000000000001 in double and 0.8f is above 0.8: a keyframe with 4 of 5 words is not scored."""
    assert int(F32(5) * F32(0.8)) == 4 and int(F32(10) * F32(0.8)) == 8 and int(F32(1) * F32(0.8)) == 0
    five = kc.bow(kc.W[:5], [0.2] * 5)
    ops = [("add", 1, *five, None), ("add", 2, *kc.bow(kc.W[1:6], [0.2] * 5), None), ("reloc", 9, *five)]
    res = kc.run_model((4, 8, 2, ops))[-1]
    assert (res["maxc"], res["minc"]) == (5, 4)
    assert [(r[0], r[1], r[2]) for r in res["rows"]] == [(0, 5, ALL), (1, 4, km.LISTED)]


def test_haloc_returns_none_below_three_kept():
    res = kc.run_model(kc.haloc_cases())
    first, excluded, own = res[8], res[9], res[10]
    assert first["cand"] == [0, 4, 5]                                      # m = 1 three times: add order
    assert [k for _, k in first["haloc"]] == [1, 0, 0, 0, 1, 1, 0, 0]
    assert first["haloc"][4] == (ONE, 1) and first["haloc"][5] == (ONE, 1)  # the empty and the NaN hash: EXIT_FAILURE as a float
    assert sum(k for _, k in excluded["haloc"]) == 2 and excluded["cand"] == []
    assert sum(k for _, k in own["haloc"]) == 2 and own["cand"] == []
    assert res[13]["cand"] == [0, 4, 5]                                    # erased keyframes are still compared
    at_bound = res[14]                                                     # maxScore 5: 5.0 * 0.8 == 4.0 in double; m = 4 is not below it
    assert float(np.float64(F32(5.0)) * np.float64(0.8)) == 4.0
    assert at_bound["haloc"][2] == (km.bits32(4.0), 0) and at_bound["haloc"][6][1] == 1
    assert res[15]["cand"] == [1, 3, 6]                                    # 101 and 103 tie at 2: add order


def test_stale_score_is_carried_into_the_next_query():
    """Query 5 scores N 1.0.  In query 6 N is listed with one word of five, not scored, and A's neighbour: its 1.0 is added to A's score
    and, strictly greater, makes N the candidate."""
    res = kc.run_model(kc.stale_score())
    q5, q6 = res[4], res[5]
    assert q5["cand"] == [0] and q5["state"][0][5] == ONE
    (n_slot, n_words, n_flags, n_best, n_score, _), (a_slot, a_words, a_flags, a_best, a_score, a_acc) = q6["rows"]     # w2's list is [N, A]
    assert (n_slot, n_words, n_flags, n_best, n_score) == (0, 1, km.LISTED, -1, ONE)
    si = np.array(a_score, np.uint32).view(np.float32)
    assert (a_slot, a_words, a_flags, a_best) == (1, 5, ALL, 0) and si < 1.0
    assert a_acc == km.bits32(F32(si + F32(1.0)))
    assert q6["cand"] == [0]
    # the loop query's neighbour test also wants words > minCommonWords: there N (1 word) does not contribute
    assert res[7]["cand"] == [1] and res[7]["rows"][1][3] == 1 and res[7]["rows"][1][5] == res[7]["rows"][1][4]


def test_never_scored_neighbour_adds_zero():
    res = kc.run_model(kc.never_scored_neighbour())[-1]
    a = [r for r in res["rows"] if r[0] == 1][0]
    assert a[2] == ALL and a[3] == 1 and a[5] == a[4] and res["cand"] == [1]


def test_connected_keyframe_is_not_listed():
    res = kc.run_model(kc.connected_not_listed())
    first, again, other = res[3], res[4], res[5]
    assert [r[0] for r in first["rows"]] == [1, 2] and first["state"][0][:3] == (0, 0, 1)      # query untouched, words end at 1
    assert [r[0] for r in again["rows"]] == [0] and again["state"][0][:3] == (3, 0, 3)         # no longer connected: listed now
    assert again["state"][1][2] == 6                                                              # same id: 3 + 3, not listed
    assert [r[0] for r in other["rows"]] == [0] and other["state"][1][:3] == (3, 0, 1)


def test_query_id_zero_lists_nobody_fresh():
    res = kc.run_model(kc.query_id_zero())
    assert res[2]["rows"] == [] and res[2]["cand"] == [] and [s[3] for s in res[2]["state"]] == [3, 3]
    assert res[3]["rows"] == [] and [s[2] for s in res[3]["state"]] == [3, 3]
    assert res[6]["rows"] == [] and [s[3] for s in res[6]["state"]] == [6, 6, 3]
    assert [r[0] for r in res[7]["rows"]] == [0, 1, 2]


def test_retention_boundary_and_min_score_equality():
    res = kc.run_model(kc.retention_boundary())
    reloc, loop_eq, loop_start, loop_none = res[3], res[4], res[5], res[6]
    by_slot = {r[0]: r for r in reloc["rows"]}
    assert by_slot[0][5] == km.bits32(0.75) and not by_slot[0][2] & km.RETAINED           # acc == 0.75f * 1.0: `>` fails
    assert reloc["cand"] == [1, 2]
    assert {r[0]: bool(r[2] & km.ENTERED) for r in loop_eq["rows"]} == {0: True, 1: True, 2: True}   # si == minScore enters
    assert loop_eq["cand"] == [1, 2]
    assert {r[0]: bool(r[2] & km.ENTERED) for r in loop_start["rows"]} == {0: False, 1: True, 2: True}
    assert loop_none["cand"] == [] and all(r[2] == km.LISTED | km.SCORED for r in loop_none["rows"])


def test_dedup_keeps_the_first_election():
    res = kc.run_model(kc.dedup_same_best())
    assert [r[3] for r in res[9]["rows"] if r[2] & km.RETAINED].count(3) >= 2
    assert res[9]["cand"].count(3) == 1 and res[9]["cand"][0] == 3


def test_script_round_trip():
    """to_script / parse_output carry a case and an answer without loss (the stand-alone programs speak this form)."""
    case = kc.cases()["add_erase_add"]
    want = kc.expected("add_erase_add")
    lines = []
    for r in want:
        if r is None:
            lines.append("ok")
        elif isinstance(r, int):
            lines.append("slot %d" % r)
        else:
            lines.append("cand %d %s" % (len(r["cand"]), " ".join(map(str, r["cand"]))))
            lines.append("table %d %d %d" % (r["maxc"], r["minc"], len(r["rows"])))
            lines += ["row " + " ".join(map(str, row)) for row in r["rows"]]
            lines.append("state %d" % len(r["state"]))
            lines += ["st " + " ".join(map(str, st)) for st in r["state"]]
    assert kc.parse_output("\n".join(lines)) == want
    assert kc.to_script(case).split()[0:4] == ["create", "8", "16", "2"]
