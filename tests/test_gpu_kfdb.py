"""The keyframe database on the device (uvo_kfdb_*, csrc/kfdb.hip) against the literal model (tests/kfdb_model.py) for exact equality on
the whole case table of tests/kfdb_cases.py: candidate lists and their order, the table of the listed keyframes, every float as its
bits, all six stored fields of every slot after every query.  Keyframe counts straddle the wavefront and workgroup edges
(1, 2, 63, 64, 65, 257, and 4100: past the list the epilogue orders in LDS), BoW lengths the 64-lane stride (1, 63, 64, 65, 200)."""
import numpy as np
import pytest

import kfdb_cases as kc

pytestmark = pytest.mark.gpu
NAMES = sorted(kc.cases())


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_model(uvo, name):
    case, want = kc.cases()[name], kc.expected(name)
    got = kc.run_api(case, lambda k, w, h: uvo.KeyFrameDatabase(k, w, h))
    assert got == want, kc.explain(got, want, case)


def test_two_databases_do_not_share_state(uvo):
    """Handles are independent: a case gives the model's answer beside a second live database, and on that one after a clear."""
    case, want = kc.cases()["stale_score"], kc.expected("stale_score")
    a, b = uvo.KeyFrameDatabase(*case[:3]), uvo.KeyFrameDatabase(*case[:3])
    got_a = kc.run_api(case, lambda *_: a)
    b.add(1, kc.Q3, None)
    got_b = kc.run_api(case[:3] + ([("clear",)] + case[3],), lambda *_: b)
    assert got_a == want and got_b[1:] == want


def test_a_database_filled_to_capacity_equals_one_with_room_to_spare(uvo):
    """KeyFrameDatabase(3, 4, 2) holding three keyframes of four words and two hash floats each: the last element of every per-slot array and
    of every mirror is written and read; the answers are the model's, and those of a database of (24, 32, 2)."""
    W = kc.W
    ops = [("add", 7, *kc.bow(W[0:4], [0.25] * 4), kc._h(1, 0)), ("add", 5, *kc.bow(W[1:5], [0.4, 0.3, 0.2, 0.1]), kc._h(0, 2)),
           ("add", 6, *kc.bow([W[0], W[2], W[3], W[6]], [0.125, 0.5, 0.25, 0.125]), kc._h(0.5, 0.5)),
           ("cov", 0, [2, 1]), ("cov", 1, [0]), ("cov", 2, [1, 0]),
           ("reloc", 1, *kc.bow(W[0:4], [0.25] * 4)), ("loop", 2, *kc.bow(W[1:5], [0.25] * 4), [0], kc.F32(0.05)),
           ("haloc", 99, kc._h(0, 0), [], kc.F32(4.0)), ("reloc", 3, *kc.bow(W[2:4], [0.5, 0.5]))]
    want = kc.run_model((3, 4, 2, ops))
    tight = kc.run_api((3, 4, 2, ops), lambda k, w, h: uvo.KeyFrameDatabase(k, w, h))
    roomy = kc.run_api((24, 32, 2, ops), lambda k, w, h: uvo.KeyFrameDatabase(k, w, h))
    assert tight == want, kc.explain(tight, want, (3, 4, 2, ops))
    assert roomy == want
    queries = [w for w in want if isinstance(w, dict)]
    assert 2 in [r[0] for r in queries[0]["rows"]] and queries[3]["cand"] == [2]             # the last slot is listed, and is a candidate


def _refused(uvo, code, fn, *args):
    with pytest.raises(uvo.UvoError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, uvo.last_error())


def test_refusals(uvo):
    """Bad input is refused, never truncated: over capacity, unsorted and duplicate ids, slots that hold no keyframe, more than 10 covisibles."""
    BAD, CAP = uvo.UVO_E_BADARG, uvo.UVO_E_CAPACITY
    for args in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (65537, 4, 4), (4, 4097, 4)):
        _refused(uvo, BAD, uvo.KeyFrameDatabase, *args)
    db = uvo.KeyFrameDatabase(3, 4, 2)
    ok = (np.array([5, 9, 11], np.uint32), np.array([0.5, 0.25, 0.25]))
    _refused(uvo, BAD, db.erase, 0)                                                        # nothing added yet
    _refused(uvo, BAD, db.add, 1, (np.array([5, 4, 11], np.uint32), ok[1]))                # unsorted
    _refused(uvo, BAD, db.add, 1, (np.array([5, 5, 11], np.uint32), ok[1]))                # duplicate
    _refused(uvo, CAP, db.add, 1, (np.arange(5, dtype=np.uint32), np.full(5, 0.2)))        # longer than max_words
    assert len(db) == 0
    assert [db.add(10 + k, ok, [1.0, 2.0]) for k in range(3)] == [0, 1, 2]
    _refused(uvo, CAP, db.add, 13, ok)                                                     # every slot taken
    _refused(uvo, BAD, db.detect_reloc, 1, (np.array([9, 5], np.uint32), np.array([0.5, 0.5])))
    _refused(uvo, BAD, db.detect_loop, 1, (np.array([5, 5], np.uint32), np.array([0.5, 0.5])), [], 0.0)
    _refused(uvo, CAP, db.detect_reloc, 1, (np.arange(5, dtype=np.uint32), np.full(5, 0.2)))
    _refused(uvo, BAD, db.detect_loop, 1, ok, [3], 0.0)                                    # connected slot out of range
    _refused(uvo, BAD, db.detect_loop, 1, ok, [], float("nan"))
    for slot in (-1, 3):
        _refused(uvo, BAD, db.erase, slot)
        _refused(uvo, BAD, db.set_covisibles, slot, [0])
    _refused(uvo, BAD, db.set_covisibles, 0, [1] * 11)
    _refused(uvo, BAD, db.set_covisibles, 0, [1, 3])                                       # a neighbour that holds no keyframe
    _refused(uvo, BAD, db.set_covisibles, 0, [-2])
    _refused(uvo, BAD, db.last_query)                                                      # no BoW query yet
    # the candidate capacity is checked, not truncated to
    import ctypes
    n, cand = ctypes.c_int(), np.zeros(1, np.int32)
    db.set_covisibles(0, [])
    rc = uvo.lib.uvo_kfdb_detect_reloc(db._h, 7, ok[0].ctypes.data, ok[1].ctypes.data, 3, cand.ctypes.data, 0, ctypes.byref(n))
    assert rc == CAP and n.value == 3
    # nothing above changed what the database holds: the refused calls left three keyframes, all listed by a query
    assert list(db.detect_reloc(8, ok)) == [0, 1, 2] and len(db.last_query()[0]) == 3
    db.erase(1)
    db.erase(1)                                                                            # twice: a no-op
    assert list(db.detect_reloc(9, ok)) == [0, 2]
    db.clear()
    _refused(uvo, BAD, db.erase, 0)                                                        # freed by clear
    _refused(uvo, BAD, db.set_covisibles, 0, [])
    assert len(db) == 0 and db.add(20, ok) == 0
    db.close()
