"""uvo_grider_fast (csrc/grider.hip: k_grid_score, k_grid_select) held to the numpy model of tests/grider_model.py at the cases of
tests/grider_cases.py -- tests/test_grider_model.py shows on the CPU what each case reaches and ties the model to the oracle.  Key points
are integers in float fields: every comparison is of bytes.

One single-level 320 x 256 handle serves the whole module, so every call finds in the handle's score plane what the calls before it
left there.  It has max_batch = 32: k_grid_select borrows the corner-count scratch of the FAST stage, which grows with the batch, and the
3 x 3 case has 441 ROIs (a max_batch = 1 handle refuses more than 127 with UVO_E_BADARG; tests/test_grider_model.py works both out on the host)."""
import ctypes

import numpy as np
import pytest

import grider_cases as gc
import grider_model as gm

pytestmark = pytest.mark.gpu

MAX_BATCH = gc.HANDLE_CFG[3]


@pytest.fixture(scope="module")
def ex(uvo):
    nfeatures, scale, nlevels, _ = gc.HANDLE_CFG
    e = uvo.ORBextractor(nfeatures, scale, nlevels, 0, 20, max_width=gc.HANDLE_W, max_height=gc.HANDLE_H, max_batch=MAX_BATCH)
    yield e
    e.close()


def _run(ex, k):
    return ex.grider_fast(k.image, k.num_features, k.grid_x, k.grid_y, k.threshold, k.nms)


def _check(ex, name):
    k = gc.fills()[name] if name in gc.fills() else gc.by_name(name)
    got, want = _run(ex, k), gc.expected(name)
    assert len(got) == len(want), (name, len(got), len(want))
    assert got.tobytes() == want.tobytes(), name


def _raw(uvo, ex, buf, w, h, stride, k, cap, num_features=None):
    """The C call on the w x h image at the start of buf; returns (status, n_out, the cap records)."""
    out, n = np.zeros(cap, uvo.KEYPOINT_DTYPE), ctypes.c_int(-7)
    rc = uvo.lib.uvo_grider_fast(ex._h, buf.ctypes.data, w, h, stride, k.num_features if num_features is None else num_features, k.grid_x, k.grid_y,
                                 k.threshold, 1 if k.nms else 0, out.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value, out


@pytest.mark.parametrize("name", [k.name for k in gc.cases()])
def test_case_equals_the_model(ex, name):
    k = gc.by_name(name)
    if k.fill:                       # the call that leaves non-zero scores where a ROI without interior must not look
        _check(ex, k.fill)
    _check(ex, name)


def test_row_stride_larger_than_the_width(uvo, ex):
    """Every image once more inside a noise-filled buffer whose rows are width + 13 bytes apart."""
    for k in gc.cases():
        h, w = k.image.shape
        buf = np.random.default_rng(5).integers(0, 256, (h, w + 13), dtype=np.uint8)
        buf[:, :w] = k.image
        want = gc.expected(k.name)
        rc, n, out = _raw(uvo, ex, buf, w, h, w + 13, k, len(want) + 8)
        assert (rc, n) == (uvo.UVO_OK, len(want)) and out[:n].tobytes() == want.tobytes(), k.name


def test_large_small_large_on_one_handle(ex):
    """The plane, the ROI lists and the counts are the previous call's wherever this call does not write them."""
    for name in ("full", "ties at the cut", "wider than max_width", "smallest interior", "full", "no interior 1 x 1", "partial blocks",
                 "more ROIs than grid cells", "wider than max_width"):
        _check(ex, name)


def test_output_capacity_one_below_the_count(uvo, ex):
    first = gc.cases()[0]
    for name in ("partial blocks", "more points than num_features + cells + 64"):
        k, want = gc.by_name(name), gc.expected(name)
        h, w = k.image.shape
        rc, n, out = _raw(uvo, ex, k.image, w, h, w, k, len(want) - 1)
        assert (rc, n) == (uvo.UVO_E_CAPACITY, len(want)), name       # refused when the results are handed out: n_out is the full count
        assert out.tobytes() == want[:-1].tobytes(), name
        _check(ex, first.name)
        rc, n, out = _raw(uvo, ex, k.image, w, h, w, k, len(want))
        assert (rc, n) == (uvo.UVO_OK, len(want)) and out.tobytes() == want.tobytes(), name


def test_num_features_at_the_handle_staging(uvo, ex):
    """Grid 1,1 keeps num_features + 1 per ROI: max_batch * uvo_extractor_max_keypoints() - 1 fills the handle's output staging exactly."""
    first = gc.cases()[0]
    limit = MAX_BATCH * ex.cap
    k = gc.by_name("corners in a partial block")
    h, w = k.image.shape
    assert (k.grid_x, k.grid_y) == (1, 1)
    want = gm.grider_fast(k.image, limit - 1, 1, 1, k.threshold, k.nms)
    assert len(want) > len(gc.expected(k.name))                        # every corner now, not the first 101
    rc, n, out = _raw(uvo, ex, k.image, w, h, w, k, limit, num_features=limit - 1)
    assert (rc, n) == (uvo.UVO_OK, len(want)) and out[:n].tobytes() == want.tobytes()
    rc, n, out = _raw(uvo, ex, k.image, w, h, w, k, limit + 1, num_features=limit)
    assert (rc, n) == (uvo.UVO_E_CAPACITY, 0) and not out.view(np.uint8).any()
    _check(ex, first.name)
    with pytest.raises(uvo.UvoError) as ei:                            # the same through the binding
        ex.grider_fast(k.image, limit, 1, 1, k.threshold, k.nms)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    _check(ex, first.name)
