"""uvo_extract_batch through the C ABI with more than one frame, in both host-buffer staging forms: the page-locked region the kernels
read and write (up to 16 frames) and the direct copies (more than 16).  Every frame is held to the oracle called frame by frame:
top-up mode with per-frame keypoints and grids, strided FullDetect input, and an output capacity smaller than a frame's result."""
import numpy as np
import pytest

from test_gpu_parity import _assert_same_features

pytestmark = pytest.mark.gpu
W, H = 320, 256
BATCHES = [3, 20]  # the pinned form, the direct-copy form


def _handles(uvo, oracle, batch, in_cap=0):
    ex = uvo.ORBextractor(500, 1.2, 6, 0, 20, max_width=W, max_height=H, max_batch=batch, max_input_keypoints=in_cap)
    return ex, oracle.extractor(500, 1.2, 6, 20)


def _extract_batch(uvo, ex, imgs, cap, kin=None, n_in=None, grids=None, min_px=0, need=None):
    """uvo_extract_batch on a (B, H, W) view (any row / frame stride); returns (rc, n_out, out_kp, out_desc)."""
    b, h, w = imgs.shape
    assert imgs.strides[2] == 1
    out_kp = np.zeros((b, cap), uvo.KEYPOINT_DTYPE)
    out_desc = np.zeros((b, cap, 32), np.uint8)
    n_out = np.zeros(b, np.int32)
    full = grids is None
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = uvo.lib.uvo_extract_batch(ex._h, b, imgs.ctypes.data, w, h, imgs.strides[1], imgs.strides[0], ptr(kin), ptr(n_in), ptr(grids),
                                   0 if full else grids.shape[2], 0 if full else grids.shape[1], int(min_px), 1 if full else 0, ptr(need),
                                   out_kp.ctypes.data, out_desc.ctypes.data, cap, n_out.ctypes.data)
    return rc, n_out, out_kp, out_desc


@pytest.mark.parametrize("batch", BATCHES)
def test_topup_batch_with_per_frame_keypoints_and_grids(uvo, oracle, synth, batch):
    in_cap, min_px = 300, 20
    rows, cols = H // min_px + 2, W // min_px + 2
    ex, oe = _handles(uvo, oracle, batch, in_cap)
    imgs = np.stack([synth.make_frame(4000 + i, W, H, n_shapes=120) for i in range(batch)])
    rng = np.random.default_rng(23 + batch)
    n_in = np.array([(0, 120, 300, 7, 45)[b % 5] for b in range(batch)], np.int32)
    need = np.array([(500, 380, 200, 30, 455)[b % 5] for b in range(batch)], np.int32)
    kin = np.zeros((batch, in_cap), uvo.KEYPOINT_DTYPE)
    grids = np.zeros((batch, cols, rows), np.int32)  # per frame: (rows, cols) column-major
    for b in range(batch):
        k = kin[b, :n_in[b]]
        k["x"] = rng.uniform(20, W - 21, n_in[b]).astype(np.float32)
        k["y"] = rng.uniform(20, H - 21, n_in[b]).astype(np.float32)
        k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = 31, -1, rng.uniform(0, 99, n_in[b]), 0, np.arange(n_in[b])
        for p in k:
            grids[b, int(p["x"] / min_px), int(p["y"] / min_px)] += 1
    g_gpu = grids.copy()
    rc, n_out, out_kp, out_desc = _extract_batch(uvo, ex, imgs, ex.cap, kin, n_in, g_gpu, min_px, need)
    assert rc == uvo.UVO_OK, rc
    for b in range(batch):
        g_orc = np.asfortranarray(grids[b].T)
        kp_o, de_o = oe(imgs[b], kin[b, :n_in[b]].copy(), g_orc, min_px, False, int(need[b]))
        _assert_same_features(out_kp[b, :n_out[b]], out_desc[b, :n_out[b]], kp_o, de_o, "batch %d frame %d n_in=%d need=%d" % (batch, b, n_in[b], need[b]))
        np.testing.assert_array_equal(g_gpu[b].T, g_orc, err_msg="grid of frame %d" % b)
    ex.close()


@pytest.mark.parametrize("batch", BATCHES)
def test_full_detect_batch_with_row_and_frame_gaps(uvo, oracle, synth, batch):
    ex, oe = _handles(uvo, oracle, batch)
    store = np.full((batch, H + 5, W + 24), 0xA5, np.uint8)  # stride > width, frame_stride > height * stride
    imgs = store[:, :H, :W]
    for b in range(batch):
        imgs[b] = synth.make_frame(5000 + b, W, H, n_shapes=120)
    assert imgs.strides[1] > W and imgs.strides[0] > H * imgs.strides[1]
    rc, n_out, out_kp, out_desc = _extract_batch(uvo, ex, imgs, ex.cap)
    assert rc == uvo.UVO_OK, rc
    for b in range(batch):
        kp_o, de_o = oe(np.ascontiguousarray(imgs[b]))
        assert len(kp_o) > 100
        _assert_same_features(out_kp[b, :n_out[b]], out_desc[b, :n_out[b]], kp_o, de_o, "batch %d frame %d" % (batch, b))
    ex.close()


@pytest.mark.parametrize("batch", BATCHES)
def test_cap_smaller_than_a_frames_result(uvo, oracle, synth, batch):
    ex, oe = _handles(uvo, oracle, batch)
    imgs = np.stack([synth.make_frame(6000 + i, W, H, n_shapes=120) for i in range(batch)])
    ref = [oe(imgs[b]) for b in range(batch)]
    cap = min(len(kp) for kp, _ in ref) // 2
    assert cap > 50
    rc, n_out, out_kp, out_desc = _extract_batch(uvo, ex, imgs, cap)
    assert rc == uvo.UVO_E_CAPACITY, rc
    for b, (kp_o, de_o) in enumerate(ref):
        assert n_out[b] == len(kp_o), "frame %d: n_out %d, oracle %d" % (b, n_out[b], len(kp_o))
        _assert_same_features(out_kp[b], out_desc[b], kp_o[:cap], de_o[:cap], "batch %d frame %d, first %d records" % (batch, b, cap))
    ex.close()
