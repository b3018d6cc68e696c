"""FaceEmbeddings, the host-only part (no GPU): mi_face_chip_rect against a restatement of crop_image_to_bbox (face_embeddings.rs:101-109 on
bbox().scale(size), types.rs:162-165,219-225), mi_l2_norm / mi_similarity_score against sequential-float32 restatements of utils.rs:30-50,
the argument refusals of the new entries, and the synthetic embedding graphs of the GPU tests through the planner and the oracle.
(The refusal of cap < D needs a handle, and a handle needs a device: it is checked in tests/test_embeddings_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import embed_synth as es

W, H = 256, 128   # powers of two: the products below are exact


def det(xmin, ymin, xmax, ymax):
    d = np.zeros(17, np.float32)
    d[:4] = (xmin, ymin, xmax, ymax)
    return d


# name -> (detection, what the case must turn out to be: checked, not assumed)
RECT_CASES = {
    "minus_half_truncates_to_0": (det(-0.5 / W, 0.25, 0.5, 0.75), lambda d, r, ok: float(d[0]) * W == -0.5 and r[0] == 0 and ok),
    "minus_1.2_is_x_minus_1": (det(-1.2 / W, 0.25, 0.5, 0.75), lambda d, r, ok: abs(float(d[0]) * W + 1.2) < 1e-5 and r[0] == -1 and not ok),
    "x_plus_w_equals_W": (det(0.5, 0.25, 1.0, 0.75), lambda d, r, ok: r[0] + r[2] == W and ok),
    "x_plus_w_equals_W_plus_1": (det(0.5, 0.25, 257.0 / W, 0.75), lambda d, r, ok: r[0] + r[2] == W + 1 and not ok),
    "y_plus_h_equals_H": (det(0.25, 0.5, 0.5, 1.0), lambda d, r, ok: r[1] + r[3] == H and ok),
    "y_minus_1": (det(0.25, -1.5 / H, 0.5, 0.5), lambda d, r, ok: r[1] == -1 and not ok),
    "w_is_0": (det(0.5, 0.25, 0.5 + 0.5 / W, 0.75), lambda d, r, ok: r[2] == 0 and r[3] > 0 and not ok),
    "h_is_0": (det(0.25, 0.5, 0.75, 0.5), lambda d, r, ok: r[3] == 0 and r[2] > 0 and not ok),
    "negative_w": (det(0.5, 0.25, 0.25, 0.75), lambda d, r, ok: r[2] < 0 and not ok),
    "nan_xmin": (det(np.nan, 0.25, 0.5, 0.75), lambda d, r, ok: np.isnan(d[0]) and r[0] == 0 and r[2] == 0 and not ok),
    "nan_ymax": (det(0.25, 0.25, 0.5, np.nan), lambda d, r, ok: np.isnan(d[3]) and r[3] == 0 and not ok),
    "1e30_xmax_saturates": (det(0.25, 0.25, 1e30, 0.75), lambda d, r, ok: r[2] == es.I32_MAX and not ok),
    "1e30_xmin_saturates": (det(1e30, 0.25, 1e30, 0.75), lambda d, r, ok: r[0] == es.I32_MAX and not ok),
    "minus_1e30_saturates": (det(-1e30, 0.25, 0.5, 0.75), lambda d, r, ok: r[0] == es.I32_MIN and r[2] == es.I32_MAX and not ok),
    "plain": (det(0.3, 0.2, 0.61, 0.83), lambda d, r, ok: ok and r[2] > 1 and r[3] > 1),
    "whole_frame": (det(0.0, 0.0, 1.0, 1.0), lambda d, r, ok: r == (0, 0, W, H) and ok),
}


@pytest.mark.parametrize("name", sorted(RECT_CASES))
def test_face_chip_rect_matches_the_restatement(mi, name):
    d, is_hit = RECT_CASES[name]
    want, want_valid = es.chip_rect(d, W, H)
    assert is_hit(d, want, want_valid), (name, want, want_valid)   # the case is what its name says
    got, got_valid = mi.face_chip_rect(d, (W, H))
    assert got == want and got_valid == want_valid


def test_face_chip_rect_random_detections(mi):
    rs = np.random.RandomState(17)
    valid = 0
    for _ in range(300):
        d = det(*(rs.uniform(-0.2, 1.2, 4).astype(np.float32)))
        want, want_valid = es.chip_rect(d, 321, 243)
        got, got_valid = mi.face_chip_rect(d, (321, 243))
        assert got == want and got_valid == want_valid
        valid += got_valid
    assert 10 < valid < 290   # both outcomes occur


def _vectors(D):
    rs = np.random.RandomState(100 + D)
    vs = [rs.standard_normal(D).astype(np.float32), (rs.standard_normal(D) * 37.5).astype(np.float32), np.zeros(D, np.float32)]
    half = np.zeros(D, np.float32)
    half[0] = half[-1] = 3.0
    return vs + [half]


@pytest.mark.parametrize("D", [1, 3, 128, 512])
def test_l2_norm_is_bit_equal_to_the_sequential_f32_restatement(mi, D):
    for v in _vectors(D):
        got = mi.l2_norm(v)
        assert got.dtype == np.float32 and got.shape == v.shape
        np.testing.assert_array_equal(got, es.l2_norm_ref(v))   # (the all-zero vector: 0 / 0 = NaN on both sides)
    assert np.isnan(mi.l2_norm(np.zeros(D, np.float32))).all()
    # an Array2 is normalised as a whole (utils.rs:31 iterates over every element)
    m = np.stack(_vectors(D)[:2])
    np.testing.assert_array_equal(mi.l2_norm(m), es.l2_norm_ref(m).reshape(m.shape))


@pytest.mark.parametrize("D", [1, 3, 128, 512])
def test_similarity_score_is_bit_equal_to_the_sequential_f32_restatement(mi, D):
    vs = _vectors(D)
    for a in vs:
        for b in vs:
            got, want = mi.similarity_score(a, b), es.similarity_score_ref(a, b)
            assert isinstance(got, np.float32)
            np.testing.assert_array_equal(got, want)
    assert np.isnan(mi.similarity_score(vs[2], vs[0]))   # a zero vector: 0 / 0


def test_restatement_accumulates_in_f32_one_element_at_a_time():
    """The vectorised restatement is the scalar loop (checked on one pair with explicit numpy float32 scalars)."""
    rs = np.random.RandomState(5)
    a, b = rs.standard_normal(130).astype(np.float32), rs.standard_normal(130).astype(np.float32)
    dot = na = nb = np.float32(0)
    for x, y in zip(a, b):
        dot = np.float32(dot + np.float32(x * y))
        na = np.float32(na + np.float32(x * x))
        nb = np.float32(nb + np.float32(y * y))
    want = np.float32(dot / np.float32(np.sqrt(na) * np.sqrt(nb)))
    assert es.similarity_score_ref(a, b) == want


def _refused(mi, rc, *words):
    assert rc == -1, rc   # MI_EINVAL
    msg = mi.lib().mi_last_error().decode()
    assert all(w in msg for w in words), msg


def test_argument_refusals_without_a_gpu(mi):
    L = mi.lib()
    buf = np.zeros(64, np.float32)
    ibuf = np.zeros(64, np.int32)
    p, ip = C.c_void_p(buf.ctypes.data), C.c_void_p(ibuf.ctypes.data)
    f = C.c_float()
    # null pointers
    _refused(mi, L.mi_l2_norm(None, 4, p), "null")
    _refused(mi, L.mi_l2_norm(p, 4, None), "null")
    _refused(mi, L.mi_l2_norm(p, 0, p), "positive")
    _refused(mi, L.mi_similarity_score(None, p, 4, C.byref(f)), "null")
    _refused(mi, L.mi_similarity_score(p, p, 4, None), "null")
    _refused(mi, L.mi_similarity_score(p, p, 0, C.byref(f)), "positive")
    _refused(mi, L.mi_similarity_matrix(0, None, 1, p, 1, 4, p, 0, None), "null")
    _refused(mi, L.mi_similarity_matrix(0, p, 1, None, 1, 4, p, 0, None), "null")
    _refused(mi, L.mi_similarity_matrix(0, p, 1, p, 1, 4, None, 0, None), "null")
    _refused(mi, L.mi_similarity_matrix(0, p, 0, p, 1, 4, p, 0, None), "positive")
    _refused(mi, L.mi_similarity_matrix(0, p, 1, p, 0, 4, p, 0, None), "positive")
    rect, valid = (C.c_int * 4)(), C.c_int()
    _refused(mi, L.mi_face_chip_rect(None, 4, 4, rect, C.byref(valid)), "null")
    h = C.c_void_p()
    _refused(mi, L.mi_fe_create(b"/nonexistent.tflite", 0, None), "null")
    _refused(mi, L.mi_fe_create_from_bytes(None, 0, 0, C.byref(h)), "null")
    n = C.c_int()
    _refused(mi, L.mi_fe_features(None, C.byref(n)), "null")
    box = (C.c_double * 4)(0, 0, 2, 2)
    _refused(mi, L.mi_fe_infer_image(None, p, 4, 4, 12, box, p, 64), "null")
    assert L.mi_fe_model(None) is None
    L.mi_fe_free(None)
    # features outside 1..4096
    for features in (0, -1, 4097):
        _refused(mi, L.mi_similarity_matrix(0, p, 1, p, 1, features, p, 0, None), "features", "4096")
    # max_items outside 1..32767, max_faces outside 1..16, batch: refused before the handle is looked at
    items = lambda max_faces, max_items, handle=None, batch=1: L.mi_fe_infer_face_items(
        handle, p, batch, 4, 4, 12, p, max_faces, ip, ip, max_items, p, ip, None, None, 0, None)
    for max_items in (0, -3, 32768, 1 << 20):
        _refused(mi, items(4, max_items), "max_items", "32767")
    for max_faces in (0, -1, 17):
        _refused(mi, items(max_faces, 8), "max_faces", "16")
    _refused(mi, items(4, 8, batch=0), "batch")
    _refused(mi, items(4, 8), "null")   # everything in range: the missing handle


def test_python_mirror_refuses_bad_budgets_before_sizing_outputs(mi):
    class NoHandle(mi.FaceEmbeddings):
        def __init__(self):   # the checks under test come before the handle is used
            self.device, self.features = 0, 8
    frames = np.zeros((1, 4, 4, 3), np.uint8)
    with pytest.raises(mi.MiError) as e:
        NoHandle().infer_items(frames, dict(faces=np.zeros((1, 17, 17), np.float32), item_frame=np.zeros(4, np.int32), item_face=np.zeros(4, np.int32)))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        mi.similarity_matrix(np.zeros((2, 4), np.float32), np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        mi.similarity_score(np.zeros(4, np.float32), np.zeros(5, np.float32))


@pytest.mark.parametrize("features,reshape", [(128, True), (512, False)])
def test_synthetic_embedding_graph_lowers_and_the_oracle_runs_it(mi, oracle, tmp_path, features, reshape):
    blob = es.embed_graph(71, features, reshape)
    for fuse in (0, 2, 4, 5):
        text = mi.plan_describe(blob, fuse)
        assert "k7x7" in text and ("GEMM over the batch" in text) == (fuse >= 2), text   # the 7 x 7 whole-frame head
        assert ("reshape" in text) == reshape, text   # the RESHAPE stays a node
    path = tmp_path / "embed.tflite"
    path.write_bytes(blob)
    x = np.random.RandomState(1).uniform(0, 1, (2, 112, 112, 3)).astype(np.float32)
    out = oracle.Model(str(path)).run(x)
    assert len(out) == 1 and out[0].reshape(2, -1).shape == (2, features)
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 1e-3
