"""mi_tracker's two rules through their host entries (no GPU): mi_track_roi_from_landmarks against the composition it states
(bbox_from_landmarks + bbox_to_roi of this library, and the oracle's bbox_to_roi fed numpy's min / max and the pixel key points), and
mi_track_detect_layout against a numpy restatement, with the fairness bound of track.hpp checked by simulation."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import model_path
from test_pipeline_faces_gpu import oracle_faces

EINVAL = -1
SIZES = [(1080, 720), (640, 640)]


def oracle_roi(oracle, lm, size):
    """the rule, restated: numpy min / max (f32 values widened to f64), eye corners 33 and 263 in pixels, orc_bbox_to_roi(1.5, 1.5, SquareLong)"""
    lm = np.asarray(lm, np.float32)
    x, y = lm[:, 0].astype(np.float64), lm[:, 1].astype(np.float64)
    bbox = (C.c_double * 4)(x.min(), y.min(), x.max(), y.max())
    w, h = float(size[0]), float(size[1])
    kp = (C.c_double * 4)(float(lm[33, 0]) * w, float(lm[33, 1]) * h, float(lm[263, 0]) * w, float(lm[263, 1]) * h)
    want = oracle.Rect()
    rc = oracle.lib().orc_bbox_to_roi(bbox, size[0], size[1], kp, 1.5, 1.5, 1, C.byref(want))
    return rc, want


def check_roi(mi, oracle, lm, size, what):
    """centre, width and height bit for bit, rotation within 1e-15 (test_align_cpu.check_roi's bound for the atan2 of two libms)"""
    lm = np.ascontiguousarray(lm, np.float32)
    got, valid = mi.track_roi_from_landmarks(lm, size)
    assert valid, what
    # this library's own composition
    box = mi.bbox_from_landmarks([mi.Landmark(*map(float, p)) for p in lm])
    w, h = float(size[0]), float(size[1])
    kp = [(float(lm[33, 0]) * w, float(lm[33, 1]) * h), (float(lm[263, 0]) * w, float(lm[263, 1]) * h)]
    own = mi.bbox_to_roi(box, size, kp, (1.5, 1.5), 1)
    rc, want = oracle_roi(oracle, lm, size)
    assert rc == 0, what
    for ref in (own, want):
        assert (got.x_center, got.y_center, got.width, got.height) == (ref.x_center, ref.y_center, ref.width, ref.height), what
        assert abs(got.rotation - ref.rotation) <= 1e-15, (what, got.rotation, ref.rotation)
    assert got.normalized and -math.pi <= got.rotation < math.pi
    return got


@pytest.fixture(scope="module")
def man_landmarks(oracle, man_image):
    """the oracle's landmarks of man.jpg (detector -> ROI -> mesh), normalised to the picture"""
    models = (oracle.Model(model_path("back")), oracle.Model(model_path("landmark")), oracle.Model(model_path("iris")))
    _, per_face = oracle_faces(oracle, models, man_image, "back", 1)
    assert per_face and per_face[0] is not None
    return np.ascontiguousarray(per_face[0]["landmarks"], np.float32)


def test_roi_of_the_oracles_landmarks(mi, oracle, man_landmarks, man_image):
    H, W = man_image.shape[:2]
    for size in [(W, H)] + SIZES:
        roi = check_roi(mi, oracle, man_landmarks, size, "man.jpg %s" % (size,))
        assert 0.2 < roi.width < 1.5 and 0.2 < roi.height < 1.5 and abs(roi.rotation) < 0.3


@pytest.mark.parametrize("size", SIZES)
def test_roi_of_random_landmark_sets(mi, oracle, size):
    rs = np.random.RandomState(20 + size[0])
    for n in range(100):
        c, r = rs.uniform(0.2, 0.8, 2), rs.uniform(0.01, 0.4)
        lm = np.concatenate([c + rs.uniform(-r, r, (468, 2)), rs.uniform(-1, 1, (468, 1))], axis=1).astype(np.float32)
        if n % 10 == 0:   # a box that leaves the frame is still normalised: xmin >= -1, xmax < 2, ymin >= -1
            lm[:, 0] += np.float32(0.9)
        check_roi(mi, oracle, lm, size, "set %d" % n)


def test_rotation_is_taken_in_pixels(mi, oracle):
    """Two eye corners at 45 degrees in PIXELS on a 2 : 1 frame (200 px right, 200 px down): in normalised coordinates the same segment
    stands at atan(2), 63.4 degrees."""
    size = (1000, 500)
    lm = np.full((468, 3), 0.5, np.float32)
    lm[0, :2], lm[1, :2] = (0.25, 0.25), (0.75, 0.75)   # the box
    lm[33, :2] = (0.4, 0.3)
    lm[263, :2] = (0.6, 0.7)
    roi = check_roi(mi, oracle, lm, size, "45 degrees")
    dx, dy = float(lm[263, 0]) * 1000.0 - float(lm[33, 0]) * 1000.0, float(lm[263, 1]) * 500.0 - float(lm[33, 1]) * 500.0
    assert abs(dx - 200.0) < 1e-4 and abs(dy - 200.0) < 1e-4
    assert abs(roi.rotation - math.pi / 4) < 1e-6, roi.rotation            # -atan2(y0 - y1, x1 - x0) of the pixel points
    assert abs(roi.rotation - math.atan(2.0)) > 0.3


@pytest.mark.parametrize("case", ["nan_x", "inf_y", "xmin_below_minus_1", "xmax_2", "all_equal"])
def test_invalid_landmark_sets(mi, case):
    rs = np.random.RandomState(5)
    lm = rs.uniform(0.3, 0.7, (468, 3)).astype(np.float32)
    assert mi.track_roi_from_landmarks(lm, (1080, 720))[1]
    if case == "nan_x":
        lm[200, 0] = np.nan
    elif case == "inf_y":
        lm[467, 1] = np.inf
    elif case == "xmin_below_minus_1":
        lm[7, 0] = np.float32(-1.0000001)
    elif case == "xmax_2":
        lm[7, 0] = 2.0
    else:
        lm[:] = np.float32(0.5)
    roi, valid = mi.track_roi_from_landmarks(lm, (1080, 720))
    assert not valid
    assert (roi.x_center, roi.y_center, roi.width, roi.height, roi.rotation, roi.normalized) == (0.0, 0.0, 0.0, 0.0, 0.0, 0)


def layout_ref(tracked, max_detect, start):
    """the detect plan, restated"""
    S = len(tracked)
    lost = [s % S for s in range(start, start + S) if tracked[s % S] == 0]
    det = np.full((max_detect,), -1, np.int32)
    used = min(len(lost), max_detect)
    det[:used] = lost[:used]
    return det, used, len(lost) - used


@pytest.mark.parametrize("S", [1, 2, 255, 256, 257, 600])
def test_detect_layout_against_the_restatement(mi, S):
    rs = np.random.RandomState(S)
    starts = range(S) if S <= 2 else sorted(set([0, 1, S // 2, S - 2, S - 1] + [int(v) for v in rs.randint(0, S, 6)]))
    masks = [np.zeros(S, np.int32), np.ones(S, np.int32), (rs.rand(S) < 0.5).astype(np.int32), (rs.rand(S) < 0.9).astype(np.int32) * 7]
    for D in sorted({1, min(2, S), S}):
        for start in starts:
            for tracked in masks:
                det, used, left = mi.track_detect_layout(tracked, D, start)
                want = layout_ref(tracked, D, start)
                np.testing.assert_array_equal(det, want[0], err_msg="S %d D %d start %d" % (S, D, start))
                assert (used, left) == want[1:]


@pytest.mark.parametrize("S,D", [(6, 2), (7, 3), (257, 16), (600, 1)])
def test_fairness_bound_by_simulation(mi, S, D):
    """Half the streams are lost for ever (they never show a face); the others are acquired by the step that gives them a slot.  Every lost
    stream must hold a slot at least once in any ceil(S / D) consecutive steps (track.hpp), so every stream that can be acquired is
    acquired within that many steps, and the hopeless ones keep being served at that rate."""
    rs = np.random.RandomState(S + D)
    hopeless = rs.permutation(S)[: S // 2]
    tracked = np.zeros(S, np.int32)
    bound = -(-S // D)
    start, last_slot = 0, np.full(S, -1)
    steps = 3 * bound if S < 600 else bound + 5
    for step in range(steps):
        det, used, left = mi.track_detect_layout(tracked, D, start)
        lost_before = tracked == 0
        for s in det[:used]:
            last_slot[s] = step
            if s not in hopeless:
                tracked[s] = 1
        waiting = step - last_slot[lost_before]
        assert waiting.max() < bound, "a lost stream waited %d steps, bound %d (step %d)" % (waiting.max(), bound, step)
        start = (start + D) % S
        if step == bound - 1:
            assert tracked.sum() == S - len(hopeless), "every stream with a face is acquired within ceil(S / D) steps"


def test_argument_refusals(mi):
    L = mi.lib()
    lm = np.full((468, 3), 0.5, np.float32)
    lm[0, :2] = 0.25
    roi, ok = mi.Rect(), C.c_int(0)
    p = C.c_void_p(lm.ctypes.data)
    assert L.mi_track_roi_from_landmarks(None, 100, 100, C.byref(roi), C.byref(ok)) == EINVAL
    assert L.mi_track_roi_from_landmarks(p, 100, 100, None, C.byref(ok)) == EINVAL
    assert L.mi_track_roi_from_landmarks(p, 100, 100, C.byref(roi), None) == EINVAL
    assert L.mi_track_roi_from_landmarks(p, 0, 100, C.byref(roi), C.byref(ok)) == EINVAL
    assert L.mi_track_roi_from_landmarks(p, 100, -1, C.byref(roi), C.byref(ok)) == EINVAL
    assert L.mi_track_roi_from_landmarks(p, 100, 100, C.byref(roi), C.byref(ok)) == 0 and ok.value == 1
    tracked, det, n = np.zeros(4, np.int32), np.full(4, 9, np.int32), np.full(2, 9, np.int32)
    pt, pd, pn = (C.c_void_p(a.ctypes.data) for a in (tracked, det, n))
    for args in [(None, 4, 2, 0, pd, pn), (pt, 4, 2, 0, None, pn), (pt, 4, 2, 0, pd, None), (pt, 0, 1, 0, pd, pn), (pt, (1 << 20) + 1, 1, 0, pd, pn),
                 (pt, 4, 0, 0, pd, pn), (pt, 4, 5, 0, pd, pn), (pt, 4, 2, -1, pd, pn), (pt, 4, 2, 4, pd, pn)]:
        assert L.mi_track_detect_layout(*args) == EINVAL, args
        assert b"" != L.mi_last_error()
    assert (det == 9).all() and (n == 9).all(), "a refused call writes nothing"
    assert L.mi_track_detect_layout(pt, 4, 2, 3, pd, pn) == 0
    np.testing.assert_array_equal(det[:2], [3, 0])
    np.testing.assert_array_equal(n, [2, 2])
    with pytest.raises(mi.MiError):
        mi.track_detect_layout([0, 1], 3)
