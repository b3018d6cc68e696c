"""Aligned face chips, the host side (csrc/face_align.hpp through mi_face_align_roi / mi_face_align_points / mi_face_align_template): the
closed-form similarity fit against a restatement in plain Python floats, against an independent least-squares solve, its validity rule, the
gather rule of the mesh and detection sources, and the oracle's view of the rotated pictures the GPU test 'alignment aligns' runs on.
Aligned chips are NOT the reference's behaviour (it crops the detector's box); nothing here touches that path."""
import math

import numpy as np
import pytest

import align_ref as ar
from conftest import model_path

SOURCES = ["points", "detection"]   # the 5-point and the 4-point template


def roi_tuple(r):
    return (r.x_center, r.y_center, r.width, r.height, r.rotation, int(r.normalized))


def check_roi(roi, valid, points, source, what):
    """an ROI of the library against the restatement: centre and side bit for bit (+ - * / sqrt only), rotation within 1e-15 (the atan2 of two
    libms; an error e moves a corner by at most side * e: under 2e-11 px at side = 16384, far below the f32 rounding of the corners)"""
    ok, kind, ref = ar.fit_ref(points, ar.TEMPLATES[source])
    assert bool(valid) == ok, (what, kind)
    if not ok:
        assert roi_tuple(roi) == ar.DEFAULT_ROI, what
        return
    xc, yc, side, rot = ref
    assert (roi.x_center, roi.y_center, roi.width, roi.height) == (xc, yc, side, side), (what, roi_tuple(roi), ref)
    assert abs(roi.rotation - rot) <= 1e-15, (what, roi.rotation, rot)
    assert int(roi.normalized) == 0


# ---------------------------------------------------------------------------------------------------- 1. the fit against the restatement
@pytest.mark.parametrize("source", SOURCES)
def test_fit_equals_the_sequential_restatement(mi, source):
    n_rot = 0
    for name, pts in ar.fit_cases(source):
        roi, valid = mi.face_align_roi(pts, source)
        assert valid, name
        check_roi(roi, valid, pts, source, name)
        n_rot += roi.rotation != 0.0
    assert n_rot >= 16
    # the placements are what they claim: without noise the fit returns the similarity the points were made with, up to their f32 rounding
    for (name, c, s, d), (_, pts) in zip(ar.PLACEMENTS, ar.fit_cases(source)):
        roi, _ = mi.face_align_roi(pts, source)
        assert abs(roi.x_center - c[0]) < 1e-3 and abs(roi.y_center - c[1]) < 1e-3 and abs(roi.width / (112.0 * s) - 1.0) < 1e-5, name
        turn = (roi.rotation - math.radians(d) + math.pi) % (2.0 * math.pi) - math.pi
        assert abs(turn) < 1e-5, (name, roi.rotation)


# ---------------------------------------------------------------------------------------------------- 2. independent optimality
def lstsq_similarity(points, template):
    """q ~ [[a,-b],[b,a]] (p - mean p) + t by numpy.linalg.lstsq in f64 -> (z = a + ib, image -> chip map)"""
    p = np.asarray(points, np.float32).astype(np.float64)
    q = np.asarray(template, np.float64)
    m = p.mean(axis=0)
    x, y = p[:, 0] - m[0], p[:, 1] - m[1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    M = np.concatenate([np.stack([x, -y, one, zero], axis=1), np.stack([y, x, zero, one], axis=1)])
    a, b, tx, ty = np.linalg.lstsq(M, np.concatenate([q[:, 0], q[:, 1]]), rcond=None)[0]
    to_chip = lambda px, py: (a * (px - m[0]) - b * (py - m[1]) + tx, b * (px - m[0]) + a * (py - m[1]) + ty)
    return complex(a, b), to_chip


@pytest.mark.parametrize("source", SOURCES)
def test_fit_is_the_least_squares_optimum(mi, source):
    t = ar.TEMPLATES[source]
    for name, pts in ar.fit_cases(source):
        roi, valid = mi.face_align_roi(pts, source)
        assert valid
        z, to_chip = lstsq_similarity(pts, t)
        if name.endswith("noisy"):
            mine = (112.0 / roi.width) * complex(math.cos(-roi.rotation), math.sin(-roi.rotation))
            assert abs(mine - z) <= 1e-12 * abs(z), (name, mine, z)
        else:
            # Rect::points of the ROI, carried to the chip by the independent solve: the chip's own corners
            h, c, s = roi.width / 2.0, math.cos(roi.rotation), math.sin(roi.rotation)
            for (dx, dy), want in zip(((-h, -h), (h, -h), (h, h), (-h, h)), ((0.0, 0.0), (112.0, 0.0), (112.0, 112.0), (0.0, 112.0))):
                got = to_chip(roi.x_center + dx * c - dy * s, roi.y_center + dx * s + dy * c)
                assert abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9, (name, got, want)


# ---------------------------------------------------------------------------------------------------- 3. invalid inputs
def test_invalid_points_give_valid_zero_and_no_exception(mi):
    good = ar.place(ar.TEMPLATE5, (160.0, 120.0))
    cases = {"S": np.full((5, 2), 77.25, np.float32), "input nan": good.copy(), "input inf": good.copy()}
    cases["input nan"][2, 1] = np.nan
    cases["input inf"][4, 0] = -np.inf
    for what, pts in cases.items():
        ok, kind, _ = ar.fit_ref(pts, ar.TEMPLATE5)
        assert not ok and kind == what.split()[0], (what, kind)   # the case is the kind it claims to be
        roi, valid = mi.face_align_roi(pts, "points")
        assert valid is False and roi_tuple(roi) == ar.DEFAULT_ROI, what
    assert np.isnan(cases["input nan"]).sum() == 1 and np.isinf(cases["input inf"]).sum() == 1
    # all four points of the detector's template equal as well
    roi, valid = mi.face_align_roi(np.zeros((4, 2), np.float32), "detection")
    assert valid is False and roi_tuple(roi) == ar.DEFAULT_ROI
    for n in (1, 6):
        for source in ("points", "mesh", "detection"):
            with pytest.raises(mi.MiError) as err:
                mi.face_align_roi(np.zeros((n, 2), np.float32), source)
            assert err.value.code == -1   # MI_EINVAL
    # the count is the template's: five points for the detector's four-point template and the other way round are refused
    for n, source in ((5, "detection"), (4, "points"), (4, "mesh")):
        with pytest.raises(mi.MiError) as err:
            mi.face_align_roi(good[:n] if n < 5 else good, source)
        assert err.value.code == -1
    with pytest.raises(ValueError):
        mi.face_align_roi(good, "box")


# ---------------------------------------------------------------------------------------------------- 4. gather rule, template
def test_gather_rule_and_template(mi):
    rs = np.random.RandomState(11)
    lm = rs.uniform(-0.2, 1.2, (468, 3)).astype(np.float32)
    det = rs.uniform(0.0, 1.0, 17).astype(np.float32)
    for size in ((540, 360), (1080, 720), (333, 17)):
        got = mi.face_align_points("mesh", lm, size)
        assert got.shape == (5, 2) and got.dtype == np.float32
        np.testing.assert_array_equal(got, ar.gather_ref("mesh", lm, *size))
        got = mi.face_align_points("detection", det, size)
        assert got.shape == (4, 2)
        np.testing.assert_array_equal(got, ar.gather_ref("detection", det, *size))
    # the indices are the ones the rule names: moving any other landmark changes nothing
    used = [33, 133, 362, 263, 1, 61, 291]
    other = lm.copy()
    other[[i for i in range(468) if i not in used]] += 1.0
    other[:, 2] -= 5.0
    np.testing.assert_array_equal(mi.face_align_points("mesh", other, (540, 360)), mi.face_align_points("mesh", lm, (540, 360)))
    for i in used:
        moved = lm.copy()
        moved[i, :2] += 0.125
        assert (mi.face_align_points("mesh", moved, (540, 360)) != mi.face_align_points("mesh", lm, (540, 360))).any(), i
    pts = rs.uniform(0, 300, (5, 2)).astype(np.float32)
    np.testing.assert_array_equal(mi.face_align_points("points", pts, (320, 240)), pts)
    for source in ("points", "mesh"):
        t = mi.face_align_template(source)
        assert t.dtype == np.float64 and t.tolist() == [list(p) for p in ar.TEMPLATE5]
    t4 = mi.face_align_template("detection")
    assert t4.tolist() == [list(p) for p in ar.TEMPLATE4] and t4[3].tolist() == [(41.5493 + 70.7299) / 2.0, (92.3655 + 92.2041) / 2.0]
    assert ar.TEMPLATE5[0] == (38.2946, 51.6963) and ar.TEMPLATE5[4] == (70.7299, 92.2041)


# ---------------------------------------------------------------------------------------------------- 5. the inputs of 'alignment aligns'
def test_oracle_finds_one_face_in_each_rotated_picture(oracle, man_image):
    """man.jpg rotated by -20, 0 and +20 degrees: the oracle's detector (back model) finds exactly one face and its mesh passes the flag"""
    frames = ar.rotated_frames(man_image)
    assert frames.shape == (3,) + man_image.shape and (frames[1] == man_image).all()
    H, W = man_image.shape[:2]
    fd, fl = oracle.Model(model_path("back")), oracle.Model(model_path("landmark"))
    anchors = oracle.ssd_anchors(oracle.FD_BACK)
    for angle, img in zip(ar.ANGLES, frames):
        assert angle == 0 or not img[0, 0].any()   # black outside the turned picture
        t, pad = oracle.image_to_tensor(img, None, (256, 256), True, (-1., 1.), False)
        rb, rs = fd.run(t[None])
        dets = oracle.fd_postprocess(rb[0], rs[0], anchors, 256.0, pad)
        assert len(dets) == 1, (angle, len(dets))
        roi = oracle.face_detection_to_roi(dets[0], (W, H))
        t2, _ = oracle.image_to_tensor(img, roi, (192, 192), False, (0., 1.), False)
        raw, flag = fl.run(t2[None])
        assert oracle.lib().orc_face_flag_passes(float(flag.reshape(-1)[-1])), angle
