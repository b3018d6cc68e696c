"""Aligned face chips on the device (mi_fe_infer_aligned_items / mi_fe_infer_image_aligned): the fitted ROIs against the host entry, the chips
bit for bit against the oracle's image_to_tensor of the WHOLE frame with that ROI, the network's rows against the handle's own model on those
chips, l2_norm bit for bit, every way an item can be invalid, item counts on both sides of the engine's batch thresholds, the mesh and
detection sources on what Pipeline.run_faces leaves in device memory, that alignment does align, and that the box path (the reference's
behaviour, which aligned chips are NOT) keeps every bit when the two families are interleaved on one handle.  The embedding network is
synthetic (embed_synth.embed_graph): scores mean nothing."""
import numpy as np
import pytest

import align_ref as ar
import embed_synth as es

pytestmark = pytest.mark.gpu

CW, CH = 320, 240
D = 128


def _torch():
    """torch carries the device-resident operands: on a GPU box a broken install is a failure, not a skip"""
    try:
        import torch
        return torch
    except Exception as e:  # noqa: BLE001
        pytest.fail("torch is needed for device-resident frames: %r" % (e,))


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


@pytest.fixture(scope="module")
def fe(gpu):
    h = gpu.FaceEmbeddings(model_bytes=es.embed_graph(71, D, True))
    yield h
    h.close()


def oracle_aligned_chip(oracle, frame, roi):
    r = oracle.Rect(roi.x_center, roi.y_center, roi.width, roi.height, roi.rotation, 0)
    chip, _ = oracle.image_to_tensor(np.ascontiguousarray(frame), r, (112, 112), False, (0., 1.), False)
    return chip


def check_rois(got, want, valid, what):
    """got: RECT_DTYPE [M]; want: the host entry's Rects: centre and side bit for bit, rotation within 1e-15 (test_align_cpu.check_roi)"""
    for j, (g, w) in enumerate(zip(got, want)):
        if valid[j]:
            assert (g["x_center"], g["y_center"], g["width"], g["height"], g["normalized"]) == (w.x_center, w.y_center, w.width, w.height, 0), (what, j)
            assert abs(g["rotation"] - w.rotation) <= 1e-15, (what, j, g["rotation"], w.rotation)
        else:
            assert tuple(g)[:6] == ar.DEFAULT_ROI, (what, j, g)
        assert g["pad"] == 0


def check_rows(gpu, fe, out, valid, chips, what):
    """validity, chips bit for bit, zeros for invalid items, embeddings == l2_norm(raw), raw == the handle's own model on these chips at this batch"""
    M = len(valid)
    np.testing.assert_array_equal(out["valid"], np.asarray(valid, np.int32), err_msg=what)
    own = fe.model.run(np.ascontiguousarray(out["chips"]))[0].reshape(M, -1)
    for j in range(M):
        np.testing.assert_array_equal(out["chips"][j], chips[j], err_msg="%s: item %d" % (what, j))
        if valid[j]:
            np.testing.assert_array_equal(out["raw"][j], own[j], err_msg="%s: raw of item %d" % (what, j))
            np.testing.assert_array_equal(out["embeddings"][j], gpu.l2_norm(out["raw"][j]), err_msg="%s: item %d" % (what, j))
        else:
            assert not out["chips"][j].any() and not out["raw"][j].any() and not out["embeddings"][j].any(), (what, j)


# ---------------------------------------------------------------------------------------------------- 1. chips and ROIs, bit for bit
def _points_case(oracle, gpu):
    """three frames with padded rows and the hand-made items: per item its frame, points, point_valid and what the host says of it"""
    buf, frames = ar.padded_frames(31, 3, CH, CW)
    T = ar.TEMPLATE5
    good = ar.place(T, (150.0, 110.0), 0.9, 5.0)
    nan = good.copy()
    nan[3, 0] = np.nan
    # (frame, points, point_valid, valid)
    items = [
        (0, ar.place(T, (56.0, 56.0)), 1, True),                     # identity placement: the chip is the frame's top left 112 x 112
        (1, ar.place(T, (160.0, 120.0), 0.5), 1, True),
        (2, ar.place(T, (160.0, 120.0), 2.3), 1, True),              # side 257.6 > 240: leaves the frame above and below
        (0, ar.place(T, (200.0, 100.0), 1.0, 30.0), 1, True),
        (1, ar.place(T, (100.0, 150.0), 1.0, -90.0), 1, True),
        (2, ar.place(T, (160.0, 120.0), 0.8, 180.0), 1, True),
        (0, ar.place(T, (10.0, 230.0), 1.0, 10.0), 1, True),         # leaves the frame on the left and at the bottom
        (1, ar.place(T, (-300.0, -300.0)), 1, True),                 # wholly outside: valid, all zeros
        (2, np.full((5, 2), 120.5, np.float32), 1, False),           # equal points
        (0, nan, 1, False),
        (1, good, 0, False),                                         # point_valid = 0
        (-1, good, 1, False),                                        # an unused slot
        (3 + 7, good, 1, False),                                     # a frame behind the batch
    ]
    rois, chips = [], []
    for b, pts, pv, ok in items:
        roi, fit_ok = gpu.face_align_roi(pts, "points")
        in_batch = 0 <= b < 3
        assert (fit_ok and bool(pv) and in_batch) == ok, (b, pv, fit_ok)   # the case is what it claims to be
        rois.append(roi)
        chips.append(oracle_aligned_chip(oracle, frames[b], roi) if ok else np.zeros((112, 112, 3), np.float32))
    # ... and the fits of the gated items would have been valid: it is the gate that makes them invalid
    assert all(gpu.face_align_roi(items[j][1], "points")[1] for j in (10, 11, 12))
    assert np.abs(chips[0] - frames[0, :112, :112].astype(np.float32) / np.float32(255.0)).mean() < 0.01
    assert chips[6].any() and not chips[6][111, 0].any() and not chips[7].any()
    return buf, frames, items, rois, chips


@pytest.fixture(scope="module")
def points_case(oracle, gpu):
    return _points_case(oracle, gpu)


@pytest.mark.parametrize("M", [13, 1, 31, 32, 33])
def test_point_items_are_the_oracles_tensors_of_the_fitted_rois(gpu, oracle, fe, points_case, M):
    torch = _torch()
    buf, frames, items, rois, chips = points_case
    idx = np.arange(M) % len(items)   # the list truncated, or gone round again
    item_frame = np.asarray([items[i][0] for i in idx], np.int32)
    points = np.stack([items[i][1] for i in idx]).astype(np.float32)
    point_valid = np.asarray([items[i][2] for i in idx], np.int32)
    valid = [items[i][3] for i in idx]
    kw = dict(source="points", want_raw=True, want_chips=True, want_rois=True)
    host = fe.infer_items_aligned(frames, dict(item_frame=item_frame), points=points, point_valid=point_valid, **kw)
    assert host["embeddings"].shape == (M, D) and host["rois"].shape == (M,)
    what = "max_items = %d" % M
    check_rows(gpu, fe, host, valid, [chips[i] for i in idx], what)
    check_rois(host["rois"], [rois[i] for i in idx], valid, what)
    # rows padded on the device as well
    dframes = torch.from_numpy(buf).cuda()[:, :, :3 * CW].unflatten(2, (CW, 3))
    assert tuple(dframes.stride()) == (CH * (3 * CW + 5), 3 * CW + 5, 3, 1)
    dev = fe.infer_items_aligned(dframes, dict(item_frame=torch.from_numpy(item_frame).cuda()), points=torch.from_numpy(points).cuda(),
                                 point_valid=torch.from_numpy(point_valid).cuda(), **kw)
    torch.cuda.synchronize()
    for k in host:
        np.testing.assert_array_equal(dev[k].cpu().numpy().view(np.uint8).reshape(-1), np.ascontiguousarray(host[k]).view(np.uint8).reshape(-1), err_msg=k)
    if M == 13:
        # no point_valid at all: item 10 becomes valid, nothing else moves
        free = fe.infer_items_aligned(frames, dict(item_frame=item_frame), points=points, **kw)
        want = list(valid)
        want[10] = True
        np.testing.assert_array_equal(free["valid"], np.asarray(want, np.int32))
        for k in ("chips", "raw", "embeddings"):
            np.testing.assert_array_equal(np.delete(free[k], 10, axis=0), np.delete(host[k], 10, axis=0), err_msg=k)
        np.testing.assert_array_equal(free["chips"][10], oracle_aligned_chip(oracle, frames[items[10][0]], rois[10]))


def test_aligned_items_refuse_a_budget_the_launches_cannot_take(gpu, fe):
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(gpu.MiError) as err:
        fe.infer_items_aligned(frames, dict(item_frame=np.zeros(32768, np.int32)), source="points", points=np.zeros((32768, 5, 2), np.float32))
    assert err.value.code == -1   # MI_EINVAL, before anything is queued
    # ... and the C entry itself, behind the wrapper's own check (buffers of the full size: nothing may be read or written anyway)
    import ctypes as C
    M = 32768
    item_frame, points = np.zeros(M, np.int32), np.zeros((M, 5, 2), np.float32)
    emb, valid = np.zeros((M, D), np.float32), np.zeros(M, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    rc = gpu.lib().mi_fe_infer_aligned_items(fe.h, ptr(frames), 1, 8, 8, 24, gpu.ALIGN_SOURCES["points"], ptr(points), None, 1, ptr(item_frame), None, M,
                                             ptr(emb), ptr(valid), None, None, None, gpu.MI_MEM_HOST, None)
    assert rc == -1 and b"max_items" in gpu.lib().mi_last_error()
    for source, n in (("points", 4), ("detection", 5), ("mesh", 6)):
        with pytest.raises(gpu.MiError) as err:
            fe.infer_aligned(np.zeros((8, 8, 3), np.uint8), np.zeros((n, 2), np.float32), source=source)
        assert err.value.code == -1   # a point count that is not the template's


# ---------------------------------------------------------------------------------------------------- 2. mesh and detection sources
@pytest.fixture(scope="module")
def faces_case(gpu, man_image):
    """Pipeline.run_faces, in device memory, of three 720 x 1080 canvases made of man.jpg and its mirror image — two faces, one face, none —
    with max_faces = 2 and max_items = 4: three used slots and a spare one"""
    torch = _torch()
    H, W = man_image.shape[:2]
    two = np.zeros((2 * H, 2 * W, 3), np.uint8)
    two[:H, :W] = man_image
    two[:H, W:] = man_image[:, ::-1]
    one = np.zeros_like(two)
    one[H:, W:] = man_image[:, ::-1]
    frames = np.stack([two, one, np.zeros_like(two)])
    dframes = torch.from_numpy(frames).cuda()
    p = gpu.Pipeline(gpu.FaceDetectionModel.BackCamera)
    dres = p.run_faces(dframes, max_faces=2, max_items=4)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in dres.items()}
    p.close()
    assert res["item_frame"].tolist() == [0, 0, 1, -1] and res["item_face"].tolist() == [0, 1, 0, -1], (res["item_frame"], res["item_face"])
    return frames, dframes, dres, res


@pytest.mark.parametrize("source", ["mesh", "detection"])
def test_mesh_and_detection_sources_on_a_device_resident_result(gpu, oracle, fe, faces_case, source):
    torch = _torch()
    frames, dframes, dres, res = faces_case
    H, W = frames.shape[1:3]
    out = fe.infer_items_aligned(dframes, dres, source=source, want_raw=True, want_chips=True, want_rois=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["rois"] = out["rois"].view(gpu.RECT_DTYPE).reshape(-1)
    M = len(res["item_frame"])
    valid, rois, chips, points = [], [], [], []
    for j in range(M):
        b, k = int(res["item_frame"][j]), int(res["item_face"][j])
        ok, roi, pts = False, None, None
        if b >= 0 and (source == "detection" or res["present"][j]):
            pts = gpu.face_align_points(source, res["landmarks"][j] if source == "mesh" else res["faces"][b, k], (W, H))
            roi, ok = gpu.face_align_roi(pts, source)
        valid.append(ok)
        rois.append(roi)
        points.append(pts)
        chips.append(oracle_aligned_chip(oracle, frames[b], roi) if ok else np.zeros((112, 112, 3), np.float32))
    assert valid[:3] == [True, True, True] and not valid[3], valid
    check_rows(gpu, fe, out, valid, chips, source)
    check_rois(out["rois"], rois, valid, source)
    # the faces are upright and about 200 px wide in man.jpg: the fit is a plausible one
    for j in range(3):
        assert 100.0 < rois[j].width < 400.0 and abs(rois[j].rotation) < 0.35, (j, rois[j])
    # one picture, its points from the host: the chip and the embedding of the matching row (the chip through an items call of one item)
    j = 1
    b = int(res["item_frame"][j])
    e, roi = fe.infer_aligned(frames[b], points[j], source="points" if source == "mesh" else source, want_roi=True)
    assert e.shape == (1, D) and e.dtype == np.float32
    assert (roi.x_center, roi.y_center, roi.width, roi.rotation) == (rois[j].x_center, rois[j].y_center, rois[j].width, rois[j].rotation)
    if source == "mesh":
        single = fe.infer_items_aligned(frames[b:b + 1], dict(item_frame=np.zeros(1, np.int32)), source="points", points=points[j][None], want_chips=True)
    else:
        single = fe.infer_items_aligned(frames[b:b + 1], dict(item_frame=np.zeros(1, np.int32), item_face=np.zeros(1, np.int32),
                                                              faces=res["faces"][b:b + 1, int(res["item_face"][j])][None]),
                                        source="detection", want_chips=True)
    assert single["valid"][0] == 1
    np.testing.assert_array_equal(single["chips"][0], out["chips"][j])
    np.testing.assert_array_equal(e[0], single["embeddings"][0])
    np.testing.assert_array_equal(e[0], out["embeddings"][j])   # ... and of the matching row of the items call itself
    with pytest.raises(gpu.MiError) as err:
        fe.infer_aligned(frames[b], np.full_like(points[j], 3.0), source="points" if source == "mesh" else source)
    assert err.value.code == -5   # MI_ERANGE: no fit


# ---------------------------------------------------------------------------------------------------- 3. alignment aligns
def test_aligned_chips_of_a_rotated_face_stay_closer_to_the_upright_one(gpu, fe, man_image):
    """man.jpg turned by -20, 0 and +20 degrees (test_align_cpu checks these pictures on the oracle): the aligned chips of a turned face differ
    from the upright one by interpolation, the box chips by the rotation itself — a strict comparison of the two paths, no constant"""
    frames = ar.rotated_frames(man_image)
    p = gpu.Pipeline(gpu.FaceDetectionModel.BackCamera)
    res = p.run_faces(frames, max_faces=1, max_items=3)
    p.close()
    assert res["item_frame"].tolist() == [0, 1, 2] and res["present"].tolist() == [1, 1, 1], (res["item_frame"], res["present"])
    box = fe.infer_items(frames, res, want_chips=True)
    aligned = fe.infer_items_aligned(frames, res, source="mesh", want_chips=True, want_rois=True)
    assert box["valid"].tolist() == [1, 1, 1] and aligned["valid"].tolist() == [1, 1, 1]
    upright = ar.ANGLES.index(0)
    for t, angle in enumerate(ar.ANGLES):
        if angle == 0:
            continue
        da = float(np.abs(aligned["chips"][t] - aligned["chips"][upright]).mean())
        db = float(np.abs(box["chips"][t] - box["chips"][upright]).mean())
        print("angle %+d: mean |aligned - upright| = %.4f, mean |box - upright| = %.4f, fitted rotation %.4f rad" % (angle, da, db, aligned["rois"][t]["rotation"]))
        assert da < db, (angle, da, db)


# ---------------------------------------------------------------------------------------------------- 4. existing paths unchanged
def box_det(x, y, w, h):
    """a normalised detection whose rectangle is (x, y, w, h): a quarter pixel inside, so that f32 rounding cannot move a truncation"""
    d = np.zeros(17, np.float32)
    d[:4] = ((x + 0.25) / CW, (y + 0.25) / CH, (x + w + 0.5) / CW, (y + h + 0.5) / CH)
    return d


def raw_det(xmin, ymin, xmax, ymax):
    d = np.zeros(17, np.float32)
    d[:4] = (xmin, ymin, xmax, ymax)
    return d


# the chip case of test_embeddings_gpu.py: (frame, detection, the rectangle it must give, or None for an invalid one)
BOX_ITEMS = [
    (0, box_det(0, 0, 1, 1), (0, 0, 1, 1)),
    (0, box_det(319, 239, 1, 1), (319, 239, 1, 1)),
    (1, box_det(17, 101, 2, 3), (17, 101, 2, 3)),
    (1, box_det(0, 0, CW, CH), (0, 0, CW, CH)),
    (2, box_det(100, 60, 112, 112), (100, 60, 112, 112)),
    (2, box_det(207, 129, 113, 111), (207, 129, 113, 111)),
    (0, box_det(20, 203, 300, 37), (20, 203, 300, 37)),
    (0, raw_det(-1.2 / CW, 0.25, 0.5, 0.75), None),
    (1, raw_det(0.5, 0.25, 321.5 / CW, 0.75), None),
    (1, raw_det(0.5, 0.25, 0.5 + 0.5 / CW, 0.75), None),
    (2, raw_det(np.nan, 0.25, 0.5, np.nan), None),
    (2, raw_det(0.25, 0.25, 1e30, 0.75), None),
]


def test_box_path_keeps_every_bit_between_aligned_calls(gpu, oracle, fe, points_case):
    buf, frames = ar.padded_frames(29, 3, CH, CW)
    F = 6
    faces = np.zeros((3, F, 17), np.float32)
    used, item_frame, item_face, want = [0, 0, 0], [], [], []
    for b, d, rect in BOX_ITEMS:
        faces[b, used[b]] = d
        item_frame.append(b)
        item_face.append(used[b])
        used[b] += 1
        got, ok = es.chip_rect(d, CW, CH)
        assert ok == (rect is not None) and (rect is None or got == rect)
        want.append(rect)
    item_frame += [-1, 1]
    item_face += [123456789, F + 93]
    want += [None, None]

    def crop_chip(b, r):
        x, y, w, h = r
        return oracle.image_to_tensor(np.ascontiguousarray(frames[b, y:y + h, x:x + w]), None, (112, 112), False, (0., 1.), False)[0]
    chips = np.stack([crop_chip(b, r) if r is not None else np.zeros((112, 112, 3), np.float32) for b, r in zip(item_frame, want)])
    result = dict(faces=faces, item_frame=np.asarray(item_frame, np.int32), item_face=np.asarray(item_face, np.int32))
    _, aframes, items, _, _ = points_case
    apoints = np.stack([it[1] for it in items]).astype(np.float32)
    aresult = dict(item_frame=np.asarray([it[0] for it in items], np.int32))
    bbox = (100.0, 60.0, 212.0, 172.0)   # item 4's rectangle on frame 2

    def box_calls():
        out = fe.infer_items(frames, result, want_raw=True, want_chips=True)
        np.testing.assert_array_equal(out["valid"], np.asarray([r is not None for r in want], np.int32))
        np.testing.assert_array_equal(out["chips"], chips)
        single = fe.infer(np.ascontiguousarray(frames[2]), bbox)
        return out, single

    def aligned_calls():
        a = fe.infer_items_aligned(aframes, aresult, source="points", points=apoints, want_raw=True, want_chips=True)
        e = fe.infer_aligned(np.ascontiguousarray(aframes[0]), items[3][1])
        return a, e
    first, first_single = box_calls()
    a1, e1 = aligned_calls()
    second, second_single = box_calls()
    a2, e2 = aligned_calls()
    third, third_single = box_calls()
    for k in first:
        np.testing.assert_array_equal(second[k], first[k], err_msg=k)
        np.testing.assert_array_equal(third[k], first[k], err_msg=k)
    np.testing.assert_array_equal(second_single, first_single)
    np.testing.assert_array_equal(third_single, first_single)
    for k in a1:
        np.testing.assert_array_equal(a2[k], a1[k], err_msg=k)
    np.testing.assert_array_equal(e2, e1)
