"""mi_render_face_items (csrc/render_kernels.hip, render_face_items_kernel): the drawing of every face of a frame from the item list of
mi_pipeline_run_faces, against the executable specification oracle/render.py.

The specification of a frame is oracle.render.render_to_image on the annotation list include/mi_face.h states for the entry: the bounds
and keypoints annotations of the frame's detections, then for every item of the frame, in slot order, mesh lines / points, left-eye lines /
points, right-eye lines / points, left iris oval / points, right iris oval / points.  The first three builders are the oracle's; the iris
builder (iris_landmarks_to_render_data, iris_landmark.rs:330-377 with get_iris_diameter, :401-418) is restated below in numpy float64.
Every comparison is over every byte of every frame.
"""
import numpy as np
import pytest

from test_pipeline_faces_gpu import canvases
from test_render_gpu import _padded, _to_numpy, _untouched

pytestmark = pytest.mark.gpu

KEYS = ("faces", "face_counts", "item_frame", "counts", "landmarks", "present", "eyes")
# one colour per group, so that the overwrite order between groups and between the faces of a frame shows in the bytes
STYLE = dict(bounds=(0, 255, 0, 255), keypoints=(0, 0, 255, 255), line_width=2, point_width=3,
             mesh_points=(255, 0, 0, 255), mesh_lines=(255, 128, 0, 255), mesh_thickness=2.0,
             eye_points=(255, 0, 255, 255), eye_lines=(0, 255, 255, 255), eye_thickness=2.0,
             iris_oval=(255, 255, 0, 255), iris_points=(250, 250, 250, 200), iris_thickness=4.0)


def _mi_style(mi, st):
    col = lambda k: mi.Color(*st[k]) if st.get(k) is not None else None
    base = mi.RenderStyle(bounds_color=col("bounds"), keypoint_color=col("keypoints"), line_width=st["line_width"], point_width=st["point_width"],
                          mesh=st.get("mesh_points") is not None, mesh_landmark_color=col("mesh_points"), mesh_connection_color=col("mesh_lines"),
                          mesh_thickness=st["mesh_thickness"], eyes=st.get("eye_points") is not None, eye_landmark_color=col("eye_points"),
                          eye_connection_color=col("eye_lines"), eye_thickness=st["eye_thickness"])
    return mi.RenderItemsStyle(base, iris_oval_color=col("iris_oval"), iris_landmark_color=col("iris_points"), iris_thickness=st["iris_thickness"])


# ------------------------------------------------------------------------------------------------------------ the specification
def iris_landmarks_to_render_data(iris5, image_size, landmark_color, oval_color, thickness):
    """iris_landmark.rs:330-377 in float64: the oval annotation (one normalised rectangle), then the points annotation.
    iris5: [5, >= 2] f32 rows Center, Left, Top, Right, Bottom (IrisIndex), widened to f64 as Landmark does."""
    p = np.asarray(iris5, np.float32).astype(np.float64)
    W, H = np.float64(image_size[0]), np.float64(image_size[1])
    out = []
    if oval_color is not None:
        def d(a, b):                       # get_iris_diameter's closure, :404-409: both ends are scaled, then subtracted
            x0, y0, x1, y1 = p[a, 0] * W, p[a, 1] * H, p[b, 0] * W, p[b, 1] * H
            dx, dy = x0 - x1, y0 - y1
            return np.sqrt(dx * dx + dy * dy)
        radius = (d(1, 3) + d(2, 4)) / np.float64(2.0) / np.float64(2.0)
        radius_h, radius_v = radius / W, radius / H        # :345-346; render_to_image multiplies by W and H again
        cx, cy = p[0, 0], p[0, 1]
        out.append(("rects", [(float(cx - radius_h), float(cy - radius_v), float(cx + radius_h), float(cy + radius_v))], float(thickness), oval_color))
    if landmark_color is not None:
        out.append(("points", [(float(q[0]), float(q[1])) for q in p], float(thickness), landmark_color))
    return out


def frame_annotations(render, b, size, data, st, slots=None, without_ovals=()):
    """the annotation list of frame b (include/mi_face.h, mi_render_face_items).  slots: the slots the frame draws, None = its run in the used
    prefix; without_ovals: (slot, eye) pairs whose oval the ABI does not draw (an empty rectangle)."""
    ann = []
    if data.get("faces") is not None:
        F = data["faces"].shape[1]
        n = min(max(int(data["face_counts"][b]), 0), F)
        ann += render.detections_to_render_data(data["faces"][b, :n], st.get("bounds"), st.get("keypoints"), st["line_width"], st["point_width"])
    if data.get("item_frame") is None:
        return ann
    if slots is None:
        used = min(max(int(data["counts"][0]), 0), len(data["item_frame"]))
        lo, hi = np.searchsorted(data["item_frame"][:used], [b, b + 1], "left")
        slots = range(lo, hi)
    for j in slots:
        if data.get("present") is not None and not data["present"][j]:
            continue
        if data.get("landmarks") is not None and st.get("mesh_points") is not None:
            ann += render.face_landmarks_to_render_data(data["landmarks"][j], st["mesh_points"], st["mesh_lines"], st["mesh_thickness"])
        if data.get("eyes") is not None:
            if st.get("eye_points") is not None:
                for e in range(2):
                    ann += render.eye_landmarks_to_render_data(data["eyes"][j, e], st["eye_points"], st["eye_lines"], st["eye_thickness"])
            for e in range(2):
                oval = None if (j, e) in without_ovals else st.get("iris_oval")
                ann += iris_landmarks_to_render_data(data["eyes"][j, e, 71:76], size, st.get("iris_points"), oval, st["iris_thickness"])
    return ann


def specification(frames, data, st, **kw):
    from oracle import render
    H, W = frames.shape[1:3]
    return np.stack([render.render_to_image(frame_annotations(render, b, (W, H), data, st, **kw), frames[b]) for b in range(len(frames))])


# ------------------------------------------------------------------------------------------------------------ synthetic item lists
BATCH, WIDTH, HEIGHT, MAX_FACES = 5, 97, 61, 3
COUNTS = [2, 0, 3, 1, 3]


def _scene(mi, max_items):
    """-> (frames u8 [5,61,97,3], result dict as Pipeline.run_faces returns it, numpy).  Slots behind the used ones hold 0.5 everywhere and
    present = 1: a renderer that drew one would show it."""
    rs = np.random.RandomState(100 + max_items)
    frames = rs.randint(0, 250, (BATCH, HEIGHT, WIDTH, 3)).astype(np.uint8)
    faces = rs.uniform(0.1, 0.7, (BATCH, MAX_FACES, 17)).astype(np.float32)
    faces[..., 2:4] = faces[..., 0:2] + rs.uniform(0.1, 0.3, (BATCH, MAX_FACES, 2)).astype(np.float32)
    item_frame, item_face, n_items, dropped = mi.face_items_layout(COUNTS, MAX_FACES, max_items)
    M = max_items
    landmarks = rs.uniform(0.05, 0.95, (M, 468, 3)).astype(np.float32)
    eyes = rs.uniform(0.05, 0.95, (M, 2, 76, 3)).astype(np.float32)
    # iris rows: Center c, Left / Right = c -/+ (r, 0), Top / Bottom = c -/+ (0, r * W / H): an oval of 2 r W = 8..15 px both ways
    c = rs.uniform(0.2, 0.8, (M, 2, 2))
    r = rs.uniform(0.04, 0.08, (M, 2))
    rv = r * WIDTH / HEIGHT
    zero = np.zeros_like(r)
    for row, (dx, dy) in enumerate(((zero, zero), (-r, zero), (zero, -rv), (r, zero), (zero, rv))):
        eyes[:, :, 71 + row, 0] = (c[..., 0] + dx).astype(np.float32)
        eyes[:, :, 71 + row, 1] = (c[..., 1] + dy).astype(np.float32)
    present = np.ones((M,), np.int32)
    landmarks[n_items:] = 0.5
    eyes[n_items:] = 0.5
    data = dict(faces=faces, face_counts=np.array(COUNTS, np.int32), item_frame=item_frame, item_face=item_face,
                counts=np.array([n_items, dropped], np.int32), landmarks=landmarks, present=present, eyes=eyes)
    return frames, data


_cache = {}


def _scene_and_specification(mi, max_items):
    if max_items not in _cache:
        frames, data = _scene(mi, max_items)
        if max_items == 12:
            data["present"][3] = 0            # a used item that is not drawn (the second face of frame 2)
        _cache[max_items] = (frames, data, specification(frames, data, STYLE))
        for v in list(data.values()) + [frames, _cache[max_items][2]]:
            v.setflags(write=False)
    return _cache[max_items]


def _to_device(data):
    import torch
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in data.items() if k in KEYS}


def _render(mi, frames, data, st, device, channels, stride=None, out_stride=None, fill=0x5A, guard=64, **kw):
    """-> (out as numpy, skipped as numpy, the whole output buffer with its padding and guard)"""
    B, H, W = frames.shape[:3]
    stride = 3 * W if stride is None else stride
    out_stride = channels * W if out_stride is None else out_stride
    fbase, fview = _padded(B, H, W, 3, stride, 0xA5, 64, device)
    obase, oview = _padded(B, H, W, channels, out_stride, fill, guard, device)
    if device:
        import torch
        fview.copy_(torch.from_numpy(np.array(frames)).cuda())
        data = _to_device(data)
    else:
        fview[...] = frames
    out, skipped = mi.render_face_items(fview, data, _mi_style(mi, st), out=oview, out_channels=channels, **kw)
    if device:
        torch.cuda.synchronize()
    assert _untouched(obase, B, H, W, channels, out_stride, fill), "bytes outside the pixels of `out` were written"
    assert _untouched(fbase, B, H, W, 3, stride, 0xA5)
    np.testing.assert_array_equal(_to_numpy(fview), frames)
    return _to_numpy(out), _to_numpy(skipped)


@pytest.mark.parametrize("max_items", [7, 12])
def test_synthetic_item_lists_equal_the_specification(mi, max_items):
    """max_items 7: a frame without an item, a frame cut by the budget (dropped = 2), several faces in one frame.  max_items 12: three unused
    slots that hold drawable values with present = 1, and a used item with present = 0."""
    frames, data, want = _scene_and_specification(mi, max_items)
    n_items, dropped = (int(v) for v in data["counts"])
    assert (n_items, dropped) == ((7, 2) if max_items == 7 else (9, 0))
    assert list(data["item_frame"][:7]) == [0, 0, 2, 2, 2, 3, 4] and (data["item_frame"][n_items:] == -1).all()
    results = {}
    for device in (False, True):
        for channels, out_stride in ((4, 4 * WIDTH + 3), (3, 3 * WIDTH + 7)):
            out, skipped = _render(mi, frames, data, STYLE, device, channels, stride=3 * WIDTH + 5, out_stride=out_stride)
            for b in range(BATCH):
                np.testing.assert_array_equal(out[b], want[b][..., :channels], err_msg="frame %d, device %s, %d channels" % (b, device, channels))
            assert not skipped.any(), skipped      # (the oracle met no empty rectangle either: it raises on one)
            results[device, channels] = out
    for channels in (4, 3):
        np.testing.assert_array_equal(results[False, channels], results[True, channels])
    # the scene shows what it is meant to show: every group's colour is on the pictures, and frame 1 (no face, no item) is the input
    from oracle import render
    for k in ("bounds", "keypoints", "mesh_points", "mesh_lines", "eye_points", "eye_lines", "iris_oval", "iris_points"):
        assert render.colour_mask(want, STYLE[k]).any(), k
    np.testing.assert_array_equal(want[1][..., :3], frames[1])


def test_one_empty_oval_is_not_drawn_and_is_counted(mi):
    from oracle import render
    frames, data, _ = _scene_and_specification(mi, 7)
    data = {k: np.array(v) for k, v in data.items()}
    data["eyes"][1, 0, 71:76] = data["eyes"][1, 0, 71]          # slot 1 (frame 0), left eye: five equal iris points, radius 0
    with pytest.raises(ValueError):                             # the oracle's verdict on that oval: imageproc panics
        render.render_to_image(frame_annotations(render, 0, (WIDTH, HEIGHT), data, STYLE), frames[0])
    want = specification(frames, data, STYLE, without_ovals={(1, 0)})
    for device in (False, True):
        out, skipped = _render(mi, frames, data, STYLE, device, 4, stride=3 * WIDTH + 5, out_stride=4 * WIDTH + 3)
        np.testing.assert_array_equal(out, want)
        assert list(skipped) == [1, 0, 0, 0, 0]


def test_without_iris_groups_it_equals_render_faces(mi):
    """max_faces = 1, max_items = batch: the per-frame arrays of mi_render_faces, compacted into items, give mi_render_faces' bytes."""
    import torch
    rs = np.random.RandomState(21)
    B, W, H = 6, 97, 61
    counts = np.array([1, 0, 1, 1, 0, 1], np.int32)
    frames = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    faces = rs.uniform(0.1, 0.7, (B, 17)).astype(np.float32)
    faces[:, 2:4] = faces[:, 0:2] + 0.2
    landmarks = rs.uniform(0.05, 0.95, (B, 468, 3)).astype(np.float32)
    eyes = rs.uniform(0.05, 0.95, (B, 2, 76, 3)).astype(np.float32)
    present = np.array([1, 0, 1, 0, 0, 1], np.int32)            # frame 3: a face whose mesh flag did not pass
    item_frame, item_face, n_items, dropped = mi.face_items_layout(counts, 1, B)
    assert n_items == 4 and dropped == 0
    src = item_frame[:n_items]
    items = dict(faces=faces.reshape(B, 1, 17), face_counts=counts, item_frame=item_frame, counts=np.array([n_items, dropped], np.int32),
                 landmarks=np.zeros_like(landmarks), present=np.zeros_like(present), eyes=np.zeros_like(eyes))
    items["landmarks"][:n_items], items["present"][:n_items], items["eyes"][:n_items] = landmarks[src], present[src], eyes[src]
    st = dict(STYLE, iris_oval=None, iris_points=None)
    style = _mi_style(mi, st)
    dev = lambda x: torch.from_numpy(x).cuda()
    for channels in (4, 3):
        want, want_skipped = mi.render_faces(dev(frames), dev(faces), dev(counts), dev(landmarks), dev(present), dev(eyes), style.base, out_channels=channels)
        got, skipped = mi.render_face_items(dev(frames), _to_device(items), style, out_channels=channels)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_to_numpy(got), _to_numpy(want))
        np.testing.assert_array_equal(_to_numpy(skipped), _to_numpy(want_skipped))
        assert (_to_numpy(got)[0, ..., :3] != frames[0]).any()


def test_end_to_end_from_run_faces_on_a_caller_stream(mi, man_image):
    import torch
    from oracle import render
    frames = canvases(man_image)
    dev = torch.from_numpy(frames).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    pipe = mi.Pipeline(mi.FaceDetectionModel.BackCamera)
    try:
        res = pipe.run_faces(dev, max_faces=4, max_items=16, stream=stream.cuda_stream)
        out, skipped = mi.render_face_items(dev, res, _mi_style(mi, STYLE), stream=stream.cuda_stream)     # the dict goes straight in
        stream.synchronize()
    finally:
        pipe.close()
    out, skipped = _to_numpy(out), _to_numpy(skipped)
    data = {k: _to_numpy(res[k]) for k in KEYS}
    assert int(data["counts"][0]) >= 8 and data["present"].sum() >= 8
    want = specification(frames, data, STYLE)
    for b in range(len(frames)):
        np.testing.assert_array_equal(out[b], want[b], err_msg="frame %d" % b)
    assert not skipped.any()
    rgba = np.concatenate([frames, np.full(frames.shape[:3] + (1,), 255, np.uint8)], axis=3)
    np.testing.assert_array_equal(out[4], rgba[4])              # black
    np.testing.assert_array_equal(out[5], rgba[5])              # noise
    mesh = render.colour_mask(out[0], STYLE["mesh_lines"])
    H, W = mesh.shape
    for quadrant in (mesh[:H // 2, :W // 2], mesh[:H // 2, W // 2:], mesh[H // 2:, :W // 2], mesh[H // 2:, W // 2:]):
        assert quadrant.any()
    assert render.colour_mask(out[0], STYLE["iris_oval"]).any() and render.colour_mask(out[0], STYLE["iris_points"]).any()


def test_in_place_rgb_with_guard_bytes_and_a_frame_alone(mi):
    import torch
    frames, data, want = _scene_and_specification(mi, 7)
    stride = 3 * WIDTH + 5
    base, view = _padded(BATCH, HEIGHT, WIDTH, 3, stride, 0xC3, 4096, True)
    view.copy_(torch.from_numpy(np.array(frames)).cuda())
    on_device = _to_device(data)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    out, skipped = mi.render_face_items(view, on_device, _mi_style(mi, STYLE), out=view, out_channels=3, stream=stream.cuda_stream)
    stream.synchronize()
    assert out is view
    np.testing.assert_array_equal(_to_numpy(view), want[..., :3])
    assert _untouched(base, BATCH, HEIGHT, WIDTH, 3, stride, 0xC3), "stride padding or the guard region behind the last frame was written"
    assert not _to_numpy(skipped).any()
    # a frame alone, with its own items and item_frame rebased to 0
    for b in range(BATCH):
        slots = np.nonzero(data["item_frame"][:int(data["counts"][0])] == b)[0]
        n = len(slots)
        alone = dict(faces=data["faces"][b:b + 1], face_counts=data["face_counts"][b:b + 1], item_frame=np.zeros((max(n, 1),), np.int32),
                     counts=np.array([n, 0], np.int32), landmarks=np.zeros((max(n, 1), 468, 3), np.float32), present=np.ones((max(n, 1),), np.int32),
                     eyes=np.zeros((max(n, 1), 2, 76, 3), np.float32))
        alone["landmarks"][:n], alone["eyes"][:n] = data["landmarks"][slots], data["eyes"][slots]
        got, _ = mi.render_face_items(np.array(frames[b:b + 1]), alone, _mi_style(mi, STYLE), out_channels=4)
        np.testing.assert_array_equal(got[0], want[b], err_msg="frame %d alone" % b)


def _halving_search(item_frame, used, b):
    """the lower bound include/mi_face.h names: the first slot of item_frame[0, used) whose frame is not below b, by halving"""
    lo, hi = 0, used
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if item_frame[mid] < b:
            lo = mid + 1
        else:
            hi = mid
    return lo


def test_lists_out_of_contract_are_handled_by_the_clamp(mi):
    """Ordinary inputs: an n_items[0] beyond max_items or below zero is clamped, an item_frame out of order draws a subset of each frame's items
    (the slots of the frame's halving-search range that name the frame).  Nothing is read or written outside the arrays."""
    frames, data, want = _scene_and_specification(mi, 7)
    detections_only = specification(frames, dict(data, item_frame=None), STYLE)
    for n, expect in ((7 + 100, want), (-5, detections_only)):
        changed = dict(data, counts=np.array([n, 0], np.int32))
        out, skipped = _render(mi, frames, changed, STYLE, True, 4, out_stride=4 * WIDTH + 3, guard=4096)
        np.testing.assert_array_equal(out, expect, err_msg="n_items[0] = %d" % n)
        assert not skipped.any()
    unsorted = dict(data, item_frame=np.array([0, 0, 3, 2, 2, 2, 4], np.int32))        # slots 2 and 5 swapped their frames
    slots = {}
    for b in range(BATCH):
        lo, hi = _halving_search(unsorted["item_frame"], 7, b), _halving_search(unsorted["item_frame"], 7, b + 1)
        slots[b] = [j for j in range(lo, hi) if unsorted["item_frame"][j] == b]
    assert slots[0] == [0, 1] and slots[1] == [] and slots[4] == [6]      # the runs the disorder does not touch are whole
    from oracle import render
    expect = np.stack([render.render_to_image(frame_annotations(render, b, (WIDTH, HEIGHT), unsorted, STYLE, slots=slots[b]), frames[b])
                       for b in range(BATCH)])
    for b in (0, 1, 4):
        np.testing.assert_array_equal(expect[b], want[b])
    out, skipped = _render(mi, frames, unsorted, STYLE, True, 4, out_stride=4 * WIDTH + 3, guard=4096)
    np.testing.assert_array_equal(out, expect)
    assert not skipped.any()
