"""The GPU renderer (mi_render_annotations / mi_render_faces, csrc/render_kernels.hip) against the executable specification
oracle/render.py (render.rs:262-479 restated) and against the reference's own renderings of man.jpg (tests/golden/*.png).

oracle.render.render_to_image knows the three annotation kinds the reference's callers build (points, lines, hollow rectangles), takes
normalised positions only and starts from an RGB picture.  Two things follow for the whole-image comparison:
  * absolute positions are generated as v = n * size in f64 from a normalised n: the product gets v with normalized = 0, the oracle gets n
    and forms the same v itself (render.rs:368-406), so both draw from identical doubles;
  * the annotation list WITHOUT its filled rectangles is compared with one render_to_image call per frame; the FULL list (all four kinds) is
    compared with a canvas composed in list order from the oracle's coverage of each annotation (render_to_image of that annotation alone
    with a sentinel colour; oracle.render._draw_filled_rect with the casts of render.rs:463-465 for the filled kind).
Items the ABI does not draw (include/mi_face.h: rectangles of size zero — the oracle raises ValueError as imageproc panics — and lines or
hollow rectangles beyond 2^20 px) are taken out of the oracle's list and counted; `skipped` must equal that count exactly.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LIMIT = 1 << 20
KINDS = {0: "points", 1: "lines", 2: "rects", 3: "filled"}


# ------------------------------------------------------------------------------------------------------------ reference pins
@pytest.fixture(scope="module")
def man_on_device(mi, man_image):
    """lib.rs:24-40 through mi_pipeline_run (BackCamera), frames and results left in device memory."""
    import torch
    frames = torch.from_numpy(np.array(man_image)).cuda().unsqueeze(0).contiguous()
    pipe = mi.Pipeline(mi.FaceDetectionModel.BackCamera)
    res = pipe.run(frames)
    torch.cuda.synchronize()
    yield frames, res
    pipe.close()


def _ref_mask(png, colour):
    from PIL import Image
    from oracle import render
    return render.colour_mask(np.asarray(Image.open(os.path.join(GOLDEN, png)).convert("RGBA")), colour)


def _check_pin(mi, man_image, out, skipped, png, colour, pixels):
    from oracle import render
    out = out.cpu().numpy()[0]
    ours = render.colour_mask(out, colour)
    ref = _ref_mask(png, colour)
    assert int(ref.sum()) == pixels
    print("%s: %d annotation pixels, %d mismatching" % (png, int(ours.sum()), int((ours ^ ref).sum())))
    assert int((ours ^ ref).sum()) == 0
    assert (out[ours] == np.array(colour, np.uint8)).all()
    np.testing.assert_array_equal(out[~ours][:, :3], man_image[~ours])      # everything else is the input picture ...
    assert (out[~ours][:, 3] == 255).all()                                   # ... with alpha 255 (to_rgba8)
    assert int(skipped.cpu().numpy()[0]) == 0


def test_bbox_pin_from_device_results(mi, man_on_device, man_image):
    from oracle import render
    frames, res = man_on_device
    style = mi.RenderStyle(bounds_color=mi.Colors.GREEN, keypoint_color=None, line_width=4, point_width=2)      # lib.rs:43-51
    out, skipped = mi.render_faces(frames, faces=res["faces"], face_counts=res["face_counts"], style=style, out_channels=4)
    _check_pin(mi, man_image, out, skipped, "man_bbox.png", render.GREEN, 552)


def test_mesh_pin_from_device_results(mi, man_on_device, man_image):
    from oracle import render
    frames, res = man_on_device
    style = mi.RenderStyle(mesh=True, mesh_landmark_color=mi.Colors.RED, mesh_connection_color=mi.Colors.RED, mesh_thickness=2.0)   # lib.rs:61-63
    out, skipped = mi.render_faces(frames, landmarks=res["landmarks"], present=res["present"], style=style, out_channels=4)
    _check_pin(mi, man_image, out, skipped, "man_landmark.png", render.RED, 2414)


def test_eye_pin_from_device_results(mi, man_on_device, man_image):
    from oracle import render
    frames, res = man_on_device
    style = mi.RenderStyle(eyes=True, eye_landmark_color=mi.Colors.RED, eye_connection_color=mi.Colors.RED, eye_thickness=2.0)      # lib.rs:66-83
    out, skipped = mi.render_faces(frames, eyes=res["eyes"], present=res["present"], style=style, out_channels=4)
    _check_pin(mi, man_image, out, skipped, "man_iris.png", render.RED, 150)


# ------------------------------------------------------------------------------------------------------------ whole-image equality
def _scene(width, height, batch, seed):
    """-> (annotation specs [(kind, first, count, thickness, rgba, normalized)], norm [B, n] f64: the normalised form of every coordinate)."""
    rs = np.random.RandomState(seed)
    c0, c1, c2, c3 = (255, 0, 0, 255), (0, 255, 0, 128), (0, 0, 255, 255), (255, 255, 0, 7)
    layout = [(3, 3, 1.0, c0, 1), (1, 10, 3.0, c1, 1), (0, 8, 5.0, c2, 0), (2, 4, 4.0, c0, 1), (1, 9, 1.0, c2, 0), (0, 8, 1.0, c1, 1),
              (3, 2, 0.0, c3, 0), (0, 3, 9.7, c0, 1), (0, 2, 40.0, c3, 0), (2, 4, 2.0, c1, 0), (1, 3, 2.0, c3, 1)]
    specs, first = [], 0
    for kind, count, thick, col, normalized in layout:
        specs.append((kind, first, count, thick, col, normalized))
        first += count * (2 if kind == 0 else 4)
    norm = rs.uniform(-0.15, 1.15, (batch, first))
    size = np.array([width, height], np.float64)
    at = lambda a, i: specs[a][1] + i * (2 if specs[a][0] == 0 else 4)
    px = lambda x, y: (np.array([x, y], np.float64) / size)        # normalised form of a position given in pixels
    for b in range(batch):
        for a, (kind, _f, count, _t, _c, _n) in enumerate(specs):   # rectangles: right/bottom mostly beyond left/top, so that most are drawn
            if kind >= 2:
                for i in range(count):
                    o = at(a, i)
                    norm[b, o + 2:o + 4] = norm[b, o:o + 2] + rs.uniform(0.06, 0.6, 2)
        # points, thickness 5 (half 2): 0, just below half (the u32 wrap), negative, beyond the canvas, NaN, beyond u32 / i32
        o = at(2, 0)
        norm[b, o:o + 12] = np.concatenate([px(0.0, 0.0), px(1.7, height - 0.5), px(-3.0, 5.2), px(width + 3.0, 2.0), px(np.nan, 4.0), px(5e9, 3e9)])
        o = at(5, 0)
        norm[b, o:o + 8] = np.concatenate([px(0.4, 0.9), px(width - 0.5, height - 0.5), px(-1e12, np.nan), px(1.5, 1e300)])
        # lines: steep, shallow, single pixel, reversed, a NaN end point
        o = at(4, 0)
        norm[b, o:o + 20] = np.concatenate([px(3.2, 1.0), px(5.9, height - 2.0), px(1.0, 2.5), px(width - 2.0, 5.5), px(4.4, 4.4), px(4.6, 4.9),
                                            px(width - 1.0, height - 1.0), px(0.0, 0.0), px(np.nan, 3.0), px(width / 2.0, np.nan)])
    # zero-size rectangles: a filled one (frame 1), a hollow one (frame 2), both again in frame 3 (one axis only); a hollow one of width 1
    for b, a, i, axes in ((1, 0, 2, (0, 1)), (2, 3, 1, (0, 1)), (3, 0, 0, (0,)), (3, 9, 2, (1,)), (3, 6, 1, (0,))):
        o = at(a, i)
        for ax in axes:
            norm[b, o + 2 + ax] = norm[b, o + ax]
    o = at(9, 0)
    norm[4, o:o + 4] = np.concatenate([px(3.2, 2.0), px(4.6, height + 9.0)])
    # far lines through the canvas, end points around +-100 000 px (frames 5 and 6), in the absolute and in the normalised line annotation
    centre = np.array([width / 2.0, height / 2.0])
    for b, a, i, d in ((5, 4, 5, (1.0, 0.37)), (5, 4, 6, (-0.81, 1.0)), (6, 4, 5, (1.0, -0.93)), (6, 10, 0, (0.2, -1.0)), (5, 10, 1, (-1.0, -0.011))):
        o = at(a, i)
        p, q = centre - 100000.0 * np.array(d) + rs.uniform(-9, 9, 2), centre + 100000.0 * np.array(d) + rs.uniform(-9, 9, 2)
        norm[b, o:o + 4] = np.concatenate([px(*p), px(*q)])
    # beyond 2^20: a line end point (frame 7), an edge of a hollow rectangle (frame 6); a filled rectangle of that size IS drawn (frame 7)
    o = at(4, 7)
    norm[7, o:o + 4] = np.concatenate([px(2.0, 2.0), px(LIMIT + 2.0, 7.0)])
    o = at(9, 1)
    norm[6, o:o + 4] = np.concatenate([px(-5.0, 3.0), px(LIMIT + 40.0, 9.0)])
    o = at(6, 0)
    norm[7, o:o + 4] = np.concatenate([px(width / 2.0, -3e6), px(4e6, height / 3.0)])
    return specs, norm


def _coords(specs, norm, width, height):
    """what the product reads: normalised annotations keep n, absolute ones get v = n * size (the multiplication render_to_image does)"""
    coords = norm.copy()
    scale = np.array([width, height], np.float64)
    for kind, first, count, _t, _c, normalized in specs:
        if not normalized:
            n = count * (2 if kind == 0 else 4)
            coords[:, first:first + n] = (norm[:, first:first + n].reshape(norm.shape[0], -1, 2) * scale).reshape(norm.shape[0], n)
    return coords


def _oracle_items(render, spec, row, width, height):
    """-> (items the ABI draws, number it does not draw) of one annotation of one frame; items in the oracle's normalised form"""
    kind, first, count, _t, _c, _n = spec
    per = 2 if kind == 0 else 4
    items = [tuple(float(v) for v in row[first + per * i:first + per * (i + 1)]) for i in range(count)]
    if kind == 0:
        return items, 0
    sx, sy = float(width), float(height)
    kept, skipped = [], 0
    for it in items:
        if kind == 1:
            far = any(abs(render._as_i32(v)) > LIMIT for v in (it[0] * sx, it[1] * sy, it[2] * sx, it[3] * sy))
        else:
            left, top = render._as_i32(it[0] * sx), render._as_i32(it[1] * sy)
            w, h = render._as_u32(it[2] * sx - it[0] * sx), render._as_u32(it[3] * sy - it[1] * sy)
            try:   # the oracle's own verdict on an empty rectangle
                render._draw_filled_rect(np.zeros((1, 1, 4), np.uint8), left, top, w, h, np.zeros(4, np.uint8))
                far = kind == 2 and any(abs(v) > LIMIT for v in (left, top, left + w - 1, top + h - 1))
            except ValueError:
                far = True
        if far:
            skipped += 1
        else:
            kept.append(it)
    return kept, skipped


def _oracle_frame(render, specs, row, frame_rgb, with_filled):
    """-> (expected RGBA of the full list or None, expected RGBA of the list without filled rectangles, skipped of each)"""
    height, width = frame_rgb.shape[:2]
    sx, sy = float(width), float(height)
    canvas = render.render_to_image([], frame_rgb)
    plain, skipped_full, skipped_plain = [], 0, 0
    for spec in specs:
        kind, _f, _n, thickness, colour, _norm = spec
        items, skipped = _oracle_items(render, spec, row, width, height)
        skipped_full += skipped
        if kind == 3:
            for it in items:
                render._draw_filled_rect(canvas, render._as_i32(it[0] * sx), render._as_i32(it[1] * sy), render._as_u32(it[2] * sx - it[0] * sx),
                                         render._as_u32(it[3] * sy - it[1] * sy), np.array(colour, np.uint8))
            continue
        skipped_plain += skipped
        plain.append((KINDS[kind], items, thickness, colour))
        if with_filled:
            covered = render.render_to_image([(KINDS[kind], items, thickness, (1, 2, 3, 0))], np.zeros_like(frame_rgb))[..., 3] == 0
            canvas[covered] = np.array(colour, np.uint8)
    return (canvas if with_filled else None), render.render_to_image(plain, frame_rgb), skipped_full, skipped_plain


_expected = {}


def _scene_and_expectation(width, height):
    from oracle import render
    if (width, height) not in _expected:
        batch = 8
        specs, norm = _scene(width, height, batch, seed=width * 1000 + height)
        frames = np.random.RandomState(7).randint(0, 256, (batch, height, width, 3)).astype(np.uint8)
        frames[frames == 255] = 254      # keep the pictures clear of the sentinel / colour values by a hair: not needed, only tidy
        _expected[(width, height)] = (specs, norm, frames, [_oracle_frame(render, specs, norm[b], frames[b], True) for b in range(batch)])
    return _expected[(width, height)]


def _annotations(mi, specs):
    return [mi.Annotation(kind, first, count, thickness, mi.Color(*colour), normalized) for kind, first, count, thickness, colour, normalized in specs]


def _padded(batch, height, width, channels, stride, fill, guard, device):
    """a [batch, height, width, channels] view of rows `stride` bytes apart inside a buffer filled with `fill`, `guard` bytes behind the last frame"""
    n = batch * height * stride
    if device:
        import torch
        base = torch.full((n + guard,), fill, dtype=torch.uint8, device="cuda")
        return base, torch.as_strided(base, (batch, height, width, channels), (height * stride, stride, channels, 1))
    base = np.full((n + guard,), fill, np.uint8)
    return base, np.lib.stride_tricks.as_strided(base, (batch, height, width, channels), (height * stride, stride, channels, 1))


def _to_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _untouched(base, batch, height, width, channels, stride, fill):
    """every byte of the buffer outside the pixels still holds `fill`"""
    b = _to_numpy(base)
    rows = b[:batch * height * stride].reshape(batch * height, stride)
    return bool((rows[:, width * channels:] == fill).all() and (b[batch * height * stride:] == fill).all())


@pytest.mark.parametrize("width,height,stride,out_stride,device", [(37, 23, 128, 160, True), (37, 23, 113, 151, True), (37, 23, 128, 160, False),
                                                                   (540, 360, 1620, 2160, True)])
def test_render_annotations_equals_specification(mi, width, height, stride, out_stride, device):
    specs, norm, frames, expected = _scene_and_expectation(width, height)
    batch = len(frames)
    coords = _coords(specs, norm, width, height)
    fbase, fview = _padded(batch, height, width, 3, stride, 0xA5, 64, device)
    if device:
        import torch
        fview.copy_(torch.from_numpy(frames).cuda())
        coords = torch.from_numpy(coords).cuda()
    else:
        fview[...] = frames
    assert len(specs) >= 6 and {s[0] for s in specs} == {0, 1, 2, 3} and len({s[4] for s in specs}) >= 3
    for with_filled in (True, False):
        use = [s for s in specs if with_filled or s[0] != 3]
        obase, oview = _padded(batch, height, width, 4, out_stride, 0x5A, 64, device)
        out, skipped = mi.render_annotations(fview, _annotations(mi, use), coords, out=oview, out_channels=4)
        if device:
            torch.cuda.synchronize()
        out, skipped = _to_numpy(out), _to_numpy(skipped)
        for b in range(batch):
            full, plain, skipped_full, skipped_plain = expected[b]
            np.testing.assert_array_equal(out[b], full if with_filled else plain, err_msg="frame %d, filled rectangles %s" % (b, with_filled))
            assert int(skipped[b]) == (skipped_full if with_filled else skipped_plain), (b, with_filled)
        assert _untouched(obase, batch, height, width, 4, out_stride, 0x5A), "bytes outside the RGBA pixels were written"
        assert _untouched(fbase, batch, height, width, 3, stride, 0xA5)
        np.testing.assert_array_equal(_to_numpy(fview), frames)
    # the deviations were all met: rectangles of size zero, a line and a hollow rectangle beyond 2^20 px
    assert [e[2] for e in expected] == [0, 1, 1, 3, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------------------ memory contract
def _simple_scene(mi, batch, width, height, seed):
    rs = np.random.RandomState(seed)
    layout = [(2, 3, 2.0, (0, 255, 0, 255)), (1, 12, 1.0, (255, 0, 0, 255)), (0, 20, 4.0, (0, 0, 255, 255)), (1, 5, 1.0, (255, 0, 255, 255))]
    specs, first = [], 0
    for kind, count, thick, col in layout:
        specs.append((kind, first, count, thick, col, 1))
        first += count * (2 if kind == 0 else 4)
    norm = rs.uniform(-0.1, 1.1, (batch, first))
    norm[:, 2:4] = norm[:, 0:2] + 0.3
    norm[:, 6:8] = norm[:, 4:6] + 0.2
    norm[:, 10:12] = norm[:, 8:10] + 0.5
    frames = rs.randint(0, 255, (batch, height, width, 3)).astype(np.uint8)
    return specs, norm, frames


def test_in_place_rgb_on_a_device_buffer_with_a_caller_stream(mi):
    import torch
    from oracle import render
    batch, width, height, stride = 5, 64, 48, 3 * 64 + 8
    specs, norm, frames = _simple_scene(mi, batch, width, height, 11)
    base, view = _padded(batch, height, width, 3, stride, 0xC3, 4096, True)
    view.copy_(torch.from_numpy(frames).cuda())
    coords = torch.from_numpy(norm).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    out, skipped = mi.render_annotations(view, _annotations(mi, specs), coords, out=view, out_channels=3, stream=stream.cuda_stream)
    stream.synchronize()
    assert out is view
    got = _to_numpy(view)
    for b in range(batch):
        anns = [(KINDS[k], _oracle_items(render, (k, f, n, t, c, 1), norm[b], width, height)[0], t, c) for k, f, n, t, c, _ in specs]
        np.testing.assert_array_equal(got[b], render.render_to_image(anns, frames[b])[..., :3], err_msg="frame %d" % b)
    assert _untouched(base, batch, height, width, 3, stride, 0xC3), "stride padding or the guard region behind the last frame was written"
    assert (got != frames).any() and not _to_numpy(skipped).any()


def test_a_frame_alone_equals_that_frame_of_the_batch_and_host_equals_device(mi):
    import torch
    batch, width, height = 6, 96, 50
    specs, norm, frames = _simple_scene(mi, batch, width, height, 12)
    anns = _annotations(mi, specs)
    for channels in (4, 3):
        host, _ = mi.render_annotations(frames, anns, norm, out_channels=channels)
        dev, _ = mi.render_annotations(torch.from_numpy(frames).cuda(), anns, torch.from_numpy(norm).cuda(), out_channels=channels)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host, _to_numpy(dev))
        assert (host[..., :3] != frames).any()
        for i in range(batch):
            alone, _ = mi.render_annotations(frames[i:i + 1], anns, norm[i:i + 1], out_channels=channels)
            np.testing.assert_array_equal(alone[0], host[i], err_msg="frame %d" % i)


def test_frames_without_a_face_come_back_unchanged(mi):
    import torch
    rs = np.random.RandomState(13)
    batch, width, height = 4, 80, 60
    frames = rs.randint(0, 256, (batch, height, width, 3)).astype(np.uint8)
    faces = rs.uniform(0.2, 0.8, (batch, 17)).astype(np.float32)
    faces[:, 2:4] = faces[:, 0:2] + 0.1
    counts = np.array([1, 0, -3, 1], np.int32)
    landmarks = rs.uniform(0.1, 0.9, (batch, 468, 3)).astype(np.float32)
    eyes = rs.uniform(0.1, 0.9, (batch, 2, 76, 3)).astype(np.float32)
    present = np.array([1, 0, 0, 0], np.int32)
    style = mi.RenderStyle(bounds_color=mi.Colors.GREEN, keypoint_color=mi.Colors.BLUE, line_width=2, point_width=3, mesh=True, mesh_thickness=2.0,
                           eyes=True, eye_landmark_color=mi.Colors.PINK, eye_thickness=2.0)
    host, skipped = mi.render_faces(frames, faces, counts, landmarks, present, eyes, style, out_channels=4)
    rgba = np.concatenate([frames, np.full((batch, height, width, 1), 255, np.uint8)], axis=3)
    for b in (1, 2):                                   # no face and no mesh: to_rgba8 of the input, nothing else
        np.testing.assert_array_equal(host[b], rgba[b])
    assert (host[0] != rgba[0]).any() and (host[3] != rgba[3]).any() and not skipped.any()
    # frame 3: a face but present = 0 -> only the detection's annotations; frame 0: all three groups, equal to the specification
    from oracle import render
    for b in (0, 3):
        ann = render.detections_to_render_data(faces[b:b + 1], (0, 255, 0, 255), (0, 0, 255, 255), 2, 3)
        if present[b]:
            ann += render.face_landmarks_to_render_data(landmarks[b], (255, 0, 0, 255), (255, 0, 0, 255), 2.0)
            for e in range(2):
                ann += render.eye_landmarks_to_render_data(eyes[b, e], (255, 0, 255, 255), (255, 0, 0, 255), 2.0)
        np.testing.assert_array_equal(host[b], render.render_to_image(ann, frames[b]), err_msg="frame %d" % b)
    dev, _ = mi.render_faces(*[torch.from_numpy(x).cuda() for x in (frames, faces, counts, landmarks, present, eyes)], style, out_channels=4)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_to_numpy(dev), host)
