"""GPU isolation tests: a kernel must never read memory it did not write first, nor another frame's pixels — even where the value it reads
would be cancelled by a zero weight, a zero mask or a max.  The parity suite feeds finite frames into buffers that hold zeros (fresh pages) or
last run's finite activations, so such reads pass there unnoticed.  Here:

  a. engine option "test_poison" fills the arena, the small-batch scratch, the output buffers and the unused tail of the input stage with
     NaN (0xFF bytes) or 3.39e38 (0x7F bytes: survives max / ReLU) before every run: the results must not move a bit;
  b. non-finite frames (NaN, +-Inf, 3.4e38 pixels) in a batch must not move a bit of any other frame's results;
  c. a device input that is a view into a larger buffer is read only inside its window;
  d. the SSD post-processing kernel on adversarial raw outputs (non-finite scores and features, the full N-key sort, an N-candidate merge,
     letterbox limits) against the oracle;
  e. the detector end to end with non-finite frames in the batch.

The poisoned frames' own network outputs are not asserted (NaN through ReLU is not defined alike by every kernel form: v_max_f32 drops a NaN).
"""
import numpy as np
import pytest

from conftest import MODEL_FILES, model_path, seeded_input
from test_gpu_parity import _raw_close

pytestmark = pytest.mark.gpu

DETECTORS = ["back", "front", "short", "full", "sparse"]
ORC_KIND = {"back": "FD_BACK", "front": "FD_FRONT", "short": "FD_SHORT", "full": "FD_FULL", "sparse": "FD_FULL_SPARSE"}
FD_KIND = {"back": "BackCamera", "front": "FrontCamera", "short": "Short", "full": "Full", "sparse": "FullSparse"}


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


def _frames(name, m, batch, seed):
    x = seeded_input(name, batch, seed, m.input_dims[1:3])
    lo, hi = (-1.0, 1.0) if name in DETECTORS else (0.0, 1.0)
    x[:: 7, : x.shape[1] // 4] = lo          # flat rows at the top of some frames (zero-ish halo and real values must agree)
    x[3:: 11, :, -5:] = hi                    # saturated right edge of others
    return x


# ------------------------------------------------------------------------------------------------ a. poisoned scratch
ALL = list(MODEL_FILES)
PLANS = [  # (id, options, models it applies to, batch sizes)
    ("default", {}, ALL, (1, 5, 33, 97, 130)),
    ("fuse0", {"fuse": 0}, ALL, (1, 5, 33)),
    ("fuse2", {"fuse": 2}, ALL, (1, 5, 33, 97)),
    ("fuse3", {"fuse": 3}, ALL, (1, 5, 33, 97)),
    ("fuse4", {"fuse": 4}, ALL, (1, 5, 33, 97, 130)),
    ("strip0", {"strip": 0}, ALL, (1, 5, 33, 97)),
    ("pipe_rows1", {"pipe_rows": 1}, DETECTORS + ["landmark"], (5, 33, 97, 130)),
    ("pipe_rows2", {"pipe_rows": 2}, DETECTORS + ["landmark"], (5, 33, 97, 130)),
    ("pipe_rows4", {"pipe_rows": 4}, DETECTORS + ["landmark"], (5, 33, 97, 130)),
    ("chunk", {"chunk": 40}, ALL, (97, 130)),                 # chunks of 40, 40, 17 / 40, 40, 40, 10
    ("lanes2", {"lanes": 2}, ALL, (5, 33, 97)),
    ("graph0", {"graph": 0}, ALL, (1, 5, 33, 97)),
    ("band2", {"band": 2}, ALL, (1, 2, 3)),
    ("tail0", {"tail": 0}, ["landmark", "iris"], (1, 5, 33, 97)),
    ("tail_g2", {"tail_g": 2}, ["landmark", "iris"], (1, 5, 33, 97)),
    ("tail_g4", {"tail_g": 4}, ["landmark", "iris"], (1, 5, 33, 97, 130)),
    ("unfused_launches", {"stem_mfma": 0, "stem_fuse": 0, "pair_fuse": 0, "mchain": 0}, ALL, (1, 5, 33, 97)),
    ("reuse0", {"reuse": 0}, ALL, (1, 33)),
    ("heads4", {"heads": 4}, ALL, (1, 33, 97)),     # the output heads spread over four side streams (the default is one)
    ("fork0", {"fork": 0}, ALL, (1, 33)),           # the output heads on the trunk's stream
    ("small_chain0", {"small_chain": 0}, DETECTORS + ["landmark"], (1, 5)),
]
POISON_CASES = [(n, pid) for pid, _o, names, _b in PLANS for n in names]
_PLAN = {pid: (o, b) for pid, o, _n, b in PLANS}


def _run_poisoned(m, x, band=False):
    """Run once clean, then with NaN, 3.39e38 and NaN again (a warm handle).  Returns the clean outputs; asserts the others equal them bit
    for bit.  On the single-launch plan (band = 2) a run that gave up is repeated on the batched plan: only runs that stayed on it compare."""
    m.set_option("test_poison", 0)
    base = [o.copy() for o in m.run(x)]
    base_ok = not band or m.get_option("band_fail_streak") == 0
    for o in base:
        assert np.isfinite(o).all()
    for p in (1, 2, 1):
        m.set_option("test_poison", p)
        assert m.get_option("test_poison") == p
        outs = m.run(x)
        if band and (not base_ok or m.get_option("band_fail_streak") != 0):
            continue
        for o, b in zip(outs, base):
            assert np.isfinite(o).all(), "poison %d reached the outputs" % p
            np.testing.assert_array_equal(o, b, err_msg="poison pattern %d" % p)
    m.set_option("test_poison", 0)
    return base


@pytest.mark.parametrize("name,plan", POISON_CASES)
def test_poisoned_scratch_gives_identical_results(gpu, oracle, name, plan):
    opts, batches = _PLAN[plan]
    m = gpu.Model(model_path(name))
    assert m.get_option("test_poison") == 0
    for k, v in opts.items():
        m.set_option(k, v)
    x = _frames(name, m, max(batches), 4242)
    for nb in batches:
        base = _run_poisoned(m, x[:nb], band=plan == "band2")
        if plan == "default" and nb == max(batches):   # the baseline itself against the oracle on a sample
            sel = [0, 64, nb - 1]
            for o, r in zip(base, oracle.Model(model_path(name)).run(x[sel], nthreads=3)):
                _raw_close(o[sel], r)
    m.close()


def test_poison_option_and_the_input_stage_tail(gpu):
    """The option reads back (values other than 1 / 2 turn it off), and a host-input call smaller than an earlier one — whose input stage then
    holds poison beyond the call's frames — gives the results of a fresh handle."""
    m = gpu.Model(model_path("front"))
    for v, want in ((1, 1), (2, 2), (3, 0), (-1, 0), (0, 0)):
        m.set_option("test_poison", v)
        assert m.get_option("test_poison") == want
    x = _frames("front", m, 40, 8)
    fresh = gpu.Model(model_path("front"))
    ref = [o.copy() for o in fresh.run(x[:5])]
    fresh.close()
    m.run(x)                                   # stage and outputs sized for 40 frames
    for p in (1, 2):
        m.set_option("test_poison", p)
        for o, r in zip(m.run(x[:5]), ref):
            np.testing.assert_array_equal(o, r)
    m.close()


# ------------------------------------------------------------------------------------------------ b. non-finite frames
def _bad_frame(kind, like, name):
    f = like.copy()
    H, W = f.shape[:2]
    if kind == "nan":
        f[:] = np.nan
    elif kind == "inf":
        f[:] = np.inf
    elif kind == "nan_pixel":
        f[0, 0, :] = np.nan
    elif kind == "neginf_pixel":
        f[H - 1, W - 1, :] = -np.inf
    elif kind == "huge_border":
        f[H - 1, W // 3, :] = 3.4e38
    return f


BAD_KINDS = ["nan", "inf", "nan_pixel", "neginf_pixel", "huge_border"]
FRAME_PLANS = [  # (id, options, models): the chunk edge lies between frames 15 / 16 (40 frames) and 1 / 2 (3 frames)
    ("default", {}, ALL),
    ("chunk", {"chunk": 16}, ALL),
    ("lanes2", {"lanes": 2}, ALL),
    ("small_chain", {"small_chain": 64}, ALL),
    ("band2", {"band": 2}, ALL),
    ("tail_g4", {"tail_g": 4}, ["landmark", "iris"]),   # (tail_g only changes the tail programs of these two)
    ("stem_mfma0", {"stem_mfma": 0}, DETECTORS),       # the detectors' first convolution on stem_conv_kernel (its clamped halo rows) at every batch
]
FRAME_CASES = [(n, pid) for pid, _o, names in FRAME_PLANS for n in names]
# first, last, both frames of a two-frame workgroup (10, 11), either side of the chunk edge (15, 16), inside a tail_g group (21)
POS40 = [0, 10, 11, 15, 16, 21, 39]
OBSERVED = {}


@pytest.mark.parametrize("name,plan", FRAME_CASES)
def test_nonfinite_frames_do_not_reach_other_frames(gpu, name, plan):
    opts = {pid: o for pid, o, _n in FRAME_PLANS}[plan]
    m = gpu.Model(model_path(name))
    for k, v in opts.items():
        m.set_option(k, v)
    for nb, positions in ((40, POS40), (3, [1]), (3, [0, 2])):
        if k_chunk := opts.get("chunk"):
            m.set_option("chunk", k_chunk if nb > 3 else 2)
        x = _frames(name, m, nb, 1000 + nb)
        base = [o.copy() for o in m.run(x)]
        band = plan == "band2"
        base_ok = not band or m.get_option("band_fail_streak") == 0
        keep = [f for f in range(nb) if f not in positions]
        for kind in BAD_KINDS:
            xb = x.copy()
            for p in positions:
                xb[p] = _bad_frame(kind, x[p], name)
            outs = m.run(xb)
            if band and (not base_ok or m.get_option("band_fail_streak") != 0):
                continue
            for o, b in zip(outs, base):
                np.testing.assert_array_equal(o[keep], b[keep], err_msg="%s frames at %s" % (kind, positions))
            # observed only: what the poisoned frames' own outputs look like under this plan
            OBSERVED[(name, plan, nb, kind)] = [(float(np.isfinite(o[positions]).mean()), float(np.isnan(o[positions]).mean()),
                                                 float(np.isinf(o[positions]).mean())) for o in outs]
    print("\nOBSERVED %s %s (40 frames; per output: finite, NaN, Inf fractions of the bad frames' values): %s" % (
        name, plan, {k: OBSERVED.get((name, plan, 40, k)) for k in BAD_KINDS}))
    m.close()


# ------------------------------------------------------------------------------------------------ c. device input window
@pytest.mark.parametrize("plan", ["default", "band2"])
@pytest.mark.parametrize("name", ALL)
def test_device_input_is_read_only_inside_its_window(gpu, name, plan):
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path(name))
    if plan == "band2":
        m.set_option("band", 2)
    for nb in (1, 3, 40):
        x = _frames(name, m, nb, 77 + nb)
        tight = torch.from_numpy(x).cuda()
        ref = [o.cpu().numpy() for o in m.run(tight)]
        ok = plan != "band2" or m.get_option("band_fail_streak") == 0
        before, after = 3, 2
        for fill in (float("nan"), 3.4e38):
            big = torch.full((before + nb + after,) + tuple(x.shape[1:]), fill, dtype=torch.float32, device="cuda")
            big[before: before + nb] = tight
            view = big[before: before + nb]
            assert view.is_contiguous() and view.data_ptr() != big.data_ptr()
            outs = [o.cpu().numpy() for o in m.run(view)]
            if not ok or (plan == "band2" and m.get_option("band_fail_streak") != 0):
                continue
            for o, r in zip(outs, ref):
                np.testing.assert_array_equal(o, r, err_msg="neighbours %r, %d frames" % (fill, nb))
    m.close()


@pytest.mark.parametrize("entry", ["back", "short", "landmark"])
def test_device_u8_frames_are_read_only_inside_their_window(gpu, man_image, entry):
    """The u8 entries (device image_to_tensor + network) on a window of a larger device buffer: neighbours of 0x00 and of 0xFF bytes give the
    same results.  The frames are not the network's size, so the bilinear resize samples up to the frame's last row and column."""
    torch = pytest.importorskip("torch")
    if entry == "landmark":
        h = gpu.FaceLandmark()
        call = lambda fr: h.infer_images(fr)
    else:
        h = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, FD_KIND[entry]))
        call = lambda fr: h.infer_images(fr, cap=16)
    img = np.ascontiguousarray(man_image[:300, :260])
    for nb in (1, 3, 40):
        frames = np.stack([np.roll(img, (5 * k, -3 * k), axis=(0, 1)) for k in range(nb)])
        res = {}
        for fill in (0x00, 0xFF):
            big = torch.full((2 + nb + 3,) + frames.shape[1:], fill, dtype=torch.uint8, device="cuda")
            big[2: 2 + nb] = torch.from_numpy(frames).cuda()
            res[fill] = [t.cpu().numpy() for t in call(big[2: 2 + nb])]
        for a, b in zip(res[0x00], res[0xFF]):
            np.testing.assert_array_equal(a, b, err_msg="%d frames" % nb)
    h.close()


# ------------------------------------------------------------------------------------------------ d. post-processing on adversarial raw outputs
def _layout(anchors, scale, centres, size):
    """raw boxes that decode to boxes of `size` (normalised) at `centres` [N, 2], whatever the anchors."""
    N = anchors.shape[0]
    rb = np.zeros((N, 16), np.float32)
    rb[:, 0:2] = (centres - anchors) * scale
    rb[:, 2:4] = size * scale
    rb[:, 4:16] = (np.tile(centres, 6) - np.tile(anchors, 6)) * scale + np.arange(12, dtype=np.float32) * 0.5
    return rb


def _grid(N):
    g = int(np.ceil(np.sqrt(N)))
    i = np.arange(N)
    return np.stack([(i % g + 0.5) / g, (i // g + 0.5) / g], 1).astype(np.float32), 1.0 / g


def _post_cases(N, anchors, scale, rs):
    grid, step = _grid(N)
    perm = rs.permutation(N)
    distinct = (0.5 + 2.5 * perm / N).astype(np.float32)
    cases = {}
    cases["distinct_disjoint"] = (_layout(anchors, scale, grid, step * 0.3), distinct)
    cases["tied_disjoint"] = (_layout(anchors, scale, grid, step * 0.3), np.full(N, 2.0, np.float32))
    centre = np.full((N, 2), 0.5, np.float32) + (rs.uniform(-0.01, 0.01, (N, 2))).astype(np.float32)
    cases["distinct_overlapping"] = (_layout(anchors, scale, centre, 0.5), distinct)
    cases["tied_overlapping"] = (_layout(anchors, scale, centre, 0.5), np.full(N, 2.0, np.float32))
    # clusters of 8 neighbours (boxes of two grid steps) with scores of every special kind
    rb = _layout(anchors, scale, grid, step * 2.0)
    sc = np.full(N, -10.0, np.float32)
    sc[:: 3] = distinct[:: 3]
    special = [np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-40, 0.0, 80.0, -80.0, 81.0]
    idx = rs.choice(N, 200, replace=False)
    for k, i in enumerate(idx):
        sc[i] = special[k % len(special)]
    cases["special_scores"] = (rb, sc)
    # non-finite box features (dropped) and keypoints (propagated into their cluster)
    rb2 = rb.copy()
    sc2 = distinct.copy()
    for k, i in enumerate(idx[:60]):
        rb2[i, k % 4] = np.nan
    for k, i in enumerate(idx[60:120]):
        rb2[i, 4 + k % 12] = [np.nan, np.inf, -np.inf][k % 3]
    cases["nonfinite_features"] = (rb2, sc2)
    # an infinite-size box scoring highest: output alone, the loop stops there
    rb3 = rb.copy()
    rb3[idx[0], 2] = np.inf
    sc3 = distinct.copy()
    sc3[idx[0]] = 5.0
    cases["infinite_head"] = (rb3, sc3)
    # an infinite-size box in the middle of the order
    rb4 = rb.copy()
    rb4[idx[1], 2:4] = np.inf
    sc4 = distinct.copy()
    sc4[idx[1]] = np.float32(np.sort(distinct)[N // 2]) + np.float32(1e-4)
    cases["infinite_middle"] = (rb4, sc4)
    # zero-width and negative-width boxes (dropped)
    rb5 = rb.copy()
    rb5[idx[:40], 2] = 0.0
    rb5[idx[40:80], 3] = -5.0
    rb5[idx[80:100], 2:4] = -np.inf
    cases["degenerate_sizes"] = (rb5, distinct)
    return cases


def _compare_post(got, cnt, ref, cap, rel=False):
    assert cnt == len(ref), (cnt, len(ref))
    k = min(cap, len(ref))
    g, r = got[:k], ref[:k]
    fin_g, fin_r = np.isfinite(g), np.isfinite(r)
    np.testing.assert_array_equal(fin_g, fin_r)
    np.testing.assert_array_equal(g[~fin_g], r[~fin_r])
    np.testing.assert_allclose(g[:, 16], r[:, 16], rtol=3e-7)
    gf, rf = np.where(fin_g[:, :16], g[:, :16], 0), np.where(fin_r[:, :16], r[:, :16], 0)
    if rel:   # coordinates near 1e36 (and beyond f32 range after the letterbox): relative
        np.testing.assert_allclose(gf, rf, rtol=2e-6, atol=2e-6)
    else:
        np.testing.assert_allclose(gf, rf, rtol=0, atol=2e-6)


POST_KINDS = [("back", "BackCamera"), ("full", "Full"), ("short", "Short")]


@pytest.mark.parametrize("name,kind", POST_KINDS)
def test_postprocess_adversarial_raw_outputs_vs_oracle(gpu, oracle, name, kind):
    fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
    anchors = fd.anchors()
    N = anchors.shape[0]
    scale = float(fd.input_size[1])
    cases = _post_cases(N, anchors, scale, np.random.RandomState(17))
    seen = {}
    for cname, (rb, sc) in cases.items():
        refs = oracle.fd_postprocess(rb, sc, anchors, scale)
        n = len(refs)
        seen[cname] = n
        for cap in sorted({1, max(1, n - 1), max(1, n)}):
            out, counts = fd.postprocess(rb[None], sc[None], None, cap=cap)
            _compare_post(out[0], counts[0], refs, cap)
    assert seen["distinct_disjoint"] == N and seen["tied_disjoint"] == N        # the full M = N sort
    assert seen["distinct_overlapping"] == 1 and seen["tied_overlapping"] == 1  # one merge of N candidates
    assert seen["infinite_head"] == 1
    fd.close()


@pytest.mark.parametrize("name,kind", POST_KINDS)
def test_postprocess_huge_coordinates_and_letterbox_limits(gpu, oracle, name, kind):
    fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
    anchors = fd.anchors()
    N = anchors.shape[0]
    scale = float(fd.input_size[1])
    grid, step = _grid(N)
    rb = _layout(anchors, scale, grid, step * 0.3)
    sc = np.full(N, -10.0, np.float32)
    rs = np.random.RandomState(5)
    idx = rs.choice(N, 64, replace=False)
    sc[idx] = (1.0 + np.arange(64) / 32.0).astype(np.float32)
    rb[idx[:16], 0] = 3e38                 # centres near f32 max (decoded: 3e38 / scale)
    rb[idx[16:32], 1] = -3e38
    rb[idx[32:40], 2] = 3e38               # huge widths
    rb[idx[40:48], 4:16] = 3e38            # huge keypoints
    # "inside": h_scale = 1 - (0 + (1 - 2^-51)) = 2^-51, just above f64 epsilon: coordinates grow by 2^51 (huge ones overflow f32 to Inf)
    pads = {"none": (0.0, 0.0, 0.0, 0.0), "inside": (0.0, 0.0, 1.0 - 2.0 ** -51, 0.0), "vertical": (0.0, 0.25, 0.0, 0.25)}
    for pname, pad in pads.items():
        refs = oracle.fd_postprocess(rb, sc, anchors, scale, pad)
        out, counts = fd.postprocess(rb[None], sc[None], np.array([pad]), cap=N)
        _compare_post(out[0], counts[0], refs, N, rel=True)
    # at the boundary: 1 - (left + right) == f64 epsilon is not > epsilon -> the reference's assert!, MI_ERANGE here
    at = (0.0, 0.0, 1.0 - 2.0 ** -52, 0.0)
    with pytest.raises(RuntimeError):
        oracle.fd_postprocess(rb, sc, anchors, scale, at)
    with pytest.raises(gpu.MiError) as e:
        fd.postprocess(rb[None], sc[None], np.array([at]), cap=8)
    assert e.value.code == -5
    fd.close()


# ------------------------------------------------------------------------------------------------ e. detector end to end with bad frames
@pytest.mark.parametrize("name", ["back", "full"])
def test_detector_with_nonfinite_frames_in_the_batch(gpu, oracle, man_image, name):
    """Face-bearing frames with NaN / Inf frames between them through FaceDetection.infer_tensor: the face frames' detections are bit-equal
    to the same batch with finite frames in those slots; each bad frame's detections are what the oracle's post-processing makes of the raw
    outputs the GPU computed for it (taken from a Model of the same graph at the same batch, which is first shown to stand in for the
    handle's network bit for bit)."""
    fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, FD_KIND[name]))
    m = gpu.Model(model_path(name))
    W, H = fd.input_size
    face, _pad = oracle.image_to_tensor(man_image, None, (W, H), True, (-1., 1.), False)
    faces = [face, np.roll(face, (H // 28, -W // 18), axis=(0, 1)), face[:, ::-1], np.clip(face * 0.9, -1, 1)]
    filler = seeded_input(name, 6, 31, (H, W)) * 0.25
    bad = [np.full_like(face, np.nan), np.full_like(face, np.inf), _bad_frame("nan_pixel", face, name),
           _bad_frame("neginf_pixel", face, name), _bad_frame("huge_border", face, name), np.full_like(face, -np.inf)]
    order = []
    for k in range(4):
        order += [("face", k), ("bad", k)]
    order += [("bad", 4), ("bad", 5)]
    x_clean = np.stack([faces[k] if t == "face" else filler[k] for t, k in order]).astype(np.float32)
    x_bad = np.stack([faces[k] if t == "face" else bad[k] for t, k in order]).astype(np.float32)
    face_pos = [i for i, (t, _k) in enumerate(order) if t == "face"]
    bad_pos = [i for i, (t, _k) in enumerate(order) if t == "bad"]
    cap = 64
    out_c, cnt_c = fd.infer_tensor(x_clean, cap=cap)
    out_b, cnt_b = fd.infer_tensor(x_bad, cap=cap)
    assert sum(cnt_c[face_pos]) >= 4
    np.testing.assert_array_equal(cnt_b[face_pos], cnt_c[face_pos])
    np.testing.assert_array_equal(out_b[face_pos], out_c[face_pos])
    N = fd.num_anchors
    # the stand-in: a Model of the same graph at the same batch, post-processed by the handle, equals infer_tensor bit for bit
    rb_c, rs_c = m.run(x_clean)
    pp_c, pc_c = fd.postprocess(rb_c.reshape(len(order), N, 16), rs_c.reshape(len(order), N), None, cap=cap)
    np.testing.assert_array_equal(pc_c, cnt_c)
    np.testing.assert_array_equal(pp_c, out_c)
    rb_b, rs_b = m.run(x_bad)
    anchors = oracle.ssd_anchors(getattr(oracle, ORC_KIND[name]))
    for f in bad_pos:
        assert 0 <= cnt_b[f] <= N
        ref = oracle.fd_postprocess(rb_b[f].reshape(N, 16), rs_b[f].reshape(N), anchors, float(H))
        _compare_post(out_b[f], cnt_b[f], ref, cap)
    print("\n%s: detections per bad frame %s" % (name, [int(cnt_b[f]) for f in bad_pos]))
    m.close()
    fd.close()
