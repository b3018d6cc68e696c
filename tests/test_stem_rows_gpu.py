"""The detectors' 5x5 first convolution with its picture rows kept in registers down a column of tiles (stem_mfma_kernel, engine option
"stem_mfma" = 1) against the row-wise MFMA form (= 2) and the packed-FMA kernel (= 0): the three compute every output by the same chain of f32 FMAs,
so every comparison here is bit for bit.

A run is "stem_run" output rows of one 64-pixel column of one frame.  Chosen per launch (0) it is a power of two that gives every wave one run, and the
row-wise form where that leaves a single row (a handful of frames): the cases here therefore also FORCE run lengths, so that the column form runs at
every size — runs that end ragged, runs longer than the frame, fewer runs than workgroups, one-row and two-row frames (shorter than the window's fill)."""
import re

import numpy as np
import pytest

import synth_tflite as st
from conftest import model_path, seeded_input
from test_gpu_isolation import _run_poisoned
from test_gpu_parity import _raw_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


def _stem_tensor(m):
    """Index of the first launch's output tensor (the plan text: `conv+relu t0[256x256x3] -> t4[128x128x24] ...`)."""
    line = [l for l in m.describe().splitlines() if not l.startswith("#")][0]
    return int(re.search(r"-> t(\d+)\[", line).group(1))


def _stem_and_outputs(m, x, opts):
    """Runs x with the options set and returns (the first convolution's output of every frame, the network's outputs)."""
    for k, v in opts.items():
        m.set_option(k, v)
    outs = [o.copy() for o in m.run(x)]
    t = _stem_tensor(m)
    stem = np.stack([m.debug_tensor(t, f, cap=1 << 20) for f in range(x.shape[0])])
    return stem, outs


def _edgy(x):
    """Large values in the first / last rows and columns (the zero padding lies beside them) and an all-zero frame."""
    x[0, 0, :, :] = 11.0
    x[0, -1, :, :] = -7.0
    x[-1, :, 0, :] = 5.0
    x[-1, :, -1, :] = -9.0
    x[-1, :, -2, :] = 3.0
    if x.shape[0] > 2:
        x[1] = 0.0
    return x


FORMS = [{"stem_mfma": 0}, {"stem_mfma": 2}, {"stem_mfma": 1, "stem_run": 0}, {"stem_mfma": 1, "stem_run": 16}, {"stem_mfma": 1, "stem_run": 5},
         {"stem_mfma": 1, "stem_run": 32}]


@pytest.mark.parametrize("name,nb", [("back", 1), ("back", 2), ("back", 3), ("back", 9), ("short", 1), ("short", 5)])
def test_first_convolution_bit_equal_in_all_forms(gpu, name, nb):
    """stem_mfma = 1 against 0 and against 2 on the shipped detectors: the stem's own output tensor (every tensor keeps its arena slot: reuse = 0) and
    the raw outputs.  One frame of BackCamera is 64 runs of 16 rows on 16 workgroups, 26 runs of 5 (the last of 3 rows) per column; 3 and 9 frames are
    no multiple of anything in the grid."""
    m = gpu.Model(model_path(name))
    m.set_option("reuse", 0)
    x = _edgy(seeded_input(name, nb, 5100 + nb, m.input_dims[1:3]))
    ref_stem, ref_outs = _stem_and_outputs(m, x, FORMS[0])
    assert np.isfinite(ref_stem).all() and np.abs(ref_stem).max() > 0
    for opts in FORMS[1:]:
        stem, outs = _stem_and_outputs(m, x, opts)
        np.testing.assert_array_equal(stem, ref_stem, err_msg=str(opts))
        for o, r in zip(outs, ref_outs):
            np.testing.assert_array_equal(o, r, err_msg=str(opts))
    m.close()


def _stem_graph(seed, h, w, act):
    """input -> 5x5 stride-2 convolution to 24 channels with `act` behind it -> 1x1 convolution to 8 channels (the graph's output)."""
    g = st.GraphBuilder(seed, [1, h, w, 3])
    x = g.conv(g.input, 24, 5, 2, act=st.ACT_RELU6 if act == "relu6" else st.ACT_NONE)
    x = g.relu(x) if act == "relu" else (g.prelu(x) if act == "prelu" else x)
    g.outputs = [g.conv(x, 8)]
    return g.finish()


# (output height, output width, frames): >= 64 tiles of 64 pixels each, or the launch stays on the packed-FMA kernel whatever the option says
BOUNDARY_SHAPES = [(1, 64, 70), (2, 64, 33), (7, 64, 11), (5, 128, 9), (7, 65, 10), (3, 127, 23)]
BOUNDARY_CASES = [(s, a) for s in BOUNDARY_SHAPES for a in ("prelu", "none", "relu6")] + [((7, 64, 11), "relu"), ((5, 128, 9), "relu")]


@pytest.mark.parametrize("shape,act", BOUNDARY_CASES, ids=["%dx%dx%d-%s" % (s + (a,)) for s, a in BOUNDARY_CASES])
def test_run_boundaries_on_small_pictures(gpu, oracle, tmp_path, shape, act):
    """Synthetic 5x5 stride-2 stems on small pictures: output heights of 1 and 2 (shorter than the window's fill: every row below the first window is
    outside the picture), heights that are no multiple of the run (7 and 5 rows in runs of 2 and 4: last runs of 1 row), runs longer than the frame (32);
    output widths of exactly one tile, two tiles, and one tile plus a pixel / two tiles less a pixel (not whole tiles: those stay on the packed-FMA
    kernel in every form, which this pins); PReLU, no activation, ReLU6 and ReLU behind the convolution.  Frame 0 and the last frame against the oracle."""
    torch = pytest.importorskip("torch")
    ho, wo, nb = shape
    path = tmp_path / "stem.tflite"
    path.write_bytes(_stem_graph(900 + ho * 131 + wo, 2 * ho, 2 * wo, act))
    m = gpu.Model(str(path))
    m.set_option("reuse", 0)
    x = _edgy(np.random.RandomState(ho * 1000 + wo).uniform(-1.0, 1.0, (nb, 2 * ho, 2 * wo, 3)).astype(np.float32))
    ref_stem, ref_outs = _stem_and_outputs(m, x, {"stem_mfma": 0})
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[0] == "stem_conv_kernel", labels
    for r, o in zip(oracle.Model(str(path)).run(x[[0, nb - 1]], nthreads=2), ref_outs):
        _raw_close(o[[0, nb - 1]], r)
    for opts in ({"stem_mfma": 2}, {"stem_mfma": 1, "stem_run": 0}, {"stem_mfma": 1, "stem_run": 2}, {"stem_mfma": 1, "stem_run": 4},
                 {"stem_mfma": 1, "stem_run": 1}, {"stem_mfma": 1, "stem_run": 32}):
        stem, outs = _stem_and_outputs(m, x, opts)
        labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
        assert labels[0] == ("stem_mfma_kernel" if wo % 64 == 0 else "stem_conv_kernel"), labels
        np.testing.assert_array_equal(stem, ref_stem, err_msg=str(opts))
        np.testing.assert_array_equal(outs[0], ref_outs[0], err_msg=str(opts))
    m.close()


def test_column_runs_under_the_scratch_poison(gpu):
    """The column form under the scratch-poison hook (tests/test_gpu_isolation.py): arena, scratch and output buffers hold NaN / 3.39e38 before every
    run and the results must not move a bit — a window that slides one picture row too far reads a neighbour's frame or the poison behind the last
    one.  Then a NaN frame in the middle of the batch: the first convolution's tensors of the frames beside it stay what they were."""
    m = gpu.Model(model_path("back"))
    x = seeded_input("back", 33, 777, m.input_dims[1:3])
    for run in (0, 16, 3):          # 33 frames: chosen per launch = runs of 4 rows
        m.set_option("stem_run", run)
        _run_poisoned(m, x)
    m.set_option("reuse", 0)
    m.set_option("stem_run", 16)
    clean, _ = _stem_and_outputs(m, x[:5], {})
    bad = x[:5].copy()
    bad[2] = np.nan
    m.set_option("test_poison", 1)
    dirty, _ = _stem_and_outputs(m, bad, {})
    m.set_option("test_poison", 0)
    np.testing.assert_array_equal(dirty[[0, 1, 3, 4]], clean[[0, 1, 3, 4]])
    m.close()


def test_detections_of_nine_frames_equal_the_row_wise_form(gpu, man_image):
    """End to end (the plan, its replay graphs, the post-processing): detections of 9 BackCamera frames with the column form — chosen per launch and
    with forced runs — equal those with stem_mfma = 2, bit for bit, on repeated calls."""
    from PIL import Image
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    face = np.asarray(Image.fromarray(man_image).resize((256, 256)), np.float32) * (2.0 / 255.0) - 1.0
    x = np.stack([np.roll(face, (7 * k, -5 * k), axis=(0, 1)) if k % 4 != 3 else np.zeros_like(face) for k in range(9)])
    fd.model.set_option("stem_mfma", 2)
    ref, ref_counts = fd.infer_tensor(x, cap=8)
    assert ref_counts.sum() > 0
    for run in (0, 16, 6):
        fd.model.set_option("stem_mfma", 1)
        fd.model.set_option("stem_run", run)
        for _ in range(2):
            out, counts = fd.infer_tensor(x, cap=8)
            np.testing.assert_array_equal(counts, ref_counts)
            np.testing.assert_array_equal(out, ref)
    fd.close()
