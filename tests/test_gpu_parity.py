"""GPU parity tests: the HIP path, called through the C ABI (ctypes), against the C oracle on the same inputs.

Tolerances (north_star "within a stated fp32 tolerance, boxes within 1e-3 IoU"):
  raw network outputs   |d| <= 1e-4 * max(1, max|x|)   (f32 convolution re-association; TFLite itself is not
                                                         bit-reproducible across its kernels)
  detections            identical count and order; coordinates <= 1e-5; box IoU >= 0.999
  post-processing alone (same raw inputs) — bit-exact except the score, which depends on the device expf (<= 2 ulp)
  landmarks             <= 1e-5 normalised units
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, MODEL_FILES, model_path, seeded_input

pytestmark = pytest.mark.gpu

RAW_TOL = 1e-4


def _raw_close(got, ref):
    ref = ref.reshape(got.shape)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= RAW_TOL * scale, "max|diff| %.3e > %.1e * %.1f" % (err, RAW_TOL, scale)
    return err


def _iou(a, b):
    x0, y0, x1, y1 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    inter = max(0.0, x1 - x0) * max(0.0, y1 - y0)
    ua = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / ua if ua > 0 else 1.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden.npz"))


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


@pytest.mark.parametrize("name", list(MODEL_FILES))
@pytest.mark.parametrize("fuse", [0, 1, 2, 3, 4, 5])
def test_network_raw_outputs_vs_oracle(gpu, oracle, name, fuse):
    m = gpu.Model(model_path(name))
    m.set_option("fuse", fuse)
    om = oracle.Model(model_path(name))
    x = seeded_input(name, 5, 4321, m.input_dims[1:3])
    outs = m.run(x)
    refs = om.run(x, nthreads=5)
    for o, r in zip(outs, refs):
        _raw_close(o, r)
    m.close()


@pytest.fixture(scope="module")
def synth_models(tmp_path_factory):
    """The synthetic graphs of tests/synth_tflite.py written out as .tflite files (oracle and product both read files)."""
    import synth_tflite
    d = tmp_path_factory.mktemp("synth")
    out = {}
    for name, (make, h, w) in synth_tflite.CASES.items():
        p = d / (name + ".tflite")
        p.write_bytes(make())
        out[name] = (str(p), h, w)
    return out


@pytest.mark.parametrize("case", sorted(__import__("synth_tflite").CASES))
@pytest.mark.parametrize("fuse", [0, 2, 3, 4, 5])
def test_synthetic_graphs_vs_oracle(gpu, oracle, synth_models, case, fuse):
    """The reference graphs' operator chains on OTHER shapes (ragged row bands, partial pixel groups, odd channel counts, chains with
    edge stages and heads at 12x12 / 6x6 / 20x20, double blocks): every lowering level against the oracle, odd batch, replayed graph."""
    path, h, w = synth_models[case]
    m = gpu.Model(path)
    m.set_option("fuse", fuse)
    om = oracle.Model(path)
    rs = np.random.RandomState(100 + fuse)
    x = rs.uniform(-1, 1, (5, h, w, 3)).astype(np.float32)
    refs = om.run(x, nthreads=5)
    outs = m.run(x)
    for o, r in zip(outs, refs):
        _raw_close(o, r)
    xd = __import__("torch").from_numpy(x).cuda()
    for _ in range(2):
        outs_d = m.run(xd)
    for o, r in zip(outs_d, refs):
        _raw_close(o.cpu().numpy(), r)
    m.close()


@pytest.mark.parametrize("case", sorted(__import__("synth_tflite").CASES))
def test_synthetic_graphs_on_the_single_launch_plan(gpu, oracle, synth_models, case):
    """Round 6: the single-launch plan's lowering grew (tiles of their own sizes placed by an interval allocator, skips with fewer channels than the
    output, stages of more than 128 channels, lateral convolutions with an up-sampled skip, inputs read back from the workspace).  Every synthetic graph
    — the reference's operator chains on OTHER shapes — runs with option band = 2 at one and two frames: where the graph has a program (wholly or as a
    prefix) its results must be the oracle's, run to run bit-identical; where it has none the batched plan answers.  band_wide = 0 likewise."""
    path, h, w = synth_models[case]
    om = oracle.Model(path)
    rs = np.random.RandomState(321)
    x = rs.uniform(-1, 1, (2, h, w, 3)).astype(np.float32)
    x[1, : h // 2] = 0.0
    refs = om.run(x, nthreads=2)
    for wide in (1, 0):
        m = gpu.Model(path)
        m.set_option("band", 2)
        m.set_option("band_wide", wide)
        for nb in (1, 2):
            outs = [o.copy() for o in m.run(x[:nb])]
            for o, r in zip(outs, refs):
                _raw_close(o, r[:nb])
            for o, o2 in zip(outs, m.run(x[:nb])):
                np.testing.assert_array_equal(o, o2)
        m.close()


@pytest.mark.parametrize("batch", [1, 97, 300])
def test_walking_band_kernel_many_items(gpu, oracle, synth_models, batch):
    """Row-band bottleneck launches put one workgroup on every CU and let it walk over its share of the bands with the next band's
    input in flight: batches whose band count is below, around and well above the CU count (ragged last bands included), for the
    synthetic 20 x 32 frame and for the real iris graph."""
    for path, h, w, lo in ((synth_models["iris_32x20_ragged_bands"][0], 40, 64, -1.0), (model_path("iris"), 64, 64, 0.0)):
        m = gpu.Model(path)
        om = oracle.Model(path)
        x = np.random.RandomState(7 + batch).uniform(lo, 1, (batch, h, w, 3)).astype(np.float32)
        refs = om.run(x, nthreads=8)
        outs = m.run(x)
        for o, r in zip(outs, refs):
            _raw_close(o, r)
        m.close()


@pytest.mark.parametrize("name", list(MODEL_FILES))
@pytest.mark.parametrize("budget_kib", [40, 78, 156])
def test_stage_programs_vs_oracle(gpu, oracle, name, budget_kib):
    """Fuse level 5 (frame-resident stage programs, resident_kernels.hip) cut differently by the LDS budget: other group
    boundaries, other LDS placements, LOAD stages and global gathers in other places — same results."""
    m = gpu.Model(model_path(name))
    m.set_option("fuse", 5)
    m.set_option("res_budget", budget_kib)
    om = oracle.Model(model_path(name))
    x = seeded_input(name, 3, 977 + budget_kib, m.input_dims[1:3])
    outs = m.run(x)
    refs = om.run(x, nthreads=3)
    for o, r in zip(outs, refs):
        _raw_close(o, r)
    # odd batch through a graph replay and a second call (the descriptors are per plan, the bases per launch)
    xd = __import__("torch").from_numpy(x).cuda()
    for _ in range(2):
        outs_d = m.run(xd)
    for o, r in zip(outs_d, refs):
        _raw_close(o.cpu().numpy(), r)
    m.close()


@pytest.mark.parametrize("name", ["back", "front", "landmark"])
def test_strip_and_pipeline_kernels_agree(gpu, name):
    """The kernels that can run a BlazeBlock are interchangeable.  However a run of blocks is cut into row-pipelined
    chains (fuse 4, "pipe" = 2 / 3 / 4 blocks per launch) the bits are the same: the chains execute the same operations
    in the same order, one or two rows per pipeline step, the 1x1 convs as packed FMAs or on v_mfma_f32_4x4x1_16b_f32 (an f32
    MFMA accumulates like an fmaf chain).  One strip-kernel launch per block (fuse 3) and the LDS-ring block kernel ("strip" = 0) agree with
    them up to the order of the 3x3 sum / the depthwise bias folded into the pointwise bias (the stride-2 block that ends
    a chain is computed that way, the stand-alone block kernel adds the bias first): raw-output tolerance of the oracle
    comparison."""
    m = gpu.Model(model_path(name))
    x = seeded_input(name, 6, 99, m.input_dims[1:3])
    m.set_option("fuse", 4)
    m.set_option("small_chain", 0)   # 6 frames would otherwise take the small-batch form (one launch per block, next test)
    chained = [o.copy() for o in m.run(x)]
    if name != "front":  # the front model has no run of equal-shape narrow blocks
        assert "row-pipelined" in m.describe()
    if name == "back":
        assert "stride-2 tail" in m.describe()
    for pipe in (2, 3):
        m.set_option("pipe", pipe)
        for o, r in zip(m.run(x), chained):
            np.testing.assert_array_equal(o, r)
    import torch
    if name != "front":  # default: two rows per step, pointwise convs on v_mfma_f32_4x4x1_16b_f32 (strip_pipe2m_kernel)
        labels = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
        assert any(k.startswith("strip_pipe2m_kernel") for k in labels), labels
    # one row per step, packed FMAs; two rows, packed-FMA pointwise convs; one row per step with the MFMA pointwise convs (the form odd heights take)
    for rows, sym in ((1, "strip_pipe_kernel"), (2, "strip_pipe2_kernel"), (4, "strip_pipe1m_kernel")):
        m.set_option("pipe_rows", rows)
        for o, r in zip(m.run(x), chained):
            np.testing.assert_array_equal(o, r)
        if name != "front":
            labels = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
            assert any(k.startswith(sym + "<") for k in labels) and not any(k.startswith("strip_pipe2m_kernel") for k in labels), labels
    m.set_option("pipe_rows", 0)
    m.set_option("fork", 0)  # output heads on the trunk's stream instead of side streams
    for o, r in zip(m.run(x), chained):
        np.testing.assert_array_equal(o, r)
    m.set_option("fork", 1)
    m.set_option("fuse", 3)
    for o, r in zip(m.run(x), chained):
        _raw_close(o, r)
    m.set_option("strip", 0)
    for o, r in zip(m.run(x), chained):
        _raw_close(o, r)
    m.close()


@pytest.mark.parametrize("name", ["back", "landmark"])
def test_small_batch_chains_run_block_by_block(gpu, oracle, name):
    """A row pipeline is a chain of dependent steps whose length does not shrink with the batch (88 us per launch for ONE BackCamera
    frame): up to `small_chain` frames (default 16; the test sets 8) the members of such a chain run as one strip-kernel launch each through a
    ping-pong scratch — FaceDetection::infer(&Mat) is a batch of one (face_detection.rs:205-267).  Batches 1, 3 and 8 against the
    oracle, against the pipelined form (tolerance: the stride-2 block that ends a chain folds its depthwise bias differently in the
    stand-alone block kernel), batch 9 back on the pipelines, and the launch labels of both."""
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path(name))
    om = oracle.Model(model_path(name))
    for nb in (1, 3, 8, 9):
        x = seeded_input(name, nb, 400 + nb, m.input_dims[1:3])
        m.set_option("small_chain", 8)
        outs = [o.copy() for o in m.run(x)]
        labels = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
        small = any("(small batch)" in k for k in labels)
        piped = any(k.startswith("strip_pipe") for k in labels)
        if name == "back":
            assert small == (nb <= 8) and piped == (nb > 8), labels
        for o, r in zip(outs, om.run(x, nthreads=4)):
            _raw_close(o, r)
        m.set_option("small_chain", 0)
        for o, r in zip(m.run(x), outs):
            _raw_close(o, r)
    m.close()


def test_mstrip_blocks_vs_oracle_and_block_kernel(gpu, oracle):
    """BackCamera's seven 32x32x48 blocks run on mstrip_kernel (depthwise stage in the MFMA operand layout, pointwise conv on
    v_mfma_f32_16x16x4_f32) from 32 frames per launch on; below that the LDS-ring block kernel takes them.  An odd batch of 35 frames
    (the last workgroup has one live wave) against the oracle frame by frame, against the block-kernel path ("strip" = 0), and frame
    7 alone (block kernel: batch 1) against frame 7 inside the batch."""
    m = gpu.Model(model_path("back"))
    x = seeded_input("back", 35, 4711, m.input_dims[1:3])
    x[5] = 0.0                       # an all-zero frame: biases only
    x[9, :, :128] = -1.0             # half-saturated frame
    outs = [o.copy() for o in m.run(x)]
    recs = m.profile(__import__("torch").from_numpy(x).cuda(), reps=1)
    labels = {r["kernel"] for r in recs}
    # round 5: the run of seven blocks is ONE launch (mstrip_chain_kernel: a workgroup per frame, a barrier between blocks, every
    # intermediate tensor still written to its arena slot)
    assert any(k.startswith("mstrip_chain_kernel") for k in labels) and sum(r["kernel"].startswith("mstrip") for r in recs) == 1, labels
    om = oracle.Model(model_path("back"))
    refs = om.run(x, nthreads=8)
    for o, r in zip(outs, refs):
        _raw_close(o, r)
    for o, r in zip(m.run(x[7:8]), outs):
        _raw_close(o[0], r[7])
    # one launch per block (option "mchain" = 0: mstrip_kernel x 7) computes the same bits: same row code, same order of every sum
    m.set_option("mchain", 0)
    recs1 = m.profile(__import__("torch").from_numpy(x).cuda(), reps=1)
    assert sum(r["kernel"].startswith("mstrip_kernel") for r in recs1) == 7, [r["kernel"] for r in recs1]
    for o, r in zip(m.run(x), outs):
        np.testing.assert_array_equal(o, r)
    m.set_option("mchain", 1)
    m.set_option("strip", 0)
    labels0 = {r["kernel"] for r in m.profile(__import__("torch").from_numpy(x).cuda(), reps=1)}
    assert not any(k.startswith("mstrip") for k in labels0)
    for o, r in zip(m.run(x), outs):
        _raw_close(o, r)
    m.close()


@pytest.mark.parametrize("name,kernels", [("full", ["mdblock_kernel", "ms2_kernel<8,1,3>", "ms2_kernel<16,2,2>", "xc_kernel"]), ("landmark", ["mdblock_kernel<pair>", "mwalk_kernel<16,4,2>", "mdblock_kernel<stem+pair>", "ms2_kernel<8,4,2>", "ms2_kernel<4,2,3>"]), ("iris", ["mbneck_kernel"])])
def test_operand_layout_kernels_vs_oracle_and_lds_kernels(gpu, oracle, name, kernels):
    """The row-walking MFMA kernels of round 3 (mdblock / mwalk / ms2 / mbneck: depthwise stages in the v_mfma_f32_16x16x4_f32 operand
    layout) take the wide double blocks and stride-2 blocks of full_range, the 48x48x32 / 24x24x64 blocks, the 96x96x16 block pair and the
    48 -> 24 stride-2 block of the face mesh and the 32x32 bottleneck pairs of the iris network from 32 (96) frames per launch on.  An odd batch of 33 frames (97 for the mesh; mbneck: the last workgroup repeats the last frame)
    against the oracle frame by frame, against the LDS-tensor kernels ("strip" = 0), and frame 7 alone (batch 1: the older kernels)
    against frame 7 inside the batch."""
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path(name))
    nb = 97 if name == "landmark" else 33   # (the 24-pixel-wide mwalk form starts at 96 ROIs)
    x = seeded_input(name, nb, 4242, m.input_dims[1:3])
    x[5] = 0.0                                   # an all-zero frame: biases only
    x[9, :, : x.shape[2] // 2] = x.min()         # half-saturated frame
    outs = [o.copy() for o in m.run(x)]
    labels = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
    for k in kernels:
        assert any(l.startswith(k) for l in labels), (k, labels)
    om = oracle.Model(model_path(name))
    refs = om.run(x, nthreads=8)
    for o, r in zip(outs, refs):
        _raw_close(o, r)
    for o, r in zip(m.run(x[7:8]), outs):
        _raw_close(o[0], r[7])
    m.set_option("strip", 0)
    labels0 = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
    assert not any(l.startswith(("mdblock", "mwalk", "mbneck", "ms2")) for l in labels0), labels0
    for o, r in zip(m.run(x), outs):
        _raw_close(o, r)
    m.close()


@pytest.mark.parametrize("name,nb", [("back", 256), ("back", 17), ("short", 256), ("front", 70), ("short", 5)])
def test_mfma_stem_bit_equal_to_the_valu_stem(gpu, oracle, name, nb):
    """Round 6: the detectors' 5x5 first convolution (face_detection.rs:235, first operator behind `interpreter.invoke()`) on the matrix cores
    (stem_mfma_kernel: lane = output pixel, v_mfma_f32_4x4x1_16b_f32 with the weights broadcast from one block of a weight
    register, the window's rows by buffer loads).  Every output is the same k-sequential chain of f32 FMAs as in stem_conv_kernel, so the two agree BIT FOR
    BIT: raw outputs of the whole network with option stem_mfma = 1 / 0, on frames whose first / last rows and columns carry large values (the zero padding
    sits beside them: one pixel left / above, two right / below), an all-zero frame, batches with a ragged last round of tiles; originals against the oracle."""
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path(name))
    x = seeded_input(name, nb, 4000 + nb, m.input_dims[1:3])
    x[1, 0, :, :] = 11.0
    x[1, -1, :, :] = -7.0
    x[2, :, 0, :] = 5.0
    x[2, :, -1, :] = -9.0
    x[2, :, -2, :] = 3.0
    x[3] = 0.0
    outs = [o.copy() for o in m.run(x)]
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[0] == "stem_mfma_kernel", labels
    m.set_option("stem_mfma", 0)
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[0] == "stem_conv_kernel", labels
    for o, o2 in zip(outs, m.run(x)):
        np.testing.assert_array_equal(o, o2)
    om = oracle.Model(model_path(name))
    sel = [0, 1, 2, 3, nb - 1]
    for o, r in zip(outs, om.run(x[sel], nthreads=5)):
        _raw_close(o[sel], r)
    m.close()


@pytest.mark.parametrize("nb", [32, 61, 200])
def test_first_convolution_inside_the_block_pair_launch(gpu, oracle, nb):
    """Round 6: the face mesh's first convolution (3x3 stride 2, 192x192x3 -> 96x96x16, PReLU; face_landmark.rs:265 behind
    `interpreter.invoke()`) runs inside the launch of the two BlazeBlocks behind it (mdblock_kernel<stem+pair>: a wave computes its pixels of x row
    r + 1 from the picture — 7 k-steps of v_mfma_f32_16x16x4_f32 over the window's 27 values, B operands straight from global memory — while it works on
    row r; the 96x96x16 tensor is neither written nor read).  Against the oracle frame by frame, against the plan with the convolution as a launch of its own
    (option stem_fuse = 0), with pictures whose last row / column (the SAME padding's zero row / column lies behind them) and first row carry large values, band
    sizes that end ragged, and through the u8 entry (which keeps the separate launch)."""
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path("landmark"))
    x = seeded_input("landmark", nb, 99 + nb, m.input_dims[1:3])
    x[1, -1, :, :] = 7.0          # the last row and column: the window of output row / column 95 ends one pixel behind them
    x[1, :, -1, :] = -5.0
    x[2, 0, :, :] = 9.0
    x[3] = 0.0
    om = oracle.Model(model_path("landmark"))
    refs = om.run(x, nthreads=8)
    outs = [o.copy() for o in m.run(x)]
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[0] == "mdblock_kernel<stem+pair>" and labels[1] == "ms2_kernel<4,2,3>", labels
    assert labels[2] == "mdblock_kernel<pair>" and labels[3] == "ms2_kernel<8,4,2>", labels   # the two 48x48x32 blocks: one launch, the tensor between them stays in LDS
    for o, r in zip(outs, refs):
        _raw_close(o, r)
    for o, o2 in zip(outs, m.run(x)):
        np.testing.assert_array_equal(o, o2)
    m.set_option("stem_fuse", 0)
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[0].startswith("stem_conv_kernel") and labels[1] == "mdblock_kernel<pair>", labels
    for o, r in zip(m.run(x), outs):
        _raw_close(o, r)
    m.set_option("pair_fuse", 0)
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[3] == labels[4] == "mwalk_kernel<8,2,3>", labels
    for o, r in zip(m.run(x), outs):
        _raw_close(o, r)
    m.set_option("stem_fuse", 1)
    m.set_option("pair_fuse", 1)
    for band in (5, 13, 96):      # rows per band (option "mdb_band"; 0 = chosen by the launcher): ragged last bands, one band per frame
        m.set_option("mdb_band", band)
        for o, r in zip(m.run(x), refs):
            _raw_close(o, r)
    m.close()


def test_first_convolution_inside_the_block_pair_launch_relu_graph(gpu, oracle, synth_models):
    """The same launches on a synthetic graph of the face mesh's shapes with ReLU behind every operator (the shipped graph has PReLU everywhere: the
    kernels' ReLU instantiations would otherwise never run): 40 frames against the oracle, the fused launches against the separate ones."""
    torch = pytest.importorskip("torch")
    path, h, w = synth_models["mesh_192_relu"]
    m = gpu.Model(path)
    x = np.random.RandomState(5).uniform(-1, 1, (40, h, w, 3)).astype(np.float32)
    x[1, -1] = 6.0
    x[1, :, -1] = -4.0
    outs = [o.copy() for o in m.run(x)]
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert labels[0] == "mdblock_kernel<stem+pair>", labels
    for o, r in zip(outs, oracle.Model(path).run(x, nthreads=8)):
        _raw_close(o, r)
    m.set_option("stem_fuse", 0)
    m.set_option("pair_fuse", 0)
    for o, r in zip(m.run(x), outs):
        _raw_close(o, r)
    m.close()


@pytest.mark.parametrize("name", ["landmark", "back"])
def test_round6_launches_in_chunks_and_lanes(gpu, oracle, name):
    """The launches of round 6 that replace two nodes' launches (the face mesh's first convolution inside the block pair's launch, its two 48x48x32 blocks as one
    launch) and the detectors' first convolution on the matrix cores, in the plans a host can ask for besides the default: the batch in chunks (a chunk's
    tensors start at an offset of the arena: 300 frames in chunks of 96 — the last one is 12 frames, below every threshold), two lanes, eager launches
    instead of graph replay.  Each against the default plan's results on the same frames (bit for bit where the kernels are the same: chunks of >= 96 frames),
    and a sample against the oracle."""
    m = gpu.Model(model_path(name))
    nb = 300
    x = seeded_input(name, nb, 606, m.input_dims[1:3])
    ref = [o.copy() for o in m.run(x)]
    om = oracle.Model(model_path(name))
    sel = [0, 95, 96, 191, 288, 299]
    for o, r in zip(ref, om.run(x[sel], nthreads=6)):
        _raw_close(o[sel], r)
    m.set_option("chunk", 96)
    for o, r in zip(m.run(x), ref):
        _raw_close(o, r)
        np.testing.assert_array_equal(o[:288], r[:288]) if name == "back" else None   # (BackCamera: the same kernels from 96 frames on; the mesh's tail picks frames per workgroup by the batch)
    m.set_option("chunk", 0)
    m.set_option("lanes", 2)
    for o, r in zip(m.run(x), ref):
        _raw_close(o, r)
    m.set_option("lanes", 1)
    m.set_option("graph", 0)
    for o, r in zip(m.run(x), ref):
        np.testing.assert_array_equal(o, r)
    m.close()


@pytest.mark.parametrize("name", ["back", "front", "full", "landmark", "iris"])
def test_batch_size_sweep_across_kernel_thresholds(gpu, oracle, name):
    """Which kernel runs a layer depends on the batch (the row-walking kernels start at 32 or 96 frames per launch, small grids spread
    their tiles, two-frame workgroups repeat the last frame of an odd batch): batches just below, at and above every threshold — and odd
    ones — must agree with the LDS-tensor kernels ("strip" = 0) on the same frames, which in turn agree with the oracle on a sample."""
    m = gpu.Model(model_path(name))
    x = seeded_input(name, 130, 777, m.input_dims[1:3])
    m.set_option("strip", 0)
    ref = [o.copy() for o in m.run(x)]
    om = oracle.Model(model_path(name))
    for o, r in zip(ref, om.run(x[[0, 31, 64, 129]], nthreads=4)):
        _raw_close(o[[0, 31, 64, 129]], r)
    m.set_option("strip", 1)
    # (37 / 70 frames: the band sizes the launchers pick there are odd — ms2_kernel's bands then start on odd output rows, which round 5 found broken)
    for nb in (1, 2, 5, 31, 32, 33, 37, 63, 70, 95, 96, 97, 128, 129, 130):
        for o, r in zip(m.run(x[:nb]), ref):
            _raw_close(o, r[:nb])
    m.close()


@pytest.mark.parametrize("name", ["landmark", "iris"])
def test_tail_programs_frames_per_workgroup(gpu, oracle, name):
    """Round 5: the small-spatial stage programs of the face mesh (24x24 -> 12x12 x2 -> 6x6 x3 -> 3x3, the two 3x3 branches) and the iris
    network (the two 8x8 -> 2x2 branches) run on tail_kernel: G frames per workgroup share the 16-pixel MFMA tiles, LDS tensors without
    borders.  Every G from 1 to what the LDS holds — with batches that leave the last workgroup partly empty and pixel tiles that
    straddle two frames — against the oracle frame by frame, bit-identical among each other (a pixel's contraction order does not
    depend on its tile slot), and against the round-4 kernels (option "tail" = 0: resident_kernel / chain_kernel)."""
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path(name))
    assert "several frames per workgroup" in m.describe()
    x = seeded_input(name, 37, 99, m.input_dims[1:3])
    x[5] = 0.0
    x[9, :, : x.shape[2] // 2] = x.max()
    om = oracle.Model(model_path(name))
    refs = om.run(x, nthreads=8)
    labels = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
    assert "tail_kernel" in labels and "resident_kernel" not in labels or name == "iris", labels
    base = None
    for g in (0, 1, 2, 3, 4, 5, 8, 16):
        m.set_option("tail_g", g)
        outs = [o.copy() for o in m.run(x)]
        for o, r in zip(outs, refs):
            _raw_close(o, r)
        if base is None:
            base = outs
        for o, b in zip(outs, base):
            np.testing.assert_array_equal(o, b)
        for nb in (1, 2, 3, 7, 36):   # (other layers of the net change kernels with the batch: tolerance, not bits)
            for o, b in zip(m.run(x[:nb]), base):
                _raw_close(o, b[:nb])
    # a batch large enough for the automatic choice to pack frames (more frames than CUs)
    m.set_option("tail_g", 0)
    xb = np.concatenate([x] * 16)[:577]
    for pre in (1, 2, 0):   # both register variants of the kernel (constants a stage ahead / two workgroups per CU), then the automatic choice
        m.set_option("tail_pre", pre)
        for o, b in zip(m.run(xb), base):   # (other layers of the net change kernels with the batch: tolerance, not bits)
            _raw_close(o, np.concatenate([b] * 16)[:577])
        for o, b in zip(m.run(x), base):
            np.testing.assert_array_equal(o, b)
    m.set_option("tail", 0)
    labels0 = {r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)}
    assert "tail_kernel" not in labels0, labels0
    for o, b in zip(m.run(x), base):
        _raw_close(o, b)
    m.close()


@pytest.mark.parametrize("case", ["iris_6x10_c256_tail", "iris_4x4_c128_down_tail", "mesh_160", "iris_32x20_ragged_bands"])
def test_tail_programs_on_other_shapes(gpu, oracle, synth_models, case):
    """tail_kernel on shapes the shipped graphs do not contain (tests/synth_tflite.py): 256-channel stages (sixteen output tiles: two per
    wave; a 1x1 contraction over 256 values streamed in two k-blocks), 6 x 10 / 5 x 5 / 10 x 16 frames whose pixels do not fill whole
    16-pixel tiles (tiles straddle frames when several frames share a workgroup; odd widths in the pixel-pair depthwise phase), a
    stride-2 block down to 2 x 2.  Every G against the oracle frame by frame and bit-identical among each other, both register variants."""
    path, h, w = synth_models[case]
    m = gpu.Model(path)
    assert "several frames per workgroup" in m.describe()
    om = oracle.Model(path)
    x = np.random.RandomState(77).uniform(-1, 1, (23, h, w, 3)).astype(np.float32)
    refs = om.run(x, nthreads=8)
    base = None
    for pre in (1, 2):
        m.set_option("tail_pre", pre)
        for g in (1, 2, 3, 5, 8):
            m.set_option("tail_g", g)
            outs = [o.copy() for o in m.run(x)]
            for o, r in zip(outs, refs):
                _raw_close(o, r)
            if base is None:
                base = outs
            for o, b in zip(outs, base):
                np.testing.assert_array_equal(o, b)
    m.close()


@pytest.mark.parametrize("name,frames", [("back", 2), ("front", 4), ("short", 4), ("landmark", 2), ("iris", 8), ("full", 2), ("sparse", 2)])
def test_single_launch_plan_vs_oracle_and_batched_plan(gpu, oracle, name, frames):
    """Round 5: the single-image plan (bandnet_kernels.hip) — everything behind the first convolution ONE launch, a row band per workgroup
    kept in LDS, halo rows handed over as tagged packets.  Option "band" = 2 runs it for every call of few enough frames: against the
    oracle frame by frame, against the batched plan (band = 0), run-to-run bit-identical (the arithmetic does not depend on who arrives
    first), eager and as a replayed graph, with one and with several rows per band, and one frame beyond what a launch takes.  The face
    mesh's program stops in front of its two whole-frame convolutions, which keep their launches behind it (three LDS tiles: the 6x6
    tensor has two readers); the iris network's (iris_landmark.rs:203) is all 54 nodes between its first convolution and its two whole-frame
    heads: the bottlenecks' skips read from a third tile, the 2x2 stride-2 convolutions as stages whose contraction runs over the four taps,
    the 2x2-max skips of the blocks behind them read from the tile the convolution read, the two branches behind the 8x8 fork one after
    the other (four tiles).  Round 6: full_range's trunk (face_detection.rs:121) — its double blocks as two stages each (the second one's skip is the
    pair's input, zero-padded where the pair widens), its down-sampling pairs (stride-2 block, then a block whose skip is the 2x2 max of the pair's
    input padded from 32 / 64 to 48 / 96 channels), LDS tiles of their own sizes (56 KB for a 96x96x32 band, 19 KB for the 8-channel tensor
    between two of them, placed by an interval allocator), the 12x12 / 6x6 layers of up to 384 channels (contraction in rounds of eight chunks, output
    tiles in turns, depthwise taps from L2), the decoder (lateral 1x1 convolutions whose skip — the bilinear x2 up-sampling of the coarser map, read from its
    owners' packets — joins behind the activation; their trunk inputs, 10 - 30 stages old, read back from the launch's workspace) and the two heads: the
    whole network behind the first convolution is one launch of 48 stages.  With option band_wide = 0 the program ends at 12x12x36 (17 stages).
    full_range_sparse: 47 stages, down to its DEPTH_TO_SPACE heads (its stride-2 blocks read an explicitly padded input: BandStage::pre)."""
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path(name))
    assert m.single_launch_workgroups(1) > 0 and m.single_launch_workgroups(frames) == frames * m.single_launch_workgroups(1)
    assert m.single_launch_workgroups(frames + 1) == 0
    x = seeded_input(name, frames + 1, 77, m.input_dims[1:3])
    x[0, : x.shape[1] // 3] = 0.0                       # rows of zeros at the top (the zero halo and real zeros must agree)
    x[1, :, x.shape[2] // 2:] = x.max()
    om = oracle.Model(model_path(name))
    refs = om.run(x, nthreads=8)
    m.set_option("band", 0)
    batched = [o.copy() for o in m.run(x)]
    m.set_option("band", 2)
    for graph in (1, 0):
        m.set_option("graph", graph)
        for nb in range(1, frames + 2):
            outs = [o.copy() for o in m.run(x[:nb])]
            for o, r, b in zip(outs, refs, batched):
                _raw_close(o, r[:nb])
                _raw_close(o, b[:nb])
            for rep in range(3):
                for o, o2 in zip(outs, m.run(x[:nb])):
                    np.testing.assert_array_equal(o, o2)
    m.set_option("graph", 1)
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x[:1]).cuda(), reps=1)]
    behind = {"landmark": ["head_dot_kernel"] * 2,     # (the whole-frame convolutions of one to four frames: a wave per output, head_kernels.hip)
              "iris": ["head_dot_kernel"] * 2}.get(name, [])
    if name in ("full", "sparse"):
        assert "bandnet_kernel" in labels[:4] and labels.count("bandnet_kernel") == 1, labels
        if name == "sparse":   # 47 stages (its explicitly padded stride-2 blocks are stages with their window one row / column earlier); the DEPTH_TO_SPACE heads stay behind it
            assert labels == ["stem_conv_kernel", "bandnet_kernel", "dw_kernel", "d2s_kernel", "block_kernel<1,1,1,1,0>", "dw_kernel", "d2s_kernel"], labels
        if name == "full":
            assert labels == ["stem_conv_kernel", "bandnet_kernel"], labels   # the whole network: 48 stages, the decoder's lateral convolutions and heads included
            m.set_option("band_wide", 0)      # the program ends in front of 12x12x36 -> 144: 17 stages, 20 launches behind it
            for o, r in zip(m.run(x[:2]), refs):
                _raw_close(o, r[:2])
            assert len(m.profile(torch.from_numpy(x[:1]).cuda(), reps=1)) == 22
            m.set_option("band_wide", 1)
    else:
        assert labels[1:] == ["bandnet_kernel"] + behind, labels
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    assert "bandnet_kernel" not in labels, labels
    # fewer workgroups per frame: several rows per band (both edge rows of a band travel), more frames per launch
    one = [o.copy() for o in m.run(x[:1])]
    for nw in {"back": (128,), "landmark": (48,), "iris": (16,), "full": (), "sparse": ()}.get(name, (32,)):   # (full: two-row bands of 96x96x32 do not fit the LDS)
        m.set_option("band_nw", nw)
        assert m.single_launch_workgroups(1) == nw
        for nb in (1, 3):
            for o, r in zip(m.run(x[:nb]), refs):
                _raw_close(o, r[:nb])
        if name == "iris":
            continue   # (16 workgroups: four two-row tiles of 32x32x64 do not fit the LDS, the program ends in front of the first 2x2 convolution again)
        for o, o1 in zip(m.run(x[:1]), one):   # the band height does not enter a pixel's arithmetic
            np.testing.assert_array_equal(o, o1)
    if name == "iris":
        # the second branch behind the 8x8 fork on the workgroups the first one leaves idle (the default), or both branches one after the
        # other on the same workgroups: who computes a pixel does not enter its arithmetic
        m.set_option("band_nw", 32)
        forked = [o.copy() for o in m.run(x[:3])]
        m.set_option("band_fork", 0)
        for o, o1 in zip(m.run(x[:3]), forked):
            np.testing.assert_array_equal(o, o1)
        m.set_option("band_fork", 1)
    m.set_option("band", 1)   # the default: only the single-image entries take it
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x[:1]).cuda(), reps=1)]
    assert "bandnet_kernel" not in labels, labels
    m.close()


def test_every_shipped_graph_has_a_single_launch_program(gpu):
    """Round 6: full_range and full_range_sparse have one too (the trunk, through the 6x6 run, to the first lateral convolution of the decoder); with
    option band_wide = 0 their programs end in front of the first tensor of more than 128 channels."""
    for name in MODEL_FILES:
        m = gpu.Model(model_path(name))
        assert m.single_launch_workgroups(1) > 0, name
        m.close()


def test_single_image_entry_on_the_single_launch_plan(gpu, oracle, gold, man_image):
    """mi_fd_infer_image (one Mat per call, face_detection.rs:205) takes the single-launch plan: the same detections as a handle with the
    plan turned off, a run that reports it gave up is repeated on the batched plan, and handles on several threads share the device's CUs
    (256 CUs, 128 workgroups per BackCamera call: the third concurrent call runs on the batched plan instead of waiting)."""
    import threading
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    assert fd.model.single_launch_workgroups(1) == 128
    off = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    off.model.set_option("band", 0)
    assert off.model.single_launch_workgroups(1) == 0
    want = off.infer(man_image, None)
    assert len(want) >= 1

    ref = gold["man_back_dets"]   # the oracle's detections on man.jpg (tests/test_pins.py asserts golden.npz equal to the oracle's run)

    def same(got):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.abs(g.data - w.data).max() <= 1e-5 and abs(g.score - w.score) <= 1e-5
        for g, r in zip(got, ref):     # ... and against the oracle itself, at the detector tolerance
            np.testing.assert_allclose(np.concatenate([g.data.reshape(-1), [g.score]]), r, atol=2e-5)

    same(fd.infer(man_image, None))
    fd.model.set_option("band_test_fail", 1)   # the next single launch "gives up": the call must repeat itself on the batched plan
    same(fd.infer(man_image, None))
    same(fd.infer(man_image, None))
    errors = []

    def worker():
        try:
            h = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
            for _ in range(40):
                same(h.infer(man_image, None))
            h.close()
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker) for _ in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    fd.close()
    off.close()


def test_single_launch_plan_with_absent_workgroups_drains_fast_and_turns_itself_off(gpu, man_image):
    """a single launch whose workgroups are not all resident.  Engine option "band_test_absent" = k makes every k-th
    workgroup of the launch leave at once WITHOUT publishing its halo packets, so its neighbours really poll packets that never come (not the
    host-side band_test_fail hook).  The call must (a) return the batched plan's detections, (b) drain in milliseconds — one bounded wait for
    the whole launch, not one per stage (round 5: 2^18 polls per stage, ~0.3 s x 42 stages) — and (c) after three such calls in a row the
    handle stops using the plan ("band" reads 0).  With option band = 2 (no caller asks band_failed()) the run is checked inside run_device and
    repeated, so Model.run never returns the void results.  The packet tags' wrap at 2^26 launches is forced through "band_test_gen"."""
    import time
    off = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    off.model.set_option("band", 0)
    want = off.infer(man_image)
    assert len(want) >= 1
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    got = fd.infer(man_image)                                # a good single launch first
    assert fd.model.get_option("band") == 1 and fd.model.get_option("band_fail_streak") == 0
    same = lambda a, b: len(a) == len(b) and all(np.allclose(x.data, y.data, atol=1e-4) and abs(x.score - y.score) < 1e-5 for x, y in zip(a, b))
    assert same(got, want)
    fd.model.set_option("band_test_absent", 4)
    times = []
    for k in range(3):
        t0 = time.perf_counter()
        got = fd.infer(man_image)
        times.append(time.perf_counter() - t0)
        assert same(got, want), k
        assert fd.model.get_option("band_fail_streak") == k + 1 or k == 2
    assert times[0] < 1.0 and max(times[1:]) < 0.06, times   # one bounded wait (a few ms) + the batched plan (built by the first of them); the old form: seconds
    assert fd.model.get_option("band") == 0                  # three in a row: the handle has stopped trying
    t0 = time.perf_counter()
    assert same(fd.infer(man_image), want)
    assert time.perf_counter() - t0 < 0.02
    fd.close()
    # band = 2: every small run takes the single launch; a launch that gave up is repeated inside the call
    m = gpu.Model(model_path("back"))
    x = seeded_input("back", 2, 77, m.input_dims[1:3])
    m.set_option("band", 0)
    ref = [o.copy() for o in m.run(x)]
    m.set_option("band", 2)
    for o, r in zip(m.run(x), ref):
        _raw_close(o, r)
    m.set_option("band_test_absent", 3)
    for o, r in zip(m.run(x), ref):
        _raw_close(o, r)
    m.set_option("band_test_absent", 0)
    # the tags wrap: host count forced to the clearing threshold, device generation moved two launches in front of 2^26
    m.set_option("band_test_gen", (1 << 26) - 4096 - 1)
    for _ in range(6):
        for o, r in zip(m.run(x), ref):
            _raw_close(o, r)
    assert m.get_option("band_wraps") == 1
    m.close()
    off.close()


def test_mesh_and_iris_single_image_entries_on_threads(gpu, gold, man_image):
    """FaceLandmark::infer / IrisLandmark::infer (face_landmark.rs:232, iris_landmark.rs:158) on the single-launch plan from eight threads, a
    handle each: 96 / 32 workgroups per call on 256 CUs — calls that do not get their CUs run on the batched plan instead (never wait), a forced
    give-up repeats itself there; every call returns the landmarks of a handle with the plan turned off, within the tolerance between the two plans."""
    import threading
    face = gpu.Rect(*[float(v) for v in gold["man_face_roi"][:5]], int(gold["man_face_roi"][5]))
    eye = gpu.Rect(*[float(v) for v in gold["man_eye_left_roi"][:5]], int(gold["man_eye_left_roi"][5]))
    fl_off, ir_off = gpu.FaceLandmark(), gpu.IrisLandmark()
    fl_off.model.set_option("band", 0)
    ir_off.model.set_option("band", 0)
    want_lm = fl_off.infer(man_image, face).array
    want_eye = ir_off.infer(man_image, eye, False)
    assert len(want_lm) == 468

    def same(lm, eyes):
        # against the ORACLE's values for the same ROIs (golden.npz, asserted equal to the oracle's run by tests/test_pins.py), at the landmark
        # tolerance of the batched plan's tests — not only against the other plan ...
        np.testing.assert_allclose(lm.array, gold["man_face_landmarks"], atol=2e-5)
        np.testing.assert_allclose(eyes.contour.array, gold["man_eye_left_contour"], atol=2e-5)
        np.testing.assert_allclose(eyes.iris.array, gold["man_eye_left_iris"], atol=2e-5)
        # ... and against the batched plan of this build (the two plans differ by re-association only)
        np.testing.assert_allclose(lm.array, want_lm, atol=2e-5)
        np.testing.assert_allclose(eyes.contour.array, want_eye.contour.array, atol=2e-5)
        np.testing.assert_allclose(eyes.iris.array, want_eye.iris.array, atol=2e-5)

    fl, ir = gpu.FaceLandmark(), gpu.IrisLandmark()
    assert fl.model.single_launch_workgroups(1) == 96 and ir.model.single_launch_workgroups(1) == 32
    same(fl.infer(man_image, face), ir.infer(man_image, eye, False))
    fl.model.set_option("band_test_fail", 1)
    ir.model.set_option("band_test_fail", 1)
    same(fl.infer(man_image, face), ir.infer(man_image, eye, False))
    errors = []

    def worker():
        try:
            a, b = gpu.FaceLandmark(), gpu.IrisLandmark()
            for _ in range(25):
                same(a.infer(man_image, face), b.infer(man_image, eye, False))
            a.close()
            b.close()
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:3]
    for h in (fl, ir, fl_off, ir_off):
        h.close()


@pytest.mark.parametrize("name", ["back", "landmark", "iris", "full"])
def test_network_matches_committed_golden(gpu, gold, name):
    m = gpu.Model(model_path(name))
    x = seeded_input(name, 2, 1234, m.input_dims[1:3])
    for k, o in enumerate(m.run(x)):
        _raw_close(o.reshape(2, -1), gold["noise_%s_out%d" % (name, k)])
    m.close()


def test_chunking_graph_and_batch_invariance(gpu):
    """Frames are independent: any chunking / hipGraph replay / batch position gives bit-identical results."""
    m = gpu.Model(model_path("front"))
    x = seeded_input("front", 13, 5, m.input_dims[1:3])
    base = [o.copy() for o in m.run(x)]
    for chunk, graph in ((4, 0), (4, 1), (0, 1), (1, 0)):
        m.set_option("chunk", chunk)
        m.set_option("graph", graph)
        for rep in range(2):
            for a, b in zip(m.run(x), base):
                np.testing.assert_array_equal(a, b)
    # frame 7 alone == frame 7 inside the batch
    for a, b in zip(m.run(x[7:8]), base):
        np.testing.assert_array_equal(a[0], b[7])
    # frame ranges on concurrent streams ("lanes"), captured into one hipGraph and eager (regression: sharing the output-head
    # side streams between concurrently captured lanes crashed graph capture)
    m.set_option("chunk", 0)
    for lanes, graph in ((2, 1), (3, 1), (2, 0)):
        m.set_option("lanes", lanes)
        m.set_option("graph", graph)
        for rep in range(2):
            for a, b in zip(m.run(x), base):
                np.testing.assert_array_equal(a, b)
    m.close()


def test_device_pointer_path_matches_host_path(gpu):
    torch = pytest.importorskip("torch")
    m = gpu.Model(model_path("back"))
    x = seeded_input("back", 3, 11, m.input_dims[1:3])
    host = m.run(x)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    dev = m.run(xd)
    torch.cuda.synchronize()
    for a, b in zip(host, dev):
        np.testing.assert_array_equal(a, b.cpu().numpy())
    m.close()


def test_postprocess_bit_exact_vs_oracle(gpu, oracle, gold):
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    np.testing.assert_array_equal(fd.anchors(), gold["anchors_back"])
    out, counts = fd.postprocess(gold["nms_raw_boxes"], gold["nms_raw_scores"], gold["nms_pads"], cap=256)
    for f in range(4):
        ref = gold["nms_dets_%d" % f]
        assert counts[f] == len(ref)
        got = out[f, : len(ref)]
        # score differs only through the device expf; everything else is the same IEEE operation sequence
        np.testing.assert_allclose(got[:, 16], ref[:, 16], rtol=3e-7)
        np.testing.assert_allclose(got[:, :16], ref[:, :16], rtol=0, atol=2e-6)
    fd.close()


def test_postprocess_edge_cases(gpu, oracle):
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    anchors = fd.anchors()
    rb = np.zeros((3, 896, 16), np.float32)
    rb[:, :, 2:4] = 30.0
    sc = np.full((3, 896), -10.0, np.float32)
    sc[1, 100] = 4.0            # single detection
    sc[2, 100] = 1e-9           # sigmoid rounds to exactly 0.5 -> dropped
    out, counts = fd.postprocess(rb, sc, None, cap=8)
    assert list(counts) == [0, 1, 0]
    ref = oracle.fd_postprocess(rb[1], sc[1], anchors, 256.0)
    np.testing.assert_allclose(out[1, 0], ref[0], atol=1e-7)
    # capacity smaller than the number of outputs: count still reports all of them
    sc2 = np.full((1, 896), 5.0, np.float32)
    rb2 = np.zeros((1, 896, 16), np.float32)
    rb2[:, :, 2:4] = 4.0        # tiny boxes on distinct anchors -> no merging between cells
    out2, counts2 = fd.postprocess(rb2, sc2, None, cap=4)
    ref2 = oracle.fd_postprocess(rb2[0], sc2[0], anchors, 256.0)
    assert counts2[0] == len(ref2) and counts2[0] > 4
    np.testing.assert_allclose(out2[0], ref2[:4], atol=1e-6)
    # the reference's letterbox assert -> MI_ERANGE
    with pytest.raises(gpu.MiError) as e:
        fd.postprocess(rb2, sc2, np.array([[0.5, 0, 0.5, 0]]), cap=4)
    assert e.value.code == -5
    fd.close()


KINDS = [("BackCamera", "back"), ("FrontCamera", "front"), ("Short", "short"), ("Full", "full"), ("FullSparse", "sparse")]
ORC_KIND = {"back": "FD_BACK", "front": "FD_FRONT", "short": "FD_SHORT", "full": "FD_FULL", "sparse": "FD_FULL_SPARSE"}


@pytest.mark.parametrize("kind,name", KINDS)
def test_detector_tensor_path_vs_oracle(gpu, oracle, man_image, kind, name):
    """Config 2 shape at test size, for every detector: face-bearing frames (the letterboxed man.jpg tensor at the model's own
    resolution, shifted / dimmed copies, two faces side by side) + noise frames through net + decode (scale = 256 / 128 / 192,
    true division) + sigmoid + weighted NMS at N = 896 / 2304, compared with the oracle detection by detection."""
    fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
    om = oracle.Model(model_path(name))
    W, H = fd.input_size
    face, _pad = oracle.image_to_tensor(man_image, None, (W, H), True, (-1., 1.), False)
    x = seeded_input(name, 8, 77, (H, W)) * 0.25
    x[0] = face
    x[2] = np.roll(face, (H // 28, -W // 18), axis=(0, 1))
    x[3] = np.clip(np.roll(face, (-H // 12, W // 10), axis=(0, 1)) * 0.9, -1, 1)
    x[5] = face[:, ::-1]
    two = np.full_like(face, -1.0)                      # two half-size faces in one frame: several heads survive NMS
    half = face[::2, ::2]
    two[: H // 2, : W // 2] = half
    two[H // 2:, W // 2:] = half[:, ::-1]
    x[6] = two
    out, counts = fd.infer_tensor(x, cap=32)
    rb, rs = om.run(x, nthreads=8)
    anchors = oracle.ssd_anchors(getattr(oracle, ORC_KIND[name]))
    total, merged = 0, 0
    for f in range(8):
        ref = oracle.fd_postprocess(rb[f], rs[f], anchors, float(H))
        assert counts[f] == len(ref), "frame %d: %d vs %d" % (f, counts[f], len(ref))
        total += len(ref)
        merged += int((1.0 / (1.0 + np.exp(-np.clip(rs[f].reshape(-1), -80, 80))) > 0.5).sum())
        for g, r in zip(out[f, : len(ref)], ref):
            assert _iou(g[:4], r[:4]) >= 0.999
            np.testing.assert_allclose(g, r, atol=2e-5)
    assert total >= 3, total                  # every kind sees real faces ...
    assert merged > total                     # ... and merges several candidates per face (weighted NMS does work)
    fd.close()


@pytest.mark.parametrize("kind,name", KINDS)
def test_detector_on_man_jpg_vs_oracle(gpu, oracle, man_image, kind, name):
    """configs[0] (FaceDetectionModel::Short on test_data/man.jpg, single image) and the same call for every other model type:
    FaceDetection::infer(&Mat, None) through mi_fd_infer_image — device image_to_tensor (letterbox to 128 / 192 / 256) + net +
    decode + NMS + letterbox removal — against the oracle's restatement of the same call.  The reference's TFLite path cannot
    run here: the oracle stands in for it."""
    H, W = man_image.shape[:2]
    fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
    faces = fd.infer(man_image, None)
    iw, ih = fd.input_size
    t, pad = oracle.image_to_tensor(man_image, None, (iw, ih), True, (-1., 1.), False)
    rb, rs = oracle.Model(model_path(name)).run(t[None])
    ref = oracle.fd_postprocess(rb[0], rs[0], oracle.ssd_anchors(getattr(oracle, ORC_KIND[name])), float(ih), pad)
    assert len(faces) == len(ref) >= 1
    for f, r in zip(faces, ref):                       # same order (descending head score)
        got = np.concatenate([f.data.reshape(-1), [f.score]])
        assert _iou(got[:4], r[:4]) >= 0.999
        np.testing.assert_allclose(got, r, atol=2e-5)
    # the face is where the reference's rendering has it (BackCamera bbox 195,74 139x139): centre within a few pixels
    xmin, ymin, xmax, ymax = faces[0].bbox()
    assert abs((xmin + xmax) / 2 * W - 264.5) < 8 and abs((ymin + ymax) / 2 * H - 143.5) < 8
    # an ROI (Option<Rect>): the left half of the picture holds no complete face for the short-range models
    roi = gpu.Rect(0.5, 0.5, 0.9, 0.9, 0.0, 1)
    faces_roi = fd.infer(man_image, roi)
    t, pad = oracle.image_to_tensor(man_image, oracle.Rect(0.5, 0.5, 0.9, 0.9, 0.0, 1), (iw, ih), True, (-1., 1.), False)
    rb, rs = oracle.Model(model_path(name)).run(t[None])
    ref = oracle.fd_postprocess(rb[0], rs[0], oracle.ssd_anchors(getattr(oracle, ORC_KIND[name])), float(ih), pad)
    assert len(faces_roi) == len(ref)
    for f, r in zip(faces_roi, ref):
        np.testing.assert_allclose(np.concatenate([f.data.reshape(-1), [f.score]]), r, atol=2e-5)
    fd.close()


def test_fd_infer_images_batch_vs_oracle_and_tensor_path(gpu, oracle, gold, man_image):
    """Batched u8 detector entry (mi_fd_infer_images; FaceDetection::infer over a batch of Mats, face_detection.rs:205-267 with the
    u8 -> f32 loop of transform.rs:292-301 on the device).  (a) 256 model-size frames (8 distinct u8 frames x 32, shuffled): copies
    bit-equal, the result equal to the tensor entry fed with the ORACLE's image_to_tensor of the same frames (device pre-processing is
    bit-exact, so the two paths must agree bit for bit), the 8 originals against the oracle's whole call.  (b) frames of another size
    (man.jpg, letterboxed) with one ROI per frame — the 26-ROI style set of test_image_to_tensor_vs_oracle — against the oracle
    detection by detection.  (c) device frames (torch uint8) equal host frames."""
    torch = pytest.importorskip("torch")
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    rs = np.random.RandomState(31)
    face = gold["man_back_u8"].astype(np.uint8)
    base = np.stack([face, face[:, ::-1].copy(), np.roll(face, (28, -21), axis=(0, 1)), (face * 0.8).astype(np.uint8)] +
                    [rs.randint(0, 256, face.shape).astype(np.uint8) for _ in range(4)])
    order = rs.permutation(256) % 8
    frames = np.ascontiguousarray(base[order])
    out, counts = fd.infer_images(frames, cap=16)
    first = {int(k): int(np.where(order == k)[0][0]) for k in range(8)}
    for i in range(256):
        j = first[int(order[i])]
        assert counts[i] == counts[j]
        np.testing.assert_array_equal(out[i, : counts[i]], out[j, : counts[j]])
    tens = np.stack([oracle.image_to_tensor(b, None, (256, 256), True, (-1., 1.), False)[0] for b in base])
    out_t, counts_t = fd.infer_tensor(np.ascontiguousarray(tens[order]), cap=16)
    np.testing.assert_array_equal(counts, counts_t)
    np.testing.assert_array_equal(out, out_t)
    om = oracle.Model(model_path("back"))
    rb, rsc = om.run(tens, nthreads=8)
    anchors = oracle.ssd_anchors(oracle.FD_BACK)
    found = 0
    for k in range(8):
        want = oracle.fd_postprocess(rb[k], rsc[k], anchors, 256.0)
        j = first[k]
        assert counts[j] == len(want)
        if len(want):
            np.testing.assert_allclose(out[j, : len(want)], want, atol=2e-5)
            found += 1
    assert found >= 3
    # (c) the same frames already in device memory
    out_d, counts_d = fd.infer_images(torch.from_numpy(frames).cuda(), cap=16)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_d.cpu().numpy(), out)
    np.testing.assert_array_equal(counts_d.cpu().numpy(), counts)
    # (b) another frame size, one ROI per frame
    rois = [None, np.array([0.5, 0.5, 0.9, 0.9, 0.0, 1]), np.array([300.0, 150.0, 333.0, 217.0, -0.7, 0]), np.array([0.5, 0.4, 0.6, 0.7, 0.3, 1]),
            np.array([0.05, 0.1, 0.5, 0.45, 2.4, 1])]
    for k in range(8):
        rois.append(np.array([rs.uniform(0.3, 0.7), rs.uniform(0.3, 0.7), rs.uniform(0.3, 0.9), rs.uniform(0.3, 0.9), rs.uniform(-3.1, 3.1), 1]))
    H, W = man_image.shape[:2]
    full = np.array([0.5, 0.5, 1.0, 1.0, 0.0, 1])
    batch = np.ascontiguousarray(np.stack([man_image] * len(rois)))
    grects = [gpu.Rect(*[float(v) for v in (r if r is not None else full)[:5]], int((r if r is not None else full)[5])) for r in rois]
    out_r, counts_r = fd.infer_images(batch, rois=grects, cap=16)
    for k, r in enumerate(rois):
        o = oracle.Rect(*[float(v) for v in r[:5]], int(r[5])) if r is not None else oracle.Rect(0.5, 0.5, 1.0, 1.0, 0.0, 1)
        t, pad = oracle.image_to_tensor(man_image, o, (256, 256), True, (-1., 1.), False)
        rbk, rsk = om.run(t[None])
        want = oracle.fd_postprocess(rbk[0], rsk[0], anchors, 256.0, pad)
        assert counts_r[k] == len(want), (k, counts_r[k], len(want))
        if len(want):
            np.testing.assert_allclose(out_r[k, : len(want)], want, atol=2e-5)
    assert counts_r[0] >= 1
    fd.close()


@pytest.mark.parametrize("kind,name,size", [("Short", "short", 128), ("Full", "full", 192), ("FullSparse", "full_sparse", 192)])
def test_fd_infer_images_u8_stem_other_detectors(gpu, oracle, gold, kind, name, size):
    """The u8 form of the first convolution (bytes normalised through a 256-entry table while the tile is filled) for the other
    detectors' stems (5x5 -> 24 at 128^2, 3x3 -> 32 at 192^2): frames of the network's own size through mi_fd_infer_images equal, bit
    for bit, the tensor entry fed with the oracle's image_to_tensor of the same frames; 37 frames (a partial last tile of workgroups)."""
    fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
    rs = np.random.RandomState(size)
    base = gold["man_back_u8"].astype(np.uint8)
    if size == 128:
        base = base.reshape(128, 2, 128, 2, 3).mean(axis=(1, 3)).astype(np.uint8)
    else:
        base = np.ascontiguousarray(base[32:224, 32:224])
    frames = np.stack([np.roll(base, (int(rs.randint(-9, 10)), int(rs.randint(-9, 10))), axis=(0, 1)) if i % 3 else rs.randint(0, 256, base.shape).astype(np.uint8)
                       for i in range(37)])
    out, counts = fd.infer_images(frames, cap=16)
    tens = np.stack([oracle.image_to_tensor(f, None, (size, size), True, (-1., 1.), False)[0] for f in frames])
    out_t, counts_t = fd.infer_tensor(tens, cap=16)
    np.testing.assert_array_equal(counts, counts_t)
    np.testing.assert_array_equal(out, out_t)
    assert int((counts > 0).sum()) >= 12
    fd.close()


def test_fd_submit_collect_two_slots(gpu, gold):
    """Host feed in two slots (mi_fd_submit_images / mi_fd_collect): four batches of pinned u8 frames alternate between the slots, the
    copy of one overlapping the kernels of the other; every batch equals the synchronous entry's result.  A slot cannot be submitted
    twice without a collect, nor collected when empty."""
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    rs = np.random.RandomState(5)
    face = gold["man_back_u8"].astype(np.uint8)
    pins = [gpu.PinnedBuffer((48, 256, 256, 3)) for _ in range(2)]
    batches = []
    for b in range(4):
        fr = np.stack([np.roll(face, (int(rs.randint(-30, 30)), int(rs.randint(-30, 30))), axis=(0, 1)) if i % 3 else rs.randint(0, 256, face.shape).astype(np.uint8)
                       for i in range(48)])
        batches.append(fr)
    want = [fd.infer_images(fr, cap=8) for fr in batches]
    got = [None] * 4
    pins[0].array[...] = batches[0]
    fd.submit_images(0, pins[0].array, cap=8)
    with pytest.raises(gpu.MiError):
        fd.submit_images(0, pins[0].array, cap=8)
    for b in range(1, 4):
        pins[b & 1].array[...] = batches[b]            # fill the other slot's frames while the previous batch runs
        fd.submit_images(b & 1, pins[b & 1].array, cap=8)
        got[b - 1] = fd.collect((b - 1) & 1)
    got[3] = fd.collect(1)
    with pytest.raises(KeyError):
        fd.collect(1)
    for (o, c), (wo, wc) in zip(got, want):
        np.testing.assert_array_equal(c, wc)
        np.testing.assert_array_equal(o, wo)
    assert sum(int((c > 0).sum()) for _, c in got) >= 64
    # a handle freed with a batch still in flight waits for it (its kernels write into the slot's pinned results)
    pins[0].array[...] = batches[0]
    fd.submit_images(0, pins[0].array, cap=8)
    fd.close()
    for p in pins:
        p.close()


def test_landmark_tensor_path_vs_oracle(gpu, oracle, gold):
    fl = gpu.FaceLandmark()
    om = oracle.Model(model_path("landmark"))
    x = seeded_input("landmark", 4, 3, (192, 192))
    x[1] = gold["man_face_u8"].astype(np.float32) / np.float32(255.0)
    g = gold["man_face_roi"]
    roi = gpu.Rect(*[float(v) for v in g[:5]], int(g[5]))
    rois = [roi, roi, gpu.Rect(270.0, 180.0, 200.0, 210.0, 0.3, 0), gpu.Rect(0.5, 0.5, 1.0, 1.0, 0.0, 1)]
    sizes = [(540, 360)] * 4
    lm, present, flags = fl.infer_tensor(x, rois=rois, image_sizes=sizes)
    raw, flag = om.run(x, nthreads=4)
    for f in range(4):
        _raw_close(flags[f:f + 1], flag[f].reshape(-1)[-1:])
        assert present[f] == oracle.lib().orc_face_flag_passes(float(flag[f].reshape(-1)[-1]))
        oroi = oracle.Rect(rois[f].x_center, rois[f].y_center, rois[f].width, rois[f].height, rois[f].rotation, rois[f].normalized)
        ref = oracle.project_landmarks(raw[f], (192, 192), sizes[f], roi=oroi)
        np.testing.assert_allclose(lm[f], ref, atol=1e-5 * max(1.0, float(np.abs(ref).max())))
    assert present[1] == 1
    np.testing.assert_allclose(lm[1], gold["man_face_landmarks"], atol=1e-5)
    # no ROI: plain normalisation
    lm2, _, _ = fl.infer_tensor(x[:2])
    ref = oracle.project_landmarks(raw[0], (192, 192), (1, 1))
    np.testing.assert_allclose(lm2[0], ref, atol=1e-5 * max(1.0, float(np.abs(ref).max())))
    fl.close()


def test_iris_tensor_path_vs_oracle(gpu, oracle, gold):
    ir = gpu.IrisLandmark()
    x = np.stack([gold["man_eye_right_u8"], gold["man_eye_left_u8"]]).astype(np.float32) / np.float32(255.0)
    rois, pads = [], []
    for tag in ("right", "left"):
        g = gold["man_eye_%s_roi" % tag]
        rois.append(gpu.Rect(*[float(v) for v in g[:5]], int(g[5])))
        pads.append(gold["man_eye_%s_pad" % tag])
    contour, iris = ir.infer_tensor(x, rois=rois, image_sizes=[(540, 360)] * 2, padding=np.array(pads), is_right_eye=[1, 0])
    for k, tag in enumerate(("right", "left")):
        np.testing.assert_allclose(contour[k], gold["man_eye_%s_contour" % tag], atol=1e-5)
        np.testing.assert_allclose(iris[k], gold["man_eye_%s_iris" % tag], atol=1e-5)
    ir.close()


def test_image_to_tensor_vs_oracle(gpu, oracle, gold, man_image):
    """Device pre-processing is byte work: bit-exact with the oracle's restatement of
    transform.rs:188-309 + OpenCV's 8-bit fixed-point warp / resize, for letterboxed, rotated, flipped, off-image and
    non-normalised ROIs, square and non-square sources."""
    rs = np.random.RandomState(21)
    tall = rs.randint(0, 256, (300, 171, 3)).astype(np.uint8)          # portrait source: pads left / right
    cases = [
        (man_image, None, (256, 256), True, (-1., 1.), False),
        (man_image, None, (128, 128), True, (-1., 1.), False),
        (man_image, None, (192, 192), True, (-1., 1.), False),
        (man_image, gold["man_face_roi"], (192, 192), False, (0., 1.), False),
        (man_image, gold["man_eye_right_roi"], (64, 64), True, (0., 1.), True),
        (man_image, gold["man_eye_left_roi"], (64, 64), True, (0., 1.), False),
        (man_image, np.array([300.0, 150.0, 333.0, 217.0, -0.7, 0]), (192, 192), True, (0., 1.), False),
        (man_image, np.array([0.5, 0.5, 0.4, 0.6, 0.2, 1]), (192, 192), False, (0., 1.), False),
        (man_image, np.array([0.05, 0.1, 0.5, 0.45, 2.4, 1]), (64, 64), True, (0., 1.), True),      # mostly outside the picture
        (man_image, np.array([0.5, 0.5, 0.3556, 0.5333, 0.0, 1]), (192, 192), True, (-1., 1.), False),  # 192 x 192 px: resize = copy
        (tall, None, (256, 256), True, (-1., 1.), False),
        (tall, None, (128, 128), True, (0., 1.), True),
        (tall, np.array([0.4, 0.6, 0.7, 0.5, -1.1, 1]), (192, 192), False, (0., 1.), False),
    ]
    for k in range(12):                                                  # seeded random ROIs
        r = np.array([rs.uniform(0.2, 0.8), rs.uniform(0.2, 0.8), rs.uniform(0.1, 0.9), rs.uniform(0.1, 0.9), rs.uniform(-3.1, 3.1), 1])
        cases.append((man_image if k % 2 else tall, r, [(64, 64), (192, 192), (256, 256)][k % 3], bool(k % 4 < 2), (0., 1.), bool(k % 5 == 0)))
    for img, roi, size, keep, rng, flip in cases:
        r = gpu.Rect(*[float(v) for v in roi[:5]], int(roi[5])) if roi is not None else None
        o = oracle.Rect(*[float(v) for v in roi[:5]], int(roi[5])) if roi is not None else None
        got, pad = gpu.image_to_tensor(img, r, size, keep, rng, flip)
        ref, rpad = oracle.image_to_tensor(img, o, size, keep, rng, flip)
        assert tuple(pad) == tuple(rpad)
        np.testing.assert_array_equal(got, ref, err_msg="roi %s size %s keep %s flip %s" % (roi, size, keep, flip))
    # a strided view (cv::Mat ROI): rows `stride` bytes apart, the last row owns only 3 * width bytes
    view = man_image[40:300, 100:420]
    got, _ = gpu.image_to_tensor(view, None, (128, 128), True, (-1., 1.), False)
    ref, _ = oracle.image_to_tensor(np.ascontiguousarray(view), None, (128, 128), True, (-1., 1.), False)
    np.testing.assert_array_equal(got, ref)


def test_single_image_entries_copy_every_row_the_warp_samples(gpu, gold, man_image):
    """FaceLandmark::infer / IrisLandmark::infer with a ROI (face_landmark.rs:250, iris_landmark.rs:188) send only the source rows the warp
    can sample to the device.  A handle whose picture buffer holds the INVERTED picture in every row (a call without ROI uploads all rows)
    must give, bit for bit, what a handle whose buffer holds the picture itself gives: a sampled row outside the copied range would be read
    from the stale contents.  Upright, rotated, tiny and mostly-off-picture ROIs."""
    poison = np.ascontiguousarray(255 - man_image)
    rs = np.random.RandomState(5)
    rois = [gold["man_face_roi"], gold["man_eye_left_roi"], gold["man_eye_right_roi"],
            np.array([0.5, 0.02, 0.3, 0.2, 0.0, 1]), np.array([0.5, 0.98, 0.3, 0.2, 3.0, 1]),           # over the top / bottom edge
            np.array([0.05, 0.1, 0.5, 0.45, 2.4, 1]), np.array([270.0, 180.0, 40.0, 30.0, 0.785, 0]),   # mostly outside; pixels, 45 degrees
            np.array([0.5, 0.5, 0.01, 0.01, 0.3, 1])]                                                    # a few pixels
    for k in range(10):
        rois.append(np.array([rs.uniform(0.1, 0.9), rs.uniform(0.0, 1.0), rs.uniform(0.02, 0.9), rs.uniform(0.02, 0.9), rs.uniform(-3.1, 3.1), 1]))
    fresh, stale = gpu.IrisLandmark(), gpu.IrisLandmark()
    fresh_fl, stale_fl = gpu.FaceLandmark(), gpu.FaceLandmark()
    for roi in rois:
        r = gpu.Rect(*[float(v) for v in roi[:5]], int(roi[5]))
        for right in (False, True):
            fresh.infer(man_image, None, right)
            stale.infer(poison, None, right)
            a, b = fresh.infer(man_image, r, right), stale.infer(man_image, r, right)
            np.testing.assert_array_equal(a.contour.array, b.contour.array, err_msg="iris roi %s" % roi)
            np.testing.assert_array_equal(a.iris.array, b.iris.array, err_msg="iris roi %s" % roi)
        fresh_fl.infer(man_image, None)
        stale_fl.infer(poison, None)
        a, b = fresh_fl.infer(man_image, r), stale_fl.infer(man_image, r)
        np.testing.assert_array_equal(a.array, b.array, err_msg="mesh roi %s" % roi)
    # a strided view (cv::Mat ROI: rows `stride` bytes apart, the last row owns only 3 * width bytes) — the copied range is cut out of it
    view, pview = man_image[40:300, 100:420], poison[40:300, 100:420]
    for roi in rois[:8]:
        r = gpu.Rect(*[float(v) for v in roi[:5]], int(roi[5]))
        if not r.normalized:
            continue
        fresh.infer(view, None, False)
        stale.infer(pview, None, False)
        a, b = fresh.infer(view, r, False), stale.infer(view, r, False)
        np.testing.assert_array_equal(a.contour.array, b.contour.array, err_msg="view, iris roi %s" % roi)
        c = fresh.infer(np.ascontiguousarray(view), r, False)
        np.testing.assert_array_equal(a.contour.array, c.contour.array, err_msg="view against its contiguous copy, roi %s" % roi)
    for h in (fresh, stale, fresh_fl, stale_fl):
        h.close()


def test_fl_and_iris_infer_images_vs_tensor_entries(gpu, oracle, gold, man_image):
    """Round 5: mi_fl_infer_images / mi_iris_infer_images take the frames as the reference's callers hold them (8UC3) plus one ROI (and
    is_right_eye) per item and warp on the device (face_landmark.rs:250, iris_landmark.rs:188-189).  On the 25-ROI set of
    test_image_to_tensor_vs_oracle (rotated, off-image, non-normalised ROIs on a landscape and a portrait source) the results equal
    the tensor entries fed with the ORACLE's image_to_tensor crops of the same items bit for bit; several items per frame, host and
    device memory, whole frames (roi = None)."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(21)
    tall = rs.randint(0, 256, (300, 171, 3)).astype(np.uint8)
    rois = [gold["man_face_roi"], gold["man_eye_right_roi"], gold["man_eye_left_roi"], np.array([300.0, 150.0, 333.0, 217.0, -0.7, 0]),
            np.array([0.5, 0.5, 0.4, 0.6, 0.2, 1]), np.array([0.05, 0.1, 0.5, 0.45, 2.4, 1]), np.array([0.5, 0.5, 0.3556, 0.5333, 0.0, 1]),
            np.array([0.4, 0.6, 0.7, 0.5, -1.1, 1])]
    for k in range(17):
        rois.append(np.array([rs.uniform(0.2, 0.8), rs.uniform(0.2, 0.8), rs.uniform(0.1, 0.9), rs.uniform(0.1, 0.9), rs.uniform(-3.1, 3.1), 1]))
    assert len(rois) == 25
    fl, iris = gpu.FaceLandmark(), gpu.IrisLandmark()
    for img in (man_image, tall):
        H, W = img.shape[:2]
        G = [gpu.Rect(*[float(v) for v in r[:5]], int(r[5])) for r in rois]
        O = [oracle.Rect(*[float(v) for v in r[:5]], int(r[5])) for r in rois]
        sizes = np.array([[W, H]] * 25, np.int32)
        # ---- face mesh: 5 frames (copies of the picture) x 5 ROIs each
        frames = np.stack([img] * 5)
        crops = np.stack([oracle.image_to_tensor(img, o, (192, 192), False, (0., 1.), False)[0] for o in O])
        want = fl.infer_tensor(crops, G, sizes)
        got = fl.infer_images(frames, G, items_per_frame=5)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        # a larger, uneven batch (7 frames x 10 ROIs)
        # (other layers of the net change kernels with the batch: tolerance, not bits, against the 25-item run)
        got70 = fl.infer_images(np.stack([img] * 7), (G * 3)[:70], items_per_frame=10)
        np.testing.assert_array_equal(got70[1], np.concatenate([want[1]] * 3)[:70])
        np.testing.assert_allclose(got70[0], np.concatenate([want[0]] * 3)[:70], atol=2e-5)
        np.testing.assert_allclose(got70[2], np.concatenate([want[2]] * 3)[:70], atol=1e-3, rtol=1e-4)
        assert got[1].sum() >= 1 or img is tall       # (the face ROI passes the flag; the portrait source is noise)
        # device memory: frames and ROIs resident, results left on the device
        roi_dev = torch.from_numpy(np.frombuffer(bytes((gpu.Rect * 25)(*G)), np.uint8).copy()).cuda()
        got_d = fl.infer_images(torch.from_numpy(frames).cuda(), roi_dev, items_per_frame=5)
        for a, b in zip(got_d, want):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
        # ---- iris: the same ROIs as eye crops, every third one a right eye (flipped in, x -> 1 - x out)
        flips = np.array([k % 3 == 0 for k in range(25)], np.int32)
        both = [oracle.image_to_tensor(img, o, (64, 64), True, (0., 1.), bool(f)) for o, f in zip(O, flips)]
        crops = np.stack([t for t, _ in both])
        pads = np.array([p for _, p in both], np.float64)
        want = iris.infer_tensor(crops, G, sizes, pads, flips)
        got = iris.infer_images(frames, G, flips, items_per_frame=5)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        # ---- whole frames (Option<Rect> = None), one item per frame
        want = fl.infer_tensor(np.stack([oracle.image_to_tensor(img, None, (192, 192), False, (0., 1.), False)[0]] * 2))
        got = fl.infer_images(frames[:2])
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        t, p = oracle.image_to_tensor(img, None, (64, 64), True, (0., 1.), False)
        want = iris.infer_tensor(np.stack([t] * 2), None, None, np.array([p, p], np.float64), None)
        got = iris.infer_images(frames[:2])
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
    fl.close()
    iris.close()


def test_fl_submit_collect_two_slots(gpu, gold, man_image):
    """mi_fl_submit_images / mi_fl_collect (round 5): the two-slot host feed of the face mesh, like the detector's.  Batches that
    alternate between the slots give what mi_fl_infer_images gives for the same frames and ROIs, bit for bit; protocol errors
    (collect before submit, submit on a pending slot) are MI_EINVAL."""
    fl = gpu.FaceLandmark()
    base = gold["man_face_roi"]
    rs = np.random.RandomState(4)
    def batch(k):
        frames = np.stack([np.roll(man_image, (int(rs.randint(-5, 6)), int(rs.randint(-5, 6))), axis=(0, 1)) for _ in range(3)])
        rois = []
        for i in range(3 * 4):
            r = base.copy(); r[0] += rs.uniform(-0.02, 0.02); r[4] += rs.uniform(-0.4, 0.4)
            rois.append(gpu.Rect(*[float(v) for v in r[:5]], int(r[5])))
        return frames, rois
    batches = [batch(k) for k in range(5)]
    want = [fl.infer_images(f, r, items_per_frame=4) for f, r in batches]
    pins = [gpu.PinnedBuffer(batches[0][0].shape) for _ in range(2)]
    import ctypes as C
    lm0, pr0 = np.zeros((12, 468, 3), np.float32), np.zeros((12,), np.int32)
    assert gpu.lib().mi_fl_collect(fl.h, 0, C.c_void_p(lm0.ctypes.data), C.c_void_p(pr0.ctypes.data), None) == -1   # MI_EINVAL: nothing was submitted
    got = []
    for k, (f, r) in enumerate(batches):
        pins[k & 1].array[...] = f
        fl.submit_images(k & 1, pins[k & 1].array, r, items_per_frame=4)
        if k == 0:
            with pytest.raises(gpu.MiError):
                fl.submit_images(0, pins[0].array, r, items_per_frame=4)      # slot 0 is pending
        if k >= 1:
            got.append(fl.collect((k - 1) & 1))
    got.append(fl.collect((len(batches) - 1) & 1))
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            np.testing.assert_array_equal(a, b)
    assert sum(int(g[1].sum()) for g in got) >= 50
    for p in pins:
        p.close()
    fl.close()


def test_full_pipeline_on_man_jpg(gpu, oracle, gold, man_image):
    """README.md:27-46 flow through the reference-shaped API; pinned by the reference's own rendering (+-2 px)."""
    H, W = man_image.shape[:2]
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    faces = fd.infer(man_image, None)
    assert len(faces) == 1
    ref = gold["man_back_dets"][0]
    got = np.concatenate([faces[0].data.reshape(-1), [faces[0].score]])
    assert _iou(got[:4], ref[:4]) >= 0.999
    np.testing.assert_allclose(got, ref, atol=2e-5)      # device pre-processing is bit-exact: tensor-path tolerance
    xmin, ymin, xmax, ymax = faces[0].bbox()
    assert int(xmin * W) == 195 and int(ymin * H) == 74 and int((xmax - xmin) * W) == 139 and int((ymax - ymin) * H) == 139
    roi = gpu.face_detection_to_roi(faces[0], (W, H))
    lms = gpu.FaceLandmark().infer(man_image, roi)
    assert len(lms) == 468
    arr = np.array([[l.x, l.y, l.z] for l in lms])
    np.testing.assert_allclose(arr, gold["man_face_landmarks"], atol=2e-5)
    left, right = gpu.iris_roi_from_face_landmarks(lms, (W, H))
    iris = gpu.IrisLandmark()
    r = iris.infer(man_image, right, True)
    l = iris.infer(man_image, left, False)
    assert len(r.contour) == 71 and len(r.iris) == 5 and len(l.eyeball_contour()) == 15
    # third stage of the chain: the eye ROIs come from the GPU's own mesh (<= 1e-5 off the oracle's), so the 64x64 crops can
    # differ in a few resampled pixels: 1e-4 normalised units (0.05 px of the 540 px picture) for the eye stage
    np.testing.assert_allclose(np.array([[p.x, p.y, p.z] for p in r.contour]), gold["man_eye_right_contour"], atol=1e-4)
    np.testing.assert_allclose(np.array([[p.x, p.y, p.z] for p in r.iris]), gold["man_eye_right_iris"], atol=1e-4)
    np.testing.assert_allclose(np.array([[p.x, p.y, p.z] for p in l.contour]), gold["man_eye_left_contour"], atol=1e-4)
    np.testing.assert_allclose(np.array([[p.x, p.y, p.z] for p in l.iris]), gold["man_eye_left_iris"], atol=1e-4)
    # ... and at the other stages' tolerance once the oracle's eye stage is given the SAME ROIs (the GPU's): what is left is the stage itself
    oir = oracle.Model(model_path("iris"))
    for res, rect, is_right in ((l, left, False), (r, right, True)):
        orect = oracle.Rect(rect.x_center, rect.y_center, rect.width, rect.height, rect.rotation, rect.normalized)
        t3, pad3 = oracle.image_to_tensor(man_image, orect, (64, 64), True, (0., 1.), is_right)
        c71, i5 = oir.run(t3[None])
        np.testing.assert_allclose(np.array([[p.x, p.y, p.z] for p in res.contour]), oracle.project_landmarks(c71[0], (64, 64), (W, H), pad3, orect, is_right), atol=2e-5)
        np.testing.assert_allclose(np.array([[p.x, p.y, p.z] for p in res.iris]), oracle.project_landmarks(i5[0], (64, 64), (W, H), pad3, orect, is_right), atol=2e-5)
    # the GPU results, drawn by the restated renderer, reproduce the reference's own PNGs pixel for pixel (lib.rs:43-83)
    from oracle import render
    from PIL import Image
    png = lambda name, col: render.colour_mask(np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGBA")), col)
    det_rows = np.array([np.concatenate([f.data.reshape(-1), [f.score]]) for f in faces])
    m = render.colour_mask(render.render_to_image(render.detections_to_render_data(det_rows, render.GREEN, None, 4, 2), man_image), render.GREEN)
    assert int((m ^ png("man_bbox.png", render.GREEN)).sum()) == 0
    m = render.colour_mask(render.render_to_image(render.face_landmarks_to_render_data(arr), man_image), render.RED)
    assert int((m ^ png("man_landmark.png", render.RED)).sum()) == 0
    eye = lambda res: np.array([[p.x, p.y, p.z] for p in res.eyeball_contour()])
    ann = render.eye_landmarks_to_render_data(eye(r)) + render.eye_landmarks_to_render_data(eye(l))
    m = render.colour_mask(render.render_to_image(ann, man_image), render.RED)
    assert int((m ^ png("man_iris.png", render.RED)).sum()) == 0
    # iris_landmark.rs:380-398: the eye contours refine the mesh; checked against the oracle's restatement on the same inputs
    refined = gpu.update_face_landmarks_with_iris_results(lms, l, r)
    want = oracle.update_face_landmarks_with_iris_results(arr, [[p.x, p.y, p.z] for p in l.contour], [[p.x, p.y, p.z] for p in r.contour])
    np.testing.assert_array_equal(np.array([[p.x, p.y, p.z] for p in refined]), want)
    # a frame without a face: empty Vec, like the reference
    assert fd.infer(np.zeros((240, 320, 3), np.uint8), None) == []
    assert gpu.FaceLandmark().infer(np.zeros((240, 320, 3), np.uint8), None) == []


def test_batch256_properties(gpu, gold):
    """BASELINE config 2 at full size (256 frames 256x256): size-independent properties instead of an oracle run."""
    torch = pytest.importorskip("torch")
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    face = (gold["man_back_u8"].astype(np.float64) * 2.0 / 255.0 - 1.0).astype(np.float32)
    rs = np.random.RandomState(0)
    x = np.empty((256, 256, 256, 3), np.float32)
    shifts = []
    for b in range(256):
        if b % 2 == 0:
            x[b] = rs.uniform(-1, 1, (256, 256, 3)).astype(np.float32)
            shifts.append(None)
        else:
            dy, dx = int(rs.randint(-32, 33)), int(rs.randint(-32, 33))
            x[b] = np.roll(face, (dy, dx), axis=(0, 1))
            shifts.append((dy, dx))
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    out, counts = fd.infer_tensor(xd, cap=16)
    torch.cuda.synchronize()
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    # (1) permutation equivariance: reversing the batch reverses the results bit-for-bit
    out_r, counts_r = fd.infer_tensor(torch.flip(xd, dims=[0]).contiguous(), cap=16)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(counts_r.cpu().numpy()[::-1], counts)
    np.testing.assert_array_equal(out_r.cpu().numpy()[::-1], out)
    # (2) every face-bearing frame finds the face; shifting the image shifts the box by the same number of pixels
    base = gold["man_back_dets"][0]
    pad = gold["man_back_pad"]
    for b in range(1, 256, 2):
        assert counts[b] >= 1
        dy, dx = shifts[b]
        d = out[b, 0]
        cx = (d[0] + d[2]) / 2 * 256 - dx
        cy = (d[1] + d[3]) / 2 * 256 - dy
        bx = ((base[0] + base[2]) / 2 * (1 - 2 * pad[0]) + pad[0]) * 256
        by = ((base[1] + base[3]) / 2 * (1 - 2 * pad[1]) + pad[1]) * 256
        assert abs(cx - bx) < 6 and abs(cy - by) < 6
    # (3) sortedness: detections of a frame are in non-increasing score order, all above threshold
    for b in range(256):
        s = out[b, : min(counts[b], 16), 16]
        assert np.all(np.diff(s) <= 0) and np.all(s > 0.5)
    fd.close()


def test_config2_batch256_originals_vs_oracle(gpu, oracle, gold):
    """BASELINE config 2 at full size, oracle-checked: 256 frames = 8 distinct frames (four face-bearing:
    plain, mirrored, rolled, dimmed; four noise) repeated 32 times in a shuffled order.  Every copy must reproduce its original
    bit for bit (frames are independent whatever workgroup / strip / band they land in), and the 8 originals are compared with
    the oracle detection by detection.  The same for BASELINE config 1's batch (ShortRange, 128x128)."""
    torch = pytest.importorskip("torch")
    for kind, name, size, okind in ((gpu.FaceDetectionModel.BackCamera, "back", 256, oracle.FD_BACK), (gpu.FaceDetectionModel.Short, "short", 128, oracle.FD_SHORT)):
        fd = gpu.FaceDetection(kind)
        rs = np.random.RandomState(9)
        u8 = gold["man_back_u8"].astype(np.float64)
        if size == 128:
            u8 = u8.reshape(128, 2, 128, 2, 3).mean(axis=(1, 3))
        face = (u8 * 2.0 / 255.0 - 1.0).astype(np.float32)
        base = np.stack([face, face[:, ::-1].copy(), np.roll(face, (size // 9, -size // 12), axis=(0, 1)), face * np.float32(0.8)] +
                        [rs.uniform(-1, 1, face.shape).astype(np.float32) for _ in range(4)])
        order = rs.permutation(256) % 8
        out, counts = fd.infer_tensor(torch.from_numpy(base[order]).cuda(), cap=16)
        torch.cuda.synchronize()
        out, counts = out.cpu().numpy(), counts.cpu().numpy()
        first = {int(k): int(np.where(order == k)[0][0]) for k in range(8)}
        for i in range(256):
            j = first[int(order[i])]
            assert counts[i] == counts[j]
            np.testing.assert_array_equal(out[i, : counts[i]], out[j, : counts[j]])
        om = oracle.Model(model_path(name))
        rb, rsc = om.run(base, nthreads=8)
        anchors = oracle.ssd_anchors(okind)
        found = 0
        for k in range(8):
            want = oracle.fd_postprocess(rb[k], rsc[k], anchors, float(size))
            j = first[k]
            assert counts[j] == len(want), (name, k, counts[j], len(want))
            if len(want):
                np.testing.assert_allclose(out[j, : len(want)], want, atol=2e-5)
                found += 1
        assert found >= 4            # the four face-bearing originals carry a detection
        fd.close()


@pytest.mark.parametrize("kind,name,size,okind", [("BackCamera", "back", 256, "FD_BACK"), ("Short", "short", 128, "FD_SHORT")])
def test_pipe_band_sizes_bit_equal_and_vs_oracle(gpu, oracle, gold, kind, name, size, okind):
    """The band height of the row pipelines (engine option "pipe_band"; bench.py sets 4096 = whole frames while two batches are in flight, i.e.
    inside its timed region — VERDICT r5 missing #3) must not change a bit: 256 frames (8 originals x 32 copies, shuffled) with
    pipe_band 0 (automatic: 2 bands per 64-row frame at this batch), 2, 32 and 4096 (ONE band per frame: bands == 1 at 128^2 and 64^2) are
    compared with each other bit for bit, and the originals of the whole-frame run with the oracle detection by detection."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(11)
    u8 = gold["man_back_u8"].astype(np.float64)
    if size == 128:
        u8 = u8.reshape(128, 2, 128, 2, 3).mean(axis=(1, 3))
    face = (u8 * 2.0 / 255.0 - 1.0).astype(np.float32)
    base = np.stack([face, face[:, ::-1].copy(), np.roll(face, (size // 7, -size // 10), axis=(0, 1)), face * np.float32(0.9)] +
                    [rs.uniform(-1, 1, face.shape).astype(np.float32) for _ in range(4)])
    order = rs.permutation(256) % 8
    xd = torch.from_numpy(base[order]).cuda()
    results = {}
    for band in (0, 2, 32, 4096):
        fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
        fd.model.set_option("pipe_band", band)
        out, counts = fd.infer_tensor(xd, cap=16)
        torch.cuda.synchronize()
        results[band] = (out.cpu().numpy(), counts.cpu().numpy())
        # the raw network outputs too (post-processing could hide a difference below the score threshold)
        raw = fd.model.run(base[order][:40])
        results[band] += tuple(raw)
        fd.close()
    for band in (2, 32, 4096):
        for a, b in zip(results[0], results[band]):
            np.testing.assert_array_equal(a, b, err_msg="pipe_band %d differs from the automatic bands" % band)
    out, counts = results[4096][:2]
    om = oracle.Model(model_path(name))
    rb, rsc = om.run(base, nthreads=8)
    anchors = oracle.ssd_anchors(getattr(oracle, okind))
    first = {int(k): int(np.where(order == k)[0][0]) for k in range(8)}
    found = 0
    for k in range(8):
        want = oracle.fd_postprocess(rb[k], rsc[k], anchors, float(size))
        j = first[k]
        assert counts[j] == len(want), (name, k, counts[j], len(want))
        if len(want):
            np.testing.assert_allclose(out[j, : len(want)], want, atol=2e-5)
            found += 1
        j40 = np.where(order[:40] == k)[0]
        for o, r in zip(results[4096][2:], (rb, rsc)):
            if len(j40):
                _raw_close(o[int(j40[0])], r[k])
    assert found >= 4


def test_config3_landmark_batch512_properties(gpu, oracle, gold):
    """BASELINE config 3 at full size (512 ROIs 192x192 through the face-mesh net + projection + face flag): the batch is 8
    distinct ROIs repeated 64 times in a shuffled order, so every copy must reproduce its original bit for bit (frames are
    independent whatever workgroup, band or stage program they land in), and the 8 originals are checked against the oracle."""
    torch = pytest.importorskip("torch")
    fl = gpu.FaceLandmark()
    rs = np.random.RandomState(5)
    face = gold["man_face_u8"].astype(np.float32) / 255.0
    base = np.stack([face, face[:, ::-1].copy(), np.roll(face, (9, -14), axis=(0, 1)), face * 0.7] + [rs.uniform(0, 1, face.shape).astype(np.float32) for _ in range(4)])
    order = rs.permutation(512) % 8
    xd = torch.from_numpy(base[order]).cuda()
    lm, present, _flags = fl.infer_tensor(xd)
    torch.cuda.synchronize()
    lm, present = lm.cpu().numpy(), present.cpu().numpy()
    first = {int(k): int(np.where(order == k)[0][0]) for k in range(8)}
    for i in range(512):
        np.testing.assert_array_equal(lm[i], lm[first[int(order[i])]])
        assert present[i] == present[first[int(order[i])]]
    assert present[first[0]] == 1 and present[first[2]] == 1          # the face crops carry a face
    om = oracle.Model(model_path("landmark"))
    raw, flag = om.run(base, nthreads=8)
    for k in range(8):
        want = raw[k].reshape(468, 3) / np.array([192.0, 192.0, 192.0])  # project_landmarks without ROI: x/w, y/h, z/w (transform.rs:351-372)
        if present[first[k]]:
            np.testing.assert_allclose(lm[first[k]], want, atol=2e-5)
    fl.close()


def test_config5_pipeline_128_frames_properties(gpu, man_image):
    """BASELINE config 5 at its per-GPU size (128 frames 192x192, full-range detector -> mesh -> 2 x iris on the device): periodic
    input, so results must be periodic bit for bit; noise frames give no face and zeroed downstream records."""
    torch = pytest.importorskip("torch")
    from PIL import Image
    img = np.asarray(Image.fromarray(man_image).resize((192, 192)))
    rs = np.random.RandomState(11)
    period = [img, rs.randint(0, 256, img.shape).astype(np.uint8), np.roll(img, (7, -5), axis=(0, 1)), np.zeros_like(img)]
    frames = torch.from_numpy(np.stack([period[b % 4] for b in range(128)])).cuda()
    pipe = gpu.Pipeline(gpu.FaceDetectionModel.Full)
    out = {k: v.cpu().numpy() for k, v in pipe.run(frames).items()}
    for k, v in out.items():
        for b in range(4, 128):
            np.testing.assert_array_equal(v[b], v[b % 4], err_msg="%s frame %d" % (k, b))
    assert out["face_counts"][0] >= 1 and out["face_counts"][2] >= 1 and out["face_counts"][3] == 0
    assert out["present"][0] == 1 and out["present"][3] == 0
    assert not out["landmarks"][3].any() and not out["eyes"][3].any()
    # the shifted frame moves the face box by about the shift (5 px left, 7 px down at 192 px; anchors sit every 4 px)
    c0 = (out["faces"][0][:2] + out["faces"][0][2:4]) / 2 * 192
    c2 = (out["faces"][2][:2] + out["faces"][2][2:4]) / 2 * 192
    assert abs((c2[0] - c0[0]) + 5) < 4 and abs((c2[1] - c0[1]) - 7) < 4
    pipe.close()


def _oracle_pipeline(oracle, models, img, kind="back"):
    """lib.rs:18-40 through the oracle, one frame."""
    fd, fl, ir = models
    H, W = img.shape[:2]
    size = fd.input_dims[1]
    t, pad = oracle.image_to_tensor(img, None, (size, size), True, (-1., 1.), False)
    rb, rs = fd.run(t[None])
    dets = oracle.fd_postprocess(rb[0], rs[0], oracle.ssd_anchors(getattr(oracle, ORC_KIND[kind])), float(size), pad)
    res = dict(count=len(dets), face=None, landmarks=None, eyes=None)
    if not len(dets):
        return res
    res["face"] = dets[0]
    roi = oracle.face_detection_to_roi(dets[0], (W, H))
    t2, pad2 = oracle.image_to_tensor(img, roi, (192, 192), False, (0., 1.), False)
    raw, flag = fl.run(t2[None])
    if not oracle.lib().orc_face_flag_passes(float(flag.reshape(-1)[-1])):
        return res
    lms = oracle.project_landmarks(raw[0], (192, 192), (W, H), pad2, roi, False)
    res["landmarks"] = lms
    left, right = oracle.iris_rois_from_face_landmarks(lms, (W, H))
    eyes = []
    for r, is_right in ((left, False), (right, True)):
        t3, pad3 = oracle.image_to_tensor(img, r, (64, 64), True, (0., 1.), is_right)
        c, i5 = ir.run(t3[None])
        eyes.append(np.concatenate([oracle.project_landmarks(c[0], (64, 64), (W, H), pad3, r, is_right),
                                    oracle.project_landmarks(i5[0], (64, 64), (W, H), pad3, r, is_right)]))
    res["eyes"] = np.stack(eyes)
    return res


def test_config5_pipeline_128_frames_originals_vs_oracle(gpu, oracle, man_image):
    """BASELINE config 5 at its per-GPU size WITH an oracle (the full-size case was property-only): 128 frames of 192x192 =
    8 distinct frames x 16 in shuffled order through mi_pipeline_run (full-range detector -> faces[0] ROI -> mesh -> 2 x iris on the
    device); every copy equals its original bit for bit wherever it sits in the batch, and the 8 originals agree with the oracle's
    frame-by-frame flow (lib.rs:18-40) at the tensor-path tolerances, as configs 2 and 3 are checked at their full sizes."""
    torch = pytest.importorskip("torch")
    from PIL import Image
    img = np.asarray(Image.fromarray(man_image).resize((192, 192)))
    rs = np.random.RandomState(5)
    originals = [img, np.roll(img, (7, -5), axis=(0, 1)), img[:, ::-1].copy(), (img.astype(np.float32) * 0.7).astype(np.uint8),
                 np.roll(img, (-9, 11), axis=(0, 1)), np.clip(img.astype(np.int32) + 30, 0, 255).astype(np.uint8),
                 rs.randint(0, 256, img.shape).astype(np.uint8), np.zeros_like(img)]
    order = rs.permutation(128) % 8
    order[:8] = np.arange(8)                      # the originals first, then 120 copies in random order
    frames = np.stack([originals[k] for k in order])
    pipe = gpu.Pipeline(gpu.FaceDetectionModel.Full)
    out = {k: v.cpu().numpy() for k, v in pipe.run(torch.from_numpy(frames).cuda()).items()}
    for k, v in out.items():
        for b in range(8, 128):
            np.testing.assert_array_equal(v[b], v[order[b]], err_msg="%s frame %d (copy of %d)" % (k, b, order[b]))
    models = (oracle.Model(model_path("full")), oracle.Model(model_path("landmark")), oracle.Model(model_path("iris")))
    n_faces = n_mesh = 0
    for b in range(8):
        ref = _oracle_pipeline(oracle, models, frames[b], "full")
        assert out["face_counts"][b] == ref["count"], b
        if ref["face"] is None:
            assert out["present"][b] == 0 and not out["faces"][b].any() and not out["landmarks"][b].any() and not out["eyes"][b].any()
            continue
        n_faces += 1
        assert _iou(out["faces"][b][:4], ref["face"][:4]) >= 0.999
        np.testing.assert_allclose(out["faces"][b], ref["face"], atol=2e-5)
        assert out["present"][b] == (ref["landmarks"] is not None)
        if ref["landmarks"] is not None:
            n_mesh += 1
            np.testing.assert_allclose(out["landmarks"][b], ref["landmarks"], atol=2e-5)
            np.testing.assert_allclose(out["eyes"][b], ref["eyes"], atol=1e-4)   # third stage of the chain, see test_full_pipeline_on_man_jpg
    assert n_faces >= 5 and n_mesh >= 5
    pipe.close()


@pytest.mark.parametrize("jpg", ["russ_cox_1.jpg", "russ_cox_2.jpg"])
def test_pipeline_on_the_reference_other_pictures(gpu, oracle, jpg):
    """The reference's two other test pictures (test_data/russ_cox_1.jpg 400x400, russ_cox_2.jpg 200x225 — a PORTRAIT source: the
    letterbox goes left / right instead of top / bottom) from their JPEG bytes through the whole lib.rs:18-40 flow: convert_image_to_mat
    on the device, FaceDetection::infer with all five model types, then faces[0] -> FaceLandmark::infer -> both IrisLandmark::infer
    calls, each against the oracle's restatement of the same call (these pictures were only opened by the JPEG tests)."""
    data = open(os.path.join(GOLDEN, jpg), "rb").read()
    image = gpu.convert_image_to_mat(data)
    np.testing.assert_array_equal(image, oracle.jpeg_decode_rgb(data))            # bit-exact decode (pinned against libjpeg-turbo in test_jpeg.py)
    H, W = image.shape[:2]
    found = 0
    for kind, name in KINDS:
        fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
        faces = fd.infer(image, None)
        iw, ih = fd.input_size
        t, pad = oracle.image_to_tensor(image, None, (iw, ih), True, (-1., 1.), False)
        if H > W:
            assert pad[0] > 0 and pad[2] > 0 and pad[1] == 0 and pad[3] == 0      # left / right letterbox
        rb, rs = oracle.Model(model_path(name)).run(t[None])
        ref = oracle.fd_postprocess(rb[0], rs[0], oracle.ssd_anchors(getattr(oracle, ORC_KIND[name])), float(ih), pad)
        assert len(faces) == len(ref), (kind, len(faces), len(ref))
        for f, r in zip(faces, ref):
            got = np.concatenate([f.data.reshape(-1), [f.score]])
            assert _iou(got[:4], r[:4]) >= 0.999
            np.testing.assert_allclose(got, r, atol=2e-5)
        fd.close()
        if not len(ref):
            continue
        found += 1
        # the rest of the chain from THIS detector's first face, against the oracle's chain from ITS first face
        models = (oracle.Model(model_path(name)), oracle.Model(model_path("landmark")), oracle.Model(model_path("iris")))
        want = _oracle_pipeline(oracle, models, image, name)
        roi = gpu.face_detection_to_roi(faces[0], (W, H))
        lms = gpu.FaceLandmark().infer(image, roi)
        if want["landmarks"] is None:
            assert lms == []
            continue
        assert len(lms) == 468
        np.testing.assert_allclose(np.array([[l.x, l.y, l.z] for l in lms]), want["landmarks"], atol=2e-5)
        left, right = gpu.iris_roi_from_face_landmarks(lms, (W, H))
        iris = gpu.IrisLandmark()
        for k, (r, is_right) in enumerate(((left, False), (right, True))):
            res = iris.infer(image, r, is_right)
            got = np.array([[p.x, p.y, p.z] for p in list(res.contour) + list(res.iris)])
            np.testing.assert_allclose(got, want["eyes"][k], atol=1e-4)            # third stage of the chain, see test_full_pipeline_on_man_jpg
    assert found >= 3, "a face is in both pictures: most detectors must find it"


@pytest.mark.parametrize("kind,name", [("BackCamera", "back"), ("Full", "full"), ("Short", "short")])
def test_batched_device_pipeline_vs_oracle(gpu, oracle, man_image, kind, name):
    """BASELINE config 5 shape at test size (Full = the detector config 5 names): frames -> detector -> faces[0] ROI -> mesh ->
    eye ROIs -> iris, all on the GPU, against the oracle's frame-by-frame flow at the tensor-path tolerances (the device
    pre-processing is bit-exact; the ROI chain runs in f64 on the device)."""
    img = man_image
    frames = np.stack([
        img,
        np.roll(img, (12, -30), axis=(0, 1)),
        img[:, ::-1].copy(),                                    # mirrored face
        (img.astype(np.float32) * 0.6).astype(np.uint8),        # darker
        np.zeros_like(img),                                     # no face
        np.random.RandomState(3).randint(0, 256, img.shape).astype(np.uint8),  # noise
    ])
    pipe = gpu.Pipeline(getattr(gpu.FaceDetectionModel, kind))
    out = pipe.run(frames)
    models = (oracle.Model(model_path(name)), oracle.Model(model_path("landmark")), oracle.Model(model_path("iris")))
    n_faces = 0
    for b in range(len(frames)):
        ref = _oracle_pipeline(oracle, models, frames[b], name)
        assert out["face_counts"][b] == ref["count"], b
        if ref["face"] is None:
            assert out["present"][b] == 0 and not out["faces"][b].any() and not out["landmarks"][b].any() and not out["eyes"][b].any()
            continue
        n_faces += 1
        assert _iou(out["faces"][b][:4], ref["face"][:4]) >= 0.999
        np.testing.assert_allclose(out["faces"][b], ref["face"], atol=2e-5)
        assert out["present"][b] == (ref["landmarks"] is not None)
        if ref["landmarks"] is not None:
            np.testing.assert_allclose(out["landmarks"][b], ref["landmarks"], atol=2e-5)
            np.testing.assert_allclose(out["eyes"][b], ref["eyes"], atol=1e-4)   # third stage of the chain, see test_full_pipeline_on_man_jpg
    assert n_faces >= 3
    # device-resident frames give the same answer
    torch = pytest.importorskip("torch")
    fd = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    out2 = pipe.run(fd)
    torch.cuda.synchronize()
    for k in out:
        np.testing.assert_array_equal(out2[k].cpu().numpy(), out[k])
    pipe.close()


def test_one_handle_from_several_threads(gpu, gold, man_image):
    """face_detection.rs:205 `infer(&self)`: callers may share a handle across threads.  Four threads hammer ONE detector, ONE
    mesh and ONE iris handle through the C ABI (ctypes releases the GIL) with different inputs each; every result must equal
    the single-threaded answer bit for bit (calls are serialised inside the handle, mi_face.h conventions)."""
    import threading
    torch = pytest.importorskip("torch")
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    fl = gpu.FaceLandmark()
    imgs = [man_image, np.roll(man_image, (10, -25), axis=(0, 1)), man_image[:, ::-1].copy(), (man_image * 0.7).astype(np.uint8)]
    face = (gold["man_back_u8"].astype(np.float64) * 2.0 / 255.0 - 1.0).astype(np.float32)
    batches = [np.stack([np.roll(face, (3 * k + j, -5 * j), axis=(0, 1)) for j in range(3)]) for k in range(4)]
    crops = [np.roll(gold["man_face_u8"].astype(np.float32) / 255.0, (2 * k, -k), axis=(0, 1))[None] for k in range(4)]
    key = lambda faces: [np.concatenate([f.data.reshape(-1), [f.score]]) for f in faces]
    want_img = [key(fd.infer(im, None)) for im in imgs]
    want_t = [fd.infer_tensor(b, cap=8) for b in batches]
    want_lm = [fl.infer_tensor(c) for c in crops]
    u8 = gold["man_back_u8"].astype(np.uint8)
    frames8 = [np.stack([np.roll(u8, (2 * k + j, -3 * j), axis=(0, 1)) for j in range(5)]) for k in range(4)]   # batched u8 entry (u8 stem)
    want_u8 = [fd.infer_images(f, cap=8) for f in frames8]
    # device tensors on four different torch streams through the asynchronous entry point
    dev = [torch.from_numpy(b).cuda() for b in batches]
    streams = [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            for it in range(12):
                got = key(fd.infer(imgs[k], None))
                assert len(got) == len(want_img[k]) and all(np.array_equal(a, b) for a, b in zip(got, want_img[k]))
                out, counts = fd.infer_tensor(batches[k], cap=8)
                assert np.array_equal(out, want_t[k][0]) and np.array_equal(counts, want_t[k][1])
                lm, present, flag = fl.infer_tensor(crops[k])
                assert np.array_equal(lm, want_lm[k][0]) and np.array_equal(present, want_lm[k][1])
                o8, c8 = fd.infer_images(frames8[k], cap=8)
                assert np.array_equal(o8, want_u8[k][0]) and np.array_equal(c8, want_u8[k][1])
                o = torch.zeros((3, 8, 17), dtype=torch.float32, device="cuda")
                c = torch.zeros((3,), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                fd.infer_tensor(dev[k], cap=8, out=o, counts=c, stream=streams[k].cuda_stream)
                streams[k].synchronize()
                oh, ch = o.cpu().numpy(), c.cpu().numpy()
                assert np.array_equal(ch, want_t[k][1]), (it, ch.tolist(), want_t[k][1].tolist())
                assert np.array_equal(oh, want_t[k][0]), (it, float(np.abs(oh - want_t[k][0]).max()), np.argwhere(oh != want_t[k][0])[:5].tolist())
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    fd.close()
    fl.close()


def test_dist_broadcast_bytes_world1(gpu, tmp_path):
    """mi_dist_broadcast_bytes (round 5: the weight broadcast of SURVEY.md section 8e on librccl directly, for hosts without
    torch.distributed).  Only a world of ONE rank can run on this box: communicator set-up, ncclBroadcast through device memory and the
    rendezvous file are exercised, the bytes come back unchanged and the handle builds from them.  No run with N > 1 exists (DESIGN.md
    section 6)."""
    blob = open(model_path("back"), "rb").read()
    idf = str(tmp_path / "nccl_id")
    out = gpu.dist_broadcast_bytes(idf, 0, 1, 0, blob)
    assert out == blob and not os.path.exists(idf)
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera, model_bytes=out)
    assert fd.input_size == (256, 256)
    fd.close()
    with pytest.raises(gpu.MiError):
        gpu.dist_broadcast_bytes(idf, 1, 1, 0, blob)          # rank outside the world
    with pytest.raises(gpu.MiError):
        gpu.dist_broadcast_bytes(str(tmp_path / "never_written"), 1, 2, 0, None, nbytes=16, timeout_ms=50)   # no root: times out, no hang


def test_two_batches_in_flight_equal_one_at_a_time(gpu, man_image):
    """bench.py keeps two batches in flight: consecutive steps alternate between two handles on two streams ("Two batches
    in flight").  Whatever pair of streams is taken — on one hardware queue the batches simply follow each other, on two they overlap — every
    batch's results must be bit-equal to the same batch run alone: the handles share no device state (arena, replay graphs, packet buffers,
    the CU count of the single-launch plan is per call).  Detector (64 frames, two different inputs) and the device pipeline (16 frames)."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(3)
    xs = [torch.from_numpy(rs.uniform(-1, 1, (64, 256, 256, 3)).astype(np.float32)).cuda() for _ in range(2)]
    fds = [gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera) for _ in range(2)]
    alone = []
    for k in range(2):
        o, c = fds[k].infer_tensor(xs[k], cap=8)
        torch.cuda.synchronize()
        alone.append((o.clone(), c.clone()))
    streams = [torch.cuda.Stream() for _ in range(5)]
    for j in range(1, 5):
        ss = (streams[0], streams[j])
        outs = [(torch.zeros((64, 8, 17), device="cuda"), torch.zeros((64,), dtype=torch.int32, device="cuda")) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(12):
            k = i & 1
            fds[k].infer_tensor(xs[k], cap=8, out=outs[k][0], counts=outs[k][1], stream=ss[k].cuda_stream)
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(outs[k][0], alone[k][0]) and torch.equal(outs[k][1], alone[k][1]), (j, k)
    # the band height bench.py sets while two batches are in flight (whole frames as bands of the row pipelines): same bits
    for fd in fds:
        fd.model.set_option("pipe_band", 4096)
    for j in (1, 2, 3):
        ss = (streams[0], streams[j])
        outs = [(torch.zeros((64, 8, 17), device="cuda"), torch.zeros((64,), dtype=torch.int32, device="cuda")) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(8):
            k = i & 1
            fds[k].infer_tensor(xs[k], cap=8, out=outs[k][0], counts=outs[k][1], stream=ss[k].cuda_stream)
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(outs[k][0], alone[k][0]) and torch.equal(outs[k][1], alone[k][1]), ("pipe_band 4096", j, k)
    for fd in fds:
        fd.close()
    frames = np.stack([np.roll(man_image[:192, 100:292], (3 * i, -2 * i), axis=(0, 1)) for i in range(16)]).astype(np.uint8)
    ft = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    pipes = [gpu.Pipeline(gpu.FaceDetectionModel.Full) for _ in range(2)]
    want = pipes[0].run(ft)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in want.items()}
    for j in (1, 2, 3, 4):
        ss = (streams[0], streams[j])
        got = [None, None]
        for i in range(6):
            got[i & 1] = pipes[i & 1].run(ft, stream=ss[i & 1].cuda_stream)
        torch.cuda.synchronize()
        for k in range(2):
            for name in want:
                assert torch.equal(got[k][name], want[name]), (j, k, name)
    for p in pipes:
        p.close()


def test_streams_on_distinct_hardware_queues(gpu):
    """mi_streams_create_distinct: the streams it returns were tested to run side by side; two detector handles alternating on them give
    the results of one handle, and destroying clears the slots.  (A request for more queues than the device has must fail cleanly.)"""
    torch = pytest.importorskip("torch")
    ss = gpu.streams_create_distinct(2)
    assert len(ss) == 2 and ss[0] and ss[1] and ss[0] != ss[1]
    rs = np.random.RandomState(4)
    x = torch.from_numpy(rs.uniform(-1, 1, (32, 128, 128, 3)).astype(np.float32)).cuda()
    fds = [gpu.FaceDetection(gpu.FaceDetectionModel.Short) for _ in range(2)]
    want, wc = fds[0].infer_tensor(x, cap=8)
    torch.cuda.synchronize()
    outs = [(torch.zeros((32, 8, 17), device="cuda"), torch.zeros((32,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    for i in range(10):
        fds[i & 1].infer_tensor(x, cap=8, out=outs[i & 1][0], counts=outs[i & 1][1], stream=ss[i & 1])
    torch.cuda.synchronize()
    for o, c in outs:
        assert torch.equal(o, want) and torch.equal(c, wc)
    for fd in fds:
        fd.close()
    gpu.streams_destroy(ss)
    three = gpu.streams_create_distinct(3)
    assert len(set(three)) == 3
    gpu.streams_destroy(three)
    with pytest.raises(gpu.MiError):
        gpu.streams_create_distinct(5)


def test_single_image_entries_from_several_processes(gpu, gold):
    """ADVICE r5 (medium), the real case: the CU budget of the single-launch plan is per PROCESS, so three processes that each call
    mi_fd_infer_image (128 workgroups per BackCamera call, 256 CUs) can put launches on the device whose workgroups are not all resident.  Every
    call must still return the oracle's detections (a launch that gave up is repeated on the batched plan; a handle that keeps giving up stops
    trying), and nobody may stall: round 5's 0.3 s per stage would make this test take minutes."""
    import subprocess, sys, time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import os, sys, time, json
import numpy as np
sys.path.insert(0, %r)
import rs_face_detection_tflite_amd as mi
from PIL import Image
img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(%r, "tests", "golden", "man.jpg")).convert("RGB")))
fd = mi.FaceDetection(mi.FaceDetectionModel.BackCamera)
fd.infer(img, None)
t0 = time.perf_counter(); worst = 0.0; rows = None
for k in range(300):
    t = time.perf_counter()
    d = fd.infer(img, None)
    worst = max(worst, time.perf_counter() - t)
    r = [np.concatenate([x.data.reshape(-1), [x.score]]).tolist() for x in d]
    if rows is None: rows = r
    assert len(r) == len(rows) and all(np.allclose(a, b, atol=2e-5) for a, b in zip(r, rows)), k
print(json.dumps({"rows": rows, "total_s": time.perf_counter() - t0, "worst_s": worst, "band": fd.model.get_option("band"), "streak": fd.model.get_option("band_fail_streak")}))
''' % (root, root)
    t0 = time.perf_counter()
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(3)]
    outs = [p.communicate(timeout=300) for p in procs]
    wall = time.perf_counter() - t0
    import json
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
        res = json.loads(so.strip().splitlines()[-1])
        assert len(res["rows"]) == 1
        np.testing.assert_allclose(np.asarray(res["rows"][0]), gold["man_back_dets"][0], atol=2e-5)
        print("process: 300 calls in %.3f s, worst call %.1f ms, band option now %d, give-ups in a row %d" % (res["total_s"], res["worst_s"] * 1e3, res["band"], res["streak"]))
        assert res["worst_s"] < 0.25, res          # one bounded wait + the batched plan, never seconds
        assert res["total_s"] < 30, res
    assert wall < 120


@pytest.mark.parametrize("frames", [1, 32])
def test_iris_profile_labels_equal_the_pinned_launch_list(gpu, frames):
    """The launch list is pinned on the CPU with fake device addresses (tests/test_launch_pins.py); the only thing the selection reads from a
    pointer is its alignment.  On the device, with real addresses, the iris network (64 x 64 input, the smallest) takes the same branches: the
    kernel labels profile() returns, in order, are the labels pinned for that model and frame count at the default options."""
    import json
    import re
    import torch
    pins = json.load(open(os.path.join(GOLDEN, "launch_pins.json")))
    want = [re.search(r'"(.*)"', line).group(1) for line in pins["iris_landmark.tflite defaults F=%d" % frames] if '"' in line]
    assert len(want) > 3
    m = gpu.Model(model_path("iris"))
    x = seeded_input("iris", frames, 77, m.input_dims[1:3])
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    m.close()
    assert labels == want
