"""Whole-frame bands of the two-row MFMA row pipeline (strip_pipe2m_kernel with bands == 1: "pipe_band" = 4096, or the automatic choice for a
handful of frames): the pipeline steps that would only see rows above the picture are skipped, and a stride-2 tail finishes its last output row in
the step that consumes the picture's last row pair instead of in a flush step of its own.

Skipping a step is equivalent to running it on rows of zeros, so everything here is bit for bit (np.testing.assert_array_equal on all raw network
outputs): the whole-frame run against (a) the same bands on strip_pipe2_kernel ("pipe_rows" = 2), which this change does not touch, and (b)
strip_pipe2m_kernel on interior bands ("pipe_band" = 2: every band but the first starts inside the picture) and on the automatic bands ("pipe_band"
= 0).  Against the oracle the tolerance is test_gpu_parity.py's for raw network outputs.  The synthetic graphs also run the two one-row forms
("pipe_rows" = 1: strip_pipe_kernel, 4: strip_pipe1m_kernel) on automatic and whole-frame bands, bit for bit against the default form: they
share the row DMA, store, hand-over and tail-store functions with the two-row forms, and these sizes reach their partial-strip and inactive-unit paths.

Every case forces the batched plan ("band" = 0) and the pipelines ("small_chain" = 0, "fuse" = 4), and reads from profile() which instantiations
ran.  The synthetic frames are the smallest at which a schedule that is off by one step shows: 18 x 18 (band_rows / 2 = 9 row pairs against a fill
of up to 7 steps: a lost or duplicated pair is a wrong row), 66 wide (two strips, the second with two live pixels), 64 wide (two units per workgroup;
an odd batch leaves the last workgroup's second unit inactive)."""
import re

import numpy as np
import pytest

from conftest import model_path, seeded_input

pytestmark = pytest.mark.gpu

RAW_TOL = 1e-4   # test_gpu_parity.py: raw network outputs, |d| <= 1e-4 * max(1, max|x|)
LABEL = re.compile(r"strip_pipe2m_kernel<(\d+),(\d+),(\d+),(\d+)>")
REACHED = set()   # (CQ, KB, NH2) of every strip_pipe2m_kernel launch the whole-frame runs of this file made


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


def _raw_close(got, ref):
    ref = ref.reshape(got.shape)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= RAW_TOL * scale, "max|diff| %.3e > %.1e * %.1f" % (err, RAW_TOL, scale)


def _pipelined(gpu, path):
    m = gpu.Model(path)
    for key, value in (("band", 0), ("small_chain", 0), ("fuse", 4)):
        m.set_option(key, value)
    return m


def _run(m, x, pipe_band, pipe_rows=0):
    m.set_option("pipe_band", pipe_band)
    m.set_option("pipe_rows", pipe_rows)
    return [np.array(o, copy=True) for o in m.run(x)]


def _instantiations(m, x, prefix="strip_pipe2m_kernel<"):
    """(CQ, KB, NH2) of the strip_pipe2m_kernel launches of the model as it is set now; no other pipeline form may run beside them."""
    import torch
    labels = [r["kernel"] for r in m.profile(torch.from_numpy(x).cuda(), reps=1)]
    pipes = [k for k in labels if k.startswith("strip_pipe")]
    assert pipes and all(k.startswith(prefix) for k in pipes), labels
    return {(int(g[0]), int(g[1]), int(g[3])) for g in (LABEL.match(k).groups() for k in pipes if LABEL.match(k))}


def _whole_frame_against_the_other_forms(m, x, tag):
    """The whole-frame run and its comparisons (a) and (b); returns the whole-frame outputs."""
    whole = _run(m, x, 4096)
    inst = _instantiations(m, x)
    assert inst, tag
    print("%s: whole-frame bands ran strip_pipe2m_kernel (CQ, KB, NH2) %s" % (tag, sorted(inst)))
    REACHED.update(inst)
    for band in (2, 0):   # (b) interior bands, automatic bands: the same kernel
        other = _run(m, x, band)
        for a, b in zip(whole, other):
            np.testing.assert_array_equal(a, b, err_msg="%s: pipe_band 4096 differs from pipe_band %d" % (tag, band))
    two = _run(m, x, 4096, pipe_rows=2)   # (a) the packed-FMA two-row form on the same whole-frame bands
    _instantiations(m, x, "strip_pipe2_kernel<")
    for a, b in zip(whole, two):
        np.testing.assert_array_equal(a, b, err_msg="%s: strip_pipe2m_kernel differs from strip_pipe2_kernel on whole frames" % tag)
    m.set_option("pipe_rows", 0)
    return whole


ONE_ROW_FORMS = {1: "strip_pipe_kernel<", 4: "strip_pipe1m_kernel<"}   # "pipe_rows" -> the kernel it selects


def _one_row_forms_agree(m, x, whole, tag):
    """The one-row forms share the row DMA, store, hand-over and tail-store functions with the two-row forms; at these sizes they reach their
    partial-strip and inactive-unit paths.  Automatic and whole-frame bands, bit for bit against the default form's outputs."""
    for rows, prefix in ONE_ROW_FORMS.items():
        for band in (0, 4096):
            got = _run(m, x, band, pipe_rows=rows)
            _instantiations(m, x, prefix)
            for a, b in zip(whole, got):
                np.testing.assert_array_equal(a, b, err_msg="%s: pipe_rows %d at pipe_band %d differs from the default form" % (tag, rows, band))
    m.set_option("pipe_rows", 0)


@pytest.mark.parametrize("pipe", [2, 3, 4])
def test_back_model_whole_frame_bands(gpu, oracle, pipe):
    """BackCamera, 3 frames (the last 64-wide workgroup has one live unit), its two runs of blocks cut into chains of at most `pipe` blocks: one to
    four stride-1 stages, plain and with either stride-2 tail."""
    m = _pipelined(gpu, model_path("back"))
    m.set_option("pipe", pipe)
    x = seeded_input("back", 3, 500 + pipe, m.input_dims[1:3])
    x[1, :2] = 0.0   # a frame whose first row pair is blank
    whole = _whole_frame_against_the_other_forms(m, x, "back pipe=%d" % pipe)
    m.close()
    refs = oracle.Model(model_path("back")).run(x, nthreads=3)
    for o, r in zip(whole, refs):
        _raw_close(o, r)


def run_of_blocks(seed, h, w, c0, n1, act="relu", co=None):
    """back_like's / mesh_like's first resolution alone: stem 5x5 s2 -> n1 BlazeBlocks(c0) at (h/2 x w/2) -> stride-2 block to `co` channels -> 1x1
    head.  back_like and mesh_like halve the frame three and four more times, so their first resolution must divide by 8 / 16: they cannot make
    an 18-row or a 66-pixel-wide one, and they are square."""
    import synth_tflite
    g = synth_tflite.GraphBuilder(seed, [1, h, w, 3])
    x = g.conv(g.input, c0, 5, 2)
    x = g.relu(x) if act == "relu" else g.prelu(x)
    for _ in range(n1):
        x = g.blaze_block(x, act=act)
    x = g.blaze_block(x, co or 2 * c0, 2, act=act)
    g.outputs = [g.conv(x, 6)]
    return g.finish()


# name -> (builder, its arguments, (input height, width), batches): the first pipelined resolution is half the input size
SYNTH = {
    # 18 x 18 = 324 pixels, the smallest even square frame that is not chain_kernel's (H W <= 256): 9 row pairs
    "run24_18x18": (run_of_blocks, (51, 36, 36, 24, 3), (36, 36), (3,)),                 # 3 stages + the 24 -> 48 tail
    "run24_18x18_tail24": (run_of_blocks, (52, 36, 36, 24, 3, "relu", 24), (36, 36), (3,)),   # 3 stages + the 24 -> 24 tail
    "run24_18x18_one_stage": (run_of_blocks, (53, 36, 36, 24, 1), (36, 36), (3,)),       # 1 stage + tail: nothing to skip at the top, no flush step
    "run24_18x18_two_stages": (run_of_blocks, (54, 36, 36, 24, 2), (36, 36), (3,)),      # 2 stages + tail
    "run16_18x18_prelu": (run_of_blocks, (55, 36, 36, 16, 3, "prelu"), (36, 36), (3,)),  # 16 channels, PReLU, 3 stages
    "run16_18x18_four": (run_of_blocks, (56, 36, 36, 16, 4), (36, 36), (3,)),            # 16 channels, 4 stages
    # 66 pixels wide: two strips, the second with two live pixels
    "run24_18x66": (run_of_blocks, (57, 36, 132, 24, 3), (36, 132), (2,)),               # the tail wave serves both strips
    "run16_20x66": (run_of_blocks, (58, 40, 132, 16, 2, "prelu"), (40, 132), (2,)),
    "run24_20x66_prelu": (run_of_blocks, (59, 40, 132, 24, 4, "prelu"), (40, 132), (2,)),   # 4 stages without a tail (only ReLU tails exist)
    # the builders' own smallest pipelined resolutions, and 64 pixels wide (two units per workgroup) at one and three frames
    "back24_24x24": ("back_like", (60, 48, 24), (48, 48), (3,)),
    "back16_24x24": ("back_like", (61, 48, 16, 3, 2), (48, 48), (3,)),
    "mesh16_32x32": ("mesh_like", (62, 64, 16), (64, 64), (3,)),
    "mesh24_32x32": ("mesh_like", (63, 64, 24), (64, 64), (3,)),
    "mesh16_64x64": ("mesh_like", (64, 128, 16), (128, 128), (1, 3)),
    "back24_64x64": ("back_like", (65, 128, 24), (128, 128), (1, 3)),                    # the tail wave serves both units
}


@pytest.fixture(scope="module")
def synth_models(tmp_path_factory):
    """The graphs above written out as .tflite files (oracle and product both read files), as test_gpu_parity.py's fixture does."""
    import synth_tflite
    d = tmp_path_factory.mktemp("synth_edges")
    out = {}
    for name, (builder, args, hw, _) in SYNTH.items():
        p = d / (name + ".tflite")
        p.write_bytes((getattr(synth_tflite, builder) if isinstance(builder, str) else builder)(*args))
        out[name] = (str(p), hw)
    return out


@pytest.mark.parametrize("case", sorted(SYNTH))
def test_synthetic_graphs_whole_frame_bands(gpu, oracle, synth_models, case):
    path, (h, w) = synth_models[case]
    m = _pipelined(gpu, path)
    for nb in SYNTH[case][3]:
        x = np.random.RandomState(700 + nb).uniform(-1, 1, (nb, h, w, 3)).astype(np.float32)
        whole = _whole_frame_against_the_other_forms(m, x, "%s B=%d" % (case, nb))
        _one_row_forms_agree(m, x, whole, "%s B=%d" % (case, nb))
        for o, r in zip(whole, oracle.Model(path).run(x, nthreads=max(1, nb))):
            _raw_close(o, r)
    m.close()


def test_two_batches_in_flight_on_whole_frame_bands(gpu):
    """Two handles on two streams with pipe_band = 4096, BackCamera, 6 frames each (the second handle takes them in reverse order): raw outputs
    bit-equal to the same batch run alone."""
    import torch
    x = seeded_input("back", 6, 801, (256, 256))
    models = [_pipelined(gpu, model_path("back")) for _ in range(2)]
    want = _run(models[0], x, 4096)
    REACHED.update(_instantiations(models[0], x))
    models[1].set_option("pipe_band", 4096)
    xs = [torch.from_numpy(x).cuda(), torch.from_numpy(x[::-1].copy()).cuda()]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [[torch.zeros_like(torch.from_numpy(o)).cuda() for o in want] for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(6):
        k = i & 1
        models[k].run(xs[k], outs=outs[k], stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        order = slice(None) if k == 0 else slice(None, None, -1)
        for got, w in zip(outs[k], want):
            np.testing.assert_array_equal(got.cpu().numpy(), w[order], err_msg="handle %d" % k)
    for m in models:
        m.close()


def test_every_instantiation_family_was_reached():
    """Runs last in the file: across the cases above the whole-frame path ran the three pinned four-stage 24-channel instantiations, a 16-channel
    pipeline, and pipelines of two and of three stages."""
    assert REACHED, "run the whole file: this test reads what the tests above recorded"
    print("strip_pipe2m_kernel (CQ, KB, NH2) reached on whole-frame bands:", sorted(REACHED))
    assert {(6, 4, 0), (6, 4, 1), (6, 4, 2)} <= REACHED, sorted(REACHED)
    assert any(cq == 4 and nh2 == 0 for cq, _, nh2 in REACHED), sorted(REACHED)
    assert any(kb == 2 for _, kb, _ in REACHED) and any(kb == 3 for _, kb, _ in REACHED), sorted(REACHED)
