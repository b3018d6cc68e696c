"""The fixed-shape instantiations of chain_kernel (option "chain_fixed", csrc/chain_kernels.hip): the detectors' 16x16x96 chain
between its two stride-2 blocks and the 8x8x96 chain of Short / Front, with the shape as constants and a ReLU epilogue.

They run the generic kernel's arithmetic in the generic kernel's order, so everything here is bit for bit: option on against
option off on the shipped detectors, chains that must fall back to the generic kernel (PReLU, ReLU6, a shape that is not
instantiated) on synthetic graphs, and a frame of a batch against the same frame alone.  Against the oracle the tolerance is
test_gpu_parity.py's for raw network outputs.  "band" = 0 everywhere: at these batch sizes the batched plan must run, not the
single-launch plan (which has no chain launch)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, model_path

pytestmark = pytest.mark.gpu

RAW_TOL = 1e-4   # test_gpu_parity.py: raw network outputs, |d| <= 1e-4 * max(1, max|x|)
BATCHES = (1, 2, 5)


def _raw_close(got, ref):
    ref = ref.reshape(got.shape)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= RAW_TOL * scale, "max|diff| %.3e > %.1e * %.1f" % (err, RAW_TOL, scale)


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


def _frames(size):
    """Five frames in [-1, 1]: the golden face, the face shifted, noise, a blank frame, the face mirrored."""
    u8 = np.load(os.path.join(GOLDEN, "golden.npz"))["man_back_u8"]
    if size == 128:
        u8 = u8[::2, ::2]
    face = (u8.astype(np.float64) * 2.0 / 255.0 - 1.0).astype(np.float32)
    noise = np.random.RandomState(977).uniform(-1, 1, face.shape).astype(np.float32)
    return np.stack([face, np.roll(face, (9, -6), axis=(0, 1)), noise, np.zeros_like(face), face[:, ::-1].copy()])


def _chain_labels(model, x):
    import torch
    return [r["kernel"] for r in model.profile(torch.from_numpy(x).cuda(), reps=1) if r["kernel"].startswith("chain_kernel")]


DETECTORS = {"back": ("BackCamera", 256), "short": ("Short", 128)}   # model type, input size


@pytest.fixture(scope="module")
def detector_runs(gpu):
    """Raw outputs and detections of both detectors with the option on and off, every batch size, computed once."""
    out = {}
    for name, (kind, size) in DETECTORS.items():
        fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
        fd.model.set_option("band", 0)
        x = _frames(size)
        for fixed in (1, 0):
            fd.model.set_option("chain_fixed", fixed)
            assert fd.model.get_option("chain_fixed") == fixed
            for nb in BATCHES:
                raw = [np.array(o, copy=True) for o in fd.model.run(x[:nb])]
                det, counts = fd.infer_tensor(x[:nb], cap=16)
                out[name, fixed, nb] = (raw, det.copy(), counts.copy())
            out[name, fixed, "labels"] = _chain_labels(fd.model, x[:2])
        # frame k alone, on the fixed path
        fd.model.set_option("chain_fixed", 1)
        out[name, "alone"] = [[np.array(o, copy=True) for o in fd.model.run(x[k:k + 1])] for k in range(5)]
        out[name, "x"] = x
        fd.close()
    return out


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_fixed_chain_bit_equal_to_generic_chain(detector_runs, name):
    """chain_fixed = 1 against chain_fixed = 0: every raw network output and the detections, 1 / 2 / 5 frames, np.array_equal;
    and a chain_kernel launch did run in both."""
    for fixed in (1, 0):
        labels = detector_runs[name, fixed, "labels"]
        assert labels and all(k == "chain_kernel<3>" for k in labels), labels
    for nb in BATCHES:
        raw1, det1, cnt1 = detector_runs[name, 1, nb]
        raw0, det0, cnt0 = detector_runs[name, 0, nb]
        assert len(raw1) == len(raw0) == 2
        for a, b in zip(raw1, raw0):
            assert a.shape == b.shape and np.array_equal(a, b), (name, nb, float(np.abs(a - b).max()))
        assert np.array_equal(cnt1, cnt0) and np.array_equal(det1, det0), (name, nb)
    if name == "back":
        assert detector_runs[name, 1, 5][2][0] >= 1   # the golden face is found (the comparison is not of empty lists)


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_fixed_chain_vs_oracle(detector_runs, oracle, name):
    om = oracle.Model(model_path(name))
    refs = om.run(detector_runs[name, "x"], nthreads=5)
    for nb in BATCHES:
        for o, r in zip(detector_runs[name, 1, nb][0], refs):
            _raw_close(o, r.reshape(5, -1)[:nb].reshape(o.shape))


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_fixed_chain_frames_are_independent(detector_runs, name):
    """Frame k of the 5-frame batch equals the same frame run alone, bit for bit, on the fixed path."""
    batch = detector_runs[name, 1, 5][0]
    for k in range(5):
        for o, a in zip(batch, detector_runs[name, "alone"][k]):
            assert np.array_equal(o.reshape(5, -1)[k], a.reshape(-1)), (name, k)


def _chain_graph(seed, size, c, act):
    """stem 3x3 s2 -> three BlazeBlocks at (size/2)^2 x c (a frame-resident chain) -> 1x1 head."""
    import synth_tflite as st
    g = st.GraphBuilder(seed, [1, size, size, 3])
    x = g.relu(g.conv(g.input, c, 3, 2))
    for _ in range(3):
        if act == "relu6":   # the activation fused into the ADD, as TFLite writes ReLU6
            y = g.conv(g.dw(x), c)
            s = g._act(g.shape(x), "add")
            g.ops.append((st.ADD, [y, x], [s], st.OPT_ADD, [("i8", st.ACT_RELU6)]))
            x = s
        else:
            x = g.blaze_block(x, act=act)
    g.outputs = [g.conv(x, 6)]
    return g.finish()


FALLBACKS = {
    # name: (builder, input size, fuse level)
    "prelu_16x16x96": (lambda: _chain_graph(71, 32, 96, "prelu"), 32, 5),     # the instantiated shape with another activation
    "relu6_16x16x96": (lambda: _chain_graph(72, 32, 96, "relu6"), 32, 5),
    "relu_12x12x64": (lambda: _chain_graph(73, 24, 64, "relu"), 24, 3),       # ReLU on shapes that are not instantiated (at level 5 a
    "relu_12x12x96": (lambda: _chain_graph(75, 24, 96, "relu"), 24, 5),       # 64-channel run of this size is a stage program, not a chain)
    "relu_16x16x96_bare": (lambda: _chain_graph(74, 32, 96, "relu"), 32, 5),  # the shape and ReLU, but no stride-2 blocks around it
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_other_chains_fall_back_to_the_generic_kernel(gpu, oracle, tmp_path, case):
    make, size, fuse = FALLBACKS[case]
    path = tmp_path / (case + ".tflite")
    path.write_bytes(make())
    m = gpu.Model(str(path))
    m.set_option("band", 0)
    m.set_option("fuse", fuse)
    x = np.random.RandomState(31).uniform(-1, 1, (5, size, size, 3)).astype(np.float32)
    refs = oracle.Model(str(path)).run(x, nthreads=5)
    outs = {}
    for fixed in (1, 0):
        m.set_option("chain_fixed", fixed)
        outs[fixed] = [np.array(o, copy=True) for o in m.run(x)]
        assert _chain_labels(m, x), "no chain_kernel launch in " + case
    for a, b, r in zip(outs[1], outs[0], refs):
        assert np.array_equal(a, b), (case, float(np.abs(a - b).max()))
        _raw_close(a, r)
    m.close()
