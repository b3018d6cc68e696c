"""The phased contraction of the fixed-shape chain kernels (option "chain_sched", csrc/chain_kernels.hip): the LDS reads of the next channel
chunk requested a block of MFMAs ahead, a chunk's depthwise FMAs as one block, its MFMAs as one block.

The phases change when an instruction is issued, never an FMA chain or an accumulator's k order, so everything here is bit for bit:
"chain_sched" = 1 against 0 (the interleaved schedule, compiled beside it) and against "chain_fixed" = 0 (the generic kernel), a frame of a
batch against the same frame alone, two batches in flight against one at a time.  Against the oracle the tolerance is test_gpu_parity.py's
for raw network outputs.  BackCamera (256 x 256) runs the 16x16x96 instantiation with its two stride-2 stages; Short (128 x 128) runs that one
and the 8x8x96 instantiation behind it, whose stages are (group, output tile) units.  "band" = 0 everywhere: at these batch sizes the batched
plan must run, not the single-launch plan (which has no chain launch)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, model_path

pytestmark = pytest.mark.gpu

RAW_TOL = 1e-4   # test_gpu_parity.py: raw network outputs, |d| <= 1e-4 * max(1, max|x|)
BATCHES = (1, 2, 5)
DETECTORS = {"back": ("BackCamera", 256), "short": ("Short", 128)}   # model type, input size
# (chain_fixed, chain_sched): the phased schedule, the interleaved schedule, the generic kernel
FORMS = {"phased": (1, 1), "interleaved": (1, 0), "generic": (0, 1)}


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


def _set_form(model, form):
    fixed, sched = FORMS[form]
    model.set_option("chain_fixed", fixed)
    model.set_option("chain_sched", sched)
    assert model.get_option("chain_fixed") == fixed and model.get_option("chain_sched") == sched


@pytest.fixture(scope="module")
def detector_runs(gpu):
    """Raw outputs and detections of both detectors in the three forms, every batch size, computed once."""
    out = {}
    for name, (kind, size) in DETECTORS.items():
        fd = gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind))
        fd.model.set_option("band", 0)
        assert fd.model.get_option("chain_sched") == 1   # the default
        x = _frames(size)
        for form in FORMS:
            _set_form(fd.model, form)
            for nb in BATCHES:
                raw = [np.array(o, copy=True) for o in fd.model.run(x[:nb])]
                det, counts = fd.infer_tensor(x[:nb], cap=16)
                out[name, form, nb] = (raw, det.copy(), counts.copy())
            out[name, form, "labels"] = _chain_labels(fd.model, x[:2])
        # frame k alone, on the phased schedule
        _set_form(fd.model, "phased")
        out[name, "alone"] = [[np.array(o, copy=True) for o in fd.model.run(x[k:k + 1])] for k in range(5)]
        out[name, "x"] = x
        fd.close()
    return out


@pytest.mark.parametrize("other", ["interleaved", "generic"])
@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_phased_chain_bit_equal(detector_runs, name, other):
    """chain_sched = 1 against chain_sched = 0 and against chain_fixed = 0: every raw network output and the detections, 1 / 2 / 5 frames,
    np.array_equal; and a chain_kernel launch did run in each."""
    for form in ("phased", other):
        labels = detector_runs[name, form, "labels"]
        assert labels and all(k == "chain_kernel<3>" for k in labels), (form, labels)
    assert len(detector_runs[name, "phased", "labels"]) == (2 if name == "short" else 1)   # Short: the 16x16 chain and the 8x8 chain behind it
    for nb in BATCHES:
        raw1, det1, cnt1 = detector_runs[name, "phased", nb]
        raw0, det0, cnt0 = detector_runs[name, other, nb]
        assert len(raw1) == len(raw0) == 2
        for a, b in zip(raw1, raw0):
            assert a.shape == b.shape and np.array_equal(a, b), (name, other, nb, float(np.abs(a - b).max()))
        assert np.array_equal(cnt1, cnt0) and np.array_equal(det1, det0), (name, other, nb)
    if name == "back":
        assert detector_runs[name, "phased", 5][2][0] >= 1   # the golden face is found (the comparison is not of empty lists)


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_phased_chain_vs_oracle(detector_runs, oracle, name):
    om = oracle.Model(model_path(name))
    refs = om.run(detector_runs[name, "x"], nthreads=5)
    for nb in BATCHES:
        for o, r in zip(detector_runs[name, "phased", nb][0], refs):
            got, ref = o, r.reshape(5, -1)[:nb].reshape(o.shape)
            scale = max(1.0, float(np.abs(ref).max()))
            err = float(np.abs(got - ref).max())
            assert err <= RAW_TOL * scale, "max|diff| %.3e > %.1e * %.1f" % (err, RAW_TOL, scale)


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_phased_chain_frames_are_independent(detector_runs, name):
    """Frame k of the 5-frame batch equals the same frame run alone, bit for bit, on the phased schedule."""
    batch = detector_runs[name, "phased", 5][0]
    for k in range(5):
        for o, a in zip(batch, detector_runs[name, "alone"][k]):
            assert np.array_equal(o.reshape(5, -1)[k], a.reshape(-1)), (name, k)


@pytest.mark.parametrize("name", sorted(DETECTORS))
def test_phased_chain_two_batches_in_flight(gpu, detector_runs, name):
    """Two handles on two streams, 5 frames each (the second handle takes the frames in reverse order): raw outputs and detections are
    bit-equal to the same batches run one at a time."""
    import torch
    kind, _ = DETECTORS[name]
    x = detector_runs[name, "x"]
    xs = [torch.from_numpy(x).cuda(), torch.from_numpy(x[::-1].copy()).cuda()]
    fds = [gpu.FaceDetection(getattr(gpu.FaceDetectionModel, kind)) for _ in range(2)]
    for fd in fds:
        fd.model.set_option("band", 0)
        _set_form(fd.model, "phased")
    want_raw, want_det, want_cnt = detector_runs[name, "phased", 5]
    streams = [torch.cuda.Stream() for _ in range(2)]
    raws = [[torch.zeros_like(torch.from_numpy(o)).cuda() for o in want_raw] for _ in range(2)]
    dets = [(torch.zeros((5, 16, 17), device="cuda"), torch.zeros((5,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(6):
        k = i & 1
        fds[k].model.run(xs[k], outs=raws[k], stream=streams[k].cuda_stream)
        fds[k].infer_tensor(xs[k], cap=16, out=dets[k][0], counts=dets[k][1], stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        order = slice(None) if k == 0 else slice(None, None, -1)
        for got, want in zip(raws[k], want_raw):
            assert np.array_equal(got.cpu().numpy(), want[order]), (name, k)
        assert np.array_equal(dets[k][1].cpu().numpy(), want_cnt[order]) and np.array_equal(dets[k][0].cpu().numpy(), want_det[order]), (name, k)
    for fd in fds:
        fd.close()
