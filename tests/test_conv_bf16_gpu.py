"""Engine option "conv_bf16" on the device: conv_bf16_kernel (the dense k x k convolutions on v_mfma_f32_32x32x16_bf16) layer by layer against
the float64 references and the derived bounds of tests/conv_bf16_ref.py, its bits against batch size, tile width and run, the way back to 0,
the synthetic network against the oracle's evaluation of its twin, and FaceEmbeddings(precision=...).

The layer cases are tests/test_resnet_gpu.py's (same conv_layer arguments, seeds and inputs) plus two: Co = 160 (two 128-wide tiles, the last
ragged) and a 5x5 kernel (25 taps: the tap mask beyond nine bits).  Every case prints its worst error / bound; F = 1 (conv_bf16_ref.F).

Observed on an MI355X (2026-10-19), worst error / bound per case: 0.0012 .. 0.0056 at conv_bf16 = 1 and 0.0076 .. 0.040 at 2, so the bounds derived
for IEEE adds hold as they stand and F stays 1.  Network (five chips): value 2 is 3.2e-5 from the oracle's evaluation of the twin (value 0: 1.6e-5;
yardstick 2.7e-4); value 1 moves the raw outputs by 4.9e-3 of their largest value, smallest cosine against value 0 0.99999215."""
import os

import numpy as np
import pytest

import conv_bf16_ref as cb
import resnet_synth as rs
from conftest import GOLDEN
from synth_tflite import VALID

pytestmark = pytest.mark.gpu
RAW_TOL = 1e-4   # x max(1, max|ref|): the project's yardstick for raw outputs (tests/test_gpu_parity.py, tests/test_resnet_gpu.py)
KERNEL = "conv_bf16_kernel"


def _torch():
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
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("conv_bf16_models")


def load(gpu, workdir, name, blob, conv_bf16=0):
    p = workdir / (name + ".tflite")
    p.write_bytes(blob)
    m = gpu.Model(str(p))
    m.set_option("conv_bf16", conv_bf16)
    assert m.get_option("conv_bf16") == conv_bf16
    return m


def labels_of(m, x):
    return [r["kernel"] for r in m.profile(_torch().from_numpy(x).cuda(), reps=1)]


# name: (conv_layer arguments, batch); the seeds follow test_resnet_gpu.py: 200 + / 300 + the position among its sorted case names
_RESNET_CASES = ["a_3x3_s1_7x7x32_to_32", "b_3x3_s2_14x14x64_to_128", "b_3x3_s2_7x7x64_to_64", "c_3x3_s1_9x11x96_to_36", "d_pad_1111_valid_8x8x32_to_32",
                 "e_2x2_s2_valid_8x8x32_to_64", "f_skip_behind_the_fused_relu", "f_skip_then_prelu", "g_c24_stays_generic"]   # sorted, as test_resnet_gpu.py numbers them
_ARGS = {
    "a_3x3_s1_7x7x32_to_32": (dict(h=7, w=7, c=32, co=32), 1),
    "b_3x3_s2_14x14x64_to_128": (dict(h=14, w=14, c=64, co=128, stride=2), 3),
    "b_3x3_s2_7x7x64_to_64": (dict(h=7, w=7, c=64, co=64, stride=2), 3),
    "c_3x3_s1_9x11x96_to_36": (dict(h=9, w=11, c=96, co=36), 2),
    "d_pad_1111_valid_8x8x32_to_32": (dict(h=8, w=8, c=32, co=32, padding=VALID, explicit_pad=(1, 1, 1, 1)), 2),
    "e_2x2_s2_valid_8x8x32_to_64": (dict(h=8, w=8, c=32, co=64, k=2, stride=2, padding=VALID), 2),
    "f_skip_behind_the_fused_relu": (dict(h=7, w=7, c=32, co=32, skip="act_then_add"), 1),
    "f_skip_then_prelu": (dict(h=7, w=7, c=32, co=32, skip="add_then_prelu"), 1),
    "g_c24_stays_generic": (dict(h=7, w=7, c=24, co=32), 2),
    # new: Co over two 128-wide tiles, the last one ragged;  25 taps
    "h_5x5x32_to_160": (dict(h=5, w=5, c=32, co=160), 2),
    "i_k5_6x6x32_to_32": (dict(h=6, w=6, c=32, co=32, k=5), 2),
}
_NEW_SEEDS = {"h_5x5x32_to_160": 20, "i_k5_6x6x32_to_32": 21}
OUTSIDE = ["e_2x2_s2_valid_8x8x32_to_64", "g_c24_stays_generic"]
INSIDE = [n for n in sorted(_ARGS) if n not in OUTSIDE]


def case(name, batch=None):
    """(blob, constants, input): test_resnet_gpu.py's draws for its cases"""
    kw, B = _ARGS[name]
    idx = _RESNET_CASES.index(name) if name in _RESNET_CASES else _NEW_SEEDS[name]
    blob, cs = rs.conv_layer(200 + idx, **kw)
    x = np.random.RandomState(300 + idx).standard_normal((batch or B, kw["h"], kw["w"], kw["c"])).astype(np.float32)
    return blob, cs, x


@pytest.mark.parametrize("name", INSIDE)
def test_single_layer_within_the_derived_bound(gpu, workdir, name):
    blob, cs, x = case(name)
    m = load(gpu, workdir, name, blob)
    for value in (1, 2):
        m.set_option("conv_bf16", value)
        assert labels_of(m, x) == [KERNEL]
        cb.check_layer(m.run(x)[0], x, cs, value, name)
    m.close()


def test_the_option_does_not_look_at_conv_mfma(gpu, workdir):
    blob, cs, x = case("c_3x3_s1_9x11x96_to_36")
    m = load(gpu, workdir, "c_no_mfma", blob, 2)
    y = m.run(x)[0]
    m.set_option("conv_mfma", 0)
    assert labels_of(m, x) == [KERNEL]
    np.testing.assert_array_equal(m.run(x)[0], y)
    m.close()


@pytest.mark.parametrize("name", OUTSIDE)
def test_layers_outside_the_rule_keep_their_kernel_and_their_bits(gpu, workdir, name):
    blob, cs, x = case(name)
    m = load(gpu, workdir, name, blob)
    labels0, y0 = labels_of(m, x), m.run(x)[0]
    assert KERNEL not in labels0 and len(labels0) == 1
    for value in (1, 2):
        m.set_option("conv_bf16", value)
        assert labels_of(m, x) == labels0
        np.testing.assert_array_equal(m.run(x)[0], y0)
    m.close()


# launch_conv_bf16 (conv_bf16_kernels.hip): 128 x 64 tiles where Co <= 64 or ceil(M / 128) * ceil(Co / 128) < the device's compute units, 128 x 128
# tiles otherwise.  Co = 160 on 5 x 5 frames: ceil(Co / 128) = 2 and M = 25 B, so B = 2 (one row tile: 2 < CUs) takes TN = 64, and B = 656
# (M = 16 400, 129 row tiles: 258) takes TN = 128 on every device of at most 258 compute units (the MI355X has 256; the test checks the count).
TN64_BATCH, TN128_BATCH, TN128_TILES = 2, 656, 258


@pytest.mark.parametrize("value", [1, 2])
@pytest.mark.parametrize("name", ["b_3x3_s2_14x14x64_to_128", "b_3x3_s2_7x7x64_to_64", "c_3x3_s1_9x11x96_to_36", "h_5x5x32_to_160"])
def test_bits_do_not_depend_on_the_batch_the_tile_width_or_the_run(gpu, workdir, name, value):
    blob, cs, x = case(name)
    m = load(gpu, workdir, name + "_bits%d" % value, blob, value)
    y = m.run(x)[0]
    np.testing.assert_array_equal(m.run(x)[0], y)   # two runs of the batch
    for i in range(len(x)):                         # frame i alone
        np.testing.assert_array_equal(m.run(x[i:i + 1])[0][0], y[i], err_msg="frame %d" % i)
    if name == "h_5x5x32_to_160":
        cus = _torch().cuda.get_device_properties(0).multi_processor_count
        assert 2 < cus <= TN128_TILES, cus          # (what makes TN64_BATCH / TN128_BATCH the two sides of the launcher's rule)
        assert len(x) == TN64_BATCH
        _, _, big = case(name, TN128_BATCH)
        big[0], big[TN128_BATCH - 1] = x[0], x[1]   # the shared frames: the first rows of the first tile, the last rows of the last (ragged) one
        yb = m.run(big)[0]
        np.testing.assert_array_equal(yb[0], y[0])
        np.testing.assert_array_equal(yb[TN128_BATCH - 1], y[1])
        cb.check_layer(yb[-3:], big[-3:], cs, value, name + ", the last frames of %d" % TN128_BATCH)
    m.close()


def test_back_to_0_gives_the_bits_of_a_fresh_handle(gpu, workdir):
    blob, cs, x = case("c_3x3_s1_9x11x96_to_36")
    fresh = load(gpu, workdir, "c_fresh", blob)
    y0 = fresh.run(x)[0]
    m = load(gpu, workdir, "c_there_and_back", blob, 2)
    y2 = m.run(x)[0]
    assert not np.array_equal(y2, y0)
    m.set_option("conv_bf16", 0)
    assert labels_of(m, x) == labels_of(fresh, x) == ["conv_mfma_kernel"]
    np.testing.assert_array_equal(m.run(x)[0], y0)
    m.set_option("conv_bf16", 1)
    m.run(x)
    m.set_option("conv_bf16", 0)
    np.testing.assert_array_equal(m.run(x)[0], y0)
    m.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------- the network
NETWORK = (3, 128, (1, 1, 1, 1))


@pytest.fixture(scope="module")
def chips():
    return np.random.RandomState(11).uniform(0, 1, (5, 112, 112, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def network(gpu, oracle, workdir, chips):
    """the oracle's evaluation of the twin and the engine's raw outputs at value 0, computed once"""
    seed, features, blocks = NETWORK
    p = workdir / "net_twin.tflite"
    p.write_bytes(rs.iresnet_like(seed, features, blocks=blocks, twin=True))
    ref = oracle.Model(str(p)).run(chips, nthreads=8)[0].reshape(len(chips), features)
    m = load(gpu, workdir, "net", rs.iresnet_like(seed, features, blocks=blocks))
    raw0 = m.run(chips)[0].reshape(5, features).copy()
    yield m, ref, raw0
    m.close()


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.parametrize("value", [1, 2])
def test_network_against_the_oracle_on_its_twin(gpu, chips, network, value):
    m, ref, raw0 = network
    _, features, blocks = NETWORK
    m.set_option("conv_bf16", value)
    labels = labels_of(m, chips)
    assert labels.count(KERNEL) == 2 * sum(blocks) and "conv_mfma_kernel" not in labels, labels
    assert labels.count("affine_kernel") == sum(blocks) + 1 and "head_gemm_kernel" in labels, labels
    y5, y1 = m.run(chips)[0].reshape(5, features), m.run(chips[:1])[0].reshape(1, features)
    np.testing.assert_array_equal(y5[0], y1[0])   # item 0 of the batch of five is the single item, bit for bit
    bound = RAW_TOL * max(1.0, float(np.abs(ref).max()))
    err0, err = float(np.abs(raw0 - ref).max()), float(np.abs(y5 - ref).max())
    print("conv_bf16 = %d: max |raw - oracle(twin)| = %.3g (value 0: %.3g), bound %.3g (max |oracle| = %.3g)" % (value, err, err0, bound, float(np.abs(ref).max())))
    rel = float(np.abs(y5 - raw0).max() / np.abs(raw0).max())
    cos = float((_unit(y5.astype(np.float64)) * _unit(raw0.astype(np.float64))).sum(axis=1).min())
    print("conv_bf16 = %d: max |raw - raw0| / max |raw0| = %.3g, smallest cosine against value 0 = %.8f" % (value, rel, cos))
    assert np.isfinite(y5).all()
    if value == 2:
        assert err <= bound, (err, bound)
    else:   # its per-layer bound is its accuracy test
        assert not np.array_equal(y5, raw0)
    m.set_option("conv_bf16", 0)
    np.testing.assert_array_equal(m.run(chips)[0].reshape(5, features), raw0)


def test_face_embeddings_precision(gpu):
    """tests/test_resnet_gpu.py's FaceEmbeddings flow at precision="bf16x3": infer is l2_norm of infer_items' raw output, bit for bit"""
    from PIL import Image
    seed, features, blocks = NETWORK
    blob = rs.iresnet_like(seed, features, blocks=blocks)
    fe = gpu.FaceEmbeddings(model_bytes=blob, precision="bf16x3")
    assert fe.precision == "bf16x3" and fe.model.get_option("conv_bf16") == 2 and fe.features == 128
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    image = np.asarray(Image.open(os.path.join(GOLDEN, "russ_cox_1.jpg")).convert("RGB"))
    H, W = image.shape[:2]
    faces = fd.infer(image)
    assert len(faces) >= 1
    b = faces[0].bbox()
    e = fe.infer(image, (b[0] * float(W), b[1] * float(H), b[2] * float(W), b[3] * float(H)))
    assert e.shape == (1, 128) and e.dtype == np.float32 and np.isfinite(e).all()
    det17 = np.concatenate([np.asarray(faces[0].data, np.float32).reshape(-1), [np.float32(faces[0].score)]]).astype(np.float32)
    one = dict(faces=det17.reshape(1, 1, 17), item_frame=np.zeros(1, np.int32), item_face=np.zeros(1, np.int32))
    out = fe.infer_items(image[None], one, want_raw=True)
    assert out["valid"][0] == 1
    np.testing.assert_array_equal(e[0], gpu.l2_norm(out["raw"][0]))
    np.testing.assert_array_equal(e[0], out["embeddings"][0])
    # the other two settings read back, and f32 is another embedding
    f32 = gpu.FaceEmbeddings(model_bytes=blob)
    bf16 = gpu.FaceEmbeddings(model_bytes=blob, precision="bf16")
    assert f32.precision == "f32" and bf16.precision == "bf16"
    e0 = f32.infer(image, (b[0] * float(W), b[1] * float(H), b[2] * float(W), b[3] * float(H)))
    assert not np.array_equal(e0, e) and float((e0[0].astype(np.float64) * e[0]).sum()) > 0.9999
    for h in (fe, f32, bf16, fd):
        h.close()
