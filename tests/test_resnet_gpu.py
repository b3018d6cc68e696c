"""ResNet-style embedding graphs on the device: conv_mfma_kernel (the dense convolutions on the f32 matrix cores) layer by layer against a
float64 evaluation with a derived bound, its bits against batch size and run, the synthetic network against the oracle's evaluation of its twin,
FaceEmbeddings on such a model, and the affine launch bit for bit.

Bound of a single layer, per output element, derived and not tuned: (K + 4) 2^-24 (sum |x w| + |bias| + |skip|) — the standard bound of an f32
sum of K products in any order, plus the epilogue's adds (resnet_synth.conv_layer_ref).  Every case prints its worst error / bound.

Case e (2x2 stride 2): the issue asked for conv_mfma_kernel here too.  The shipped iris graph has 2x2 stride-2 convolutions with 64 and 128 input
channels, and its pinned launch lists (tests/golden/launch_pins.json, fuse = 2) would have changed; the selection rule was narrowed instead, as the
issue prescribes, to windows that overlap (not k x k stride k).  The case stays, on the kernel the rule gives it, within the same bound."""
import os

import numpy as np
import pytest

import resnet_synth as rs
from conftest import GOLDEN
from synth_tflite import SAME, VALID

pytestmark = pytest.mark.gpu
RAW_TOL = 1e-4   # x max(1, max|ref|): the tolerance tests/test_gpu_parity.py uses for raw outputs of shipped and synthetic graphs


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
    return tmp_path_factory.mktemp("resnet_models")


def load(gpu, workdir, name, blob, conv_mfma=1):
    p = workdir / (name + ".tflite")
    p.write_bytes(blob)
    m = gpu.Model(str(p))
    m.set_option("conv_mfma", conv_mfma)
    assert m.get_option("conv_mfma") == conv_mfma
    return m


def labels_of(m, x):
    return [r["kernel"] for r in m.profile(_torch().from_numpy(x).cuda(), reps=1)]


# name: (conv_layer arguments, batch, the kernel the selection rule gives the layer)
LAYERS = {
    # 49 rows: less than one tile, padding on all four sides
    "a_3x3_s1_7x7x32_to_32": (dict(h=7, w=7, c=32, co=32), 1, "conv_mfma_kernel"),
    # stride 2 on an even size (TF SAME pads bottom / right only) and on an odd one; three frames: a tile holds pixels of several frames
    "b_3x3_s2_14x14x64_to_128": (dict(h=14, w=14, c=64, co=128, stride=2), 3, "conv_mfma_kernel"),
    "b_3x3_s2_7x7x64_to_64": (dict(h=7, w=7, c=64, co=64, stride=2), 3, "conv_mfma_kernel"),
    # three K chunks a tap, ragged Co, a frame that is not square; 198 rows: a tile boundary inside a frame
    "c_3x3_s1_9x11x96_to_36": (dict(h=9, w=11, c=96, co=36), 2, "conv_mfma_kernel"),
    "d_pad_1111_valid_8x8x32_to_32": (dict(h=8, w=8, c=32, co=32, padding=VALID, explicit_pad=(1, 1, 1, 1)), 2, "conv_mfma_kernel"),
    "e_2x2_s2_valid_8x8x32_to_64": (dict(h=8, w=8, c=32, co=64, k=2, stride=2, padding=VALID), 2, None),   # (see the module's docstring)
    "f_skip_behind_the_fused_relu": (dict(h=7, w=7, c=32, co=32, skip="act_then_add"), 1, "conv_mfma_kernel"),
    "f_skip_then_prelu": (dict(h=7, w=7, c=32, co=32, skip="add_then_prelu"), 1, "conv_mfma_kernel"),
    "g_c24_stays_generic": (dict(h=7, w=7, c=24, co=32), 2, "conv_generic_kernel"),
}


def layer_input(name, B, cs_kwargs):
    seed = sorted(LAYERS).index(name)
    return np.random.RandomState(300 + seed).standard_normal((B, cs_kwargs["h"], cs_kwargs["w"], cs_kwargs["c"])).astype(np.float32)


def check_layer(y, x, cs, what):
    ref, bound = rs.conv_layer_ref(x, cs)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    ratio = float((np.abs(y.astype(np.float64) - ref) / bound).max())
    print("%s: worst |error| / bound = %.3f (max |ref| = %.3g, K = %d)" % (what, ratio, float(np.abs(ref).max()), cs["k"] ** 2 * x.shape[3]))
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_single_layer_within_the_derived_bound(gpu, workdir, name):
    kw, B, kernel = LAYERS[name]
    blob, cs = rs.conv_layer(200 + sorted(LAYERS).index(name), **kw)
    x = layer_input(name, B, kw)
    m = load(gpu, workdir, name, blob)
    labels = labels_of(m, x)
    if kernel is not None:
        assert labels == [kernel], labels
    else:
        assert "conv_mfma_kernel" not in labels and len(labels) == 1, labels
    check_layer(m.run(x)[0], x, cs, name)
    m.close()


def test_folded_pad_gives_the_bits_of_same_padding(gpu, workdir):
    """case d: PAD (1,1,1,1) + VALID on the weights of a SAME convolution (same seed, same draws)"""
    kw = dict(h=8, w=8, c=32, co=32)
    blob_pad, _ = rs.conv_layer(77, padding=VALID, explicit_pad=(1, 1, 1, 1), **kw)
    blob_same, cs = rs.conv_layer(77, padding=SAME, **kw)
    x = np.random.RandomState(78).standard_normal((2, 8, 8, 32)).astype(np.float32)
    a, b = load(gpu, workdir, "d_pad", blob_pad), load(gpu, workdir, "d_same", blob_same)
    assert labels_of(a, x) == ["conv_mfma_kernel"] and labels_of(b, x) == ["conv_mfma_kernel"]
    ya, yb = a.run(x)[0], b.run(x)[0]
    np.testing.assert_array_equal(ya, yb)
    check_layer(yb, x, cs, "d, SAME")
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["b_3x3_s2_14x14x64_to_128", "b_3x3_s2_7x7x64_to_64", "c_3x3_s1_9x11x96_to_36"])
def test_bits_do_not_depend_on_the_batch_or_the_run(gpu, workdir, name):
    kw, B, _ = LAYERS[name]
    blob, cs = rs.conv_layer(200 + sorted(LAYERS).index(name), **kw)
    x = layer_input(name, B, kw)
    m = load(gpu, workdir, name + "_bits", blob)
    y = m.run(x)[0]
    np.testing.assert_array_equal(m.run(x)[0], y)   # two runs of the batch
    for i in range(B):                              # frame i alone
        np.testing.assert_array_equal(m.run(x[i:i + 1])[0][0], y[i], err_msg="frame %d" % i)
    # the parent's kernel on the same yardstick
    m.set_option("conv_mfma", 0)
    assert labels_of(m, x) == ["conv_generic_kernel"]
    check_layer(m.run(x)[0], x, cs, name + ", conv_mfma = 0")
    m.close()


# ---------------------------------------------------------------------------------------------------- the network
NETWORKS = {"c32_128": (3, 128, (1, 1, 1, 1)), "c32_512_two_blocks": (4, 512, (2, 1, 1, 1))}


@pytest.fixture(scope="module")
def chips():
    return np.random.RandomState(11).uniform(0, 1, (5, 112, 112, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def twin_outputs(oracle, workdir, chips):
    """name -> the oracle's evaluation of the network's twin on the five chips, computed once"""
    made = {}

    def get(name):
        if name not in made:
            seed, features, blocks = NETWORKS[name]
            p = workdir / (name + "_twin.tflite")
            p.write_bytes(rs.iresnet_like(seed, features, blocks=blocks, twin=True))
            made[name] = oracle.Model(str(p)).run(chips, nthreads=8)[0].reshape(len(chips), features)
        return made[name]
    return get


@pytest.mark.parametrize("name", sorted(NETWORKS))
def test_network_against_the_oracle_on_its_twin(gpu, workdir, chips, twin_outputs, name):
    seed, features, blocks = NETWORKS[name]
    ref = twin_outputs(name)
    m = load(gpu, workdir, name, rs.iresnet_like(seed, features, blocks=blocks))
    labels = labels_of(m, chips)
    assert labels.count("conv_mfma_kernel") == 2 * sum(blocks) and labels.count("affine_kernel") == sum(blocks) + 1 and "head_gemm_kernel" in labels, labels
    y5, y1 = m.run(chips)[0].reshape(5, features), m.run(chips[:1])[0].reshape(1, features)
    bound = RAW_TOL * max(1.0, float(np.abs(ref).max()))
    for what, got, want in (("B = 5", y5, ref), ("B = 1", y1, ref[:1])):
        err = float(np.abs(got - want).max())
        print("%s %s: max |raw - oracle(twin)| = %.3g, bound %.3g (max |oracle| = %.3g)" % (name, what, err, bound, float(np.abs(ref).max())))
        assert err <= bound, (name, what, err, bound)
    np.testing.assert_array_equal(y5[0], y1[0])   # item 0 of the batch of five is the single item, bit for bit
    m.close()


def test_face_embeddings_on_the_network(gpu, workdir):
    """the flow of test_embeddings_gpu.py's reference test, with the ResNet-style model: BackCamera's first box on a picture, infer, and the
    batched entry on two frames"""
    from PIL import Image
    seed, features, blocks = NETWORKS["c32_128"]
    fe = gpu.FaceEmbeddings(model_bytes=rs.iresnet_like(seed, features, blocks=blocks))
    assert fe.features == 128
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
    out1 = fe.infer_items(image[None], one, want_raw=True)
    assert out1["valid"][0] == 1
    np.testing.assert_array_equal(e[0], gpu.l2_norm(out1["raw"][0]))
    np.testing.assert_array_equal(e[0], out1["embeddings"][0])
    two = dict(faces=np.stack([det17.reshape(1, 17)] * 2), item_frame=np.array([0, 1], np.int32), item_face=np.zeros(2, np.int32))
    out2 = fe.infer_items(np.stack([image, image[:, ::-1]]), two, want_raw=True)
    assert list(out2["valid"]) == [1, 1]
    np.testing.assert_array_equal(out2["raw"][0], out1["raw"][0])
    np.testing.assert_array_equal(out2["embeddings"][0], e[0])
    np.testing.assert_array_equal(out2["embeddings"][1], gpu.l2_norm(out2["raw"][1]))
    assert not np.array_equal(out2["raw"][1], out2["raw"][0])   # the mirrored frame is another chip
    fe.close()
    fd.close()


@pytest.mark.parametrize("c", [7, 20, 32])   # (7: the scalar form; 20 and 32: float4)
def test_affine_launch_bit_for_bit(gpu, workdir, c):
    """input -> MUL -> ADD -> PRELU as one launch against numpy float32 in the same order, fl(fl(x s) + t): a separate multiply and add"""
    blob, s, t, alpha = rs.affine_graph(40 + c, c)
    x = np.random.RandomState(50 + c).standard_normal((3, 5, 7, c)).astype(np.float32)
    m = load(gpu, workdir, "affine_%d" % c, blob)
    assert labels_of(m, x) == ["affine_kernel"]
    v = (x * s).astype(np.float32) + t
    assert v.dtype == np.float32
    want = np.where(v >= 0, v, (alpha * v).astype(np.float32)).astype(np.float32)
    np.testing.assert_array_equal(m.run(x)[0], want)
    m.close()


def test_widened_affine_computes_what_the_unwidened_graph_computes(gpu, workdir):
    """pad_odd_channels through a MUL / ADD pair (30 -> 32 channels, scale 1 and shift 0 appended): fuse 5 against the op-by-op plan, which widens nothing"""
    x = np.random.RandomState(12).uniform(-1, 1, (3, 16, 16, 3)).astype(np.float32)
    m = load(gpu, workdir, "odd_width", rs.odd_width_graph(10))
    assert "affine_kernel" in labels_of(m, x)
    y5 = m.run(x)[0]
    m.set_option("fuse", 0)
    y0 = m.run(x)[0]
    err, bound = float(np.abs(y5 - y0).max()), RAW_TOL * max(1.0, float(np.abs(y0).max()))
    print("widened affine: max |fuse 5 - fuse 0| = %.3g, bound %.3g" % (err, bound))
    assert err <= bound and float(np.abs(y0).max()) > 1e-2
    m.close()
