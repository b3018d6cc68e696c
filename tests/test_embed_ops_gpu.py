"""AVERAGE_POOL_2D, MEAN, L2_NORMALIZATION, SUB, DIV and TRANSPOSE on the device (embed_ops_kernels.hip, the divisor form of affine_kernel): every
operator bit for bit against its restatement in tests/embed_ops_synth.py (one k-ordered f32 chain per output element) and inside the float64 bound
derived there; the bits against batch size and run; the pooled-head network against the oracle's evaluation of its twin; the ONNX-style network
(csrc/layout.hpp removes its transposes) bit for bit against its NHWC writing and against the oracle; FaceEmbeddings on both.

Shapes are H x W x C.  RAW_TOL is the project's standard for raw outputs: 1e-4 x max(1, max |ref|)."""
import os

import numpy as np
import pytest

import embed_ops_synth as es
from conftest import GOLDEN
from synth_tflite import ACT_NONE, ACT_RELU, SAME, VALID

pytestmark = pytest.mark.gpu
RAW_TOL = 1e-4


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
    return tmp_path_factory.mktemp("embed_ops_models")


def load(gpu, workdir, name, blob, fuse=None):
    p = workdir / (name + ".tflite")
    p.write_bytes(blob)
    m = gpu.Model(str(p))
    if fuse is not None:
        m.set_option("fuse", fuse)
    return m


def labels_of(m, x):
    return [r["kernel"] for r in m.profile(_torch().from_numpy(x).cuda(), reps=1)]


def frames(seed, b, h, w, c):
    return np.random.RandomState(seed).standard_normal((b, h, w, c)).astype(np.float32)


def within(y, ref, bound, what):
    ratio = float((np.abs(y.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())
    print("%s: worst |error| / bound = %.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


# ---------------------------------------------------------------------------------------------------- average pool / MEAN
POOLS = {
    # name: (H, W, C, kh, kw, stride, padding, activation, frames)
    "global_7x7x40_valid": (7, 7, 40, 7, 7, 1, VALID, ACT_NONE, 3),
    "3x3_s2_same_9x11x12_edge_windows": (9, 11, 12, 3, 3, 2, SAME, ACT_NONE, 2),   # edge windows have fewer taps
    "2x2_s2_valid_8x8x7_scalar_relu": (8, 8, 7, 2, 2, 2, VALID, ACT_RELU, 2),      # C = 7: the scalar path
}


@pytest.mark.parametrize("name", sorted(POOLS))
def test_average_pool_bit_for_bit_and_within_the_bound(gpu, workdir, name):
    h, w, c, kh, kw, s, padding, act, b = POOLS[name]
    x = frames(400 + sorted(POOLS).index(name), b, h, w, c)
    m = load(gpu, workdir, name, es.avgpool_graph(h, w, c, kh, kw, s, padding, act))
    assert labels_of(m, x) == ["avgpool_kernel"]
    y = m.run(x)[0]
    want = es.avgpool_ref(x, kh, kw, s, padding, act)
    assert y.shape == want.shape
    np.testing.assert_array_equal(y, want)
    within(y, *es.avgpool_f64(x, kh, kw, s, padding, act), name)
    m.close()


@pytest.mark.parametrize("keep_dims", [True, False])
@pytest.mark.parametrize("axes", [(1, 2), (-3, -2)])
@pytest.mark.parametrize("h,w,c", [(7, 7, 40), (5, 3, 7)])
def test_mean_is_the_whole_frame_average_pool(gpu, workdir, h, w, c, axes, keep_dims):
    x = frames(410 + c, 3, h, w, c)
    tag = "%dx%dx%d_%s_%d" % (h, w, c, "neg" if axes[0] < 0 else "pos", keep_dims)
    mm = load(gpu, workdir, "mean_" + tag, es.mean_graph(h, w, c, axes, keep_dims))
    mp = load(gpu, workdir, "meanpool_" + tag, es.avgpool_graph(h, w, c, h, w))
    assert labels_of(mm, x) == ["avgpool_kernel"]
    ym, yp = mm.run(x)[0], mp.run(x)[0]
    assert ym.shape == ((3, 1, 1, c) if keep_dims else (3, c)), ym.shape
    np.testing.assert_array_equal(ym.reshape(3, c), yp.reshape(3, c))
    np.testing.assert_array_equal(yp, es.avgpool_ref(x, h, w))
    mm.close()
    mp.close()


# ---------------------------------------------------------------------------------------------------- L2_NORMALIZATION
@pytest.mark.parametrize("shape", [(1, 128), (1, 1, 1, 37), (1, 4, 4, 8)])
def test_l2_normalization_bit_for_bit_and_within_the_bound(gpu, workdir, shape):
    n = int(np.prod(shape))
    in_shape = shape if len(shape) == 4 else (1, 1, 1, n)
    x = np.random.RandomState(420 + n).standard_normal((3,) + tuple(in_shape[1:])).astype(np.float32)
    x.reshape(3, -1, shape[-1])[1, 0] = 0.0   # one all-zero row: zeros, no NaN
    m = load(gpu, workdir, "l2norm_%d_%d" % (len(shape), n), es.l2norm_graph(shape))
    assert labels_of(m, x) == ["l2norm_rows_kernel<wave per row>"]
    y = m.run(x)[0]
    rows = x.reshape(3, -1, shape[-1])
    want = es.l2norm_ref(rows)
    np.testing.assert_array_equal(y.reshape(want.shape), want)
    assert np.isfinite(y).all() and not y.reshape(want.shape)[1, 0].any()
    within(y.reshape(want.shape), *es.l2norm_f64(rows), "l2norm %s" % (shape,))
    m.close()


def test_l2_normalization_thread_per_row_form(gpu, workdir):
    """[1,24,24,8]: 576 rows a frame, four frames: past the row count at which a thread takes a row; the same bits"""
    x = frames(431, 4, 24, 24, 8)
    m = load(gpu, workdir, "l2norm_rows", es.l2norm_graph((1, 24, 24, 8)))
    assert labels_of(m, x) == ["l2norm_rows_kernel<thread per row>"]
    assert labels_of(m, x[:1]) == ["l2norm_rows_kernel<wave per row>"]
    y = m.run(x)[0]
    np.testing.assert_array_equal(y, es.l2norm_ref(x))
    np.testing.assert_array_equal(m.run(x[:1])[0][0], y[0])   # the other form on frame 0: the same chain
    m.close()


# ---------------------------------------------------------------------------------------------------- SUB / DIV
def _arith_cases(c):
    rs = np.random.RandomState(440 + c)
    per = rs.uniform(0.5, 3.0, c).astype(np.float32) * np.where(rs.rand(c) < 0.3, -1, 1).astype(np.float32)
    return {
        "x-c": ("x-c", per, lambda x: x - per),
        "c-x": ("c-x", per, lambda x: per - x),
        "x/128": ("x/c", np.float32(128.0), lambda x: x / np.float32(128.0)),
        "x/c": ("x/c", per, lambda x: x / per),
        "x-scalar": ("x-c", np.float32(0.4), lambda x: x - np.float32(0.4)),
        "x/scalar": ("x/c", np.float32(3.0), lambda x: x / np.float32(3.0)),
    }


@pytest.mark.parametrize("case", ["x-c", "c-x", "x/128", "x/c", "x-scalar", "x/scalar"])
@pytest.mark.parametrize("c", [7, 32])   # (7: the scalar form; 32: float4)
def test_sub_and_div_by_constants(gpu, workdir, c, case):
    kind, const, f = _arith_cases(c)[case]
    x = frames(450 + c, 3, 5, 7, c)
    want = f(x)
    assert want.dtype == np.float32
    m = load(gpu, workdir, "arith_%d_%s" % (c, case.replace("/", "div").replace("-", "sub")), es.arith_graph(kind, c, const=const), fuse=0)
    assert labels_of(m, x) == ["affine_kernel"]
    np.testing.assert_array_equal(m.run(x)[0], want)   # fuse 0: the operator's own bits
    m.set_option("fuse", 5)
    y5 = m.run(x)[0]
    err, bound = float(np.abs(y5 - want).max()), RAW_TOL * max(1.0, float(np.abs(want).max()))
    print("%s C = %d, fuse 5: max |error| = %.3g, bound %.3g" % (case, c, err, bound))
    assert err <= bound
    m.close()


# ---------------------------------------------------------------------------------------------------- TRANSPOSE
TILED = {(0, 3, 1, 2), (0, 2, 3, 1)}


@pytest.mark.parametrize("back", [False, True])
@pytest.mark.parametrize("h,w,c,b,perm", [(5, 7, 3, 2, (0, 3, 1, 2)), (5, 7, 3, 2, (0, 2, 3, 1)), (5, 7, 3, 2, (0, 2, 1, 3)), (5, 7, 3, 2, (0, 1, 3, 2)),
                                          (33, 35, 40, 3, (0, 3, 1, 2)), (33, 35, 40, 3, (0, 2, 3, 1))])
def test_transpose_equals_numpy(gpu, workdir, h, w, c, b, perm, back):
    """as the graph's output, and followed by its inverse; 33 x 35 x 40 crosses the 32 x 32 tiles' edges in both directions"""
    x = frames(460 + h, b, h, w, c)
    m = load(gpu, workdir, "transpose_%d_%s_%d" % (h, "".join(map(str, perm)), back), es.transpose_graph(h, w, c, perm, back))
    inv = tuple(int(i) for i in np.argsort(perm))
    kernel = lambda p: "transpose_tiled_kernel" if p in TILED else "transpose_kernel"   # noqa: E731
    assert labels_of(m, x) == [kernel(perm)] + ([kernel(inv)] if back else [])
    np.testing.assert_array_equal(m.run(x)[0], x if back else np.transpose(x, perm))
    m.close()


# ---------------------------------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("name", ["pool", "l2norm", "transpose"])
def test_bits_do_not_depend_on_the_batch_or_the_run(gpu, workdir, name):
    blob, shape = {"pool": (es.avgpool_graph(9, 11, 12, 3, 3, 2, SAME), (9, 11, 12)), "l2norm": (es.l2norm_graph((1, 4, 4, 8)), (4, 4, 8)),
                   "transpose": (es.transpose_graph(33, 35, 40, (0, 3, 1, 2)), (33, 35, 40))}[name]
    x = frames(470, 5, *shape)
    m = load(gpu, workdir, "bits_" + name, blob)
    y5 = m.run(x)[0]
    np.testing.assert_array_equal(m.run(x)[0], y5)
    np.testing.assert_array_equal(m.run(x[:1])[0][0], y5[0])
    m.close()


# ---------------------------------------------------------------------------------------------------- the pooled-head network
@pytest.fixture(scope="module")
def chips():
    return np.random.RandomState(11).uniform(0, 1, (2, 112, 112, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def twin_vectors(oracle, workdir, chips):
    """the oracle's evaluation of pooled_head's twin on the chips (the vector in front of the L2_NORMALIZATION), computed once"""
    p = workdir / "pooled_twin.tflite"
    p.write_bytes(es.pooled_head(5, 128, twin=True))
    return oracle.Model(str(p)).run(chips, nthreads=8)[0].reshape(len(chips), 128)


@pytest.mark.parametrize("pool", ["avgpool", "mean", "mean_keep"])
def test_pooled_head_against_the_oracle_on_its_twin(gpu, workdir, chips, twin_vectors, pool):
    ref = es.l2norm_f64(twin_vectors)[0]
    m = load(gpu, workdir, "pooled_" + pool, es.pooled_head(5, 128, pool))
    labels = labels_of(m, chips)
    assert labels.count("avgpool_kernel") == 1 and labels.count("affine_kernel") == 2 and labels[-1] == "l2norm_rows_kernel<wave per row>", labels
    bound = RAW_TOL * max(1.0, float(np.abs(ref).max()))
    for fuse in (5, 0):
        m.set_option("fuse", fuse)
        y = m.run(chips)[0].reshape(2, 128)
        err = float(np.abs(y - ref).max())
        print("pooled_head(%s) fuse %d: max |raw - l2norm(oracle(twin))| = %.3g, bound %.3g" % (pool, fuse, err, bound))
        assert err <= bound, (pool, fuse, err, bound)
        np.testing.assert_allclose(np.sqrt((y.astype(np.float64) ** 2).sum(axis=1)), 1.0, atol=1e-5)
    m.close()


def test_face_embeddings_on_the_pooled_head(gpu):
    """FaceEmbeddings loads the pooled-head model from bytes; infer is l2_norm of the raw output; infer_items on a two-frame run_faces-shaped list"""
    from PIL import Image
    fe = gpu.FaceEmbeddings(model_bytes=es.pooled_head(5, 128))
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
    two = dict(faces=np.stack([det17.reshape(1, 17)] * 2), item_frame=np.array([0, 1], np.int32), item_face=np.zeros(2, np.int32))
    out = fe.infer_items(np.stack([image, image[:, ::-1]]), two, want_raw=True)
    assert list(out["valid"]) == [1, 1]
    np.testing.assert_array_equal(out["embeddings"][0], e[0])
    for k in (0, 1):
        np.testing.assert_array_equal(out["embeddings"][k], gpu.l2_norm(out["raw"][k]))
        assert abs(float(np.sqrt((out["raw"][k].astype(np.float64) ** 2).sum())) - 1.0) < 1e-5   # the model's own L2_NORMALIZATION
    assert not np.array_equal(out["raw"][1], out["raw"][0])   # the mirrored frame is another chip
    fe.close()
    fd.close()


# ---------------------------------------------------------------------------------------------------- the ONNX-exported idiom
@pytest.fixture(scope="module")
def onnx_twin_outputs(oracle, workdir, chips):
    """the oracle's evaluation of onnx_style's twin on the chips, computed once"""
    p = workdir / "onnx_twin.tflite"
    p.write_bytes(es.onnx_style(6, 128, layout="twin"))
    return oracle.Model(str(p)).run(chips, nthreads=8)[0].reshape(len(chips), 128)


def test_onnx_style_network_is_its_nhwc_network_bit_for_bit(gpu, workdir, chips, onnx_twin_outputs):
    """onnx_style(c0 = 32, blocks = (1, 1, 1, 1), D = 128) on two chips: the "nchw" writing (every TRANSPOSE removed by the layout normalisation) and the
    "nhwc" writing give the same bits at fuse 0 and 5, and both lie within RAW_TOL of the oracle's evaluation of the twin"""
    ref = onnx_twin_outputs
    bound = RAW_TOL * max(1.0, float(np.abs(ref).max()))
    a, b = load(gpu, workdir, "onnx_nchw", es.onnx_style(6, 128, layout="nchw")), load(gpu, workdir, "onnx_nhwc", es.onnx_style(6, 128, layout="nhwc"))
    la, lb = labels_of(a, chips), labels_of(b, chips)
    assert la == lb and not any("transpose" in k for k in la), (la, lb)
    for fuse in (5, 0):
        a.set_option("fuse", fuse)
        b.set_option("fuse", fuse)
        ya, yb = a.run(chips)[0].reshape(2, 128), b.run(chips)[0].reshape(2, 128)
        np.testing.assert_array_equal(ya, yb)
        err = float(np.abs(ya - ref).max())
        print("onnx_style fuse %d: max |raw - oracle(twin)| = %.3g, bound %.3g (max |oracle| = %.3g)" % (fuse, err, bound, float(np.abs(ref).max())))
        assert err <= bound, (fuse, err, bound)
    a.close()
    b.close()


def test_a_channel_first_output_is_the_transposed_nhwc_output(gpu, workdir, chips):
    """the one materialised TRANSPOSE of a network whose output stays channel-first: the NHWC network's feature map, transposed"""
    a = load(gpu, workdir, "onnx_map_nchw", es.onnx_style(6, 128, layout="nchw", out="feature_map"))
    b = load(gpu, workdir, "onnx_map_nhwc", es.onnx_style(6, 128, layout="nhwc", out="feature_map"))
    la = labels_of(a, chips)
    assert la[-1] == "transpose_tiled_kernel" and sum("transpose" in k for k in la) == 1 and la[:-1] == labels_of(b, chips), la
    ya, yb = a.run(chips)[0], b.run(chips)[0]
    assert ya.shape == (2, 256, 7, 7) and yb.shape == (2, 7, 7, 256)
    np.testing.assert_array_equal(ya, np.transpose(yb, (0, 3, 1, 2)))
    a.close()
    b.close()


def test_face_embeddings_loads_the_onnx_style_model(gpu):
    fe = gpu.FaceEmbeddings(model_bytes=es.onnx_style(6, 128, layout="nchw"))
    assert fe.features == 128
    image = np.random.RandomState(5).randint(0, 256, (240, 320, 3)).astype(np.uint8)
    e = fe.infer(image, (0.25 * 320, 0.25 * 240, 0.75 * 320, 0.75 * 240))
    assert e.shape == (1, 128) and np.isfinite(e).all() and abs(float(np.sqrt((e.astype(np.float64) ** 2).sum())) - 1.0) < 1e-5
    fe.close()
