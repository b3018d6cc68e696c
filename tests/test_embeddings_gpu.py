"""FaceEmbeddings on the device (face_embeddings.rs:22-109, utils.rs:30-50): the face chips of every item bit for bit against the oracle's
image_to_tensor of the numpy crop, the caller's network against the oracle's interpreter, l2_norm bit for bit against the host entry, item
counts on both sides of the engine's batch thresholds, the reference's own two-picture flow, and the cosine-similarity matrix on the f32
matrix cores against the sequential-float32 restatement.  The embedding networks are synthetic (embed_synth.embed_graph): the reference ships
no model, so the scores mean nothing — only that every stage computes what the reference's arithmetic computes."""
import os

import numpy as np
import pytest

import embed_synth as es
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RAW_TOL = 1e-4   # x max(1, max|ref|): the tolerance tests/test_gpu_parity.py uses for raw outputs of shipped and synthetic graphs
MODELS = {"d128_reshape": (128, True), "d512": (512, False)}
KINDS = {"back": "BackCamera", "full": "Full"}


def _torch():
    """torch carries the device-resident operands: on a GPU box a broken install is a failure, not a skip"""
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
def model_files(tmp_path_factory):
    """name -> path of the synthetic embedding network, generated once per module"""
    d = tmp_path_factory.mktemp("embed_models")
    paths = {}
    for i, (name, (features, reshape)) in enumerate(sorted(MODELS.items())):
        p = d / (name + ".tflite")
        p.write_bytes(es.embed_graph(71 + i, features, reshape))
        paths[name] = str(p)
    return paths


@pytest.fixture(scope="module")
def embedders(gpu, model_files):
    made = {}

    def get(name):
        if name not in made:
            made[name] = gpu.FaceEmbeddings(model_files[name])
        return made[name]
    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def oracle_models(oracle, model_files):
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle.Model(model_files[name])
        return made[name]
    return get


def oracle_chip(oracle, frame, rect):
    x, y, w, h = rect
    chip, _ = oracle.image_to_tensor(np.ascontiguousarray(frame[y:y + h, x:x + w]), None, (112, 112), False, (0., 1.), False)
    return chip


def check_raw(raw, ref, what):
    ref = ref.reshape(raw.shape)
    err, bound = float(np.abs(raw - ref).max()), RAW_TOL * max(1.0, float(np.abs(ref).max()))
    print("%s: max |raw - oracle| = %.3g, bound %.3g (max |oracle| = %.3g)" % (what, err, bound, float(np.abs(ref).max())))
    assert err <= bound, (what, err, bound)


def check_norm(gpu, out):
    """embeddings == mi_l2_norm(raw) row by row, bit for bit; zeros where valid is 0"""
    for j in range(len(out["valid"])):
        if out["valid"][j]:
            np.testing.assert_array_equal(out["embeddings"][j], gpu.l2_norm(out["raw"][j]))
        else:
            assert not out["embeddings"][j].any() and not out["raw"][j].any()
            if "chips" in out:
                assert not out["chips"][j].any()


# ---------------------------------------------------------------------------------------------------- 1. chips, bit for bit
CW, CH = 320, 240


def box_det(x, y, w, h):
    """a normalised detection whose rectangle is (x, y, w, h): a quarter pixel inside, so that f32 rounding cannot move a truncation"""
    d = np.zeros(17, np.float32)
    d[:4] = ((x + 0.25) / CW, (y + 0.25) / CH, (x + w + 0.5) / CW, (y + h + 0.5) / CH)
    return d


def raw_det(xmin, ymin, xmax, ymax):
    d = np.zeros(17, np.float32)
    d[:4] = (xmin, ymin, xmax, ymax)
    return d


# (frame, detection, the rectangle it must give, or None for an invalid one)
CHIP_ITEMS = [
    (0, box_det(0, 0, 1, 1), (0, 0, 1, 1)),
    (0, box_det(319, 239, 1, 1), (319, 239, 1, 1)),
    (1, box_det(17, 101, 2, 3), (17, 101, 2, 3)),
    (1, box_det(0, 0, CW, CH), (0, 0, CW, CH)),
    (2, box_det(100, 60, 112, 112), (100, 60, 112, 112)),
    (2, box_det(207, 129, 113, 111), (207, 129, 113, 111)),   # ends on the right and bottom edges
    (0, box_det(20, 203, 300, 37), (20, 203, 300, 37)),
    (0, raw_det(-1.2 / CW, 0.25, 0.5, 0.75), None),             # x = -1
    (1, raw_det(0.5, 0.25, 321.5 / CW, 0.75), None),            # x + w = W + 1
    (1, raw_det(0.5, 0.25, 0.5 + 0.5 / CW, 0.75), None),        # w = 0
    (2, raw_det(np.nan, 0.25, 0.5, np.nan), None),              # NaN
    (2, raw_det(0.25, 0.25, 1e30, 0.75), None),                 # saturates
]


@pytest.fixture(scope="module")
def chip_case(oracle):
    """frames with padded rows, the hand-made faces / item list, and per item the expected rectangle, validity and oracle chip"""
    rs = np.random.RandomState(29)
    stride = 3 * CW + 5
    buf = rs.randint(0, 256, (3, CH, stride)).astype(np.uint8)
    frames = buf[:, :, :3 * CW].reshape(3, CH, CW, 3)   # a view: rows stride bytes apart
    assert np.shares_memory(frames, buf) and frames.strides == (CH * stride, stride, 3, 1)
    F = 6
    faces = np.zeros((3, F, 17), np.float32)
    used = [0, 0, 0]
    item_frame, item_face, want = [], [], []
    for b, d, rect in CHIP_ITEMS:
        k = used[b]
        used[b] += 1
        faces[b, k] = d
        item_frame.append(b)
        item_face.append(k)
        got_rect, ok = es.chip_rect(d, CW, CH)
        assert ok == (rect is not None) and (rect is None or got_rect == rect), (d[:4], got_rect, ok)   # the case is what it claims to be
        want.append(rect)
    # the invalid kinds actually differ
    inv = [es.chip_rect(d, CW, CH)[0] for _, d, r in CHIP_ITEMS if r is None]
    assert inv[0][0] == -1 and inv[1][0] + inv[1][2] == CW + 1 and inv[2][2] == 0 and inv[3][0] == 0 and inv[3][3] == 0 and inv[4][2] == es.I32_MAX
    # an unused slot with a garbage face index, and a slot whose face index lies outside the array
    item_frame += [-1, 1]
    item_face += [123456789, F + 93]
    want += [None, None]
    chips = np.stack([oracle_chip(oracle, frames[b], r) if r is not None else np.zeros((112, 112, 3), np.float32)
                      for b, r in zip(item_frame, want)])
    result = dict(faces=faces, item_frame=np.asarray(item_frame, np.int32), item_face=np.asarray(item_face, np.int32))
    return buf, frames, result, want, chips


@pytest.mark.parametrize("where", ["host", "device"])
def test_chips_are_the_oracles_tensors_of_the_crops(gpu, embedders, chip_case, where):
    buf, frames, result, want, chips = chip_case
    fe = embedders("d128_reshape")
    if where == "device":
        torch = _torch()
        # rows padded on the device as well
        dframes = torch.from_numpy(buf).cuda()[:, :, :3 * CW].unflatten(2, (CW, 3))
        assert tuple(dframes.stride()) == (CH * (3 * CW + 5), 3 * CW + 5, 3, 1)
        out = fe.infer_items(dframes, {k: torch.from_numpy(v).cuda() for k, v in result.items()}, want_raw=True, want_chips=True)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        out = fe.infer_items(frames, result, want_raw=True, want_chips=True)
    np.testing.assert_array_equal(out["valid"], np.asarray([r is not None for r in want], np.int32))
    for j, r in enumerate(want):
        np.testing.assert_array_equal(out["chips"][j], chips[j], err_msg="item %d, rectangle %s" % (j, r))
    check_norm(gpu, out)
    assert out["embeddings"].shape == (len(want), 128) and out["raw"][out["valid"] == 1].any(axis=1).all()


# ---------------------------------------------------------------------------------------------------- 2. end to end on real detections
def canvases(img):
    """Canvases of 720 rows x 1080 columns from man.jpg (360 x 540) and its mirror image: four, three, two, one face(s), all black, noise."""
    H, W = img.shape[:2]
    mirror = img[:, ::-1]
    four = np.concatenate([np.concatenate([img, mirror], axis=1), np.concatenate([mirror, img], axis=1)], axis=0)
    three, two, one = four.copy(), four.copy(), np.zeros_like(four)
    three[H:, W:] = 0
    two[H:] = 0
    one[:H, :W] = img
    noise = np.random.RandomState(3).randint(0, 256, four.shape).astype(np.uint8)
    return np.stack([four, three, two, one, np.zeros_like(four), noise])


@pytest.fixture(scope="module")
def frames(man_image):
    f = canvases(man_image)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def run16(gpu, frames):
    """kind -> Pipeline.run_faces(the six canvases, max_faces = 4, max_items = 16) from host memory, once per detector"""
    cache = {}

    def get(kind):
        if kind not in cache:
            p = gpu.Pipeline(getattr(gpu.FaceDetectionModel, KINDS[kind]))
            cache[kind] = p.run_faces(frames, max_faces=4, max_items=16)
            p.close()
        return cache[kind]
    return get


@pytest.fixture(scope="module")
def item_reference(gpu, oracle, oracle_models, frames, run16):
    """(kind, model) -> {(frame, face): (rect, valid, oracle chip, oracle raw output)} for the items of run16(kind): the oracle's tensors of the
    crops face_chip_rect gives for the GPU's own faces, and the oracle's interpreter on them.  Computed once."""
    chips_cache, cache = {}, {}

    def get(kind, name):
        res = run16(kind)
        if kind not in chips_cache:
            per = {}
            for b, k in zip(res["item_frame"], res["item_face"]):
                if b >= 0:
                    rect, ok = gpu.face_chip_rect(res["faces"][b, k], (frames.shape[2], frames.shape[1]))
                    assert (rect, ok) == es.chip_rect(res["faces"][b, k], frames.shape[2], frames.shape[1])
                    per[(int(b), int(k))] = (rect, ok, oracle_chip(oracle, frames[b], rect) if ok else None)
            chips_cache[kind] = per
        if (kind, name) not in cache:
            per = chips_cache[kind]
            keys = [key for key in sorted(per) if per[key][1]]
            raw = oracle_models(name).run(np.stack([per[key][2] for key in keys]), nthreads=8)[0].reshape(len(keys), -1)
            cache[(kind, name)] = {key: per[key] + ((raw[keys.index(key)] if key in keys else None),) for key in per}
        return cache[(kind, name)]
    return get


def check_items(gpu, out, item_frame, item_face, ref, what):
    """every item of a call against the oracle: validity, chips bit for bit, raw outputs at RAW_TOL, embeddings == l2_norm(raw)"""
    got, want = [], []
    for j, (b, k) in enumerate(zip(item_frame, item_face)):
        rect, ok, chip, raw = ref[(int(b), int(k))] if b >= 0 else (None, False, None, None)
        assert bool(out["valid"][j]) == bool(ok), (what, j)
        if ok:
            np.testing.assert_array_equal(out["chips"][j], chip, err_msg="%s: item %d (frame %d face %d), rectangle %s" % (what, j, b, k, rect))
            got.append(out["raw"][j])
            want.append(raw)
    check_raw(np.stack(got), np.stack(want), what)
    check_norm(gpu, out)
    return len(got)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_detected_face_against_the_oracle(gpu, embedders, frames, run16, item_reference, kind, name):
    res = run16(kind)
    out = embedders(name).infer_items(frames, res, want_raw=True, want_chips=True)
    assert out["embeddings"].shape == (16, MODELS[name][0])
    n = check_items(gpu, out, res["item_frame"], res["item_face"], item_reference(kind, name), "%s %s" % (kind, name))
    assert n >= 10, "only %d valid items: the canvases hold 4 + 3 + 2 + 1 faces" % n
    assert not out["valid"][int(res["counts"][0]):].any()


def test_device_resident_items_equal_the_host_call(gpu, embedders, frames, run16):
    torch = _torch()
    res = run16("back")
    fe = embedders("d128_reshape")
    host = fe.infer_items(frames, res, want_raw=True, want_chips=True)
    dres = {k: torch.from_numpy(np.ascontiguousarray(res[k])).cuda() for k in ("faces", "item_frame", "item_face")}
    stream = torch.cuda.Stream()
    dev = fe.infer_items(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), dres, want_raw=True, want_chips=True, stream=stream.cuda_stream)
    stream.synchronize()
    for k in host:
        np.testing.assert_array_equal(dev[k].cpu().numpy(), host[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------- 3. item counts across plan thresholds
def resized_list(res, M):
    """run16's item list truncated, or padded by going round it again, to M items (its unused slots come round as well)"""
    idx = np.arange(M) % len(res["item_frame"])
    return dict(faces=res["faces"], item_frame=np.ascontiguousarray(res["item_frame"][idx]), item_face=np.ascontiguousarray(res["item_face"][idx]))


@pytest.mark.parametrize("M", [1, 31, 32, 33])
def test_item_counts_on_both_sides_of_the_batch_thresholds(gpu, embedders, frames, run16, item_reference, M):
    lst = resized_list(run16("back"), M)
    out = embedders("d128_reshape").infer_items(frames, lst, want_raw=True, want_chips=True)
    assert out["embeddings"].shape == (M, 128)
    check_items(gpu, out, lst["item_frame"], lst["item_face"], item_reference("back", "d128_reshape"), "max_items = %d" % M)


def test_scratch_regrowth_leaves_results_unchanged(gpu, model_files, frames, run16):
    fe = gpu.FaceEmbeddings(model_files["d128_reshape"])   # a fresh handle: its scratch grows, shrinks in use, grows no further
    res = run16("back")
    outs = [fe.infer_items(frames, resized_list(res, M), want_raw=True, want_chips=True) for M in (33, 1, 33)]
    fresh = gpu.FaceEmbeddings(model_files["d128_reshape"])
    one = fresh.infer_items(frames, resized_list(res, 1), want_raw=True, want_chips=True)
    for k in outs[0]:
        np.testing.assert_array_equal(outs[2][k], outs[0][k], err_msg=k)
        np.testing.assert_array_equal(outs[1][k], one[k], err_msg=k)
    fe.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------- 4. the reference's own flow
def test_reference_flow_on_the_two_russ_cox_pictures(gpu, oracle, embedders, oracle_models):
    """face_embeddings.rs:118-146: BackCamera infer, faces[0].bbox().scale(size), FaceEmbeddings::infer on both pictures, similarity_score"""
    from PIL import Image
    fd = gpu.FaceDetection(gpu.FaceDetectionModel.BackCamera)
    name = "d128_reshape"
    fe = embedders(name)
    embeddings = []
    for pic in ("russ_cox_1.jpg", "russ_cox_2.jpg"):
        image = np.asarray(Image.open(os.path.join(GOLDEN, pic)).convert("RGB"))
        H, W = image.shape[:2]
        faces = fd.infer(image)
        assert len(faces) >= 1
        b = faces[0].bbox()
        bbox = (b[0] * float(W), b[1] * float(H), b[2] * float(W), b[3] * float(H))   # BBox::scale, in f64
        rect, ok = gpu.face_chip_rect(faces[0], (W, H))
        print(pic, "rectangle", rect, "valid", ok)
        assert ok and rect[2] > 50 and rect[3] > 50
        e = fe.infer(image, bbox)
        assert e.shape == (1, 128) and e.dtype == np.float32
        # the batched entry on the same box
        det17 = np.concatenate([np.asarray(faces[0].data, np.float32).reshape(-1), [np.float32(faces[0].score)]]).astype(np.float32)
        lst = dict(faces=det17.reshape(1, 1, 17), item_frame=np.zeros(1, np.int32), item_face=np.zeros(1, np.int32))
        out = fe.infer_items(image[None], lst, want_raw=True, want_chips=True)
        assert out["valid"][0] == 1
        np.testing.assert_array_equal(e[0], out["embeddings"][0])
        # the oracle chain, before normalisation
        chip = oracle_chip(oracle, image, rect)
        np.testing.assert_array_equal(out["chips"][0], chip)
        check_raw(out["raw"][0], oracle_models(name).run(chip[None])[0].reshape(-1), pic)
        np.testing.assert_array_equal(e[0], gpu.l2_norm(out["raw"][0]))
        embeddings.append(e)
        # where the reference panics: a box one pixel past the right edge
        with pytest.raises(gpu.MiError) as err:
            fe.infer(image, (W - 10.0, 0.0, W + 1.0, 10.0))
        assert err.value.code == -5   # MI_ERANGE
        fe.infer(image, (W - 10.0, 0.0, float(W), 10.0))   # ... and the box that ends on it is taken
        with pytest.raises(gpu.MiError) as err:
            fe.infer(image, bbox, cap=127)
        assert err.value.code == -1   # MI_EINVAL: cap < D
    score = gpu.similarity_score(embeddings[0].reshape(-1), embeddings[1].reshape(-1))
    np.testing.assert_array_equal(score, es.similarity_score_ref(embeddings[0], embeddings[1]))
    assert np.isfinite(score) and -1.0001 <= score <= 1.0001   # (a synthetic model: the value itself means nothing)
    fd.close()


def test_models_that_are_not_embedding_networks_are_refused(gpu, tmp_path):
    import synth_tflite as st
    cases = {"two outputs": es.embed_graph(9, 128, False, second_output=True), "input is not 112 x 112": st.iris_like(12, 32, 32, 64, 32, 3)}
    for what, blob in cases.items():
        with pytest.raises(gpu.MiError) as err:
            gpu.FaceEmbeddings(model_bytes=blob)
        assert err.value.code == -1 and "incompatible model" in str(err.value), (what, str(err.value))
    with pytest.raises(gpu.MiError) as err:
        gpu.FaceEmbeddings(str(tmp_path / "missing.tflite"))
    assert err.value.code == -2   # MI_EIO
    fe = gpu.FaceEmbeddings(model_bytes=es.embed_graph(5, 3, False))   # [1,1,1,D] with a small odd D
    assert fe.features == 3 and fe.model.input_dims == [1, 112, 112, 3]
    fe.close()


# ---------------------------------------------------------------------------------------------------- 5. similarity matrix
SIM_SHAPES = [(1, 1, 1), (33, 65, 130), (64, 256, 512), (5, 7, 4096)]


@pytest.fixture(scope="module")
def sim_cases():
    """(n, m, D) -> (a, b, the sequential-f32 restatement)"""
    cache = {}

    def get(shape):
        if shape not in cache:
            n, m, D = shape
            rs = np.random.RandomState(n * 1000 + m)
            a, b = rs.standard_normal((n, D)).astype(np.float32), rs.standard_normal((m, D)).astype(np.float32)
            if D > 1:
                # element 0 and element D-1 each carry half the norm: a dropped head or tail of K shows at the 0.1 level
                a[0], b[0] = 0.0, 0.0
                a[0, 0] = a[0, -1] = b[0, 0] = b[0, -1] = 2.0
                if n > 2:
                    a[2] = 0.0   # a zero row: 0 / 0
                if m > 3:
                    b[3] = 0.0
                    b[1] = a[min(1, n - 1)] * 3.0   # a parallel pair
            ref = es.similarity_matrix_ref(a, b)
            if D > 1:
                assert abs(ref[0, 0] - 1.0) < 1e-6 and (n <= 2 or np.isnan(ref[2]).all())
            cache[shape] = (a, b, ref)
        return cache[shape]
    return get


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape", SIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_similarity_matrix_against_the_sequential_f32_restatement(gpu, sim_cases, shape, where):
    n, m, D = shape
    a, b, ref = sim_cases(shape)
    if where == "device":
        torch = _torch()
        got = gpu.similarity_matrix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    else:
        got = gpu.similarity_matrix(a, b)
    assert got.shape == (n, m) and got.dtype == np.float32
    # each of two f32 evaluations of a cosine, in any summation order, lies within about (2 D + 4) 2^-24 of the exact value (sum |a_i b_i| <= |a| |b|)
    atol = (4 * D + 8) * 2.0 ** -24
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    err = float(np.nanmax(np.abs(got - ref))) if not np.isnan(ref).all() else 0.0
    print("similarity %s %s: max |gpu - restatement| = %.3g, atol %.3g" % (shape, where, err, atol))
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol, equal_nan=True)
    # the restatement is what the host entry computes
    for i, j in ((0, 0), (n - 1, m - 1)):
        np.testing.assert_array_equal(gpu.similarity_score(a[i], b[j]), ref[i, j])
