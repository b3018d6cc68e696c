"""mi_pipeline_run_faces: the device pipeline for EVERY face of a frame (detector -> per face: ROI -> mesh -> eye ROIs -> 2 x iris), the
faces of a batch compacted on the device into a fixed number of items.  Checked against the oracle's face-by-face restatement of
lib.rs:24-40, against mi_pipeline_run (bit for bit at max_faces = 1), against mi_face_items_layout (the host statement of the item
list) and for what the unused slots hold."""
import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

ORC_KIND = {"back": "FD_BACK", "full": "FD_FULL"}
KINDS = {"back": "BackCamera", "full": "Full"}
KEYS = ("faces", "face_counts", "item_frame", "item_face", "counts", "landmarks", "present", "eyes")


def _iou(a, b):
    x0, y0, x1, y1 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    inter = max(0.0, x1 - x0) * max(0.0, y1 - y0)
    ua = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / ua if ua > 0 else 1.0


def _torch():
    """torch carries the device-resident frames: on a GPU box a broken install is a failure, not a skip"""
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


def oracle_faces(oracle, models, img, kind, max_faces):
    """lib.rs:18-40 through the oracle for one frame, the flow of lines 29-40 for each of its first max_faces detections.
    -> (all detections, [dict(landmarks, eyes) per face; None where the mesh flag did not pass])"""
    fd, fl, ir = models
    H, W = img.shape[:2]
    size = fd.input_dims[1]
    t, pad = oracle.image_to_tensor(img, None, (size, size), True, (-1., 1.), False)
    rb, rs = fd.run(t[None])
    dets = oracle.fd_postprocess(rb[0], rs[0], oracle.ssd_anchors(getattr(oracle, ORC_KIND[kind])), float(size), pad)
    per_face = []
    for det in dets[:max_faces]:
        roi = oracle.face_detection_to_roi(det, (W, H))
        t2, pad2 = oracle.image_to_tensor(img, roi, (192, 192), False, (0., 1.), False)
        raw, flag = fl.run(t2[None])
        if not oracle.lib().orc_face_flag_passes(float(flag.reshape(-1)[-1])):
            per_face.append(None)
            continue
        lms = oracle.project_landmarks(raw[0], (192, 192), (W, H), pad2, roi, False)
        left, right = oracle.iris_rois_from_face_landmarks(lms, (W, H))
        eyes = []
        for r, is_right in ((left, False), (right, True)):
            t3, pad3 = oracle.image_to_tensor(img, r, (64, 64), True, (0., 1.), is_right)
            c, i5 = ir.run(t3[None])
            eyes.append(np.concatenate([oracle.project_landmarks(c[0], (64, 64), (W, H), pad3, r, is_right),
                                        oracle.project_landmarks(i5[0], (64, 64), (W, H), pad3, r, is_right)]))
        per_face.append(dict(landmarks=lms, eyes=np.stack(eyes)))
    return dets, per_face


@pytest.fixture(scope="module")
def frames(man_image):
    f = canvases(man_image)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def reference(oracle, frames):
    """kind -> per frame (detections, per-face results) of the oracle, computed once per detector."""
    cache = {}

    def get(kind):
        if kind not in cache:
            models = (oracle.Model(model_path(kind)), oracle.Model(model_path("landmark")), oracle.Model(model_path("iris")))
            cache[kind] = [oracle_faces(oracle, models, f, kind, 4) for f in frames]
        return cache[kind]
    return get


@pytest.fixture(scope="module")
def pipes(gpu):
    """One pipeline handle per detector for the whole module (loading and planning three networks is most of a test's time)."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = gpu.Pipeline(getattr(gpu.FaceDetectionModel, KINDS[kind]))
        return made[kind]
    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def run16(pipes, frames):
    """kind -> run_faces(the six canvases, max_faces = 4, max_items = 16) from host memory, once per detector."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = pipes(kind).run_faces(frames, max_faces=4, max_items=16)
        return cache[kind]
    return get


def check_unused(out, max_items):
    n = int(out["counts"][0])
    assert 0 <= n <= max_items
    assert (out["item_frame"][:n] >= 0).all() and (out["item_face"][:n] >= 0).all()
    assert (out["item_frame"][n:] == -1).all() and (out["item_face"][n:] == -1).all() and (out["present"][n:] == 0).all()
    assert not out["landmarks"][n:].any() and not out["eyes"][n:].any()
    assert out["landmarks"].shape == (max_items, 468, 3) and out["eyes"].shape == (max_items, 2, 76, 3)


def check_against_reference(gpu, out, ref, max_faces, max_items):
    """faces, counts, the item list and every used item against the oracle's per-face flow (tolerances of the existing pipeline tests)."""
    B = len(ref)
    counts = [len(dets) for dets, _ in ref]
    np.testing.assert_array_equal(out["face_counts"], counts)
    assert out["faces"].shape == (B, max_faces, 17)
    for b, (dets, _) in enumerate(ref):
        n = min(len(dets), max_faces)
        for k in range(n):
            assert _iou(out["faces"][b, k, :4], dets[k][:4]) >= 0.999, (b, k)
            np.testing.assert_allclose(out["faces"][b, k], dets[k], atol=2e-5, err_msg="face %d of frame %d" % (k, b))
        assert not out["faces"][b, n:].any(), "records behind frame %d's last detection must be zeros" % b
    item_frame, item_face, n_items, dropped = gpu.face_items_layout(counts, max_faces, max_items)
    np.testing.assert_array_equal(out["item_frame"], item_frame)
    np.testing.assert_array_equal(out["item_face"], item_face)
    assert [int(v) for v in out["counts"]] == [n_items, dropped] and (out["n_items"], out["dropped"]) == (n_items, dropped)
    n_mesh = 0
    for j in range(n_items):
        want = ref[item_frame[j]][1][item_face[j]]
        assert out["present"][j] == (want is not None), j
        if want is None:
            assert not out["eyes"][j].any()
            continue
        n_mesh += 1
        np.testing.assert_allclose(out["landmarks"][j], want["landmarks"], atol=2e-5, err_msg="item %d" % j)
        np.testing.assert_allclose(out["eyes"][j], want["eyes"], atol=1e-4, err_msg="item %d" % j)   # third stage of the chain
    check_unused(out, max_items)
    return n_mesh


@pytest.mark.parametrize("kind", ["back", "full"])
def test_every_face_against_the_oracle(gpu, reference, run16, kind):
    ref = reference(kind)
    counts = [len(dets) for dets, _ in ref]
    # the oracle's own counts first: the batch must hold a frame without a face, one with at least two and one with four
    assert counts[0] == 4 and counts[1] == 3, counts
    assert 0 in counts and any(c >= 2 for c in counts) and 4 in counts, counts
    assert sum(min(c, 4) for c in counts) <= 16
    n_mesh = check_against_reference(gpu, run16(kind), ref, 4, 16)
    assert n_mesh >= 8, "at least 8 items must pass the mesh flag, got %d" % n_mesh


def test_item_budget_and_max_faces_limits(gpu, reference, run16, pipes, frames):
    ref, full = reference("full"), run16("full")
    counts = [len(dets) for dets, _ in ref]
    total = sum(min(c, 4) for c in counts)
    out = pipes("full").run_faces(frames, max_faces=4, max_items=5)
    assert [int(v) for v in out["counts"]] == [5, total - 5]
    np.testing.assert_array_equal(out["item_frame"], [0, 0, 0, 0, 1])
    np.testing.assert_array_equal(out["item_face"], [0, 1, 2, 3, 0])
    np.testing.assert_array_equal(out["faces"], full["faces"])              # the budget never touches the detector's results
    np.testing.assert_array_equal(out["face_counts"], full["face_counts"])
    np.testing.assert_array_equal(out["present"], full["present"][:5])
    np.testing.assert_allclose(out["landmarks"], full["landmarks"][:5], atol=2e-5)
    np.testing.assert_allclose(out["eyes"], full["eyes"][:5], atol=1e-4)
    assert check_against_reference(gpu, out, ref, 4, 5) >= 1
    # max_faces = 2: at most the first two faces of a frame
    out2 = pipes("full").run_faces(frames, max_faces=2, max_items=16)
    assert out2["faces"].shape == (len(frames), 2, 17)
    np.testing.assert_array_equal(out2["faces"], full["faces"][:, :2])
    want_frames = [b for b, c in enumerate(counts) for _ in range(min(c, 2))]
    np.testing.assert_array_equal(out2["item_frame"][:len(want_frames)], want_frames)
    assert out2["item_face"].max() <= 1 and out2["n_items"] == len(want_frames) and out2["dropped"] == 0
    check_against_reference(gpu, out2, ref, 2, 16)


@pytest.mark.parametrize("kind", ["back", "full"])
def test_max_faces_one_equals_pipeline_run_bit_for_bit(gpu, man_image, pipes, kind):
    """The six-frame batch of test_batched_device_pipeline_vs_oracle: with max_faces = 1 and max_items = batch the mesh and iris networks
    see batches of the size mi_pipeline_run gives them, and results do not depend on the position in a batch."""
    img = man_image
    batch = np.stack([img, np.roll(img, (12, -30), axis=(0, 1)), img[:, ::-1].copy(), (img.astype(np.float32) * 0.6).astype(np.uint8),
                      np.zeros_like(img), np.random.RandomState(3).randint(0, 256, img.shape).astype(np.uint8)])
    pipe = pipes(kind)
    top1 = pipe.run(batch)
    out = pipe.run_faces(batch, max_faces=1, max_items=len(batch))
    np.testing.assert_array_equal(out["face_counts"], top1["face_counts"])
    np.testing.assert_array_equal(out["faces"][:, 0], top1["faces"])
    with_face = [b for b in range(len(batch)) if top1["face_counts"][b] > 0]
    assert len(with_face) >= 3 and len(with_face) < len(batch)
    np.testing.assert_array_equal(out["item_frame"][:out["n_items"]], with_face)     # frames without a face have no item
    assert out["n_items"] == len(with_face) and out["dropped"] == 0
    for j in range(out["n_items"]):
        b = out["item_frame"][j]
        assert out["present"][j] == top1["present"][b]
        np.testing.assert_array_equal(out["landmarks"][j], top1["landmarks"][b], err_msg="item %d, frame %d" % (j, b))
        np.testing.assert_array_equal(out["eyes"][j], top1["eyes"][b], err_msg="item %d, frame %d" % (j, b))
    assert top1["present"][with_face].sum() >= 1
    check_unused(out, len(batch))


def test_unused_slots_and_unwritten_memory(gpu, run16, frames):
    """Slots behind the last item hold -1 / -1 / 0 and zeros, and nothing the call returns depends on what the NETWORKS' memory held:
    option test_poison fills every network's scratch and output buffers with NaN bytes (1) or huge floats (2) before every run.  It does
    not reach the pipeline's own buffers (the result block of a host-memory call, the items' ROIs and valid flags): for those, stale
    contents are what the growing-then-shrinking budget of test_memory_kinds_and_calling_patterns leaves behind."""
    plain = run16("full")
    check_unused(plain, 16)
    assert plain["n_items"] < 16
    pipe = gpu.Pipeline(gpu.FaceDetectionModel.Full)
    for poison in (1, 2):
        pipe.set_option("test_poison", poison)
        out = pipe.run_faces(frames, max_faces=4, max_items=16)
        for k in KEYS:
            np.testing.assert_array_equal(out[k], plain[k], err_msg="%s with test_poison %d" % (k, poison))
    pipe.close()


def test_item_list_scan_across_chunks(gpu, man_image, pipes):
    """300 frames (more than one chunk of the item kernel's scan) of 192 x 192 with period [face, black, face shifted, noise]: the item
    list equals the host layout's, and every item equals the item of the same source frame in the first period bit for bit."""
    torch = _torch()
    from PIL import Image
    img = np.asarray(Image.fromarray(man_image).resize((192, 192)))
    period = [img, np.zeros_like(img), np.roll(img, (7, -5), axis=(0, 1)), np.random.RandomState(11).randint(0, 256, img.shape).astype(np.uint8)]
    B, M = 300, 160
    dev = torch.from_numpy(np.stack([period[b % 4] for b in range(B)])).cuda()
    out = {k: v.cpu().numpy() for k, v in pipes("full").run_faces(dev, max_faces=2, max_items=M).items()}
    counts = out["face_counts"]
    for b in range(4, B):
        assert counts[b] == counts[b % 4]
        np.testing.assert_array_equal(out["faces"][b], out["faces"][b % 4])
    assert counts[0] >= 1 and counts[2] >= 1 and counts[1] == 0
    item_frame, item_face, n_items, dropped = gpu.face_items_layout(counts, 2, M)
    np.testing.assert_array_equal(out["item_frame"], item_frame)
    np.testing.assert_array_equal(out["item_face"], item_face)
    assert [int(v) for v in out["counts"]] == [n_items, dropped] and int(out["n_items"]) == n_items
    assert n_items >= 150 and item_frame[:n_items].max() >= 256, "the items must come from both chunks of the scan"
    first = {}    # (source frame, face) -> item of the first period
    for j in range(n_items):
        key = (item_frame[j] % 4, item_face[j])
        if item_frame[j] < 4:
            first[key] = j
            continue
        i = first[key]
        assert out["present"][j] == out["present"][i]
        np.testing.assert_array_equal(out["landmarks"][j], out["landmarks"][i], err_msg="item %d (frame %d) vs item %d" % (j, item_frame[j], i))
        np.testing.assert_array_equal(out["eyes"][j], out["eyes"][i], err_msg="item %d (frame %d) vs item %d" % (j, item_frame[j], i))
    assert out["present"][:n_items].sum() >= 150
    check_unused(out, M)


def test_memory_kinds_and_calling_patterns(gpu, reference, run16, pipes, frames):
    torch = _torch()
    plain = run16("full")
    pipe = pipes("full")
    # results left in device memory equal the ones handed out in host memory
    dev = torch.from_numpy(np.array(frames)).cuda()
    torch.cuda.synchronize()
    out = pipe.run_faces(dev, max_faces=4, max_items=16)
    torch.cuda.synchronize()
    for k in KEYS:
        np.testing.assert_array_equal(out[k].cpu().numpy(), plain[k], err_msg=k)
    assert int(out["n_items"]) == plain["n_items"] and int(out["dropped"]) == plain["dropped"]
    # one handle, a growing and then a shrinking budget
    small = pipe.run_faces(frames, max_faces=4, max_items=3)
    big = pipe.run_faces(frames, max_faces=4, max_items=16)
    again = pipe.run_faces(frames, max_faces=4, max_items=3)
    for k in KEYS:
        np.testing.assert_array_equal(big[k], plain[k], err_msg=k)
        np.testing.assert_array_equal(again[k], small[k], err_msg=k)
    assert small["n_items"] == 3 and small["dropped"] == plain["n_items"] - 3
    check_against_reference(gpu, small, reference("full"), 4, 3)
    # a batch of one: the four-face canvas, the default budget (batch * max_faces)
    one = pipe.run_faces(frames[:1], max_faces=4)
    assert one["landmarks"].shape[0] == 4 and one["n_items"] == 4 and one["dropped"] == 0
    assert check_against_reference(gpu, one, reference("full")[:1], 4, 4) >= 1
