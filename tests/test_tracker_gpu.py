"""mi_tracker on the device: acquisition equals mi_pipeline_run bit for bit; a tracked step is checked teacher-forced (against the host rule,
mi_fl_infer_images and the oracle, each fed the GPU's own previous landmarks, so that rounding does not compound through the loop); a
moving, turning face is followed without the detector; loss, re-acquisition, the detector budget and its fairness, the plan's scan across
chunks, unwritten memory, memory kinds and argument refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import model_path
from test_pipeline_faces_gpu import KINDS, _torch, canvases

pytestmark = pytest.mark.gpu

KEYS = ("faces", "face_counts", "source", "rois", "landmarks", "present", "eyes", "det_stream", "n_detect")
EINVAL = -1


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


@pytest.fixture(scope="module")
def frames(man_image):
    f = canvases(man_image)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def baseline(gpu, frames):
    """kind -> (a Pipeline, its run(frames)); the BackCamera one is made and run before this module creates its first tracker"""
    made = {}

    def get(kind):
        if kind not in made:
            pipe = gpu.Pipeline(getattr(gpu.FaceDetectionModel, KINDS[kind]))
            made[kind] = (pipe, pipe.run(frames))
        return made[kind]
    get("back")
    yield get
    for pipe, _ in made.values():
        pipe.close()


@pytest.fixture(scope="module")
def trackers(gpu, baseline):
    """One six-stream tracker per detector for the whole module."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = gpu.Tracker(getattr(gpu.FaceDetectionModel, KINDS[kind]), 6)
        return made[kind]
    yield get
    for t in made.values():
        t.close()


@pytest.fixture(scope="module")
def acquired(trackers, frames):
    """kind -> the step right after a reset with max_detect = 6, computed once per detector"""
    cache = {}

    def get(kind):
        if kind not in cache:
            t = trackers(kind)
            t.reset()
            cache[kind] = t.step(frames, max_detect=6)
        return cache[kind]
    return get


@pytest.fixture(scope="module")
def oracle_nets(oracle):
    return oracle.Model(model_path("landmark")), oracle.Model(model_path("iris"))


@pytest.fixture(scope="module")
def mesh(gpu):
    fl = gpu.FaceLandmark()
    yield fl
    fl.close()


def host(out):
    """a step's dict as numpy arrays (rois as RECT_DTYPE records), wherever it lies"""
    import rs_face_detection_tflite_amd as m
    res = {}
    for k, v in out.items():
        a = v.cpu().numpy() if type(v).__module__.startswith("torch") else np.asarray(v)
        res[k] = a.view(m.RECT_DTYPE).reshape(-1) if k == "rois" and a.dtype != m.RECT_DTYPE else a
    return res


def assert_same(a, b, what):
    a, b = host(a), host(b)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def check_zero_slots(out):
    """streams without a result hold zeros"""
    for s in np.nonzero(out["source"] == 0)[0]:
        assert not out["faces"][s].any() and out["present"][s] == 0 and not out["landmarks"][s].any() and not out["eyes"][s].any(), s
        assert out["rois"][s].tobytes() == bytes(48), s
    for s in np.nonzero(out["source"] != 1)[0]:
        assert not out["faces"][s].any(), s
    for s in np.nonzero(out["present"] == 0)[0]:      # (the mesh's landmarks of a ROI whose face flag failed are reported, as mi_pipeline_run's)
        assert not out["eyes"][s].any(), s


def check_state_follows(gpu, tracker, out, size):
    """the state after a step: the tracked ROI of the step's own landmarks where present, lost everywhere else"""
    st = tracker.state()
    for s in range(len(out["present"])):
        roi, valid = gpu.track_roi_from_landmarks(out["landmarks"][s], size) if out["present"][s] else (None, False)
        assert st["tracked"][s] == int(valid), s
        if valid:
            check_roi(st["rois"][s], roi, "state of stream %d" % s)
        else:
            assert st["rois"][s].tobytes() == bytes(48), s
    return st


def check_roi(got, want, what):
    """got: a RECT_DTYPE record of the device; want: the host entry's Rect — centre and size bit for bit, rotation within 1e-15"""
    assert (got["x_center"], got["y_center"], got["width"], got["height"], got["normalized"], got["pad"]) == \
        (want.x_center, want.y_center, want.width, want.height, 1, 0), what
    assert abs(got["rotation"] - want.rotation) <= 1e-15, (what, got["rotation"], want.rotation)


def oracle_mesh_iris(oracle, nets, img, rec):
    """lib.rs:30-40 through the oracle on the ROI `rec` (a RECT_DTYPE record) -> dict(landmarks, eyes), or None where the mesh flag does not pass"""
    fl, ir = nets
    H, W = img.shape[:2]
    roi = oracle.Rect(float(rec["x_center"]), float(rec["y_center"]), float(rec["width"]), float(rec["height"]), float(rec["rotation"]), 1)
    t2, pad2 = oracle.image_to_tensor(img, roi, (192, 192), False, (0., 1.), False)
    raw, flag = fl.run(t2[None])
    if not oracle.lib().orc_face_flag_passes(float(flag.reshape(-1)[-1])):
        return None
    lms = oracle.project_landmarks(raw[0], (192, 192), (W, H), pad2, roi, False)
    left, right = oracle.iris_rois_from_face_landmarks(lms, (W, H))
    eyes = []
    for r, is_right in ((left, False), (right, True)):
        t3, pad3 = oracle.image_to_tensor(img, r, (64, 64), True, (0., 1.), is_right)
        c, i5 = ir.run(t3[None])
        eyes.append(np.concatenate([oracle.project_landmarks(c[0], (64, 64), (W, H), pad3, r, is_right),
                                    oracle.project_landmarks(i5[0], (64, 64), (W, H), pad3, r, is_right)]))
    return dict(landmarks=lms, eyes=np.stack(eyes))


def check_tracked_step(gpu, oracle, nets, mesh, frames, prev, out):
    """A step on `frames` whose previous step gave `prev`, teacher-forced: source 2 exactly where prev was present, the ROI is the host rule's
    of prev's own landmarks, the landmarks are mi_fl_infer_images' on those ROIs bit for bit, and the oracle's mesh and iris on that ROI agree
    within the chain's tolerances (landmarks 2e-5, eyes 1e-4)."""
    S, H, W = frames.shape[:3]
    np.testing.assert_array_equal(out["source"] == 2, prev["present"] != 0)
    rects = []
    for s in range(S):
        if prev["present"][s]:
            roi, valid = gpu.track_roi_from_landmarks(prev["landmarks"][s], (W, H))
            assert valid, s
            check_roi(out["rois"][s], roi, "stream %d" % s)
        rec = out["rois"][s]
        rects.append(gpu.Rect(rec["x_center"], rec["y_center"], rec["width"], rec["height"], rec["rotation"], 1) if out["source"][s]
                     else gpu.Rect(0.5, 0.5, 1.0, 1.0, 0.0, 1))
    lm, present, _ = mesh.infer_images(np.ascontiguousarray(frames), rois=rects)
    for s in np.nonzero(out["source"] == 2)[0]:
        assert out["present"][s] == present[s], s
        if present[s]:
            np.testing.assert_array_equal(out["landmarks"][s], lm[s], err_msg="stream %d" % s)
        want = oracle_mesh_iris(oracle, nets, frames[s], out["rois"][s])
        assert out["present"][s] == (want is not None), s
        if want is not None:
            np.testing.assert_allclose(out["landmarks"][s], want["landmarks"], atol=2e-5, err_msg="stream %d" % s)
            np.testing.assert_allclose(out["eyes"][s], want["eyes"], atol=1e-4, err_msg="stream %d" % s)
    check_zero_slots(out)


# ---------------------------------------------------------------------------------------------------- 1. acquisition
@pytest.mark.parametrize("kind", ["back", "full"])
def test_acquisition_equals_the_pipeline(gpu, baseline, acquired, trackers, frames, kind):
    out, top1 = acquired(kind), baseline(kind)[1]
    np.testing.assert_array_equal(out["det_stream"], np.arange(6))
    np.testing.assert_array_equal(out["n_detect"], [6, 0])
    for k in ("faces", "face_counts", "landmarks", "present", "eyes"):
        np.testing.assert_array_equal(out[k], top1[k], err_msg=k)
    np.testing.assert_array_equal(out["source"], (top1["face_counts"] > 0).astype(np.int32))
    assert list(out["source"][:4]) == [1, 1, 1, 1] and out["source"][4] == 0 and out["present"][:4].all()
    H, W = frames.shape[1:3]
    for s in np.nonzero(out["source"] == 1)[0]:
        d = gpu.Detection(out["faces"][s, :16].reshape(8, 2).copy(), float(out["faces"][s, 16]))
        check_roi(out["rois"][s], gpu.face_detection_to_roi(d, (W, H)), "detector ROI of stream %d" % s)
    check_zero_slots(out)


# ---------------------------------------------------------------------------------------------------- 2. a tracked step
def test_tracked_step_teacher_forced(gpu, oracle, oracle_nets, mesh, acquired, trackers, frames):
    t, first = trackers("back"), acquired("back")
    t.reset()
    again = t.step(frames, max_detect=6)
    assert_same(again, first, "a reset tracker repeats its acquisition")
    H, W = frames.shape[1:3]
    check_state_follows(gpu, t, again, (W, H))
    out = t.step(frames, max_detect=6)
    assert list(out["source"][:4]) == [2, 2, 2, 2] and out["present"][:4].all()
    np.testing.assert_array_equal(out["det_stream"], [4, 5, -1, -1, -1, -1])    # only the black and the noise stream are lost
    np.testing.assert_array_equal(out["n_detect"], [2, 0])
    check_tracked_step(gpu, oracle, oracle_nets, mesh, frames, again, out)
    check_state_follows(gpu, t, out, (W, H))


# ---------------------------------------------------------------------------------------------------- 3. the sequence
def moving_sequence(man_image):
    """six canvases of 720 rows x 1080 columns: man.jpg at (100 + 24 k, 100 + 12 k), turned by 6 k degrees"""
    from PIL import Image
    seq = np.zeros((6, 720, 1080, 3), np.uint8)
    h, w = man_image.shape[:2]
    for k in range(6):
        pic = np.asarray(Image.fromarray(man_image).rotate(6 * k, resample=Image.BILINEAR))
        seq[k, 100 + 12 * k:100 + 12 * k + h, 100 + 24 * k:100 + 24 * k + w] = pic
    return seq


def test_moving_turning_face_is_followed_without_the_detector(gpu, oracle, oracle_nets, mesh, man_image):
    seq = moving_sequence(man_image)
    t = gpu.Tracker(gpu.FaceDetectionModel.BackCamera, 2)
    prev, rotations = None, []
    for k in range(6):
        pair = np.stack([seq[k], np.zeros_like(seq[k])])    # stream 1 stays black
        out = t.step(pair, max_detect=1)
        np.testing.assert_array_equal(out["det_stream"], [0] if k == 0 else [1], err_msg="step %d" % k)
        assert out["source"][0] == (1 if k == 0 else 2) and out["source"][1] == 0, k
        assert out["present"][0] == 1 and out["present"][1] == 0, k
        if prev is not None:
            check_tracked_step(gpu, oracle, oracle_nets, mesh, pair, prev, out)
        st = check_state_follows(gpu, t, out, (1080, 720))
        assert list(st["tracked"]) == [1, 0]
        rotations.append(float(st["rois"][0]["rotation"]))
        prev = out
    t.close()
    assert all(b < a for a, b in zip(rotations, rotations[1:])), rotations      # the ROI turns with the picture
    assert abs(rotations[-1] - (-0.54)) <= 0.05, rotations                      # the oracle loop's final rotation


# ---------------------------------------------------------------------------------------------------- 4. loss and re-acquisition
def test_loss_and_reacquisition(gpu, acquired, trackers, frames):
    t, first = trackers("back"), acquired("back")
    t.reset()
    t.step(frames, max_detect=6)
    assert list(t.state()["tracked"]) == [1, 1, 1, 1, 0, 0]
    gone = np.array(frames)
    gone[3] = 0
    out = t.step(gone, max_detect=6)
    assert out["source"][3] == 2 and out["present"][3] == 0 and not out["eyes"][3].any()
    st = t.state()
    assert list(st["tracked"]) == [1, 1, 1, 0, 0, 0] and st["rois"][3].tobytes() == bytes(48)
    back = t.step(frames, max_detect=6)
    np.testing.assert_array_equal(back["det_stream"], [3, 4, 5, -1, -1, -1])
    np.testing.assert_array_equal(back["n_detect"], [3, 0])
    assert back["source"][3] == 1 and list(back["source"]) == [2, 2, 2, 1, 0, 0]
    for k in ("faces", "face_counts", "landmarks", "present", "eyes"):
        np.testing.assert_array_equal(back[k][3], first[k][3], err_msg=k)
    assert back["rois"][3].tobytes() == first["rois"][3].tobytes()
    assert list(t.state()["tracked"]) == [1, 1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------- 5. budget and fairness
def test_budget_and_fairness(gpu, acquired, trackers, frames):
    t, first = trackers("back"), acquired("back")
    t.reset()
    S, D = 6, 2
    bound = -(-S // D)
    for step in range(4):
        tracked = t.state()["tracked"]
        det, used, left = gpu.track_detect_layout(tracked, D, (step * D) % S)
        out = t.step(frames, max_detect=D)
        np.testing.assert_array_equal(out["det_stream"], det, err_msg="step %d" % step)
        np.testing.assert_array_equal(out["n_detect"], [used, left], err_msg="step %d" % step)
        slots = set(int(s) for s in det if s >= 0)
        for s in range(S):
            want = 2 if tracked[s] else 1 if s in slots and first["face_counts"][s] > 0 else 0
            assert out["source"][s] == want, (step, s)
            assert out["face_counts"][s] == (first["face_counts"][s] if s in slots else 0), (step, s)
            assert out["present"][s] == (1 if want and s < 4 else 0), (step, s)
        check_zero_slots(out)
        if step == bound - 1:   # the black and the noise stream never starve a face stream beyond the bound
            assert list(t.state()["tracked"][:4]) == [1, 1, 1, 1]
    assert list(t.state()["tracked"]) == [1, 1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------- 6. the plan's scan across chunks
def scan_masks(S):
    """name -> tracked [S].  The plan scans the cyclic positions from `start` on in chunks of 256, and the test steps at start 0 and at start 8
    with eight slots, so a mask makes the slots cross the chunk's edge only if fewer than eight of its lost streams lie in streams 0..255 AND
    in streams 8..263.  A mask drawn with one density for all 300 streams cannot promise that (dense: the first chunk takes every slot;
    sparse: no slot is left for the second), so both masks are built around the edge: one by hand, fixed, with the edge's own streams (255,
    256) in it; one seeded, with two lost streams drawn among 0..7, three among 8..255, two among 256..263 and about 0.7 of 264..299."""
    fixed = np.ones(S, np.int32)
    fixed[[0, 17, 100, 200, 255] + list(range(256, S, 3))] = 0
    rng = np.random.default_rng(20261021)
    seeded = np.ones(S, np.int32)
    for lo, hi, n in ((0, 8, 2), (8, 256, 3), (256, 264, 2)):
        seeded[rng.choice(np.arange(lo, hi), n, replace=False)] = 0
    seeded[264:][rng.random(S - 264) < 0.7] = 0
    return {"fixed": fixed, "seeded": seeded}


@pytest.mark.parametrize("which", ["fixed", "seeded"])
def test_plan_scan_across_chunks(gpu, man_image, which):
    torch = _torch()
    S, D = 300, 8
    dev = torch.from_numpy(np.array(man_image)).cuda().unsqueeze(0).repeat(S, 1, 1, 1).contiguous()
    H, W = man_image.shape[:2]
    mask = scan_masks(S)[which]
    rois = np.zeros((S,), gpu.RECT_DTYPE)
    for f, v in (("x_center", 0.5), ("y_center", 0.5), ("width", 0.9), ("height", 0.9 * W / H), ("normalized", 1)):
        rois[f] = v
    t = gpu.Tracker(gpu.FaceDetectionModel.BackCamera, S)
    lost = int((mask == 0).sum())
    assert lost > 2 * D
    for step in range(2):      # start 0, then start 8
        t.set_state(rois, mask)
        st = t.state()
        np.testing.assert_array_equal(st["tracked"], mask)
        assert st["rois"].tobytes() == rois.tobytes()
        out = host(t.step(dev, max_detect=D))
        det, used, left = gpu.track_detect_layout(mask, D, step * D)
        np.testing.assert_array_equal(out["det_stream"], det, err_msg="step %d" % step)
        np.testing.assert_array_equal(out["n_detect"], [used, left])
        at = (det - step * D) % S      # the slots' cyclic positions: some in the first chunk of 256, some beyond it
        assert used == D and left == lost - D and at.min() < 256 <= at.max()
        want = np.where(mask != 0, 2, 0)
        want[det] = 1
        np.testing.assert_array_equal(out["source"], want)
        assert out["present"][want == 1].all() and not out["present"][want == 0].any()   # (the seeded ROIs are no face's: their flags may fail)
        check_zero_slots(out)
    t.close()


# ---------------------------------------------------------------------------------------------------- 7. unwritten memory
def three_steps(t, frames):
    """reset, then an acquisition on a budget of three, a mixed step and a step with a lost stream"""
    t.reset()
    outs = [t.step(frames, max_detect=3), t.step(frames, max_detect=3)]
    gone = np.array(frames)
    gone[1] = 0
    outs.append(t.step(gone, max_detect=3))
    outs.append(t.step(frames, max_detect=3))
    return outs


def test_unwritten_memory(gpu, trackers, frames):
    """option test_poison fills every network's scratch and output buffers with NaN bytes (1) or huge floats (2) before every run: nothing a
    step returns depends on them, and streams without a result hold zeros"""
    plain = three_steps(trackers("full"), frames)
    assert any((o["source"] == 0).any() for o in plain) and any((o["det_stream"] == -1).any() for o in plain)
    for o in plain:
        check_zero_slots(o)
    t = gpu.Tracker(gpu.FaceDetectionModel.Full, 6)
    for poison in (1, 2):
        t.set_option("test_poison", poison)
        for n, (a, b) in enumerate(zip(three_steps(t, frames), plain)):
            assert_same(a, b, "step %d with test_poison %d" % (n, poison))
    t.close()


# ---------------------------------------------------------------------------------------------------- 8. memory kinds
def test_memory_kinds_and_handles(gpu, baseline, trackers, frames):
    torch = _torch()
    t = trackers("back")
    plain = three_steps(t, frames)
    dev = torch.from_numpy(np.array(frames)).cuda()
    gone = dev.clone()
    gone[1] = 0
    torch.cuda.synchronize()

    def on_device(stream):
        t.reset()
        outs = [t.step(f, max_detect=3, stream=stream) for f in (dev, dev, gone, dev)]
        torch.cuda.synchronize()
        return outs
    for n, (a, b) in enumerate(zip(on_device(None), plain)):
        assert_same(a, b, "device tensors, step %d" % n)
    side = torch.cuda.Stream()
    for n, (a, b) in enumerate(zip(on_device(side.cuda_stream), plain)):
        assert_same(a, b, "a caller's stream, step %d" % n)
    # two handles, interleaved, the second on other pictures
    other = gpu.Tracker(gpu.FaceDetectionModel.BackCamera, 6)
    flipped = np.ascontiguousarray(frames[::-1])
    t.reset()
    outs = []
    gone_h = np.array(frames)
    gone_h[1] = 0
    for f in (frames, frames, gone_h, frames):
        other.step(flipped, max_detect=2)
        outs.append(t.step(f, max_detect=3))
    for n, (a, b) in enumerate(zip(outs, plain)):
        assert_same(a, b, "beside another handle, step %d" % n)
    assert list(other.state()["tracked"]) == [0, 0, 1, 1, 1, 1]
    other.close()
    # a Pipeline on the side gives the bits it gave before this module's first tracker existed
    pipe, before = baseline("back")
    after = pipe.run(frames)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_argument_refusals_leave_the_state_untouched(gpu, trackers, frames):
    t = trackers("back")
    t.reset()
    t.step(frames, max_detect=2)      # start is 2 now, streams 0 and 1 are tracked
    before = t.state()
    S, H, W = frames.shape[:3]
    f = np.ascontiguousarray(frames)
    bufs = dict(faces=np.zeros((S, 17), np.float32), face_counts=np.zeros(S, np.int32), source=np.zeros(S, np.int32), rois=np.zeros((S, 48), np.uint8),
                landmarks=np.zeros((S, 468, 3), np.float32), present=np.zeros(S, np.int32), eyes=np.zeros((S, 2, 76, 3), np.float32),
                det_stream=np.zeros(S, np.int32), n_detect=np.zeros(2, np.int32))
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    names = list(bufs)

    def call(frames_p=C.c_void_p(f.ctypes.data), width=W, height=H, stride=3 * W, D=2, mem=0, null=None, handle=t.h):
        args = [None if k == null else ptr[k] for k in names]
        return t.L.mi_tracker_step(handle, frames_p, width, height, stride, D, *args, mem, None)
    assert call(frames_p=None) == EINVAL and call(handle=None) == EINVAL
    for k in names:
        assert call(null=k) == EINVAL, k
    for D in (0, -1, S + 1):
        assert call(D=D) == EINVAL, D
    assert call(width=0) == EINVAL and call(height=0) == EINVAL and call(stride=3 * W - 1) == EINVAL and call(mem=2) == EINVAL
    with pytest.raises(gpu.MiError):
        t.step(frames[:5], max_detect=2)
    with pytest.raises(gpu.MiError):
        t.step(frames, max_detect=7)
    assert t.L.mi_tracker_reset(t.h, 6) == EINVAL and t.L.mi_tracker_reset(t.h, -2) == EINVAL and t.L.mi_tracker_reset(None, 0) == EINVAL
    rois, tracked = np.zeros(6, gpu.RECT_DTYPE), np.ones(6, np.int32)
    pr, pt = C.c_void_p(rois.ctypes.data), C.c_void_p(tracked.ctypes.data)
    for args in [(None, 0, 6, pr, pt), (t.h, 0, 6, None, pt), (t.h, 0, 6, pr, None), (t.h, -1, 2, pr, pt), (t.h, 0, 0, pr, pt), (t.h, 1, 6, pr, pt), (t.h, 6, 1, pr, pt)]:
        assert t.L.mi_tracker_set_state(*args) == EINVAL, args
    assert t.L.mi_tracker_get_state(t.h, None, pt) == EINVAL and t.L.mi_tracker_get_state(t.h, pr, None) == EINVAL
    assert t.L.mi_tracker_set_option(t.h, None, 1) == EINVAL and t.L.mi_tracker_set_option(None, b"test_poison", 1) == EINVAL
    for bad in (0, 32768):
        h = C.c_void_p()
        assert t.L.mi_tracker_create(int(gpu.FaceDetectionModel.BackCamera), None, 0, bad, C.byref(h)) == EINVAL and not h.value
    after = t.state()
    assert after["rois"].tobytes() == before["rois"].tobytes() and list(after["tracked"]) == list(before["tracked"]) == [1, 1, 0, 0, 0, 0]
    assert not any(v.any() for v in bufs.values()), "a refused step writes nothing"
    out = t.step(frames, max_detect=2)      # the plan's start was not advanced either
    np.testing.assert_array_equal(out["det_stream"], [2, 3])
    # reset of one stream
    t.reset(0)
    assert list(t.state()["tracked"]) == [0, 1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------- the measurement option, frames of the wrong rank
def test_launches_only_steps_are_refused_off_geometry_and_leave_no_state(gpu, frames):
    """option track_launches_only: a step is MI_EINVAL unless the handle's last full step had its max_detect and frame size (the launches
    read what that step left), a refused step changes nothing, and clearing the option drops the state those steps made"""
    t = gpu.Tracker(gpu.FaceDetectionModel.BackCamera, 6)
    t.set_option("track_launches_only", 1)
    with pytest.raises(gpu.MiError):      # no full step yet
        t.step(frames, max_detect=3)
    t.set_option("track_launches_only", 0)
    full = t.step(frames, max_detect=3)
    before = t.state()
    assert list(before["tracked"]) == [1, 1, 1, 0, 0, 0]
    t.set_option("track_launches_only", 1)
    with pytest.raises(gpu.MiError):      # another budget
        t.step(frames, max_detect=2)
    with pytest.raises(gpu.MiError):      # another frame size
        t.step(frames[:, :600], max_detect=3)
    after = t.state()
    assert after["rois"].tobytes() == before["rois"].tobytes() and list(after["tracked"]) == list(before["tracked"])
    t.step(frames, max_detect=3)          # the geometry of the last full step: taken
    t.set_option("track_launches_only", 0)
    st = t.state()
    assert not st["tracked"].any() and st["rois"].tobytes() == bytes(48 * 6)
    assert_same(t.step(frames, max_detect=3), full, "the first full step after the option")      # (the plan starts at stream 0 again)
    t.close()


def test_frames_of_the_wrong_rank_are_a_value_error(gpu, trackers, frames):
    torch = _torch()
    t = trackers("back")
    for bad in (frames[0], frames[..., :2], torch.from_numpy(np.array(frames[0])).cuda()):
        with pytest.raises(ValueError):
            t.step(bad, max_detect=2)
