"""What the every-face pipeline costs: mi_pipeline_run and mi_pipeline_run_faces on 128 device-resident 192x192 frames (the shape of bench.py's
config 5), full-range detector, results left in device memory, one caller stream.  HIP events around one call, 5 warm-up calls per shape, the
median of `--reps` calls (min and max are kept: the spread is part of the result).  Writes profiles/faces_probe.json.

  run                      mi_pipeline_run (top-1 face per frame): the yardstick
  run_faces 1 x 128        max_faces = 1, max_items = 128: the same networks on the same batch sizes plus the one item-list launch
  run_faces 4 x {128,256,512}   how the time follows the item budget (the mesh runs on max_items items, the iris network on twice as many,
                           whatever the detector finds: the frames here hold one face or none)

`--parent-lib PATH` (a libmiface.so built from the parent commit: MI_VARIANT=parent build.sh in a checkout of it) adds mi_pipeline_run of
that library, measured in fresh processes that alternate with this commit's, so that both see the same box in the same minutes.  Each
measurement runs in a child process of its own, which binds the few entries it calls itself (the parent's library has no
mi_pipeline_run_faces for api.py to bind).

The check: mi_pipeline_run of the two libraries must agree within the run-to-run spread recorded here, or the probe exits with status 1.
A library's time is the median of its processes' medians.  The spread is the larger of (a) the largest distance between two process
medians of one library — what repeating the same command on the same code moves — and (b) the largest p10..p90 width of the calls of
one process — what a single median is uncertain by.  Verdict, difference and spread go into the JSON."""
import argparse
import ctypes as C
import datetime
import json
import os
import platform
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SIZE, WARM = 128, 192, 5


def frames_u8():
    import numpy as np
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "man.jpg")).convert("RGB").resize((SIZE, SIZE)))
    rs = np.random.RandomState(5)
    originals = [img, np.roll(img, (7, -5), axis=(0, 1)), img[:, ::-1].copy(), (img.astype(np.float32) * 0.7).astype(np.uint8),
                 np.roll(img, (-9, 11), axis=(0, 1)), np.clip(img.astype(np.int32) + 30, 0, 255).astype(np.uint8),
                 rs.randint(0, 256, img.shape).astype(np.uint8), np.zeros_like(img)]
    return np.ascontiguousarray(np.stack([originals[b % 8] for b in range(B)]))


def bind(path):
    import torch  # noqa: F401  (first: the library must share torch's HIP runtime)
    L = C.CDLL(path)
    vp, ci = C.c_void_p, C.c_int
    L.mi_last_error.restype = C.c_char_p
    L.mi_pipeline_create.argtypes = [ci, C.c_char_p, ci, C.POINTER(vp)]
    L.mi_pipeline_free.argtypes = [vp]
    L.mi_pipeline_free.restype = None
    L.mi_pipeline_run.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    if hasattr(L, "mi_pipeline_run_faces"):
        L.mi_pipeline_run_faces.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    return L


def child(lib, reps, with_faces):
    import numpy as np
    import torch
    L = bind(lib)
    if L.mi_device_count() < 1:
        raise RuntimeError("faces_probe needs an MI355X: no HIP device visible")
    MI_FD_FULL, MI_MEM_DEVICE = 3, 1

    def check(rc):
        if rc:
            raise RuntimeError(L.mi_last_error().decode())

    frames = torch.from_numpy(frames_u8()).cuda()
    pipe = C.c_void_p()
    check(L.mi_pipeline_create(MI_FD_FULL, os.fsencode(os.path.join(ROOT, "models")), 0, C.byref(pipe)))
    stream = torch.cuda.Stream()
    sp, fp = C.c_void_p(stream.cuda_stream), C.c_void_p(frames.data_ptr())
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def timed(call):
        for _ in range(WARM):
            call()
        stream.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms = np.sort(np.asarray(ms))
        q = lambda f: round(float(ms[min(int(f * len(ms)), len(ms) - 1)]), 4)
        return {"ms_median": q(0.5), "ms_p10": q(0.1), "ms_p90": q(0.9), "ms_min": q(0.0), "ms_max": q(1.0), "reps": reps}

    out = {}
    o = [z((B, 17), torch.float32), z((B,), torch.int32), z((B, 468, 3), torch.float32), z((B,), torch.int32), z((B, 2, 76, 3), torch.float32)]
    torch.cuda.synchronize()
    out["run"] = timed(lambda: check(L.mi_pipeline_run(pipe, fp, B, SIZE, SIZE, 3 * SIZE, *[ptr(t) for t in o], MI_MEM_DEVICE, sp)))
    out["run"]["faces_found"] = int((o[1] > 0).sum().item())
    if with_faces:
        for F, M in ((1, 128), (4, 128), (4, 256), (4, 512)):
            f = [z((B, F, 17), torch.float32), z((B,), torch.int32), z((M,), torch.int32), z((M,), torch.int32), z((2,), torch.int32),
                 z((M, 468, 3), torch.float32), z((M,), torch.int32), z((M, 2, 76, 3), torch.float32)]
            torch.cuda.synchronize()
            r = timed(lambda: check(L.mi_pipeline_run_faces(pipe, fp, B, SIZE, SIZE, 3 * SIZE, F, M, *[ptr(t) for t in f], MI_MEM_DEVICE, sp)))
            r["items_used"], r["items_dropped"] = (int(v) for v in f[4].cpu())
            out["run_faces max_faces=%d max_items=%d" % (F, M)] = r
    torch.cuda.synchronize()
    L.mi_pipeline_free(pipe)
    out["device"] = torch.cuda.get_device_name(0)
    print("FACES_PROBE " + json.dumps(out))


def spawn(lib, reps, with_faces):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", os.path.abspath(lib), "--reps", str(reps)] + (["--with-faces"] if with_faces else [])
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
    line = [l for l in text.splitlines() if l.startswith("FACES_PROBE ")][-1]
    return json.loads(line[len("FACES_PROBE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3, help="processes per library, alternating")
    ap.add_argument("--lib", default=os.path.join(ROOT, "rs-face-detection-tflite_amd", "libmiface.so"), help="this commit's library")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faces_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--with-faces", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.lib, a.reps, a.with_faces)
    runs = []
    for r in range(a.rounds):
        if a.parent_lib:
            runs.append({"library": "parent commit", "round": r, "results": spawn(a.parent_lib, a.reps, False)})
        runs.append({"library": "this commit", "round": r, "results": spawn(a.lib, a.reps, True)})
    device = runs[-1]["results"].pop("device")
    for x in runs:
        x["results"].pop("device", None)
    med = lambda lib, key: sorted(x["results"][key]["ms_median"] for x in runs if x["library"] == lib and key in x["results"])
    mid = lambda v: v[len(v) // 2]
    this_run = med("this commit", "run")
    summary = {"run, this commit, ms (median of each process)": this_run}
    ok = True
    if a.parent_lib:
        parent_run = med("parent commit", "run")
        between = max(this_run[-1] - this_run[0], parent_run[-1] - parent_run[0])
        within = max(x["results"]["run"]["ms_p90"] - x["results"]["run"]["ms_p10"] for x in runs)
        spread, diff = max(between, within), mid(this_run) - mid(parent_run)
        ok = abs(diff) <= spread
        summary.update({"run, parent commit, ms (median of each process)": parent_run,
                        "run, this commit minus parent commit, ms (medians of the process medians)": round(diff, 4),
                        "run-to-run spread, ms": round(spread, 4),
                        "spread (a) between process medians of one library, ms": round(between, 4),
                        "spread (b) widest p10..p90 of the calls of one process, ms": round(within, 4),
                        "run agrees with the parent commit within the spread": ok})
    for key in runs[-1]["results"]:
        if key.startswith("run_faces"):
            v = med("this commit", key)
            summary[key + ", ms (median of each process)"] = v
            summary[key + ", minus run, ms"] = round(mid(v) - mid(this_run), 4)
    doc = {"what": "mi_pipeline_run / mi_pipeline_run_faces, %d device-resident %dx%d frames, Full detector, HIP events, median of %d calls after %d warm-up calls"
                   % (B, SIZE, SIZE, a.reps, WARM),
           "box": a.box, "device": device, "date": datetime.date.today().isoformat(), "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))
    if not ok:
        sys.exit("mi_pipeline_run differs from the parent commit by more than the run-to-run spread")


if __name__ == "__main__":
    main()
