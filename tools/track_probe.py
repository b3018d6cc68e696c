"""What tracking saves over detecting every frame: mi_pipeline_run against mi_tracker_step on 128 device-resident 192x192 frames (the shape of
bench.py's config 5, tools/faces_probe.py's frames: 96 of them hold a face), full-range detector, results left in device memory, HIP events
around one call on one caller stream.  The contenders take turns in ONE process (`--turns` turns of `--reps / --turns` calls each, after 5
warm-up calls per turn), so that all of them see the same box in the same minutes; a contender's figures are the median and the p10..p90 of
all its calls.  Writes profiles/track_probe.json.

  (a) run             mi_pipeline_run: the yardstick (the parent's entry, unchanged)
  (b) step steady     mi_tracker_step, max_detect = 16, steady state: the face streams tracked, the faceless ones lost
  (c) step acquire    mi_tracker_step right after mi_tracker_reset, max_detect = 128: the networks of (a) at the batch sizes of (a), plus the
                      tracker's own three launches (the reset is outside the timed region)
  (n) new launches    those three launches alone (option "track_launches_only"), at max_detect = 128 and 16, on a handle of their own:
                      such steps leave a state that means nothing, and clearing the option drops it
  (d) detector 128/16 the detector network alone at batch 128 and at batch 16 (mi_model_run), for scale

Verdicts, written into the JSON met or not:
  1. the median of (b) is below the p10 of (a)
  2. (c) - (a) is no more than (a)'s own p10..p90 width plus the new launches measured alone (medians)"""
import argparse
import ctypes as C
import datetime
import json
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B, SIZE, WARM = 128, 192, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    from faces_probe import frames_u8
    if mi.device_count() < 1:
        raise RuntimeError("track_probe needs an MI355X: no HIP device visible")
    L = mi.lib()
    MEM = mi.MI_MEM_DEVICE
    frames = torch.from_numpy(frames_u8()).cuda()
    stream = torch.cuda.Stream()
    sp, fp = C.c_void_p(stream.cuda_stream), C.c_void_p(frames.data_ptr())
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def check(rc):
        if rc:
            raise RuntimeError(L.mi_last_error().decode())

    full = mi.FaceDetectionModel.Full
    pipe = mi.Pipeline(full)
    po = [z((B, 17), torch.float32), z((B,), torch.int32), z((B, 468, 3), torch.float32), z((B,), torch.int32), z((B, 2, 76, 3), torch.float32)]
    run = lambda: check(L.mi_pipeline_run(pipe.h, fp, B, SIZE, SIZE, 3 * SIZE, *[ptr(t) for t in po], MEM, sp))

    def tracker_outputs(D):
        return [z((B, 17), torch.float32), z((B,), torch.int32), z((B,), torch.int32), z((B, 48), torch.uint8), z((B, 468, 3), torch.float32),
                z((B,), torch.int32), z((B, 2, 76, 3), torch.float32), z((D,), torch.int32), z((2,), torch.int32)]
    # one handle per max_detect: it is part of the geometry a handle keeps uploaded
    steady, acquire, alone = mi.Tracker(full, B), mi.Tracker(full, B), mi.Tracker(full, B)
    so, ao, no = tracker_outputs(16), tracker_outputs(B), {16: tracker_outputs(16), B: tracker_outputs(B)}
    torch.cuda.synchronize()
    step16 = lambda: check(L.mi_tracker_step(steady.h, fp, SIZE, SIZE, 3 * SIZE, 16, *[ptr(t) for t in so], MEM, sp))
    step128 = lambda: check(L.mi_tracker_step(acquire.h, fp, SIZE, SIZE, 3 * SIZE, B, *[ptr(t) for t in ao], MEM, sp))
    step_alone = lambda D: lambda: check(L.mi_tracker_step(alone.h, fp, SIZE, SIZE, 3 * SIZE, D, *[ptr(t) for t in no[D]], MEM, sp))
    run()
    stream.synchronize()
    faces_found = int((po[1] > 0).sum().item())
    for _ in range(3 * B // 16):       # three times the fairness bound: every face stream has been acquired
        step16()
    stream.synchronize()
    tracked_before = int(steady.state()["tracked"].sum())

    det = mi.Model(os.path.join(ROOT, "models", "face_detection_full_range.tflite"))
    x128 = (frames.float() / 127.5 - 1.0).contiguous()
    x16 = x128[:16].contiguous()
    outs128 = [torch.empty([B] + d[1:], dtype=torch.float32, device="cuda") for d in det.output_dims]
    outs16 = [torch.empty([16] + d[1:], dtype=torch.float32, device="cuda") for d in det.output_dims]
    torch.cuda.synchronize()

    def model_run(x, outs):
        ptrs = (C.c_void_p * len(outs))(*[ptr(o) for o in outs])
        return lambda: check(L.mi_model_run(det.h, ptr(x), int(x.shape[0]), ptrs, MEM, sp))

    # name -> (what runs before every call, outside the timed region; the timed call)
    contenders = {
        "(a) run": (None, run),
        "(b) step steady, max_detect 16": (None, step16),
        "(c) step acquire, max_detect 128": (acquire.reset, step128),      # (the reset synchronises)
        "(d) detector alone, batch 128": (None, model_run(x128, outs128)),
        "(d) detector alone, batch 16": (None, model_run(x16, outs16)),
    }
    ms = {k: [] for k in contenders}
    ms["(n) new launches alone, max_detect 128"], ms["(n) new launches alone, max_detect 16"] = [], []

    def timed(before, call, n, sink):
        for _ in range(WARM):
            if before:
                before()
            call()
        stream.synchronize()
        for _ in range(n):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            sink.append(e0.elapsed_time(e1))
    per_turn = max(a.reps // a.turns, 1)
    for _ in range(a.turns):
        for k, (before, call) in contenders.items():
            timed(before, call, per_turn, ms[k])
        # the tracker's own launches alone, on the buffers a full step of the same geometry left
        for D in (B, 16):
            call = step_alone(D)
            call()
            alone.set_option("track_launches_only", 1)
            timed(None, call, per_turn, ms["(n) new launches alone, max_detect %d" % D])
            alone.set_option("track_launches_only", 0)
    stream.synchronize()
    tracked_after = int(steady.state()["tracked"].sum())

    def stats(v):
        v = np.sort(np.asarray(v))
        q = lambda f: round(float(v[min(int(f * len(v)), len(v) - 1)]), 4)
        return {"ms_median": q(0.5), "ms_p10": q(0.1), "ms_p90": q(0.9), "ms_min": q(0.0), "ms_max": q(1.0), "calls": len(v)}
    res = {k: stats(v) for k, v in ms.items()}
    ra, rb, rc = res["(a) run"], res["(b) step steady, max_detect 16"], res["(c) step acquire, max_detect 128"]
    new128 = res["(n) new launches alone, max_detect 128"]["ms_median"]
    width = round(ra["ms_p90"] - ra["ms_p10"], 4)
    d128, d16 = res["(d) detector alone, batch 128"]["ms_median"], res["(d) detector alone, batch 16"]["ms_median"]
    summary = {
        "faces found by (a)": faces_found, "streams tracked in (b) before / after the timing": [tracked_before, tracked_after],
        "(a) - (b), ms (medians)": round(ra["ms_median"] - rb["ms_median"], 4),
        "(d) batch 128 - batch 16, ms (medians)": round(d128 - d16, 4),
        "(c) - (a), ms (medians)": round(rc["ms_median"] - ra["ms_median"], 4),
        "(a) p10..p90 width, ms": width,
        "new launches alone, ms (median, max_detect 128)": new128,
        "verdict 1: median of (b) below p10 of (a)": bool(rb["ms_median"] < ra["ms_p10"]),
        "verdict 2: (c) - (a) <= (a)'s p10..p90 width + new launches alone": bool(rc["ms_median"] - ra["ms_median"] <= width + new128),
    }
    doc = {"what": "mi_pipeline_run against mi_tracker_step, %d device-resident %dx%d frames, Full detector, HIP events on one caller stream, contenders "
                   "taking turns in one process: %d turns of %d calls after %d warm-up calls" % (B, SIZE, SIZE, a.turns, per_turn, WARM),
           "box": a.box, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "summary": summary, "results": res}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
    for h in (steady, acquire, alone, pipe, det):
        h.close()


if __name__ == "__main__":
    main()
