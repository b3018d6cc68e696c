"""Time of the device renderer at the pipeline's operating point: mi_render_faces (bounds + keypoints, mesh, both eyes; RGBA out) on 128
device-resident 256x256 frames whose faces / landmarks / eyes mi_pipeline_run left in device memory.  HIP events around one call on a
caller stream, a warm-up, the median of `--reps` repetitions; the same for the canvas phase alone (no group drawn), so that the share of the
one-workgroup-per-frame draw phase can be read off.  Writes profiles/render_probe.json.

Bytes: the canvas phase reads 3 and writes 4 bytes per pixel; the draw phase's few thousand pixels per frame are not counted.  The fraction
is of the HBM rate a float4 copy reaches on this chip (6.29 TB/s).  At this size the pictures (25 + 34 MB) fit the 256 MB Infinity Cache, so a
rate above the HBM figure would say "cache", not "faster than memory": the probe also runs 1024 frames (201 + 268 MB), which do not fit."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_COPY_BYTES_PER_S = 6.29e12


def measure(batch, reps, warm):
    import torch
    from PIL import Image
    import rs_face_detection_tflite_amd as mi
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "man.jpg")).convert("RGB").resize((256, 256)))
    run_batch = min(batch, 128)
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.roll(img, (k % 7, -(k % 5)), axis=(0, 1)) for k in range(run_batch)]))).cuda()
    pipe = mi.Pipeline(mi.FaceDetectionModel.BackCamera)
    res = pipe.run(frames)
    torch.cuda.synchronize()
    if batch > run_batch:      # the same results repeated: the renderer's work per frame is what matters, not which face it draws
        rep = lambda t: t.repeat((batch // run_batch,) + (1,) * (t.dim() - 1)).contiguous()
        frames, res = rep(frames), {k: rep(v) for k, v in res.items()}
    style_all = mi.RenderStyle(bounds_color=mi.Colors.GREEN, keypoint_color=mi.Colors.BLUE, line_width=4, point_width=2, mesh=True, mesh_thickness=2.0,
                               eyes=True, eye_thickness=2.0)
    style_none = mi.RenderStyle()
    out = torch.empty((batch, 256, 256, 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    results = {}
    for tag, style in (("all three groups", style_all), ("canvas phase only (no group drawn)", style_none)):
        call = lambda: mi.render_faces(frames, res["faces"], res["face_counts"], res["landmarks"], res["present"], res["eyes"], style, out=out,
                                       out_channels=4, stream=stream.cuda_stream)
        for _ in range(warm):
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
        med = float(ms[len(ms) // 2])
        nbytes = 7.0 * batch * 256 * 256
        if style is style_all:
            drawn = int((out[0, :, :, :3] != frames[0]).any(dim=2).sum().item())
        results[tag] = {"ms_per_batch_median": round(med, 4), "ms_min": round(float(ms[0]), 4), "ms_max": round(float(ms[-1]), 4), "reps": reps,
                        "bytes_per_batch": nbytes, "bytes_per_s": round(nbytes / (med * 1e-3), 1),
                        "fraction_of_hbm_copy_rate": round(nbytes / (med * 1e-3) / HBM_COPY_BYTES_PER_S, 4)}
    pipe.close()
    return {"frames": batch, "frame": "256x256 RGB -> RGBA", "faces_found": int((res["face_counts"] > 0).sum().item()),
            "pixels_drawn_in_frame_0": drawn, "timing": results}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_probe.json"))
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 repetitions")
    import rs_face_detection_tflite_amd as mi
    if mi.device_count() < 1:
        sys.exit("render_probe needs a GPU: no HIP device visible")
    report = {"entry": "mi_render_faces, MI_MEM_DEVICE, caller stream, HIP events around one call", "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S,
              "runs": [measure(128, args.reps, args.warmup), measure(1024, args.reps, args.warmup)]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
