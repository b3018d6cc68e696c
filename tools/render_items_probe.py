"""Time of mi_render_face_items next to mi_render_faces at the pipeline's operating point: 128 device-resident 256x256 frames, the results of
one real Pipeline.run_faces call (BackCamera, max_faces = 1, max_items = 128) left in device memory, RGBA out, every group drawn.  HIP events
around one call on a caller stream, a warm-up, then `--reps` rounds in which the four cases take turns in a rotating order (so that a drift of the box,
and what the case before left in the caches, hits all of them alike); the median of each case with its p10..p90.  Writes profiles/render_items_probe.json.

  a  mi_render_faces on one face per frame (the per-frame arrays gathered from the item list)
  b  mi_render_face_items, max_faces = 1, max_items = 128, both iris groups off: the same pixels as (a), checked byte for byte
  c  the same with both iris groups on
  d  4 faces per frame at 512 items, iris groups on: the items of (c) four times per frame, the copies moved by 0.02 of the picture each

No threshold is fixed: the statement to read off is whether the median of (b) lies inside the p10..p90 of (a) that this run itself records,
and (d - c) / 384, the time one more face of a frame costs with every group on ((d - b) / 384, also recorded, adds the iris groups of the
first face to that)."""
import argparse
import datetime
import json
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 128


def measure(reps, warm):
    import torch
    from PIL import Image
    import rs_face_detection_tflite_amd as mi
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "man.jpg")).convert("RGB").resize((256, 256)))
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.roll(img, (k % 7, -(k % 5)), axis=(0, 1)) for k in range(BATCH)]))).cuda()
    pipe = mi.Pipeline(mi.FaceDetectionModel.BackCamera)
    res = pipe.run_faces(frames, max_faces=1, max_items=BATCH)
    torch.cuda.synchronize()
    pipe.close()
    n_items = int(res["counts"][0].item())
    item_frame = res["item_frame"][:n_items].long()
    # (a) reads per-frame arrays: item j back at its frame (frames without an item keep zeros and present = 0)
    per_frame = {k: torch.zeros((BATCH,) + tuple(res[k].shape[1:]), dtype=res[k].dtype, device="cuda") for k in ("landmarks", "present", "eyes")}
    for k, v in per_frame.items():
        v[item_frame] = res[k][:n_items]
    # (d) every item four times, in frame order, copy c moved by 0.02 * c of the picture in x and y
    four = {}
    shift = (0.02 * torch.arange(4, device="cuda", dtype=torch.float32)).repeat(BATCH)        # [512], per item
    for k in ("landmarks", "eyes"):
        v = per_frame[k].repeat_interleave(4, dim=0).clone()
        v[..., :2] += shift.view(-1, *([1] * (v.dim() - 1)))
        four[k] = v.contiguous()
    faces4 = res["faces"].repeat(1, 4, 1).clone()                                               # [128, 4, 17]
    faces4[..., :16] += (0.02 * torch.arange(4, device="cuda", dtype=torch.float32)).view(1, 4, 1)
    four.update(faces=faces4.contiguous(), face_counts=torch.where(res["face_counts"] > 0, 4, 0).to(torch.int32),
                item_frame=torch.arange(BATCH, device="cuda", dtype=torch.int32).repeat_interleave(4).contiguous(),
                counts=torch.tensor([4 * BATCH, 0], dtype=torch.int32, device="cuda"), present=per_frame["present"].repeat_interleave(4).contiguous())
    base = mi.RenderStyle(bounds_color=mi.Colors.GREEN, keypoint_color=mi.Colors.BLUE, line_width=4, point_width=2, mesh=True, mesh_thickness=2.0,
                          eyes=True, eye_thickness=2.0)
    no_iris = mi.RenderItemsStyle(base)
    iris = mi.RenderItemsStyle(base, iris_oval_color=mi.Colors.PINK, iris_landmark_color=mi.Colors.WHITE, iris_thickness=1.0)
    outs = {tag: torch.empty((BATCH, 256, 256, 4), dtype=torch.uint8, device="cuda") for tag in "abcd"}
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    faces1 = res["faces"][:, 0].contiguous()
    calls = {
        "a": lambda: mi.render_faces(frames, faces1, res["face_counts"], per_frame["landmarks"], per_frame["present"], per_frame["eyes"], base,
                                     out=outs["a"], out_channels=4, stream=s),
        "b": lambda: mi.render_face_items(frames, res, no_iris, out=outs["b"], out_channels=4, stream=s),
        "c": lambda: mi.render_face_items(frames, res, iris, out=outs["c"], out_channels=4, stream=s),
        "d": lambda: mi.render_face_items(frames, four, iris, out=outs["d"], out_channels=4, stream=s),
    }
    torch.cuda.synchronize()
    for _ in range(warm):
        for call in calls.values():
            call()
    stream.synchronize()
    ms = {tag: [] for tag in calls}
    tags = list(calls)
    for r in range(reps):
        for tag in tags[r % 4:] + tags[:r % 4]:     # the order rotates: every case follows every other one equally often
            call = calls[tag]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            ms[tag].append(a.elapsed_time(b))
    stat = lambda v: {"ms_median": round(float(np.median(v)), 4), "ms_p10": round(float(np.percentile(v, 10)), 4),
                      "ms_p90": round(float(np.percentile(v, 90)), 4), "reps": len(v)}
    timing = {tag: stat(v) for tag, v in ms.items()}
    drawn = lambda tag: int((outs[tag][0, :, :, :3] != frames[0]).any(dim=2).sum().item())
    a, b, c, d = (timing[tag] for tag in "abcd")
    return {
        "frames": BATCH, "frame": "256x256 RGB -> RGBA", "items_found": n_items, "items_present": int(res["present"].sum().item()),
        "cases": {"a": "mi_render_faces, one face per frame", "b": "mi_render_face_items, max_faces 1, max_items 128, iris groups off",
                  "c": "the same, iris groups on", "d": "4 faces per frame, 512 items, iris groups on"},
        "timing": timing,
        "pixels_drawn_in_frame_0": {tag: drawn(tag) for tag in "abcd"},
        "b_equals_a_byte_for_byte": bool(torch.equal(outs["a"], outs["b"])),
        "b_median_inside_p10_p90_of_a": bool(a["ms_p10"] <= b["ms_median"] <= a["ms_p90"]),
        "b_minus_a_ms": round(b["ms_median"] - a["ms_median"], 4),
        "ms_per_extra_face": round((d["ms_median"] - c["ms_median"]) / 384.0, 6),
        "ms_per_extra_face_from_b": round((d["ms_median"] - b["ms_median"]) / 384.0, 6),
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--box", default="", help="name of the machine, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_items_probe.json"))
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 repetitions")
    import rs_face_detection_tflite_amd as mi
    if mi.device_count() < 1:
        sys.exit("render_items_probe needs a GPU: no HIP device visible")
    import torch
    report = {"entries": "mi_render_faces / mi_render_face_items, MI_MEM_DEVICE, caller stream, HIP events around one call, cases interleaved",
              "box": args.box or "%s (host %s)" % (torch.cuda.get_device_name(0), socket.gethostname()), "date": datetime.date.today().isoformat(), "run": measure(args.reps, args.warmup)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
