"""What aligned chips cost next to the box path.  The set-up of tools/embeddings_probe.py: 128 device-resident 720 x 1080 frames, 512 items, the
SYNTHETIC D = 128 network (tests/embed_synth.embed_graph: its time describes no real model), HIP events around one call on one caller stream,
5 warm-up calls each, then `--reps` rounds in which the contenders run in a rotating order in one process; the median with p10..p90.
Writes profiles/align_probe.json.

  (a) mi_fe_infer_face_items      the box path: four boxes of 100 .. 300 pixels per frame
  (b) mi_fe_infer_aligned_items   MI_ALIGN_MESH: per item a mesh whose eye corners, nose tip and mouth corners sit where the five-point template
                                  falls in a square of the box's area around the box's centre, turned by up to 0.4 rad (all other landmarks
                                  random), so both paths sample as many source pixels (--side long: the square of the box's longer side)
  (c) mi_model_run                the network alone on 512 chips

(b) is measured against (a), never against itself.  Expectation: (b) - (c) <= (a) - (c) + (a)'s own p10..p90 spread — both paths have two launches
in front of the network and four source taps per output pixel."""
import argparse
import ctypes as C
import datetime
import json
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARM = 5
TEMPLATE = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_probe.json"))
    ap.add_argument("--side", choices=("area", "long"), default="area",
                    help="the square a mesh's points span: of the box's area (both paths sample as many source pixels) or of its longer side")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    import embed_synth as es
    if mi.device_count() < 1:
        raise RuntimeError("align_probe needs an MI355X: no HIP device visible")
    stream = torch.cuda.Stream()
    B, H, W, F, M, D = 128, 720, 1080, 4, 512, 128
    rs = np.random.RandomState(7)
    frames = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda()
    faces = np.zeros((B, F, 17), np.float32)
    landmarks = rs.uniform(0.0, 1.0, (M, 468, 3)).astype(np.float32)
    for b in range(B):
        for k in range(F):   # boxes of 100 .. 300 pixels, inside the frame
            w, h = rs.randint(100, 301, 2)
            x, y = rs.randint(0, W - w), rs.randint(0, H - h)
            faces[b, k, :4] = ((x + 0.25) / W, (y + 0.25) / H, (x + w + 0.5) / W, (y + h + 0.5) / H)
            # the template scaled into a square around the box's centre, turned by up to 0.4 rad
            side, t = (float(w) * float(h)) ** 0.5 if a.side == "area" else float(max(w, h)), rs.uniform(-0.4, 0.4)
            cx, cy, c, s = x + w / 2.0, y + h / 2.0, np.cos(t) * side / 112.0, np.sin(t) * side / 112.0
            pts = [(cx + c * (u - 56.0) - s * (v - 56.0), cy + s * (u - 56.0) + c * (v - 56.0)) for u, v in TEMPLATE]
            lm = landmarks[b * F + k]
            for idx, p in zip(((33, 133), (362, 263), (1, 1), (61, 61), (291, 291)), pts):
                for i in idx:
                    lm[i, 0], lm[i, 1] = p[0] / W, p[1] / H
    item_frame, item_face = np.repeat(np.arange(B, dtype=np.int32), F), np.tile(np.arange(F, dtype=np.int32), B)
    res = {k: torch.from_numpy(v).cuda() for k, v in dict(faces=faces, item_frame=item_frame, item_face=item_face, landmarks=landmarks,
                                                          present=np.ones(M, np.int32)).items()}
    fe = mi.FaceEmbeddings(model_bytes=es.embed_graph(71, D, True))
    box = fe.infer_items(frames, res, stream=stream.cuda_stream)
    aligned = fe.infer_items_aligned(frames, res, source="mesh", want_rois=True, stream=stream.cuda_stream)
    stream.synchronize()
    valid = {"box": int(box["valid"].sum().item()), "aligned": int(aligned["valid"].sum().item())}
    sides = aligned["rois"].cpu().numpy().view(mi.RECT_DTYPE).reshape(-1)["width"]
    L = mi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    emb, val = box["embeddings"], box["valid"]
    chips = torch.rand((M, 112, 112, 3), dtype=torch.float32, device="cuda")
    raw = torch.zeros((M, D), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    outs = (C.c_void_p * 1)(raw.data_ptr())
    s = C.c_void_p(stream.cuda_stream)

    def box_path():
        mi.api._check(L.mi_fe_infer_face_items(fe.h, ptr(frames), B, W, H, 3 * W, ptr(res["faces"]), F, ptr(res["item_frame"]), ptr(res["item_face"]), M,
                                               ptr(emb), ptr(val), None, None, mi.MI_MEM_DEVICE, s))

    def aligned_path():
        mi.api._check(L.mi_fe_infer_aligned_items(fe.h, ptr(frames), B, W, H, 3 * W, mi.ALIGN_SOURCES["mesh"], ptr(res["landmarks"]), ptr(res["present"]), 1,
                                                  ptr(res["item_frame"]), None, M, ptr(emb), ptr(val), None, None, None, mi.MI_MEM_DEVICE, s))

    def network():
        mi.api._check(L.mi_model_run(fe.model.h, ptr(chips), M, outs, mi.MI_MEM_DEVICE, s))
    contenders = [("a", box_path), ("b", aligned_path), ("c", network)]
    for _, call in contenders:
        for _ in range(WARM):
            call()
    stream.synchronize()
    ms = {name: [] for name, _ in contenders}
    for r in range(a.reps):
        for i in range(len(contenders)):
            name, call = contenders[(i + r) % len(contenders)]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))

    def stats(v):
        v = np.sort(np.asarray(v))
        q = lambda f: round(float(v[min(int(f * len(v)), len(v) - 1)]), 4)
        return {"ms_median": q(0.5), "ms_p10": q(0.1), "ms_p90": q(0.9), "reps": len(v)}
    ra, rb, rc = stats(ms["a"]), stats(ms["b"]), stats(ms["c"])
    extra_a, extra_b = ra["ms_median"] - rc["ms_median"], rb["ms_median"] - rc["ms_median"]
    spread_a = ra["ms_p90"] - ra["ms_p10"]
    doc = {"what": "aligned chips against the box path: %d device-resident %dx%d frames, %d items, synthetic D = %d network; HIP events on one caller "
                   "stream, %d rounds after %d warm-up calls, contenders in a rotating order in one process" % (B, H, W, M, D, a.reps, WARM),
           "box": a.box, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "valid_items": valid,
           "square of a mesh's points": "of the box's area" if a.side == "area" else "of the box's longer side",
           "fitted ROI side, px (min / median / max)": [round(float(v), 1) for v in (sides.min(), np.median(sides), sides.max())],
           "(a) mi_fe_infer_face_items (box path)": ra, "(b) mi_fe_infer_aligned_items (mesh source)": rb,
           "(c) mi_model_run alone, %d chips" % M: rc,
           "(a) - (c), ms": round(extra_a, 4), "(b) - (c), ms": round(extra_b, 4), "(a) p10..p90 spread, ms": round(spread_a, 4),
           "expectation": "(b) - (c) <= (a) - (c) + (a)'s p10..p90 spread",
           "expectation met": bool(extra_b <= extra_a + spread_a),
           "note": "the network is synthetic (mesh-like trunk to 7x7x128, one whole-frame convolution): its time describes no real model"}
    fe.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
