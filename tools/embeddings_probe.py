"""What the embedding flow costs on the device.  HIP events around one call on one caller stream, 5 warm-up calls, the median of `--reps`
calls with p10..p90 (as tools/faces_probe.py).  Writes profiles/embeddings_probe.json.  Record only: nothing existed before to compare with.

  (a) mi_fe_infer_face_items   128 device-resident 720 x 1080 frames, 512 items (four boxes of 100 .. 300 pixels per frame), a SYNTHETIC D = 128
                               network (tests/embed_synth.embed_graph: the reference ships no model, so the network's time describes no real
                               model).  Reported apart: the whole call, the network alone (mi_model_run on the handle's engine, 512 x
                               [112,112,3]) and their difference: the two chip launches and the l2_norm launch.
  (b) mi_similarity_matrix     n = 512 queries against a gallery of m = 65536, D = 512, device memory: ms and TFLOP/s (2 n m D flop), next to
                               the 157.3 TFLOP/s f32 matrix peak of the MI355X and the 122 TFLOP/s of an untuned 4096^3 GEMM on the same
                               instruction (v_mfma_f32_32x32x2_f32)."""
import argparse
import datetime
import json
import os
import platform
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARM = 5
F32_MATRIX_PEAK_TFLOPS, UNTUNED_GEMM_TFLOPS = 157.3, 122.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embeddings_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    import embed_synth as es
    if mi.device_count() < 1:
        raise RuntimeError("embeddings_probe needs an MI355X: no HIP device visible")
    stream = torch.cuda.Stream()

    def timed(call):
        for _ in range(WARM):
            call()
        stream.synchronize()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        ms = np.sort(np.asarray(ms))
        q = lambda f: round(float(ms[min(int(f * len(ms)), len(ms) - 1)]), 4)
        return {"ms_median": q(0.5), "ms_p10": q(0.1), "ms_p90": q(0.9), "reps": a.reps}

    # ---- (a)
    B, H, W, F, M, D = 128, 720, 1080, 4, 512, 128
    rs = np.random.RandomState(7)
    frames = torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda()
    faces = np.zeros((B, F, 17), np.float32)
    for b in range(B):
        for k in range(F):   # boxes of 100 .. 300 pixels, inside the frame
            w, h = rs.randint(100, 301, 2)
            x, y = rs.randint(0, W - w), rs.randint(0, H - h)
            faces[b, k, :4] = ((x + 0.25) / W, (y + 0.25) / H, (x + w + 0.5) / W, (y + h + 0.5) / H)
    item_frame, item_face = np.repeat(np.arange(B, dtype=np.int32), F), np.tile(np.arange(F, dtype=np.int32), B)
    res = {k: torch.from_numpy(v).cuda() for k, v in dict(faces=faces, item_frame=item_frame, item_face=item_face).items()}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "embed.tflite")
        with open(path, "wb") as f:
            f.write(es.embed_graph(71, D, True))
        fe = mi.FaceEmbeddings(path)
    out = fe.infer_items(frames, res, stream=stream.cuda_stream)
    stream.synchronize()
    valid = int(out["valid"].sum().item())
    import ctypes as C
    L = mi.lib()
    emb, val = out["embeddings"], out["valid"]
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def whole():
        mi.api._check(L.mi_fe_infer_face_items(fe.h, ptr(frames), B, W, H, 3 * W, ptr(res["faces"]), F, ptr(res["item_frame"]), ptr(res["item_face"]), M,
                                               ptr(emb), ptr(val), None, None, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))
    chips = torch.rand((M, 112, 112, 3), dtype=torch.float32, device="cuda")
    raw = torch.zeros((M, D), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    outs = (C.c_void_p * 1)(raw.data_ptr())

    def network():
        mi.api._check(L.mi_model_run(fe.model.h, ptr(chips), M, outs, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))
    r_whole, r_net = timed(whole), timed(network)
    case_a = {"what": "mi_fe_infer_face_items: %d device-resident %dx%d frames, %d items, synthetic D = %d network" % (B, H, W, M, D),
              "valid_items": valid, "whole call": r_whole, "network alone (mi_model_run, %d chips)" % M: r_net,
              "chip + l2_norm launches (whole call minus network), ms": round(r_whole["ms_median"] - r_net["ms_median"], 4),
              "note": "the network is synthetic (mesh-like trunk to 7x7x128, one whole-frame convolution): its time describes no real model"}
    fe.close()
    del frames, chips

    # ---- (b)
    n, m, D2 = 512, 65536, 512
    g = torch.Generator(device="cuda").manual_seed(3)
    qa = torch.randn((n, D2), dtype=torch.float32, device="cuda", generator=g)
    gb = torch.randn((m, D2), dtype=torch.float32, device="cuda", generator=g)
    sim = torch.empty((n, m), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def matrix():
        mi.api._check(L.mi_similarity_matrix(0, ptr(qa), n, ptr(gb), m, D2, ptr(sim), mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))
    r_sim = timed(matrix)
    ref = torch.nn.functional.normalize(qa[:8].double(), dim=1) @ torch.nn.functional.normalize(gb[:4096].double(), dim=1).T
    err = float((sim[:8, :4096].double() - ref).abs().max().item())
    tflops = 2.0 * n * m * D2 / (r_sim["ms_median"] * 1e-3) / 1e12
    case_b = {"what": "mi_similarity_matrix: n = %d, m = %d, D = %d, device memory" % (n, m, D2), "time": r_sim, "tflops": round(tflops, 2),
              "f32 matrix peak, TFLOP/s": F32_MATRIX_PEAK_TFLOPS, "fraction of peak": round(tflops / F32_MATRIX_PEAK_TFLOPS, 3),
              "untuned 4096^3 GEMM on the same instruction, TFLOP/s": UNTUNED_GEMM_TFLOPS, "max |out - f64 cosine| on a corner": err}
    doc = {"what": "FaceEmbeddings on the device: HIP events on one caller stream, median of %d calls after %d warm-up calls" % (a.reps, WARM),
           "box": a.box, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "infer_face_items": case_a,
           "similarity_matrix": case_b}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
