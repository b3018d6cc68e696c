"""What a ResNet-style embedding network costs on the device, with its dense convolutions on conv_mfma_kernel (option conv_mfma = 1, the default)
and on conv_generic_kernel (conv_mfma = 0).  HIP events around one call on one caller stream, 5 warm-up calls, the median of `--reps` calls with
p10..p90 (as tools/embeddings_probe.py); the two settings are two handles on the same graph that take turns call by call in one process.
Writes profiles/resnet_probe.json.

  (a) the four IResNet body shapes as single layers, 3x3 stride 1 SAME, 128 items: 56x56x64, 28x28x128, 14x14x256, 7x7x512 (C -> C): ms and
      TFLOP/s (2 M K N flop) next to the 157.3 TFLOP/s f32 matrix peak, and next to the 97.7 TFLOP/s that sim_tile.hpp — the tile this kernel is
      modelled on, a plain GEMM without the gather — reached at 512 x 65536 x 512 (profiles/embeddings_probe.json)
  (b) tests/resnet_synth.iresnet_like(c0 = 64, blocks = (2, 2, 2, 2)), D = 512, 512 chips through mi_model_run
  (c) mi_fe_infer_face_items with that model: 128 device-resident 720 x 1080 frames, 512 items (as tools/embeddings_probe.py measures the synthetic one)

The requirement the figures are held to: on each shape of (a) and on (b) the new kernel's median lies below the generic kernel's p10."""
import argparse
import ctypes as C
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
F32_MATRIX_PEAK_TFLOPS, SIM_TILE_TFLOPS = 157.3, 97.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_probe.json"))
    ap.add_argument("--items", type=int, default=128, help="items of the single layers (a)")
    ap.add_argument("--chips", type=int, default=512, help="chips of the network run (b) and items of (c)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    import resnet_synth as rs
    if mi.device_count() < 1:
        raise RuntimeError("resnet_probe needs an MI355X: no HIP device visible")
    stream = torch.cuda.Stream()
    L = mi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def taking_turns(calls):
        """calls: name -> callable; every contender warmed up, then one timed call each, round after round"""
        for call in calls.values():
            for _ in range(WARM):
                call()
        stream.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, call in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call()
                t1.record(stream)
                t1.synchronize()
                ms[k].append(t0.elapsed_time(t1))
        out = {}
        for k, v in ms.items():
            v = np.sort(np.asarray(v))
            q = lambda f: round(float(v[min(int(f * len(v)), len(v) - 1)]), 4)
            out[k] = {"ms_median": q(0.5), "ms_p10": q(0.1), "ms_p90": q(0.9), "reps": a.reps}
        return out

    def two_handles(blob, d):
        path = os.path.join(d, "g.tflite")
        with open(path, "wb") as f:
            f.write(blob)
        hs = {}
        for key, v in (("conv_mfma=1", 1), ("conv_mfma=0", 0)):
            hs[key] = mi.Model(path)
            hs[key].set_option("conv_mfma", v)
        return hs

    def runner(m, x, outs):
        po = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        B = int(x.shape[0])
        return lambda: mi.api._check(L.mi_model_run(m.h, ptr(x), B, po, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))

    def verdict(r):
        r["median of conv_mfma=1 below p10 of conv_mfma=0"] = bool(r["conv_mfma=1"]["ms_median"] < r["conv_mfma=0"]["ms_p10"])
        r["speedup (medians)"] = round(r["conv_mfma=0"]["ms_median"] / r["conv_mfma=1"]["ms_median"], 2)
        return r

    # ---- (a)
    layers = []
    for hw, c in ((56, 64), (28, 128), (14, 256), (7, 512)):
        blob, _ = rs.conv_layer(500 + c, hw, hw, c, c)
        x = torch.randn((a.items, hw, hw, c), dtype=torch.float32, device="cuda")
        with tempfile.TemporaryDirectory() as d:
            hs = two_handles(blob, d)
        ys = {k: torch.zeros((a.items, hw, hw, c), dtype=torch.float32, device="cuda") for k in hs}
        torch.cuda.synchronize()
        kernels = {k: [r["kernel"] for r in m.profile(x, reps=1)] for k, m in hs.items()}
        r = verdict(taking_turns({k: runner(m, x, [ys[k]]) for k, m in hs.items()}))
        flop = 2.0 * a.items * hw * hw * (9 * c) * c
        for k in hs:
            r[k]["tflops"] = round(flop / (r[k]["ms_median"] * 1e-3) / 1e12, 2)
            r[k]["fraction of the f32 matrix peak"] = round(r[k]["tflops"] / F32_MATRIX_PEAK_TFLOPS, 3)
            r[k]["kernels"] = kernels[k]
        r["max |conv_mfma=1 - conv_mfma=0|"] = float((ys["conv_mfma=1"] - ys["conv_mfma=0"]).abs().max().item())
        r["shape"] = "%dx%dx%d -> %d, 3x3 s1 SAME, %d items: M = %d, N = %d, K = %d" % (hw, hw, c, c, a.items, a.items * hw * hw, c, 9 * c)
        layers.append(r)
        for m in hs.values():
            m.close()
        del x, ys

    # ---- (b), (c)
    D, c0, blocks = 512, 64, (2, 2, 2, 2)
    blob = rs.iresnet_like(21, D, c0=c0, blocks=blocks)
    chips = torch.rand((a.chips, 112, 112, 3), dtype=torch.float32, device="cuda")
    with tempfile.TemporaryDirectory() as d:
        hs = two_handles(blob, d)
    raws = {k: torch.zeros((a.chips, D), dtype=torch.float32, device="cuda") for k in hs}
    torch.cuda.synchronize()
    net = verdict(taking_turns({k: runner(m, chips, [raws[k]]) for k, m in hs.items()}))
    macs = hs["conv_mfma=1"].plan_stats()[1]
    for k in hs:
        net[k]["tflops, whole network (2 x the plan's MACs per frame x chips over the call's time)"] = round(2.0 * macs * a.chips / (net[k]["ms_median"] * 1e-3) / 1e12, 2)
    net["max |conv_mfma=1 - conv_mfma=0|"] = float((raws["conv_mfma=1"] - raws["conv_mfma=0"]).abs().max().item())
    net["max |raw|"] = float(raws["conv_mfma=1"].abs().max().item())
    net["what"] = "iresnet_like(c0 = %d, blocks = %s), D = %d: %d chips through mi_model_run, %.3g MACs per chip" % (c0, blocks, D, a.chips, macs)
    for m in hs.values():
        m.close()
    del chips, raws

    B, H, W, F = a.chips // 4, 720, 1080, 4
    M = B * F
    rng = np.random.RandomState(7)
    frames = torch.from_numpy(rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda()
    faces = np.zeros((B, F, 17), np.float32)
    for b in range(B):
        for k in range(F):   # boxes of 100 .. 300 pixels, inside the frame
            w, h = rng.randint(100, 301, 2)
            x, y = rng.randint(0, W - w), rng.randint(0, H - h)
            faces[b, k, :4] = ((x + 0.25) / W, (y + 0.25) / H, (x + w + 0.5) / W, (y + h + 0.5) / H)
    item_frame, item_face = np.repeat(np.arange(B, dtype=np.int32), F), np.tile(np.arange(F, dtype=np.int32), B)
    res = {k: torch.from_numpy(v).cuda() for k, v in dict(faces=faces, item_frame=item_frame, item_face=item_face).items()}
    fes = {}
    for key, v in (("conv_mfma=1", 1), ("conv_mfma=0", 0)):
        fes[key] = mi.FaceEmbeddings(model_bytes=blob)
        fes[key].model.set_option("conv_mfma", v)
    outs = {k: fe.infer_items(frames, res, stream=stream.cuda_stream) for k, fe in fes.items()}
    stream.synchronize()

    def whole(k):
        fe, emb, val = fes[k], outs[k]["embeddings"], outs[k]["valid"]
        return lambda: mi.api._check(L.mi_fe_infer_face_items(fe.h, ptr(frames), B, W, H, 3 * W, ptr(res["faces"]), F, ptr(res["item_frame"]), ptr(res["item_face"]), M,
                                                               ptr(emb), ptr(val), None, None, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))
    items = verdict(taking_turns({k: whole(k) for k in fes}))
    items["what"] = "mi_fe_infer_face_items: %d device-resident %dx%d frames, %d items, the network of (b)" % (B, H, W, M)
    items["valid_items"] = int(outs["conv_mfma=1"]["valid"].sum().item())
    for fe in fes.values():
        fe.close()

    doc = {"what": "ResNet-style embedding graphs: conv_mfma_kernel (conv_mfma = 1) against conv_generic_kernel (conv_mfma = 0), two handles taking turns; HIP events on one "
                   "caller stream, median of %d calls after %d warm-up calls" % (a.reps, WARM),
           "box": a.box, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "f32 matrix peak, TFLOP/s": F32_MATRIX_PEAK_TFLOPS,
           "sim_tile.hpp at 512 x 65536 x 512 (mi_similarity_matrix, profiles/embeddings_probe.json), TFLOP/s": SIM_TILE_TFLOPS,
           "note": "the networks are synthetic (tests/resnet_synth.py): the reference's ArcFace model cannot be fetched and has not been run",
           "single layers": layers, "network": net, "infer_face_items": items}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
