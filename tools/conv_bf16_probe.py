"""What engine option "conv_bf16" buys on a ResNet-style embedding network: conv_bf16_kernel at 1 ("bf16": operands rounded to bf16) and at 2
("bf16x3": operands split into two bf16 values, three MFMAs for one) against conv_mfma_kernel (0, with conv_mfma = 1).  HIP events around one
call on one caller stream, 5 warm-up calls, the median of `--reps` calls with p10..p90 (as tools/resnet_probe.py); the three settings are three
handles on the same graph that take turns call by call in one process.  Writes profiles/conv_bf16_probe.json.

  (a) the four IResNet body shapes as single layers, 3x3 stride 1 SAME, 128 items: 56x56x64, 28x28x128, 14x14x256, 7x7x512 (C -> C)
  (b) tests/resnet_synth.iresnet_like(c0 = 64, blocks = (2, 2, 2, 2)), D = 512, 512 chips through mi_model_run
  (c) mi_fe_infer_face_items with that model: 128 device-resident 720 x 1080 frames, 512 items

Per case: ms, TFLOP/s (2 M K N of the convolution — at 2 the USEFUL flop, not the tripled ones), the share of the 2.5 PFLOP/s dense bf16
matrix peak, input + output bytes over the time; for the network max |raw - raw0| / max |raw0| and the smallest cosine against value 0 over the
chips.  The requirement: on every shape of (a) and on (b) the medians of 1 and 2 lie below the p10 of 0.  Also: how far 2 is behind 1."""
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
BF16_MATRIX_PEAK_TFLOPS, F32_MATRIX_PEAK_TFLOPS = 2500.0, 157.3
KEYS = (("conv_bf16=0", 0), ("conv_bf16=1", 1), ("conv_bf16=2", 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bf16_probe.json"))
    ap.add_argument("--items", type=int, default=128, help="items of the single layers (a)")
    ap.add_argument("--chips", type=int, default=512, help="chips of the network run (b) and items of (c)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    import resnet_synth as rs
    if mi.device_count() < 1:
        raise RuntimeError("conv_bf16_probe needs an MI355X: no HIP device visible")
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

    def three_handles(blob, d):
        path = os.path.join(d, "g.tflite")
        with open(path, "wb") as f:
            f.write(blob)
        hs = {}
        for key, v in KEYS:
            hs[key] = mi.Model(path)
            hs[key].set_option("conv_mfma", 1)
            hs[key].set_option("conv_bf16", v)
        return hs

    def runner(m, x, outs):
        po = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        B = int(x.shape[0])
        return lambda: mi.api._check(L.mi_model_run(m.h, ptr(x), B, po, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))

    def verdict(r):
        for k in ("conv_bf16=1", "conv_bf16=2"):
            r["median of %s below p10 of conv_bf16=0" % k] = bool(r[k]["ms_median"] < r["conv_bf16=0"]["ms_p10"])
            r["speedup of %s over conv_bf16=0 (medians)" % k] = round(r["conv_bf16=0"]["ms_median"] / r[k]["ms_median"], 2)
        r["conv_bf16=2 behind conv_bf16=1 (ratio of medians)"] = round(r["conv_bf16=2"]["ms_median"] / r["conv_bf16=1"]["ms_median"], 3)
        return r

    def closeness(r, ys):
        y0 = ys["conv_bf16=0"].double()
        for k in ("conv_bf16=1", "conv_bf16=2"):
            y = ys[k].double()
            r[k]["max |y - y0| / max |y0|"] = float(((y - y0).abs().max() / y0.abs().max()).item())

    # ---- (a)
    layers = []
    for hw, c in ((56, 64), (28, 128), (14, 256), (7, 512)):
        blob, _ = rs.conv_layer(500 + c, hw, hw, c, c)
        x = torch.randn((a.items, hw, hw, c), dtype=torch.float32, device="cuda")
        with tempfile.TemporaryDirectory() as d:
            hs = three_handles(blob, d)
        ys = {k: torch.zeros((a.items, hw, hw, c), dtype=torch.float32, device="cuda") for k in hs}
        torch.cuda.synchronize()
        kernels = {k: [r["kernel"] for r in m.profile(x, reps=1)] for k, m in hs.items()}
        r = verdict(taking_turns({k: runner(m, x, [ys[k]]) for k, m in hs.items()}))
        flop = 2.0 * a.items * hw * hw * (9 * c) * c
        io_bytes = 2.0 * a.items * hw * hw * c * 4
        for k in hs:
            r[k]["tflops (useful)"] = round(flop / (r[k]["ms_median"] * 1e-3) / 1e12, 2)
            r[k]["fraction of the bf16 matrix peak"] = round(r[k]["tflops (useful)"] / BF16_MATRIX_PEAK_TFLOPS, 4)
            r[k]["input + output, TB/s"] = round(io_bytes / (r[k]["ms_median"] * 1e-3) / 1e12, 3)
            r[k]["kernels"] = kernels[k]
        closeness(r, ys)
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
        hs = three_handles(blob, d)
    raws = {k: torch.zeros((a.chips, D), dtype=torch.float32, device="cuda") for k in hs}
    torch.cuda.synchronize()
    net = verdict(taking_turns({k: runner(m, chips, [raws[k]]) for k, m in hs.items()}))
    macs = hs["conv_bf16=0"].plan_stats()[1]
    io_bytes = 4.0 * a.chips * (112 * 112 * 3 + D)
    for k in hs:
        tf = 2.0 * macs * a.chips / (net[k]["ms_median"] * 1e-3) / 1e12
        net[k]["tflops, whole network (2 x the plan's MACs per frame x chips over the call's time; useful flop)"] = round(tf, 2)
        net[k]["fraction of the bf16 matrix peak"] = round(tf / BF16_MATRIX_PEAK_TFLOPS, 4)
        net[k]["input + output of the call, TB/s"] = round(io_bytes / (net[k]["ms_median"] * 1e-3) / 1e12, 5)
    closeness(net, raws)
    unit = lambda t: t.double() / t.double().norm(dim=1, keepdim=True)
    for k in ("conv_bf16=1", "conv_bf16=2"):
        net[k]["smallest cosine against conv_bf16=0 over the chips"] = float((unit(raws[k]) * unit(raws["conv_bf16=0"])).sum(dim=1).min().item())
    for k, m in hs.items():   # where the call's time goes: Model.profile (eager launches, an event between launches, 3 repetitions), summed by kernel
        by = {}
        for r in m.profile(chips, reps=3):
            by[r["kernel"]] = round(by.get(r["kernel"], 0.0) + float(r["ms"]), 3)
        net[k]["ms by kernel (Model.profile, eager launches)"] = by
    net["max |raw0|"] = float(raws["conv_bf16=0"].abs().max().item())
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
    fes = {key: mi.FaceEmbeddings(model_bytes=blob, precision=("f32", "bf16", "bf16x3")[v]) for key, v in KEYS}
    outs = {k: fe.infer_items(frames, res, stream=stream.cuda_stream) for k, fe in fes.items()}
    stream.synchronize()

    def whole(k):
        fe, emb, val = fes[k], outs[k]["embeddings"], outs[k]["valid"]
        return lambda: mi.api._check(L.mi_fe_infer_face_items(fe.h, ptr(frames), B, W, H, 3 * W, ptr(res["faces"]), F, ptr(res["item_frame"]), ptr(res["item_face"]), M,
                                                               ptr(emb), ptr(val), None, None, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))
    items = verdict(taking_turns({k: whole(k) for k in fes}))
    io_bytes = float(B) * H * W * 3 + 4.0 * M * D
    for k in fes:
        tf = 2.0 * macs * M / (items[k]["ms_median"] * 1e-3) / 1e12
        items[k]["tflops, the network's useful flop over the call's time"] = round(tf, 2)
        items[k]["fraction of the bf16 matrix peak"] = round(tf / BF16_MATRIX_PEAK_TFLOPS, 4)
        items[k]["frames in + embeddings out, TB/s"] = round(io_bytes / (items[k]["ms_median"] * 1e-3) / 1e12, 4)
    for k in ("conv_bf16=1", "conv_bf16=2"):
        items[k]["smallest cosine against conv_bf16=0 over the items"] = float((outs[k]["embeddings"].double() * outs["conv_bf16=0"]["embeddings"].double()).sum(dim=1).min().item())
    items["what"] = "mi_fe_infer_face_items: %d device-resident %dx%d frames, %d items, the network of (b)" % (B, H, W, M)
    items["valid_items"] = int(outs["conv_bf16=0"]["valid"].sum().item())
    for fe in fes.values():
        fe.close()

    doc = {"what": "engine option conv_bf16: conv_bf16_kernel at 1 (bf16) and 2 (bf16x3) against conv_mfma_kernel (0, conv_mfma = 1), three handles taking turns; HIP events "
                   "on one caller stream, median of %d calls after %d warm-up calls" % (a.reps, WARM),
           "box": a.box, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "bf16 matrix peak (dense), TFLOP/s": BF16_MATRIX_PEAK_TFLOPS, "f32 matrix peak, TFLOP/s": F32_MATRIX_PEAK_TFLOPS,
           "note": "the networks are synthetic (tests/resnet_synth.py): the reference's ArcFace model cannot be fetched and has not been run",
           "single layers": layers, "network": net, "infer_face_items": items}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
