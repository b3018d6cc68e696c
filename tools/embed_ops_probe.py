"""What the operators of pooled-head / ONNX-exported embedding graphs cost on the device (embed_ops_kernels.hip).  HIP events around one call on one
caller stream, 5 warm-up calls, the median of `--reps` calls with p10..p90 (as tools/resnet_probe.py); the contenders take turns in one process, in
an order that rotates round by round.  Writes profiles/embed_ops_probe.json.

  (a) TRANSPOSE NHWC -> NCHW and back on `--items` items of 56x56x64 and of 7x7x512 (transpose_tiled_kernel through mi_model_run) against
      torch.permute(...).contiguous() of the same tensor on the same stream — the stock routine a user would otherwise get.
      Requirement: our median at or below torch's p90 (the margin is torch's own run-to-run spread).
  (b) tests/embed_ops_synth.onnx_style(c0 = 64, blocks = (2, 2, 2, 2)), D = 512, `--items` chips through mi_model_run: the "nchw" writing (its
      transposes removed by csrc/layout.hpp) against the "nhwc" writing.  The launch lists are equal, so the two medians should differ by less than
      the wider of the two p10..p90 ranges.
  (c) informational: avgpool_kernel (the 7x7 whole-frame average of 7x7x512) and l2norm_rows_kernel ([1,512]) at `--items` items, with the bytes per
      second they reach beside the float4-copy rate README quotes.
"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box", default=platform.node(), help="the name the measured machine goes by in the JSON (default: its host name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_ops_probe.json"))
    ap.add_argument("--items", type=int, default=512)
    a = ap.parse_args()
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    import embed_ops_synth as es
    if mi.device_count() < 1:
        raise RuntimeError("embed_ops_probe needs an MI355X: no HIP device visible")
    stream = torch.cuda.Stream()
    L = mi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def taking_turns(calls):
        """calls: name -> callable; every contender warmed up, then one timed call each per round, the order rotating round by round"""
        names = list(calls)
        for call in calls.values():
            for _ in range(WARM):
                call()
        stream.synchronize()
        ms = {k: [] for k in calls}
        for r in range(a.reps):
            for k in names[r % len(names):] + names[:r % len(names)]:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                calls[k]()
                t1.record(stream)
                t1.synchronize()
                ms[k].append(t0.elapsed_time(t1))
        out = {}
        for k, v in ms.items():
            v = np.sort(np.asarray(v))
            q = lambda f: round(float(v[min(int(f * len(v)), len(v) - 1)]), 4)
            out[k] = {"ms_median": q(0.5), "ms_p10": q(0.1), "ms_p90": q(0.9), "reps": a.reps}
        return out

    def model(blob):
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "g.tflite")
            with open(path, "wb") as f:
                f.write(blob)
            return mi.Model(path)

    def runner(m, x, y):
        po = (C.c_void_p * 1)(y.data_ptr())
        B = int(x.shape[0])
        return lambda: mi.api._check(L.mi_model_run(m.h, ptr(x), B, po, mi.MI_MEM_DEVICE, C.c_void_p(stream.cuda_stream)))

    def gbps(nbytes, r):
        return round(nbytes / (r["ms_median"] * 1e-3) / 1e9, 1)

    # ---- (a)
    transposes = []
    for h, w, c in ((56, 56, 64), (7, 7, 512)):
        for what, shape, perm in (("NHWC -> NCHW", (h, w, c), (0, 3, 1, 2)), ("NCHW -> NHWC", (c, h, w), (0, 2, 3, 1))):
            x = torch.randn((a.items,) + shape, dtype=torch.float32, device="cuda")
            y = torch.zeros((a.items,) + tuple(shape[p - 1] for p in perm[1:]), dtype=torch.float32, device="cuda")
            m = model(es.transpose_graph(*shape, perm))
            torch.cuda.synchronize()
            kernels = [r["kernel"] for r in m.profile(x, reps=1)]
            keep = []

            def stock():
                with torch.cuda.stream(stream):
                    keep[:] = [x.permute(*perm).contiguous()]
            r = taking_turns({"transpose_kernel": runner(m, x, y), "torch permute().contiguous()": stock})
            stream.synchronize()
            r["equal to torch"] = bool(torch.equal(y, keep[0]))
            r["kernels"] = kernels
            nbytes = 2 * 4 * x.numel()
            for k in ("transpose_kernel", "torch permute().contiguous()"):
                r[k]["GB/s (read + write)"] = gbps(nbytes, r[k])
            r["our median at or below torch's p90"] = bool(r["transpose_kernel"]["ms_median"] <= r["torch permute().contiguous()"]["ms_p90"])
            r["shape"] = "%s, %d items of %dx%dx%d" % (what, a.items, h, w, c)
            transposes.append(r)
            m.close()
            del x, y, keep

    # ---- (b)
    D, c0, blocks = 512, 64, (2, 2, 2, 2)
    chips = torch.rand((a.items, 112, 112, 3), dtype=torch.float32, device="cuda")
    hs = {layout: model(es.onnx_style(21, D, c0=c0, blocks=blocks, layout=layout)) for layout in ("nchw", "nhwc")}
    raws = {k: torch.zeros((a.items, D), dtype=torch.float32, device="cuda") for k in hs}
    torch.cuda.synchronize()
    lists = {k: [r["kernel"] for r in m.profile(chips[:8], reps=1)] for k, m in hs.items()}
    net = taking_turns({k: runner(m, chips, raws[k]) for k, m in hs.items()})
    stream.synchronize()
    spread = max(net[k]["ms_p90"] - net[k]["ms_p10"] for k in hs)
    net["launch lists equal"] = bool(lists["nchw"] == lists["nhwc"])
    net["transposes in the nchw launch list"] = sum("transpose" in k for k in lists["nchw"])
    net["outputs equal bit for bit"] = bool(torch.equal(raws["nchw"], raws["nhwc"]))
    net["|difference of the medians|, ms"] = round(abs(net["nchw"]["ms_median"] - net["nhwc"]["ms_median"]), 4)
    net["the wider p10..p90 range, ms"] = round(spread, 4)
    net["medians differ by less than the wider p10..p90 range"] = bool(abs(net["nchw"]["ms_median"] - net["nhwc"]["ms_median"]) < spread)
    net["what"] = "onnx_style(c0 = %d, blocks = %s), D = %d: %d chips through mi_model_run, the \"nchw\" writing against the \"nhwc\" writing" % (c0, blocks, D, a.items)
    for m in hs.values():
        m.close()
    del chips, raws

    # ---- (c)
    info = []
    for what, blob, in_shape, out_shape in (("avgpool_kernel: 7x7 VALID on 7x7x512", es.avgpool_graph(7, 7, 512, 7, 7), (7, 7, 512), (1, 1, 512)),
                                            ("l2norm_rows_kernel: [1,512]", es.l2norm_graph((1, 1, 1, 512)), (1, 1, 512), (1, 1, 512))):
        x = torch.randn((a.items,) + in_shape, dtype=torch.float32, device="cuda")
        y = torch.zeros((a.items,) + out_shape, dtype=torch.float32, device="cuda")
        m = model(blob)
        torch.cuda.synchronize()
        kernels = [r["kernel"] for r in m.profile(x, reps=1)]
        r = taking_turns({"run": runner(m, x, y)})["run"]
        r["GB/s (read + write)"] = gbps(4 * (x.numel() + y.numel()), r)
        r["what"], r["kernels"], r["items"] = what, kernels, a.items
        info.append(r)
        m.close()

    doc = {"what": "operators of pooled-head / ONNX-exported embedding graphs; HIP events on one caller stream, median of %d calls after %d warm-up calls, "
                   "contenders in a rotating order in one process" % (a.reps, WARM),
           "box": a.box, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "transpose against torch": transposes,
           "network, ONNX-style against NHWC": net,
           "informational": info}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
