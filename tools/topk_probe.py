"""What identification against a gallery costs on the device.  Writes profiles/topk_probe.json.

One process, device-resident operands, HIP events around one call on a caller stream, `--warmup` calls of every contender, then `--reps`
rounds in which the contenders take turns in a rotating order (as tools/render_items_probe.py): the median with p10..p90.

  large   n = 512 queries against a gallery of m = 65536, D = 512 (the shape of mi_similarity_matrix's figure in profiles/embeddings_probe.json),
          k in {1, 5, 16}:
            (a) mi_similarity_matrix alone
            (b) (a) followed by torch.topk of its output on the same stream: what a caller did before mi_gallery_topk
            (c) mi_gallery_topk
          REQUIRED: the median of (c) is below (b)'s p10 for every k.  (c) against (a) is reported as measured.  (c)'s results are checked
          against torch.topk of (a)'s output where the k-th and (k+1)-th scores of a row differ (exact ties may be ordered differently by torch).
  small   n = 4 (a handful of faces from one frame) against the same gallery, k = 5: `splits` automatic and forced to its neighbours — the
          case automatic `splits` exists for."""
import argparse
import ctypes as C
import datetime
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, M, D = 512, 65536, 512
KS = (1, 5, 16)
SMALL_N, SMALL_K = 4, 5
SMALL_SPLITS = (0, 8, 16, 32, 48, 64)   # 0: automatic


def rotate(calls, reps, warm, stream, torch, np):
    """name -> callable; every contender warmed up, then `reps` rounds in a rotating order -> name -> {ms_median, ms_p10, ms_p90, reps}"""
    for _ in range(warm):
        for call in calls.values():
            call()
    stream.synchronize()
    ms = {tag: [] for tag in calls}
    tags = list(calls)
    for r in range(reps):
        o = r % len(tags)
        for tag in tags[o:] + tags[:o]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            calls[tag]()
            t1.record(stream)
            t1.synchronize()
            ms[tag].append(t0.elapsed_time(t1))
    return {tag: {"ms_median": round(float(np.median(v)), 4), "ms_p10": round(float(np.percentile(v, 10)), 4),
                  "ms_p90": round(float(np.percentile(v, 90)), 4), "reps": len(v)} for tag, v in ms.items()}


def measure(reps, warm):
    import numpy as np
    import torch
    import rs_face_detection_tflite_amd as mi
    L = mi.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cuda").manual_seed(3)
    queries = torch.randn((N, D), dtype=torch.float32, device="cuda", generator=g)
    rows = torch.randn((M, D), dtype=torch.float32, device="cuda", generator=g)
    sim = torch.empty((N, M), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gallery = mi.Gallery(rows)
    stream = torch.cuda.Stream()
    s = C.c_void_p(stream.cuda_stream)

    def matrix():
        mi.api._check(L.mi_similarity_matrix(0, ptr(queries), N, ptr(rows), M, D, ptr(sim), mi.MI_MEM_DEVICE, s))
    large = {}
    for k in KS:
        index = torch.empty((N, k), dtype=torch.int32, device="cuda")
        score = torch.empty((N, k), dtype=torch.float32, device="cuda")
        label = torch.empty((N, k), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        kept = {}

        def matrix_then_torch_topk():
            matrix()
            with torch.cuda.stream(stream):
                kept["topk"] = torch.topk(sim, k, dim=1)

        def gallery_topk():
            mi.api._check(L.mi_gallery_topk(gallery.h, ptr(queries), N, k, ptr(index), ptr(score), ptr(label), mi.MI_MEM_DEVICE, s))
        timing = rotate({"a": matrix, "b": matrix_then_torch_topk, "c": gallery_topk}, reps, warm, stream, torch, np)
        # the results: (c)'s scores are (a)'s bits; the indices are torch's wherever torch had no tie to break at the cut
        stream.synchronize()
        values, indices = kept["topk"]
        more = torch.topk(sim, k + 1, dim=1).values
        decided = (more[:, k - 1] > more[:, k])
        scores_equal = bool(torch.equal(score.view(torch.int32), values.view(torch.int32)))
        rows_equal = bool((index[decided].long() == indices[decided]).all().item()) if k == 1 else \
            bool((torch.sort(index[decided].long(), dim=1).values == torch.sort(indices[decided], dim=1).values).all().item())
        a, b, c = (timing[t] for t in "abc")
        large["k=%d" % k] = {"timing": timing, "c_median_below_b_p10": bool(c["ms_median"] < b["ms_p10"]),
                             "c_over_a": round(c["ms_median"] / a["ms_median"], 3), "b_minus_a_ms": round(b["ms_median"] - a["ms_median"], 4),
                             "scores_bit_equal_to_torch_topk_of_a": scores_equal, "rows_equal_where_torch_had_no_tie": rows_equal,
                             "rows_decided": int(decided.sum().item())}
    # ---- the small batch
    small_q = queries[:SMALL_N].contiguous()
    index = torch.empty((SMALL_N, SMALL_K), dtype=torch.int32, device="cuda")
    score = torch.empty((SMALL_N, SMALL_K), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    handles = {}
    for splits in SMALL_SPLITS:
        h = mi.Gallery(rows)
        h.set_option("splits", splits)
        handles["splits=%s" % (splits or "auto")] = h
    call_of = lambda h: (lambda: mi.api._check(L.mi_gallery_topk(h.h, ptr(small_q), SMALL_N, SMALL_K, ptr(index), ptr(score), None, mi.MI_MEM_DEVICE, s)))
    small = rotate({tag: call_of(h) for tag, h in handles.items()}, reps, warm, stream, torch, np)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for h in handles.values():
        h.close()
    gallery.close()
    return {"large": {"shape": "n = %d, m = %d, D = %d" % (N, M, D),
                      "contenders": {"a": "mi_similarity_matrix", "b": "mi_similarity_matrix, then torch.topk on the same stream", "c": "mi_gallery_topk"},
                      "by_k": large, "required_c_median_below_b_p10_for_every_k": all(v["c_median_below_b_p10"] for v in large.values())},
            "small": {"shape": "n = %d, m = %d, D = %d, k = %d" % (SMALL_N, M, D, SMALL_K), "compute_units": cus,
                      "automatic_splits": min(64, cus, M // 128), "timing": small}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--box", default="", help="name of the machine, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_probe.json"))
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 repetitions")
    import rs_face_detection_tflite_amd as mi
    if mi.device_count() < 1:
        sys.exit("topk_probe needs a GPU: no HIP device visible")
    import torch
    report = {"entries": "mi_similarity_matrix / torch.topk / mi_gallery_topk, MI_MEM_DEVICE, caller stream, HIP events around one call, contenders in turn",
              "box": args.box or "%s (host %s)" % (torch.cuda.get_device_name(0), socket.gethostname()), "date": datetime.date.today().isoformat(),
              "run": measure(args.reps, args.warmup)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))
