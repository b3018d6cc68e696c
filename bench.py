#!/usr/bin/env python3
"""bench.py — BASELINE.json metric: faces/sec at batch=256 (256x256 BackCamera) per GPU, 1/2/4/8-GPU weak scaling.

    python bench.py                      # N = 1, configs[1] of BASELINE.json (the headline)
    python bench.py --gpus 8             # starts 8 ranks itself (one process per GPU, RCCL) and prints rank 0's line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P bench.py --gpus 8
    python bench.py --config 1           # ShortRange / FrontCamera 128x128, 256 frames/GPU (configs[0]'s model, batched)
    python bench.py --config 3           # FaceLandmark 192x192, 512 ROIs/GPU           (configs[2])
    python bench.py --config 5 --gpus 8  # full_range -> mesh -> 2 x iris, 128 frames/GPU (configs[4])

One "step" = one pass of the hot path over one batch per GPU, inputs already resident in HBM:
  config 2 (default; with --gpus N it is configs[3]): BackCamera network + SSD decode + sigmoid + weighted NMS + letterbox
           removal on 256 synthetic 256x256 frames per GPU;
  config 3: face-mesh network + face flag + landmark projection on 512 ROIs per GPU;
  config 5: mi_pipeline_run on 128 RGB frames of 192x192 per GPU (device pre-processing, three networks, ROI maths).
One process per GPU.  With N > 1 the frozen .tflite bytes are broadcast from rank 0 over RCCL (torch.distributed "nccl"),
frames are sharded per GPU and no data-path collective exists (frames are independent): "scaling": "weak".

A plain run sets up, warms up, times the K steps once and prints ONE JSON line on rank 0 (`metric`, `value`, `unit`,
`ms_per_step`, ...).  With --full that line also carries what takes runs of its own: repeated timing windows, the
one-batch-in-flight figure, `roofline` (dominant kernel, timed live with HIP events on the launch stream), configs 1 / 3 / 5
as `secondary_configs`, the host-fed variant, the single-image latencies and, at N = 1, `cpu_baseline` (the C oracle on the
host cores — a *port*: the reference's TFLite path cannot be built here).

    python bench.py --dump-outputs DIR   # also writes the last timed step's outputs as DIR/<name>.npy (float32)
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_PEAK_TFLOPS = 157.3  # dense f32 (MFMA = packed VALU FMA), /opt/skills/guides/MI355X_MICROARCH.md
# what the two pipes sustain on this part, every CU busy, two waves per SIMD (tools/valu_bench.hip, profiles/r03_valu_mfma_issue_rates.txt):
# reported beside `frac` (which stays achieved / data-sheet peak) as `frac_of_measured_ceiling`
# (round 4: the row pipelines' mix — 18 v_pk_fma_f32 + 24 v_mfma_f32_4x4x1_16b_f32 per stage — sustains 141 TFLOP/s, profiles/r04_valu_mfma_issue_rates.txt)
MEASURED_CEILING_TFLOPS = {"valu v_pk_fma_f32": 116.0, "mfma f32": 145.0, "mfma f32 4x4x1 (1x1 convs) + valu v_pk_fma_f32 (depthwise)": 141.0}
HBM_PEAK_GBS = 8000.0    # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)


# ------------------------------------------------------------------------------------------------- launcher (N > 1, no torchrun)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def kfd_gpu_nodes():
    """Number of GPU nodes the kernel driver lists, read from sysfs text files (no HIP, no amdsmi, no torch): a KFD topology
    node with simd_count > 0 is a GPU (CPU nodes have 0).  None when the topology is not readable (no driver, a container
    that hides /sys/class/kfd)."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        nodes = os.listdir(base)
    except OSError:
        return None
    count, readable = 0, 0
    for node in nodes:
        try:
            with open(os.path.join(base, node, "properties")) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
        except OSError:
            continue                    # a node the device cgroup hides from this container
        readable += 1
        if int(props.get("simd_count", "0")) > 0:
            count += 1
    return count if readable else None


def launch_ranks(args, argv):
    """`python bench.py --gpus N` without an external launcher.  This process never imports torch and makes no HIP / amdsmi call
    (a process that has touched the GPU must not start other programs on this pool): it reads the KFD topology from sysfs only
    to refuse early, starts N fresh child processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, lets rank 0 print the
    JSON line on the inherited stdout, and exits with the first non-zero child status after relaying that rank's stderr tail.
    Every child checks `torch.cuda.device_count() >= WORLD_SIZE` itself (exit status 2) before it touches a device."""
    import tempfile
    n = args.gpus
    if not args.rehearse:
        nodes = kfd_gpu_nodes()
        if nodes is not None and nodes < n:
            sys.stderr.write("bench.py: --gpus %d but only %d GPU(s) visible; refusing to run a smaller job under that label\n" % (n, nodes))
            return 2
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(n), BENCH_SPAWNED="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs, logs = [], []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        log = tempfile.TemporaryFile(mode="w+")
        logs.append(log)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=e, stderr=log))
    rc, failed = 0, None
    deadline = time.time() + 3600
    alive = list(procs)
    while alive and time.time() < deadline:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc, failed = code, procs.index(p)
                for q in alive:        # a rank died: the others would wait at the next barrier for ever
                    q.terminate()
        time.sleep(0.05)
    for p in alive:
        p.kill()
        rc = rc or 1
    for r, log in enumerate(logs):     # the dead rank's stderr tail first, then whatever the others said (warnings)
        log.seek(0)
        text = log.read()
        if text and (failed is None or r == failed):
            sys.stderr.write("".join("[rank %d] %s\n" % (r, line) for line in text[-4000:].splitlines()))
        log.close()
    sys.stderr.write("bench.py launcher: %d rank(s), status %d, torch imported in the launcher: %s\n" % (n, rc, "torch" in sys.modules))
    return rc


# ------------------------------------------------------------------------------------------------- synthetic inputs
def _gold():
    import numpy as np
    return np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))


def make_frames(batch, seed, size=256):
    """SURVEY.md §8d config 2 frame mix: 50% U(-1,1) noise, 50% face-bearing (committed man-face tensor with a seeded
    +-32 px roll and 0.8-1.2 gain) so that NMS sees real candidates."""
    import numpy as np
    u8 = _gold()["man_back_u8"].astype(np.float64)
    if size == 128:   # config 1 (front / short, 128x128): the same picture, 2x2 box-filtered; the roll scales with the frame
        u8 = u8.reshape(128, 2, 128, 2, 3).mean(axis=(1, 3))
    face = (u8 * 2.0 / 255.0 - 1.0).astype(np.float32)
    rs = np.random.RandomState(seed)
    x = np.empty((batch, size, size, 3), np.float32)
    for b in range(batch):
        if b % 2 == 0:
            x[b] = rs.uniform(-1, 1, (size, size, 3)).astype(np.float32)
        else:
            dy, dx = int(rs.randint(-size // 8, size // 8 + 1)), int(rs.randint(-size // 8, size // 8 + 1))
            x[b] = np.clip(np.roll(face, (dy, dx), axis=(0, 1)) * np.float32(rs.uniform(0.8, 1.2)), -1, 1)
    return x


def make_rois(batch, seed):
    """Config 3: 50% the committed 192x192 face crop with a seeded jitter, 50% U(0,1)."""
    import numpy as np
    face = _gold()["man_face_u8"].astype(np.float32) / np.float32(255.0)
    rs = np.random.RandomState(seed)
    x = np.empty((batch, 192, 192, 3), np.float32)
    for b in range(batch):
        if b % 2 == 0:
            x[b] = rs.uniform(0, 1, (192, 192, 3)).astype(np.float32)
        else:
            x[b] = np.roll(face, (int(rs.randint(-8, 9)), int(rs.randint(-8, 9))), axis=(0, 1))
    return x


def make_rgb_frames(batch, seed, size=192):
    """Config 5: 192x192 RGB frames, 50% the man picture (resized, seeded shift), 50% noise."""
    import numpy as np
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "man.jpg")).convert("RGB").resize((size, size)))
    rs = np.random.RandomState(seed)
    return np.stack([np.roll(img, (int(rs.randint(-10, 11)), int(rs.randint(-10, 11))), axis=(0, 1)) if b % 2
                     else rs.randint(0, 256, img.shape).astype(np.uint8) for b in range(batch)])


# ------------------------------------------------------------------------------------------------- CPU baseline (oracle = port)
def usable_cpus():
    """Host threads this process may actually run on: the scheduler affinity mask, cut down by a cgroup CPU quota if one is set
    (os.cpu_count() reports the whole host, which a 1-GPU box shares with seven others)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            fields = open(path).read().split()
            quota = int(fields[0]) if fields[0] != "max" else -1
            period = int(fields[1]) if len(fields) > 1 else int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0:
                n = max(1, min(n, quota // period))
        except (OSError, ValueError, IndexError):
            pass
    return n


CPU_THREADS_NOTE = ("threads = min(usable CPUs (affinity mask and cgroup quota), frames in the batch); one frame per thread, as "
                    "the reference runs TFLite single-threaded per image")


def cpu_baseline(x_host, threads, model_file="face_detection_back.tflite", kind="FD_BACK"):
    """The oracle (CPU port of the same graph + glue) on the GPU box's host cores, bounded sample: all cores over frames."""
    from oracle import pyoracle as po
    om = po.Model(os.path.join(ROOT, "models", model_file))
    anchors = po.ssd_anchors(getattr(po, kind))
    scale = float(x_host.shape[1])
    n = min(len(x_host), max(threads, 64))
    om.run(x_host[: min(n, threads)], nthreads=threads)  # warm (page-in, thread pool)
    t0 = time.time()
    frames = 0
    while time.time() - t0 < 10.0:
        rb, rs = om.run(x_host[:n], nthreads=threads)
        for f in range(n):
            po.fd_postprocess(rb[f], rs[f], anchors, scale)
        frames += n
    dt = time.time() - t0
    return {"value": round(frames / dt, 1), "unit": "faces/s", "cores": threads, "host_cpus": os.cpu_count(), "kind": "port",
            "sample": "%d frames of the same batch (net + decode + NMS), C oracle, OpenMP over frames, %.1f s" % (frames, dt),
            "threads_note": CPU_THREADS_NOTE}


def cpu_baseline_1thread(x_host, model_file="face_detection_back.tflite", kind="FD_BACK"):
    """The reference's own operating point (face_detection.rs:207-210: one image per call, one thread, the interpreter
    rebuilt inside every call): model parse + run + post-processing per frame, one thread."""
    from oracle import pyoracle as po
    path = os.path.join(ROOT, "models", model_file)
    anchors = po.ssd_anchors(getattr(po, kind))
    scale = float(x_host.shape[1])
    t0 = time.time()
    frames = 0
    while time.time() - t0 < 8.0:
        om = po.Model(path)                                    # InterpreterBuilder::build + allocate_tensors, per call
        rb, rs = om.run(x_host[frames % len(x_host)][None], nthreads=1)
        po.fd_postprocess(rb[0], rs[0], anchors, scale)
        frames += 1
    dt = time.time() - t0
    return {"value": round(frames / dt, 2), "unit": "faces/s", "cores": 1, "kind": "port",
            "sample": "%d single-frame calls (model parse + net + decode + NMS each), C oracle, 1 thread, %.1f s" % (frames, dt)}


def cpu_baseline_landmark(x_host, threads):
    """Config 3 on the host: the oracle's face mesh net over ROIs (OpenMP over ROIs) + face flag + landmark projection."""
    import numpy as np
    from oracle import pyoracle as po
    om = po.Model(os.path.join(ROOT, "models", "face_landmark.tflite"))
    n = min(len(x_host), max(threads, 64))
    om.run(x_host[: min(n, threads)], nthreads=threads)
    t0 = time.time()
    rois = 0
    while time.time() - t0 < 10.0:
        raw, flag = om.run(x_host[:n], nthreads=threads)
        for f in range(n):
            if po.lib().orc_face_flag_passes(float(flag[f].reshape(-1)[-1])):
                po.project_landmarks(raw[f], (192, 192), (192, 192))
        rois += n
    dt = time.time() - t0
    return {"value": round(rois / dt, 1), "unit": "ROIs/s", "cores": threads, "host_cpus": os.cpu_count(), "kind": "port",
            "sample": "%d ROIs of the same batch (net + flag + projection), C oracle, OpenMP over ROIs, %.1f s" % (rois, dt),
            "threads_note": CPU_THREADS_NOTE}


def cpu_baseline_pipeline(frames_u8, threads):
    """Config 5 on the host: lib.rs:18-40 through the oracle, staged over the batch so every net runs OpenMP-over-frames and the
    per-frame glue (crop / warp, decode + NMS, ROI maths) runs on a thread pool (ctypes drops the GIL inside the C calls)."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from oracle import pyoracle as po
    fd = po.Model(os.path.join(ROOT, "models", "face_detection_full_range.tflite"))
    fl = po.Model(os.path.join(ROOT, "models", "face_landmark.tflite"))
    ir = po.Model(os.path.join(ROOT, "models", "iris_landmark.tflite"))
    anchors = po.ssd_anchors(po.FD_FULL)
    size = fd.input_dims[1]
    pool = ThreadPoolExecutor(threads)

    def one_pass(imgs):
        H, W = imgs.shape[1:3]
        pre = list(pool.map(lambda im: po.image_to_tensor(im, None, (size, size), True, (-1., 1.), False), imgs))
        rb, rs = fd.run(np.stack([t for t, _ in pre]), nthreads=threads)
        dets = list(pool.map(lambda i: po.fd_postprocess(rb[i], rs[i], anchors, float(size), pre[i][1]), range(len(imgs))))
        faces = [i for i, d in enumerate(dets) if len(d)]
        if not faces:
            return 0
        rois = [po.face_detection_to_roi(dets[i][0], (W, H)) for i in faces]
        pre2 = list(pool.map(lambda k: po.image_to_tensor(imgs[faces[k]], rois[k], (192, 192), False, (0., 1.), False), range(len(faces))))
        raw, flag = fl.run(np.stack([t for t, _ in pre2]), nthreads=threads)
        ok = [k for k in range(len(faces)) if po.lib().orc_face_flag_passes(float(flag[k].reshape(-1)[-1]))]
        lms = {k: po.project_landmarks(raw[k], (192, 192), (W, H), pre2[k][1], rois[k], False) for k in ok}
        eyes = []
        for k in ok:
            left, right = po.iris_rois_from_face_landmarks(lms[k], (W, H))
            eyes += [(k, left, False), (k, right, True)]
        if eyes:
            pre3 = list(pool.map(lambda e: po.image_to_tensor(imgs[faces[e[0]]], e[1], (64, 64), True, (0., 1.), e[2]), eyes))
            c, i5 = ir.run(np.stack([t for t, _ in pre3]), nthreads=threads)
            for j, (k, r, flip) in enumerate(eyes):
                po.project_landmarks(c[j], (64, 64), (W, H), pre3[j][1], r, flip)
                po.project_landmarks(i5[j], (64, 64), (W, H), pre3[j][1], r, flip)
        return len(ok)

    n = min(len(frames_u8), max(threads, 64))
    one_pass(frames_u8[: min(n, threads)])
    t0 = time.time()
    frames = present = 0
    while time.time() - t0 < 10.0:
        present = one_pass(frames_u8[:n])
        frames += n
    dt = time.time() - t0
    pool.shutdown()
    return {"value": round(frames / dt, 1), "unit": "frames/s", "cores": threads, "host_cpus": os.cpu_count(), "kind": "port",
            "sample": "%d frames of the same batch (%d of each %d carry a face through all three nets), C oracle staged over the batch, "
                      "nets OpenMP over frames, glue on a %d-thread pool, %.1f s" % (frames, present, n, threads, dt),
            "threads_note": CPU_THREADS_NOTE}


# ------------------------------------------------------------------------------------------------- roofline helpers
def kernel_source_hash():
    """Hash of the kernel + planner sources: stamps profiles/pmc_summary.json so a stale PMC figure is never reported."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
    host_only = ("capi.cpp", "jpeg.cpp", "tflite_graph.cpp", "host_glue.cpp")  # no launch depends on them: editing them does not stale a PMC figure
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".cpp", ".hpp")) and name not in host_only:
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def is_valu_kernel(label):
    """The strip / stem kernels do their contractions with packed VALU FMAs (v_pk_fma_f32), the others on MFMA; both have the
    same dense f32 peak on gfx950."""
    return label.startswith(("strip_", "stem_conv")) and not label.startswith("strip_pipe2m")


def pipe_of(label):
    if label.startswith("strip_pipe2m"):
        return "mfma f32 4x4x1 (1x1 convs) + valu v_pk_fma_f32 (depthwise)"
    return "valu v_pk_fma_f32" if is_valu_kernel(label) else "mfma f32"


def roofline_of(records, workload_tag):
    """records: list of per-launch dicts {"kernel","ms","bytes","macs"} (HIP-event timed, grouped by kernel symbol as rocprofv3 --stats does)."""
    by = {}
    for r in records:
        k = by.setdefault(r["kernel"], {"ms": 0.0, "bytes": 0.0, "macs": 0.0, "calls": 0})
        k["ms"] += r["ms"]; k["bytes"] += r["bytes"]; k["macs"] += r["macs"]; k["calls"] += 1
    dom = max(by, key=lambda k: by[k]["ms"])
    d = by[dom]
    gbps = d["bytes"] / (d["ms"] * 1e-3) / 1e9
    tflops = 2 * d["macs"] / (d["ms"] * 1e-3) / 1e12
    hbm_frac, flop_frac = gbps / HBM_PEAK_GBS, tflops / F32_PEAK_TFLOPS
    traffic, note = None, "no PMC summary for this workload"
    tpath = os.environ.get("MI_PMC_SUMMARY") or os.path.join(ROOT, "profiles", "pmc_summary.json")
    if os.path.exists(tpath):
        try:
            for pm in json.load(open(tpath)).get("entries", []):
                if pm.get("workload") == workload_tag and pm.get("kernel") == dom:
                    if pm.get("source_hash") == kernel_source_hash():
                        traffic, note = pm.get("hbm_bytes_per_launch"), "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), profiles/pmc_summary.json, same kernel sources"
                    else:
                        note = "profiles/pmc_summary.json was measured on other kernel sources: not reported"
        except Exception:  # noqa: BLE001
            pass
    rocprof_ns = rocprof_steady_ns = rocprof2_ns = None
    if os.path.exists(tpath):
        try:
            for pm in json.load(open(tpath)).get("entries", []):
                if pm.get("workload") == workload_tag and pm.get("kernel") == dom and pm.get("source_hash") == kernel_source_hash():
                    rocprof_ns = pm.get("rocprof_avg_ns")
                    rocprof_steady_ns = pm.get("rocprof_steady_ns")
                    rocprof2_ns = pm.get("rocprof_in_flight2_avg_ns")
        except Exception:  # noqa: BLE001
            pass
    common = {"kernel": dom, "launches_per_step": d["calls"], "avg_launch_ms": round(d["ms"] / d["calls"], 5),
              "algorithmic_bytes_per_launch": round(d["bytes"] / d["calls"]), "algorithmic_flops_per_launch": round(2 * d["macs"] / d["calls"]),
              "hbm_GBps": round(gbps, 1), "hbm_frac": round(hbm_frac, 4), "f32_TFLOPs": round(tflops, 2), "f32_frac": round(flop_frac, 4),
              "traffic_note": note}
    if hbm_frac >= flop_frac:
        roof = {"bound": "hbm", "achieved": round(gbps, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(hbm_frac, 4), "traffic": traffic}
    else:   # FLOP-bound launch: the dense f32 rate; "pipe" says whether the kernel reaches it on MFMA or with packed VALU FMAs
        pipe = pipe_of(dom)
        roof = {"bound": "f32", "pipe": pipe, "achieved": round(tflops, 2),
                "peak": F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(flop_frac, 4), "traffic": traffic,
                "measured_ceiling": MEASURED_CEILING_TFLOPS[pipe], "frac_of_measured_ceiling": round(tflops / MEASURED_CEILING_TFLOPS[pipe], 4)}
    roof.update(common)
    if rocprof_ns:  # the same symbol's average duration in `rocprofv3 --kernel-trace --stats` of this workload (profiles/<round>_kernel_stats_config*.csv)
        work = 2 * d["macs"] / d["calls"] if roof["bound"] == "f32" else d["bytes"] / d["calls"]
        peak = F32_PEAK_TFLOPS * 1e12 if roof["bound"] == "f32" else HBM_PEAK_GBS * 1e9
        roof["rocprof"] = {"avg_launch_ms": round(rocprof_ns / 1e6, 5), "frac": round(work / (rocprof_ns * 1e-9) / peak, 4),
                           "note": "avg = TotalDurationNs / Calls of profiles/<round>_kernel_stats_config*.csv (the trace run is 10 warm-up + 100 timed steps, so the "
                                   "ramp-up dispatches weigh < 2 %); steady = per launch of a step the median over its dispatches without the first two "
                                   "(profiles/<round>_kernel_steady_config*.csv).  rocprofv3 durations are not additive over a step (consecutive kernels' "
                                   "intervals overlap) and tracing slows the step by 1-3 % (DESIGN.md section 5)"}
        if rocprof_steady_ns:
            roof["rocprof"]["steady_launch_ms"] = round(rocprof_steady_ns / 1e6, 5)
            roof["rocprof"]["steady_frac"] = round(work / (rocprof_steady_ns * 1e-9) / peak, 4)
        if rocprof2_ns:   # the same symbol in a kernel trace of the TIMED mode (two batches in flight, whole-frame bands; VERDICT r5 missing #3)
            roof["rocprof_in_flight"] = {"batches_in_flight": 2, "avg_launch_ms": round(rocprof2_ns / 1e6, 5), "frac": round(work / (rocprof2_ns * 1e-9) / peak, 4),
                                         "note": "profiles/<round>_kernel_stats_config*_in_flight2.csv: rocprofv3 --kernel-trace --stats of bench.py --in-flight 2 (the default); with another "
                                                 "batch's kernels on the chip a launch's [start, end] interval holds time it spent sharing CUs, so this duration is longer than the kernel "
                                                 "running alone"}
    # one record per (kernel, shape): a symbol that runs on two shapes (the 128^2 and 64^2 pipelines) is not averaged here
    shapes = {}
    for r in records:
        k = shapes.setdefault((r["kernel"], r.get("shape", "")), {"ms": 0.0, "bytes": 0.0, "macs": 0.0, "calls": 0})
        k["ms"] += r["ms"]; k["bytes"] += r["bytes"]; k["macs"] += r["macs"]; k["calls"] += 1
    roof["by_shape"] = [{"kernel": k[0], "shape": k[1], "calls": v["calls"], "avg_launch_ms": round(v["ms"] / v["calls"], 5),
                         "TFLOPs": round(2 * v["macs"] / max(v["ms"], 1e-9) / 1e9, 2), "f32_frac": round(2 * v["macs"] / max(v["ms"], 1e-9) / 1e9 / F32_PEAK_TFLOPS, 4),
                         "GBps": round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1), "hbm_frac": round(v["bytes"] / max(v["ms"], 1e-9) / 1e6 / HBM_PEAK_GBS, 4)}
                        for k, v in sorted(shapes.items(), key=lambda kv: -kv[1]["ms"])]
    roof["step_algorithmic"] = {"flops": round(2 * sum(r["macs"] for r in records)), "bytes": round(sum(r["bytes"] for r in records))}
    roof["net_event_ms"] = round(sum(r["ms"] for r in records), 4)
    roof["kernels"] = {k: {"ms": round(v["ms"], 4), "calls": v["calls"], "GBps": round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1),
                           "TFLOPs": round(2 * v["macs"] / max(v["ms"], 1e-9) / 1e9, 2)} for k, v in by.items()}
    return roof


# ------------------------------------------------------------------------------------------------- one rank
MIN_TIMED_S = 0.5
MODEL_FILES = {1: ["face_detection_short_range.tflite"], 2: ["face_detection_back.tflite"], 3: ["face_landmark.tflite"],
               5: ["face_detection_full_range.tflite", "face_landmark.tflite", "iris_landmark.tflite"]}
DEFAULT_BATCH = {1: 256, 2: 256, 3: 512, 5: 128}


def rehearse(args, rank, world):
    """CPU rehearsal of the N > 1 plumbing (gloo): rendezvous, model broadcast, host-side lowering of the received bytes,
    sharding, barrier + max-over-ranks timing, one JSON line from rank 0 — no kernels, `value` null."""
    import torch
    import torch.distributed as dist
    from importlib import import_module
    import rs_face_detection_tflite_amd as mi
    mdist = import_module("rs_face_detection_tflite_amd.dist")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cpu")
    plans = []
    for f in MODEL_FILES[args.config]:
        blob = mdist.broadcast_model_bytes(os.path.join(ROOT, "models", f) if rank == 0 else "/nonexistent", dist, dev)
        plans.append(hashlib.md5(mi.plan_describe(blob, 5).encode()).hexdigest())
    B = args.batch or DEFAULT_BATCH[args.config]
    lo, hi = mdist.shard_range(world * B, world, rank)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001 * (rank + 1))
    dist.barrier()
    elapsed = mdist.max_over_ranks(time.perf_counter() - t0, dist, dev)
    local_rank = int(os.environ.get("LOCAL_RANK", "-1"))
    shards = [None] * world
    dist.all_gather_object(shards, (lo, hi, plans, rank, local_rank))
    gathered = None
    if args.gather:  # optional result collection of SURVEY.md 8e: every rank's per-frame counts on every rank (all_gather of fixed-size records)
        mine = torch.arange(lo, hi, dtype=torch.int32)  # stand-in for the shard's detection counts: its global frame numbers
        parts = mdist.gather_counts(mine, dist, dev)
        gathered = bool(torch.equal(torch.cat(parts), torch.arange(0, world * B, dtype=torch.int32)))
    if rank == 0:
        print(json.dumps({"metric": "rehearsal (gloo, CPU, no kernels)", "value": None, "unit": "faces/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
                          "rehearsal": True, "config": {"workload": "config %d" % args.config, "global_batch": world * B,
                                                        "shards": [s[:2] for s in shards], "plans_identical": all(s[2] == plans for s in shards),
                                                        # the device a rank binds on a GPU node is cuda:LOCAL_RANK (run_rank): one distinct device per rank
                                                        "rank_to_device": ["rank %d -> cuda:%d" % (s[3], s[4]) for s in shards],
                                                        "gathered_counts_in_rank_order": gathered}}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def dump_outputs(outdir, outputs):
    """What the timed path handed its caller in the last timed step, as float32 .npy files under `outdir`: the detection rows
    past a frame's count (slots the device path leaves untouched, mi_face.h) are written as zeros."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    arrays = {name: t.detach().cpu().numpy() for name, t in outputs.items()}
    if "detections" in arrays:
        det, cnt = arrays["detections"], arrays["counts"]
        det[np.arange(det.shape[1])[None, :] >= cnt[:, None]] = 0.0
    for name, a in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), a.astype(np.float32))


def run_rank(args):
    import numpy as np
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.rehearse:
        return rehearse(args, rank, world)
    if torch.cuda.device_count() < world:     # every rank checks for itself, before anything touches a device
        sys.stderr.write("bench.py: --gpus %d but only %d GPU(s) visible; refusing to run a smaller job under that label\n" % (world, torch.cuda.device_count()))
        raise SystemExit(2)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    import ctypes as C
    from importlib import import_module
    import rs_face_detection_tflite_amd as mi
    mdist = import_module("rs_face_detection_tflite_amd.dist")

    # ---- weights: rank 0 reads the frozen .tflite files, every other rank receives them over RCCL/xGMI (one-time, timed apart)
    torch.cuda.synchronize()
    t0 = time.time()
    blobs = [mdist.broadcast_model_bytes(os.path.join(ROOT, "models", f) if rank == 0 else "/nonexistent", dist, device) for f in MODEL_FILES[args.config]]
    torch.cuda.synchronize()
    bcast_ms = (time.time() - t0) * 1e3 if world > 1 else 0.0

    B = args.batch or DEFAULT_BATCH[args.config]
    L = mi.lib()
    x_host = None
    NW = max(1, min(int(args.in_flight), 4))   # batches in flight: consecutive steps alternate between NW handles on NW streams

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.mi_last_error().decode())

    # One WORKER = one handle (its own arena and replay graphs) + its own result buffers; every worker reads the same resident input.
    # A step is one pass of the hot path over one batch through ONE worker, straight through the C ABI, asynchronous on the stream it is given.
    workers = []
    if args.config in (1, 2):
        size = 256 if args.config == 2 else 128
        kind = mi.FaceDetectionModel.BackCamera if args.config == 2 else mi.FaceDetectionModel.Short
        tag = ("back256_b%d" if args.config == 2 else "short128_b%d") % B
        cap = 16
        x_host = make_frames(B, seed=rank, size=size)
        x = torch.from_numpy(x_host).to(device)
        xp = C.c_void_p(x.data_ptr())
        for k in range(NW):
            fd = mi.FaceDetection(kind, device=local_rank, model_bytes=blobs[0])
            for key in ("fuse", "chunk", "lanes", "heads"):
                if getattr(args, key) is not None:
                    fd.model.set_option(key, getattr(args, key))
            if NW > 1:
                # with another batch in flight the row pipelines take whole frames as bands: fewer fill steps, and the CUs a short grid leaves idle
                # are the other batch's (profiles/r05_in_flight.txt: 1.221 -> 1.194 ms; with ONE batch in flight the automatic choice is better)
                fd.model.set_option("pipe_band", 4096)
            for kv in args.opt:
                kk, v = kv.split("=")
                fd.model.set_option(kk, int(v))
            out = torch.zeros((B, cap, 17), dtype=torch.float32, device=device)
            cnt = torch.zeros((B,), dtype=torch.int32, device=device)
            def step_k(spp, h=fd.h, op=C.c_void_p(out.data_ptr()), cp=C.c_void_p(cnt.data_ptr())):
                check(L.mi_fd_infer_tensor(h, xp, B, None, op, cap, cp, mi.MI_MEM_DEVICE, spp))
            workers.append(dict(step=step_k, keep=(fd, out, cnt), counts=cnt, found=lambda cnt=cnt: int((cnt > 0).sum().item()),
                                outputs=dict(detections=out, counts=cnt)))
        fd = workers[0]["keep"][0]
        counts = workers[0]["counts"]
        if args.config == 2:
            metric, unit = "faces/sec at batch=256 (256x256 back-camera) per GPU", "faces/s"
            workload = ("BackCamera BlazeFace 256x256, batch=%d frames/GPU, net + SSD decode + sigmoid + weighted NMS (configs[1]%s); "
                        "50%% noise / 50%% face-bearing frames, inputs resident in HBM" % (B, ", sharded as configs[3]" if world > 1 else ""))
        else:
            metric, unit = "faces/sec at batch=256 (128x128 short-range / front-camera) per GPU", "faces/s"
            workload = ("ShortRange (= FrontCamera bytes) BlazeFace 128x128, batch=%d frames/GPU, net + SSD decode + sigmoid + weighted NMS "
                        "(configs[0]'s model on north_star's 128x128 batch); 50%% noise / 50%% face-bearing frames, inputs resident in HBM" % B)
        models = [(fd.model, x)]
    elif args.config == 3:
        tag = "landmark192_b%d" % B
        x = torch.from_numpy(make_rois(B, seed=rank)).to(device)
        xp = C.c_void_p(x.data_ptr())
        for k in range(NW):
            fl = mi.FaceLandmark(device=local_rank, model_bytes=blobs[0])
            for kv in args.opt:
                kk, v = kv.split("=")
                fl.model.set_option(kk, int(v))
            lm = torch.zeros((B, 468, 3), dtype=torch.float32, device=device)
            present = torch.zeros((B,), dtype=torch.int32, device=device)
            flags = torch.zeros((B,), dtype=torch.float32, device=device)
            def step_k(spp, h=fl.h, a=C.c_void_p(lm.data_ptr()), b=C.c_void_p(present.data_ptr()), c=C.c_void_p(flags.data_ptr())):
                check(L.mi_fl_infer_tensor(h, xp, B, None, None, a, b, c, mi.MI_MEM_DEVICE, spp))
            workers.append(dict(step=step_k, keep=(fl, lm, present, flags), found=lambda present=present: int(present.sum().item()),
                                outputs=dict(landmarks=lm, present=present, flags=flags)))
        metric, unit = "ROIs/sec, FaceLandmark 192x192 at batch=512 per GPU (configs[2])", "ROIs/s"
        workload = "FaceLandmark 192x192, batch=%d ROIs/GPU, net + face flag + landmark projection (configs[2]); 50%% noise / 50%% face crops, inputs resident in HBM" % B
        models = [(workers[0]["keep"][0].model, x)]
    else:
        tag = "pipeline192_b%d" % B
        frames = torch.from_numpy(make_rgb_frames(B, seed=rank)).to(device)
        fp = C.c_void_p(frames.data_ptr())
        for k in range(NW):
            pipe = mi.Pipeline(mi.FaceDetectionModel.Full, device=local_rank, model_bytes=blobs)
            for kv in args.opt:
                kk, v = kv.split("=")
                for m in pipe.models:
                    m.set_option(kk, int(v))
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
            o = dict(faces=z((B, 17), torch.float32), face_counts=z((B,), torch.int32), landmarks=z((B, 468, 3), torch.float32),
                     present=z((B,), torch.int32), eyes=z((B, 2, 76, 3), torch.float32))
            ptrs = [C.c_void_p(o[n].data_ptr()) for n in ("faces", "face_counts", "landmarks", "present", "eyes")]
            def step_k(spp, h=pipe.h, ptrs=ptrs):
                check(L.mi_pipeline_run(h, fp, B, 192, 192, 3 * 192, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], mi.MI_MEM_DEVICE, spp))
            workers.append(dict(step=step_k, keep=(pipe, o), found=lambda o=o: int(o["present"].sum().item()), outputs=o))
        pipe = workers[0]["keep"][0]
        metric, unit = "frames/sec, full_range detection -> face_landmark -> 2 x iris_landmark at 128 frames per GPU (configs[4])", "frames/s"
        workload = ("full_range 192x192 -> faces[0] ROI -> face_landmark 192x192 -> eye ROIs -> 2 x iris_landmark 64x64, batch=%d RGB frames/GPU, "
                    "every stage on the device (configs[4]); 50%% noise / 50%% face-bearing frames, frames resident in HBM" % B)
        g = torch.Generator(device="cpu").manual_seed(rank)
        models = [(pipe.models[0], torch.rand((B, 192, 192, 3), generator=g).mul(2).sub(1).to(device)),
                  (pipe.models[1], torch.rand((B, 192, 192, 3), generator=g).to(device)),
                  (pipe.models[2], torch.rand((2 * B, 64, 64, 3), generator=g).to(device))]
    found = workers[0]["found"]

    def close_workers():
        for w in workers:
            w["keep"][0].close()

    # ---- the streams.  HIP streams share the device's hardware queues (GPU_MAX_HW_QUEUES = 4), handed out as streams are first used, and the
    # handles own side streams of their own: two streams that land on ONE hardware queue run strictly one after the other (what round 4's
    # two-stream probe measured without knowing it).  So the pair of streams is CHOSEN: a few steps are timed on (stream 0, stream j) for a
    # handful of candidates, outside the timed region, and the fastest pair is kept (`timing.stream_pair_probe_ms`).
    cand = [torch.cuda.Stream(device=device) for _ in range(4 + NW if NW > 1 else 1)]
    spp = [C.c_void_p(cand[0].cuda_stream) for _ in range(NW)]
    state = {"i": 0}

    def step():
        i = state["i"]
        state["i"] = i + 1
        workers[i % NW]["step"](spp[i % NW])

    def time_steps(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    pair_probe = {}
    if NW > 1:
        for _ in range(2 * NW):
            step()
        used = {0}
        for k in range(1, NW):   # worker k's stream: the candidate that gives the shortest step beside the streams chosen so far
            probe = {}
            for j in range(1, len(cand)):
                if j in used:
                    continue
                spp[k] = C.c_void_p(cand[j].cuda_stream)
                time_steps(2 * NW)
                probe[j] = round(time_steps(6 * NW), 4)
            best = min(probe, key=probe.get)
            spp[k] = C.c_void_p(cand[best].cuda_stream)
            used.add(best)
            pair_probe["worker %d" % k] = probe
        state["i"] = 0

    # ---- per-launch HIP-event pass for the roofline object (eager replays of the same plans on resident inputs of the same shapes, grouped
    # by kernel symbol like rocprofv3 --stats does), every rank alike.  The W warm-up steps and the K timed steps follow it directly.
    # (two passes: this one, whose figures are discarded — the chip comes out of the host-side set-up idle and its clocks are still ramping —
    # and the recorded one behind the timed windows, on a chip in the state the windows were measured in)
    event_profile = args.full and not (args.no_event_profile and world == 1)
    if event_profile:
        for m, xin in models:
            m.profile(xin, reps=3)
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed = mdist.max_over_ranks(elapsed, dist, device)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, workers[(state["i"] - 1) % NW]["outputs"])
    n_found = found()
    # ---- the same K-step window again until >= MIN_TIMED_S of device time has been sampled (the first window above stays the
    # reported one: `ms_per_step` and `value`); median / min over all windows go into extra keys.  The number of windows is
    # decided from rank 0's clock and shared, so every rank runs the same count.
    windows = [elapsed]
    n_extra = max(4, int(MIN_TIMED_S / max(elapsed, 1e-6)) + 1) if args.full and not args.single_window else 0
    n_extra = int(mdist.max_over_ranks(float(min(n_extra, 2000)), dist, device))
    for _ in range(n_extra):
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        windows.append(time.perf_counter() - t0)
    if dist and n_extra:
        windows = [mdist.max_over_ranks(w, dist, device) for w in windows[:1]] + \
                  [float(v) for v in mdist.max_over_ranks_vec(windows[1:], dist, device)]

    # the same K steps with ONE batch in flight (one handle, one stream), for comparison (extra key, never `value`)
    one_in_flight_ms = None
    if args.full and NW > 1:
        if args.config in (1, 2):
            # ... with the band sizes that are best for one batch in flight (the automatic ones); the recorded per-launch pass for `roofline`
            # below runs on this handle too: it describes every kernel running alone, like the rocprofv3 passes (--in-flight 1)
            workers[0]["keep"][0].model.set_option("pipe_band", 0)
            for _ in range(3):
                workers[0]["step"](spp[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            workers[0]["step"](spp[0])
        torch.cuda.synchronize()
        one_in_flight_ms = (time.perf_counter() - t0) / args.steps * 1e3
    gathered = None
    if args.gather and args.config in (1, 2):  # optional result collection, outside the timed window
        parts = mdist.gather_counts(counts, dist, device)
        gathered = [int((p > 0).sum().item()) for p in parts]
    if rank == 0:
        recs = []
        if event_profile:
            for m, xin in models:
                # per launch: the median of three passes of five executions each (one pass read a single launch 30 % long once in a while — a
                # neighbouring process's burst on the box — and the dominant symbol's figure with it; the rocprofv3 average beside it did not move)
                passes = [m.profile(xin, reps=5) for _ in range(3)]
                for i, r in enumerate(passes[0]):
                    if all(len(p) == len(passes[0]) and p[i]["kernel"] == r["kernel"] for p in passes):
                        r["ms"] = sorted(p[i]["ms"] for p in passes)[1]
                recs += passes[0]
        value = world * B * args.steps / elapsed
        result = {
            "metric": metric, "value": round(value, 1), "unit": unit,
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": bool(args.full),
            # the in-flight setting beside the headline, and the one-handle figure (the measurement of rounds 1 - 4, and what `roofline`
            # and every profile under profiles/ describe) as a first-class field — round-over-round comparisons are like for like
            "batches_in_flight": NW,
            "value_one_batch_in_flight": round(world * B / (one_in_flight_ms * 1e-3), 1) if one_in_flight_ms else (round(value, 1) if NW == 1 else None),
            "ms_per_step_one_batch_in_flight": round(one_in_flight_ms, 4) if one_in_flight_ms else (round(elapsed / args.steps * 1e3, 4) if NW == 1 else None),
            "timing": {"windows": len(windows), "steps_per_window": args.steps, "timed_s": round(sum(windows), 4),
                       "ms_per_step_median": round(sorted(windows)[len(windows) // 2] / args.steps * 1e3, 4),
                       "ms_per_step_min": round(min(windows) / args.steps * 1e3, 4),
                       "ms_per_step_max": round(max(windows) / args.steps * 1e3, 4),
                       "batches_in_flight": NW,
                       "ms_per_step_one_batch_in_flight": round(one_in_flight_ms, 4) if one_in_flight_ms else None,
                       "stream_pair_probe_ms": pair_probe or None,
                       "in_flight_note": ("consecutive steps alternate between %d handles (each with its own arena, replay graphs and result buffers) on %d streams, so the "
                                          "tail of batch n runs beside the head of batch n + 1; every step is still one full pass over one batch and the K steps are "
                                          "bracketed by synchronisation as before.  The second stream is chosen from %d candidates by timing a few steps (streams "
                                          "that share a hardware queue run one after the other); with two in flight the row pipelines take whole frames as bands "
                                          "(option pipe_band); ms_per_step_one_batch_in_flight and `roofline` are taken afterwards on one handle with the automatic "
                                          "band sizes (every kernel running alone); --in-flight 1 gives the one-handle figure" % (NW, NW, len(cand) - 1)) if NW > 1 else None,
                       "note": "ms_per_step / value = the first window (the driver's K steps, directly behind the W warm-up steps); the others repeat it. "
                               "Before the warm-up steps a per-launch HIP-event pass over the plan runs once (figures discarded; the recorded pass "
                               "for `roofline` runs behind the windows)" if event_profile else
                               "ms_per_step / value = the K timed steps, directly behind the W warm-up steps, timed once (--full repeats the window "
                               "and adds the per-launch event passes)"},
            "config": {"workload": workload, "global_batch": world * B, "batches_in_flight": NW, "frames_with_faces": n_found,
                       "parallelism": "frames sharded %d/GPU, one process per GPU, no data-path collective" % B,
                       "weight_broadcast_ms": round(bcast_ms, 3), "weight_broadcast_bytes": sum(len(b) for b in blobs),
                       "frames_with_faces_per_rank": gathered,
                       "plan": " | ".join(m.describe().splitlines()[0] for m, _ in models)},
            "roofline": roofline_of(recs, tag) if recs else None,
        }
        if not recs:  # a plain run, or --no-event-profile (rocprofv3 kernel-trace runs: the dispatch sequence stays one step after the other)
            print(json.dumps(result), flush=True)
            close_workers()
            if dist:
                dist.barrier()
                dist.destroy_process_group()
            return
        # the whole step against the same roofs (algorithmic FLOPs / bytes of all launches over ms_per_step)
        sa = result["roofline"].pop("step_algorithmic")
        ms_step = elapsed / args.steps * 1e3
        result["roofline"]["whole_step"] = {"algorithmic_flops": sa["flops"], "algorithmic_bytes": sa["bytes"],
                                            "f32_frac": round(sa["flops"] / (ms_step * 1e-3) / 1e12 / F32_PEAK_TFLOPS, 4),
                                            "hbm_frac": round(sa["bytes"] / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        if world == 1 and args.config == 2 and not args.no_host_feed:
            # the same workload fed from HOST memory as u8 frames (what the reference's callers hold), outside the timed window and never
            # `value`: two-slot feed, the copy of batch n + 1 on its own stream while batch n runs (mi_fd_submit_images / mi_fd_collect)
            try:
                u8 = np.clip((x_host + 1.0) * 127.5, 0, 255).astype(np.uint8)
                pins = [mi.PinnedBuffer(u8.shape) for _ in range(2)]
                for pb in pins:
                    pb.array[...] = u8
                nbatches = 40
                fd.submit_images(0, pins[0].array, cap=cap)
                t0 = time.perf_counter()
                for bi in range(1, nbatches + 1):
                    fd.submit_images(bi & 1, pins[bi & 1].array, cap=cap)
                    _, hc = fd.collect((bi - 1) & 1)
                dt = (time.perf_counter() - t0) / nbatches
                fd.collect(nbatches & 1)
                result["host_feed"] = {"frames_per_s": round(B / dt, 1), "ms_per_batch": round(dt * 1e3, 4), "input": "u8 RGB frames in pinned host memory, %d B per frame" % (u8.nbytes // B),
                                       "h2d_bytes_per_batch": int(u8.nbytes), "frames_with_faces": int((hc > 0).sum()),
                                       "note": "mi_fd_submit_images / mi_fd_collect, two slots; includes H2D copy, device image_to_tensor (u8 stem), net, post-processing, results to host"}
                for pb in pins:
                    pb.close()
            except Exception as e:  # noqa: BLE001
                result["host_feed"] = {"error": str(e)}
        if getattr(args, "secondary_results", None) is not None:
            # configs 1 / 3 / 5, run as child processes by main() BEFORE this process imported torch or made a HIP call (VERDICT r4 item 7a:
            # a process that has initialised the GPU starts no other program); a failed child is an explicit error record AND raises the
            # top-level flag, so a line that lost its 128x128 / 192x192 figures cannot be mistaken for a complete one
            result["secondary_configs"] = args.secondary_results
            result["secondary_errors"] = sum(1 for v in args.secondary_results.values() if "error" in v)
        if world == 1 and not args.no_latency:
            # the reference's own operating point: ONE image per call through the three `infer`s (face_detection.rs:205-267,
            # face_landmark.rs:232-306, iris_landmark.rs:158-248), host Mat in, results out — outside the timed window
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            try:
                import latency_probe
                result["single_image_latency_us"] = latency_probe.measure(n=args.latency_calls)
                # the same calls timed at the C ABI (arguments marshalled once): what a Rust / C++ host sees, without the Python wrapper
                result["single_image_latency_us_c_abi"] = latency_probe.measure_c_abi(n=args.latency_calls)
            except Exception as e:  # noqa: BLE001
                result["single_image_latency_us"] = {"error": str(e)}
        if not args.no_cpu_baseline and world == 1 and args.config in (1, 2):  # CPU baseline: rank 0 at N = 1 only
            threads = max(1, min(usable_cpus(), B))
            mf, kd = MODEL_FILES[args.config][0], ("FD_BACK" if args.config == 2 else "FD_SHORT")
            result["cpu_baseline"] = cpu_baseline(x_host, threads, mf, kd)
            result["cpu_baseline_1thread"] = cpu_baseline_1thread(x_host, mf, kd)
        elif not args.no_cpu_baseline and world == 1 and args.config == 3:
            result["cpu_baseline"] = cpu_baseline_landmark(x.cpu().numpy(), max(1, min(usable_cpus(), B)))
        elif not args.no_cpu_baseline and world == 1:
            result["cpu_baseline"] = cpu_baseline_pipeline(frames.cpu().numpy(), max(1, min(usable_cpus(), B)))
    close_workers()
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result), flush=True)


def run_secondary_configs(args):
    """north_star's other batch shapes (128x128 short-range detector, 192x192 face mesh, 192x192 device pipeline) measured by the SAME
    invocation, each in a child process with the same K / W, so that the driver's run carries them too (BASELINE configs[0]'s model at
    batch 256, configs[2] and the 1-GPU shard of configs[4]; parity-test cases, never `value`).  Called from main() while this process
    has not imported torch nor loaded a HIP library: the children have the GPU to themselves, one after the other, and the headline
    measurement starts on a warm chip afterwards."""
    assert "torch" not in sys.modules, "secondary configs must run before this process touches the GPU"
    out = {}
    for c in (1, 3, 5):
        key = "config %d" % c
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", str(c), "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--full", "--no-cpu-baseline", "--no-latency", "--no-secondary", "--no-host-feed"], capture_output=True, text=True, timeout=300)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                out[key] = {"error": "child exited with status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:].replace("\n", " | "))}
                continue
            dd = json.loads(lines[-1])
            rf = dd.get("roofline") or {}
            out[key] = {
                "metric": dd["metric"], "value": dd["value"], "unit": dd["unit"], "ms_per_step": dd["ms_per_step"],
                "ms_per_step_median": dd["timing"]["ms_per_step_median"], "batches_in_flight": dd.get("batches_in_flight"),
                "ms_per_step_one_batch_in_flight": dd.get("ms_per_step_one_batch_in_flight"), "value_one_batch_in_flight": dd.get("value_one_batch_in_flight"),
                "workload": dd["config"]["workload"],
                "roofline": {k: rf.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms")},
                "whole_step": rf.get("whole_step")}
        except Exception as e:  # noqa: BLE001
            out[key] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", type=int, default=2, choices=[1, 2, 3, 5],
                    help="BASELINE config: 2 = headline (4 with --gpus N), 1 = short-range / front 128x128 batch, 3 = face mesh, 5 = pipeline")
    ap.add_argument("--batch", type=int, default=None, help="units per GPU (default 256 / 256 / 512 / 128 for config 1 / 2 / 3 / 5)")
    ap.add_argument("--spawn", action="store_true", help="go through the rank launcher even for --gpus 1 (one child process)")
    ap.add_argument("--single-window", action="store_true", help="time the K steps once only (no repeated windows)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-event-profile", action="store_true", help="N = 1: skip the per-launch HIP-event pass (no roofline object); for rocprofv3 kernel-trace runs")
    ap.add_argument("--no-secondary", action="store_true", help="config 2, N = 1: skip the child runs of configs 1 / 3 / 5 (extra key secondary_configs)")
    ap.add_argument("--no-host-feed", action="store_true", help="skip the host-fed u8 variant of config 2 (N = 1, extra key, outside the timed window)")
    ap.add_argument("--no-latency", action="store_true", help="skip the single-image per-call latency block (N = 1)")
    ap.add_argument("--latency-calls", type=int, default=200)
    ap.add_argument("--gather", action="store_true", help="N > 1: collect every rank's per-frame detection counts on rank 0 (dist.gather_counts), outside the timed window")
    ap.add_argument("--rehearse", action="store_true", help="CPU rehearsal of the multi-rank plumbing over gloo (no kernels)")
    ap.add_argument("--in-flight", type=int, default=2, choices=[1, 2, 3, 4], help="batches in flight: 2 = consecutive steps alternate between two handles on two streams (default), 1 = one handle")
    ap.add_argument("--fuse", type=int, default=None)
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--lanes", type=int, default=None)
    ap.add_argument("--heads", type=int, default=None)
    ap.add_argument("--opt", action="append", default=[], help="engine option key=value (development), every model of the configuration")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: repeated windows, one batch in flight, roofline (per-launch event pass), "
                         "configs 1 / 3 / 5, host feed, single-image latency, CPU baseline (the --no-* options switch these off one by one)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step as DIR/<name>.npy (float32; rank 0's shard)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.rehearse or args.spawn):
        sys.exit(launch_ranks(args, sys.argv[1:]))
    args.secondary_results = None
    if args.full and int(os.environ.get("WORLD_SIZE", "1")) == 1 and args.config == 2 and not args.no_secondary and not args.rehearse:
        args.secondary_results = run_secondary_configs(args)
    run_rank(args)


if __name__ == "__main__":
    main()
