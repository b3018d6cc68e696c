"""GPU parity at the rounding floor: every launch of the hand-written hot path, run as a slice of its shipped graph (tests/tfl_slice.py), and every
whole network, against a float64 evaluation of the same graph on the same input (tests/slice_refs.py).

Criterion, per output tensor and checked frame (E = the larger of the C oracle's and torch's error against float64 on that input, M = 32 from the
spread of three f32 evaluations on the CPU, test_slices_cpu.py; never from a GPU run):
    max|gpu - f64| / scale <= max(M * E_max, 4 * 2^-24)      rms(gpu - f64) / scale <= max(M * E_rms, 2^-24)      scale = max(1, max|f64|)
Why M x E: the f32 MFMA on gfx950 is a k-ordered IEEE fmaf chain with no wider accumulation and no flushing, and the VALU paths are built with
-ffp-contract=off plus explicit FMAs: a correct kernel is one more valid f32 ordering, of the same class as the CPU evaluations.  RAW_TOL
(test_gpu_parity.py: 1e-4 x scale against the C oracle, at whole networks' outputs) is 70 to 3000 times the floor and stays as it is.

a. slices: every slice of the table with profile()'s labels equal to the launch list pinned for it on the CPU (tests/golden/slice_labels.json), at 3 frames
   (noise, picture, edgy: the small-batch forms) and at 33 (above every batch threshold: the three frames at 0, 16, 32, the other 30 against the C
   oracle within (M + 1) x the largest E_max of the three); slices with a tail_kernel, chain_kernel or strip_pipe* launch also with tail_pre = 2,
   chain_fixed = 0, pipe_rows = 4: another form of the kernel, the same graph, the same bound.
b. whole networks: the seven graphs at fuse 0, 2 and 5 on their three frames, at fuse 5 also the batch of 33, and band = 2 on the picture frame alone
   (the single-launch bandnet_kernel, which no slice reaches as such).

Observed on an MI355X (2026-10-21), 70 cases, none rejected; every case prints its ratios.  Worst gpu / E per launch label, (max, rms), over
outputs, frames, 3 and 33 frames and the variants, taken from the smallest slice that runs the label (its other labels in brackets share the figure):
  stem_mfma_kernel, stem_conv_kernel                           1.00  1.00   (the C oracle's bits)
  strip_pipe2m_kernel<6,4,1,0> [strip_kernel<6,1> x4 (small batch)], strip_pipe1m with pipe_rows = 4    4.09  2.20   back:69-101, the edgy frame
  strip_pipe2m_kernel<6,4,1,1>                                 2.06  1.80
  strip_pipe2m_kernel<6,4,1,2> [strip_kernel<6,1> x3 + block_kernel (small batch)]                      4.75  2.69   back:101-136, the noise frame
  strip_kernel<6,1>                                            1.25  1.44
  mstrip_chain_kernel<12,1> [mstrip_kernel<12,1>, block_kernel<1,1,3,1,0> x7]                           3.30  2.36
  chain_kernel<3> (with its views; chain_fixed = 0 alike)      2.13  1.10
  mdblock_kernel<stem+pair> [ms2_kernel<4,2,3>, strip_kernel<4,0> x2 (small batch)]                     2.28  1.83
  mdblock_kernel<pair> [ms2_kernel<8,4,2>, strip_kernel<8,0>]  2.66  2.04
  ms2_kernel<4,2,3>  1.77  1.95      ms2_kernel<8,4,2>  2.56  2.18      ms2_kernel<8,1,3> [block_kernel<2,1,3,1,1>]  1.37  1.28
  block_kernel<2,1,3,1,0>  1.24  1.11      block_kernel<1,2,3,1,0>  1.22  1.07      block_kernel<2,1,3,2,0> / <1,1,3,1,0>  1.66  1.00
  tail_kernel [head_gemm_kernel, head_dot_kernel] (tail_pre = 2 alike)                                  1.51  1.39
  mbneck_kernel [bneck_kernel at 3 frames]  2.36  2.14      bneck_kernel  1.14  0.99      resident_kernel  1.34  1.07
  mdblock_kernel [dblock_kernel at 3 frames]  1.87  1.73      dblock_kernel  1.20  1.08
  pw_few_kernel, block_kernel<1,1,1,1,0>  1.37  1.19      dw_kernel, d2s_kernel, block_kernel<2,1,1,1,0>  2.17  1.24
  the detectors' remainder front / short:12-out (block_kernel<1,1,3,2,0>, <2,2,3,1,0>, mstrip_chain, chain x2)   1.91  1.67
  the pyramids full:84-342 (xc_kernel, resident_kernel, ms2_kernel<16,2,2>, block_kernel<3,1,3,1,1>, ...: 14 labels)  0.97  0.81
                sparse:131-523 (xc_kernel, resident_kernel, block_kernel<4,1,3,1,0>, ...: 13 labels)               3.52  2.22
  whole networks, fuse 0 / 2 / 5, 3 and 33 frames: 1.5 .. 2.6 (max), 1.5 .. 1.9 (rms); band = 2 (bandnet_kernel): 0.1 .. 2.1
  the 30 unchecked frames of each batch of 33 against the C oracle: at most 0.16 of (M + 1) x E_max, but for the whole back network's scores, 0.64:
  5.3e-6 x scale at one noise frame (frame 18 of the batch) on which the C oracle and torch are themselves 3.0e-6 from float64, twelve times their
  error on the three checked frames (evaluated on the CPU afterwards): the frame's own floor, not the kernels'
The bound is M = 32 x E: the largest ratio, 4.75, is 0.15 of it.  The row pipelines and mstrip run about twice E in rms on every frame: their depthwise
stage and pointwise contraction round in another order than the three CPU evaluations, at 3e-7 .. 7e-7 x scale absolute, inside the range of E over
the table (1.2e-7 .. 8.1e-7 for back).  No launch label has a bound of its own.
"""
import json
import os

import numpy as np
import pytest

import slice_refs
import tfl_slice
from conftest import MODEL_FILES, ROOT

pytestmark = pytest.mark.gpu

# a setting that changes the kernel's form but not the graph, per kind of launch
VARIANTS = (("tail_kernel", "tail_pre", 2), ("chain_kernel", "chain_fixed", 0), ("strip_pipe", "pipe_rows", 4))


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """name -> {id: Case}: the graph's slices and itself with their frames, float64, C and torch evaluations, computed once."""
    d = tmp_path_factory.mktemp("slices")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = slice_refs.build_cases(name, d, extra=30)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def pins():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "slice_labels.json")))


def _labels(m, x):
    import torch
    return [r["kernel"] for r in m.profile(torch.from_numpy(np.ascontiguousarray(x)).cuda(), reps=1)]


def _check3(case, m, what):
    ok, text = case.judge([o.copy() for o in m.run(case.x3)])
    print("[%s, 3 frames]\n%s" % (what, text))
    return ok


def _check33(case, m, what, batch):
    x, c33 = batch
    outs = [o.copy() for o in m.run(x)]
    ok, text = case.judge([o[list(slice_refs.CHECKED)] for o in outs])
    ok2, text2 = case.judge_rest(outs, c33)
    print("[%s, 33 frames]\n%s\n%s" % (what, text, text2))
    return ok and ok2


@pytest.mark.parametrize("sid", tfl_slice.ALL_IDS)
def test_slice_vs_float64(gpu, refs, pins, sid):
    case = refs(sid.split(":")[0])[sid]
    batch = case.batch33()
    m = gpu.Model(case.path)
    bad = []
    for frames, x in ((3, case.x3), (33, batch[0])):
        labels = _labels(m, x)
        print("labels at %d frames: %s" % (frames, labels))
        assert labels == pins[sid]["F=%d" % frames], (sid, frames)
    if not _check3(case, m, "defaults"):
        bad.append("defaults, 3 frames")
    if not _check33(case, m, "defaults", batch):
        bad.append("defaults, 33 frames")
    for kernel, option, value in VARIANTS:
        if not any(k.startswith(kernel) for f in (3, 33) for k in pins[sid]["F=%d" % f]):
            continue
        m.set_option(option, value)
        what = "%s = %d" % (option, value)
        print("labels with %s: %s / %s" % (what, _labels(m, case.x3), _labels(m, batch[0])))
        if option == "pipe_rows":   # one row per step with the MFMA pointwise convolutions
            assert any(k.startswith("strip_pipe1m_kernel<") for k in _labels(m, batch[0]))
        if not _check3(case, m, what):
            bad.append(what + ", 3 frames")
        if not _check33(case, m, what, batch):
            bad.append(what + ", 33 frames")
    m.close()
    assert not bad, (sid, bad)


@pytest.mark.parametrize("name", list(MODEL_FILES))
@pytest.mark.parametrize("fuse", [0, 2, 5])
def test_network_vs_float64(gpu, refs, name, fuse):
    case = refs(name)[name]
    m = gpu.Model(case.path)
    m.set_option("fuse", fuse)
    bad = []
    if not _check3(case, m, "fuse %d" % fuse):
        bad.append("3 frames")
    if fuse == 5:
        if not _check33(case, m, "fuse 5", case.batch33()):
            bad.append("33 frames")
        m.set_option("band", 2)
        x = case.x3[1:2]
        labels = _labels(m, x)
        print("labels with band = 2 at 1 frame:", labels)
        assert any(k.startswith("bandnet_kernel") for k in labels)
        ok, text = case.judge([o.copy() for o in m.run(x)], frames=(1,))
        print("[band = 2, the picture frame]\n" + text)
        if not ok:
            bad.append("band = 2")
    m.close()
    assert not bad, (name, fuse, bad)
