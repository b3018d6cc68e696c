"""The slices of tests/tfl_slice.py and the float64 yardstick of tests/slice_refs.py, checked on the CPU (no GPU, reference evaluations only).

a. fed one into the next through the C oracle, the slices of a chain reproduce the whole network's outputs bit for bit (seven graphs, two frames);
b. every launch label of every shipped graph's default launch list, at 1 and at 32 frames, is in the launch list of the slice the table assigns it
   to, template arguments and all (tests/launches_dump.cpp, `tensors` mode, built the way test_launch_pins.py builds it); the slices' own lists at
   1, 3, 32 and 33 frames are pinned in tests/golden/slice_labels.json, which is what test_f64_parity_gpu.py holds profile() against;
c. the yardstick and its spread: E_max and E_rms (slice_refs.py) of three valid f32 evaluations (the C oracle, torch, torch with oneDNN off) of every
   slice and every whole graph on its three frames, and the largest ratio between any two of them over all cases;
d. the criterion M x E rejects, at the slice, planted faults that RAW_TOL (test_gpu_parity.py) accepts at the network's outputs.

Measured (x86-64, torch CPU, 56 cases x 3 frames, every output tensor):
  spread, max:  10.2 (iris:149-out, the 15-value iris output: C / torch 7.8e-7, oneDNN off 7.7e-8); per graph's cases back 1.5, front / short 1.9,
                full 2.5, sparse 4.0, landmark 3.6, iris 10.2
  spread, rms:   5.9 (same case); back 1.3, front / short 1.4, full 2.0, sparse 2.0, landmark 3.6, iris 5.9
The spread on the back detector's slices alone is the 1.5 / 1.3 the yardstick was proposed with (M = 4); over the full table it is more than 2, so M
is the next power of two that is at least twice the spread: M = 32, and the test asserts spread <= M / 2 = 16.  The widest ratios are on outputs of
1 to 15 values, where the maximum of so few rounding errors is itself a noisy figure, and where torch's own contraction over the whole frame (oneDNN
off; the iris / landmark heads, K = 512 .. 1152) is several times closer to float64 than the k-ordered chain of the C oracle, whose bits torch with
oneDNN reproduces there.  M is never taken from a GPU run.
Floors (E of any of the three evaluations, over a graph's cases, relative to scale = max(1, max|f64|)):
  graph      E_max                  E_rms
  back       1.2e-7 .. 8.1e-7       4.5e-9 .. 6.0e-8
  front      1.6e-7 .. 1.4e-6       4.0e-9 .. 1.3e-7
  short      1.6e-7 .. 1.4e-6       4.0e-9 .. 1.3e-7
  full       3.6e-8 .. 9.2e-7       4.4e-9 .. 2.5e-7
  sparse     7.4e-8 .. 7.2e-7       1.7e-9 .. 4.5e-8
  landmark   3.2e-8 .. 7.3e-7       4.3e-9 .. 3.5e-7
  iris       7.7e-8 .. 8.2e-7       4.9e-9 .. 2.6e-7
RAW_TOL = 1e-4 is 70 to 3000 times these; M x E_max is 4e-6 .. 4.5e-5 at the widest and a few 1e-6 .. 1e-5 for most cases.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import slice_refs
import tfl_slice
from conftest import ROOT, model_path
from oracle.np import evaluate, tfl3

RAW_TOL = 1e-4          # tests/test_gpu_parity.py
FRAMES_PINNED = (1, 3, 32, 33)
# caps of NOT_COVERED: none for the graphs whose every label a slice reaches, two labels for the others
NOT_COVERED_CAP = {"back": 0, "landmark": 0, "iris": 0, "front": 2, "short": 2, "full": 2, "sparse": 2}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("slices")
    out = {}
    for name in tfl_slice.CHAINS:
        out.update(slice_refs.build_cases(name, d, plain=True))
    return out


def test_slicer_refuses_a_cut_that_needs_another_activation():
    g = tfl3.load(model_path("back"))
    with pytest.raises(ValueError, match="does not follow from tensor 7"):
        tfl_slice.slice_graph(g, 7, [12])       # the block's skip reads tensor 4
    with pytest.raises(ValueError):
        tfl_slice.slice_graph(tfl3.load(model_path("full")), 193, [256])   # the xc launch's skip reads tensor 186
    assert set(tfl_slice.THERE_FOR) == set(tfl_slice.ALL_IDS) and len(tfl_slice.ALL_IDS) == 49


@pytest.mark.parametrize("name", list(tfl_slice.CHAINS))
def test_slices_chain_to_the_whole_network(cases, name):
    """The chain's slices fed one into the next through the C oracle (frames 0 and 1: slice_refs.build_cases makes each slice's input that way), the
    last one's outputs against the whole network's: bit for bit."""
    chain = [sid for sid, _, _, in_chain in tfl_slice.table(name) if in_chain]
    whole, last = cases[name], cases[chain[-1]]
    for sid, nxt in zip(chain, chain[1:]):     # each slice's output is the next one's input, as the C oracle computes it
        np.testing.assert_array_equal(cases[sid].ref["c"][0][:2], cases[nxt].x3[:2])
    np.testing.assert_array_equal(cases[chain[0]].x3[:2], whole.x3[:2])
    assert len(last.ref["c"]) == len(whole.ref["c"])
    for a, b in zip(last.ref["c"], whole.ref["c"]):
        np.testing.assert_array_equal(a[:2], b[:2])


@pytest.fixture(scope="module")
def launch_labels(tmp_path_factory):
    """{parent file name or slice id: {F: [labels]}} as launches_dump's `tensors` mode prints them at the defaults."""
    tmp = tmp_path_factory.mktemp("slice_launches")
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    hipcc, csrc = "/opt/rocm/bin/hipcc", os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
    o = str(tmp / "launches_dump.o")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "launches_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    exe = str(tmp / "launches_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)
    files = {}
    for name in tfl_slice.CHAINS:
        g = tfl3.load(model_path(name))
        files[name] = model_path(name)
        for sid, tin, touts, _ in tfl_slice.table(name):
            p = tmp / (sid.replace(":", "_") + ".tflite")
            p.write_bytes(tfl_slice.slice_graph(g, tin, touts or list(g.outputs)))
            files[sid] = str(p)
    r = subprocess.run([exe, "tensors"] + list(files.values()), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    by_file, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            fname, _, f = line[3:].split(" ")
            cur = by_file.setdefault(fname, {}).setdefault(int(f[2:]), [])
        else:
            assert not line.startswith("threw"), line
            m = re.match(r'\d+ "(.*)" in=', line)
            if m:
                cur.append(m.group(1))
    return {key: by_file[os.path.basename(path)] for key, path in files.items()}


def test_every_parent_label_is_in_its_slice(launch_labels):
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "slice_labels.json")))
    assert set(pins) == set(launch_labels)
    for key, per_f in launch_labels.items():
        assert {"F=%d" % f: per_f[f] for f in FRAMES_PINNED} == pins[key], key
    assert set(tfl_slice.NOT_COVERED) <= set(NOT_COVERED_CAP)
    for name in tfl_slice.CHAINS:
        not_covered = tfl_slice.NOT_COVERED.get(name, {})
        assert len(not_covered) <= NOT_COVERED_CAP[name] and all(reason for reason in not_covered.values())
        for k, f in ((0, 32), (1, 1)):
            reached = set()
            for sid, _, _, _ in tfl_slice.table(name):
                there_for = tfl_slice.THERE_FOR[sid][k]
                assert set(there_for) <= set(launch_labels[sid][f]), (sid, f, there_for, launch_labels[sid][f])
                reached |= set(there_for)
            parent = set(launch_labels[name][f])
            assert parent - reached == set(not_covered) & parent, (name, f, parent - reached)
    # the launches the two cut rules are there for
    assert "mdblock_kernel<stem+pair>" in launch_labels["landmark:0-35"][32] and "mdblock_kernel<pair>" in launch_labels["landmark:35-65"][32]
    assert launch_labels["back:0-4"][32] == ["stem_mfma_kernel"] and launch_labels["back:136-out"][32] == ["mstrip_chain_kernel<12,1>", "chain_kernel<3>"]


def test_spread_of_the_f32_evaluations(cases):
    """E_max and E_rms of the C oracle, torch and torch with oneDNN off against float64, per case, output and frame: the largest ratio between any two of
    them is at most M / 2.  (A case where one of them is exact has no ratio; the criterion's floors are for those.)"""
    worst = {"max": (0.0, None), "rms": (0.0, None)}
    for sid, c in cases.items():
        for o, f in enumerate(c.ref["f64"]):
            es = [slice_refs.errors(c.ref[k][o], f) for k in ("c", "torch", "plain")]
            for j, what in enumerate(("max", "rms")):
                a = np.stack([e[j] for e in es])
                for frame in range(3):
                    if a[:, frame].min() > 0:
                        r = float(a[:, frame].max() / a[:, frame].min())
                        if r > worst[what][0]:
                            worst[what] = (r, (sid, o, frame, a[:, frame].tolist()))
    print("spread: max %.2f at %s; rms %.2f at %s" % (worst["max"] + worst["rms"]))
    assert len(cases) == 56
    assert worst["max"][0] <= slice_refs.M / 2 and worst["rms"][0] <= slice_refs.M / 2, worst
    assert slice_refs.M == 32


def _first_conv_bias(graph):
    """The bias of the first convolution that has one (the shipped graphs' depthwise biases are all zero: raising one by 2^-10 x 0 plants nothing)."""
    for op in graph.ops:
        if op.code in (tfl3.CONV_2D, tfl3.DEPTHWISE_CONV_2D) and np.abs(graph.tensors[op.inputs[2]].data).max() > 0:
            return graph.tensors[op.inputs[2]]


FAULTS = ("last row x (1 + s 2^-10)", "corner pixel moved s of the way to its neighbour", "first bias, channel 0, + s 2^-10 max|bias|")


@pytest.mark.parametrize("name,sid", [("back", "back:69-101"), ("landmark", "landmark:65-74"), ("iris", "iris:33-47")])
def test_criterion_rejects_what_raw_tol_accepts(cases, name, sid):
    """A middle slice evaluated in torch f32 with one planted fault: the criterion rejects every fault at the slice, on the noise frame and on the
    picture frame.  The same faulty tensor carried through the rest of the chain (torch f32) to the network's outputs, against the C oracle under
    RAW_TOL: at least one fault per graph passes there.  Where none does at full size (s = 1) the faults are halved until one does, and at every
    size tried the criterion still rejects all three at the slice.  Measured: landmark and iris at s = 1 (the row and the bias fault on both frames: 5e-6 .. 8e-5
    x scale at the outputs; the corner 1.5e-4 .. 2e-3); back at s = 1/2 (the row fault on the noise frame 5.7e-5, the bias fault 7.0e-5 / 5.5e-5; at
    s = 1 they are 1.1e-4 .. 2.7e-4, the corner 1e-2).  At the slice the faintest fault is 20 times the bound (back's halved bias fault, rms)."""
    case, whole = cases[sid], cases[name]
    chain = [s for s, _, _, in_chain in tfl_slice.table(name) if in_chain]
    behind = chain[chain.index(sid) + 1:]
    assert case.judge([r[:2] for r in case.ref["torch"]], frames=(0, 1))[0]      # the unfaulted evaluation passes
    size, passes_raw_tol = 1.0, 0
    while not passes_raw_tol and size >= 2.0 ** -6:
        for fault in FAULTS:
            x = case.x3[:2].copy()
            g = tfl3.load(case.path)
            if fault == FAULTS[0]:
                x[:, -1] *= np.float32(1 + size * 2.0 ** -10)
            elif fault == FAULTS[1]:
                x[:, 0, 0] += np.float32(size) * (x[:, 0, 1] - x[:, 0, 0])
            else:
                b = _first_conv_bias(g)
                v = np.array(b.data, dtype=np.float32)
                v[0] += np.float32(size * 2.0 ** -10 * np.abs(v).max())
                b.data = v
            assert fault == FAULTS[2] or not np.array_equal(x, case.x3[:2])
            y = evaluate.run(g, x)
            for frame in (0, 1):
                ok, text = case.judge([r[frame:frame + 1] for r in y], frames=(frame,))
                print("s = %g, %s | %s" % (size, fault, text))
                assert not ok, (fault, size, frame)
            t = y[0]
            for s in behind:
                t = evaluate.run(cases[s].graph, t)
                t = t[0] if s != behind[-1] else t
            for frame in (0, 1):
                worst = max(float(np.abs(o[frame] - r[frame].reshape(o[frame].shape)).max()) / max(1.0, float(np.abs(r[frame]).max())) for o, r in zip(t, whole.ref["c"]))
                print("%s: s = %g, %s, frame %d, at the network's outputs: %.2e x scale, RAW_TOL %s it" % (
                    name, size, fault, frame, worst, "accepts" if worst <= RAW_TOL else "rejects"))
                passes_raw_tol += worst <= RAW_TOL
        if not passes_raw_tol:
            size /= 2
    print("%s: faults of size s = %g: %d of 6 (fault, frame) pairs pass RAW_TOL" % (name, size, passes_raw_tol))
    assert passes_raw_tol >= 1
