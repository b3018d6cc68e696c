"""The float64 yardstick of tests/test_slices_cpu.py and tests/test_f64_parity_gpu.py (test infrastructure): input frames, the slices' inputs,
the reference evaluations and the criterion.  Everything here runs on the CPU.

Per shipped graph three frames: 0 a seeded noise frame in the model's input range, 1 the man.jpg tensor (the letterboxed picture for the detectors,
the face crop for the mesh, the right-eye crop for iris), 2 a copy of frame 0.  A slice's input is, for frames 0 and 1, the C oracle's f32 tensor at
its cut (the output of the slices in front of it); for frame 2 the edgy frame made of frame 0's tensor: a quarter of it, with the first row +m, the last
row -0.7 m, the first column +0.5 m and the last column -0.9 m, m the tensor's largest magnitude: large values on the frame's border, where halo
rows, band seams and padding live.  A batch of 33 (above every batch threshold of the launch lists) holds these three at frames 0, 16 and 32
and 30 intermediates of fresh noise frames between them.

Per case (a slice or a whole graph), per output tensor and per checked frame, against a float64 evaluation of the same graph on the same input
(oracle/np/evaluate.py, dtype float64: the constants are the file's f32 / f16 values):
    E_max = max|y - f64| / scale      E_rms = rms(y - f64) / scale      scale = max(1, max|f64|)
of an f32 evaluation y.  The criterion for a result `got`, with E the larger of the C oracle's and torch's errors on that input:
    max|got - f64| / scale <= max(M * E_max, 4 * 2^-24)     rms(got - f64) / scale <= max(M * E_rms, 2^-24)
M = 32 is the power of two that is at least twice the spread measured among three valid f32 orderings on the CPU, 10.2 over the full table
(test_slices_cpu.py; on the back detector's slices alone the spread is 1.5, and M would be 4); the floors are a few ulp at the tensor's scale
and matter where the references happen to be exact (one-element outputs, zero frames).  M is never taken from a GPU run.
"""
import os

import numpy as np
import torch

import tfl_slice
from conftest import GOLDEN, INPUT_RANGE, model_path
from oracle import pyoracle
from oracle.np import evaluate, tfl3

M = 32
FLOOR_MAX, FLOOR_RMS = 4 * 2.0 ** -24, 2.0 ** -24
NOISE_SEED = 20260
CHECKED = (0, 16, 32)      # where the three frames sit in a batch of 33


def network_frames(name, extra=0):
    """[3 + extra, H, W, 3]: the three frames of the graph, then `extra` fresh noise frames."""
    om = pyoracle.Model(model_path(name))
    h, w = om.input_dims[1:3]
    lo, hi = INPUT_RANGE[name]
    noise = np.random.RandomState(NOISE_SEED).uniform(lo, hi, (1 + extra, h, w, 3)).astype(np.float32)
    gold = np.load(os.path.join(GOLDEN, "golden.npz"))
    if name == "landmark":
        pic = (gold["man_face_u8"].astype(np.float64) / 255.0).astype(np.float32)
    elif name == "iris":
        pic = (gold["man_eye_right_u8"].astype(np.float64) / 255.0).astype(np.float32)
    else:
        man = pyoracle.jpeg_decode_rgb(open(os.path.join(GOLDEN, "man.jpg"), "rb").read())
        pic, _ = pyoracle.image_to_tensor(man, None, (w, h), True, (-1.0, 1.0), False)
    return np.concatenate([noise[:1], pic[None], noise[:1], noise[1:]])


def edgy(t):
    """The edgy frame of one frame's tensor [H, W, C]."""
    m = np.float32(np.abs(t).max())
    e = (np.float32(0.25) * t).astype(np.float32)
    e[0], e[-1] = m, np.float32(-0.7) * m
    e[:, 0], e[:, -1] = np.float32(0.5) * m, np.float32(-0.9) * m
    return e


def errors(y, f64):
    """(E_max, E_rms) per frame of one output tensor, [B, ...] each."""
    b = f64.shape[0]
    f = f64.reshape(b, -1)
    d = y.reshape(b, -1).astype(np.float64) - f
    scale = np.maximum(1.0, np.abs(f).max(axis=1))
    return np.abs(d).max(axis=1) / scale, np.sqrt((d * d).mean(axis=1)) / scale


class Case:
    """A slice (or a whole graph) as a model file with its three input frames and the evaluations of them.
    ref[k] = list per output of [3, ...] arrays, k in f64 / c / torch / plain (torch with oneDNN off, on request)."""

    def __init__(self, sid, path, x3, rest=None, plain=False):
        self.sid, self.path, self.x3, self.rest = sid, path, x3, rest
        self.graph = tfl3.load(path)
        self.oracle = pyoracle.Model(path)
        self.ref = {"f64": evaluate.run(self.graph, x3, dtype=np.float64), "c": self.oracle.run(x3, nthreads=3), "torch": evaluate.run(self.graph, x3)}
        if plain:
            with torch.backends.mkldnn.flags(enabled=False):
                self.ref["plain"] = evaluate.run(self.graph, x3)
        # E: per output (E_max [3], E_rms [3]), the larger of the C oracle's and torch's
        self.E = []
        for o, f in enumerate(self.ref["f64"]):
            (cm, cr), (tm, tr) = errors(self.ref["c"][o], f), errors(self.ref["torch"][o], f)
            self.E.append((np.maximum(cm, tm), np.maximum(cr, tr)))

    def bounds(self, o):
        return np.maximum(M * self.E[o][0], FLOOR_MAX), np.maximum(M * self.E[o][1], FLOOR_RMS)

    def judge(self, outs, frames=(0, 1, 2)):
        """outs: per output [len(frames), ...] results for the case's frames `frames`.  -> (accepted, text): the criterion over every output and
        frame, and per output and frame the ratios got / E (max, rms) and got / bound."""
        ok, lines = True, []
        for o, got in enumerate(outs):
            f = self.ref["f64"][o][list(frames)]
            gm, gr = errors(np.asarray(got).reshape(f.shape), f)
            bm, br = (b[list(frames)] for b in self.bounds(o))
            em, er = (e[list(frames)] for e in self.E[o])
            for k, fr in enumerate(frames):
                good = gm[k] <= bm[k] and gr[k] <= br[k]
                ok = ok and good
                lines.append("%s out %d frame %d: max %.3e (E %.3e, x%.2f of E, %.2f of bound)  rms %.3e (E %.3e, x%.2f of E, %.2f of bound)%s" % (
                    self.sid, o, fr, gm[k], em[k], gm[k] / max(em[k], 1e-300), gm[k] / bm[k], gr[k], er[k], gr[k] / max(er[k], 1e-300), gr[k] / br[k],
                    "" if good else "  REJECTED"))
        return ok, "\n".join(lines)

    def batch33(self):
        """(x [33, ...], C oracle's outputs on it): the three frames at 0, 16, 32, the 30 noise intermediates between them."""
        assert self.rest is not None and len(self.rest) == 30
        x = np.concatenate([self.x3[:1], self.rest[:15], self.x3[1:2], self.rest[15:], self.x3[2:]])
        return x, self.oracle.run(x, nthreads=8)

    def judge_rest(self, outs33, c33):
        """The 30 unchecked frames of a batch of 33 against the C oracle alone: |got - C| / scale <= (M + 1) * the largest E_max of the three checked
        frames (triangle inequality over the float64 value: got within M E of it, C within E), scale = max(1, max|C|) per frame."""
        ok, lines = True, []
        rest = [i for i in range(33) if i not in CHECKED]
        for o, (got, c) in enumerate(zip(outs33, c33)):
            g, c = np.asarray(got).reshape(33, -1)[rest].astype(np.float64), c.reshape(33, -1)[rest].astype(np.float64)
            d = np.abs(g - c).max(axis=1) / np.maximum(1.0, np.abs(c).max(axis=1))
            bound = max((M + 1) * float(self.E[o][0].max()), FLOOR_MAX)
            ok = ok and bool((d <= bound).all())
            lines.append("%s out %d, 30 frames vs C: worst %.3e, bound %.3e%s" % (self.sid, o, d.max(), bound, "" if (d <= bound).all() else "  REJECTED"))
        return ok, "\n".join(lines)


def build_cases(name, tmpdir, extra=0, plain=False, only=None):
    """{id: Case} of one shipped graph: the whole graph under its name, and its slices (tfl_slice.table) written into tmpdir.  extra = 30 adds the
    noise intermediates of the batch of 33.  only: ids to build (the chain's intermediates are computed regardless)."""
    graph = tfl3.load(model_path(name))
    frames = network_frames(name, extra)
    cases = {}
    if only is None or name in only:
        cases[name] = Case(name, model_path(name), frames[:3], frames[3:] if extra else None, plain)
    base = np.concatenate([frames[:2], frames[3:]])         # frame 0, frame 1, the noise frames: what the cuts' tensors are computed of
    at = {graph.inputs[0]: base}
    files = {}

    def model_of(tin, touts):
        key = (tin, tuple(touts))
        if key not in files:
            p = os.path.join(str(tmpdir), "%s_%d_%s.tflite" % (name, tin, "_".join(map(str, touts))))
            with open(p, "wb") as f:
                f.write(tfl_slice.slice_graph(graph, tin, touts))
            files[key] = p
        return files[key]

    cuts = tfl_slice.CHAINS[name]
    for k in range(len(cuts) - 1):
        at[cuts[k + 1]] = pyoracle.Model(model_of(cuts[k], [cuts[k + 1]])).run(at[cuts[k]], nthreads=8)[0]
    for sid, tin, touts, _ in tfl_slice.table(name):
        if only is not None and sid not in only:
            continue
        if tin not in at:   # a cut inside a chain slice: from the last chain cut in front of it
            for c in reversed(cuts):
                try:
                    at[tin] = pyoracle.Model(model_of(c, [tin])).run(at[c], nthreads=8)[0]
                    break
                except ValueError:
                    continue
        t = at[tin]
        x3 = np.stack([t[0], t[1], edgy(t[0])])
        cases[sid] = Case(sid, model_of(tin, touts or list(graph.outputs)), x3, t[2:] if extra else None, plain)
    return cases
