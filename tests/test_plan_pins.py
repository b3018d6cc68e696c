"""Everything the graph lowering (build_plan: the csrc/plan*.cpp sources and layout.hpp) returns — the Graph as the lowering left it, every Node field by
field through members, head nodes and stages, Plan::branch, the storage table, the arena, the traffic / MAC figures and the describe() text — for the
shipped models, the synthetic graphs of tests/synth_tflite.py, tests/embed_ops_synth.py and tests/resnet_synth.py (smallest sizes; the ONNX-style
writings are the only inputs that exercise layout.hpp) and one row with MI_NO_WIDEN_GROUPS set, against pins.  CPU only: the lowering is host code, linked
here (host side of hipcc) against the product's objects the way test_launch_pins.py links its driver.

The pins (tests/golden/plan_pins.json) were made from the code this set of modules replaced, not from the modules: tests/plan_dump.cpp, with its own
printing code, was built against the unmodified single-file plan.cpp (2318 lines, build_plan_impl one function) and layout.hpp of the parent commit,
and `python tests/test_plan_pins.py --write` run there.  Regenerated from the split sources the file is byte-identical.
The rows at the defaults keep, in the clear, the plan-level lines (graph header, branch, arena and figures, the describe() text) and one hash per kind of
table line (tensors, operators, nodes, stages, head pairs, storage; for the synthetic graphs the node lines of describe() too: its header line stays);
every other row is one hash of all its lines (the whole text is many megabytes)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import embed_ops_synth as es
import resnet_synth as rs
import synth_tflite
from conftest import MODELS, ROOT

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
PINS = os.path.join(ROOT, "tests", "golden", "plan_pins.json")
SHIPPED_ROWS = ("defaults", "fuse=0", "fuse=1", "fuse=2", "fuse=3", "fuse=4", "tail=0", "pipe=0", "pipe=2", "pipe=3", "res=64k", "fuse=4+pipe=2")
SYNTH_ROWS = ("defaults", "fuse=2", "fuse=0")
TABLES = "TONSPR"   # line tags of the per-tensor / per-operator / per-node / per-stage / per-pair / per-storage lines
ENV_ROW = ("face_detection_front.tflite", "MI_NO_WIDEN_GROUPS")


def _refused_mean():
    return es.mean_graph(5, 7, 8, (3,))


def _refused_hwc_constant():
    g = es.EmbedOpsBuilder(9, [1, 5, 7, 8])
    g.outputs = [g.sub_const(g.input, np.ones((5, 7, 8)))]
    return g.finish()


# the graphs that embed_ops_synth.py and resnet_synth.py build, at their smallest sizes, and two that the lowering refuses (the message is part of the pin)
EXTRA = {
    "avgpool_global": lambda: es.avgpool_graph(7, 7, 40, 7, 7),
    "avgpool_3x3_s2_same": lambda: es.avgpool_graph(9, 11, 12, 3, 3, 2, synth_tflite.SAME),
    "mean_keep": lambda: es.mean_graph(7, 7, 40, (1, 2), True),
    "mean_negative_axes_view": lambda: es.mean_graph(5, 3, 7, (-3, -2), False),
    "l2norm_rank2": lambda: es.l2norm_graph((1, 128)),
    "l2norm_rank4": lambda: es.l2norm_graph((1, 4, 4, 8)),
    "x_minus_c": lambda: es.arith_graph("x-c", 7, const=np.arange(1, 8)),
    "c_minus_x": lambda: es.arith_graph("c-x", 7, const=np.arange(1, 8)),
    "x_div_128": lambda: es.arith_graph("x/c", 32, const=128.0),
    "x_div_c": lambda: es.arith_graph("x/c", 32, const=np.linspace(0.7, 3.1, 32)),
    "transpose_to_nchw": lambda: es.transpose_graph(5, 7, 3, (0, 3, 1, 2)),
    "transpose_and_back": lambda: es.transpose_graph(33, 35, 40, (0, 2, 3, 1), back=True),
    "transpose_identity": lambda: es.transpose_graph(5, 7, 3, (0, 1, 2, 3)),
    "pooled_head_avgpool": lambda: es.pooled_head(3, 16, "avgpool"),
    "pooled_head_mean": lambda: es.pooled_head(3, 16, "mean"),
    "pooled_head_mean_keep": lambda: es.pooled_head(3, 16, "mean_keep"),
    "onnx_style_nchw": lambda: es.onnx_style(3, 16, c0=8, layout="nchw"),
    "onnx_style_nhwc": lambda: es.onnx_style(3, 16, c0=8, layout="nhwc"),
    "onnx_style_twin": lambda: es.onnx_style(3, 16, c0=8, layout="twin"),
    "onnx_style_nchw_feature_map": lambda: es.onnx_style(3, 16, c0=8, layout="nchw", out="feature_map"),
    "onnx_style_nchw_two_blocks": lambda: es.onnx_style(3, 16, c0=8, blocks=(2, 1, 1, 1), layout="nchw"),
    "iresnet_like": lambda: rs.iresnet_like(3, 16, c0=8),
    "conv_layer_explicit_pad": lambda: rs.conv_layer(5, 6, 5, 8, 8, 3, 2, synth_tflite.VALID, (1, 0, 1, 0))[0],
    "conv_layer_act_then_add": lambda: rs.conv_layer(6, 6, 5, 8, 8, skip="act_then_add")[0],
    "conv_layer_add_then_prelu": lambda: rs.conv_layer(7, 6, 5, 8, 8, skip="add_then_prelu")[0],
    "affine_graph": lambda: rs.affine_graph(8, 7)[0],
    "fold_graph": lambda: rs.fold_graph(9)[0],
    "odd_width_graph": lambda: rs.odd_width_graph(10),
    "refused_mean_over_channels": _refused_mean,
    "refused_sub_by_an_hwc_constant": _refused_hwc_constant,
}


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def pinned(cfg, lines):
    """A configuration as the pin file keeps it: at the defaults the plan-level lines and one hash per table (for a synthetic graph the node lines of
    describe() count as a table too), else one hash."""
    if cfg.split()[1] != "defaults":
        return sha(lines)
    shipped = os.path.exists(os.path.join(MODELS, cfg.split()[0]))

    def table_of(line):
        if line[:1] in TABLES and line[1:2] == " ":
            return line[0]
        return "D" if not shipped and line.startswith("D ") and not line.startswith("D #") else None

    tables = []
    for tag in TABLES + ("" if shipped else "D"):
        rows = [line for line in lines if table_of(line) == tag]
        tables.append("%s x%d %s" % (tag, len(rows), sha(rows)))
    return tables + [line for line in lines if table_of(line) is None]


def parse(stdout, rename=None):
    got, cur = {}, None
    for line in stdout.splitlines():
        if line.startswith("== "):
            cur = got.setdefault(rename(line[3:]) if rename else line[3:], [])
        else:
            cur.append(line)
    return got


def build_driver(tmp):
    """tests/plan_dump.cpp linked against the product's objects"""
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    hipcc = "/opt/rocm/bin/hipcc"
    o = os.path.join(tmp, "plan_dump.o")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "plan_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    exe = os.path.join(tmp, "plan_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)
    return exe


def synth_names():
    return sorted(synth_tflite.CASES) + sorted(EXTRA)


def dump(tmp):
    """Every configuration's lines, as plan_dump prints them."""
    exe = build_driver(tmp)
    files = []
    for name in synth_names():
        blob = synth_tflite.CASES[name][0]() if name in synth_tflite.CASES else EXTRA[name]()
        files.append(os.path.join(tmp, name + ".tflite"))
        with open(files[-1], "wb") as f:
            f.write(blob)
    models = sorted(n for n in os.listdir(MODELS) if n.endswith(".tflite"))
    got = {}
    for which, paths in (("shipped", [os.path.join(MODELS, n) for n in models]), ("synth", files)):
        r = subprocess.run([exe, which] + paths, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got.update(parse(r.stdout))
    # MI_NO_WIDEN_GROUPS is read once into a static: a process of its own
    r = subprocess.run([exe, "env", os.path.join(MODELS, ENV_ROW[0])], capture_output=True, text=True, timeout=600, env=dict(os.environ, MI_NO_WIDEN_GROUPS="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    got.update(parse(r.stdout, lambda cfg: cfg.replace(" env", " " + ENV_ROW[1])))
    return models, got


@pytest.fixture(scope="module")
def lowered(tmp_path_factory):
    return dump(str(tmp_path_factory.mktemp("plan_dump")))


def test_plans_match_their_pins(lowered):
    models, got = lowered
    assert len(models) == 7
    # the set of configurations is complete: every shipped model at every level, with the tail form off, at every pipe_max, at the small LDS budget;
    # every synthetic graph at levels 5, 2 and 0; the one row with the environment variable
    want = {"%s %s" % (m, row) for m in models for row in SHIPPED_ROWS}
    want |= {"%s.tflite %s" % (c, row) for c in synth_names() for row in SYNTH_ROWS}
    want.add(" ".join(ENV_ROW))
    assert set(got) == want and len(want) == 7 * 12 + 3 * (len(synth_tflite.CASES) + len(EXTRA)) + 1
    pins = json.load(open(PINS))
    assert set(pins) == want
    for cfg in sorted(pins):
        now = pinned(cfg, got[cfg])
        if now != pins[cfg]:
            print(cfg)
            print("\n".join(got[cfg][-60:]))
        assert now == pins[cfg], (cfg, now, pins[cfg])
    # only the graphs written to be refused are refused, and with the operator's name
    threw = {cfg: got[cfg][0] for cfg in got if got[cfg] and got[cfg][0].startswith("threw")}
    assert set(threw) == {"%s.tflite %s" % (c, row) for c in ("refused_mean_over_channels", "refused_sub_by_an_hwc_constant") for row in SYNTH_ROWS}, threw
    assert all(("MEAN" in msg) == ("mean" in cfg) and ("SUB" in msg) == ("sub" in cfg) for cfg, msg in threw.items()), threw
    # the environment variable's row is a different plan from the defaults row
    assert got[" ".join(ENV_ROW)] != got[ENV_ROW[0] + " defaults"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_plan_pins.py --write   (after the product is built: writes tests/golden/plan_pins.json from the tree's lowering)")
    with tempfile.TemporaryDirectory() as tmp:
        _, got = dump(tmp)
    with open(PINS, "w") as f:
        # one configuration per line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(cfg), json.dumps(pinned(cfg, got[cfg]))) for cfg in sorted(got)) + "\n}\n")
    print("%d configurations, %d bytes" % (len(got), os.path.getsize(PINS)))
