"""AVERAGE_POOL_2D, MEAN, L2_NORMALIZATION, SUB, DIV and TRANSPOSE through the host side (no GPU): the reader and the lowering take the synthetic
graphs of tests/embed_ops_synth.py at every fusion level (the parent commit: "plan: builtin operator N unsupported"), graphs outside the rules are
refused with a message that names the operator, a power-of-two DIV merges into its neighbour while any other DIV keeps a launch of its own, the
new kernels neither spill nor use scratch, the layout normalisation (csrc/layout.hpp) turns the ONNX-style writing of a network into the plan of its
NHWC writing, and the host lowering survives mutated blobs of these graphs under AddressSanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import embed_ops_synth as es
from conftest import ROOT
from synth_tflite import ACT_RELU, SAME

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
LINE = re.compile(r"^(\w+)((?:\+[\w()]+)*) t(\d+)\[[^\]]*\] -> t(\d+)\[")


def nodes_of(text):
    """(kind, suffixes like '+prelu', input tensor, output tensor) per plan node"""
    out = []
    for line in text.splitlines()[1:]:
        m = LINE.match(line)
        assert m, line
        out.append((m.group(1), m.group(2), int(m.group(3)), int(m.group(4))))
    return out

GRAPHS = {
    "avgpool_global": lambda: es.avgpool_graph(7, 7, 40, 7, 7),
    "avgpool_3x3_s2_same": lambda: es.avgpool_graph(9, 11, 12, 3, 3, 2, SAME),
    "avgpool_relu_scalar": lambda: es.avgpool_graph(8, 8, 7, 2, 2, 2, act=ACT_RELU),
    "mean_keep": lambda: es.mean_graph(7, 7, 40, (1, 2), True),
    "mean_negative_axes_view": lambda: es.mean_graph(5, 3, 7, (-3, -2), False),
    "mean_repeated_axes": lambda: es.mean_graph(5, 3, 7, (1, 2, -2), True),
    "l2norm_rank2": lambda: es.l2norm_graph((1, 128)),
    "l2norm_rank4": lambda: es.l2norm_graph((1, 4, 4, 8)),
    "x_minus_c": lambda: es.arith_graph("x-c", 7, const=np.arange(1, 8)),
    "c_minus_x": lambda: es.arith_graph("c-x", 7, const=np.arange(1, 8)),
    "x_div_128": lambda: es.arith_graph("x/c", 32, const=128.0),
    "x_div_c": lambda: es.arith_graph("x/c", 32, const=np.linspace(0.7, 3.1, 32)),
    "transpose_to_nchw": lambda: es.transpose_graph(5, 7, 3, (0, 3, 1, 2)),
    "transpose_and_back": lambda: es.transpose_graph(33, 35, 40, (0, 2, 3, 1), back=True),
    "transpose_hw": lambda: es.transpose_graph(5, 7, 3, (0, 2, 1, 3)),
    "pooled_head_avgpool": lambda: es.pooled_head(3, 128, "avgpool"),
    "pooled_head_mean": lambda: es.pooled_head(3, 512, "mean"),
    "pooled_head_mean_keep": lambda: es.pooled_head(3, 128, "mean_keep"),
    "onnx_style_nchw": lambda: es.onnx_style(3, 128, layout="nchw"),
    "onnx_style_nhwc": lambda: es.onnx_style(3, 128, layout="nhwc"),
    "onnx_style_twin": lambda: es.onnx_style(3, 128, layout="twin"),
}
NEW_KINDS = {"avgpool": "pool", "mean": "pool", "l2norm": "l2norm", "x_": "affine", "c_": "affine", "transpose": "transpose"}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_every_synthetic_graph_lowers_at_every_level(mi, name):
    blob = GRAPHS[name]()
    for fuse in (0, 2, 4, 5):
        kinds = [n[0] for n in nodes_of(mi.plan_describe(blob, fuse))]   # (the parent commit: "plan: builtin operator N unsupported")
        for prefix, kind in NEW_KINDS.items():
            if name.startswith(prefix):
                assert kind in kinds, (name, fuse, kinds)
        if name.startswith("pooled_head"):
            assert kinds.count("pool") == 1 and kinds.count("l2norm") == 1 and kinds[-1] == "l2norm", (fuse, kinds)


def test_transposes_keep_one_node_each_and_the_identity_none(mi):
    for fuse in (0, 5):
        kinds = lambda blob: [n[0] for n in nodes_of(mi.plan_describe(blob, fuse))]   # noqa: E731
        assert kinds(es.transpose_graph(5, 7, 3, (0, 3, 1, 2))) == ["transpose"]               # a channel-first graph output: exactly one
        assert kinds(es.transpose_graph(5, 7, 3, (0, 3, 1, 2), back=True)) == ["transpose"] * 2
        assert "transpose" not in kinds(es.transpose_graph(5, 7, 3, (0, 1, 2, 3)))             # the identity is an alias (a view)
        text = mi.plan_describe(es.transpose_graph(5, 7, 3, (0, 3, 1, 2)), fuse)
        assert "t0[5x7x3] -> t2[3x5x7] perm 0312" in text, text


def test_mean_without_keep_dims_is_a_view_of_the_pool(mi):
    nodes = nodes_of(mi.plan_describe(es.mean_graph(5, 3, 7, (1, 2), False), 5))
    assert [n[0] for n in nodes] == ["pool", "reshape"] and nodes[1][2] == nodes[0][3], nodes
    assert "k5x3 s1 valid" in mi.plan_describe(es.mean_graph(5, 3, 7, (1, 2), False), 5)


# ---------------------------------------------------------------------------------------------------- layout normalisation
def _stripped(text):
    """plan lines without tensor ids and operator indices"""
    return [re.sub(r" ops\{[^}]*\}", "", re.sub(r"\bt\d+", "t", line)) for line in text.splitlines()[1:]]


@pytest.mark.parametrize("blocks", [(1, 1, 1, 1), (2, 1, 1, 1)])
def test_the_onnx_style_network_lowers_to_the_nhwc_network_s_plan(mi, blocks):
    """every TRANSPOSE of the "nchw" writing disappears: its node list is the "nhwc" writing's at every level, up to tensor ids"""
    blobs = {layout: es.onnx_style(3, 128, blocks=blocks, layout=layout) for layout in ("nchw", "nhwc", "twin")}
    for fuse in (0, 2, 4, 5):
        texts = {layout: mi.plan_describe(blob, fuse) for layout, blob in blobs.items()}
        assert "transpose" not in texts["nchw"], texts["nchw"]
        assert _stripped(texts["nchw"]) == _stripped(texts["nhwc"]), fuse
        assert "k7x7" in texts["nchw"] and ("GEMM over the batch" in texts["nchw"]) == (fuse >= 2)


def test_a_channel_first_graph_output_gets_exactly_one_transpose(mi):
    for fuse in (0, 5):
        kinds = [n[0] for n in nodes_of(mi.plan_describe(es.onnx_style(3, 128, layout="nchw", out="feature_map"), fuse))]
        assert kinds.count("transpose") == 1 and kinds[-1] == "transpose", kinds
        assert kinds[:-1] == [n[0] for n in nodes_of(mi.plan_describe(es.onnx_style(3, 128, layout="nhwc", out="feature_map"), fuse))]


def _channel_first(build):
    """[1,6,5,8] -> TRANSPOSE (0,3,1,2) -> build(g, the channel-first tensor [1,8,6,5])"""
    g = _g((1, 6, 5, 8))
    y = build(g, g.transpose(g.input, (0, 3, 1, 2)))
    g.outputs = list(y) if isinstance(y, (list, tuple)) else [y]
    return g.finish()


def test_readers_outside_the_table_share_one_materialised_transpose(mi):
    # two L2_NORMALIZATIONs (over W of the NCHW tensor: no row of the table) and the tensor as a graph output: one launch for all three
    blob = _channel_first(lambda g, t: [g.l2norm(t), g.l2norm(t), t])
    for fuse in (0, 5):
        assert [n[0] for n in nodes_of(mi.plan_describe(blob, fuse))] == ["transpose", "l2norm", "l2norm"]
    # the rows of the table, one by one: no transpose remains when the result goes back through TRANSPOSE (0,2,3,1)
    back = lambda g, t: g.transpose(t, (0, 2, 3, 1))   # noqa: E731
    rows = {
        "relu": lambda g, t: back(g, g.relu(t)),
        "mul_1c11": lambda g, t: back(g, g.mul_const(t, np.linspace(0.5, 1.5, 8).reshape(1, 8, 1, 1))),
        "sub_c11_const_first": lambda g, t: back(g, g.sub_const(t, np.linspace(0.5, 1.5, 8).reshape(8, 1, 1), const_first=True)),
        "div_scalar": lambda g, t: back(g, g.div_const(t, np.float32(3.0))),
        "add_two_channel_first": lambda g, t: back(g, g.add(g.relu(t), t)),
        "mean_23_keep": lambda g, t: back(g, g.mean(t, (2, 3), True)),
        "mean_23": lambda g, t: g.mean(t, (-1, 2), False),
    }
    for name, build in rows.items():
        for fuse in (0, 5):
            kinds = [n[0] for n in nodes_of(mi.plan_describe(_channel_first(build), fuse))]
            assert "transpose" not in kinds and len(kinds) >= 1, (name, fuse, kinds)
    # a constant along another axis of the channel-first tensor is no row: the MUL reads the materialised tensor, and is refused there by name
    with pytest.raises(mi.MiError) as e:
        mi.plan_describe(_channel_first(lambda g, t: g.mul_const(t, np.ones((1, 1, 6, 1)))), 5)
    assert "MUL" in str(e.value) and "per-channel" in str(e.value)


# ---------------------------------------------------------------------------------------------------- refusals
def _g(shape=(1, 5, 7, 8)):
    return es.EmbedOpsBuilder(9, list(shape))


def _out(g, y):
    g.outputs = [y]
    return g.finish()


def _rank3_transpose():
    g = _g()
    return _out(g, g.transpose(g.reshape(g.input, [1, 35, 8]), (0, 2, 1)))


REFUSALS = {
    "mean_over_the_channel_axis": (lambda: es.mean_graph(5, 7, 8, (3,)), ("MEAN", "axes")),
    "mean_over_the_batch_axis": (lambda: es.mean_graph(5, 7, 8, (0, 1, 2)), ("MEAN", "axes")),
    "mean_over_one_spatial_axis": (lambda: es.mean_graph(5, 7, 8, (1,)), ("MEAN", "axes")),
    "mean_axis_out_of_range": (lambda: es.mean_graph(5, 7, 8, (1, 7)), ("MEAN", "axis")),
    "mean_axes_not_constant": (lambda: (lambda g: _out(g, g.mean(g.input, (1, 2), axes_const=False)))(_g()), ("MEAN", "constant")),
    "mean_of_a_rank_2_tensor": (lambda: (lambda g: _out(g, g.mean(g.reshape(g.input, [1, 280]), (1,))))(_g()), ("MEAN", "[1,H,W,C]")),
    "l2norm_with_an_activation": (lambda: (lambda g: _out(g, g.l2norm(g.input, act=ACT_RELU)))(_g()), ("L2_NORMALIZATION", "activation")),
    "avgpool_output_shape": (lambda: (lambda g: _out(g, g.avgpool(g.input, 2, 2, 2, out_shape=[1, 3, 4, 8])))(_g()), ("AVERAGE_POOL_2D", "output shape")),
    "avgpool_valid_window_larger_than_the_frame": (lambda: (lambda g: _out(g, g.avgpool(g.input, 9, 9, out_shape=[1, 1, 1, 8])))(_g()), ("AVERAGE_POOL_2D", "window")),
    "avgpool_of_a_channel_first_tensor": (lambda: _channel_first(lambda g, t: g.avgpool(t, 2, 2, 2)), ("AVERAGE_POOL_2D", "channel-first")),
    "maxpool_of_a_channel_first_tensor": (lambda: _channel_first(lambda g, t: g.maxpool(t)), ("MAX_POOL_2D", "channel-first")),
    "c_div_x": (lambda: (lambda g: _out(g, g.div_const(g.input, np.ones(8), const_first=True)))(_g()), ("DIV", "c / x")),
    "div_by_zero": (lambda: (lambda g: _out(g, g.div_const(g.input, [1, 2, 0, 4, 5, 6, 7, 8])))(_g()), ("DIV", "zero")),
    "div_by_infinity": (lambda: (lambda g: _out(g, g.div_const(g.input, np.float32(np.inf))))(_g()), ("DIV", "non-finite")),
    "sub_of_two_activations": (lambda: (lambda g: _out(g, g.sub(g.input, g.relu(g.input))))(_g()), ("SUB", "two activations")),
    "div_of_two_activations": (lambda: (lambda g: _out(g, g.div(g.input, g.relu(g.input))))(_g()), ("DIV", "two activations")),
    "sub_by_an_hwc_constant": (lambda: (lambda g: _out(g, g.sub_const(g.input, np.ones((5, 7, 8)))))(_g()), ("SUB", "per-channel")),
    "div_by_a_channel_first_constant": (lambda: (lambda g: _out(g, g.div_const(g.input, np.full((1, 5, 1, 1), 3.0))))(_g()), ("DIV", "per-channel")),
    "transpose_repeated_entry": (lambda: (lambda g: _out(g, g.transpose(g.input, (0, 1, 1, 2), out_shape=[1, 5, 5, 7])))(_g()), ("TRANSPOSE", "permutation")),
    "transpose_entry_out_of_range": (lambda: (lambda g: _out(g, g.transpose(g.input, (0, 1, 2, 4))))(_g()), ("TRANSPOSE", "permutation")),
    "transpose_negative_entry": (lambda: (lambda g: _out(g, g.transpose(g.input, (0, 1, 2, -1))))(_g()), ("TRANSPOSE", "permutation")),
    "transpose_moves_the_batch_axis": (lambda: (lambda g: _out(g, g.transpose(g.input, (1, 0, 2, 3))))(_g()), ("TRANSPOSE", "batch")),
    "transpose_rank_3": (_rank3_transpose, ("TRANSPOSE", "rank 4")),
    "transpose_perm_not_constant": (lambda: (lambda g: _out(g, g.transpose(g.input, (0, 3, 1, 2), perm_const=False)))(_g()), ("TRANSPOSE", "constant")),
    "transpose_output_shape": (lambda: (lambda g: _out(g, g.transpose(g.input, (0, 3, 1, 2), out_shape=[1, 5, 7, 8])))(_g()), ("TRANSPOSE", "output shape")),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_graphs_outside_the_rules_are_refused_by_name(mi, name):
    make, words = REFUSALS[name]
    for fuse in (0, 5):
        with pytest.raises(mi.MiError) as e:
            mi.plan_describe(make(), fuse)
        assert all(w in str(e.value) for w in words), str(e.value)


# ---------------------------------------------------------------------------------------------------- fold rules
def _conv_then_div(const):
    g = _g((1, 6, 5, 8))
    return _out(g, g.prelu(g.div_const(g.add_const(g.mul_const(g.input)), const)))


def test_a_power_of_two_div_merges_and_any_other_div_keeps_its_launch(mi):
    # MUL -> ADD -> DIV by 4 -> PRELU: one affine launch with the activation from level 1 on
    kinds = [n[0] + n[1] for n in nodes_of(mi.plan_describe(_conv_then_div(np.float32(4.0)), 5))]
    assert kinds == ["affine+prelu"], kinds
    # ... by 3: x * (1 / 3) is a different number, so the division stays a launch (with the PRELU), the MUL / ADD pair in front merges without it
    text = mi.plan_describe(_conv_then_div(np.float32(3.0)), 5)
    kinds = [n[0] + n[1] for n in nodes_of(text)]
    assert kinds == ["affine", "affine+prelu"] and text.count("divisor form") == 1 and "divisor form" in text.splitlines()[2], text
    # per channel, one entry no power of two: the divisor form for all
    assert "divisor form" in mi.plan_describe(es.arith_graph("x/c", 8, const=[2, 4, 8, 16, 0.5, 0.25, 3, 2]), 0)
    assert "divisor form" not in mi.plan_describe(es.arith_graph("x/c", 8, const=[2, 4, 8, 16, 0.5, 0.25, -2, 2]), 0)
    # one launch per operator at level 0
    assert [n[0] for n in nodes_of(mi.plan_describe(_conv_then_div(np.float32(4.0)), 0))] == ["affine"] * 3 + ["act"]
    # a division does not fold into the convolution in front of it either
    g = _g((1, 6, 5, 8))
    text = mi.plan_describe(_out(g, g.prelu(g.div_const(g.conv(g.input, 8, 3), np.float32(3.0)))), 5)
    assert [n[0] + n[1] for n in nodes_of(text)] == ["conv", "affine+prelu"], text


# ---------------------------------------------------------------------------------------------------- ISA
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_do_not_spill(tmp_path):
    """tools/isa_report.py on embed_ops_kernels.hip and on kernels.hip's affine_kernel: no scratch, no spilled registers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    out = str(tmp_path / "embed_ops.s")
    isa_report.compile_asm(os.path.join(isa_report.CSRC, "embed_ops_kernels.hip"), out)
    ks = {k["pretty"]: k for k in isa_report.kernels(out)}
    for want in ("avgpool_kernel<1>", "avgpool_kernel<4>", "l2norm_rows_kernel<true>", "l2norm_rows_kernel<false>", "transpose_kernel", "transpose_tiled_kernel"):
        assert any(want in name for name in ks), (want, sorted(ks))
    out2 = str(tmp_path / "kernels.s")
    isa_report.compile_asm(os.path.join(isa_report.CSRC, "kernels.hip"), out2)
    affine = {k["pretty"]: k for k in isa_report.kernels(out2) if "affine_kernel" in k["pretty"]}
    assert len(affine) == 4, sorted(affine)   # float4 and scalar, multiplicative and divisor form
    ks.update(affine)
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 64, (name, k)   # memory-bound kernels: full occupancy
    tiled = [k for name, k in ks.items() if "transpose_tiled_kernel" in name][0]
    assert tiled["lds"] == 32 * 33 * 4, tiled


# ---------------------------------------------------------------------------------------------------- AddressSanitizer
# the host modules built with AddressSanitizer (the lowering is plan.cpp and its plan_*.cpp passes); their plain objects are not linked.
# tests/test_lowering_asan.py takes the list from here
HOST = ("plan", "plan_ops", "plan_widen", "plan_rewrite", "plan_chain", "plan_resident", "plan_layout", "consts", "bandplan", "launches", "tflite_graph")


def test_lowering_of_mutated_embedding_graphs_under_address_sanitizer(tmp_path):
    """The host lowering built as tests/test_lowering_asan.py builds it (same sources, same flags, tests/asan_lowering.cpp unchanged) over 150
    mutations each of the pooled-head graph, the ONNX-style network and a graph of TRANSPOSE / MEAN / PAD operators: mutated perms, axes, paddings
    and shapes must be refused, never read out of bounds."""
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(f for f in (os.path.join(build, n) for n in os.listdir(build)) if f.endswith(".o") and os.path.basename(f) not in [m + ".o" for m in HOST])
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    flags = ["-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-fsanitize=address", "-fno-gpu-sanitize", "-fno-omit-frame-pointer"]
    hipcc = "/opt/rocm/bin/hipcc"
    mine = []
    for src in [os.path.join(CSRC, m + ".cpp") for m in HOST] + [os.path.join(ROOT, "tests", "asan_lowering.cpp")]:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([hipcc] + flags + ["-x", "hip", "-c", src, "-o", o], stderr=subprocess.DEVNULL)
        mine.append(o)
    exe = str(tmp_path / "asan_lowering")
    subprocess.check_call([hipcc, "-fsanitize=address", "-fno-gpu-sanitize", "--offload-arch=gfx950", "-o", exe] + mine + objs, stderr=subprocess.DEVNULL)

    def layout_ops():
        g = es.EmbedOpsBuilder(21, [1, 9, 11, 8])
        x = g.transpose(g.sub_const(g.input, np.arange(8)), (0, 3, 1, 2))
        x = g.transpose(g.pad_spatial(g.transpose(x, (0, 2, 3, 1)), 1, 1, 1, 1), (0, 1, 3, 2))
        x = g.avgpool(g.transpose(x, (0, 1, 3, 2)), 3, 3, 2, SAME)
        g.outputs = [g.l2norm(g.mean(g.div_const(x, np.float32(3.0)), (1, 2), False))]
        return g.finish()

    blobs = []
    for name, blob in (("pooled_head", es.pooled_head(3, 128)), ("onnx_style_nchw", es.onnx_style(3, 16, c0=8, layout="nchw")), ("layout_ops", layout_ops())):
        rs = np.random.RandomState(7)
        orig = np.frombuffer(blob, np.uint8)
        head = 16000   # the synthetic writer puts the tables of the tensors and operators in front of the constants: two mutations in three go there
        unmutated = str(tmp_path / (name + ".bin"))
        open(unmutated, "wb").write(blob)
        blobs.append(unmutated)
        for r in range(150):
            b = orig.copy()
            hi = len(b) if r % 3 == 0 else min(len(b), head)
            for _ in range(rs.randint(1, 6)):
                b[rs.randint(0, hi)] = rs.randint(0, 256)
            f = str(tmp_path / ("%s_%03d.bin" % (name, r)))
            open(f, "wb").write(b.tobytes())
            blobs.append(f)
    r = subprocess.run([exe] + blobs, capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    ok, refused, packed, unpacked, band_ready, band_none, band_threw, planned, lowered, lower_threw = (int(v) for v in r.stdout.split()[1::2])
    print(r.stdout)
    assert ok + refused == 2 * len(blobs)
    assert ok >= 6 and refused > 100         # the three graphs as they are lower at both levels; mutations are refused, or lower
    assert packed + unpacked == ok and lowered + lower_threw == 2 * packed and lowered >= 12
