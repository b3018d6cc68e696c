"""ResNet-style embedding graphs through the host side (no GPU): FULLY_CONNECTED, MUL and ADD by per-channel constants in the reader and the
lowering.  The synthetic network of tests/resnet_synth.py lowers at every fusion level with its FULLY_CONNECTED as the whole-frame head and
its batch normalisations folded where the rule allows; the oracle evaluates the network's twin; graphs outside the rule are refused with a
message that names the operator; and the fold is restated in float64 against the constants the packer uploads."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import resnet_synth as rs
from conftest import ROOT

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
LINE = re.compile(r"^(\w+)((?:\+[\w()]+)*) t(\d+)\[[^\]]*\] -> t(\d+)\[")


def nodes_of(text):
    """(kind, suffixes like '+prelu+skip', input tensor, output tensor) per plan node"""
    out = []
    for line in text.splitlines()[1:]:
        m = LINE.match(line)
        assert m, line
        out.append((m.group(1), m.group(2), int(m.group(3)), int(m.group(4))))
    return out


@pytest.mark.parametrize("seed,features,blocks", [(3, 128, (1, 1, 1, 1)), (4, 512, (2, 1, 1, 1))])
def test_the_network_lowers_with_its_head_and_its_folded_normalisations(mi, seed, features, blocks):
    blob = rs.iresnet_like(seed, features, blocks=blocks)
    for fuse in (0, 2, 4, 5):
        text = mi.plan_describe(blob, fuse)   # (the parent commit: "plan: builtin operator 9 unsupported")
        assert "k7x7" in text and ("GEMM over the batch" in text) == (fuse >= 2), text   # the FULLY_CONNECTED as the whole-frame head
        nodes = nodes_of(text)
        assert sum(kind == "affine" for kind, *_ in nodes) == rs.affine_launches(blocks, fuse), text
        if fuse == 0:
            continue   # one launch per operator: nothing folds
        # no affine remains behind a convolution that has no activation, no skip, and nobody else reading it
        producer = {out: (kind, sfx) for kind, sfx, _, out in nodes}
        readers = {}
        for _, _, src, _ in nodes:
            readers[src] = readers.get(src, 0) + 1
        for kind, _, src, _ in nodes:
            if kind == "affine" and src in producer:
                pk, psfx = producer[src]
                assert not (pk in ("conv", "dw") and psfx == "" and readers[src] == 1), (src, text)
        # every convolution behind a normalisation carries it: 3 per block + the stem + the head, in launches of their own
        assert sum(kind == "conv" for kind, *_ in nodes) == 1 + 2 * sum(blocks) + len(blocks) + 1, text


def test_the_oracle_runs_the_twin(oracle, tmp_path):
    path = tmp_path / "twin.tflite"
    path.write_bytes(rs.iresnet_like(3, 128, twin=True))
    x = np.random.RandomState(1).uniform(0, 1, (2, 112, 112, 3)).astype(np.float32)
    out = oracle.Model(str(path)).run(x)
    assert len(out) == 1 and out[0].reshape(2, -1).shape == (2, 128)
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 1e-3


def _fc_graph(**kw):
    g = rs.ResnetBuilder(5, [1, 4, 4, 8])
    g.outputs = [g.fc(g.reshape(g.input, [1, 128]), 16, **kw)]
    return g.finish()


def _mul_two_activations():
    g = rs.ResnetBuilder(6, [1, 4, 4, 8])
    g.outputs = [g.mul(g.input, g.prelu(g.input))]
    return g.finish()


def _mul_by_a_frame():
    g = rs.ResnetBuilder(7, [1, 4, 4, 8])
    g.outputs = [g.mul_const(g.input, g.rng.uniform(0.5, 1.5, (4, 4, 8)).astype(np.float32))]
    return g.finish()


REFUSALS = {
    "fc_weights_format_1": (lambda: _fc_graph(weights_format=1), ("FULLY_CONNECTED", "weights_format")),
    "fc_k_does_not_match_its_input": (lambda: _fc_graph(k=136), ("FULLY_CONNECTED", "136", "128")),
    "mul_of_two_activations": (_mul_two_activations, ("MUL", "two activations")),
    "mul_by_an_hwc_constant": (_mul_by_a_frame, ("MUL", "per-channel")),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_graphs_outside_the_rule_are_refused_by_name(mi, name):
    make, words = REFUSALS[name]
    for fuse in (0, 5):
        with pytest.raises(mi.MiError) as e:
            mi.plan_describe(make(), fuse)
        assert all(w in str(e.value) for w in words), str(e.value)


def test_accepted_forms_lower(mi):
    """either operand order, a scalar constant, a FULLY_CONNECTED on a rank-2 tensor that no RESHAPE made (1x1 on [1,1,1,K]), a fused RELU"""
    g = rs.ResnetBuilder(8, [1, 4, 4, 8])
    x = g.add_const(g.mul_const(g.input, const_first=True), np.float32([0.25]), const_first=True)
    y = g.fc(g.reshape(x, [1, 128]), 24, act=1)
    g.outputs = [g.fc(y, 8)]
    text = mi.plan_describe(g.finish(), 5)
    kinds = [n[0] + n[1] for n in nodes_of(text)]
    # (the second FULLY_CONNECTED is a 1x1 convolution on [1,1,1,24]: from level 2 on those run on the block kernel, "pointwise")
    assert kinds == ["affine", "conv+relu", "reshape", "reshape", "block", "reshape"], text
    assert "k4x4" in text and "t15[1x1x24] -> t17[1x1x8] pointwise" in text, text
    assert "[1x1x24] -> t17[1x1x8] k1x1" in mi.plan_describe(g.finish(), 1)


def test_odd_channel_counts_are_widened_through_an_affine(mi):
    blob = rs.odd_width_graph(10)
    narrow, wide = mi.plan_describe(blob, 0), mi.plan_describe(blob, 5)
    assert "affine" in narrow and "x30]" in narrow and "x32]" not in narrow, narrow
    affine = [line for line in wide.splitlines() if line.startswith("affine")]
    assert len(affine) == 1 and "[8x8x32] -> " in affine[0] and "x30]" not in wide, wide


def test_the_fold_is_w_times_s_and_b_times_s_plus_t_rounded_once(tmp_path):
    """conv -> MUL -> ADD: the constants the packer uploads for the convolution (read back the way tests/test_const_pins.py reads packed
    constants: a driver linked against the product's host objects) are w s and b s + t, computed in float64 and rounded once."""
    blob, w, b, s, t = rs.fold_graph(9)
    model = tmp_path / "fold.tflite"
    model.write_bytes(blob)
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    hipcc = "/opt/rocm/bin/hipcc"
    o = str(tmp_path / "resnet_consts_dump.o")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "resnet_consts_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    exe = str(tmp_path / "resnet_consts_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)

    def packed(fuse):
        lines = subprocess.run([exe, str(model), str(fuse)], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
        assert len(lines) == 3 and lines[0] == "conv %d %d" % (w.shape[0], w[0].size), lines[:1]
        words = lambda line, tag: np.array([int(v, 16) for v in line.split()[1:]], np.uint32).view(np.float32) if line.startswith(tag + " ") else None
        return words(lines[1], "w"), words(lines[2], "b")

    w64, b64, s64, t64 = (v.astype(np.float64) for v in (w, b, s, t))
    want_w = (w64.reshape(w.shape[0], -1) * s64[:, None]).astype(np.float32).reshape(-1)
    want_b = (b64 * s64 + t64).astype(np.float32)
    assert (want_w != w.reshape(-1)).mean() > 0.9   # the case is one: the scale changes nearly every weight
    for fuse in (1, 5):
        got_w, got_b = packed(fuse)
        np.testing.assert_array_equal(got_w, want_w)
        np.testing.assert_array_equal(got_b, want_b)
    got_w, got_b = packed(0)   # one launch per operator: the convolution keeps its own constants
    np.testing.assert_array_equal(got_w, w.reshape(-1))
    np.testing.assert_array_equal(got_b, b)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_conv_mfma_instantiations_do_not_spill(tmp_path):
    """tools/isa_report.py on conv_mfma_kernels.hip: both tiles without scratch, at two waves per SIMD or better, their LDS within a quarter of the CU's"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    out = str(tmp_path / "conv_mfma.s")
    isa_report.compile_asm(os.path.join(isa_report.CSRC, "conv_mfma_kernels.hip"), out)
    ks = {k["pretty"]: k for k in isa_report.kernels(out)}
    assert sorted(ks) == ["conv_mfma_kernel<128>", "conv_mfma_kernel<64>"], sorted(ks)
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 256 and k["lds"] <= 40 * 1024, (name, k)
