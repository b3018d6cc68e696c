"""Engine option "conv_bf16" through the host side (no GPU): the bf16 planes the packer appends (bit for bit against numpy's round to nearest
even), the blob at value 0, the launch labels of the host-only lowering, the derived bound's power to tell a wrong rounding from the right one,
the new kernel's registers and LDS, and FaceEmbeddings' precision argument."""
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_bf16_ref as cb
import resnet_synth as rs
from conftest import MODEL_FILES, ROOT, model_path
from synth_tflite import VALID

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/conv_bf16_consts_dump.cpp linked against the product's host objects, the way test_resnet_cpu.py builds its driver"""
    tmp = tmp_path_factory.mktemp("conv_bf16_dump")
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    o, exe = str(tmp / "conv_bf16_consts_dump.o"), str(tmp / "conv_bf16_consts_dump")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "conv_bf16_consts_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    run.tmp = tmp
    return run


def packed(dump, name, blob, value, fuse=5):
    """-> (default_equal, [conv record]): record = dict(shape, wrows, hi, lo offsets, w / hi / lo arrays where printed)"""
    path = dump.tmp / (name + ".tflite")
    path.write_bytes(blob)
    lines = dump("consts", path, fuse, value)
    head = lines[0].split()
    assert head[0] == "blob" and head[2] == "default_equal", lines[0]
    convs = []
    for line in lines[1:]:
        tag, rest = line.split(" ", 1)
        if tag == "conv":
            f = rest.split()
            convs.append(dict(shape=tuple(int(v) for v in f[1:5]), wrows=int(f[6]), hi_off=int(f[8]), lo_off=int(f[10])))
        elif tag == "w":
            convs[-1]["w"] = np.array([int(v, 16) for v in rest.split()], np.uint32).view(np.float32)
        else:
            assert tag in ("hi", "lo"), line
            convs[-1][tag] = np.array([int(v, 16) for v in rest.split()], np.uint16)
    return int(head[3]) == 1, convs


INSIDE = {
    "a_7x7x32_to_32": dict(h=7, w=7, c=32, co=32),
    "b_14x14x64_to_128_s2": dict(h=14, w=14, c=64, co=128, stride=2),
    "c_9x11x96_to_36": dict(h=9, w=11, c=96, co=36),
    "k5_6x6x32_to_32": dict(h=6, w=6, c=32, co=32, k=5),
}
OUTSIDE = {
    "g_c24": dict(h=7, w=7, c=24, co=32),
    "e_2x2_s2": dict(h=8, w=8, c=32, co=64, k=2, stride=2, padding=VALID),
    "whole_frame_head": dict(h=3, w=3, c=32, co=8, k=3, padding=VALID),
}


def check_planes(conv, value):
    assert conv["wrows"] >= 0 and "w" in conv
    if value == 0:
        assert conv["hi_off"] < 0 and conv["lo_off"] < 0 and "hi" not in conv and "lo" not in conv, conv
        return
    w = conv["w"]
    assert conv["hi_off"] >= 0 and conv["hi"].shape == w.shape
    np.testing.assert_array_equal(conv["hi"], cb.bf16_bits(w))
    if value == 2:
        hi, lo = cb.split_bf16(w)
        np.testing.assert_array_equal(cb.bf16_value(conv["hi"]), hi)
        np.testing.assert_array_equal(conv["lo"], cb.bf16_bits(lo))
        assert conv["lo_off"] > conv["hi_off"]
        # the split is worth something: hi + lo is w to 2^-16 or better, and lo is not all zeros
        assert np.abs(w.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)).max() <= 2.0 ** -16 * np.abs(w).max() and conv["lo"].any()
    else:
        assert conv["lo_off"] < 0 and "lo" not in conv


@pytest.mark.parametrize("value", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(INSIDE))
def test_planes_of_a_single_layer_are_numpys_rounding(dump, name, value):
    blob, cs = rs.conv_layer(7, **INSIDE[name])
    same, convs = packed(dump, name, blob, value)
    assert same == (value == 0)     # value 0: the one-argument call's blob, byte for byte
    assert len(convs) == 1
    np.testing.assert_array_equal(convs[0]["w"], cs["w"].reshape(-1))
    check_planes(convs[0], value)


@pytest.mark.parametrize("value", [0, 1, 2])
def test_planes_of_the_network(dump, value):
    blocks = (1, 1, 1, 1)
    same, convs = packed(dump, "iresnet", rs.iresnet_like(3, 128, blocks=blocks), value)
    assert same == (value == 0)
    with_rows = [c for c in convs if c["wrows"] >= 0]
    assert len(with_rows) == 2 * sum(blocks)   # the 3x3 convolutions of the blocks: not the stem (C = 3), the 1x1 shortcuts or the head
    for c in convs:
        if c["wrows"] >= 0:
            assert c["shape"][1:3] == (3, 3) and c["shape"][3] % 32 == 0
            check_planes(c, value)
        else:
            assert c["hi_off"] < 0 and c["lo_off"] < 0, c


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_a_convolution_outside_the_rule_has_no_plane(dump, name):
    blob, _ = rs.conv_layer(8, **OUTSIDE[name])
    for value in (0, 1, 2):
        for fuse in (0, 5):
            same, convs = packed(dump, name, blob, value, fuse)
            assert same                         # nothing is appended: the blob is the default one at every value
            assert len(convs) == 1 or (fuse == 5 and not convs)   # (from level 2 on the 2x2 stride-2 step is a stage program, no Conv node)
            for c in convs:
                assert c["wrows"] < 0 and c["hi_off"] < 0 and c["lo_off"] < 0, c


def launch_lines(dump, path, value, F, fuse=5):
    return dump("launches", path, fuse, value, F)


def test_launch_labels_of_the_network(dump):
    blocks = (2, 1, 1, 1)
    path = dump.tmp / "iresnet_2111.tflite"
    path.write_bytes(rs.iresnet_like(4, 512, blocks=blocks))
    for F in (1, 5):
        at0 = launch_lines(dump, path, 0, F)
        labels0 = [l.split()[0] for l in at0]
        assert labels0.count("conv_mfma_kernel") == 2 * sum(blocks) and "conv_bf16_kernel" not in labels0 and all(l.endswith("bf16=0") for l in at0)
        for value in (1, 2):
            at = launch_lines(dump, path, value, F)
            labels = [l.split()[0] for l in at]
            assert labels.count("conv_bf16_kernel") == 2 * sum(blocks) and "conv_mfma_kernel" not in labels, labels
            assert len(at) == len(at0)
            for l0, l in zip(at0, at):
                if l.split()[0] == "conv_bf16_kernel":
                    assert l0.split()[0] == "conv_mfma_kernel" and l.endswith("bf16=1") and l0.split()[1:4] == l.split()[1:4], (l0, l)
                else:
                    assert l == l0   # nothing else in the plan changes


@pytest.mark.parametrize("name", sorted(MODEL_FILES))
def test_shipped_graphs_lower_the_same_at_every_value(dump, name):
    for fuse, F in ((5, 1), (5, 32), (2, 4)):
        at0 = launch_lines(dump, model_path(name), 0, F, fuse)
        assert len(at0) >= 1 and "conv_bf16_kernel" not in " ".join(at0)
        for value in (1, 2):
            assert launch_lines(dump, model_path(name), value, F, fuse) == at0


# ---------------------------------------------------------------------------------------------------- the bound tells right from wrong
def _patches_case_a(x):
    """[49, 288] windows of a 7x7x32 frame, 3x3 SAME, in (ky, kx, c) order"""
    xp = np.zeros((9, 9, 32), x.dtype)
    xp[1:8, 1:8] = x
    return np.stack([xp[oy:oy + 3, ox:ox + 3].reshape(-1) for oy in range(7) for ox in range(7)])


def test_the_mode_1_bound_refuses_truncated_operands():
    """case a's shape (7x7x32 -> 32, K = 288): operands truncated to bf16 instead of rounded leave the mode-1 bound on more than half of the
    elements; the rounded operands accumulated in f32 in the kernel's order (k ascending) stay far inside it."""
    blob, cs = rs.conv_layer(200, h=7, w=7, c=32, co=32)
    x = np.random.RandomState(300).standard_normal((1, 7, 7, 32)).astype(np.float32)
    ref, bound = cb.layer_ref(x, cs, 1)
    ref, bound = ref.reshape(49, 32), bound.reshape(49, 32)
    w = cs["w"].reshape(32, 288)
    # wrong: truncation, evaluated exactly
    wrong = _patches_case_a(cb.trunc_bf16(x[0]).astype(np.float64)) @ cb.trunc_bf16(w).astype(np.float64).T + cs["b"].astype(np.float64)
    ratio = np.abs(wrong - ref) / bound
    print("truncated operands: %.1f %% of the elements beyond the bound at F = %g, median ratio %.1f" % (100 * (ratio > 1).mean(), cb.F, float(np.median(ratio))))
    assert (ratio > 1).mean() > 0.5
    # right: round to nearest even, accumulated in f32 one k after the other
    a, b = _patches_case_a(cb.rne_bf16(x[0])), cb.rne_bf16(w)
    acc = np.zeros((49, 32), np.float32)
    for k in range(288):
        acc += a[:, k:k + 1] * b[None, :, k]
        assert acc.dtype == np.float32
    right = acc + cs["b"]
    ratio = np.abs(right.astype(np.float64) - ref) / bound
    print("rounded operands, f32 accumulation: worst ratio %.4f" % float(ratio.max()))
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------------------------------------------- ISA
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv_bf16_instantiations_do_not_spill(tmp_path):
    """tools/isa_report.py on conv_bf16_kernels.hip: the four instantiations launch_conv_bf16 launches, without scratch, at two waves per SIMD or
    better, LDS within a quarter of the CU's, each with the bf16 MFMA and the packed conversion in its code"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    out = str(tmp_path / "conv_bf16.s")
    isa_report.compile_asm(os.path.join(isa_report.CSRC, "conv_bf16_kernels.hip"), out)
    ks = {k["pretty"]: k for k in isa_report.kernels(out)}
    assert sorted(ks) == sorted("conv_bf16_kernel<%d, %s>" % (tn, s) for tn in (64, 128) for s in ("false", "true")), sorted(ks)
    text = open(out).read()
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 256 and k["lds"] <= 40 * 1024, (name, k)
        start = text.index("\n%s:" % k["name"])
        body = text[start:text.index("s_endpgm", start)]
        assert "v_mfma_f32_32x32x16_bf16" in body and "v_cvt_pk_bf16_f32" in body, name
        # per loop body: 2 k-steps a chunk x 2 x TN / 64 tiles a wave; three MFMAs for one in the split form, two chunks a body in the plain form
        split = name.endswith("true>")
        assert body.count("v_mfma_f32_32x32x16_bf16") == (3 if split else 2) * 2 * 2 * (int(name.split("<")[1].split(",")[0]) // 64), name


def test_face_embeddings_refuses_an_unknown_precision(mi):
    with pytest.raises(ValueError):
        mi.FaceEmbeddings(model_bytes=b"", precision="fp8")
    with pytest.raises(ValueError):
        mi.FaceEmbeddings(model_path="/nonexistent.tflite", precision="")
