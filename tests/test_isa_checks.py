"""Build-time checks on the gfx950 ISA of the kernels that live at the register limit (mrow.hpp's LDS reads and their
waits are separate asm statements, correct only while the compiler neither spills nor copies the values in between).  Cross-compiles
the sources to assembly (no GPU needed) and reads the kernel descriptors: no scratch, no spilled VGPRs."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402

# file -> (extra flags as in build.sh, kernels that must not use scratch: substring filter, "" = every kernel of the file)
CASES = {
    "mstrip_kernels.hip": (["-fno-slp-vectorize"], [""]),
    "mwalk_kernels.hip": (["-fno-slp-vectorize"], [""]),
    "ms2_kernels.hip": (["-fno-slp-vectorize"], [""]),
    "mdblock_kernels.hip": (["-fno-slp-vectorize"], [""]),
    # round 5: the stage programs with several frames per workgroup — both register variants spill-free (a version with spills ran 15 % slower),
    # and the 128-register variant really is one: two workgroups per CU depend on it
    "tail_kernels.hip": ([], [""]),
    # round 5: the single-launch plan — one workgroup per CU, 256 registers a lane available, none of them in scratch
    "bandnet_kernels.hip": ([], [""]),
    # the strip kernels and the row pipelines of BASELINE config 2 (four stages, 24 channels, plain and with either stride-2 tail), all four
    # forms: they share the frame functions of strip_kernels.hip, so a change to one of those is a change to every kernel
    "strip_kernels.hip": (["-DMI_DEV_ONE"], [""]),
    # the first convolution, all three forms: the two MFMA forms share what a wave holds and does per picture row (StemWave), so a change to
    # that is a change to both
    "stem_kernels.hip": ([], [""]),
}


def _compile(item):
    name, (flags, _) = item
    out = os.path.join("/tmp", "isa_check_%d_%s.s" % (os.getpid(), name))
    isa_report.compile_asm(os.path.join(isa_report.CSRC, name), out, flags)
    ks = isa_report.kernels(out)
    os.unlink(out)
    return name, ks


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_register_limit_kernels_do_not_spill():
    with ThreadPoolExecutor(max_workers=3) as ex:
        results = dict(ex.map(_compile, CASES.items()))
    for name, (_, filters) in CASES.items():
        ks = results[name]
        assert ks, name
        for f in filters:
            sel = [k for k in ks if f in k["pretty"]]
            assert sel, (name, f)
            for k in sel:
                # (bandnet_kernel runs at the limit of the scalar register file: hipcc keeps nine scalars in lanes of a vector register and
                # reserves a 20-byte private segment for them that no instruction of the kernel touches)
                unused_reserve = name == "bandnet_kernels.hip" and k["scratch"] <= 32 and k["scratch_ops"] == 0
                assert (k["scratch"] == 0 or unused_reserve) and k["vspill"] == 0, (name, k["pretty"], k["vgpr"], k["vspill"], k["scratch"], k["scratch_ops"])
                assert k["vgpr"] + k["agpr"] <= 256, (name, k["pretty"])      # two waves per SIMD
                if name == "mdblock_kernels.hip" and "mdblock_kernel<MD<4, 4, 1, 2, 3," in k["pretty"]:
                    assert k["vgpr"] + k["agpr"] <= 168, (name, k["pretty"], k["vgpr"])   # the face mesh's block pair (with and without the first convolution in front): three waves per SIMD, four workgroups per CU
                if k["pretty"].startswith(("strip_kernel<4,", "strip_kernel<6,")):
                    assert k["vgpr"] + k["agpr"] <= 168, (name, k["pretty"], k["vgpr"])   # their launch bound: three waves per SIMD
                if k["pretty"].startswith("mi::stem_mfma_kernel<"):
                    assert k["vgpr"] + k["agpr"] <= 256, (name, k["pretty"], k["vgpr"], k["agpr"])   # launch_stem_mfma runs it at two workgroups of four waves per CU: two waves per SIMD
                if "tail_kernel<false>" in k["pretty"]:
                    assert k["vgpr"] + k["agpr"] <= 128, (name, k["pretty"], k["vgpr"])   # four waves per SIMD
