"""The constant blob, the stage programs and every offset table that consts.cpp packs for the shipped models, against pins.  CPU only: the
packer is host code, linked here (host side of hipcc) against the product's objects the way test_lowering_asan.py links its driver.

The pins (tests/golden/const_blob_pins.json) were made from the code this packer replaced, not from the packer: the lines of the former
Model::rebuild() that packed the blob and resolved the programs were compiled unchanged as a function of their own, with host stand-ins for
hipMalloc / hipMemcpy, and what they uploaded was hashed by tests/consts_dump.cpp's own printing code.  The former code had two slots with
several meanings, which were mapped onto today's fields by the kind of node: node_mwalk_ of a Chain node became node_chain_pair (of any other
node: node_mwalk); MemberOff::strip became strip for the members of a Chain node, cblob for the stages of an xc node and for the first block
of a dblock / bneck pair, and mconsts for the second block of such a pair."""
import json
import os
import subprocess

from conftest import MODELS, ROOT

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")


def test_packed_constants_of_the_shipped_models_match_their_pins(tmp_path):
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    hipcc = "/opt/rocm/bin/hipcc"
    o = str(tmp_path / "consts_dump.o")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "consts_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    exe = str(tmp_path / "consts_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)
    models = sorted(n for n in os.listdir(MODELS) if n.endswith(".tflite"))
    assert len(models) == 7
    r = subprocess.run([exe] + [os.path.join(MODELS, n) for n in models], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        t = line.split()
        got[" ".join(t[:3])] = dict(x.split("=") for x in t[3:])
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "const_blob_pins.json")))
    assert len(pins) == 7 * 6 and sorted(got) == sorted(pins)
    for cfg in sorted(pins):
        assert len(pins[cfg]) == 21
        for field in sorted(pins[cfg]):
            assert got[cfg].get(field) == pins[cfg][field], (cfg, field, got[cfg].get(field), pins[cfg][field])
