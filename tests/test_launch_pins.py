"""The launch list that launches.cpp makes of a chunk (which kernel runs for which plan node, with which arguments, on which stream, behind which
event), for the shipped models and the synthetic graphs, against pins.  CPU only: the lowering is host code, linked here (host side of hipcc)
against the product's objects the way test_band_pins.py links its driver.

The pins (tests/golden/launch_pins.json) were made from the code this module replaced, not from the module: Model::enqueue_chunk, Model::node_label,
Model::tensor_ptr / tensor_ptr_mut and Model::schedule_side_streams were compiled unchanged as members of a struct with the same member names, with
launch_* / record_event / wait_event renamed by macros to recorders that noted the launcher, the argument struct, the stream and the events, and
the swallowed nodes were read off the labels the old function gave them; that list was printed by tests/launches_dump.cpp's own printing code.
The rows at the defaults are kept in the clear, every other row as a hash of the same lines (the whole text is over a megabyte)."""
import hashlib
import json
import os
import re
import subprocess

import pytest

import synth_tflite
from conftest import MODELS, ROOT

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
FRAMES = (1, 4, 5, 16, 17, 31, 32)
ROWS = ("defaults", "strip=0", "pair_fuse=0", "stem_fuse=0", "mchain=0", "small_chain=0", "stem_mfma=0", "fork=0", "heads=4", "lanes=2", "fuse=2")
MESH, BACK, IRIS = "face_landmark.tflite", "face_detection_back.tflite", "iris_landmark.tflite"


def pinned(cfg, lines):
    """A configuration as the pin file keeps it: the lines themselves at the defaults, else their hash."""
    return lines if cfg.split()[1] == "defaults" else hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def parse(stdout):
    got, cur = {}, None
    for line in stdout.splitlines():
        if line.startswith("== "):
            cur = got.setdefault(line[3:], [])
        else:
            cur.append(line)
    return got


def labels(lines):
    return [re.search(r'"(.*)"', line).group(1) for line in lines if '"' in line]


@pytest.fixture(scope="module")
def synth_models(tmp_path_factory):
    """The synthetic graphs of tests/synth_tflite.py written out as .tflite files (as test_gpu_parity.py's fixture of the same name)."""
    d = tmp_path_factory.mktemp("synth")
    out = {}
    for name, (make, h, w) in synth_tflite.CASES.items():
        p = d / (name + ".tflite")
        p.write_bytes(make())
        out[name] = (str(p), h, w)
    return out


@pytest.fixture(scope="module")
def lowered(tmp_path_factory, synth_models):
    """Every configuration's launch list, as launches_dump prints it."""
    tmp = tmp_path_factory.mktemp("launches_dump")
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    hipcc = "/opt/rocm/bin/hipcc"
    o = str(tmp / "launches_dump.o")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "launches_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    exe = str(tmp / "launches_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)
    models = sorted(n for n in os.listdir(MODELS) if n.endswith(".tflite"))
    assert len(models) == 7
    got = {}
    for which, files in (("shipped", [os.path.join(MODELS, n) for n in models]), ("synth", [synth_models[c][0] for c in sorted(synth_models)])):
        r = subprocess.run([exe, which] + files, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got.update(parse(r.stdout))
    return models, got


def test_launch_lists_match_their_pins(lowered):
    models, got = lowered
    # the set of configurations is complete: every shipped model under every option row at every frame count on either side of a batch-dependent
    # rule, the single-launch plan at 1 and 4 frames, the u8 input form; every synthetic graph at the defaults and at fuse level 2
    want = {"%s %s F=%d" % (m, row, f) for m in models for row in ROWS for f in FRAMES}
    want |= {"%s band=2 F=%d" % (m, f) for m in models for f in (1, 4)} | {"%s u8 F=%d" % (m, f) for m in models for f in (1, 32)}
    want |= {"%s.tflite %s F=%d" % (c, row, f) for c in synth_tflite.CASES for row in ("defaults", "fuse=2") for f in (1, 32)}
    assert set(got) == want and len(want) == 7 * (11 * 7 + 2 + 2) + 4 * len(synth_tflite.CASES)
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_pins.json")))
    assert set(pins) == want
    for cfg in sorted(pins):
        assert not any(line.startswith("threw") for line in got[cfg]), (cfg, got[cfg])
        assert pinned(cfg, got[cfg]) == pins[cfg], (cfg, got[cfg], pins[cfg])
    # every shipped model's first convolution has the u8 form (takes_u8_input): the u8 rows hold a launch list each
    assert not [m for m in models if got[m + " u8 F=1"] == ["no u8 input form"]]


def test_selection_facts_in_the_clear(lowered):
    """What the GPU tests state through profile() labels, seen on the CPU."""
    _, got = lowered
    mesh32 = labels(got[MESH + " defaults F=32"])
    assert mesh32[:4] == ["mdblock_kernel<stem+pair>", "ms2_kernel<4,2,3>", "mdblock_kernel<pair>", "ms2_kernel<8,4,2>"]
    unfused = labels(got[MESH + " stem_fuse=0 F=32"])
    assert unfused[0].startswith("stem_conv_kernel") and unfused[1] == "mdblock_kernel<pair>"
    mstrip = [k for k in labels(got[BACK + " defaults F=32"]) if k.startswith("mstrip")]
    assert len(mstrip) == 1 and mstrip[0].startswith("mstrip_chain_kernel")
    assert sum(k.startswith("mstrip_kernel") for k in labels(got[BACK + " mchain=0 F=32"])) == 7
    assert "mbneck_kernel" in labels(got[IRIS + " defaults F=32"])
    assert "mbneck_kernel" not in labels(got[IRIS + " defaults F=31"])
