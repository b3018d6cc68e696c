"""The single-launch plan that bandplan.cpp makes of the shipped models and of the synthetic graphs, against pins.  CPU only: the planner is
host code, linked here (host side of hipcc) against the product's objects the way test_const_pins.py links its driver.

The pins (tests/golden/band_plan_pins.json) were made from the code this planner replaced, not from the planner: Model::build_bandnet and
Model::build_bandnet_try were compiled unchanged as members of a struct with the same member names, with host stand-ins for hipMalloc /
hipMemcpy / hipMemset / hipHostMalloc and 256 compute units, and what they uploaded and stored was printed by tests/bandplan_dump.cpp's own
printing code (a graph they left without a plan: an empty plan)."""
import json
import os
import subprocess

import pytest

import synth_tflite
from conftest import MODELS, ROOT

CSRC = os.path.join(ROOT, "rs-face-detection-tflite_amd", "csrc")
DEFAULTS, NARROW = "opt_nw=128 opt_wide=1 opt_fork=1", "opt_nw=128 opt_wide=0 opt_fork=1"


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


def test_single_launch_plans_match_their_pins(tmp_path, synth_models):
    build = os.path.join(ROOT, "rs-face-detection-tflite_amd", "build")
    objs = sorted(os.path.join(build, n) for n in os.listdir(build) if n.endswith(".o"))
    assert len(objs) >= 15, "build the product first (__graft_entry__.build())"
    hipcc = "/opt/rocm/bin/hipcc"
    o = str(tmp_path / "bandplan_dump.o")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-x", "hip", "-c", os.path.join(ROOT, "tests", "bandplan_dump.cpp"), "-o", o], stderr=subprocess.DEVNULL)
    exe = str(tmp_path / "bandplan_dump")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, o] + objs, stderr=subprocess.DEVNULL)
    models = sorted(n for n in os.listdir(MODELS) if n.endswith(".tflite"))
    assert len(models) == 7
    got = {}
    # the shipped models under all five option rows, the synthetic graphs under the two that test_synthetic_graphs_on_the_single_launch_plan sets
    for rows, files in ((5, [os.path.join(MODELS, n) for n in models]), (2, [synth_models[c][0] for c in sorted(synth_models)])):
        r = subprocess.run([exe, str(rows)] + files, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        for line in r.stdout.splitlines():
            t = line.split()
            got[" ".join(t[:4])] = dict(x.split("=") for x in t[4:])
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "band_plan_pins.json")))
    assert len(pins) == 7 * 5 + 2 * len(synth_tflite.CASES) and sorted(got) == sorted(pins)
    for cfg in sorted(pins):
        assert len(pins[cfg]) == 17
        for field in sorted(pins[cfg]):
            assert got[cfg].get(field) == pins[cfg][field], (cfg, field, got[cfg].get(field), pins[cfg][field])
    # in the clear: every shipped model has a single-launch program at the defaults, of the stage counts DESIGN.md names
    for n in models:
        assert got[n + " " + DEFAULTS]["ready"] == "1", n
    stages = {"face_detection_back.tflite": 36, "face_detection_front.tflite": 20, "face_detection_short_range.tflite": 20,
              "face_detection_full_range.tflite": 48, "face_landmark.tflite": 22}
    for n, k in stages.items():
        assert got[n + " " + DEFAULTS]["nstages"] == str(k), n
    assert got["face_detection_full_range.tflite " + NARROW]["nstages"] == "17"
