"""The launch sequence of one teacher step is fixed: the complete {profiler class: launches} map of optimizer step 0
(igi_prof_read, full names, nothing filtered) for every case of tests/teacher_step_cases.py, unsplit (phase -1) and as the
two phases of the data-parallel step, the default-network cases under both settings of igi_teacher_set_latz_fuse.
tests/golden/teacher_step_launches.json was recorded before teacher_fwd_bwd was cut into stages:
    python tests/test_gpu_teacher_step_launches.py > tests/golden/teacher_step_launches.json
The cut csrc/teacher.h documents is asserted too: both phases together launch exactly the kernels of the unsplit step plus
the second k_slab_reduce."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "teacher_step_launches.json")

from tests import teacher_step_cases as K   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = K.step_cases()
KEYS = [(name, latz) for name, c in CASES.items() for latz in ((1, 0) if c["default_net"] else (1,))]


def _key(name, latz):
    return name if latz else name + " latz_fuse=0"


def _launches(eng, phase):
    import torch
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        if phase < 0:
            eng.fwd_bwd(0, 0)
        else:
            eng.fwd_bwd_phase(0, 0, phase)
        torch.cuda.synchronize()
        return {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)


def record(name, latz):
    """{"whole": map of phase -1, "phase0": ..., "phase1": ...} of optimizer step 0"""
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    prev = L.igi_teacher_set_latz_fuse(latz)
    try:
        eng, ro = K.make_engine(CASES[name])
        eng.prepare(ro)
        return {"whole": _launches(eng, -1), "phase0": _launches(eng, 0), "phase1": _launches(eng, 1)}
    finally:
        L.igi_teacher_set_latz_fuse(prev)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(_key(*k) for k in KEYS)
    return want


@pytest.mark.parametrize("name,latz", KEYS, ids=[_key(*k) for k in KEYS])
def test_step_launches_equal_the_recording(name, latz, golden):
    got = record(name, latz)
    print(json.dumps(got, indent=1))
    both = dict(got["phase0"])
    for k, v in got["phase1"].items():
        both[k] = both.get(k, 0) + v
    whole = dict(got["whole"])
    whole["k_slab_reduce"] = whole.get("k_slab_reduce", 0) + 1
    assert both == whole
    assert got == golden[_key(name, latz)]


if __name__ == "__main__":
    print(json.dumps({_key(*k): record(*k) for k in KEYS}, indent=0))
