"""The student's launch plans are fixed: the workspace-size entries (no GPU needed) expose the split factors, tile heights
and the fused soft-argmax of the tactile plan (igi_tactile_workspace_bytes) and the rows per split of the Linear weight
gradients (igi_linear_workspace_bytes, igi_mlp_workspace_bytes).  tests/golden/student_plans.json is their value over the
sweep below, recorded before the A/B switches that used to move them were retired, with nothing set:
    python tests/test_student_plans_cpu.py > tests/golden/student_plans.json
At that commit each of IGI_CONV_TALL=0, IGI_CONV_BM192=0, IGI_SSA_FUSE=0, IGI_LIN_SK_ROWS=256 and IGI_TAC_SK=3,5,7 alone
changed at least one value of the sweep."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "student_plans.json")

TACTILE_BATCH = (32, 64, 96, 512, 2048, 6144, 8192, 16384, 32768)
TACTILE_HW = (32, 64, 224)
LINEAR_ROWS = (32, 100, 2048, 8192, 65536)
LINEAR_IN_OUT = ((24, 256), (256, 128), (512, 512), (128, 32))
# the student's Linear chains: lin_encoder, compress_pcl_enc (two objects), output layers + latent predictor
MLP_CHAINS = ((24, 64, 32), (512, 64, 32), (128, 32, 64, 32, 8))
RETIRED = {"IGI_CONV_TALL": "0", "IGI_CONV_BM192": "0", "IGI_SSA_FUSE": "0", "IGI_LIN_SK_ROWS": "256", "IGI_TAC_SK": "3,5,7"}


def plan_table():
    sys.path.insert(0, ROOT)
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    t = {}
    for b in TACTILE_BATCH:
        for hw in TACTILE_HW:
            cfg = _lib.TactileCfg(b, hw, hw, 16)
            t[f"tactile {b} {hw}x{hw}"] = int(L.igi_tactile_workspace_bytes(C.byref(cfg)))
    for rows in LINEAR_ROWS:
        for i, o in LINEAR_IN_OUT:
            t[f"linear {rows} {i}->{o}"] = int(L.igi_linear_workspace_bytes(rows, i, o))
        for dims in MLP_CHAINS:
            t[f"mlp {rows} {'-'.join(map(str, dims))}"] = int(L.igi_mlp_workspace_bytes(rows, len(dims) - 1, (C.c_int32 * len(dims))(*dims)))
    return t


def _child_table(extra_env):
    env = {k: v for k, v in os.environ.items() if k not in RETIRED}
    env.update(extra_env)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_student_plans_equal_the_recorded_table():
    want = _golden()
    assert len(want) == len(TACTILE_BATCH) * len(TACTILE_HW) + len(LINEAR_ROWS) * (len(LINEAR_IN_OUT) + len(MLP_CHAINS))
    assert _child_table({}) == want


def test_retired_switches_no_longer_move_the_student_plans():
    assert _child_table(RETIRED) == _golden()


if __name__ == "__main__":
    print(json.dumps(plan_table(), indent=0))
