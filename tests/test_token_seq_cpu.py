"""Host-side checks of the token encoder's sequence limit (no device needed): the plan accepts 9 .. 32 tokens per sample
and refuses 33, the workspace scales with the token rows, the fake kernels give the right metadata at 32 tokens, and
tests/golden/make_golden_student_seq.py regenerates the committed fixture exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from isaacgyminsertion_amd import _lib, ops  # noqa: F401  (ops registers torch.ops.mi355ppo)


def _cfg(batch, seq, training=0):
    return _lib.TokenCfg(batch, seq, 32, 2, 128, 2, 0.1, training)


def test_the_plan_takes_up_to_32_tokens_and_refuses_33():
    L = _lib.lib()
    per_stack = int(L.igi_token_param_count(C.byref(_cfg(4, 3))))
    assert per_stack == 2 * (3 * 32 * 32 + 3 * 32 + 32 * 32 + 32 + 128 * 32 + 128 + 32 * 128 + 32 + 4 * 32)
    for seq in range(1, 33):
        assert int(L.igi_token_param_count(C.byref(_cfg(4, seq)))) == per_stack, seq      # parameters do not depend on seq
        assert int(L.igi_token_workspace_bytes(C.byref(_cfg(4, seq)))) > 4 * seq * 32 * 4, seq
    assert int(L.igi_token_param_count(C.byref(_cfg(4, 33)))) == _lib.IGI_E_UNSUPPORTED
    assert int(L.igi_token_workspace_bytes(C.byref(_cfg(4, 33)))) == 0
    with pytest.raises(RuntimeError, match=r"at most 32 .*sequence_length x modalities"):
        ops._token_cfg(torch.empty(4, 33, 32), 2, 128, 2, 0.1, False)


def test_the_workspace_grows_linearly_in_the_token_rows():
    """Beyond 9 tokens nothing in the plan depends on batch and seq separately (no one-launch backward records), and past
    16384 rows the LayerNorm partial blocks are at their cap: equal row counts give equal workspaces, and equal steps in
    the row count give equal steps in bytes (up to the 16-byte rounding of each of the plan's ~20 arrays)."""
    L = _lib.lib()

    def ws(batch, seq):
        return int(L.igi_token_workspace_bytes(C.byref(_cfg(batch, seq, 1))))

    assert ws(4096, 12) == ws(1536, 32) == ws(3072, 16)                # 49152 rows each
    base, step = ws(2048, 16), ws(4096, 16) - ws(2048, 16)
    assert step > 2048 * 16 * 32 * 4 * 20                               # ~20 row-sized arrays of >= 32 floats per layer pair
    for k in (2, 3, 4):
        assert abs(ws(2048 * (k + 1), 16) - (base + k * step)) <= 1024, k
    assert abs((ws(2048, 32) - ws(2048, 16)) - step) <= 1024            # doubling seq = doubling batch


def test_fake_kernels_give_the_shapes_at_32_tokens():
    from torch._subclasses.fake_tensor import FakeTensorMode
    L = _lib.lib()
    n = int(L.igi_token_param_count(C.byref(_cfg(7, 32))))
    nbytes = int(L.igi_token_workspace_bytes(C.byref(_cfg(7, 32, 1))))
    with FakeTensorMode():
        x, params = torch.empty(7, 32, 32), torch.empty(n)
        y, ws = torch.ops.mi355ppo.token_encoder_fwd(x, params, 2, 128, 2, 0.1, True, 5)
        assert y.shape == (7, 32, 32) and y.dtype == torch.float32
        assert ws.dtype == torch.uint8 and ws.shape == (nbytes,)
        dx, grads = torch.ops.mi355ppo.token_encoder_bwd(torch.empty(7, 32, 32), params, ws, 2, 128, 2, 0.1, True, 5)
        assert dx.shape == (7, 32, 32) and grads.shape == (n,)
        with pytest.raises(RuntimeError, match="at most 32"):
            torch.ops.mi355ppo.token_encoder_fwd(torch.empty(7, 33, 32), params, 2, 128, 2, 0.1, True, 5)


def test_the_generator_regenerates_the_committed_fixture_exactly():
    """(In a child process: importing the reference registers import-only stand-ins for gym, cv2, torchvision ... in
    sys.modules, which must not leak into the rest of the suite.)"""
    import subprocess
    import sys
    import tempfile
    from tests.golden import make_golden_student_seq as mg
    from tests.golden import ref_harness as rh
    if not os.path.isdir(rh.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([sys.executable, os.path.join(mg.HERE, "make_golden_student_seq.py"), d], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        fresh = mg.load(d)
        names = sorted(os.listdir(d))
    stored = mg.load()
    assert names == sorted(mg.file_names()) == sorted(n for n in os.listdir(mg.HERE) if n.startswith("student_seq."))
    assert set(fresh) == set(stored)
    for k, v in fresh.items():
        assert v.dtype == stored[k].dtype and np.array_equal(v, stored[k]), k
    for name in names:                                                 # and every file stays a committable size
        assert os.path.getsize(os.path.join(mg.HERE, name)) < 1 << 20, name
