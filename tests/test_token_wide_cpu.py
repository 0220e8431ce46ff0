"""Host-side checks of the token encoder's widths (no device needed): the plan accepts d_model 32 / 64 / 128 with heads
of 16 / 32 / 64 features and refuses everything else, the Python layer refuses the same set by name before the library
call, the fake kernels give the right metadata, the test helpers' masks and float64 restatement hold at every width, the
student builds with the reference's state_dict at 64 and 128 wide, and tests/golden/make_golden_student_wide.py
regenerates its committed files exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from isaacgyminsertion_amd import _lib, ops  # noqa: F401  (ops registers torch.ops.mi355ppo)
from tests import token_wide_ref as w

LAYERS = 2


def _cfg(d, H, ff, batch=4, seq=3, training=0, layers=LAYERS):
    return _lib.TokenCfg(batch, seq, d, H, ff, layers, 0.1, training)


@pytest.mark.parametrize("d,H", w.NEW_PAIRS)
def test_parameter_count_is_that_of_the_torch_layers(d, H):
    ff = 4 * d
    layer = nn.TransformerEncoderLayer(d_model=d, nhead=H, dim_feedforward=ff, activation="gelu", batch_first=True,
                                       norm_first=True)
    want = LAYERS * sum(p.numel() for p in layer.parameters())
    assert int(_lib.lib().igi_token_param_count(C.byref(_cfg(d, H, ff)))) == want
    assert int(_lib.lib().igi_token_param_count(C.byref(_cfg(d, H, 100, layers=1)))) == \
        sum(p.numel() for p in nn.TransformerEncoderLayer(d, H, 100).parameters())


@pytest.mark.parametrize("d,H", w.NEW_PAIRS)
def test_workspace_is_positive_and_linear_in_the_rows(d, H):
    """Off (32, 2) nothing in the plan depends on batch and seq separately (no one-launch backward records), and past 16384
    rows the LayerNorm partial blocks are at their cap: equal steps in the row count give equal steps in bytes (up to the
    16-byte rounding of each of the plan's ~20 arrays)."""
    L = _lib.lib()

    def ws(batch, seq):
        return int(L.igi_token_workspace_bytes(C.byref(_cfg(d, H, 4 * d, batch, seq, 1))))

    assert ws(4, 3) > 4 * 3 * d * 4
    assert ws(4096, 12) == ws(1536, 32) == ws(3072, 16)
    base, step = ws(2048, 16), ws(4096, 16) - ws(2048, 16)
    assert step > 2048 * 16 * d * 4 * 20
    for k in (2, 3, 4):
        assert abs(ws(2048 * (k + 1), 16) - (base + k * step)) <= 1024, k


def test_the_stock_configuration_is_unchanged():
    """(32, 2): the parameter count, and workspace sizes recorded from the library before the widths were added (3 tokens:
    with the one-launch backward's gradient records; 12 tokens: without)."""
    L = _lib.lib()
    assert int(L.igi_token_param_count(C.byref(_cfg(32, 2, 128)))) == 2 * 12704
    got = {(b, s, t): int(L.igi_token_workspace_bytes(C.byref(_cfg(32, 2, 128, b, s, t))))
           for b, s, t in STOCK_WORKSPACE}
    assert got == STOCK_WORKSPACE


# {(batch, seq, training): bytes}
STOCK_WORKSPACE = {(4, 3, 0): 524864, (2048, 3, 1): 94732480, (8192, 2, 1): 194838720, (30000, 3, 1): 887313088,
                   (37, 8, 1): 7195328, (512, 12, 1): 68714688, (130, 32, 0): 49319104}


@pytest.mark.parametrize("d,H", w.REFUSED_PAIRS)
def test_other_widths_are_refused_by_the_library_and_by_name_in_python(d, H):
    L = _lib.lib()
    assert int(L.igi_token_param_count(C.byref(_cfg(d, H, 4 * d)))) == _lib.IGI_E_UNSUPPORTED
    assert int(L.igi_token_workspace_bytes(C.byref(_cfg(d, H, 4 * d)))) == 0
    with pytest.raises(RuntimeError, match=r"d_model in \[32, 64, 128\] with heads of .* in \[16, 32, 64\] .*no fallback"):
        ops._token_cfg(torch.empty(4, 3, d), H, 4 * d, 2, 0.1, False)


def test_supported_widths_pass_the_python_check():
    for d, H in w.NEW_PAIRS + [(32, 2)]:
        cfg = ops._token_cfg(torch.empty(4, 3, d), H, 4 * d, 2, 0.1, False)
        assert (cfg.d_model, cfg.nhead) == (d, H)


@pytest.mark.parametrize("d,H", [(64, 4), (128, 2)])
def test_fake_kernels_give_the_shapes(d, H):
    from torch._subclasses.fake_tensor import FakeTensorMode
    L = _lib.lib()
    n = int(L.igi_token_param_count(C.byref(_cfg(d, H, 4 * d, 7, 5))))
    nbytes = int(L.igi_token_workspace_bytes(C.byref(_cfg(d, H, 4 * d, 7, 5, 1))))
    assert n > 0 and nbytes > 0
    with FakeTensorMode():
        x, params = torch.empty(7, 5, d), torch.empty(n)
        y, ws = torch.ops.mi355ppo.token_encoder_fwd(x, params, H, 4 * d, 2, 0.1, True, 5)
        assert y.shape == (7, 5, d) and y.dtype == torch.float32
        assert ws.dtype == torch.uint8 and ws.shape == (nbytes,)
        dx, grads = torch.ops.mi355ppo.token_encoder_bwd(torch.empty(7, 5, d), params, ws, H, 4 * d, 2, 0.1, True, 5)
        assert dx.shape == (7, 5, d) and grads.shape == (n,)


def test_wide_masks_at_32_are_the_oracle_stack_masks():
    from oracle import token_dropout as td
    seed = 0x2B5C9D1E00F0A7C3
    a = w.wide_masks(5, 7, 2, 32, 128, 0.1, seed, 2)
    b = td.stack_masks(5, 7, 2, 128, 0.1, seed, 2)
    assert len(a) == len(b) == 2
    for la, lb in zip(a, b):
        assert len(la) == len(lb) == 4
        for ma, mb in zip(la, lb):
            assert ma.dtype == mb.dtype and torch.equal(ma, mb)
    assert 0.8 < float((a[0][1] != 0).double().mean()) < 0.97


@pytest.mark.parametrize("d,H", w.NEW_PAIRS)
def test_the_float64_restatement_is_torch_transformer_encoder(d, H):
    """oracle.student.encoder_layer (the train-mode tests' reference) against nn.TransformerEncoder, float64, dropout off."""
    stack = w.wide_stack(d, H, 4 * d, 2)
    x, dy = w.inputs(d, 3, 5)
    yr, dxr, gr = w.eval_run(stack, x, dy, torch.float64)
    y, dx, g = w.restated(stack, H, x, dy, None, torch.float64)
    assert (y - yr).abs().max() <= 1e-12 and (dx - dxr).abs().max() <= 1e-12
    assert list(g) == list(gr)
    for n in gr:
        assert (g[n] - gr[n]).abs().max() <= 1e-12, n


@pytest.mark.parametrize("tag", ["lin_h10_d64", "tac_lin_d64h2", "lin_h3_d128"])
def test_the_student_builds_with_the_reference_state_dict(tag):
    """Names and shapes recorded from the reference's MultiModalModel (tests/golden/student_wide_keys.json): 64 / 4,
    64 / 2 with a tactile encoder, 128 / 2."""
    from isaacgyminsertion_amd.algo.models.transformer.tact import MultiModalModel
    from tests.golden import make_golden_student_wide as mg
    case = {c[0]: c for c in mg.CASES}[tag]
    model = MultiModalModel(**mg.model_kwargs(*case[1:7]))
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == mg.load_keys()[tag]


def test_mismatched_encoding_sizes_are_refused_at_construction():
    from isaacgyminsertion_amd.algo.models.transformer.tact import MultiModalModel
    from tests.golden import make_golden_student_wide as mg
    kw = mg.model_kwargs(1, True, 64, 4, 2, 4)
    kw["lin_encoding_size"] = 32
    with pytest.raises(ValueError, match=r"tactile_encoding_size = 64 .*lin_encoding_size = 32"):
        MultiModalModel(**kw)
    kw = mg.model_kwargs(1, False, 64, 4, 2, 4)
    kw.update(include_img=True, img_encoding_size=128, seg_encoding_size=16)     # seg is not included: not named
    with pytest.raises(ValueError, match=r"img_encoding_size = 128$"):
        MultiModalModel(**kw)


def test_the_generator_regenerates_the_committed_files_exactly():
    """(In a child process: importing the reference registers import-only stand-ins for gym, cv2, torchvision ... in
    sys.modules, which must not leak into the rest of the suite.)"""
    import json
    import subprocess
    import sys
    import tempfile
    from tests.golden import make_golden_student_wide as mg
    from tests.golden import ref_harness as rh
    if not os.path.isdir(rh.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([sys.executable, os.path.join(mg.HERE, "make_golden_student_wide.py"), d], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        fresh = mg.load(d)
        fresh_keys = mg.load_keys(d)
        names = sorted(os.listdir(d))
    stored = mg.load()
    committed = sorted(n for n in os.listdir(mg.HERE) if n.startswith("student_wide") and not n.endswith(".py"))
    assert names == sorted(mg.file_names() + [mg.KEYS_FILE]) == committed
    assert set(fresh) == set(stored)
    for k, v in fresh.items():
        assert v.dtype == stored[k].dtype and np.array_equal(v, stored[k]), k
    assert fresh_keys == mg.load_keys() and json.dumps(fresh_keys)
    for name in names:                                                 # and every file stays a committable size
        assert os.path.getsize(os.path.join(mg.HERE, name)) < 1 << 20, name
