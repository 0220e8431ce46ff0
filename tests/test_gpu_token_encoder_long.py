"""HipTransformerEncoder over 9 .. 32 tokens per sample: the tile attention kernels (k_attn_tile_fwd / k_attn_tile_bwd: one
32 x 32 matrix-pipe tile per (sample, head), S a runtime argument) and the one-launch forward k_token_fwd_long, on the
weights, inputs and bounds of tests/test_gpu_token_encoder.py (whose helpers are used as they are).  Every shape here
raises RuntimeError (IGI_E_UNSUPPORTED) on a library that stops at 8 tokens.

The bounds hold at these sizes with room to spare: ATen's own fp32 nn.TransformerEncoder against its float64 evaluation
uses at most 4.6 % (output), 1.7 % (input gradient) and 2.0 % (parameter gradients) of them at these shapes.  Every test
prints the share of each bound it used (pytest -s)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from tests import test_gpu_token_encoder as te

pytestmark = pytest.mark.gpu


def _figures(ym, xm, named_grads, yr, dxr, gr, grad_abs):
    """[(name, error, bound)] with test_matches_torch_transformer_encoder's bounds (grad_abs: its absolute terms, which
    differ between the dropout-off and the train-mode test: (1e-7, 1e-6) and (1e-6, 1e-6))."""
    figs = [("y", (ym.detach().double().cpu() - yr).abs().max().item(), 2e-5 * max(1.0, yr.abs().max().item())),
            ("dx", (xm.grad.double().cpu() - dxr).abs().max().item(), 1e-4 * dxr.abs().max().item() + grad_abs[0])]
    for n, q in named_grads:
        assert q.grad is not None, n
        figs.append((n, (q.grad.double().cpu() - gr[n]).abs().max().item(), 1e-4 * gr[n].abs().max().item() + grad_abs[1]))
    return figs


def _report(tag, figs):
    for n, err, bound in figs:
        print(f"[{tag}] {n}: err {err:.3e} bound {bound:.3e} ({100 * err / bound:.1f} % of the bound)")
    print(f"[{tag}] worst share: y {100 * figs[0][1] / figs[0][2]:.1f} %, dx {100 * figs[1][1] / figs[1][2]:.1f} %, "
          f"parameters {100 * max(e / b for _, e, b in figs[2:]):.1f} %")
    assert not [f for f in figs if not f[1] <= f[2]]


@functools.lru_cache(maxsize=None)
def _eval_reference(B, S):
    """nn.TransformerEncoder in float64, dropout off, on test_matches_torch_transformer_encoder's weights and inputs:
    computed once per shape, shared by both forward paths, never modified."""
    layer = te._layer()
    te._set_dropout(layer, 0.0)
    ref = nn.TransformerEncoder(copy.deepcopy(layer), num_layers=2, enable_nested_tensor=False).double()
    with torch.no_grad():
        for i, a in enumerate(ref.layers[1].parameters()):
            a.copy_((torch.randn(a.shape, generator=torch.Generator().manual_seed(100 + i)) * 0.3).double())
    g = torch.Generator().manual_seed(B + S)
    x = torch.randn(B, S, 32, generator=g)
    dy = torch.randn(B, S, 32, generator=g)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.double())
    return x, dy, yr.detach(), xr.grad, {n: a.grad for n, a in ref.named_parameters()}


# (37, 9) one token above the register kernels, ragged tile; (5, 17) across the 16-row half of the tile; (67, 31) one below
# the cap; (3, 32) fewer samples than a workgroup holds; (130, 32) full workgroups and a ragged last one; (512, 12) many
EVAL_SHAPES = [(37, 9), (5, 17), (67, 31), (3, 32), (130, 32), (512, 12)]


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("B,S", EVAL_SHAPES)
def test_long_sequences_match_torch_transformer_encoder(B, S, fused, monkeypatch):
    """Dropout off, against nn.TransformerEncoder in float64; ``fused`` = 1: k_token_fwd_long (the default), 0: the
    launch-per-operation forward with k_attn_tile_fwd.  The backward is launch-per-operation with k_attn_tile_bwd either
    way."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    x, dy, yr, dxr, gr = _eval_reference(B, S)
    layer = te._layer()
    te._set_dropout(layer, 0.0)
    mine = HipTransformerEncoder(layer, num_layers=2)
    with torch.no_grad():
        for i, b in enumerate(mine.layers[1].parameters()):
            b.copy_(torch.randn(b.shape, generator=torch.Generator().manual_seed(100 + i)) * 0.3)
    mine = mine.cuda()
    assert list(gr) == [n for n, _ in mine.named_parameters()]
    monkeypatch.setenv("IGI_TOKEN_FUSED", fused)
    xm = x.cuda().requires_grad_(True)
    ym = mine(xm)
    ym.backward(dy.cuda())
    _report(f"eval {B}x{S} fused={fused}", _figures(ym, xm, mine.named_parameters(), yr, dxr, gr, (1e-7, 1e-6)))


@pytest.mark.parametrize("B,S", [(100, 9), (37, 32), (512, 12)])
def test_one_launch_forward_is_bitwise_the_launch_per_operation_forward_beyond_8_tokens(B, S, monkeypatch):
    """k_token_fwd_long against the launch-per-operation forward under dropout 0.1: output, input gradient and every
    parameter gradient bit-identical (the backward reads the saved activations, so equal gradients pin each of them)."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    layer = te._layer(3)
    te._set_dropout(layer, 0.1)
    enc = HipTransformerEncoder(layer, num_layers=2).cuda().train()
    g = torch.Generator().manual_seed(B * 10 + S)
    x = torch.randn(B, S, 32, generator=g).cuda()
    dy = torch.randn(B, S, 32, generator=g).cuda()
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("IGI_TOKEN_FUSED", mode)
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        xm = x.clone().requires_grad_(True)
        y = enc(xm)
        y.backward(dy)
        out[mode] = [y.detach().clone(), xm.grad.clone()] + [q.grad.clone() for q in enc.parameters()]
    assert torch.isfinite(out["1"][0]).all()
    for i, (a, b) in enumerate(zip(out["0"], out["1"])):
        assert torch.equal(a, b), (i, (a - b).abs().max().item())


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("B,S,p", [(33, 9, 0.1), (2, 17, 0.5), (130, 32, 0.1)])
def test_train_mode_matches_the_masked_float64_restatement_beyond_8_tokens(B, S, p, fused, monkeypatch):
    """Dropout ON against oracle.student.encoder_layer in float64 with the masks oracle/token_dropout.py recomputes from
    the drawn seed (the helpers and bounds of test_train_mode_matches_the_masked_float64_restatement).  A wrong
    attention-mask element is an O(0.1 .. 1) error: this pins the element numbering ((b H + h) S + i) S + j of the tile
    kernels, whose lanes and registers walk i and j in the matrix pipe's order."""
    x, dy, seed, masks, (yr, dxr, gr) = te._train_reference(B, S, p)      # cached per case
    assert masks[0][0].shape == (B, 2, S, S)
    assert not torch.equal(masks[0][0][:, 0], masks[0][0][:, 1])
    enc, _ = te._train_stack(p)
    monkeypatch.setenv("IGI_TOKEN_FUSED", fused)
    monkeypatch.setenv("IGI_TOKEN_FUSED_BWD", fused)
    torch.manual_seed(1000 + B)                           # the encoder's draw is the next one: seed
    xm = x.cuda().requires_grad_(True)
    ym = enc(xm)
    ym.backward(dy.cuda())
    assert [n for n, _ in enc.named_parameters()] == list(gr)
    _report(f"train {B}x{S} p={p} fused={fused}", _figures(ym, xm, enc.named_parameters(), yr, dxr, gr, (1e-6, 1e-6)))


def test_two_runs_from_one_seed_are_bit_identical():
    """(130, 32), dropout 0.1: forward and backward, twice from the same seed (no atomics anywhere on the path)."""
    enc, _ = te._train_stack(0.1)
    g = torch.Generator().manual_seed(162)
    x = torch.randn(130, 32, 32, generator=g).cuda()
    dy = torch.randn(130, 32, 32, generator=g).cuda()
    runs = []
    for _ in range(2):
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        xm = x.clone().requires_grad_(True)
        y = enc(xm)
        y.backward(dy)
        runs.append([y.detach().clone(), xm.grad.clone()] + [q.grad.clone() for q in enc.parameters()])
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    torch.manual_seed(6)
    assert not torch.equal(enc(x), runs[0][0])              # and another seed is another mask


def _profiled(fn):
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    return out, classes


def test_which_kernels_run_at_12_and_at_8_tokens(monkeypatch):
    """Through the library's launch profiler: 12 tokens with the defaults are ONE forward launch (k_token_fwd_long, no GEMM, no
    attention kernel); with IGI_TOKEN_FUSED=0 the two layers launch k_attn_tile_fwd twice; the backward launches
    k_attn_tile_bwd twice; 8 tokens still run k_token_fwd<8> (class "k_token_fwd<S>": the register
    kernels, which exist for S <= 8 only) and none of the new kernels."""
    monkeypatch.delenv("IGI_TOKEN_FUSED", raising=False)
    monkeypatch.delenv("IGI_TOKEN_FUSED_BWD", raising=False)
    enc, _ = te._train_stack(0.1)
    enc.eval()
    x12 = torch.randn(64, 12, 32, device="cuda")
    x8 = torch.randn(64, 8, 32, device="cuda")
    with torch.no_grad():
        _, c = _profiled(lambda: enc(x12))
    assert c.get("k_token_fwd_long") == 1 and not [k for k in c if k.startswith(("gemm", "k_attn", "k_token_fwd<"))], c
    monkeypatch.setenv("IGI_TOKEN_FUSED", "0")
    with torch.no_grad():
        _, c = _profiled(lambda: enc(x12))
    assert c.get("k_attn_tile_fwd") == 2 and "k_token_fwd_long" not in c and "k_token_fwd<S>" not in c, c
    monkeypatch.delenv("IGI_TOKEN_FUSED")
    xg = x12.clone().requires_grad_(True)
    y = enc(xg)
    _, c = _profiled(lambda: y.sum().backward())
    assert c.get("k_attn_tile_bwd") == 2 and "k_attn_tile_fwd" not in c, c
    with torch.no_grad():
        _, c = _profiled(lambda: enc(x8))
    assert c.get("k_token_fwd<S>") == 1 and not [k for k in c if k.startswith(("gemm", "k_attn", "k_token_fwd_long"))], c


def test_33_tokens_are_refused_with_the_limit_named():
    enc, _ = te._train_stack(0.0)
    with pytest.raises(RuntimeError, match=r"at most 32 .*sequence_length x modalities"):
        enc(torch.zeros(2, 33, 32, device="cuda"))
    from isaacgyminsertion_amd import _lib
    import ctypes as C
    cfg = _lib.TokenCfg(2, 33, 32, 2, 128, 2, 0.0, 0)
    assert int(_lib.lib().igi_token_param_count(C.byref(cfg))) == _lib.IGI_E_UNSUPPORTED
