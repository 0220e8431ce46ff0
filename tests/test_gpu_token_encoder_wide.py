"""HipTransformerEncoder at d_model 32 / 64 / 128 with heads of 16 / 32 / 64 features: the wide LayerNorm kernels
(k_resid_ln_fwd<D>, k_ln_bwd<D>) and the tile attention kernels templated on the head width (k_attn_tile_fwd<DH, DM>,
k_attn_tile_bwd<DH, DM>), which every configuration but (32, 2) runs launch per operation at every S from 1 to 32.
Every shape here raises RuntimeError (IGI_E_UNSUPPORTED) on a library that stops at (32, 2).

Weights, inputs, masks and references: tests/token_wide_ref.py.  Bounds: those of test_gpu_token_encoder_long.py, unchanged
(y 2e-5 * max(1, max|y|); dx 1e-4 * max|dx| + a; parameters 1e-4 * max|g| + 1e-6; a = 1e-7 with dropout off, 1e-6 in
train mode).  The float32 evaluation of the float64 references themselves (nn.TransformerEncoder / the masked
restatement on the CPU) uses at most 7.8 % (y), 5.0 % (dx) and 3.6 % (parameters) of them over the cases below.  Every test
prints the share of each bound it used (pytest -s)."""
import pytest
import torch

from tests import token_wide_ref as w

pytestmark = pytest.mark.gpu


def _report(tag, figs):
    for n, err, bound in figs:
        print(f"[{tag}] {n}: err {err:.3e} bound {bound:.3e} ({100 * err / bound:.1f} % of the bound)")
    sy, sx, sp = w.shares(figs)
    print(f"[{tag}] worst share: y {100 * sy:.1f} %, dx {100 * sx:.1f} %, parameters {100 * sp:.1f} %")
    assert not [f for f in figs if not f[1] <= f[2]]


def _run(enc, x, dy, seed_key=None):
    enc.zero_grad(set_to_none=True)
    if seed_key is not None:
        torch.manual_seed(seed_key)                      # the encoder's draw is the next one
    xm = x.cuda().requires_grad_(True)
    y = enc(xm)
    y.backward(dy.cuda())
    return y.detach(), xm.grad, {n: q.grad for n, q in enc.named_parameters()}


@pytest.mark.parametrize("d,H,ff,layers,B,S", w.EVAL_CASES)
def test_wide_configurations_match_torch_transformer_encoder(d, H, ff, layers, B, S):
    """Dropout off, against nn.TransformerEncoder in float64.  (37, 9), (5, 17), (67, 31), (130, 32): the tile's ragged and
    full shapes at each head width; (3, 3), (5, 1), (33, 8): S below 9 on the tile kernels (one-entry softmax at S = 1);
    ff = 100: ff != 4 d; (4096, 5): more rows than 256 LayerNorm blocks of 64; (1, 32) x 3 layers: one sample."""
    x, dy, yr, dxr, gr = w.eval_reference(d, H, ff, layers, B, S)
    enc = w.hip_encoder(w.wide_stack(d, H, ff, layers)).cuda()
    assert list(gr) == [n for n, _ in enc.named_parameters()]
    y, dx, g = _run(enc, x, dy)
    _report(f"eval d={d} H={H} ff={ff} L={layers} {B}x{S}", w.figures(y, dx, g, yr, dxr, gr, (1e-7, 1e-6)))


@pytest.mark.parametrize("d,H,ff,layers,B,S,p", w.TRAIN_CASES)
def test_wide_train_mode_matches_the_masked_float64_restatement(d, H, ff, layers, B, S, p):
    """Dropout ON against oracle.student.encoder_layer in float64 with wide_masks from the drawn seed: pins the element
    numbers row * d + f, row * ff + c and ((b H + h) S + i) S + j at every width (a wrong mask element is an O(0.1 .. 1)
    error) and, at DH = 64, that both column passes of P . V see the same dropout factors."""
    x, dy, seed, masks, (yr, dxr, gr) = w.train_reference(d, H, ff, layers, B, S, p)
    assert masks[0][0].shape == (B, H, S, S) and masks[0][1].shape == (B, S, d) and masks[0][2].shape == (B, S, ff)
    if H > 1:
        assert not torch.equal(masks[0][0][:, 0], masks[0][0][:, 1])       # two heads do not share a mask
    enc = w.hip_encoder(w.wide_stack(d, H, ff, layers, p)).cuda().train()
    assert [n for n, _ in enc.named_parameters()] == list(gr)
    y, dx, g = _run(enc, x, dy, seed_key=1000 + B)
    _report(f"train d={d} H={H} {B}x{S} p={p}", w.figures(y, dx, g, yr, dxr, gr, (1e-6, 1e-6)))


@pytest.mark.parametrize("d,H,ff,B,S", [(64, 4, 256, 130, 32), (128, 2, 512, 37, 9)])
def test_wide_runs_from_one_seed_are_bit_identical(d, H, ff, B, S):
    """Forward and backward twice from the same seed (fixed-order sums, no atomics); another seed is another mask; eval mode
    is deterministic."""
    enc = w.hip_encoder(w.wide_stack(d, H, ff, 2, 0.1)).cuda().train()
    x, dy = w.inputs(d, B, S)
    a = _run(enc, x, dy, seed_key=5)
    b = _run(enc, x, dy, seed_key=5)
    assert torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
    c = _run(enc, x, dy, seed_key=6)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    enc.eval()
    with torch.no_grad():
        assert torch.equal(enc(x.cuda()), enc(x.cuda()))


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


ONE_LAUNCH = ("k_token_fwd", "k_token_bwd")


@pytest.mark.parametrize("d,H,S", [(64, 4, 9), (128, 2, 3), (32, 1, 3)])
def test_which_kernels_run_off_the_stock_width(d, H, S, monkeypatch):
    """Through the library's launch profiler, with the switches at their defaults: the tile attention kernels run once per
    layer, forward and backward, also at S = 3; no one-launch kernel and no register attention kernel runs (the register
    kernels have no profiler class: with k_attn_tile_* counted once per layer there is no launch left for them)."""
    monkeypatch.delenv("IGI_TOKEN_FUSED", raising=False)
    monkeypatch.delenv("IGI_TOKEN_FUSED_BWD", raising=False)
    enc = w.hip_encoder(w.wide_stack(d, H, 4 * d, 2)).cuda().eval()
    x = torch.randn(64, S, d, device="cuda")
    with torch.no_grad():
        _, c = _profiled(lambda: enc(x))
    assert c.get("k_attn_tile_fwd") == 2 and not [k for k in c if k.startswith(ONE_LAUNCH)], c
    xg = x.clone().requires_grad_(True)
    y = enc(xg)
    _, c = _profiled(lambda: y.sum().backward())
    assert c.get("k_attn_tile_bwd") == 2 and "k_attn_tile_fwd" not in c and not [k for k in c if k.startswith(ONE_LAUNCH)], c


def test_the_stock_width_still_runs_the_one_launch_forward(monkeypatch):
    """(32, 2) at the shape (32, 1) was profiled at above: k_token_fwd<3>, one launch, no attention kernel."""
    monkeypatch.delenv("IGI_TOKEN_FUSED", raising=False)
    enc = w.hip_encoder(w.wide_stack(32, 2, 128, 2)).cuda().eval()
    with torch.no_grad():
        _, c = _profiled(lambda: enc(torch.randn(64, 3, 32, device="cuda")))
    assert c.get("k_token_fwd<S>") == 1 and not [k for k in c if k.startswith(("gemm", "k_attn"))], c


def test_the_fused_switch_selects_nothing_at_64_wide(monkeypatch):
    enc = w.hip_encoder(w.wide_stack(64, 4, 256, 2, 0.1)).cuda().train()
    x, dy = w.inputs(64, 33, 3)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("IGI_TOKEN_FUSED", mode)
        monkeypatch.setenv("IGI_TOKEN_FUSED_BWD", mode)
        out[mode] = _run(enc, x, dy, seed_key=11)
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])
    for n in out["0"][2]:
        assert torch.equal(out["0"][2][n], out["1"][2][n]), n


def test_opcheck_at_64_wide_two_heads():
    enc = w.hip_encoder(w.wide_stack(64, 2, 256, 1)).cuda()
    x = torch.randn(3, 5, 64, device="cuda", requires_grad=True)
    params = enc.flat_parameters().detach().contiguous().requires_grad_(True)
    # (the utilities tests/test_gpu_ops.py runs on this op at 32 wide, for its reason: the workspace the forward returns is
    #  scratch of the backward op, which AOT's partitioner rejects; the backward op takes the static AOT check as well)
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.mi355ppo.token_encoder_fwd, (x, params, 2, 256, 1, 0.0, False, 0), test_utils=tests)
    _, ws = torch.ops.mi355ppo.token_encoder_fwd(x.detach(), params.detach(), 2, 256, 1, 0.1, True, 1234)
    torch.library.opcheck(torch.ops.mi355ppo.token_encoder_bwd,
                          (torch.randn(3, 5, 64, device="cuda"), params.detach(), ws, 2, 256, 1, 0.1, True, 1234),
                          test_utils=tests + ("test_aot_dispatch_static",))
