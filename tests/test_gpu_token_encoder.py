"""igi_token_forward / igi_token_backward (HipTransformerEncoder) against nn.TransformerEncoder in fp64 on the
same weights and inputs (dropout off), plus the statistical / reproducibility properties of its dropout.
Tolerance: 2-layer d=32 fp32 network with O(1) activations: 2e-5 absolute on outputs, 1e-4 relative to the
largest entry on gradients (sums over up to 4096 x 3 token rows).

Train mode (dropout on) is pinned further down against oracle.student.encoder_layer in float64 with the masks
oracle/token_dropout.py recomputes from the seed the module draws: output, input gradient and every parameter gradient,
on each of the four kernel paths (one-launch / launch-per-operation, forward / backward)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _layer(seed=0):
    torch.manual_seed(seed)
    layer = nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=128, activation="gelu",
                                       batch_first=True, norm_first=True)
    with torch.no_grad():
        for p in layer.parameters():       # O(1)-scale, non-trivial LayerNorm weights
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() > 1 else 0.2) + (1.0 if p.dim() == 1 and p.numel() == 32 else 0.0))
    return layer


@pytest.mark.parametrize("B,S", [(64, 3), (5, 2), (1, 1), (4096, 3), (33, 8)])
def test_matches_torch_transformer_encoder(B, S):
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    layer = _layer()
    for m in layer.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    layer.self_attn.dropout = 0.0
    ref = nn.TransformerEncoder(copy.deepcopy(layer), num_layers=2, enable_nested_tensor=False).double()
    mine = HipTransformerEncoder(layer, num_layers=2).cuda()
    assert list(ref.state_dict().keys()) == list(mine.state_dict().keys())
    with torch.no_grad():           # different weights per layer
        for i, (a, b) in enumerate(zip(ref.layers[1].parameters(), mine.layers[1].parameters())):
            v = torch.randn(a.shape, generator=torch.Generator().manual_seed(100 + i)) * 0.3
            a.copy_(v.double()); b.copy_(v.cuda())
    g = torch.Generator().manual_seed(B + S)
    x = torch.randn(B, S, 32, generator=g)
    dy = torch.randn(B, S, 32, generator=g)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.double())
    xm = x.cuda().requires_grad_(True)
    ym = mine(xm)
    ym.backward(dy.cuda())
    assert (ym.double().cpu() - yr).abs().max() <= 2e-5 * max(1.0, yr.abs().max().item())
    assert (xm.grad.double().cpu() - xr.grad).abs().max() <= 1e-4 * xr.grad.abs().max().item() + 1e-7
    for (n, a), b in zip(ref.named_parameters(), mine.parameters()):
        assert b.grad is not None, n
        err = (b.grad.double().cpu() - a.grad).abs().max().item()
        assert err <= 1e-4 * a.grad.abs().max().item() + 1e-6, (n, err)


def test_dropout_is_reproducible_unbiased_and_consistent_between_forward_and_backward():
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    enc = HipTransformerEncoder(_layer(), num_layers=2).cuda().train()
    x = torch.randn(2048, 3, 32, device="cuda")
    torch.manual_seed(7)
    y1 = enc(x)
    torch.manual_seed(7)
    y2 = enc(x)
    y3 = enc(x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)         # seeded by torch's generator
    enc.eval()
    y0 = enc(x)
    assert torch.equal(y0, enc(x))
    # inverted dropout is unbiased: the train-mode mean over many masks approaches the eval output of a LINEAR probe;
    # here: the residual stream is linear in the branch outputs, so compare first moments loosely
    enc.train()
    acc = torch.zeros_like(y0)
    for _ in range(32):
        acc += enc(x)
    rel = ((acc / 32 - y0).abs().mean() / y0.abs().mean()).item()
    assert rel < 0.2, rel
    # gradient check through the SAME masks: finite difference along a random direction, fp32 tolerances
    xs = torch.randn(16, 3, 32, device="cuda", requires_grad=True)
    v = torch.randn_like(xs)
    torch.manual_seed(11)
    out = enc(xs)
    (gx,) = torch.autograd.grad(out.sum(), xs)
    eps = 1e-2
    torch.manual_seed(11)
    fp = enc(xs.detach() + eps * v).sum()
    torch.manual_seed(11)
    fm = enc(xs.detach() - eps * v).sum()
    fd = ((fp - fm) / (2 * eps)).item()
    an = (gx * v).sum().item()
    assert abs(fd - an) <= 2e-2 * max(1.0, abs(an)), (fd, an)


def test_dropout_rate():
    """mask density: feed zeros through a layer whose ff bias is the only non-zero path."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    layer = _layer()
    with torch.no_grad():
        for p in layer.parameters():
            p.zero_()
        layer.linear2.bias.fill_(1.0)          # ff branch output = 1 everywhere before its dropout
    enc = HipTransformerEncoder(layer, num_layers=1).cuda().train()
    y = enc(torch.zeros(4096, 3, 32, device="cuda"))
    kept = (y != 0).float().mean().item()
    assert abs(kept - 0.9) < 0.01, kept
    assert torch.allclose(y[y != 0], torch.full_like(y[y != 0], 1 / 0.9), atol=1e-6)


@pytest.mark.parametrize("B,S,p", [(512, 3, 0.1), (37, 3, 0.1), (1, 1, 0.0), (100, 8, 0.1), (2, 2, 0.5), (4096, 4, 0.1)])
def test_one_launch_forward_is_bitwise_the_launch_per_operation_forward(B, S, p, monkeypatch):
    """k_token_fwd (the whole stack in one launch, IGI_TOKEN_FUSED=1, the default) against the 17-launch forward it replaces:
    output, input gradient and every parameter gradient bit-identical (the backward reads the saved activations, so equal
    gradients pin every one of them), dropout on."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    layer = _layer(3)
    for m in layer.modules():
        if isinstance(m, nn.Dropout):
            m.p = p
    layer.self_attn.dropout = p
    enc = HipTransformerEncoder(layer, num_layers=2).cuda().train()
    g = torch.Generator().manual_seed(B * 10 + S)
    x = torch.randn(B, S, 32, generator=g).cuda()
    dy = torch.randn(B, S, 32, generator=g).cuda()
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("IGI_TOKEN_FUSED", mode)
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)                      # the dropout seed is drawn from torch's CPU generator
        xm = x.clone().requires_grad_(True)
        y = enc(xm)
        y.backward(dy)
        out[mode] = [y.detach().clone(), xm.grad.clone()] + [q.grad.clone() for q in enc.parameters()]
    assert torch.isfinite(out["1"][0]).all()
    for i, (a, b) in enumerate(zip(out["0"], out["1"])):
        assert torch.equal(a, b), (i, (a - b).abs().max().item())


@pytest.mark.parametrize("B,S,p", [(512, 3, 0.1), (37, 3, 0.1), (1, 1, 0.0), (100, 8, 0.1), (4096, 2, 0.1), (2048, 4, 0.0), (40000, 3, 0.1)])
def test_one_launch_backward_agrees_with_the_launch_per_operation_backward(B, S, p, monkeypatch):
    """k_token_bwd (IGI_TOKEN_FUSED_BWD=1, the default) against the ~20-launch backward: the same formulas and dropout masks,
    sums associated per workgroup record instead of per split-row slab -> agreement to fp32 rounding (1e-5 of the largest
    entry of each gradient), and bitwise reproducible run to run.  (40000 x 3: more than 1024 records, the library keeps the
    launch-per-operation backward -- both settings then run the same code.)"""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    layer = _layer(5)
    for m in layer.modules():
        if isinstance(m, nn.Dropout):
            m.p = p
    layer.self_attn.dropout = p
    enc = HipTransformerEncoder(layer, num_layers=2).cuda().train()
    g = torch.Generator().manual_seed(B * 10 + S)
    x = torch.randn(B, S, 32, generator=g).cuda()
    dy = torch.randn(B, S, 32, generator=g).cuda()
    out = {}
    for mode in ("0", "1", "1b"):
        monkeypatch.setenv("IGI_TOKEN_FUSED_BWD", mode[0])
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        xm = x.clone().requires_grad_(True)
        enc(xm).backward(dy)
        out[mode] = [xm.grad.clone()] + [q.grad.clone() for q in enc.parameters()]
    names = ["dx"] + [n for n, _ in enc.named_parameters()]
    for n, a, b, c in zip(names, out["0"], out["1"], out["1b"]):
        assert torch.isfinite(b).all(), n
        assert torch.equal(b, c), n
        err = (a - b).abs().max().item()
        assert err <= 1e-5 * a.abs().max().item() + 1e-7, (n, err, a.abs().max().item())


# ---- train mode against the float64 restatement with the recomputed masks ---------------------------------------------
def _set_dropout(layer, p):
    for m in layer.modules():
        if isinstance(m, nn.Dropout):
            m.p = p
    layer.self_attn.dropout = p


def _train_stack(p, num_layers=2):
    """HipTransformerEncoder on the weights test_matches_torch_transformer_encoder uses (O(1) scale, non-trivial LayerNorm
    weights, layer 1 different from layer 0), dropout p, train mode; with its per-layer state_dicts in float64 on the CPU."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    layer = _layer()
    _set_dropout(layer, p)
    enc = HipTransformerEncoder(layer, num_layers=num_layers)
    with torch.no_grad():
        for lyr in enc.layers[1:]:
            for i, q in enumerate(lyr.parameters()):
                q.copy_(torch.randn(q.shape, generator=torch.Generator().manual_seed(100 + i)) * 0.3)
    sds = [{k: v.detach().double().clone() for k, v in lyr.state_dict().items()} for lyr in enc.layers]
    return enc.cuda().train(), sds


def _drawn_seed(k):
    """The dropout seed HipTransformerEncoder.forward draws right after torch.manual_seed(k)."""
    torch.manual_seed(k)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _restated(x, sds, masks, dy):
    """oracle.student.encoder_layer over the stack in x's dtype with constant masks: (y, dx, {layer.name: gradient})."""
    from oracle import student as os_
    sds = [{k: v.to(x.dtype).requires_grad_(True) for k, v in sd.items()} for sd in sds]
    x = x.clone().requires_grad_(True)
    y = x
    for sd, m in zip(sds, masks):
        y = os_.encoder_layer(y, sd, 2, None if m is None else tuple(t.to(x.dtype) for t in m))
    y.backward(dy.to(x.dtype))
    return y.detach(), x.grad, {f"layers.{l}.{k}": v.grad for l, sd in enumerate(sds) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _train_reference(B, S, p):
    """Inputs, the seed of torch.manual_seed(1000 + B) and the float64 restatement of one train-mode forward / backward;
    computed once per case, shared by the runs of both kernel paths, never modified."""
    from oracle import token_dropout as td
    _, sds = _train_stack(p)
    g = torch.Generator().manual_seed(B + S)
    x = torch.randn(B, S, 32, generator=g)
    dy = torch.randn(B, S, 32, generator=g)
    seed = _drawn_seed(1000 + B)
    masks = td.stack_masks(B, S, 2, 128, p, seed, 2)
    return x, dy, seed, masks, _restated(x.double(), sds, masks, dy)


TRAIN_CASES = [(1, 1, 0.1), (2, 2, 0.5), (5, 2, 0.1), (37, 3, 0.1), (20, 5, 0.3), (33, 8, 0.1), (601, 3, 0.1),
               (10800, 3, 0.1), (8200, 4, 0.1)]


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("B,S,p", TRAIN_CASES)
def test_train_mode_matches_the_masked_float64_restatement(B, S, p, fused, monkeypatch):
    """Dropout ON: output, input gradient and every parameter gradient of HipTransformerEncoder against
    oracle.student.encoder_layer in float64 with the masks oracle/token_dropout.py recomputes from the drawn seed --
    a reference that shares no code with the library.  ``fused`` = 1: k_token_fwd / k_token_bwd where the library
    dispatches to them (the defaults); 0: the launch-per-operation forward and backward.  Cases: (1, 1) R < 4 and a
    one-entry softmax; (2, 2, 0.5) scale 2; (5, 2), (37, 3) one sample per backward workgroup; (20, 5, 0.3), (33, 8)
    S > 4 (16-sample forward workgroups, launch-per-operation backward either way); (601, 3) two samples per workgroup,
    ragged; (10800, 3) full 42 / 21-sample workgroups, ragged, backward grid 515; (8200, 4) 32 / 16 samples, ragged.
    Bounds: those of test_matches_torch_transformer_encoder for the same network with dropout off -- output
    2e-5 * max(1, max|y|), gradients 1e-4 of the tensor's largest entry + 1e-6; a wrong mask on one element is an
    O(0.1 .. 1) error.  Measured on the MI355X, worst over the cases and both path settings: output 3.5 %, input gradient
    2.0 %, parameter gradients 1.6 % of the bound (the same restatement in float32 on the CPU: up to 4.8 %), so the
    bounds stand unwidened.  Every figure is printed before the assertions (pytest -s)."""
    x, dy, seed, masks, (yr, dxr, gr) = _train_reference(B, S, p)
    assert masks[0][0].shape == (B, 2, S, S)
    if B * S * S >= 64:                                   # nhead = 2, and the two heads do not share a mask
        assert not torch.equal(masks[0][0][:, 0], masks[0][0][:, 1])
    enc, _ = _train_stack(p)
    assert enc.layers[0].self_attn.num_heads == 2
    monkeypatch.setenv("IGI_TOKEN_FUSED", fused)
    monkeypatch.setenv("IGI_TOKEN_FUSED_BWD", fused)
    torch.manual_seed(1000 + B)                           # the encoder's draw is the next one: seed
    xm = x.cuda().requires_grad_(True)
    ym = enc(xm)
    ym.backward(dy.cuda())
    assert [n for n, _ in enc.named_parameters()] == list(gr)
    figs = [("y", (ym.detach().double().cpu() - yr).abs().max().item(), 2e-5 * max(1.0, yr.abs().max().item())),
            ("dx", (xm.grad.double().cpu() - dxr).abs().max().item(), 1e-4 * dxr.abs().max().item() + 1e-6)]
    for n, q in enc.named_parameters():
        assert q.grad is not None, n
        figs.append((n, (q.grad.double().cpu() - gr[n]).abs().max().item(), 1e-4 * gr[n].abs().max().item() + 1e-6))
    for n, err, bound in figs:
        print(f"[train {B}x{S} p={p} fused={fused}] {n}: err {err:.3e} bound {bound:.3e}")
    assert not [f for f in figs if not f[1] <= f[2]]


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("B,S", [(37, 3), (33, 8)])
def test_feed_forward_site_mask_is_the_restated_one(B, S, fused, monkeypatch):
    """Mask probe: all parameters zero, linear2.bias = 1 -> every layer adds drop(1) to a zero residual stream, so the
    output IS the feed-forward-site mask (site 4 l + 3, element row * 32 + f).  One layer: y = the restated mask of layer
    0, element for element; two layers: y (1 - p) = the sum of the keep patterns of layers 0 and 1.  Explicit seed with
    a non-zero high word.  If this fails, the restatement (hash, threshold, element or site number) is what is wrong."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    from oracle import token_dropout as td
    monkeypatch.setenv("IGI_TOKEN_FUSED", fused)
    layer = _layer()
    with torch.no_grad():
        for q in layer.parameters():
            q.zero_()
        layer.linear2.bias.fill_(1.0)
    p, seed = 0.1, 0x2B5C9D1E00F0A7C3
    assert seed > 2 ** 32
    keep = [torch.from_numpy(td.layer_masks(B, S, 2, 128, p, seed, l)[3] != 0) for l in (0, 1)]
    assert not torch.equal(keep[0], keep[1]) and 0.8 < keep[0].float().mean() < 0.97
    x = torch.zeros(B, S, 32, device="cuda")
    for num_layers in (1, 2):
        enc = HipTransformerEncoder(layer, num_layers=num_layers).cuda()
        y, _ = torch.ops.mi355ppo.token_encoder_fwd(x, enc.flat_parameters().contiguous(), 2, 128, num_layers, p, True, seed)
        y = y.cpu()
        if num_layers == 1:
            assert torch.equal(y != 0, keep[0]), (y != 0).ne(keep[0]).sum().item()
        want = sum(k.float() for k in keep[:num_layers])
        assert torch.allclose(y * (1 - p), want, rtol=0, atol=1e-6), (y * (1 - p) - want).abs().max().item()


def test_eval_mode_ignores_dropout_probability_and_seed():
    """training = False with p = 0.1 is bit-equal to p = 0 in train mode, whatever the seed: output, input gradient,
    parameter gradient."""
    enc, _ = _train_stack(0.1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 3, 32, generator=g).cuda()
    dy = torch.randn(37, 3, 32, generator=g).cuda()
    flat = enc.flat_parameters().detach().contiguous()

    def run(p, training, seed):
        xm, fm = x.clone().requires_grad_(True), flat.clone().requires_grad_(True)
        y, _ = torch.ops.mi355ppo.token_encoder_fwd(xm, fm, 2, 128, 2, p, training, seed)
        y.backward(dy)
        return y.detach(), xm.grad, fm.grad

    base = run(0.0, True, 3)
    for got in (run(0.1, False, 3), run(0.1, False, 0x2B5C9D1E00F0A7C3)):
        for a, b in zip(base, got):
            assert torch.equal(a, b)
    assert not torch.equal(base[0], run(0.1, True, 3)[0])
    enc.eval()                                               # and through the module
    assert torch.equal(enc(x), base[0])
