"""Weights, dropout masks and float64 references for the token encoder beyond 32 features (helper of
tests/test_token_wide_cpu.py and tests/test_gpu_token_encoder_wide.py; not a test).

``wide_masks`` restates the kernels' dropout element numbering for any width from oracle.token_dropout.keep_scale:

  site 4 l + 0  attention probabilities   element ((b * H + h) * S + i) * S + j     mask (B, H, S, S)
  site 4 l + 1  self-attention branch     element row * d + f,  row = b * S + s      mask (B, S, d)
  site 4 l + 2  GELU output               element row * ff + c                       mask (B, S, ff)
  site 4 l + 3  feed-forward branch       element row * d + f                        mask (B, S, d)

``wide_layer`` / ``wide_stack`` draw weights whose matrices shrink with sqrt(32 / fan_in): the activations then stay at
the magnitude of the 32-wide tests (max |y| about 20), so those tests' bounds carry over unchanged."""
import copy
import functools
import math

import numpy as np
import torch
import torch.nn as nn

# (d_model, nhead): the pairs the library takes beyond the stock (32, 2)
NEW_PAIRS = [(32, 1), (64, 4), (64, 2), (64, 1), (128, 8), (128, 4), (128, 2)]
REFUSED_PAIRS = [(48, 3), (64, 8), (96, 3), (256, 4), (128, 1)]


def wide_masks(B, S, H, d, ff, p, seed, layers):
    """The four masks of every layer as float64 torch tensors, in the shapes oracle.student.encoder_layer multiplies with."""
    from oracle import token_dropout as td
    att = np.arange(B * H * S * S, dtype=np.uint64).reshape(B, H, S, S)
    row = np.arange(B * S * d, dtype=np.uint64).reshape(B, S, d)
    hid = np.arange(B * S * ff, dtype=np.uint64).reshape(B, S, ff)
    return [tuple(torch.from_numpy(m) for m in (td.keep_scale(p, seed, 4 * l + td.SITE_ATTN, att),
                                                td.keep_scale(p, seed, 4 * l + td.SITE_SA, row),
                                                td.keep_scale(p, seed, 4 * l + td.SITE_FF_ACT, hid),
                                                td.keep_scale(p, seed, 4 * l + td.SITE_FF, row)))
            for l in range(layers)]


def _draw(named_parameters, gen):
    """matrices randn * 0.3 * sqrt(32 / fan_in); vectors randn * 0.2, plus 1 for the LayerNorm weights"""
    with torch.no_grad():
        for n, q in named_parameters:
            v = torch.randn(q.shape, generator=gen(n))
            if q.dim() > 1:
                v = v * (0.3 * math.sqrt(32.0 / q.shape[1]))
            else:
                v = v * 0.2 + (1.0 if n in ("norm1.weight", "norm2.weight") else 0.0)
            q.copy_(v)


def set_dropout(layer, p):
    for m in layer.modules():
        if isinstance(m, nn.Dropout):
            m.p = p
    layer.self_attn.dropout = p


def wide_layer(d, H, ff, seed=0):
    layer = nn.TransformerEncoderLayer(d_model=d, nhead=H, dim_feedforward=ff, activation="gelu", batch_first=True,
                                       norm_first=True)
    g = torch.Generator().manual_seed(seed)
    _draw(layer.named_parameters(), lambda n: g)
    return layer


def wide_stack(d, H, ff, layers, p=0.0, seed=0):
    """[layer modules] of a stack on the CPU in float32, dropout p: layer 0 = wide_layer, layer l >= 1 redrawn parameter by
    parameter from Generator().manual_seed(100 * l + i)."""
    out = []
    for l in range(layers):
        layer = wide_layer(d, H, ff, seed)
        if l:
            names = [n for n, _ in layer.named_parameters()]
            _draw(layer.named_parameters(), lambda n, l=l: torch.Generator().manual_seed(100 * l + names.index(n)))
        set_dropout(layer, p)
        out.append(layer)
    return out


def hip_encoder(stack):
    """HipTransformerEncoder holding the stack's weights (still on the CPU)."""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    enc = HipTransformerEncoder(stack[0], num_layers=len(stack))
    for mine, src in zip(enc.layers, stack):
        mine.load_state_dict(src.state_dict())
    return enc


def inputs(d, B, S):
    g = torch.Generator().manual_seed(B + S)             # (the 32-wide tests' convention)
    return torch.randn(B, S, d, generator=g), torch.randn(B, S, d, generator=g)


def torch_encoder(stack, dtype=torch.float64):
    """nn.TransformerEncoder on the stack's weights, dropout off."""
    ref = nn.TransformerEncoder(copy.deepcopy(stack[0]), num_layers=len(stack), enable_nested_tensor=False)
    for mine, src in zip(ref.layers, stack):
        mine.load_state_dict(src.state_dict())
        set_dropout(mine, 0.0)
    return ref.to(dtype)


def eval_run(stack, x, dy, dtype):
    """(y, dx, {name: gradient}) of nn.TransformerEncoder in ``dtype``, dropout off."""
    ref = torch_encoder(stack, dtype)
    xr = x.to(dtype).requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.to(dtype))
    return yr.detach(), xr.grad, {n: a.grad for n, a in ref.named_parameters()}


@functools.lru_cache(maxsize=None)
def eval_reference(d, H, ff, layers, B, S):
    """Inputs and the float64 nn.TransformerEncoder result of a dropout-off case: computed once, never modified."""
    x, dy = inputs(d, B, S)
    return (x, dy) + eval_run(wide_stack(d, H, ff, layers), x, dy, torch.float64)


def restated(stack, H, x, dy, masks, dtype):
    """oracle.student.encoder_layer over the stack in ``dtype`` with constant masks (None: no dropout)."""
    from oracle import student as os_
    sds = [{k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in lyr.state_dict().items()} for lyr in stack]
    xr = x.to(dtype).requires_grad_(True)
    y = xr
    for l, sd in enumerate(sds):
        y = os_.encoder_layer(y, sd, H, None if masks is None else tuple(t.to(dtype) for t in masks[l]))
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, {f"layers.{l}.{k}": v.grad for l, sd in enumerate(sds) for k, v in sd.items()}


def drawn_seed(k):
    """The dropout seed HipTransformerEncoder.forward draws right after torch.manual_seed(k)."""
    torch.manual_seed(k)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


@functools.lru_cache(maxsize=None)
def train_reference(d, H, ff, layers, B, S, p):
    """Inputs, the seed of torch.manual_seed(1000 + B), its masks and the float64 restatement of one train-mode forward /
    backward: computed once per case, never modified."""
    x, dy = inputs(d, B, S)
    seed = drawn_seed(1000 + B)
    masks = wide_masks(B, S, H, d, ff, p, seed, layers)
    return x, dy, seed, masks, restated(wide_stack(d, H, ff, layers, p), H, x, dy, masks, torch.float64)


def figures(y, dx, grads, yr, dxr, gr, grad_abs):
    """[(name, error, bound)] with the bounds of tests/test_gpu_token_encoder_long.py::_figures: y 2e-5 * max(1, max|y|),
    dx 1e-4 * max|dx| + grad_abs[0], parameters 1e-4 * max|g| + grad_abs[1].  y / dx / grads: the values under test."""
    figs = [("y", (y.double().cpu() - yr).abs().max().item(), 2e-5 * max(1.0, yr.abs().max().item())),
            ("dx", (dx.double().cpu() - dxr).abs().max().item(), 1e-4 * dxr.abs().max().item() + grad_abs[0])]
    for n, q in grads.items():
        figs.append((n, (q.double().cpu() - gr[n]).abs().max().item(), 1e-4 * gr[n].abs().max().item() + grad_abs[1]))
    return figs


def shares(figs):
    """worst share of its bound: (y, dx, parameters)"""
    return figs[0][1] / figs[0][2], figs[1][1] / figs[1][2], max(e / b for _, e, b in figs[2:])


# dropout off, against nn.TransformerEncoder float64: (d, H, ff, layers, B, S)
EVAL_CASES = [(64, 4, 256, 2, 37, 9), (64, 2, 256, 2, 5, 17), (64, 1, 256, 2, 3, 3), (64, 4, 256, 2, 130, 32),
              (128, 2, 512, 2, 37, 9), (128, 8, 512, 2, 67, 31), (128, 4, 512, 2, 130, 32), (128, 2, 100, 1, 5, 1),
              (32, 1, 128, 2, 33, 8), (64, 4, 256, 2, 4096, 5), (128, 2, 512, 3, 1, 32)]
# train mode, against oracle.student.encoder_layer float64 with wide_masks: (d, H, ff, layers, B, S, p)
TRAIN_CASES = [(64, 4, 256, 2, 33, 9, 0.1), (128, 2, 512, 2, 2, 17, 0.5), (128, 8, 512, 2, 130, 32, 0.1),
               (64, 2, 256, 2, 37, 3, 0.1), (32, 1, 128, 2, 100, 8, 0.1)]
