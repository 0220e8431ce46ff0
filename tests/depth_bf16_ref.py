"""CPU restatement of the depth backbone (DepthOnlyFCBackbone54x96, csrc/depth.h) with the arithmetic of its opt-in
bf16-input mode (igi_depth_set_bf16_inputs), shared by tests/test_gpu_depth_bf16.py, tests/test_depth_bf16_cpu.py and
tools/depth_bf16_accuracy.py.

Under the mode every product term of conv2 (forward, data gradient, weight gradient) and of the 64768 -> 128 Linear
(forward, data gradient, weight gradient) is float(bf16(a)) * float(bf16(b)); conv1 with its max-pool, the 128 -> latent
Linear, the biases, the bias-gradient sums, ELU and ELU' are plain.  ``rnd`` below is that rounding (``bf16r``), or the
identity: with the identity ``forward`` + ``backward`` are oracle/encoders.py:depth_backbone and its autograd gradient
(tests/test_depth_bf16_cpu.py holds them together in float64 to 1e-12), so the restatement is the reference's network.

``backward`` takes the activations as ARGUMENTS: the GPU test hands it the device's own a1 / arg-max bytes / a2 / h3, so
ELU' and the pool routing are the device's and no image has to be left out for a near-tie."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

KEYS = ["image_compression.%d.%s" % (i, n) for i in (0, 3, 6, 8) for n in ("weight", "bias")]
W1, B1, W2, B2, WF1, BF1, WF2, BF2 = KEYS


def bf16r(t):
    """round to nearest even to bf16, back in t's dtype (fp64 values pass through fp32 first, as on the device, where
    every operand is an fp32 value)"""
    return t.float().bfloat16().to(t.dtype)


def ident(t):
    return t


def elu_grad_from_out(a):
    """ELU'(z) from a = ELU(z): 1 where a > 0, else a + 1 (csrc: elu1_grad_from_out)"""
    return torch.where(a > 0, torch.ones_like(a), a + 1.0)


def pool_bytes(ind):
    """flat indices of F.max_pool2d(z, 2, 2, return_indices=True) on 50 x 92 maps -> the device's arg-max bytes
    (2 * dy + dx inside the 2 x 2 window), same shape"""
    py = torch.arange(25).view(1, 1, 25, 1)
    px = torch.arange(46).view(1, 1, 1, 46)
    iy, ix = ind // 92, ind % 92
    return ((iy - 2 * py) * 2 + (ix - 2 * px)).to(torch.uint8)


def pool_indices(idx):
    """the inverse: arg-max bytes (B, 32, 25, 46) -> flat indices into the 50 x 92 pre-pool maps"""
    py = torch.arange(25).view(1, 1, 25, 1)
    px = torch.arange(46).view(1, 1, 1, 46)
    pos = idx.long()
    return (2 * py + (pos >> 1)) * 92 + 2 * px + (pos & 1)


def forward(x, sd, rnd=bf16r):
    """the whole forward in x's dtype -> dict(a1, idx, a2, h3, y): NCHW maps, arg-max bytes as the device stores them"""
    z1 = F.conv2d(x, sd[W1], sd[B1])
    p1, ind = F.max_pool2d(z1, 2, 2, return_indices=True)
    a1 = F.elu(p1)
    a2 = F.elu(F.conv2d(rnd(a1), rnd(sd[W2]), None) + sd[B2].view(1, -1, 1, 1))
    h3 = F.elu(F.linear(rnd(a2.flatten(1)), rnd(sd[WF1]), None) + sd[BF1])
    return dict(a1=a1, idx=pool_bytes(ind), a2=a2, h3=h3, y=F.linear(h3, sd[WF2], sd[BF2]))


def backward(x, gy, sd, a1, idx, a2, h3, rnd=bf16r, chunk=64):
    """d<y, gy>/d(params) from the given activations, in x's dtype: every conv2 / fc1 operand (dz, activation, weight)
    passes through ``rnd`` before each product, bias gradients are plain sums, conv1's weight gradient is the plain
    product of the images with g1 routed to the arg-max positions.  Chunked over the batch (additive over images)."""
    g = {k: torch.zeros_like(v) for k, v in sd.items()}
    wf1r, w2r = rnd(sd[WF1]), rnd(sd[W2])
    for i in range(0, x.shape[0], chunk):
        s = slice(i, min(i + chunk, x.shape[0]))
        n = s.stop - s.start
        g[WF2] += gy[s].t() @ h3[s]
        g[BF2] += gy[s].sum(0)
        dz3 = (gy[s] @ sd[WF2]) * elu_grad_from_out(h3[s])
        dz3r, a2r = rnd(dz3), rnd(a2[s].flatten(1))
        g[WF1] += dz3r.t() @ a2r
        g[BF1] += dz3.sum(0)
        dz2 = (dz3r @ wf1r).view(n, 64, 23, 44) * elu_grad_from_out(a2[s])
        dz2r, a1r = rnd(dz2), rnd(a1[s])
        g[W2] += conv2d_weight(a1r, sd[W2].shape, dz2r)
        g[B2] += dz2.sum((0, 2, 3))
        g1 = conv2d_input(a1[s].shape, w2r, dz2r) * elu_grad_from_out(a1[s])
        dz1 = F.max_unpool2d(g1, pool_indices(idx[s]), 2, 2, output_size=(50, 92))
        g[W1] += conv2d_weight(x[s], sd[W1].shape, dz1)
        g[B1] += g1.sum((0, 2, 3))
    return g
