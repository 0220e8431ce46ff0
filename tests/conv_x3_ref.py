"""CPU restatement of the split-bf16 arithmetic of the tactile convolutions (igi_conv_set_bf16x3; csrc/gemm_dma.h,
gemm_dma_conv_x3_kernel), shared by tests/test_conv_x3_cpu.py, tests/test_gpu_tactile_x3.py and tools/conv_x3_accuracy.py.

    x = hi + mid + lo      hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)   (nearest even; the differences
                           are exact in fp32)
    a * w = mid*mid + lo*hi + hi*lo + mid*hi + hi*mid + hi*hi       (a plane first, w plane second; smallest first)

Every plane product is exact in fp32; the kernel adds the sixteen products of a 16-k step and the accumulator inside one
v_mfma_f32_32x32x16_bf16 per plane pair, in the order above, and walks the reduction in 16-k steps.  The order INSIDE one
instruction is the hardware's; this restatement uses torch's fp32 matmul for it.

Range of the exact split: 2^-103 <= |x| <= the largest bf16 whatever the denormal mode (no subnormal arises anywhere);
with gradual underflow -- torch on the CPU, this file -- down to |x| >= 2^-110 (LO_EXACT_MIN), below which lo rounds."""
import torch

# (plane of a, plane of w) in issue order; 0 = hi, 1 = mid, 2 = lo
SIX = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))
NINE = ((2, 2), (2, 1), (1, 2)) + SIX
LO_EXACT_MIN = 2.0 ** -110      # smallest binade whose ulp (2^-133) is still a bf16 (subnormal) number
NORMAL_EXACT_MIN = 2.0 ** -103  # ... whose ulp (2^-126) is still a NORMAL bf16 / fp32 number


def split3(x):
    """fp32 tensor -> (hi, mid, lo), each an fp32 tensor holding a bf16 value"""
    assert x.dtype == torch.float32
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    q = r - mid
    lo = q.bfloat16().float()
    return hi, mid, lo


def contract(a, w, products=6, kstep=16):
    """(M, K) x (N, K) -> (M, N): the six (or nine) plane products per 16-k step in the kernel's issue order, fp32"""
    assert a.dtype == torch.float32 and w.dtype == torch.float32 and a.shape[1] == w.shape[1]
    pairs = {6: SIX, 9: NINE}[products]
    pa, pw = split3(a), split3(w)
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], kstep):
        for i, j in pairs:
            acc = acc + pa[i][:, k0:k0 + kstep] @ pw[j][:, k0:k0 + kstep].t()
    return acc


def bf16r(t):
    """the ONE-plane mode's rounding (igi_conv_set_bf16_inputs): nearest even to bf16, back in t's dtype"""
    return t.float().bfloat16().to(t.dtype)
