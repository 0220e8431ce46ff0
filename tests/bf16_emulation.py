"""CPU statement of the bf16-input mode's Linear arithmetic, shared by tests/test_bf16_mode_cpu.py and the teacher test of
the mode (tests/test_gpu_teacher.py): an autograd Function for ``torch.nn.functional.linear`` that rounds BOTH operands of
the forward, the data-gradient and the weight-gradient product to bf16 (nearest even) and multiplies in the operands'
own precision -- fp64 in the tests, so that rounding is the only difference from the exact product.  The bias and the
bias gradient are never rounded."""
import contextlib

import torch


def bf16r(t):
    """round to nearest even to bf16, back in t's dtype (the values pass through fp32: on the device they ARE fp32)"""
    return t.float().bfloat16().to(t.dtype)


class RoundedLinear(torch.autograd.Function):
    """y = rnd(x) rnd(W)^T + b;  dx = rnd(dy) rnd(W);  dW = rnd(dy)^T rnd(x);  db = column sums of dy"""

    @staticmethod
    def forward(ctx, x, weight, bias, rnd):
        ctx.save_for_backward(x, weight)
        ctx.rnd, ctx.has_bias = rnd, bias is not None
        y = rnd(x) @ rnd(weight).t()
        return y + bias if bias is not None else y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        rnd = ctx.rnd
        dyr = rnd(dy)
        dy2, x2 = dyr.reshape(-1, dy.shape[-1]), rnd(x).reshape(-1, x.shape[-1])
        dx = dyr @ rnd(weight)
        dw = dy2.t() @ x2
        db = dy.reshape(-1, dy.shape[-1]).sum(0) if ctx.has_bias else None
        return dx, dw, db, None


@contextlib.contextmanager
def patched_linear(rnd):
    """torch.nn.functional.linear computes in fp64 for the block -- every operand is taken to double first -- with both
    operands of its three products passed through ``rnd`` (None: plain autograd in fp64)."""
    orig = torch.nn.functional.linear

    def linear(x, weight, bias=None):
        x, weight = x.double(), weight.double()
        bias = bias.double() if bias is not None else None
        if rnd is None:
            return orig(x, weight, bias)
        return RoundedLinear.apply(x, weight, bias, rnd)

    torch.nn.functional.linear = linear
    try:
        yield
    finally:
        torch.nn.functional.linear = orig


def oracle_first_step_grad(orc, rnd):
    """The raw gradient of optimizer step 0 of a prepared oracle.teacher.TeacherOracle (record_grads=1, max_steps=1) with
    its Linears under patched_linear(rnd), per parameter name, as fp64 tensors.  (The step writes the fresh mu / sigma
    back into the rollout arena: those two are taken to fp64 first.)"""
    for k in ("mus", "sigmas"):
        orc.data[k] = orc.data[k].double()
    with patched_linear(rnd):
        flat = orc.update(record_grads=1, max_steps=1)["grads"][0].double()
    out, o = {}, 0
    for k, q in orc.p.items():
        out[k] = flat[o:o + q.numel()].reshape(q.shape)
        o += q.numel()
    assert o == flat.numel()
    return out
