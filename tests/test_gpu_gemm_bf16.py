"""The opt-in bf16-input mode of the Linear products (igi_gemm_set_bf16_inputs / IGI_GEMM_BF16=1) through igi_gemm_f32 and
through the ``linear`` / ``linear_bwd`` ops, and the exact-split experiment (igi_gemm_set_bf16x3).

Arithmetic under test: every product term is float(bf16(a)) * float(bf16(b)) (round to nearest even, exact in fp32),
accumulated in fp32 by v_mfma_f32_32x32x16_bf16; bias, activations and their derivatives are the fp32 path's.

Reference and bound (those of test_gpu_gemm.py and test_gpu_tactile_bf16.py):
    ref  = bf16r(a).double() @ bf16r(b).double().T        bf16r(t) = t.float().bfloat16().to(t.dtype)
    |err| <= 2e-6 * (|bf16r(a)| @ |bf16r(b)|.T) + 1e-6    per entry, epilogues applied to the rounded product
Every case runs with the switch off and on (restored in ``finally``) and is classified by outcome:
    bf16: the mode-on result meets the rounded bound AND the un-rounded fp64 product of the same operands violates that
          bound somewhere (rounding moves every term by up to 2^-9: for Gaussian operands the violation is over 250x);
    fp32: the mode-on result is bit-identical to the mode-off result.
CASES below is the written statement of today's dispatch (gemm() in csrc/gemm_dma.h): a product is bf16 under the switch
when it is k-contiguous in A, not gathered, takes the LDS-DMA kernel, has N > 64, more than 128 tiles of 128 x 128 and
K > 32; everything else stays fp32.  A tuning change edits that one table.

Measured on an MI355X (worst err / bound per group): see DESIGN.md, "What the bf16-input tests establish"."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, FP32 = "bf16", "fp32"


def _bf16r(t):
    """round to nearest even to bf16, back in t's dtype"""
    return t.float().bfloat16().to(t.dtype)


class _switch:
    """igi_gemm_set_bf16_inputs / igi_gemm_set_bf16x3 for a block; the previous setting is restored on exit"""

    def __init__(self, value, which="igi_gemm_set_bf16_inputs"):
        self.value, self.which = int(value), which

    def __enter__(self):
        from isaacgyminsertion_amd import _lib
        self.fn = getattr(_lib.lib(), self.which)
        self.prev = self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(self.prev)
        return False


def _switches():
    """(bf16 inputs, x3) as they stand -- read by setting and putting back"""
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    a = L.igi_gemm_set_bf16_inputs(0)
    L.igi_gemm_set_bf16_inputs(a)
    b = L.igi_gemm_set_bf16x3(0)
    L.igi_gemm_set_bf16x3(b)
    return a, b


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, seed):
    """operands and both fp64 products, computed once per shape and shared by the layouts (left unchanged)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(N, K, generator=g) * 0.3
    bias = torch.randn(N, generator=g)
    aux = torch.tanh(torch.randn(M, N, generator=g))
    c0 = torch.randn(M, N, generator=g)
    ar, br = _bf16r(a).double(), _bf16r(b).double()
    return dict(a=a, b=b, bias=bias, aux=aux, c0=c0, ref_r=ar @ br.t(), mag_r=ar.abs() @ br.abs().t(),
                ref_x=a.double() @ b.double().t())


def _gemm(akc, bkc, a, b, c0, bias, aux, epi, accumulate):
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    (M, K), N = a.shape, b.shape[0]
    A = (a if akc else a.t()).contiguous().cuda()
    B = (b if bkc else b.t()).contiguous().cuda()
    Cd, biasd, auxd = c0.clone().cuda(), bias.cuda(), aux.cuda()
    rc = L.igi_gemm_f32(int(akc), int(bkc), M, N, K, _lib.ptr(A), K if akc else M, _lib.ptr(B), K if bkc else N,
                        _lib.ptr(Cd), N, _lib.ptr(biasd), _lib.ptr(auxd), N, epi, accumulate, _lib.current_stream())
    _lib.check(rc, "igi_gemm_f32")
    torch.cuda.synchronize()
    return Cd.cpu()


def _epilogue(ref, o, epi):
    """the fused epilogues of include/igi_ppo.h on an fp64 product (as test_gpu_gemm.py::_run applies 1, 2, 3)"""
    bias, aux = o["bias"].double(), o["aux"].double()
    if epi == 1:
        return torch.tanh(ref + bias)
    if epi == 2:
        return ref * (1.0 - aux ** 2)
    if epi == 3:
        return ref + bias
    if epi == 4:
        return torch.relu(ref + bias)
    if epi == 5:
        return ref * (aux > 0)
    if epi == 6:
        return torch.nn.functional.elu(ref + bias)
    if epi == 7:
        return ref * torch.where(aux > 0, torch.ones_like(aux), aux + 1.0)
    return ref


def _classify(on, off, ref_r, ref_x, bound, tag):
    """-> (class or None, worst err / bound of the mode-on result, the un-rounded product's worst err / bound)"""
    worst = float(((on.double() - ref_r).abs() / bound).max())
    viol = float(((on.double() - ref_x).abs() / bound).max())
    same = torch.equal(on, off)
    print(f"[{tag}] mode on: max err / bound = {worst:.3f} against the rounded product, {viol:.1f} against the "
          f"un-rounded one; bit-identical to mode off: {same}")
    if same:
        return FP32, worst, viol
    if worst <= 1.0 and viol > 1.0:
        return BF16, worst, viol
    return None, worst, viol


def _run_case(akc, bkc, M, N, K, epi=0, accumulate=0):
    o = _operands(M, N, K, M + N + K)
    args = (akc, bkc, o["a"], o["b"], o["c0"], o["bias"], o["aux"], epi, accumulate)
    with _switch(0):
        off = _gemm(*args)
    with _switch(1):
        on = _gemm(*args)
    acc = o["c0"].double() if accumulate else 0.0
    bound = 2e-6 * (o["mag_r"] + (o["c0"].abs().double() if accumulate else 0.0)) + 1e-6
    ref_r, ref_x = _epilogue(o["ref_r"] + acc, o, epi), _epilogue(o["ref_x"] + acc, o, epi)
    tag = f"{'T' if akc else 'F'}{'T' if bkc else 'F'} {M}x{N}x{K} epi{epi} acc{accumulate}"
    cls, worst, viol = _classify(on, off, ref_r, ref_x, bound, tag)
    # the fp32 path itself, against the un-rounded product and ITS bound (what test_gpu_gemm.py states)
    bound_x = 2e-6 * (o["a"].abs().double() @ o["b"].abs().double().t() +
                      (o["c0"].abs().double() if accumulate else 0.0)) + 1e-6
    worst_off = float(((off.double() - ref_x).abs() / bound_x).max())
    assert worst_off <= 1.0, (tag, "mode off", worst_off)
    return cls, worst, viol


# (id, a_kcontig, b_kcontig, M, N, K, epilogue, accumulate, expected class)
CASES = [
    # bf16: both B layouts; 129 m-tiles with one row in the last, two k-tiles (prologue only)
    ("tt-16385x128x64", 1, 1, 16385, 128, 64, 0, 0, BF16),
    ("tf-16385x128x64", 1, 0, 16385, 128, 64, 0, 0, BF16),
    # second n-tile half empty, three k-tiles
    ("tt-8200x192x96", 1, 1, 8200, 192, 96, 0, 0, BF16),
    ("tf-8200x192x96", 1, 0, 8200, 192, 96, 0, 0, BF16),
    # the two-stage ring wraps sixteen times
    ("tt-4100x512x1024", 1, 1, 4100, 512, 1024, 0, 0, BF16),
    ("tf-4100x512x1024", 1, 0, 4100, 512, 1024, 0, 0, BF16),
    # N not a multiple of 4: the narrow (element-wise) epilogue
    ("tt-8320x130x64", 1, 1, 8320, 130, 64, 0, 0, BF16),
    # every fused epilogue of the enum on the bf16 tile; epilogue 2 at TF is the data gradient's real form
    ("tt-epi1", 1, 1, 8320, 256, 128, 1, 0, BF16),
    ("tt-epi2", 1, 1, 8320, 256, 128, 2, 0, BF16),
    ("tt-epi3", 1, 1, 8320, 256, 128, 3, 0, BF16),
    ("tt-epi4", 1, 1, 8320, 256, 128, 4, 0, BF16),
    ("tt-epi5", 1, 1, 8320, 256, 128, 5, 0, BF16),
    ("tt-epi6", 1, 1, 8320, 256, 128, 6, 0, BF16),
    ("tt-epi7", 1, 1, 8320, 256, 128, 7, 0, BF16),
    ("tf-epi2", 1, 0, 8320, 256, 128, 2, 0, BF16),
    # fp32 by the rule
    ("tt-16384x128x64-exactly-128-tiles", 1, 1, 16384, 128, 64, 0, 0, FP32),
    ("tt-16385x128x32-one-k-tile", 1, 1, 16385, 128, 32, 0, 0, FP32),
    ("tt-16385x64x64-narrow", 1, 1, 16385, 64, 64, 0, 0, FP32),
    ("ff-8320x256x128", 0, 0, 8320, 256, 128, 0, 0, FP32),
    ("ft-8320x256x128", 0, 1, 8320, 256, 128, 0, 0, FP32),
    ("tt-8320x256x128-accumulate", 1, 1, 8320, 256, 128, 0, 1, FP32),
    ("tt-8320x256x48-k48", 1, 1, 8320, 256, 48, 0, 0, FP32),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_product_class_under_the_switch(case):
    """Each product of CASES, switch off and on, lands in the class the table states (module docstring).
    Measured on an MI355X: worst err / bound of the bf16 cases against the rounded product 0.061 (plain products), 0.058
    (epilogues); the un-rounded product of the same operands misses the bound by 286x - 1246x; the fp32 cases are at
    <= 0.2 of the un-rounded bound.  The switch is as it was afterwards."""
    _id, akc, bkc, M, N, K, epi, accumulate, want = case
    start = _switches()
    cls, worst, viol = _run_case(akc, bkc, M, N, K, epi, accumulate)
    assert cls == want, (case, cls, worst, viol)
    assert _switches() == start


def _rounding_operand(rows=16512, cols=128):
    """Rows 0 .. rows/2: standard normals.  The rest: column j holds the tie t_j = 1 + (2 j + 1) 2^-8 -- all 128 ties of
    a binade; each goes to the neighbour with an even 7-bit mantissa: 1 + 2^-8 -> 1 (down), 1 + 3 * 2^-8 -> 1 + 2^-6
    (up), 64 of either direction -- exactly (row % 3 == 0), one fp32 ulp above it (1) or below it (2), scaled by 2^e
    with e walking -120 .. 120 over the rows (every exponent short of the subnormals and of overflow) and negated in
    every other block of 241 rows."""
    g = torch.Generator().manual_seed(77)
    a = torch.randn(rows, cols, generator=g)
    half = rows // 2
    r = torch.arange(rows - half)
    ties = 1.0 + (2.0 * torch.arange(cols, dtype=torch.float64) + 1.0) * 2.0 ** -8      # exact in fp32 (8 fraction bits)
    t = ties.float().view(torch.int32).repeat(rows - half, 1)
    t = t + torch.tensor([0, 1, -1], dtype=torch.int32)[r % 3].unsqueeze(1)               # +- one fp32 ulp
    v = t.view(torch.float32).double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), (r % 241 - 120).double()).unsqueeze(1)
    v = v * torch.where((r // 241) % 2 == 1, -1.0, 1.0).double().unsqueeze(1)
    a[half:] = v.float()                                                                   # a power-of-two scaling: exact
    assert torch.equal(a[half:].double(), v)
    return a


def _rne_bits(a):
    """bf16 round-to-nearest-even of finite fp32 values in integer arithmetic (independent of torch's conversion)"""
    u = a.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("bkc", [1, 0], ids=["tt", "tf"])
def test_rounding_is_to_nearest_even_exactly(bkc):
    """C = A @ P^T with P an asymmetric permutation matrix: every output is ONE rounded operand times one (the other 127
    products of its row are exact zeros), so C == bf16r(A)[:, perm] bit for bit -- ties to even in both directions at every
    exponent from 2^-120 to 2^120, their negatives, the values one fp32 ulp either side of a tie, and normals.
    Truncation, round-half-up, or a swap of the k 0-7 and k 8-15 halves between the lane groups each fail it; the
    permutation (perm[n] != n, not an involution) catches a transposed B image.
    Kept out: values that round to a bf16 subnormal or to infinity (inf * 0 would poison the row, and the matrix
    unit's handling of subnormal inputs is not something this project states); each row holds ONE magnitude, so no
    product of a row is below another's rounding unit."""
    from isaacgyminsertion_amd import _lib  # noqa: F401
    a = _rounding_operand()
    M, K = a.shape
    N = K
    perm = (torch.arange(N) * 37 + 11) % N                     # 37 is odd: a bijection of 0..127 with no fixed structure
    assert sorted(perm.tolist()) == list(range(N)) and not torch.equal(perm[perm], torch.arange(N))
    p = torch.zeros(N, K)
    p[torch.arange(N), perm] = 1.0                             # P(n, k) = [k == perm[n]]
    want = _bf16r(a)
    assert torch.equal(want, _rne_bits(a))
    assert bool(torch.isfinite(want).all()) and float(want.abs().min()) >= 2.0 ** -126
    assert int((want != a).sum()) > a.numel() // 2             # the operand is not representable: rounding happens
    want = want[:, perm]
    zero = torch.zeros(M, N)
    start = _switches()
    with _switch(1):
        got = _gemm(1, bkc, a, p, zero, torch.zeros(N), zero, 0, 0)
    with _switch(0):
        off = _gemm(1, bkc, a, p, zero, torch.zeros(N), zero, 0, 0)
    assert _switches() == start
    assert torch.equal(off, a[:, perm])                        # the fp32 path passes the operand through
    bad = (got != want)
    assert not bool(bad.any()), (int(bad.sum()), torch.nonzero(bad)[:8].tolist())


def test_exact_split_experiment():
    """igi_gemm_set_bf16x3(9) and (6) at 8320 x 256 x 256 (k-contiguous operands, 130 tiles) both meet the fp32 bound
    against the UN-rounded fp64 product (the terms 6 drops are below 2^-26 of each product), both differ from the
    bf16-input mode's result; a K = 128 product is bit-identical to switch-off; the switch ends at 0.
    Measured on an MI355X: max err / bound 0.141 (9 products), 0.141 (6 products)."""
    M, N, K = 8320, 256, 256
    o = _operands(M, N, K, M + N + K)
    args = (1, 1, o["a"], o["b"], o["c0"], o["bias"], o["aux"], 0, 0)
    bound = 2e-6 * (o["a"].abs().double() @ o["b"].abs().double().t()) + 1e-6
    start = _switches()
    assert start == (0, 0)
    with _switch(1):
        bf = _gemm(*args)
    for products in (9, 6):
        with _switch(products, "igi_gemm_set_bf16x3"):
            assert _switches() == (0, products)
            got = _gemm(*args)
        worst = float(((got.double() - o["ref_x"]).abs() / bound).max())
        print(f"[x3 = {products}] max err / bound against the un-rounded product = {worst:.3f}")
        assert worst <= 1.0, (products, worst)
        assert not torch.equal(got, bf)
    o2 = _operands(M, N, 128, M + N + 128)
    args2 = (1, 1, o2["a"], o2["b"], o2["c0"], o2["bias"], o2["aux"], 0, 0)
    off = _gemm(*args2)
    with _switch(9, "igi_gemm_set_bf16x3"):
        on = _gemm(*args2)
    assert torch.equal(on, off)
    assert _switches() == (0, 0)


def test_mode_on_is_reproducible():
    """two mode-on runs of the ragged case (8200 x 192 x 96, TF) are bit-identical"""
    o = _operands(8200, 192, 96, 8200 + 192 + 96)
    args = (1, 0, o["a"], o["b"], o["c0"], o["bias"], o["aux"], 0, 0)
    with _switch(1):
        first = _gemm(*args)
        second = _gemm(*args)
    assert torch.equal(first, second)
    assert _switches() == (0, 0)


# ---- the mode through the ops (torch.ops.mi355ppo.linear / linear_bwd -> csrc/linear.h)

def _linear_ops(rows, inf, outf, need_dw, seed):
    """forward (act none, with bias) and backward of one Linear through the ops, switch off and on"""
    from isaacgyminsertion_amd import ops  # noqa: F401
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, inf, generator=g)
    w = torch.randn(outf, inf, generator=g) / inf ** 0.5
    b = torch.randn(outf, generator=g) * 0.1
    dy = torch.randn(rows, outf, generator=g)
    out = {}
    for on in (0, 1):
        with _switch(on):
            xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
            y = torch.ops.mi355ppo.linear(xd, wd, bd, 0)
            dx, dw, db = torch.ops.mi355ppo.linear_bwd(xd, wd, y, dyd, 0, True, need_dw, need_dw)
            torch.cuda.synchronize()
            out[on] = dict(y=y.cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())
    return x, w, b, dy, out


def test_linear_op_training_layer():
    """``linear`` at 16640 rows, 64 -> 128 (130 tiles): the forward is in the bf16 class.  Its backward with dW and dx
    wanted is gemm_dma_mlp_level_kernel, fp32 in either mode: dx, dW and db are bit-identical to switch-off.
    Measured on an MI355X: forward max err / bound 0.056 against the rounded product, 1030 against the un-rounded one."""
    x, w, b, dy, out = _linear_ops(16640, 64, 128, True, 21)
    xr, wr = _bf16r(x).double(), _bf16r(w).double()
    bound = 2e-6 * (xr.abs() @ wr.abs().t()) + 1e-6
    cls, worst, viol = _classify(out[1]["y"], out[0]["y"], xr @ wr.t() + b.double(), x.double() @ w.double().t() + b.double(),
                                 bound, "linear fwd 16640 x 64 -> 128")
    assert cls == BF16, (cls, worst, viol)
    for k in ("dx", "dw", "db"):
        assert out[1][k].numel() > 0 and torch.equal(out[1][k], out[0][k]), k
    assert _switches() == (0, 0)


def test_linear_op_frozen_layer():
    """A frozen layer (dx only) at 16640 rows, 128 -> 64: the data gradient goes through gemm() and is in the bf16 class
    against bf16r(dy) @ bf16r(W); the same op at 256 rows (two tiles) is bit-identical to switch-off.  (The split
    between this and the training layer above is written down in DESIGN.md.)
    Measured on an MI355X: dx max err / bound 0.042 against the rounded product, 985 against the un-rounded one."""
    x, w, b, dy, out = _linear_ops(16640, 128, 64, False, 22)
    dyr, wr = _bf16r(dy).double(), _bf16r(w).double()
    bound = 2e-6 * (dyr.abs() @ wr.abs()) + 1e-6
    cls, worst, viol = _classify(out[1]["dx"], out[0]["dx"], dyr @ wr, dy.double() @ w.double(), bound,
                                 "frozen dx 16640 x 128 -> 64")
    assert cls == BF16, (cls, worst, viol)
    assert out[1]["dw"].numel() == 0 and out[1]["db"].numel() == 0
    # the forward of this layer has 64 outputs: fp32
    assert torch.equal(out[1]["y"], out[0]["y"])
    _x, _w, _b, _dy, small = _linear_ops(256, 128, 64, False, 23)
    assert torch.equal(small[1]["dx"], small[0]["dx"]) and torch.equal(small[1]["y"], small[0]["y"])
    assert _switches() == (0, 0)
