"""The grouped weight-gradient launchers (csrc/gemm_dma.h: gemm_wgrad_multi in fp32, gemm_wgrad_group's two grouped grids
in the bf16-input mode) on lists of this file's choosing, through the test entry igi_gemm_wgrad_group.  Before, they
were only reached through a whole teacher step, at 2e-4 of the largest gradient entry.

Per problem and batch entry (dz [rows][out], x [rows][in]; the split-K slabs are summed here in fp64):
    dW ref = dz.double().T @ x.double()        |err| <= 2e-6 * (|dz|.T @ |x|) + 1e-6     (abs-product over all rows)
    db ref = dz.double().sum(0)                |err| <= 2e-6 * sum|dz| + 1e-6             (never rounded, either mode)
In the bf16 class both operands of dW pass through bf16r first.  Classes as in test_gpu_gemm_bf16.py: bf16 = meets the
rounded bound while the un-rounded product violates it; fp32 = the raw slabs are bit-identical to the switch-off run.
Under the switch a problem is bf16 when it is eligible for the LDS-DMA kernel, has in > 64 and finds room among the four
entries of the 128-wide group; in <= 64 takes the fp32 64-wide group, anything else a launch of its own (fp32).

Every output buffer ends in a guard tail of NaN that must stay NaN, every element inside must be written (finite)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, FP32 = "bf16", "fp32"
GUARD = 64

# (out, in, rows, nbatch, splitk)
SIX = [
    (256, 128, 416, 1, 3),     # 13 k-tiles in three splits: 160, 160 and 96 rows (ragged last split)
    (128, 256, 416, 2, 1),     # two batched nets, two column tiles
    (512, 32, 256, 1, 1),      # <= 32 inputs: the 256 x 32 tile of the fp32 grid
    (8, 128, 128, 1, 1),       # eight outputs: one mostly empty row tile
    (128, 23, 256, 1, 1),      # in % 4 != 0: not eligible, runs on its own in the middle of the list
    (256, 64, 1024, 1, 4),     # the 64-wide tile, four even splits
]
SIX_CLASSES = [BF16, BF16, FP32, BF16, FP32, FP32]
SEVEN = [
    (128, 128, 128, 1, 1),
    (64, 64, 256, 1, 2),
    (256, 32, 256, 1, 1),
    (128, 192, 160, 1, 1),     # second column tile half empty
    (32, 128, 128, 2, 1),
    (128, 64, 128, 1, 1),
    (256, 128, 288, 1, 3),     # the seventh: DMA_MULTI_MAX = 6 entries are taken, it runs on its own (split-K, bias sums)
]
FIVE = [
    (128, 128, 256, 1, 1),
    (256, 128, 128, 1, 1),
    (64, 128, 416, 1, 3),
    (128, 128, 128, 2, 1),
    (256, 128, 256, 1, 2),     # the fifth 128-wide problem: DMA_GROUP_MAX = 4 entries are taken, so it is fp32
]
FIVE_CLASSES = [BF16, BF16, BF16, BF16, FP32]


def _bf16r(t):
    return t.float().bfloat16().to(t.dtype)


class _switch:
    def __init__(self, on):
        self.on = int(on)

    def __enter__(self):
        from isaacgyminsertion_amd import _lib
        self.prev = _lib.lib().igi_gemm_set_bf16_inputs(self.on)

    def __exit__(self, *exc):
        from isaacgyminsertion_amd import _lib
        _lib.lib().igi_gemm_set_bf16_inputs(self.prev)
        return False


@functools.lru_cache(maxsize=None)
def _inputs(shapes, seed):
    """host operands and fp64 references of one list (computed once, shared by the modes, left unchanged)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (o, i, rows, nb, sk) in shapes:
        dz = torch.randn(nb, rows, o, generator=g)
        x = torch.randn(nb, rows, i, generator=g) * 0.5
        d = dict(dz=dz, x=x)
        for tag, (a, b) in (("x", (dz.double(), x.double())), ("r", (_bf16r(dz).double(), _bf16r(x).double()))):
            d["ref_" + tag] = a.transpose(1, 2) @ b
            d["bound_" + tag] = 2e-6 * (a.abs().transpose(1, 2) @ b.abs()) + 1e-6
        d["db_ref"] = dz.double().sum(1)
        d["db_bound"] = 2e-6 * dz.double().abs().sum(1) + 1e-6
        out.append(d)
    return out


def _launch(shapes, seed, with_bias=True):
    """one call of the entry -> per problem the raw slabs (with their guard tails) on the host"""
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    ins = _inputs(tuple(shapes), seed)
    arr = (_lib.WgradProblem * len(shapes))()
    keep, outs = [], []
    for k, ((o, i, rows, nb, sk), d) in enumerate(zip(shapes, ins)):
        dz, x = d["dz"].cuda(), d["x"].cuda()
        dw = torch.full((sk * nb * o * i + GUARD,), float("nan"), device="cuda")
        db = torch.full((sk * nb * o + GUARD,), float("nan"), device="cuda") if with_bias else None
        keep.append((dz, x))
        outs.append((dw, db))
        arr[k] = _lib.WgradProblem(dz=dz.data_ptr(), x=x.data_ptr(), dweight=dw.data_ptr(),
                                   dbias=db.data_ptr() if with_bias else None, dz_batch_stride=rows * o,
                                   x_batch_stride=rows * i, lddz=o, ldx=i, out_features=o, in_features=i, rows=rows,
                                   nbatch=nb, splitk=sk)
    _lib.check(L.igi_gemm_wgrad_group(arr, len(shapes), _lib.current_stream()), "igi_gemm_wgrad_group")
    torch.cuda.synchronize()
    return [(dw.cpu(), db.cpu() if db is not None else None) for dw, db in outs]


def _sums(shape, raw):
    """guard tails untouched, everything inside written; -> (dW, db) with the slabs added in fp64"""
    (o, i, rows, nb, sk), (dw, db) = shape, raw
    assert bool(torch.isnan(dw[-GUARD:]).all()) and bool(torch.isfinite(dw[:-GUARD]).all()), shape
    w = dw[:-GUARD].double().reshape(sk, nb, o, i).sum(0)
    if db is None:
        return w, None
    assert bool(torch.isnan(db[-GUARD:]).all()) and bool(torch.isfinite(db[:-GUARD]).all()), shape
    return w, db[:-GUARD].double().reshape(sk, nb, o).sum(0)


def _ratios(shape, raw, d):
    w, b = _sums(shape, raw)
    r = float(((w - d["ref_r"]).abs() / d["bound_r"]).max())       # against the rounded product, its bound
    x = float(((w - d["ref_x"]).abs() / d["bound_x"]).max())       # against the un-rounded product, its bound
    xr = float(((w - d["ref_x"]).abs() / d["bound_r"]).max())      # the un-rounded product against the rounded bound
    bb = float(((b - d["db_ref"]).abs() / d["db_bound"]).max()) if b is not None else 0.0
    return r, x, xr, bb


def _check_fp32_list(shapes, seed, name):
    ins = _inputs(tuple(shapes), seed)
    first, second = _launch(shapes, seed), _launch(shapes, seed)
    for k, (shape, d) in enumerate(zip(shapes, ins)):
        _r, x, _xr, bb = _ratios(shape, first[k], d)
        print(f"[{name} fp32 mode] problem {k} {shape}: dW max err / bound = {x:.3f}, db = {bb:.3f}")
        assert x <= 1.0 and bb <= 1.0, (name, k, shape, x, bb)
        assert torch.equal(first[k][0][:-GUARD], second[k][0][:-GUARD]) and torch.equal(first[k][1][:-GUARD], second[k][1][:-GUARD])
    return first


def test_fp32_list_of_six():
    """The six problems of SIX in one call, switch off: every dW and db within the bound of the un-rounded product
    (ragged last split, batched nets, the 256 x 32 and 64-wide tiles beside the 128-wide ones, the ineligible problem
    in the middle on its own), guard tails untouched, two runs bit-identical.
    Measured on an MI355X: worst dW err / bound 0.136, db 0.045."""
    _check_fp32_list(SIX, 101, "six")


def test_fp32_list_of_seven_overflows_the_table():
    """Seven eligible problems: six fill the grid's table, the seventh runs on its own and is as right as the rest.
    Measured on an MI355X: worst dW err / bound 0.117, db 0.067."""
    _check_fp32_list(SEVEN, 102, "seven")


def test_fp32_list_without_bias_sums():
    """dbias = NULL: the weight gradients are bit-identical to the run that also emitted the bias sums"""
    with_b, without = _launch(SIX, 101), _launch(SIX, 101, with_bias=False)
    for k, shape in enumerate(SIX):
        _sums(shape, without[k])
        assert torch.equal(with_b[k][0][:-GUARD], without[k][0][:-GUARD]), shape


@pytest.mark.parametrize("name,shapes,classes,seed", [("six", SIX, SIX_CLASSES, 101), ("five", FIVE, FIVE_CLASSES, 103)],
                         ids=["six", "five"])
def test_bf16_mode_lists(name, shapes, classes, seed):
    """The same six, and five problems of in = 128, under igi_gemm_set_bf16_inputs(1): in > 64 with a free entry in the
    128-wide group is in the bf16 class, in <= 64, the ineligible problem and the fifth 128-wide problem (the group holds
    DMA_GROUP_MAX = 4) are in the fp32 class -- exactly the tables above; db meets its un-rounded bound in both classes;
    two runs are bit-identical; the switch is off again afterwards.
    Measured on an MI355X: bf16 class dW err / bound <= 0.041 against the rounded product, >= 360 against the un-rounded
    one; db <= 0.050."""
    from isaacgyminsertion_amd import _lib
    ins = _inputs(tuple(shapes), seed)
    with _switch(0):
        off = _launch(shapes, seed)
    with _switch(1):
        on, again = _launch(shapes, seed), _launch(shapes, seed)
    assert _lib.lib().igi_gemm_set_bf16_inputs(0) == 0
    got = []
    for k, (shape, d) in enumerate(zip(shapes, ins)):
        r, x, xr, bb = _ratios(shape, on[k], d)
        same = torch.equal(on[k][0][:-GUARD], off[k][0][:-GUARD]) and torch.equal(on[k][1][:-GUARD], off[k][1][:-GUARD])
        print(f"[{name} bf16 mode] problem {k} {shape}: dW max err / bound = {r:.3f} against the rounded product, {xr:.1f} "
              f"against the un-rounded one; db = {bb:.3f}; bit-identical to mode off: {same}")
        got.append(FP32 if same else (BF16 if (r <= 1.0 and xr > 1.0) else None))
        assert bb <= 1.0, (name, k, shape, bb)
        if same:
            assert x <= 1.0, (name, k, shape, x)
        assert torch.equal(on[k][0][:-GUARD], again[k][0][:-GUARD]) and torch.equal(on[k][1][:-GUARD], again[k][1][:-GUARD])
    assert got == classes, (got, classes)


def test_refusals():
    """count 0, count 9, a null list and a null operand are IGI_E_BADARG (nothing is launched)"""
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    t = torch.zeros(1024, device="cuda")
    ok = _lib.WgradProblem(dz=t.data_ptr(), x=t.data_ptr(), dweight=t.data_ptr(), dbias=None, dz_batch_stride=0,
                           x_batch_stride=0, lddz=4, ldx=4, out_features=4, in_features=4, rows=32, nbatch=1, splitk=1)
    arr = (_lib.WgradProblem * 9)(*([ok] * 9))
    s = _lib.current_stream()
    assert L.igi_gemm_wgrad_group(arr, 0, s) == -1
    assert L.igi_gemm_wgrad_group(arr, 9, s) == -1
    assert L.igi_gemm_wgrad_group(None, 1, s) == -1
    for field in ("dz", "x", "dweight"):
        one = (_lib.WgradProblem * 1)(ok)
        setattr(one[0], field, None)
        assert L.igi_gemm_wgrad_group(one, 1, s) == -1, field
    torch.cuda.synchronize()
    assert not bool(t.any())
