"""CPU-side parts of the bf16-input mode's tests: the test entry igi_gemm_wgrad_group refuses bad lists before it touches a
device, its ctypes structure is the header's, and the emulation Function the teacher test of the mode measures against
(tests/bf16_emulation.py) is autograd's Linear when nothing is rounded.  (That the header compiles as C99 and that every
declared symbol is exported: tests/test_host_api.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from tests.bf16_emulation import RoundedLinear, bf16r, oracle_first_step_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wgrad_group_entry_refuses_bad_lists():
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    ok = _lib.WgradProblem(dz=C.addressof(buf), x=C.addressof(buf), dweight=C.addressof(buf), dbias=None, dz_batch_stride=0,
                           x_batch_stride=0, lddz=4, ldx=4, out_features=4, in_features=4, rows=4, nbatch=1, splitk=1)
    arr = (_lib.WgradProblem * 9)(*([ok] * 9))
    assert L.igi_gemm_wgrad_group(arr, 0, None) == -1                     # IGI_E_BADARG
    assert L.igi_gemm_wgrad_group(arr, 9, None) == -1
    assert L.igi_gemm_wgrad_group(arr, -1, None) == -1
    assert L.igi_gemm_wgrad_group(None, 1, None) == -1
    assert b"igi_gemm_wgrad_group" in L.igi_last_error()
    for field, bad in (("dz", None), ("x", None), ("dweight", None), ("rows", 0), ("out_features", 0), ("in_features", -3),
                       ("nbatch", 0), ("splitk", 0), ("lddz", 3), ("ldx", 3)):
        one = (_lib.WgradProblem * 2)(ok, ok)
        setattr(one[1], field, bad)
        assert L.igi_gemm_wgrad_group(one, 2, None) == -1, field


def test_wgrad_problem_struct_is_the_headers(tmp_path):
    from isaacgyminsertion_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in _lib.WgradProblem._fields_]
    src = tmp_path / "layout.c"
    hdr = os.path.join(ROOT, "include", "igi_ppo.h")
    lines = ['  printf("%d", (int)sizeof(igi_wgrad_problem));'] + \
            [f'  printf(" %d", (int)offsetof(igi_wgrad_problem, {f}));' for f in fields]
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{hdr}"\nint main(void) {{\n' + "\n".join(lines) +
                   "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_lib.WgradProblem)] + [getattr(_lib.WgradProblem, f).offset for f in fields]
    assert got == want


@pytest.mark.parametrize("bias", [True, False])
def test_emulation_function_is_autograd_when_nothing_is_rounded(bias):
    """RoundedLinear with the identity for ``rnd`` against torch.nn.functional.linear's own autograd in fp64 (2-D and 3-D
    inputs): 1e-12 relative.  With bf16r the forward is the product of the rounded operands, the data and weight
    gradients are those of the rounded operands with the rounded dy, and the bias gradient is the un-rounded sum."""
    g = torch.Generator().manual_seed(0)
    for shape in ((37, 23), (5, 7, 23)):
        x = torch.randn(*shape, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(11, 23, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(11, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
        dy = torch.randn(*shape[:-1], 11, generator=g, dtype=torch.float64)
        ins = [t for t in (x, w, b) if t is not None]
        y0 = torch.nn.functional.linear(x, w, b)
        g0 = torch.autograd.grad(y0, ins, dy)
        y1 = RoundedLinear.apply(x, w, b, lambda t: t)
        g1 = torch.autograd.grad(y1, ins, dy)
        for a, r in zip((y1,) + g1, (y0,) + g0):
            assert a.shape == r.shape and float((a - r).detach().abs().max()) <= 1e-12 * float(r.detach().abs().max())
        if len(shape) != 2:
            continue
        y2 = RoundedLinear.apply(x, w, b, bf16r)
        g2 = torch.autograd.grad(y2, ins, dy)
        xr, wr, dyr = bf16r(x.detach()), bf16r(w.detach()), bf16r(dy)
        assert not torch.equal(xr, x.detach()) and torch.equal(xr, xr.float().double())
        assert torch.equal(y2, xr @ wr.t() + b if bias else xr @ wr.t())
        assert torch.equal(g2[0], dyr @ wr) and torch.equal(g2[1], dyr.t() @ xr)
        if bias:
            assert torch.equal(g2[2], dy.sum(0))


def test_patched_oracle_step_runs_in_fp64_and_restores_linear():
    """The teacher oracle under patched_linear: un-rounded it is the fp32 oracle's first-step gradient to fp32 accuracy
    (1e-5 of the largest entry), rounded it is a different gradient within a percent or so; F.linear is put back."""
    from oracle import synth, teacher as ot
    N, T, E = 64, 8, 2
    units, priv_units = [64, 48, 32], [48, 32, 8]
    init, ro, perm = synth.teacher_problem(N, T, units, priv_units, seed=9, done_p=0.1)
    orig = torch.nn.functional.linear

    def grad(rnd, patched=True):
        orc = ot.TeacherOracle(init, perm, N, T, E, units, priv_units)
        orc.prepare(ro)
        if not patched:
            return orc.update(record_grads=1, max_steps=1)["grads"][0].double()
        return torch.cat([v.reshape(-1) for v in oracle_first_step_grad(orc, rnd).values()])

    g32, g64, gemu = grad(None, patched=False), grad(None), grad(bf16r)
    assert torch.nn.functional.linear is orig
    scale = float(g64.abs().max())
    assert float((g32 - g64).abs().max()) <= 1e-5 * scale
    d = float((gemu - g64).abs().max())
    assert 1e-5 * scale < d < 5e-2 * scale, (d, scale)
