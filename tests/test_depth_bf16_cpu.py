"""The opt-in bf16-input mode of the depth backbone, host side (no GPU): the switch of the C ABI
(igi_depth_set_bf16_inputs: exported, declared and bound; off by default; returns the previous setting; a negative argument
only reads; IGI_DEPTH_BF16=1 starts it on), igi_depth_activation_layout against the workspace size, the Python surface
(ops.depth_bf16_inputs, the Runner's config key), the register / scratch budget of the bf16 instantiations depth.h's
launch paths build, and the CPU restatement the GPU tests measure against (tests/depth_bf16_ref.py) held to the oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import depth_bf16_ref as ref  # noqa: E402
from make_golden_depth import depth_case  # noqa: E402  (seeded inputs only; the reference is not imported)


def test_symbols_are_declared_exported_and_bound():
    from isaacgyminsertion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "igi_ppo.h")).read()
    assert re.search(r"\bint igi_depth_set_bf16_inputs\(int on\);", hdr)
    assert re.search(r"\bint igi_depth_activation_layout\(const igi_depth_cfg\* cfg, int64_t offsets\[3\], int64_t rows\[3\]\);", hdr)
    assert "IGI_DEPTH_BF16" in hdr
    L = _lib.lib()
    for name in ("igi_depth_set_bf16_inputs", "igi_depth_activation_layout"):
        assert name in _lib.exported_symbols() and hasattr(L, name), name


def _child(code, **env):
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("IGI_DEPTH_BF16", "IGI_CONV_BF16", "IGI_GEMM_BF16"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1]


_PROBE = ("from isaacgyminsertion_amd import _lib\n"
          "L = _lib.lib()\n"
          "a = L.igi_depth_set_bf16_inputs(1); b = L.igi_depth_set_bf16_inputs(0); c = L.igi_depth_set_bf16_inputs(5)\n"
          "q = L.igi_depth_set_bf16_inputs(-1); d = L.igi_depth_set_bf16_inputs(0)\n"
          "print(a, b, c, q, d, L.igi_conv_set_bf16_inputs(-1), L.igi_gemm_set_bf16_inputs(0))\n")


def test_off_by_default_setter_returns_previous_and_environment_starts_it_on():
    # every call returns what was in force before it; a negative argument only queries; the two other switches are
    # different ones: they stay off throughout, and their environment variables do not start this one
    assert _child(_PROBE) == "0 1 0 1 1 0 0"
    assert _child(_PROBE, IGI_DEPTH_BF16="1") == "1 1 0 1 1 0 0"
    assert _child(_PROBE, IGI_DEPTH_BF16="0") == "0 1 0 1 1 0 0"
    assert _child(_PROBE, IGI_CONV_BF16="1") == "0 1 0 1 1 1 0"
    assert _child(_PROBE, IGI_GEMM_BF16="1") == "0 1 0 1 1 0 1"


def test_python_setter_and_context_manager_restore():
    from isaacgyminsertion_amd import _lib, ops
    L = _lib.lib()
    start = L.igi_depth_set_bf16_inputs(0)
    try:
        assert ops.depth_bf16_inputs_enabled() is False
        s = ops.depth_bf16_inputs(True)                  # plain setter
        assert s.previous is False and ops.depth_bf16_inputs_enabled() is True
        with ops.depth_bf16_inputs(False) as c:          # context manager: off inside, restored behind
            assert c.previous is True and ops.depth_bf16_inputs_enabled() is False
        assert ops.depth_bf16_inputs_enabled() is True
        with pytest.raises(ValueError):
            with ops.depth_bf16_inputs(False):
                raise ValueError("restored on the way out of an exception too")
        assert ops.depth_bf16_inputs_enabled() is True
        assert ops.conv_bf16_inputs_enabled() is False   # the tactile switch never moved
    finally:
        L.igi_depth_set_bf16_inputs(start)


def test_runner_reads_the_config_key():
    """offline_train.model.depth_bf16_inputs: True / False are applied around the model's forward and the process switch is
    restored; absent (default_config does not carry the key: absent = off) leaves the switch alone.  The tactile key is
    another switch: neither key moves the other's."""
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu")
    assert "depth_bf16_inputs" not in cfg.offline_train.model
    L = _lib.lib()
    start, cstart = L.igi_depth_set_bf16_inputs(0), L.igi_conv_set_bf16_inputs(0)
    try:
        seen = {}
        for key in (True, False, None):
            r = Runner.__new__(Runner)                   # the mode handling alone: no model is built on the CPU
            r.conv_bf16_inputs, r.depth_bf16_inputs = None, key
            for outer in (False, True):
                L.igi_depth_set_bf16_inputs(int(outer))
                with r._conv_mode():
                    seen[(key, outer)] = ops.depth_bf16_inputs_enabled()
                    assert ops.conv_bf16_inputs_enabled() is False
                assert ops.depth_bf16_inputs_enabled() is outer
        assert seen == {(True, False): True, (True, True): True, (False, False): False, (False, True): False,
                        (None, False): False, (None, True): True}
        L.igi_depth_set_bf16_inputs(0)
        r = Runner.__new__(Runner)
        r.conv_bf16_inputs, r.depth_bf16_inputs = True, None     # the tactile key alone does not reach the depth switch
        with r._conv_mode():
            assert ops.conv_bf16_inputs_enabled() is True and ops.depth_bf16_inputs_enabled() is False
        assert ops.conv_bf16_inputs_enabled() is False
        src = open(os.path.join(ROOT, "isaacgyminsertion_amd", "algo", "models", "transformer", "runner.py")).read()
        assert re.search(r"model\.get\('depth_bf16_inputs', False\)", src)
    finally:
        L.igi_depth_set_bf16_inputs(start)
        L.igi_conv_set_bf16_inputs(cstart)


def test_activation_layout_is_consistent_with_the_workspace():
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()
    for B in (32, 64, 768):
        cfg = _lib.DepthCfg(B, 32)
        off, rows = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        assert L.igi_depth_activation_layout(C.byref(cfg), off, rows) == 0
        total = int(L.igi_depth_workspace_bytes(C.byref(cfg)))
        assert list(rows) == [B * 25 * 46, B * 23 * 44, B]
        size = [4 * 32 * rows[0] + 32 * rows[0], 4 * 64 * rows[1], 4 * 128 * rows[2]]   # a1 + its arg-max bytes, a2, h3
        spans = sorted((off[i], off[i] + size[i]) for i in range(3))
        assert spans[0][0] >= 0 and spans[-1][1] <= total, (spans, total)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(2)), spans       # disjoint
        assert all(o % 256 == 0 for o in off), list(off)
        # the same offsets whatever the latent width: the activations precede everything that depends on it
        off2, rows2 = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        assert L.igi_depth_activation_layout(C.byref(_lib.DepthCfg(B, 8)), off2, rows2) == 0
        assert list(off2) == list(off) and list(rows2) == list(rows)
    off, rows = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    for b, latent in [(33, 32), (32800, 32), (32, 6), (0, 32)]:      # what make_depth_plan refuses
        assert L.igi_depth_activation_layout(C.byref(_lib.DepthCfg(b, latent)), off, rows) != 0, (b, latent)
    assert L.igi_depth_activation_layout(C.byref(_lib.DepthCfg(32, 32)), None, rows) != 0
    assert L.igi_depth_activation_layout(None, off, rows) != 0


def test_restatement_without_rounding_is_the_oracle():
    """tests/depth_bf16_ref.py with the rounding replaced by the identity, in float64, on the case tests/golden/depth.npz
    pins (depth_case(): 32 images): forward and all eight gradients equal oracle/encoders.py:depth_backbone and its
    autograd gradient to 1e-12 of each tensor's largest entry, and the oracle's fp32 output is the fixture's.  With the
    rounding on, the same functions differ from it (the helper does round)."""
    from oracle import encoders as oe
    sd, x, dy = depth_case()
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "depth.npz"))
    with torch.no_grad():
        np.testing.assert_allclose(oe.depth_backbone(x, sd).numpy(), fixture["y"], atol=2e-5, rtol=1e-4)
    y64, g64 = oe.value_and_grads(oe.depth_backbone, x, sd, dy, dtype=torch.float64)
    sd64 = {k: v.double() for k, v in sd.items()}
    assert list(sd64) == ref.KEYS
    f = ref.forward(x.double(), sd64, rnd=ref.ident)
    assert float((f["y"] - y64).abs().max()) <= 1e-12 * float(y64.abs().max())
    g = ref.backward(x.double(), dy.double(), sd64, f["a1"], f["idx"], f["a2"], f["h3"], rnd=ref.ident, chunk=16)
    for k in ref.KEYS:
        err, scale = float((g[k] - g64[k]).abs().max()), float(g64[k].abs().max())
        assert err <= 1e-12 * scale, (k, err, scale)
    assert int(f["idx"].max()) <= 3 and int(f["idx"][:, :, :2, :5].max()) == 0    # flat corner: the first maximum wins
    fr = ref.forward(x.double(), sd64)
    assert torch.equal(fr["a1"], f["a1"]) and torch.equal(fr["idx"], f["idx"])   # conv1 is not rounded
    assert float((fr["a2"] - f["a2"]).abs().max()) > 1e-5 and float((fr["y"] - y64).abs().max()) > 1e-6
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3], dtype=torch.float64)   # ties go to the even mantissa
    assert ref.bf16r(t).tolist() == [1.0, 1.0 + 2.0 ** -6, float(torch.tensor(-0.3).bfloat16())]


def test_bf16_instantiations_of_the_depth_paths_do_not_spill():
    """Cross-compile of depth.h's launch paths (-> gemm()): every bf16-input instantiation they can reach -- the im2col
    twins gemm_dma_conv_bf16_kernel<BN, A_KC, B_KC, GATHER, NS, BM> of conv2's tiles at every batch regime and the three
    gemm_dma_bf16_kernel<A_KC, B_KC> of the big Linear (the <false, false> weight-gradient launch exists for this mode
    only) -- uses no scratch and fits two 512-thread workgroups per CU (128 registers), as its fp32 twin does."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    filt = shutil.which("c++filt")
    if not os.path.exists(hipcc) or filt is None:
        pytest.skip("hipcc / c++filt not available")
    src = ('#include "depth.h"\n'
           'int run(const igi_depth_cfg* c, const float* x, const float* p, float* y, float* g, void* ws, size_t n, hipStream_t s) {\n'
           '  return igi::depth_forward(c, x, p, y, ws, n, s) + igi::depth_backward(c, x, y, p, g, ws, n, s); }\n')
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "dep.hip")
        with open(f, "w") as fh:
            fh.write(src)
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-c",
                            "-I", os.path.join(ROOT, "isaacgyminsertion_amd", "csrc"),
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "x.o"), f],
                           capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    dem = subprocess.run([filt], input="\n".join(b.split()[0] for b in blocks), capture_output=True, text=True).stdout.split("\n")
    found = {}
    for b, name in zip(blocks, dem):
        m = re.search(r"(gemm_dma_conv_bf16_kernel|gemm_dma_bf16_kernel)<([^>]*)>", name)
        if not m:
            continue
        key = m.group(1) + "<" + m.group(2).replace(" ", "") + ">"
        a = re.search(r"AGPRs: (\d+)", b)
        regs = int(re.search(r"VGPRs: (\d+)", b).group(1)) + (int(a.group(1)) if a else 0)
        found[key] = (regs, int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)),
                      int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    print(found)
    want = {"gemm_dma_conv_bf16_kernel<64,true,true,1,3,128>",       # conv2 forward and data gradient, <= 64 (<= 96) images
            "gemm_dma_conv_bf16_kernel<64,true,true,1,2,256>",       # conv2 forward from 160 images
            "gemm_dma_conv_bf16_kernel<32,true,true,1,2,256>",       # data gradient from 128 images, row-major
            "gemm_dma_conv_bf16_kernel<32,true,true,4,2,256>",       # ... position-major at multiples of 256
            "gemm_dma_conv_bf16_kernel<64,false,false,5,3,128>",     # weight gradient: three 128-row tap tiles
            "gemm_dma_bf16_kernel<true,true>", "gemm_dma_bf16_kernel<true,false>", "gemm_dma_bf16_kernel<false,false>"}
    assert want <= set(found), want - set(found)
    for key, (regs, scratch, _lds) in found.items():
        assert scratch == 0 and regs <= 128, (key, regs, scratch)
