"""The opt-in split-bf16 mode of the tactile CNN's convolutions, host side (no GPU): the exact three-plane split and the
six-product restatement the GPU tests measure against (tests/conv_x3_ref.py), the switch of the C ABI
(igi_conv_set_bf16x3: exported, declared and bound; off by default; returns the previous setting; IGI_CONV_BF16X3=1
starts it on; a switch of its own), its Python surface (ops.conv_bf16x3, the config key, Runner), and the register /
scratch budget of every split-bf16 im2col instantiation the encoder's launch paths build -- with the register counts of
the fp32 and bf16-input instantiations held to what they were before the mode existed."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_x3_ref as ref  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------
# the split
# ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32)


def _values():
    g = torch.Generator().manual_seed(11)
    n = 1 << 16
    mant = 1.0 + torch.rand(n, generator=g)                                   # 24 random significant bits
    expo = torch.randint(-60, 61, (n,), generator=g).float()
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    rnd = (sign * mant * torch.exp2(expo)).float()
    pow2 = torch.exp2(torch.arange(-60, 61).float())
    # bf16 rounding ties: 8 significant bits + exactly half a bf16 ulp (even and odd kept bit), with and without a
    # sticky bit behind the half; and the same one level down (a tie in the mid plane)
    m8 = torch.arange(128, 256).float()                                       # 1.xxxxxxx in units of 2^-7
    ties = torch.cat([(m8 + 0.5) / 128, (m8 + 0.5 + 2.0 ** -16) / 128, (m8 + 0.5 - 2.0 ** -16) / 128,
                      (m8 + 2.0 ** -9 + 2.0 ** -17) / 128, (m8 + 0.25 + 2.0 ** -9) / 128])
    ties = torch.cat([ties * s for s in (1.0, 2.0 ** -37, 2.0 ** 41)])
    return torch.cat([rnd, pow2, -pow2, ties, -ties]).float()


def test_split_is_exact_and_each_plane_is_the_stated_conversion():
    x = _values()
    assert float(x.abs().min()) >= 2.0 ** -60 and float(x.abs().max()) < 2.0 ** 61
    hi, mid, lo = ref.split3(x)
    assert torch.equal(_bits((hi + mid) + lo), _bits(x))                      # bit for bit
    assert torch.equal(_bits(hi + (mid + lo)), _bits(x))
    # the planes are what the contract states: three nearest-even conversions, two exact differences
    assert torch.equal(hi, x.bfloat16().float())
    assert torch.equal(mid, (x - hi).bfloat16().float())
    assert torch.equal(lo, (x - hi - mid).bfloat16().float())
    assert torch.equal((x.double() - hi.double()).float().double(), x.double() - hi.double())          # exact in fp32
    assert torch.equal(((x - hi).double() - mid.double()).float().double(), (x - hi).double() - mid.double())
    for p in (hi, mid, lo):
        assert torch.equal(p, p.bfloat16().float())                           # each plane IS a bf16 value
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert bool((lo != 0).any()) and bool((mid != 0).any())


def test_split_of_zero():
    """+0 splits to three +0 planes, bit for bit.  -0: hi keeps the sign, mid = lo = +0 (x - hi = +0 under nearest even),
    so the planes sum to +0 -- equal to -0 in value, not in bits; no product term can tell the two apart."""
    z = torch.tensor([0.0, -0.0])
    hi, mid, lo = ref.split3(z)
    assert torch.equal(_bits(hi), _bits(z))
    assert _bits(mid).tolist() == [0, 0] and _bits(lo).tolist() == [0, 0]
    s = (hi + mid) + lo
    assert int(_bits(s)[0]) == 0 and float(s[1]) == 0.0
    assert torch.equal(s, z)


def test_underflow_boundary_from_both_sides():
    """Documented range: exact for |x| >= 2^-110 under gradual underflow (ulp(x) = 2^-133 is the smallest bf16
    subnormal); one binade below, an x whose last bit is set loses it.  From 2^-103 up no subnormal arises at all."""
    g = torch.Generator().manual_seed(12)
    mant = 1.0 + torch.rand(4096, generator=g)
    mant[0], mant[1] = 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23
    for e in (-110, -109, -104, -103):
        x = (mant.double() * 2.0 ** e).float()
        assert float(x.abs().min()) >= ref.LO_EXACT_MIN
        hi, mid, lo = ref.split3(torch.cat([x, -x]))
        assert torch.equal(_bits((hi + mid) + lo), _bits(torch.cat([x, -x]))), e
    x = (mant.double() * 2.0 ** -103).float()
    for p in ref.split3(x):
        nz = p[p != 0].abs()
        assert float(nz.min()) >= 2.0 ** -126                                  # every non-zero plane is a normal number
    below = torch.tensor([(1.0 + 2.0 ** -23) * 2.0 ** -111], dtype=torch.float64).float()
    assert float(below) < ref.LO_EXACT_MIN
    hi, mid, lo = ref.split3(below)
    assert not torch.equal((hi + mid) + lo, below)                            # 2^-134 is no bf16 number: lo rounded
    assert float(((hi + mid) + lo - below).abs()) == 2.0 ** -134


# ---------------------------------------------------------------------------------------------------------------
# the restatement against fp64
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [192, 512, 576])
def test_restatement_holds_the_gemm_bound_and_the_rounded_product_does_not(K):
    """ReLU-like activations against N(0, 0.05^2) weights: the six-product restatement stays within the project's GEMM
    bound 2e-6 * (|a| (*) |W|) + 1e-6 of fp64, the bf16-rounded product of the same inputs is far outside it, and the
    three dropped products (mid*lo, lo*mid, lo*lo) move the result by less than a tenth of the bound."""
    g = torch.Generator().manual_seed(K)
    a = torch.relu(torch.randn(256, K, generator=g))
    w = torch.randn(64, K, generator=g) * 0.05
    exact = a.double() @ w.double().t()
    bound = 2e-6 * (a.abs().double() @ w.abs().double().t()) + 1e-6
    six, nine = ref.contract(a, w, 6), ref.contract(a, w, 9)
    r6 = float(((six.double() - exact).abs() / bound).max())
    r9 = float(((nine.double() - exact).abs() / bound).max())
    rb = float(((ref.bf16r(a).double() @ ref.bf16r(w).double().t() - exact).abs() / bound).max())
    print(f"K = {K}: six {r6:.3f}, nine {r9:.3f}, bf16-rounded {rb:.1f} (max err / bound)")
    assert r6 <= 1.0 and r9 <= 1.0
    assert rb > 1.0
    assert float(((six.double() - nine.double()).abs() / bound).max()) <= 0.1


# ---------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------
def test_switch_is_exported_declared_and_bound():
    from isaacgyminsertion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "igi_ppo.h")).read()
    assert re.search(r"\bint igi_conv_set_bf16x3\(int on\);", hdr)
    assert "igi_conv_set_bf16x3" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "igi_conv_set_bf16x3")
    assert "IGI_CONV_BF16X3" in hdr


def _child(code, **env):
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("IGI_CONV_BF16", "IGI_CONV_BF16X3", "IGI_GEMM_BF16", "IGI_GEMM_X3"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1]


# x3: set 1, set 0, set 5, query, set 0 -> the previous values; then the one-plane switch and the plain products' experiment
_PROBE = ("from isaacgyminsertion_amd import _lib\n"
          "L = _lib.lib()\n"
          "a = L.igi_conv_set_bf16x3(1); b = L.igi_conv_set_bf16x3(0); c = L.igi_conv_set_bf16x3(5)\n"
          "q = L.igi_conv_set_bf16x3(-1); d = L.igi_conv_set_bf16x3(0)\n"
          "print(a, b, c, q, d, L.igi_conv_set_bf16_inputs(-1), L.igi_gemm_set_bf16x3(0))\n")


def test_off_by_default_and_setter_returns_previous():
    assert _child(_PROBE) == "0 1 0 1 1 0 0"


def test_environment_variable_starts_it_on_and_only_it():
    assert _child(_PROBE, IGI_CONV_BF16X3="1") == "1 1 0 1 1 0 0"
    assert _child(_PROBE, IGI_CONV_BF16X3="0") == "0 1 0 1 1 0 0"
    assert _child(_PROBE, IGI_CONV_BF16="1") == "0 1 0 1 1 1 0"       # the one-plane switch does not start this one
    assert _child(_PROBE, IGI_GEMM_X3="6") == "0 1 0 1 1 0 6"         # nor does the plain products' experiment
    probe = ("from isaacgyminsertion_amd import _lib\nL = _lib.lib()\n"
             "print(L.igi_conv_set_bf16_inputs(-1), L.igi_conv_set_bf16x3(-1), L.igi_gemm_set_bf16_inputs(0))\n")
    assert _child(probe, IGI_CONV_BF16X3="1") == "0 1 0"              # ... and this one starts no other
    probe = ("from isaacgyminsertion_amd import _lib\nL = _lib.lib()\n"
             "L.igi_conv_set_bf16x3(1); print(L.igi_conv_set_bf16_inputs(-1), L.igi_gemm_set_bf16x3(0))\n"
             "L.igi_conv_set_bf16_inputs(1); L.igi_gemm_set_bf16x3(6); print(L.igi_conv_set_bf16x3(0))\n")
    assert _child(probe) == "1"                                       # setters do not reach each other either


def test_python_setter_and_context_manager_restore():
    from isaacgyminsertion_amd import _lib, ops
    L = _lib.lib()
    start = L.igi_conv_set_bf16x3(0)
    try:
        assert ops.conv_bf16x3_enabled() is False
        s = ops.conv_bf16x3(True)                       # plain setter
        assert s.previous is False and ops.conv_bf16x3_enabled() is True
        assert ops.conv_bf16_inputs_enabled() is bool(L.igi_conv_set_bf16_inputs(-1))
        with ops.conv_bf16x3(False) as c:               # context manager: off inside, restored behind
            assert c.previous is True and ops.conv_bf16x3_enabled() is False
        assert ops.conv_bf16x3_enabled() is True
        with pytest.raises(ValueError):
            with ops.conv_bf16x3(False):
                raise ValueError("restored on the way out of an exception too")
        assert ops.conv_bf16x3_enabled() is True
    finally:
        L.igi_conv_set_bf16x3(start)


def test_config_key_and_runner_reads_it():
    """default_config carries offline_train.model.conv_bf16x3 = False; a Runner applies the key around its model's
    forward and restores the process switch; without the key it leaves the switch alone; the one-plane switch is not
    touched by this key."""
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu")
    assert cfg.offline_train.model.conv_bf16x3 is False
    L = _lib.lib()
    start, start1 = L.igi_conv_set_bf16x3(0), L.igi_conv_set_bf16_inputs(0)
    try:
        seen = {}
        for key in (True, False, None):
            r = Runner.__new__(Runner)                  # the mode handling alone: no model is built on the CPU
            r.conv_bf16_inputs = None
            r.conv_bf16x3 = key
            for outer in (False, True):
                L.igi_conv_set_bf16x3(int(outer))
                with r._conv_mode():
                    seen[(key, outer)] = ops.conv_bf16x3_enabled()
                    assert ops.conv_bf16_inputs_enabled() is False
                assert ops.conv_bf16x3_enabled() is outer
        assert seen == {(True, False): True, (True, True): True, (False, False): False, (False, True): False,
                        (None, False): False, (None, True): True}
        src = open(os.path.join(ROOT, "isaacgyminsertion_amd", "algo", "models", "transformer", "runner.py")).read()
        assert re.search(r"model\.get\('conv_bf16x3', False\)", src)
    finally:
        L.igi_conv_set_bf16x3(start)
        L.igi_conv_set_bf16_inputs(start1)


def test_runner_refuses_both_keys():
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu")
    cfg.offline_train.model.conv_bf16_inputs = True
    cfg.offline_train.model.conv_bf16x3 = True
    with pytest.raises(ValueError, match="conv_bf16x3"):
        Runner(cfg)


# ---------------------------------------------------------------------------------------------------------------
# registers
# ---------------------------------------------------------------------------------------------------------------
# VGPRs + AGPRs of every fp32 and bf16-input instantiation tactile.h reaches, from a compile of the commit before this mode
# (same flags as below)
PARENT_REGS = {
    "gemm_dma_conv_bf16_kernel<32,false,false,3,2,256>": 66, "gemm_dma_conv_bf16_kernel<32,false,false,5,2,256>": 66,
    "gemm_dma_conv_bf16_kernel<32,true,true,1,2,256>": 84, "gemm_dma_conv_bf16_kernel<32,true,true,4,2,256>": 66,
    "gemm_dma_conv_bf16_kernel<64,false,false,3,2,256>": 123,
    "gemm_dma_conv_bf16_kernel<64,false,false,3,3,128>": 103,
    "gemm_dma_conv_bf16_kernel<64,false,false,5,2,192>": 100,
    "gemm_dma_conv_bf16_kernel<64,false,false,5,2,256>": 110,
    "gemm_dma_conv_bf16_kernel<64,false,false,5,3,128>": 95, "gemm_dma_conv_bf16_kernel<64,true,true,1,2,256>": 112,
    "gemm_dma_conv_bf16_kernel<64,true,true,1,3,128>": 78, "gemm_dma_conv_bf16_kernel<64,true,true,4,2,256>": 92,
    "gemm_dma_conv_bf16_kernel<64,true,true,6,2,256>": 113, "gemm_dma_kernel<128,false,false,0,2,128>": 92,
    "gemm_dma_kernel<128,false,false,2,2,128>": 92, "gemm_dma_kernel<128,false,false,3,2,128>": 92,
    "gemm_dma_kernel<128,false,true,0,2,128>": 92, "gemm_dma_kernel<128,true,false,0,2,128>": 92,
    "gemm_dma_kernel<128,true,false,1,2,128>": 92, "gemm_dma_kernel<128,true,true,0,2,128>": 92,
    "gemm_dma_kernel<128,true,true,1,2,128>": 92, "gemm_dma_kernel<32,false,false,3,2,256>": 75,
    "gemm_dma_kernel<32,false,false,5,2,256>": 66, "gemm_dma_kernel<32,true,false,1,2,256>": 85,
    "gemm_dma_kernel<32,true,true,1,2,256>": 86, "gemm_dma_kernel<32,true,true,4,2,256>": 66,
    "gemm_dma_kernel<64,false,false,0,3,128>": 94, "gemm_dma_kernel<64,false,false,2,3,128>": 96,
    "gemm_dma_kernel<64,false,false,3,2,256>": 94, "gemm_dma_kernel<64,false,false,3,3,128>": 96,
    "gemm_dma_kernel<64,false,false,5,2,192>": 95, "gemm_dma_kernel<64,false,false,5,2,256>": 92,
    "gemm_dma_kernel<64,false,false,5,3,128>": 94, "gemm_dma_kernel<64,false,true,0,3,128>": 66,
    "gemm_dma_kernel<64,true,false,0,3,128>": 66, "gemm_dma_kernel<64,true,false,1,2,256>": 114,
    "gemm_dma_kernel<64,true,false,1,3,128>": 80, "gemm_dma_kernel<64,true,true,0,3,128>": 66,
    "gemm_dma_kernel<64,true,true,1,2,256>": 104, "gemm_dma_kernel<64,true,true,1,3,128>": 72,
    "gemm_dma_kernel<64,true,true,4,2,256>": 92, "gemm_dma_kernel<64,true,true,6,2,256>": 106,
}


def test_x3_conv_instantiations_do_not_spill_and_the_others_keep_their_registers():
    """Cross-compile of the tactile encoder's launch paths (tactile.h -> gemm()): every split-bf16 im2col instantiation --
    gemm_dma_conv_x3_kernel<BN, A_KC, B_KC, GATHER, NS, BM> -- uses no scratch and fits two 512-thread workgroups per CU
    (128 registers).  All the tiles the encoder can take must be there.  The fp32 (gemm_dma_kernel) and bf16-input
    (gemm_dma_conv_bf16_kernel) instantiations of the same translation unit use the registers they used before."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    filt = shutil.which("c++filt")
    if filt is None:
        pytest.skip("no c++filt")
    src = ('#include "tactile.h"\n'
           'int run(const igi_tactile_cfg* c, const float* x, const float* p, float* y, float* g, void* ws, size_t n, hipStream_t s) {\n'
           '  return igi::tactile_forward(c, x, p, y, ws, n, s) + igi::tactile_backward(c, y, p, g, ws, n, s); }\n')
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "tac.hip")
        with open(f, "w") as fh:
            fh.write(src)
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-c",
                            "-I", os.path.join(ROOT, "isaacgyminsertion_amd", "csrc"),
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "x.o"), f],
                           capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    names = [b.split()[0] for b in blocks]
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    found, others = set(), {}
    for b, name in zip(blocks, dem):
        m = re.search(r"(gemm_dma_conv_x3_kernel|gemm_dma_conv_bf16_kernel|gemm_dma_kernel)<([^>]*)>", name)
        if not m:
            continue
        key = m.group(2).replace(" ", "")
        vgpr = int(re.search(r"VGPRs: (\d+)", b).group(1))
        a = re.search(r"AGPRs: (\d+)", b)
        regs = vgpr + (int(a.group(1)) if a else 0)
        if m.group(1) != "gemm_dma_conv_x3_kernel":
            others[f"{m.group(1)}<{key}>"] = regs
            continue
        found.add(key)
        print(f"gemm_dma_conv_x3_kernel<{key}>: {regs} registers")
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, key
        assert regs <= 128, (key, regs)
    want = {"64,true,true,1,2,256", "32,true,true,1,2,256", "64,true,true,6,2,256",
            "64,true,true,4,2,256", "32,true,true,4,2,256",
            "32,false,false,5,2,256", "64,false,false,5,2,256", "64,false,false,5,2,192",
            "32,false,false,3,2,256", "64,false,false,3,2,256",
            "64,true,true,1,3,128", "64,false,false,5,3,128", "64,false,false,3,3,128"}
    assert want <= found, want - found
    assert PARENT_REGS and others == PARENT_REGS, {k: (PARENT_REGS.get(k), others.get(k))
                                                   for k in set(others) | set(PARENT_REGS)
                                                   if PARENT_REGS.get(k) != others.get(k)}
