"""The seeded draws have one table (csrc/draws.h) and one host restatement in the product (isaacgyminsertion_amd/draws.py):
the restatement against the pinned hashes, against the tests' independent numpy one (oracle/token_dropout.py, which never
imports it) and, where the host has a ``g++``, against tools/draws_check.cpp -- the header itself, compiled for the host --
line for line; the table of the header, of the module and of the test references; the Gaussian.  No GPU."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle.token_dropout import tok_hash
from tests import img_augment_ref as A
from tests import img_online_ref, pcl_augment_ref, tactile_augment_ref, tactile_online_ref
from tests.test_oracle_token_dropout import PINNED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "isaacgyminsertion_amd")
SEEDS = [0, 3, 0x1234567890ABCDEF, 2 ** 63 - 2]


def _D():
    from isaacgyminsertion_amd import draws
    return draws


# ---- the hash --------------------------------------------------------------------------------------------------------------
def test_hash_reproduces_the_pinned_values():
    D = _D()
    for seed, site, idx, want in PINNED:
        assert int(D.tok_hash(seed, site, torch.tensor([idx]))[0]) == want, (seed, site, idx)
        assert int(D.tok_hash((seed & 0xFFFFFFFF, seed >> 32), site, torch.tensor([idx + 2 ** 32]))[0]) == want


@pytest.mark.parametrize("seed", SEEDS)
def test_hash_equals_the_oracle_on_random_elements(seed):
    D = _D()
    idx = torch.randint(0, 2 ** 33, (5000,), generator=torch.Generator().manual_seed(1))
    assert int(idx.max()) >= 2 ** 32                                   # the wrap is exercised
    for site in (0, 7, 14, 22, 30):
        got = D.tok_hash(seed, site, idx)
        assert got.dtype == torch.int64 and got.shape == idx.shape
        assert np.array_equal(got.numpy(), tok_hash(seed, site, idx.numpy()).astype(np.int64)), site


@pytest.mark.parametrize("seed_episode", SEEDS)
def test_hash_with_a_seed_per_element(seed_episode):
    """The point cloud's per-episode seed ``seed_episode + (episode << 32)``: the high word handed over as a tensor."""
    D = _D()
    g = torch.Generator().manual_seed(2)
    episode = torch.randint(0, 2 ** 31, (300,), generator=g)
    idx = torch.randint(0, 2 ** 33, (300,), generator=g)
    for site in (6, 15, 16):
        got = D.tok_hash((seed_episode, (seed_episode >> 32) + episode), site, idx)
        want = [int(tok_hash((seed_episode + (int(ep) << 32)) & (2 ** 64 - 1), site, [int(i)])[0]) for ep, i in zip(episode, idx)]
        assert got.tolist() == want
    grid = D.tok_hash((seed_episode, ((seed_episode >> 32) + episode)[:, None]), 6, idx[:4][None])      # broadcast
    assert grid.shape == (300, 4) and torch.equal(grid[:, 0], D.tok_hash((seed_episode, (seed_episode >> 32) + episode), 6,
                                                                         idx[:1].expand(300)))


# ---- the compiled header ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_lines(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path_factory.mktemp("draws") / "draws_check")
    subprocess.run([gxx, "-std=c++17", os.path.join(ROOT, "tools", "draws_check.cpp"), "-o", exe], check=True, cwd=ROOT,
                   timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def _bits(t):
    """float64 tensor, exactly representable in fp32 -> the fp32 bit patterns."""
    assert torch.equal(t.float().double(), t)
    return [f"{int(b) & 0xFFFFFFFF:08x}" for b in t.float().view(torch.int32)]


def test_check_program_agrees_line_for_line(check_lines):
    D = _D()
    kinds = {k: [ln[1:] for ln in check_lines if ln[0] == k] for k in ("hash", "threshold", "unit", "index", "plane", "site")}
    assert sum(len(v) for v in kinds.values()) == len(check_lines) and all(kinds.values())
    for seed, site, e, h in kinds["hash"]:
        assert int(D.tok_hash(int(seed), int(site), torch.tensor([int(e)]))[0]) == int(h), (seed, site, e)
    printed = {(int(s), int(k), int(e)): int(h) for s, k, e, h in kinds["hash"]}
    for seed, site, e, want in PINNED:                                 # the pinned list is this program's output
        assert printed[(seed, site, e)] == want
    thr = {float(p): int(t) for p, t in kinds["threshold"]}
    assert {0.0, 0.1, 0.3, 0.5, 1.0} <= set(thr) and thr[1.0] == 4294967296 and thr[0.0] == 0
    for p, t in thr.items():
        assert D.threshold(p) == t == A.threshold(p), p
    h = torch.tensor([int(ln[0]) for ln in kinds["unit"]])
    assert {0, 255, 256, 0xFFFFFFFF} <= set(h.tolist())
    assert _bits(D.u(h)) == [ln[1] for ln in kinds["unit"]] and _bits(D.unit(h)) == [ln[2] for ln in kinds["unit"]]
    for hh, n, i in kinds["index"]:
        assert int(D.index(torch.tensor([int(hh)]), int(n))[0]) == int(i) < int(n)
    assert [(n, int(v)) for n, v in kinds["plane"]] == list(D.PLANES.items())
    assert [(n, int(v)) for n, v in kinds["site"]] == list(D.SITES.items())


# ---- the table -------------------------------------------------------------------------------------------------------------
DEFINES = r"\b(\w*(?:_SITE_\w+|_PLANE_\w+|_NOISE_PLANE)) = (\d+)"


def test_table_of_the_header_the_module_and_the_references():
    D = _D()
    hdr = open(os.path.join(PKG, "csrc", "draws.h")).read()
    parsed = {n: int(v) for n, v in re.findall(DEFINES, hdr)}
    assert parsed == {**D.PLANES, **D.SITES} and len(parsed) == len(D.PLANES) + len(D.SITES)
    assert "static_assert(draw_numbers_fill(DRAW_SITES, 2 * sizeof(DRAW_PLANES) / sizeof(DrawName))" in hdr
    for n in parsed:                                                   # every constant has its row in the checked arrays
        assert f"IGI_DRAW_ROW({n})" in hdr, n
    # pairwise distinct; plane p occupies sites 2p and 2p + 1, the sites follow without a gap
    assert sorted(D.PLANES.values()) == list(range(len(D.PLANES)))
    assert sorted(D.SITES.values()) == list(range(2 * len(D.PLANES), 31))
    # the references' own statements of the numbers
    assert {k: D.SITES["IMG_SITE_" + k] for k in img_online_ref.SITES} == img_online_ref.SITES
    assert {k: D.SITES["TAC_SITE_" + k] for k in tactile_online_ref.SITES} == tactile_online_ref.SITES
    assert D.PLANES["TAC_NOISE_PLANE"] == tactile_augment_ref.NOISE_PLANE
    assert (D.PLANES["IMG_PLANE_DEPTH"], D.PLANES["IMG_PLANE_MASK"]) == (0, 1)      # img_augment_ref.augment: plane k of (img, seg)
    R = pcl_augment_ref
    assert {k: v for k, v in D.PLANES.items() if k.startswith("PCL_")} == \
        {"PCL_" + k: getattr(R, k) for k in dir(R) if k.startswith("PLANE_")}
    assert {k: v for k, v in D.SITES.items() if k.startswith("PCL_")} == \
        {"PCL_" + k: getattr(R, k) for k in dir(R) if k.startswith("SITE_")}
    n_ref = len(img_online_ref.SITES) + len(tactile_online_ref.SITES) + sum(k.startswith("SITE_") for k in dir(R))
    assert n_ref == len(D.SITES)


def test_nothing_else_defines_a_number_or_restates_the_hash():
    others = [p for p in glob.glob(os.path.join(PKG, "csrc", "*")) if os.path.basename(p) != "draws.h"]
    assert len(others) > 20
    for p in others:
        assert not re.findall(DEFINES, open(p, errors="replace").read()), p
    py = [p for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)] + glob.glob(os.path.join(ROOT, "*.py"))
    py = [p for p in py if os.path.abspath(p) != os.path.join(PKG, "draws.py")]
    assert len(py) > 20
    for p in py:
        assert "9e3779b1" not in open(p, errors="replace").read().lower(), p
    assert "0x9E3779B1" in open(os.path.join(PKG, "draws.py")).read()


# ---- the Gaussian ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [0, 2, 6])
def test_gauss_float64_within_4_ulp_of_the_reference(plane):
    D = _D()
    seed, n = 0x1234567890ABCDEF, 4096
    got = D.gauss(seed, plane, D.elements((n,)), torch.float64)
    want = A.gauss(seed, plane, (n,))
    assert got.dtype == torch.float64
    # in ulps of the reference's own value: both form the cosine's argument (2 pi) u2 with the same two roundings, so what
    # differs is the branch of ln u1 and the last place of log / sqrt / cos
    err = (got - want).abs() / torch.from_numpy(np.spacing(want.abs().numpy()))
    print(f"plane {plane}: largest difference {float(err.max()):.3f} ulp")
    assert float(err.max()) <= 4.0


def test_gauss_fp32_equals_the_parent_commit_bit_for_bit():
    """tests/golden/draws_gauss_f32.npz: ``utils._hash_gauss(seed, plane, (256,), torch.float32, "cpu")`` of the commit
    before the function moved here, for planes 0, 2 and 6 -- generated once there."""
    D = _D()
    G = np.load(os.path.join(ROOT, "tests", "golden", "draws_gauss_f32.npz"))
    seed, planes, z = int(G["seed"]), G["planes"].tolist(), G["z"]
    assert planes == [0, 2, 6] and z.shape == (3, 256) and z.dtype == np.float32
    for k, plane in enumerate(planes):
        got = D.gauss(seed, plane, D.elements((256,)), torch.float32)
        assert got.dtype == torch.float32
        assert np.array_equal(got.numpy().view(np.int32), z[k].view(np.int32)), plane
    grid = D.gauss(seed, 2, D.elements((4, 8, 8)), torch.float32)                  # an output tensor's shape
    assert grid.shape == (4, 8, 8) and np.array_equal(grid.reshape(-1).numpy(), z[1])


def test_keep_grid_is_the_comparison_cell_by_cell():
    D = _D()
    seed, site, p = 2 ** 63 - 2, D.SITES["IMG_SITE_KEEP"], 0.3
    keep = D.keep_grid(seed, site, p, (5, 3, 6))
    want = tok_hash(seed, site, np.arange(90)).astype(np.int64) >= A.threshold(p)
    assert keep.dtype == torch.uint8 and keep.shape == (5, 3, 6) and np.array_equal(keep.reshape(-1).numpy() != 0, want)
    assert bool(D.keep_grid(seed, site, 0.0, (90,)).all()) and not bool(D.keep_grid(seed, site, 1.0, (90,)).any())
