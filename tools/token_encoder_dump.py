#!/usr/bin/env python
"""Bit dump of the student's token encoder, to compare two builds of the library in separate, fresh processes:

    python tools/token_encoder_dump.py OUT.json [--root TREE]

Runs the forward and backward of a 2-layer stack (d 32, 2 heads, ff 128) from fixed seeded inputs and parameters over CASES
(the smallest batches that reach each kernel path and each partial-tile edge), in eval mode and in train mode (dropout 0.1,
a fixed seed), with IGI_TOKEN_FUSED / IGI_TOKEN_FUSED_BWD both at 1 (the one-launch kernels where the library dispatches to
them) and both at 0 (launch per operation), and writes the SHA-256 digests of y, dx and the parameter gradient per case,
mode and path.  Neither path has atomics and both sum in fixed orders, so two builds that compute the same thing give the
same digests: tests/test_gpu_token_encoder_bits.py holds this tree to tests/golden/token_encoder_bits.json.
--root: the tree whose package and library to load (default: this one)."""
import argparse
import hashlib
import json
import os
import sys

# (B, S): register attention + one-launch backward, one sample per workgroup | two samples per workgroup, partial tail |
# full 128-row forward / 64-row backward workgroups, partial tail | register attention, launch-per-operation backward |
# tile attention: one sample per workgroup, several, and a partial tail
CASES = [(5, 1), (7, 3), (3, 4), (601, 3), (8200, 4), (6, 5), (4, 8), (3, 9), (2, 32), (515, 32)]
MODES = {"eval": False, "train": True}
PATHS = {"fused": "1", "per_op": "0"}
NHEAD, FF, LAYERS, DROPOUT, SEED = 2, 128, 2, 0.1, 0x2B5C9D1E00F0A7C3
PER_LAYER = 4 * 32 * 32 + 3 * 32 + 32 + 2 * 32 * FF + FF + 32 + 4 * 32


def case_id(B, S):
    return f"{B}x{S}"


def inputs(B, S):
    """x, dy (B, S, 32) and the flat parameter vector, on the CPU: O(1) scale, LayerNorm weights around 1."""
    import torch
    g = torch.Generator().manual_seed(1000 * B + S)
    x = torch.randn(B, S, 32, generator=g)
    dy = torch.randn(B, S, 32, generator=g)
    params = torch.randn(LAYERS * PER_LAYER, generator=torch.Generator().manual_seed(77)) * 0.3
    for l in range(LAYERS):
        end = (l + 1) * PER_LAYER
        params[end - 128:end - 96] += 1.0     # norm1.weight
        params[end - 64:end - 32] += 1.0      # norm2.weight
    return x, dy, params


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(B, S):
    """{mode: {path: {"y" | "dx" | "grad": digest}}} of one case, through torch.ops.mi355ppo.token_encoder_fwd."""
    import torch
    import isaacgyminsertion_amd.ops  # noqa: F401  (registers torch.ops.mi355ppo)
    x, dy, params = inputs(B, S)
    out = {}
    saved = {k: os.environ.get(k) for k in ("IGI_TOKEN_FUSED", "IGI_TOKEN_FUSED_BWD")}
    try:
        for mode, training in MODES.items():
            out[mode] = {}
            for path, flag in PATHS.items():
                os.environ["IGI_TOKEN_FUSED"] = os.environ["IGI_TOKEN_FUSED_BWD"] = flag   # read by the library per call
                xm, fm = x.cuda().requires_grad_(True), params.cuda().requires_grad_(True)
                y, _ = torch.ops.mi355ppo.token_encoder_fwd(xm, fm, NHEAD, FF, LAYERS, DROPOUT, training, SEED)
                y.backward(dy.cuda())
                torch.cuda.synchronize()
                out[mode][path] = {"y": _sha(y), "dx": _sha(xm.grad), "grad": _sha(fm.grad)}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))    # the package and its library are --root's
    import isaacgyminsertion_amd
    from isaacgyminsertion_amd import _lib
    assert os.path.abspath(isaacgyminsertion_amd.__file__).startswith(os.path.abspath(args.root) + os.sep)
    rec = {"tool": "tools/token_encoder_dump.py",
           "config": f"{LAYERS} layers, d 32, {NHEAD} heads, ff {FF}; train: dropout {DROPOUT}, seed {SEED:#x}",
           "cases": {case_id(B, S): run_case(B, S) for B, S in CASES}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(CASES)} cases: {_lib.lib().igi_build_info().decode()} -> {args.out}")


if __name__ == "__main__":
    main()
