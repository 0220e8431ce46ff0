#!/usr/bin/env python
"""One forward + backward of the student's two-layer token encoder at sequence lengths beyond 8 tokens, beside ATen.

    python tools/bench_token_seq.py [--pairs R] [--iters K] [--control-only] [--shapes BxS,...] [--root TREE]
                                    [--out profiles/token_seq.json]

Shapes (B, S): (2048, 12), (2048, 32), (8192, 9) -- the tile attention kernels and k_token_fwd_long -- and (2048, 3), the
register-attention path, as a control that must not move against the parent commit; --shapes picks others (8192x2: the
one-launch kernels at full workgroups).  --root: the tree whose package and library to time (default: this one), to set
another commit's build beside this one in the same job.  Train mode, dropout 0.1, the weights
of tests/test_gpu_token_encoder.py.  ``HipTransformerEncoder`` and ATen's fp32 ``nn.TransformerEncoder`` (the only other
implementation of these shapes) run on the same device in R alternating pairs of K iterations each (forward, backward of
a fixed upstream gradient; device synchronise around every round; ms per iteration).  The two draw different dropout
masks (the mask stream is each library's own), which does not change the work.  Medians and spreads go to the record,
stamped with the library's build hash.  No bar: the figures are stated in README / DESIGN as they come out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(2048, 12), (2048, 32), (8192, 9), (2048, 3)]


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _layer(p):
    import torch
    import torch.nn as nn
    torch.manual_seed(0)
    layer = nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=128, activation="gelu", batch_first=True,
                                       norm_first=True, dropout=p)
    with torch.no_grad():
        for q in layer.parameters():
            q.copy_(torch.randn_like(q) * (0.3 if q.dim() > 1 else 0.2) + (1.0 if q.dim() == 1 and q.numel() == 32 else 0.0))
    return layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_seq.json"))
    ap.add_argument("--control-only", action="store_true", help="time the 2048 x 3 control alone (any commit's build takes it)")
    ap.add_argument("--shapes", default="", help="comma-separated BxS list instead of the default shapes")
    ap.add_argument("--root", default=ROOT, help="the tree whose package and library to load")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import torch.nn as nn
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_seq: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    p = 0.1
    layer = _layer(p)
    nets = {"hip": HipTransformerEncoder(layer, num_layers=2).cuda().train(),
            "aten": nn.TransformerEncoder(layer, num_layers=2, enable_nested_tensor=False).cuda().train()}
    rows = {}
    shapes = [tuple(int(v) for v in t.split("x")) for t in args.shapes.split(",") if t] or (SHAPES[-1:] if args.control_only else SHAPES)
    for B, S in shapes:
        g = torch.Generator().manual_seed(B + S)
        x = torch.randn(B, S, 32, generator=g).cuda().requires_grad_(True)
        dy = torch.randn(B, S, 32, generator=g).cuda()

        def step(net):
            x.grad = None
            for q in net.parameters():
                q.grad = None
            net(x).backward(dy)

        for net in nets.values():                  # warm-up: code loading, algorithm choice, clocks
            for _ in range(20):
                step(net)
        torch.cuda.synchronize()
        ms = {k: [] for k in nets}
        for _ in range(args.pairs):
            for name, net in nets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    step(net)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.iters)
        _lib.prof_enable(True)                     # which kernels the library ran (a separate, untimed iteration)
        try:
            step(nets["hip"])
            torch.cuda.synchronize()
            classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
        finally:
            _lib.prof_enable(False)
        med = {k: _median(v) for k, v in ms.items()}
        rows[f"{B}x{S}"] = {
            "fwd_bwd_ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "fwd_bwd_ms_median": {k: round(v, 4) for k, v in med.items()},
            "fwd_bwd_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "hip_over_aten": round(med["hip"] / med["aten"], 4),
            "library_launches": classes,
        }
        print(f"[token_seq] {B} x {S}: hip {med['hip']:.4f} ms, aten {med['aten']:.4f} ms per forward + backward", flush=True)
    rec = {
        "tool": "tools/bench_token_seq.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "config": f"2 x TransformerEncoderLayer(32, 2 heads, ff 128, gelu, norm_first), train mode, dropout {p}; forward + "
                  f"backward per iteration (host clock around {args.iters} iterations ending in a device synchronise: launch "
                  f"overheads of both implementations included); {args.pairs} alternating rounds",
        "control": "2048x3 runs the register attention kernels this change does not touch",
        "shapes": rows,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
