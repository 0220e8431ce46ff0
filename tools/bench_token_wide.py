#!/usr/bin/env python
"""One forward + backward of the student's two-layer token encoder at widths 64 and 128, beside ATen; and the stock
32-wide encoder beside another build of the library (the parent commit's) as a control.

    python tools/bench_token_wide.py [--pairs R] [--iters K] [--parent-root TREE] [--out profiles/token_wide.json]

Wide shapes (d, heads, B x S): (64, 4, 2048 x 3), (64, 4, 2048 x 12), (128, 2, 2048 x 3), (128, 8, 512 x 32): the
launch-per-operation path with the wide LayerNorm and the tile attention kernels.  ``HipTransformerEncoder`` and ATen's
fp32 ``nn.TransformerEncoder`` run on the same device in R alternating rounds of K iterations each (forward, backward of a
fixed upstream gradient; train mode, dropout 0.1; host clock around the K iterations ending in a device synchronise; ms
per iteration).  The two draw different dropout masks (the mask stream is each library's own), which does not change
the work.

Control shapes: (32, 2) at 2048 x 3 and 2048 x 12, this tree's build against the build of --parent-root (a checkout of
the parent commit with its library built): one worker process per build and round, one at a time and before this
process opens the device, the builds alternating within the job.  "Not slower" means inside the parent's own
round-to-round spread.  Without --parent-root the control is recorded as not measured.

Medians and min .. max go to the record, stamped with the library's build hash.  No bar: the figures are stated in
README / DESIGN as they come out.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE = [(64, 4, 2048, 3), (64, 4, 2048, 12), (128, 2, 2048, 3), (128, 8, 512, 32)]
CONTROL = [(32, 2, 2048, 3), (32, 2, 2048, 12)]
P_DROP = 0.1


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _layer(d, heads):
    """matrices randn * 0.3 * sqrt(32 / fan_in), vectors randn * 0.2 (+ 1 for the LayerNorm weights): O(1) activations"""
    import torch
    import torch.nn as nn
    layer = nn.TransformerEncoderLayer(d_model=d, nhead=heads, dim_feedforward=4 * d, activation="gelu", batch_first=True,
                                       norm_first=True, dropout=P_DROP)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, q in layer.named_parameters():
            v = torch.randn(q.shape, generator=g)
            q.copy_(v * 0.3 * math.sqrt(32.0 / q.shape[1]) if q.dim() > 1 else v * 0.2 + (1.0 if n.endswith("norm1.weight") or n.endswith("norm2.weight") else 0.0))
    return layer


class _Case:
    """The nets and tensors of one shape; ``round(name, iters)`` times ``iters`` forward + backward passes of one net."""

    def __init__(self, d, heads, B, S, with_aten):
        import torch
        import torch.nn as nn
        from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
        layer = _layer(d, heads)
        self.nets = {"hip": HipTransformerEncoder(layer, num_layers=2).cuda().train()}
        if with_aten:
            self.nets["aten"] = nn.TransformerEncoder(layer, num_layers=2, enable_nested_tensor=False).cuda().train()
        g = torch.Generator().manual_seed(B + S)
        self.x = torch.randn(B, S, d, generator=g).cuda().requires_grad_(True)
        self.dy = torch.randn(B, S, d, generator=g).cuda()
        for name in self.nets:                      # warm-up: code loading, algorithm choice, clocks
            for _ in range(20):
                self.step(name)
        torch.cuda.synchronize()

    def step(self, name):
        net = self.nets[name]
        self.x.grad = None
        for q in net.parameters():
            q.grad = None
        net(self.x).backward(self.dy)

    def round(self, name, iters):
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            self.step(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def launches(self):
        import torch
        from isaacgyminsertion_amd import _lib
        _lib.prof_enable(True)                      # which kernels the library ran (a separate, untimed iteration)
        try:
            self.step("hip")
            torch.cuda.synchronize()
            return {c["name"]: c["launches"] for c in _lib.prof_read()}
        finally:
            _lib.prof_enable(False)


def _summary(ms):
    return {"fwd_bwd_ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "fwd_bwd_ms_median": {k: round(_median(v), 4) for k, v in ms.items()},
            "fwd_bwd_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}


def worker(root, iters):
    """Control worker: loads the package and library of ``root``, times one round of every control shape (after the case's
    own warm-up and one short round) and prints {"build": hash, "ms": {shape: ms per iteration}}."""
    sys.path.insert(0, os.path.abspath(root))
    import torch
    torch.cuda.init()                               # torch's HIP runtime first, as in every other entry point: the library shares it
    from isaacgyminsertion_amd import _lib
    ms = {}
    for d, heads, B, S in CONTROL:
        case = _Case(d, heads, B, S, with_aten=False)
        case.round("hip", 20)
        ms[f"d{d}_h{heads}_{B}x{S}"] = case.round("hip", iters)
    print(json.dumps({"build": _lib.lib().igi_build_info().decode(), "ms": ms}), flush=True)


def control(parent_root, pairs, iters):
    """One worker process per (build, round), one at a time, the builds alternating: no other process has the device open
    while a round is timed.  (Two workers kept up side by side, one of them idle, took turns at a fast and a slow mode --
    0.29 and 0.56 ms at 2048 x 3 -- whichever build they had loaded.)"""
    roots = {"this": ROOT, "parent": parent_root}
    builds, ms = {}, {}
    for _ in range(pairs):
        for name, root in roots.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, "--iters", str(iters)],
                               capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(f"bench_token_wide: the control worker of {root} failed:\n{r.stderr[-2000:]}")
            ans = json.loads(r.stdout.strip().splitlines()[-1])
            builds[name] = ans["build"]
            for shape, t in ans["ms"].items():
                ms.setdefault(shape, {k: [] for k in roots})[name].append(t)
    rows = {"builds": builds}
    for shape, v in ms.items():
        row = _summary(v)
        lo, hi = row["fwd_bwd_ms_min_max"]["parent"]
        row["this_over_parent"] = round(row["fwd_bwd_ms_median"]["this"] / row["fwd_bwd_ms_median"]["parent"], 4)
        row["this_median_inside_parent_min_max"] = bool(row["fwd_bwd_ms_median"]["this"] <= hi)
        rows[shape] = row
        print(f"[token_wide] control {shape}: this {row['fwd_bwd_ms_median']['this']:.4f} ms, parent "
              f"{row['fwd_bwd_ms_median']['parent']:.4f} ms ({lo:.4f} .. {hi:.4f})", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_wide.json"))
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built (the control)")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.iters)
    # the control first: this process opens the device only after the last worker has gone
    ctl = control(args.parent_root, args.pairs, args.iters) if args.parent_root else "not measured"
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_wide: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    rows = {}
    for d, heads, B, S in WIDE:
        case = _Case(d, heads, B, S, with_aten=True)
        ms = {k: [] for k in case.nets}
        for _ in range(args.pairs):
            for name in case.nets:
                ms[name].append(case.round(name, args.iters))
        row = _summary(ms)
        row["hip_over_aten"] = round(row["fwd_bwd_ms_median"]["hip"] / row["fwd_bwd_ms_median"]["aten"], 4)
        row["library_launches"] = case.launches()
        rows[f"d{d}_h{heads}_{B}x{S}"] = row
        print(f"[token_wide] ({d}, {heads}) {B} x {S}: hip {row['fwd_bwd_ms_median']['hip']:.4f} ms, aten "
              f"{row['fwd_bwd_ms_median']['aten']:.4f} ms per forward + backward", flush=True)
        del case
    rec = {
        "tool": "tools/bench_token_wide.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "config": f"2 x TransformerEncoderLayer(d, heads, ff 4 d, gelu, norm_first), train mode, dropout {P_DROP}; forward + "
                  f"backward per iteration (host clock around {args.iters} iterations ending in a device synchronise: launch "
                  f"overheads of both implementations included); {args.pairs} alternating rounds",
        "shapes": rows,
        "control": ctl,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
