#!/usr/bin/env python
"""What the depth backbone's bf16-input mode costs in accuracy: output and gradient of one backbone at 768 images
(tests/golden/make_golden_depth.py:depth_case(32, 768, seed=768)) with the mode off and on, against the UN-rounded float64
network of oracle/encoders.py:depth_backbone on the same inputs.  Per parameter tensor max|g - g64| / max|g64| both ways, the
same for the output, next to the fp32 CPU oracle's own distance from float64.

Images in which a pool window's two largest pre-pool values are within 5e-7 of each other (oracle/encoders.py:
depth_pool_near_ties) carry no upstream gradient, as in tests/test_gpu_depth_scale.py: which of the two an fp32 sum calls the
larger is not defined by the reference either, in either mode (conv1 is fp32 in both).  The share is in the record.

    python tools/depth_bf16_accuracy.py --out profiles/depth_bf16_accuracy.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def device_run(sd, x, gy, on):
    from isaacgyminsertion_amd import ops
    from isaacgyminsertion_amd.algo.models.transformer.depth_backbone import DepthOnlyFCBackbone54x96
    m = DepthOnlyFCBackbone54x96(latent_dim=gy.shape[1])
    m.load_state_dict(sd)
    m = m.cuda()
    with ops.depth_bf16_inputs(on):
        y = m(x.cuda())
        y.backward(gy.cuda())
        torch.cuda.synchronize()
    return y.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bf16_accuracy.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    from make_golden_depth import depth_case
    from oracle import encoders as oe
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B = args.images
    sd, x, dy = depth_case(latent=32, batch=B, seed=B)
    near = oe.depth_pool_near_ties(x, sd)
    gy = dy.clone()
    gy[near] = 0.0
    y_off, g_off = device_run(sd, x, gy, False)
    y_on, g_on = device_run(sd, x, gy, True)
    y32, g32 = oe.value_and_grads(oe.depth_backbone, x, sd, gy, chunk=64)
    y64, g64 = oe.value_and_grads(oe.depth_backbone, x, sd, gy, dtype=torch.float64, chunk=64)

    def row(off, on, o32, ref):
        scale = float(ref.abs().max())
        return {"max_abs_fp64": scale, "fp32_path_err": float((off.double() - ref).abs().max()) / scale,
                "bf16_mode_err": float((on.double() - ref).abs().max()) / scale,
                "fp32_cpu_oracle_err": float((o32.double() - ref).abs().max()) / scale}

    rec = {"what": f"one depth backbone at {B} images (depth_case(32, {B}, seed={B})), mode off / on against the un-rounded "
                   "float64 network (oracle/encoders.py:depth_backbone): per tensor max|g - g64| / max|g64|, the same for the "
                   "output y; fp32_cpu_oracle_err = the fp32 CPU oracle against float64 on the same scale",
           "build": ge.library_hash(), "images": B, "images_without_upstream_gradient": int(near.sum()),
           "output": row(y_off, y_on, y32, y64),
           "gradients": {k: row(g_off[k], g_on[k], g32[k], g64[k]) for k in sd}}
    print(json.dumps(rec, indent=1))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
