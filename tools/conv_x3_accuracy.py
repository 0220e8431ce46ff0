#!/usr/bin/env python
"""Accuracy of the split-bf16 mode of the tactile convolutions next to the fp32 path and the one-plane bf16-input mode:
the raw step-0 gradient of the student on the two tactile + lin instances of tests/golden/student.npz (``tac_lin``: well
conditioned; ``tac_lin_illcond``: the conv stack under the soft-argmax cancels heavily) under each arithmetic, against the
UN-rounded fp64 gradient of oracle/student.py on the same minibatch -- the method of tools/conv_bf16_accuracy.py.  Per
tensor: max |g - g64| / max |g64| in three columns, fp32 | x3 | bf16, next to the reference's own fp32 noise recorded in
the fixture (grad0_ref_noise = max |reference fp32 - its fp64 rerun|).

    python tools/conv_x3_accuracy.py --out profiles/conv_x3_accuracy.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"fp32": {}, "x3": {"conv_bf16x3": True}, "bf16": {"conv_bf16_inputs": True}}


def step0_gradient(G, tag, keys):
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    n, T, E, tactile, pcl, img = [int(x) for x in G[f"{tag}/flags"]]
    cfg = default_config(num_envs=n, horizon_length=T, rl_device="cuda:0", mini_epochs=E, obs_info=True,
                         tactile_info=True, pcl_info=False, img_info=False, seg_info=False, num_points=8)
    cfg.offline_train.model.conv_bf16_inputs = bool(keys.get("conv_bf16_inputs", False))
    cfg.offline_train.model.conv_bf16x3 = bool(keys.get("conv_bf16x3", False))
    env = SyntheticInsertionEnv(n, device="cuda:0", tactile_hw=(32, 64), pcl_points=0, img_hw=None)
    agent = ExtrinsicAdapt(env, None, cfg)
    model = agent.student.model
    init = {k[len(tag) + 6:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/init/")}
    model.load_state_dict(init)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    for k in agent.storage.storage_dict:
        agent.storage.storage_dict[k].copy_(torch.from_numpy(G[f"{tag}/in/{k}"]))
    agent.storage.indices.copy_(torch.from_numpy(G[f"{tag}/perm"]))
    agent.storage.prepare_training()
    agent.set_student_train()
    b = agent.storage[0]
    mb = agent.minibatch_size
    data = {"teacher_actions": b["teacher_actions"].reshape(mb, -1).cpu(),
            "tactile": b["n_tactile"].reshape(mb, 3, -1).cpu(), "student_obs": b["n_student_obs"].reshape(mb, -1).cpu()}
    grad0 = {}

    def probe(step, m):
        if step == 0:
            grad0.update({k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()
                          if p.requires_grad and p.grad is not None})

    agent.grad_probe = probe
    agent.update()
    torch.cuda.synchronize()
    return grad0, init, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_x3_accuracy.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    from oracle import student as os_
    torch.set_num_threads(min(16, torch.get_num_threads()))
    G = np.load(os.path.join(ROOT, "tests", "golden", "student.npz"))
    rec = {"what": "step-0 gradient of the student (tactile + lin, tests/golden/student.npz) with the tactile convolutions in "
                   "fp32, split-bf16 (x3: conv_bf16x3) and bf16-input (bf16: conv_bf16_inputs) arithmetic against the "
                   "un-rounded fp64 gradient (oracle/student.py): per tensor max|g - g64| / max|g64|; ref_fp32_noise = the "
                   "reference's own fp32 run against its fp64 rerun (grad0_ref_noise of the fixture) on the same scale",
           "build": ge.library_hash(), "cases": {}}
    for tag in ("tac_lin", "tac_lin_illcond"):
        grads = {}
        for mode, keys in MODES.items():
            grads[mode], init, data = step0_gradient(G, tag, keys)
        _, g64 = os_.loss_and_grads(init, data["teacher_actions"], data["tactile"], data["student_obs"], None, (32, 64),
                                    dtype=torch.float64)
        rows = {}
        for k, ref in g64.items():
            if ref is None or float(ref.abs().max()) == 0.0 or k not in grads["fp32"]:
                continue
            scale = float(ref.abs().max())
            noise_key = f"{tag}/grad0_ref_noise/{k}"
            rows[k] = {"max_abs_g64": scale,
                       **{f"{mode}_err": float((grads[mode][k].double() - ref).abs().max()) / scale for mode in MODES},
                       "ref_fp32_noise": (float(G[noise_key]) / scale) if noise_key in G.files else None}
        rec["cases"][tag] = rows
        tac = {k: v for k, v in rows.items() if k.startswith("tactile_encoder.")}
        print(tag, json.dumps({k: {a: (float(f"{b:.3g}") if isinstance(b, float) else b) for a, b in v.items()}
                               for k, v in tac.items()}, indent=1), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
