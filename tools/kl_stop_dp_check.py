#!/usr/bin/env python
"""KL early stopping under data parallelism, two processes on ONE GPU over gloo (as tools/lr_schedule_dp_check.py: both
ranks on cuda:0, a real torch.distributed group): each rank has its own rollout (seeds 1234 / 1235) on the small ragged
network of the early-stopping tests, an identical start, and runs TeacherEngine.update_dp with kl_early_stop -- the step's
estimator travels as one float through the reducer (bucket 4) and every rank must stop at the same step.

    python tools/kl_stop_dp_check.py        # one JSON line: per rank the stop step, the estimator record, a parameter sum

The parent never touches the GPU; a failing rank ends the other one (torch.multiprocessing.spawn)."""
import json
import os
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, T, E = 100, 6, 3
UNITS, PRIV_UNITS = [48, 40, 24], [24, 16, 8]
LR0, THR = 5e-3, 5e-3


def worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from oracle import synth
    init0, _, _ = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, seed=1234)      # identical start on every rank
    _, ro, perm = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, seed=1234 + rank)
    res = {}
    for mode in ("alone", "serial", "overlapped"):
        eng = TeacherEngine(N, T, E, units=UNITS, priv_units=PRIV_UNITS, perm=perm, device="cuda:0", lr=LR0,
                            kl_early_stop=True, kl_threshold=THR if mode != "alone" else 1e9)
        eng.load_params(init0)
        eng.prepare(ro)
        if mode == "alone":               # this rank's own estimator sequence, nothing stops: what the mean is made of
            eng.update()
        else:
            kw = dict(all_reduce_async=lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True)) \
                if mode == "overlapped" else {}
            eng.update_dp(lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM), world, **kw)
        torch.cuda.synchronize()
        res[mode] = dict(stop=eng.stop_step, adam_t=eng.adam_t, approx_kl=eng.approx_kl().tolist(),
                         params_sum=float(eng.params.double().sum().item()),
                         rms_count=float(eng.rms_obs[-1].item()))
    dist.barrier()
    dist.destroy_process_group()
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    world = 2
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(worker, args=(world, 29634, outdir), nprocs=world, join=True)
        ranks = [json.load(open(os.path.join(outdir, f"rank{r}.json"))) for r in range(world)]
    print(json.dumps({"check": "kl early stop, dp 2 ranks on one GPU (gloo)", "lr0": LR0, "kl_threshold": THR,
                      "mb": N * T // E, "ranks": ranks}))
