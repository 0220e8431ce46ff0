"""Child process of tests/test_gpu_kl_stop.py::test_cpp_and_python_registrations_agree: ONE registration of
torch.ops.mi355ppo (the C++ one of csrc/torch_ops.cpp or the Python one of ops.py, as tests/cpp_ops_child.py) runs the
teacher update with the early-stopping tail behind hand-built lists -- icfg + [1], fcfg + [kl_threshold], the state list
+ stop_state -- first with a threshold nothing reaches, then, from the same start, with 1.5 thr between the estimator
that run recorded for a step k and the largest before it, once in one call and once step by step.  Lists of today's length keep working.

    python tests/cpp_ops_stop_child.py cpp|py out.npz"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(which, path):
    if which == "cpp":
        torch.ops.load_library(os.path.join(ROOT, "isaacgyminsertion_amd", "libigi_torch_ops.so"))
        assert "isaacgyminsertion_amd.ops" not in sys.modules
    else:
        import isaacgyminsertion_amd.ops  # noqa: F401
    o = torch.ops.mi355ppo
    from isaacgyminsertion_amd import _lib          # ctypes only: struct layouts + size queries of the C ABI
    from oracle import synth
    dev = torch.device("cuda:0")
    N, T, E = 64, 8, 4
    units, priv_units = [64, 48, 32], [48, 32, 8]
    init, ro, perm = synth.teacher_problem(N, T, units, priv_units, seed=9, done_p=0.1)
    M = _lib.IGI_MAX_LAYERS
    icfg = [15, 64, 6, 3] + priv_units + [0] * (M - 3) + [3] + units + [0] * (M - 3) + [N, T, E]
    fcfg = [0.99, 0.95, 3e-3, 0.9, 0.999, 1e-8, 0.2, 4.0, 0.0, 1e-4, 1.0, 1e-5]
    cfg = _lib.TeacherCfg()
    cfg.obs_dim, cfg.priv_dim, cfg.act_dim, cfg.n_priv_layers, cfg.n_layers = 15, 64, 6, 3, 3
    for i in range(3):
        cfg.priv_units[i], cfg.units[i] = priv_units[i], units[i]
    cfg.num_envs, cfg.horizon, cfg.mini_epochs = N, T, E
    L = _lib.lib()
    n = L.igi_teacher_param_offsets(C.byref(cfg), None, None, 0)
    off, sz = (C.c_int64 * n)(), (C.c_int64 * n)()
    L.igi_teacher_param_offsets(C.byref(cfg), off, sz, n)
    P = int(L.igi_teacher_param_count(C.byref(cfg)))
    f32 = dict(dtype=torch.float32, device=dev)

    def rms(d):
        s = torch.zeros(2 * d + 1, dtype=torch.float64, device=dev)
        s[d:2 * d] = 1.0
        s[2 * d] = 1.0
        return s

    def fresh():
        params = torch.zeros(P, **f32)
        for (k, v), o_, s_ in zip(init.items(), off, sz):
            params[o_:o_ + s_] = v.reshape(-1).to(dev)
        return [params, torch.zeros(P, **f32), torch.zeros(P, **f32), torch.zeros(P, **f32), rms(15), rms(64), rms(1),
                perm.to(dev), torch.zeros(T, N, 1, **f32), torch.zeros(T, N, **f32), torch.zeros(T, N, 1, **f32),
                torch.zeros(T, N, 1, **f32), torch.zeros(T, N, 6, **f32), torch.zeros(T, N, 6, **f32),
                torch.zeros(E * E, _lib.IGI_STATS_PER_STEP, **f32),
                torch.zeros(int(L.igi_teacher_workspace_bytes(C.byref(cfg))), dtype=torch.uint8, device=dev)]

    rollout = [ro[k].to(dev).contiguous() for k in ("obses", "priv_info", "rewards", "values", "neglogpacs", "dones",
                                                     "actions", "mus", "sigmas", "last_values")]
    words = _lib.stop_state_words(E * E)
    out = {}

    def update(thr, stepwise=False):
        state, stop = fresh(), torch.full((words,), -1, dtype=torch.int32, device=dev)
        o.gae_advnorm(rollout, state, icfg, fcfg, True)              # today's lists: the other ops do not take the tail
        st, ic, fc = state + [stop], icfg + [1], fcfg + [thr]
        if stepwise:
            for slot in range(E * E):
                o.ppo_minibatch_fwd_bwd(rollout, st, ic, fc, slot % E, slot, -1)
                o.ppo_clip_adam(st, ic, fc, slot, slot + 1, 1.0)
        else:
            o.ppo_update(rollout, st, ic, fc, 0)
        torch.cuda.synchronize()
        return state, stop

    state, stop = update(1e9)
    out["params_through"], out["stats_through"], out["stop_through"] = state[0].clone(), state[14].clone(), stop.clone()
    plain = fresh()                                                  # the same update through today's lists
    o.gae_advnorm(rollout, plain, icfg, fcfg, True)
    o.ppo_update(rollout, plain, icfg, fcfg, 0)
    out["params_plain"], out["stats_plain"] = plain[0].clone(), plain[14].clone()
    seq = stop[2:].view(torch.float32).double().cpu().numpy()
    # the stop aimed at: the first step from the fourth on whose estimator is 1.3 x everything before it
    k = next(k for k in range(3, E * E) if seq[k] >= 1.3 * seq[:k].max())
    thr = float(np.sqrt(seq[:k].max() * seq[k])) / 1.5
    out["thr"], out["target"] = torch.tensor(thr, dtype=torch.float64), torch.tensor(k)
    state, stop = update(thr)
    out["params_stopped"], out["adam_m_stopped"], out["rms_obs_stopped"] = state[0].clone(), state[2].clone(), state[4].clone()
    out["stop_stopped"] = stop.clone()
    state, stop = update(thr, stepwise=True)
    out["params_stepwise"], out["stop_stepwise"] = state[0].clone(), stop.clone()
    refused = []
    state, stop = fresh(), torch.full((words,), -1, dtype=torch.int32, device=dev)
    o.gae_advnorm(rollout, state, icfg, fcfg, True)
    for bad_state, bad_i, bad_f in ((state, icfg + [1], fcfg + [thr]),                    # the tensor is missing
                                    (state + [stop[:-1].contiguous()], icfg + [1], fcfg + [thr]),
                                    (state + [stop], icfg + [0], fcfg + [thr]),
                                    (state + [stop], icfg + [1], fcfg + [0.0]),
                                    (state + [stop.float()], icfg + [1], fcfg + [thr])):
        try:
            o.ppo_update(rollout, bad_state, bad_i, bad_f, 0)
            refused.append(0)
        except RuntimeError:
            refused.append(1)
    out["refused"] = torch.tensor(refused)
    torch.cuda.synchronize()
    np.savez(path, **{k: t.detach().cpu().numpy() for k, t in out.items()})


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2])
