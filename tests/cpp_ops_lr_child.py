"""Child process of tests/test_gpu_lr_schedule.py::test_cpp_and_python_registrations_agree_under_the_schedule: ONE
registration of torch.ops.mi355ppo (the C++ one of csrc/torch_ops.cpp or the Python one of ops.py, as
tests/cpp_ops_child.py) runs prepare, a whole update and a step-wise second update with the adaptive schedule's longer
lists -- icfg + [1], fcfg + [kl_threshold, lr_min, lr_max], the state list + lr_state.

    python tests/cpp_ops_lr_child.py cpp|py out.npz"""
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
    icfg = [15, 64, 6, 3] + priv_units + [0] * (M - 3) + [3] + units + [0] * (M - 3) + [N, T, E] + [1]
    fcfg = [0.99, 0.95, 2.5e-4, 0.9, 0.999, 1e-8, 0.2, 4.0, 0.0, 1e-4, 1.0, 1e-5] + [0.004, 1e-6, 1e-2]
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
    params = torch.zeros(P, **f32)
    for (k, v), o_, s_ in zip(init.items(), off, sz):
        params[o_:o_ + s_] = v.reshape(-1).to(dev)

    def rms(d):
        s = torch.zeros(2 * d + 1, dtype=torch.float64, device=dev)
        s[d:2 * d] = 1.0
        s[2 * d] = 1.0
        return s

    lr_state = torch.zeros(_lib.lr_state_doubles(E), dtype=torch.float64, device=dev)
    lr_state[0] = 2.5e-4
    state = [params, torch.zeros(P, **f32), torch.zeros(P, **f32), torch.zeros(P, **f32), rms(15), rms(64), rms(1),
             perm.to(dev), torch.zeros(T, N, 1, **f32), torch.zeros(T, N, **f32), torch.zeros(T, N, 1, **f32),
             torch.zeros(T, N, 1, **f32), torch.zeros(T, N, 6, **f32), torch.zeros(T, N, 6, **f32),
             torch.zeros(E * E, _lib.IGI_STATS_PER_STEP, **f32),
             torch.zeros(int(L.igi_teacher_workspace_bytes(C.byref(cfg))), dtype=torch.uint8, device=dev), lr_state]
    rollout = [ro[k].to(dev).contiguous() for k in ("obses", "priv_info", "rewards", "values", "neglogpacs", "dones",
                                                     "actions", "mus", "sigmas", "last_values")]
    out = {}
    refused = []
    for bad_state, bad_i, bad_f in ((state[:16], icfg, fcfg), (state, icfg[:-1], fcfg), (state, icfg, fcfg[:12]),
                                    (state, icfg[:-1] + [2], fcfg)):
        try:
            o.gae_advnorm(rollout, bad_state, bad_i, bad_f, True)
            refused.append(0)
        except RuntimeError:
            refused.append(1)
    out["refused"] = torch.tensor(refused)
    o.gae_advnorm(rollout, state, icfg, fcfg, True)
    o.ppo_update(rollout, state, icfg, fcfg, 0)
    out["params_after"], out["stats"], out["lr_state"] = state[0].clone(), state[14].clone(), lr_state.clone()
    o.gae_advnorm(rollout, state, icfg, fcfg, True)
    slot = 0
    for _ in range(E):
        for i in range(E):
            o.ppo_minibatch_fwd_bwd(rollout, state, icfg, fcfg, i, slot, -1)
            o.ppo_clip_adam(state, icfg, fcfg, slot, E * E + slot + 1, 1.0)
            slot += 1
    out["params_after2"], out["stats2"], out["lr_state2"] = state[0].clone(), state[14].clone(), lr_state.clone()
    mu, val, lat = o.actor_critic_infer(state, icfg, fcfg, rollout[0][0], rollout[1][0], True, True)
    out["mu"] = mu
    torch.cuda.synchronize()
    np.savez(path, **{k: t.detach().cpu().numpy() for k, t in out.items()})


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2])
