"""Child process of tests/test_shared_critic_cpu.py::test_cpp_registration_decodes_a_shared_cfg and of
tests/test_gpu_shared_critic.py::test_cpp_and_python_registrations_agree_on_a_shared_teacher: ONE registration of
torch.ops.mi355ppo (the C++ one of csrc/torch_ops.cpp or the Python one of ops.py, as tests/cpp_ops_child.py) takes the
shared-trunk cfg -- icfg + [1, 0] behind (num_envs, horizon, mini_epochs), ahead of the schedule and early-stopping tails.

    python tests/cpp_ops_shared_child.py decode             (CPU: prints one JSON line)
    python tests/cpp_ops_shared_child.py run cpp|py out.npz (GPU)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, E = 64, 8, 4
UNITS, PRIV_UNITS = [64, 48, 32], [48, 32, 8]
FCFG = [0.99, 0.95, 2.5e-4, 0.9, 0.999, 1e-8, 0.2, 4.0, 0.0, 1e-4, 1.0, 1e-5]
SCHED_F = [0.004, 1e-6, 1e-2]


def _icfg(M, tail):
    return [15, 64, 6, 3] + PRIV_UNITS + [0] * (M - 3) + [3] + UNITS + [0] * (M - 3) + [N, T, E] + tail


def _load(which):
    if which == "cpp":
        torch.ops.load_library(os.path.join(ROOT, "isaacgyminsertion_amd", "libigi_torch_ops.so"))
        assert "isaacgyminsertion_amd.ops" not in sys.modules
    else:
        import isaacgyminsertion_amd.ops  # noqa: F401
    return torch.ops.mi355ppo


def decode():
    """CPU: the decoder runs ahead of the tensor checks, so a cfg it accepts ends in the CPU-tensor refusal and one it
    does not ends in its own message."""
    o = _load("cpp")
    from isaacgyminsertion_amd import _lib
    M = _lib.IGI_MAX_LAYERS
    state = [torch.zeros(4) for _ in range(17)]
    rollout = [torch.zeros(4) for _ in range(10)]

    def kind(icfg, fcfg, st):
        try:
            o.gae_advnorm(rollout, st, icfg, fcfg, True)
        except RuntimeError as e:
            msg = str(e)
            for key in ("shared-trunk fields", "teacher cfg"):
                if key in msg:
                    return key
            return "tensor" if "expected a HIP (cuda) tensor" in msg else msg[:200]
        return "accepted"
    out = {"plain": kind(_icfg(M, []), FCFG, state[:16]),
           "shared": kind(_icfg(M, [1, 0]), FCFG, state[:16]),
           "shared_sched": kind(_icfg(M, [1, 0, 1]), FCFG + SCHED_F, state),
           "field_2": kind(_icfg(M, [2, 0]), FCFG, state[:16]),
           "nine_ints": kind(_icfg(M, [1]), FCFG, state[:16])}
    print(json.dumps(out))


def run(which, path):
    o = _load(which)
    from isaacgyminsertion_amd import _lib          # ctypes only: struct layouts + size queries of the C ABI
    from tests import shared_critic_ref as sr
    dev = torch.device("cuda:0")
    init, ro, perm = sr.problem(N, T, UNITS, PRIV_UNITS, seed=9, done_p=0.1)
    M = _lib.IGI_MAX_LAYERS
    icfg, fcfg = _icfg(M, [1, 0]), list(FCFG)
    cfg = _lib.TeacherCfg()
    cfg.obs_dim, cfg.priv_dim, cfg.act_dim, cfg.n_priv_layers, cfg.n_layers = 15, 64, 6, 3, 3
    for i in range(3):
        cfg.priv_units[i], cfg.units[i] = PRIV_UNITS[i], UNITS[i]
    cfg.num_envs, cfg.horizon, cfg.mini_epochs, cfg.shared_parameters = N, T, E, 1
    L = _lib.lib()
    n = L.igi_teacher_param_offsets(C.byref(cfg), None, None, 0)
    assert n == len(init) == 17
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

    state = [params, torch.zeros(P, **f32), torch.zeros(P, **f32), torch.zeros(P, **f32), rms(15), rms(64), rms(1),
             perm.to(dev), torch.zeros(T, N, 1, **f32), torch.zeros(T, N, **f32), torch.zeros(T, N, 1, **f32),
             torch.zeros(T, N, 1, **f32), torch.zeros(T, N, 6, **f32), torch.zeros(T, N, 6, **f32),
             torch.zeros(E * E, _lib.IGI_STATS_PER_STEP, **f32),
             torch.zeros(int(L.igi_teacher_workspace_bytes(C.byref(cfg))), dtype=torch.uint8, device=dev)]
    rollout = [ro[k].to(dev).contiguous() for k in ("obses", "priv_info", "rewards", "values", "neglogpacs", "dones",
                                                     "actions", "mus", "sigmas", "last_values")]
    out = {}
    refused = []
    for bad_i in (icfg[:-2] + [2, 0], icfg[:-1], icfg[:-2]):   # field not 1; 9 + 2M ints; a separate-critic cfg on this state
        try:
            o.gae_advnorm(rollout, state, bad_i, fcfg, True)
            refused.append(0)
        except RuntimeError:
            refused.append(1)
    out["refused"] = torch.tensor(refused)
    o.gae_advnorm(rollout, state, icfg, fcfg, True)
    o.ppo_update(rollout, state, icfg, fcfg, 0)
    out["params_after"], out["stats"] = state[0].clone(), state[14].clone()
    # a second update step by step, under the early-stopping tail (a threshold no step reaches: it runs through)
    stop = torch.zeros(_lib.stop_state_words(E * E), dtype=torch.int32, device=dev)
    stop[0] = -1
    st2, ic2, fc2 = state + [stop], icfg + [1], fcfg + [10.0]
    o.gae_advnorm(rollout, state, icfg, fcfg, True)
    slot = 0
    for _ in range(E):
        for i in range(E):
            o.ppo_minibatch_fwd_bwd(rollout, st2, ic2, fc2, i, slot, -1)
            o.ppo_clip_adam(st2, ic2, fc2, slot, E * E + slot + 1, 1.0)
            slot += 1
    out["params_after2"], out["stats2"], out["stop"] = state[0].clone(), state[14].clone(), stop.clone()
    mu, val, lat = o.actor_critic_infer(state, icfg, fcfg, rollout[0][0], rollout[1][0], True, True)
    out["mu"], out["val"], out["lat"] = mu, val, lat
    torch.cuda.synchronize()
    np.savez(path, **{k: t.detach().cpu().numpy() for k, t in out.items()})


if __name__ == "__main__":
    if sys.argv[1] == "decode":
        decode()
    else:
        run(sys.argv[2], sys.argv[3])
