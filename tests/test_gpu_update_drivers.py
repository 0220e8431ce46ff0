"""The teacher update's drivers against each other: update(), update_dp() through a callback that reduces nothing at
world 1, and update_dp_native() on a one-rank communicator with the overlapped and the serial schedule run ONE loop
(csrc/teacher.h teacher_update_steps) and differ only in what they put between the stages of a step.  So on one rank
all four must leave the same bits behind, and their launches may differ only by what the exchange adds: the second
slab reduction of a two-phase step, the scheduler's second half, the stop's decision kernel.

The library is compared with itself; the single-GPU update is held to the oracle by test_gpu_teacher.py,
test_gpu_lr_schedule.py and test_gpu_kl_stop.py.  Every comparison is exact."""
import pytest
import torch

from tests import kl_stop_cases as K
from tests import lr_schedule_cases as L

pytestmark = pytest.mark.gpu

DRIVERS = ("single", "callback", "rccl_overlap", "rccl_serial")
TWO_PHASE = ("callback", "rccl_overlap")
SLAB, SCHED = "k_slab_reduce", "k_lr_schedule"      # SCHED: the scheduler's class, which k_stop_decide shares
STATE = ("params", "adam_m", "adam_v", "rms_obs", "rms_priv", "mus_w", "sigmas_w")

# id: (K.CASES entry, kl_early_stop, adaptive rate, mini-epochs the host enqueues (None: all E))
CASES = {
    "C-stop": ("C", True, False, None),                  # stop at step 4
    "C-plain": ("C", False, False, None),                # the plain loop at the same shape
    "C_contacts-stop": ("C_contacts", True, False, None),   # stop at step 6, the first step of a mini-epoch
    # stop at step 6 of 16; the scheduler runs on the partial mean; the look-ahead ends the enqueueing after mini-epoch 2
    "adaptive-stop": ("adaptive", True, True, 3),
    "adaptive-rate-only": ("adaptive", False, True, None),  # the rate exchange alone
    "no_stop": ("no_stop", True, False, None),           # a threshold nothing reaches: the look-ahead waits, nothing stops
}


@pytest.fixture(scope="module")
def comm():
    from isaacgyminsertion_amd.utils.dist import NativeComm
    torch.cuda.set_device(0)
    c = NativeComm(rank=0, world=1)
    yield c
    c.close()


def _run(name, stopping, adaptive, driver, comm):
    """One update by `driver` on a fresh engine: (what it left behind, launches per profiler class)."""
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    c = K.CASES[name]
    N, T, E = c["shape"]
    P, Ec = c["contacts"]
    init, ro, perm = K.case_problem(name)
    eng = TeacherEngine(N, T, E, units=c["units"], priv_units=c["priv_units"], perm=perm, device="cuda:0", obs_dim=L.OBS,
                        contact_points=P, contact_emb=Ec, lr=c["lr"], kl_early_stop=stopping,
                        kl_threshold=c["thr"], lr_schedule="adaptive" if adaptive else "fixed")
    eng.load_params(init)
    eng.prepare(ro)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        if driver == "single":
            eng.update()
        elif driver == "callback":
            eng.update_dp(all_reduce=lambda t: None, world_size=1)
        else:
            eng.update_dp_native(comm, overlap=(driver == "rccl_overlap"))
        torch.cuda.synchronize()
        launches = {}
        for cl in _lib.prof_read():
            launches[cl["name"]] = launches.get(cl["name"], 0) + cl["launches"]
    finally:
        _lib.prof_enable(False)
    s = eng.stop_step
    out = {k: getattr(eng, k).clone() for k in STATE}
    out["stats"] = eng.stats.clone() if s is None else torch.cat([eng.stats[:s].reshape(-1), eng.stats[s, :5]])
    if adaptive:                 # the exchange scratch (lr_state[1]) is only written by the data-parallel paths
        out["lr_state"] = torch.cat([eng.lr_state[:1], eng.lr_state[2:]])
    if stopping:
        out["approx_kl"] = eng.approx_kl()
    out["counts"] = torch.tensor([-1 if s is None else s, eng.steps_applied, eng.adam_t])
    return out, {k: v for k, v in launches.items() if v}, eng.n_mb


@pytest.mark.parametrize("case", list(CASES))
def test_the_four_drivers_leave_the_same_bits_and_differ_only_by_their_exchange(case, comm):
    name, stopping, adaptive, enq_epochs = CASES[case]
    if stopping:
        K.assert_margins(name)
    E = K.CASES[name]["shape"][2]
    runs = {d: _run(name, stopping, adaptive, d, comm) for d in DRIVERS}
    ref, base, n_mb = runs["single"]
    want_stop = K.CASES[name]["stop"] if stopping else None
    assert ref["counts"].tolist() == [-1 if want_stop is None else want_stop,
                                      E * n_mb if want_stop is None else want_stop,
                                      E * n_mb if want_stop is None else want_stop]
    for d in DRIVERS[1:]:
        got = runs[d][0]
        assert got.keys() == ref.keys()
        for k in ref:
            assert torch.equal(ref[k], got[k]), (d, k)

    epochs = E if enq_epochs is None else enq_epochs      # mini-epochs the host enqueues
    steps = epochs * n_mb
    assert base["k_sumsq_stats"] == steps, base
    print(f"{case}: {steps} steps in {epochs} mini-epochs enqueued; update(): {base.get(SLAB)} {SLAB}, "
          f"{base.get(SCHED, 0)} {SCHED}")
    assert runs["callback"][1] == runs["rccl_overlap"][1]
    for d in DRIVERS[1:]:
        want = dict(base)
        want[SLAB] = base[SLAB] + (steps if d in TWO_PHASE else 0)
        sched = base.get(SCHED, 0) + (epochs if adaptive else 0) + (steps if stopping else 0)
        if sched:
            want[SCHED] = sched
        assert runs[d][1] == want, (d, {k: (runs[d][1].get(k), want.get(k)) for k in set(want) | set(runs[d][1])
                                        if runs[d][1].get(k) != want.get(k)})
