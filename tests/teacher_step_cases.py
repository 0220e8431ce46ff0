"""The teacher configurations that pin the step's plans (tests/test_teacher_plans_cpu.py), its launch sequence
(tests/test_gpu_teacher_step_launches.py) and the one-off bit dump (tools/teacher_step_dump.py): every case of the two tables
of tests/test_gpu_teacher_shapes.py, the default network at mb = 2048 (15-wide observation: k_fwd12, the row-block levels,
LATZ and the first-layer weight gradient from the dZ1 tiles all live there) and the same network with a shared trunk."""
from tests import test_gpu_teacher_shapes as S

DEFAULT_NTE = (256, 16, 2)      # mb = 2048


def _case(nte, units, priv_units, obs_dim=15, P=0, E=0, only_contact=False, shared=False, default_net=False):
    return dict(nte=tuple(nte), units=list(units), priv_units=list(priv_units), obs_dim=obs_dim, P=P, E=E,
                only_contact=bool(only_contact), shared=bool(shared), default_net=default_net)


def step_cases():
    """name -> case; default_net marks the cases recorded under both settings of igi_teacher_set_latz_fuse."""
    cases = {}
    for name, (nte, units, priv_units, obs_dim, _, _, _) in S.NO_CONTACT_CASES.items():
        cases[name] = _case(nte, units, priv_units, obs_dim=obs_dim, default_net=units == S.DEFAULT_UNITS)
    for name, (nte, units, priv_units, P, E, oc, _, _) in S.CONTACT_CASES.items():
        cases["contact_" + name] = _case(nte, units, priv_units, P=P, E=E, only_contact=oc, default_net=units == S.DEFAULT_UNITS)
    cases["default"] = _case(DEFAULT_NTE, S.DEFAULT_UNITS, S.DEFAULT_PRIV_UNITS, default_net=True)
    cases["default_shared"] = _case(DEFAULT_NTE, S.DEFAULT_UNITS, S.DEFAULT_PRIV_UNITS, shared=True, default_net=True)
    return cases


def make_cfg(case, nte=None):
    from isaacgyminsertion_amd.teacher_native import make_cfg as mk
    N, T, Ep = nte or case["nte"]
    return mk(case["obs_dim"], S.PRIV, S.ACT, case["units"], case["priv_units"], N, T, Ep, contact_points=case["P"],
              contact_emb=case["E"], only_contact=case["only_contact"], shared_parameters=case["shared"])[0]


def make_engine(case, seed=1234):
    """(engine with the case's initial parameters loaded, rollout) -- the problem of tests/test_gpu_teacher_shapes.py."""
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    (N, T, Ep), c = case["nte"], case
    if c["shared"]:
        from tests import shared_critic_ref as sr
        init, ro, perm = sr.problem(N, T, c["units"], c["priv_units"], seed=seed)
    else:
        init, ro, perm = S._problem(N, T, c["units"], c["priv_units"], c["obs_dim"], c["P"], c["E"], c["only_contact"], seed=seed)
    eng = TeacherEngine(N, T, Ep, units=c["units"], priv_units=c["priv_units"], perm=perm, obs_dim=c["obs_dim"],
                        contact_points=c["P"], contact_emb=c["E"], only_contact=c["only_contact"],
                        shared_parameters=c["shared"])
    eng.load_params(init)
    return eng, ro
