"""The arrowhead factor-and-solve (ldl_arrow_solve, on M and on the Newton Hessian) keeps the parent's bits.

Same record-or-compare mechanism as tests/test_gpu_bits_vs_parent.py (its docstring): the fixtures
under tests/golden/bits_parent_ldl/ were recorded on an MI355X with the build of the commit before
the round-11 work on ldl_arrow_solve (the leg rounds' exchanges), an edit that may move values
between lanes, LDS words and registers and must leave every value, operation order and FMA
contraction as it was.  PP3_RECORD_PARENT_BITS=1 at the parent commit writes the fixtures;
otherwise the module compares.

Cases (the smallest shapes at which a re-laid leg elimination can go wrong; each asserts that it
holds the contacts and limit rows it claims, from the pipeline record of the first substep and from
jnt_range at the start state):
  physics_kernel, 2 and 5 airborne envs, 1 and 3 substeps   (the M solve; H = M + frictionloss D; the
                                                             odd count's clamped last half)
  physics_kernel, 8 envs with ONE foot down, leg g = 0..3, another g in the two halves of every wave,
      1 and 3 substeps; the same states through one fused env step, NC = 8 and NC = 16
  physics_kernel, 4 envs with all four feet down
  physics_kernel, 6 airborne envs with one hinge past its limit at level 0, 1 or 2 of a leg (the
      limit row's D on that level's diagonal), another level in the two halves of every wave
  physics_kernel, 4 envs: a leg-leg env beside a standing one (the whole wave on ldl_arrow_solve_b or
      the dense path), and a plain standing pair in the next wave
  physics_kernel, 10-box model, 4 envs over the rails       (the CULL instantiation)
  flat model, 5 envs x 2 steps fused, domain randomisation on (other masses: another M)
  flat model with solver iterations = 2, 6 envs x 2 steps fused
  policy rollout, 20 envs x 2 steps                          (not a multiple of 16: partial tile)
  flat model, 5 envs: a reset, then one step
  flat model, 5 envs x 4 steps fused with the pipeline record

A base-only contact (support 4) cannot be posed: the model's collidable geoms are the ground plane,
the obstacle boxes and two spheres per leg (bodies 3 g + 3 and 3 g + 4); the base body carries none
(test_base_body_has_no_collision_geom asserts it), so every contact's support is a leg.
"""
import os

import numpy as np
import pytest

import common
from pupperv3_mjx import MODEL_XML, _abi, _lib
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_bits_vs_parent import RECORD, _acts, _bits, _fused, _hip_identity
from test_gpu_bits_vs_parent_lds import _physics_bits, _rollout_bits
from test_gpu_bits_vs_parent_rows import _con_geoms, _ncon, active_limits

pytestmark = pytest.mark.gpu

DIR = os.path.join(common.GOLDEN, "bits_parent_ldl")


def _check_or_record(case, got):
    path = os.path.join(DIR, case + ".npz")
    version, device = _hip_identity()
    if RECORD:
        os.makedirs(DIR, exist_ok=True)
        np.savez_compressed(path, hip_runtime_version=np.int64(version), device_name=np.array(device), **got)
        return
    assert os.path.exists(path), f"fixture {path} is missing: record it at the parent commit (module docstring)"
    want = np.load(path)
    rec = (int(want["hip_runtime_version"]), str(want["device_name"]))
    assert rec == (version, device), (
        f"fixture recorded with HIP runtime / device {rec}, this machine has {(version, device)}: "
        "re-record the fixtures with the parent commit's build on this machine (module docstring)")
    assert sorted(got) == sorted(k for k in want.files if k not in ("hip_runtime_version", "device_name"))
    for k, v in got.items():
        w = want[k]
        assert v.dtype == w.dtype and v.shape == w.shape, (k, v.dtype, w.dtype, v.shape, w.shape)
        bad = np.argwhere(v != w)
        assert bad.size == 0, f"{case}: {k} differs from the parent's bits at {len(bad)} places, first {bad[0]}"


@pytest.fixture(scope="module")
def flat_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_ldl_flat"), 0)


@pytest.fixture(scope="module")
def box_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_ldl_box"), 10)


def _leg_of_geom(model):
    """geom id -> leg 0..3 of its body (bodies 2 + 3 g .. 4 + 3 g), -1 for the world, 4 for the base"""
    return {int(model.cgeom_id[g]): common._leg_of_body(int(model.cgeom_bodyid[g])) for g in range(model.ncgeom)}


def _contact_legs(model, pipe, i):
    """sorted legs of env i's contacts with the world (a leg-leg contact raises)"""
    leg = _leg_of_geom(model)
    out = []
    for a, b in _con_geoms(pipe, i):
        la, lb = leg[int(a)], leg[int(b)]
        assert min(la, lb) == -1, (i, a, b)
        out.append(max(la, lb))
    return sorted(out)


def states_with_feet_down(model, legs_per_env, seed):
    """Seeded states whose contacts are exactly one ground contact of each leg in legs_per_env[i]
    (rejection sampling of base height, tilt and joint angles against the oracle, as
    common.states_with_self_contact does)."""
    from oracle import oracle as O
    leg = _leg_of_geom(model)
    rs = np.random.RandomState(seed)
    qs = []
    for want in legs_per_env:
        for _ in range(100000):
            q = np.zeros(19)
            q[2] = rs.uniform(0.10, 0.19)
            ax = rs.normal(size=3)
            ax /= np.linalg.norm(ax)
            ang = rs.uniform(0, 0.5)
            q[3:7] = np.concatenate([[np.cos(ang / 2)], ax * np.sin(ang / 2)])
            q[7:] = np.array(common.DEFAULT_POSE) + rs.uniform(-0.5, 0.5, 12)
            p = O.mj_step(model, q, np.zeros(18), np.zeros(18), q[7:].copy(), nsteps=1)[3]
            k = int(p[_abi.P_NCON])
            g = p[_abi.P_CON_GEOM:_abi.P_CON_GEOM + 2 * k].reshape(k, 2).astype(int)
            # (penetrating by a clear margin, so fp32 collision on the device sees the same set)
            d = p[_abi.P_CON_DIST:_abi.P_CON_DIST + k]
            if (sorted(max(leg[a], leg[b]) for a, b in g) == sorted(want) and all(min(leg[a], leg[b]) == -1 for a, b in g)
                    and np.all(d < -1e-4)):
                qs.append(q)
                break
        else:
            raise AssertionError(f"no state with feet {want} down")
    n = len(qs)
    qpos = np.array(qs)
    return qpos, rs.normal(scale=0.3, size=(n, 18)), np.zeros((n, 18)), qpos[:, 7:] + rs.uniform(-0.3, 0.3, size=(n, 12))


ONE_FOOT = ([0], [1], [2], [3], [1], [2], [3], [0])  # each wave (envs 2w, 2w + 1): two different legs


@pytest.fixture(scope="module")
def one_foot_states(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=8, create_device=False)
    return states_with_feet_down(e.sys_model.struct, ONE_FOOT, seed=60)


def test_base_body_has_no_collision_geom(flat_path, box_path):
    for path in (flat_path, box_path):
        m = PupperV3Env(**common.fixture_kwargs(path), num_envs=2, create_device=False).sys_model.struct
        assert all(int(m.cgeom_bodyid[g]) != 1 for g in range(m.ncgeom))


@pytest.mark.parametrize("n", [2, 5])
def test_airborne(flat_path, n):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        states = common.random_physics_states(n, seed=61 + n, mode="air")
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            assert np.all(_ncon(pipe) == 0), _ncon(pipe)
        assert np.all(active_limits(e, states[0]) == 0)
    finally:
        e.close()
    _check_or_record(f"air_{n}", got)


def _step_from(env, states, seed):
    """One fused env step (the step kernel's instantiation) from the crafted qpos / qvel, the rest of
    the record as a reset leaves it."""
    n = env.num_envs
    env.reset(make_keys(seed, n))
    env.synchronize()
    rec = env._get(_abi.F_STATE).copy()
    rec[:, _abi.S_QPOS:_abi.S_QPOS + 19] = states[0]
    rec[:, _abi.S_QVEL:_abi.S_QVEL + 18] = states[1]
    env._put(_abi.F_STATE, rec)
    return _fused(env, _acts(seed + 1, 1, n), "step_")


@pytest.mark.parametrize("cap", [8, 16])
def test_one_foot_down_each_leg(flat_path, one_foot_states, cap):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=8, max_contacts=cap)
    try:
        assert e.config_struct.ncon_max == cap
        m = e.sys_model.struct
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, one_foot_states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                legs = [_contact_legs(m, pipe, i) for i in range(8)]
                print("contact legs per env:", legs)
                assert legs == [list(w) for w in ONE_FOOT], legs
                assert all(legs[2 * w] != legs[2 * w + 1] for w in range(4))
        got.update(_step_from(e, one_foot_states, 62))
    finally:
        e.close()
    _check_or_record(f"one_foot_nc{cap}", got)


def test_four_feet_down(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=4)
    try:
        m = e.sys_model.struct
        states = states_with_feet_down(m, [[0, 1, 2, 3]] * 4, seed=64)
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                assert all(_contact_legs(m, pipe, i) == [0, 1, 2, 3] for i in range(4))
    finally:
        e.close()
    _check_or_record("four_feet", got)


LIMIT_AT = ((0, 0), (1, 1), (2, 1), (3, 2), (1, 2), (2, 0))  # (leg, level) per env: two levels in every wave


def test_limit_row_at_each_level(flat_path):
    n = len(LIMIT_AT)
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        jr = e.sys_model.jnt_range
        qpos, qvel, qws, ctrl = common.random_physics_states(n, seed=65, mode="air")
        qpos[:, 7:] = common.DEFAULT_POSE
        for i, (g, lv) in enumerate(LIMIT_AT):
            d = 3 * g + lv
            lo, hi = jr[1 + d]
            qpos[i, 7 + d] = lo - 0.01 if abs(lo - qpos[i, 7 + d]) < abs(hi - qpos[i, 7 + d]) else hi + 0.01
        assert all(LIMIT_AT[2 * w][1] != LIMIT_AT[2 * w + 1][1] for w in range(n // 2))
        assert {lv for _, lv in LIMIT_AT} == {0, 1, 2}
        assert active_limits(e, qpos).tolist() == [1] * n
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, (qpos, qvel, qws, ctrl), nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                assert np.all(_ncon(pipe) == 0), _ncon(pipe)
    finally:
        e.close()
    _check_or_record("limit_levels", got)


def test_leg_leg_wave_beside_plain_wave(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=4)
    try:
        m = e.sys_model.struct
        ll = common.states_with_self_contact(m, e.sys_model.jnt_range, 1, seed=66)
        st = common.random_physics_states(3, seed=67, mode="stand")
        states = tuple(np.concatenate([a, b]) for a, b in zip(ll, st))  # ll, stand | stand, stand
        states[0][1:, 2] = 0.13
        leg = _leg_of_geom(m)
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                print("ncon per env:", _ncon(pipe).tolist())
                assert any(leg[int(a)] >= 0 and leg[int(b)] >= 0 for a, b in _con_geoms(pipe, 0))
                for i in (1, 2, 3):
                    assert len(_contact_legs(m, pipe, i)) >= 1
    finally:
        e.close()
    _check_or_record("legleg_beside_plain", got)


def test_obstacle_model(box_path):
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=4)
    try:
        assert e._L.pp3_narrow_cull(e._h) == 1
        states = common.states_on_boxes(e.sys_model.struct, 4, seed=68, z_range=(0.13, 0.15))
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                print("ncon per env:", _ncon(pipe).tolist())
                assert _ncon(pipe).min() >= 1
    finally:
        e.close()
    _check_or_record("boxes_4", got)


def test_fused_domain_randomised(flat_path):
    from pupperv3_mjx import domain_randomization as dr, rng
    n, K = 5, 2
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        sysb, _ = dr.domain_randomize(e.sys, rng.split(rng.PRNGKey(69), n))
        e.set_domain_randomization(sysb)
        e.reset(make_keys(70, n))
        got = _rollout_bits(e, _acts(71, K, n))
    finally:
        e.close()
    _check_or_record("dr_5x2", got)


def test_two_newton_iterations(require_gpu, tmp_path_factory):
    xml = open(MODEL_XML).read()
    assert xml.count('iterations="1"') == 1
    path = os.path.join(str(tmp_path_factory.mktemp("bits_ldl_iter2")), "model_iter2.xml")
    with open(path, "w") as f:
        f.write(xml.replace('iterations="1"', 'iterations="2"'))
    n, K = 6, 2
    e = PupperV3Env(**common.fixture_kwargs(path), num_envs=n, pipeline_output=True)
    try:
        assert e.sys_model.struct.iterations == 2
        e.reset(make_keys(72, n))
        got = _rollout_bits(e, _acts(73, K, n))
    finally:
        e.close()
    _check_or_record("iter2_6x2", got)


def test_policy_rollout_partial_tile(flat_path):
    from pupperv3_mjx import export
    from test_gpu_policy import _policy
    n, K = 20, 2
    assert n % 16
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    dp = export.DevicePolicy(_policy([72, 128, 128, 24], "elu"))
    try:
        st, tr = e.rollout_policy(e.reset(make_keys(74, n)), dp, K)
        got = {"state": _bits(e._get(_abi.F_STATE))}
        for k in ("obs", "reward", "done", "action"):
            got[k] = _bits(tr[k])
    finally:
        dp.close()
        e.close()
    _check_or_record("policy_20x2", got)


def test_reset_then_one_step(flat_path):
    n = 5
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, pipeline_output=True)
    ab = _lib.DeviceBuffer(n * _abi.NU * 4)
    try:
        e.reset(make_keys(75, n))
        e.synchronize()
        got = {"reset_state": _bits(e._get(_abi.F_STATE)), "reset_obs": _bits(e._get(_abi.F_OBS))}
        ab.upload(np.ascontiguousarray(_acts(76, 1, n)[0]))
        e.step_device(ab.ptr.value)
        e.synchronize()
        got.update(state=_bits(e._get(_abi.F_STATE)), obs=_bits(e._get(_abi.F_OBS)),
                   reward=_bits(e._get(_abi.F_REWARD)), done=_bits(e._get(_abi.F_DONE)),
                   pipeline=_bits(e._get(_abi.F_PIPELINE)), metrics=_bits(e._get(_abi.F_METRICS)))
    finally:
        ab.free()
        e.close()
    _check_or_record("reset_step_5", got)


def test_fused_odd_env_count_with_pipeline_record(flat_path):
    n, K = 5, 4
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, pipeline_output=True)
    try:
        e.reset(make_keys(77, n))
        got = _rollout_bits(e, _acts(78, K, n))
    finally:
        e.close()
    _check_or_record("pipeline_5x4", got)
