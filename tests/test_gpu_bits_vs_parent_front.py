"""The smooth-dynamics front half of the substep (kinematics, com / cinert / cdof, the RNE velocity
chain and the body forces) keeps the parent's bits.

Same record-or-compare mechanism as tests/test_gpu_bits_vs_parent.py (its docstring): the fixtures
under tests/golden/bits_parent_front/ were recorded on an MI355X with the build of the commit before
the RNE chain moved from one lane per leg to one lane per body, an edit that moves values between
lanes, LDS words and registers and must leave every value, operation order and FMA contraction as
it was.  PP3_RECORD_PARENT_BITS=1 at the parent commit writes the fixtures; otherwise the module
compares.

Cases (the smallest shapes at which a re-mapped front half can go wrong; each asserts that it holds
what it claims):
  physics_kernel, 2 and 5 airborne envs, 1 and 3 substeps: random base orientation, base linear and
      angular velocity non-zero, twelve distinct joint angles and velocities, different in the two
      halves of every wave (substep 1 has no deferred Euler step, later ones do; the odd count's
      clamped last half)
  physics_kernel, 4 standing envs with all four feet down, 3 substeps; the same states through one
      fused env step, NC = 8 and NC = 16                     (the contact Jacobians' com and gxpos)
  physics_kernel, 10-box model, 4 envs over the rails        (the CULL instantiation)
  flat model, 5 envs x 2 steps fused, domain randomisation on (per-env mass / inertia / ipos)
  observation_history = 3 with three-entry latency rows, 5 envs x 2 steps  (Caps<16, 8>)
  policy rollout, 20 envs x 2 steps                          (not a multiple of 16: partial tile)
  flat model, 5 envs: a reset, then one step                 (the reset kernel's forward pass)
  flat model, 5 envs x 4 steps fused with the pipeline record (xpos, xquat, cvel, com and the
                                                              sensors' acceleration path)
  physics_kernel, 4 envs: a leg-leg env beside a standing one (the dense path)
"""
import os

import numpy as np
import pytest

import common
from pupperv3_mjx import _abi, _lib
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_bits_vs_parent import RECORD, _acts, _bits, _hip_identity
from test_gpu_bits_vs_parent_lds import _physics_bits, _rollout_bits
from test_gpu_bits_vs_parent_ldl import _contact_legs, _leg_of_geom, _step_from, states_with_feet_down
from test_gpu_bits_vs_parent_rows import _con_geoms, _ncon

pytestmark = pytest.mark.gpu

DIR = os.path.join(common.GOLDEN, "bits_parent_front")


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
    return common.write_model(tmp_path_factory.mktemp("bits_front_flat"), 0)


@pytest.fixture(scope="module")
def box_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_front_box"), 10)


def _tumbling_states(n, seed):
    """Airborne states with a random base orientation, every base and joint velocity non-zero and
    twelve distinct joint angles and velocities per env."""
    rs = np.random.RandomState(seed)
    qpos, qvel, qws, ctrl = common.random_physics_states(n, seed=seed, mode="air")
    q = rs.normal(size=(n, 4))
    qpos[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    qvel[:, :3] = rs.uniform(0.2, 1.0, size=(n, 3)) * rs.choice([-1.0, 1.0], size=(n, 3))
    qvel[:, 3:6] = rs.uniform(0.5, 2.0, size=(n, 3)) * rs.choice([-1.0, 1.0], size=(n, 3))
    return qpos, qvel, qws, ctrl


@pytest.mark.parametrize("n", [2, 5])
def test_airborne_tumbling(flat_path, n):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        states = _tumbling_states(n, seed=80 + n)
        qpos, qvel = states[0], states[1]
        assert np.all(np.abs(qpos[:, 4:7]) > 1e-3)  # no axis-aligned orientation
        assert np.all(np.abs(qvel[:, :6]) >= 0.2)
        for i in range(n):
            assert len(set(qpos[i, 7:].tolist())) == 12 and len(set(qvel[i, 6:].tolist())) == 12
        for w in range(n // 2):  # the two halves of a wave hold different states
            assert not np.any(qpos[2 * w, 3:] == qpos[2 * w + 1, 3:]) and not np.any(qvel[2 * w] == qvel[2 * w + 1])
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            assert np.all(_ncon(pipe) == 0), _ncon(pipe)
    finally:
        e.close()
    _check_or_record(f"air_{n}", got)


@pytest.fixture(scope="module")
def standing_states(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=4, create_device=False)
    return states_with_feet_down(e.sys_model.struct, [[0, 1, 2, 3]] * 4, seed=82)


@pytest.mark.parametrize("cap", [8, 16])
def test_standing_feet_down(flat_path, standing_states, cap):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=4, max_contacts=cap)
    try:
        assert e.config_struct.ncon_max == cap
        # the fused step runs the instantiation of this cap: NC = 8 with the small caps, NC = 16 with
        # the generic ones (the two caps hold the same four contacts, so their bits agree; what differs
        # is the kernel that makes them)
        v = int(_lib.load().pp3_diag_step_variant(e._h, 1, 0))
        assert (v >> 8, v & 0xff) == ((2, 2) if cap == 8 else (16, 8)), v
        m = e.sys_model.struct
        got = {}
        _, pipe1 = _physics_bits(e, standing_states, 1, "s1_")
        assert all(_contact_legs(m, pipe1, i) == [0, 1, 2, 3] for i in range(4))
        got.update(_physics_bits(e, standing_states, 3, "s3_")[0])
        got.update(_step_from(e, standing_states, 83))
    finally:
        e.close()
    _check_or_record(f"standing_nc{cap}", got)


def test_obstacle_model(box_path):
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=4)
    try:
        assert e._L.pp3_narrow_cull(e._h) == 1
        states = common.states_on_boxes(e.sys_model.struct, 4, seed=84, z_range=(0.13, 0.15))
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
        sysb, _ = dr.domain_randomize(e.sys, rng.split(rng.PRNGKey(85), n))
        e.set_domain_randomization(sysb)
        e.reset(make_keys(86, n))
        got = _rollout_bits(e, _acts(87, K, n))
    finally:
        e.close()
    _check_or_record("dr_5x2", got)


def test_large_caps(flat_path):
    n, K = 5, 2
    e = PupperV3Env(**common.fixture_kwargs(flat_path, observation_history=3, latency_distribution=(0.2, 0.5, 0.3),
                                            imu_latency_distribution=(0.3, 0.3, 0.4)), num_envs=n)
    try:
        for fused in (0, 1):
            v = int(_lib.load().pp3_diag_step_variant(e._h, fused, 0))
            assert (v >> 8, v & 0xff) == (16, 8), (fused, v)
        e.reset(make_keys(88, n))
        got = _rollout_bits(e, _acts(89, K, n))
    finally:
        e.close()
    _check_or_record("caps16_8_5x2", got)


def test_policy_rollout_partial_tile(flat_path):
    from pupperv3_mjx import export
    from test_gpu_policy import _policy
    n, K = 20, 2
    assert n % 16
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    dp = export.DevicePolicy(_policy([72, 128, 128, 24], "elu"))
    try:
        st, tr = e.rollout_policy(e.reset(make_keys(90, n)), dp, K)
        got = {"state": _bits(e._get(_abi.F_STATE)), "metrics": _bits(e._get(_abi.F_METRICS))}
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
        e.reset(make_keys(91, n))
        e.synchronize()
        got = {"reset_state": _bits(e._get(_abi.F_STATE)), "reset_obs": _bits(e._get(_abi.F_OBS))}
        ab.upload(np.ascontiguousarray(_acts(92, 1, n)[0]))
        e.step_device(ab.ptr.value)
        e.synchronize()
        got.update(state=_bits(e._get(_abi.F_STATE)), obs=_bits(e._get(_abi.F_OBS)),
                   reward=_bits(e._get(_abi.F_REWARD)), done=_bits(e._get(_abi.F_DONE)),
                   pipeline=_bits(e._get(_abi.F_PIPELINE)), metrics=_bits(e._get(_abi.F_METRICS)))
    finally:
        ab.free()
        e.close()
    _check_or_record("reset_step_5", got)


def test_fused_with_pipeline_record(flat_path):
    n, K = 5, 4
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, pipeline_output=True)
    try:
        e.reset(make_keys(93, n))
        got = _rollout_bits(e, _acts(94, K, n))
    finally:
        e.close()
    _check_or_record("pipeline_5x4", got)


def test_leg_leg_env_beside_standing(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=4)
    try:
        m = e.sys_model.struct
        ll = common.states_with_self_contact(m, e.sys_model.jnt_range, 1, seed=95)
        st = common.random_physics_states(3, seed=96, mode="stand")
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
    _check_or_record("legleg_beside_standing", got)
