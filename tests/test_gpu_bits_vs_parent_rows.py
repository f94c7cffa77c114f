"""The constraint-row pass computes the parent's bits where the contact rows change lanes.

Same record-or-compare mechanism as tests/test_gpu_bits_vs_parent.py (its docstring): the fixtures
under tests/golden/bits_parent_rows/ were recorded on an MI355X with the build of the commit before
the contact rows' J . qvel moved into the warm start's row pass (row_dotk at K = 3, in Newton lane
order r = l + 32 t instead of the edge-row loop's e = l), an edit that changes which lane holds a
contact row's R, D and aref and which PairCon record it prefetches, and must leave every value,
operation order and FMA contraction as it was.  PP3_RECORD_PARENT_BITS=1 at the parent commit writes
the fixtures; otherwise the module compares.

Cases (the smallest shapes that reach what the edit moves; each asserts that it holds the rows it
claims: the number of active limit rows nl from jnt_range and the margin at the start state, the
contacts from the pipeline record of the first substep):
  physics_kernel, 8 envs standing with 1, 2 or 3 hinges past their limit, 1 and 3 substeps
      (the contact rows start at 12 + nl: another offset, and another parity, in the two halves of
      every wave)
  physics_kernel, 8 envs knees-down on the rails with one limit active, NC = 8 and NC = 16
      (nl = 1 and >= 5 contacts: contact 4's pyramid rows are 29..32, across row slots 0 and 1)
  physics_kernel, 8 envs: an airborne env (ncon = 0) in a wave with a standing one
  physics_kernel, 8 envs: a leg-leg env in a wave with a standing one   (full rows at K = 3)
  physics_kernel, 8 envs over the rails: sphere-box and plane-sphere contacts in one env
      (PairCon records that differ per pair: the prefetch keyed by the row)
  flat model with solver iterations = 2, 6 envs x 3 steps fused         (the iter > 0 row pass)
  flat model, 5 envs x 4 steps fused with the pipeline record
  flat model, 5 envs: a reset, then one step
"""
import os

import numpy as np
import pytest

import common
from pupperv3_mjx import MODEL_XML, _abi, _lib
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_bits_vs_parent import RECORD, _acts, _bits, _hip_identity
from test_gpu_bits_vs_parent_lds import _physics_bits, _rollout_bits

pytestmark = pytest.mark.gpu

DIR = os.path.join(common.GOLDEN, "bits_parent_rows")
NFR = 12  # frictionloss rows (one per hinge dof): the limit rows follow, then four rows per contact
HIP_PITCH = (1, 4, 7, 10)  # index into qpos[7:] of each leg's second hinge (0 in the default pose)


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
    return common.write_model(tmp_path_factory.mktemp("bits_rows_flat"), 0)


@pytest.fixture(scope="module")
def box_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_rows_box"), 10)


def active_limits(env, qpos):
    """Active limit rows per env at qpos, as the limit phase decides them: a limited hinge whose
    distance to one end of jnt_range is below the joint's margin (float32, as the kernel)."""
    m, jr = env.sys_model.struct, np.asarray(env.sys_model.jnt_range, dtype=np.float32)
    q = np.asarray(qpos, dtype=np.float32)[:, 7:]
    nl = np.zeros(len(q), dtype=int)
    for j in range(1, _abi.NJNT):
        if not m.jnt_limited[j]:
            continue
        margin = np.float32(m.jnt_margin[j])
        nl += (q[:, j - 1] - jr[j, 0] < margin).astype(int) + (jr[j, 1] - q[:, j - 1] < margin).astype(int)
    return nl


def past_hip_limit(env, qpos, env_i, legs, by=0.01):
    """Put the hip-pitch hinge of each leg in `legs` of env env_i `by` rad past the end of its range
    that is next to the default pose (the right legs' lower end, the left legs' upper end)."""
    jr = env.sys_model.jnt_range
    for g in legs:
        j = 1 + HIP_PITCH[g]
        lo, hi = jr[j]
        qpos[env_i, 7 + HIP_PITCH[g]] = lo - by if abs(lo) < abs(hi) else hi + by


def _ncon(pipe):
    return pipe[:, _abi.P_NCON].astype(int)


def _con_geoms(pipe, i):
    k = int(pipe[i, _abi.P_NCON])
    return pipe[i, _abi.P_CON_GEOM:_abi.P_CON_GEOM + 2 * k].reshape(k, 2).astype(int)


NL_PER_ENV = (1, 2, 2, 3, 3, 1, 1, 3)  # each wave (envs 2w, 2w + 1): two different counts


def limit_contact_states(env):
    qpos, qvel, qws, ctrl = common.random_physics_states(8, seed=31, mode="stand")
    qpos[:, 2] = 0.13
    for i, k in enumerate(NL_PER_ENV):
        past_hip_limit(env, qpos, i, range(k))
    return qpos, qvel, qws, ctrl


def test_limit_rows_with_contacts(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=8)
    try:
        states = limit_contact_states(e)
        nl = active_limits(e, states[0])
        assert nl.tolist() == list(NL_PER_ENV), nl
        assert all(nl[2 * w] != nl[2 * w + 1] for w in range(4)) and {1, 2, 3} <= set(nl.tolist())
        assert any((nl[2 * w] - nl[2 * w + 1]) % 2 for w in range(4))  # the offset's parity differs in a wave
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                print("nl per env:", nl.tolist(), "ncon per env:", _ncon(pipe).tolist())
                assert _ncon(pipe).min() >= 1, _ncon(pipe)
    finally:
        e.close()
    _check_or_record("limits_contacts", got)


def straddle_states(env):
    """test_gpu_bits_vs_parent_lds.test_row_slot_1's knees-down states on the rails, with env i's
    leg i % 4 hip past its limit: nl = 1 in every env."""
    n = 8
    m = env.sys_model.struct
    qpos, qvel, qws, ctrl = common.states_on_boxes(m, n, seed=11, z_range=(0.085, 0.10))
    qpos[:, 7:] = (np.array(common.DEFAULT_POSE) + np.tile([0, 0.0, 0.6, 0, 0.0, -0.6], 2)  # knees down
                   + np.random.RandomState(12).uniform(-0.1, 0.1, size=(n, 12)))
    for i in range(n):
        past_hip_limit(env, qpos, i, [i % 4])
    return qpos, qvel, qws, ctrl


@pytest.mark.parametrize("cap", [8, 16])
def test_contact_rows_across_row_slots(box_path, cap):
    """12 frictionloss rows + 1 limit row + 4 c: contact 4 holds rows 29..32, the first three in
    row slot 0 and the last in row slot 1."""
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=8, max_contacts=cap)
    try:
        assert e.config_struct.ncon_max == cap
        states = straddle_states(e)
        nl = active_limits(e, states[0])
        got, pipe = _physics_bits(e, states, 1, "")
        ncon = _ncon(pipe)
        print("nl per env:", nl.tolist(), "ncon per env:", ncon.tolist())
        assert np.all(nl == 1), nl
        c = 4
        assert NFR + 1 + 4 * c < 32 <= NFR + 1 + 4 * c + 3
        assert ncon.max() > c, ncon  # contact 4 exists: its rows straddle the slots
    finally:
        e.close()
    _check_or_record(f"straddle_nc{cap}", got)


def air_stand_states():
    """Every wave: an airborne env (even) next to a standing one (odd)."""
    qpos, qvel, qws, ctrl = common.random_physics_states(8, seed=33, mode="stand")
    qpos[1::2, 2] = 0.13
    qpos[0::2, 2] = 0.5
    return qpos, qvel, qws, ctrl


def test_airborne_with_standing(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=8)
    try:
        states = air_stand_states()
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                ncon = _ncon(pipe)
                print("ncon per env:", ncon.tolist())
                assert np.all(ncon[0::2] == 0) and np.all(ncon[1::2] >= 1), ncon
    finally:
        e.close()
    _check_or_record("air_stand", got)


def test_leg_leg_with_plain(flat_path):
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=8)
    try:
        m = e.sys_model.struct
        ll = common.states_with_self_contact(m, e.sys_model.jnt_range, 4, seed=34)
        st = common.random_physics_states(4, seed=35, mode="stand")
        states = tuple(np.stack([a, b], axis=1).reshape((8,) + a.shape[1:]) for a, b in zip(ll, st))  # ll, st, ll, ...
        static = {int(m.cgeom_id[g]) for g in range(m.ncgeom) if m.cgeom_bodyid[g] == 0}
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                print("ncon per env:", _ncon(pipe).tolist())
                for w in range(4):
                    assert any(a not in static and b not in static for a, b in _con_geoms(pipe, 2 * w)), w
                    g = _con_geoms(pipe, 2 * w + 1)
                    assert len(g) >= 1 and all(a in static or b in static for a, b in g), (w, g)
    finally:
        e.close()
    _check_or_record("legleg_plain", got)


def test_box_and_plane_contacts_in_one_env(box_path):
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=8)
    try:
        m = e.sys_model.struct
        kind = {int(m.cgeom_id[g]): int(m.cgeom_type[g]) for g in range(m.ncgeom)}
        states = common.states_on_boxes(m, 8, seed=36, z_range=(0.13, 0.15))
        got = {}
        for nsteps in (1, 3):
            bits, pipe = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
            if nsteps == 1:
                both = []
                for i in range(8):
                    kinds = {kind[a] for a, b in _con_geoms(pipe, i)} | {kind[b] for a, b in _con_geoms(pipe, i)}
                    both.append(_abi.GEOM_BOX in kinds and _abi.GEOM_PLANE in kinds)
                print("ncon per env:", _ncon(pipe).tolist(), "box and plane contacts:", both)
                assert sum(both) >= 2, both
    finally:
        e.close()
    _check_or_record("box_plane", got)


def test_two_newton_iterations(require_gpu, tmp_path_factory):
    xml = open(MODEL_XML).read()
    assert xml.count('iterations="1"') == 1
    path = os.path.join(str(tmp_path_factory.mktemp("bits_rows_iter2")), "model_iter2.xml")
    with open(path, "w") as f:
        f.write(xml.replace('iterations="1"', 'iterations="2"'))
    n, K = 6, 3
    e = PupperV3Env(**common.fixture_kwargs(path), num_envs=n, pipeline_output=True)
    try:
        assert e.sys_model.struct.iterations == 2
        e.reset(make_keys(37, n))
        got = _rollout_bits(e, _acts(38, K, n))
    finally:
        e.close()
    _check_or_record("iter2_6x3", got)


def test_fused_odd_env_count_with_pipeline_record(flat_path):
    n, K = 5, 4
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, pipeline_output=True)
    try:
        e.reset(make_keys(39, n))
        got = _rollout_bits(e, _acts(40, K, n))
    finally:
        e.close()
    _check_or_record("pipeline_5x4", got)


def test_reset_then_one_step(flat_path):
    n = 5
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, pipeline_output=True)
    ab = _lib.DeviceBuffer(n * _abi.NU * 4)
    try:
        e.reset(make_keys(41, n))
        e.synchronize()
        got = {"reset_state": _bits(e._get(_abi.F_STATE)), "reset_obs": _bits(e._get(_abi.F_OBS))}
        ab.upload(np.ascontiguousarray(_acts(42, 1, n)[0]))
        e.step_device(ab.ptr.value)
        e.synchronize()
        got.update(state=_bits(e._get(_abi.F_STATE)), obs=_bits(e._get(_abi.F_OBS)),
                   reward=_bits(e._get(_abi.F_REWARD)), done=_bits(e._get(_abi.F_DONE)),
                   pipeline=_bits(e._get(_abi.F_PIPELINE)), metrics=_bits(e._get(_abi.F_METRICS)))
    finally:
        ab.free()
        e.close()
    _check_or_record("reset_step_5", got)
