"""The LDS readers that tests/test_gpu_bits_vs_parent.py does not reach compute the parent's bits.

Same record-or-compare mechanism as that module (its docstring): the fixtures under
tests/golden/bits_parent_lds/ were recorded on an MI355X with the build of the commit before the
env block's fields were re-ordered for aligned 8- and 16-byte LDS reads, an edit that changes load
widths and addresses only and must leave every value, operation order and FMA contraction as it was.
PP3_RECORD_PARENT_BITS=1 at the parent commit writes the fixtures; otherwise the module compares.

Cases (the smallest shapes that reach each reader):
  physics_kernel, 8 envs with a leg-leg contact, 1 and 3 substeps     (ldl_arrow_solve_b)
  physics_kernel, 8 envs with disjoint leg pairs, 1 and 3 substeps    (dense_search's dense fallback,
                                                                       row_dotk's full-row branch)
  physics_kernel, 8 envs knees-down on the rails, NC = 8 and NC = 16  (row slot 1: nefc > 32)
  6 envs x 4 steps fused with the pipeline record                      (write_pipeline)
  6 envs x 4 steps fused, domain randomisation on
  6 envs x 4 steps fused, auto-reset with an episode length of 2
  6 envs: a reset, then one step                                       (env_reset_kernel's layout)
"""
import os

import numpy as np
import pytest

import common
import gpu_harness as G
from pupperv3_mjx import _abi, _lib, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_bits_vs_parent import RECORD, _acts, _bits, _fused, _hip_identity

pytestmark = pytest.mark.gpu

DIR = os.path.join(common.GOLDEN, "bits_parent_lds")


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
    return common.write_model(tmp_path_factory.mktemp("bits_lds_flat"), 0)


@pytest.fixture(scope="module")
def box_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_lds_box"), 10)


def _physics_bits(env, states, nsteps, tag):
    """(bits of qpos / qvel / qacc_warmstart / the pipeline record after nsteps raw substeps, the
    pipeline record itself)"""
    q, v, w, p = G.gpu_physics(env, *states, nsteps)
    return {tag + "qpos": _bits(q), tag + "qvel": _bits(v), tag + "qws": _bits(w), tag + "pipe": _bits(p)}, p


@pytest.fixture(scope="module")
def leg_leg_states(box_path):
    """(one-pair states, disjoint-pair states in test_disjoint_leg_pairs_dense_fallback's pairing
    order), 8 envs each, found once against the oracle."""
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=8, create_device=False)
    m, jr = e.sys_model.struct, e.sys_model.jnt_range
    one = common.states_with_self_contact(m, jr, 8, seed=50)
    d = common.states_with_self_contact(m, jr, 6, seed=5, kind="disjoint")
    o = common.states_with_self_contact(m, jr, 2, seed=6)
    order = [0, 1, 2, 3, 6, 4, 7, 5]  # rows 6, 7 = the one-pair states, each paired with a disjoint one
    return one, tuple(np.concatenate([x, y])[order] for x, y in zip(d, o))


@pytest.mark.parametrize("kind", ["any", "disjoint"])
def test_leg_leg_newton_paths(box_path, leg_leg_states, kind):
    states = leg_leg_states[kind == "disjoint"]
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=8)
    try:
        got = {}
        for nsteps in (1, 3):
            bits, _ = _physics_bits(e, states, nsteps, f"s{nsteps}_")
            got.update(bits)
    finally:
        e.close()
    _check_or_record("legleg_" + kind, got)


@pytest.mark.parametrize("cap", [8, 16])
def test_row_slot_1(box_path, cap):
    """More than 32 constraint rows (12 frictionloss rows + 4 per contact, from 6 contacts on):
    lanes hold a second row each."""
    n = 8
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=n, max_contacts=cap)
    try:
        m = e.sys_model.struct
        assert e.config_struct.ncon_max == cap
        qpos, qvel, qws, ctrl = common.states_on_boxes(m, n, seed=11, z_range=(0.085, 0.10))
        qpos[:, 7:] = (np.array(common.DEFAULT_POSE) + np.tile([0, 0.0, 0.6, 0, 0.0, -0.6], 2)  # knees down
                       + np.random.RandomState(12).uniform(-0.1, 0.1, size=(n, 12)))
        got, pipe = _physics_bits(e, (qpos, qvel, qws, ctrl), 1, "")
        ncon = pipe[:, _abi.P_NCON].astype(int)
        print("ncon per env:", ncon.tolist())
        assert ncon.max() >= 6, ncon  # row slot 1 is really used
    finally:
        e.close()
    _check_or_record(f"rowslot1_nc{cap}", got)


def _rollout_bits(e, acts):
    got = _fused(e, acts)
    got["pipeline"] = _bits(e._get(_abi.F_PIPELINE))
    got["metrics"] = _bits(e._get(_abi.F_METRICS))
    return got


def test_fused_with_pipeline_record(flat_path):
    n, K = 6, 4
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, pipeline_output=True)
    try:
        e.reset(make_keys(20, n))
        got = _rollout_bits(e, _acts(21, K, n))
    finally:
        e.close()
    _check_or_record("pipeline_6x4", got)


def test_fused_domain_randomised(flat_path):
    from pupperv3_mjx import domain_randomization as dr, rng
    n, K = 6, 4
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        sysb, _ = dr.domain_randomize(e.sys, rng.split(rng.PRNGKey(22), n))
        e.set_domain_randomization(sysb)
        e.reset(make_keys(23, n))
        got = _rollout_bits(e, _acts(24, K, n))
    finally:
        e.close()
    _check_or_record("dr_6x4", got)


def test_fused_auto_reset(flat_path):
    n, K = 6, 4
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        w = wrappers.wrap(e, episode_length=2)
        w.reset(make_keys(25, n))
        got = _rollout_bits(e, _acts(26, K, n))
        got["episode"] = _bits(e._get(_abi.F_EPISODE))
        assert np.any(got["done"] != 0)  # episodes of two steps: the in-kernel reset ran
    finally:
        e.close()
    _check_or_record("autoreset_6x4", got)


def test_reset_then_one_step(flat_path):
    n = 6
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    ab = _lib.DeviceBuffer(n * _abi.NU * 4)
    try:
        e.reset(make_keys(27, n))
        e.synchronize()
        got = {"reset_state": _bits(e._get(_abi.F_STATE)), "reset_obs": _bits(e._get(_abi.F_OBS))}
        ab.upload(np.ascontiguousarray(_acts(28, 1, n)[0]))
        e.step_device(ab.ptr.value)
        e.synchronize()
        got.update(state=_bits(e._get(_abi.F_STATE)), obs=_bits(e._get(_abi.F_OBS)),
                   reward=_bits(e._get(_abi.F_REWARD)), done=_bits(e._get(_abi.F_DONE)))
    finally:
        ab.free()
        e.close()
    _check_or_record("reset_step_6", got)
