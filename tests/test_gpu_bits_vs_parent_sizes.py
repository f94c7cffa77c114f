"""The step kernels compiled for the model's history and lag sizes compute the parent's bits.

Same record-or-compare mechanism as tests/test_gpu_bits_vs_parent.py (its docstring): the fixtures
under tests/golden/bits_parent_sizes/ were recorded on an MI355X with the build of the commit before
env_step_kernel took its observation-history and latency-row extents from a size trait (Caps<2, 2>
when observation_history, len(latency_distribution) and len(imu_latency_distribution) are all <= 2
and the contact cap is 8; Caps<16, 8>, the code as it was, otherwise).  The edit changes array
extents, trip counts and guards only and must leave every value, operation order and FMA contraction
as it was.  PP3_RECORD_PARENT_BITS=1 at the parent commit writes the fixtures; otherwise the module
compares, and asserts through pp3_diag_step_variant which instantiation each case launches.

Cases (6 envs x 4 steps unless noted; state record, obs, reward, done, metrics and the trajectory
rows, fused and as single-step launches):
  H = 2, La = Li = 2                                  small caps
  the same with 5 envs                                small caps, the odd last wave (own == false lanes)
  La = 1, Li = 2 and La = 2, Li = 1                   small caps, guards inside the cap
  H = 3                                               generic: the shifted window overlaps its source
  H = 15                                              generic
  La = Li = 8                                         generic, at the lag cap
  La = 3, and Li = 3                                  generic, just past the small cap
  H = 1                                               small caps, nothing to move
  max_contacts = 16                                   generic (the small caps are built for NC = 8 only)
  auto-reset with episodes of 2 steps, action_repeat 1 and 2; domain randomisation; 10 boxes (CULL);
  resample_velocity_step = 2 (the resample branch)    small caps
  policy rollout and sampled policy rollout, 16 envs x 3 steps        (NWV = 8, observation tile)
  physics_kernel on 8 envs over the boxes, knees-down envs (more than 32 constraint rows) sharing
  their waves with standing envs, and the same envs re-paired so that no wave mixes, 1 and 3 substeps

Without fixtures (3 envs x 2 steps, the fused launch against the per-step path): the instantiations
that the cases above leave out -- the cull with the generic caps at contact cap 8 and 16, fused and
single-step, and the policy rollouts with the generic caps (flat; with the cull; sampled with the cull).
"""
import os

import numpy as np
import pytest

import common
import gpu_harness as G
from pupperv3_mjx import _abi, _lib, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_bits_vs_parent import RECORD, _acts, _bits, _fused, _hip_identity, _over_rails, _single

pytestmark = pytest.mark.gpu

DIR = os.path.join(common.GOLDEN, "bits_parent_sizes")
SMALL, GENERIC = (2, 2), (16, 8)


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


def _assert_variant(e, want, policy=False):
    """Every launch kind of env e takes the instantiation with caps `want` = (history, lag).  (The
    parent's library has no such query: nothing to assert while recording.)"""
    if RECORD:
        return
    L = _lib.load()
    for fused in (0, 1):
        v = int(L.pp3_diag_step_variant(e._h, fused, int(policy)))
        assert (v >> 8, v & 0xff) == want, (fused, policy, v, want)


def _buffers(e, tag=""):
    return {tag + k: _bits(e._get(f)) for k, f in (("buf_obs", _abi.F_OBS), ("buf_reward", _abi.F_REWARD),
                                                   ("buf_done", _abi.F_DONE), ("metrics", _abi.F_METRICS))}


@pytest.fixture(scope="module")
def flat_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_sizes_flat"), 0)


@pytest.fixture(scope="module")
def box_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_sizes_box"), 10)


def _both_kernels(path, case, variant, n=6, K=4, seed=40, setup=None, episode=False, **over):
    """K steps of n envs as one fused launch and as single-step launches (action_repeat > 1: both
    are per-step launches), which must agree with each other and with the parent."""
    acts = _acts(seed + 1, K, n)
    got = {}
    for mode in ("fused", "single"):
        e = PupperV3Env(**common.fixture_kwargs(path, **over), num_envs=n)
        try:
            _assert_variant(e, variant)
            st = e.reset(make_keys(seed, n))
            if setup is not None:
                setup(e, st)
            got.update(_fused(e, acts, "fused_") if mode == "fused" else _single(e, acts, "single_"))
            got.update(_buffers(e, mode + "_"))
            if episode:
                got[mode + "_episode"] = _bits(e._get(_abi.F_EPISODE))
        finally:
            e.close()
    if case is not None:  # (None: no fixture, the two launch kinds against each other only)
        _check_or_record(case, got)
    for k in ("state", "obs", "reward", "done", "buf_obs", "buf_reward", "buf_done", "metrics"):
        np.testing.assert_array_equal(got["fused_" + k], got["single_" + k], err_msg=k)
    return got


LAG8 = tuple(float(v) for v in np.arange(1, 9) / 36.0)


@pytest.mark.parametrize("case,variant,n,over", [
    ("h2_la2_li2", SMALL, 6, {}),
    ("h2_la2_li2_5envs", SMALL, 5, {}),
    ("h2_la1_li2", SMALL, 6, dict(latency_distribution=(1.0,))),
    ("h2_la2_li1", SMALL, 6, dict(imu_latency_distribution=(1.0,))),
    ("h1", SMALL, 6, dict(observation_history=1)),
    ("h3", GENERIC, 6, dict(observation_history=3)),
    ("h15", GENERIC, 6, dict(observation_history=15)),
    ("h2_la8_li8", GENERIC, 6, dict(latency_distribution=LAG8, imu_latency_distribution=LAG8[::-1])),
    ("h2_la3", GENERIC, 6, dict(latency_distribution=(0.2, 0.5, 0.3))),
    ("h2_li3", GENERIC, 6, dict(imu_latency_distribution=(0.3, 0.3, 0.4))),
    ("resample2", SMALL, 6, dict(resample_velocity_step=2)),
])
def test_sizes(flat_path, case, variant, n, over):
    got = _both_kernels(flat_path, case, variant, n=n, **over)
    if case == "resample2":  # the command was resampled: the step counter went back to 0
        assert np.all(got["fused_state"][:, _abi.S_STEP].view(np.float32) <= 2.0)


def test_ncon_max_16_is_generic(flat_path):
    _both_kernels(flat_path, "nc16", GENERIC, max_contacts=16)


@pytest.mark.parametrize("repeat", [1, 2])
def test_small_caps_auto_reset(flat_path, repeat):
    def setup(e, st):
        w = wrappers.wrap(e, episode_length=2, action_repeat=repeat)
        w.reset(make_keys(42, e.num_envs))

    got = _both_kernels(flat_path, f"autoreset_ep2_repeat{repeat}", SMALL, setup=setup, episode=True)
    assert np.any(got["fused_done"] != 0)  # episodes of two steps: the in-kernel reset ran


def test_small_caps_domain_randomised(flat_path):
    from pupperv3_mjx import domain_randomization as dr, rng

    def setup(e, st):
        sysb, _ = dr.domain_randomize(e.sys, rng.split(rng.PRNGKey(43), e.num_envs))
        e.set_domain_randomization(sysb)
        e.reset(make_keys(44, e.num_envs))

    _both_kernels(flat_path, "dr", SMALL, setup=setup)


def test_small_caps_boxes(box_path):
    def setup(e, st):
        assert e._L.pp3_narrow_cull(e._h) == 1
        _over_rails(e, st, seed=45)

    _both_kernels(box_path, "boxes", SMALL, setup=setup)


@pytest.mark.parametrize("sample", [False, True])
def test_policy_rollouts(flat_path, sample):
    from pupperv3_mjx import export, rng
    from test_gpu_policy import _policy
    from test_gpu_policy_sample import _training
    n, K = 16, 3
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    dp = export.DevicePolicy(_training([72, 64, 24]) if sample else _policy([72, 128, 128, 24], "elu"))
    try:
        assert e._L.pp3_rollout_policy_fused(e._h) == 1
        _assert_variant(e, SMALL, policy=True)
        st = e.reset(make_keys(46, n))
        if sample:
            st, tr, key = e.rollout_policy_sample(st, dp, K, rng.PRNGKey(47))
        else:
            st, tr = e.rollout_policy(st, dp, K)
        got = {"state": _bits(e._get(_abi.F_STATE))}
        got.update(_buffers(e))
        for k in sorted(tr):
            got[k] = _bits(tr[k])
        if sample:
            got["key"] = np.asarray(key, dtype=np.uint32).copy()
    finally:
        dp.close()
        e.close()
    _check_or_record("policy_sample_16x3" if sample else "policy_16x3", got)


@pytest.mark.parametrize("over", [dict(observation_history=3), dict(max_contacts=16)], ids=["h3", "nc16"])
def test_cull_generic_fused_equals_single(box_path, over):
    """The CULL instantiations with the generic caps, contact cap 8 and 16, which no case above
    launches: 3 envs (the padded half wave runs) x 2 steps over the rails, one fused launch against
    single-step launches."""
    def setup(e, st):
        assert e._L.pp3_narrow_cull(e._h) == 1
        _over_rails(e, st, seed=48)

    _both_kernels(box_path, None, GENERIC, n=3, K=2, seed=49, setup=setup, **over)


@pytest.mark.parametrize("boxes,sample", [(False, False), (True, False), (True, True)])
def test_policy_rollouts_generic_equal_per_step(flat_path, box_path, boxes, sample):
    """The fused policy rollouts with the generic caps (observation_history 3: the MLP reads the
    observations from global memory), flat and with the cull, deterministic and sampled: 3 envs x 2
    steps, bit-equal to the per-step path (the stand-alone policy kernel, then a step)."""
    from pupperv3_mjx import export, rng
    from test_gpu_policy import _policy
    from test_gpu_policy_sample import _assert_same, _loop_reference, _training
    n, K = 3, 2
    envs = [PupperV3Env(**common.fixture_kwargs(box_path if boxes else flat_path, observation_history=3), num_envs=n)
            for _ in range(2)]
    dp = export.DevicePolicy(_training([108, 64, 24]) if sample else _policy([108, 64, 24], "elu"))
    ab = _lib.DeviceBuffer(n * 12 * 4)
    try:
        for e in envs:
            assert e._L.pp3_rollout_policy_fused(e._h) == 1 and e._L.pp3_narrow_cull(e._h) == int(boxes)
            _assert_variant(e, GENERIC, policy=True)
        s1, s2 = envs[0].reset(make_keys(50, n)), envs[1].reset(make_keys(50, n))
        if sample:
            key = rng.PRNGKey(51)
            s1, tr, k1 = envs[0].rollout_policy_sample(s1, dp, K, key)
            s2, ref, k2 = _loop_reference(envs[1], envs[1], s2, dp, K, key)
            _assert_same(tr, ref)
            np.testing.assert_array_equal(k1, k2)
        else:
            s1, tr = envs[0].rollout_policy(s1, dp, K)
            for t in range(K):
                dp.act_env(envs[1], ab.ptr.value)
                envs[1].synchronize()
                a = np.zeros((n, 12), dtype=np.float32)
                ab.download(a)
                s2 = envs[1].step(s2, a)
                np.testing.assert_array_equal(tr["action"][t], a)
                for k in ("obs", "reward", "done"):
                    np.testing.assert_array_equal(tr[k][t], getattr(s2, k), err_msg=k)
        np.testing.assert_array_equal(s1._record, s2._record)
    finally:
        ab.free()
        dp.close()
        for e in envs:
            e.close()


def _physics(e, states, tag):
    got = {}
    for nsteps in (1, 3):
        q, v, w, p = G.gpu_physics(e, *states, nsteps)
        t = f"{tag}s{nsteps}_"
        got.update({t + "qpos": _bits(q), t + "qvel": _bits(v), t + "qws": _bits(w), t + "pipe": _bits(p)})
    return got


def test_row_slots_mixed_and_unmixed_waves(box_path):
    """Envs with more than 32 constraint rows (12 frictionloss rows + 4 per contact: 6 contacts and
    up, the knees-down states of test_gpu_bits_vs_parent_lds.test_row_slot_1) next to envs with at
    most 32: paired k s k s k s k s every wave holds one of each; as k k k k s s s s no wave mixes."""
    n = 8
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=n)
    try:
        _assert_variant(e, SMALL)
        m = e.sys_model.struct
        knees = list(common.states_on_boxes(m, n, seed=11, z_range=(0.085, 0.10)))
        knees[0][:, 7:] = (np.array(common.DEFAULT_POSE) + np.tile([0, 0.0, 0.6, 0, 0.0, -0.6], 2)
                           + np.random.RandomState(12).uniform(-0.1, 0.1, size=(n, 12)))
        stand = common.states_on_boxes(m, n, seed=13)
        # which envs are which, by the contact count of their first substep
        nk = G.gpu_physics(e, *knees, 1)[3][:, _abi.P_NCON].astype(int)
        ns = G.gpu_physics(e, *stand, 1)[3][:, _abi.P_NCON].astype(int)
        print("ncon knees-down:", nk.tolist(), "standing:", ns.tolist())
        heavy, light = np.flatnonzero(nk >= 6), np.flatnonzero(ns <= 5)
        assert heavy.size >= 1 and light.size >= 1, (nk, ns)
        hi, lo = np.resize(heavy, 4), np.resize(light, 4)
        mixed = tuple(np.stack([x for i, j in zip(hi, lo) for x in (k[i], s[j])]) for k, s in zip(knees, stand))
        apart = tuple(np.concatenate([k[hi], s[lo]]) for k, s in zip(knees, stand))
        got = {"heavy": hi.astype(np.uint32), "light": lo.astype(np.uint32)}
        got.update(_physics(e, mixed, "mixed_"))
        got.update(_physics(e, apart, "apart_"))
        # an env's result does not depend on the env it shares its wave with
        order = [0, 2, 4, 6, 1, 3, 5, 7]
        for k in ("s1_qpos", "s1_qvel", "s1_qws", "s3_qpos", "s3_qvel", "s3_qws"):
            np.testing.assert_array_equal(got["mixed_" + k][order], got["apart_" + k], err_msg=k)
    finally:
        e.close()
    _check_or_record("rowslots_8", got)
