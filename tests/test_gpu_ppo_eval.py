"""The PPO evaluator on the device: the pp3_eval_* kernels (csrc/pp3_ppo.hip) against the numpy f32
restatement tests/ppo_eval_ref.py bit for bit, evaluator.Evaluator end to end against a host loop
over wrap(env).step, and ppo.train against hand-chained train_iteration calls."""
import ctypes as C

import numpy as np
import pytest

import common
import ppo_eval_ref as R
from pupperv3_mjx import _abi, _lib, domain_randomization, evaluator, export, ppo, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env
from test_export import _brax_like_params

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
VP = C.c_void_p
ERR_ARG = _abi.ERR_ARG


# ------------------------------------------------------------------------------ kernels on synthetic buffers
class _Dev:
    """Host arrays uploaded once; .ptr(name) their device addresses, .get(name) downloads."""

    def __init__(self, **arrays):
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        self.bufs = {k: _lib.DeviceBuffer(v.nbytes) for k, v in self.host.items()}
        for k, v in self.host.items():
            self.bufs[k].upload(v)

    def ptr(self, name, offset_floats=0):
        return VP(self.bufs[name].ptr.value + 4 * offset_floats)

    def get(self, name):
        out = np.empty_like(self.host[name])
        self.bufs[name].download(out)
        return out

    def free(self):
        for b in self.bufs.values():
            b.free()


def _padded(rs, rows, n, stride, fill):
    """[rows][stride] with `fill(rows, n)` in the first n columns and NaN behind (reading one poisons)"""
    a = np.full((rows, stride), np.nan, F)
    a[:, :n] = fill(rows, n)
    return a


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


@pytest.mark.parametrize("nsteps", [1, 5, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_kernels_equal_the_restatement_bitwise(require_gpu, n, nsteps):
    """Three per-step accumulates, then the row chain over `nsteps` rows (step0 = 3, action_repeat 3),
    then the reduce twice: every accumulator word and all 42 outputs are the restatement's bits.
    metrics_stride 23, episode_stride 6, row_stride n + 3, the padding NaN; rewards and metrics of mixed
    sign, done with probability 0.2."""
    L = require_gpu
    rs = np.random.RandomState(1000 * n + nsteps)
    ms, es, rstride, T = 23, 6, n + 3, 3
    normal = lambda r, c: (rs.normal(size=(r, c)) * 10.0 ** rs.randint(-2, 3, size=(r, c))).astype(F)  # noqa: E731
    flags = lambda r, c: (rs.uniform(size=(r, c)) < 0.2).astype(F)  # noqa: E731
    steps = [rs.randint(1, 1000, size=n).astype(F) for _ in range(T)]
    met = [_padded(rs, n, 19, ms, normal) for _ in range(T)]
    epi = []
    for t in range(T):
        e = np.full((n, es), np.nan, F)
        e[:, _abi.EP_STEPS] = steps[t]
        epi.append(e)
    rew1, done1 = normal(T, n), flags(T, n)
    rows_r, rows_d = _padded(rs, nsteps, n, rstride, normal), _padded(rs, nsteps, n, rstride, flags)
    d = _Dev(acc=np.full((R.WORDS, n), np.nan, F), out=np.zeros(42, F), rew1=rew1, done1=done1, met=np.stack(met),
             epi=np.stack(epi), rows_r=rows_r, rows_d=rows_d)
    try:
        assert L.pp3_eval_reset(0, n, d.ptr("acc"), None) == 0, L.pp3_ppo_last_error()
        want = R.reset(n)
        np.testing.assert_array_equal(_bits(d.get("acc")), _bits(want))
        for t in range(T):
            rc = L.pp3_eval_accumulate(0, n, d.ptr("rew1", t * n), d.ptr("done1", t * n), d.ptr("met", t * n * ms), ms,
                                       d.ptr("epi", t * n * es), es, d.ptr("acc"), None)
            assert rc == 0, L.pp3_ppo_last_error()
            want = R.accumulate(want, rew1[t], done1[t], met[t], steps[t])
            np.testing.assert_array_equal(_bits(d.get("acc")), _bits(want), err_msg=f"step {t}")
        if n >= 63:  # both branches of `active` enter the row chain
            assert (want[R.ACTIVE] == 0).any() and (want[R.ACTIVE] == 1).any()
        rc = L.pp3_eval_accumulate_rows(0, nsteps, n, rstride, d.ptr("rows_r"), d.ptr("rows_d"), T, 3, d.ptr("acc"), None)
        assert rc == 0, L.pp3_ppo_last_error()
        want = R.accumulate_rows(want, rows_r[:, :n], rows_d[:, :n], T, 3)
        got = d.get("acc")
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg="row chain")
        assert np.all(np.isfinite(got))
        assert L.pp3_eval_reduce(0, n, d.ptr("acc"), d.ptr("out"), None) == 0, L.pp3_ppo_last_error()
        out1 = d.get("out")
        assert L.pp3_eval_reduce(0, n, d.ptr("acc"), d.ptr("out"), None) == 0
        out2 = d.get("out")
        np.testing.assert_array_equal(_bits(out1), _bits(out2))
        np.testing.assert_array_equal(_bits(out1), _bits(R.reduce(want)))
        np.testing.assert_array_equal(_bits(d.get("acc")), _bits(want))  # the reduce only reads
    finally:
        d.free()


def test_argument_errors_launch_nothing(require_gpu):
    L = require_gpu
    n, K = 8, 3
    sentinel = np.arange(R.WORDS * n, dtype=F).reshape(R.WORDS, n) + 0.5
    d = _Dev(acc=sentinel, out=np.full(42, -7.0, F), v=np.zeros(n, F), met=np.zeros((n, 19), F),
             epi=np.zeros((n, 4), F), rows=np.zeros((K, n), F))
    p = d.ptr
    try:
        bad = [
            L.pp3_eval_reset(0, n, None, None), L.pp3_eval_reset(0, 0, p("acc"), None),
            L.pp3_eval_accumulate(0, n, None, p("v"), p("met"), 19, p("epi"), 4, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("v"), None, p("met"), 19, p("epi"), 4, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("v"), p("v"), None, 19, p("epi"), 4, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("v"), p("v"), p("met"), 19, None, 4, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("v"), p("v"), p("met"), 19, p("epi"), 4, None, None),
            L.pp3_eval_accumulate(0, 0, p("v"), p("v"), p("met"), 19, p("epi"), 4, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("v"), p("v"), p("met"), 18, p("epi"), 4, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("v"), p("v"), p("met"), 19, p("epi"), 3, p("acc"), None),
            L.pp3_eval_accumulate(0, n, p("acc", 19 * n), p("v"), p("met"), 19, p("epi"), 4, p("acc"), None),  # reward in acc
            L.pp3_eval_accumulate(0, n, p("v"), p("v"), p("acc"), 19, p("epi"), 4, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, None, p("rows"), 0, 1, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, p("rows"), None, 0, 1, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, p("rows"), p("rows"), 0, 1, None, None),
            L.pp3_eval_accumulate_rows(0, 0, n, n, p("rows"), p("rows"), 0, 1, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, 0, n, p("rows"), p("rows"), 0, 1, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n - 1, p("rows"), p("rows"), 0, 1, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, p("rows"), p("rows"), -1, 1, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, p("rows"), p("rows"), 0, 0, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, p("rows"), p("rows"), 1 << 23, 2, p("acc"), None),
            L.pp3_eval_accumulate_rows(0, K, n, n, p("acc"), p("rows"), 0, 1, p("acc"), None),
            L.pp3_eval_reduce(0, n, None, p("out"), None), L.pp3_eval_reduce(0, n, p("acc"), None, None),
            L.pp3_eval_reduce(0, 0, p("acc"), p("out"), None),
            L.pp3_eval_reduce(0, n, p("acc"), p("acc", 5), None),
        ]
        assert bad == [ERR_ARG] * len(bad), bad
        assert b"pp3_eval_reduce" in L.pp3_ppo_last_error()
        np.testing.assert_array_equal(d.get("acc"), sentinel)
        np.testing.assert_array_equal(d.get("out"), np.full(42, -7.0, F))
    finally:
        d.free()


# ------------------------------------------------------------------------------ end to end
TERMINAL_Z = 0.129
START = domain_randomization.StartPositionRandomization(x_min=-1.0, x_max=1.0, y_min=-1.0, y_max=1.0, z_min=0.09,
                                                        z_max=0.24)
NAMES = ("total_dist",) + _abi.REWARD_NAMES
CHUNK = 3


def _nets(seed=0):
    """(deployment dict: 12 outputs, tanh of the mean; training dict: the 24-column head) of one small net"""
    p = _brax_like_params(np.random.RandomState(seed), [72, 32, 24])
    args = ("elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12), True, 2, 30.0, 30.0)
    return export.convert_params(p, *args), export.convert_training_params(p, *args)


def _envs(tmp_path, n, count, **kw):
    """Envs whose start height ranges from inside the terminal height to well above it: at
    terminal_body_z = 0.129 an env that starts low is done by its own `done` at the first step, one
    that starts high lasts until the episode length cuts it (checked on the CPU oracle for the keys
    used below, in f32 and f64, and asserted in the tests)."""
    path = common.write_model(tmp_path, 0)
    kw = {**dict(terminal_body_z=TERMINAL_Z, start_position_config=START), **kw}
    return [PupperV3Env(**common.fixture_kwargs(path, **kw), num_envs=n) for _ in range(count)]


def _download(buf, shape):
    a = np.empty(shape, F)
    buf.download(a)
    return a


def _host_loop(w, dp, sampled, key, unroll):
    """The Evaluator's unroll restated on the host: reset with split(k, N), the action of
    pp3_policy_act / pp3_policy_sample on the step's key, wrap(env).step, and the restatement on
    state.reward / done / metrics / info["steps"].  -> (accumulator, done [T][N], truncation [T][N])"""
    env = w.env
    n = env.num_envs
    _, k = rng.split(np.asarray(key, U), 2)
    st = w.reset(rng.split(k, n))
    acc = R.reset(n)
    buf = _lib.DeviceBuffer(4 * n * 12)
    dones, truncs = [], []
    try:
        K = k
        for _ in range(unroll):
            if sampled:
                cur, K = rng.split(K, 2)
                dp.sample_env(env, cur, buf.ptr.value)
            else:
                dp.act_env(env, buf.ptr.value)
            env.synchronize()
            st = w.step(st, _download(buf, (n, 12)))
            met = np.stack([np.asarray(st.metrics[name], F) for name in NAMES], axis=1)
            acc = R.accumulate(acc, np.array(st.reward), np.array(st.done), met, np.asarray(st.info["steps"], F))
            dones.append(np.array(st.done))
            truncs.append(np.array(st.info["truncation"]))
    finally:
        buf.free()
    return acc, np.stack(dones), np.stack(truncs)


def _first_done(dones, truncs):
    """per env: (wrapper step of its first done, whether the env's own done ended it)"""
    assert dones.any(axis=0).all()  # the episode length cuts whoever is left at the last step
    t = dones.argmax(axis=0)
    own = truncs[t, np.arange(dones.shape[1])] == 0
    return t, own


def _evaluate(w, dp, L, ar, sampled, key, metrics):
    ev = evaluator.Evaluator(w, dp, L, ar, key=key, deterministic=not sampled, metrics=metrics, chunk=CHUNK)
    try:
        res = ev.run_evaluation()
        return ev.accumulators(), res
    finally:
        ev.close()


@pytest.mark.parametrize("sampled", [False, True], ids=["deterministic", "sampled"])
@pytest.mark.parametrize("L, ar", [(7, 1), (8, 2)])
def test_evaluator_equals_the_host_loop_bitwise(require_gpu, tmp_path, L, ar, sampled):
    """5 envs (an odd last wave), chunk 3 (chunks 3, 3, 1 / 3, 1): the metrics path's 22 words per env
    are the host loop's; the reward path's reward, active and episode_steps are the metrics path's."""
    n, unroll, key = 5, L // ar, rng.PRNGKey(100)
    envs = _envs(tmp_path, n, 2)
    det, smp = _nets()
    dp = export.DevicePolicy(smp if sampled else det)
    try:
        ws = [wrappers.wrap(e, episode_length=L, action_repeat=ar) for e in envs]
        want, dones, truncs = _host_loop(ws[1], dp, sampled, key, unroll)
        t, own = _first_done(dones, truncs)
        # the conditions the comparison needs (not measurements): an env ended by its own done before
        # the last step and off a chunk boundary; an env that lasted until the truncation
        assert np.any(own & (t < unroll - 1) & ((t + 1) % CHUNK != 0)), (t, own)
        assert np.any(~own & (t == unroll - 1)), (t, own)
        got, res = _evaluate(ws[0], dp, L, ar, sampled, key, metrics=True)
        assert got.shape == want.shape == (22, n)
        np.testing.assert_array_equal(_bits(got), _bits(want))  # every env, every word
        np.testing.assert_array_equal(got[R.ACTIVE], np.zeros(n))
        np.testing.assert_array_equal(got[R.STEPS], (t + 1) * ar)
        assert np.any(got[:19] != 0) and len(np.unique(got[19])) == n
        fused, res_r = _evaluate(ws[0], dp, L, ar, sampled, key, metrics=False)
        for c in (19, R.ACTIVE, R.STEPS):
            np.testing.assert_array_equal(_bits(fused[c]), _bits(got[c]), err_msg=str(c))
        np.testing.assert_array_equal(fused[:19], np.zeros((19, n), F))
        assert res_r["eval/episode_reward"] == res["eval/episode_reward"]
        assert res_r["eval/avg_episode_length"] == res["eval/avg_episode_length"]
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_run_evaluation_keys_values_and_key_chain(require_gpu, tmp_path):
    n, L, key = 5, 7, rng.PRNGKey(100)
    envs = _envs(tmp_path, n, 2)
    det, _ = _nets()
    dp = export.DevicePolicy(det)
    try:
        ws = [wrappers.wrap(e, episode_length=L) for e in envs]
        want_acc, _, _ = _host_loop(ws[1], dp, False, key, L)
        want = R.reduce(want_acc)
        ev = evaluator.Evaluator(ws[0], dp, L, key=key, chunk=CHUNK)
        first = ev.run_evaluation({"training/sps": 12.0})
        names = evaluator.METRIC_NAMES
        assert names == NAMES + ("reward",)
        keys = ({f"eval/episode_{m}" for m in names} | {f"eval/episode_{m}_std" for m in names}
                | {"eval/avg_episode_length", "eval/std_episode_length", "eval/epoch_eval_time", "eval/sps",
                   "eval/walltime", "training/sps"})
        assert set(first) == keys
        for c, m in enumerate(names):
            assert first[f"eval/episode_{m}"] == float(want[c]) and first[f"eval/episode_{m}_std"] == float(want[21 + c]), m
        assert first["eval/avg_episode_length"] == float(want[20]) and first["eval/std_episode_length"] == float(want[41])
        assert first["training/sps"] == 12.0 and first["eval/epoch_eval_time"] > 0
        assert first["eval/sps"] == n * L / first["eval/epoch_eval_time"]
        # the second call advances the key: other resets, other numbers; the walltime accumulates
        second = ev.run_evaluation(aggregate_episodes=False)
        k1 = rng.split(key, 2)[0]
        want2, _, _ = _host_loop(ws[1], dp, False, k1, L)
        for c, m in enumerate(names):
            np.testing.assert_array_equal(_bits(second[f"eval/episode_{m}"]), _bits(want2[c]), err_msg=m)
            assert f"eval/episode_{m}_std" not in second
        np.testing.assert_array_equal(second["eval/episode_steps"], want2[R.STEPS])
        np.testing.assert_array_equal(second["eval/active_episodes"], want2[R.ACTIVE])
        assert second["eval/avg_episode_length"] == float(R.reduce(want2)[20])
        assert np.any(want2[19] != want_acc[19])
        assert second["eval/walltime"] == first["eval/walltime"] + second["eval/epoch_eval_time"]
        ev.close()
        # the same key in a fresh Evaluator reproduces the first; the reward path reports reward and length only
        again = evaluator.Evaluator(ws[0], dp, L, key=key, chunk=CHUNK)
        third = again.run_evaluation()
        again.close()
        timing = ("eval/epoch_eval_time", "eval/sps", "eval/walltime", "training/sps")
        assert {k: v for k, v in third.items() if k not in timing} == {k: v for k, v in first.items() if k not in timing}
        fused = evaluator.Evaluator(ws[0], dp, L, key=key, metrics=False, chunk=CHUNK)
        fourth = fused.run_evaluation()
        fused.close()
        assert set(fourth) == {"eval/episode_reward", "eval/episode_reward_std", "eval/avg_episode_length",
                               "eval/std_episode_length", "eval/epoch_eval_time", "eval/sps", "eval/walltime"}
        for k in ("eval/episode_reward", "eval/episode_reward_std", "eval/avg_episode_length", "eval/std_episode_length"):
            assert fourth[k] == first[k], k
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_evaluator_refuses_a_mismatch(require_gpu, tmp_path):
    (e,) = _envs(tmp_path, 2, 1)
    det, smp = _nets()
    dp = export.DevicePolicy(det)
    try:
        with pytest.raises(ValueError, match="wrapped"):
            evaluator.Evaluator(e, dp, 7, key=rng.PRNGKey(0))
        w = wrappers.wrap(e, episode_length=8, action_repeat=2)
        for L, ar in ((7, 2), (8, 1)):
            with pytest.raises(ValueError, match="eval env's"):
                evaluator.Evaluator(w, dp, L, ar, key=rng.PRNGKey(0))
        ev = evaluator.Evaluator(w, dp, 8, 2, key=rng.PRNGKey(0), deterministic=False)
        with pytest.raises(_lib.PupperHipError):  # a deployment policy cannot sample: an error, not a fallback
            ev.run_evaluation()
        ev.close()
    finally:
        dp.close()
        e.close()


@pytest.mark.parametrize("sampled", [False, True], ids=["deterministic", "sampled"])
def test_per_step_policy_path_max_contacts_16(require_gpu, tmp_path, sampled):
    """max_contacts = 16: pp3_rollout_policy[_sample] is per step a policy launch then a step launch;
    4 envs, 4 steps: the reward path still equals the metrics path, which equals the host loop."""
    n, L, key = 4, 4, rng.PRNGKey(100)
    envs = _envs(tmp_path, n, 2, max_contacts=16)
    det, smp = _nets()
    dp = export.DevicePolicy(smp if sampled else det)
    try:
        assert envs[0]._L.pp3_rollout_policy_fused(envs[0]._h) == 0
        ws = [wrappers.wrap(e, episode_length=L) for e in envs]
        want, _, _ = _host_loop(ws[1], dp, sampled, key, L)
        got, _ = _evaluate(ws[0], dp, L, 1, sampled, key, metrics=True)
        np.testing.assert_array_equal(_bits(got), _bits(want))
        fused, _ = _evaluate(ws[0], dp, L, 1, sampled, key, metrics=False)
        for c in (19, R.ACTIVE, R.STEPS):
            np.testing.assert_array_equal(_bits(fused[c]), _bits(got[c]), err_msg=str(c))
    finally:
        dp.close()
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ train()
def _state_bits(learner):
    return np.concatenate([learner._download(net, which) for net in (0, 1) for which in (0, 2, 3)]).view(U)


def test_train_schedule_keys_callbacks_and_evaluations(require_gpu, tmp_path):
    """6 training envs, 4 eval envs, unroll_length 3, 2 minibatches, num_evals 3, 70 timesteps: 2
    iterations per epoch, progress at 0, 36, 72 steps; the parameters are those of 4 hand-written
    train_iteration calls on the schedule's keys; every reported eval/episode_reward is a stand-alone
    Evaluator's on the parameters policy_params_fn received; learning_rate sees 0 .. 3."""
    import ppo_loss_ref as PR
    from test_gpu_ppo_learn import _dicts
    n, ne, K, L = 6, 4, 3, 5
    case = PR.random_case(3, K=K, B=n, in_dim=72, hidden=(16,), activation="elu", with_normalizer=False)
    pol, val = _dicts(case)
    envs = _envs(tmp_path, n, 2) + _envs(tmp_path, ne, 2)
    learners = [ppo.PPOLearner(pol, val, max_rows=(K + 1) * n) for _ in range(2)]
    handles = []
    try:
        wt = [wrappers.wrap(e, episode_length=L) for e in envs[:2]]
        we = [wrappers.wrap(e, episode_length=L) for e in envs[2:]]
        key = rng.PRNGKey(21)
        lr_calls, progress, received = [], [], []
        lr = lambda i: (lr_calls.append(i), 1e-3 / (1 + i))[1]  # noqa: E731
        actor, critic, metrics = ppo.train(
            learners[0], wt[0], we[0], num_timesteps=70, episode_length=L, unroll_length=K, num_minibatches=2,
            learning_rate=lr, num_evals=3, key=key, progress_fn=lambda s, m: progress.append((s, dict(m))),
            policy_params_fn=lambda s, p, ns: received.append((s, p, ns)))
        handles += [actor, critic]
        assert lr_calls == [0, 1, 2, 3] and learners[0].t == 8
        assert [s for s, _ in progress] == [0, 36, 72] == [s for s, _, _ in received]
        assert metrics == progress[-1][1] and all(ns is None for _, _, ns in received)
        assert "training/total_loss" in progress[1][1] and "training/total_loss" not in progress[0][1]
        assert all("eval/episode_tracking_lin_vel" in m and "eval/avg_episode_length" in m for _, m in progress)
        # the same iterations by hand, on the documented keys
        k_train, k_env, k_eval = rng.split(key, 3)
        a2, c2 = learners[1].make_policies()
        handles += [a2, c2]
        state = wt[1].reset(rng.split(k_env, n))
        for i in range(4):
            k_train, k_it = rng.split(k_train, 2)
            state, _, _ = learners[1].train_iteration(wt[1], state, k_it, a2, c2, K, num_minibatches=2, lr=1e-3 / (1 + i),
                                                      shuffle=True, device_rng=True)
        np.testing.assert_array_equal(_state_bits(learners[0]), _state_bits(learners[1]))
        start = np.concatenate([a.ravel() for kb in case["policy"] for a in kb])
        assert np.any(learners[0]._download(0, 0) != start)
        # each evaluation, stand-alone: the evaluator's key chain from k_eval, the parameters as received
        k = k_eval
        rewards = []
        for (_, m), (_, params, _) in zip(progress, received):
            d = dict(pol, layers=[dict(layer, weights=[kk, b]) for layer, (kk, b) in zip(pol["layers"], params["policy"])])
            dp = export.DevicePolicy(d)
            ev = evaluator.Evaluator(we[1], dp, L, key=k, deterministic=False)
            alone = ev.run_evaluation()
            ev.close(), dp.close()
            assert alone["eval/episode_reward"] == m["eval/episode_reward"]
            assert alone["eval/avg_episode_length"] == m["eval/avg_episode_length"]
            rewards.append(m["eval/episode_reward"])
            k = rng.split(k, 2)[0]
        assert len(set(rewards)) == 3
        # a deployment handle of the trained parameters: tanh of the actor's first 12 columns
        dpol = learners[0].deterministic_policy()
        handles.append(dpol)
        x = np.random.RandomState(0).normal(size=(7, 72)).astype(F)
        bufs = [_lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(4 * 7 * 12), _lib.DeviceBuffer(4 * 7 * 24)]
        bufs[0].upload(x)
        dpol.act(bufs[0].ptr.value, 72, 7, bufs[1].ptr.value, 12)
        actor.act(bufs[0].ptr.value, 72, 7, bufs[2].ptr.value, 24)
        envs[0].synchronize()
        got, logits = _download(bufs[1], (7, 12)), _download(bufs[2], (7, 24))
        for b in bufs:
            b.free()
        assert np.all(np.abs(got - np.tanh(logits[:, :12].astype(np.float64))) <= 2e-5 * (1 + np.abs(got)))
        # no evaluator: the same training, no callbacks
        with pytest.raises(ValueError, match="episode_length"):
            ppo.train(learners[1], wt[1], None, num_timesteps=18, episode_length=L + 1, unroll_length=K, key=key)
    finally:
        for h in handles:
            h.close()
        for l in learners:
            l.close()
        for e in envs:
            e.close()
