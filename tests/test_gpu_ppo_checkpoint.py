"""Checkpoints on the device: the env's and the learner's state_dict / load_state_dict round trips
into fresh objects, bit for bit, and ppo.train(checkpoint_path=, restore=): a run resumed from the
file written at its first epoch boundary ends with the bits of the uninterrupted run."""
import os

import numpy as np
import pytest

from pupperv3_mjx import _abi, ppo, rng, wrappers
from test_gpu_ppo_eval import _envs

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
D = 72
ENV_FIELDS = (_abi.F_STATE, _abi.F_OBS, _abi.F_REWARD, _abi.F_DONE, _abi.F_METRICS, _abi.F_EPISODE,
              _abi.F_FIRST_STATE, _abi.F_FIRST_OBS)
TIMING = ("eval/epoch_eval_time", "eval/sps", "eval/walltime", "training/sps", "training/walltime")


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _fields(env):
    return {f: env._get(f).view(U).copy() for f in ENV_FIELDS}


def _assert_same_arrays(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        g, v = np.asarray(got[k]), np.asarray(v)
        assert g.dtype == v.dtype and g.shape == v.shape, k
        assert g.tobytes() == v.tobytes(), k


def _steps(w, state, actions):
    """-> (state, per step (obs bits, reward bits, done bits, truncation))"""
    out = []
    for a in actions:
        state = w.step(state, a)
        out.append((_bits(state.obs).copy(), _bits(state.reward).copy(), _bits(state.done).copy(),
                    np.array(state.info["truncation"])))
    return state, out


# ------------------------------------------------------------------------------ the env
@pytest.mark.parametrize("ar", [1, 2])
def test_env_round_trip_into_a_fresh_env_is_bit_equal(require_gpu, tmp_path, ar):
    """6 envs, episode_length 5: 4 wrapper steps, state_dict, 3 more; a fresh env loaded with the dict
    takes the same 3 steps to the same bits.  Inside those 3 steps an episode is cut by its length and
    one ends by the env's own done, so the restored done flags (the auto-reset's steps := 0), episode
    record and first state are all read."""
    n, L = 6, 5
    # _envs' start heights (0.09 .. 0.24) around a terminal height of 0.15: with action_repeat 2 the done
    # flag follows the last repeat, by which a robot started below _envs' own 0.129 has been pushed
    # back above it, so the own-done envs the assertions below need would be missing there
    envs = _envs(tmp_path, n, 2, terminal_body_z=0.15)
    try:
        wa, wb = (wrappers.wrap(e, episode_length=L, action_repeat=ar) for e in envs)
        acts = np.random.RandomState(ar).uniform(-0.3, 0.3, size=(7, n, 12)).astype(F)
        # (the keys of test_gpu_ppo_eval's evaluations, whose envs are known to start on both sides of the
        # terminal height)
        st = wa.reset(rng.split(rng.split(rng.PRNGKey(100), 2)[1], n))
        st, _ = _steps(wa, st, acts[:4])
        sd = wa.state_dict()
        assert int(sd["layout_num_envs"]) == n and int(sd["layout_episode_length"]) == L
        assert int(sd["layout_action_repeat"]) == ar and sd[f"field_{_abi.F_STATE}"].dtype == U
        at4 = (_bits(st.obs).copy(), _bits(st.reward).copy(), _bits(st.done).copy())
        first_obs = np.array(st.info["first_obs"])
        st, want = _steps(wa, st, acts[4:])
        done = np.stack([d.view(F) for _, _, d, _ in want])
        trunc = np.stack([t for _, _, _, t in want])
        assert np.any((done == 1) & (trunc == 1)), "no episode was cut by its length in the 3 steps"
        assert np.any((done == 1) & (trunc == 0)), "no episode ended by the env's own done in the 3 steps"
        assert np.any(done == 0)
        # the fresh env: never reset, loaded, stepped
        sb = wb.load_state_dict(sd)
        assert envs[1].holds(sb)
        for got, w in zip((_bits(sb.obs), _bits(sb.reward), _bits(sb.done)), at4):
            np.testing.assert_array_equal(got, w)
        np.testing.assert_array_equal(_bits(sb.info["first_obs"]), _bits(first_obs))
        _assert_same_arrays({k: v for k, v in wb.state_dict().items()}, sd)
        sb, got = _steps(wb, sb, acts[4:])
        for t, (g, w) in enumerate(zip(got, want)):
            for name, a, b in zip(("obs", "reward", "done", "truncation"), g, w):
                np.testing.assert_array_equal(a, b, err_msg=f"step {4 + t} {name}")
        fa, fb = _fields(envs[0]), _fields(envs[1])
        for f in ENV_FIELDS:
            np.testing.assert_array_equal(fb[f], fa[f], err_msg=f"field {f}")
        assert np.any(fa[_abi.F_STATE] != sd[f"field_{_abi.F_STATE}"])  # (the comparison can fail)
    finally:
        for e in envs:
            e.close()


def test_env_refuses_a_dict_of_another_layout_and_uploads_nothing(require_gpu, tmp_path):
    n, L = 6, 5
    envs = _envs(tmp_path, n, 2) + _envs(tmp_path, n - 1, 1)
    try:
        w = wrappers.wrap(envs[0], episode_length=L)
        w.reset(rng.split(rng.PRNGKey(1), n))
        before = _fields(envs[0])
        longer = wrappers.wrap(envs[1], episode_length=L + 2)
        longer.reset(rng.split(rng.PRNGKey(2), n))
        fewer = wrappers.wrap(envs[2], episode_length=L)
        fewer.reset(rng.split(rng.PRNGKey(3), n - 1))
        good = w.state_dict()
        missing = {k: v for k, v in good.items() if k != f"field_{_abi.F_DONE}"}
        for bad, what in ((longer.state_dict(), "episode_length"), (fewer.state_dict(), "num_envs"),
                          (envs[1].state_dict(), "episode_length"), (missing, "field")):
            with pytest.raises(ValueError, match=what):
                w.load_state_dict(bad)
        with pytest.raises(ValueError, match="episode_length"):  # a wrapper's dict into the bare env
            envs[0].load_state_dict(good)
        after = _fields(envs[0])
        for f in ENV_FIELDS:
            np.testing.assert_array_equal(after[f], before[f], err_msg=f"field {f}")
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ the learner
def _iteration(learner, w, state, key, actor, critic, K):
    return learner.train_iteration(w, state, key, actor, critic, K, num_minibatches=2, lr=1e-3, shuffle=True,
                                   max_grad_norm=1.0, update_normalizer=True, device_rng=True)


def test_learner_round_trip_into_a_fresh_learner_is_bit_equal(require_gpu, tmp_path):
    """3 iterations (running statistics, shuffle, clip, device draws), state_dict; a fresh learner of
    the same shapes (other parameters) loads it, a fresh env the env's; one further iteration on each
    leaves params, m, v, the normaliser rows, the count and t bit-equal."""
    n, K = 6, 3
    envs = _envs(tmp_path, n, 2)
    shapes = dict(policy_hidden_layer_sizes=(16,), value_hidden_layer_sizes=(12,), max_rows=(K + 1) * n)
    la = ppo.make_learner(rng.PRNGKey(1), D, **shapes)
    lb = ppo.make_learner(rng.PRNGKey(2), D, **shapes)
    lc = ppo.make_learner(rng.PRNGKey(3), D, **dict(shapes, policy_hidden_layer_sizes=(8,)))
    handles = []
    try:
        wa, wb = (wrappers.wrap(e, episode_length=5) for e in envs)
        handles += la.make_policies()
        state = wa.reset(rng.split(rng.PRNGKey(100), n))
        key = rng.PRNGKey(17)
        for _ in range(3):
            key, k_it = rng.split(key, 2)
            state, _, _ = _iteration(la, wa, state, k_it, handles[0], handles[1], K)
        sd, env_sd = la.state_dict(), wa.state_dict()
        assert int(sd["t"]) == 6 and int(sd["count"]) == 3 * K * n and sd["normalizer"].shape == (3, D)
        assert sd["policy_m"].any() and sd["value_v"].any()
        # a dict of another width is refused, and the refusing learner keeps its own state
        own = lc.state_dict()
        with pytest.raises(ValueError, match="policy_widths"):
            lc.load_state_dict(sd)
        with pytest.raises(ValueError, match="policy_params"):
            lc.load_state_dict(dict(own, policy_params=own["policy_params"][:-1]))
        _assert_same_arrays(lc.state_dict(), own)
        lb.load_state_dict(sd)
        _assert_same_arrays(lb.state_dict(), sd)
        handles += lb.make_policies()
        state_b = wb.load_state_dict(env_sd)
        key, k_it = rng.split(key, 2)
        _, ma, _ = _iteration(la, wa, state, k_it, handles[0], handles[1], K)
        _, mb, _ = _iteration(lb, wb, state_b, k_it, handles[2], handles[3], K)
        assert ma == mb and all(np.isfinite(v) for v in ma.values())
        end_a, end_b = la.state_dict(), lb.state_dict()
        _assert_same_arrays(end_b, end_a)
        assert int(end_a["t"]) == 8 and np.any(end_a["policy_params"] != sd["policy_params"])
        assert np.any(end_a["normalizer"] != sd["normalizer"])
        _assert_same_arrays(wb.state_dict(), wa.state_dict())
    finally:
        for h in handles:
            h.close()
        for l in (la, lb, lc):
            l.close()
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ train()
def test_train_resumed_from_a_checkpoint_ends_with_the_uninterrupted_bits(require_gpu, tmp_path):
    """6 training envs, 4 eval envs, unroll_length 3, episode_length 5, 2 minibatches, num_evals 3, 70
    timesteps (2 iterations per epoch; evaluations and checkpoints at 0, 36, 72 steps), a callable
    learning rate, the running normaliser and the clip.  Run B, on fresh objects, restores the file
    run A wrote at 36 steps."""
    n, ne, K, L = 6, 4, 3, 5
    envs = _envs(tmp_path, n, 2) + _envs(tmp_path, ne, 2)
    shapes = dict(policy_hidden_layer_sizes=(16,), value_hidden_layer_sizes=(16,), max_rows=(K + 1) * n)
    la = ppo.make_learner(rng.PRNGKey(1), D, **shapes)
    lb = ppo.make_learner(rng.PRNGKey(2), D, **shapes)
    handles = []
    try:
        wt = [wrappers.wrap(e, episode_length=L) for e in envs[:2]]
        we = [wrappers.wrap(e, episode_length=L) for e in envs[2:]]
        key = rng.PRNGKey(21)
        path = lambda s: os.path.join(str(tmp_path), f"ck_{s}.npz")  # noqa: E731

        def run(learner, w, e, **kw):
            lr_calls, progress, order = [], [], []
            lr = lambda i: (lr_calls.append(i), 1e-3 / (1 + i))[1]  # noqa: E731
            args = dict(num_timesteps=70, episode_length=L, unroll_length=K, num_minibatches=2, learning_rate=lr,
                        num_evals=3, key=key, normalize_observations=True, max_grad_norm=1.0,
                        progress_fn=lambda s, m: (progress.append((s, dict(m))), order.append(("progress", s))),
                        policy_params_fn=lambda s, p, ns: order.append(("params", s, os.path.exists(path(s)))))
            actor, critic, metrics = ppo.train(learner, w, e, **{**args, **kw})
            handles.extend([actor, critic])
            return lr_calls, progress, order, metrics

        lr_a, prog_a, order_a, metrics_a = run(la, wt[0], we[0], checkpoint_path=path)
        assert lr_a == [0, 1, 2, 3] and [s for s, _ in prog_a] == [0, 36, 72]
        assert sorted(os.listdir(tmp_path)) == ["ck_0.npz", "ck_36.npz", "ck_72.npz", "model_0.xml"]
        # progress_fn, policy_params_fn, then the checkpoint: the file did not exist at the callbacks
        assert order_a == [x for s in (0, 36, 72) for x in (("progress", s), ("params", s, False))]
        ck = ppo.load_checkpoint(path(36))
        assert set(ck) == {"learner", "env", "evaluator", "loop"}
        assert int(ck["loop"]["iteration"]) == 2 and int(ck["loop"]["epoch"]) == 1 and int(ck["learner"]["t"]) == 4
        k_train = rng.split(key, 3)[0]
        for _ in range(2):
            k_train = rng.split(k_train, 2)[0]
        np.testing.assert_array_equal(ck["loop"]["k_train"], k_train)
        np.testing.assert_array_equal(ck["evaluator"]["key"], rng.split(rng.split(rng.split(key, 3)[2], 2)[0], 2)[0])
        end_a, env_a = la.state_dict(), wt[0].state_dict()
        assert np.any(end_a["policy_params"] != ck["learner"]["policy_params"])  # (the comparison can fail)
        assert np.any(env_a[f"field_{_abi.F_STATE}"] != ck["env"][f"field_{_abi.F_STATE}"])
        # the last file holds the state the run ended with
        last = ppo.load_checkpoint(path(72))
        _assert_same_arrays(last["learner"], end_a)
        _assert_same_arrays(last["env"], env_a)
        # another schedule is refused before anything is loaded
        own, own_env = lb.state_dict(), _fields(envs[1])
        for change in (dict(num_minibatches=3), dict(num_timesteps=200)):
            with pytest.raises(ValueError, match="schedule"):
                run(lb, wt[1], we[1], restore=path(36), **change)
        _assert_same_arrays(lb.state_dict(), own)
        for f, v in _fields(envs[1]).items():
            np.testing.assert_array_equal(v, own_env[f], err_msg=f"field {f}")
        # run B
        lr_b, prog_b, _, metrics_b = run(lb, wt[1], we[1], restore=path(36))
        assert lr_b == [2, 3]
        assert [s for s, _ in prog_b] == [72]
        assert set(metrics_b) == set(metrics_a) and set(TIMING) <= set(metrics_a)
        for k in metrics_a:
            if k not in TIMING:
                assert metrics_b[k] == metrics_a[k] and np.isfinite(metrics_a[k]), k
        assert metrics_b["training/walltime"] > float(ck["loop"]["walltime"])  # (the saved walltime continues)
        _assert_same_arrays(lb.state_dict(), end_a)
        _assert_same_arrays(wt[1].state_dict(), env_a)
        fa, fb = _fields(envs[0]), _fields(envs[1])
        for f in ENV_FIELDS:
            np.testing.assert_array_equal(fb[f], fa[f], err_msg=f"field {f}")
    finally:
        for h in handles:
            h.close()
        for l in (la, lb):
            l.close()
        for e in envs:
            e.close()
