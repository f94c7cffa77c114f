"""PPO metrics on the device: the pp3_episode_stats_*, pp3_sum_gathered_f32, pp3_eval_column_sums and
pp3_eval_finish kernels (csrc/pp3_ppo.hip) against the numpy f32 restatement tests/ppo_metrics_ref.py
bit for bit; ppo.EpisodeStats behind train_iteration against a host loop over wrap(env).step;
collect_ppo(host_batch=False); ppo.train(log_training_metrics=True)."""
import ctypes as C
import os

import numpy as np
import pytest

import ppo_eval_ref as R
import ppo_metrics_ref as M
from pupperv3_mjx import _abi, _lib, ppo, rng, wrappers
from test_gpu_ppo_eval import _Dev, _bits, _download, _envs, _padded

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
ERR_ARG = _abi.ERR_ARG


# ------------------------------------------------------------------------------ kernels on synthetic buffers
def _ok(L, rc):
    assert rc == 0, L.pp3_ppo_last_error()


@pytest.mark.parametrize("nsteps", [1, 5, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_episode_stats_equal_the_restatement_bitwise(require_gpu, n, nsteps):
    """begin from an episode field of stride 6 (NaN in the words not read), then the row chain with
    row_stride n + 3 (NaN padding), action_repeat 3, done with probability 0.3, rewards of mixed sign
    and scale, a non-zero carry with pd = 1 on some envs; truncation given and NULL; each twice."""
    L = require_gpu
    rs = np.random.RandomState(1000 * n + nsteps)
    es, stride, ar = 6, n + 3, 3
    normal = lambda r, c: (rs.normal(size=(r, c)) * 10.0 ** rs.randint(-2, 3, size=(r, c))).astype(F)  # noqa: E731
    flags = lambda r, c: (rs.uniform(size=(r, c)) < 0.3).astype(F)  # noqa: E731
    epi = np.full((n, es), np.nan, F)
    epi[:, _abi.EP_SUM_REWARD] = normal(1, n)[0]
    epi[:, _abi.EP_LENGTH] = rs.randint(0, 40, size=n) * float(ar)
    pd0 = flags(1, n)[0]
    if n >= 63:
        assert (pd0 == 1).any() and (pd0 == 0).any()
    rew, done = _padded(rs, nsteps, n, stride, normal), _padded(rs, nsteps, n, stride, flags)
    trunc = _padded(rs, nsteps, n, stride, lambda r, c: done[:r, :c] * (rs.uniform(size=(r, c)) < 0.5))
    dn = done[:, :n]
    if n >= 63:  # a done on the last row; with more than one row consecutive dones and two episodes in one call
        assert dn[-1].any()
        assert nsteps == 1 or ((dn[1:] * dn[:-1]).any() and (dn.sum(0) >= 2).any())
    d = _Dev(epi=epi, pd=pd0, rew=rew, done=done, trunc=trunc, carry=np.full((3, n), np.nan, F),
             part=np.full((4, n), np.nan, F), out=np.full(4, np.nan, F))
    p = d.ptr
    try:
        seeded = M.episode_begin(epi, pd0, _abi.EP_SUM_REWARD, _abi.EP_LENGTH)
        for tr_name in ("trunc", None):
            want_carry, want_part = M.episode_rows(seeded, rew[:, :n], dn, None if tr_name is None else trunc[:, :n], ar)
            want_out = M.episode_out4(want_part)
            got = []
            for _ in range(2):
                _ok(L, L.pp3_episode_stats_begin(0, n, p("epi"), es, p("pd"), p("carry"), None))
                np.testing.assert_array_equal(_bits(d.get("carry")), _bits(seeded))
                _ok(L, L.pp3_episode_stats_rows(0, nsteps, n, stride, p("rew"), p("done"),
                                                p(tr_name) if tr_name else None, ar, p("carry"), p("part"), p("out"), None))
                got.append((d.get("carry"), d.get("part"), d.get("out")))
            for a, b in zip(got[0], got[1]):
                np.testing.assert_array_equal(_bits(a), _bits(b))
            for a, b, what in zip(got[0], (want_carry, want_part, want_out), ("carry", "part", "out4")):
                np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{what} ({tr_name})")
                assert np.all(np.isfinite(a))
            assert got[0][2][0] == dn.sum()
            if tr_name is None:
                assert got[0][2][3] == 0
        # a second call continues from the carry the first wrote back: two calls equal one over both
        _ok(L, L.pp3_episode_stats_begin(0, n, p("epi"), es, p("pd"), p("carry"), None))
        for _ in range(2):
            _ok(L, L.pp3_episode_stats_rows(0, nsteps, n, stride, p("rew"), p("done"), p("trunc"), ar, p("carry"),
                                            p("part"), p("out"), None))
        both, _ = M.episode_rows(seeded, np.concatenate([rew[:, :n]] * 2), np.concatenate([dn] * 2),
                                 np.concatenate([trunc[:, :n]] * 2), ar)
        np.testing.assert_array_equal(_bits(d.get("carry")), _bits(both))
    finally:
        d.free()


SHARDS = {1025: [(1025,), (513, 512)], 10: [(10,), (4, 4, 2)]}


@pytest.mark.parametrize("n, cuts", [(n, c) for n, cs in SHARDS.items() for c in cs])
def test_eval_chain_equals_the_restatement_bitwise(require_gpu, n, cuts):
    """Per-shard pp3_eval_column_sums stacked into [world][22] -> pp3_sum_gathered_f32 -> pp3_eval_finish,
    twice (means, then deviations); no collective.  One shard: also pp3_eval_reduce's 42 outputs."""
    L = require_gpu
    rs = np.random.RandomState(n + len(cuts))
    acc = (rs.normal(size=(R.WORDS, n)) * 10.0 ** rs.randint(-2, 3, size=(R.WORDS, n))).astype(F)
    acc[R.STEPS] = rs.randint(1, 1000, size=n)
    world = len(cuts)
    edges = np.concatenate([[0], np.cumsum(cuts)])
    shards = [np.ascontiguousarray(acc[:, a:b]) for a, b in zip(edges[:-1], edges[1:])]
    d = _Dev(gathered=np.full((world, 22), np.nan, F), total=np.full(22, np.nan, F), out=np.full(42, np.nan, F),
             ref=np.full(42, np.nan, F), **{f"acc{r}": s for r, s in enumerate(shards)})
    p = d.ptr
    try:
        for which, mean in ((0, None), (1, p("out"))):
            for r, s in enumerate(shards):
                _ok(L, L.pp3_eval_column_sums(0, s.shape[1], p(f"acc{r}"), mean, p("gathered", 22 * r), None))
            _ok(L, L.pp3_sum_gathered_f32(0, p("gathered"), world, 22, p("total"), None))
            g = d.get("gathered")
            want_g = np.stack([M.column_sums(s, None if which == 0 else d.get("out")[:21]) for s in shards])
            np.testing.assert_array_equal(_bits(g), _bits(want_g), err_msg=f"column sums {which}")
            np.testing.assert_array_equal(_bits(d.get("total")), _bits(M.sum_gathered(g)))
            assert d.get("total")[21] == n
            _ok(L, L.pp3_eval_finish(0, p("total"), which, p("out"), None))
        got = d.get("out")
        np.testing.assert_array_equal(_bits(got), _bits(M.eval_chain(shards)))
        assert np.all(np.isfinite(got))
        if world == 1:
            _ok(L, L.pp3_eval_reduce(0, n, p("acc0"), p("ref"), None))
            np.testing.assert_array_equal(_bits(got), _bits(d.get("ref")))
        else:  # every env weighs the same: the whole accumulator's mean, to f32 summation error
            np.testing.assert_allclose(got[:20], acc[:20].astype(np.float64).mean(1), rtol=1e-5, atol=1e-4)
    finally:
        d.free()


def test_sum_gathered_is_rank_ordered(require_gpu):
    L = require_gpu
    rs = np.random.RandomState(3)
    for world, count in ((1, 4), (3, 22), (64, 300)):
        g = (rs.normal(size=(world, count)) * 10.0 ** rs.randint(-3, 4, size=(world, count))).astype(F)
        d = _Dev(g=g, out=np.full(count, np.nan, F))
        try:
            _ok(L, L.pp3_sum_gathered_f32(0, d.ptr("g"), world, count, d.ptr("out"), None))
            np.testing.assert_array_equal(_bits(d.get("out")), _bits(M.sum_gathered(g)))
        finally:
            d.free()


def test_argument_errors_launch_nothing(require_gpu):
    L = require_gpu
    n, K = 8, 3
    s3, s4 = np.arange(3 * n, dtype=F).reshape(3, n) + 0.5, np.arange(4 * n, dtype=F).reshape(4, n) + 0.25
    acc = np.arange(22 * n, dtype=F).reshape(22, n)
    d = _Dev(carry=s3, part=s4, out=np.full(4, -7.0, F), epi=np.zeros((n, 4), F), v=np.zeros(n, F),
             rows=np.zeros((K, n), F), acc=acc, o22=np.full(22, -3.0, F), o42=np.full(42, -5.0, F),
             g=np.zeros((2, 22), F))
    p = d.ptr
    rows = lambda **kw: L.pp3_episode_stats_rows(*[{**dict(  # noqa: E731
        device=0, nsteps=K, n=n, stride=n, rew=p("rows"), done=p("rows"), trunc=p("rows"), ar=1, carry=p("carry"),
        part=p("part"), out=p("out"), stream=None), **kw}[k] for k in (
            "device", "nsteps", "n", "stride", "rew", "done", "trunc", "ar", "carry", "part", "out", "stream")])
    try:
        assert rows() == 0 and rows(trunc=None) == 0  # (the valid call, so every refusal below is its one change)
        d.bufs["carry"].upload(s3), d.bufs["part"].upload(s4), d.bufs["out"].upload(np.full(4, -7.0, F))
        bad = [
            L.pp3_episode_stats_begin(0, n, None, 4, p("v"), p("carry"), None),
            L.pp3_episode_stats_begin(0, n, p("epi"), 4, None, p("carry"), None),
            L.pp3_episode_stats_begin(0, n, p("epi"), 4, p("v"), None, None),
            L.pp3_episode_stats_begin(0, 0, p("epi"), 4, p("v"), p("carry"), None),
            L.pp3_episode_stats_begin(0, n, p("epi"), 3, p("v"), p("carry"), None),
            L.pp3_episode_stats_begin(0, n, p("carry"), 4, p("v"), p("carry"), None),
            L.pp3_episode_stats_begin(0, n, p("epi"), 4, p("carry", 2 * n), p("carry"), None),
            rows(rew=None), rows(done=None), rows(carry=None), rows(part=None), rows(out=None),
            rows(n=0), rows(nsteps=0), rows(stride=n - 1), rows(ar=0),
            rows(nsteps=1 << 21),  # nsteps * n = 2^24
            rows(rew=p("carry")), rows(done=p("part")), rows(trunc=p("part", 3 * n)), rows(part=p("carry", n)),
            rows(out=p("part", 5)), rows(out=p("carry", 1)), rows(out=p("rows", 2)),
            L.pp3_sum_gathered_f32(0, None, 2, 22, p("o22"), None), L.pp3_sum_gathered_f32(0, p("g"), 2, 22, None, None),
            L.pp3_sum_gathered_f32(0, p("g"), 0, 22, p("o22"), None),
            L.pp3_sum_gathered_f32(0, p("g"), _abi.LEARN_MAX_WORLD + 1, 22, p("o22"), None),
            L.pp3_sum_gathered_f32(0, p("g"), 2, 0, p("o22"), None),
            L.pp3_sum_gathered_f32(0, p("g"), 2, 22, p("g", 30), None),
            L.pp3_eval_column_sums(0, n, None, None, p("o22"), None),
            L.pp3_eval_column_sums(0, n, p("acc"), None, None, None),
            L.pp3_eval_column_sums(0, 0, p("acc"), None, p("o22"), None),
            L.pp3_eval_column_sums(0, n, p("acc"), None, p("acc", 9), None),
            L.pp3_eval_column_sums(0, n, p("acc"), p("o22"), p("o22", 0), None),
            L.pp3_eval_finish(0, None, 0, p("o42"), None), L.pp3_eval_finish(0, p("o22"), 0, None, None),
            L.pp3_eval_finish(0, p("o22"), 2, p("o42"), None), L.pp3_eval_finish(0, p("o22"), -1, p("o42"), None),
            L.pp3_eval_finish(0, p("o42", 10), 1, p("o42"), None),
        ]
        assert bad == [ERR_ARG] * len(bad), bad
        assert b"pp3_eval_finish" in L.pp3_ppo_last_error()
        for name, want in (("carry", s3), ("part", s4), ("out", np.full(4, -7.0, F)), ("acc", acc),
                           ("o22", np.full(22, -3.0, F)), ("o42", np.full(42, -5.0, F)), ("g", np.zeros((2, 22), F))):
            np.testing.assert_array_equal(d.get(name), want, err_msg=name)
    finally:
        d.free()


# ------------------------------------------------------------------------------ end to end
def _small_learner(n, K, seed=3):
    import ppo_loss_ref as PR
    from test_gpu_ppo_learn import _dicts
    case = PR.random_case(seed, K=K, B=n, in_dim=72, hidden=(16,), activation="elu", with_normalizer=False)
    pol, val = _dicts(case)
    return lambda: ppo.PPOLearner(pol, val, max_rows=(K + 1) * n)


def _batch_rows(w):
    b = w.ppo_device_batch()
    w.env.synchronize()
    out = {}
    for name in ("reward", "done", "truncation"):
        ptr, shape = b[name]
        out[name] = np.empty(shape, F)
        _lib.check(w.env._L.pp3_memcpy_d2h(out[name].ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out[name].nbytes))
    return out


def _record(w):
    """(ret, len, pd) [3][n] of the env's own fields, as pp3_episode_stats_begin reads them"""
    w.env.synchronize()
    return M.episode_begin(w.env._get(_abi.F_EPISODE), w.env._get(_abi.F_DONE), _abi.EP_SUM_REWARD, _abi.EP_LENGTH)


def _iteration_keys(key, count):
    ks = []
    for _ in range(count):
        key, k_it = rng.split(key, 2)
        ks.append(k_it)
    return ks


def test_episode_stats_of_train_iterations_equal_the_wrapper_host_loop(require_gpu, tmp_path):
    """5 envs, episode_length 5, unroll 3, four train_iteration(episode_stats=) calls with the sampled
    actor (lr 0: the host loop below samples from the same parameters in every iteration).  Per
    iteration out4 and the carry are the restatement's on the downloaded rows and the carry is the
    env's record; the totals are those of a host loop over wrap(env).step reading
    info["episode_metrics"] and info["truncation"] at the done steps."""
    n, K, L, iters = 5, 3, 5, 4
    envs = _envs(tmp_path, n, 2)
    learner = _small_learner(n, K)()
    handles = []
    stats = ppo.EpisodeStats()
    try:
        w, wh = (wrappers.wrap(e, episode_length=L) for e in envs)
        with pytest.raises(ValueError, match="wrapped"):
            stats.begin(envs[0])
        actor, critic = learner.make_policies()
        handles += [actor, critic]
        keys = _iteration_keys(rng.PRNGKey(7), iters)
        reset_keys = rng.split(rng.split(rng.PRNGKey(100), 2)[1], n)  # (test_gpu_ppo_eval's resets: low and high starters)
        state = w.reset(reset_keys)
        start = learner._download(0, 0)
        want_total = [0, 0.0, 0.0, 0.0]
        all_done, begins = [], []
        for it in range(iters):
            before = _record(w)
            begins.append(before)
            state, _, _ = learner.train_iteration(w, state, keys[it], actor, critic, K, lr=0.0, episode_stats=stats)
            rows = _batch_rows(w)
            want_carry, want_part = M.episode_rows(before, rows["reward"], rows["done"], rows["truncation"], 1)
            want_out = M.episode_out4(want_part)
            np.testing.assert_array_equal(_bits(stats.last), _bits(want_out), err_msg=f"iteration {it}")
            np.testing.assert_array_equal(_bits(stats.carry()), _bits(want_carry), err_msg=f"iteration {it}")
            np.testing.assert_array_equal(_bits(stats.carry()), _bits(_record(w)), err_msg=f"iteration {it}")
            np.testing.assert_array_equal(_bits(stats.local_out4()), _bits(want_out))
            want_total = [want_total[0] + int(want_out[0])] + [a + float(b) for a, b in zip(want_total[1:], want_out[1:])]
            all_done.append(rows["done"])
        np.testing.assert_array_equal(learner._download(0, 0).view(U), start.view(U))  # lr 0: the same actor throughout
        count, sums = stats.read()
        assert [count, sums["sum_reward"], sums["length"], sums["truncated"]] == want_total
        dones = np.concatenate(all_done)
        # the conditions (not measurements): an episode in progress at a rollout boundary that ends
        # later, a truncated episode, consecutive dones
        assert any(((b[2] == 0) & (b[1] > 0) & (d != 0).any(0)).any() for b, d in zip(begins[1:], all_done[1:]))
        assert sums["truncated"] >= 1 and sums["truncated"] < count
        assert (dones[1:] * dones[:-1]).any()

        # the host loop: the same reset, per iteration the collect's key chain from split(k_it)[0]
        st = wh.reset(reset_keys)
        buf = _lib.DeviceBuffer(4 * n * 12)
        host_total, plain = [0, 0.0, 0.0, 0.0], np.zeros(4)
        try:
            for it in range(iters):
                chain = rng.split(keys[it], 2)[0]
                part = np.zeros((4, n), F)
                for t in range(K):
                    cur, chain = rng.split(chain, 2)
                    actor.sample_env(wh.env, cur, buf.ptr.value)
                    wh.env.synchronize()
                    st = wh.step(st, _download(buf, (n, 12)))
                    d = np.array(st.done) != 0
                    np.testing.assert_array_equal(np.array(st.done), all_done[it][t])
                    em = st.info["episode_metrics"]
                    for c, x in enumerate((np.ones(n, F), em["sum_reward"], em["length"], st.info["truncation"])):
                        part[c] = np.where(d, (part[c] + np.asarray(x, F)).astype(F), part[c])
                        plain[c] += np.asarray(x, np.float64)[d].sum()
                out = M.episode_out4(part)
                host_total = [host_total[0] + int(out[0])] + [a + float(b) for a, b in zip(host_total[1:], out[1:])]
        finally:
            buf.free()
        assert host_total == want_total
        assert count == plain[0] and sums["length"] == plain[2] and sums["truncated"] == plain[3]
        assert abs(sums["sum_reward"] - plain[1]) <= 1e-5 * max(1.0, abs(plain[1]))
        m = stats.metrics()
        assert m == {"episode/count": count, "episode/sum_reward": sums["sum_reward"] / count,
                     "episode/length": sums["length"] / count, "episode/truncated": sums["truncated"] / count}
        stats.reset()
        assert stats.metrics() == {"episode/count": 0}
    finally:
        stats.close()
        for h in handles:
            h.close()
        learner.close()
        for e in envs:
            e.close()


def test_collect_ppo_without_the_host_batch(require_gpu, tmp_path):
    n, K, L = 5, 3, 5
    envs = _envs(tmp_path, n, 2)
    learner = _small_learner(n, K)()
    handles = []
    try:
        ws = [wrappers.wrap(e, episode_length=L) for e in envs]
        actor, critic = learner.make_policies()
        handles += [actor, critic]
        key = rng.PRNGKey(5)
        res = []
        for w, host in zip(ws, (True, False)):
            st = w.reset(rng.split(rng.PRNGKey(100), n))
            st, batch, k = w.collect_ppo(st, actor, critic, K, key, host_batch=host)
            assert (batch is None) == (not host)
            dev = w.ppo_device_batch()
            w.env.synchronize()
            arrays = {}
            for name, (ptr, shape) in dev.items():
                arrays[name] = np.empty(shape, F)
                _lib.check(w.env._L.pp3_memcpy_d2h(arrays[name].ctypes.data_as(C.c_void_p), C.c_void_p(ptr),
                                                    arrays[name].nbytes))
            assert w.env.holds(st)
            res.append((st, batch, k, arrays))
        (sa, batch, ka, da), (sb, _, kb, db) = res
        np.testing.assert_array_equal(ka, kb)
        assert set(da) == set(db) == set(batch)
        for name in da:
            np.testing.assert_array_equal(_bits(da[name]), _bits(db[name]), err_msg=name)
            np.testing.assert_array_equal(_bits(batch[name]), _bits(db[name]), err_msg=name)
        for f in ("obs", "reward", "done"):
            np.testing.assert_array_equal(_bits(getattr(sa, f)), _bits(getattr(sb, f)), err_msg=f)
        np.testing.assert_array_equal(sa._record.view(U), sb._record.view(U))
        # the state goes on as the host-batch one does
        for w, s in ((ws[0], sa), (ws[1], sb)):
            s2, _, _ = w.collect_ppo(s, actor, critic, K, ka, host_batch=False)
            res.append(np.array(s2.obs))
        np.testing.assert_array_equal(_bits(res[2]), _bits(res[3]))
    finally:
        for h in handles:
            h.close()
        learner.close()
        for e in envs:
            e.close()


def _state_bits(learner):
    return np.concatenate([learner._download(net, which) for net in (0, 1) for which in (0, 2, 3)]).view(U)


EPISODE_KEYS = ("episode/count", "episode/sum_reward", "episode/length", "episode/truncated")


def test_train_logs_training_episode_metrics(require_gpu, tmp_path):
    """6 + 4 envs, unroll 3, 2 minibatches, num_evals 3, 70 timesteps: 2 epochs of 2 iterations,
    reports at 0, 36, 72 steps."""
    n, ne, K, L = 6, 4, 3, 5
    make = _small_learner(n, K)
    envs = _envs(tmp_path, n, 3) + _envs(tmp_path, ne, 2)
    learners = [make() for _ in range(5)]
    lA, lH, lC, lN, lB = learners
    handles = []
    stats = ppo.EpisodeStats()
    try:
        wt = [wrappers.wrap(e, episode_length=L) for e in envs[:3]]
        we = [wrappers.wrap(e, episode_length=L) for e in envs[3:]]
        key = rng.PRNGKey(21)
        path = lambda s: os.path.join(str(tmp_path), f"ck_{s}.npz")  # noqa: E731
        args = dict(num_timesteps=70, episode_length=L, unroll_length=K, num_minibatches=2, learning_rate=1e-3,
                    num_evals=3, key=key)

        def run(learner, w, e, **kw):
            progress = []
            actor, critic, metrics = ppo.train(learner, w, e, **{**args, **kw},
                                               progress_fn=lambda s, m: progress.append((s, dict(m))))
            handles.extend([actor, critic])
            return progress, metrics

        prog_a, metrics_a = run(lA, wt[0], we[0], log_training_metrics=True, checkpoint_path=path)
        assert [s for s, _ in prog_a] == [0, 36, 72] and metrics_a == prog_a[-1][1]
        assert not any(k.startswith("episode/") for k in prog_a[0][1])
        # the same iterations by hand with an EpisodeStats of their own; the accumulators reset between reports
        k_train, k_env, _ = rng.split(key, 3)
        a2, c2 = lH.make_policies()
        handles += [a2, c2]
        state = wt[1].reset(rng.split(k_env, n))
        reports = []
        for epoch in range(2):
            for _ in range(2):
                k_train, k_it = rng.split(k_train, 2)
                state, _, _ = lH.train_iteration(wt[1], state, k_it, a2, c2, K, num_minibatches=2, lr=1e-3, shuffle=True,
                                                 device_rng=True, episode_stats=stats)
            reports.append(stats.metrics())
            stats.reset()
        for (_, m), want in zip(prog_a[1:], reports):
            assert want["episode/count"] > 0 and set(want) == set(EPISODE_KEYS)
            assert {k: m[k] for k in EPISODE_KEYS} == want
            assert "eval/episode_reward" in m and "training/total_loss" in m
        assert reports[0] != reports[1]
        # the flag changes no learner bit
        prog_c, _ = run(lC, wt[1], we[1])
        assert not any(k.startswith("episode/") for _, m in prog_c for k in m)
        np.testing.assert_array_equal(_state_bits(lA), _state_bits(lH))
        np.testing.assert_array_equal(_state_bits(lA), _state_bits(lC))
        for (_, ma), (_, mc) in zip(prog_a, prog_c):
            assert ma["eval/episode_reward"] == mc["eval/episode_reward"]
        # no eval env: progress_fn at each epoch end with the training metrics; without the flag, never
        prog_n, metrics_n = run(lN, wt[1], None, log_training_metrics=True)
        assert [s for s, _ in prog_n] == [36, 72] and metrics_n == prog_n[-1][1]
        for (_, m), want in zip(prog_n, reports):
            assert {k: m[k] for k in EPISODE_KEYS} == want and "training/sps" in m
            assert not any(k.startswith("eval/") for k in m)
        np.testing.assert_array_equal(_state_bits(lN), _state_bits(lA))
        # interrupted at the first checkpoint after an epoch and resumed on fresh objects
        prog_b, _ = run(lB, wt[2], we[1], log_training_metrics=True, restore=path(36))
        assert [s for s, _ in prog_b] == [72]
        assert {k: prog_b[0][1][k] for k in EPISODE_KEYS} == reports[1]
        np.testing.assert_array_equal(_state_bits(lB), _state_bits(lA))
    finally:
        stats.close()
        for h in handles:
            h.close()
        for l in learners:
            l.close()
        for e in envs:
            e.close()
