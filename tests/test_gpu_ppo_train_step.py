"""The rest of Brax's training_step on the device (csrc/pp3_learn.hip): the running normaliser
(pp3_learner_normalizer_update), the env index behind the loss (pp3_learner_set_env_index,
pp3_ppo_loss_grad_indexed), the global-norm clip (pp3_grad_clip) and PPOLearner.train_iteration's
shuffle / max_grad_norm / update_normalizer.

Normaliser parity rule (the project's, as in test_gpu_ppo_learn.py): for each of mean,
summed_variance and std, err = max |x - ref64| / max |ref64| against the float64 restatement
(tests/ppo_train_ref.py), and err <= 5 x the largest err of the SAME restatement in float32 numpy over
16 seeds at that shape, computed here.  The indexed loss and the un-clipped gradients are compared bit
for bit; the clip's bounds are the worst case of an any-order f32 sum of n non-negative terms."""
import ctypes as C

import numpy as np
import pytest

import common
import ppo_loss_ref as R
import ppo_train_ref as T
from pupperv3_mjx import _lib, ppo, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_ppo_learn import _act_and_sample, _bits, _dicts, _forward, _learner

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
NAMES = ("mean", "summed_variance", "std")


# ------------------------------------------------------------------------------ helpers
def _small_learner(in_dim):
    case = R.random_case(0, K=1, B=2, in_dim=in_dim, hidden=(8,), activation="tanh", with_normalizer=False)
    return _learner(case, max_rows=4)


def _err(x, ref):
    """max |x - ref| / max |ref| (0 when x equals ref everywhere)."""
    num = float(np.abs(np.asarray(x, np.float64) - ref).max())
    return 0.0 if num == 0.0 else num / float(np.abs(ref).max())


class _Norm:
    """obs on the device and a (mean, summed_variance, std) state buffer for direct calls."""

    def __init__(self, L, learner, obs):
        self.L, self.learner = L, learner
        self.D = obs.shape[-1]
        self.obs = _lib.DeviceBuffer(obs.nbytes)
        self.obs.upload(obs)
        self.state = _lib.DeviceBuffer(12 * self.D)

    def args(self, rows, count_new, std_min=T.STD_MIN, std_max=T.STD_MAX):
        b = self.state.ptr.value
        return dict(h=self.learner._h, obs=self.obs.ptr, rows=rows, count=float(F(count_new)), std_min=std_min,
                    std_max=std_max, mean=C.c_void_p(b), sv=C.c_void_p(b + 4 * self.D), std=C.c_void_p(b + 8 * self.D),
                    stream=None)

    def get(self):
        out = np.empty((3, self.D), F)
        self.state.download(out)
        return out

    def run(self, rows, count_new, mean, sv, std, **kw):
        self.state.upload(np.stack([np.asarray(a, F) for a in (mean, sv, std)]))
        assert self.L.pp3_learner_normalizer_update(*self.args(rows, count_new, **kw).values()) == 0, \
            self.L.pp3_learn_last_error()
        return self.get()

    def free(self):
        self.obs.free(), self.state.free()


def _norm_case(seed, rows, D, chained):
    """(obs f32 [rows, D], count_new, mean, summed_variance, std) with columns offset by up to 2 and stds
    in 0.1 .. 3.  chained: the state is the f64 update of an earlier 2000-row matrix of the same columns
    rounded to f32, its summed_variance and count scaled to a count of 10^6."""
    rs = np.random.RandomState(1000 * seed + rows + D)
    loc, scale = rs.uniform(-2, 2, size=D), rs.uniform(0.1, 3, size=D)
    x = rs.normal(loc=loc, scale=scale, size=(rows, D)).astype(F)
    if not chained:
        return (x, rows) + T.initial_state(D, F)[1:]
    y = rs.normal(loc=loc, scale=scale, size=(2000, D)).astype(F)
    m, s, sd = T.normalizer_update(y, 2000, *T.initial_state(D)[1:3])
    count = 10 ** 6
    return x, count + rows, m.astype(F), (s * (count / 2000)).astype(F), sd.astype(F)


def _bound(rows, D, chained):
    """5 x the f32 numpy restatement's largest error over 16 seeds, per quantity."""
    bound = dict.fromkeys(NAMES, 0.0)
    for seed in range(16):
        x, count, mean, sv, _ = _norm_case(seed, rows, D, chained)
        ref = T.normalizer_update(x, count, mean, sv)
        got = T.normalizer_update(x, count, mean, sv, dtype=F)
        for k, a, b in zip(NAMES, got, ref):
            bound[k] = max(bound[k], 5 * _err(a, b))
    return bound


# ------------------------------------------------------------------------------ normaliser
SHAPES = [(1, 36), (7, 72), (3001, 72), (3001, 540), (ppo.NORM_RANGES, 36), (ppo.NORM_RANGES + 1, 36)]


@pytest.mark.parametrize("chained", [False, True], ids=["first", "chained"])
@pytest.mark.parametrize("rows, D", SHAPES)
def test_normalizer_update_matches_the_f64_reference(require_gpu, rows, D, chained):
    bound = _bound(rows, D, chained)
    x, count, mean, sv, std = _norm_case(0, rows, D, chained)
    ref = T.normalizer_update(x, count, mean, sv)
    learner = _small_learner(D)
    dev = _Norm(require_gpu, learner, x)
    try:
        got = dev.run(rows, count, mean, sv, std)
        again = dev.run(rows, count, mean, sv, std)
    finally:
        dev.free(), learner.close()
    np.testing.assert_array_equal(got.view(U), again.view(U))  # the same bits twice
    assert np.all(np.isfinite(got))
    errs = {k: _err(a, b) for k, a, b in zip(NAMES, got, ref)}
    for k in NAMES:
        print(f"normaliser ({rows}, {D}) {'chained' if chained else 'first'} {k}: err {errs[k]:.3e} bound {bound[k]:.3e}")
    bad = {k: (errs[k], bound[k]) for k in NAMES if not errs[k] <= bound[k]}
    assert not bad, bad


def test_normalizer_known_answers_are_exact(require_gpu):
    D = 36
    row = ((np.arange(D) - 18) / 8).astype(F)  # small dyadic values
    learner = _small_learner(D)
    dev = _Norm(require_gpu, learner, np.tile(row, (64, 1)))
    unit = _Norm(require_gpu, learner, np.random.RandomState(2).normal(size=(64, D)).astype(F))
    try:
        _, mean, sv, std = T.initial_state(D, F)
        got = dev.run(64, 64, mean, sv, std)
        np.testing.assert_array_equal(got[0].view(U), row.view(U))
        np.testing.assert_array_equal(got[1].view(U), np.zeros(D, U))
        np.testing.assert_array_equal(got[2].view(U), np.full(D, F(T.STD_MIN)).view(U))
        capped = unit.run(64, 64, mean, sv, std, std_max=0.5)
        np.testing.assert_array_equal(capped[2].view(U), np.full(D, F(0.5)).view(U))
        assert np.all(capped[1] > 0.25 * 64)
    finally:
        dev.free(), unit.free(), learner.close()


def test_normalizer_does_not_read_the_bootstrap_row(require_gpu):
    K, N, D = 3, 5, 36
    obs = np.random.RandomState(3).normal(size=(K + 1, N, D)).astype(F)
    obs[K] = np.nan
    learner = _small_learner(D)
    full, cut = _Norm(require_gpu, learner, obs), _Norm(require_gpu, learner, obs[:K])
    try:
        _, mean, sv, std = T.initial_state(D, F)
        got = full.run(K * N, K * N, mean, sv, std)
        want = cut.run(K * N, K * N, mean, sv, std)
    finally:
        full.free(), cut.free(), learner.close()
    assert np.all(np.isfinite(got))
    np.testing.assert_array_equal(got.view(U), want.view(U))


# ------------------------------------------------------------------------------ indexed loss
class _Arrays:
    """Full batch arrays [K(+1)][N][..] on the device."""

    def __init__(self, arrays):
        self.bufs = {}
        for name in ("obs_all", "raw_action", "log_prob", "reward", "done", "truncation", "eps"):
            a = np.ascontiguousarray(arrays[name], dtype=F)
            self.bufs[name] = _lib.DeviceBuffer(a.nbytes)
            self.bufs[name].upload(a)

    def run(self, learner, K, B, N, e0, hp, indexed):
        learner.loss_and_grad_device(K, B, N, e0, *(b.ptr.value for b in self.bufs.values()), None,
                                     **{k: hp[k] for k in ppo.HPARAMS}, indexed=indexed)
        return _bits(learner.metrics(), learner.grads())

    def free(self):
        for b in self.bufs.values():
            b.free()


INDEXED = {  # K, B, N, e0, in_dim, hidden, activation
    "offset_stride_elu": (2, 7, 24, 3, 72, (40, 24), "elu"),
    "row_chunk_plus_one_tanh": (1, ppo.ROW_CHUNK + 1, ppo.ROW_CHUNK + 4, 2, 36, (20,), "tanh"),
}


@pytest.mark.parametrize("name", list(INDEXED))
def test_indexed_loss_equals_the_plain_loss_on_the_permuted_batch_bitwise(require_gpu, name):
    K, B, N, e0, in_dim, hidden, act = INDEXED[name]
    case = R.random_case(0, K=K, B=N, in_dim=in_dim, hidden=hidden, activation=act, with_normalizer=True)
    X = case["batch"]
    P = rng.permutation(rng.PRNGKey(5), N)
    assert np.any(P[e0:e0 + B] != np.arange(e0, e0 + B))
    permuted = {k: v[:, P] for k, v in X.items()}  # X'[:, j] = X[:, P[j]]
    poisoned = {k: np.full_like(v, np.nan) for k, v in X.items()}
    for k, v in X.items():
        poisoned[k][:, P[e0:e0 + B]] = v[:, P[e0:e0 + B]]
    learner = _learner(case, max_rows=(K + 1) * B)
    bufs = [_Arrays(a) for a in (X, permuted, poisoned)]
    try:
        plain = bufs[0].run(learner, K, B, N, e0, case["hp"], False)
        want = bufs[1].run(learner, K, B, N, e0, case["hp"], False)
        learner.set_env_index(P)
        got = bufs[2].run(learner, K, B, N, e0, case["hp"], True)
        learner.set_env_index(np.arange(N))
        ident = bufs[0].run(learner, K, B, N, e0, case["hp"], True)
    finally:
        for b in bufs:
            b.free()
        learner.close()
    assert np.all(np.isfinite(got.view(F)))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ident, plain)
    assert np.mean(got != plain) > 0.9


# ------------------------------------------------------------------------------ clip
def test_grad_clip_leaves_small_gradients_alone_and_scales_large_ones(require_gpu):
    L = require_gpu
    case = R.random_case(0, K=2, B=4, in_dim=36, hidden=(20,), activation="tanh", with_normalizer=False)
    learner = _learner(case)
    rs = np.random.RandomState(4)
    try:
        counts = [learner.buffer(net, 0)[1] for net in (0, 1)]
        assert counts == [37 * 20 + 21 * 24, 37 * 20 + 21] and all(c % 256 for c in counts)
        n = sum(counts)
        g = [rs.normal(scale=10.0 ** rs.uniform(-4, 1, size=c)).astype(F) for c in counts]

        def upload():
            for net in (0, 1):
                _lib.check(L.pp3_memcpy_h2d(C.c_void_p(learner.buffer(net, 1)[0]), g[net].ctypes.data_as(C.c_void_p),
                                            g[net].nbytes))

        norm64, _ = T.clip_by_global_norm(g, np.inf)
        upload()
        learner.clip_gradients(float(F(2 * norm64)))
        for net in (0, 1):
            np.testing.assert_array_equal(learner._download(net, 1).view(U), g[net].view(U))
        rel = abs(learner.grad_norm() - norm64) / norm64
        print(f"clip: norm {learner.grad_norm():.9g} f64 {norm64:.9g} rel {rel:.3e} bound {(n + 2) * 2.0 ** -24:.3e}")
        assert rel <= (n + 2) * 2.0 ** -24
        max_norm = float(F(norm64 / 3))
        _, want = T.clip_by_global_norm(g, max_norm)
        learner.clip_gradients(max_norm)
        got = [learner._download(net, 1).astype(np.float64) for net in (0, 1)]
        tol = (n + 8) * 2.0 ** -24
        for net in (0, 1):
            slack = np.abs(got[net] - want[net]) - tol * np.abs(g[net]) * max_norm / norm64
            assert np.all(slack <= 0), (net, float(slack.max()))
        after, _ = T.clip_by_global_norm(got, np.inf)
        assert abs(after - max_norm) / max_norm <= tol
        assert abs(learner.grad_norm() - norm64) / norm64 <= (n + 2) * 2.0 ** -24  # the norm before clipping
        learner.clip_gradients(max_norm)  # clipped to the bound: at most a rounding over it, scaled again or left
        assert abs(learner.grad_norm() - max_norm) / max_norm <= tol + (n + 2) * 2.0 ** -24
    finally:
        learner.close()


# ------------------------------------------------------------------------------ train_iteration
def _download(L, ptr, shape):
    out = np.empty(shape, F)
    _lib.check(L.pp3_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
    return out


def test_train_iteration_with_shuffle_clip_and_running_normaliser(require_gpu, tmp_path):
    """32 envs, K = 4, twice: 2 updates x 2 shuffled minibatches each, clip, the running normaliser from
    Brax's initial state.  The normaliser after the first iteration is held to the parity rule on the
    rows the env produced: 5 x the f32 numpy restatement's largest error over 16 seeds at that shape,
    a seed being an order of those very rows.  (Random columns of another distribution do not give
    this matrix's bound: the env's observations have columns whose spread is a small fraction of
    their offset, and there the f32 rounding of mean' alone moves summed_variance and the std's
    square root, for any f32 implementation; the f64 result does not depend on the row order.)"""
    n, K, D = 32, 4, 72
    case = R.random_case(6, K=K, B=n, in_dim=D, hidden=(64, 32), activation="elu", with_normalizer=False)
    path = common.write_model(tmp_path, 0)
    env = PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.21, observation_history=2), num_envs=n)
    pol, val = _dicts(case)
    learner = ppo.PPOLearner(pol, val, running_statistics=True, max_rows=(K + 1) * n)
    actor, critic = learner.make_policies()
    indices = []
    set_index = learner.set_env_index
    learner.set_env_index = lambda index, stream=None: indices.append(np.array(index)) or set_index(index, stream)
    try:
        w = wrappers.wrap(env, episode_length=3)
        state = w.reset(make_keys(3, n))
        key = rng.PRNGKey(12)
        want_indices = []
        for it in range(2):
            k_perm = rng.split(rng.split(key, 2)[1], 2)[1]
            for _ in range(2):
                k_perm, k_u = rng.split(k_perm, 2)
                want_indices.append(T.permutation(k_u, n)[0])
            state, metrics, key = learner.train_iteration(w, state, key, actor, critic, K, num_minibatches=2,
                                                          num_updates_per_batch=2, lr=1e-4, shuffle=True,
                                                          max_grad_norm=0.5, update_normalizer=True)
            assert all(np.isfinite(v) for v in metrics.values()), metrics
            assert learner.t == 4 * (it + 1)
            assert np.isfinite(learner.grad_norm()) and learner.grad_norm() > 0
            ns = learner.normalizer_state()
            assert ns["count"] == (it + 1) * K * n
            if it == 0:
                ptr, shape = w.ppo_device_batch()["observation"]
                obs = _download(require_gpu, ptr, shape).reshape(K * n, D)
                ref = T.normalizer_update(obs, K * n, *T.initial_state(D)[1:3])
                bound = dict.fromkeys(NAMES, 0.0)
                for seed in range(16):
                    rows = obs[np.random.RandomState(seed).permutation(K * n)]
                    got32 = T.normalizer_update(rows, K * n, *T.initial_state(D, F)[1:3], dtype=F)
                    for k, a, b in zip(NAMES, got32, ref):
                        bound[k] = max(bound[k], 5 * _err(a, b))
                worst = int(np.abs(ns["std"] - ref[2]).argmax())
                print(f"worst std column {worst}: mean {ref[0][worst]:.6g} std {ref[2][worst]:.6g} of max {ref[2].max():.6g}")
                for k, want in zip(NAMES, ref):
                    err = _err(ns[k], want)
                    print(f"train_iteration normaliser {k}: err {err:.3e} bound {bound[k]:.3e}")
                    assert err <= bound[k], (k, err, bound[k])
        assert learner.t == 8
        assert len(indices) == 4
        for got, want in zip(indices, want_indices):
            np.testing.assert_array_equal(got, want)
        assert np.any(indices[0] != indices[1]) and np.any(indices[2] != indices[3])
        # the handles hold the trained networks with the UPDATED statistics folded in
        end, ns = learner.params(), learner.normalizer_state()
        assert np.any(ns["mean"] != 0) and np.any(ns["std"] != 1)
        x = np.random.RandomState(8).normal(size=(19, D)).astype(F)
        for name, handle in (("policy", actor), ("value", critic)):
            (k0, b0), rest = end[name][0], end[name][1:]
            want = _forward([R.fold(k0, b0, ns["mean"], ns["std"])] + rest, "elu", x, np.float64)
            got = _act_and_sample(handle, x, rng.PRNGKey(1))["act"]
            assert np.all(np.abs(got - want) <= 2e-5 * (1 + np.abs(want))), name
    finally:
        actor.close(), critic.close(), learner.close(), env.close()


def test_train_iteration_defaults_issue_the_existing_calls(require_gpu, tmp_path):
    """With shuffle, max_grad_norm and update_normalizer off, one iteration leaves the parameters a
    second learner gets from loss_and_grad / adam_step / sync by hand, bit for bit."""
    n, K = 32, 4
    case = R.random_case(6, K=K, B=n, in_dim=72, hidden=(64, 32), activation="elu", with_normalizer=True)
    path = common.write_model(tmp_path, 0)
    envs = [PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.21, observation_history=2), num_envs=n)
            for _ in range(2)]
    learners = [_learner(case), _learner(case)]
    handles = [l.make_policies() for l in learners]
    try:
        ws = [wrappers.wrap(e, episode_length=3) for e in envs]
        states = [w.reset(make_keys(3, n)) for w in ws]
        key = rng.PRNGKey(12)
        learners[0].train_iteration(ws[0], states[0], key, *handles[0], K, num_minibatches=2, num_updates_per_batch=2,
                                    lr=1e-4)
        k_collect, k_eps = rng.split(key, 2)
        ws[1].collect_ppo(states[1], *handles[1], K, k_collect)
        for _ in range(2):
            for mb in range(2):
                learners[1].loss_and_grad(ws[1], mb * (n // 2), n // 2, k_eps)
                learners[1].adam_step(1e-4)
        learners[1].sync(*handles[1])
        a, b = learners[0].params(), learners[1].params()
        start = [a0 for kb in case["policy"] for a0 in kb]
        for net in ("policy", "value"):
            for (ka, ba), (kb, bb) in zip(a[net], b[net]):
                np.testing.assert_array_equal(ka.view(U), kb.view(U))
                np.testing.assert_array_equal(ba.view(U), bb.view(U))
        assert np.any(a["policy"][0][0] != start[0]) and learners[0].t == learners[1].t == 4
    finally:
        for h in handles:
            h[0].close(), h[1].close()
        for l in learners:
            l.close()
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(require_gpu):
    L = require_gpu
    nan, inf = float("nan"), float("inf")
    case = R.random_case(0, K=3, B=8, in_dim=36, hidden=(20,), activation="tanh", with_normalizer=True)
    learner = _learner(case, max_rows=32)
    batch = _Arrays(case["batch"])
    dev = _Norm(L, learner, np.random.RandomState(0).normal(size=(10, 36)).astype(F))
    SENT = F(-777.25)
    try:
        def fill():
            for net in (0, 1):  # gradients, metrics and the normaliser state hold a sentinel no refused call may touch
                ptr, cnt = learner.buffer(net, 1)
                s = np.full(cnt, SENT, F)
                _lib.check(L.pp3_memcpy_h2d(C.c_void_p(ptr), s.ctypes.data_as(C.c_void_p), s.nbytes))
            learner._metrics.upload(np.full(4, SENT, F))
            learner._gnorm.upload(np.full(1, SENT, F))
            dev.state.upload(np.full((3, 36), SENT, F))

        def untouched():
            got = np.zeros(4, F)
            learner._metrics.download(got)
            return (all(np.all(learner._download(net, 1) == SENT) for net in (0, 1)) and np.all(got == SENT)
                    and np.all(dev.get() == SENT) and learner.grad_norm() == SENT)

        def refused(fn, args, name):
            assert fn(*args) == 1, (name, args)
            assert name.encode() in L.pp3_learn_last_error(), L.pp3_learn_last_error()

        fill()
        # the normaliser update
        good = dev.args(10, 10)
        for change in (dict(h=None), dict(obs=None), dict(mean=None), dict(sv=None), dict(std=None), dict(rows=0),
                       dict(rows=-1), dict(count=nan), dict(count=inf), dict(count=9.0), dict(std_min=nan),
                       dict(std_max=inf), dict(std_max=nan), dict(std_min=0.0), dict(std_min=-1.0),
                       dict(std_min=2.0, std_max=1.0)):
            refused(L.pp3_learner_normalizer_update, {**good, **change}.values(), "pp3_learner_normalizer_update")
        # the clip
        for bad in (nan, inf, 0.0, -1.0):
            refused(L.pp3_grad_clip, (learner._h, bad, learner._gnorm.ptr, None), "pp3_grad_clip")
        refused(L.pp3_grad_clip, (None, 1.0, learner._gnorm.ptr, None), "pp3_grad_clip")
        # the index and the indexed loss
        p = {k: C.c_void_p(b.ptr.value) for k, b in batch.bufs.items()}
        mean, std = learner._norm_ptrs()
        loss = dict(h=learner._h, K=3, B=5, N=8, e0=1, obs_all=p["obs_all"], raw_action=p["raw_action"],
                    log_prob=p["log_prob"], reward=p["reward"], done=p["done"], truncation=p["truncation"], eps=p["eps"],
                    mean=mean, std=std, discount=0.97, lam=0.95, scaling=1.0, clip=0.3, ent=0.01, norm=1,
                    metrics=learner._metrics.ptr, stream=None)
        refused(L.pp3_ppo_loss_grad_indexed, loss.values(), "pp3_ppo_loss_grad_indexed")  # no index set yet
        ident = np.arange(9, dtype=np.int32)
        iptr = lambda a: a.ctypes.data_as(C.c_void_p)
        refused(L.pp3_learner_set_env_index, (None, iptr(ident), 8, None), "pp3_learner_set_env_index")
        refused(L.pp3_learner_set_env_index, (learner._h, None, 8, None), "pp3_learner_set_env_index")
        refused(L.pp3_learner_set_env_index, (learner._h, iptr(ident), 0, None), "pp3_learner_set_env_index")
        for entry in (8, -1):
            wrong = np.arange(8, dtype=np.int32)
            wrong[6] = entry
            refused(L.pp3_learner_set_env_index, (learner._h, iptr(wrong), 8, None), "pp3_learner_set_env_index")
        refused(L.pp3_ppo_loss_grad_indexed, loss.values(), "pp3_ppo_loss_grad_indexed")  # still none: nothing was copied
        assert L.pp3_learner_set_env_index(learner._h, iptr(ident), 9, None) == 0
        refused(L.pp3_ppo_loss_grad_indexed, loss.values(), "pp3_ppo_loss_grad_indexed")  # an index for 9 envs
        learner.set_env_index(np.arange(8))  # a valid index: pp3_ppo_loss_grad's own errors hold behind it
        for change in (dict(h=None), dict(eps=None), dict(B=0), dict(e0=4), dict(K=7), dict(clip=0.0), dict(mean=None)):
            refused(L.pp3_ppo_loss_grad_indexed, {**loss, **change}.values(), "pp3_ppo_loss_grad_indexed")
        with pytest.raises(_lib.PupperHipError):
            learner.set_env_index([0, 1, 2, 8, 4, 5, 6, 7])
        with pytest.raises(_lib.PupperHipError):
            learner.clip_gradients(0.0)
        assert untouched()
        # the good calls still run
        assert L.pp3_learner_normalizer_update(*good.values()) == 0
        assert np.all(np.isfinite(dev.get())) and np.all(dev.get() != SENT)
        learner.set_env_index(np.arange(8)[::-1])
        assert L.pp3_ppo_loss_grad_indexed(*loss.values()) == 0
        assert np.all(np.isfinite(learner._download(0, 1))) and np.all(learner._download(0, 1) != SENT)
        learner.clip_gradients(1e-3)
        assert np.isfinite(learner.grad_norm()) and learner.grad_norm() > 1e-3
    finally:
        dev.free()
        batch.free()
        learner.close()
