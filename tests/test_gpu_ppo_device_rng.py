"""The PPO learner's random inputs drawn on the device (csrc/pp3_learn.hip): the entropy noise
(pp3_learner_draw_noise), one round of the shuffle (pp3_permute_by_bits), the env permutation
(pp3_learner_shuffle_env_index) and PPOLearner.train_iteration(device_rng=True).

The permutation, the ties and the wiring are compared bit for bit with pupperv3_mjx/rng.py.  The
noise's uniform is the host's bit for bit, so only erfinvf and one product are measured, against
sqrt(2) * erfinv(u) in float64 (scipy), err = |got - want| / (1 + |want|).  The bound follows
test_gpu_policy_sample.py's convention: 4 x the largest error measured on an MI355X over the cases of
test_noise_matches_the_f64_recipe, rounded up to one digit, under a ceiling of 1e-5 above which a
difference is a bug and not rounding."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import erfinv

import common
import ppo_loss_ref as R
from pupperv3_mjx import _abi, _lib, ppo, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_ppo_learn import _dicts, _learner

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
# measured on an MI355X over the six cases of test_noise_matches_the_f64_recipe: 1.72e-7 (the (5, 300)
# draw in the legacy layout; the figures per case are in that test's docstring); 4 x that = 6.9e-7,
# rounded up to one digit
NOISE_BOUND = 7e-7
NOISE_CEILING = 1e-5
assert NOISE_BOUND <= NOISE_CEILING


# ------------------------------------------------------------------------------ helpers
def _small_learner():
    case = R.random_case(0, K=1, B=2, in_dim=36, hidden=(8,), activation="tanh", with_normalizer=False)
    return _learner(case, max_rows=4)


def _download(L, ptr, shape, dtype=F):
    out = np.empty(shape, dtype)
    _lib.check(L.pp3_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
    return out


def _draw(L, learner, key, K, N, part):
    """pp3_learner_draw_noise on the default stream, downloaded: (f32 [K][N][12], device address)."""
    k = np.ascontiguousarray(np.asarray(key, U).reshape(2))
    out = C.c_void_p()
    rc = L.pp3_learner_draw_noise(learner._h, k.ctypes.data_as(C.c_void_p), K, N, part, C.byref(out), None)
    assert rc == 0, L.pp3_learn_last_error()
    return _download(L, out.value, (K, N, _abi.NU)), out.value


def _noise_want(key, shape, part):
    """sqrt(2) * erfinv(u) in float64 on jax's uniform (the host's bits)."""
    lo = np.nextafter(F(-1.0), F(0.0))
    return np.sqrt(2.0) * erfinv(rng.uniform(key, shape, lo, 1.0, bool(part)).astype(np.float64))


def _noise_err(got, want):
    return float((np.abs(got.astype(np.float64) - want) / (1.0 + np.abs(want))).max())


# ------------------------------------------------------------------------------ the permutation
SIZES = (1, 2, 3, 37, 64, 1625, 1626, 4096, 8192, 8193, 20000)


@pytest.mark.parametrize("part", [1, 0], ids=["partitionable", "legacy_layout"])
def test_shuffle_env_index_is_rng_permutation_bitwise(require_gpu, part):
    """Every size on one learner, ascending (the buffers grow) then descending (a larger allocation
    serves a smaller n); odd n in the legacy layout is the padded counter layout."""
    learner = _small_learner()
    try:
        for n in SIZES + SIZES[::-1]:
            key = rng.PRNGKey(100 + n)
            want = rng.permutation(key, n, bool(part))
            learner.shuffle_env_index(key, n, partitionable=part)
            got = learner.env_index()
            assert got.dtype == np.int32 and got.shape == (n,)
            np.testing.assert_array_equal(got, want, err_msg=f"n = {n}")
            learner.shuffle_env_index(rng.PRNGKey(7), n, partitionable=part)  # another key in between
            if n > 3:
                assert np.any(learner.env_index() != want)
            learner.shuffle_env_index(key, n, partitionable=part)
            np.testing.assert_array_equal(learner.env_index(), got, err_msg=f"n = {n}, second call")
        assert learner.rng_buffers()["index"][1] == 1
        assert learner.rng_buffers()["noise"] == (None, 0)
    finally:
        learner.close()


def test_shuffled_index_serves_the_indexed_loss_and_set_env_index_replaces_it(require_gpu):
    """The shuffle fills the buffer set_env_index fills, with its bookkeeping: the indexed loss runs
    behind either, with the same bits when the index is the same."""
    from test_gpu_ppo_train_step import _Arrays
    K, B, N, e0 = 2, 7, 24, 3
    case = R.random_case(0, K=K, B=N, in_dim=72, hidden=(40, 24), activation="elu", with_normalizer=True)
    learner = _learner(case, max_rows=(K + 1) * B)
    batch = _Arrays(case["batch"])
    key = rng.PRNGKey(5)
    try:
        with pytest.raises(_lib.PupperHipError):  # no index yet
            batch.run(learner, K, B, N, e0, case["hp"], True)
        learner.shuffle_env_index(key, N)
        assert learner.rng_buffers()["index"][1] == N
        got = batch.run(learner, K, B, N, e0, case["hp"], True)
        learner.set_env_index(rng.permutation(key, N))
        want = batch.run(learner, K, B, N, e0, case["hp"], True)
        learner.shuffle_env_index(key, N + 1)  # an index for another num_envs is refused, as set_env_index's is
        with pytest.raises(_lib.PupperHipError):
            batch.run(learner, K, B, N, e0, case["hp"], True)
    finally:
        batch.free()
        learner.close()
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------ ties
TIES = {
    "all_equal": lambda n: np.full(n, 0xDEADBEEF, U),
    "mod_3": lambda n: (np.arange(n) % 3).astype(U),
    "descending_pairs": lambda n: ((n - 1 - np.arange(n)) // 2).astype(U),
    "high_bit_pairs": lambda n: (((n - 1 - np.arange(n)) // 2) * 0x9E3779B1 % 2 ** 32).astype(U) | U(0x80000000),
}


@pytest.mark.parametrize("n", [5, 64, 1000, 8192, 8193])
@pytest.mark.parametrize("name", list(TIES))
def test_permute_by_bits_is_the_stable_argsort(require_gpu, name, n):
    L = require_gpu
    bits = TIES[name](n)
    assert len(np.unique(bits)) < n
    x = np.random.RandomState(n).permutation(n).astype(np.int32) * 3 - 7  # not the identity, not even indices
    want = x[np.argsort(bits, kind="stable")]
    bd, xd = _lib.DeviceBuffer(bits.nbytes), _lib.DeviceBuffer(x.nbytes)
    try:
        bd.upload(bits), xd.upload(x)
        assert L.pp3_permute_by_bits(0, bd.ptr, n, xd.ptr, None) == 0, L.pp3_learn_last_error()
        got = _download(L, xd.ptr.value, n, np.int32)
        np.testing.assert_array_equal(_download(L, bd.ptr.value, n, U), bits)  # bits are read only
    finally:
        bd.free(), xd.free()
    np.testing.assert_array_equal(got, want)
    if name == "all_equal":
        np.testing.assert_array_equal(got, x)


# ------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("part", [1, 0], ids=["partitionable", "legacy_layout"])
@pytest.mark.parametrize("K, N", [(1, 1), (3, 7), (5, 300)])
def test_noise_matches_the_f64_recipe(require_gpu, K, N, part):
    """Largest |got - want| / (1 + |want|) measured on an MI355X, partitionable / legacy layout:
    (1, 1) 5.26e-8 / 9.46e-8, (3, 7) 1.24e-7 / 1.04e-7, (5, 300) 1.63e-7 / 1.72e-7; NOISE_BOUND =
    4 x 1.72e-7 = 6.9e-7 rounded up to one digit = 7e-7.  (train_iteration's (3, 32) draw against the
    host path's rng.normal: 1.33e-7.)"""
    learner = _small_learner()
    try:
        key = rng.PRNGKey(31 + K)
        got, _ = _draw(require_gpu, learner, key, K, N, part)
        again, _ = _draw(require_gpu, learner, key, K, N, part)
        other, _ = _draw(require_gpu, learner, rng.PRNGKey(32 + K), K, N, part)
        assert learner.rng_buffers()["noise"][1] == K * N * _abi.NU
    finally:
        learner.close()
    err = _noise_err(got, _noise_want(key, (K, N, _abi.NU), part))
    print(f"noise ({K}, {N}) partitionable {part}: err {err:.3e} bound {NOISE_BOUND:.1e}")
    assert np.all(np.isfinite(got))
    np.testing.assert_array_equal(got.view(U), again.view(U))
    assert np.all(other != got) if K * N == 1 else np.mean(other != got) > 0.99
    assert err <= NOISE_BOUND, err
    # and against the host path itself (scipy's float64 erfinv rounded to f32), to the same bound
    host = rng.normal(key, (K, N, _abi.NU), bool(part))
    assert _noise_err(got, host.astype(np.float64)) <= NOISE_BOUND


def test_noise_word_i_depends_on_i_alone_in_the_partitionable_layout(require_gpu):
    """The flat prefix of a (3, 7) draw is the (1, 7) draw of the same key; in the legacy layout the
    counters pair up by the draw's size, so it is not."""
    learner = _small_learner()
    try:
        key = rng.PRNGKey(9)
        big, addr = _draw(require_gpu, learner, key, 3, 7, 1)
        small, addr2 = _draw(require_gpu, learner, key, 1, 7, 1)
        big0, _ = _draw(require_gpu, learner, key, 3, 7, 0)
        small0, _ = _draw(require_gpu, learner, key, 1, 7, 0)
        assert addr == addr2  # the buffer is reused, not grown
    finally:
        learner.close()
    np.testing.assert_array_equal(big[0].view(U), small[0].view(U))
    assert np.mean(big0[0] != small0[0]) > 0.9


# ------------------------------------------------------------------------------ train_iteration
def _setup(tmp_path, case, n, count=2, **learner_kw):
    path = common.write_model(tmp_path, 0)
    envs = [PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.21, observation_history=2), num_envs=n)
            for _ in range(count)]
    pol, val = _dicts(case)
    learners = [ppo.PPOLearner(pol, val, normalizer=case["normalizer"], max_rows=(case["K"] + 1) * n, **learner_kw)
                for _ in range(count)]
    handles = [l.make_policies() for l in learners]
    ws = [wrappers.wrap(e, episode_length=3) for e in envs]
    states = [w.reset(make_keys(3, n)) for w in ws]
    return envs, learners, handles, ws, states


def _teardown(envs, learners, handles):
    for h in handles:
        h[0].close(), h[1].close()
    for l in learners:
        l.close()
    for e in envs:
        e.close()


def _state_bits(learner):
    """Parameters and both Adam moments of both nets, as bits."""
    return np.concatenate([learner._download(net, which) for net in (0, 1) for which in (0, 2, 3)]).view(U)


def _metric_bits(metrics):
    return np.array([metrics[k] for k in ppo.METRICS], F).view(U)


def test_train_iteration_device_rng_draws_from_the_documented_keys(require_gpu, tmp_path):
    """32 envs, K = 3, 2 passes x 2 shuffled minibatches with the clip, device_rng on.  A second learner
    and env from the same seeds replay the iteration by hand from the captured noise and indices; the
    indices are rng.permutation of each pass's k_u and the noise is rng.normal(k_eps) to NOISE_BOUND."""
    n, K, D, lr, gmax = 32, 3, 72, 1e-4, 0.5
    case = R.random_case(6, K=K, B=n, in_dim=D, hidden=(64, 32), activation="elu", with_normalizer=True)
    envs, learners, handles, ws, states = _setup(tmp_path, case, n)
    A, B_ = learners
    indices, host_calls = [], []
    shuffle = A.shuffle_env_index
    A.shuffle_env_index = lambda *a, **kw: (shuffle(*a, **kw), indices.append(A.env_index()))[0]
    A.set_env_index = lambda *a, **kw: host_calls.append("set_env_index")
    A._eps_for = lambda *a, **kw: host_calls.append("_eps_for")
    noise = None
    try:
        key = rng.PRNGKey(12)
        _, metrics, _ = A.train_iteration(ws[0], states[0], key, *handles[0], K, num_minibatches=2,
                                          num_updates_per_batch=2, lr=lr, shuffle=True, max_grad_norm=gmax,
                                          device_rng=True)
        addr, cap = A.rng_buffers()["noise"]
        assert cap == K * n * _abi.NU and not host_calls and len(indices) == 2 and A.t == 4
        noise = _download(require_gpu, addr, (K, n, _abi.NU))
        # the keys of train_iteration's docstring
        k_collect, k_eps = rng.split(key, 2)
        k_perm = rng.split(k_eps, 2)[1]
        want_indices = []
        for _ in range(2):
            k_perm, k_u = rng.split(k_perm, 2)
            want_indices.append(rng.permutation(k_u, n))
        for got, want in zip(indices, want_indices):
            np.testing.assert_array_equal(got, want)
        assert np.any(indices[0] != indices[1])
        err = _noise_err(noise, rng.normal(k_eps, (K, n, _abi.NU)).astype(np.float64))
        print(f"train_iteration noise against rng.normal(k_eps): err {err:.3e}")
        assert err <= NOISE_BOUND, err
        # the replay by hand
        eps = _lib.DeviceBuffer(noise.nbytes)
        eps.upload(noise)
        try:
            ws[1].collect_ppo(states[1], *handles[1], K, k_collect)
            dev = ws[1].ppo_device_batch()
            B_._env = envs[1]
            stream = envs[1]._L.pp3_stream(envs[1]._h)
            for p in range(2):
                B_.set_env_index(indices[p])
                for mb in range(2):
                    B_.loss_and_grad_device(K, n // 2, n, mb * (n // 2), dev["observation"][0], dev["raw_action"][0],
                                            dev["log_prob"][0], dev["reward"][0], dev["done"][0], dev["truncation"][0],
                                            eps.ptr.value, stream, **ppo.HPARAMS, indexed=True)
                    B_.clip_gradients(gmax)
                    B_.adam_step(lr)
            B_.sync(*handles[1])
            want_metrics = B_.metrics()
            np.testing.assert_array_equal(_state_bits(A), _state_bits(B_))
            np.testing.assert_array_equal(_metric_bits(metrics), _metric_bits(want_metrics))
            assert A.grad_norm() == B_.grad_norm() and B_.t == 4
            start = np.concatenate([a.ravel() for kb in case["policy"] for a in kb])
            assert np.any(A._download(0, 0) != start)
            # one draw per (key, shape, env): the same key on the other env, whose stream the first
            # draw was not ordered on, draws again; a second call on that env does not
            draws = []
            draw = A.draw_entropy_noise
            A.draw_entropy_noise = lambda env, *a: (draws.append(env), draw(env, *a))[1]
            A.loss_and_grad(ws[0], 0, n // 2, k_eps, device_rng=True)
            assert not draws
            A.loss_and_grad(ws[1], 0, n // 2, k_eps, device_rng=True)
            A.loss_and_grad(ws[1], n // 2, n // 2, k_eps, device_rng=True)
            assert draws == [envs[1]]
            envs[1].synchronize()
            np.testing.assert_array_equal(_download(require_gpu, addr, (K, n, _abi.NU)).view(U), noise.view(U))
        finally:
            eps.free()
    finally:
        _teardown(envs, learners, handles)


def test_train_iteration_without_the_switch_is_the_host_path(require_gpu, tmp_path):
    """device_rng off (the default): the parameters, moments and metrics of the hand-chained host
    sequence (rng.permutation through set_env_index, rng.normal uploaded), bit for bit, and the
    learner owns no noise buffer afterwards."""
    n, K, lr, gmax = 32, 3, 1e-4, 0.5
    case = R.random_case(6, K=K, B=n, in_dim=72, hidden=(64, 32), activation="elu", with_normalizer=True)
    envs, learners, handles, ws, states = _setup(tmp_path, case, n)
    A, B_ = learners
    device_calls = []
    A.shuffle_env_index = lambda *a, **kw: device_calls.append("shuffle_env_index")
    A.draw_entropy_noise = lambda *a, **kw: device_calls.append("draw_entropy_noise")
    try:
        key = rng.PRNGKey(12)
        _, metrics, _ = A.train_iteration(ws[0], states[0], key, *handles[0], K, num_minibatches=2,
                                          num_updates_per_batch=2, lr=lr, shuffle=True, max_grad_norm=gmax)
        k_collect, k_eps = rng.split(key, 2)
        ws[1].collect_ppo(states[1], *handles[1], K, k_collect)
        k_perm = rng.split(k_eps, 2)[1]
        for _ in range(2):
            k_perm, k_u = rng.split(k_perm, 2)
            B_._env = envs[1]
            B_.set_env_index(rng.permutation(k_u, n))
            for mb in range(2):
                B_.loss_and_grad(ws[1], mb * (n // 2), n // 2, k_eps, indexed=True)
                B_.clip_gradients(gmax)
                B_.adam_step(lr)
        B_.sync(*handles[1])
        np.testing.assert_array_equal(_state_bits(A), _state_bits(B_))
        np.testing.assert_array_equal(_metric_bits(metrics), _metric_bits(B_.metrics()))
        assert not device_calls and A.t == B_.t == 4
        for l in learners:
            assert l.rng_buffers()["noise"] == (None, 0) and l._dev_eps is None
            assert l.rng_buffers()["index"][1] == n
    finally:
        _teardown(envs, learners, handles)
