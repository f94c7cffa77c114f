"""The PPO learner on the device (csrc/pp3_learn.hip): pp3_ppo_loss_grad, pp3_adam_step,
pp3_policy_load_params and pupperv3_mjx.ppo.PPOLearner.

Parity rule (the project's "5 x the f32 oracle's own error", test_gpu_physics.py): for every
parameter tensor of both nets and the four metrics, err = max |x - ref64| / max |ref64| against the
float64 torch restatement (tests/ppo_loss_ref.py), and err <= 5 x the largest err of the SAME
restatement run in float32 on the CPU over 16 seeds at that shape, computed here.  The seeds are
the first (ascending from 0) whose float64 reference meets the conditions of
ppo_loss_ref.meets_conditions (kinks and clip boundaries kept 1e-4 / 1e-3 away, all four clip cases
present, std(adv) > 0); the device runs the first of them.  Adam's m and v, the NULL-normaliser
reload and the fused rollout on a reloaded handle are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import ppo_loss_ref as R
from pupperv3_mjx import _lib, export, ppo, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys

pytestmark = pytest.mark.gpu

F = np.float32


# ------------------------------------------------------------------------------ helpers
def _dicts(case, zero=False):
    """The case's nets in the converted-dict form (un-folded), optionally with all-zero weights."""
    def net(layers, **extra):
        n = len(layers)
        z = (lambda a: np.zeros_like(a)) if zero else (lambda a: a)
        return dict(in_shape=[None, case["in_dim"]], observation_history=case["in_dim"] // 36,
                    layers=[dict(type="dense", activation=case["activation"] if i < n - 1 else "linear",
                                 shape=[None, len(b)], weights=[z(k), z(b)]) for i, (k, b) in enumerate(layers)], **extra)
    hp = case["hp"]
    return (net(case["policy"], distribution=dict(type="normal_tanh", min_std=hp["min_std"], var_scale=hp["var_scale"])),
            net(case["value"]))


def _learner(case, max_rows=None):
    pol, val = _dicts(case)
    return ppo.PPOLearner(pol, val, normalizer=case["normalizer"],
                          max_rows=max_rows or (case["K"] + 1) * case["B"])


class _Batch:
    """The case's minibatch placed at envs [e0, e0 + B) of a batch of N envs on the device; every
    other env's rows are NaN (reading one poisons the result)."""
    NAMES = ("obs_all", "raw_action", "log_prob", "reward", "done", "truncation", "eps")

    def __init__(self, case, N, e0):
        self.K, self.B, self.N, self.e0 = case["K"], case["B"], N, e0
        self.bufs = {}
        for name in self.NAMES:
            a = case["batch"][name]
            full = np.full((a.shape[0], N) + a.shape[2:], np.nan, F)
            full[:, e0:e0 + self.B] = a
            self.bufs[name] = _lib.DeviceBuffer(full.nbytes)
            self.bufs[name].upload(full)

    def run(self, learner, hp):
        p = {k: b.ptr.value for k, b in self.bufs.items()}
        learner.loss_and_grad_device(self.K, self.B, self.N, self.e0, p["obs_all"], p["raw_action"], p["log_prob"],
                                     p["reward"], p["done"], p["truncation"], p["eps"], None,
                                     **{k: hp[k] for k in ppo.HPARAMS})
        return learner.metrics(), learner.grads()

    def free(self):
        for b in self.bufs.values():
            b.free()


def _bits(metrics, grads):
    return np.concatenate([np.array([metrics[k] for k in R.METRICS], F)] +
                          [a.ravel() for net in ("policy", "value") for kb in grads[net] for a in kb]).view(np.uint32)


# ------------------------------------------------------------------------------ gradient parity
SHIPPED = (256, 128, 128)
PARITY = {  # K, B, N, e0, in_dim, hidden, activation, normaliser, normalize_advantage
    "one_tile_relu": (3, 5, 8, 0, 36, (20,), "relu", True, True),
    "offset_stride_elu": (2, 17, 24, 3, 72, (40, 24), "elu", False, False),
    "row_chunk_plus_one_tanh": (1, ppo.ROW_CHUNK + 1, ppo.ROW_CHUNK + 4, 2, 36, (20,), "tanh", True, True),
    "no_hidden_layer": (3, 5, 8, 1, 36, (), "linear", False, True),
    "sigmoid": (3, 5, 8, 3, 36, (20,), "sigmoid", True, False),
    "linear_hidden": (2, 17, 17, 0, 36, (40, 24), "linear", True, True),
    "shipped_shape": (2, 24, 24, 0, 72, SHIPPED, "tanh", True, True),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_loss_and_gradients_match_the_f64_reference(require_gpu, name):
    K, B, N, e0, in_dim, hidden, act, norm, normadv = PARITY[name]
    found = R.cases_meeting_conditions(16, K=K, B=B, in_dim=in_dim, hidden=hidden, activation=act, with_normalizer=norm,
                                       normalize_advantage=normadv)
    bound = {}
    for case, (m64, g64, aux) in found:
        assert R.meets_conditions(case, aux)
        assert case["batch"]["done"].sum() >= 2 and case["batch"]["truncation"].sum() >= 1
        m32, g32, _ = R.reference(case, torch.float32)
        for k, e in R.tensor_errors(m32, g32, m64, g64).items():
            bound[k] = max(bound.get(k, 0.0), 5 * e)
    case, (m64, g64, _) = found[0]
    learner, batch = _learner(case), _Batch(case, N, e0)
    try:
        metrics, grads = batch.run(learner, case["hp"])
    finally:
        batch.free()
        learner.close()
    errs = R.tensor_errors(metrics, grads, m64, g64)
    for k in errs:
        print(f"{name} {k}: err {errs[k]:.3e} bound {bound[k]:.3e}")
    assert len(errs) == 4 + 4 * (len(hidden) + 1)
    bad = {k: (errs[k], bound[k]) for k in errs if not errs[k] <= bound[k]}
    assert not bad, bad


def test_two_calls_give_the_same_bits_and_gradients_are_overwritten(require_gpu):
    kw = dict(K=2, B=17, in_dim=72, hidden=(40, 24), activation="elu", with_normalizer=True)
    a, b = R.random_case(0, **kw), R.random_case(1, **kw)
    b["policy"], b["value"], b["normalizer"] = a["policy"], a["value"], a["normalizer"]
    learner, fresh = _learner(a), _learner(a)
    ba, bb = _Batch(a, 24, 3), _Batch(b, 20, 1)
    try:
        first = _bits(*ba.run(learner, a["hp"]))
        again = _bits(*ba.run(learner, a["hp"]))
        other = _bits(*bb.run(learner, a["hp"]))
        back = _bits(*ba.run(learner, a["hp"]))
        new = _bits(*ba.run(fresh, a["hp"]))
    finally:
        ba.free(), bb.free(), learner.close(), fresh.close()
    assert np.all(np.isfinite(first.view(F)))
    np.testing.assert_array_equal(first, again)
    assert np.mean(first != other) > 0.9
    np.testing.assert_array_equal(first, back)
    np.testing.assert_array_equal(first, new)


# ------------------------------------------------------------------------------ Adam
def test_adam_step_moments_bitwise_and_update_within_rounding(require_gpu):
    case = R.random_case(0, K=2, B=4, in_dim=36, hidden=(20,), activation="tanh", with_normalizer=False)
    learner = _learner(case)
    L = require_gpu
    lr, b1, b2, eps = 3e-4, 0.9, 0.999, 1e-8
    rs = np.random.RandomState(3)
    try:
        counts = [learner.buffer(net, 0)[1] for net in (0, 1)]
        assert counts == [37 * 20 + 21 * 24, 37 * 20 + 21] and all(c % 256 for c in counts)
        state = {net: dict(p=learner._download(net, 0), m=np.zeros(counts[net], F), v=np.zeros(counts[net], F))
                 for net in (0, 1)}
        for t in (1, 2, 3):
            g = {net: rs.normal(scale=10.0 ** rs.uniform(-4, 1, size=counts[net])).astype(F) for net in (0, 1)}
            for net in (0, 1):
                _lib.check(L.pp3_memcpy_h2d(C.c_void_p(learner.buffer(net, 1)[0]), g[net].ctypes.data_as(C.c_void_p),
                                            g[net].nbytes))
            learner.adam_step(lr, b1, b2, eps)
            assert learner.t == t
            for net in (0, 1):
                s = state[net]
                p_ref, m_ref, v_ref = R.adam(s["p"], g[net], s["m"], s["v"], lr, b1, b2, eps, t)
                p, m, v = (learner._download(net, w) for w in (0, 2, 3))
                np.testing.assert_array_equal(m.view(np.uint32), m_ref.view(np.uint32))
                np.testing.assert_array_equal(v.view(np.uint32), v_ref.view(np.uint32))
                c1, c2 = F(1.0 - b1 ** t), F(1.0 - b2 ** t)
                step = -(float(F(lr)) * (m.astype(np.float64) / c1)) / (np.sqrt(v.astype(np.float64) / c2) + float(F(eps)))
                got = p.astype(np.float64) - s["p"].astype(np.float64)
                tol = 16 * 2.0 ** -24 * np.abs(step) + np.spacing(np.abs(s["p"])).astype(np.float64)
                assert np.all(np.abs(got - step) <= tol), (t, net, float((np.abs(got - step) / tol).max()))
                assert np.abs(got).max() > 1e-5
                state[net] = dict(p=p, m=m, v=v)
    finally:
        learner.close()


# ------------------------------------------------------------------------------ reload
def _act_and_sample(dp, x, key):
    n = x.shape[0]
    out_dim = dp.out_dim
    bufs = [_lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(4 * n * out_dim)] + [_lib.DeviceBuffer(4 * n * w) for w in (12, 12, 1, 24)]

    def dl(buf, shape):
        a = np.zeros(shape, F)
        buf.download(a)
        return a

    try:
        bufs[0].upload(x)
        dp.act(bufs[0].ptr.value, x.shape[1], n, bufs[1].ptr.value, out_dim)
        out = {"act": dl(bufs[1], (n, out_dim))}
        if dp.distribution is not None:
            dp.sample(bufs[0].ptr.value, x.shape[1], n, key, bufs[2].ptr.value, 12, bufs[3].ptr.value, bufs[4].ptr.value,
                      bufs[5].ptr.value)
            out.update(action=dl(bufs[2], (n, 12)), raw=dl(bufs[3], (n, 12)), log_prob=dl(bufs[4], (n,)),
                       logits=dl(bufs[5], (n, 24)))
        return out
    finally:
        for b in bufs:
            b.free()


def test_reload_without_normaliser_is_a_fresh_handle_bit_for_bit(require_gpu):
    case = R.random_case(2, K=2, B=4, in_dim=72, hidden=(40, 24), activation="elu", with_normalizer=False)
    learner = _learner(case)
    x = np.random.RandomState(5).normal(size=(37, 72)).astype(F)
    key = rng.PRNGKey(7)
    handles = []
    try:
        for net in (0, 1):
            fresh = export.DevicePolicy(_dicts(case)[net])
            loaded = export.DevicePolicy(_dicts(case, zero=True)[net])
            handles += [fresh, loaded]
            before = _act_and_sample(loaded, x, key)
            assert np.all(before["act"] == 0)
            learner.sync(*((loaded, None) if net == 0 else (None, loaded)))
            want, got = _act_and_sample(fresh, x, key), _act_and_sample(loaded, x, key)
            assert set(got) == ({"act", "action", "raw", "log_prob", "logits"} if net == 0 else {"act"})
            for k in want:
                np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
            assert np.abs(got["act"]).max() > 1e-2
    finally:
        for h in handles:
            h.close()
        learner.close()


def _fold32(kernel, bias, mean, std):
    """The reload's layer 0 in f32 numpy (k ascending)."""
    k2 = (kernel / std[:, None]).astype(F)
    s = np.zeros(kernel.shape[1], F)
    for k in range(kernel.shape[0]):
        s = s + (mean[k] / std[k]) * kernel[k]
    return k2, (bias - s).astype(F)


def _forward(layers, act, x, dtype):
    h = x.astype(dtype)
    for i, (k, b) in enumerate(layers):
        h = h @ k.astype(dtype) + b.astype(dtype)
        if i < len(layers) - 1:
            h = export._act_np(h, act).astype(dtype)
    return h


def test_reload_with_normaliser_matches_the_f64_fold(require_gpu):
    """policy_forward on the f64 fold is the reference; the bound is 5 x the f32 numpy restatement's
    own error (fold and forward in f32) over 16 seeds at this shape."""
    kw = dict(K=2, B=4, in_dim=72, hidden=(40, 24), activation="elu", with_normalizer=True)
    n = 37
    bound = {0: 0.0, 1: 0.0}
    for seed in range(16):
        case = R.random_case(seed, **kw)
        x = np.random.RandomState(100 + seed).normal(size=(n, 72)).astype(F)
        for net, name in ((0, "policy"), (1, "value")):
            (k0, b0), rest = case[name][0], case[name][1:]
            ref = _forward([R.fold(k0, b0, *case["normalizer"])] + rest, "elu", x, np.float64)
            got = _forward([_fold32(k0, b0, *case["normalizer"])] + rest, "elu", x, F)
            bound[net] = max(bound[net], 5 * R.rel_err(got, ref))
        if seed == 0:
            first, x0 = case, x
    learner = _learner(first)
    handles = [export.DevicePolicy(d) for d in _dicts(first, zero=True)]
    try:
        learner.sync(*handles)
        for net, name in ((0, "policy"), (1, "value")):
            (k0, b0), rest = first[name][0], first[name][1:]
            ref = _forward([R.fold(k0, b0, *first["normalizer"])] + rest, "elu", x0, np.float64)
            got = _act_and_sample(handles[net], x0, rng.PRNGKey(1))
            for k in (("act", "logits") if net == 0 else ("act",)):
                err = R.rel_err(got[k], ref)
                print(f"reload {name} {k}: err {err:.3e} bound {bound[net]:.3e}")
                assert err <= bound[net], (name, k, err, bound[net])
    finally:
        for h in handles:
            h.close()
        learner.close()


@pytest.mark.parametrize("n", [16, 40])
def test_fused_sampled_rollout_runs_on_a_reloaded_handle(require_gpu, tmp_path, n):
    """pp3_rollout_policy_sample on a handle after pp3_policy_load_params equals the per-step path
    (pp3_policy_sample then step) bit for bit; n = 40 has the ragged last tile."""
    from test_gpu_policy_sample import _assert_same, _loop_reference
    case = R.random_case(4, K=2, B=4, in_dim=72, hidden=(64, 32), activation="elu", with_normalizer=True)
    path = common.write_model(tmp_path, 0)
    envs = [PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.25, observation_history=2), num_envs=n)
            for _ in range(2)]
    learner = _learner(case)
    dp = export.DevicePolicy(_dicts(case, zero=True)[0])
    try:
        assert envs[0]._L.pp3_rollout_policy_fused(envs[0]._h) == 1
        learner.sync(dp, None)
        envs[0].synchronize()  # (the reload ran on the default stream)
        ws = [wrappers.wrap(e, episode_length=5) for e in envs]
        s1, s2 = ws[0].reset(make_keys(2, n)), ws[1].reset(make_keys(2, n))
        key = rng.PRNGKey(9)
        s1, tr, k1 = ws[0].rollout_policy_sample(s1, dp, 8, key)
        s2, ref, k2 = _loop_reference(ws[1], envs[1], s2, dp, 8, key)
        _assert_same(tr, ref)
        np.testing.assert_array_equal(s1._record, s2._record)
        assert np.abs(tr["action"]).max() > 1e-2 and np.all(np.isfinite(tr["log_prob"]))
    finally:
        dp.close()
        learner.close()
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ the loop
def test_three_iterations_lower_the_loss_and_collect_on_reloaded_handles(require_gpu, tmp_path):
    """32 envs, K = 4, three times: collect, one loss_and_grad, adam_step (lr 1e-4), sync.  The first
    minibatch's total loss, re-evaluated by the f64 reference on the parameters after the first step,
    is lower than before it; each next collect_ppo runs on the reloaded handles (its values are the
    trained critic's)."""
    n, K = 32, 4
    case = R.random_case(5, K=K, B=n, in_dim=72, hidden=(64, 32), activation="elu", with_normalizer=True)
    path = common.write_model(tmp_path, 0)
    env = PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.21, observation_history=2), num_envs=n)
    learner = _learner(case)
    actor, critic = learner.make_policies()
    hp = dict(ppo.HPARAMS)
    try:
        w = wrappers.wrap(env, episode_length=3)
        state = w.reset(make_keys(2, n))
        key = rng.PRNGKey(11)
        totals = []
        for it in range(3):
            k_collect, k_eps, key = rng.split(key, 3)
            state, batch, _ = w.collect_ppo(state, actor, critic, K, k_collect)
            batch = {k: np.array(v) for k, v in batch.items()}
            # the critic that collected is the learner's current one, folded
            vparams = learner.params()["value"]
            (k0, b0), rest = vparams[0], vparams[1:]
            want = _forward([R.fold(k0, b0, *case["normalizer"])] + rest, "elu", batch["observation"].reshape(K * n, 72),
                            np.float64)[:, 0]
            assert np.all(np.abs(batch["value"].ravel() - want) <= 2e-5 * (1 + np.abs(want))), it
            learner.loss_and_grad(w, 0, n, k_eps, **hp)
            m = learner.metrics()
            host = dict(obs_all=np.concatenate([batch["observation"], batch["obs"][-1:]]), raw_action=batch["raw_action"],
                        log_prob=batch["log_prob"], reward=batch["reward"], done=batch["done"],
                        truncation=batch["truncation"], eps=rng.normal(k_eps, (K, n, 12), env._partitionable))
            before = learner.params()
            ref_before = R.loss_and_grad(before["policy"], before["value"], "elu", host, torch.float64, case["normalizer"],
                                         **hp)[0]["total_loss"]
            assert abs(m["total_loss"] - ref_before) <= 1e-4 * (1 + abs(ref_before)), (m, ref_before)
            learner.adam_step(1e-4)
            learner.sync(actor, critic)
            after = learner.params()
            ref_after = R.loss_and_grad(after["policy"], after["value"], "elu", host, torch.float64, case["normalizer"],
                                        **hp)[0]["total_loss"]
            totals.append((ref_before, ref_after))
            assert any(np.any(a[0] != b[0]) for a, b in zip(before["value"], after["value"]))
        print("total loss before / after each step:", totals)
        assert totals[0][1] < totals[0][0], totals
        assert learner.t == 3
    finally:
        actor.close(), critic.close(), learner.close(), env.close()


def test_train_iteration_runs_minibatches_and_reloads(require_gpu, tmp_path):
    """PPOLearner.train_iteration twice: 2 updates x 2 contiguous minibatches each (4 Adam steps per
    iteration), one upload of the entropy noise per iteration, handles reloaded with what was trained."""
    n, K = 32, 4
    case = R.random_case(6, K=K, B=n, in_dim=72, hidden=(64, 32), activation="elu", with_normalizer=True)
    path = common.write_model(tmp_path, 0)
    env = PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.21, observation_history=2), num_envs=n)
    learner = _learner(case)
    actor, critic = learner.make_policies()
    try:
        w = wrappers.wrap(env, episode_length=3)
        state = w.reset(make_keys(3, n))
        key = rng.PRNGKey(12)
        start = learner.params()
        noise = []
        for it in range(2):
            state, metrics, key = learner.train_iteration(w, state, key, actor, critic, K, num_minibatches=2,
                                                          num_updates_per_batch=2, lr=1e-4)
            assert set(metrics) == set(ppo.METRICS) and all(np.isfinite(v) for v in metrics.values()), metrics
            assert learner.t == 4 * (it + 1)
            noise.append(learner._eps[0])
        assert noise[0] != noise[1]  # a new key's noise per iteration, shared by its minibatches
        end = learner.params()
        for net in ("policy", "value"):
            assert all(np.any(a[0] != b[0]) and np.all(np.isfinite(b[0])) for a, b in zip(start[net], end[net]))
        # the handles hold the trained, folded networks
        x = np.random.RandomState(8).normal(size=(19, 72)).astype(F)
        for name, handle in (("policy", actor), ("value", critic)):
            (k0, b0), rest = end[name][0], end[name][1:]
            want = _forward([R.fold(k0, b0, *case["normalizer"])] + rest, "elu", x, np.float64)
            got = _act_and_sample(handle, x, rng.PRNGKey(1))["act"]
            assert np.all(np.abs(got - want) <= 2e-5 * (1 + np.abs(want))), name
        with pytest.raises(ValueError):
            learner.train_iteration(w, state, key, actor, critic, K, num_minibatches=5)
    finally:
        actor.close(), critic.close(), learner.close(), env.close()


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(require_gpu):
    L = require_gpu
    case = R.random_case(0, K=3, B=5, in_dim=36, hidden=(20,), activation="tanh", with_normalizer=True)
    learner = _learner(case, max_rows=20)
    batch = _Batch(case, 8, 0)
    other = export.DevicePolicy(_dicts(R.random_case(0, K=3, B=5, in_dim=36, hidden=(24,), activation="tanh",
                                                     with_normalizer=True))[0])
    SENT = F(-777.25)
    try:
        for net in (0, 1):  # gradients and metrics hold a sentinel no refused call may touch
            ptr, cnt = learner.buffer(net, 1)
            s = np.full(cnt, SENT, F)
            _lib.check(L.pp3_memcpy_h2d(C.c_void_p(ptr), s.ctypes.data_as(C.c_void_p), s.nbytes))
        learner._metrics.upload(np.full(4, SENT, F))
        p = {k: C.c_void_p(b.ptr.value) for k, b in batch.bufs.items()}
        mean, std = learner._norm_ptrs()
        good = dict(h=learner._h, K=3, B=5, N=8, e0=0, obs_all=p["obs_all"], raw_action=p["raw_action"],
                    log_prob=p["log_prob"], reward=p["reward"], done=p["done"], truncation=p["truncation"], eps=p["eps"],
                    mean=mean, std=std, discount=0.97, lam=0.95, scaling=1.0, clip=0.3, ent=0.01, norm=1,
                    metrics=learner._metrics.ptr, stream=None)
        bad = [dict(h=None), dict(obs_all=None), dict(raw_action=None), dict(log_prob=None), dict(reward=None),
               dict(done=None), dict(truncation=None), dict(eps=None), dict(metrics=None), dict(mean=None),
               dict(B=0), dict(K=0), dict(e0=4), dict(e0=-1), dict(N=4), dict(K=4), dict(B=6, N=9),
               dict(discount=float("nan")), dict(lam=float("inf")), dict(scaling=float("nan")), dict(ent=float("inf")),
               dict(clip=0.0), dict(clip=-0.1), dict(clip=float("nan"))]
        for change in bad:
            a = {**good, **change}
            rc = L.pp3_ppo_loss_grad(*a.values())
            assert rc == 1, change
            assert b"pp3_ppo_loss_grad" in L.pp3_learn_last_error()
        for args in ((float("nan"), 0.9, 0.999, 1e-8, 0.1, 0.001), (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.001),
                     (1e-3, 0.9, 0.999, 1e-8, 0.1, -1.0), (1e-3, float("inf"), 0.999, 1e-8, 0.1, 0.001)):
            assert L.pp3_adam_step(learner._h, *args, None) == 1, args
        # a handle of another shape
        in_dim, outs, _ = learner._shapes[0]
        before = _act_and_sample(other, np.ones((3, 36), F), rng.PRNGKey(0))["act"]
        rc = L.pp3_policy_load_params(other._h, C.c_void_p(learner.buffer(0, 0)[0]), in_dim, len(outs),
                                      outs.ctypes.data_as(C.c_void_p), mean, std, None)
        assert rc == 1 and b"shape" in L.pp3_learn_last_error()
        np.testing.assert_array_equal(_act_and_sample(other, np.ones((3, 36), F), rng.PRNGKey(0))["act"], before)
        for net in (0, 1):
            assert np.all(learner._download(net, 1) == SENT)
            assert np.all(learner._download(net, 0) == np.concatenate([a.ravel() for kb in case[("policy", "value")[net]]
                                                                       for a in kb]))
        got = np.zeros(4, F)
        learner._metrics.download(got)
        assert np.all(got == SENT)
        # the good call still runs
        assert L.pp3_ppo_loss_grad(*good.values()) == 0
        assert np.all(np.isfinite(learner._download(0, 1))) and np.all(learner._download(0, 1) != SENT)
        with pytest.raises(_lib.PupperHipError):
            learner.loss_and_grad_device(3, 5, 8, 4, *(b.ptr.value for b in batch.bufs.values()))
    finally:
        other.close()
        batch.free()
        learner.close()
