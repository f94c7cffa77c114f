"""The learner across ranks in one process (csrc/pp3_learn.hip; the contract is the comment above
pp3_learner_allreduce_grads in include/pupper_hip.h): the rank-ordered reduce kernel at any world
size from a synthetic gathered buffer (pp3_learner_reduce_gathered), and the whole path -- pack,
all-gather, reduce; the normaliser's split finish -- over a ONE-rank RCCL communicator, where it must
leave every bit as the plain path leaves it.  Several ranks: tests/test_gpu_ppo_multirank.py."""
import ctypes as C
import os

import numpy as np
import pytest

import common
import ppo_dp_ref as DP
import ppo_loss_ref as R
from pupperv3_mjx import _abi, _lib, ppo, rng, sharding, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_gpu_ppo_learn import _Batch, _bits, _dicts, _learner
from test_gpu_ppo_train_step import _Norm, _norm_case, _small_learner

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32


@pytest.fixture(scope="module")
def comm(require_gpu, tmp_path_factory):
    os.environ["PP3_RDZV_DIR"] = str(tmp_path_factory.mktemp("rdzv"))
    c = sharding.Comm(0, 1, 0, tag="_ppo_ranks")
    yield c
    c.close()


def _ragged_learner():
    """in_dim 36, one hidden layer of 7: 451 policy and 267 value parameters, neither a multiple of 4
    (nor of a wave or a workgroup), so the blob boundaries fall inside a workgroup of the reduce."""
    case = R.random_case(0, K=1, B=2, in_dim=36, hidden=(7,), activation="tanh", with_normalizer=False)
    learner = _learner(case, max_rows=4)
    counts = [learner.buffer(net, 1)[1] for net in (0, 1)]
    assert counts == [37 * 7 + 8 * 24, 37 * 7 + 8] and all(c % 4 for c in counts)
    return learner, counts


def _grad_bits(L, learner, counts, metrics):
    out = [np.empty(c, F) for c in counts] + [np.empty(4, F)]
    for net in (0, 1):
        _lib.check(L.pp3_memcpy_d2h(out[net].ctypes.data_as(C.c_void_p), C.c_void_p(learner.buffer(net, 1)[0]),
                                    out[net].nbytes))
    metrics.download(out[2])
    return np.concatenate(out).view(U)


# ------------------------------------------------------------------------------ the reduce kernel
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_reduce_gathered_is_the_rank_ordered_sum_bitwise(require_gpu, world):
    L = require_gpu
    learner, counts = _ragged_learner()
    n0, n = counts[0], sum(counts)
    total = n + 4
    rs = np.random.RandomState(world)
    g = rs.normal(scale=10.0 ** rs.uniform(-3, 2, size=(world, total))).astype(F)
    # columns whose sum depends on the order of the ranks, at both ends of every piece
    marks = [0, 1, n0 - 1, n0, n0 + 1, n - 1, n, total - 1]
    pattern = np.array([1e8, 1.0, -1e8, 3.0, -1.0, 2.0 ** -20, -3e7, 1.0], F)
    for j, col in enumerate(marks):
        g[:, col] = np.roll(pattern, j)[:world]
    want = DP.reduce_ranks(list(g))
    if world >= 3:  # the marked columns do tell the orders apart
        exact = (g.astype(np.float64).sum(axis=0) / world).astype(F)
        assert np.any(want[marks] != exact[marks])
    src, metrics = _lib.DeviceBuffer(g.nbytes), _lib.DeviceBuffer(16)
    try:
        src.upload(g)
        got = []
        for _ in range(2):
            for net in (0, 1):  # poison: every output element is written by the call
                s = np.full(counts[net], np.nan, F)
                _lib.check(L.pp3_memcpy_h2d(C.c_void_p(learner.buffer(net, 1)[0]), s.ctypes.data_as(C.c_void_p), s.nbytes))
            metrics.upload(np.full(4, np.nan, F))
            assert L.pp3_learner_reduce_gathered(learner._h, src.ptr, world, metrics.ptr, None) == 0, \
                L.pp3_learn_last_error()
            got.append(_grad_bits(L, learner, counts, metrics))
    finally:
        src.free(), metrics.free(), learner.close()
    np.testing.assert_array_equal(got[0], want.view(U))
    np.testing.assert_array_equal(got[1], got[0])
    if world == 1:
        np.testing.assert_array_equal(got[0], g[0].view(U))


# ------------------------------------------------------------------------------ one-rank communicator
def test_allreduce_gradients_over_one_rank_changes_no_bit(require_gpu, comm):
    kw = dict(K=2, B=17, in_dim=72, hidden=(40, 24), activation="elu", with_normalizer=True)
    case = R.random_case(0, **kw)
    learner, batch = _learner(case), _Batch(case, 24, 3)
    try:
        before = _bits(*batch.run(learner, case["hp"]))
        learner.allreduce_gradients(comm)
        after = _bits(learner.metrics(), learner.grads())
        learner.allreduce_gradients(comm)  # and again, on the workspace the first call sized
        again = _bits(learner.metrics(), learner.grads())
    finally:
        batch.free(), learner.close()
    assert np.all(np.isfinite(before.view(F))) and np.any(before != 0)
    np.testing.assert_array_equal(after, before)
    np.testing.assert_array_equal(again, before)


def test_allgather_device_over_one_rank_copies_the_send(require_gpu, comm):
    a = np.random.RandomState(0).normal(size=1001).astype(F)
    send, recv = _lib.DeviceBuffer(a.nbytes), _lib.DeviceBuffer(a.nbytes)
    try:
        send.upload(a)
        recv.upload(np.full(a.size, np.nan, F))
        comm.allgather_device(send.ptr.value, recv.ptr.value, a.size)
        got = np.empty_like(a)
        recv.download(got)
        np.testing.assert_array_equal(got.view(U), a.view(U))
        for bad in ((None, recv.ptr.value, 4), (send.ptr.value, None, 4), (send.ptr.value, recv.ptr.value, 0)):
            with pytest.raises(_lib.PupperHipError):
                comm.allgather_device(*bad)
    finally:
        send.free(), recv.free()


@pytest.mark.parametrize("chained", [False, True], ids=["first", "chained"])
@pytest.mark.parametrize("rows, D", [(1, 36), (7, 72), (1025, 36)])
def test_normalizer_update_ranks_over_one_rank_is_the_plain_update_bitwise(require_gpu, comm, rows, D, chained):
    L = require_gpu
    x, count, mean, sv, std = _norm_case(0, rows, D, chained)
    learner = _small_learner(D)
    dev = _Norm(L, learner, x)
    try:
        want = dev.run(rows, count, mean, sv, std)
        got = []
        for _ in range(2):
            dev.state.upload(np.stack([np.asarray(a, F) for a in (mean, sv, std)]))
            a = list(dev.args(rows, count).values())
            assert L.pp3_learner_normalizer_update_ranks(a[0], comm._h, *a[1:]) == 0, L.pp3_learn_last_error()
            got.append(dev.get())
    finally:
        dev.free(), learner.close()
    assert np.all(np.isfinite(want)) and np.any(want[0] != np.asarray(mean, F))
    np.testing.assert_array_equal(got[0].view(U), want.view(U))
    np.testing.assert_array_equal(got[1].view(U), want.view(U))


def test_train_iteration_over_one_rank_ends_on_the_plain_path_bits(require_gpu, comm):
    """32 envs, K = 4, 2 passes over 2 shuffled minibatches, clip, running normaliser: with the
    one-rank communicator (statistics through the ranks path, allreduce_gradients before every clip)
    parameters, Adam moments and statistics end bit for bit where the plain call leaves them."""
    n, K = 32, 4
    case = R.random_case(6, K=K, B=n, in_dim=72, hidden=(64, 32), activation="elu", with_normalizer=False)
    kwargs = common.fixture_kwargs(common.MODEL_XML, terminal_body_z=0.21, observation_history=2)
    envs = [PupperV3Env(**kwargs, num_envs=n) for _ in range(2)]
    pol, val = _dicts(case)
    learners = [ppo.PPOLearner(pol, val, running_statistics=True, max_rows=(K + 1) * n) for _ in range(2)]
    handles = [l.make_policies() for l in learners]
    calls = []
    reduce = learners[1].allreduce_gradients
    learners[1].allreduce_gradients = lambda c, stream=None: calls.append(c) or reduce(c, stream)
    try:
        ws = [wrappers.wrap(e, episode_length=3) for e in envs]
        states = [w.reset(make_keys(3, n)) for w in ws]
        key = rng.PRNGKey(12)
        out = []
        for i, c in enumerate((None, comm)):
            _, metrics, _ = learners[i].train_iteration(ws[i], states[i], key, *handles[i], K, num_minibatches=2,
                                                        num_updates_per_batch=2, lr=1e-4, shuffle=True,
                                                        max_grad_norm=0.5, update_normalizer=True, comm=c)
            ns = learners[i].normalizer_state()
            assert ns["count"] == K * n
            out.append([np.array([metrics[k] for k in ppo.METRICS], F)] +
                       [learners[i]._download(net, which) for net in (0, 1) for which in (0, 1, 2, 3)] +
                       [ns["mean"], ns["std"], ns["summed_variance"]])
        assert len(calls) == 4 and all(c is comm for c in calls)
        assert learners[0].t == learners[1].t == 4
        assert np.any(out[0][1] != np.concatenate([a.ravel() for kb in case["policy"] for a in kb]))  # it trained
        for a, b in zip(*out):
            assert np.all(np.isfinite(a))
            np.testing.assert_array_equal(a.view(U), b.view(U))
    finally:
        for h in handles:
            h[0].close(), h[1].close()
        for l in learners:
            l.close()
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(require_gpu, comm):
    L = require_gpu
    nan, inf = float("nan"), float("inf")
    learner, counts = _ragged_learner()
    total = sum(counts) + 4
    dev = _Norm(L, learner, np.random.RandomState(0).normal(size=(10, 36)).astype(F))
    src, metrics = _lib.DeviceBuffer(4 * total * 2), _lib.DeviceBuffer(16)
    src.upload(np.ones(2 * total, F))
    SENT = F(-777.25)
    # the handle's first field is its device (struct pp3_learner, csrc/pp3_learn.hip): another value
    # there is a learner "on another device" for the argument check, which comes before any HIP call
    device_field = C.c_int.from_address(learner._h.value)
    assert device_field.value == 0
    try:
        def fill():
            for net in (0, 1):
                s = np.full(counts[net], SENT, F)
                _lib.check(L.pp3_memcpy_h2d(C.c_void_p(learner.buffer(net, 1)[0]), s.ctypes.data_as(C.c_void_p), s.nbytes))
            metrics.upload(np.full(4, SENT, F))
            dev.state.upload(np.full((3, 36), SENT, F))

        def untouched():
            return bool(np.all(_grad_bits(L, learner, counts, metrics).view(F) == SENT) and np.all(dev.get() == SENT))

        def refused(fn, args, name):
            assert fn(*args) == _abi.ERR_ARG, (name, args)
            assert name.encode() in L.pp3_learn_last_error(), L.pp3_learn_last_error()

        fill()
        h, c, m = learner._h, comm._h, metrics.ptr
        for args in ((None, c, m, None), (h, None, m, None), (h, c, None, None)):
            refused(L.pp3_learner_allreduce_grads, args, "pp3_learner_allreduce_grads")
        for args in ((None, src.ptr, 2, m, None), (h, None, 2, m, None), (h, src.ptr, 2, None, None),
                     (h, src.ptr, 0, m, None), (h, src.ptr, -1, m, None), (h, src.ptr, _abi.LEARN_MAX_WORLD + 1, m, None)):
            refused(L.pp3_learner_reduce_gathered, args, "pp3_learner_reduce_gathered")
        good = dict(dev.args(10, 10))
        good = {"h": good.pop("h"), "comm": c, **good}
        for change in (dict(h=None), dict(comm=None), dict(obs=None), dict(mean=None), dict(sv=None), dict(std=None),
                       dict(rows=0), dict(rows=-1), dict(count=nan), dict(count=inf), dict(count=9.0), dict(std_min=nan),
                       dict(std_max=inf), dict(std_min=0.0), dict(std_min=2.0, std_max=1.0)):
            refused(L.pp3_learner_normalizer_update_ranks, {**good, **change}.values(),
                    "pp3_learner_normalizer_update_ranks")
        device_field.value = 1
        try:
            assert L.pp3_comm_device(c) == 0
            refused(L.pp3_learner_allreduce_grads, (h, c, m, None), "pp3_learner_allreduce_grads")
            assert b"different devices" in L.pp3_learn_last_error()
            refused(L.pp3_learner_normalizer_update_ranks, good.values(), "pp3_learner_normalizer_update_ranks")
            assert b"different devices" in L.pp3_learn_last_error()
        finally:
            device_field.value = 0
        with pytest.raises(_lib.PupperHipError):
            learner._check(L.pp3_learner_allreduce_grads(h, None, m, None))
        assert untouched()
        # the good calls still run
        assert L.pp3_learner_reduce_gathered(h, src.ptr, 2, m, None) == 0
        got = _grad_bits(L, learner, counts, metrics).view(F)
        np.testing.assert_array_equal(got, np.ones(total, F))
        assert L.pp3_learner_allreduce_grads(h, c, m, None) == 0
        assert L.pp3_learner_normalizer_update_ranks(*good.values()) == 0
        np.testing.assert_array_equal(_grad_bits(L, learner, counts, metrics).view(F), np.ones(total, F))
        assert np.all(np.isfinite(dev.get())) and np.all(dev.get() != SENT)
    finally:
        dev.free(), src.free(), metrics.free(), learner.close()
