"""Data-parallel PPO across rank processes on ONE GPU, through the loopback test transport (as
tests/test_gpu_multirank.py runs the env gather): tests/_learn_worker.py is one rank.

(world, G) = (2, 12) gives equal shards of 6 envs; (3, 10) gives sharding.shard_bounds' ragged
4 + 4 + 2, the smallest case where the order of three ranks and unequal row counts both matter.
What is held:
  * allreduce_gradients leaves, on every rank, exactly ppo_dp_ref.reduce_ranks of the ranks' local
    gradients and metrics (the header's rank-ordered f32 sum and division), bit for bit;
  * update_normalizer(env, comm) leaves the same bits on every rank, and they meet the project's
    normaliser parity rule against the f64 update on all ranks' rows (ppo_train_ref.normalizer_update):
    err = max |x - ref64| / max |ref64| <= 5 x the largest err of the f32 numpy statement of the ranks
    formula (ppo_dp_ref.normalizer_update_ranks) over 16 seeds at the same shard shapes, a seed being an
    order of those very rows (as in test_gpu_ppo_train_step.py: the env's observation columns decide the
    size of any f32 implementation's error, the f64 result does not depend on the order);
  * after a whole train_iteration(comm=...) parameters, gradients, Adam moments, statistics and metrics
    are bit-identical across ranks, and differ from the rank's own comm=None iteration from the same
    start, so the reduce did take place."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ppo_dp_ref as DP
import ppo_train_ref as T
from pupperv3_mjx import sharding

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOOPBACK_LIB = os.path.join(HERE, "loopback", "libpupper_hip_loopback.so")
F = np.float32
U = np.uint32
K = 3
NAMES = ("mean", "summed_variance", "std")


@pytest.fixture
def loopback_env(require_gpu, tmp_path):
    if not os.path.exists(LOOPBACK_LIB) or not os.path.exists(os.path.join(HERE, "loopback", "libpp3_loopback_rccl.so")):
        pytest.fail("loopback test build missing: make -C pupperv3-mjx_amd/csrc loopback (__graft_entry__.build)")
    d = tmp_path / "lb"
    d.mkdir()
    return dict(os.environ, PP3_LIB_PATH=LOOPBACK_LIB, PP3_ALLOW_DIAG_BUILD="1", PP3_LOOPBACK_DIR=str(d),
                PP3_RDZV_DIR=str(d), PP3_LAUNCH_ID=f"lbl{os.getpid()}.{tmp_path.name}", PP3_WORKER_DEVICE="0")


def _err(x, ref):
    num = float(np.abs(np.asarray(x, np.float64) - ref).max())
    return 0.0 if num == 0.0 else num / float(np.abs(ref).max())


def _run_ranks(env, out, world, G, timeout=150.0):
    """Starts the rank processes and waits for all of them; the first rank that fails (or the time
    limit) ends the others at once, so none is left polling for a peer that is gone."""
    worker = os.path.join(HERE, "_learn_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(out), str(G)], env=env)
             for r in range(world)]
    t0 = time.monotonic()
    try:
        while True:
            codes = [p.poll() for p in procs]
            if all(c is not None for c in codes) or any(c not in (None, 0) for c in codes):
                break
            if time.monotonic() - t0 > timeout:
                break
            time.sleep(0.02)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    return codes


@pytest.mark.parametrize("world,G", [(2, 12), (3, 10)])
def test_ranks_reduce_in_rank_order_and_stay_bit_identical(loopback_env, tmp_path, world, G):
    codes = _run_ranks(loopback_env, tmp_path, world, G)
    assert codes == [0] * world, codes
    load = lambda name: [np.load(tmp_path / f"{name}_{r}.npy") for r in range(world)]
    shards = [sharding.shard_bounds(G, world, r)[1] for r in range(world)]
    if world == 3:
        assert len(set(shards)) > 1  # ragged

    # gradients and metrics: the rank-ordered mean of the ranks' local ones, on every rank
    local, reduced = load("local"), load("reduced")
    assert all(np.any(local[0] != local[r]) for r in range(1, world))  # each rank had its own shard and key
    want = DP.reduce_ranks([a.view(F) for a in local])
    assert np.all(np.isfinite(want)) and np.any(want != 0)
    for r in range(world):
        np.testing.assert_array_equal(reduced[r], want.view(U), err_msg=f"rank {r}")

    # statistics: the same bits everywhere, and the parity rule against f64 on all rows
    norm, obs = load("norm"), load("obs")
    assert [o.shape[0] for o in obs] == [K * s for s in shards]
    for r in range(1, world):
        np.testing.assert_array_equal(norm[r].view(U), norm[0].view(U), err_msg=f"rank {r}")
    rows = np.concatenate(obs)
    D = rows.shape[1]
    _, mean0, sv0, _ = T.initial_state(D)
    ref = T.normalizer_update(rows, K * G, mean0, sv0)
    cuts = np.cumsum([K * s for s in shards])[:-1]
    bound = dict.fromkeys(NAMES, 0.0)
    for seed in range(16):
        perm = rows[np.random.RandomState(seed).permutation(K * G)]
        got32 = DP.normalizer_update_ranks(np.split(perm, cuts), K * G, *T.initial_state(D, F)[1:3], dtype=F)
        for k, a, b in zip(NAMES, got32, ref):
            bound[k] = max(bound[k], 5 * _err(a, b))
    for k, got, want64 in zip(NAMES, norm[0], ref):
        err = _err(got, want64)
        print(f"ranks normaliser ({world}, {G}) {k}: err {err:.3e} bound {bound[k]:.3e}")
        assert err <= bound[k], (k, err, bound[k])

    # one whole iteration: the replicas end bit-identical, and not where they end on their own
    end, plain = load("end"), load("plain")
    assert np.all(np.isfinite(end[0]))
    for r in range(1, world):
        np.testing.assert_array_equal(end[r].view(U), end[0].view(U), err_msg=f"rank {r}")
    for r in range(world):
        assert np.mean(end[r] != plain[r]) > 0.5, r
