"""The PPO metrics across rank processes on ONE GPU, through the loopback test transport (the fixture
of tests/test_gpu_ppo_multirank.py): tests/_metrics_worker.py is one rank.  (world, G) = (2, 12) gives
equal shards, (3, 10) the ragged 4 + 4 + 2.  What is held: the episode statistics a
train_iteration(comm=, episode_stats=) accumulates and the means and stds an Evaluator(comm=comm)
reports are bit-identical on every rank, equal the restatement (tests/ppo_metrics_ref.py) applied to
the ranks' saved pieces in rank order, and differ from each rank's own local numbers."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ppo_eval_ref as R
import ppo_metrics_ref as M
from pupperv3_mjx import sharding

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOOPBACK_LIB = os.path.join(HERE, "loopback", "libpupper_hip_loopback.so")
F, U = np.float32, np.uint32
K = 3


@pytest.fixture
def loopback_env(require_gpu, tmp_path):
    if not os.path.exists(LOOPBACK_LIB) or not os.path.exists(os.path.join(HERE, "loopback", "libpp3_loopback_rccl.so")):
        pytest.fail("loopback test build missing: make -C pupperv3-mjx_amd/csrc loopback (__graft_entry__.build)")
    d = tmp_path / "lb"
    d.mkdir()
    return dict(os.environ, PP3_LIB_PATH=LOOPBACK_LIB, PP3_ALLOW_DIAG_BUILD="1", PP3_LOOPBACK_DIR=str(d),
                PP3_RDZV_DIR=str(d), PP3_LAUNCH_ID=f"lbm{os.getpid()}.{tmp_path.name}", PP3_WORKER_DEVICE="0")


def _run_ranks(env, out, world, G, timeout=150.0):
    """Starts the rank processes (at most 3) and waits for all of them; the first rank that fails (or
    the time limit) ends the others at once, so none is left polling for a peer that is gone."""
    assert world <= 3
    worker = os.path.join(HERE, "_metrics_worker.py")
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
def test_metrics_are_summed_in_rank_order_and_identical_on_every_rank(loopback_env, tmp_path, world, G):
    codes = _run_ranks(loopback_env, tmp_path, world, G)
    assert codes == [0] * world, codes
    load = lambda name: [np.load(tmp_path / f"{name}_{r}.npy") for r in range(world)]  # noqa: E731
    shards = [sharding.shard_bounds(G, world, r)[1] for r in range(world)]
    if world == 3:
        assert shards == [4, 4, 2]

    # training episode statistics: the rank-ordered sum of the ranks' own four numbers, on every rank
    out4, stats = load("out4"), load("stats")
    want = M.sum_gathered(np.stack(out4))
    assert want[0] > 0 and all(o[0] > 0 for o in out4)  # every shard finished episodes
    for r in range(world):
        assert stats[r][0] == int(want[0])
        np.testing.assert_array_equal(stats[r][1:], want[1:].astype(np.float64), err_msg=f"rank {r}")
        assert np.any(stats[r] != out4[r].astype(np.float64)), r  # not the rank's own numbers

    # evaluation: the chain over the ranks' accumulators, on every rank; not the rank's own reduce
    acc, ev = load("acc"), load("eval")
    assert [a.shape for a in acc] == [(R.WORDS, s) for s in shards]
    want42 = M.eval_chain(acc)
    assert np.all(np.isfinite(want42)) and np.any(want42[:R.NCOL - 1] != 0)
    for r in range(world):
        np.testing.assert_array_equal(ev[r][:42].astype(F).view(U), want42.view(U), err_msg=f"rank {r}")
        assert ev[r][:42].astype(F).astype(np.float64).tolist() == ev[r][:42].tolist()  # (they were f32 values)
        assert round(ev[r][42] / K) == G  # eval/sps counts every rank's envs
        own = R.reduce(acc[r])
        assert own[R.NCOL - 1] != want42[R.NCOL - 1] and own[R.NOUT + R.NCOL - 1] != want42[R.NOUT + R.NCOL - 1], r
    whole = np.concatenate(acc, axis=1).astype(np.float64)
    np.testing.assert_allclose(want42[:R.NCOL], whole[:R.NCOL].mean(1), rtol=1e-5, atol=1e-6)
