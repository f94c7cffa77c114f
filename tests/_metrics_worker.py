"""One rank of tests/test_gpu_ppo_metrics_multirank.py (not a test module):
  python tests/_metrics_worker.py RANK WORLD OUTDIR GLOBAL_ENVS
The fixture of tests/_learn_worker.py: every rank builds the same small learner, owns its shard of the
global env batch on device PP3_WORKER_DEVICE and its own PRNG key.  Saved into OUTDIR
  out4_R / stats_R   this rank's own four episode numbers of one train_iteration(comm=, episode_stats=)
                     and what the EpisodeStats accumulated (count, sum_reward, length, truncated)
  acc_R / eval_R     the accumulator [22][n] after one Evaluator(comm=comm).run_evaluation() and the 42
                     reported means and stds (out42's order), then eval/sps * eval/epoch_eval_time."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import common  # noqa: E402
import ppo_loss_ref as R  # noqa: E402
from pupperv3_mjx import evaluator, ppo, rng, sharding, wrappers  # noqa: E402
from pupperv3_mjx.environment import PupperV3Env  # noqa: E402
from test_gpu_ppo_learn import _dicts  # noqa: E402

K, L = 3, 3
rank, world, out, G = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
device = int(os.environ.get("PP3_WORKER_DEVICE", rank))
start, n = sharding.shard_bounds(G, world, rank)
comm = sharding.Comm(rank, world, device)
env = PupperV3Env(**common.fixture_kwargs(common.MODEL_XML, terminal_body_z=0.21, observation_history=2), num_envs=n,
                  device=device)
w = wrappers.wrap(env, episode_length=L)
case = R.random_case(6, K=1, B=2, in_dim=env.observation_size, hidden=(16, 8), activation="elu", with_normalizer=False)
pol, val = _dicts(case)
key = rng.split(rng.PRNGKey(12), world)[rank]


def save(name, a):
    np.save(os.path.join(out, f"{name}_{rank}.npy"), np.asarray(a))


learner = ppo.PPOLearner(pol, val, max_rows=(K + 1) * n, device=device)
actor, critic = learner.make_policies()
stats = ppo.EpisodeStats()
state = w.reset(sharding.shard_keys(3, G, world, rank))
learner.train_iteration(w, state, key, actor, critic, K, lr=1e-3, comm=comm, episode_stats=stats)
save("out4", stats.local_out4())
count, sums = stats.read()
assert count == int(stats.last[0])
save("stats", np.array([count, sums["sum_reward"], sums["length"], sums["truncated"]], np.float64))

ev = evaluator.Evaluator(w, actor, L, key=key, deterministic=False, comm=comm)
res = ev.run_evaluation()
save("acc", ev.accumulators())
names = evaluator.METRIC_NAMES
save("eval", np.array([res[f"eval/episode_{m}"] for m in names] + [res["eval/avg_episode_length"]] +
                      [res[f"eval/episode_{m}_std"] for m in names] + [res["eval/std_episode_length"]] +
                      [res["eval/sps"] * res["eval/epoch_eval_time"]], np.float64))
per_rank = ev.run_evaluation(aggregate_episodes=False)  # stays this rank's columns (both ranks still call it)
assert per_rank["eval/episode_reward"].shape == (n,)
ev.close()
stats.close()
actor.close(), critic.close(), learner.close()
comm.barrier()
env.close()
comm.close()
