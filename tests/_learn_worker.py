"""One rank of tests/test_gpu_ppo_multirank.py (not a test module):
  python tests/_learn_worker.py RANK WORLD OUTDIR GLOBAL_ENVS
Every rank builds the same small learner from the same seed, owns its shard of the global env batch
(sharding.shard_bounds) on device PP3_WORKER_DEVICE (the loopback transport: every rank on that
one device) and its own PRNG key, and saves into OUTDIR
  local_R / reduced_R   metrics and gradients of one loss_and_grad on its shard, before and after
                        allreduce_gradients
  obs_R / norm_R        the rows update_normalizer(env, comm) read, and the statistics after it
  end_R                 parameters, gradients, Adam moments, statistics and metrics after one
                        train_iteration(comm=comm): 1 minibatch, 2 passes, shuffle, clip, normaliser
  plain_R               the same after the same iteration from the same start with comm=None."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import common  # noqa: E402
import ppo_loss_ref as R  # noqa: E402
from pupperv3_mjx import _lib, ppo, rng, sharding, wrappers  # noqa: E402
from pupperv3_mjx.environment import PupperV3Env  # noqa: E402
from test_gpu_ppo_learn import _bits, _dicts  # noqa: E402

F = np.float32
K = 3
rank, world, out, G = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
device = int(os.environ.get("PP3_WORKER_DEVICE", rank))
start, n = sharding.shard_bounds(G, world, rank)
comm = sharding.Comm(rank, world, device)
env = PupperV3Env(**common.fixture_kwargs(common.MODEL_XML, terminal_body_z=0.21, observation_history=2), num_envs=n,
                  device=device)
w = wrappers.wrap(env, episode_length=3)
D = env.observation_size
case = R.random_case(6, K=1, B=2, in_dim=D, hidden=(16, 8), activation="elu", with_normalizer=False)  # every rank's seed
pol, val = _dicts(case)
key = rng.split(rng.PRNGKey(12), world)[rank]  # this rank's own key, as Brax gives each device its own
L = _lib.load()


def fresh():
    learner = ppo.PPOLearner(pol, val, running_statistics=True, max_rows=(K + 1) * n, device=device)
    return learner, learner.make_policies(), w.reset(sharding.shard_keys(3, G, world, rank))


def batch_observation():
    ptr, shape = w.ppo_device_batch()["observation"]
    env.synchronize()
    a = np.empty(shape, F)
    _lib.check(L.pp3_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes))
    return a


def save(name, a):
    np.save(os.path.join(out, f"{name}_{rank}.npy"), a)


def end_state(learner, metrics, rows):
    ns = learner.normalizer_state()
    assert ns["count"] == rows, (ns["count"], rows)
    return np.concatenate([learner._download(net, which) for net in (0, 1) for which in (0, 1, 2, 3)] +
                          [ns["mean"], ns["summed_variance"], ns["std"], np.array([metrics[k] for k in ppo.METRICS], F)])


# one loss and gradient, reduced; one statistics update
learner, (actor, critic), state = fresh()
k_collect, k_eps = rng.split(key, 2)
w.collect_ppo(state, actor, critic, K, k_collect)
learner.loss_and_grad(w, 0, n, k_eps)
save("local", _bits(learner.metrics(), learner.grads()))
learner.allreduce_gradients(comm)
save("reduced", _bits(learner.metrics(), learner.grads()))
save("obs", batch_observation().reshape(K * n, D))
learner.update_normalizer(w, comm)
ns = learner.normalizer_state()
assert ns["count"] == K * G, ns["count"]
save("norm", np.stack([ns["mean"], ns["summed_variance"], ns["std"]]))
actor.close(), critic.close(), learner.close()

# one whole iteration with the communicator, then the same from the same start without it
runs = {}
for name, c in (("end", comm), ("plain", None)):
    learner, (actor, critic), state = fresh()
    _, metrics, _ = learner.train_iteration(w, state, key, actor, critic, K, num_minibatches=1, num_updates_per_batch=2,
                                            lr=1e-3, shuffle=True, max_grad_norm=0.5, update_normalizer=True, comm=c)
    assert learner.t == 2
    runs[name] = (batch_observation(), end_state(learner, metrics, K * (n if c is None else G)))
    save(name, runs[name][1])
    actor.close(), critic.close(), learner.close()
# both iterations collected the same batch (the same start, old parameters, key): what differs after is the reduce
np.testing.assert_array_equal(runs["end"][0].view(np.uint32), runs["plain"][0].view(np.uint32))
comm.barrier()
env.close()
comm.close()
