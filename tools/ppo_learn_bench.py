"""Cost of the PPO learner step at the training shape (4096 envs, K = 20, after 200 warm-up steps),
between device events, medians over `--repeat` alternating rounds with the run-to-run spread
(min .. max) beside them:
  (a) pp3_ppo_loss_grad + pp3_adam_step on one 256-env minibatch (5,120 rows) and on the whole
      batch (81,920 rows), actor 72 -> 256 -> 128 -> 128 -> 24 and critic .. -> 1, elu;
  (b) the reload of both handles (pp3_policy_load_params);
  (c) reference 1: the sampled rollout of the same run (pp3_rollout_policy_sample_timed, K steps);
  (d) reference 2, the yardstick for time: the same loss and gradient by torch eager autograd in
      f32 on the same device and rows (tests/ppo_loss_ref.py `loss`, no optimiser step);
  (e) the rest of training_step: pp3_learner_normalizer_update over the batch's K * envs rows (with the
      GB/s of its two sweeps) beside the same update in torch eager f32 on the same rows; pp3_grad_clip
      below the bound (norm only) and above it (norm and scaling); (a) through
      pp3_ppo_loss_grad_indexed on a permutation of the envs.  Skipped on a library without them.
"plain_grad_crc32" / "rollout_crc32" (the first plain loss's gradients and metrics; an untimed
  (f) across ranks, on this one GPU: pp3_learner_allreduce_grads over a ONE-rank RCCL communicator (pack,
      all-gather, reduce kernel); the reduce kernel alone on a resident [8][count] buffer
      (pp3_learner_reduce_gathered, world 8); pp3_learner_normalizer_update_ranks over the same
      communicator beside (e)'s update without one; in rounds of their own after those of (a)-(e), each
      also as a share of (a)'s minibatch step and of (c).  RCCL between devices is not measured here.
      Skipped on a library without them.
  (g) the iteration's random inputs, in rounds of their own after those of (f): pp3_learner_draw_noise of
      [K][envs][12] and pp3_learner_shuffle_env_index of `envs` between device events, each also as a
      share of the sampled rollout timed in the same rounds; the host time (wall clock) of rng.normal
      and rng.permutation at those shapes and of train_iteration's scalar key splits at one update
      pass; the whole PPOLearner.train_iteration(shuffle=True, num_minibatches=envs / minibatch) in
      wall-clock ms from call to return (its closing metrics() waits for the device) with device_rng
      off and on, alternating.  Skipped on a library without them.
rollout's outputs) compare the plain path's result bits between two builds (PP3_LIB_PATH).
One child process under a time limit.

  python tools/ppo_learn_bench.py [--envs 4096 --warmup 200 --steps 20 --minibatch 256 --repeat 9 --timeout 300]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd"), os.path.join(ROOT, "tests")]


def child(E: int, W: int, K: int, MB: int, R: int) -> None:
    from collections import OrderedDict
    from types import SimpleNamespace

    import zlib

    import numpy as np
    import torch

    import bench
    import ppo_loss_ref as ref
    from pupperv3_mjx import MODEL_XML, _abi, _lib, export, ppo, rng
    from pupperv3_mjx.environment import PupperV3Env

    env = PupperV3Env(**bench.bench_kwargs(MODEL_XML), num_envs=E, device=0, pipeline_output=False)
    L = env._L
    raw_lib = _lib.load()  # (the HIP runtime's event calls resolve through the library's handle)
    st = env.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(0), E)))
    _lib.check(L.pp3_set_auto_reset(env._h, 1000))
    D = env.observation_size
    rs = np.random.RandomState(7)

    def net(last):
        sizes = [D, 256, 128, 128, last]
        layers = OrderedDict((f"hidden_{i}", {"kernel": rs.normal(scale=1 / np.sqrt(sizes[i]), size=(sizes[i], sizes[i + 1])),
                                              "bias": np.zeros(sizes[i + 1])}) for i in range(len(sizes) - 1))
        return (SimpleNamespace(mean=np.zeros(D), std=np.ones(D)), {"params": layers})

    pdict = export.convert_training_params(net(2 * _abi.NU), "elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12),
                                           True, env._observation_history, 30.0, 30.0)
    vdict = export.convert_value_params(net(1), "elu", env._observation_history)
    normalizer = (rs.normal(scale=0.1, size=D).astype(np.float32), rs.uniform(0.5, 2.0, size=D).astype(np.float32))
    learner = ppo.PPOLearner(pdict, vdict, normalizer=normalizer, max_rows=(K + 1) * E)
    actor, critic = learner.make_policies()
    key = np.array(rng.PRNGKey(1), dtype=np.uint32)
    for w0 in range(0, W, K):  # (in unrolls of K: the trajectory each one returns stays small)
        st, _, key = env.rollout_policy_sample(st, actor, min(K, W - w0), key)
    st, batch, key = env.collect_ppo(st, actor, critic, K, key)
    k_eps = rng.PRNGKey(2)
    stream = C.c_void_p(L.pp3_stream(env._h))
    ms = C.c_float()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert raw_lib.hipEventCreate(C.byref(e)) == 0

    def timed(fn):
        assert raw_lib.hipEventRecord(ev[0], stream) == 0
        fn()
        assert raw_lib.hipEventRecord(ev[1], stream) == 0
        assert raw_lib.hipEventSynchronize(ev[1]) == 0
        assert raw_lib.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return ms.value

    def step(B, indexed=False):
        learner.loss_and_grad(env, 0, B, k_eps, indexed=indexed)
        learner.adam_step(3e-4)

    def crc(*arrays):
        c = 0
        for a in arrays:
            c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
        return c

    # the same rows for torch: its own copies on the same device
    dev = torch.device("cuda:0")
    eps = rng.normal(k_eps, (K, E, 12), env._partitionable)
    host = dict(obs_all=np.concatenate([batch["observation"], batch["obs"][-1:]]), raw_action=batch["raw_action"],
                log_prob=batch["log_prob"], reward=batch["reward"], done=batch["done"], truncation=batch["truncation"], eps=eps)
    tb = {B: {k: torch.tensor(np.ascontiguousarray(v[:, :B]), device=dev) for k, v in host.items()} for B in (MB, E)}
    tnorm = tuple(torch.tensor(a, device=dev) for a in normalizer)
    cur = learner.params()
    tparams = {name: [(torch.tensor(k, device=dev, requires_grad=True), torch.tensor(b, device=dev, requires_grad=True))
                      for k, b in cur[name]] for name in ("policy", "value")}
    flat = [p for name in ("policy", "value") for kb in tparams[name] for p in kb]
    tev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def torch_step(B):
        tev[0].record()
        m, _ = ref.loss(tparams["policy"], tparams["value"], "elu", tb[B], torch.float32, tnorm, **ppo.HPARAMS)
        grads = torch.autograd.grad(m["total_loss"], flat)
        tev[1].record()
        tev[1].synchronize()
        return tev[0].elapsed_time(tev[1]), float(m["total_loss"]), grads

    # parity of what is timed: the two compute the same loss
    learner.loss_and_grad(env, 0, MB, k_eps)
    ours = learner.metrics()["total_loss"]
    plain_crc = crc(np.array(list(learner.metrics().values()), np.float32), learner._download(0, 1), learner._download(1, 1))
    _, theirs, _ = torch_step(MB)
    act, raw = _lib.DeviceBuffer(4 * K * E * 12), _lib.DeviceBuffer(4 * K * E * 12)
    logp, rew, done = (_lib.DeviceBuffer(4 * K * E) for _ in range(3))
    obs = _lib.DeviceBuffer(4 * K * E * D)
    kin, kout = np.array(key, dtype=np.uint32), np.zeros(2, dtype=np.uint32)

    def rollout():
        _lib.check(L.pp3_rollout_policy_sample_timed(env._h, actor._h, K, kin.ctypes.data_as(C.c_void_p),
                                                     kout.ctypes.data_as(C.c_void_p), act.ptr, raw.ptr, logp.ptr, rew.ptr,
                                                     done.ptr, obs.ptr, C.byref(ms)))
        return ms.value

    rollout()
    got_bufs = []
    for buf, count in ((act, K * E * 12), (raw, K * E * 12), (logp, K * E), (rew, K * E), (done, K * E), (obs, K * E * D)):
        a = np.empty(count, np.float32)
        buf.download(a)
        got_bufs.append(a)
    rollout_crc = crc(*got_bufs)

    # the rest of training_step (a library with the entry points): the normaliser on a state of its
    # own, the clip on the gradients the step before it left, the indexed loss on a permutation
    extra = hasattr(raw_lib, "pp3_grad_clip")
    rows = K * E
    obs_ptr = env.ppo_device_batch()["observation"][0]
    nstate = _lib.DeviceBuffer(12 * D)
    nstate.upload(np.stack([np.zeros(D), np.zeros(D), np.ones(D)]).astype(np.float32))
    ncount = [0]

    def norm_update():
        ncount[0] += rows
        b = nstate.ptr.value
        rc = raw_lib.pp3_learner_normalizer_update(learner._h, C.c_void_p(obs_ptr), rows, float(np.float32(ncount[0])), 1e-6,
                                                   1e6, C.c_void_p(b), C.c_void_p(b + 4 * D), C.c_void_p(b + 8 * D), stream)
        assert rc == 0, raw_lib.pp3_learn_last_error()

    tx = tb[E]["obs_all"][:K].reshape(rows, D)
    tstate = [torch.zeros(D, device=dev), torch.zeros(D, device=dev), 0]

    def torch_norm():
        tev[0].record()
        mean, sv, count = tstate
        count += rows
        d = tx - mean
        mean2 = mean + d.sum(0) / count
        sv2 = sv + (d * (tx - mean2)).sum(0)
        std = torch.clamp(torch.sqrt(torch.clamp(sv2, min=0) / count), 1e-6, 1e6)
        tev[1].record()
        tev[1].synchronize()
        tstate[:] = [mean2, sv2, count]
        return tev[0].elapsed_time(tev[1]), mean2, std

    norm_check = None
    if extra:
        timed(norm_update)
        first = np.empty((3, D), np.float32)
        nstate.download(first)
        _, tmean, tstd = torch_norm()
        norm_check = {"mean": float(np.abs(first[0] - tmean.cpu().numpy()).max() / np.abs(first[0]).max()),
                      "std": float(np.abs(first[2] - tstd.cpu().numpy()).max() / np.abs(first[2]).max())}
        learner._env = env
        learner.set_env_index(rng.permutation(rng.PRNGKey(3), E))

    # across ranks: a one-rank communicator (made after the rounds of (a)-(e), which so run in the process
    # they ran in before), a resident [8][count] buffer, a normaliser state of its own
    ranks = extra and hasattr(raw_lib, "pp3_learner_allreduce_grads")
    if ranks:
        from pupperv3_mjx import sharding
        comm = None
        count = learner.buffer(0, 1)[1] + learner.buffer(1, 1)[1] + 4
        gathered = _lib.DeviceBuffer(4 * 8 * count)
        gathered.upload(rs.normal(scale=1e-2, size=(8, count)).astype(np.float32))
        rmetrics = _lib.DeviceBuffer(16)
        rstate = _lib.DeviceBuffer(12 * D)
        rstate.upload(np.stack([np.zeros(D), np.zeros(D), np.ones(D)]).astype(np.float32))
        rcount = [0]

        def reduce8():
            rc = raw_lib.pp3_learner_reduce_gathered(learner._h, gathered.ptr, 8, rmetrics.ptr, stream)
            assert rc == 0, raw_lib.pp3_learn_last_error()

        def norm_update_ranks():
            rcount[0] += rows
            b = rstate.ptr.value
            rc = raw_lib.pp3_learner_normalizer_update_ranks(
                learner._h, comm._h, C.c_void_p(obs_ptr), rows, float(np.float32(rcount[0])), 1e-6, 1e6, C.c_void_p(b),
                C.c_void_p(b + 4 * D), C.c_void_p(b + 8 * D), stream)
            assert rc == 0, raw_lib.pp3_learn_last_error()

    names = ("learn_minibatch_ms", "learn_batch_ms", "reload_ms", "rollout_ms", "torch_minibatch_ms", "torch_batch_ms")
    if extra:
        names += ("norm_update_ms", "torch_norm_ms", "clip_norm_only_ms", "clip_scale_ms", "learn_minibatch_indexed_ms",
                  "learn_batch_indexed_ms")
    out = {k: [] for k in names}
    for r in range(R + 2):  # rounds 0 and 1 warm every shape up
        got = dict(learn_minibatch_ms=timed(lambda: step(MB)), torch_minibatch_ms=torch_step(MB)[0],
                   learn_batch_ms=timed(lambda: step(E)), torch_batch_ms=torch_step(E)[0],
                   reload_ms=timed(lambda: learner.sync(actor, critic)), rollout_ms=rollout())
        if extra:
            got.update(norm_update_ms=timed(norm_update), torch_norm_ms=torch_norm()[0],
                       learn_minibatch_indexed_ms=timed(lambda: step(MB, True)),
                       learn_batch_indexed_ms=timed(lambda: step(E, True)),
                       clip_norm_only_ms=timed(lambda: learner.clip_gradients(1e30)),
                       clip_scale_ms=timed(lambda: learner.clip_gradients(1e-3)))
        if r >= 2:
            for k, v in got.items():
                out[k].append(round(v, 4))
    if ranks:  # (f): its own alternating rounds, the plain update again beside the ranks one
        comm = sharding.Comm(0, 1, 0, tag=f"_learn_bench{os.getpid()}")
        rnames = ("allreduce_one_rank_ms", "norm_update_ranks_ms", "norm_update_beside_ranks_ms", "reduce_world8_ms")
        out.update({k: [] for k in rnames})
        for r in range(R + 2):
            learner.loss_and_grad(env, 0, MB, k_eps)  # (the world-8 reduce overwrote the gradients)
            got = dict(allreduce_one_rank_ms=timed(lambda: learner.allreduce_gradients(comm)),
                       norm_update_ranks_ms=timed(norm_update_ranks), norm_update_beside_ranks_ms=timed(norm_update),
                       reduce_world8_ms=timed(reduce8))
            if r >= 2:
                for k, v in got.items():
                    out[k].append(round(v, 4))
    device_rng = hasattr(raw_lib, "pp3_learner_draw_noise")
    if device_rng:  # (g): its own alternating rounds after all of the above, which so run as they ran before
        import time
        gnames = ("draw_noise_ms", "shuffle_ms", "rollout_beside_draws_ms", "host_normal_ms", "host_permutation_ms",
                  "host_key_splits_ms", "train_iteration_host_rng_ms", "train_iteration_device_rng_ms")
        out.update({k: [] for k in gnames})
        learner._env = env
        part = env._partitionable

        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def key_splits(k):  # train_iteration's host key work at one update pass
            _, k_eps2 = rng.split(k, 2, part)
            rng.split(rng.split(k_eps2, 2, part)[1], 2, part)

        tkey = [np.array(rng.PRNGKey(4), dtype=np.uint32)]
        tstate = [st]

        def iteration(on):
            tstate[0], _, tkey[0] = learner.train_iteration(env, tstate[0], tkey[0], actor, critic, K, num_minibatches=E // MB,
                                                            shuffle=True, device_rng=on)

        for r in range(R + 2):
            kr = rng.PRNGKey(100 + r)
            got = dict(draw_noise_ms=timed(lambda: learner.draw_entropy_noise(env, kr, (K, E, 12))),
                       shuffle_ms=timed(lambda: learner.shuffle_env_index(kr, E)),
                       rollout_beside_draws_ms=rollout(),
                       host_normal_ms=wall(lambda: rng.normal(kr, (K, E, 12), part)),
                       host_permutation_ms=wall(lambda: rng.permutation(kr, E, part)),
                       host_key_splits_ms=wall(lambda: key_splits(kr)),
                       train_iteration_host_rng_ms=wall(lambda: iteration(False)),
                       train_iteration_device_rng_ms=wall(lambda: iteration(True)))
            if r >= 2:
                for k, v in got.items():
                    out[k].append(round(v, 4))
    med = {k: sorted(x)[len(x) // 2] for k, x in out.items()}
    spread = {k: [min(x), max(x)] for k, x in out.items()}
    final = learner.metrics()
    print(json.dumps({"envs": E, "warmup": W, "steps": K, "minibatch_envs": MB, "rounds": R,
                      "rows": {"minibatch": K * MB, "batch": K * E}, "median_ms": med, "min_max_ms": spread,
                      "learn_over_torch": {"minibatch": round(med["learn_minibatch_ms"] / med["torch_minibatch_ms"], 3),
                                           "batch": round(med["learn_batch_ms"] / med["torch_batch_ms"], 3)},
                      "learn_batch_share_of_rollout": round(med["learn_batch_ms"] / med["rollout_ms"], 3),
                      **({"norm_update_gb_per_s": round(2 * rows * D * 4 / (med["norm_update_ms"] * 1e6), 1),
                          "norm_update_over_torch": round(med["norm_update_ms"] / med["torch_norm_ms"], 3),
                          "share_of_rollout": {k: round(med[k] / med["rollout_ms"], 4)
                                               for k in ("norm_update_ms", "clip_scale_ms", "learn_batch_indexed_ms")},
                          "indexed_over_plain": {"minibatch": round(med["learn_minibatch_indexed_ms"] / med["learn_minibatch_ms"], 3),
                                                 "batch": round(med["learn_batch_indexed_ms"] / med["learn_batch_ms"], 3)},
                          "norm_first_update_vs_torch": norm_check} if extra else {}),
                      **({"across_ranks": {
                          "reduced_floats_per_rank": count, "reduce_world8_gb_per_s": round(
                              9 * count * 4 / (med["reduce_world8_ms"] * 1e6), 1),
                          "norm_update_ranks_over_plain": round(
                              med["norm_update_ranks_ms"] / med["norm_update_beside_ranks_ms"], 3),
                          "share_of_minibatch_step": {k: round(med[k] / med["learn_minibatch_ms"], 4) for k in rnames},
                          "share_of_rollout": {k: round(med[k] / med["rollout_ms"], 5) for k in rnames}}}
                         if ranks else {}),
                      **({"device_rng": {
                          "noise_floats": K * E * 12, "minibatches": E // MB,
                          "share_of_rollout": {k: round(med[k] / med["rollout_beside_draws_ms"], 5)
                                               for k in ("draw_noise_ms", "shuffle_ms")},
                          "host_normal_over_draw": round(med["host_normal_ms"] / med["draw_noise_ms"], 1),
                          "host_permutation_over_shuffle": round(med["host_permutation_ms"] / med["shuffle_ms"], 1),
                          "train_iteration_device_over_host_rng": round(
                              med["train_iteration_device_rng_ms"] / med["train_iteration_host_rng_ms"], 3),
                          "key_splits_share_of_train_iteration_device_rng": round(
                              med["host_key_splits_ms"] / med["train_iteration_device_rng_ms"], 4)}}
                         if device_rng else {}),
                      "plain_grad_crc32": plain_crc, "rollout_crc32": rollout_crc,
                      "first_total_loss": {"learner": ours, "torch": theirs},
                      "losses_finite": bool(all(np.isfinite(v) for v in final.values()))}), flush=True)
    nstate.free()
    if ranks:
        gathered.free(), rmetrics.free(), rstate.free()
        comm.close()
    for e in ev:
        raw_lib.hipEventDestroy(e)
    actor.close()
    critic.close()
    learner.close()
    env.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--minibatch", type=int, default=256, help="envs of the small minibatch")
    ap.add_argument("--repeat", type=int, default=9, help="timed rounds (medians and min .. max are reported)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.envs, args.warmup, args.steps, args.minibatch, args.repeat)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(args.envs), "--warmup", str(args.warmup),
           "--steps", str(args.steps), "--minibatch", str(args.minibatch), "--repeat", str(args.repeat)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s", file=sys.stderr)
        return 124
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-2000:])
        return out.returncode
    print(out.stdout.strip().split("\n")[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
