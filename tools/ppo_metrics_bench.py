"""Cost of the PPO metrics at `--envs` envs and unrolls of `--steps` steps after `--warmup` warm-up
steps, medians over `--repeat` alternating rounds with the run-to-run spread (min .. max) beside them:
  (a) stats_pair_us      pp3_episode_stats_begin + pp3_episode_stats_rows (EpisodeStats.begin / add) on
                         a collected batch: `--batch` pairs queued behind each other, one wait, per pair;
      collect_ms         the sampled collection they ride on (collect_ppo(host_batch=False) and a wait),
                         timed in the same rounds; stats_share = pair / collect;
  (b) iteration_device_ms / iteration_host_ms   train_iteration wall clock (4 minibatches, shuffle, device
                         draws, episode statistics on) with collect_ppo(host_batch=False), what it calls,
                         against the same iteration with the batch downloaded (host_batch=True forced);
  (c) eval_comm_ms / eval_plain_ms   Evaluator.run_evaluation (reward path, `--eval-steps` steps) with a
                         one-rank communicator (two all-gathers of 22 floats, five more launches)
                         against without; "eval_agree": both report the same bits.
Two or more ranks on separate GPUs are not measured here (one GPU).  One child process under a time
limit; the result line is printed and appended to `--out`.

  python tools/ppo_metrics_bench.py [--envs 4096 --steps 20 --warmup 200 --repeat 9 --timeout 900]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd"), os.path.join(ROOT, "tests")]


def child(E: int, K: int, W: int, R: int, batch: int, eval_steps: int) -> None:
    from collections import OrderedDict

    import numpy as np

    import bench
    from pupperv3_mjx import MODEL_XML, evaluator, ppo, rng, sharding, wrappers
    from pupperv3_mjx.environment import PupperV3Env

    env = PupperV3Env(**bench.bench_kwargs(MODEL_XML), num_envs=E, device=0, pipeline_output=False)
    w = wrappers.wrap(env, episode_length=eval_steps)
    learner = ppo.make_learner(rng.PRNGKey(1), env.observation_size, max_rows=(K + 1) * E)
    actor, critic = learner.make_policies()
    stats = ppo.EpisodeStats()
    key = np.array(rng.PRNGKey(2), dtype=np.uint32)
    holder = {"state": w.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(0), E))), "key": key}
    for w0 in range(0, W, K):
        holder["state"], _, holder["key"] = w.collect_ppo(holder["state"], actor, critic, min(K, W - w0), holder["key"],
                                                          host_batch=False)
    env.synchronize()

    def collect():
        holder["state"], _, holder["key"] = w.collect_ppo(holder["state"], actor, critic, K, holder["key"], host_batch=False)
        env.synchronize()

    def pairs():
        for j in range(batch):
            stats.begin(w)
            stats.add(w)
            stats._pending = j == batch - 1  # (queued only: the last pair's numbers are read after the wait)
        env.synchronize()
        stats.fetch()

    mode = {"force": None}  # (b): the batch download train_iteration no longer makes, forced back on
    plain_collect = env.collect_ppo
    env.collect_ppo = lambda *a, host_batch=True, **k: plain_collect(
        *a, host_batch=host_batch if mode["force"] is None else mode["force"], **k)

    def iteration(host):
        mode["force"] = host
        try:
            holder["key"], k_it = rng.split(holder["key"], 2)
            holder["state"], _, _ = learner.train_iteration(w, holder["state"], k_it, actor, critic, K, num_minibatches=4,
                                                            shuffle=True, device_rng=True, episode_stats=stats)
        finally:
            mode["force"] = None

    result = {"envs": E, "steps": K, "warmup": W, "rounds": R, "pairs_per_wait": batch, "eval_steps": eval_steps}
    pieces = OrderedDict((("collect_ms", collect), ("stats_pairs_ms", pairs),
                          ("iteration_device_ms", lambda: iteration(False)), ("iteration_host_ms", lambda: iteration(True))))
    try:
        comm = sharding.Comm(0, 1, 0, tag="_metrics_bench")
    except Exception as exc:  # (no RCCL on this host: (c) is left out and says so)
        comm = None
        result["eval_comm_error"] = str(exc)[:200]
    evs = {}
    if comm is not None:
        k_eval = np.array(rng.PRNGKey(3), dtype=np.uint32)
        for name, c in (("eval_plain_ms", None), ("eval_comm_ms", comm)):
            evs[name] = evaluator.Evaluator(w, actor, eval_steps, key=k_eval, deterministic=False, metrics=False, comm=c)

        def run_eval(name):
            evs[name]._key = k_eval.copy()  # every round evaluates the same episodes
            t0 = time.perf_counter()
            out = evs[name].run_evaluation()
            holder["ms"] = 1e3 * (time.perf_counter() - t0)
            # (the evaluation reset the env: the training pieces go on from a fresh reset, outside the timing)
            holder["state"] = w.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(0), E)))
            return out

        for name in evs:
            pieces[name] = lambda name=name: run_eval(name)
    last = {name: fn() for name, fn in pieces.items()}  # one untimed pass of everything
    holder.pop("ms", None)
    times = {name: [] for name in pieces}
    names = list(pieces)
    for r in range(R):
        for name in names[r % len(names):] + names[:r % len(names)]:  # the order rotates
            t0 = time.perf_counter()
            last[name] = pieces[name]()
            times[name].append(holder.pop("ms", None) or 1e3 * (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in times.items()}
    result["median_ms"] = {k: round(v, 4) for k, v in med.items()}
    result["min_max_ms"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
    result["stats_pair_us"] = round(1e3 * med["stats_pairs_ms"] / batch, 3)
    result["stats_share_of_collect"] = round(med["stats_pairs_ms"] / batch / med["collect_ms"], 6)
    result["iteration_device_over_host"] = round(med["iteration_device_ms"] / med["iteration_host_ms"], 4)
    result["batch_download_mb"] = round(4e-6 * K * E * (env.observation_size + 2 * 12 + 7), 2)  # (K rows of every array)
    if evs:
        same = ("eval/episode_reward", "eval/episode_reward_std", "eval/avg_episode_length", "eval/std_episode_length")
        result["eval_comm_over_plain"] = round(med["eval_comm_ms"] / med["eval_plain_ms"], 4)
        result["eval_agree"] = all(last["eval_comm_ms"][k] == last["eval_plain_ms"][k] for k in same)
        for e in evs.values():
            e.close()
        comm.close()
    count, _ = stats.read()
    result["episodes_counted"] = count
    stats.close()
    actor.close(), critic.close(), learner.close()
    env.close()
    print(json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20, help="unroll length K")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=9, help="timed rounds (medians and min .. max are reported)")
    ap.add_argument("--batch", type=int, default=100, help="begin + rows pairs behind one wait")
    ap.add_argument("--eval-steps", type=int, default=100, help="episode length of (c)'s evaluations")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_metrics_bench.txt"), help="result lines are appended here")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.envs, args.steps, args.warmup, args.repeat, args.batch, args.eval_steps)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(args.envs), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--repeat", str(args.repeat), "--batch", str(args.batch),
           "--eval-steps", str(args.eval_steps)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s", file=sys.stderr)
        return 124
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-2000:])
        return out.returncode
    line = out.stdout.strip().split("\n")[-1]
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
