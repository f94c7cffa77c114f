"""Cost of a checkpoint (ppo.save_checkpoint / load_checkpoint) and of the device initialisation
(PPOLearner.init_params) at `--envs` envs with the README's nets (72 -> 256 -> 128 -> 128 -> 24 and
.. -> 1, running statistics), after `--warmup` warm-up steps and one training iteration (so that the
moments and the normaliser hold numbers), in wall-clock ms from call to return, medians over `--repeat`
alternating rounds with the run-to-run spread (min .. max) beside them:
  save_ms      save_checkpoint of the learner, the wrapped env with its state, an evaluator key and a
               loop part: the downloads, the .npz written under a temporary name, fsync, rename;
  load_ms      load_checkpoint of that file: the .npz read back into plain arrays;
  restore_ms   the dict put back: learner.load_state_dict, wrap(env).load_state_dict, handles reloaded;
  init_ms      init_params on the env's stream and the wait for it;
  rollout_ms   the sampled rollout of `--unroll` steps (wrap(env).rollout_policy_sample) in the same
               rounds: what a checkpoint per epoch costs, in rollouts.
One child process under a time limit; the result line is printed and appended to `--out`.

  python tools/ppo_checkpoint_bench.py [--envs 4096 --unroll 20 --warmup 200 --repeat 9 --timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd"), os.path.join(ROOT, "tests")]


def child(E: int, K: int, W: int, R: int) -> None:
    from collections import OrderedDict

    import numpy as np

    import bench
    from pupperv3_mjx import MODEL_XML, ppo, rng, wrappers
    from pupperv3_mjx.environment import PupperV3Env

    env = PupperV3Env(**bench.bench_kwargs(MODEL_XML), num_envs=E, device=0, pipeline_output=False)
    w = wrappers.wrap(env, episode_length=1000)
    learner = ppo.make_learner(rng.PRNGKey(0), env.observation_size, max_rows=(K + 1) * E)
    actor, critic = learner.make_policies()
    key = np.array(rng.PRNGKey(1), dtype=np.uint32)
    st = w.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(2), E)))
    for w0 in range(0, W, 20):
        st, _, key = w.rollout_policy_sample(st, actor, min(20, W - w0), key)
    st, _, _ = learner.train_iteration(w, st, rng.PRNGKey(3), actor, critic, K, num_minibatches=16, shuffle=True,
                                       max_grad_norm=1.0, update_normalizer=True, device_rng=True)
    loop = dict(k_train=np.array(rng.PRNGKey(4), dtype=np.uint32), iteration=np.asarray(1, np.int64),
                epoch=np.asarray(1, np.int64), walltime=np.asarray(0.0))
    evaluator = {"key": np.array(rng.PRNGKey(5), dtype=np.uint32)}
    box = {"state": st, "key": key}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ck.npz")

        def save():
            ppo.save_checkpoint(path, learner, w, box["state"], evaluator, loop)

        def load():
            box["ck"] = ppo.load_checkpoint(path)

        def restore():
            learner.load_state_dict(box["ck"]["learner"])
            learner.sync(actor, critic)
            box["state"] = w.load_state_dict(box["ck"]["env"])

        def init():
            learner.init_params(rng.PRNGKey(0))
            env.synchronize()

        def rollout():
            box["state"], _, box["key"] = w.rollout_policy_sample(box["state"], actor, K, box["key"])

        pieces = OrderedDict((("save_ms", save), ("load_ms", load), ("restore_ms", restore), ("init_ms", init),
                              ("rollout_ms", rollout)))
        for fn in pieces.values():  # one untimed pass of everything
            fn()
        times = {name: [] for name in pieces}
        names = list(pieces)
        for r in range(R):
            if r % len(names):  # the order rotates; a restore always follows a save and a load of this state
                save(), load()
            for name in names[r % len(names):] + names[:r % len(names)]:
                t0 = time.perf_counter()
                pieces[name]()
                times[name].append(1e3 * (time.perf_counter() - t0))
        size = os.path.getsize(path)
    med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    print(json.dumps({
        "envs": E, "unroll": K, "warmup": W, "rounds": R, "file_bytes": size,
        "learner_floats": int(sum(learner.buffer(n, 0)[1] for n in (0, 1))), "median_ms": med,
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
        "save_over_rollout": round(med["save_ms"] / med["rollout_ms"], 3)}), flush=True)
    actor.close(), critic.close(), learner.close(), env.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=20, help="steps of the rollout timed beside the checkpoint")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=9, help="timed rounds (medians and min .. max are reported)")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_checkpoint_bench.txt"),
                    help="result lines are appended here")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.envs, args.unroll, args.warmup, args.repeat)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(args.envs), "--unroll", str(args.unroll),
           "--warmup", str(args.warmup), "--repeat", str(args.repeat)]
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
