"""Cost of the PPO batch's parts at the training shape, each between HIP events on the env's stream:
  (a) pp3_rollout_policy_sample over K steps with the truncation row off and on
      (pp3_rollout_policy_sample_timed; actor 72 -> 256 -> 128 -> 128 -> 24),
  (b) the critic over the (K + 1) * N observation rows (pp3_policy_act, 72 -> 256 -> 128 -> 128 -> 1),
  (c) pp3_gae over the K x N rows.
One child process under a time limit: set up, W warm-up steps, then `--repeat` rounds of
(a-off, a-on, b, c) on a restored state; medians per part and (b) + (c) as a share of (a).

  python tools/ppo_collect_bench.py [--envs 4096 --warmup 200 --steps 20 --repeat 7 --timeout 120]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd")]


def child(E: int, W: int, K: int, R: int) -> None:
    from collections import OrderedDict
    from types import SimpleNamespace

    import numpy as np

    import bench
    from pupperv3_mjx import MODEL_XML, _abi, _lib, export, rng
    from pupperv3_mjx.environment import PupperV3Env

    env = PupperV3Env(**bench.bench_kwargs(MODEL_XML), num_envs=E, device=0, pipeline_output=False)
    L = env._L
    raw_lib = _lib.load()  # (the HIP runtime's event calls resolve through the library's handle)
    st = env.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(0), E)))
    rec = st._record.copy()
    rec[:, _abi.S_COMMAND:_abi.S_COMMAND + 3] = [0.5, 0.0, 0.0]
    env._put(_abi.F_STATE, rec)
    _lib.check(L.pp3_set_auto_reset(env._h, 1000))
    D = env.observation_size
    rs = np.random.RandomState(7)

    def net(last):
        sizes = [D, 256, 128, 128, last]
        layers = OrderedDict((f"hidden_{i}", {"kernel": rs.normal(scale=1 / np.sqrt(sizes[i]), size=(sizes[i], sizes[i + 1])),
                                              "bias": np.zeros(sizes[i + 1])}) for i in range(len(sizes) - 1))
        return (SimpleNamespace(mean=np.zeros(D), std=np.ones(D)), {"params": layers})

    pol = export.DevicePolicy(export.convert_training_params(net(2 * _abi.NU), "elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12),
                                                             -np.ones(12), True, env._observation_history, 30.0, 30.0), 0)
    val = export.DevicePolicy(export.convert_value_params(net(1), "elu", env._observation_history), 0)
    n_max = max(W, K)
    act, raw = _lib.DeviceBuffer(4 * n_max * E * 12), _lib.DeviceBuffer(4 * n_max * E * 12)
    logp, rew, done, trunc, vs, adv = (_lib.DeviceBuffer(4 * n_max * E) for _ in range(6))
    obs_all, val_all = _lib.DeviceBuffer(4 * (K + 1) * E * D), _lib.DeviceBuffer(4 * (K + 1) * E)
    kin, kout = np.array(rng.PRNGKey(1), dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    kp, ko = kin.ctypes.data_as(C.c_void_p), kout.ctypes.data_as(C.c_void_p)
    ms = C.c_float()
    stream = C.c_void_p(L.pp3_stream(env._h))
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

    def rollout(n, row):
        _lib.check(L.pp3_set_truncation_trajectory(env._h, trunc.ptr if row else None, n if row else 0))
        _lib.check(L.pp3_rollout_policy_sample_timed(env._h, pol._h, n, kp, ko, act.ptr, raw.ptr, logp.ptr, rew.ptr, done.ptr,
                                                     C.c_void_p(obs_all.ptr.value + 4 * E * D), C.byref(ms)))
        _lib.check(L.pp3_set_truncation_trajectory(env._h, None, 0))
        return ms.value

    fields = [_abi.F_STATE, _abi.F_OBS, _abi.F_REWARD, _abi.F_DONE, _abi.F_EPISODE]
    if W:
        _lib.check(L.pp3_rollout_policy_sample(env._h, pol._h, W, kp, ko, act.ptr, raw.ptr, logp.ptr, None, None, None, None))
    env.synchronize()
    snap = {f: _lib.DeviceBuffer(4 * E * env.device_field(f)[1]) for f in fields}
    for f, b in snap.items():  # every round starts from the state after the warm-up
        _lib.check(L.pp3_memcpy_d2d(b.ptr, C.c_void_p(env.device_field(f)[0]), b.nbytes, stream))
    _lib.check(L.pp3_memcpy_d2d(obs_all.ptr, C.c_void_p(env.device_field(_abi.F_OBS)[0]), 4 * E * D, stream))
    out = {"rollout_row_off_ms": [], "rollout_row_on_ms": [], "critic_ms": [], "gae_ms": []}
    for r in range(R + 1):  # round 0 is a warm-up of its own (first launches of the critic and pp3_gae)
        got = {}
        for name, row in (("rollout_row_off_ms", False), ("rollout_row_on_ms", True)):
            for f, b in snap.items():
                _lib.check(L.pp3_memcpy_d2d(C.c_void_p(env.device_field(f)[0]), b.ptr, b.nbytes, stream))
            got[name] = rollout(K, row)
        got["critic_ms"] = timed(lambda: val.act(obs_all.ptr.value, D, (K + 1) * E, val_all.ptr.value, 1, stream.value))
        got["gae_ms"] = timed(lambda: _lib.check(L.pp3_gae(
            0, K, E, E, rew.ptr, done.ptr, trunc.ptr, val_all.ptr, C.c_void_p(val_all.ptr.value + 4 * K * E), 0.97, 0.95, 1.0,
            vs.ptr, adv.ptr, stream)))
        if r:
            for k, v in got.items():
                out[k].append(round(v, 4))
    v = np.zeros((K, E), dtype=np.float32)
    vs.download(v)
    med = {k: sorted(x)[len(x) // 2] for k, x in out.items()}
    print(json.dumps({"envs": E, "warmup": W, "steps": K, "rounds": R, "fused": int(L.pp3_rollout_policy_fused(env._h)),
                      "runs_ms": out, "median_ms": med,
                      "critic_plus_gae_share_of_rollout": round((med["critic_ms"] + med["gae_ms"]) / med["rollout_row_off_ms"], 4),
                      "row_on_minus_off_ms": round(med["rollout_row_on_ms"] - med["rollout_row_off_ms"], 4),
                      "targets_finite": bool(np.all(np.isfinite(v)))}), flush=True)
    for e in ev:
        raw_lib.hipEventDestroy(e)
    pol.close()
    val.close()
    env.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=7, help="timed rounds (medians are reported)")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.envs, args.warmup, args.steps, args.repeat)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(args.envs), "--warmup", str(args.warmup),
           "--steps", str(args.steps), "--repeat", str(args.repeat)]
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
