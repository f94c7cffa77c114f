"""Rate of the sampled policy rollout (pp3_rollout_policy_sample_timed: PPO data collection, the
tanh-Gaussian head in the fused launch) next to the deterministic one (pp3_rollout_policy_timed)
on the same env and the same network 72 -> 256 -> 128 -> 128 -> 24 (the deterministic policy is
its deployment export, -> 12).  Each mode runs in a child process of its own under a time limit:
set up, ~200 ms of the same launches as GPU pre-warm (state restored), W warm-up steps through the
same entry point, then the K timed steps (HIP events around the launch).  One JSON line per mode
and a summary line.

  python tools/policy_sample_bench.py [--envs 4096 --warmup 200 --steps 200 --repeat 1 --timeout 120]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd")]


def child(mode: str, E: int, W: int, K: int) -> None:
    from collections import OrderedDict
    from types import SimpleNamespace

    import numpy as np

    import bench
    from pupperv3_mjx import MODEL_XML, _abi, _lib, export, rng
    from pupperv3_mjx.environment import PupperV3Env

    env = PupperV3Env(**bench.bench_kwargs(MODEL_XML), num_envs=E, device=0, pipeline_output=False)
    L = env._L
    st = env.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(0), E)))
    rec = st._record.copy()
    rec[:, _abi.S_COMMAND:_abi.S_COMMAND + 3] = [0.5, 0.0, 0.0]
    env._put(_abi.F_STATE, rec)
    rs = np.random.RandomState(7)
    sizes = [env.observation_size, 256, 128, 128, 2 * _abi.NU]
    layers = OrderedDict((f"hidden_{i}", {"kernel": rs.normal(scale=1 / np.sqrt(sizes[i]), size=(sizes[i], sizes[i + 1])),
                                          "bias": np.zeros(sizes[i + 1])}) for i in range(len(sizes) - 1))
    params = (SimpleNamespace(mean=np.zeros(sizes[0]), std=np.ones(sizes[0])), {"params": layers})
    conv = export.convert_training_params if mode == "sample" else export.convert_params
    pol = export.DevicePolicy(conv(params, "elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12), True,
                                   env._observation_history, 30.0, 30.0), 0)
    n_max = max(W, K, 20)
    D = env.observation_size
    act, raw = _lib.DeviceBuffer(4 * n_max * E * 12), _lib.DeviceBuffer(4 * n_max * E * 12)
    logp, rew, done = (_lib.DeviceBuffer(4 * n_max * E) for _ in range(3))
    obs = _lib.DeviceBuffer(4 * K * E * D)
    key = rng.PRNGKey(1)
    kin, kout = np.array(key, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    kp, ko = kin.ctypes.data_as(C.c_void_p), kout.ctypes.data_as(C.c_void_p)
    ms = C.c_float()

    def run(n, timed=False, traj=False):
        o = (rew.ptr, done.ptr, obs.ptr) if traj else (None, None, None)
        if mode == "sample":
            if timed:
                _lib.check(L.pp3_rollout_policy_sample_timed(env._h, pol._h, n, kp, ko, act.ptr, raw.ptr, logp.ptr, *o,
                                                             C.byref(ms)))
            else:
                _lib.check(L.pp3_rollout_policy_sample(env._h, pol._h, n, kp, ko, act.ptr, raw.ptr, logp.ptr, *o, None))
            kin[:] = kout
        elif timed:
            _lib.check(L.pp3_rollout_policy_timed(env._h, pol._h, n, act.ptr, *o, C.byref(ms)))
        else:
            _lib.check(L.pp3_rollout_policy(env._h, pol._h, n, act.ptr, *o, None))

    fields = [_abi.F_STATE, _abi.F_OBS, _abi.F_REWARD, _abi.F_DONE]
    stream = L.pp3_stream(env._h)
    snap = {f: _lib.DeviceBuffer(4 * E * env.device_field(f)[1]) for f in fields}
    for f, b in snap.items():
        _lib.check(L.pp3_memcpy_d2d(b.ptr, C.c_void_p(env.device_field(f)[0]), b.nbytes, stream))
    t0, n_pw = time.perf_counter(), 0
    while time.perf_counter() - t0 < 0.2:  # GPU pre-warm: the clocks of a busy GPU (bench.py does the same)
        run(20)
        for f, b in snap.items():
            _lib.check(L.pp3_memcpy_d2d(C.c_void_p(env.device_field(f)[0]), b.ptr, b.nbytes, stream))
        n_pw += 1
        if n_pw % 4 == 0:
            env.synchronize()
    if W:
        run(W)
    env.synchronize()
    run(K, timed=True, traj=True)
    a = np.zeros((E, 12), dtype=np.float32)
    _lib.check(L.pp3_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(act.ptr.value + 4 * (K - 1) * E * 12), a.nbytes))
    print(json.dumps({"mode": mode, "envs": E, "warmup": W, "steps": K, "kernel_ms": round(ms.value, 3),
                      "us_per_step": round(1e3 * ms.value / K, 3),
                      "env_steps_per_s": round(E * K / (ms.value / 1e3), 1),
                      "fused": int(L.pp3_rollout_policy_fused(env._h)), "actions_finite": bool(np.all(np.isfinite(a)))}),
          flush=True)
    pol.close()
    env.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=1, help="alternate the two modes this many times")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per child process")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.envs, args.warmup, args.steps)
        return 0
    rates = {"deterministic": [], "sample": []}
    for _ in range(args.repeat):
        for mode in ("deterministic", "sample"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--envs", str(args.envs), "--warmup",
                   str(args.warmup), "--steps", str(args.steps)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{mode}: no result within {args.timeout} s; stopping", file=sys.stderr)
                return 124
            if out.returncode != 0:  # nothing more is started on the GPU after a failed child
                sys.stderr.write(out.stderr[-2000:])
                return out.returncode
            line = out.stdout.strip().split("\n")[-1]
            print(line, flush=True)
            rates[mode].append(json.loads(line))
    med = {m: sorted(r["us_per_step"] for r in v)[len(v) // 2] for m, v in rates.items()}
    print(json.dumps({"summary": "us per step (median)", **med,
                      "sample_minus_deterministic_us": round(med["sample"] - med["deterministic"], 3),
                      "sample_env_steps_per_s": round(args.envs / (med["sample"] * 1e-6), 1),
                      "deterministic_env_steps_per_s": round(args.envs / (med["deterministic"] * 1e-6), 1)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
