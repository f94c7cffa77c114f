"""The kernels compute the parent commit's results bit for bit.

The fixtures under tests/golden/bits_parent/ were recorded on an MI355X with the build of the commit
before the issue-slot pass on the fused step kernel (re-laid pair tables, register copies, EXEC
regions: edits that must leave every value, operation order and FMA contraction as they were).
Each holds, after a short run, the state record as uint32 and the obs / reward / done rows of
every step, and the HIP runtime version and the device's ISA name it was recorded with.

The comparison is against THAT machine's parent build: code generation of the unchanged parts
may differ under another ROCm or device, so a fixture from another runtime or device FAILS (it does
not skip) and asks for a re-record: check out the parent commit, build it, and run this module with
PP3_RECORD_PARENT_BITS=1 (it then writes the fixtures instead of comparing), and commit them.

Cases (the smallest shapes that reach each instantiation and table path):
  flat 6 envs x 12 steps, fused and as 12 single-step launches   (both kernels, NC = 8)
  flat 5 envs x 6 steps fused                                     (tail wave, clamped second env)
  max_contacts = 16, 6 envs x 6 steps                             (NC = 16)
  10 boxes, 6 envs over the rails, 8 steps fused and single-step  (112 pairs = 3.5 batches, CULL)
  per-env terrain, 6 envs x 8 steps
  policy rollout, 40 envs x 3 steps                               (NWV = 8 kernel, partial tile)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
from pupperv3_mjx import _abi, _lib, obstacles
from pupperv3_mjx.environment import PupperV3Env, make_keys

pytestmark = pytest.mark.gpu

DIR = os.path.join(common.GOLDEN, "bits_parent")
RECORD = os.environ.get("PP3_RECORD_PARENT_BITS", "") not in ("", "0")


def _hip_identity():
    """(the HIP runtime version of the ROCm installation the extension is built with and linked
    against, device 0's ISA name).  The version is what that installation's hipRuntimeGetVersion
    returns, HIP_VERSION of its hip_version.h (major * 10^7 + minor * 10^5 + patch), read from the
    header so that the answer does not depend on the process: one that has imported another
    package's bundled HIP runtime first runs the extension on that one and cannot load the
    installation's beside it.  Where it can be loaded, its hipRuntimeGetVersion must agree.  The
    ISA name (gcnArchName, e.g. gfx950:sramecc+:xnack-) stands for the device: its marketing name
    differs between runtimes on one machine (empty or generic).  It is found in the device
    properties by its "gfx" prefix; its offset differs between ROCm releases and the buffer is
    larger than any release's struct."""
    L = _lib.load()
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    hdr = open(os.path.join(rocm, "include", "hip", "hip_version.h")).read()
    num = [int(re.search(r"#define\s+HIP_VERSION_%s\s+(\d+)" % k, hdr).group(1)) for k in ("MAJOR", "MINOR", "PATCH")]
    version = num[0] * 10000000 + num[1] * 100000 + num[2]
    try:
        hip = C.CDLL(os.path.join(rocm, "lib", "libamdhip64.so"))
    except OSError:  # another HIP runtime (and its HSA runtime) is already in this process
        hip = None
    if hip is not None:
        v = C.c_int(0)
        assert hip.hipRuntimeGetVersion(C.byref(v)) == 0 and v.value == version, (v.value, version)
    prop = C.create_string_buffer(16384)
    assert L.hipGetDevicePropertiesR0600(prop, 0) == 0  # (the runtime this process runs the extension on)
    i = prop.raw.find(b"gfx")
    assert i >= 0, "no gcnArchName in the device properties"
    return version, prop.raw[i:prop.raw.index(b"\0", i)].decode()


def _check_or_record(case, got):
    path = os.path.join(DIR, case + ".npz")
    version, device = _hip_identity()
    if RECORD:
        os.makedirs(DIR, exist_ok=True)
        np.savez_compressed(path, hip_runtime_version=np.int64(version), device_name=np.array(device), **got)
        return
    assert os.path.exists(path), f"fixture {path} is missing: record it at the parent commit (module docstring)"
    want = np.load(path)
    rec = (int(want["hip_runtime_version"]), str(want["device_name"]))
    assert rec == (version, device), (
        f"fixture recorded with HIP runtime / device {rec}, this machine has {(version, device)}: "
        "re-record the fixtures with the parent commit's build on this machine (module docstring)")
    assert sorted(got) == sorted(k for k in want.files if k not in ("hip_runtime_version", "device_name"))
    for k, v in got.items():
        w = want[k]
        assert v.dtype == w.dtype and v.shape == w.shape, (k, v.dtype, w.dtype, v.shape, w.shape)
        bad = np.argwhere(v != w)
        assert bad.size == 0, f"{case}: {k} differs from the parent's bits at {len(bad)} places, first {bad[0]}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()


def _fused(env, acts, tag=""):
    """K steps from the state the device buffers hold, as one fused launch (pp3_rollout: the
    <NC, true> kernel) with its trajectory rows.  (Device API: env.rollout(state, ...) would first
    write `state` back over a start state edited with _put.)"""
    K, n, D = acts.shape[0], env.num_envs, env.observation_size
    bufs = [_lib.DeviceBuffer(b) for b in (acts.nbytes, K * n * 4, K * n * 4, K * n * D * 4)]
    try:
        bufs[0].upload(np.ascontiguousarray(acts, dtype=np.float32))
        env.rollout_device(bufs[0].ptr.value, n * _abi.NU, K, bufs[1].ptr.value, bufs[2].ptr.value, bufs[3].ptr.value)
        env.synchronize()
        out = {tag + "state": _bits(env._get(_abi.F_STATE))}
        for k, b, shape in (("reward", bufs[1], (K, n)), ("done", bufs[2], (K, n)), ("obs", bufs[3], (K, n, D))):
            a = np.empty(shape, np.float32)
            b.download(a)
            out[tag + k] = _bits(a)
        return out
    finally:
        for b in bufs:
            b.free()


def _single(env, acts, tag=""):
    """The same steps as single-step launches (pp3_step: the <NC, false> kernel)."""
    n = env.num_envs
    ab = _lib.DeviceBuffer(n * _abi.NU * 4)
    rows = {"obs": [], "reward": [], "done": []}
    try:
        for a in acts:
            ab.upload(np.ascontiguousarray(a, dtype=np.float32))
            env.step_device(ab.ptr.value)
            env.synchronize()
            for k, f in (("obs", _abi.F_OBS), ("reward", _abi.F_REWARD), ("done", _abi.F_DONE)):
                rows[k].append(_bits(env._get(f)).reshape((n, -1) if k == "obs" else (n,)))
        out = {tag + "state": _bits(env._get(_abi.F_STATE))}
        for k, v in rows.items():
            out[tag + k] = np.stack(v)
        return out
    finally:
        ab.free()


def _acts(seed, K, n):
    return np.random.RandomState(seed).uniform(-1, 1, size=(K, n, _abi.NU)).astype(np.float32)


def _over_rails(env, st, seed):
    """Move the reset state's base over the model's rails (configs[4]'s start, as test_gpu_cull)."""
    rows = common.model_terrain_rows(env.sys_model.struct)
    specs = [obstacles.BoxSpec("", float(r[0]), float(r[1]), tuple(float(v) for v in r[3:7]),
                               tuple(float(v) for v in r[7:10])) for r in rows]
    rec = st._record.copy()
    rec[:, _abi.S_QPOS:_abi.S_QPOS + 2] = obstacles.rail_start_xy(specs, env.num_envs, seed=seed)
    env._put(_abi.F_STATE, rec)


@pytest.fixture(scope="module")
def flat_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_flat"), 0)


@pytest.fixture(scope="module")
def box_path(require_gpu, tmp_path_factory):
    return common.write_model(tmp_path_factory.mktemp("bits_box"), 10)


def test_flat_fused_and_single_step(flat_path):
    n, K = 6, 12
    acts = _acts(1, K, n)
    got = {}
    for mode in ("fused", "single"):
        e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
        try:
            e.reset(make_keys(0, n))
            got.update(_fused(e, acts, "fused_") if mode == "fused" else _single(e, acts, "single_"))
        finally:
            e.close()
    for k in ("state", "obs", "reward", "done"):  # (the fused launch is the single-step launches, bit for bit)
        np.testing.assert_array_equal(got["fused_" + k], got["single_" + k])
    _check_or_record("flat_6x12", got)


def test_flat_odd_env_count(flat_path):
    n, K = 5, 6
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    try:
        e.reset(make_keys(1, n))
        got = _fused(e, _acts(2, K, n))
    finally:
        e.close()
    _check_or_record("flat_5x6", got)


def test_ncon_max_16(flat_path):
    n, K = 6, 6
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n, max_contacts=16)
    try:
        assert e.config_struct.ncon_max == 16
        e.reset(make_keys(2, n))
        got = _fused(e, _acts(3, K, n))
    finally:
        e.close()
    _check_or_record("nc16_6x6", got)


def test_obstacle_boxes_fused_and_single_step(box_path):
    n, K = 6, 8
    acts = _acts(4, K, n)
    got = {}
    for mode in ("fused", "single"):
        e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=n)
        try:
            assert e._L.pp3_narrow_cull(e._h) == 1
            st = e.reset(make_keys(3, n))
            _over_rails(e, st, seed=4)
            got.update(_fused(e, acts, "fused_") if mode == "fused" else _single(e, acts, "single_"))
        finally:
            e.close()
    for k in ("state", "obs", "reward", "done"):
        np.testing.assert_array_equal(got["fused_" + k], got["single_" + k])
    _check_or_record("boxes_6x8", got)


def test_per_env_terrain(box_path):
    n, K = 6, 8
    e = PupperV3Env(**common.fixture_kwargs(box_path), num_envs=n)
    try:
        st = e.reset(make_keys(4, n))
        e.set_terrain(common.terrain_under(st._record[:, _abi.S_QPOS:_abi.S_QPOS + 2].astype(np.float64), 10, seed=5))
        got = _fused(e, _acts(5, K, n))
    finally:
        e.close()
    _check_or_record("terrain_6x8", got)


def test_policy_rollout(flat_path):
    from pupperv3_mjx import export
    from test_gpu_policy import _policy
    n, K = 40, 3
    e = PupperV3Env(**common.fixture_kwargs(flat_path), num_envs=n)
    dp = export.DevicePolicy(_policy([72, 128, 128, 24], "elu"))
    try:
        st, tr = e.rollout_policy(e.reset(make_keys(5, n)), dp, K)
        got = {"state": _bits(e._get(_abi.F_STATE))}
        for k in ("obs", "reward", "done", "action"):
            got[k] = _bits(tr[k])
    finally:
        dp.close()
        e.close()
    _check_or_record("policy_40x3", got)
