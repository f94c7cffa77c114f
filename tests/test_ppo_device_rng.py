"""The device draws of the PPO learner (pp3_learner_draw_noise, pp3_permute_by_bits,
pp3_learner_shuffle_env_index; their query pp3_learner_rng_buffers): exported, declared in
include/pupper_hip.h, bound, and refusing bad arguments before any GPU work (no GPU here)."""
import ctypes as C
import os
import re

from pupperv3_mjx import _abi, _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pupper_hip.h")
ENTRY_POINTS = ("pp3_learner_draw_noise", "pp3_permute_by_bits", "pp3_learner_shuffle_env_index",
                "pp3_learner_rng_buffers")
FAKE = C.c_void_p(16)  # a non-null address no refused call may follow


def _refused(L, fn, args):
    assert getattr(L, fn)(*args) == 1, (fn, args)  # PP3_ERR_ARG
    assert fn.encode() in L.pp3_learn_last_error(), L.pp3_learn_last_error()


def test_entry_points_are_exported_declared_and_bound():
    L = _lib.load()
    src = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int


def test_draw_noise_refuses_bad_arguments_without_gpu_work():
    L = _lib.load()
    key = (C.c_uint32 * 2)(0, 1)
    out = C.c_void_p(0x55)
    good = dict(h=FAKE, key=key, K=20, N=4096, part=1, out=C.byref(out), stream=None)
    for change in (dict(h=None), dict(key=None), dict(out=None), dict(K=0), dict(K=-1), dict(N=0), dict(N=-5),
                   dict(K=2 ** 15, N=2 ** 15),             # 12 * 2^30 elements
                   dict(K=1, N=178956971),                 # 12 N = 2^31 + 4
                   dict(K=2 ** 31 - 1, N=2 ** 31 - 1)):    # (the product does not wrap)
        _refused(L, "pp3_learner_draw_noise", {**good, **change}.values())
    assert out.value == 0x55


def test_permute_by_bits_refuses_bad_arguments_without_gpu_work():
    L = _lib.load()
    good = dict(device=0, bits=FAKE, n=64, x=FAKE, stream=None)
    for change in (dict(bits=None), dict(x=None), dict(device=-1), dict(n=0), dict(n=-1),
                   dict(n=_abi.SHUFFLE_MAX_ENVS + 1)):
        _refused(L, "pp3_permute_by_bits", {**good, **change}.values())


def test_shuffle_env_index_refuses_bad_arguments_without_gpu_work():
    L = _lib.load()
    key = (C.c_uint32 * 2)(0, 1)
    good = dict(h=FAKE, key=key, n=4096, part=1, stream=None)
    for change in (dict(h=None), dict(key=None), dict(n=0), dict(n=-1), dict(n=_abi.SHUFFLE_MAX_ENVS + 1)):
        _refused(L, "pp3_learner_shuffle_env_index", {**good, **change}.values())


def test_rng_buffers_refuses_null_arguments():
    L = _lib.load()
    ip, n, zp, cnt = C.c_void_p(), C.c_int32(), C.c_void_p(), C.c_int64()
    good = dict(h=FAKE, ip=C.byref(ip), n=C.byref(n), zp=C.byref(zp), cnt=C.byref(cnt))
    for name in good:
        _refused(L, "pp3_learner_rng_buffers", {**good, name: None}.values())

