"""ctypes binding of the C-ABI in include/pupper_hip.h (libpupper_hip.so, built in-tree).

This is the binding a maintainer adds on the reference side.  There is
no fallback: if the HIP library is missing or no GPU is visible, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PP3_LIB_PATH") or os.path.join(_HERE, "libpupper_hip.so")
_lib = None


class PupperHipError(RuntimeError):
    pass


# The binding table: one line per entry point, "<restype>[?] <name> <argtypes ...>" in the codes of
# CTYPES.  "?" marks an entry an older build of the library lacks (one loaded through PP3_LIB_PATH for
# a kernel A/B): it is skipped when missing.  tests/test_abi.py holds every line against the prototype
# in the header.
_HEADER_TABLE = """
n pp3_abi_version
z pp3_struct_size n
s pp3_last_error
n pp3_device_count
n pp3_create M E i i P
n pp3_destroy p
i pp3_num_envs p
i pp3_state_stride p
i pp3_env_device p
n pp3_reset p p p p
n pp3_step p p p
n pp3_rollout p p l i p p p p
n pp3_set_dr p p
n pp3_set_pipeline_output p i
n pp3_set_terrain p p i
i pp3_terrain_slots p
n pp3_physics_step p p i p
n pp3_set_auto_reset p i
n pp3_set_action_repeat p i
n pp3_field p i P L
n pp3_copy_field_to_host p i p z
n pp3_copy_field_from_host p i p z
n pp3_synchronize p
n pp3_copy_field_to_host_async p i p z
n pp3_outputs_to_host p p
n pp3_host_device_ptr p P
p pp3_stream p
n? pp3_event_create p P
n? pp3_event_record p p
n? pp3_event_synchronize p
n? pp3_event_destroy p
n pp3_device_malloc i z P
n pp3_device_free p
n pp3_memcpy_h2d p p z
n pp3_memcpy_d2h p p z
n pp3_memcpy_d2d p p z p
n pp3_memcpy_h2d_async p p z p
n pp3_host_malloc z P
n pp3_host_free p
n pp3_fill_uniform p p l u u f f p
n pp3_step_timed p p l i F
n pp3_rollout_timed p p l i p p p F
n pp3_render i p p i p i p p i i i F p p
s pp3_render_last_error
n pp3_policy_create i i i p p p P
n pp3_policy_act p p l i p l p
n pp3_policy_out_dim p
n pp3_policy_destroy p
n pp3_rollout_policy p p i p p p p p
n pp3_rollout_policy_timed p p i p p p p F
s pp3_policy_last_error
n? pp3_policy_set_distribution p i f f
n? pp3_policy_sample p p l i p i p l p p p p
n? pp3_rollout_policy_sample p p i p p p p p p p p p
n? pp3_rollout_policy_sample_timed p p i p p p p p p p p F
n? pp3_set_truncation_trajectory p p i
n? pp3_gae i i i l p p p p p f f f p p p
s? pp3_ppo_last_error
n? pp3_eval_reset i i p p
n? pp3_eval_accumulate i i p p p l p l p p
n? pp3_eval_accumulate_rows i i i l p p i i p p
n? pp3_eval_reduce i i p p p
n? pp3_sum_gathered_f32 i p i l p p
n? pp3_eval_column_sums i i p p p p
n? pp3_eval_finish i p i p p
n? pp3_episode_stats_begin i i p l p p p
n? pp3_episode_stats_rows i i i l p p p i p p p p
n? pp3_learner_create i i i p p p i p p p f f l P
n? pp3_learner_destroy p
n? pp3_learner_buffers p i i P L
n? pp3_ppo_loss_grad p i i i i p p p p p p p p p f f f f f i p p
n? pp3_adam_step p f f f f f f p
n? pp3_policy_load_params p p i i p p p p
s? pp3_learn_last_error
n? pp3_learner_normalizer_update p p l f f f p p p p
n? pp3_learner_set_env_index p p i p
n? pp3_ppo_loss_grad_indexed p i i i i p p p p p p p p p f f f f f i p p
n? pp3_grad_clip p f p p
n? pp3_learner_allreduce_grads p p p p
n? pp3_learner_reduce_gathered p p i p p
n? pp3_learner_normalizer_update_ranks p p p l f f f p p p p
n? pp3_learner_draw_noise p p i i i P p
n? pp3_permute_by_bits i p i p p
n? pp3_learner_shuffle_env_index p p i i p
n? pp3_learner_rng_buffers p P I P L
n? pp3_learner_init_params p p i p
n pp3_comm_unique_id p
n pp3_comm_init p i i i P
n pp3_comm_destroy p
i pp3_comm_rank p
i pp3_comm_world p
s pp3_comm_last_error
n pp3_gather p p i i p p
n pp3_gather_rollout p p p p p i i i p p
n? pp3_comm_allgather_f32 p p p l p
i? pp3_comm_device p
n pp3_comm_allreduce p p p i i
n pp3_comm_barrier p
"""
# include/pupper_hip_diag.h: diagnostic entry points (per-phase / per-wave clocks of a -DPP3_PHASE_PROF
# build; the product library exports them only to return PP3_ERR_ARG)
_DIAG_TABLE = """
n pp3_phase_profile Q i i
n pp3_wave_profile U i
i? pp3_rollout_policy_fused p
i? pp3_narrow_cull p
i? pp3_diag_step_variant p i i
"""
# code -> (kind the header must declare, ctypes type); the upper-case codes are typed pointers
CTYPES = {
    "n": ("int", C.c_int), "i": ("int32", C.c_int32), "l": ("int64", C.c_int64), "u": ("uint32", C.c_uint32),
    "z": ("size_t", C.c_size_t), "f": ("float", C.c_float), "p": ("pointer", C.c_void_p), "s": ("pointer", C.c_char_p),
    "P": ("pointer", C.POINTER(C.c_void_p)), "F": ("pointer", C.POINTER(C.c_float)),
    "I": ("pointer", C.POINTER(C.c_int32)), "L": ("pointer", C.POINTER(C.c_int64)),
    "U": ("pointer", C.POINTER(C.c_uint32)), "Q": ("pointer", C.POINTER(C.c_uint64)),
    "M": ("pointer", C.POINTER(_abi.Model)), "E": ("pointer", C.POINTER(_abi.EnvConfig)),
}


def _parse(table: str) -> dict:
    """{name: (restype code, argtype codes, optional)} of a table above."""
    rows = (line.split() for line in table.strip().splitlines())
    return {r[1]: (r[0][0], tuple(r[2:]), r[0].endswith("?")) for r in rows}


BINDINGS = _parse(_HEADER_TABLE)
EXPORTED_SYMBOLS = tuple(BINDINGS)
DIAG_SYMBOLS = tuple(_parse(_DIAG_TABLE))
BINDINGS.update(_parse(_DIAG_TABLE))


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PupperHipError(
            f"HIP extension not built: {LIB_PATH} is missing (run __graft_entry__.build() or make -C "
            "pupperv3-mjx_amd/csrc); there is no CPU fallback for the environment step.")
    L = C.CDLL(LIB_PATH)
    for name, (ret, args, optional) in BINDINGS.items():
        if optional and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = CTYPES[ret][1]
        fn.argtypes = [CTYPES[a][1] for a in args]
    if L.pp3_abi_version() != _abi.ABI_VERSION:
        raise PupperHipError("ABI version mismatch between libpupper_hip.so and pupperv3_mjx/_abi.py")
    if L.pp3_struct_size(0) != C.sizeof(_abi.Model) or L.pp3_struct_size(1) != C.sizeof(_abi.EnvConfig):
        raise PupperHipError("struct layout mismatch between include/pupper_hip.h and pupperv3_mjx/_abi.py")
    _lib = L
    return L


_LAST_ERROR = {"env": "pp3_last_error", "policy": "pp3_policy_last_error", "ppo": "pp3_ppo_last_error",
               "learn": "pp3_learn_last_error", "comm": "pp3_comm_last_error", "render": "pp3_render_last_error"}


def check(rc: int, domain: str = "env") -> None:
    """Raises PupperHipError with the library's message for a non-zero return code; `domain` names the
    part of the library whose pp3_*_last_error holds it."""
    if rc != 0:
        msg = getattr(load(), _LAST_ERROR[domain])().decode(errors="replace")
        raise PupperHipError(f"pupper_hip error {rc}: {msg}")


class BlockPool(list):
    """Free PinnedBlocks of one size.  A retired pool (an unroll length the env no longer uses, a
    closed env) frees its free blocks, and a leased block released into it later is freed at once
    instead of being kept: nothing waits for the cyclic garbage collector."""

    def __init__(self):
        super().__init__()
        self.retired = False

    def release(self, block: "PinnedBlock") -> None:
        if self.retired:
            block.free()
        else:
            self.append(block)

    def retire(self) -> None:
        self.retired = True
        while self:
            self.pop().free()


def _release(pool, block) -> None:
    """A released lease (_BlockRef.__del__): the block goes back to its pool (or is freed there)."""
    if isinstance(pool, BlockPool):
        pool.release(block)
    else:
        pool.append(block)


class PinnedBlock:
    """Page-locked host memory (pp3_host_malloc) exposed to numpy through __array_interface__:
    arrays made from it keep it alive, and when the last one dies the block goes back to its pool
    (BlockPool.release), so host-API output arrays never alias a block that a later step reuses.
    The block does not reference its pool (no reference cycle)."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(load().pp3_host_malloc(max(self.nbytes, 4), C.byref(self.ptr)))
        self.__array_interface__ = {"shape": (self.nbytes // 4,), "typestr": "<f4", "version": 3,
                                    "data": (self.ptr.value, False)}
        # (a lease's arrays are read-only from the start: no per-view flag update)
        self._ro_interface = dict(self.__array_interface__, data=(self.ptr.value, True))
        self._dev = None

    def device_ptr(self) -> int:
        """The block's device address (pp3_host_device_ptr; cached): kernels store into it directly."""
        if self._dev is None:
            d = C.c_void_p()
            check(load().pp3_host_device_ptr(self.ptr, C.byref(d)))
            self._dev = d.value
        return self._dev

    @staticmethod
    def take(nbytes: int, pool: list) -> "_BlockRef":
        """A block from `pool` (a BlockPool of free blocks) or a new one, leased: it returns there when
        the lease and every array made from it have died.  The lease's arrays are read-only (the
        blocks hold launch outputs the host only reads)."""
        b = pool.pop() if pool else PinnedBlock(nbytes)
        return _BlockRef(b, pool)

    def free(self) -> None:
        if self.ptr:
            load().pp3_host_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _BlockRef:
    """One lease of a PinnedBlock: numpy arrays made from it reference this object, whose death
    returns the block to its pool (__del__: reference counting releases it the moment the last
    array dies, without a weakref.finalize registration per lease)."""

    def __init__(self, block: PinnedBlock, pool: list):
        self.block = block
        self.ptr = block.ptr
        self._pool = pool
        self.__array_interface__ = block._ro_interface

    def __del__(self):
        pool, self._pool = self._pool, None
        if pool is not None:
            try:
                _release(pool, self.block)
            except Exception:  # (interpreter shutdown)
                pass

    def device_ptr(self) -> int:
        return self.block.device_ptr()


class DeviceBuffer:
    """Minimal owning device allocation (no torch needed)."""

    def __init__(self, nbytes: int, device: int = 0):
        L = load()
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(L.pp3_device_malloc(device, max(self.nbytes, 4), C.byref(self.ptr)))

    def upload(self, arr) -> None:
        import numpy as np
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        check(load().pp3_memcpy_h2d(self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, arr) -> None:
        check(load().pp3_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), self.ptr, arr.nbytes))

    def free(self) -> None:
        if self.ptr:
            load().pp3_device_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffers:
    """Named device buffers of one owner, kept between calls and grown on demand."""

    def __init__(self, device: int = 0):
        self.device = int(device)
        self._bufs = {}

    def get(self, name: str, nbytes: int) -> DeviceBuffer:
        """The buffer kept under `name`; one too small is freed and allocated anew (its address changes)."""
        b = self._bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self._bufs[name] = DeviceBuffer(nbytes, self.device)
        return b

    def free_all(self) -> None:
        while self._bufs:
            self._bufs.popitem()[1].free()
