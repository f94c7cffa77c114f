// pp3_host.hip -- the env library's C ABI that launches no kernel of pp3_env.hip: handle lifetime,
// getters, events, the pp3_set_* switches, per-env terrain, fields and their copies, host and
// device memory, the timed wrappers.  Nothing here decides a kernel's code: an edit to this file
// leaves the kernel source hash, and so a measured counter profile, valid.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pp3_device.h"
#include "pp3_env_host.h"
#include "pp3_mlp.h"

using namespace pp3;

// envs per workgroup of the largest launch (the policy rollouts: one MLP tile, two envs per wave)
constexpr int TERRAIN_ROW_PAD = pp3pol::TILE;
static_assert(TERRAIN_ROW_PAD == 2 * pp3pol::NWAVE && TERRAIN_ROW_PAD % 2 == 0, "terrain rows cover whole workgroups");

static thread_local std::string g_err;
int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" {

int pp3_abi_version(void) { return PP3_ABI_VERSION; }

const char* pp3_last_error(void) { return g_err.c_str(); }

int pp3_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int alloc_env_buffers(pp3_env* e, const DevModel& hm);

int pp3_create(const pp3_model_t* model, const pp3_env_config_t* cfg, int32_t num_envs, int32_t device, pp3_env_t** out) {
  if (!model || !cfg || !out || num_envs < 1) return set_err(PP3_ERR_ARG, "bad arguments to pp3_create");
  if (diag_build()) {  // pp3_diag.h: a diagnostic library is never the product
    const char* ok = getenv("PP3_ALLOW_DIAG_BUILD");
    if (!ok || strcmp(ok, "1") != 0)
      return set_err(PP3_ERR_ARG, "pp3_create: this library is a diagnostic build (PP3_PHASE_PROF / PP3_DEBUG); "
                                  "set PP3_ALLOW_DIAG_BUILD=1 to use it for diagnostics");
  }
  DevModel hm;
  int rc = build_devmodel(model, cfg, &hm);
  if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  pp3_env* e = new pp3_env();
  memset(e, 0, sizeof(*e));
  e->action_repeat = 1;
  e->device = device;
  e->N = num_envs;
  e->stride = hm.stride;
  e->H = hm.H;
  e->La = hm.La;
  e->Li = hm.Li;
  e->partitionable = hm.partitionable;
  e->nbox = hm.nbox;
  e->cull = hm.cull_on;
  {
    // contact cap: 8 deepest per env by default, flat or with obstacle boxes (the reference's
    // MJX keeps max_contact_points = 5, test_pupper_model.xml:227-230); 16 on request
    e->nc = cfg->ncon_max > 0 ? cfg->ncon_max : 8;
    if (e->nc != 8 && e->nc != 16) {
      delete e;
      return set_err(PP3_ERR_ARG, "ncon_max must be 0 (auto), 8 or 16");
    }
  }
  rc = alloc_env_buffers(e, hm);
  if (rc) {
    pp3_destroy(e);  // frees what was allocated (hipFree(nullptr) is a no-op)
    return rc;
  }
  *out = e;
  return PP3_OK;
}

// device buffers of a new handle (pp3_create); on failure the caller destroys the handle
static int alloc_env_buffers(pp3_env* e, const DevModel& hm) {
  const size_t N = (size_t)e->N;
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  HIPCHK(hipMalloc(&e->dmodel, sizeof(DevModel)));
  HIPCHK(hipMemcpy(e->dmodel, &hm, sizeof(DevModel), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&e->state, N * e->stride * sizeof(float)));
  HIPCHK(hipMalloc(&e->obs, N * PP3_OBS_DIM * e->H * sizeof(float)));
  HIPCHK(hipMalloc(&e->reward, N * sizeof(float)));
  HIPCHK(hipMalloc(&e->done, N * sizeof(float)));
  HIPCHK(hipMalloc(&e->metrics, N * PP3_NMETRIC * sizeof(float)));
  HIPCHK(hipMalloc(&e->dr, N * PP3_NDR * sizeof(float)));
  HIPCHK(hipMalloc(&e->pipe, N * PP3_PIPE_STRIDE * sizeof(float)));
  HIPCHK(hipMalloc(&e->action, N * PP3_NU * sizeof(float)));
  HIPCHK(hipMemset(e->state, 0, N * e->stride * sizeof(float)));
  HIPCHK(hipMemset(e->obs, 0, N * PP3_OBS_DIM * e->H * sizeof(float)));
  HIPCHK(hipMemset(e->pipe, 0, N * PP3_PIPE_STRIDE * sizeof(float)));
  HIPCHK(hipMemset(e->action, 0, N * PP3_NU * sizeof(float)));
  HIPCHK(hipEventCreate(&e->ev0));
  HIPCHK(hipEventCreate(&e->ev1));
  return PP3_OK;
}

int pp3_destroy(pp3_env_t* e) {
  if (!e) return PP3_OK;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  void* bufs[] = {e->dmodel, e->state, e->obs, e->reward, e->done, e->metrics, e->dr, e->pipe, e->action,
                  e->episode, e->first_state, e->first_obs, e->terrain};
  for (void* b : bufs) (void)hipFree(b);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return PP3_OK;
}

int32_t pp3_num_envs(const pp3_env_t* e) { return e ? e->N : 0; }
int32_t pp3_state_stride(const pp3_env_t* e) { return e ? e->stride : 0; }
int32_t pp3_env_device(const pp3_env_t* e) { return e ? e->device : -1; }

int32_t pp3_narrow_cull(const pp3_env_t* e) { return e ? (e->cull ? 1 : 0) : -1; }

void* pp3_stream(pp3_env_t* e) { return e ? (void*)e->stream : nullptr; }

// completion markers of the host API's asynchronous step (timing disabled: a record is one packet)
int pp3_event_create(pp3_env_t* e, void** out) {
  if (!e || !out) return set_err(PP3_ERR_ARG, "pp3_event_create: null argument");
  HIPCHK(hipSetDevice(e->device));
  hipEvent_t ev;
  HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  *out = (void*)ev;
  return PP3_OK;
}
int pp3_event_record(pp3_env_t* e, void* ev) {
  if (!e || !ev) return set_err(PP3_ERR_ARG, "pp3_event_record: null argument");
  HIPCHK(hipEventRecord((hipEvent_t)ev, e->stream));
  return PP3_OK;
}
int pp3_event_synchronize(void* ev) {
  if (!ev) return set_err(PP3_ERR_ARG, "pp3_event_synchronize: null event");
  HIPCHK(hipEventSynchronize((hipEvent_t)ev));
  return PP3_OK;
}
int pp3_event_destroy(void* ev) {
  if (ev) HIPCHK(hipEventDestroy((hipEvent_t)ev));
  return PP3_OK;
}

int pp3_set_auto_reset(pp3_env_t* e, int32_t episode_length) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  if (episode_length > 0 && !e->episode) {
    HIPCHK(hipMalloc(&e->episode, sizeof(float) * (size_t)e->N * PP3_EP_STRIDE));
    HIPCHK(hipMalloc(&e->first_state, sizeof(float) * (size_t)e->N * PP3_FIRST_STRIDE));
    HIPCHK(hipMalloc(&e->first_obs, sizeof(float) * (size_t)e->N * PP3_OBS_DIM * e->H));
    HIPCHK(hipMemsetAsync(e->episode, 0, sizeof(float) * (size_t)e->N * PP3_EP_STRIDE, e->stream));
    // until the next pp3_reset the current state is the "first" state
    HIPCHK(hipMemcpy2DAsync(e->first_state, sizeof(float) * PP3_FIRST_STRIDE, e->state, sizeof(float) * e->stride,
                            sizeof(float) * PP3_FIRST_STRIDE, e->N, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->first_obs, e->obs, sizeof(float) * (size_t)e->N * PP3_OBS_DIM * e->H,
                          hipMemcpyDeviceToDevice, e->stream));
  }
  e->episode_length = episode_length > 0 ? episode_length : 0;
  if (e->episode_length == 0) e->action_repeat = 1;
  return PP3_OK;
}

int pp3_set_truncation_trajectory(pp3_env_t* e, float* trunc_dev, int32_t max_steps) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  if (trunc_dev && max_steps < 1) return set_err(PP3_ERR_ARG, "pp3_set_truncation_trajectory: max_steps must be >= 1");
  e->traj_trunc = trunc_dev;
  e->trunc_steps = trunc_dev ? max_steps : 0;
  return PP3_OK;
}

int pp3_set_action_repeat(pp3_env_t* e, int32_t action_repeat) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  if (action_repeat < 1) return set_err(PP3_ERR_ARG, "action_repeat must be >= 1");
  if (action_repeat > 1 && e->episode_length <= 0)
    return set_err(PP3_ERR_ARG, "action_repeat > 1 needs auto-reset mode (pp3_set_auto_reset first)");
  e->action_repeat = action_repeat;
  return PP3_OK;
}

int pp3_set_dr(pp3_env_t* e, const float* dr_dev) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  if (!dr_dev) { e->dr_on = 0; return PP3_OK; }
  HIPCHK(hipMemcpyAsync(e->dr, dr_dev, (size_t)e->N * PP3_NDR * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  e->dr_on = 1;
  return PP3_OK;
}

int32_t pp3_terrain_slots(const pp3_env_t* e) { return e ? e->nbox : 0; }

int pp3_set_terrain(pp3_env_t* e, const float* boxes, int32_t n_boxes) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  uint64_t ptr = 0;
  if (boxes) {
    if (n_boxes != e->nbox)
      return set_err(PP3_ERR_ARG, "pp3_set_terrain: n_boxes must equal the model's world box-geom count (" +
                                      std::to_string(e->nbox) + ")");
    if (n_boxes == 0) return set_err(PP3_ERR_ARG, "pp3_set_terrain: the model has no box geoms to use as slots");
    // The kernels index the table by the unclamped env slot of the launch: 2 * block + half in the
    // one-wave launches, and every slot of the policy rollouts' whole TERRAIN_ROW_PAD-env workgroups
    // (the waves past N still run the physics).  So the rows are padded to a multiple of the largest
    // workgroup, and a padding row holds absent boxes.
    const size_t rows = ((size_t)e->N + TERRAIN_ROW_PAD - 1) / TERRAIN_ROW_PAD * TERRAIN_ROW_PAD;
    std::vector<TerrainRec> rec(rows * n_boxes);
    memset(rec.data(), 0, rec.size() * sizeof(TerrainRec));
    for (size_t i = 0; i < rows; i++)
      for (int b = 0; b < n_boxes; b++) {
        TerrainRec& r = rec[i * n_boxes + b];
        const float* x = i < (size_t)e->N ? boxes + (i * n_boxes + b) * PP3_TERRAIN_BOX : nullptr;
        // a padding row or an absent box: far below the floor, zero size, identity rotation (a zero
        // rotation would map every sphere centre to the box centre: a contact with each)
        if (!x || !(x[7] > 0 || x[8] > 0 || x[9] > 0)) {
          r.p[2] = -1e4f;
          r.R[0] = r.R[4] = r.R[8] = 1.0f;
          continue;
        }
        double q[4] = {x[3], x[4], x[5], x[6]};
        const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!(qn > 0)) return set_err(PP3_ERR_ARG, "pp3_set_terrain: zero quaternion");
        for (int k = 0; k < 4; k++) q[k] /= qn;
        double R[9];
        quat2mat_d(q, R);
        for (int k = 0; k < 3; k++) { r.p[k] = x[k]; r.half[k] = x[7 + k]; }
        for (int k = 0; k < 9; k++) r.R[k] = (float)R[k];
      }
    HIPCHK(hipStreamSynchronize(e->stream));
    if (!e->terrain) HIPCHK(hipMalloc(&e->terrain, rows * n_boxes * sizeof(TerrainRec)));
    HIPCHK(hipMemcpy(e->terrain, rec.data(), rec.size() * sizeof(TerrainRec), hipMemcpyHostToDevice));
    ptr = (uint64_t)(uintptr_t)e->terrain;
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  HIPCHK(hipMemcpy((char*)e->dmodel + offsetof(DevModel, terrain), &ptr, sizeof(ptr), hipMemcpyHostToDevice));
  return PP3_OK;
}

int pp3_set_pipeline_output(pp3_env_t* e, int32_t enable) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  e->pipe_on = enable ? 1 : 0;
  return PP3_OK;
}

int pp3_field(pp3_env_t* e, int32_t field, void** ptr, int64_t* elems) {
  if (!e || !ptr) return set_err(PP3_ERR_ARG, "null argument");
  int64_t n = 0;
  void* p = nullptr;
  switch (field) {
    case PP3_F_STATE: p = e->state; n = e->stride; break;
    case PP3_F_OBS: p = e->obs; n = (int64_t)PP3_OBS_DIM * e->H; break;
    case PP3_F_REWARD: p = e->reward; n = 1; break;
    case PP3_F_DONE: p = e->done; n = 1; break;
    case PP3_F_METRICS: p = e->metrics; n = PP3_NMETRIC; break;
    case PP3_F_DR: p = e->dr; n = PP3_NDR; break;
    case PP3_F_PIPELINE: p = e->pipe; n = PP3_PIPE_STRIDE; break;
    case PP3_F_ACTION: p = e->action; n = PP3_NU; break;
    case PP3_F_EPISODE: p = e->episode; n = PP3_EP_STRIDE; break;
    case PP3_F_FIRST_STATE: p = e->first_state; n = PP3_FIRST_STRIDE; break;
    case PP3_F_FIRST_OBS: p = e->first_obs; n = (int64_t)PP3_OBS_DIM * e->H; break;
    default: return set_err(PP3_ERR_ARG, "unknown field");
  }
  *ptr = p;
  if (elems) *elems = n;
  return PP3_OK;
}

}  // extern "C"

// What the three field copies of `fn` check first: the field's device pointer for a host block of
// `bytes`, with the env's device current (`hint`: how a missing field gets allocated)
static int copy_field_ptr(pp3_env_t* e, int32_t field, size_t bytes, const std::string& fn, const char* hint, void** p) {
  int64_t n;
  int rc = pp3_field(e, field, p, &n);
  if (rc) return rc;
  if (bytes != (size_t)n * e->N * 4) return set_err(PP3_ERR_ARG, fn + ": size mismatch");
  if (!*p) return set_err(PP3_ERR_ARG, fn + ": field not allocated" + hint);
  HIPCHK(hipSetDevice(e->device));
  return PP3_OK;
}
static const char* const AUTO_RESET_HINT = " (auto-reset fields need pp3_set_auto_reset)";

extern "C" {

int pp3_copy_field_to_host(pp3_env_t* e, int32_t field, void* host, size_t bytes) {
  void* p;
  int rc = copy_field_ptr(e, field, bytes, "pp3_copy_field_to_host", AUTO_RESET_HINT, &p);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost));
  return PP3_OK;
}

int pp3_copy_field_from_host(pp3_env_t* e, int32_t field, const void* host, size_t bytes) {
  void* p;
  int rc = copy_field_ptr(e, field, bytes, "pp3_copy_field_from_host", AUTO_RESET_HINT, &p);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  if (field == PP3_F_DR) e->dr_on = 1;
  return PP3_OK;
}

int pp3_copy_field_to_host_async(pp3_env_t* e, int32_t field, void* host, size_t bytes) {
  void* p;
  int rc = copy_field_ptr(e, field, bytes, "pp3_copy_field_to_host_async", "", &p);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, e->stream));
  return PP3_OK;
}

int pp3_synchronize(pp3_env_t* e) {
  if (!e) return set_err(PP3_ERR_ARG, "null env");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipDeviceSynchronize());
  return PP3_OK;
}

int pp3_host_device_ptr(void* host, void** dev) {
  if (!host || !dev) return set_err(PP3_ERR_ARG, "pp3_host_device_ptr: null argument");
  *dev = nullptr;
  if (hipHostGetDevicePointer(dev, host, 0) != hipSuccess || !*dev)
    return set_err(PP3_ERR_ARG, "pp3_host_device_ptr: not page-locked memory from pp3_host_malloc");
  return PP3_OK;
}

int pp3_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return PP3_OK;
}

int pp3_host_malloc(size_t bytes, void** out) {
  if (!out) return set_err(PP3_ERR_ARG, "pp3_host_malloc: null output");
  HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return PP3_OK;
}
int pp3_host_free(void* p) {
  HIPCHK(hipHostFree(p));
  return PP3_OK;
}

int pp3_device_malloc(int32_t device, size_t bytes, void** out) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(out, bytes));
  return PP3_OK;
}
int pp3_device_free(void* p) {
  HIPCHK(hipFree(p));
  return PP3_OK;
}
int pp3_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return PP3_OK;
}
int pp3_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return PP3_OK;
}
int pp3_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PP3_OK;
}

}  // extern "C"

// The *_timed entry points: what `launch` puts on the env's stream between two events, and the
// time between them once the second has completed
template <class F>
static int timed(pp3_env_t* e, float* kernel_ms_total, F launch) {
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  const int rc = launch();
  if (rc) return rc;
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipEventSynchronize(e->ev1));
  HIPCHK(hipEventElapsedTime(kernel_ms_total, e->ev0, e->ev1));
  return PP3_OK;
}

extern "C" {

int pp3_step_timed(pp3_env_t* e, const float* actions_dev, int64_t action_stride, int32_t nsteps,
                   float* kernel_ms_total) {
  if (!e || !actions_dev || !kernel_ms_total) return set_err(PP3_ERR_ARG, "null argument");
  return timed(e, kernel_ms_total, [&] {
    for (int i = 0; i < nsteps; i++) {
      int rc = pp3_step(e, actions_dev + (size_t)i * (size_t)action_stride, e->stream);
      if (rc) return rc;
    }
    return (int)PP3_OK;
  });
}

int pp3_rollout_timed(pp3_env_t* e, const float* actions_dev, int64_t action_stride, int32_t nsteps,
                      float* reward_dev, float* done_dev, float* obs_dev, float* kernel_ms_total) {
  if (!e || !actions_dev || !kernel_ms_total) return set_err(PP3_ERR_ARG, "null argument");
  return timed(e, kernel_ms_total, [&] {
    return pp3_rollout(e, actions_dev, action_stride, nsteps, reward_dev, done_dev, obs_dev, e->stream);
  });
}

int pp3_rollout_policy_timed(pp3_env_t* e, pp3_policy_t* policy, int32_t nsteps, float* actions_dev,
                             float* reward_dev, float* done_dev, float* obs_dev, float* kernel_ms_total) {
  if (!e || !policy || !actions_dev || !kernel_ms_total) return set_err(PP3_ERR_ARG, "null argument");
  return timed(e, kernel_ms_total, [&] {
    return pp3_rollout_policy(e, policy, nsteps, actions_dev, reward_dev, done_dev, obs_dev, e->stream);
  });
}

int pp3_rollout_policy_sample_timed(pp3_env_t* e, pp3_policy_t* policy, int32_t nsteps, const uint32_t* key,
                                    uint32_t* key_out, float* actions_dev, float* raw_dev, float* logp_dev,
                                    float* reward_dev, float* done_dev, float* obs_dev, float* kernel_ms_total) {
  if (!e || !policy || !key || !key_out || !actions_dev || !kernel_ms_total) return set_err(PP3_ERR_ARG, "null argument");
  return timed(e, kernel_ms_total, [&] {
    return pp3_rollout_policy_sample(e, policy, nsteps, key, key_out, actions_dev, raw_dev, logp_dev, reward_dev, done_dev,
                                     obs_dev, e->stream);
  });
}

}  // extern "C"
