// pp3_env_host.h -- what the env library's three translation units share on the host and the C ABI
// does not show: pp3_env.hip (the kernels and their launches), pp3_host.hip (the rest of the ABI:
// handle, fields, copies, events, memory, timed wrappers) and pp3_model.hip (the host model
// builder).  pp3_learn.hip takes the host threefry from here.  Nothing in it is exported: hidden
// visibility throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "pupper_hip.h"

namespace pp3 {
struct DevModel;  // pp3_device.h
}

#pragma GCC visibility push(hidden)

struct pp3_env {
  int device;
  int N;
  int stride;
  int H;
  int La, Li;  // latency rows' lengths (with H: which size caps the step kernels are launched with)
  hipStream_t stream;
  pp3::DevModel* dmodel;
  float* state;
  float* obs;  // [N][36H], updated in place by every step (stable pointer: pp3_field(PP3_F_OBS))
  float* reward;
  float* done;
  float* metrics;
  float* dr;
  int dr_on;
  float* pipe;
  int pipe_on;
  int nc;  // contact cap (kernel template): 8 on flat terrain, 16 with obstacle geoms
  float* action;
  float* episode;      // auto-reset mode buffers (null when off)
  float* first_state;
  float* first_obs;
  int episode_length;
  int action_repeat;  // auto-reset mode: launches per wrapper step (1 otherwise)
  float* terrain;  // TerrainRec[N padded to whole 16-env workgroups][nbox] (pp3_set_terrain), null until first set
  int nbox;        // world box-geom slots in the model
  int cull;        // DevModel::cull_on: steps launch env_step_kernel<..., CULL = true>
  int partitionable;  // the config's rng_partitionable (the sampled policy rollout's host key chain)
  float* traj_trunc;  // pp3_set_truncation_trajectory: the rollouts' truncation rows (caller's buffer) or null
  int trunc_steps;    // its capacity in steps
  hipEvent_t ev0, ev1;
};

// the one thread-local message behind pp3_last_error (pp3_host.hip); returns code
int set_err(int code, const std::string& msg);
#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return set_err(PP3_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// pp3_env.hip: PP3_DIAG_BUILD of pp3_diag.h (that header also defines the diagnostic builds' device
// symbols, so only the kernels' translation unit includes it)
bool diag_build();

inline hipStream_t stream_of(pp3_env_t* e, void* s) { return s ? (hipStream_t)s : e->stream; }

// pp3_model.hip: float64 host arithmetic only, no HIP runtime call
int build_devmodel(const pp3_model_t* mm, const pp3_env_config_t* c, pp3::DevModel* d);
void quat2mat_d(const double q[4], double R[9]);
namespace pp3 {
namespace model_limits {  // what build_devmodel checks the model against: the kernels' HMAX and
constexpr int HMAX = 16;  // NROBOT_GEOM, which live with the device code (pp3_env.hip asserts that
constexpr int NROBOT_GEOM = 8;  // these are equal to them)
}  // namespace model_limits
}  // namespace pp3

// Host restatement of threefry (pp3_device.h threefry and pp3_mlp.h head_threefry are the device's)
inline void host_threefry(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1, uint32_t& y0, uint32_t& y1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  static const int rot[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  x0 += k0;
  x1 += k1;
  for (int i = 0; i < 5; i++) {
    for (int q = 0; q < 4; q++) {
      x0 += x1;
      x1 = (x1 << rot[i & 1][q]) | (x1 >> (32 - rot[i & 1][q]));
      x1 ^= x0;
    }
    x0 += ks[(i + 1) % 3];
    x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
  }
  y0 = x0;
  y1 = x1;
}
// jax.random.split(k): out[2i], out[2i + 1] = the words of split(k)[i], i in {0, 1}
inline void host_split(uint32_t k0, uint32_t k1, int part, uint32_t out[4]) {
  if (part) {
    host_threefry(k0, k1, 0u, 0u, out[0], out[1]);
    host_threefry(k0, k1, 0u, 1u, out[2], out[3]);
  } else {  // flat words [y0(0,2), y0(1,3), y1(0,2), y1(1,3)]: key i = words 2i, 2i + 1
    host_threefry(k0, k1, 0u, 2u, out[0], out[2]);
    host_threefry(k0, k1, 1u, 3u, out[1], out[3]);
  }
}

#pragma GCC visibility pop
