// pp3_ppo.hip -- Brax PPO's value targets on the device (pp3_gae): generalised advantage
// estimation over a collected unroll ([ext] brax 0.12.1 training/agents/ppo/losses.py compute_gae,
// restated from memory; the recurrence in include/pupper_hip.h is the contract).
//
// One lane per env: every row load and store is coalesced over N.  The K steps are a serial
// dependent chain per lane (t = K-1 .. 0); the loads do not depend on it, so they are issued GAE_U
// steps at a time, one group ahead of the chain, instead of one exposed memory latency per step.
// Every *, + and - is rounded on its own, in the association of the contract, so the result is the
// f32 restatement's bit for bit: plain operators under `#pragma clang fp contract(off)` (hipcc
// contracts them into fused multiply-adds by default, and HIP's __fmul_rn / __fadd_rn are plain
// operators in its headers, contracted like any other: a first version built on them was 1 ulp
// off the restatement).
#include <hip/hip_runtime.h>

#include <math.h>

#include <string>

#include "pupper_hip.h"

namespace pp3ppo {

constexpr int GAE_U = 4;  // steps whose loads are in flight together
constexpr int GAE_BLOCK = 256;

struct GaeArgs {
  const float* reward;      // [nsteps][row_stride]
  const float* done;
  const float* truncation;
  const float* values;
  const float* bootstrap;   // [n]
  float* vs;                // [nsteps][row_stride]
  float* adv;
  int64_t row_stride;
  int nsteps, n;
  float discount, lambda, reward_scaling;
};

struct GaeRows {
  float r[GAE_U], d[GAE_U], tr[GAE_U], v[GAE_U];
};

// rows t0, t0 - 1, .. t0 - GAE_U + 1 of lane i (those >= 0)
__device__ __forceinline__ void gae_load(const GaeArgs& a, int t0, int i, GaeRows& w) {
#pragma unroll
  for (int j = 0; j < GAE_U; j++) {
    const int t = t0 - j;
    if (t >= 0) {
      const size_t at = (size_t)t * (size_t)a.row_stride + (size_t)i;
      w.r[j] = a.reward[at];
      w.d[j] = a.done[at];
      w.tr[j] = a.truncation[at];
      w.v[j] = a.values[at];
    } else {
      w.r[j] = w.d[j] = w.tr[j] = w.v[j] = 0.0f;
    }
  }
}

__global__ __launch_bounds__(GAE_BLOCK) void gae_kernel(GaeArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * GAE_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  float vnext = a.bootstrap[i];  // values[t + 1]
  float vsnext = vnext;          // vs[t + 1]
  float acc = 0.0f;
  GaeRows cur, nxt;
  gae_load(a, a.nsteps - 1, i, cur);
  for (int t0 = a.nsteps - 1; t0 >= 0; t0 -= GAE_U) {
    gae_load(a, t0 - GAE_U, i, nxt);  // the next group's loads, ahead of this group's chain
#pragma unroll
    for (int j = 0; j < GAE_U; j++) {
      const int t = t0 - j;
      if (t >= 0) {
        const float v = cur.v[j];
        const float tm = 1.0f - cur.tr[j];
        const float term = cur.d[j] * tm;
        const float g = a.discount * (1.0f - term);
        const float r = cur.r[j] * a.reward_scaling;
        const float delta = ((r + g * vnext) - v) * tm;
        acc = delta + (((g * tm) * a.lambda) * acc);
        const float vs = acc + v;
        const float ad = ((r + g * vsnext) - v) * tm;
        const size_t at = (size_t)t * (size_t)a.row_stride + (size_t)i;
        a.vs[at] = vs;
        a.adv[at] = ad;
        vnext = v;
        vsnext = vs;
      }
    }
    cur = nxt;
  }
}

}  // namespace pp3ppo

using namespace pp3ppo;

static thread_local std::string g_ppo_err;
static int ppo_err(int code, const std::string& m) {
  g_ppo_err = m;
  return code;
}
#define PPOHIP(x)                                                                                     \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) return ppo_err(PP3_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

extern "C" {

const char* pp3_ppo_last_error(void) { return g_ppo_err.c_str(); }

int pp3_gae(int32_t device, int32_t nsteps, int32_t n, int64_t row_stride, const float* reward, const float* done,
            const float* truncation, const float* values, const float* bootstrap, float discount, float lambda,
            float reward_scaling, float* vs, float* adv, void* stream) {
  if (!reward || !done || !truncation || !values || !bootstrap || !vs || !adv)
    return ppo_err(PP3_ERR_ARG, "pp3_gae: null argument");
  if (nsteps < 1 || n < 1) return ppo_err(PP3_ERR_ARG, "pp3_gae: nsteps and n must be >= 1");
  if (row_stride < n) return ppo_err(PP3_ERR_ARG, "pp3_gae: row_stride shorter than n");
  if (!isfinite(discount) || !isfinite(lambda) || !isfinite(reward_scaling))
    return ppo_err(PP3_ERR_ARG, "pp3_gae: discount, lambda and reward_scaling must be finite");
  const float* ins[] = {reward, done, truncation, values, bootstrap};
  for (const float* p : ins)
    if (p == vs || p == adv) return ppo_err(PP3_ERR_ARG, "pp3_gae: in-place is not supported (an output aliases an input)");
  if (vs == adv) return ppo_err(PP3_ERR_ARG, "pp3_gae: vs and adv must be different buffers");
  PPOHIP(hipSetDevice(device));
  GaeArgs a;
  a.reward = reward;
  a.done = done;
  a.truncation = truncation;
  a.values = values;
  a.bootstrap = bootstrap;
  a.vs = vs;
  a.adv = adv;
  a.row_stride = row_stride;
  a.nsteps = nsteps;
  a.n = n;
  a.discount = discount;
  a.lambda = lambda;
  a.reward_scaling = reward_scaling;
  hipLaunchKernelGGL(gae_kernel, dim3((n + GAE_BLOCK - 1) / GAE_BLOCK), dim3(GAE_BLOCK), 0, (hipStream_t)stream, a);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

}  // extern "C"
