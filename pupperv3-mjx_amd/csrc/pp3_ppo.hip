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
//
// PPO evaluation (pp3_eval_*): Brax's EvalWrapper accumulator and the Evaluator's mean / std over the
// eval envs, in the same style.  The accumulator is column-major ([22][n]), so one lane per env reads
// and writes every column coalesced; pp3_eval_accumulate follows one wrapper step and reads the env's
// own reward / done / metrics / episode buffers, pp3_eval_accumulate_rows follows a fused K-step
// launch and chains over its reward / done rows with the loads a group ahead, as gae_kernel does.
// pp3_eval_reduce is one 1024-lane workgroup with the learner's scalar-sum order (csrc/pp3_learn.hip
// block_sum) and its residual-corrected quotient and square root, restated here under contract(off).
//
// Training episode statistics (pp3_episode_stats_*): EpisodeWrapper's sum_reward / length record
// rebuilt from a collected batch's reward / done / truncation rows, the same one-lane-per-env chain
// with the loads a group ahead, then the evaluation reduce's one-workgroup sum of the four per-env
// columns.  pp3_sum_gathered_f32, pp3_eval_column_sums and pp3_eval_finish cut pp3_eval_reduce at the
// two places where a sum over ranks goes in; on one rank's data they are its bits.
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

// ---- PPO evaluation ----
constexpr int EVAL_NCOL = PP3_EVAL_NCOL;   // episode_metrics: total_dist, the 18 reward terms, reward
constexpr int EVAL_ACTIVE = PP3_EVAL_ACTIVE;
constexpr int EVAL_STEPS = PP3_EVAL_STEPS;
constexpr int EVAL_WORDS = PP3_EVAL_WORDS;
constexpr int EVAL_NOUT = PP3_EVAL_NOUT;   // reduced columns: the 20 metrics, then episode_steps
constexpr int EVAL_BLOCK = 256;
constexpr int EVAL_U = 4;                  // steps whose loads are in flight together
constexpr int EVAL_RED = 1024;             // the reduce's single workgroup

__global__ __launch_bounds__(EVAL_BLOCK) void eval_reset_kernel(int n, float* __restrict__ acc) {
  const size_t idx = (size_t)blockIdx.x * EVAL_BLOCK + threadIdx.x;
  const size_t n0 = (size_t)n;
  if (idx >= n0 * EVAL_WORDS) return;
  acc[idx] = (idx >= n0 * EVAL_ACTIVE && idx < n0 * (EVAL_ACTIVE + 1)) ? 1.0f : 0.0f;
}

struct EvalStepArgs {
  const float *reward, *done;  // [n]
  const float* metrics;        // [n][metrics_stride], PP3_NMETRIC words read
  const float* episode;        // [n][episode_stride], word PP3_EP_STEPS read
  float* acc;                  // [EVAL_WORDS][n]
  int64_t metrics_stride, episode_stride;
  int n;
};

// One wrapper step.  A lane's 19 metric words are consecutive, so the wave's 19 loads walk the same
// cache lines: each line is fetched once; the accumulator columns are coalesced.
__global__ __launch_bounds__(EVAL_BLOCK) void eval_accumulate_kernel(EvalStepArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const size_t n = (size_t)a.n;
  const float active = a.acc[n * EVAL_ACTIVE + i];
  const float* m = a.metrics + (size_t)i * (size_t)a.metrics_stride;
  float x[EVAL_NCOL];
#pragma unroll
  for (int c = 0; c < PP3_NMETRIC; c++) x[c] = m[c];
  x[EVAL_NCOL - 1] = a.reward[i];
  const float d = a.done[i];
  const float steps = a.episode[(size_t)i * (size_t)a.episode_stride + PP3_EP_STEPS];
  if (active != 0.0f) a.acc[n * EVAL_STEPS + i] = steps;
#pragma unroll
  for (int c = 0; c < EVAL_NCOL; c++) {
    const float em = a.acc[n * c + i];
    a.acc[n * c + i] = em + x[c] * active;
  }
  a.acc[n * EVAL_ACTIVE + i] = active * (1.0f - d);
}

struct EvalRowsArgs {
  const float *reward, *done;  // [nsteps][row_stride]
  float* acc;
  int64_t row_stride;
  int nsteps, n, step0, action_repeat;
};

struct EvalRows {
  float r[EVAL_U], d[EVAL_U];
};

// rows t0 .. t0 + EVAL_U - 1 of lane i; a row past the end reads the last row again (in bounds, and
// the chain does not use it), which keeps the loads free of branches
__device__ __forceinline__ void eval_load(const EvalRowsArgs& a, int t0, int i, EvalRows& w) {
#pragma unroll
  for (int j = 0; j < EVAL_U; j++) {
    const int t = min(t0 + j, a.nsteps - 1);
    const size_t at = (size_t)t * (size_t)a.row_stride + (size_t)i;
    w.r[j] = a.reward[at];
    w.d[j] = a.done[at];
  }
}

// The K steps of a fused launch on the reward column, active and episode_steps: a serial chain per
// lane in step order, the next group's loads issued ahead of this group's chain.
__global__ __launch_bounds__(EVAL_BLOCK) void eval_rows_kernel(EvalRowsArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const size_t n = (size_t)a.n;
  float em = a.acc[n * (EVAL_NCOL - 1) + i];
  float active = a.acc[n * EVAL_ACTIVE + i];
  float es = a.acc[n * EVAL_STEPS + i];
  EvalRows cur, nxt;
  eval_load(a, 0, i, cur);
  for (int t0 = 0; t0 < a.nsteps; t0 += EVAL_U) {
    eval_load(a, t0 + EVAL_U, i, nxt);
#pragma unroll
    for (int j = 0; j < EVAL_U; j++) {
      const int t = t0 + j;
      if (t < a.nsteps) {
        if (active != 0.0f) es = (float)((a.step0 + t + 1) * a.action_repeat);  // (exact: below 2^24)
        em = em + cur.r[j] * active;
        active = active * (1.0f - cur.d[j]);
      }
    }
    cur = nxt;
  }
  a.acc[n * (EVAL_NCOL - 1) + i] = em;
  a.acc[n * EVAL_ACTIVE + i] = active;
  a.acc[n * EVAL_STEPS + i] = es;
}

// pp3_learn.hip's div_rn and block_sum (a / b with one residual step on the build's fast division;
// lane partial sums met in a binary tree in LDS), restated for this file's kernels
__device__ __forceinline__ float eval_div_rn(float a, float b) {
  const float q = a / b;
  return fmaf(fmaf(-q, b, a), 1.0f / b, q);
}

// sqrt(var): the build's fast sqrt is within 1 ulp; one residual step
__device__ __forceinline__ float eval_sqrt_rn(float var) {
  float sd = sqrtf(var);
  if (sd > 0.0f && sd < INFINITY) sd = fmaf(fmaf(-sd, sd, var), 0.5f / sd, sd);
  return sd;
}

__device__ __forceinline__ float eval_block_sum(float v, float* sh) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = EVAL_RED / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

// out[k] = mean, out[EVAL_NOUT + k] = population std over the n envs of reduced column k, one
// workgroup: lane i adds envs i, i + 1024, .. ascending, then the tree; two passes per column.
__global__ __launch_bounds__(EVAL_RED) void eval_reduce_kernel(int n, const float* __restrict__ acc,
                                                               float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float sh[EVAL_RED];
  const float fn = (float)n;
  for (int k = 0; k < EVAL_NOUT; k++) {
    const float* col = acc + (size_t)n * (k < EVAL_NCOL ? k : EVAL_STEPS);
    float s = 0.0f;
    for (int e = threadIdx.x; e < n; e += EVAL_RED) s = s + col[e];
    const float mean = eval_div_rn(eval_block_sum(s, sh), fn);
    float q = 0.0f;
    for (int e = threadIdx.x; e < n; e += EVAL_RED) {
      const float d = col[e] - mean;
      q = q + d * d;
    }
    const float var = eval_div_rn(eval_block_sum(q, sh), fn);
    if (threadIdx.x == 0) {
      out[k] = mean;
      out[EVAL_NOUT + k] = eval_sqrt_rn(var);
    }
  }
}

// ---- evaluation reduce, cut for a sum over ranks ----
// out22[k] = this shard's sum of reduced column k (mean21 == nullptr) or of its squared deviations
// from mean21[k], in eval_reduce_kernel's order; out22[EVAL_NOUT] = n.  One workgroup.
__global__ __launch_bounds__(EVAL_RED) void eval_column_sums_kernel(int n, const float* __restrict__ acc,
                                                                    const float* __restrict__ mean21,
                                                                    float* __restrict__ out22) {
#pragma clang fp contract(off)
  __shared__ float sh[EVAL_RED];
  for (int k = 0; k < EVAL_NOUT; k++) {
    const float* col = acc + (size_t)n * (k < EVAL_NCOL ? k : EVAL_STEPS);
    float s = 0.0f;
    if (mean21) {
      const float mean = mean21[k];
      for (int e = threadIdx.x; e < n; e += EVAL_RED) {
        const float d = col[e] - mean;
        s = s + d * d;
      }
    } else {
      for (int e = threadIdx.x; e < n; e += EVAL_RED) s = s + col[e];
    }
    const float tot = eval_block_sum(s, sh);
    if (threadIdx.x == 0) out22[k] = tot;
  }
  if (threadIdx.x == 0) out22[EVAL_NOUT] = (float)n;
}

// which 0: out42[k] = sums22[k] / sums22[21]; which 1: out42[21 + k] = sqrt(sums22[k] / sums22[21])
__global__ __launch_bounds__(64) void eval_finish_kernel(const float* __restrict__ sums22, int which,
                                                         float* __restrict__ out42) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  if (k >= EVAL_NOUT) return;
  const float q = eval_div_rn(sums22[k], sums22[EVAL_NOUT]);
  if (which == 0)
    out42[k] = q;
  else
    out42[EVAL_NOUT + k] = eval_sqrt_rn(q);
}

// out[i] = ((g_0[i] + g_1[i]) + g_2[i]) + ..: the project's rank-ordered sum, one lane per entry
__global__ __launch_bounds__(EVAL_BLOCK) void sum_gathered_kernel(const float* __restrict__ gathered, int world,
                                                                  int64_t count, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (i >= count) return;
  float s = gathered[i];
  for (int r = 1; r < world; r++) s = s + gathered[(size_t)r * (size_t)count + (size_t)i];
  out[i] = s;
}

// ---- training episode statistics ----
constexpr int EPS_CARRY = 3;  // carry rows: ret, len, pd
constexpr int EPS_PART = 4;   // part rows / out4: episodes, sum of returns, sum of lengths, truncated episodes

__global__ __launch_bounds__(EVAL_BLOCK) void episode_begin_kernel(int n, const float* __restrict__ episode,
                                                                   int64_t episode_stride, const float* __restrict__ done,
                                                                   float* __restrict__ carry) {
  const int i = blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float* ep = episode + (size_t)i * (size_t)episode_stride;
  carry[i] = ep[PP3_EP_SUM_REWARD];
  carry[(size_t)n + i] = ep[PP3_EP_LENGTH];
  carry[2 * (size_t)n + i] = done[i];
}

struct EpisodeRowsArgs {
  const float *reward, *done, *truncation;  // [nsteps][row_stride]; truncation may be null (read as 0)
  float* carry;                             // [3][n]
  float* part;                              // [4][n]
  int64_t row_stride;
  int nsteps, n, action_repeat;
};

struct EpisodeRows {
  float r[EVAL_U], d[EVAL_U], tr[EVAL_U];
};

// rows t0 .. t0 + EVAL_U - 1 of lane i, a row past the end reading the last row again (eval_load)
__device__ __forceinline__ void episode_load(const EpisodeRowsArgs& a, int t0, int i, EpisodeRows& w) {
#pragma unroll
  for (int j = 0; j < EVAL_U; j++) {
    const int t = min(t0 + j, a.nsteps - 1);
    const size_t at = (size_t)t * (size_t)a.row_stride + (size_t)i;
    w.r[j] = a.reward[at];
    w.d[j] = a.done[at];
    w.tr[j] = a.truncation ? a.truncation[at] : 0.0f;
  }
}

// EpisodeWrapper's two lines per step (the step kernel's `(ep_rec + rout) * keep`), sampled at the
// done steps: a serial chain per lane in step order, the next group's loads ahead of this group's.
__global__ __launch_bounds__(EVAL_BLOCK) void episode_rows_kernel(EpisodeRowsArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const size_t n = (size_t)a.n;
  float ret = a.carry[i], len = a.carry[n + i], pd = a.carry[2 * n + i];
  float cnt = 0.0f, sret = 0.0f, slen = 0.0f, strunc = 0.0f;
  const float rep = (float)a.action_repeat;
  EpisodeRows cur, nxt;
  episode_load(a, 0, i, cur);
  for (int t0 = 0; t0 < a.nsteps; t0 += EVAL_U) {
    episode_load(a, t0 + EVAL_U, i, nxt);
#pragma unroll
    for (int j = 0; j < EVAL_U; j++) {
      if (t0 + j < a.nsteps) {
        const float keep = 1.0f - pd;
        ret = (ret + cur.r[j]) * keep;
        len = (len + rep) * keep;
        if (cur.d[j] != 0.0f) {
          cnt = cnt + 1.0f;
          sret = sret + ret;
          slen = slen + len;
          strunc = strunc + cur.tr[j];
        }
        pd = cur.d[j];
      }
    }
    cur = nxt;
  }
  a.carry[i] = ret;
  a.carry[n + i] = len;
  a.carry[2 * n + i] = pd;
  a.part[i] = cnt;
  a.part[n + i] = sret;
  a.part[2 * n + i] = slen;
  a.part[3 * n + i] = strunc;
}

// out4[c] = the sum of part row c over the n envs in eval_reduce_kernel's order.  One workgroup.
__global__ __launch_bounds__(EVAL_RED) void episode_reduce_kernel(int n, const float* __restrict__ part,
                                                                  float* __restrict__ out4) {
#pragma clang fp contract(off)
  __shared__ float sh[EVAL_RED];
  for (int c = 0; c < EPS_PART; c++) {
    const float* col = part + (size_t)n * c;
    float s = 0.0f;
    for (int e = threadIdx.x; e < n; e += EVAL_RED) s = s + col[e];
    const float tot = eval_block_sum(s, sh);
    if (threadIdx.x == 0) out4[c] = tot;
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

// [p, p + np) and [q, q + nq) (floats) share a word
static bool eval_overlap(const float* p, size_t np, const float* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + 4 * nq && b < a + 4 * np;
}

int pp3_eval_reset(int32_t device, int32_t n, float* acc, void* stream) {
  if (!acc) return ppo_err(PP3_ERR_ARG, "pp3_eval_reset: null argument");
  if (n < 1) return ppo_err(PP3_ERR_ARG, "pp3_eval_reset: n must be >= 1");
  PPOHIP(hipSetDevice(device));
  const size_t words = (size_t)n * EVAL_WORDS;
  hipLaunchKernelGGL(eval_reset_kernel, dim3((unsigned)((words + EVAL_BLOCK - 1) / EVAL_BLOCK)), dim3(EVAL_BLOCK), 0,
                     (hipStream_t)stream, n, acc);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_eval_accumulate(int32_t device, int32_t n, const float* reward, const float* done, const float* metrics,
                        int64_t metrics_stride, const float* episode, int64_t episode_stride, float* acc,
                        void* stream) {
  if (!reward || !done || !metrics || !episode || !acc)
    return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate: null argument");
  if (n < 1) return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate: n must be >= 1");
  if (metrics_stride < PP3_NMETRIC) return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate: metrics_stride shorter than PP3_NMETRIC");
  if (episode_stride < PP3_EP_STRIDE) return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate: episode_stride shorter than PP3_EP_STRIDE");
  const size_t n0 = (size_t)n, words = n0 * EVAL_WORDS;
  if (eval_overlap(acc, words, reward, n0) || eval_overlap(acc, words, done, n0) ||
      eval_overlap(acc, words, metrics, n0 * (size_t)metrics_stride) ||
      eval_overlap(acc, words, episode, n0 * (size_t)episode_stride))
    return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate: the accumulator aliases an input");
  PPOHIP(hipSetDevice(device));
  EvalStepArgs a;
  a.reward = reward;
  a.done = done;
  a.metrics = metrics;
  a.episode = episode;
  a.acc = acc;
  a.metrics_stride = metrics_stride;
  a.episode_stride = episode_stride;
  a.n = n;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3((n + EVAL_BLOCK - 1) / EVAL_BLOCK), dim3(EVAL_BLOCK), 0,
                     (hipStream_t)stream, a);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_eval_accumulate_rows(int32_t device, int32_t nsteps, int32_t n, int64_t row_stride, const float* reward,
                             const float* done, int32_t step0, int32_t action_repeat, float* acc, void* stream) {
  if (!reward || !done || !acc) return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate_rows: null argument");
  if (nsteps < 1 || n < 1) return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate_rows: nsteps and n must be >= 1");
  if (row_stride < n) return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate_rows: row_stride shorter than n");
  if (step0 < 0 || action_repeat < 1 || ((int64_t)step0 + nsteps) * action_repeat >= (1 << 24))
    return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate_rows: step0 >= 0, action_repeat >= 1 and (step0 + nsteps) * "
                                "action_repeat < 2^24 are required");
  const size_t words = (size_t)n * EVAL_WORDS, rows = (size_t)(nsteps - 1) * (size_t)row_stride + (size_t)n;
  if (eval_overlap(acc, words, reward, rows) || eval_overlap(acc, words, done, rows))
    return ppo_err(PP3_ERR_ARG, "pp3_eval_accumulate_rows: the accumulator aliases an input");
  PPOHIP(hipSetDevice(device));
  EvalRowsArgs a;
  a.reward = reward;
  a.done = done;
  a.acc = acc;
  a.row_stride = row_stride;
  a.nsteps = nsteps;
  a.n = n;
  a.step0 = step0;
  a.action_repeat = action_repeat;
  hipLaunchKernelGGL(eval_rows_kernel, dim3((n + EVAL_BLOCK - 1) / EVAL_BLOCK), dim3(EVAL_BLOCK), 0,
                     (hipStream_t)stream, a);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_eval_reduce(int32_t device, int32_t n, const float* acc, float* out42, void* stream) {
  if (!acc || !out42) return ppo_err(PP3_ERR_ARG, "pp3_eval_reduce: null argument");
  if (n < 1) return ppo_err(PP3_ERR_ARG, "pp3_eval_reduce: n must be >= 1");
  if (eval_overlap(acc, (size_t)n * EVAL_WORDS, out42, 2 * EVAL_NOUT))
    return ppo_err(PP3_ERR_ARG, "pp3_eval_reduce: the output aliases the accumulator");
  PPOHIP(hipSetDevice(device));
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(EVAL_RED), 0, (hipStream_t)stream, n, acc, out42);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_eval_column_sums(int32_t device, int32_t n, const float* acc, const float* mean21, float* out22,
                         void* stream) {
  if (!acc || !out22) return ppo_err(PP3_ERR_ARG, "pp3_eval_column_sums: null argument");
  if (n < 1) return ppo_err(PP3_ERR_ARG, "pp3_eval_column_sums: n must be >= 1");
  if (eval_overlap(acc, (size_t)n * EVAL_WORDS, out22, EVAL_NOUT + 1) ||
      (mean21 && eval_overlap(mean21, EVAL_NOUT, out22, EVAL_NOUT + 1)))
    return ppo_err(PP3_ERR_ARG, "pp3_eval_column_sums: the output overlaps an input");
  PPOHIP(hipSetDevice(device));
  hipLaunchKernelGGL(eval_column_sums_kernel, dim3(1), dim3(EVAL_RED), 0, (hipStream_t)stream, n, acc, mean21, out22);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_eval_finish(int32_t device, const float* sums22, int32_t which, float* out42, void* stream) {
  if (!sums22 || !out42) return ppo_err(PP3_ERR_ARG, "pp3_eval_finish: null argument");
  if (which != 0 && which != 1) return ppo_err(PP3_ERR_ARG, "pp3_eval_finish: which must be 0 (means) or 1 (stds)");
  if (eval_overlap(sums22, EVAL_NOUT + 1, out42, 2 * EVAL_NOUT))
    return ppo_err(PP3_ERR_ARG, "pp3_eval_finish: the output overlaps the sums");
  PPOHIP(hipSetDevice(device));
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums22, which, out42);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_sum_gathered_f32(int32_t device, const float* gathered, int32_t world, int64_t count, float* out,
                         void* stream) {
  if (!gathered || !out) return ppo_err(PP3_ERR_ARG, "pp3_sum_gathered_f32: null argument");
  if (world < 1 || world > PP3_LEARN_MAX_WORLD)
    return ppo_err(PP3_ERR_ARG, "pp3_sum_gathered_f32: world must be 1 .. PP3_LEARN_MAX_WORLD");
  if (count < 1 || count > (int64_t)1 << 30) return ppo_err(PP3_ERR_ARG, "pp3_sum_gathered_f32: count must be 1 .. 2^30");
  if (eval_overlap(gathered, (size_t)world * (size_t)count, out, (size_t)count))
    return ppo_err(PP3_ERR_ARG, "pp3_sum_gathered_f32: the output overlaps the gathered rows");
  PPOHIP(hipSetDevice(device));
  hipLaunchKernelGGL(sum_gathered_kernel, dim3((unsigned)((count + EVAL_BLOCK - 1) / EVAL_BLOCK)), dim3(EVAL_BLOCK), 0,
                     (hipStream_t)stream, gathered, world, count, out);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_episode_stats_begin(int32_t device, int32_t n, const float* episode, int64_t episode_stride, const float* done,
                            float* carry, void* stream) {
  if (!episode || !done || !carry) return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_begin: null argument");
  if (n < 1) return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_begin: n must be >= 1");
  if (episode_stride < PP3_EP_STRIDE)
    return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_begin: episode_stride shorter than PP3_EP_STRIDE");
  const size_t n0 = (size_t)n;
  if (eval_overlap(carry, EPS_CARRY * n0, episode, n0 * (size_t)episode_stride) ||
      eval_overlap(carry, EPS_CARRY * n0, done, n0))
    return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_begin: carry overlaps an input");
  PPOHIP(hipSetDevice(device));
  hipLaunchKernelGGL(episode_begin_kernel, dim3((n + EVAL_BLOCK - 1) / EVAL_BLOCK), dim3(EVAL_BLOCK), 0,
                     (hipStream_t)stream, n, episode, episode_stride, done, carry);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_episode_stats_rows(int32_t device, int32_t nsteps, int32_t n, int64_t row_stride, const float* reward,
                           const float* done, const float* truncation, int32_t action_repeat, float* carry,
                           float* part, float* out4, void* stream) {
  if (!reward || !done || !carry || !part || !out4)
    return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: null argument");
  if (nsteps < 1 || n < 1) return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: nsteps and n must be >= 1");
  if (row_stride < n) return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: row_stride shorter than n");
  if (action_repeat < 1) return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: action_repeat must be >= 1");
  if ((int64_t)nsteps * n >= (1 << 24))
    return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: nsteps * n < 2^24 is required (the count stays exact in f32)");
  const size_t n0 = (size_t)n, rows = (size_t)(nsteps - 1) * (size_t)row_stride + n0;
  struct Span {
    const float* p;
    size_t words;
  };
  const Span outs[] = {{carry, EPS_CARRY * n0}, {part, EPS_PART * n0}, {out4, EPS_PART}};
  const Span ins[] = {{reward, rows}, {done, rows}, {truncation, truncation ? rows : 0}};
  for (int i = 0; i < 3; i++) {
    for (const Span& in : ins)
      if (in.words && eval_overlap(outs[i].p, outs[i].words, in.p, in.words))
        return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: an output overlaps an input");
    for (int j = i + 1; j < 3; j++)
      if (eval_overlap(outs[i].p, outs[i].words, outs[j].p, outs[j].words))
        return ppo_err(PP3_ERR_ARG, "pp3_episode_stats_rows: carry, part and out4 must not overlap");
  }
  PPOHIP(hipSetDevice(device));
  EpisodeRowsArgs a;
  a.reward = reward;
  a.done = done;
  a.truncation = truncation;
  a.carry = carry;
  a.part = part;
  a.row_stride = row_stride;
  a.nsteps = nsteps;
  a.n = n;
  a.action_repeat = action_repeat;
  hipLaunchKernelGGL(episode_rows_kernel, dim3((n + EVAL_BLOCK - 1) / EVAL_BLOCK), dim3(EVAL_BLOCK), 0,
                     (hipStream_t)stream, a);
  PPOHIP(hipGetLastError());
  hipLaunchKernelGGL(episode_reduce_kernel, dim3(1), dim3(EVAL_RED), 0, (hipStream_t)stream, n, (const float*)part, out4);
  PPOHIP(hipGetLastError());
  return PP3_OK;
}

}  // extern "C"
