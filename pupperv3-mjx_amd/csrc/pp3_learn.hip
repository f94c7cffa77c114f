// pp3_learn.hip -- the PPO learner step on the device: compute_ppo_loss's gradients
// (pp3_ppo_loss_grad), Adam (pp3_adam_step) and the reload of an actor / critic handle from the
// trained blob (pp3_policy_load_params).  include/pupper_hip.h states the contract.
//
// Matrix work: one LDS-tiled GEMM kernel (gemm_kernel) on v_mfma_f32_16x16x4_f32, the exact-f32
// MFMA of pp3_mlp.h, in three operand shapes per layer:
//   forward   Y  = act(X W + b)            A = X [R][K],        B = W [K][M]
//   delta     D' = (D W^T) * act'(Y')      A = D [R][M],        B = W read transposed
//   gradient  G  = [X 1]^T D               A = X read transposed (+ a row of ones: the bias
//                                          gradient is row K of G, which is the blob's layout),
//                                          B = D, summed over rows in chunks of PP3_LEARN_ROW_CHUNK
//                                          into per-chunk partials, then added in chunk order.
// A workgroup of 4 waves owns a 64 x 64 output tile (each wave 2 x 2 MFMA tiles), walks the
// reduction 16 deep per LDS stage, and reads its operands through (row, column) strides with both
// indices checked: rows past R and columns past a layer's width read as zero and are never
// dereferenced.  Nothing is accumulated with atomics: every sum has one fixed order, so a call
// repeats bit for bit.
//
// Around the loss (Brax's training_step beyond compute_ppo_loss): the running normaliser
// (pp3_learner_normalizer_update: two coalesced sweeps over the observation matrix, each thread on one
// column, per-row-range partials, a single-block finish), shuffled minibatches (a validated env index
// the three batch-reading kernels read through; NULL is the contiguous range) and the global-norm
// gradient clip (pp3_grad_clip), all with the same fixed-order sums.
//
// The iteration's random inputs, on request drawn here instead of on the host: the entropy noise
// (pp3_learner_draw_noise: the sampling head's recipe, one thread per element) and the env permutation
// (pp3_learner_shuffle_env_index: jax's _shuffle, per round a host split, a random-bits kernel and a
// one-workgroup bitonic sort of (bits << 32) | i; the permute alone: pp3_permute_by_bits).
//
// The networks' first parameters (pp3_learner_init_params: lecun_uniform kernels from the same
// uniform, zero biases, one thread per blob element, one launch per net over a layer table).
//
// Across ranks (data-parallel PPO over a pp3_comm_t): the gradient blobs and the metrics are packed
// into one send, all-gathered, and added in rank order by one kernel (pp3_learner_allreduce_grads;
// the kernel alone: pp3_learner_reduce_gathered); the normaliser's finish is cut in two around an
// all-gather of one [in_dim] row per sweep (pp3_learner_normalizer_update_ranks).  No ncclAllReduce:
// its order of additions is not fixed.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "pp3_env_host.h"
#include "pp3_mlp.h"
#include "pupper_hip.h"

namespace pp3learn {

using pp3pol::f32x4;

constexpr int BT = 64;       // output tile of a workgroup (rows and columns)
constexpr int KT = 16;       // reduction depth per LDS stage
constexpr int LDT = BT + 16; // LDS row stride: the 4 k rows of an MFMA operand land 16 banks apart
constexpr int NTHREAD = 256;
constexpr int ROW_CHUNK = PP3_LEARN_ROW_CHUNK;
constexpr int RED_BLOCK = 1024;  // the single workgroup of the row reductions
constexpr int NU = PP3_NU;

enum { EPI_FWD = 0, EPI_DELTA = 1, EPI_PARTIAL = 2 };

struct GemmArgs {
  const float* A;  // A(i, k) = A[i * a_si + k * a_sk]
  const float* B;  // B(k, n) = B[k * b_sk + n * b_sn]
  float* C;        // C(i, n) = C[i * c_ld + n] (+ chunk * Mi * c_ld for EPI_PARTIAL)
  const float* bias;   // EPI_FWD: [Nn]
  const float* yprev;  // EPI_DELTA: the post-activation output the delta is taken through, [Mi][Nn]
  int64_t a_si, a_sk, b_sk, b_sn, c_ld;
  int Mi, Nn, Kd;
  int kchunk;    // reduction range of blockIdx.z: [z * kchunk, min(Kd, (z + 1) * kchunk))
  int ones_row;  // >= 0: A(ones_row, k) = 1 for k < Kd (the bias row of the weight gradient)
  int act;
};

__device__ __forceinline__ float act_grad_from_output(float y, int act) {
  switch (act) {
    case PP3_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
    case PP3_ACT_ELU: return y > 0.0f ? 1.0f : y + 1.0f;
    case PP3_ACT_TANH: return 1.0f - y * y;
    case PP3_ACT_SIGMOID: return y * (1.0f - y);
    default: return 1.0f;
  }
}

template <int EPI>
__global__ __launch_bounds__(NTHREAD) void gemm_kernel(GemmArgs g) {
  __shared__ float As[KT][LDT];  // [k][i]
  __shared__ float Bs[KT][LDT];  // [k][n]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * BT, n0 = blockIdx.x * BT;
  const int kbeg = blockIdx.z * g.kchunk;
  const int kend = min(g.Kd, kbeg + g.kchunk);
  const int wi = 32 * (wave >> 1), wj = 32 * (wave & 1);
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // each operand is staged along its contiguous index
  const bool a_kfast = g.a_sk == 1, b_nfast = g.b_sn == 1;
  for (int k0 = kbeg; k0 < kend; k0 += KT) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int ii, kk;
      if (a_kfast) { kk = tid & 15; ii = (tid >> 4) + 16 * j; }
      else         { ii = tid & 63; kk = (tid >> 6) + 4 * j; }
      const int i = i0 + ii, k = k0 + kk;
      float v = 0.0f;
      if (i < g.Mi && k < kend) v = (i == g.ones_row) ? 1.0f : g.A[(size_t)i * g.a_si + (size_t)k * g.a_sk];
      As[kk][ii] = v;
      int nn, kb;
      if (b_nfast) { nn = tid & 63; kb = (tid >> 6) + 4 * j; }
      else         { kb = tid & 15; nn = (tid >> 4) + 16 * j; }
      const int n = n0 + nn, k2 = k0 + kb;
      Bs[kb][nn] = (n < g.Nn && k2 < kend) ? g.B[(size_t)k2 * g.b_sk + (size_t)n * g.b_sn] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < KT / 4; kb++) {
      const int kr = 4 * kb + (lane >> 4), c = lane & 15;
      const float a0 = As[kr][wi + c], a1 = As[kr][wi + 16 + c];
      const float b0 = Bs[kr][wj + c], b1 = Bs[kr][wj + 16 + c];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  float* C = g.C;
  if (EPI == EPI_PARTIAL) C += (size_t)blockIdx.z * (size_t)g.Mi * (size_t)g.c_ld;
#pragma unroll
  for (int ti = 0; ti < 2; ti++)
#pragma unroll
    for (int tj = 0; tj < 2; tj++) {
      const int n = n0 + wj + 16 * tj + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = i0 + wi + 16 * ti + 4 * (lane >> 4) + r;
        if (i < g.Mi && n < g.Nn) {
          float v = acc[ti][tj][r];
          if (EPI == EPI_FWD) v = pp3pol::activate(v + g.bias[n], g.act);
          if (EPI == EPI_DELTA) v *= act_grad_from_output(g.yprev[(size_t)i * g.Nn + n], g.act);
          C[(size_t)i * g.c_ld + n] = v;
        }
      }
    }
}

// a / b to the correctly rounded quotient (but for rare double roundings): the build's fast division is
// within 2.5 ulp, and one residual step removes that.  For the quotients whose error the loss
// amplifies: the normalised observation (every logit inherits it) and the head's standardised action
// (it enters log_prob squared, at |zr| up to ~10).
__device__ __forceinline__ float div_rn(float a, float b) {
  const float q = a / b;
  return fmaf(fmaf(-q, b, a), 1.0f / b, q);
}

// grad[i] = sum over chunks c ascending of part[c][i]
__global__ __launch_bounds__(NTHREAD) void sum_partials_kernel(const float* __restrict__ part, int nchunk, int count,
                                                               float* __restrict__ grad) {
  const int i = blockIdx.x * NTHREAD + threadIdx.x;
  if (i >= count) return;
  float s = 0.0f;
  for (int c = 0; c < nchunk; c++) s += part[(size_t)c * count + i];
  grad[i] = s;
}

// x0[t * B + e][k] = (obs_all[t][env(e)][k] - mean[k]) / std[k], t <= K; env(e) = e0 + e, or
// index[e0 + e] when there is an index
__global__ __launch_bounds__(NTHREAD) void gather_obs_kernel(const float* __restrict__ obs, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, int rows, int B, int N,
                                                             int e0, const int32_t* __restrict__ index, int in_dim,
                                                             float* __restrict__ x0) {
  const size_t idx = (size_t)blockIdx.x * NTHREAD + threadIdx.x;
  if (idx >= (size_t)rows * in_dim) return;
  const int r = (int)(idx / in_dim), k = (int)(idx - (size_t)r * in_dim);
  const int t = r / B, e = r - t * B;
  const int env = index ? index[e0 + e] : e0 + e;
  float v = obs[((size_t)t * N + env) * in_dim + k];
  if (mean) v = div_rn(v - mean[k], stdv[k]);
  x0[idx] = v;
}

// A fixed-order sum by the one workgroup that runs it: thread i adds elements i, i + RED_BLOCK, ..
// ascending, then the RED_BLOCK sums meet in a binary tree in LDS.  All threads get the result.
__device__ __forceinline__ float block_sum(float v, float* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = RED_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

struct RowArgs {
  const float *reward, *done, *trunc, *old_logp, *raw, *eps;  // the batch, row stride N
  const float* values;  // [(K + 1) B] the value net's output
  const float* logits;  // [R][24]
  float *vs, *adv;      // [R]
  float *row_a, *row_b; // [R] per-row loss terms
  float* dvalue;        // [R] d total / d baseline
  float* dlogits;       // [R][24]
  float* stats;         // [4]: v_loss, adv mean, adv std
  float* metrics;       // [4]: total, policy, value, entropy
  int K, B, N, e0;
  const int32_t* index;  // null: row e of the minibatch is env e0 + e; else env index[e0 + e]
  float discount, lambda, reward_scaling, clip_eps, entropy_cost, min_std, var_scale;
  int normalize;
};

// the pp3_gae recurrence on the minibatch's columns (one lane per env), the value loss terms and
// d v_loss / d baseline
__global__ __launch_bounds__(NTHREAD) void value_head_kernel(RowArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * NTHREAD + threadIdx.x;
  if (e >= a.B) return;
  const int R = a.K * a.B;
  float vnext = a.values[(size_t)a.K * a.B + e];
  float vsnext = vnext, acc = 0.0f;
  const int env = a.index ? a.index[a.e0 + e] : a.e0 + e;
  for (int t = a.K - 1; t >= 0; t--) {
    const size_t at = (size_t)t * a.N + env;
    const int r = t * a.B + e;
    const float v = a.values[r];
    const float tm = 1.0f - a.trunc[at];
    const float term = a.done[at] * tm;
    const float g = a.discount * (1.0f - term);
    const float rw = a.reward[at] * a.reward_scaling;
    const float delta = ((rw + g * vnext) - v) * tm;
    acc = delta + (((g * tm) * a.lambda) * acc);
    const float vs = acc + v;
    const float ad = ((rw + g * vsnext) - v) * tm;
    a.vs[r] = vs;
    a.adv[r] = ad;
    const float d = vs - v;
    a.row_a[r] = d * d;
    a.dvalue[r] = (0.5f * (v - vs)) / (float)R;
    vnext = v;
    vsnext = vs;
  }
}

// v_loss and the advantage's mean and population std (two passes), one workgroup
__global__ __launch_bounds__(RED_BLOCK) void value_stats_kernel(RowArgs a) {
  __shared__ float sh[RED_BLOCK];
  const int R = a.K * a.B;
  float s = 0.0f, m = 0.0f;
  for (int r = threadIdx.x; r < R; r += RED_BLOCK) {
    s += a.row_a[r];
    m += a.adv[r];
  }
  const float vsum = block_sum(s, sh);
  const float mean = block_sum(m, sh) / (float)R;
  float q = 0.0f;
  for (int r = threadIdx.x; r < R; r += RED_BLOCK) {
    const float d = a.adv[r] - mean;
    q += d * d;
  }
  const float var = block_sum(q, sh) / (float)R;
  if (threadIdx.x == 0) {
    a.stats[0] = 0.25f * (vsum / (float)R);
    a.stats[1] = mean;
    a.stats[2] = sqrtf(var);
  }
}

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// per row: the clipped surrogate and the entropy term, and d total / d logits
__global__ __launch_bounds__(NTHREAD) void policy_head_kernel(RowArgs a) {
  const int r = blockIdx.x * NTHREAD + threadIdx.x;
  const int R = a.K * a.B;
  if (r >= R) return;
  const int t = r / a.B, e = r - t * a.B;
  const size_t at = (size_t)t * a.N + (a.index ? a.index[a.e0 + e] : a.e0 + e);
  const float* lg = a.logits + (size_t)r * 2 * NU;
  const float* raw = a.raw + at * NU;
  const float* eps = a.eps + at * NU;
  float adv = a.adv[r];
  if (a.normalize) adv = (adv - a.stats[1]) / (a.stats[2] + 1e-8f);
  const float invR = 1.0f / (float)R;
  float loc[NU], scale[NU], zr[NU], sg[NU];
  float logp = 0.0f, ent = 0.0f;
#pragma unroll
  for (int j = 0; j < NU; j++) {
    loc[j] = lg[j];
    const float s = lg[NU + j];
    scale[j] = (softplusf(s) + a.min_std) * a.var_scale;
    sg[j] = sigmoidf(s) * a.var_scale;
    zr[j] = div_rn(raw[j] - loc[j], scale[j]);
    const float ls = logf(scale[j]);
    logp += -0.5f * zr[j] * zr[j] - ls - 0.918938533f - 2.0f * (0.693147181f - raw[j] - softplusf(-2.0f * raw[j]));
    const float act = loc[j] + scale[j] * eps[j];
    ent += 0.5f + 0.918938533f + ls + 2.0f * (0.693147181f - act - softplusf(-2.0f * act));
  }
  const float rho = expf(logp - a.old_logp[at]);
  const float rc = fminf(fmaxf(rho, 1.0f - a.clip_eps), 1.0f + a.clip_eps);
  const float s1 = rho * adv, s2 = rc * adv;
  a.row_a[r] = fminf(s1, s2);
  a.row_b[r] = ent;
  // the minimum is the unclipped branch (or both): its slope in rho is adv; the clipped branch is flat
  const float dlogp = (s1 <= s2) ? -(adv * rho) * invR : 0.0f;
  const float dent = -a.entropy_cost * invR;
  float* dl = a.dlogits + (size_t)r * 2 * NU;
#pragma unroll
  for (int j = 0; j < NU; j++) {
    const float th = tanhf(loc[j] + scale[j] * eps[j]);
    const float dloc = dlogp * (zr[j] / scale[j]) + dent * (-2.0f * th);
    const float dscale = dlogp * ((zr[j] * zr[j] - 1.0f) / scale[j]) + dent * (1.0f / scale[j] - 2.0f * th * eps[j]);
    dl[j] = dloc;
    dl[NU + j] = dscale * sg[j];
  }
}

__global__ __launch_bounds__(RED_BLOCK) void metrics_kernel(RowArgs a) {
  __shared__ float sh[RED_BLOCK];
  const int R = a.K * a.B;
  float p = 0.0f, h = 0.0f;
  for (int r = threadIdx.x; r < R; r += RED_BLOCK) {
    p += a.row_a[r];
    h += a.row_b[r];
  }
  const float ps = block_sum(p, sh), hs = block_sum(h, sh);
  if (threadIdx.x == 0) {
    const float pl = -(ps / (float)R), el = -a.entropy_cost * (hs / (float)R), vl = a.stats[0];
    a.metrics[0] = pl + vl + el;
    a.metrics[1] = pl;
    a.metrics[2] = vl;
    a.metrics[3] = el;
  }
}

__global__ __launch_bounds__(NTHREAD) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t count,
                                                       float lr, float b1, float b2, float eps, float c1, float c2) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * NTHREAD + threadIdx.x;
  if (i >= count) return;
  const float gi = g[i];
  const float mi = b1 * m[i] + (1.0f - b1) * gi;
  const float vi = b2 * v[i] + ((1.0f - b2) * gi) * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] = p[i] - (lr * (mi / c1)) / (sqrtf(vi / c2) + eps);
}

// ---- the running normaliser (running_statistics.update) ----
// Column sums over the row-major obs [rows][in_dim] in two levels.  The rows are cut into
// NORM_RANGES equal ranges of rpr = ceil(rows / NORM_RANGES) rows (the last ones short or empty; empty
// ones are not launched); a workgroup sums one range, the single finishing workgroup the ranges.
// In both, a workgroup of T threads is laid out as G = T / w groups of w = min(in_dim, W) columns:
// thread (g, k) stays on column c0 + k and adds entries g, g + G, .. ascending, so one trip of the
// workgroup reads G consecutive rows (G w consecutive floats when w = in_dim); the G sums of a column
// are then added in LDS in group order; columns past w take further trips (c0 += w).  The order
// depends on (rows, in_dim) alone.
constexpr int NORM_RANGES = 1024;
constexpr int NORM_FIN_COLS = 64;  // W of the finish (the sweep's is its workgroup: NTHREAD)

// PASS 0: part[range][k] = sum_r (obs[r][k] - mean[k])
// PASS 1: part[range][k] = sum_r (obs[r][k] - mean[k]) * (obs[r][k] - mean_new[k])
template <int PASS>
__global__ __launch_bounds__(NTHREAD) void norm_sweep_kernel(const float* __restrict__ obs, int64_t rows, int64_t rpr,
                                                             int in_dim, const float* __restrict__ mean,
                                                             const float* __restrict__ mean_new,
                                                             float* __restrict__ part) {
  __shared__ float sh[NTHREAD];
  const int tid = threadIdx.x;
  const int w = min(in_dim, NTHREAD), G = NTHREAD / w;
  const int g = tid / w, kk = tid - g * w;
  const int64_t r0 = (int64_t)blockIdx.x * rpr;
  const int64_t r1 = min(rows, r0 + rpr);
  for (int c0 = 0; c0 < in_dim; c0 += w) {
    const int k = c0 + kk;
    float s = 0.0f;
    if (g < G && k < in_dim) {
      const float m0 = mean[k];
      const float m1 = PASS ? mean_new[k] : 0.0f;
#pragma unroll 4
      for (int64_t r = r0 + g; r < r1; r += G) {
        const float x = obs[(size_t)r * (size_t)in_dim + k];
        const float d = x - m0;
        s += PASS ? d * (x - m1) : d;
      }
    }
    __syncthreads();
    sh[tid] = s;
    __syncthreads();
    if (g == 0 && k < in_dim) {
      for (int j = 1; j < G; j++) s += sh[j * w + kk];
      part[(size_t)blockIdx.x * in_dim + k] = s;
    }
  }
}

// S[k] = sum over the nr ranges of part[range][k], then
// PASS 0: mean_new[k] = mean[k] + S / count
// PASS 1: sv[k] += S; std[k] = clip(sqrt(max(sv[k], 0) / count), std_min, std_max); mean[k] = mean_new[k]
// The range sum of the finishing workgroup (RED_BLOCK threads): the thread that ends up with column
// k's sum S calls fin(k, S).
template <class Fin>
__device__ __forceinline__ void norm_range_sums(const float* __restrict__ part, int nr, int in_dim, float* sh, Fin fin) {
  const int tid = threadIdx.x;
  const int w = min(in_dim, NORM_FIN_COLS), G = RED_BLOCK / w;
  const int g = tid / w, kk = tid - g * w;
  for (int c0 = 0; c0 < in_dim; c0 += w) {
    const int k = c0 + kk;
    float s = 0.0f;
    if (g < G && k < in_dim) {
      // (unrolled so that the loads of 16 partials are in flight together; the adds keep their order)
#pragma unroll 16
      for (int r = g; r < nr; r += G) s += part[(size_t)r * in_dim + k];
    }
    __syncthreads();
    sh[tid] = s;
    __syncthreads();
    if (g == 0 && k < in_dim) {
      for (int j = 1; j < G; j++) s += sh[j * w + kk];
      fin(k, s);
    }
  }
}

// What follows a column's sum: `t` is S / count (PASS 0) or S (PASS 1) on one GPU, and across ranks
// the rank-ordered sum of the ranks' such terms.
// PASS 0: mean_new[k] = mean[k] + t
// PASS 1: sv[k] += t; std[k] = clip(sqrt(max(sv[k], 0) / count), std_min, std_max); mean[k] = mean_new[k]
template <int PASS>
__device__ __forceinline__ void norm_apply(int k, float t, float count, float std_min, float std_max,
                                           float* __restrict__ mean, float* __restrict__ mean_new,
                                           float* __restrict__ sv, float* __restrict__ stdv) {
  if (PASS == 0) {
    mean_new[k] = mean[k] + t;
  } else {
    const float v = sv[k] + t;
    sv[k] = v;
    // (the build's fast sqrt is within 1 ulp; one residual step, as in div_rn)
    const float q = div_rn(fmaxf(v, 0.0f), count);
    float sd = sqrtf(q);
    if (sd > 0.0f && sd < INFINITY) sd = fmaf(fmaf(-sd, sd, q), 0.5f / sd, sd);
    stdv[k] = fminf(fmaxf(sd, std_min), std_max);
    mean[k] = mean_new[k];
  }
}

template <int PASS>
__global__ __launch_bounds__(RED_BLOCK) void norm_finish_kernel(const float* __restrict__ part, int nr, int in_dim,
                                                                float count, float std_min, float std_max,
                                                                float* __restrict__ mean, float* __restrict__ mean_new,
                                                                float* __restrict__ sv, float* __restrict__ stdv) {
  __shared__ float sh[RED_BLOCK];
  norm_range_sums(part, nr, in_dim, sh, [&](int k, float s) {
    norm_apply<PASS>(k, PASS == 0 ? div_rn(s, count) : s, count, std_min, std_max, mean, mean_new, sv, stdv);
  });
}

// ---- the same update across ranks: norm_finish_kernel cut in two around an all-gather ----
// row[k] = S / count (PASS 0: count is the global count') or S (PASS 1), this rank's term
template <int PASS>
__global__ __launch_bounds__(RED_BLOCK) void norm_reduce_kernel(const float* __restrict__ part, int nr, int in_dim,
                                                                float count, float* __restrict__ row) {
  __shared__ float sh[RED_BLOCK];
  norm_range_sums(part, nr, in_dim, sh, [&](int k, float s) { row[k] = PASS == 0 ? div_rn(s, count) : s; });
}

// t = ((rows[0][k] + rows[1][k]) + ..) over the ranks ascending, then norm_apply
template <int PASS>
__global__ __launch_bounds__(NTHREAD) void norm_apply_ranks_kernel(const float* __restrict__ rows, int world, int in_dim,
                                                                   float count, float std_min, float std_max,
                                                                   float* __restrict__ mean, float* __restrict__ mean_new,
                                                                   float* __restrict__ sv, float* __restrict__ stdv) {
  const int k = blockIdx.x * NTHREAD + threadIdx.x;
  if (k >= in_dim) return;
  float t = rows[k];
  for (int r = 1; r < world; r++) t += rows[(size_t)r * in_dim + k];
  norm_apply<PASS>(k, t, count, std_min, std_max, mean, mean_new, sv, stdv);
}

// ---- gradients and metrics across ranks (pmean): gather, then add in rank order ----
// The gradient blobs and the 4 metrics as one array of n + 4 floats: element i is g0[i] for i < n0,
// g1[i - n0] for i < n, else metrics[i - n].
__global__ __launch_bounds__(NTHREAD) void pack_grads_kernel(const float* __restrict__ g0, int64_t n0,
                                                             const float* __restrict__ g1, int64_t n,
                                                             const float* __restrict__ metrics, float* __restrict__ send) {
  const int64_t i = (int64_t)blockIdx.x * NTHREAD + threadIdx.x;
  if (i >= n + 4) return;
  send[i] = i < n0 ? g0[i] : (i < n ? g1[i - n0] : metrics[i - n]);
}

// element i <- (((gathered[0][i] + gathered[1][i]) + gathered[2][i]) + ..) / world, each addition
// rounded on its own, the quotient correctly rounded; at world 1 the value itself
__global__ __launch_bounds__(NTHREAD) void reduce_ranks_kernel(const float* __restrict__ gathered, int world, int64_t n0,
                                                               int64_t n, float* __restrict__ g0, float* __restrict__ g1,
                                                               float* __restrict__ metrics) {
  const int64_t i = (int64_t)blockIdx.x * NTHREAD + threadIdx.x;
  const int64_t total = n + 4;
  if (i >= total) return;
  float s = gathered[i];
  for (int r = 1; r < world; r++) s += gathered[(size_t)r * (size_t)total + i];
  if (world > 1) s = div_rn(s, (float)world);
  if (i < n0) g0[i] = s;
  else if (i < n) g1[i - n0] = s;
  else metrics[i - n] = s;
}

// ---- the global-norm clip (optax.clip_by_global_norm) ----
// The gradient blobs as one array, policy then value: element i is g0[i] for i < n0, else g1[i - n0].
constexpr int CLIP_CHUNK = 16 * NTHREAD;  // elements per workgroup of both clip kernels

// the NTHREAD values of a workgroup in a binary tree in LDS; all threads get the result
__device__ __forceinline__ float tree_sum(float v, float* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = NTHREAD / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

// part[b] = sum of g^2 over chunk b: thread i adds elements i, i + NTHREAD, .. ascending, then the tree
__global__ __launch_bounds__(NTHREAD) void grad_sumsq_kernel(const float* __restrict__ g0, int64_t n0,
                                                             const float* __restrict__ g1, int64_t n,
                                                             float* __restrict__ part) {
  __shared__ float sh[NTHREAD];
  const int64_t base = (int64_t)blockIdx.x * CLIP_CHUNK + threadIdx.x;
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < CLIP_CHUNK / NTHREAD; j++) {
    const int64_t i = base + (int64_t)j * NTHREAD;
    if (i < n) {
      const float v = i < n0 ? g0[i] : g1[i - n0];
      s += v * v;
    }
  }
  s = tree_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Every workgroup adds the nblk partials in the same order (thread i: partials i, i + NTHREAD, ..,
// then the tree), so all hold the same norm; below max_norm nothing is stored.
__global__ __launch_bounds__(NTHREAD) void grad_clip_kernel(float* __restrict__ g0, int64_t n0, float* __restrict__ g1,
                                                            int64_t n, const float* __restrict__ part, int nblk,
                                                            float max_norm, float* __restrict__ norm_out) {
#pragma clang fp contract(off)
  __shared__ float sh[NTHREAD];
  float s = 0.0f;
  for (int b = threadIdx.x; b < nblk; b += NTHREAD) s += part[b];
  const float norm = sqrtf(tree_sum(s, sh));
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = norm;
  if (norm < max_norm) return;
  const int64_t base = (int64_t)blockIdx.x * CLIP_CHUNK + threadIdx.x;
#pragma unroll
  for (int j = 0; j < CLIP_CHUNK / NTHREAD; j++) {
    const int64_t i = base + (int64_t)j * NTHREAD;
    if (i < n) {
      float* p = i < n0 ? g0 + i : g1 + (i - n0);
      *p = (*p / norm) * max_norm;
    }
  }
}

// One layer of a handle's fragment-order weights from the blob (pp3_policy_create's packing);
// layer 0 folded with the normaliser when there is one.
struct RepackArgs {
  const float* src;  // the layer's kernel [K][M], then bias [M]
  float* w;          // [ntile][ngrp][64][4]
  float* b;          // [Mp]
  const float *mean, *stdv;  // null, or [K]
  int K, M, Mp, ngrp, ntile;
};
__global__ __launch_bounds__(NTHREAD) void repack_kernel(RepackArgs a) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * NTHREAD + threadIdx.x;
  const int nw = a.ntile * a.ngrp * 256;
  if (idx < nw) {
    const int j = idx & 3, ln = (idx >> 2) & 63, tg = idx >> 8;
    const int g = tg % a.ngrp, t = tg / a.ngrp;
    const int k = 4 * (4 * g + j) + (ln >> 4), m = pp3pol::TILE * t + (ln & 15);
    float v = 0.0f;
    if (k < a.K && m < a.M) {
      v = a.src[(size_t)k * a.M + m];
      if (a.stdv) v = div_rn(v, a.stdv[k]);
    }
    a.w[idx] = v;
  } else if (idx < nw + a.Mp) {
    const int m = idx - nw;
    float v = 0.0f;
    if (m < a.M) {
      v = a.src[(size_t)a.K * a.M + m];
      if (a.stdv) {
        float s = 0.0f;
        for (int k = 0; k < a.K; k++) s += div_rn(a.mean[k], a.stdv[k]) * a.src[(size_t)k * a.M + m];
        v = v - s;
      }
    }
    a.b[m] = v;
  }
}

// ---- the iteration's random inputs on the device: entropy noise and the minibatch shuffle ----
// (pp3_mlp.h's head_threefry / head_uniform from this translation unit: no kernel elsewhere changes)
using pp3pol::HeadKey;

// out[i] = jax.random.normal(key, (count,))[i] by the sampling head's recipe
__global__ __launch_bounds__(NTHREAD) void draw_noise_kernel(HeadKey key, int count, int part, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * NTHREAD + threadIdx.x;
  if (i >= count) return;
  const float u = pp3pol::head_uniform(key, count, (int)i, -0x1.fffffep-1f, part);
  out[i] = 1.41421356f * erfinvf(u);
}

// bits[i] = jax's 32-bit random_bits(key, (n,))[i] (head_uniform's word, before it becomes a float);
// iota non-null: also iota[i] = i.  bits null: the iota alone.
__global__ __launch_bounds__(NTHREAD) void shuffle_bits_kernel(HeadKey key, int n, int part, uint32_t* __restrict__ bits,
                                                               int32_t* __restrict__ iota) {
  const int i = blockIdx.x * NTHREAD + threadIdx.x;
  if (i >= n) return;
  if (iota) iota[i] = i;
  if (!bits) return;
  uint32_t y0, y1, w;
  if (part) {
    pp3pol::head_threefry(key.a, key.b, 0u, (uint32_t)i, y0, y1);
    w = y0 ^ y1;
  } else {  // the counters 0 .. n-1 (padded to even with a 0) split in halves: x0 = first, x1 = second
    const int h = (n + (n & 1)) / 2;
    const int lane = i % h, half = i / h;
    pp3pol::head_threefry(key.a, key.b, (uint32_t)lane, (lane + h >= n) ? 0u : (uint32_t)(lane + h), y0, y1);
    w = half ? y1 : y0;
  }
  bits[i] = w;
}

// ---- network initialisation (pp3_learner_init_params): one launch per net over its whole blob ----
// The layer table: blob elements [begin, begin + kcount) are layer l's kernel, element begin + j
// being u_j * scale with u_j = jax.random.uniform(key, (kcount,), f32, -1, 1)[j]; the elements from
// there to the next layer's begin (the blob's end for the last layer) are its bias, zero.
struct InitLayer {
  HeadKey key;
  int begin, kcount;
  float scale;
};
struct InitArgs {
  InitLayer layer[PP3_POLICY_MAX_LAYERS];
  int n_layers, count, part;
  float *p, *g, *m, *v;  // parameters, gradients, Adam moments: [count] each
};

// one thread per blob element: the parameter, and zeros for its gradient and moments
__global__ __launch_bounds__(NTHREAD) void init_params_kernel(InitArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * NTHREAD + threadIdx.x;
  if (i >= a.count) return;
  InitLayer ly = a.layer[0];  // the last layer that begins at or before i (begins ascend)
#pragma unroll
  for (int l = 1; l < PP3_POLICY_MAX_LAYERS; l++)
    if (l < a.n_layers && i >= a.layer[l].begin) ly = a.layer[l];
  const int j = i - ly.begin;
  float w = 0.0f;
  if (j < ly.kcount) w = pp3pol::head_uniform(ly.key, ly.kcount, j, -1.0f, a.part) * ly.scale;
  a.p[i] = w;
  a.g[i] = 0.0f;
  a.m[i] = 0.0f;
  a.v[i] = 0.0f;
}

// x := x[stable_argsort(bits)], one workgroup.  The keys are (bits[i] << 32) | i, all distinct, so
// the order is the stable one whatever the network; slots n .. P-1 (P: n rounded up to a power of
// two) hold all-ones keys, above every real key (i <= 65535), and end up last.  A bitonic network on
// the P slots: in LDS while P <= SORT_LDS_KEYS, else in `scratch` [P] in global memory, where the
// workgroup's barrier orders the passes as it does in LDS.  Then slot i < n takes x[low word]: all
// gathers read x before the barrier, all stores follow it.
constexpr int SORT_LDS_KEYS = 8192;  // 64 KiB of 8-byte keys
constexpr int SORT_MAX_N = 65536;

__device__ __forceinline__ void bitonic_sort_gather(uint64_t* __restrict__ k, const uint32_t* __restrict__ bits, int n, int P,
                                                    int32_t* __restrict__ x) {
  const int tid = threadIdx.x;
  for (int i = tid; i < P; i += RED_BLOCK) k[i] = i < n ? ((uint64_t)bits[i] << 32) | (uint32_t)i : ~0ull;
  __syncthreads();
  for (int len = 2; len <= P; len <<= 1)
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += RED_BLOCK) {
        const int lo = 2 * t - (t & (j - 1)), hi = lo + j;  // the pair (lo, lo + j), lo with bit j clear
        const uint64_t a = k[lo], b = k[hi];
        const bool up = (lo & len) == 0;
        if ((a > b) == up) {
          k[lo] = b;
          k[hi] = a;
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < n; i += RED_BLOCK) k[i] = (uint32_t)x[(uint32_t)k[i]];
  __syncthreads();
  for (int i = tid; i < n; i += RED_BLOCK) x[i] = (int32_t)(uint32_t)k[i];
}

__global__ __launch_bounds__(RED_BLOCK) void permute_lds_kernel(const uint32_t* __restrict__ bits, int n, int P,
                                                                int32_t* __restrict__ x) {
  __shared__ uint64_t keys[SORT_LDS_KEYS];
  bitonic_sort_gather(keys, bits, n, P, x);
}

__global__ __launch_bounds__(RED_BLOCK) void permute_global_kernel(const uint32_t* __restrict__ bits, int n, int P,
                                                                   int32_t* __restrict__ x, uint64_t* __restrict__ scratch) {
  bitonic_sort_gather(scratch, bits, n, P, x);
}

struct NetShape {
  int n_layers, in_dim;
  int K[PP3_POLICY_MAX_LAYERS], M[PP3_POLICY_MAX_LAYERS], act[PP3_POLICY_MAX_LAYERS];
  size_t off[PP3_POLICY_MAX_LAYERS];  // the layer's kernel in the blob; its bias follows at off + K * M
  size_t count, width_sum;
  int max_width;
};

}  // namespace pp3learn

using namespace pp3learn;

struct pp3_learner {
  int device;
  int max_rows;
  NetShape net[2];  // 0: policy, 1: value
  float min_std, var_scale;
  float* blob[2][4];  // params, grads, m, v
  float* x0;          // [max_rows][in_dim]
  float* y;           // the layers' outputs of the net in flight, [rows][width] one after another
  float* d[2];        // deltas, ping-pong, [max_rows][max width]
  float* part;        // weight-gradient partials [chunks][(K + 1) M]
  float *vs, *adv, *row_a, *row_b, *stats;
  float* norm_part;  // the normaliser's partials [NORM_RANGES][in_dim]
  float* norm_mean;  // [in_dim] mean' between the two sweeps
  float* clip_part;  // [clip_blocks] the clip's partial sums of squares
  int clip_blocks;
  // Across ranks (allocated at the first call for a world size): this rank's packed gradients and
  // metrics [count + 4] followed by the gathered [world][count + 4]; likewise the normaliser's row.
  float* rank_grads;
  float* rank_norm;  // [1 + world][in_dim]
  int rank_grads_world, rank_norm_world;
  // The env index: the device copy, and two pinned staging blocks taken in turn, each with the event
  // of the copy that last read it (pp3_learner_set_env_index waits for that one before refilling).
  int32_t* idx_dev;
  int32_t* idx_host[2];
  hipEvent_t idx_ev[2];
  int idx_cap, idx_n, idx_turn;  // allocated entries; entries set (0: none); the next staging block
  // The device draws (allocated at first use, grown on demand): the entropy noise of
  // pp3_learner_draw_noise, and the shuffle's random words [cap] and, past SORT_LDS_KEYS envs, its
  // sort keys [cap rounded up to a power of two].
  float* noise;
  int64_t noise_cap;
  uint32_t* shuf_bits;
  uint64_t* shuf_keys;
  int shuf_cap;
};

static thread_local std::string g_lerr;
static int lerr(int code, const std::string& m) {
  g_lerr = m;
  return code;
}
#define LHIP(x)                                                                                  \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) return lerr(PP3_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

static bool net_shape(int in_dim, int n_layers, const int32_t* outs, const int32_t* acts, NetShape& s) {
  if (!outs || !acts || n_layers < 1 || n_layers > PP3_POLICY_MAX_LAYERS) return false;
  if (in_dim < 1 || in_dim > PP3_POLICY_MAX_WIDTH) return false;
  s = NetShape{};
  s.n_layers = n_layers;
  s.in_dim = in_dim;
  int K = in_dim;
  for (int i = 0; i < n_layers; i++) {
    if (outs[i] < 1 || outs[i] > PP3_POLICY_MAX_WIDTH) return false;
    if (acts[i] < PP3_ACT_LINEAR || acts[i] > PP3_ACT_SIGMOID) return false;
    s.K[i] = K;
    s.M[i] = outs[i];
    s.act[i] = acts[i];
    s.off[i] = s.count;
    s.count += (size_t)(K + 1) * outs[i];
    s.width_sum += outs[i];
    s.max_width = outs[i] > s.max_width ? outs[i] : s.max_width;
    K = outs[i];
  }
  return s.act[n_layers - 1] == PP3_ACT_LINEAR;
}

static void launch_gemm(int epi, const GemmArgs& g, int nchunk, hipStream_t st) {
  const dim3 grid((g.Nn + BT - 1) / BT, (g.Mi + BT - 1) / BT, nchunk), block(NTHREAD);
  if (epi == EPI_FWD) hipLaunchKernelGGL(gemm_kernel<EPI_FWD>, grid, block, 0, st, g);
  else if (epi == EPI_DELTA) hipLaunchKernelGGL(gemm_kernel<EPI_DELTA>, grid, block, 0, st, g);
  else hipLaunchKernelGGL(gemm_kernel<EPI_PARTIAL>, grid, block, 0, st, g);
}

// the outputs of all layers of net `s` on `rows` rows of x0 -> L->y; returns the last layer's
static const float* forward(pp3_learner* L, const NetShape& s, const float* params, int rows, hipStream_t st) {
  const float* x = L->x0;
  float* y = L->y;
  for (int l = 0; l < s.n_layers; l++) {
    GemmArgs g{};
    g.A = x; g.a_si = s.K[l]; g.a_sk = 1;
    g.B = params + s.off[l]; g.b_sk = s.M[l]; g.b_sn = 1;
    g.bias = params + s.off[l] + (size_t)s.K[l] * s.M[l];
    g.C = y; g.c_ld = s.M[l];
    g.Mi = rows; g.Nn = s.M[l]; g.Kd = s.K[l]; g.kchunk = s.K[l]; g.ones_row = -1; g.act = s.act[l];
    launch_gemm(EPI_FWD, g, 1, st);
    x = y;
    y += (size_t)rows * s.M[l];
  }
  return x;
}

// every layer's gradient from the last layer's delta `dlast` [R][M_last]; the layer outputs in
// L->y were laid out for `rows` rows per layer (rows >= R)
static void backward(pp3_learner* L, const NetShape& s, const float* params, float* grads, const float* dlast, int rows,
                     int R, hipStream_t st) {
  std::vector<const float*> yl(s.n_layers);
  const float* y = L->y;
  for (int l = 0; l < s.n_layers; l++) {
    yl[l] = y;
    y += (size_t)rows * s.M[l];
  }
  const int nchunk = (R + ROW_CHUNK - 1) / ROW_CHUNK;
  const float* d = dlast;
  int pp = 0;
  for (int l = s.n_layers - 1; l >= 0; l--) {
    const float* xin = l ? yl[l - 1] : L->x0;
    GemmArgs g{};  // G = [X 1]^T D
    g.A = xin; g.a_si = 1; g.a_sk = s.K[l];
    g.B = d; g.b_sk = s.M[l]; g.b_sn = 1;
    g.C = L->part; g.c_ld = s.M[l];
    g.Mi = s.K[l] + 1; g.Nn = s.M[l]; g.Kd = R; g.kchunk = ROW_CHUNK; g.ones_row = s.K[l];
    launch_gemm(EPI_PARTIAL, g, nchunk, st);
    const int cnt = (s.K[l] + 1) * s.M[l];
    hipLaunchKernelGGL(sum_partials_kernel, dim3((cnt + NTHREAD - 1) / NTHREAD), dim3(NTHREAD), 0, st, L->part, nchunk,
                       cnt, grads + s.off[l]);
    if (l == 0) break;
    GemmArgs b{};  // D' = (D W^T) * act'(Y')
    b.A = d; b.a_si = s.M[l]; b.a_sk = 1;
    b.B = params + s.off[l]; b.b_sk = 1; b.b_sn = s.M[l];
    b.C = L->d[pp]; b.c_ld = s.K[l];
    b.yprev = yl[l - 1];
    b.Mi = R; b.Nn = s.K[l]; b.Kd = s.M[l]; b.kchunk = s.M[l]; b.ones_row = -1; b.act = s.act[l - 1];
    launch_gemm(EPI_DELTA, b, 1, st);
    d = L->d[pp];
    pp ^= 1;
  }
}

// waits for the copies still reading the staging blocks, then frees the index's three allocations
static void free_env_index(pp3_learner* L) {
  for (int i = 0; i < 2; i++) {
    if (L->idx_ev[i]) {
      (void)hipEventSynchronize(L->idx_ev[i]);
      (void)hipEventDestroy(L->idx_ev[i]);
    }
    if (L->idx_host[i]) (void)hipHostFree(L->idx_host[i]);
    L->idx_ev[i] = nullptr;
    L->idx_host[i] = nullptr;
  }
  if (L->idx_dev) (void)hipFree(L->idx_dev);
  L->idx_dev = nullptr;
  L->idx_cap = L->idx_n = 0;
}

// room for num_envs entries in the index's device copy and staging blocks
static int reserve_env_index(pp3_learner* L, int32_t num_envs, const char* fn) {
  if (num_envs <= L->idx_cap) return PP3_OK;
  free_env_index(L);  // (hipFree waits for the queued work that reads the old copy)
  const size_t bytes = (size_t)num_envs * sizeof(int32_t);
  bool ok = hipMalloc(&L->idx_dev, bytes) == hipSuccess;
  for (int i = 0; i < 2; i++)
    ok = ok && hipHostMalloc(&L->idx_host[i], bytes, hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&L->idx_ev[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    free_env_index(L);
    return lerr(PP3_ERR_NOMEM, std::string(fn) + ": allocation failed");
  }
  L->idx_cap = num_envs;
  return PP3_OK;
}

// pp3_ppo_loss_grad (index null) and pp3_ppo_loss_grad_indexed: one path; `fn` names the entry point
static int loss_grad(const char* fn, pp3_learner* L, int32_t nsteps, int32_t batch, int32_t num_envs, int32_t e0,
                     const int32_t* index, const float* obs_all, const float* raw_action, const float* log_prob,
                     const float* reward, const float* done, const float* truncation, const float* eps,
                     const float* mean, const float* std_dev, float discount, float gae_lambda, float reward_scaling,
                     float clip_eps, float entropy_cost, int32_t normalize_advantage, float* metrics_dev, void* stream) {
  const std::string f(fn);
  if (!L || !obs_all || !raw_action || !log_prob || !reward || !done || !truncation || !eps || !metrics_dev)
    return lerr(PP3_ERR_ARG, f + ": null argument");
  if ((mean == nullptr) != (std_dev == nullptr))
    return lerr(PP3_ERR_ARG, f + ": mean and std are given together or not at all");
  if (batch < 1 || nsteps < 1) return lerr(PP3_ERR_ARG, f + ": batch and nsteps must be >= 1");
  if (e0 < 0 || num_envs < 1 || (int64_t)e0 + batch > num_envs)
    return lerr(PP3_ERR_ARG, f + ": the env range [e0, e0 + batch) must lie inside num_envs");
  if (((int64_t)nsteps + 1) * batch > L->max_rows)
    return lerr(PP3_ERR_ARG, f + ": (nsteps + 1) * batch exceeds the learner's max_rows");
  if (!isfinite(discount) || !isfinite(gae_lambda) || !isfinite(reward_scaling) || !isfinite(clip_eps) ||
      !isfinite(entropy_cost))
    return lerr(PP3_ERR_ARG, f + ": the hyper-parameters must be finite");
  if (!(clip_eps > 0.0f)) return lerr(PP3_ERR_ARG, f + ": clip_eps must be > 0");
  LHIP(hipSetDevice(L->device));
  hipStream_t st = (hipStream_t)stream;
  const int K = nsteps, B = batch, R = K * B, RV = (K + 1) * B;
  const NetShape &ps = L->net[0], &vsn = L->net[1];
  const size_t nx = (size_t)RV * ps.in_dim;
  hipLaunchKernelGGL(gather_obs_kernel, dim3((unsigned)((nx + NTHREAD - 1) / NTHREAD)), dim3(NTHREAD), 0, st, obs_all,
                     mean, std_dev, RV, B, num_envs, e0, index, ps.in_dim, L->x0);
  RowArgs a{};
  a.reward = reward; a.done = done; a.trunc = truncation; a.old_logp = log_prob; a.raw = raw_action; a.eps = eps;
  a.vs = L->vs; a.adv = L->adv; a.row_a = L->row_a; a.row_b = L->row_b; a.stats = L->stats; a.metrics = metrics_dev;
  a.K = K; a.B = B; a.N = num_envs; a.e0 = e0; a.index = index;
  a.discount = discount; a.lambda = gae_lambda; a.reward_scaling = reward_scaling; a.clip_eps = clip_eps;
  a.entropy_cost = entropy_cost; a.min_std = L->min_std; a.var_scale = L->var_scale;
  a.normalize = normalize_advantage ? 1 : 0;
  // the critic: baseline and bootstrap rows, targets, its gradient
  a.values = forward(L, vsn, L->blob[1][0], RV, st);
  a.dvalue = L->d[1];  // [R][1]: the value net's last delta
  hipLaunchKernelGGL(value_head_kernel, dim3((B + NTHREAD - 1) / NTHREAD), dim3(NTHREAD), 0, st, a);
  hipLaunchKernelGGL(value_stats_kernel, dim3(1), dim3(RED_BLOCK), 0, st, a);
  // (backward writes its deltas to d[0], d[1], d[0], ..: each product reads one buffer and writes the other)
  backward(L, vsn, L->blob[1][0], L->blob[1][1], a.dvalue, RV, R, st);
  // the actor
  a.logits = forward(L, ps, L->blob[0][0], R, st);
  a.dlogits = L->d[1];
  hipLaunchKernelGGL(policy_head_kernel, dim3((R + NTHREAD - 1) / NTHREAD), dim3(NTHREAD), 0, st, a);
  hipLaunchKernelGGL(metrics_kernel, dim3(1), dim3(RED_BLOCK), 0, st, a);
  backward(L, ps, L->blob[0][0], L->blob[0][1], a.dlogits, R, R, st);
  LHIP(hipGetLastError());
  return PP3_OK;
}

extern "C" {

const char* pp3_learn_last_error(void) { return g_lerr.c_str(); }

int pp3_learner_create(int32_t device, int32_t in_dim, int32_t policy_layers, const int32_t* policy_out_dims,
                       const int32_t* policy_acts, const float* policy_weights, int32_t value_layers,
                       const int32_t* value_out_dims, const int32_t* value_acts, const float* value_weights,
                       float min_std, float var_scale, int64_t max_rows, pp3_learner_t** out) {
  if (!policy_weights || !value_weights || !out) return lerr(PP3_ERR_ARG, "pp3_learner_create: null argument");
  NetShape ps, vs;
  if (!net_shape(in_dim, policy_layers, policy_out_dims, policy_acts, ps) || ps.M[policy_layers - 1] != 2 * NU)
    return lerr(PP3_ERR_ARG, "pp3_learner_create: the policy needs 1..8 layers of width 1..576, a linear last layer of 24");
  if (!net_shape(in_dim, value_layers, value_out_dims, value_acts, vs) || vs.M[value_layers - 1] != 1)
    return lerr(PP3_ERR_ARG, "pp3_learner_create: the value net needs 1..8 layers of width 1..576, a linear last layer of 1");
  if (!(min_std >= 0.0f) || !(min_std < INFINITY) || !(var_scale > 0.0f) || !(var_scale < INFINITY))
    return lerr(PP3_ERR_ARG, "pp3_learner_create: min_std must be >= 0 and var_scale > 0");
  if (max_rows < 2 || max_rows > (1 << 21)) return lerr(PP3_ERR_ARG, "pp3_learner_create: max_rows in 2 .. 2^21");
  if (device < 0) return lerr(PP3_ERR_ARG, "pp3_learner_create: device");
  LHIP(hipSetDevice(device));
  pp3_learner* L = new pp3_learner();
  L->device = device;
  L->max_rows = (int)max_rows;
  L->net[0] = ps;
  L->net[1] = vs;
  L->min_std = min_std;
  L->var_scale = var_scale;
  const size_t rows = (size_t)max_rows;
  const size_t wsum = ps.width_sum > vs.width_sum ? ps.width_sum : vs.width_sum;
  size_t wmax = ps.max_width > vs.max_width ? ps.max_width : vs.max_width;
  if ((size_t)in_dim > wmax) wmax = in_dim;
  const size_t nchunk = (rows + ROW_CHUNK - 1) / ROW_CHUNK;
  size_t pmax = 0;
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < L->net[n].n_layers; l++) {
      const size_t c = (size_t)(L->net[n].K[l] + 1) * L->net[n].M[l];
      pmax = c > pmax ? c : pmax;
    }
  bool ok = true;
  auto alloc = [&](float** p, size_t count) {
    *p = nullptr;
    ok = ok && hipMalloc(p, count * sizeof(float)) == hipSuccess && hipMemset(*p, 0, count * sizeof(float)) == hipSuccess;
  };
  for (int n = 0; n < 2; n++)
    for (int w = 0; w < 4; w++) alloc(&L->blob[n][w], L->net[n].count);
  alloc(&L->x0, rows * in_dim);
  alloc(&L->y, rows * wsum);
  alloc(&L->d[0], rows * wmax);
  alloc(&L->d[1], rows * wmax);
  alloc(&L->part, nchunk * pmax);
  alloc(&L->vs, rows);
  alloc(&L->adv, rows);
  alloc(&L->row_a, rows);
  alloc(&L->row_b, rows);
  alloc(&L->stats, 4);
  alloc(&L->norm_part, (size_t)NORM_RANGES * in_dim);
  alloc(&L->norm_mean, in_dim);
  L->clip_blocks = (int)((ps.count + vs.count + CLIP_CHUNK - 1) / CLIP_CHUNK);
  alloc(&L->clip_part, L->clip_blocks);
  ok = ok && hipMemcpy(L->blob[0][0], policy_weights, ps.count * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(L->blob[1][0], value_weights, vs.count * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    pp3_learner_destroy(L);
    return lerr(PP3_ERR_NOMEM, "pp3_learner_create: device allocation failed");
  }
  *out = L;
  return PP3_OK;
}

int pp3_learner_destroy(pp3_learner_t* L) {
  if (!L) return PP3_OK;
  (void)hipSetDevice(L->device);
  for (int n = 0; n < 2; n++)
    for (int w = 0; w < 4; w++) (void)hipFree(L->blob[n][w]);
  float* ws[] = {L->x0, L->y, L->d[0], L->d[1], L->part, L->vs, L->adv, L->row_a, L->row_b, L->stats,
                 L->norm_part, L->norm_mean, L->clip_part, L->rank_grads, L->rank_norm};
  for (float* p : ws) (void)hipFree(p);
  (void)hipFree(L->noise);
  (void)hipFree(L->shuf_bits);
  (void)hipFree(L->shuf_keys);
  free_env_index(L);
  delete L;
  return PP3_OK;
}

int pp3_learner_buffers(pp3_learner_t* L, int32_t net, int32_t which, float** ptr, int64_t* count) {
  if (!L || !ptr || !count) return lerr(PP3_ERR_ARG, "pp3_learner_buffers: null argument");
  if (net < 0 || net > 1 || which < 0 || which > 3)
    return lerr(PP3_ERR_ARG, "pp3_learner_buffers: net is 0 (policy) or 1 (value), which 0 .. 3 (params, grads, m, v)");
  *ptr = L->blob[net][which];
  *count = (int64_t)L->net[net].count;
  return PP3_OK;
}

int pp3_ppo_loss_grad(pp3_learner_t* L, int32_t nsteps, int32_t batch, int32_t num_envs, int32_t e0,
                      const float* obs_all, const float* raw_action, const float* log_prob, const float* reward,
                      const float* done, const float* truncation, const float* eps, const float* mean,
                      const float* std_dev, float discount, float gae_lambda, float reward_scaling, float clip_eps,
                      float entropy_cost, int32_t normalize_advantage, float* metrics_dev, void* stream) {
  return loss_grad("pp3_ppo_loss_grad", L, nsteps, batch, num_envs, e0, nullptr, obs_all, raw_action, log_prob, reward,
                   done, truncation, eps, mean, std_dev, discount, gae_lambda, reward_scaling, clip_eps, entropy_cost,
                   normalize_advantage, metrics_dev, stream);
}

int pp3_learner_set_env_index(pp3_learner_t* L, const int32_t* index_host, int32_t num_envs, void* stream) {
  if (!L || !index_host) return lerr(PP3_ERR_ARG, "pp3_learner_set_env_index: null argument");
  if (num_envs < 1) return lerr(PP3_ERR_ARG, "pp3_learner_set_env_index: num_envs must be >= 1");
  for (int32_t i = 0; i < num_envs; i++)
    if (index_host[i] < 0 || index_host[i] >= num_envs)
      return lerr(PP3_ERR_ARG, "pp3_learner_set_env_index: entry " + std::to_string(i) + " is outside [0, num_envs)");
  LHIP(hipSetDevice(L->device));
  if (const int rc = reserve_env_index(L, num_envs, "pp3_learner_set_env_index")) return rc;
  const int s = L->idx_turn;
  LHIP(hipEventSynchronize(L->idx_ev[s]));  // the copy that last read this staging block (none: returns at once)
  const size_t bytes = (size_t)num_envs * sizeof(int32_t);
  memcpy(L->idx_host[s], index_host, bytes);
  LHIP(hipMemcpyAsync(L->idx_dev, L->idx_host[s], bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  LHIP(hipEventRecord(L->idx_ev[s], (hipStream_t)stream));
  L->idx_turn = s ^ 1;
  L->idx_n = num_envs;
  return PP3_OK;
}

int pp3_ppo_loss_grad_indexed(pp3_learner_t* L, int32_t nsteps, int32_t batch, int32_t num_envs, int32_t e0,
                              const float* obs_all, const float* raw_action, const float* log_prob,
                              const float* reward, const float* done, const float* truncation, const float* eps,
                              const float* mean, const float* std_dev, float discount, float gae_lambda,
                              float reward_scaling, float clip_eps, float entropy_cost, int32_t normalize_advantage,
                              float* metrics_dev, void* stream) {
  if (L && L->idx_n == 0)
    return lerr(PP3_ERR_ARG, "pp3_ppo_loss_grad_indexed: no env index is set (pp3_learner_set_env_index)");
  if (L && L->idx_n != num_envs)
    return lerr(PP3_ERR_ARG, "pp3_ppo_loss_grad_indexed: the env index was set for another num_envs");
  return loss_grad("pp3_ppo_loss_grad_indexed", L, nsteps, batch, num_envs, e0, L ? L->idx_dev : nullptr, obs_all,
                   raw_action, log_prob, reward, done, truncation, eps, mean, std_dev, discount, gae_lambda,
                   reward_scaling, clip_eps, entropy_cost, normalize_advantage, metrics_dev, stream);
}

int pp3_learner_normalizer_update(pp3_learner_t* L, const float* obs, int64_t rows, float count_new, float std_min,
                                  float std_max, float* mean, float* summed_variance, float* std_dev, void* stream) {
  if (!L || !obs || !mean || !summed_variance || !std_dev)
    return lerr(PP3_ERR_ARG, "pp3_learner_normalizer_update: null argument");
  if (rows < 1) return lerr(PP3_ERR_ARG, "pp3_learner_normalizer_update: rows must be >= 1");
  if (!isfinite(count_new) || count_new < (float)rows)
    return lerr(PP3_ERR_ARG, "pp3_learner_normalizer_update: count_new must be finite and >= rows");
  if (!isfinite(std_min) || !isfinite(std_max) || !(std_min > 0.0f) || !(std_min <= std_max))
    return lerr(PP3_ERR_ARG, "pp3_learner_normalizer_update: std_min and std_max must be finite, 0 < std_min <= std_max");
  LHIP(hipSetDevice(L->device));
  hipStream_t st = (hipStream_t)stream;
  const int in_dim = L->net[0].in_dim;
  const int64_t rpr = (rows + NORM_RANGES - 1) / NORM_RANGES;
  const int nr = (int)((rows + rpr - 1) / rpr);  // the non-empty ranges, <= NORM_RANGES
  hipLaunchKernelGGL(norm_sweep_kernel<0>, dim3(nr), dim3(NTHREAD), 0, st, obs, rows, rpr, in_dim, mean, L->norm_mean,
                     L->norm_part);
  hipLaunchKernelGGL(norm_finish_kernel<0>, dim3(1), dim3(RED_BLOCK), 0, st, L->norm_part, nr, in_dim, count_new,
                     std_min, std_max, mean, L->norm_mean, summed_variance, std_dev);
  hipLaunchKernelGGL(norm_sweep_kernel<1>, dim3(nr), dim3(NTHREAD), 0, st, obs, rows, rpr, in_dim, mean, L->norm_mean,
                     L->norm_part);
  hipLaunchKernelGGL(norm_finish_kernel<1>, dim3(1), dim3(RED_BLOCK), 0, st, L->norm_part, nr, in_dim, count_new,
                     std_min, std_max, mean, L->norm_mean, summed_variance, std_dev);
  LHIP(hipGetLastError());
  return PP3_OK;
}

}  // extern "C"

// ---- the device draws ----
// key, sub = jax.random.split(key) on the host (pp3_env_host.h host_split), for the shuffle's
// per-round keys
static void learn_host_split(HeadKey& key, HeadKey& sub, int part) {
  uint32_t w[4];
  host_split(key.a, key.b, part, w);
  key = HeadKey{w[0], w[1]};
  sub = HeadKey{w[2], w[3]};
}

static int sort_slots(int n) {
  int P = 2;
  while (P < n) P <<= 1;
  return P;
}

// x := x[stable_argsort(bits)]; keys: [sort_slots(n)] when n > SORT_LDS_KEYS
static void launch_permute(const uint32_t* bits, int n, int32_t* x, uint64_t* keys, hipStream_t st) {
  const int P = sort_slots(n);
  if (P <= SORT_LDS_KEYS) hipLaunchKernelGGL(permute_lds_kernel, dim3(1), dim3(RED_BLOCK), 0, st, bits, n, P, x);
  else hipLaunchKernelGGL(permute_global_kernel, dim3(1), dim3(RED_BLOCK), 0, st, bits, n, P, x, keys);
}

extern "C" {

int pp3_learner_draw_noise(pp3_learner_t* L, const uint32_t* key, int32_t nsteps, int32_t num_envs, int32_t partitionable,
                           float** eps_dev_out, void* stream) {
  if (!L || !key || !eps_dev_out) return lerr(PP3_ERR_ARG, "pp3_learner_draw_noise: null argument");
  if (nsteps < 1 || num_envs < 1) return lerr(PP3_ERR_ARG, "pp3_learner_draw_noise: nsteps and num_envs must be >= 1");
  const int64_t rows = (int64_t)nsteps * num_envs;
  if (rows > INT32_MAX / NU) return lerr(PP3_ERR_ARG, "pp3_learner_draw_noise: nsteps * num_envs * 12 must be below 2^31");
  const int64_t count = rows * NU;
  LHIP(hipSetDevice(L->device));
  if (count > L->noise_cap) {  // (hipFree waits for the queued work that reads the old buffer)
    (void)hipFree(L->noise);
    L->noise = nullptr;
    L->noise_cap = 0;
    if (hipMalloc(&L->noise, (size_t)count * sizeof(float)) != hipSuccess)
      return lerr(PP3_ERR_NOMEM, "pp3_learner_draw_noise: device allocation failed");
    L->noise_cap = count;
  }
  hipLaunchKernelGGL(draw_noise_kernel, dim3((unsigned)((count + NTHREAD - 1) / NTHREAD)), dim3(NTHREAD), 0,
                     (hipStream_t)stream, HeadKey{key[0], key[1]}, (int)count, partitionable ? 1 : 0, L->noise);
  LHIP(hipGetLastError());
  *eps_dev_out = L->noise;
  return PP3_OK;
}

int pp3_permute_by_bits(int32_t device, const uint32_t* bits_dev, int32_t n, int32_t* x_dev, void* stream) {
  if (!bits_dev || !x_dev) return lerr(PP3_ERR_ARG, "pp3_permute_by_bits: null argument");
  if (device < 0) return lerr(PP3_ERR_ARG, "pp3_permute_by_bits: device");
  if (n < 1 || n > SORT_MAX_N) return lerr(PP3_ERR_ARG, "pp3_permute_by_bits: n must be in 1 .. 65536");
  LHIP(hipSetDevice(device));
  uint64_t* keys = nullptr;
  if (n > SORT_LDS_KEYS && hipMalloc(&keys, (size_t)sort_slots(n) * sizeof(uint64_t)) != hipSuccess)
    return lerr(PP3_ERR_NOMEM, "pp3_permute_by_bits: device allocation failed");
  launch_permute(bits_dev, n, x_dev, keys, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (keys) (void)hipFree(keys);  // (waits for the sort that uses them)
  LHIP(e);
  return PP3_OK;
}

int pp3_learner_shuffle_env_index(pp3_learner_t* L, const uint32_t* key, int32_t num_envs, int32_t partitionable,
                                  void* stream) {
  if (!L || !key) return lerr(PP3_ERR_ARG, "pp3_learner_shuffle_env_index: null argument");
  if (num_envs < 1 || num_envs > SORT_MAX_N)
    return lerr(PP3_ERR_ARG, "pp3_learner_shuffle_env_index: num_envs must be in 1 .. 65536");
  LHIP(hipSetDevice(L->device));
  const int n = num_envs, part = partitionable ? 1 : 0;
  if (const int rc = reserve_env_index(L, n, "pp3_learner_shuffle_env_index")) return rc;
  if (n > L->shuf_cap) {  // (hipFree waits for the queued work that uses the old ones)
    (void)hipFree(L->shuf_bits);
    (void)hipFree(L->shuf_keys);
    L->shuf_bits = nullptr;
    L->shuf_keys = nullptr;
    L->shuf_cap = 0;
    bool ok = hipMalloc(&L->shuf_bits, (size_t)n * sizeof(uint32_t)) == hipSuccess;
    if (n > SORT_LDS_KEYS) ok = ok && hipMalloc(&L->shuf_keys, (size_t)sort_slots(n) * sizeof(uint64_t)) == hipSuccess;
    if (!ok) {
      (void)hipFree(L->shuf_bits);
      (void)hipFree(L->shuf_keys);
      L->shuf_bits = nullptr;
      L->shuf_keys = nullptr;
      return lerr(PP3_ERR_NOMEM, "pp3_learner_shuffle_env_index: device allocation failed");
    }
    L->shuf_cap = n;
  }
  hipStream_t st = (hipStream_t)stream;
  const int rounds = (int)ceil(3.0 * log((double)n) / log(4294967295.0));
  const dim3 grid((n + NTHREAD - 1) / NTHREAD), block(NTHREAD);
  HeadKey k{key[0], key[1]}, sub{0u, 0u};
  if (rounds == 0) hipLaunchKernelGGL(shuffle_bits_kernel, grid, block, 0, st, sub, n, part, (uint32_t*)nullptr, L->idx_dev);
  for (int r = 0; r < rounds; r++) {
    learn_host_split(k, sub, part);
    hipLaunchKernelGGL(shuffle_bits_kernel, grid, block, 0, st, sub, n, part, L->shuf_bits,
                       r == 0 ? L->idx_dev : (int32_t*)nullptr);
    launch_permute(L->shuf_bits, n, L->idx_dev, L->shuf_keys, st);
  }
  LHIP(hipGetLastError());
  L->idx_n = n;
  return PP3_OK;
}

int pp3_learner_init_params(pp3_learner_t* L, const uint32_t* key, int32_t partitionable, void* stream) {
  if (!L || !key) return lerr(PP3_ERR_ARG, "pp3_learner_init_params: null argument");
  LHIP(hipSetDevice(L->device));
  const int part = partitionable ? 1 : 0;
  HeadKey k_net[2] = {HeadKey{key[0], key[1]}, HeadKey{0u, 0u}};
  learn_host_split(k_net[0], k_net[1], part);  // k_policy, k_value = split(key)
  for (int n = 0; n < 2; n++) {
    const NetShape& s = L->net[n];
    InitArgs a{};
    a.n_layers = s.n_layers;
    a.count = (int)s.count;  // (at most 8 layers of 577 x 576)
    a.part = part;
    a.p = L->blob[n][0]; a.g = L->blob[n][1]; a.m = L->blob[n][2]; a.v = L->blob[n][3];
    for (int l = 0; l < s.n_layers; l++) {
      HeadKey k_l{0u, 0u};
      learn_host_split(k_net[n], k_l, part);  // k_net, k_l = split(k_net)
      a.layer[l].key = k_l;
      a.layer[l].begin = (int)s.off[l];
      a.layer[l].kcount = s.K[l] * s.M[l];
      a.layer[l].scale = sqrtf(3.0f * (1.0f / (float)s.K[l]));
    }
    hipLaunchKernelGGL(init_params_kernel, dim3((unsigned)((a.count + NTHREAD - 1) / NTHREAD)), dim3(NTHREAD), 0,
                       (hipStream_t)stream, a);
  }
  LHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_learner_rng_buffers(pp3_learner_t* L, int32_t** index_dev, int32_t* index_n, float** noise_dev,
                            int64_t* noise_count) {
  if (!L || !index_dev || !index_n || !noise_dev || !noise_count)
    return lerr(PP3_ERR_ARG, "pp3_learner_rng_buffers: null argument");
  *index_dev = L->idx_n ? L->idx_dev : nullptr;
  *index_n = L->idx_n;
  *noise_dev = L->noise;
  *noise_count = L->noise_cap;
  return PP3_OK;
}

}  // extern "C"

// [1 + world][count] floats at *buf, allocated at the first call for this world size (hipFree waits
// for the queued work that reads the old one)
static int rank_workspace(const char* fn, float** buf, int* have_world, int world, size_t count) {
  if (*buf && *have_world == world) return PP3_OK;
  (void)hipFree(*buf);
  *buf = nullptr;
  *have_world = 0;
  if (hipMalloc(buf, (size_t)(1 + world) * count * sizeof(float)) != hipSuccess)
    return lerr(PP3_ERR_NOMEM, std::string(fn) + ": device allocation failed");
  *have_world = world;
  return PP3_OK;
}

// the communicator's argument rules, shared by the two entry points that take one; sets *world
static int check_comm(const std::string& f, pp3_learner* L, pp3_comm_t* comm, int* world) {
  if (pp3_comm_device(comm) != L->device)
    return lerr(PP3_ERR_ARG, f + ": the learner and the communicator are on different devices");
  *world = pp3_comm_world(comm);
  if (*world < 1 || *world > PP3_LEARN_MAX_WORLD)
    return lerr(PP3_ERR_ARG, f + ": the communicator's world size must be in 1 .. 64");
  return PP3_OK;
}

static void launch_reduce_ranks(pp3_learner* L, const float* gathered, int world, float* metrics_dev, hipStream_t st) {
  const int64_t n0 = (int64_t)L->net[0].count, n = n0 + (int64_t)L->net[1].count;
  hipLaunchKernelGGL(reduce_ranks_kernel, dim3((unsigned)((n + 4 + NTHREAD - 1) / NTHREAD)), dim3(NTHREAD), 0, st,
                     gathered, world, n0, n, L->blob[0][1], L->blob[1][1], metrics_dev);
}

extern "C" {

int pp3_learner_reduce_gathered(pp3_learner_t* L, const float* gathered_dev, int32_t world, float* metrics_dev,
                                void* stream) {
  if (!L || !gathered_dev || !metrics_dev) return lerr(PP3_ERR_ARG, "pp3_learner_reduce_gathered: null argument");
  if (world < 1 || world > PP3_LEARN_MAX_WORLD)
    return lerr(PP3_ERR_ARG, "pp3_learner_reduce_gathered: world must be in 1 .. 64");
  LHIP(hipSetDevice(L->device));
  launch_reduce_ranks(L, gathered_dev, world, metrics_dev, (hipStream_t)stream);
  LHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_learner_allreduce_grads(pp3_learner_t* L, pp3_comm_t* comm, float* metrics_dev, void* stream) {
  const std::string f = "pp3_learner_allreduce_grads";
  if (!L || !comm || !metrics_dev) return lerr(PP3_ERR_ARG, f + ": null argument");
  int world;
  if (const int rc = check_comm(f, L, comm, &world)) return rc;
  LHIP(hipSetDevice(L->device));
  const int64_t n0 = (int64_t)L->net[0].count, n = n0 + (int64_t)L->net[1].count, total = n + 4;
  if (const int rc = rank_workspace(f.c_str(), &L->rank_grads, &L->rank_grads_world, world, (size_t)total)) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* send = L->rank_grads;
  float* gathered = L->rank_grads + total;
  hipLaunchKernelGGL(pack_grads_kernel, dim3((unsigned)((total + NTHREAD - 1) / NTHREAD)), dim3(NTHREAD), 0, st,
                     L->blob[0][1], n0, L->blob[1][1], n, metrics_dev, send);
  LHIP(hipGetLastError());
  if (const int rc = pp3_comm_allgather_f32(comm, send, gathered, total, stream))
    return lerr(rc, f + ": " + pp3_comm_last_error());
  launch_reduce_ranks(L, gathered, world, metrics_dev, st);
  LHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_learner_normalizer_update_ranks(pp3_learner_t* L, pp3_comm_t* comm, const float* obs, int64_t rows,
                                        float count_new, float std_min, float std_max, float* mean,
                                        float* summed_variance, float* std_dev, void* stream) {
  const std::string f = "pp3_learner_normalizer_update_ranks";
  if (!L || !comm || !obs || !mean || !summed_variance || !std_dev) return lerr(PP3_ERR_ARG, f + ": null argument");
  if (rows < 1) return lerr(PP3_ERR_ARG, f + ": rows must be >= 1");
  if (!isfinite(count_new) || count_new < (float)rows)
    return lerr(PP3_ERR_ARG, f + ": count_new must be finite and >= rows");
  if (!isfinite(std_min) || !isfinite(std_max) || !(std_min > 0.0f) || !(std_min <= std_max))
    return lerr(PP3_ERR_ARG, f + ": std_min and std_max must be finite, 0 < std_min <= std_max");
  int world;
  if (const int rc = check_comm(f, L, comm, &world)) return rc;
  LHIP(hipSetDevice(L->device));
  const int in_dim = L->net[0].in_dim;
  if (const int rc = rank_workspace(f.c_str(), &L->rank_norm, &L->rank_norm_world, world, (size_t)in_dim)) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* row = L->rank_norm;
  float* gathered = L->rank_norm + in_dim;
  const int64_t rpr = (rows + NORM_RANGES - 1) / NORM_RANGES;
  const int nr = (int)((rows + rpr - 1) / rpr);  // the non-empty ranges, <= NORM_RANGES
  const dim3 cols((in_dim + NTHREAD - 1) / NTHREAD);
  hipLaunchKernelGGL(norm_sweep_kernel<0>, dim3(nr), dim3(NTHREAD), 0, st, obs, rows, rpr, in_dim, mean, L->norm_mean,
                     L->norm_part);
  hipLaunchKernelGGL(norm_reduce_kernel<0>, dim3(1), dim3(RED_BLOCK), 0, st, L->norm_part, nr, in_dim, count_new, row);
  LHIP(hipGetLastError());
  if (const int rc = pp3_comm_allgather_f32(comm, row, gathered, in_dim, stream))
    return lerr(rc, f + ": " + pp3_comm_last_error());
  hipLaunchKernelGGL(norm_apply_ranks_kernel<0>, cols, dim3(NTHREAD), 0, st, gathered, world, in_dim, count_new, std_min,
                     std_max, mean, L->norm_mean, summed_variance, std_dev);
  hipLaunchKernelGGL(norm_sweep_kernel<1>, dim3(nr), dim3(NTHREAD), 0, st, obs, rows, rpr, in_dim, mean, L->norm_mean,
                     L->norm_part);
  hipLaunchKernelGGL(norm_reduce_kernel<1>, dim3(1), dim3(RED_BLOCK), 0, st, L->norm_part, nr, in_dim, count_new, row);
  LHIP(hipGetLastError());
  if (const int rc = pp3_comm_allgather_f32(comm, row, gathered, in_dim, stream))
    return lerr(rc, f + ": " + pp3_comm_last_error());
  hipLaunchKernelGGL(norm_apply_ranks_kernel<1>, cols, dim3(NTHREAD), 0, st, gathered, world, in_dim, count_new, std_min,
                     std_max, mean, L->norm_mean, summed_variance, std_dev);
  LHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_grad_clip(pp3_learner_t* L, float max_norm, float* norm_dev, void* stream) {
  if (!L) return lerr(PP3_ERR_ARG, "pp3_grad_clip: null learner");
  if (!isfinite(max_norm) || !(max_norm > 0.0f)) return lerr(PP3_ERR_ARG, "pp3_grad_clip: max_norm must be finite and > 0");
  LHIP(hipSetDevice(L->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t n0 = (int64_t)L->net[0].count, n = n0 + (int64_t)L->net[1].count;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(L->clip_blocks), dim3(NTHREAD), 0, st, L->blob[0][1], n0, L->blob[1][1], n,
                     L->clip_part);
  hipLaunchKernelGGL(grad_clip_kernel, dim3(L->clip_blocks), dim3(NTHREAD), 0, st, L->blob[0][1], n0, L->blob[1][1], n,
                     L->clip_part, L->clip_blocks, max_norm, norm_dev);
  LHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_adam_step(pp3_learner_t* L, float lr, float b1, float b2, float eps, float c1, float c2, void* stream) {
  if (!L) return lerr(PP3_ERR_ARG, "pp3_adam_step: null learner");
  if (!isfinite(lr) || !isfinite(b1) || !isfinite(b2) || !isfinite(eps) || !isfinite(c1) || !isfinite(c2))
    return lerr(PP3_ERR_ARG, "pp3_adam_step: the hyper-parameters must be finite");
  if (!(c1 > 0.0f) || !(c2 > 0.0f)) return lerr(PP3_ERR_ARG, "pp3_adam_step: c1 and c2 must be > 0");
  LHIP(hipSetDevice(L->device));
  for (int n = 0; n < 2; n++) {
    const int64_t cnt = (int64_t)L->net[n].count;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((cnt + NTHREAD - 1) / NTHREAD)), dim3(NTHREAD), 0, (hipStream_t)stream,
                       L->blob[n][0], L->blob[n][1], L->blob[n][2], L->blob[n][3], cnt, lr, b1, b2, eps, c1, c2);
  }
  LHIP(hipGetLastError());
  return PP3_OK;
}

int pp3_policy_load_params(pp3_policy_t* policy, const float* params_dev, int32_t in_dim, int32_t n_layers,
                           const int32_t* out_dims, const float* mean_dev, const float* std_dev, void* stream) {
  if (!policy || !params_dev || !out_dims) return lerr(PP3_ERR_ARG, "pp3_policy_load_params: null argument");
  if ((mean_dev == nullptr) != (std_dev == nullptr))
    return lerr(PP3_ERR_ARG, "pp3_policy_load_params: mean and std are given together or not at all");
  const pp3pol::Net* net = pp3_policy_net(policy);
  float* base = pp3_policy_weights(policy);
  if (pp3_policy_device(policy) < 0 || !base)
    return lerr(PP3_ERR_ARG, "pp3_policy_load_params: a host-side policy handle has no weights on a device");
  if (net->n_layers != n_layers || net->in_dim != in_dim)
    return lerr(PP3_ERR_ARG, "pp3_policy_load_params: the blob's shape differs from the handle's");
  for (int l = 0; l < n_layers; l++)
    if (net->layer[l].M != out_dims[l]) return lerr(PP3_ERR_ARG, "pp3_policy_load_params: the blob's shape differs from the handle's");
  LHIP(hipSetDevice(pp3_policy_device(policy)));
  size_t off = 0;
  for (int l = 0; l < n_layers; l++) {
    const pp3pol::Layer& Ly = net->layer[l];
    RepackArgs r;
    r.src = params_dev + off;
    r.w = base + (Ly.w - net->layer[0].w);
    r.b = base + (Ly.b - net->layer[0].w);
    r.mean = l == 0 ? mean_dev : nullptr;
    r.stdv = l == 0 ? std_dev : nullptr;
    r.K = Ly.K; r.M = Ly.M; r.Mp = Ly.Mp; r.ngrp = Ly.ngrp; r.ntile = Ly.Mp / pp3pol::TILE;
    const int total = r.ntile * r.ngrp * 256 + r.Mp;
    hipLaunchKernelGGL(repack_kernel, dim3((total + NTHREAD - 1) / NTHREAD), dim3(NTHREAD), 0, (hipStream_t)stream, r);
    off += (size_t)(Ly.K + 1) * Ly.M;
  }
  LHIP(hipGetLastError());
  return PP3_OK;
}

}  // extern "C"
