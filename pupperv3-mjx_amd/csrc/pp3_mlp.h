// pp3_mlp.h -- the exported-format policy MLP on one 16-environment tile, shared by the
// stand-alone policy kernel (pp3_policy.hip mlp_kernel: pp3_policy_act) and the fused
// policy-in-the-loop rollout (pp3_env.hip env_step_kernel<NC, true, 8>: pp3_rollout_policy).
// One source for both, so the two compute the same instructions and give bit-identical actions.
// With a SampleHead (pp3_policy_sample, pp3_rollout_policy_sample) the last layer feeds the
// tanh-Gaussian sampling head below instead of being the action.
//
// Format: export.py:13-81 convert_params (dense layers, observation normalisation folded into
// the first layer, final layer = the mean half of the Gaussian head, final activation tanh).
// Every layer is a [16 x K] x [K x M] product on the f32-input matrix cores
// (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation), the eight waves splitting the
// layer's 16-column output tiles.  Activations stay in LDS between layers; weights are read
// straight from global memory (the whole MLP is a few hundred KB and stays L2-resident) in
// MFMA-fragment order: the host stores, per 16-column tile and group of 4 k-blocks, the 64 lanes'
// B values as one float4 per lane, so one 16-byte load per lane (1 KB contiguous per wave) feeds
// four MFMAs.  32 k-blocks of a tile are in flight before its MFMAs.  A: lane l holds
// X[row l&15][k0 + (l>>4)], B: W[k0 + (l>>4)][c0 + (l&15)], C/D: col l&15, row 4(l>>4)+r.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "pupper_hip.h"

namespace pp3pol {

constexpr int TILE = 16;                    // environments per tile (one workgroup)
constexpr int NWAVE = 8;                    // waves per tile
constexpr int MAXW = PP3_POLICY_MAX_WIDTH;  // widest layer (padded)
constexpr int CG8 = 8;                      // groups of 4 k-blocks (32 k-blocks = 128 inputs) per chunk

struct Layer {
  const float* w;  // fragment order [Mp/16][ngrp][64 lanes][4], zero padded
  const float* b;  // [Mp]
  int K, Kp, M, Mp, act;
  int ngrp;  // groups of 4 k-blocks (16 inputs)
};
struct Net {
  Layer layer[PP3_POLICY_MAX_LAYERS];
  int n_layers, in_dim, out_dim;
};

// LDS activations of one tile: two buffers of [TILE][MAXW + 4] floats (74 KB)
typedef float TileBuf[2][TILE][MAXW + 4];
typedef float TileRows[TILE][MAXW + 4];  // one of the two
typedef __attribute__((address_space(3))) float LdsTileBuf[2][TILE][MAXW + 4];  // (explicitly LDS)
constexpr size_t TILE_BUF_BYTES = sizeof(TileBuf);

__device__ __forceinline__ float activate(float x, int act) {
  switch (act) {
    case PP3_ACT_RELU: return fmaxf(x, 0.0f);
    case PP3_ACT_ELU: return x > 0.0f ? x : expm1f(x);
    case PP3_ACT_TANH: return tanhf(x);
    case PP3_ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
    default: return x;
  }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The network as the fused rollout sees it: inside its kernel arguments (constant address space,
// so the layer records are scalar loads)
typedef __attribute__((address_space(4))) const Net KNet;

// One chunk (CG groups of 4 k-blocks) of tile t's B fragments, starting at group g0 (groups past
// ngrp read as zero)
template <int CG>
__device__ __forceinline__ void load_chunk(const Layer& L, int t, int g0, int lane, f32x4 (&bq)[CG]) {
  const f32x4* wf = reinterpret_cast<const f32x4*>(L.w) + ((size_t)t * L.ngrp + g0) * 64 + lane;
#pragma unroll
  for (int q = 0; q < CG; q++) bq[q] = (g0 + q < L.ngrp) ? wf[(size_t)q * 64] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// wave-uniform values kept in SGPRs: an out-of-line caller passes them in VGPRs (the function ABI),
// which would make every loop bound and predicate below look divergent (exec-mask branches
// around each load); readfirstlane of a value already in an SGPR is free
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T>
__device__ __forceinline__ T* uni(T* p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (T*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// the same for a chunk that lies wholly inside the layer (no predicates)
template <int CG>
__device__ __forceinline__ void load_chunk_full(const Layer& L, int t, int g0, int lane, f32x4 (&bq)[CG]) {
  const f32x4* wf = reinterpret_cast<const f32x4*>(L.w) + ((size_t)t * L.ngrp + g0) * 64 + lane;
#pragma unroll
  for (int q = 0; q < CG; q++) bq[q] = wf[(size_t)q * 64];
}

template <class NetT>
__device__ __forceinline__ Layer layer_of(NetT& net, int li) {
  Layer L;  // (field by field: a constant-address-space record has no copy constructor)
  L.w = uni(net.layer[li].w); L.b = uni(net.layer[li].b); L.K = uni(net.layer[li].K); L.Kp = uni(net.layer[li].Kp);
  L.M = uni(net.layer[li].M); L.Mp = uni(net.layer[li].Mp); L.act = uni(net.layer[li].act);
  L.ngrp = uni(net.layer[li].ngrp);
  return L;
}

// ---- The stochastic head: Brax PPO's tanh-Gaussian actor on the full 2 x 12 final layer ----
// (export.py convert_training_params keeps both halves, linear).  Per env row, loc_j = y[j] and
// s_j = y[12 + j]:
//   scale_j  = (softplus(s_j) + min_std) * var_scale          ([ext] brax 0.12.1
//              training/distribution.py NormalTanhDistribution, defaults min_std 0.001, var_scale 1:
//              quoted from memory, Brax is not vendored in the reference)
//   z_j      = sqrt(2) * erfinv(u_j), u_j = jax.random.uniform(key, (N, 12), minval =
//              nextafter(-1, 0), maxval = 1)[env][j]: jax.random.normal's recipe on the threefry
//              stream (the uniform is bit-exact with rng.uniform; the device library's erfinvf is
//              not bit-pinned to XLA's erf_inv, so z agrees with jax to f32 rounding, not bitwise)
//   raw_j    = loc_j + scale_j * z_j,   action_j = tanh(raw_j)
//   log_prob = sum_j [ -zr_j^2 / 2 - log(scale_j) - log(2 pi) / 2 - 2 (log 2 - raw_j - softplus(-2 raw_j)) ]
//              with zr_j = (raw_j - loc_j) / scale_j from the f32 raw_j as stored (what the learner's
//              log_prob(logits, raw_action) recomputes), summed over j ascending.
// No FMA contraction, so the stand-alone kernel and the fused rollout round alike.
constexpr int HEAD_NU = PP3_NU;         // actions per env
constexpr int HEAD_COLS = 2 * HEAD_NU;  // the head's final-layer width (two 16-column tiles)
struct NoHead {};                       // mlp_tile's default: the deterministic (deployment) policy
struct SampleHead {
  float* raw;     // [n][12] pre-tanh samples, or null
  float* logp;    // [n], or null
  float* logits;  // [n][24] the final layer as computed (debug / tests), or null
  uint32_t k0, k1;  // this step's key
  int count, part;  // elements of the key's draw (N * 12), jax_threefry_partitionable
  float min_std, var_scale;
};

// jax's threefry2x32 and the head's three uses of it (split(key)[i], the 32-bit random_bits word i
// of `count`, uniform in [lo, 1)), restated here instead of calling pp3_device.h threefry / split_i /
// bits_i / uniform_i: those are shared with the env kernels, and call sites with these argument
// ranges (count = N * 12, word index up to N * 12, split into 2) joining them changed the code the
// compiler emits for the env step and reset kernels (value ranges it propagates into the shared
// helpers' arguments), which must stay what it was.  tests/test_gpu_policy_sample.py pins these
// to the host rng bit for bit, as tests/test_gpu_env.py pins the others.
struct HeadKey { uint32_t a, b; };
__device__ __forceinline__ void head_threefry(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1, uint32_t& y0,
                                              uint32_t& y1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  x0 += k0;
  x1 += k1;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int r0 = (i & 1) ? 17 : 13, r1 = (i & 1) ? 29 : 15, r2 = (i & 1) ? 16 : 26, r3 = (i & 1) ? 24 : 6;
    x0 += x1; x1 = (x1 << r0) | (x1 >> (32 - r0)); x1 ^= x0;
    x0 += x1; x1 = (x1 << r1) | (x1 >> (32 - r1)); x1 ^= x0;
    x0 += x1; x1 = (x1 << r2) | (x1 >> (32 - r2)); x1 ^= x0;
    x0 += x1; x1 = (x1 << r3) | (x1 >> (32 - r3)); x1 ^= x0;
    x0 += ks[(i + 1) % 3];
    x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
  }
  y0 = x0;
  y1 = x1;
}
// jax.random.split(k)[i], i in {0, 1}
__device__ __forceinline__ HeadKey head_split2(HeadKey k, int i, int part) {
  HeadKey r;
  uint32_t y0, y1;
  if (part) {
    head_threefry(k.a, k.b, 0u, (uint32_t)i, y0, y1);
    r.a = y0;
    r.b = y1;
  } else {  // flat words [y0(0,2), y0(1,3), y1(0,2), y1(1,3)]: key i = words 2i, 2i + 1
    head_threefry(k.a, k.b, 0u, 2u, y0, y1);
    r.a = i ? y1 : y0;
    head_threefry(k.a, k.b, 1u, 3u, y0, y1);
    r.b = i ? y1 : y0;
  }
  return r;
}
// jax.random.uniform(key, (count,), minval = lo, maxval = 1)[i], float32, bit-exact with jax
__device__ __forceinline__ float head_uniform(HeadKey k, int count, int i, float lo, int part) {
#pragma clang fp contract(off)
  uint32_t y0, y1, w;
  if (part) {
    head_threefry(k.a, k.b, 0u, (uint32_t)i, y0, y1);
    w = y0 ^ y1;
  } else {  // the counters 0 .. count-1 (padded to even with a 0) split in halves: x0 = first, x1 = second
    const int h = (count + (count & 1)) / 2;
    const int lane = i % h, half = i / h;
    head_threefry(k.a, k.b, (uint32_t)lane, (lane + h >= count) ? 0u : (uint32_t)(lane + h), y0, y1);
    w = half ? y1 : y0;
  }
  const float f = __uint_as_float((w >> 9) | 0x3F800000u) - 1.0f;
  const float v = f * (1.0f - lo) + lo;
  return v > lo ? v : lo;
}

__device__ __forceinline__ float softplus(float x) {
#pragma clang fp contract(off)
  return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
}

// Y: the final layer's 16 x 32 outputs in LDS (a barrier since they were written).  Threads
// 0 .. 191 sample one (row, j) each and leave the log-prob term in columns 32 .. 43 of the row;
// after a barrier threads 0 .. 15 sum their row.  Ends with a barrier (Y is free again).
template <class RowsT>
__device__ __forceinline__ void sample_head(RowsT& Y, const SampleHead& hd, float* __restrict__ act, int act_stride,
                                            int n, int row0, int tid) {
#pragma clang fp contract(off)
  const int r = tid / HEAD_NU, j = tid - r * HEAD_NU;
  const int row = row0 + r;
  if (tid < TILE * HEAD_NU && row < n) {
    const float loc = Y[r][j], s = Y[r][HEAD_NU + j];
    const float scale = (softplus(s) + hd.min_std) * hd.var_scale;
    const float u = head_uniform(HeadKey{hd.k0, hd.k1}, hd.count, row * HEAD_NU + j, -0x1.fffffep-1f, hd.part);
    const float z = 1.41421356f * erfinvf(u);
    const float raw = loc + scale * z;
    const float zr = (raw - loc) / scale;
    Y[r][2 * TILE + j] =
        -0.5f * zr * zr - logf(scale) - 0.918938533f - 2.0f * (0.693147181f - raw - softplus(-2.0f * raw));
    act[(size_t)row * act_stride + j] = tanhf(raw);
    if (hd.raw) hd.raw[(size_t)row * HEAD_NU + j] = raw;
    if (hd.logits) {
      hd.logits[(size_t)row * HEAD_COLS + j] = loc;
      hd.logits[(size_t)row * HEAD_COLS + HEAD_NU + j] = s;
    }
  }
  __syncthreads();
  if (tid < TILE && row0 + tid < n && hd.logp) {
    float sum = 0.0f;
    for (int q = 0; q < HEAD_NU; q++) sum += Y[tid][2 * TILE + q];
    hd.logp[row0 + tid] = sum;
  }
  __syncthreads();
}

// The MLP of observation rows row0 .. row0+15 (rows >= n read as zero, get no action) ->
// act[row * act_stride + col] for col < out_dim.  Called by all 64 * NWAVE threads of the
// workgroup (tid = threadIdx.x); `buf` is the workgroup's LDS scratch.  Ends with a barrier.
// NetT: Net (a kernel's by-value argument) or KNet.  Weight chunks are loaded where they are
// multiplied (a one-chunk-ahead prefetch measured slower: profiles/AB_LOG.md).  `in` (InT = float[TILE][W] in LDS, W >= in_dim, in_dim a multiple of
// 4): the observation rows are already there (written by the env step, a barrier since), so the
// first layer reads them in place instead of staging `obs` from global memory; rows past n may
// hold anything (a row's outputs depend on that row only, and they are not stored).
// CG: groups of 4 k-blocks per chunk (8 in the stand-alone kernel; the fused rollout's out-of-line
// call uses 4, whose registers fit the callee's caller-saved VGPRs: no save / restore through
// scratch per call).  The MFMA sequence does not depend on it.
// HeadT: NoHead (the last layer's activations are the actions) or SampleHead: the last layer (24
// linear columns) stays in LDS and sample_head draws the actions from it (act = the tanh'ed
// samples); a compile-time choice, the NoHead code is what it was without it.
template <class NetT, class BufT = TileBuf, class InT = TileRows, int CG = CG8, class HeadT = NoHead>
__device__ __forceinline__ void mlp_tile(NetT& net, const float* __restrict__ obs, int obs_stride,
                                         float* __restrict__ act, int act_stride, int n, int row0, BufT& buf,
                                         int tid, InT* in = nullptr, HeadT head = HeadT()) {
  constexpr bool SAMPLE = std::is_same<HeadT, SampleHead>::value;
  // the wave index is wave-uniform: readfirstlane says so, so the tile / chunk / group loops below
  // become scalar branches instead of exec-mask divergence
  const int lane = tid & 63, wave = uni(tid >> 6);
  n = uni(n);
  row0 = uni(row0);
  act = uni(act);
  act_stride = uni(act_stride);
  if (!in) {
    // observation tile -> LDS (rows past n are zero)
    const int kp0 = uni(net.layer[0].Kp), in_dim = uni(net.in_dim);
    obs = uni(obs);
    obs_stride = uni(obs_stride);
    for (int i = tid; i < TILE * kp0; i += 64 * NWAVE) {
      const int r = i / kp0, k = i - r * kp0;
      const int row = row0 + r;
      buf[0][r][k] = (row < n && k < in_dim) ? obs[(size_t)row * obs_stride + k] : 0.0f;
    }
    __syncthreads();
  }
  // one layer's output tiles of this wave: X the [TILE][.] input rows, Y the output rows
  auto layer = [&](auto& X, auto& Y, const Layer& L, bool last) {
    const int ntile = L.Mp / TILE;
    for (int t = wave; t < ntile; t += NWAVE) {
      const int c0 = t * TILE;
      const int col = c0 + (lane & 15);
      const float bias = L.b[col];  // (issued before the weight chunks: its wait never waits for them)
      // two independent accumulators (even / odd k blocks) cover the dependent MFMA latency
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
      const int ar = lane & 15, kk = lane >> 4;
      const int nblk = L.Kp / 4;
      for (int g0 = 0; g0 < L.ngrp; g0 += CG) {
        // a whole chunk (every group and k block inside the layer) runs without per-element
        // predicates; the ragged last chunk keeps them.  The MFMA sequence is the same either way.
        const bool full = g0 + CG <= L.ngrp && 4 * (g0 + CG) <= nblk;
        f32x4 bq[CG];
        float av[CG][4];
        if (full) {
          load_chunk_full(L, t, g0, lane, bq);
        } else {
          load_chunk(L, t, g0, lane, bq);  // every load of the chunk in flight together
        }
        if (full) {
#pragma unroll
          for (int q = 0; q < CG; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) av[q][j] = X[ar][4 * (4 * (g0 + q) + j) + kk];
        } else {
#pragma unroll
          for (int q = 0; q < CG; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const int kb = 4 * (g0 + q) + j;
              av[q][j] = kb < nblk ? X[ar][4 * kb + kk] : 0.0f;
            }
        }
#pragma unroll
        for (int q = 0; q < CG; q++) {
          if (full || g0 + q < L.ngrp) {  // uniform; padded blocks of a ragged group multiply zeros
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][0], bq[q].x, acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][1], bq[q].y, acc1, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][2], bq[q].z, acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][3], bq[q].w, acc1, 0, 0, 0);
          }
        }
      }
      acc += acc1;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 4 * (lane >> 4) + r;
        const float v = activate(acc[r] + bias, L.act);
        if (!last || SAMPLE) {
          Y[row][col] = v;
        } else if (col < L.M && row0 + row < n) {
          act[(size_t)(row0 + row) * act_stride + col] = v;
        }
      }
    }
    __syncthreads();
  };
  int cur = 0;
  const int n_layers = uni(net.n_layers);
  for (int li = 0; li < n_layers; li++) {
    const Layer L = layer_of(net, li);
    const bool last = li == n_layers - 1;
    if (li == 0 && in) layer(*in, buf[1], L, last);
    else layer(buf[cur], buf[cur ^ 1], L, last);
    cur ^= 1;
  }
  if constexpr (SAMPLE) sample_head(buf[cur], head, act, act_stride, n, row0, tid);
}

}  // namespace pp3pol

// the device-side network of a policy handle (pp3_policy.hip; C++ linkage, not part of the C ABI)
const pp3pol::Net* pp3_policy_net(const pp3_policy_t* p);
int pp3_policy_device(const pp3_policy_t* p);
// the handle's weight allocation, writable (pp3_learn.hip reloads it); net->layer[i].w / .b point into it,
// layer 0's w at its start
float* pp3_policy_weights(pp3_policy_t* p);
// the policy's tanh-Gaussian head, if pp3_policy_set_distribution gave it one
bool pp3_policy_distribution(const pp3_policy_t* p, float* min_std, float* var_scale);
