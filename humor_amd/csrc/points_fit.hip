// The points3d data term of a point-cloud fit as one op (value + gradient w.r.t. the predicted vertices): replaces the op chain of
// FittingLoss.points3d_loss (humor/fitting/fitting_loss.py:378-396 -> chamfer both ways, sqrt, robust_std = two torch.median sorts per
// sequence, bisquare weights, sum; fitting_utils.py:192-249) on gfx950.
//
// Forward, four launches:
//   (a) chamfer_nn_kernel (chamfer.hip, through chamfer_nn.h), observation -> vertex ONLY: d2 / idx bit-identical to the chamfer op.
//   (b) pf_scale_kernel, one block per sequence: the reference's robust scale without a sort.  torch.median = the LOWER median, rank
//       (N - 1) / 2 of N = T * n_obs values.  The residuals r = sqrt(d2) are non-negative, so their order is the order of their bit
//       patterns and median(sqrt(d2)) = sqrt(selected d2): a four-pass, 8-bit radix select on the bits (LDS histogram, integer atomics),
//       then a second select over |r - med| for the MAD; sigma = MAD / 0.67449.  A NaN distance makes sigma NaN (torch.median propagates it).
//   (c) pf_weight_kernel: norm = r / (sigma * tune), w = (1 - norm^2)^2, 0 where norm >= 1 -- the reference's operation order (no
//       contraction: -ffp-contract=off); MAD = 0 gives r / 0 = inf -> weight 0 as there.  Per-point terms w * (r * r), summed pairwise per
//       block of 1024 points (4 per thread, LDS tree) into partials;
//   (d) pf_reduce_kernel: the partials of a sequence in a fixed order, loss[b] = 0.5 * sum.
// Backward, one launch: g_pred[b,t,v] = g_loss * sum_{i: idx_i = v} w_i (pred_v - obs_i).  One block per frame with V * 3 fp32 accumulators
// in LDS (82 680 B at V = 6890: the dynamic-LDS attribute is raised).  All waves zero them and, per group of 512 observations, form the
// addends w_i (pred_v - obs_i) and stage them in LDS (their dependent global reads in flight together); ONE wave walks the staged group in index
// order, 64 at a time: every lane finds its rank among the lower lanes with the same target vertex (broadcast reads of the staged indices), then
// round r lets the rank-r lanes do a plain read-modify-write -- the addresses of a round are unique and every vertex receives its addends in index order,
// so the result is the same bits on every call and no floating-point atomic is issued.  All waves stream g_loss * accumulator out: every element of
// g_pred is written, no zero-fill launch.  At d2 = 0 the contribution is w * 0 = 0 (the limit of the smooth objective; the op chain's
// sqrt backward gives inf * 0 = NaN there).
//
// No kernel here can spin: every loop's trip count is fixed by the shapes, except the rounds loop, which is bounded by the wave width
// (64) and leaves early, wave-uniformly, at the largest rank computed BEFORE the loop.  No host reads; workspaces come from the caller.
#include "chamfer_nn.h"

namespace ha {

constexpr int PF_SEL_THREADS = 512;          // pf_scale_kernel: one block per sequence
constexpr int PF_WBLOCK = 1024;              // points per block of pf_weight_kernel (256 threads x 4)
constexpr int PF_MAX_LDS = 150 * 1024;       // accumulators of the backward: V * 12 B must fit
constexpr int PF_BWD_THREADS = 512;          // pf_backward_kernel: one block per frame; observations staged per group of this many

// Block-wide radix select: the bit pattern of the rank-k smallest of key(i), i < n (keys compared as unsigned: non-negative floats).
// hist [256] and st [2] live in LDS; every thread of the block calls it and gets the result.
template <class Key>
__device__ __forceinline__ unsigned block_radix_select(int n, unsigned k, Key key, unsigned* hist, unsigned* st) {
  const int tid = threadIdx.x;
  unsigned prefix = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int e = tid; e < 256; e += PF_SEL_THREADS) hist[e] = 0u;
    __syncthreads();
    // (four keys per trip, loaded before the first is binned: the pass is bound by the latency of its reads, one block per sequence)
    int i = tid;
    for (; i + 3 * PF_SEL_THREADS < n; i += 4 * PF_SEL_THREADS) {
      unsigned u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = key(i + j * PF_SEL_THREADS);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((u[j] & himask) == prefix) atomicAdd(&hist[(u[j] >> shift) & 255u], 1u);
    }
    for (; i < n; i += PF_SEL_THREADS) {
      const unsigned u = key(i);
      if ((u & himask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {
      // wave 0: lane l owns bins 4 l .. 4 l + 3; inclusive scan of the lane sums, then the one lane whose range holds rank k picks the bin.
      // (The keys matching `prefix` number more than k by induction, so exactly one lane qualifies.)
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned s = (c0 + c1) + (c2 + c3);
      unsigned inc = s;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl(inc, (tid - d) & 63);
        if (tid >= d) inc += o;
      }
      const unsigned exc = inc - s;
      if (k >= exc && k < inc) {
        unsigned r = k - exc;
        int bin = 0;
        if (r >= c0) { r -= c0; bin = 1; if (r >= c1) { r -= c1; bin = 2; if (r >= c2) { r -= c2; bin = 3; } } }
        st[0] = prefix | ((unsigned)(4 * tid + bin) << shift);
        st[1] = r;
      }
    }
    __syncthreads();
    prefix = st[0];
    k = st[1];
  }
  return prefix;
}

__global__ __launch_bounds__(PF_SEL_THREADS) void pf_scale_kernel(int n, const float* __restrict__ d2, float* __restrict__ dev,
                                                                  float* __restrict__ med_d2, float* __restrict__ sigma) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // unsigned [256] histogram | [2] select state | [1] NaN count
  unsigned* hist = reinterpret_cast<unsigned*>(smem);
  unsigned* st = hist + 256;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* D = d2 + (size_t)b * n;
  float* E = dev + (size_t)b * n;
  if (tid == 0) st[2] = 0u;
  __syncthreads();
  unsigned nan = 0u;
  for (int i = tid; i < n; i += PF_SEL_THREADS) {
    const float v = D[i];
    nan |= (v != v) ? 1u : 0u;
  }
  if (nan) atomicAdd(&st[2], 1u);
  const unsigned k = (unsigned)((n - 1) / 2);      // the lower median, as torch.median
  const float m2 = __uint_as_float(block_radix_select(n, k, [&](int i) { return __float_as_uint(D[i]); }, hist, st));
  const float med = sqrtf(m2);
  // (thread tid writes and later reads back only its own elements i = tid + j * PF_SEL_THREADS: no fence needed in between)
  for (int i = tid; i < n; i += PF_SEL_THREADS) E[i] = fabsf(sqrtf(D[i]) - med);
  const float mad = __uint_as_float(block_radix_select(n, k, [&](int i) { return __float_as_uint(E[i]); }, hist, st));
  if (tid == 0) {
    const bool any_nan = st[2] != 0u;              // (written before the first barrier of the first select)
    const float qnan = __uint_as_float(0x7fc00000u);
    med_d2[b] = any_nan ? qnan : m2;
    sigma[b] = any_nan ? qnan : mad / 0.67449f;
  }
}

// 256 values (one per thread) summed as a fixed tree through LDS; thread 0 returns the total
__device__ __forceinline__ float block_tree_sum256(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void pf_weight_kernel(int n, const float* __restrict__ d2, int robust, float tune,
                                                        const float* __restrict__ sigma, float* __restrict__ weight,
                                                        float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // [256]
  const int b = blockIdx.y, tid = threadIdx.x;
  const size_t row = (size_t)b * n;
  const float denom = robust ? sigma[b] * tune : 0.f;
  float t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = blockIdx.x * PF_WBLOCK + j * 256 + tid;
    t[j] = 0.f;
    if (i < n) {
      const float r = sqrtf(d2[row + i]);
      float w = 1.f;
      if (robust) {
        const float norm = r / denom;
        w = 1.0f - norm * norm;
        w = w * w;
        if (norm >= 1.0f) w = 0.f;               // (a NaN norm keeps its NaN weight, as torch.where(norm >= 1, 0, w))
      }
      weight[row + i] = w;
      t[j] = w * (r * r);
    }
  }
  const float s = block_tree_sum256((t[0] + t[1]) + (t[2] + t[3]), smem);
  if (tid == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void pf_reduce_kernel(int nblk, const float* __restrict__ partial, float* __restrict__ loss) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // [256]
  const int b = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int p = tid; p < nblk; p += 256) s += partial[(size_t)b * nblk + p];
  s = block_tree_sum256(s, smem);
  if (tid == 0) loss[b] = 0.5f * s;
}

typedef int pf_i4 __attribute__((ext_vector_type(4)));

// LDS of the backward: [V * 3] accumulators (rounded up to 4 floats) | staged group: target vertex [PF_BWD_THREADS] (int) | cx | cy | cz
__host__ __device__ static inline int pf_bwd_stage_off(int V) { return (V * 3 + 3) & ~3; }

__global__ __launch_bounds__(PF_BWD_THREADS) void pf_backward_kernel(int n_obs, int V, const float* __restrict__ obs,
                                                                     const float* __restrict__ pred, const int* __restrict__ idx,
                                                                     const float* __restrict__ weight, const float* __restrict__ g_loss,
                                                                     float* __restrict__ g_pred) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int nacc = V * 3;
  int* sv = reinterpret_cast<int*>(smem + pf_bwd_stage_off(V));
  float* sx = smem + pf_bwd_stage_off(V) + PF_BWD_THREADS;
  float* sy = sx + PF_BWD_THREADS;
  float* sz = sy + PF_BWD_THREADS;
  const float* O = obs + (size_t)f * n_obs * 3;
  const float* P = pred + (size_t)f * V * 3;
  const int* I = idx + (size_t)f * n_obs;
  const float* W = weight + (size_t)f * n_obs;
  for (int e = tid; e < nacc; e += PF_BWD_THREADS) smem[e] = 0.f;
  for (int g0 = 0; g0 < n_obs; g0 += PF_BWD_THREADS) {
    // every wave: the addends of the group's observations (the dependent global reads of all of them in flight at once)
    const int j = g0 + tid;
    int v = -1;                                   // (no observation: never equal to a live lane's vertex)
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (j < n_obs) {
      const int vi = I[j];
      if (vi >= 0 && vi < V) {                    // (indices come from the forward; anything else is ignored, not followed)
        v = vi;
        const float w = W[j];
        cx = w * (P[vi * 3] - O[j * 3]);
        cy = w * (P[vi * 3 + 1] - O[j * 3 + 1]);
        cz = w * (P[vi * 3 + 2] - O[j * 3 + 2]);
      }
    }
    __syncthreads();                              // the accumulators are zeroed / wave 0 has walked the previous group
    sv[tid] = v; sx[tid] = cx; sy[tid] = cy; sz[tid] = cz;
    __syncthreads();
    if (tid < 64) {
      // wave 0: the group in index order, 64 observations per step
      const int cnt = n_obs - g0 < PF_BWD_THREADS ? n_obs - g0 : PF_BWD_THREADS;
      for (int c = 0; c < cnt; c += 64) {
        const int lv = sv[c + tid];
        const float lx = sx[c + tid], ly = sy[c + tid], lz = sz[c + tid];
        int rank = 0;                             // lower lanes of this step with the same target vertex: 16 broadcast reads of four staged
        const pf_i4* q = reinterpret_cast<const pf_i4*>(sv + c);      // indices each, all issued before the first is used
        int lane = tid, pad = 0;
        HA_OPAQUE2(lane, pad);                    // (keeps the 64 `s < lane` masks from being hoisted out of the step loop into spilled SGPRs)
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) {
          const pf_i4 o = q[s4];
#pragma unroll
          for (int u = 0; u < 4; ++u) rank += (4 * s4 + u < lane && o[u] == lv) ? 1 : 0;
        }
        int top = lv >= 0 ? rank : 0;             // the largest rank of a live lane, in every lane
        for (int off = 32; off > 0; off >>= 1) {
          const int o = __shfl_xor(top, off);
          top = o > top ? o : top;
        }
        for (int r = 0; r < 64; ++r) {
          if (r > top) break;                     // wave-uniform; `top` does not change inside the loop
          if (lv >= 0 && rank == r) {
            smem[lv * 3] += lx;
            smem[lv * 3 + 1] += ly;
            smem[lv * 3 + 2] += lz;
          }
          wave_sync();
        }
      }
    }
  }
  __syncthreads();
  const float g = g_loss[0];
  float* G = g_pred + (size_t)f * nacc;
  for (int e = tid; e < nacc; e += PF_BWD_THREADS) G[e] = g * smem[e];
}

static inline int pf_nblk(int n) { return ceil_div(n, PF_WBLOCK); }

static int pf_check_shapes(const char* who, int B, int T, int n_obs, int V) {
  HA_REQUIRE(B >= 0 && T >= 1 && n_obs >= 1 && V >= 1, "%s: need B >= 0, T >= 1, n_obs >= 1, V >= 1", who);
  HA_REQUIRE((int64_t)B * T <= 65535, "%s: at most 65535 frames per call", who);
  HA_REQUIRE((int64_t)T * n_obs < (int64_t)1 << 30 && (int64_t)V * 3 < (int64_t)1 << 30, "%s: sequence too large", who);
  return HA_OK;
}

}  // namespace ha

using namespace ha;

extern "C" int ha_points_fit_workspace(int B, int T, int n_obs, int V, int64_t* bytes) {
  HA_REQUIRE(bytes, "ha_points_fit_workspace: null argument");
  if (int rc = pf_check_shapes("ha_points_fit_workspace", B, T, n_obs, V)) return rc;
  const int n = T * n_obs;
  *bytes = ((int64_t)B * n + (int64_t)B * pf_nblk(n)) * (int64_t)sizeof(float);      // |r - med| per point | block partials of the sum
  return HA_OK;
}

extern "C" int ha_points_fit_forward(int B, int T, int n_obs, const float* obs, int V, const float* pred, int robust, float tune, float* d2,
                                     int32_t* idx, float* weight, float* med_d2, float* sigma, float* loss, void* ws, void* stream) {
  if (int rc = pf_check_shapes("ha_points_fit_forward", B, T, n_obs, V)) return rc;
  HA_REQUIRE(robust == 0 || robust == 1, "ha_points_fit_forward: robust must be 0 (none) or 1 (bisquare)");
  HA_REQUIRE(obs && pred && d2 && idx && weight && loss && ws, "ha_points_fit_forward: null argument");
  HA_REQUIRE(!robust || (med_d2 && sigma), "ha_points_fit_forward: med_d2 and sigma are needed with the bisquare weights");
  if (B == 0) return HA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n = T * n_obs, nblk = pf_nblk(n);
  float* dev = static_cast<float*>(ws);
  float* partial = dev + (size_t)B * n;
  if (int rc = chamfer_nn_launch(B * T, n_obs, obs, V, pred, d2, idx, st)) return rc;
  if (robust) {
    HA_LAUNCH(pf_scale_kernel, dim3(B), dim3(PF_SEL_THREADS), (256 + 4) * sizeof(float), st, n, d2, dev, med_d2, sigma);
    HA_LAUNCH_CHECK();
  }
  HA_LAUNCH(pf_weight_kernel, dim3(nblk, B), dim3(256), 256 * sizeof(float), st, n, d2, robust, tune, sigma, weight, partial);
  HA_LAUNCH_CHECK();
  HA_LAUNCH(pf_reduce_kernel, dim3(B), dim3(256), 256 * sizeof(float), st, nblk, partial, loss);
  HA_LAUNCH_CHECK();
  return HA_OK;
}

extern "C" int ha_points_fit_backward(int B, int T, int n_obs, const float* obs, int V, const float* pred, const int32_t* idx,
                                      const float* weight, const float* g_loss, float* g_pred, void* ws, void* stream) {
  (void)ws;                                       // (the backward needs no scratch; the argument keeps the call shape of the forward)
  if (int rc = pf_check_shapes("ha_points_fit_backward", B, T, n_obs, V)) return rc;
  HA_REQUIRE(obs && pred && idx && weight && g_loss && g_pred, "ha_points_fit_backward: null argument");
  HA_REQUIRE((size_t)V * 3 * sizeof(float) <= (size_t)PF_MAX_LDS, "ha_points_fit_backward: V = %d needs %zu B of LDS accumulators (limit %d B)", V,
             (size_t)V * 3 * sizeof(float), PF_MAX_LDS);
  const size_t lds = ((size_t)pf_bwd_stage_off(V) + 4 * PF_BWD_THREADS) * sizeof(float);
  if (B == 0) return HA_OK;
  hipStream_t st = (hipStream_t)stream;
#ifndef HA_SIMT_EMU
  if (lds > 64 * 1024) {
    // more than the default 64 KB of dynamic LDS: raised once per device (a function attribute, not a stream operation)
    static bool attr_set[64] = {};
    int dev = 0;
    HA_CHECK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      HA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pf_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       PF_MAX_LDS + 16 + 4 * PF_BWD_THREADS * (int)sizeof(float)));
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
#endif
  HA_LAUNCH(pf_backward_kernel, dim3(B * T), dim3(PF_BWD_THREADS), lds, st, n_obs, V, obs, pred, idx, weight, g_loss, g_pred);
  HA_LAUNCH_CHECK();
  return HA_OK;
}
