// Device bodies of the init-state mixture kernels (gmm.hip), as block-level functions: ha_gmm_nll launches them as kernels of their own,
// ha_fit_loss (fitloss.hip) runs them as block roles inside its two launches.
#pragma once
#include "common.h"

namespace ha {

constexpr int GMM_WAVES = 8, GMM_NI = 4;     // D <= 64 * GMM_NI

// argument checks of ha_gmm_nll (gmm.hip), shared with ha_fit_loss; `who` prefixes the message
int gmm_check_args(const ha_gmm_args& a, const char* who);

// dynamic LDS of gmm_comp_block, in floats
inline size_t gmm_comp_lds_floats(int D) { return (size_t)(2 + GMM_WAVES) * D + GMM_WAVES; }

__device__ __forceinline__ float gmm_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// out[i] = sum_j M[j][i] * v[j] over the block: wave w takes the rows j = w, w + GMM_WAVES, ...; partials meet in `part` [GMM_WAVES][D]
__device__ __forceinline__ void gmm_matvec_t(const float* __restrict__ M, const float* v, float* part, int D, int wave, int lane) {
  float acc[GMM_NI];
#pragma unroll
  for (int q = 0; q < GMM_NI; ++q) acc[q] = 0.f;
  // (latency, not bandwidth, bounds this kernel: eight rows = up to 32 loads in flight per trip; out-of-range lanes / rows read a
  // valid address and contribute zero)
  for (int j0 = wave; j0 < D; j0 += 8 * GMM_WAVES) {
    float m[8][GMM_NI], vj[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u * GMM_WAVES;
      const bool on = j < D;
      vj[u] = on ? v[j] : 0.f;
      const float* row = M + (size_t)(on ? j : 0) * D;
#pragma unroll
      for (int q = 0; q < GMM_NI; ++q) {
        const int i = lane + 64 * q;
        m[u][q] = (64 * q < D) ? row[i < D ? i : 0] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < GMM_NI; ++q) acc[q] = fmaf(m[u][q], vj[u], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < GMM_NI; ++q) {
    const int i = lane + 64 * q;
    if (i < D) part[wave * D + i] = acc[q];
  }
}

// One block of GMM_WAVES * 64 threads per (sequence, component) `blk` = b * K + k: lp[b][k] and gpart[b][k][:].
// smem: gmm_comp_lds_floats(D) floats.
__device__ __forceinline__ void gmm_comp_block(const ha_gmm_args& a, int blk, float* smem) {
  const int D = a.D;
  float* diff = smem;                 // [D]
  float* y = diff + D;                // [D]
  float* part = y + D;                // [GMM_WAVES][D]
  float* red = part + GMM_WAVES * D;  // [GMM_WAVES]
  const int b = blk / a.K, k = blk - b * a.K, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // x_b: the segments side by side
  for (int i = tid; i < D; i += GMM_WAVES * 64) {
    int o = i, sidx = 0;
    while (sidx + 1 < a.nseg && o >= a.seg_width[sidx]) { o -= a.seg_width[sidx]; ++sidx; }
    diff[i] = a.seg[sidx][(size_t)b * a.seg_stride[sidx] + o] - a.means[(size_t)k * D + i];
  }
  __syncthreads();
  // y = Linv (x - mu): contraction over the columns of Linv = the rows of its transpose
  gmm_matvec_t(a.LinvT + (size_t)k * D * D, diff, part, D, wave, lane);
  __syncthreads();
  float q = 0.f;
  for (int i = tid; i < D; i += GMM_WAVES * 64) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < GMM_WAVES; ++w) s += part[w * D + i];
    y[i] = s;
    q = fmaf(s, s, q);
  }
  q = gmm_wave_sum(q);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < GMM_WAVES; ++w) s += red[w];
    a.lp[(size_t)b * a.K + k] = a.cst[k] - 0.5f * s;
  }
  // d(-lp)/dx = Linv^T y: contraction over the rows of Linv
  gmm_matvec_t(a.Linv + (size_t)k * D * D, y, part, D, wave, lane);
  __syncthreads();
  for (int i = tid; i < D; i += GMM_WAVES * 64) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < GMM_WAVES; ++w) s += part[w * D + i];
    a.gpart[((size_t)b * a.K + k) * D + i] = s;
  }
}

// One wave, lane k holding v = lp[b][k] (-inf from K on): nll_b = -logsumexp_k v (returned in every lane); lane k < K also gets its mixture
// weight softmax_k(v).
__device__ __forceinline__ float gmm_wave_nll_of(float v, int K, int lane, float& weight) {
  float m = v;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  const float e = lane < K ? expf(v - m) : 0.f;
  const float s = gmm_wave_sum(e);
  weight = e / s;
  return -(m + logf(s));
}
__device__ __forceinline__ float gmm_wave_nll(const ha_gmm_args& a, int b, int lane, float& weight) {
  return gmm_wave_nll_of(lane < a.K ? a.lp[(size_t)b * a.K + lane] : -INFINITY, a.K, lane, weight);
}

// d nll_b / dx_i = sum_k wk[k] gpart[b][k][i], in ascending k
__device__ __forceinline__ float gmm_mix_grad(const ha_gmm_args& a, int b, int i, const float* wk) {
  float g = 0.f;
  const float* gp = a.gpart + (size_t)b * a.K * a.D + i;
  for (int k0 = 0; k0 < a.K; k0 += 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = gp[(size_t)(k0 + u < a.K ? k0 + u : 0) * a.D];
#pragma unroll
    for (int u = 0; u < 8; ++u) g = fmaf(k0 + u < a.K ? wk[k0 + u] : 0.f, t[u], g);
  }
  return g;
}

}  // namespace ha
