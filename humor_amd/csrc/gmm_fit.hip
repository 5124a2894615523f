// Fitting the init-state Gaussian mixture (humor/train/train_state_prior.py:97-123: scikit-learn's GaussianMixture, full covariances) --
// the two data passes of one EM iteration on gfx950.  gmm.hip evaluates such a mixture for a handful of rows; this file fits one to millions.
//
//   E step, gmm_fit_estep_kernel: one block per tile of 64 rows and EVERY component, so x leaves HBM once.  The tile is staged in LDS as it is;
//     wave w takes the components k = w, w + 4, ... and forms y = (x - mu_k) P_k with v_mfma_f32_32x32x2_f32 (exact fp32), both 32-row halves of
//     the tile against one B operand read from L2 (P_k [D, D] row-major: a lane's operand is one float of a 128-byte row segment).  mu_k is
//     subtracted when the A operand is read from LDS -- BEFORE the product: x P - mu P cancels badly for data far from the origin.  An upper
//     triangular P (the factor scikit-learn keeps, chol(cov)^-T) lets column tile c stop at contraction index 32 (c + 1).
//     lp[n][k] = cst_k - |y|^2 / 2 meets in LDS; loglik[n] = logsumexp_k lp[n][k]; resp[n][k] = exp(lp - loglik) goes out as one contiguous
//     block; the tile's sum of loglik is a wave butterfly (fixed order) -> ll_part[block].
//   M step, gmm_fit_mstep_kernel: block (k, s) walks the rows of split s in chunks of 64: d = x - m_k staged in LDS (m_k = the mean that went
//     into the E step: sum r x x^T - nk mu mu^T loses its digits in fp32), sxx += (r d)^T d on the MFMA over the upper 32 x 32 tiles only
//     (wave w: tiles w, w + 4, ...; the matrix is symmetric), sx and nk on the VALU.  Per-block partials [nk | sx | sxx]; gmm_fit_reduce_kernel
//     adds the splits up in ascending order and mirrors the upper triangle: no floating-point atomics, the same bits on every call.
//     Blocks of one split sit next to each other in the grid (k fastest), so its K readers of a row meet in L2.
//
// Every loop's trip count is fixed by the shapes.  No host reads; buffers come from the caller (ha_gmm_fit_workspace).
#include "common.h"

namespace ha {

typedef float gf_f16 __attribute__((ext_vector_type(16)));

constexpr int GF_ROWS = 64;            // rows per tile (two MFMA row blocks)
constexpr int GF_THREADS = 256;        // four waves
constexpr int GF_WAVES = GF_THREADS / 64;
constexpr int GF_MAX_D = 256, GF_MAX_K = 64;
constexpr int GF_TARGET_BLOCKS = 1024; // M step: K * splits aims at this many blocks (four per CU)

struct gf_estep_args {
  int N, D, K, upper;
  const float* x; int64_t xs;
  const float* means; const float* P; const float* cst;
  float* resp; float* loglik; float* ll_part;
};

struct gf_mstep_args {
  int N, D, K, cps;                    // cps: chunks of GF_ROWS rows per split
  const float* x; int64_t xs;
  const float* resp; const float* shift;
  float* part;
};

__host__ __device__ static inline int gf_estep_ldx(int D) { return D | 1; }      // odd row pitch: the 32 rows of an A operand on 32 banks
static inline size_t gf_estep_lds_floats(int D, int K) { return (size_t)GF_ROWS * gf_estep_ldx(D) + GF_WAVES * D + GF_ROWS * K + GF_ROWS; }
static inline size_t gf_mstep_lds_floats(int D) { return (size_t)GF_ROWS * D + GF_ROWS; }
static inline int64_t gf_chunks(int N) { return ((int64_t)N + GF_ROWS - 1) / GF_ROWS; }
// rows are split over blocks in whole chunks: (chunks per split, splits)
static inline void gf_splits(int N, int K, int* cps, int* S) {
  const int64_t nch = gf_chunks(N);
  int64_t want = GF_TARGET_BLOCKS / K;
  if (want < 1) want = 1;
  if (want > nch) want = nch;
  const int64_t c = (nch + want - 1) / want;
  *cps = (int)c;
  *S = (int)((nch + c - 1) / c);
}
__host__ __device__ static inline size_t gf_part_floats(int D) { return 1 + (size_t)D + (size_t)D * D; }

__device__ __forceinline__ gf_f16 gf_zero() {
  gf_f16 v;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
  return v;
}

__global__ __launch_bounds__(GF_THREADS) void gmm_fit_estep_kernel(gf_estep_args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // (dynamic LDS only: the host emulator tier has no static LDS)
  const int D = a.D, K = a.K, ldx = gf_estep_ldx(D);
  float* xs = smem;                        // [GF_ROWS][ldx] the row tile, as read
  float* mus = xs + GF_ROWS * ldx;         // [GF_WAVES][D]  the mean of the component each wave works on
  float* lpS = mus + GF_WAVES * D;         // [GF_ROWS][K]
  float* llS = lpS + GF_ROWS * K;          // [GF_ROWS]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int64_t n0 = (int64_t)blockIdx.x * GF_ROWS;
  const int rows = a.N - n0 < GF_ROWS ? (int)(a.N - n0) : GF_ROWS;
  for (int r = wave; r < GF_ROWS; r += GF_WAVES) {
    const bool on = r < rows;                                        // (rows past N: zeros, computed and never stored)
    const float* src = a.x + (size_t)(n0 + (on ? r : 0)) * a.xs;
    for (int c = lane; c < D; c += 64) xs[r * ldx + c] = on ? src[c] : 0.f;
  }
  __syncthreads();
  const int nct = (D + 31) / 32;
  float* mu = mus + wave * D;
  for (int k = wave; k < K; k += GF_WAVES) {
    wave_sync();                                                     // the previous component's reads of mu
    for (int c = lane; c < D; c += 64) mu[c] = a.means[(size_t)k * D + c];
    wave_sync();
    const float* Pk = a.P + (size_t)k * D * D;
    gf_f16 q0 = gf_zero(), q1 = gf_zero();
    for (int ct = 0; ct < nct; ++ct) {
      const int col = ct * 32 + l31;
      const bool col_ok = col < D;
      const int kend = a.upper && (ct + 1) * 32 < D ? (ct + 1) * 32 : D;      // P[i][j] = 0 for i > j: nothing below the tile's last row
      gf_f16 acc0 = gf_zero(), acc1 = gf_zero();
      for (int k0 = 0; k0 < kend; k0 += 16) {
        // eight k-steps: every operand is loaded (guarded, never past an array) before the first product
        float b[8], a0[8], a1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int kk = k0 + 2 * u + half;
          const bool ok = kk < kend;
          b[u] = (ok && col_ok) ? Pk[(size_t)kk * D + col] : 0.f;
          const float m = ok ? mu[kk] : 0.f;
          a0[u] = ok ? xs[l31 * ldx + kk] - m : 0.f;
          a1[u] = ok ? xs[(32 + l31) * ldx + kk] - m : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b[u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], b[u], acc1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        q0[r] = fmaf(acc0[r], acc0[r], q0[r]);
        q1[r] = fmaf(acc1[r], acc1[r], q1[r]);
      }
    }
    // |y|^2 of a row: over the 32 lanes (columns) of its half
    const float ck = a.cst[k];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v0 = q0[r], v1 = q1[r];
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) {
        v0 += __shfl_xor(v0, off);
        v1 += __shfl_xor(v1, off);
      }
      if (l31 == 0) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        lpS[row * K + k] = ck - 0.5f * v0;
        lpS[(32 + row) * K + k] = ck - 0.5f * v1;
      }
    }
  }
  __syncthreads();
  if (tid < 64) {
    float ll = 0.f;
    if (tid < rows) {
      const float* lp = lpS + tid * K;
      float m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmaxf(m, lp[k]);
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += expf(lp[k] - m);                // (a NaN lp is dropped by fmaxf and comes back here)
      ll = m + logf(s);
      a.loglik[n0 + tid] = ll;
    }
    llS[tid] = ll;
    float v = ll;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (tid == 0) a.ll_part[blockIdx.x] = v;
  }
  __syncthreads();
  if (a.resp) {
    float* out = a.resp + (size_t)n0 * K;                              // the tile's rows are one contiguous block of resp
    for (int e = tid; e < rows * K; e += GF_THREADS) out[e] = expf(lpS[e] - llS[e / K]);
  }
}

template <int MT>
__global__ __launch_bounds__(GF_THREADS) void gmm_fit_mstep_kernel(gf_mstep_args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, K = a.K;
  float* ds = smem;                        // [GF_ROWS][D] x - m_k
  float* rs = ds + GF_ROWS * D;            // [GF_ROWS]    r[n][k]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int k = blockIdx.x, s = blockIdx.y;
  const int nt = (D + 31) / 32, ntri = nt * (nt + 1) / 2;
  // this wave's tiles (ti <= tj) of the upper triangle, numbered row by row
  int ti[MT], tj[MT];
  bool on[MT];
  gf_f16 acc[MT];
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const int t = wave + GF_WAVES * u;
    on[u] = t < ntri;
    int i = 0, rem = on[u] ? t : 0;
    while (rem >= nt - i) { rem -= nt - i; ++i; }
    ti[u] = i;
    tj[u] = i + rem;
    acc[u] = gf_zero();
  }
  float sxa = 0.f, nka = 0.f;
  // this lane's columns of the shift (D <= 256 = 4 x 64), read once
  float sh[GF_MAX_D / 64];
#pragma unroll
  for (int q = 0; q < GF_MAX_D / 64; ++q) sh[q] = lane + 64 * q < D ? a.shift[(size_t)k * D + lane + 64 * q] : 0.f;
  // the lane's operand columns per tile; a column past D reads column 0 and is zeroed (a slot without a tile repeats tile (0, 0): the
  // products keep the loop free of branches and are never stored)
  int ci[MT], cj[MT];
  bool iok[MT], jok[MT];
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const int i = ti[u] * 32 + l31, j = tj[u] * 32 + l31;
    iok[u] = i < D; jok[u] = j < D;
    ci[u] = iok[u] ? i : 0; cj[u] = jok[u] ? j : 0;
  }
  const int64_t nch = ((int64_t)a.N + GF_ROWS - 1) / GF_ROWS;
  const int64_t c0 = (int64_t)s * a.cps, c1 = c0 + a.cps < nch ? c0 + a.cps : nch;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t n0 = c * GF_ROWS;
    const int rows = a.N - n0 < GF_ROWS ? (int)(a.N - n0) : GF_ROWS;
    __syncthreads();                                                   // the previous chunk has been read
    for (int r = wave; r < GF_ROWS; r += GF_WAVES) {
      const bool row_on = r < rows;                                    // (rows past N: d = 0 and r = 0)
      const float* src = a.x + (size_t)(n0 + (row_on ? r : 0)) * a.xs;
#pragma unroll
      for (int q = 0; q < GF_MAX_D / 64; ++q) {
        const int col = lane + 64 * q;
        if (col < D) ds[r * D + col] = row_on ? src[col] - sh[q] : 0.f;
      }
    }
    if (tid < GF_ROWS) rs[tid] = tid < rows ? a.resp[(size_t)(n0 + tid) * K + k] : 0.f;
    __syncthreads();
    if (tid < D) {                                                     // (thread 0 is always among them: it owns nk)
      for (int r = 0; r < GF_ROWS; ++r) {
        const float w = rs[r];
        nka += w;
        sxa = fmaf(w, ds[r * D + tid], sxa);
      }
    }
#pragma unroll 4
    for (int ks = 0; ks < GF_ROWS / 2; ++ks) {
      const int row = 2 * ks + half;
      const float w = rs[row];
      float av[MT], bv[MT];
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        const float di = ds[row * D + ci[u]], dj = ds[row * D + cj[u]];
        av[u] = iok[u] ? w * di : 0.f;
        bv[u] = jok[u] ? dj : 0.f;
      }
#pragma unroll
      for (int u = 0; u < MT; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc[u], 0, 0, 0);
    }
  }
  float* out = a.part + ((size_t)s * K + k) * gf_part_floats(D);
  if (tid == 0) out[0] = nka;
  if (tid < D) out[1 + tid] = sxa;
  float* oxx = out + 1 + D;
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    if (on[u]) {
      const int j = tj[u] * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ti[u] * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i < D && j < D) oxx[(size_t)i * D + j] = acc[u][r];
      }
    }
  }
}

// nk [K], sx [K, D], sxx [K, D, D] = the splits' partials in ascending order; sxx[i][j] and sxx[j][i] both from the upper-triangle entry
__global__ __launch_bounds__(256) void gmm_fit_reduce_kernel(int S, int K, int D, const float* __restrict__ part, float* __restrict__ nk,
                                                             float* __restrict__ sx, float* __restrict__ sxx) {
  const size_t E = gf_part_floats(D);
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (e >= E) return;
  size_t src = e;
  if (e >= (size_t)(1 + D)) {
    const int i = (int)((e - 1 - D) / D), j = (int)((e - 1 - D) % D);
    src = 1 + D + (size_t)(i < j ? i : j) * D + (i < j ? j : i);
  }
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += part[((size_t)s * K + k) * E + src];
  if (e == 0) nk[k] = acc;
  else if (e < (size_t)(1 + D)) sx[(size_t)k * D + (e - 1)] = acc;
  else sxx[(size_t)k * D * D + (e - 1 - D)] = acc;
}

static int gf_check_shapes(const char* who, int N, int D, int K) {
  HA_REQUIRE(N >= 1 && D >= 1 && D <= GF_MAX_D && K >= 1 && K <= GF_MAX_K, "%s: need N >= 1, 1 <= D <= %d, 1 <= K <= %d", who, GF_MAX_D, GF_MAX_K);
  return HA_OK;
}

// more than the default 64 KB of dynamic LDS: raised once per device and kernel (a function attribute, not a stream operation)
template <class Kernel>
static int gf_allow_lds(Kernel kernel, size_t bytes, bool* done) {
#ifndef HA_SIMT_EMU
  if (bytes > 64 * 1024) {
    int dev = 0;
    HA_CHECK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !done[dev]) {
      // (the E step's need at the limits of the ABI, 86.5 KB, covers the M step's 65.8 KB)
      HA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(gf_estep_lds_floats(GF_MAX_D, GF_MAX_K) * sizeof(float))));
      if (dev >= 0 && dev < 64) done[dev] = true;
    }
  }
#else
  (void)kernel; (void)bytes; (void)done;
#endif
  return HA_OK;
}

template <int MT>
static int gf_mstep_launch(const gf_mstep_args& a, int S, hipStream_t st) {
  static bool done[64] = {};
  const size_t lds = gf_mstep_lds_floats(a.D) * sizeof(float);
  if (int rc = gf_allow_lds(gmm_fit_mstep_kernel<MT>, lds, done)) return rc;
  HA_LAUNCH(gmm_fit_mstep_kernel<MT>, dim3(a.K, S), dim3(GF_THREADS), lds, st, a);
  HA_LAUNCH_CHECK();
  return HA_OK;
}

}  // namespace ha

using namespace ha;

extern "C" int ha_gmm_fit_workspace(int N, int D, int K, int64_t* estep_blocks, int64_t* mstep_floats) {
  HA_REQUIRE(estep_blocks && mstep_floats, "ha_gmm_fit_workspace: null argument");
  if (int rc = gf_check_shapes("ha_gmm_fit_workspace", N, D, K)) return rc;
  int cps = 0, S = 0;
  gf_splits(N, K, &cps, &S);
  *estep_blocks = gf_chunks(N);
  *mstep_floats = (int64_t)S * K * (int64_t)gf_part_floats(D);
  return HA_OK;
}

extern "C" int ha_gmm_fit_estep(int N, int D, int K, const float* x, int64_t x_stride, const float* means, const float* P, int upper,
                                const float* cst, float* resp, float* loglik, float* ll_part, void* stream) {
  if (int rc = gf_check_shapes("ha_gmm_fit_estep", N, D, K)) return rc;
  HA_REQUIRE(x && means && P && cst && loglik && ll_part, "ha_gmm_fit_estep: null argument");
  HA_REQUIRE(x_stride >= D, "ha_gmm_fit_estep: the row stride %lld is below the row width %d", (long long)x_stride, D);
  HA_REQUIRE(upper == 0 || upper == 1, "ha_gmm_fit_estep: upper must be 0 (dense factor) or 1 (upper triangular)");
  hipStream_t st = (hipStream_t)stream;
  gf_estep_args a{N, D, K, upper, x, x_stride, means, P, cst, resp, loglik, ll_part};
  static bool done[64] = {};
  const size_t lds = gf_estep_lds_floats(D, K) * sizeof(float);
  if (int rc = gf_allow_lds(gmm_fit_estep_kernel, lds, done)) return rc;
  HA_LAUNCH(gmm_fit_estep_kernel, dim3((unsigned)gf_chunks(N)), dim3(GF_THREADS), lds, st, a);
  HA_LAUNCH_CHECK();
  return HA_OK;
}

extern "C" int ha_gmm_fit_mstep(int N, int D, int K, const float* x, int64_t x_stride, const float* resp, const float* shift, float* nk,
                                float* sx, float* sxx, void* ws, void* stream) {
  if (int rc = gf_check_shapes("ha_gmm_fit_mstep", N, D, K)) return rc;
  HA_REQUIRE(x && resp && shift && nk && sx && sxx && ws, "ha_gmm_fit_mstep: null argument");
  HA_REQUIRE(x_stride >= D, "ha_gmm_fit_mstep: the row stride %lld is below the row width %d", (long long)x_stride, D);
  hipStream_t st = (hipStream_t)stream;
  int cps = 0, S = 0;
  gf_splits(N, K, &cps, &S);
  gf_mstep_args a{N, D, K, cps, x, x_stride, resp, shift, static_cast<float*>(ws)};
  // upper tiles per wave: D <= 64: 1, <= 96: 2, <= 160: 4, <= 256: 9
  const int nt = ceil_div(D, 32), mt = ceil_div(nt * (nt + 1) / 2, GF_WAVES);
  int rc;
  if (mt <= 1) rc = gf_mstep_launch<1>(a, S, st);
  else if (mt <= 2) rc = gf_mstep_launch<2>(a, S, st);
  else if (mt <= 4) rc = gf_mstep_launch<4>(a, S, st);
  else rc = gf_mstep_launch<9>(a, S, st);
  if (rc != HA_OK) return rc;
  HA_LAUNCH(gmm_fit_reduce_kernel, dim3((unsigned)((gf_part_floats(D) + 255) / 256), K), dim3(256), 0, st, S, K, D, a.part, nk, sx, sxx);
  HA_LAUNCH_CHECK();
  return HA_OK;
}
