// Device bodies of the short launches at the stage-3 turn-arounds, as block-level functions: the roll-out (rollout.hip, rollout_persist.hip)
// launches them as kernels of their own, ha_fit_pre_forward / _backward (fitpre.hip) and ha_rollout_post_backward (fitpost.hip) run them as
// block roles beside their own blocks -- work that neither reads what the host launch writes nor is read by it, so no block waits for another.
// The kernel boundary between the host launch and the persistent kernel behind it on the same stream is the only ordering they need.
#pragma once
#include "common.h"

namespace ha {

// ha_tune_set("turn_merge"): one bit per part (the HA_TURN_* values of the header); 0 = every ridden kernel keeps its own launch
extern int g_turn_merge;

// What a host launch has done to a region of a roll-out stash, keyed by the region's address: a roll-out entry point that is told
// "already cleared" / "already laid out" / "partials picked up" takes the mark and refuses the call when it is not there.
enum { TURN_MARK_CLEARED = 1, TURN_MARK_LAID = 2, TURN_MARK_DZ_PENDING = 4 };
void turn_mark(const void* p, unsigned bits);
bool turn_take(const void* p, unsigned bits);     // true when every bit was set; the bits are cleared either way
void turn_forget(const void* p);

constexpr int TURN_ZD = 48;              // latent width (ZD of rollout.hip, P_ZD of rollout_persist.hip)
constexpr int TURN_CLR_WORDS = 1024;     // words one clearing block zeroes

// offset of channel c inside one row's view of a quad-interleaved tile: element (c, row) of tile rt of a C-channel slab
// (C % 4 == 0) is slab[rt * C * 32 + row * 4 + qoff(c)]
__device__ __forceinline__ size_t qoff(int c) { return (size_t)(c >> 2) * 128 + (c & 3); }

constexpr int MAXSPLIT = 5;   // K-slices / SPB never exceeds this for the supported layer widths (K <= 1280)

// sums `nsplit` (<= MAXSPLIT) partial slabs of element (channel c, row) of tile rt.  All loads are unconditional (clamped
// slab index, zero weight beyond nsplit) so they issue back-to-back instead of one round trip per slab.
__device__ __forceinline__ float slab_sum(const float* base, int nsplit, int RT, int C, int rt, int c, int row) {
  const size_t stride = (size_t)RT * C * 32;
  const float* p = base + (size_t)rt * C * 32 + (size_t)row * 4 + qoff(c);
  float t[MAXSPLIT];
#pragma unroll
  for (int s = 0; s < MAXSPLIT; ++s) t[s] = p[(size_t)(s < nsplit ? s : 0) * stride];
  float v = t[0];
#pragma unroll
  for (int s = 1; s < MAXSPLIT; ++s) v += s < nsplit ? t[s] : 0.f;
  return v;
}

// The adjoint of the prior's output layout for (sequence row r, step t), by the 64 lanes of one wave: g_mu | g_var * var | zero padding
// -> g_pri_all [S][RT][pri_pad][32], the slab the first GEMM of the prior's adjoint reads.  var = exp(log-variance) from the forward's
// output slabs (step t at pri_out0 + t * step_stride).  Rows >= B of the tile are written as zeros.
__device__ __forceinline__ void prior_adjoint_rows(const float* __restrict__ g_prior_mu, const float* __restrict__ g_prior_var,
                                                   const float* __restrict__ pri_out0, size_t step_stride, int pri_nsplit, int pri_pad,
                                                   float* __restrict__ g_pri_all, int B, int S, int RT, int r, int t, int lane) {
  const int rt = r >> 5, rr = r & 31;
  const float* po = pri_out0 + (size_t)t * step_stride;
  float var = 0.f;
  if (r < B && lane < TURN_ZD) var = expf(slab_sum(po, pri_nsplit, RT, pri_pad, rt, TURN_ZD + lane, rr));
  const size_t o = ((size_t)r * S + t) * TURN_ZD + lane;
  float* GP = g_pri_all + ((size_t)t * RT + rt) * pri_pad * 32 + (size_t)rr * 4;
  if (lane < TURN_ZD) {
    const bool live = r < B;
    GP[qoff(lane)] = (live && g_prior_mu) ? g_prior_mu[o] : 0.f;
    GP[qoff(TURN_ZD + lane)] = (live && g_prior_var) ? g_prior_var[o] * var : 0.f;
  }
  for (int c = 2 * TURN_ZD + lane; c < pri_pad; c += 64) GP[qoff(c)] = 0.f;
}

// g_z[b][t][c] = sum of the DZ_SLOTS partial products of the persistent adjoint ([S][DZ_SLOTS][32][48]), fixed order, + g_z_add; element i
constexpr int TURN_DZ_SLOTS = 31;        // DZ_SLOTS of rollout_persist.hip (asserted there)
__device__ __forceinline__ void dz_reduce_elem(const float* __restrict__ part, float* __restrict__ g_z, const float* __restrict__ g_z_add,
                                               int B, int S, int i) {
  if (i >= B * S * TURN_ZD) return;
  const int c = i % TURN_ZD, t = (i / TURN_ZD) % S, b = i / (TURN_ZD * S);
  float v = 0.f;
  for (int sl = 0; sl < TURN_DZ_SLOTS; ++sl) v += part[(((size_t)t * TURN_DZ_SLOTS + sl) * 32 + b) * TURN_ZD + c];
  g_z[i] = g_z_add ? v + g_z_add[i] : v;
}

// clearing block `blk` of a region of n 4-byte words: TURN_CLR_WORDS words, by all threads of the block
__device__ __forceinline__ void zero_words_block(unsigned* __restrict__ p, size_t n, size_t blk) {
  const size_t lo = blk * TURN_CLR_WORDS, hi = lo + TURN_CLR_WORDS < n ? lo + TURN_CLR_WORDS : n;
  for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) p[i] = 0u;
}
inline unsigned zero_words_blocks(size_t n) { return (unsigned)((n + TURN_CLR_WORDS - 1) / TURN_CLR_WORDS); }

}  // namespace ha
