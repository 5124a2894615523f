// Negative log-likelihood of the stage-3 initial state under the init-state Gaussian mixture, value and gradient
// (humor/fitting/fitting_loss.py:416-429 init_motion_prior_loss: -sum_b MixtureSameFamily(Categorical(w),
// MultivariateNormal(mu, cov)).log_prob(x_b), x_b = joints | joints_vel | trans_vel | root_orient_vel of frame 0, 138 floats).
//
//   lp[b][k] = c_k - 0.5 |Linv_k (x_b - mu_k)|^2,   c_k = log w_k - log det L_k - D/2 log 2 pi,   L_k = chol(cov_k)
//   nll_b    = -logsumexp_k lp[b][k],    d nll_b / dx = sum_k softmax_k(lp[b]) Linv_k^T Linv_k (x_b - mu_k)
//
// Two launches where the op-by-op evaluation (broadcast difference, batched mat-vec, squares, logsumexp and their autograd) takes 34:
//   gmm_comp_kernel   one block per (sequence, component): y = Linv (x - mu) and Linv^T y as two passes over the 76 KB factor,
//                     each wave a slice of the contraction index, every load a coalesced row segment;
//   gmm_mix_kernel    one block per sequence: logsumexp over the components, the mixture-weighted gradient.
#include "gmm_dev.h"

namespace ha {

__global__ __launch_bounds__(GMM_WAVES * 64) void gmm_comp_kernel(ha_gmm_args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  gmm_comp_block(a, blockIdx.x, smem);
}

__global__ __launch_bounds__(256) void gmm_mix_kernel(ha_gmm_args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // (dynamic LDS only: the host emulator tier has no static LDS)
  float* wk = smem;                                                   // [64] mixture weights
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 64) {
    const float nll = gmm_wave_nll(a, b, tid, wk[tid]);
    if (tid == 0) a.nll[b] = nll;
  }
  __syncthreads();
  for (int i = tid; i < a.D; i += 256) a.g_x[(size_t)b * a.D + i] = gmm_mix_grad(a, b, i, wk);
}

int gmm_check_args(const ha_gmm_args& a, const char* who) {
  HA_REQUIRE(a.B >= 1 && a.K >= 1 && a.K <= 64 && a.D >= 1 && a.D <= 64 * GMM_NI, "%s: need B >= 1, 1 <= K <= 64, 1 <= D <= %d", who, 64 * GMM_NI);
  HA_REQUIRE(a.nseg >= 1 && a.nseg <= 4, "%s: 1..4 input segments", who);
  int width = 0;
  for (int s = 0; s < a.nseg; ++s) {
    HA_REQUIRE(a.seg[s] && a.seg_width[s] >= 1 && a.seg_stride[s] >= a.seg_width[s], "%s: segment %d is null or has a stride below its width", who, s);
    width += a.seg_width[s];
  }
  HA_REQUIRE(width == a.D, "%s: the segment widths add up to %d, the mixture has %d dimensions", who, width, a.D);
  HA_REQUIRE(a.means && a.Linv && a.LinvT && a.cst && a.lp && a.gpart && a.nll && a.g_x, "%s: null tensor", who);
  return HA_OK;
}

}  // namespace ha

using namespace ha;

extern "C" int ha_gmm_nll(const ha_gmm_args* args, void* stream) {
  HA_REQUIRE(args, "ha_gmm_nll: null argument");
  const ha_gmm_args& a = *args;
  const int rc = gmm_check_args(a, "ha_gmm_nll");
  if (rc != HA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  HA_LAUNCH(gmm_comp_kernel, dim3(a.B * a.K), dim3(GMM_WAVES * 64), gmm_comp_lds_floats(a.D) * sizeof(float), st, a);
  HA_LAUNCH_CHECK();
  HA_LAUNCH(gmm_mix_kernel, dim3(a.B), dim3(256), 64 * sizeof(float), st, a);
  HA_LAUNCH_CHECK();
  return HA_OK;
}
