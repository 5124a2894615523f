// What MotionOptimizer.rollout_latent_motion does with the roll-out's output, in one launch per direction
// (humor/fitting/motion_optimizer.py:950-1019): rotation matrices -> axis-angle for the root and the 21 body joints
// (rotation_matrix_to_angle_axis, transforms.py:243-389), frame 0 (the optimised initial state) prepended, contact logits ->
// sigmoid confidences / 0.5-thresholded labels scattered to the 22 SMPL joints through CONTACT_INDS (amass_utils.py:21-23) with
// frame 0 copied from frame 1, and -- when a floor is optimised -- the inverse cam2prior map of the root trajectory back into the
// camera frame (apply_cam2prior(..., inverse=True), motion_optimizer.py:678-742: R^T rodrigues(root) -> axis-angle,
// R^T (trans - trans_0) - t).  Replaces ~100 element-wise / gather / cat launches per closure (forward + autograd backward).
// One wavefront per frame (b, t); lane j < 22 owns SMPL joint j (lane 0 also the root trajectory and the camera-frame map).
// The adjoint's per-sequence sums (d/dR, d/dt of cam2prior, d/dtrans_0) are written as per-frame partials and added in frame
// order by a second small launch: no atomics.
#include <string.h>

#include <mutex>
#include <unordered_map>

#include "rot_math.h"
#include "turn_dev.h"

namespace ha {

__device__ const int CONTACT_INDS_DEV[9] = {0, 4, 5, 7, 8, 10, 11, 20, 21};
constexpr int PW = 348, NPART = 15;       // world state width; per-frame partial sums: g_R (9) | g_t (3) | g_trans0 (3)

__device__ __forceinline__ int contact_slot(int joint) {
#pragma unroll
  for (int k = 0; k < 9; ++k)
    if (CONTACT_INDS_DEV[k] == joint) return k;
  return -1;
}

__global__ __launch_bounds__(64) void rollout_post_fwd_kernel(ha_rollout_post_args a) {
  const int T = a.S + 1, f = blockIdx.x, b = f / T, t = f - b * T, j = threadIdx.x;
  const float* w = t > 0 ? a.world + ((size_t)b * a.S + (t - 1)) * PW : nullptr;
  float aa_root[3] = {0.f, 0.f, 0.f}, tr[3] = {0.f, 0.f, 0.f};
  if (j < 22) {
    // rotation of joint j (root or body j-1) as axis-angle
    float aa[3];
    if (t == 0) {
      const float* src = j == 0 ? a.root0 + (size_t)b * 3 : a.pose0 + (size_t)b * 63 + (j - 1) * 3;
      aa[0] = src[0]; aa[1] = src[1]; aa[2] = src[2];
    } else {
      float R[9];
      const float* src = j == 0 ? w + 6 : w + 18 + 9 * (j - 1);
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = src[i];
      rotmat_to_aa(R, aa);
    }
    float* dst = j == 0 ? a.root_orient + (size_t)f * 3 : a.pose_body + (size_t)f * 63 + (j - 1) * 3;
    dst[0] = aa[0]; dst[1] = aa[1]; dst[2] = aa[2];
    if (j == 0) { aa_root[0] = aa[0]; aa_root[1] = aa[1]; aa_root[2] = aa[2]; }
    // joint position
    const float* js = t == 0 ? a.joints0 + ((size_t)b * 22 + j) * 3 : w + 207 + 3 * j;
    float* jd = a.joints + ((size_t)f * 22 + j) * 3;
    jd[0] = js[0]; jd[1] = js[1]; jd[2] = js[2];
    // contacts: frame 0 repeats frame 1 (motion_optimizer.py:990-996)
    const int k = contact_slot(j);
    float conf = 0.f, lab = 0.f;
    if (k >= 0) {
      const float* wc = a.world + ((size_t)b * a.S + (t > 0 ? t - 1 : 0)) * PW + 339;
      conf = 1.0f / (1.0f + expf(-wc[k]));
      lab = conf > 0.5f ? 1.f : 0.f;
    }
    a.contacts_conf[(size_t)f * 22 + j] = conf;
    a.contacts[(size_t)f * 22 + j] = lab;
  }
  if (j == 0) {
    const float* ts = t == 0 ? a.trans0 + (size_t)b * 3 : w;
    tr[0] = ts[0]; tr[1] = ts[1]; tr[2] = ts[2];
    float* td = a.trans + (size_t)f * 3;
    td[0] = tr[0]; td[1] = tr[1]; td[2] = tr[2];
    if (a.c2p_R) {
      const float* R = a.c2p_R + (size_t)b * 9;
      const float* t0 = a.trans0 + (size_t)b * 3;
      float Rm[9], N[9], aa[3];
      rodrigues(aa_root, Rm);
      mat3_tmul(R, Rm, N);                       // R^T Rm
      rotmat_to_aa(N, aa);
      float* cr = a.cam_root_orient + (size_t)f * 3;
      cr[0] = aa[0]; cr[1] = aa[1]; cr[2] = aa[2];
      const float d[3] = {tr[0] - t0[0], tr[1] - t0[1], tr[2] - t0[2]};
      float o[3];
      mat3_tvec(R, d, o);                        // R^T d
      float* ct = a.cam_trans + (size_t)f * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) ct[c] = o[c] - a.c2p_t[(size_t)b * 3 + c];
    }
  }
}

__global__ __launch_bounds__(64) void rollout_post_bwd_kernel(ha_rollout_post_args a) {
  const int T = a.S + 1, f = blockIdx.x, b = f / T, t = f - b * T, j = threadIdx.x;
  const float* w = t > 0 ? a.world + ((size_t)b * a.S + (t - 1)) * PW : nullptr;
  float* gw = t > 0 ? a.g_world + ((size_t)b * a.S + (t - 1)) * PW : nullptr;
  auto in3 = [&](const float* p, size_t off, float (&o)[3]) {
    if (p) { o[0] = p[off]; o[1] = p[off + 1]; o[2] = p[off + 2]; } else { o[0] = o[1] = o[2] = 0.f; }
  };
  float part[NPART];
#pragma unroll
  for (int i = 0; i < NPART; ++i) part[i] = 0.f;
  if (gw) {                                        // channels no output reads: translational / angular / joint velocities
    for (int c = 3 + j; c < 6; c += 64) gw[c] = 0.f;
    for (int c = 15 + j; c < 18; c += 64) gw[c] = 0.f;
    for (int c = 273 + j; c < 339; c += 64) gw[c] = 0.f;
  }
  if (j < 22) {
    // ---- joint rotation: adjoint of R -> axis-angle (root: plus the camera-frame branch) ---------------------------------------
    float g_aa[3];
    if (j == 0) in3(a.g_root_orient, (size_t)f * 3, g_aa);
    else in3(a.g_pose_body, (size_t)f * 63 + (j - 1) * 3, g_aa);
    if (j == 0) {
      float g_tr[3];
      in3(a.g_trans, (size_t)f * 3, g_tr);
      if (a.c2p_R) {
        const float* R = a.c2p_R + (size_t)b * 9;
        const float* t0 = a.trans0 + (size_t)b * 3;
        const float* aa_root = a.root_orient + (size_t)f * 3;       // forward output (frame 0: root0)
        float g_cr[3], g_ct[3];
        in3(a.g_cam_root_orient, (size_t)f * 3, g_cr);
        in3(a.g_cam_trans, (size_t)f * 3, g_ct);
        // cam_root = aa(N), N = R^T Rm, Rm = rodrigues(aa_root)
        float Rm[9], N[9], gN[9], gRm[9], gaa[3];
        const float ar[3] = {aa_root[0], aa_root[1], aa_root[2]};
        rodrigues(ar, Rm);
        mat3_tmul(R, Rm, N);
        rotmat_to_aa_bwd(N, g_cr, gN);
        mat3_mul(R, gN, gRm);                    // gRm = R gN
        // gR[j][i] += sum_k Rm[j][k] gN[i][k]  ->  gR += Rm gN^T
        float gR[9];
        mat3_mult(Rm, gN, gR);
        rodrigues_bwd(ar, gRm, gaa);
#pragma unroll
        for (int c = 0; c < 3; ++c) g_aa[c] += gaa[c];
        // cam_trans = R^T (x_t - x_0) - t
        const float* xt = t == 0 ? t0 : w;
        const float d[3] = {xt[0] - t0[0], xt[1] - t0[1], xt[2] - t0[2]};
        float Rg[3];
        mat3_vec(R, g_ct, Rg);                   // R g_ct
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          g_tr[c] += Rg[c];
          part[12 + c] -= Rg[c];
          part[9 + c] -= g_ct[c];
        }
        // gR[j][i] += d_j g_ct_i
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) gR[r * 3 + c] += d[r] * g_ct[c];
#pragma unroll
        for (int i = 0; i < 9; ++i) part[i] = gR[i];
      }
      if (t == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) part[12 + c] += g_tr[c];
      } else {
        gw[0] = g_tr[0]; gw[1] = g_tr[1]; gw[2] = g_tr[2];
      }
    }
    if (t == 0) {
      float* dst = j == 0 ? a.g_root0 + (size_t)b * 3 : a.g_pose0 + (size_t)b * 63 + (j - 1) * 3;
      dst[0] = g_aa[0]; dst[1] = g_aa[1]; dst[2] = g_aa[2];
    } else {
      float R[9], gR[9];
      const float* src = j == 0 ? w + 6 : w + 18 + 9 * (j - 1);
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = src[i];
      rotmat_to_aa_bwd(R, g_aa, gR);
      float* dst = j == 0 ? gw + 6 : gw + 18 + 9 * (j - 1);
#pragma unroll
      for (int i = 0; i < 9; ++i) dst[i] = gR[i];
    }
    // ---- joint positions ------------------------------------------------------------------------------------------------------------
    float gj[3];
    in3(a.g_joints, ((size_t)f * 22 + j) * 3, gj);
    float* jd = t == 0 ? a.g_joints0 + ((size_t)b * 22 + j) * 3 : gw + 207 + 3 * j;
    jd[0] = gj[0]; jd[1] = gj[1]; jd[2] = gj[2];
    // ---- contacts: confidence of frame t comes from the logits of step max(t-1, 0); frame 1's logits also feed frame 0 -----------------
    const int k = contact_slot(j);
    if (k >= 0 && t > 0) {
      const float conf = a.contacts_conf[(size_t)f * 22 + j];
      float g = a.g_contacts_conf ? a.g_contacts_conf[(size_t)f * 22 + j] : 0.f;
      if (t == 1 && a.g_contacts_conf) g += a.g_contacts_conf[(size_t)(f - 1) * 22 + j];
      gw[339 + k] = g * conf * (1.0f - conf);
    }
  }
  if (j == 0) {
    float* P = a.partial + (size_t)f * NPART;
#pragma unroll
    for (int i = 0; i < NPART; ++i) P[i] = part[i];
  }
}

// per sequence: sums of the per-frame partials in frame order
__global__ __launch_bounds__(64) void rollout_post_reduce_kernel(ha_rollout_post_args a) {
  const int T = a.S + 1, b = blockIdx.x, i = threadIdx.x;
  if (i >= NPART) return;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += a.partial[((size_t)b * T + t) * NPART + i];
  if (i < 9) { if (a.g_c2p_R) a.g_c2p_R[(size_t)b * 9 + i] = s; }
  else if (i < 12) { if (a.g_c2p_t) a.g_c2p_t[(size_t)b * 3 + (i - 9)] = s; }
  else a.g_trans0[(size_t)b * 3 + (i - 12)] = s;
}

constexpr int POST_CH = 64;               // frames per staged chunk of rollout_post_sums_kernel
constexpr int POST_LD = (POST_CH * NPART + 255) / 256;      // loads per thread and chunk

// rollout_post_reduce_kernel and the optional row-sum task (ha_seq_sum_add's work) in one launch of 256-thread blocks.
// Blocks < B: the sequence's T x 15 partials are contiguous -- all threads fetch a chunk of POST_CH frames at once (independent, coalesced
// loads instead of one dependent load per frame and lane), lanes < 15 then add in ascending t as rollout_post_reduce_kernel does.
// The next B blocks (with sum_src): seq_sum_add_block for one sequence each.
// Then the turn-around riders (turn_dev.h; the host passes their fields only when they ride): one block per four (row, step) pairs of the prior
// adjoint's layout pass -- a wave each, as prior_io_kernel's blocks -- and one block per TURN_CLR_WORDS exchange words to clear.
__global__ __launch_bounds__(256) void rollout_post_sums_kernel(ha_rollout_post_args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];     // [POST_CH][15] | [4][64]
  const int T = a.S + 1, i = threadIdx.x;
  if ((int)blockIdx.x >= a.B) {
    int blk = blockIdx.x - a.B;
    const int nsum = a.sum_src ? a.B : 0;
    if (blk < nsum) {
      seq_sum_add_block(a.sum_src, a.sum_add1, a.sum_add2, a.sum_out, blk, T, a.sum_W, smem);
      return;
    }
    blk -= nsum;
    const int rows = a.lay_RT * 32, items = a.lay_dst ? rows * a.S : 0, nlay = (items + 3) >> 2;
    if (blk < nlay) {
      const int item = blk * 4 + (i >> 6);
      if (item < items)
        prior_adjoint_rows(a.lay_g_mu, a.lay_g_var, a.lay_pri_out, (size_t)a.lay_step_stride, 1, a.lay_pad, a.lay_dst, a.B, a.S, a.lay_RT,
                           item % rows, item / rows, i & 63);
      return;
    }
    zero_words_block(reinterpret_cast<unsigned*>(a.clr), (size_t)a.clr_words, blk - nlay);
    return;
  }
  const int b = blockIdx.x;
  const float* P = a.partial + (size_t)b * T * NPART;
  float s = 0.f;
  for (int t0 = 0; t0 < T; t0 += POST_CH) {
    const int nt = T - t0 < POST_CH ? T - t0 : POST_CH;
    float r[POST_LD];                 // (unconditional loads, index clamped to the chunk: a load under a condition is waited for on its own)
#pragma unroll
    for (int u = 0; u < POST_LD; ++u) { const int e = i + 256 * u; r[u] = P[(size_t)t0 * NPART + (e < nt * NPART ? e : nt * NPART - 1)]; }
#pragma unroll
    for (int u = 0; u < POST_LD; ++u) { const int e = i + 256 * u; if (e < nt * NPART) smem[e] = r[u]; }
    __syncthreads();
    if (i < NPART)
      for (int t = 0; t < nt; ++t) s += smem[t * NPART + i];
    __syncthreads();
  }
  if (i >= NPART) return;
  if (i < 9) { if (a.g_c2p_R) a.g_c2p_R[(size_t)b * 9 + i] = s; }
  else if (i < 12) { if (a.g_c2p_t) a.g_c2p_t[(size_t)b * 3 + (i - 9)] = s; }
  else a.g_trans0[(size_t)b * 3 + (i - 12)] = s;
}

// the riders as launches of their own ("turn_merge" bit HA_TURN_POST off): the grid of prior_io_kernel (rollout.hip)
__global__ __launch_bounds__(64) void prior_layout_kernel(ha_rollout_post_args a) {
  prior_adjoint_rows(a.lay_g_mu, a.lay_g_var, a.lay_pri_out, (size_t)a.lay_step_stride, 1, a.lay_pad, a.lay_dst, a.B, a.S, a.lay_RT,
                     blockIdx.x, blockIdx.y, threadIdx.x);
}

extern int g_loss_merge;      // fitloss.hip
int g_turn_merge = HA_TURN_DZ | HA_TURN_POST | HA_TURN_FWD_CLEAR;

// ---- marks of the turn-around riders (turn_dev.h): region address -> what a host launch has done to it since its last use -----------
static std::mutex g_turn_mu;
static std::unordered_map<const void*, unsigned> g_turn_marks;
void turn_mark(const void* p, unsigned bits) {
  std::lock_guard<std::mutex> lk(g_turn_mu);
  g_turn_marks[p] |= bits;
}
bool turn_take(const void* p, unsigned bits) {
  std::lock_guard<std::mutex> lk(g_turn_mu);
  const auto it = g_turn_marks.find(p);
  if (it == g_turn_marks.end()) return false;
  const bool all = (it->second & bits) == bits;
  it->second &= ~bits;
  if (!it->second) g_turn_marks.erase(it);
  return all;
}
void turn_forget(const void* p) {
  std::lock_guard<std::mutex> lk(g_turn_mu);
  g_turn_marks.erase(p);
}

}  // namespace ha

using namespace ha;

extern "C" int ha_rollout_post_forward(const ha_rollout_post_args* args, void* stream) {
  HA_REQUIRE(args, "ha_rollout_post_forward: null argument");
  const ha_rollout_post_args& a = *args;
  HA_REQUIRE(a.B >= 1 && a.S >= 1, "ha_rollout_post_forward: B and S must be >= 1");
  HA_REQUIRE(a.world && a.trans0 && a.root0 && a.pose0 && a.joints0, "ha_rollout_post_forward: null input");
  HA_REQUIRE(a.trans && a.root_orient && a.pose_body && a.joints && a.contacts_conf && a.contacts, "ha_rollout_post_forward: null output");
  HA_REQUIRE((a.c2p_R == nullptr) == (a.c2p_t == nullptr), "ha_rollout_post_forward: c2p_R and c2p_t go together");
  HA_REQUIRE(!a.c2p_R || (a.cam_trans && a.cam_root_orient), "ha_rollout_post_forward: camera-frame outputs missing");
  HA_LAUNCH(rollout_post_fwd_kernel, dim3(a.B * (a.S + 1)), dim3(64), 0, (hipStream_t)stream, a);
  HA_LAUNCH_CHECK();
  return HA_OK;
}

extern "C" int ha_rollout_post_backward(const ha_rollout_post_args* args, void* stream) {
  HA_REQUIRE(args, "ha_rollout_post_backward: null argument");
  const ha_rollout_post_args& a = *args;
  HA_REQUIRE(a.B >= 1 && a.S >= 1, "ha_rollout_post_backward: B and S must be >= 1");
  HA_REQUIRE(a.world && a.trans0 && a.root_orient && a.contacts_conf, "ha_rollout_post_backward: forward tensors missing");
  HA_REQUIRE(a.g_world && a.g_trans0 && a.g_root0 && a.g_pose0 && a.g_joints0 && a.partial, "ha_rollout_post_backward: null output");
  HA_REQUIRE(!a.c2p_R || (a.g_c2p_R && a.g_c2p_t), "ha_rollout_post_backward: cam2prior gradient outputs missing");
  HA_REQUIRE(!a.sum_src || (a.sum_out && a.sum_W >= 1 && a.sum_W <= 64), "ha_rollout_post_backward: the row-sum task needs sum_out and 1 <= sum_W <= 64");
  HA_REQUIRE(!a.lay_dst || (a.lay_pri_out && a.lay_RT == (a.B + 31) / 32 && a.lay_pad >= 2 * TURN_ZD && a.lay_pad % 4 == 0 && a.lay_step_stride >= 0 &&
                            (int64_t)a.lay_RT * 32 * a.S < ((int64_t)1 << 29)),
             "ha_rollout_post_backward: the layout task needs lay_pri_out, lay_RT = ceil(B / 32) and lay_pad >= 96, a multiple of 4");
  HA_REQUIRE(!a.clr || (a.clr_words >= 1 && a.clr_words < ((int64_t)1 << 31)), "ha_rollout_post_backward: the clear task needs 1 <= clr_words < 2^31");
  hipStream_t st = (hipStream_t)stream;
  const bool ride = g_loss_merge && (g_turn_merge & HA_TURN_POST);
  if (a.sum_src && !g_loss_merge) {
    const int rc = ha_seq_sum_add(a.B, a.S + 1, a.sum_W, a.sum_src, a.sum_add1, a.sum_add2, a.sum_out, stream);
    if (rc != HA_OK) return rc;
  }
  HA_LAUNCH(rollout_post_bwd_kernel, dim3(a.B * (a.S + 1)), dim3(64), 0, st, a);
  HA_LAUNCH_CHECK();
  if (g_loss_merge) {
    ha_rollout_post_args k = a;
    if (!ride) { k.lay_dst = nullptr; k.clr = nullptr; }
    const unsigned nlay = k.lay_dst ? (unsigned)((a.lay_RT * 32 * a.S + 3) / 4) : 0u, nclr = k.clr ? zero_words_blocks((size_t)a.clr_words) : 0u;
    HA_LAUNCH(rollout_post_sums_kernel, dim3(a.B * (a.sum_src ? 2 : 1) + nlay + nclr), dim3(256), POST_CH * NPART * sizeof(float), st, k);
  } else HA_LAUNCH(rollout_post_reduce_kernel, dim3(a.B), dim3(64), 0, st, a);
  HA_LAUNCH_CHECK();
  if (!ride) {
    if (a.lay_dst) {
      HA_LAUNCH(prior_layout_kernel, dim3(a.lay_RT * 32, a.S), dim3(64), 0, st, a);
      HA_LAUNCH_CHECK();
    }
    if (a.clr) {
      zero_async(a.clr, (size_t)a.clr_words * 4, st);
      HA_LAUNCH_CHECK();
    }
  }
  if (a.lay_dst) turn_mark(a.lay_dst, TURN_MARK_LAID);
  if (a.clr) turn_mark(a.clr, TURN_MARK_CLEARED);
  return HA_OK;
}
