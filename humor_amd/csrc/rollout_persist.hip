// Persistent, weight-stationary forward of the HuMoR decoder roll-out on gfx950 (humor/models/humor_model.py:785-1017 for
// B <= 32 sequences): ONE launch for all S steps instead of 5 dependent launches per step.
//
// Why: at 32 rows the launch chain is a latency chain (5 dispatches x ~6.5 us per step; the 138 MFLOP of a step are ~1 us of the
// chip's fp32 matrix rate).  The structure that removes the dispatches without a whole-chip barrier per layer:
//   * the sequences are independent, so the batch is cut into 8 TEAMS of 4 sequences, one team per XCD (32 CUs, one L2):
//     a team never talks to another team -- no cross-XCD traffic, no grid barrier;
//   * the decoder's 2.16 M fp32 weights (8.7 MB) do not fit one CU, but they fit the REGISTER FILES of one XCD: every wave of a
//     team (32 CUs x 4 SIMDs, one wave per SIMD, 512 VGPRs) keeps its 286-register share of the four layers for the whole launch
//     (8 x 8.7 MB = 70 MB of the chip's 128 MB of VGPRs) -- per step only activations move;
//   * 4 rows are the native M of v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4 outer products per instruction = 16 k's of one
//     4-row x 4-column tile): a wave owns 8 (4) output columns of a layer and the WHOLE K, so there is no cross-wave reduction,
//     only a 16-lane-group reduction of the accumulators;
//   * a layer's output (4 rows x <=1024 channels) goes to the other 31 CUs of the team as 8-byte {value, tag} granules through
//     the team's L2: the data is its own flag (tag = 4 step + layer + 1), consumers sweep it with L1-bypassing (sc1) loads until
//     every tag matches -- one memory round trip per layer, no counters, no fences; GroupNorm + ReLU run on the consumer side
//     (every CU needs the whole activation as its A operand anyway), the residual composition / heading alignment / frame changes
//     of the step ("glue") run redundantly on every CU, one wave per sequence.
// Teams are formed at run time from HW_REG_XCC_ID (a block joins the team of the XCD it landed on), so results never depend on
// the dispatcher's placement; what the path needs is 32 resident blocks per XCD -- every wait is bounded, a team that does not
// complete reports through a host-mapped error word and the caller falls back to the launch chain.
//
// The kernel fills the same stash as the launch-chain forward (states of all steps, accumulated world transforms, one
// pre-activation slab per decoder layer and step), so the batched prior and the existing adjoint run unchanged behind it.
#include "rollout_persist.h"

#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "rot_math.h"
#include "lane_reduce.h"
#include "turn_dev.h"

namespace ha {

namespace {
constexpr int P_DIN = 339, P_DINP = 340, P_XPAD = 352, P_ZD = 48, P_RAW = 216, P_RAWPAD = 224, P_STATE = 348;
constexpr int P_H0 = 1024, P_H1 = 1024, P_H2 = 512;
constexpr int TEAM_CUS = 32, NTEAMS = 8, ROWS = 4, NWAVES_TEAM = TEAM_CUS * 4;
// K chunks (16 k's each) per layer: main part + 3 chunks of latent skip
constexpr int NC0 = P_XPAD / 16, NC1 = P_H0 / 16, NC2 = P_H1 / 16, NC3 = P_H2 / 16, NCZ = P_ZD / 16;
// weight registers of a wave: [chunk][column group] per layer
constexpr int R0 = 0, R1 = R0 + (NC0 + NCZ) * 2, R2 = R1 + (NC1 + NCZ) * 2, R3 = R2 + (NC2 + NCZ), NREG = R3 + (NC3 + NCZ);
// Register plan of a wave (512 registers: 256 AGPRs + 256 VGPRs).  The MFMAs' B operand is read where the weight lives; everything the
// VALU touches must be a VGPR.  Round 4: the ACCUMULATORS are VGPR quads (the results are summed and published by VALU code: no
// v_accvgpr_read per value) and the AGPR half holds weights only -- all 256 of it in the forward (the remaining 30 weights are VGPRs),
// 224 of the adjoint's 246 (its prefetch registers keep the VGPR half full; beyond 224 the allocator starts copying weights INTO AGPRs in front of the asm MFMAs -- an unguarded hazard, wrong gradients measured: tools/isa_census.py reports such copies and tests/test_build.py refuses them).  Round 3 had 200 weights + the 32
// accumulator registers in AGPRs and 86 / 46 VGPR-class weights that the allocator parked in AGPRs and copied back (v_accvgpr_read +
// s_nop) in front of every use: L2 / L3 products at 17 cycles per MFMA instead of 8 (profiles/r04_persist).
#ifndef HA_NWA
#define HA_NWA 256
#endif
#ifndef HA_NWA_B
#define HA_NWA_B 224
#endif
#ifdef HA_ACC_A
#define HA_ACC "a"
#else
#define HA_ACC "v"
#endif
constexpr int NWA = HA_NWA;                // weight registers kept in AGPRs (the MFMAs' B operand reads them there); the rest in VGPRs
constexpr int L3_WAVES = P_RAW / 4;      // 54 waves own the 216 output columns of the last layer
// exchange space (bytes): 64-byte header, then per team the four activations as granules [channel][4 rows] x 8 B
constexpr unsigned XCH_HDR = 256;
constexpr unsigned ACT_OFF0 = 0, ACT_OFF1 = ACT_OFF0 + P_H0 * 32, ACT_OFF2 = ACT_OFF1 + P_H1 * 32, ACT_OFF3 = ACT_OFF2 + P_H2 * 32;
constexpr unsigned TEAM_BYTES = ACT_OFF3 + P_XPAD * 32;       // (the adjoint's last buffer, dL/dx through layer 0, is the widest: 352 channels)
constexpr unsigned XCH_BYTES = XCH_HDR + NTEAMS * TEAM_BYTES;
// LDS (floats)
constexpr int L_XS0 = 0, L_XS1 = L_XS0 + P_XPAD * 4, L_XS2 = L_XS1 + P_H0 * 4, L_XS3 = L_XS2 + P_H1 * 4, L_ZS = L_XS3 + P_H2 * 4;
// (the state rows and the accumulated transforms are double-buffered: step t reads buffer t & 1 and writes the other one, so the
// waves of a CU can work on the same sequence side by side -- see the glue)
constexpr int L_SX = L_ZS + P_ZD * 4, L_SRAW = L_SX + 2 * ROWS * P_XPAD, L_SW = L_SRAW + ROWS * P_RAWPAD, L_SG = L_SW + ROWS * P_XPAD;
constexpr int L_GSZ = ROWS * 12 + 16;
constexpr int L_SGL = L_SG + 2 * L_GSZ, L_T2J = L_SGL + ROWS * 32, L_ZERO = L_T2J + 16, L_MISC = L_ZERO + 16, L_GB = L_MISC + 64, L_TOTAL = L_GB + 4 * (P_H0 + P_H1 + P_H2);   // L_GB: GroupNorm affine, gamma | beta of the three activations
// per-step results of a team (world states, next state slab, accumulated transforms) leave through all 32 CUs, COPY_PER_CU floats each
constexpr int COPY_WORLD = ROWS * P_STATE, COPY_XT = ROWS * P_DINP, COPY_G = ROWS * 12, COPY_GL = ROWS * 32;
constexpr int COPY_TOTAL = COPY_WORLD + COPY_XT + COPY_G + COPY_GL;
constexpr int COPY_PER_CU = (COPY_TOTAL + TEAM_CUS - 1) / TEAM_CUS;
#ifdef HA_SIMT_EMU
static int SPIN_LIMIT = 40000;           // (host emulator: a poll sleeps 20 ms; the failure-protocol test lowers the bound -- tests/simt_emu/rollout_persist_emu.cpp)
#else
constexpr int SPIN_LIMIT = 40000;        // bounded waits (~1 us per spin)
#endif

// ---- persistent adjoint: transposed layers, K chunks = forward output channels / 16 ---------------------------------------------
constexpr int BC3 = P_RAWPAD / 16, BC2 = P_H2 / 16, BC1 = P_H1 / 16, BC0 = P_H0 / 16;
// weight registers of a wave: main products (dL/d activation), then its share of the dL/dz products
constexpr int BR3 = 0, BR2 = BR3 + BC3, BR1 = BR2 + BC2 * 2, BR0 = BR1 + BC1 * 2;
constexpr int BC0_LDS = 24, BC0_REG = BC0 - BC0_LDS;      // layer 0: the last BC0_LDS chunks' weights live in LDS (register budget)
constexpr int DZ0_CH = 8, DZ1_CH = 8, DZ2_CH = 4, DZ3_CH = 2;             // chunks per dL/dz task (12 column groups x K splits)
constexpr int DZ0_WAVES = 12 * (BC0 / DZ0_CH), DZ1_WAVES = 12 * (BC1 / DZ1_CH), DZ2_WAVES = 12 * (BC2 / DZ2_CH), DZ3_WAVES = 12 * (BC3 / DZ3_CH);
constexpr int BRZ0 = BR0 + BC0_REG, BRZ1 = BRZ0 + DZ0_CH, BRZ2 = BRZ1 + DZ1_CH, BRZ3 = BRZ2 + DZ2_CH, NREG_B_ALL = BRZ3 + DZ3_CH;
constexpr int NREG_B = BRZ0, NDZ = NREG_B_ALL - NREG_B;       // registers: the main products; LDS: the wave's dL/dz weights [NDZ][64 lanes]
constexpr int NLW = NDZ + BC0_LDS;                            // LDS-resident weight vectors per wave: dL/dz tasks, then layer 0's tail
constexpr int NWA_B = HA_NWA_B;
constexpr int L0T_WAVES = P_XPAD / 4 - 3;      // 85 waves own the 340 columns of dL/dx through layer 0
// partial dL/dz slots per (step, sequence): K splits of the four layers, summed in this order by dz_reduce_kernel
constexpr int DZ_S0 = 0, DZ_S1 = DZ_S0 + BC0 / DZ0_CH, DZ_S2 = DZ_S1 + BC1 / DZ1_CH, DZ_S3 = DZ_S2 + BC2 / DZ2_CH, DZ_SLOTS = DZ_S3 + BC3 / DZ3_CH;
// exchange space of the adjoint (granules [channel][4 rows] x 8 B per team; same region as the forward's)
constexpr unsigned GA_OFF3 = 0, GA_OFF2 = GA_OFF3 + P_H2 * 32, GA_OFF1 = GA_OFF2 + P_H1 * 32, GX_OFF0 = GA_OFF1 + P_H0 * 32;
static_assert(GX_OFF0 + P_XPAD * 32 <= TEAM_BYTES, "the adjoint's exchange buffers fit the forward's region");
// LDS of the adjoint (floats): per-step inputs double-buffered (prefetched one step ahead), operands, adjoint states
constexpr int PF_X = 0, PF_RAW = PF_X + ROWS * P_XPAD, PF_GW = PF_RAW + ROWS * P_RAWPAD, PF_GL = PF_GW + ROWS * P_XPAD, PF_G = PF_GL + ROWS * 32;
constexpr int PF_GXP = PF_G + 64, PF_SIZE = PF_GXP + ROWS * P_XPAD;
constexpr int LB_PF = 0, LB_D3 = LB_PF + 2 * PF_SIZE, LB_D1 = LB_D3 + P_RAWPAD * 4, LB_D0 = LB_D1 + P_H1 * 4;
constexpr int LB_D2 = LB_D0;       // (dh2 and dh0 live two phases apart: same space)
constexpr int LB_GXN = LB_D0 + P_H0 * 4, LB_GXD = LB_GXN + ROWS * P_XPAD, LB_CARRY = LB_GXD + ROWS * P_XPAD, LB_MISC = LB_CARRY + 80;
constexpr int LB_GB = LB_MISC + 64, LB_WZ = LB_GB + 2 * (P_H0 + P_H1 + P_H2);      // GroupNorm affine: gamma | beta of the three activations
constexpr int LB_EXTRA = LB_WZ + 4 * NLW * 64;                                     // (LDS-resident weights of the CU's four waves end here)
// glue adjoint hand-offs: heading | root rotation set-ups [row][16 | 8], dL/dpR columns | dL/dW [row][12 | 12], t2j [row][4]
constexpr int LB_PREP = LB_EXTRA, LB_COL = LB_PREP + ROWS * 24, LB_T2J = LB_COL + ROWS * 24, LB_TOTAL = LB_T2J + ROWS * 4;
// the 27 sums of the glue adjoint go through LDS (transposed partials, stride RED_LD: conflict-free 16-byte row reads), in the space of
// the dh1 operand, which is dead between the end of one step and the layer-1 phase of the next
constexpr int RED_LD = 36, RED_BLOCK = 27 * RED_LD + 36;
static_assert(4 * RED_BLOCK <= P_H1 * 4, "reduction scratch fits the dh1 operand");
static_assert(LB_TOTAL * 4 <= 160 * 1024, "the adjoint's LDS fits one CU");
}  // namespace

size_t persist_ws_floats() { return (XCH_BYTES + 3) / 4; }
int persist_dz_slots() { return DZ_SLOTS; }

struct PersistArgs {
  int B, S;
  const float* Wreg;        // [128 waves][NREG][64 lanes]
  const float* bias[4];     // [1024] [1024] [512] [224]
  const float* gamma[3];    // GroupNorm affine of the inputs of layers 1..3
  const float* beta[3];
  const float* past_in0;
  const float* z_seq;
  float* world;
  float* xT;
  float* steps;
  size_t per_step, off_G, off_dec[4];
  size_t off_gn[3], off_gl;  // per step: GroupNorm statistics [16 groups][32 rows][2] of the three hidden activations; glue record [32 rows][32]
  size_t off_ht[3];          // per step: the hidden pre-activations again, team layout [8 teams][channel][4 rows]
  float* t2j;
  unsigned char* xch;
  unsigned* err;            // host-mapped error word
  int inject;               // test hook (ha_tune_set "rollout_persist_inject"): member 3 of team 0 leaves at once -> the team's bounded waits run out
  int hidden_slabs;         // 1: the hidden pre-activations also as launch-chain slabs (off_dec[0..2]); 0: team layout (off_ht) only
};

struct PersistNet {
  int device = 0;
  float* Wreg = nullptr;
  float* Wreg_b = nullptr;          // transposed layers for the adjoint
  float* Wreg_pf = nullptr;         // pipelined forward (32 < B <= 256): role-ordered packing, rollout_pipe.inc
  float* Wreg_pb = nullptr;         // pipelined adjoint
  float* bias[4] = {nullptr, nullptr, nullptr, nullptr};
  float* gamma[3] = {nullptr, nullptr, nullptr};
  float* beta[3] = {nullptr, nullptr, nullptr};
  unsigned* err_host = nullptr;    // hipHostMalloc'ed, mapped
  unsigned* err_dev = nullptr;
  bool disabled = false;
  bool reported = false;            // the failure has been returned to a caller once
  long long launches = 0, launches_bwd = 0;
};

// (the exchange consumers below -- sweeps, slot map, GroupNorm (+ adjoint) -- also compile for the host SIMT emulator: tests/test_rollout_emu.py
// runs them against PyTorch through the ha_emu_* hooks of tests/simt_emu/rollout_persist_emu.cpp, which includes this file; everything from the MFMA code on is gfx950 only)
typedef float pvf4 __attribute__((ext_vector_type(4)));
typedef unsigned puv4 __attribute__((ext_vector_type(4)));

struct PersistBwdArgs;
#ifdef HA_PERSIST_TIMING
// profiling build only (tools/persist_phase_timing.py): phase timestamps (s_memtime) of one wave for steps PT_T0 .. PT_T0 + 7
constexpr int PT_T0 = 8, PT_N = 24;
__device__ unsigned long long g_pts[2][8][PT_N];      // [0]: team 0 member 5 (an ordinary CU), [1]: team 0 member 0 (the writer)
#define PT(i)                                                                        \
  do {                                                                               \
    if (pt_on && t >= PT_T0 && t < PT_T0 + 8) g_pts[pt_slot][t - PT_T0][i] = clock64(); \
  } while (0)
#define PT_ARGS , bool pt_on, int pt_slot, int t
#define PT_PASS , pt_on, pt_slot, t
__device__ unsigned long long g_ptb[8][PT_N];         // adjoint: team 0 member 5, steps S-1-PT_T0 downwards
__device__ unsigned g_spin_hist[1024][8];             // per wave: sweeps (all steps) that needed 0, 1, .. 6, >= 7 extra polls
#ifdef HA_PERSIST_SPINS
#define PT_SPINS(n) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_spin_hist[blockIdx.x * 4 + (threadIdx.x >> 6)][(n) < 7 ? (n) : 7], 1u); } while (0)
#else
#define PT_SPINS(n)
#endif
#define PTB(i)                                                                                       \
  do {                                                                                               \
    if (ptb_on && (a.S - 1 - t) >= PT_T0 && (a.S - 1 - t) < PT_T0 + 8) g_ptb[a.S - 1 - t - PT_T0][i] = clock64(); \
  } while (0)
#define PTB_ARGS , bool ptb_on, int t, const PersistBwdArgs& a
#define PTB_PASS , ptb_on, t, a
__device__ unsigned long long g_ptc[2][8][8];         // adjoint glue, finer: [0] = wave 0 (rotations), [1] = wave 2 (vector tasks) of team 0 member 5
#define PTC(w, i)                                                                                                   \
  do {                                                                                                              \
    if (team == 0 && m == 5 && tid == 128 * (w) && (a.S - 1 - t) >= PT_T0 && (a.S - 1 - t) < PT_T0 + 8) g_ptc[w][a.S - 1 - t - PT_T0][i] = clock64(); \
  } while (0)
#else
#define PT_SPINS(n)
#define PT(i)
#define PT_ARGS
#define PT_PASS
#define PTB(i)
#define PTB_ARGS
#define PTB_PASS
#define PTC(w, i)
#endif

__device__ __forceinline__ size_t pq(int c) { return (size_t)(c >> 2) * 128 + (c & 3); }

__device__ __forceinline__ float as_f(unsigned u) { return __uint_as_float(u); }
__device__ __forceinline__ unsigned as_u(float f) { return __float_as_uint(f); }

// Sweeps this thread's NQ channels (channel tid + 256 q: 4 granules = 32 bytes each) until every tag matches; the loads bypass
// the CU's L1 (sc1).  Returns false when the wait ran out (a team member never published).
template <int NQ>
__device__ __forceinline__ bool sweep(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned tag, int nch, int tid, float (&x)[NQ][4]) {
  for (int spins = 0;; ++spins) {
    unsigned diff = 0;          // (no short-circuit: one straight-line batch of loads and compares)
    puv4 lo[NQ], hi[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      lo[q] = puv4{0u, tag, 0u, tag};
      hi[q] = lo[q];
      if (tid + 256 * q < nch) {          // channels beyond the activation's width: nothing to wait for
        lo[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + (unsigned)(tid + 256 * q) * 32u, 0, 16);
        hi[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + (unsigned)(tid + 256 * q) * 32u + 16u, 0, 16);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      diff |= (lo[q].y ^ tag) | (lo[q].w ^ tag) | (hi[q].y ^ tag) | (hi[q].w ^ tag);
      x[q][0] = as_f(lo[q].x); x[q][1] = as_f(lo[q].z); x[q][2] = as_f(hi[q].x); x[q][3] = as_f(hi[q].z);
    }
    if (__all(diff == 0)) { PT_SPINS(spins); return true; }
    if (spins > SPIN_LIMIT) return false;
    __builtin_amdgcn_s_sleep(1);
  }
}

// The same wait for a GroupNorm'ed hidden activation, in HALF granules: the thread's k-th load is piece tid + 256 k (16 bytes: one row
// pair of slot (tid >> 1) + 128 k), so a wave's load instruction covers 1 KB of contiguous exchange space -- every 128-byte line is
// requested by ONE instruction.  (sweep() above reads bytes 0-15 and 16-31 of a 32-byte slot with two instructions: the same number of
// instructions, but each touches twice the lines, half of every line unused; the texture path processes a 64 x 16-byte request line by
// line, and it is shared by everything a CU loads.)  The lane's row pair is its parity: rows 2 (tid & 1), 2 (tid & 1) + 1.
template <int NK>
__device__ __forceinline__ bool sweep_pairs(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned tag, int tid, float (&x)[NK][2]) {
  for (int spins = 0;; ++spins) {
    unsigned diff = 0;
    puv4 v[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + (unsigned)(tid + 256 * k) * 16u, 0, 16);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      diff |= (v[k].y ^ tag) | (v[k].w ^ tag);
      x[k][0] = as_f(v[k].x); x[k][1] = as_f(v[k].z);
    }
    if (__all(diff == 0)) { PT_SPINS(spins); return true; }
    if (spins > SPIN_LIMIT) return false;
    __builtin_amdgcn_s_sleep(1);
  }
}

// Exchange slots of a GroupNorm'ed activation.  The consumer's k-th load covers slot (tid >> 1) + 128 k (sweep_pairs) and wants its
// NK = GW / 8 values of a row to belong to ONE normalisation group, the group spread over exactly one 16-lane DPP row (8 slots x 2 row
// pairs):
//     slot (tid, k)  <->  channel GW (tid / 16) + 8 k + ((tid / 2) % 8)
// so a group's statistics are NK - 1 lane-local adds + one 3-stage DPP reduction over the row's lanes of equal parity
// (lr::parity_sum2: every such lane gets the bitwise identical total) -- no v_permlane swaps, no operand copies (round 3: channel =
// tid + 256 q, a group = a whole wave, 2 x wave_sum16 per layer = the issue-bound 2.1 k cycles of the phase tables).
// GW = 0: identity (no GroupNorm on the consumer side; swept with sweep()).
template <int GW>
__device__ __forceinline__ int xslot(int col) {
  if constexpr (GW == 0) return col;
  else return 8 * (col / GW) + (col & 7) + 128 * ((col >> 3) & (GW / 8 - 1));
}
template <int GW>
__device__ __forceinline__ int xchan(int tid, int k) { return GW * (tid >> 4) + 8 * k + ((tid >> 1) & 7); }

typedef float pvf2 __attribute__((ext_vector_type(2)));
template <int NK>
__device__ __forceinline__ float sum_k(const float (&v)[NK][2], int i) {
  if constexpr (NK == 8) return ((v[0][i] + v[1][i]) + (v[2][i] + v[3][i])) + ((v[4][i] + v[5][i]) + (v[6][i] + v[7][i]));
  else return (v[0][i] + v[1][i]) + (v[2][i] + v[3][i]);
}
// (the same tree on row pairs: the two rows of a lane are the two halves of packed fp32 instructions, v_pk_add / v_pk_mul)
template <int NK>
__device__ __forceinline__ pvf2 sum_kv(const pvf2 (&v)[NK]) {
  if constexpr (NK == 8) return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  else return (v[0] + v[1]) + (v[2] + v[3]);
}
// GroupNorm (two-pass statistics per row and group of GROUP = 8 NK channels) + ReLU of the thread's NK channels x 2 rows, the finished A
// operand to LDS as [channel][4 rows]
// stats (or null): the (mean, rstd) of every (group, row) go to stats[group][32 rows][2] for the adjoint (one CU of the team writes)
template <int NK, int GROUP>
__device__ __forceinline__ void norm_pairs(const float (&x)[NK][2], const float (&gam)[NK], const float (&bet)[NK], float* xs, int tid, float* stats, int row0) {
  static_assert(GROUP == 8 * NK && (NK == 4 || NK == 8), "a 16-lane row holds one group");
  const float inv_n = 1.0f / (float)GROUP;
  pvf2 xv[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) xv[k] = pvf2{x[k][0], x[k][1]};
  const pvf2 s1 = sum_kv<NK>(xv);
  float mu[2] = {s1[0], s1[1]};
  lr::parity_sum2(mu);
  const pvf2 muv = pvf2{mu[0], mu[1]} * inv_n;
  pvf2 d[NK], sq[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) { d[k] = xv[k] - muv; sq[k] = d[k] * d[k]; }
  const pvf2 s2 = sum_kv<NK>(sq);
  float var[2] = {s2[0], s2[1]};
  lr::parity_sum2(var);
  // (v_rsq_f32 itself: the argument is >= 1e-5, so rsqrtf's denormal pre-scaling never applies and the result is the same)
  const pvf2 rs2 = {__builtin_amdgcn_rsqf(var[0] * inv_n + 1e-5f), __builtin_amdgcn_rsqf(var[1] * inv_n + 1e-5f)};
  const int hp = tid & 1;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    pvf2 o = d[k] * rs2 * gam[k] + bet[k];
    o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f);
    *reinterpret_cast<pvf2*>(xs + (size_t)xchan<GROUP>(tid, k) * 4 + 2 * hp) = o;
  }
  if (stats && (tid & 14) == 0)          // two lanes per group (= 16-lane row): one per row pair
    *reinterpret_cast<pvf4*>(stats + ((size_t)(tid >> 4) * 32 + row0 + 2 * hp) * 2) = pvf4{muv[0], rs2[0], muv[1], rs2[1]};
}
// GroupNorm affine in LDS.  Forward (DUP): {gamma, beta, gamma, beta} per channel, so that a thread reads its channel's pair at the very
// index it stores the channel's row pair at ([channel][4 rows] + 2 (tid & 1)): one address register serves both.  Adjoint (LDS is
// short there): {gamma, beta} per channel.
template <bool DUP>
__device__ __forceinline__ void gb_fill(float* gb_lds, const float* gamma, const float* beta, int n, int tid) {
  for (int c = tid; c < n; c += 256) {
    if constexpr (DUP) *reinterpret_cast<pvf4*>(gb_lds + (size_t)c * 4) = pvf4{gamma[c], beta[c], gamma[c], beta[c]};
    else *reinterpret_cast<pvf2*>(gb_lds + (size_t)c * 2) = pvf2{gamma[c], beta[c]};
  }
}
template <int GROUP, bool DUP>
__device__ __forceinline__ pvf2 gb_at(const float* gb_lds, int tid, int k) {
  if constexpr (DUP) return *reinterpret_cast<const pvf2*>(gb_lds + (size_t)xchan<GROUP>(tid, k) * 4 + 2 * (tid & 1));
  else return *reinterpret_cast<const pvf2*>(gb_lds + (size_t)xchan<GROUP>(tid, k) * 2);
}
// consumer side of a hidden activation: sweep, GroupNorm + ReLU
template <int NQ, int GROUP, int PTI = 0>
__device__ __forceinline__ bool gather_norm(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned tag, const float* gb_lds,
                                            float* xs, int tid, float* stats, int row0 PT_ARGS) {
  constexpr int NK = 2 * NQ;
  float x[NK][2];
  if (!sweep_pairs<NK>(rs, off, tag, tid, x)) return false;
  PT(PTI);
  float gam[NK], bet[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const pvf2 gb = gb_at<GROUP, true>(gb_lds, tid, k);
    gam[k] = gb[0]; bet[k] = gb[1];
  }
  norm_pairs<NK, GROUP>(x, gam, bet, xs, tid, stats, row0);
  return true;
}

// one layer's share of a wave: all K chunks against the resident weight registers.  The A operands come from LDS in batches of
// MB chunks, the next batch's reads issued ahead of the current batch's MFMAs (the compiler otherwise waits for every read right
// before its first use: one LDS round trip per 4 MFMAs); two accumulators per column group break the 2-pass dependent chain.
constexpr int MB = 16;
template <int NC_MAIN, int NZ, int FIRST>
__device__ __forceinline__ void load_a(const float* xs, const float* zs, int lane, float (&av)[MB]) {
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int c = FIRST + i;
    if (c < NC_MAIN) av[i] = xs[64 * c + lane];
    else if (c < NC_MAIN + NZ) av[i] = zs[64 * (c - NC_MAIN) + lane];
  }
}
// The MFMAs are written as inline asm so that the weight operand can stay in the AGPR half of the wave's 512 registers: the B
// operand of an MFMA may be an AGPR, but the compiler only reads weights it has first copied to a VGPR (v_accvgpr_read + s_nop + MFMA
// through ONE temporary: 32 cycles per MFMA measured, against 8 of issue).  NWA weight registers live in AGPRs ("a"), the rest in
// VGPRs ("v").  8 accumulators (AGPR quads) per wave are used round-robin: a dependent accumulate has ~64 cycles of latency, and
// the asm statements are volatile so the rotation (distance 8 between two MFMAs on one accumulator) is kept as written.  The
// compiler's hazard recogniser does not look inside asm: the first MFMA of a chain takes the literal 0 as its C operand (no
// compiler-written accumulator is read), and mma_layer ends with s_nop 7 before the VALU reads the results.
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int R, bool FIRST, bool VNOP = true, int NWAS = 1, int NWVS = 1>
__device__ __forceinline__ void mfma_w(pvf4& acc, float av, const float (&wa)[NWAS], const float (&wv)[NWVS]) {
  constexpr int NWA = NWAS;
#ifdef HA_SIMT_EMU
  // v_mfma_f32_4x4x1_16b_f32 on the host emulator: 16 independent blocks of four lanes; in block b the lane 4 b + j gets, for the rows i = 0..3,
  // D[i] (+)= A(lane 4 b + i) * B(lane 4 b + j)
  const float bw = R < NWA ? wa[R < NWA ? R : 0] : wv[R < NWA ? 0 : R - NWA];
  const int l = (int)(threadIdx.x & 63);
  pvf4 d = FIRST ? pvf4{0.f, 0.f, 0.f, 0.f} : acc;
  for (int i = 0; i < 4; ++i) d[i] = fmaf(__shfl(av, (l & ~3) | i), bw, d[i]);
  acc = d;
#else
  if constexpr (R < NWA) {
    if constexpr (FIRST) asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, 0" : "=&" HA_ACC(acc) : "v"(av), "a"(wa[R]));
    else asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+" HA_ACC(acc) : "v"(av), "a"(wa[R]));
  } else if constexpr (!VNOP) {
    // (kernels whose VGPR-class weights demonstrably never leave their registers -- tools/isa_census_pipe.py / tests/test_build.py hold
    // the pipelined kernels to zero v_accvgpr traffic -- need no wait states in front of the MFMA)
    if constexpr (FIRST) asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, 0" : "=&" HA_ACC(acc) : "v"(av), "v"(wv[R - NWA]));
    else asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+" HA_ACC(acc) : "v"(av), "v"(wv[R - NWA]));
  } else {
    // (a VGPR-class weight may be parked in an AGPR by the register allocator and copied back right in front of the asm: that copy
    // is a VALU write the MFMA must not read within two wait states, and the hazard recogniser does not look inside the asm)
    if constexpr (FIRST) asm volatile("s_nop 1\n\tv_mfma_f32_4x4x1_16b_f32 %0, %1, %2, 0" : "=&" HA_ACC(acc) : "v"(av), "v"(wv[R - NWA]));
    else asm volatile("s_nop 1\n\tv_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+" HA_ACC(acc) : "v"(av), "v"(wv[R - NWA]));
  }
#endif
}
template <int NC_MAIN, int NZ, int NCG, int ROFF, int FIRST, int NWAS, int NWVS>
__device__ __forceinline__ void mma_batch(const float (&av)[MB], const float (&wa)[NWAS], const float (&wv)[NWVS], pvf4 (&acc)[NCG][8 / NCG]) {
  constexpr int NACC = 8 / NCG;
  constexpr int NCZ = NZ;
  // (compile-time chunk index: the weight register and the accumulator are template arguments of mfma_w)
  auto body = [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    constexpr int c = FIRST + i;
    if constexpr (c < NC_MAIN + NCZ) {
      if constexpr (NCG == 2) {
        mfma_w<ROFF + c * 2 + 0, (c < NACC)>(acc[0][c % NACC], av[i], wa, wv);
        mfma_w<ROFF + c * 2 + 1, (c < NACC)>(acc[1][c % NACC], av[i], wa, wv);
      } else {
        mfma_w<ROFF + c, (c < NACC)>(acc[0][c % NACC], av[i], wa, wv);
      }
    }
  };
  static_for(body, std::make_integer_sequence<int, MB>{});
}
template <int NC_MAIN, int NZ, int NCG, int ROFF, int FIRST, int NWAS, int NWVS>
struct MmaSteps {
  static __device__ __forceinline__ void run(const float* xs, const float* zs, const float (&wa)[NWAS], const float (&wv)[NWVS], int lane,
                                             float (&cur)[MB], pvf4 (&acc)[NCG][8 / NCG]) {
    if constexpr (FIRST < NC_MAIN + NZ) {
      float nxt[MB];
      if constexpr (FIRST + MB < NC_MAIN + NZ) load_a<NC_MAIN, NZ, FIRST + MB>(xs, zs, lane, nxt);
      HA_SCHED_FENCE();
      mma_batch<NC_MAIN, NZ, NCG, ROFF, FIRST>(cur, wa, wv, acc);
      HA_SCHED_FENCE();
      MmaSteps<NC_MAIN, NZ, NCG, ROFF, FIRST + MB, NWAS, NWVS>::run(xs, zs, wa, wv, lane, nxt, acc);
    }
  }
};
// result: sums[4 g + i] = the lane's partial (its k-block) of column group g, row i
// (NC_MAIN chunks from xs, then NZ chunks from zs; when fewer chunks than chains exist only the first NC_MAIN + NZ chains are used)
template <int NC_MAIN, int NZ, int NCG, int ROFF, int NWAS, int NWVS>
__device__ __forceinline__ void mma_layer(const float* xs, const float* zs, const float (&wa)[NWAS], const float (&wv)[NWVS], int lane,
                                          float (&sums)[4 * NCG]) {
  constexpr int NACC = (8 / NCG) < (NC_MAIN + NZ) ? (8 / NCG) : (NC_MAIN + NZ);
  static_assert(NCG == 1 || NC_MAIN + NZ >= 4, "two column groups: four chains each");
  pvf4 acc[NCG][8 / NCG];
  float first[MB];
  load_a<NC_MAIN, NZ, 0>(xs, zs, lane, first);
  MmaSteps<NC_MAIN, NZ, NCG, ROFF, 0, NWAS, NWVS>::run(xs, zs, wa, wv, lane, first, acc);
  // MFMA results -> VALU reads: a hazard the compiler cannot see (the MFMAs are opaque asm to it).  The wait is tied to every
  // accumulator ("+a"), otherwise the scheduler may place an accumulator read between the last MFMA and a free-standing s_nop.
#ifndef HA_SIMT_EMU
  if constexpr (NCG == 2)
    asm volatile("s_nop 7" : "+" HA_ACC(acc[0][0]), "+" HA_ACC(acc[0][1]), "+" HA_ACC(acc[0][2]), "+" HA_ACC(acc[0][3]), "+" HA_ACC(acc[1][0]), "+" HA_ACC(acc[1][1]), "+" HA_ACC(acc[1][2]), "+" HA_ACC(acc[1][3]));
  else if constexpr (NACC == 8)
    asm volatile("s_nop 7" : "+" HA_ACC(acc[0][0]), "+" HA_ACC(acc[0][1]), "+" HA_ACC(acc[0][2]), "+" HA_ACC(acc[0][3]), "+" HA_ACC(acc[0][4]), "+" HA_ACC(acc[0][5]), "+" HA_ACC(acc[0][6]), "+" HA_ACC(acc[0][7]));
  else
    static_assert(NCG == 2 || NACC == 8, "accumulator fence");
#endif
#pragma unroll
  for (int g = 0; g < NCG; ++g) {
#pragma unroll
    for (int k = 1; k < NACC; ++k) acc[g][0] += acc[g][k];
#pragma unroll
    for (int i = 0; i < 4; ++i) sums[4 * g + i] = acc[g][0][i];
  }
}

// publishes the wave's NCG column groups (columns col0 + 4 g + j) of layer-output `off`.  The k-block partials are summed with the
// reduce-scatter of lane_reduce.h, which leaves lane (half h, row parity p, column j, k-block 0) with
//   NCG = 2: column group h, rows 2 p and 2 p + 1  -> ONE 16-byte store of two {value, tag} granules,
//   NCG = 1: row 2 h + p                            -> ONE 8-byte granule;
// the same lanes write the plain pre-activation slab [channel quads][32 rows][4] for the adjoint / prior.
// ht (or null): a second copy of the pre-activations in the team's own layout [channel][4 rows] (16 contiguous bytes per channel: the
// persistent adjoint reads its h with one coalesced 16-byte load per channel instead of four scattered 4-byte loads from the slab)
// GW: the consumer's slot mapping (xslot)
template <int NCG, bool SC1, int GW>
__device__ __forceinline__ void publish(const float (&sums)[4 * NCG], float bias_lane, int col0, unsigned char* team_xch, __amdgpu_buffer_rsrc_t rs,
                                        unsigned off, unsigned tag, float* slab, int row0, int lane, float* ht = nullptr) {
  const int h = lane >> 5, p = (lane >> 4) & 1, j = lane & 3;
  const bool storer = (lane & 12) == 0;
  if constexpr (NCG == 2) {
    float o[2];
    lr::block_sum8(sums, o);
    if (storer) {
      const int col = col0 + 4 * h + j;
      const float v0 = o[0] + bias_lane, v1 = o[1] + bias_lane;
      const puv4 gr = {as_u(v0), tag, as_u(v1), tag};
      const unsigned goff = off + (unsigned)xslot<GW>(col) * 32u + (unsigned)p * 16u;
      if (SC1) __builtin_amdgcn_raw_buffer_store_b128(gr, rs, goff, 0, 16);
      else *reinterpret_cast<puv4*>(team_xch + goff) = gr;
      if (slab) {
        float* sp = slab + pq(col) + (size_t)(row0 + 2 * p) * 4;
        sp[0] = v0;
        sp[4] = v1;
      }
      if (ht) {
        *reinterpret_cast<pvf2*>(ht + (size_t)col * 4 + 2 * p) = pvf2{v0, v1};
      }
    }
  } else {
    const float t = lr::block_sum4(sums);
    if (storer) {
      const int col = col0 + j, row = 2 * h + p;
      const float v0 = t + bias_lane;
      typedef unsigned puv2 __attribute__((ext_vector_type(2)));
      const puv2 gr = {as_u(v0), tag};
      const unsigned goff = off + (unsigned)xslot<GW>(col) * 32u + (unsigned)row * 8u;
      if (SC1) __builtin_amdgcn_raw_buffer_store_b64(gr, rs, goff, 0, 16);
      else *reinterpret_cast<puv2*>(team_xch + goff) = gr;
      if (slab) slab[pq(col) + (size_t)(row0 + row) * 4] = v0;
      if (ht) ht[(size_t)col * 4 + row] = v0;
    }
  }
}


// The 3x3 helpers of common.h with contraction allowed (the library is built -ffp-contract=off; the glue chains of this file are
// instruction-issue bound on one or two waves per CU, and a*b + c*d + e*f as mul + 2 fma is 3 instructions instead of 5 -- and rounds
// once less).  Only the persistent kernels' glue uses them.
namespace pg {
__device__ __forceinline__ void mat3_mul(const float A[9], const float B[9], float C[9]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void mat3_tmul(const float A[9], const float B[9], float C[9]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void mat3_mult(const float A[9], const float B[9], float C[9]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1] + A[i * 3 + 2] * B[j * 3 + 2];
}
__device__ __forceinline__ void mat3_vec(const float A[9], const float v[3], float o[3]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
__device__ __forceinline__ void mat3_tvec(const float A[9], const float v[3], float o[3]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
}  // namespace pg

// rodrigues() of common.h with ONE argument reduction for sine and cosine and the norm / its reciprocal from v_sqrt_f32 / v_rcp_f32
// (1 ulp each, arguments >= 1e-8: no denormals).  The glue is a dependent chain on one lane per sequence: the IEEE sqrtf and division
// are ~10 dependent instructions each, and the unit axis they produce differs from the correctly rounded one by an ulp or two.
#if defined(HA_GLUE_IEEE) || defined(HA_SIMT_EMU)      // (A/B builds and the host emulator: correctly rounded division / square root in the glue chains)
__device__ __forceinline__ float hw_rcp(float x) { return 1.0f / x; }
__device__ __forceinline__ float hw_sqrt(float x) { return sqrtf(x); }
#else
__device__ __forceinline__ float hw_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float hw_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
#endif
__device__ __forceinline__ void rodrigues_sc(const float r[3], float R[9]) {
#pragma clang fp contract(fast)
  const float ux = r[0] + 1e-8f, uy = r[1] + 1e-8f, uz = r[2] + 1e-8f;
  const float t = hw_sqrt(ux * ux + uy * uy + uz * uz);
  const float it = hw_rcp(t);
  const float nx = r[0] * it, ny = r[1] * it, nz = r[2] * it;
  float s, c;
  sincosf(t, &s, &c);
  const float c1 = 1.0f - c;
  const float nn = nx * nx + ny * ny + nz * nz;
  R[0] = 1.0f + c1 * (nx * nx - nn);
  R[1] = -s * nz + c1 * (nx * ny);
  R[2] = s * ny + c1 * (nx * nz);
  R[3] = s * nz + c1 * (nx * ny);
  R[4] = 1.0f + c1 * (ny * ny - nn);
  R[5] = -s * nx + c1 * (ny * nz);
  R[6] = -s * ny + c1 * (nx * nz);
  R[7] = s * nx + c1 * (ny * nz);
  R[8] = 1.0f + c1 * (nz * nz - nn);
}
// w2a_fwd() of rot_math.h (heading alignment, transforms.py:17-42); returns the heading angle.  The rotation is rodrigues() of the
// axis-angle (0, 0, az) written out: nx = ny = 0 exactly, so only the z-rotation block is computed (same operations on the entries
// that are not identically 0 / 1).
__device__ __forceinline__ float w2a_sc(const float pR[9], float W[9]) {
#pragma clang fp contract(fast)
  const float rx = -pR[0], ry = -pR[3];
  const float nrm = hw_sqrt(rx * rx + ry * ry);
  const float u = rx * hw_rcp(nrm + 1e-6f);
  const float angle = acosf(fminf(fmaxf(u, -1.0f), 1.0f));
  const float sg = -ry * hw_rcp(fabsf(ry) + 1e-6f);
  const float az = sg * angle;
  const float e = 1e-8f, uz = az + 1e-8f;
  const float t = hw_sqrt(e * e + e * e + uz * uz);
  const float nz = az * hw_rcp(t);
  float s, c;
  sincosf(t, &s, &c);
  const float c1 = 1.0f - c;
  const float nn = nz * nz;
  W[0] = 1.0f + c1 * (0.f - nn);
  W[1] = -s * nz;
  W[2] = 0.f;
  W[3] = s * nz;
  W[4] = W[0];
  W[5] = 0.f;
  W[6] = 0.f;
  W[7] = 0.f;
  W[8] = 1.0f;
  return angle;
}

// the XCD this block runs on (HW_REG_XCC_ID) and the host-mapped error word; host emulator: one team, blocks 0 .. 31 on "XCD" 0
#ifdef HA_SIMT_EMU
__device__ __forceinline__ unsigned xcc_id() { return (unsigned)(blockIdx.x / TEAM_CUS) & 7u; }
__device__ __forceinline__ void err_store(unsigned* err, unsigned v) { std::atomic_ref<unsigned>(*err).store(v); }
#else
__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u; }
__device__ __forceinline__ void err_store(unsigned* err, unsigned v) { __hip_atomic_store(err, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
#endif

template <bool SC1>
__global__ __launch_bounds__(256) HA_WAVES_PER_EU(1, 1) void rollout_persist_fwd_kernel(PersistArgs a) {
  HA_DYN_LDS(smem);
  float* xs0 = smem + L_XS0;
  float* xs1 = smem + L_XS1;
  float* xs2 = smem + L_XS2;
  float* xs3 = smem + L_XS3;
  float* zs = smem + L_ZS;
  float* sX = smem + L_SX;
  float* sRAW = smem + L_SRAW;
  float* sW = smem + L_SW;
  float* sG = smem + L_SG;
  float* sGL = smem + L_SGL;
  float* sT2J = smem + L_T2J;
  volatile int* misc = reinterpret_cast<volatile int*>(smem + L_MISC);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;

  // ---- team formation: a block belongs to the XCD it runs on ------------------------------------------------------------
  if (tid == 0) {
    const unsigned xcc = xcc_id();
    unsigned* cnt = reinterpret_cast<unsigned*>(a.xch);
    misc[0] = (int)xcc;
    misc[1] = (int)atomicAdd(cnt + xcc, 1u);
    misc[2] = 0;
  }
  __syncthreads();
  // (block-uniform values out of LDS: readfirstlane keeps them -- and the buffer descriptor built from them -- in SGPRs)
  const int team = __builtin_amdgcn_readfirstlane(misc[0]), m = __builtin_amdgcn_readfirstlane(misc[1]);
  if (m >= TEAM_CUS) {        // more than 32 blocks on this XCD: another XCD is short of one, its team will time out
    if (tid == 0) err_store(a.err, 0x100u | (unsigned)team);
    return;
  }
  if (a.S == 0) return;       // residency / placement probe
  if (a.inject && team == 0 && m == 3) return;
  const int g = m * 4 + wave;                 // wave of the team
  const int row0 = team * ROWS;               // the team's sequences
  unsigned char* team_xch = a.xch + XCH_HDR + (size_t)team * TEAM_BYTES;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(team_xch, 0, TEAM_BYTES, 0x00020000);
  const bool writer = m == 0;                 // member 0 writes the per-sequence results (world states, state slabs)

  // ---- resident weights -------------------------------------------------------------------------------------------------
  float wa[NWA], wv[NREG - NWA > 0 ? NREG - NWA : 1];
  {
    const float* wp = a.Wreg + (size_t)g * NREG * 64 + lane;
#pragma unroll
    for (int r = 0; r < NWA; ++r) wa[r] = wp[(size_t)r * 64];
#pragma unroll
    for (int r = NWA; r < NREG; ++r) wv[r - NWA] = wp[(size_t)r * 64];
  }
  // bias of the column this lane publishes (publish(): two-group layers lane (h, j) -> column 4 h + j of the wave's eight)
  const int j4 = lane & 3, h4 = 4 * (lane >> 5);
  const float b0 = a.bias[0][8 * g + h4 + j4], b1 = a.bias[1][8 * g + h4 + j4], b2 = a.bias[2][4 * g + j4];
  const float b3 = g < L3_WAVES ? a.bias[3][4 * g + j4] : 0.f;
  float* sGb1 = smem + L_GB;
  float* sGb2 = sGb1 + 4 * P_H0;
  float* sGb3 = sGb2 + 4 * P_H1;
  gb_fill<true>(sGb1, a.gamma[0], a.beta[0], P_H0, tid);
  gb_fill<true>(sGb2, a.gamma[1], a.beta[1], P_H1, tid);
  gb_fill<true>(sGb3, a.gamma[2], a.beta[2], P_H2, tid);

  // ---- initial state: x_0 (row-major copy for the glue, [channel][row] copy as the A operand), z_0, world transform ---------
  for (int e = tid; e < ROWS * P_XPAD; e += 256) {
    const int i = e / P_XPAD, c = e - i * P_XPAD, r = row0 + i;
    const float v = (c < P_DIN && r < a.B) ? a.past_in0[(size_t)r * P_DIN + c] : 0.f;
    sX[e] = v;
    xs0[c * 4 + i] = v;
    if (writer && c < P_DINP) a.xT[pq(c) + (size_t)r * 4] = v;
  }
  // The second state buffer: the glue writes channels 0 .. 338 of the buffer it fills, copy_out sends channels 0 .. 339 (P_DINP) of it to
  // the state slab the prior network reads.  LDS is not cleared between kernels: without this fill the pad channel of every odd step was
  // whatever the CU's previous kernel left there (round 5: NaN gradients on a fresh box -- 0 x NaN in the prior's first layer -- where the
  // builder's box held small finite numbers; tools/nan_hunt.py --cu-poison reproduces it anywhere).  The glue record's unused tail likewise.
  for (int e = tid; e < ROWS * P_XPAD; e += 256) sX[ROWS * P_XPAD + e] = 0.f;
  if (tid < ROWS * 32) sGL[tid] = 0.f;
  const int zi = tid / P_ZD, zc = tid - zi * P_ZD;          // thread <-> (row, latent channel) for tid < 192
  const bool zlive = tid < ROWS * P_ZD && row0 + zi < a.B;
  if (tid < ROWS * P_ZD) zs[zc * 4 + zi] = zlive ? a.z_seq[((size_t)(row0 + zi) * a.S) * P_ZD + zc] : 0.f;
  // per-sequence constants / accumulated world transform of the team's rows in LDS: t2j = -(x0[207], x0[208], 0); G = I, gt = 0
  if (tid < ROWS) {
    const int r = row0 + tid;
    const bool live = r < a.B;
    float* Gs0 = sG + tid * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) Gs0[i] = (i == 0 || i == 4 || i == 8) ? 1.f : 0.f;
    sT2J[tid * 4 + 0] = live ? -a.past_in0[(size_t)r * P_DIN + 207] : 0.f;
    sT2J[tid * 4 + 1] = live ? -a.past_in0[(size_t)r * P_DIN + 208] : 0.f;
    sT2J[tid * 4 + 2] = 0.f;
    sT2J[tid * 4 + 3] = 0.f;
    if (writer) {
      float* Gs = a.steps + a.off_G + (size_t)r * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) Gs[i] = Gs0[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) a.t2j[(size_t)r * 3 + c] = sT2J[tid * 4 + c];
    }
  }

  // The results of step t (world states of the team's sequences, the next state slab, the accumulated transforms) sit in every CU's
  // LDS after the glue (every CU computes them): CU m writes elements [m, m + 1) x COPY_PER_CU of the team's record, one coalesced
  // store per thread.  Element order: world [row][348] | state slab quads [quad][row][4] | transforms [row][12] | glue record [row][32].
  auto copy_out = [&](int t) {
    const float* sXn = sX + ((t + 1) & 1) * ROWS * P_XPAD;        // written by the glue of step t
    const float* sGn = sG + ((t + 1) & 1) * L_GSZ;
    if (tid < COPY_PER_CU) {
      const int e = m * COPY_PER_CU + tid;
      if (e < COPY_WORLD) {
        const int i = e / P_STATE, c = e - i * P_STATE;
        if (row0 + i < a.B) a.world[((size_t)(row0 + i) * a.S + t) * P_STATE + c] = sW[i * P_XPAD + c];
      } else if (e < COPY_WORLD + COPY_XT) {
        const int e2 = e - COPY_WORLD, q = e2 >> 4, i = (e2 >> 2) & 3, k = e2 & 3;
        a.xT[(size_t)(t + 1) * P_DINP * 32 + (size_t)q * 128 + (size_t)(row0 + i) * 4 + k] = sXn[i * P_XPAD + 4 * q + k];
      } else if (e < COPY_WORLD + COPY_XT + COPY_G) {
        const int e3 = e - COPY_WORLD - COPY_XT;
        a.steps[(size_t)(t + 1) * a.per_step + a.off_G + (size_t)row0 * 12 + e3] = sGn[e3];
      } else if (e < COPY_TOTAL) {
        const int e4 = e - COPY_WORLD - COPY_XT - COPY_G;
        a.steps[(size_t)t * a.per_step + a.off_gl + (size_t)row0 * 32 + e4] = sGL[e4];
      }
    }
  };
  // phase-2 task of this lane (wave = sequence): lanes 0..21 joint positions, 22 root translation, 23..44 joint velocities, 45 / 46 root
  // linear / angular velocity, 47..49 the columns of the predicted root rotation (source: the glue record; stride 3)
  int p2_a, p2_b, p2_dst;
  float p2_fA, p2_fT;
  bool p2_col;
  {
    int ra, xa;
    if (lane < 22) { ra = 75 + 3 * lane; xa = 207 + 3 * lane; }
    else if (lane == 22) { ra = 0; xa = 0; }
    else if (lane < 45) { ra = 141 + 3 * (lane - 23); xa = 273 + 3 * (lane - 23); }
    else if (lane == 45) { ra = 3; xa = 3; }
    else { ra = 9; xa = 15; }
    p2_col = lane >= 47;
    p2_fA = lane <= 22 ? 1.f : 0.f;
    p2_fT = lane < 22 ? 1.f : 0.f;
    p2_a = p2_col ? L_ZERO : L_SRAW + wave * P_RAWPAD + ra;
    p2_b = p2_col ? L_SGL + wave * 32 + 9 + (lane - 47) : L_SX + wave * P_XPAD + xa;
    p2_dst = p2_col ? 6 + (lane - 47) : xa;
  }
  if (tid < 16) smem[L_ZERO + tid] = 0.f;
  // What step t leaves for later (nothing of the next step's input depends on it): the world-frame columns of the root rotation
  // G^T R_root (lanes 50..52 of the sequence's wave) and the transform update G' = G W, gt' (lane 53).  They run in the shadow of the
  // NEXT step's layer-1 sweep (after its layer-0 publish); copy_out follows one barrier later.
  auto deferred = [&](int tp) {
    if (lane >= 50 && lane < 54) {
      const int i = wave;
      const float* X = sX + (tp & 1) * ROWS * P_XPAD + i * P_XPAD;
      const float* RW = sRAW + i * P_RAWPAD;
      const float* GL = sGL + i * 32;
      const float* Gp = sG + (tp & 1) * L_GSZ + i * 12;
      float G[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) G[e] = Gp[e];
      if (lane < 53) {
        const int kk = lane - 50;
        float v[3], o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = GL[9 + 3 * c + kk];
        pg::mat3_tvec(G, v, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) sW[i * P_XPAD + 6 + 3 * c + kk] = o[c];
      } else {
        // wtrans = G^T ptrans - gt ; G' = G W ; gt' = (-wtrans.x, -wtrans.y, 0)
        float W[9], GW[9], ptr[3], wtr[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) W[e] = GL[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) ptr[c] = RW[c] + X[c];
        pg::mat3_tvec(G, ptr, wtr);
        pg::mat3_mul(G, W, GW);
        pvf4* gs = reinterpret_cast<pvf4*>(sG + ((tp + 1) & 1) * L_GSZ + i * 12);
        gs[0] = pvf4{GW[0], GW[1], GW[2], GW[3]};
        gs[1] = pvf4{GW[4], GW[5], GW[6], GW[7]};
        gs[2] = pvf4{GW[8], -(wtr[0] - Gp[9]), -(wtr[1] - Gp[10]), 0.f};
      }
    }
  };
#ifdef HA_PERSIST_TIMING
  const bool pt_on = team == 0 && (m == 5 || m == 0) && tid == 0;
  const int pt_slot = m == 0 ? 1 : 0;
#endif
  bool fail = false;
  for (int t = 0; t < a.S; ++t) {
    const unsigned tag = 4u * (unsigned)t;
    float* sp = a.steps + (size_t)t * a.per_step;
    // latent of the next step: requested behind the first sweep of the step (in front of it, the sweep's in-order vmcnt wait would include
    // this load's latency), written to LDS in the glue phase
    float z_next = 0.f;
    __syncthreads();                                   // xs0 / zs of this step are complete
    PT(0);
    // ---- layer 0: [x_t | z_t] (raw) -> 1024 ---------------------------------------------------------------------------
    {
      float acc[8];
      mma_layer<NC0, NCZ, 2, R0>(xs0, zs, wa, wv, lane, acc);
      PT(1);
      publish<2, SC1, 64>(acc, b0, 8 * g, team_xch, rs, ACT_OFF0, tag + 1, a.hidden_slabs ? sp + a.off_dec[0] : nullptr, row0, lane, sp + a.off_ht[0] + (size_t)team * P_H0 * 4);
      PT(2);
    }
    if (t > 0) deferred(t - 1);       // (in the shadow of the layer-1 sweep)
    // ---- layer 1 ----------------------------------------------------------------------------------------------------------
    if (!gather_norm<4, 64, 3>(rs, ACT_OFF0, tag + 1, sGb1, xs1, tid, m == 1 ? sp + a.off_gn[0] : nullptr, row0 PT_PASS)) fail = true;
    if (zlive && t + 1 < a.S) z_next = a.z_seq[((size_t)(row0 + zi) * a.S + (t + 1)) * P_ZD + zc];
    PT(4);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PT(5);
    {
      float acc[8];
      mma_layer<NC1, NCZ, 2, R1>(xs1, zs, wa, wv, lane, acc);
      PT(6);
      publish<2, SC1, 64>(acc, b1, 8 * g, team_xch, rs, ACT_OFF1, tag + 2, a.hidden_slabs ? sp + a.off_dec[1] : nullptr, row0, lane, sp + a.off_ht[1] + (size_t)team * P_H1 * 4);
      PT(7);
    }
    if (t > 0) copy_out(t - 1);       // the previous step's results leave in the shadow of the layer-2 sweep (stores only; the deferred
                                      // tasks' LDS writes are one barrier back)
    // ---- layer 2 ----------------------------------------------------------------------------------------------------------
    if (!gather_norm<4, 64, 8>(rs, ACT_OFF1, tag + 2, sGb2, xs2, tid, m == 2 ? sp + a.off_gn[1] : nullptr, row0 PT_PASS)) fail = true;
    PT(9);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PT(10);
    {
      float acc[4];
      mma_layer<NC2, NCZ, 1, R2>(xs2, zs, wa, wv, lane, acc);
      PT(11);
      publish<1, SC1, 32>(acc, b2, 4 * g, team_xch, rs, ACT_OFF2, tag + 3, a.hidden_slabs ? sp + a.off_dec[2] : nullptr, row0, lane, sp + a.off_ht[2] + (size_t)team * P_H2 * 4);
      PT(12);
    }
    // ---- layer 3 (GroupNorm groups of 32) -------------------------------------------------------------------------------
    if (!gather_norm<2, 32, 13>(rs, ACT_OFF2, tag + 3, sGb3, xs3, tid, m == 3 ? sp + a.off_gn[2] : nullptr, row0 PT_PASS)) fail = true;
    PT(14);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PT(15);
    if (g < L3_WAVES) {       // (wave-uniform)
      float acc[4];
      mma_layer<NC3, NCZ, 1, R3>(xs3, zs, wa, wv, lane, acc);
      PT(16);
      publish<1, SC1, 0>(acc, b3, 4 * g, team_xch, rs, ACT_OFF3, tag + 4, sp + a.off_dec[3], row0, lane);
      PT(17);
    }
    // ---- glue: decoder output of the 4 rows -> every CU --------------------------------------------------------------------
    {
      float x[1][4];
      if (!sweep<1>(rs, ACT_OFF3, tag + 4, P_RAW, tid, x)) fail = true;
      if (tid < P_RAW) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sRAW[i * P_RAWPAD + tid] = x[0][i];
      }
    }
    PT(18);
    if (fail) misc[2] = 1;
    __syncthreads();                                   // also: every wave of this CU is past its layer-3 reads of zs / xs3
    if (misc[2]) break;
    PT(19);
    if (tid < ROWS * P_ZD) zs[zc * 4 + zi] = z_next;
    // ---- glue (humor_model.py:870-1001 after the decoder): the CU's four waves work on the team's four sequences side by side ----
    // Round 3 ran one wave per sequence through the whole chain (rotations -> heading alignment -> both frame changes -> ~90 LDS
    // stores per lane): ~1 100 instructions per wave and step, 5.5-6 k cycles.  Now the chain is cut where its dependences are:
    //   phase 1, waves 0-1: the body rotations -- lane (sequence, joint): R = rodrigues(delta) R_in for the 21 body joints;
    //            wave 2: the four root rotations, the heading alignment W = world2aligned(R_root) and the glue record (the long chain);
    //            wave 3: everything that needs only the OLD accumulated transform -- the world-frame positions / velocities
    //            G^T (p + t2j) - t2j - gt, G^T v and the contact logits;
    //   phase 2, wave = sequence: the frame change by W, one 3-vector task per lane (22 joint positions, root translation, 22 joint
    //            velocities, root velocities, the three columns of R_root -> W R_root), three lanes for the world-frame columns
    //            G^T R_root and one for the transform update G' = G W.
    // States and transforms are double-buffered in LDS (read t & 1, write the other), so no wave overwrites what another still reads.
    {
      const float* Xc = sX + (t & 1) * ROWS * P_XPAD;
      float* Xn = sX + ((t + 1) & 1) * ROWS * P_XPAD;
      const float* Gc = sG + (t & 1) * L_GSZ;
      float* Gn = sG + ((t + 1) & 1) * L_GSZ;
      if (wave < 3) {
        // waves 0, 1: the 21 body rotations of sequences (0, 1) / (2, 3), lane = (sequence, joint); wave 2: the four roots (lanes 0..3),
        // the one long dependent chain of the step, on a wave of its own
        const int i = wave < 2 ? 2 * wave + (lane >> 5) : (lane & 3), jj = wave < 2 ? (lane & 31) : 21;
        const bool root = wave == 2;
        if (root ? lane < ROWS : jj < 21) {
          const float* X = Xc + i * P_XPAD;
          const float* RW = sRAW + i * P_RAWPAD;
          const int aoff = root ? 6 : 12 + 3 * jj, roff = root ? 6 : 18 + 9 * jj;
          float aa[3], Rin[9], dR[9], pR[9];
#pragma unroll
          for (int c = 0; c < 3; ++c) aa[c] = RW[aoff + c];
#pragma unroll
          for (int k = 0; k < 9; ++k) Rin[k] = X[roff + k];
          rodrigues_sc(aa, dR);
          pg::mat3_mul(dR, Rin, pR);
          if (!root) {         // (wave-uniform)
            float* d1 = Xn + i * P_XPAD + roff;
            float* d2 = xs0 + roff * 4 + i;
            float* d3 = sW + i * P_XPAD + roff;
#pragma unroll
            for (int k = 0; k < 9; ++k) { d1[k] = pR[k]; d2[4 * k] = pR[k]; d3[k] = pR[k]; }
          } else {
            // record for phase 2 and for the adjoint of this step: heading alignment W, predicted root rotation pR = dR Rin, dR, heading angle
            float Wm[9];
            const float angle = w2a_sc(pR, Wm);
            float* gl = sGL + i * 32;
#pragma unroll
            for (int k = 0; k < 9; ++k) { gl[k] = Wm[k]; gl[9 + k] = pR[k]; gl[18 + k] = dR[k]; }
            gl[27] = angle;
          }
        }
      } else {
#pragma clang fp contract(fast)
        // wave 3: everything that needs only the OLD accumulated transform, two sequences per pass
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int i = 2 * pass + (lane >> 5), k = lane & 31;
          const float* X = Xc + i * P_XPAD;
          const float* RW = sRAW + i * P_RAWPAD;
          float* Wn = sW + i * P_XPAD;
          float G[9], gt[3], t2[3];
#pragma unroll
          for (int e = 0; e < 9; ++e) G[e] = Gc[i * 12 + e];
#pragma unroll
          for (int c = 0; c < 3; ++c) { gt[c] = Gc[i * 12 + 9 + c]; t2[c] = sT2J[i * 4 + c]; }
          // position-like: joints (k < 22): G^T (p + t2j) - t2j - gt ; root translation (k = 22): G^T p - gt ; lanes 23..31: contact logits
          if (k <= 22) {
            const int ra = k < 22 ? 75 + 3 * k : 0, xa = k < 22 ? 207 + 3 * k : 0;
            const float fT = k < 22 ? 1.f : 0.f;
            float q[3], o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = (RW[ra + c] + X[xa + c]) + fT * t2[c];
            pg::mat3_tvec(G, q, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) Wn[xa + c] = (o[c] - fT * t2[c]) - gt[c];
          } else {
            Wn[339 + k - 23] = RW[207 + k - 23];
          }
          // velocity-like: joint velocities (k < 22), root linear (22) and angular (23) velocity: G^T v
          if (k <= 23) {
            const int ra = k < 22 ? 141 + 3 * k : (k == 22 ? 3 : 9), xa = k < 22 ? 273 + 3 * k : (k == 22 ? 3 : 15);
            float q[3], o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = RW[ra + c] + X[xa + c];
            pg::mat3_tvec(G, q, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) Wn[xa + c] = o[c];
          }
        }
      }
      PT(20);
      __syncthreads();
      PT(21);
      if (lane < 50) {
#pragma clang fp contract(fast)
        // phase 2, wave = sequence: q = (source) + fA (-ptrans.xy) + fT t2j ; o = W q - fT t2j, one 3-vector task per lane (the lane's
        // constants -- LDS offsets, strides, flags -- are set up once before the step loop: p2_*)
        const int i = wave;
        const float* X = Xc + i * P_XPAD;
        const float* RW = sRAW + i * P_RAWPAD;
        const float* GL = sGL + i * 32;
        const float* A = smem + p2_a;
        const float* Bq = smem + p2_b + (p2_col ? 0 : (t & 1) * ROWS * P_XPAD);
        const int sb = p2_col ? 3 : 1, sa = p2_col ? 0 : 1;
        float M[9], q[3], o[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) M[e] = GL[e];
        const float ad0 = -(RW[0] + X[0]), ad1 = -(RW[1] + X[1]);          // - predicted root translation (x, y)
        const float t20 = sT2J[i * 4], t21 = sT2J[i * 4 + 1];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = A[c * sa] + Bq[c * sb];
        q[0] = (q[0] + p2_fA * ad0) + p2_fT * t20;
        q[1] = (q[1] + p2_fA * ad1) + p2_fT * t21;
        pg::mat3_vec(M, q, o);
        o[0] -= p2_fT * t20;
        o[1] -= p2_fT * t21;
        float* d1 = Xn + i * P_XPAD + p2_dst;
        float* d2 = xs0 + p2_dst * 4 + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) { d1[c * sb] = o[c]; d2[4 * c * sb] = o[c]; }
      }
    }
    PT(22);
  }
  __syncthreads();
  if (!misc[2]) {
    deferred(a.S - 1);
    __syncthreads();
    copy_out(a.S - 1);
  }
  if (misc[2]) {
    // A team that did not complete (a bounded wait ran out): the launch is asynchronous -- inside a captured hipGraph no entry point sees
    // the error word before the results are consumed -- so the results themselves say so: every output row of this team becomes NaN
    // (every CU that noticed fills all of it: the failure may BE a missing member), and the loss and gradients computed from them with
    // it.  The host-mapped word tells the optimiser why.
    const float nanv = as_f(0x7fc00000u);
    for (size_t e = tid; e < (size_t)ROWS * a.S * P_STATE; e += 256) {
      const int i = (int)(e / ((size_t)a.S * P_STATE));
      if (row0 + i < a.B) a.world[(size_t)row0 * a.S * P_STATE + e] = nanv;
    }
    if (tid == 0) err_store(a.err, 0x200u | (unsigned)team);
  }
}


// a (x) b accumulated into M (3x3): M[i][k] += a_i b_k
__device__ __forceinline__ void outer_acc3(float M[9], const float a[3], const float b[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) M[i * 3 + k] = fmaf(a[i], b[k], M[i * 3 + k]);
}

// a dL/dz task (or layer 0's LDS-resident K tail): CH chunks of the activation adjoint against LDS-resident weight vectors.  All
// operands are read first, then the MFMAs run on min(CH, 8) independent accumulators.
template <int CH>
__device__ __forceinline__ void dz_mma(const float* xs, const float* wl, int lane, float (&acc)[4]) {
  constexpr int NCH = CH < 8 ? CH : 8;
  float av[CH], bv[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) { av[i] = xs[64 * i + lane]; bv[i] = wl[64 * i + lane]; }
  pvf4 c[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) c[k] = pvf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < CH; ++i) c[i % NCH] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[i], bv[i], c[i % NCH], 0, 0, 0);
#pragma unroll
  for (int k = 1; k < NCH; ++k) c[0] += c[k];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = c[0][i];
}
// one K-split partial of dL/dz (columns 4 cg .. 4 cg + 3 of the latent, the team's 4 rows) -> part[t][slot][row][48]
__device__ __forceinline__ void dz_store(const float (&acc)[4], float* part, int t, int slot, int cg, int row0, int lane) {
  const float v = lr::block_sum4(acc);
  if ((lane & 12) == 0) {
    const int row = 2 * (lane >> 5) + ((lane >> 4) & 1), j = lane & 3;
    part[(((size_t)t * DZ_SLOTS + slot) * 32 + row0 + row) * P_ZD + 4 * cg + j] = v;
  }
}


// ---------------------------------------------------------------------------------------------------
// Persistent adjoint: the reverse scan over the S steps as ONE launch, same teams / exchange as the forward.
// Per step t (S-1 .. 0) and team: total adjoint of x_{t+1} (own direct part + prior part + the layer-0 input gradient of step t+1
// from the team) -> glue adjoint (one wave per sequence) -> dL/d(decoder output) -> four transposed layer products with the
// GroupNorm/ReLU adjoints on the consumer side (statistics from the forward's stash), dL/dz as K-split partial products.
// ---------------------------------------------------------------------------------------------------
struct PersistBwdArgs {
  int B, S;
  const float* Wreg;        // [128 waves][NREG_B][64 lanes]
  const float* gamma[3];
  const float* beta[3];
  const float* g_world;     // [B][S][348] or null
  const float* gx_pri;      // [S][gxp_pad][32] or null: dL/dx_t through the prior, all steps
  int gxp_pad;
  const float* xT;
  const float* steps;
  size_t per_step, off_G, off_dec[4], off_gn[3], off_gl, off_ht[3];
  const float* t2j;
  float* g_past0;           // [B][339]
  float* dz_part;           // [S][DZ_SLOTS][32][48]
  unsigned char* xch;
  unsigned* err;
};

// Lanes of ONE wave handing data to each other through LDS.  The hardware executes a wave's LDS instructions in program order, but to the
// compiler two divergent regions (`if (lane == a) store` ... `if (lane == b) load`) are independent and it may emit them in either
// order (seen: the consumer region ahead of the producer region, NaNs).  wave_barrier is a convergent no-op the optimiser cannot move
// code across; the empty asm keeps memory accesses on their side of it.
__device__ __forceinline__ void wave_lds_order() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// rodrigues() / rodrigues_bwd() of common.h in two parts, so that the part that does not depend on the incoming gradient (norm, reciprocal, sine / cosine: the long
// dependent chain) can run early and on another wave: rod_prep() -> {n, s, c, 1/t}; rod_adj() = dL/dr from dL/dR.  Norm and
// reciprocal from v_sqrt_f32 / v_rcp_f32 as in the forward's rodrigues_sc.
struct RodPrep {
  float n[3], s, c, it;
};
__device__ __forceinline__ void rod_prep(const float r[3], RodPrep& p) {
#pragma clang fp contract(fast)
  const float ux = r[0] + 1e-8f, uy = r[1] + 1e-8f, uz = r[2] + 1e-8f;
  const float t = hw_sqrt(ux * ux + uy * uy + uz * uz);
  p.it = hw_rcp(t);
  p.n[0] = r[0] * p.it; p.n[1] = r[1] * p.it; p.n[2] = r[2] * p.it;
  sincosf(t, &p.s, &p.c);
}
__device__ __forceinline__ void rod_R(const RodPrep& p, float R[9]) {
#pragma clang fp contract(fast)
  const float nx = p.n[0], ny = p.n[1], nz = p.n[2], s = p.s, c1 = 1.0f - p.c;
  const float nn = nx * nx + ny * ny + nz * nz;
  R[0] = 1.0f + c1 * (nx * nx - nn);
  R[1] = -s * nz + c1 * (nx * ny);
  R[2] = s * ny + c1 * (nx * nz);
  R[3] = s * nz + c1 * (nx * ny);
  R[4] = 1.0f + c1 * (ny * ny - nn);
  R[5] = -s * nx + c1 * (ny * nz);
  R[6] = -s * ny + c1 * (nx * nz);
  R[7] = s * nx + c1 * (ny * nz);
  R[8] = 1.0f + c1 * (nz * nz - nn);
}
__device__ __forceinline__ void rod_adj(const RodPrep& p, const float r[3], const float gR[9], float gr[3]) {
#pragma clang fp contract(fast)
  const float nx = p.n[0], ny = p.n[1], nz = p.n[2], s = p.s, c = p.c, it = p.it, c1 = 1.0f - p.c;
  const float nn = nx * nx + ny * ny + nz * nz;
  const float gK_dot = -nz * gR[1] + ny * gR[2] + nz * gR[3] - nx * gR[5] - ny * gR[6] + nx * gR[7];
  const float tr = gR[0] + gR[4] + gR[8];
  const float nGn = nx * (gR[0] * nx + gR[1] * ny + gR[2] * nz) + ny * (gR[3] * nx + gR[4] * ny + gR[5] * nz) +
                    nz * (gR[6] * nx + gR[7] * ny + gR[8] * nz);
  const float gK2_dot = nGn - nn * tr;
  const float gt = c * gK_dot + s * gK2_dot;
  const float sx = (gR[0] + gR[0]) * nx + (gR[1] + gR[3]) * ny + (gR[2] + gR[6]) * nz;
  const float sy = (gR[3] + gR[1]) * nx + (gR[4] + gR[4]) * ny + (gR[5] + gR[7]) * nz;
  const float sz = (gR[6] + gR[2]) * nx + (gR[7] + gR[5]) * ny + (gR[8] + gR[8]) * nz;
  const float gnx = s * (gR[7] - gR[5]) + c1 * (sx - 2.0f * tr * nx);
  const float gny = s * (gR[2] - gR[6]) + c1 * (sy - 2.0f * tr * ny);
  const float gnz = s * (gR[3] - gR[1]) + c1 * (sz - 2.0f * tr * nz);
  const float gn_r = gnx * r[0] + gny * r[1] + gnz * r[2];
  const float k = (gt - gn_r * it * it) * it;
  gr[0] = gnx * it + k * (r[0] + 1e-8f);
  gr[1] = gny * it + k * (r[1] + 1e-8f);
  gr[2] = gnz * it + k * (r[2] + 1e-8f);
}
// the heading alignment's scalars from the glue record (pR[0], pR[3], angle): everything w2a_bwd needs besides dL/dW
struct HeadPrep {
  float rx, ry, nrm, u, xp, angle, s, az;
};
__device__ __forceinline__ void head_prep(float pR0, float pR3, float angle, HeadPrep& o) {
  o.rx = -pR0;
  o.ry = -pR3;
  o.nrm = hw_sqrt(o.rx * o.rx + o.ry * o.ry);
  o.u = o.rx * hw_rcp(o.nrm + 1e-6f);
  o.xp = fminf(fmaxf(o.u, -1.0f), 1.0f);
  o.angle = angle;
  o.s = -o.ry * hw_rcp(fabsf(o.ry) + 1e-6f);
  o.az = o.s * o.angle;
}
// w2a_bwd() of rot_math.h given the rotation set-up of (0, 0, az): dL/dpR[0], dL/dpR[3] from dL/dW
__device__ __forceinline__ void head_adj(const HeadPrep& o, const RodPrep& p, const float gW[9], float& g_p0, float& g_p3) {
#pragma clang fp contract(fast)
  const float aa[3] = {0.f, 0.f, o.az};
  float gaa[3];
  rod_adj(p, aa, gW, gaa);
  const float g_az = gaa[2];
  const float g_s = o.angle * g_az;
  const float g_angle = o.s * g_az;
  // (1 - u^2 = (ry^2 + eps (2 nrm + eps)) / d^2 without the cancellation of 1 - u u: see w2a_bwd)
  const float g_xp = -g_angle * (o.nrm + 1e-6f) * __builtin_amdgcn_rsqf(o.ry * o.ry + 1e-6f * (2.0f * o.nrm + 1e-6f));
  const float g_u = (o.u >= -1.0f && o.u <= 1.0f) ? g_xp : 0.f;
  const float id = hw_rcp(o.nrm + 1e-6f);
  float g_rx = g_u * id;
  float g_ry = 0.f;
  const float g_nrm = -g_u * o.rx * (id * id);
  if (o.nrm > 0.f) {
    const float inr = hw_rcp(o.nrm);
    g_rx += g_nrm * o.rx * inr;
    g_ry += g_nrm * o.ry * inr;
  }
  const float ar = fabsf(o.ry), da = ar + 1e-6f, ida = hw_rcp(da);
  const float sgn = o.ry > 0.f ? 1.f : (o.ry < 0.f ? -1.f : 0.f);
  const float ds = -(da - o.ry * sgn) * (ida * ida);
  g_ry += g_s * ds;
  g_p0 = -g_rx;
  g_p3 = -g_ry;
}


// consumer side of an activation adjoint: sweep dL/da (a = ReLU(GroupNorm(h))), the forward's h and statistics, GroupNorm/ReLU
// adjoint (gn_apply mode 3 of the launch chain: dh = rstd (dxh - mean(dxh) - xh mean(dxh xh))), dh to LDS as [channel][4 rows].
// The forward's pre-activations and statistics come from HBM / the Infinity Cache (~2 us): they are requested one phase early
// (gnb_issue, before the previous layer's MFMAs) so that the sweep's loads do not queue behind them.
template <int NQ>
struct GnbRegs {
  pvf2 h[2 * NQ];             // the thread's row pair of its 2 NQ channels (xchan)
  pvf4 s;                     // (mean, rstd) of the two rows in the thread's group (one group per 16-lane row)
};
// ht: the team's copy of the pre-activations, [channel][4 rows]
template <int NQ, int GROUP>
__device__ __forceinline__ void gnb_issue(const float* ht, const float* stats, int row0, int tid, GnbRegs<NQ>& r) {
  const int hp = tid & 1;
#pragma unroll
  for (int k = 0; k < 2 * NQ; ++k) r.h[k] = *reinterpret_cast<const pvf2*>(ht + (size_t)xchan<GROUP>(tid, k) * 4 + 2 * hp);
  r.s = *reinterpret_cast<const pvf4*>(stats + ((size_t)(tid >> 4) * 32 + row0 + 2 * hp) * 2);
}
template <int NQ, int GROUP, int PTI = 0>
__device__ __forceinline__ bool gather_norm_bwd(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned tag, const float* gb_lds,
                                                const GnbRegs<NQ>& r, float* ds, int tid PTB_ARGS) {
  constexpr int NK = 2 * NQ;
  static_assert(GROUP == 8 * NK, "a 16-lane row holds one group");
  const float mean[2] = {r.s.x, r.s.z}, rstd[2] = {r.s.y, r.s.w};
  float xh[NK][2];
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int i = 0; i < 2; ++i) xh[k][i] = (r.h[k][i] - mean[i]) * rstd[i];
  float ga[NK][2];
  if (!sweep_pairs<NK>(rs, off, tag, tid, ga)) return false;
  PTB(PTI);
  const float inv_n = 1.0f / (float)GROUP;
  float dxh[NK][2], dx2[NK][2];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const pvf2 gb = gb_at<GROUP, false>(gb_lds, tid, k);
    const float gam = gb[0], bet = gb[1];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float y = xh[k][i] * gam + bet;
      dxh[k][i] = (y > 0.f ? ga[k][i] : 0.f) * gam;
      dx2[k][i] = dxh[k][i] * xh[k][i];
    }
  }
  // m[0..1] = sum of dxh, m[2..3] = sum of dxh xh over the group, per row
  // (scalar form: the packed-fp32 form of norm_pairs measured 1 % slower here -- the pairs have to be assembled with copies first)
  float m[4] = {sum_k<NK>(dxh, 0), sum_k<NK>(dxh, 1), sum_k<NK>(dx2, 0), sum_k<NK>(dx2, 1)};
  lr::parity_sum4(m);
  const int hp = tid & 1;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    pvf2 o;
#pragma unroll
    for (int i = 0; i < 2; ++i) o[i] = rstd[i] * (dxh[k][i] - m[i] * inv_n - xh[k][i] * (m[2 + i] * inv_n));
    *reinterpret_cast<pvf2*>(ds + (size_t)xchan<GROUP>(tid, k) * 4 + 2 * hp) = o;
  }
  return true;
}


template <bool SC1>
__global__ __launch_bounds__(256) HA_WAVES_PER_EU(1, 1) void rollout_persist_bwd_kernel(PersistBwdArgs a) {
  HA_DYN_LDS(smem);
  float* sD3 = smem + LB_D3;
  float* sD2 = smem + LB_D2;
  float* sD1 = smem + LB_D1;
  float* sD0 = smem + LB_D0;
  float* sGXN = smem + LB_GXN;
  float* sGXD = smem + LB_GXD;
  float* sCarry = smem + LB_CARRY;
  volatile int* misc = reinterpret_cast<volatile int*>(smem + LB_MISC);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;

  if (tid == 0) {
    const unsigned xcc = xcc_id();
    unsigned* cnt = reinterpret_cast<unsigned*>(a.xch);
    misc[0] = (int)xcc;
    misc[1] = (int)atomicAdd(cnt + xcc, 1u);
    misc[2] = 0;
  }
  __syncthreads();
  const int team = __builtin_amdgcn_readfirstlane(misc[0]), m = __builtin_amdgcn_readfirstlane(misc[1]);
  if (m >= TEAM_CUS) {
    if (tid == 0) err_store(a.err, 0x300u | (unsigned)team);
    return;
  }
  const int g = m * 4 + wave;
  const int row0 = team * ROWS;
  unsigned char* team_xch = a.xch + XCH_HDR + (size_t)team * TEAM_BYTES;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(team_xch, 0, TEAM_BYTES, 0x00020000);

  // ---- resident transposed weights ------------------------------------------------------------------------------------------
  float wa[NWA_B < NREG_B ? NWA_B : NREG_B], wv[NREG_B - NWA_B > 0 ? NREG_B - NWA_B : 1];
  float* sWz = smem + LB_WZ + wave * NLW * 64;
  {
    const float* wp = a.Wreg + (size_t)g * (NREG_B_ALL + BC0_LDS) * 64 + lane;
#pragma unroll
    for (int r = 0; r < NWA_B && r < NREG_B; ++r) wa[r] = wp[(size_t)r * 64];
#pragma unroll
    for (int r = NWA_B; r < NREG_B; ++r) wv[r - NWA_B] = wp[(size_t)r * 64];
#pragma unroll
    for (int r = 0; r < NLW; ++r) sWz[r * 64 + lane] = wp[(size_t)(NREG_B + r) * 64];
  }
  // GroupNorm affine of the three hidden activations in LDS (register budget: 292 weight registers per wave)
  float* sGb1 = smem + LB_GB;
  float* sGb2 = sGb1 + 2 * P_H0;
  float* sGb3 = sGb2 + 2 * P_H1;
  gb_fill<false>(sGb1, a.gamma[0], a.beta[0], P_H0, tid);
  gb_fill<false>(sGb2, a.gamma[1], a.beta[1], P_H1, tid);
  gb_fill<false>(sGb3, a.gamma[2], a.beta[2], P_H2, tid);

  // ---- per-step inputs: (channel quad, row) per thread, 16-byte loads, one step ahead ---------------------------------------
  // x_t (state slab), decoder output (slab 3), dL/dworld_t, glue record, accumulated transform, dL/dx_{t+1} through the prior
  const int pq_q = tid >> 2, pq_i = tid & 3;                  // first pass: quads 0..63; second pass: quads 64..127
  // two halves, each in four 16-byte registers: A = state, decoder output, glue record, transform (requested behind the dL/dx sweep at the
  // top of a step, live across the glue adjoint); B = dL/dworld and the prior part (requested behind the first layer sweep, live across the layer-2 product)
  pvf4 pf[4];
  const pvf4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto prefetch_a_issue = [&](int tp) {
#pragma unroll
    for (int k = 0; k < 4; ++k) pf[k] = zero4;
    const int r = row0 + pq_i;
    if (tp >= 0) {
      const float* sp = a.steps + (size_t)tp * a.per_step;
      const float* xs = a.xT + (size_t)tp * P_DINP * 32 + (size_t)r * 4;
      pf[0] = *reinterpret_cast<const pvf4*>(xs + (size_t)pq_q * 128);
      if (pq_q + 64 < P_DINP / 4) pf[1] = *reinterpret_cast<const pvf4*>(xs + (size_t)(pq_q + 64) * 128);
      if (pq_q < P_RAW / 4) pf[2] = *reinterpret_cast<const pvf4*>(sp + a.off_dec[3] + (size_t)pq_q * 128 + (size_t)r * 4);
      if (pq_q < 8) pf[3] = *reinterpret_cast<const pvf4*>(sp + a.off_gl + (size_t)r * 32 + 4 * pq_q);
      else if (pq_q < 11) pf[3] = *reinterpret_cast<const pvf4*>(sp + a.off_G + (size_t)r * 12 + 4 * (pq_q - 8));
    }
  };
  auto prefetch_a_store = [&](int tp) {
    float* b = smem + LB_PF + (tp & 1) * PF_SIZE;
    *reinterpret_cast<pvf4*>(b + PF_X + pq_i * P_XPAD + 4 * pq_q) = pf[0];
    if (pq_q + 64 < P_XPAD / 4) *reinterpret_cast<pvf4*>(b + PF_X + pq_i * P_XPAD + 4 * (pq_q + 64)) = pf[1];
    if (pq_q < P_RAWPAD / 4) *reinterpret_cast<pvf4*>(b + PF_RAW + pq_i * P_RAWPAD + 4 * pq_q) = pf[2];
    if (pq_q < 8) *reinterpret_cast<pvf4*>(b + PF_GL + pq_i * 32 + 4 * pq_q) = pf[3];
    else if (pq_q < 11) *reinterpret_cast<pvf4*>(b + PF_G + pq_i * 12 + 4 * (pq_q - 8)) = pf[3];
  };
  auto prefetch_b_issue = [&](int tp) {        // tp >= -1; the prior part belongs to step tp + 1
#pragma unroll
    for (int k = 0; k < 4; ++k) pf[k] = zero4;
    const int r = row0 + pq_i;
    if (tp >= 0 && a.g_world && r < a.B) {
      const float* gw = a.g_world + ((size_t)r * a.S + tp) * P_STATE;
      pf[0] = *reinterpret_cast<const pvf4*>(gw + 4 * pq_q);
      if (pq_q + 64 < P_STATE / 4) pf[1] = *reinterpret_cast<const pvf4*>(gw + 4 * (pq_q + 64));
    }
    if (a.gx_pri && tp + 1 < a.S) {
      const float* gp = a.gx_pri + (size_t)(tp + 1) * a.gxp_pad * 32 + (size_t)r * 4;
      pf[2] = *reinterpret_cast<const pvf4*>(gp + (size_t)pq_q * 128);
      if (pq_q + 64 < P_DINP / 4) pf[3] = *reinterpret_cast<const pvf4*>(gp + (size_t)(pq_q + 64) * 128);
    }
  };
  auto prefetch_b_store = [&](int tp) {
    float* b = smem + LB_PF + (tp & 1) * PF_SIZE;
    *reinterpret_cast<pvf4*>(b + PF_GW + pq_i * P_XPAD + 4 * pq_q) = pf[0];
    if (pq_q + 64 < P_XPAD / 4) *reinterpret_cast<pvf4*>(b + PF_GW + pq_i * P_XPAD + 4 * (pq_q + 64)) = pf[1];
    *reinterpret_cast<pvf4*>(b + PF_GXP + pq_i * P_XPAD + 4 * pq_q) = pf[2];
    if (pq_q + 64 < P_XPAD / 4) *reinterpret_cast<pvf4*>(b + PF_GXP + pq_i * P_XPAD + 4 * (pq_q + 64)) = pf[3];
  };

  // per-sequence carried adjoints of wave `wave`'s row (identical in every lane): dL/dG', dL/dgt', dL/dt2j so far
  // (kept in LDS between the steps, sCarry[row][16]: dL/dG' 9 | dL/dgt' 3 | dL/dt2j 3 -- and the row's t2j at [row][64 + ..])
  if (lane < 16) sCarry[wave * 16 + lane] = 0.f;
  if (tid < ROWS * 4) smem[LB_T2J + tid] = (tid & 3) < 3 ? a.t2j[(size_t)(row0 + (tid >> 2)) * 3 + (tid & 3)] : 0.f;
  if (tid < ROWS) smem[LB_PREP + tid * 24 + 22] = 0.f;          // the glue adjoint's hand-off flags (a step publishes t + 1 >= 1)
  for (int e = tid; e < ROWS * P_XPAD; e += 256) { sGXD[e] = 0.f; sGXN[e] = 0.f; }

  prefetch_a_issue(a.S - 1);
  prefetch_a_store(a.S - 1);
  prefetch_b_issue(a.S - 1);
  prefetch_b_store(a.S - 1);

#ifdef HA_PERSIST_TIMING
  const bool ptb_on = team == 0 && m == 5 && tid == 0;
#endif
  bool fail = false;
  for (int t = a.S - 1; t >= 0; --t) {
    const unsigned tag = 4u * (unsigned)(a.S - 1 - t);
    const float* sp = a.steps + (size_t)t * a.per_step;
    const float* cur = smem + LB_PF + (t & 1) * PF_SIZE;
    // ---- total adjoint of x_{t+1}: own direct part + prior part + the team's layer-0 input gradient of step t+1 ----------------
    __syncthreads();                                   // the prefetched buffer of this step and sGXD of step t+1 are complete
    PTB(0);
    {
      float gx[2][4];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) gx[q][i] = 0.f;
      if (t < a.S - 1 && !sweep<2>(rs, GX_OFF0, tag, P_XPAD, tid, gx)) fail = true;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = tid + 256 * q;
        if (c < P_XPAD) {
#pragma unroll
          for (int i = 0; i < 4; ++i) sGXN[i * P_XPAD + c] = sGXD[i * P_XPAD + c] + cur[PF_GXP + i * P_XPAD + c] + gx[q][i];
        }
      }
    }
    PTB(1);
    // the next step's state / decoder output / glue record: requested BEHIND the sweep (vmcnt counts in order: a sweep issued after these
    // loads waits for their HBM / Infinity-Cache latency too), written to LDS behind the glue adjoint (round 5: -0.8 % per roll-out)
    prefetch_a_issue(t - 1);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PTB(2);
    // ---- glue adjoint: the CU's four waves side by side (round 3: one wave per sequence, 9.2 k cycles) --------------------------
    //   waves 0-1, lane = (sequence, rotation): the 21 body-rotation adjoints of sequences (0, 1) / (2, 3), p = dR R_in, complete; in the
    //              same instruction stream the rotation SET-UPS (norm, reciprocal, sine / cosine) of the root rotation (lane 21) and of
    //              the heading rotation (lane 22); lanes 23..31 pass the contact logits on.  Lane 21 then waits (LDS flag, no barrier)
    //              for dL/dW and the dL/dpR columns and runs the one dependent chain of the step: heading-alignment adjoint ->
    //              root-rotation adjoint;
    //   waves 2-3, lane = (sequence, vector task): the 27 vector tasks (22 joints, root translation / velocities, the three columns of
    //              the predicted root rotation), branch-free (per-lane offsets, strides and 0 / 1 factors), in two halves: FIRST what the
    //              chain above needs -- the next-input frame change (dL/dW: 9 sums + the carried part) and the dL/dpR columns, published
    //              with a flag -- then the world-frame half (dL/dG, dL/dgt, dL/dwt, dL/dt2j: 18 sums), the carries and the outputs.
    //   Sums over the half-wave go through LDS: partials transposed [quantity][lane], lane q sums row q (fixed order) and OWNS total q
    //   (adds its element of the carried product, writes it where it is needed): a third of the instructions of the cross-lane form.
    PTC(0, 0);
    PTC(1, 0);
    int gi = 2 * (wave & 1) + (lane >> 5), gv = lane & 31;                // sequence of the team, rotation / vector task of this lane
    // (opaque to the optimiser: otherwise every lane-dependent LDS offset below is hoisted out of the step loop and lives in a VGPR for
    // the whole launch -- the register file holds the weights, and the allocator then starts copying weights around, tests/test_build.py)
    HA_OPAQUE2(gi, gv);
    {
      const float* X = cur + PF_X + gi * P_XPAD;
      const float* RW = cur + PF_RAW + gi * P_RAWPAD;
      const float* GWp = cur + PF_GW + gi * P_XPAD;
      const float* GL = cur + PF_GL + gi * 32;
      const float* Gp = cur + PF_G + gi * 12;
      const float* GXN = sGXN + gi * P_XPAD;
      float* GXD = sGXD + gi * P_XPAD;
      // hand-off flag of this sequence: plain LDS accesses (ds_read / ds_write) fenced by compiler barriers -- a `volatile int*` made from
      // the LDS array turns into FLAT accesses, which are not ordered with the wave's ds_write stream (measured: stale dL/dW on the consumer)
      float* flag = smem + LB_PREP + gi * 24 + 22;
      RodPrep rp_root;
      float aa_root[3] = {0.f, 0.f, 0.f};
      rp_root.n[0] = rp_root.n[1] = rp_root.n[2] = rp_root.s = rp_root.c = rp_root.it = 0.f;
      if (wave < 2) {
        if (gv < 23) {
          const bool body = gv < 21;
          float aa[3];
          HeadPrep hp;
          if (gv < 22) {
            const int ao = body ? 12 + 3 * gv : 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) aa[c] = RW[ao + c];
          } else {
            head_prep(GL[9], GL[12], GL[27], hp);
            aa[0] = 0.f; aa[1] = 0.f; aa[2] = hp.az;
          }
          RodPrep rp;
          rod_prep(aa, rp);
          PTC(0, 1);
          if (body) {
            const int ao = 12 + 3 * gv, ro = 18 + 9 * gv;
            float gp[9], Rin[9], gd[9], dRm[9], gRin[9], gaa[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) { Rin[i] = X[ro + i]; gp[i] = GWp[ro + i] + GXN[ro + i]; }
            pg::mat3_mult(gp, Rin, gd);            // dL/ddR = dL/dp Rin^T
            rod_adj(rp, aa, gd, gaa);
            rod_R(rp, dRm);
            pg::mat3_tmul(dRm, gp, gRin);          // dL/dRin = dR^T dL/dp
#pragma unroll
            for (int c = 0; c < 3; ++c) sD3[(ao + c) * 4 + gi] = gaa[c];
#pragma unroll
            for (int i = 0; i < 9; ++i) GXD[ro + i] = gRin[i];
          } else if (gv == 22) {
            float* pp = smem + LB_PREP + gi * 24;        // heading set-up -> lane 21 (same wave: LDS is in order)
            pp[0] = hp.rx; pp[1] = hp.ry; pp[2] = hp.nrm; pp[3] = hp.u; pp[4] = hp.xp; pp[5] = hp.angle; pp[6] = hp.s; pp[7] = hp.az;
            pp[8] = rp.n[0]; pp[9] = rp.n[1]; pp[10] = rp.n[2]; pp[11] = rp.s; pp[12] = rp.c; pp[13] = rp.it;
          }
          PTC(0, 2);
          if (gv == 21) { rp_root = rp; aa_root[0] = aa[0]; aa_root[1] = aa[1]; aa_root[2] = aa[2]; }
        } else {
          // lanes 23..31: the contact logits pass straight through; the padding channels of the operand stay zero
          const int k = gv - 23;
          sD3[(207 + k) * 4 + gi] = GWp[339 + k];
          if (k < P_RAWPAD - P_RAW) sD3[(P_RAW + k) * 4 + gi] = 0.f;
        }
      } else {
#pragma clang fp contract(fast)
        // ---- vector tasks, v = 0..26 (27..31 idle: all their factors are 0) ----------------------------------------------------
        const int v = gv;
        const bool isj = v < 22, isroot = v == 22, iscol = v >= 24 && v < 27;
        const int kc = v - 24;
        const int rp = isj ? 75 + 3 * v : 0, xp = isj ? 207 + 3 * v : 0;                      // position sources (raw, x)
        const int rv = isj ? 141 + 3 * v : (isroot ? 3 : 9);                                  // velocity source (raw)
        const int xv = isj ? 273 + 3 * v : (isroot ? 3 : (v == 23 ? 15 : 6 + kc));            // velocity channels (x; columns: stride 3)
        const int sv = iscol ? 3 : 1;
        const float fpos = v <= 22 ? 1.f : 0.f, ft2 = isj ? 1.f : 0.f, fact = v < 27 ? 1.f : 0.f, f22 = isroot ? 1.f : 0.f, fraw = iscol ? 0.f : 1.f;
        float W[9], G[9], t2j[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) { W[i] = GL[i]; G[i] = Gp[i]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) t2j[c] = ft2 * smem[LB_T2J + gi * 4 + c];
        const float* velB = iscol ? GL + 9 + kc : X + xv;
        float pos[3], vel[3], gwp[3], gwv[3], gxp[3], gxv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          pos[c] = RW[rp + c] + X[xp + c];
          vel[c] = fraw * RW[rv + c] + velB[c * sv];
          gwp[c] = fpos * GWp[xp + c];
          gxp[c] = fpos * GXN[xp + c];
          gwv[c] = fact * GWp[xv + c * sv];
          gxv[c] = fact * GXN[xv + c * sv];
        }
        gwp[0] -= f22 * sCarry[gi * 16 + 9];          // carried gt' = (-wtrans.x, -wtrans.y, 0)
        gwp[1] -= f22 * sCarry[gi * 16 + 10];
        const float wt0 = -(RW[0] + X[0]), wt1 = -(RW[1] + X[1]);           // - predicted root translation (x, y)
        float* red = smem + LB_D1 + ((wave - 2) * 2 + (lane >> 5)) * RED_BLOCK;
        float* mine = red + v;
        float* carry = sCarry + gi * 16;
        // ---- first half: next input  y = W (p + wt + tj) - tj ,  W v  ->  dL/dW, the W^T parts of dL/dp, dL/dv, dL/dwt, dL/dt2j ----
        float gpos[3], gvel[3], gwt[3], gt2[3];
        {
          float q[3], gW[9];
          q[0] = pos[0] + wt0 + t2j[0];
          q[1] = pos[1] + wt1 + t2j[1];
          q[2] = pos[2] + t2j[2];
          pg::mat3_tvec(W, gxp, gpos);
          pg::mat3_tvec(W, gxv, gvel);
#pragma unroll
          for (int c = 0; c < 3; ++c) { gwt[c] = gpos[c]; gt2[c] = ft2 * (gpos[c] - gxp[c]); }
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) gW[3 * i + k] = fmaf(gxp[i], q[k], gxv[i] * vel[k]);
          // the world-frame part of the velocity-type adjoint already here: lanes 24..26 hold dL/dpR columns the chain waits for
          float o[3];
          pg::mat3_vec(G, gwv, o);
#pragma unroll
          for (int c = 0; c < 3; ++c) gvel[c] += o[c];
          PTC(1, 1);
#pragma unroll
          for (int i = 0; i < 9; ++i) mine[i * RED_LD] = gW[i];
          wave_lds_order();
          if (v < 9) {
            const pvf4* row = reinterpret_cast<const pvf4*>(red + v * RED_LD);
            pvf4 acc = row[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) acc += row[k];
            // carried: G' = G W : dL/dW += G^T dL/dG' -- element 3 i + j = sum_k G[3 k + i] dG'[3 k + j]
            const int i = v / 3, j = v - 3 * i;
            const float cr = (Gp[i] * carry[j] + Gp[3 + i] * carry[3 + j]) + Gp[6 + i] * carry[6 + j];
            smem[LB_COL + gi * 24 + 12 + v] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + cr;
          }
          if (iscol) {
#pragma unroll
            for (int c = 0; c < 3; ++c) smem[LB_COL + gi * 24 + 3 * kc + c] = gvel[c];
          }
          wave_lds_order();          // dL/dW (lanes 0..8) and the columns (lanes 24..26) are stored before the flag (lane 0)
          if (v == 0) *flag = as_f((unsigned)(t + 1));          // (after the stores above in program order: LDS executes a wave's operations in order)
          PTC(1, 2);
        }
        // ---- second half: world  y = G^T (p + tj) - tj - gt ,  G^T v  ->  dL/dG, dL/dgt, the G parts of dL/dp, dL/dt2j -------------
        {
          float q[3], o[3], gG[9];
#pragma unroll
          for (int c = 0; c < 3; ++c) q[c] = pos[c] + t2j[c];
          pg::mat3_vec(G, gwp, o);
#pragma unroll
          for (int c = 0; c < 3; ++c) { gpos[c] += o[c]; gt2[c] += ft2 * (o[c] - gwp[c]); }
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) gG[3 * i + k] = fmaf(q[i], gwp[k], vel[i] * gwv[k]);
          wave_lds_order();        // (the first half's rows have been read)
#pragma unroll
          for (int i = 0; i < 9; ++i) mine[i * RED_LD] = gG[i];
#pragma unroll
          for (int c = 0; c < 3; ++c) { mine[(9 + c) * RED_LD] = -gwp[c]; mine[(12 + c) * RED_LD] = gwt[c]; mine[(15 + c) * RED_LD] = gt2[c]; }
          wave_lds_order();
          PTC(1, 3);
          float tot = 0.f;
          if (v < 18) {
            const pvf4* row = reinterpret_cast<const pvf4*>(red + v * RED_LD);
            pvf4 acc = row[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) acc += row[k];
            tot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            red[27 * RED_LD + v] = tot;
          }
          // owner lanes: 0..8 dL/dG (+ dL/dG' W^T, element 3 i + j = sum_k dG'[3 i + k] W[3 j + k]) -> carry; 9..11 dL/dgt -> carry;
          // 12..14 dL/dwt (lane 22 reads it back); 15..17 dL/dt2j, accumulated over the steps
          float r = tot;
          if (v < 9) {
            const int i = v / 3, j = v - 3 * i;
            r = tot + ((carry[3 * i] * GL[3 * j] + carry[3 * i + 1] * GL[3 * j + 1]) + carry[3 * i + 2] * GL[3 * j + 2]);
          }
          wave_lds_order();          // every lane has read the old carry and the totals are stored
          if (v < 12) carry[v] = r;
          else if (v >= 15 && v < 18) carry[12 + v - 15] += r;
          // root translation: wt = (-ptrans.x, -ptrans.y, 0)
          wave_lds_order();
          gpos[0] -= f22 * red[27 * RED_LD + 12];
          gpos[1] -= f22 * red[27 * RED_LD + 13];
          PTC(1, 4);
          // outputs of the vector tasks: dL/d(decoder output) (A operand of the transposed last layer, [channel][row]) and the direct
          // part of dL/dx_t
          if (v <= 23) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              sD3[(rv + c) * 4 + gi] = gvel[c];
              GXD[xv + c] = gvel[c];
            }
            if (v <= 22) {
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                sD3[(rp + c) * 4 + gi] = gpos[c];
                GXD[xp + c] = gpos[c];
              }
            }
          }
          PTC(1, 5);
        }
      }
      wave_lds_order();          // lane 22's heading set-up is in LDS before lane 21 reads it
      if (wave < 2 && gv == 21) {
#pragma clang fp contract(fast)
        // ---- the chain: wait for dL/dW and the dL/dpR columns of this sequence (waves 2-3, first half) ----
        for (int spins = 0; spins < SPIN_LIMIT; ++spins) {
          asm volatile("" ::: "memory");
          if (as_u(*flag) == (unsigned)(t + 1)) break;
          __builtin_amdgcn_s_sleep(1);
        }
        asm volatile("" ::: "memory");
        // heading alignment W = world2aligned(pR): dL/dpR[0], dL/dpR[3]
        float g0, g3;
        {
          const float* pp = smem + LB_PREP + gi * 24;
          HeadPrep h2;
          h2.rx = pp[0]; h2.ry = pp[1]; h2.nrm = pp[2]; h2.u = pp[3]; h2.xp = pp[4]; h2.angle = pp[5]; h2.s = pp[6]; h2.az = pp[7];
          RodPrep rw;
          rw.n[0] = pp[8]; rw.n[1] = pp[9]; rw.n[2] = pp[10]; rw.s = pp[11]; rw.c = pp[12]; rw.it = pp[13];
          float gW[9];
#pragma unroll
          for (int i = 0; i < 9; ++i) gW[i] = smem[LB_COL + gi * 24 + 12 + i];
          head_adj(h2, rw, gW, g0, g3);
        }
        // root rotation p = dR Rin: dL/dp = the three column adjoints (+ the heading alignment's part)
        float gp[9], Rin[9], gd[9], gRin[9], gaa[3];
        const float* col = smem + LB_COL + gi * 24;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          Rin[i] = X[6 + i];
          gp[i] = col[3 * (i % 3) + i / 3];
        }
        gp[0] += g0;
        gp[3] += g3;
        pg::mat3_mult(gp, Rin, gd);            // dL/ddR = dL/dp Rin^T
        rod_adj(rp_root, aa_root, gd, gaa);
        pg::mat3_tmul(GL + 18, gp, gRin);      // dL/dRin = dR^T dL/dp (dR from the forward's glue record)
#pragma unroll
        for (int c = 0; c < 3; ++c) sD3[(6 + c) * 4 + gi] = gaa[c];
#pragma unroll
        for (int i = 0; i < 9; ++i) GXD[6 + i] = gRin[i];
      }
    }
    PTC(0, 3);
    PTB(3);
    prefetch_a_store(t - 1);
    __syncthreads();
    PTB(4);
    // ---- transposed layer 3: dL/d(decoder output) [216] -> dL/da3 [512] (+ dz) ------------------------------------------------
    GnbRegs<2> gr2;
    gnb_issue<2, 32>(sp + a.off_ht[2] + (size_t)team * P_H2 * 4, sp + a.off_gn[2], row0, tid, gr2);
    {
      float acc[4];
      mma_layer<BC3, 0, 1, BR3>(sD3, sD3, wa, wv, lane, acc);
      PTB(5);
      publish<1, SC1, 32>(acc, 0.f, 4 * g, team_xch, rs, GA_OFF3, tag + 1, nullptr, row0, lane);
      if (g < DZ3_WAVES) {
        float accz[4];
        dz_mma<DZ3_CH>(sD3 + 64 * DZ3_CH * (g % (BC3 / DZ3_CH)), sWz + (BRZ3 - BRZ0) * 64, lane, accz);
        dz_store(accz, a.dz_part, t, DZ_S3 + g % (BC3 / DZ3_CH), g / (BC3 / DZ3_CH), row0, lane);
      }
    }
    // ---- layer 2 ------------------------------------------------------------------------------------------------------------
    PTB(6);
    if (!gather_norm_bwd<2, 32, 7>(rs, GA_OFF3, tag + 1, sGb3, gr2, sD2, tid PTB_PASS)) fail = true;
    prefetch_b_issue(t - 1);          // (dL/dworld and the prior's dL/dx of the next step: behind the sweep, stored behind the layer-2 product)
    PTB(8);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PTB(9);
    GnbRegs<4> gr1;
    gnb_issue<4, 64>(sp + a.off_ht[1] + (size_t)team * P_H1 * 4, sp + a.off_gn[1], row0, tid, gr1);
    {
      float acc[8];
      mma_layer<BC2, 0, 2, BR2>(sD2, sD2, wa, wv, lane, acc);
      PTB(10);
      publish<2, SC1, 64>(acc, 0.f, 8 * g, team_xch, rs, GA_OFF2, tag + 2, nullptr, row0, lane);
      if (g < DZ2_WAVES) {
        float accz[4];
        dz_mma<DZ2_CH>(sD2 + 64 * DZ2_CH * (g % (BC2 / DZ2_CH)), sWz + (BRZ2 - BRZ0) * 64, lane, accz);
        dz_store(accz, a.dz_part, t, DZ_S2 + g % (BC2 / DZ2_CH), g / (BC2 / DZ2_CH), row0, lane);
      }
    }
    prefetch_b_store(t - 1);
    // ---- layer 1 ------------------------------------------------------------------------------------------------------------
    PTB(11);
    if (!gather_norm_bwd<4, 64, 12>(rs, GA_OFF2, tag + 2, sGb2, gr1, sD1, tid PTB_PASS)) fail = true;
    PTB(13);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PTB(14);
    GnbRegs<4> gr0;
    gnb_issue<4, 64>(sp + a.off_ht[0] + (size_t)team * P_H0 * 4, sp + a.off_gn[0], row0, tid, gr0);
    {
      float acc[8];
      mma_layer<BC1, 0, 2, BR1>(sD1, sD1, wa, wv, lane, acc);
      PTB(15);
      publish<2, SC1, 64>(acc, 0.f, 8 * g, team_xch, rs, GA_OFF1, tag + 3, nullptr, row0, lane);
      if (g < DZ1_WAVES) {
        float accz[4];
        dz_mma<DZ1_CH>(sD1 + 64 * DZ1_CH * (g % (BC1 / DZ1_CH)), sWz + (BRZ1 - BRZ0) * 64, lane, accz);
        dz_store(accz, a.dz_part, t, DZ_S1 + g % (BC1 / DZ1_CH), g / (BC1 / DZ1_CH), row0, lane);
      }
    }
    // ---- layer 0 ------------------------------------------------------------------------------------------------------------
    PTB(16);
    if (!gather_norm_bwd<4, 64, 17>(rs, GA_OFF1, tag + 3, sGb1, gr0, sD0, tid PTB_PASS)) fail = true;
    PTB(18);
    if (fail) misc[2] = 1;
    __syncthreads();
    if (misc[2]) break;
    PTB(19);
    {
      float acc[4];
      if (g < L0T_WAVES) {
        float tail[4];
        mma_layer<BC0_REG, 0, 1, BR0>(sD0, sD0, wa, wv, lane, acc);
        dz_mma<BC0_LDS>(sD0 + 64 * BC0_REG, sWz + NDZ * 64, lane, tail);        // the LDS-resident tail of K
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += tail[i];
      } else { acc[0] = acc[1] = acc[2] = acc[3] = 0.f; }
      PTB(20);
      if (g < P_XPAD / 4) publish<1, SC1, 0>(acc, 0.f, 4 * g, team_xch, rs, GX_OFF0, tag + 4, nullptr, row0, lane);     // (waves 85..87: the zero padding)
      if (g < DZ0_WAVES) {
        float accz[4];
        dz_mma<DZ0_CH>(sD0 + 64 * DZ0_CH * (g % (BC0 / DZ0_CH)), sWz, lane, accz);
        dz_store(accz, a.dz_part, t, DZ_S0 + g % (BC0 / DZ0_CH), g / (BC0 / DZ0_CH), row0, lane);
      }
    }
    PTB(21);
  }
  // ---- dL/dpast_in0 = total adjoint of x_0 (the t2j = -(x0[207], x0[208], 0) dependence included) -------------------------------
  __syncthreads();
  if (!misc[2]) {
    float gx[2][4];
    const float* cur = smem + LB_PF + 1 * PF_SIZE;          // buffer of "step -1": only its prior part (step 0) is populated
    if (!sweep<2>(rs, GX_OFF0, 4u * (unsigned)a.S, P_XPAD, tid, gx)) misc[2] = 1;
    __syncthreads();
    if (!misc[2] && m == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = tid + 256 * q;
        if (c < P_DIN) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float vsum = sGXD[i * P_XPAD + c] + cur[PF_GXP + i * P_XPAD + c] + gx[q][i];
            if (c == 207) vsum -= sCarry[i * 16 + 12];
            if (c == 208) vsum -= sCarry[i * 16 + 13];
            if (row0 + i < a.B) a.g_past0[(size_t)(row0 + i) * P_DIN + c] = vsum;
          }
        }
      }
    }
  }
  if (misc[2]) {
    // (as in the forward: the failed team's gradients become NaN -- dL/dpast_in0 directly, dL/dz through its partial products)
    const float nanv = as_f(0x7fc00000u);
    for (int e = tid; e < ROWS * P_DIN; e += 256) {
      const int i = e / P_DIN;
      if (row0 + i < a.B) a.g_past0[(size_t)row0 * P_DIN + e] = nanv;
    }
    for (size_t e = tid; e < (size_t)a.S * ROWS * P_ZD; e += 256) {
      const int tt = (int)(e / (ROWS * P_ZD)), r = (int)(e % (ROWS * P_ZD));
      a.dz_part[(((size_t)tt * DZ_SLOTS) * 32 + row0) * P_ZD + r] = nanv;          // slot 0 of every step
    }
    if (tid == 0) err_store(a.err, 0x400u | (unsigned)team);
  }
}


// g_z[b][t][c] = sum of the DZ_SLOTS partial products, fixed order
// (the body is shared with ha_fit_pre_backward, which can run it as a block role: turn_dev.h)
static_assert(DZ_SLOTS == TURN_DZ_SLOTS && P_ZD == TURN_ZD, "turn_dev.h restates the shape of the dL/dz partials");
__global__ void dz_reduce_kernel(const float* __restrict__ part, float* __restrict__ g_z, const float* __restrict__ g_z_add, int B, int S) {
  dz_reduce_elem(part, g_z, g_z_add, B, S, blockIdx.x * blockDim.x + threadIdx.x);
}

#include "rollout_pipe.inc"

#ifdef HA_PERSIST_TIMING
}  // namespace ha
extern "C" int ha_debug_persist_timing(unsigned long long* out /* [2][8][24] */) {
  HA_CHECK_HIP(hipDeviceSynchronize());
  HA_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(ha::g_pts), sizeof(unsigned long long) * 2 * 8 * 24));
  return HA_OK;
}
extern "C" int ha_debug_persist_spins(unsigned* out /* [8] */, int reset) {
  HA_CHECK_HIP(hipDeviceSynchronize());
  std::vector<unsigned> h(1024 * 8);
  HA_CHECK_HIP(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(ha::g_spin_hist), sizeof(unsigned) * 8 * 1024));
  for (int b = 0; b < 8; ++b) out[b] = 0;
  for (int w = 0; w < 1024; ++w)
    for (int b = 0; b < 8; ++b) out[b] += h[w * 8 + b];
  if (reset) {
    std::fill(h.begin(), h.end(), 0u);
    HA_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ha::g_spin_hist), h.data(), sizeof(unsigned) * 8 * 1024));
  }
  return HA_OK;
}
extern "C" int ha_debug_persist_timing_glue(unsigned long long* out /* [2][8][8] */) {
  HA_CHECK_HIP(hipDeviceSynchronize());
  HA_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(ha::g_ptc), sizeof(unsigned long long) * 2 * 8 * 8));
  return HA_OK;
}
extern "C" int ha_debug_pipe_timing(unsigned long long* out /* [2][4][4][8][12] */) {
  HA_CHECK_HIP(hipDeviceSynchronize());
  HA_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(ha::g_ppt), sizeof(unsigned long long) * 2 * 4 * 4 * 8 * 12));
  return HA_OK;
}
extern "C" int ha_debug_persist_timing_bwd(unsigned long long* out /* [8][24] */) {
  HA_CHECK_HIP(hipDeviceSynchronize());
  HA_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(ha::g_ptb), sizeof(unsigned long long) * 8 * 24));
  return HA_OK;
}
namespace ha {
#endif

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
template <typename T>
static int p_upload(T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  HA_CHECK_HIP(hipMalloc((void**)dst, src.size() * sizeof(T)));
  HA_CHECK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return HA_OK;
}

void persist_destroy(PersistNet* p) {
  if (!p) return;
#ifndef HA_SIMT_EMU
  DeviceGuard guard(p->device);
  if (p->Wreg) (void)hipFree(p->Wreg);
  if (p->Wreg_b) (void)hipFree(p->Wreg_b);
  if (p->Wreg_pf) (void)hipFree(p->Wreg_pf);
  if (p->Wreg_pb) (void)hipFree(p->Wreg_pb);
  for (float* q : p->bias)
    if (q) (void)hipFree(q);
  for (float* q : p->gamma)
    if (q) (void)hipFree(q);
  for (float* q : p->beta)
    if (q) (void)hipFree(q);
  if (p->err_host) (void)hipHostFree(p->err_host);
#endif
  delete p;
}

bool persist_usable(PersistNet* p) {
  if (!p || p->disabled) return false;
  if (p->err_host && *reinterpret_cast<volatile unsigned*>(p->err_host) != 0) p->disabled = true;   // sticky: reported by an earlier launch
  return !p->disabled;
}

long long persist_launches(PersistNet* p) { return p ? p->launches : 0; }
long long persist_launches_bwd(PersistNet* p) { return p ? p->launches_bwd : 0; }

// A persistent launch runs asynchronously: a failure (its bounded waits ran out, e.g. because another process's kernel held part of
// the chip) is only known to the host later.  The first entry point called after that returns an error ONCE -- the results of the
// failed call are invalid and the caller must know -- and from then on the launch chain serves this network.
bool persist_take_failure(PersistNet* p) {
  if (!p || p->reported || !p->err_host || *reinterpret_cast<volatile unsigned*>(p->err_host) == 0) return false;
  p->reported = true;
  p->disabled = true;
  return true;
}

// The caller has read the error word itself (ha_humor_persist_status) and handled the failure: no entry point needs to return it again.
void persist_ack_failure(PersistNet* p) {
  if (!p || !p->err_host || *reinterpret_cast<volatile unsigned*>(p->err_host) == 0) return;
  p->reported = true;
  p->disabled = true;
}

unsigned persist_error_word(PersistNet* p) { return (p && p->err_host) ? *reinterpret_cast<volatile unsigned*>(p->err_host) : 0u; }

// Pipelined adjoint: register c * NCGW + cg = K chunk c (forward output channels 16 c .. 16 c + 15 of the layer) of column group cg (forward
// input columns) of the role's transposed layer; behind them the wave's LDS-resident dL/dz vectors.  (Shared with the emulator test hook.)
static void pack_pipe_backward(const float* const* w, std::vector<float>& wq) {
  const int Kin[4] = {P_DIN + P_ZD, P_H0 + P_ZD, P_H1 + P_ZD, P_H2 + P_ZD}, Cmain[4] = {P_DIN, P_H0, P_H1, P_H2}, Nout[4] = {P_H0, P_H1, P_H2, P_RAW};
  auto W = [&](int l, int k, int col) -> float { return (k >= 0 && k < Nout[l] && col >= 0 && col < Kin[l]) ? w[l][(size_t)k * Kin[l] + col] : 0.f; };
  const size_t stride = (size_t)(QB_NREG + QB_NLW) * 64;
  for (int g = 0; g < NWAVES_TEAM; ++g) {
    const int m = g / 4;
    if (m >= PRG_M0 && m < PR1_M0) continue;       // the glue CU holds no weights
    const int l = m < PRG_M0 ? 0 : (m < PR2_M0 ? 1 : (m < PR3_M0 ? 2 : 3));
    const int m0[4] = {PR0_M0, PR1_M0, PR2_M0, PR3_M0}, ncgw[4] = {QB0_CG, QB1_CG, QB2_CG, QB3_CG}, nch[4] = {BC0, BC1, BC2, BC3};
    const int gw = g - 4 * m0[l];
    for (int ln = 0; ln < 64; ++ln) {
      const int b = ln >> 2, j = ln & 3;
      float* dst = wq.data() + (size_t)g * stride + ln;
      for (int c = 0; c < nch[l]; ++c)
        for (int cg = 0; cg < ncgw[l]; ++cg) {
          const int col = 4 * (ncgw[l] * gw + cg) + j;
          dst[(size_t)(c * ncgw[l] + cg) * 64] = col < Cmain[l] ? W(l, 16 * c + b, col) : 0.f;
        }
      float* dz = dst + (size_t)QB_NREG * 64;
      if (l == 3 && gw < 6) {
        for (int k = 0; k < 2; ++k)
          for (int i = 0; i < BC3; ++i) dz[(size_t)(k * BC3 + i) * 64] = W(3, 16 * i + b, Cmain[3] + 4 * (2 * gw + k) + j);
      } else if (l == 2 && gw < 24) {
        for (int i = 0; i < 16; ++i) dz[(size_t)i * 64] = W(2, 16 * (16 * (gw % 2) + i) + b, Cmain[2] + 4 * (gw / 2) + j);
      } else if (l == 1 && gw < 48) {
        for (int i = 0; i < 16; ++i) dz[(size_t)i * 64] = W(1, 16 * (16 * (gw % 4) + i) + b, Cmain[1] + 4 * (gw / 4) + j);
      } else if (l == 0) {
        const int zks = gw >> 2, zc0 = 3 * (gw & 3);
        for (int k = 0; k < 3; ++k)
          for (int i = 0; i < QZ0_CH; ++i) {
            const int c = QZ0_CH * zks + i;      // (the 65th chunk of the last K fifth does not exist: zero vector)
            dz[(size_t)(k * QZ0_CH + i) * 64] = c < BC0 ? W(0, 16 * c + b, Cmain[0] + 4 * (zc0 + k) + j) : 0.f;
          }
      }
    }
  }
}

// Pipelined forward: wave g = 4 m + w of a team belongs to the role of CU m; register c * NCGW + cg = K chunk c of column group cg of the role's
// layer.  (Shared with the emulator test hook ha_emu_pipe_layer.)
static void pack_pipe_forward(const float* const* w, std::vector<float>& wp) {
  const int Kin[4] = {P_DIN + P_ZD, P_H0 + P_ZD, P_H1 + P_ZD, P_H2 + P_ZD}, Cmain[4] = {P_DIN, P_H0, P_H1, P_H2};
  const int NCm[4] = {NC0, NC1, NC2, NC3}, Nout[4] = {P_H0, P_H1, P_H2, P_RAW};
  for (int g = 0; g < NWAVES_TEAM; ++g) {
    const int m = g / 4;
    if (m >= PRG_M0 && m < PR1_M0) continue;             // (the glue CU holds no weights)
    const int l = m < PR1_M0 ? 0 : (m < PR2_M0 ? 1 : (m < PR3_M0 ? 2 : 3));
    const int m0[4] = {PR0_M0, PR1_M0, PR2_M0, PR3_M0}, ncgw[4] = {PF0_CG, PF1_CG, PF2_CG, PF3_CG};
    const int gw = g - 4 * m0[l];
    for (int c = 0; c < NCm[l] + NCZ; ++c)
      for (int cg = 0; cg < ncgw[l]; ++cg)
        for (int ln = 0; ln < 64; ++ln) {
          const int b = ln >> 2, j = ln & 3;
          const int col = 4 * (ncgw[l] * gw + cg) + j;
          int k;
          if (c < NCm[l]) { k = 16 * c + b; if (k >= Cmain[l]) k = -1; }
          else k = Cmain[l] + 16 * (c - NCm[l]) + b;
          float v = 0.f;
          if (col < Nout[l] && k >= 0) v = w[l][(size_t)col * Kin[l] + k];
          wp[((size_t)g * PF_NREG + c * ncgw[l] + cg) * 64 + ln] = v;
        }
  }
}

// Adjoint: B operand lane (b, j) of chunk c = W_l[forward output 16 c + b][forward input column]; per wave NREG_B_ALL registers (the four transposed
// products, then the dL/dz weights) + BC0_LDS LDS-resident chunks of layer 0.  (Shared with the emulator test hook ha_emu_persist_layer_t.)
static void pack_backward(const float* const* w, std::vector<float>& wb) {
  const int Kin[4] = {P_DIN + P_ZD, P_H0 + P_ZD, P_H1 + P_ZD, P_H2 + P_ZD}, Nout[4] = {P_H0, P_H1, P_H2, P_RAW};
  auto W = [&](int l, int k, int col) -> float { return (k < Nout[l] && col < Kin[l]) ? w[l][(size_t)k * Kin[l] + col] : 0.f; };
  for (int g = 0; g < NWAVES_TEAM; ++g)
    for (int ln = 0; ln < 64; ++ln) {
      const int b = ln >> 2, j = ln & 3;
      float* dst = wb.data() + (size_t)g * (NREG_B_ALL + BC0_LDS) * 64 + ln;
      auto put = [&](int reg, float v) { dst[(size_t)reg * 64] = v; };
      for (int c = 0; c < BC3; ++c) put(BR3 + c, 4 * g + j < P_H2 ? W(3, 16 * c + b, 4 * g + j) : 0.f);
      for (int c = 0; c < BC2; ++c)
        for (int cg = 0; cg < 2; ++cg) put(BR2 + c * 2 + cg, W(2, 16 * c + b, 8 * g + 4 * cg + j));
      for (int c = 0; c < BC1; ++c)
        for (int cg = 0; cg < 2; ++cg) put(BR1 + c * 2 + cg, W(1, 16 * c + b, 8 * g + 4 * cg + j));
      for (int c = 0; c < BC0; ++c)
        put(c < BC0_REG ? BR0 + c : NREG_B_ALL + (c - BC0_REG), (g < L0T_WAVES && 4 * g + j < P_DIN) ? W(0, 16 * c + b, 4 * g + j) : 0.f);
      if (g < DZ0_WAVES)
        for (int i = 0; i < DZ0_CH; ++i) put(BRZ0 + i, W(0, 16 * ((g % (BC0 / DZ0_CH)) * DZ0_CH + i) + b, P_DIN + 4 * (g / (BC0 / DZ0_CH)) + j));
      if (g < DZ1_WAVES)
        for (int i = 0; i < DZ1_CH; ++i) put(BRZ1 + i, W(1, 16 * ((g % (BC1 / DZ1_CH)) * DZ1_CH + i) + b, P_H0 + 4 * (g / (BC1 / DZ1_CH)) + j));
      if (g < DZ2_WAVES)
        for (int i = 0; i < DZ2_CH; ++i) put(BRZ2 + i, W(2, 16 * ((g % (BC2 / DZ2_CH)) * DZ2_CH + i) + b, P_H1 + 4 * (g / (BC2 / DZ2_CH)) + j));
      if (g < DZ3_WAVES)
        for (int i = 0; i < DZ3_CH; ++i) put(BRZ3 + i, W(3, 16 * ((g % (BC3 / DZ3_CH)) * DZ3_CH + i) + b, P_H2 + 4 * (g / (BC3 / DZ3_CH)) + j));
    }
}

// Register-stationary packing of forward layer l (weights [Nout][Kin], row-major): wave g of a team, register RO[l] + c NCG + cg, lane (b, j) =
// W[column (8 | 4) g + 4 cg + j][input 16 c + b] -- the B operand of the wave's c-th v_mfma_f32_4x4x1 of column group cg (main chunks first, then
// the latent skip's).  (Shared with the emulator test hook ha_emu_persist_layer: tests/test_rollout_emu.py.)
static void pack_forward_layer(int l, const float* Wl, std::vector<float>& wr) {
  const int Kin[4] = {P_DIN + P_ZD, P_H0 + P_ZD, P_H1 + P_ZD, P_H2 + P_ZD}, Cmain[4] = {P_DIN, P_H0, P_H1, P_H2};
  const int NCm[4] = {NC0, NC1, NC2, NC3}, NCGv[4] = {2, 2, 1, 1}, RO[4] = {R0, R1, R2, R3}, Nout[4] = {P_H0, P_H1, P_H2, P_RAW};
  for (int g = 0; g < NWAVES_TEAM; ++g)
    for (int c = 0; c < NCm[l] + NCZ; ++c)
      for (int cg = 0; cg < NCGv[l]; ++cg)
        for (int ln = 0; ln < 64; ++ln) {
          const int b = ln >> 2, j = ln & 3;
          const int col = (NCGv[l] == 2 ? 8 * g : 4 * g) + 4 * cg + j;
          int k;
          if (c < NCm[l]) { k = 16 * c + b; if (k >= Cmain[l]) k = -1; }
          else k = Cmain[l] + 16 * (c - NCm[l]) + b;
          float v = 0.f;
          if (col < Nout[l] && k >= 0) v = Wl[(size_t)col * Kin[l] + k];
          wr[((size_t)g * NREG + RO[l] + c * NCGv[l] + cg) * 64 + ln] = v;
        }
}

int persist_create(PersistNet** out, int device, const ha_mlp_desc* d) {
  *out = nullptr;
#ifdef HA_SIMT_EMU
  (void)device; (void)d;
  return HA_OK;        // the host emulator runs blocks one after another: no persistent teams there
#else
  // the shape this path is built for: the default HuMoR decoder [339 + 48] -> 1024 -> 1024 -> 512 -> 216 with the latent skip
  if (!(d->n_linear == 4 && d->in_dim == P_DIN + P_ZD && d->skip_dim == P_ZD && d->out_dims[0] == P_H0 && d->out_dims[1] == P_H1 &&
        d->out_dims[2] == P_H2 && d->out_dims[3] == P_RAW))
    return HA_OK;
  hipDeviceProp_t prop;
  HA_CHECK_HIP(hipGetDeviceProperties(&prop, device));
  if (prop.multiProcessorCount != NTEAMS * TEAM_CUS) return HA_OK;
  PersistNet* p = new PersistNet();
  p->device = device;
  const int Kin[4] = {P_DIN + P_ZD, P_H0 + P_ZD, P_H1 + P_ZD, P_H2 + P_ZD}, Cmain[4] = {P_DIN, P_H0, P_H1, P_H2};
  const int NCm[4] = {NC0, NC1, NC2, NC3}, NCGv[4] = {2, 2, 1, 1}, RO[4] = {R0, R1, R2, R3}, Nout[4] = {P_H0, P_H1, P_H2, P_RAW};
  std::vector<float> wr((size_t)NWAVES_TEAM * NREG * 64, 0.f);
  for (int l = 0; l < 4; ++l) pack_forward_layer(l, d->w[l], wr);
  int rc = p_upload(&p->Wreg, wr);
  if (rc == HA_OK) {
    std::vector<float> wb((size_t)NWAVES_TEAM * (NREG_B_ALL + BC0_LDS) * 64, 0.f);
    pack_backward(d->w, wb);
    rc = p_upload(&p->Wreg_b, wb);
  }
  if (rc == HA_OK) {
    std::vector<float> wp((size_t)NWAVES_TEAM * PF_NREG * 64, 0.f);
    pack_pipe_forward(d->w, wp);
    rc = p_upload(&p->Wreg_pf, wp);
  }
  if (rc == HA_OK) {
    std::vector<float> wq((size_t)NWAVES_TEAM * (QB_NREG + QB_NLW) * 64, 0.f);
    pack_pipe_backward(d->w, wq);
    rc = p_upload(&p->Wreg_pb, wq);
  }
  const int bpad[4] = {P_H0, P_H1, P_H2, P_RAWPAD};
  for (int l = 0; l < 4 && rc == HA_OK; ++l) {
    std::vector<float> bv(bpad[l], 0.f);
    for (int i = 0; i < Nout[l]; ++i) bv[i] = d->b[l][i];
    rc = p_upload(&p->bias[l], bv);
  }
  for (int l = 1; l < 4 && rc == HA_OK; ++l) {
    if (!d->gn_gamma[l] || !d->gn_beta[l]) { rc = HA_ERR_INVALID_ARG; set_error("persist_create: GroupNorm affine of layer %d missing", l); break; }
    std::vector<float> gv(d->gn_gamma[l], d->gn_gamma[l] + Cmain[l]), bv(d->gn_beta[l], d->gn_beta[l] + Cmain[l]);
    rc = p_upload(&p->gamma[l - 1], gv);
    if (rc == HA_OK) rc = p_upload(&p->beta[l - 1], bv);
  }
  if (rc == HA_OK) {
    hipError_t e = hipHostMalloc((void**)&p->err_host, 64, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&p->err_dev, p->err_host, 0);
    if (e != hipSuccess) { set_error("persist_create: host-mapped error word: %s", hipGetErrorString(e)); rc = HA_ERR_HIP; }
    else *p->err_host = 0;
  }
  if (rc == HA_OK) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_persist_fwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_persist_fwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_persist_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LB_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_persist_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LB_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_pipe_fwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, PL_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_pipe_fwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, PL_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_pipe_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, QL_TOTAL * 4);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(rollout_pipe_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, QL_TOTAL * 4);
    if (e != hipSuccess) { set_error("persist_create: LDS attribute: %s", hipGetErrorString(e)); rc = HA_ERR_HIP; }
  }
  if (rc == HA_OK) {
    // placement / residency probe: one launch of the real kernel with zero steps; every XCD must have received exactly 32 blocks
    unsigned char* xch = nullptr;
    hipError_t e = hipMalloc((void**)&xch, XCH_HDR);
    if (e == hipSuccess) e = hipMemset(xch, 0, XCH_HDR);
    if (e == hipSuccess) {
      PersistArgs a;
      memset(&a, 0, sizeof(a));
      a.xch = xch;
      a.err = p->err_dev;
      HA_LAUNCH(rollout_persist_fwd_kernel<false>, dim3(NTEAMS * TEAM_CUS), dim3(256), L_TOTAL * 4, 0, a);
      e = hipDeviceSynchronize();
    }
    unsigned cnt[NTEAMS] = {0};
    if (e == hipSuccess) e = hipMemcpy(cnt, xch, sizeof(cnt), hipMemcpyDeviceToHost);
    if (xch) (void)hipFree(xch);
    bool even = e == hipSuccess && *p->err_host == 0;
    for (int i = 0; i < NTEAMS; ++i) even = even && cnt[i] == (unsigned)TEAM_CUS;
    if (!even) { persist_destroy(p); return HA_OK; }      // not an error: the launch chain serves this device
  }
  if (rc != HA_OK) { persist_destroy(p); return rc; }
  *out = p;
  return HA_OK;
#endif
}

int persist_forward(PersistNet* p, const PersistFwd& f, int variant, hipStream_t st) {
#ifdef HA_SIMT_EMU
  (void)p; (void)f; (void)variant; (void)st;
  set_error("persistent roll-out: not available on the host emulator");
  return HA_ERR_INVALID_ARG;
#else
  HA_REQUIRE(p && f.B >= 1 && f.B <= 32 * PG_MAX && f.S >= 1, "persistent roll-out: needs 1 <= B <= 256 sequences");
  HA_REQUIRE(f.S < (1 << 28), "persistent roll-out: too many steps");
  if (f.B > NTEAMS * ROWS) {
    // 32 < B <= 256: the layer-parallel pipeline (rollout_pipe.inc), one group of 4 sequences per team and 32-row tile
    zero_async(f.ws, PX_BYTES, st);
    HA_LAUNCH_CHECK();
    PipeArgs a;
    memset(&a, 0, sizeof(a));
    a.B = f.B; a.S = f.S; a.NG = (f.B + 31) / 32;
    a.Wreg = p->Wreg_pf;
    for (int l = 0; l < 4; ++l) { a.bias[l] = p->bias[l]; a.off_dec[l] = f.off_dec[l]; a.dec_pad[l] = f.dec_pad[l]; }
    for (int l = 0; l < 3; ++l) { a.gamma[l] = p->gamma[l]; a.beta[l] = p->beta[l]; a.off_gn[l] = f.off_gn[l]; a.off_ht[l] = f.off_ht[l]; }
    a.past_in0 = f.past_in0; a.z_seq = f.z_seq; a.world = f.world; a.xT = f.xT; a.steps = f.steps;
    a.per_step = f.per_step; a.off_G = f.off_G; a.off_gl = f.off_gl;
    a.t2j = f.t2j;
    a.hidden_slabs = f.hidden_slabs ? 1 : 0;
    a.inject = (variant >> 1) & 1;
    a.xch = reinterpret_cast<unsigned char*>(f.ws);
    a.err = p->err_dev;
    if (variant & 1) HA_LAUNCH(rollout_pipe_fwd_kernel<true>, dim3(NTEAMS * TEAM_CUS), dim3(256), PL_TOTAL * 4, st, a);
    else HA_LAUNCH(rollout_pipe_fwd_kernel<false>, dim3(NTEAMS * TEAM_CUS), dim3(256), PL_TOTAL * 4, st, a);
    HA_LAUNCH_CHECK();
    ++p->launches;
    return HA_OK;
  }
  if (!f.ws_cleared) {                    // (else a launch in front has done it as a block role: turn_dev.h)
    zero_async(f.ws, XCH_BYTES, st);      // tags, team counters (tag 0 never matches); a kernel, not a memset node: common.h
    HA_LAUNCH_CHECK();
  }
  PersistArgs a;
  memset(&a, 0, sizeof(a));
  a.B = f.B; a.S = f.S;
  a.Wreg = p->Wreg;
  for (int l = 0; l < 4; ++l) a.bias[l] = p->bias[l];
  for (int l = 0; l < 3; ++l) { a.gamma[l] = p->gamma[l]; a.beta[l] = p->beta[l]; }
  a.past_in0 = f.past_in0; a.z_seq = f.z_seq; a.world = f.world; a.xT = f.xT; a.steps = f.steps;
  a.per_step = f.per_step; a.off_G = f.off_G;
  for (int l = 0; l < 4; ++l) a.off_dec[l] = f.off_dec[l];
  for (int l = 0; l < 3; ++l) { a.off_gn[l] = f.off_gn[l]; a.off_ht[l] = f.off_ht[l]; }
  a.off_gl = f.off_gl;
  a.t2j = f.t2j;
  a.xch = reinterpret_cast<unsigned char*>(f.ws);
  a.err = p->err_dev;
  a.inject = (variant >> 1) & 1;
  a.hidden_slabs = f.hidden_slabs ? 1 : 0;
  if (variant & 1) HA_LAUNCH(rollout_persist_fwd_kernel<true>, dim3(NTEAMS * TEAM_CUS), dim3(256), L_TOTAL * 4, st, a);
  else HA_LAUNCH(rollout_persist_fwd_kernel<false>, dim3(NTEAMS * TEAM_CUS), dim3(256), L_TOTAL * 4, st, a);
  HA_LAUNCH_CHECK();
  ++p->launches;
  return HA_OK;
#endif
}

int persist_backward(PersistNet* p, const PersistBwd& f, int variant, hipStream_t st) {
#ifdef HA_SIMT_EMU
  (void)p; (void)f; (void)variant; (void)st;
  set_error("persistent roll-out: not available on the host emulator");
  return HA_ERR_INVALID_ARG;
#else
  HA_REQUIRE(p && f.B >= 1 && f.B <= 32 * PG_MAX && f.S >= 1, "persistent roll-out adjoint: needs 1 <= B <= 256 sequences");
  if (f.B > NTEAMS * ROWS) {
    // 32 < B <= 256: the layer-parallel pipelined adjoint (rollout_pipe.inc)
    zero_async(f.ws, PX_BYTES, st);
    HA_LAUNCH_CHECK();
    PipeBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = f.B; a.S = f.S; a.NG = (f.B + 31) / 32;
    a.Wreg = p->Wreg_pb;
    for (int l = 0; l < 3; ++l) { a.gamma[l] = p->gamma[l]; a.beta[l] = p->beta[l]; a.off_gn[l] = f.off_gn[l]; a.off_ht[l] = f.off_ht[l]; }
    for (int l = 0; l < 4; ++l) { a.off_dec[l] = f.off_dec[l]; a.dec_pad[l] = f.dec_pad[l]; }
    a.g_world = f.g_world; a.gx_pri = f.gx_pri; a.gxp_pad = f.gxp_pad;
    a.xT = f.xT; a.steps = f.steps; a.per_step = f.per_step; a.off_G = f.off_G; a.off_gl = f.off_gl;
    a.t2j = f.t2j; a.g_past0 = f.g_past0; a.dz_part = f.dz_part;
    a.xch = reinterpret_cast<unsigned char*>(f.ws);
    a.err = p->err_dev;
    if (variant & 1) HA_LAUNCH(rollout_pipe_bwd_kernel<true>, dim3(NTEAMS * TEAM_CUS), dim3(256), QL_TOTAL * 4, st, a);
    else HA_LAUNCH(rollout_pipe_bwd_kernel<false>, dim3(NTEAMS * TEAM_CUS), dim3(256), QL_TOTAL * 4, st, a);
    HA_LAUNCH_CHECK();
    const int n = f.B * f.S * P_ZD;
    HA_LAUNCH(pipe_dz_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)f.dz_part, f.g_z, f.g_z_add, f.B, f.S, a.NG * 32);
    HA_LAUNCH_CHECK();
    ++p->launches_bwd;
    return HA_OK;
  }
  if (!f.ws_cleared) {
    zero_async(f.ws, XCH_BYTES, st);
    HA_LAUNCH_CHECK();
  }
  PersistBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.B = f.B; a.S = f.S;
  a.Wreg = p->Wreg_b;
  for (int l = 0; l < 3; ++l) { a.gamma[l] = p->gamma[l]; a.beta[l] = p->beta[l]; }
  a.g_world = f.g_world; a.gx_pri = f.gx_pri; a.gxp_pad = f.gxp_pad;
  a.xT = f.xT; a.steps = f.steps; a.per_step = f.per_step; a.off_G = f.off_G;
  for (int l = 0; l < 4; ++l) a.off_dec[l] = f.off_dec[l];
  for (int l = 0; l < 3; ++l) { a.off_gn[l] = f.off_gn[l]; a.off_ht[l] = f.off_ht[l]; }
  a.off_gl = f.off_gl;
  a.t2j = f.t2j; a.g_past0 = f.g_past0; a.dz_part = f.dz_part;
  a.xch = reinterpret_cast<unsigned char*>(f.ws);
  a.err = p->err_dev;
  if (variant & 1) HA_LAUNCH(rollout_persist_bwd_kernel<true>, dim3(NTEAMS * TEAM_CUS), dim3(256), LB_TOTAL * 4, st, a);
  else HA_LAUNCH(rollout_persist_bwd_kernel<false>, dim3(NTEAMS * TEAM_CUS), dim3(256), LB_TOTAL * 4, st, a);
  HA_LAUNCH_CHECK();
  if (!f.defer_dz) {
    const int n = f.B * f.S * P_ZD;
    HA_LAUNCH(dz_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)f.dz_part, f.g_z, f.g_z_add, f.B, f.S);
    HA_LAUNCH_CHECK();
  }
  ++p->launches_bwd;
  return HA_OK;
#endif
}


}  // namespace ha
