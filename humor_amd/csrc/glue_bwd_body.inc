// Body of the backward glue kernels (rollout.hip: glue_bwd_kernel<ROTW, DELTA> with FB = false, glue_bwd_fb_kernel with FB = true).  Included
// into each kernel instead of called, so that the kernels without feedback compile to what they were before the feedback variant existed.
// Expects in scope: ROTW, DELTA, FB (compile-time constants), GlueParams p, GlueFeedback fb, GlueFeedbackAdj fa.
  using RL = RawLayout<ROTW>;
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rt = r >> 5, rr = r & 31;
  if (r >= p.B) return;
  const bool last = p.t == p.S - 1;      // no step t+1 behind this one
  const bool final_collect = p.t < 0;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sX = smem + S_X;
  float* sRAW = smem + S_RAW;
  float* sGXN = smem + S_GXN;
  float* sGW = smem + S_GW;
  float* sSH = smem + S_SH;
  float* sRED = smem + S_RED;
  float* sROT = smem + S_FB_ROT;   // FB: the 22 predicted rotations (root | body)
  float* sCH = smem + S_FB_CH;     // FB: the joint wave's chain [22][12]
  float* sGAM = smem + S_FB_GAM;   // FB: gradient arriving on every fed-back joint
  float* sDO = smem + S_FB_DO;     // FB: dL/d(rest offset) of every joint
  float* sGR = smem + S_FB_GR;     // FB: dL/d(predicted rotation) through the feedback, for the root and the body-rotation wave
  // ---- total adjoint of x_{t+1}: direct part + layer-0 input-gradient slabs of step t+1 (all 256 threads stage) -------
  if (last) {
    for (int c = tid; c < D_IN; c += 256) sGXN[c] = 0.f;
  } else {
    stage_slabs<1, 256>(sGXN, p.gx_dir_in, 1, p.RT, D_INP, D_IN, rt, rr, tid, false);
    stage_slabs<1, 256>(sGXN, p.gxp_pri, p.gxp_pri_nsplit, p.RT, p.gxp_pri_pad, D_IN, rt, rr, tid, true);
    stage_slabs<1, 256>(sGXN, p.gxp_dec, p.gxp_dec_nsplit, p.RT, p.gxp_dec_pad, D_IN, rt, rr, tid, true);
  }
  if (!final_collect) {
    stage_slabs<1, 256>(sX, p.xT, 1, p.RT, D_INP, D_IN, rt, rr, tid, false);
    stage_slabs<1, 256>(sRAW, p.dec_out, p.dec_nsplit, p.RT, p.dec_pad, RL::D, rt, rr, tid, false);
    const float* GWp = p.g_world ? p.g_world + ((size_t)r * p.S + p.t) * D_STATE : nullptr;
    for (int c = tid; c < D_STATE; c += 256) sGW[c] = GWp ? GWp[c] : 0.f;
  }
  // per-sequence state: issued before the barrier so that it overlaps the staging round trip
  float* carry = p.carry + (size_t)r * 16;
  float G[9], gt[3], t2j[3], gGn[9], ggtn[3], g_t2j_acc[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) { G[i] = 0.f; gGn[i] = 0.f; }
#pragma unroll
  for (int c = 0; c < 3; ++c) { gt[c] = 0.f; t2j[c] = 0.f; ggtn[c] = 0.f; g_t2j_acc[c] = 0.f; }
  if (!final_collect && wave < 2) {
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = p.Gs[(size_t)r * 12 + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) { gt[c] = p.Gs[(size_t)r * 12 + 9 + c]; t2j[c] = p.t2j[(size_t)r * 3 + c]; }
    if (!last && wave == 0) {
      // incoming carried adjoints of (G', gt') = state after this step
#pragma unroll
      for (int i = 0; i < 9; ++i) gGn[i] = carry[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ggtn[c] = carry[9 + c]; g_t2j_acc[c] = carry[12 + c]; }
    }
  }
  // FB: joint j's offset from its parent in the rest pose (the root: its rest position) and its subtree, issued with the loads above
  float fb_t[3] = {0.f, 0.f, 0.f};
  int fb_anc = 0, fb_sub = 0;
  if constexpr (FB) {
    if (!final_collect && wave == 1 && lane < NJT) {
      fb_anc = fb.anc[lane];
      fb_sub = fa.sub[lane];
      const int par = fb_anc & 31;
      const float* rj = fb.rest + (size_t)r * NJT * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) fb_t[c] = par < NJT ? rj[3 * lane + c] - rj[3 * par + c] : rj[3 * lane + c];
    }
  }
  __syncthreads();
  auto GXN = [&](int c) -> float { return sGXN[c]; };
  auto gw = [&](int c) { return sGW[c]; };
  if (final_collect) {
    // dz of step 0 ; dL/dpast_in0 = adjoint of x_0 ; t2j = -(x0[207], x0[208], 0)
    if (p.g_z && tid < ZD) {
      float v = 0.f;
      for (int i = 0; i < p.dz_n; ++i) v += slab_sum(p.dz_src[i], p.dz_nsplit[i], p.RT, p.dz_pad[i], rt, p.dz_off[i] + tid, rr);
      p.g_z[((size_t)r * p.S + (p.t + 1)) * ZD + tid] = v;
    }
    for (int c = tid; c < D_IN; c += 256) {
      float v = GXN(c);
      if (c == 207) v -= carry[12];
      if (c == 208) v -= carry[13];
      p.g_past0[(size_t)r * D_IN + c] = v;
    }
    return;
  }

  float* GD = p.g_dec_out + (size_t)rt * p.dec_pad * 32 + (size_t)rr * 4;   // adjoint of the decoder raw output (quad layout)
  float* GX = p.gx_dir_out + (size_t)rt * D_INP * 32 + (size_t)rr * 4;
  PredState s;
  W2A wa;
  // lane-local partial sums of the adjoints shared by the whole sequence (W, G, gt, wt, t2j)
  float gW[9], gG[9], ggt[3] = {0.f, 0.f, 0.f}, gwt[3] = {0.f, 0.f, 0.f}, gt2[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 9; ++i) { gW[i] = 0.f; gG[i] = 0.f; }

  // ---- phase 1 (before W is known) ---------------------------------------------------------------------
  if (wave == 0) {
    if (lane == 0) {
      predict_root<ROTW, DELTA>(sX, sRAW, s);
      w2a_fwd(s.pR, wa);
#pragma unroll
      for (int i = 0; i < 9; ++i) sSH[i] = wa.W[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) sSH[9 + c] = s.ptrans[c];
      if constexpr (FB) {
#pragma unroll
        for (int i = 0; i < 9; ++i) sROT[i] = s.pR[i];
      }
    }
  } else if (wave == 1) {
    if (lane < NJT) predict_joints<ROTW, DELTA>(sX, sRAW, lane, s);
  } else if (wave == 2) {
    // body rotation: pB = dB * Bin goes unchanged to both outputs (no dependence on W or G)
    if (lane >= 1 && lane < NJT) {
      const int bidx = lane - 1;
      predict_body<ROTW, DELTA>(sX, sRAW, bidx, s);
      if constexpr (FB) {
#pragma unroll
        for (int i = 0; i < 9; ++i) sROT[9 * lane + i] = s.pB[i];
      } else {
      float gpB[9], gdB[9], gBin[9], gaa[ROTW];
#pragma unroll
      for (int i = 0; i < 9; ++i) gpB[i] = gw(18 + 9 * bidx + i) + GXN(18 + 9 * bidx + i);
      if constexpr (DELTA) {
        mat3_mult(gpB, s.Bin, gdB);      // gdB = gpB * Bin^T
        mat3_tmul(s.dB, gpB, gBin);      // gBin = dB^T * gpB
      } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) { gdB[i] = gpB[i]; gBin[i] = 0.f; }
      }
      delta_rot_bwd<ROTW>(s.raw_aa_b, gdB, gaa);
#pragma unroll
      for (int c = 0; c < ROTW; ++c) GD[qoff(RL::BODY + ROTW * bidx + c)] = gaa[c];
#pragma unroll
      for (int i = 0; i < 9; ++i) GX[qoff(18 + 9 * bidx + i)] = gBin[i];
      }
    }
  } else {
    // dz of step t+1, contacts, padded decoder channels, prior output adjoint
    if (!last && p.g_z && lane < ZD) {
      float v = 0.f;
      for (int i = 0; i < p.dz_n; ++i) v += slab_sum(p.dz_src[i], p.dz_nsplit[i], p.RT, p.dz_pad[i], rt, p.dz_off[i] + lane, rr);
      p.g_z[((size_t)r * p.S + (p.t + 1)) * ZD + lane] = v;
    }
    if (lane >= 32 && lane < 32 + 9) GD[qoff(RL::CONT + lane - 32)] = gw(339 + lane - 32);
    for (int c = RL::D + lane; c < p.dec_pad; c += 64) GD[qoff(c)] = 0.f;
    if (p.g_pri_out) {
      float* GP = p.g_pri_out + (size_t)rt * p.pri_pad * 32 + (size_t)rr * 4;
      if (lane < ZD) {
        const size_t o = ((size_t)r * p.S + p.t) * ZD + lane;
        GP[qoff(lane)] = p.g_prior_mu ? p.g_prior_mu[o] : 0.f;
        // var = exp(logvar): d/dlogvar = g_var * var (recomputed from the stashed prior output slabs)
        const float var = expf(slab_sum(p.pri_out, p.pri_nsplit, p.RT, p.pri_pad, rt, ZD + lane, rr));
        GP[qoff(ZD + lane)] = p.g_prior_var ? p.g_prior_var[o] * var : 0.f;
      }
      for (int c = 2 * ZD + lane; c < p.pri_pad; c += 64) GP[qoff(c)] = 0.f;
    }
  }
  __syncthreads();
  float W[9], ptr[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = sSH[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) ptr[c] = sSH[9 + c];
  const float wt[3] = {-ptr[0], -ptr[1], 0.f};

  // ---- phase 2: joints (wave 1) next to the root (wave 0, lane 0) ----------------------------------------
  float gptrans[3] = {0.f, 0.f, 0.f}, gptvel[3] = {0.f, 0.f, 0.f}, gprvel[3] = {0.f, 0.f, 0.f}, gpR[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) gpR[i] = 0.f;
  float fbj[3] = {0.f, 0.f, 0.f}, fb_gam[3] = {0.f, 0.f, 0.f}, fb_aa[3] = {0.f, 0.f, 0.f}, fb_T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) fb_T[i] = 0.f;
  if (wave == 1) {
    if constexpr (FB) {      // (the whole wave: wave_sync is a wavefront barrier)
      // the forward's chain again (glue_fwd_body.inc): T_j = [A_j | p_j] by pointer jumping, complete in sCH behind the last round
      const bool isj = lane < NJT;
      if (isj) {
        float Rp[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rp[i] = sROT[9 * lane + i];
        rotmat_to_aa(Rp, fb_aa);
        rodrigues(fb_aa, fb_T);
#pragma unroll
        for (int c = 0; c < 3; ++c) fb_T[9 + c] = fb_t[c];
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if (k < fb.nrounds) {
          if (isj) {
#pragma unroll
            for (int i = 0; i < 12; ++i) sCH[lane * 12 + i] = fb_T[i];
          }
          wave_sync();
          const int a = (fb_anc >> (5 * k)) & 31;
          if (isj && a < NJT) {
            float A[12], Rn[9], tn[3];
#pragma unroll
            for (int i = 0; i < 12; ++i) A[i] = sCH[a * 12 + i];
            mat3_mul(A, fb_T, Rn);
            mat3_vec(A, fb_T + 9, tn);
#pragma unroll
            for (int i = 0; i < 9; ++i) fb_T[i] = Rn[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) fb_T[9 + c] = tn[c] + A[9 + c];
          }
          wave_sync();
        }
      }
      if (isj) {
#pragma unroll
        for (int i = 0; i < 12; ++i) sCH[lane * 12 + i] = fb_T[i];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) fbj[c] = fb_T[9 + c] + ptr[c];
    }
    if (lane < NJT) {
      const int j = lane;
    float g[3], q[3], o[3], gpj[3] = {0.f, 0.f, 0.f}, gjv[3] = {0.f, 0.f, 0.f};
    // world joints: wj = G^T (pj + t2j) - t2j - gt
#pragma unroll
    for (int c = 0; c < 3; ++c) { g[c] = gw(207 + 3 * j + c); q[c] = s.pj[c] + t2j[c]; }
    mat3_vec(G, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) { gpj[c] += o[c]; gt2[c] += o[c] - g[c]; ggt[c] -= g[c]; }
    outer_acc(gG, q, g);
    // world joint velocities: G^T jv
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = gw(273 + 3 * j + c);
    mat3_vec(G, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) gjv[c] += o[c];
    outer_acc(gG, s.jv, g);
    // next-input joints: W (pj + wt + t2j) - t2j
#pragma unroll
    for (int c = 0; c < 3; ++c) { g[c] = GXN(207 + 3 * j + c); q[c] = (FB ? fbj[c] : s.pj[c]) + wt[c] + t2j[c]; }
    mat3_tvec(W, g, o);
    if constexpr (FB) {      // the body model's joint stood here: its gradient goes down the chain, the regressed joint keeps the world part
#pragma unroll
      for (int c = 0; c < 3; ++c) { fb_gam[c] = o[c]; sGAM[3 * j + c] = o[c]; gwt[c] += o[c]; gt2[c] += o[c] - g[c]; }
    } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { gpj[c] += o[c]; gwt[c] += o[c]; gt2[c] += o[c] - g[c]; }
    }
    outer_acc(gW, g, q);
    // next-input joint velocities: W jv
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = GXN(273 + 3 * j + c);
    mat3_tvec(W, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) gjv[c] += o[c];
    outer_acc(gW, g, s.jv);
    // residual composition: pj = raw + x
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      GD[qoff(RL::JNT + 3 * j + c)] = gpj[c];
      GX[qoff(207 + 3 * j + c)] = DELTA ? gpj[c] : 0.f;
      GD[qoff(RL::JVEL + 3 * j + c)] = gjv[c];
      GX[qoff(273 + 3 * j + c)] = DELTA ? gjv[c] : 0.f;
    }
    }
    if constexpr (FB) {
      wave_sync();       // sCH (the chains) and sGAM (the arriving gradients) of every joint
      float dO[3] = {0.f, 0.f, 0.f};
      if (lane < NJT) {
        // P = sum of gamma over the subtree, Sm = sum of gamma (p_m - p_j)^T: ascending joints, one owner
        float P[3] = {0.f, 0.f, 0.f}, Sm[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Sm[i] = 0.f;
        for (int m = 0; m < NJT; ++m) {
          if ((fb_sub >> m) & 1) {
            float gm[3], d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { gm[c] = sGAM[3 * m + c]; d[c] = sCH[m * 12 + 9 + c] - fb_T[9 + c]; P[c] += gm[c]; }
            outer_acc(Sm, gm, d);
          }
        }
        const int par = fb_anc & 31;
        float Ap[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        if (par < NJT) {
#pragma unroll
          for (int i = 0; i < 9; ++i) Ap[i] = sCH[par * 12 + i];
        }
        mat3_tvec(Ap, P, dO);            // dL/do_j = A_parent^T P_j
        float M1[9], gQ[9], gaa[3], Rp[9], gR[9];
        mat3_mul(Sm, fb_T, M1);
        mat3_tmul(Ap, M1, gQ);           // dL/dQ_j = A_parent^T S_j A_j
        rodrigues_bwd(fb_aa, gQ, gaa);
#pragma unroll
        for (int i = 0; i < 9; ++i) Rp[i] = sROT[9 * lane + i];
        rotmat_to_aa_bwd(Rp, gaa, gR);
#pragma unroll
        for (int i = 0; i < 9; ++i) sGR[9 * lane + i] = gR[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) sDO[3 * lane + c] = dO[c];
      }
      wave_sync();
      if (lane < NJT) {
        // o_j = J_j - J_parent(j): dL/dJ_j = dL/do_j - sum over the children's dL/do_c (ascending); this lane owns (sequence, joint) in every step
#pragma unroll
        for (int m = 1; m < NJT; ++m) {
          if ((fb.anc[m] & 31) == lane) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dO[c] -= sDO[3 * m + c];
          }
        }
        float* gr = fa.g_rest + ((size_t)r * NJT + lane) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) gr[c] += dO[c];
      }
      // fb_j = p_j + ptrans: the predicted translation takes the sum over the joints
#pragma unroll
      for (int c = 0; c < 3; ++c) fb_gam[c] = wave_sum(fb_gam[c]);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sRED[27 + c] = fb_gam[c];
      }
    }
    // reduce the joint lanes' partial sums and hand them to the root
#pragma unroll
    for (int i = 0; i < 9; ++i) { gW[i] = wave_sum(gW[i]); gG[i] = wave_sum(gG[i]); }
#pragma unroll
    for (int c = 0; c < 3; ++c) { ggt[c] = wave_sum(ggt[c]); gwt[c] = wave_sum(gwt[c]); gt2[c] = wave_sum(gt2[c]); }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) { sRED[i] = gW[i]; sRED[9 + i] = gG[i]; }
#pragma unroll
      for (int c = 0; c < 3; ++c) { sRED[18 + c] = ggt[c]; sRED[21 + c] = gwt[c]; sRED[24 + c] = gt2[c]; }
    }
  } else if (wave == 0 && lane == 0) {
    float g[3], o[3], q[3];
    // carried: gt' = (-wtrans.x, -wtrans.y, 0)
    float gwtr[3] = {gw(0) - ggtn[0], gw(1) - ggtn[1], gw(2)};
    // wtrans = G^T ptrans - gt
    mat3_vec(G, gwtr, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) { gptrans[c] += o[c]; ggt[c] -= gwtr[c]; }
    outer_acc(gG, s.ptrans, gwtr);
    // wtvel = G^T ptvel
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = gw(3 + c);
    mat3_vec(G, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) gptvel[c] += o[c];
    outer_acc(gG, s.ptvel, g);
    // wR = G^T pR : gpR += G gwR ; gG += pR gwR^T
    float gwR[9], M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) gwR[i] = gw(6 + i);
    mat3_mul(G, gwR, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) gpR[i] += M[i];
    mat3_mult(s.pR, gwR, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) gG[i] += M[i];
    // wrvel = G^T prvel
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = gw(15 + c);
    mat3_vec(G, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) gprvel[c] += o[c];
    outer_acc(gG, s.prvel, g);
    // G' = G W : gG += gG' W^T ; gW += G^T gG'
    mat3_mult(gGn, W, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) gG[i] += M[i];
    mat3_tmul(G, gGn, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) gW[i] += M[i];
    // next input: trans' = W (ptrans + wt)
#pragma unroll
    for (int c = 0; c < 3; ++c) { g[c] = GXN(c); q[c] = s.ptrans[c] + wt[c]; }
    mat3_tvec(W, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) { gptrans[c] += o[c]; gwt[c] += o[c]; }
    outer_acc(gW, g, q);
    // tvel' = W ptvel
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = GXN(3 + c);
    mat3_tvec(W, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) gptvel[c] += o[c];
    outer_acc(gW, g, s.ptvel);
    // R' = W pR : gpR += W^T gR' ; gW += gR' pR^T
    float gRn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) gRn[i] = GXN(6 + i);
    mat3_tmul(W, gRn, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) gpR[i] += M[i];
    mat3_mult(gRn, s.pR, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) gW[i] += M[i];
    // rvel' = W prvel
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = GXN(15 + c);
    mat3_tvec(W, g, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) gprvel[c] += o[c];
    outer_acc(gW, g, s.prvel);
  }
  __syncthreads();

  // ---- phase 3: the root finishes (heading alignment and root rotation adjoints, carried state) -------------
  if (wave == 0 && lane == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { gW[i] += sRED[i]; gG[i] += sRED[9 + i]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { ggt[c] += sRED[18 + c]; gwt[c] += sRED[21 + c]; gt2[c] += sRED[24 + c]; }
    if constexpr (FB) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gptrans[c] += sRED[27 + c];
#pragma unroll
      for (int i = 0; i < 9; ++i) gpR[i] += sGR[i];
    }
    // wt = (-ptrans.x, -ptrans.y, 0)
    gptrans[0] -= gwt[0];
    gptrans[1] -= gwt[1];
    // W = world2aligned(pR)
    float g0, g3;
    w2a_bwd(wa, gW, g0, g3);
    gpR[0] += g0;
    gpR[3] += g3;
    // pR = dR * Rin
    float gdR[9], gRin[9], gaa[ROTW];
    if constexpr (DELTA) {
      mat3_mult(gpR, s.Rin, gdR);
      mat3_tmul(s.dR, gpR, gRin);
    } else {
#pragma unroll
      for (int i = 0; i < 9; ++i) { gdR[i] = gpR[i]; gRin[i] = 0.f; }
    }
    delta_rot_bwd<ROTW>(s.raw_aa_r, gdR, gaa);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      GD[qoff(c)] = gptrans[c];        GX[qoff(c)] = DELTA ? gptrans[c] : 0.f;
      GD[qoff(3 + c)] = gptvel[c];   GX[qoff(3 + c)] = DELTA ? gptvel[c] : 0.f;
      GD[qoff(RL::RVEL + c)] = gprvel[c];   GX[qoff(15 + c)] = DELTA ? gprvel[c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < ROTW; ++c) GD[qoff(RL::ROOT + c)] = gaa[c];
#pragma unroll
    for (int i = 0; i < 9; ++i) GX[qoff(6 + i)] = gRin[i];
    // carry to step t-1
#pragma unroll
    for (int i = 0; i < 9; ++i) carry[i] = gG[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) { carry[9 + c] = ggt[c]; carry[12 + c] = g_t2j_acc[c] + gt2[c]; }
  }
  if constexpr (FB) {
    // the body rotations' adjoint, held back until the feedback's share of dL/dpB has arrived
    if (wave == 2 && lane >= 1 && lane < NJT) {
      const int bidx = lane - 1;
      float gpB[9], gdB[9], gBin[9], gaa[ROTW];
#pragma unroll
      for (int i = 0; i < 9; ++i) gpB[i] = gw(18 + 9 * bidx + i) + GXN(18 + 9 * bidx + i) + sGR[9 * lane + i];
      if constexpr (DELTA) {
        mat3_mult(gpB, s.Bin, gdB);      // gdB = gpB * Bin^T
        mat3_tmul(s.dB, gpB, gBin);      // gBin = dB^T * gpB
      } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) { gdB[i] = gpB[i]; gBin[i] = 0.f; }
      }
      delta_rot_bwd<ROTW>(s.raw_aa_b, gdB, gaa);
#pragma unroll
      for (int c = 0; c < ROTW; ++c) GD[qoff(RL::BODY + ROTW * bidx + c)] = gaa[c];
#pragma unroll
      for (int i = 0; i < 9; ++i) GX[qoff(18 + 9 * bidx + i)] = gBin[i];
    }
  }
