// Body of the forward glue kernels (rollout.hip: glue_fwd_kernel<ROTW, DELTA> with FB = false, glue_fwd_fb_kernel with FB = true).  Included
// into each kernel instead of called, so that the kernels without feedback compile to what they were before the feedback variant existed.
// Expects in scope: ROTW, DELTA, FB (compile-time constants), GlueParams p, GlueFeedback fb.
  using RL = RawLayout<ROTW>;
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rt = r >> 5, rr = r & 31;
  const bool valid = r < p.B;
  float* XN = p.xT_next + (size_t)rt * D_INP * 32 + (size_t)rr * 4;
  if (!valid) {
    for (int c = tid; c < D_INP; c += 192) XN[qoff(c)] = 0.f;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sX = smem + S_X;
  float* sRAW = smem + S_RAW;
  float* sSH = smem + S_SH;
  float* sROT = smem + S_GXN;     // FB: the 22 predicted rotations (root | body), then the joint wave's chain [22][12] behind them
  float* sCH = smem + S_GW;
  stage_slabs<1, 192>(sX, p.xT, 1, p.RT, D_INP, D_IN, rt, rr, tid, false);
  stage_slabs<1, 192>(sRAW, p.dec_out, p.dec_nsplit, p.RT, p.dec_pad, RL::D, rt, rr, tid, false);
  if (tid == 0) XN[qoff(D_IN)] = 0.f;      // pad channel of the next state slab
  float G[9], gt[3], t2j[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) G[i] = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) { gt[c] = 0.f; t2j[c] = 0.f; }
  if (wave < 2) {
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = p.Gs[(size_t)r * 12 + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) { gt[c] = p.Gs[(size_t)r * 12 + 9 + c]; t2j[c] = p.t2j[(size_t)r * 3 + c]; }
  }
  // FB: joint j's offset from its parent in the rest pose (the root: its rest position), issued with the loads above
  float fb_t[3] = {0.f, 0.f, 0.f};
  int fb_anc = 0;
  if constexpr (FB) {
    if (wave == 1 && lane < NJT) {
      fb_anc = fb.anc[lane];
      const int par = fb_anc & 31;
      const float* rj = fb.rest + (size_t)r * NJT * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) fb_t[c] = par < NJT ? rj[3 * lane + c] - rj[3 * par + c] : rj[3 * lane + c];
    }
  }
  __syncthreads();
  float* WO = p.world + ((size_t)r * p.S + p.t) * D_STATE;
  PredState s;
  if (wave == 0) {
    // heading alignment from the predicted root orientation
    if (lane == 0) {
      predict_root<ROTW, DELTA>(sX, sRAW, s);
      W2A wa;
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
  } else {
    if (lane >= 1 && lane < NJT) {
      predict_body<ROTW, DELTA>(sX, sRAW, lane - 1, s);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        XN[qoff(18 + 9 * (lane - 1) + i)] = s.pB[i];
        WO[18 + 9 * (lane - 1) + i] = s.pB[i];
      }
      if constexpr (FB) {
#pragma unroll
        for (int i = 0; i < 9; ++i) sROT[9 * lane + i] = s.pB[i];
      }
    }
    if (lane >= 32 && lane < 32 + 9) {
      const int c = lane - 32;
      WO[339 + c] = sRAW[RL::CONT + c];
    }
    if (p.prior_mu && lane < ZD) {
      const float mu = slab_sum(p.pri_out, p.pri_nsplit, p.RT, p.pri_pad, rt, lane, rr);
      const float lv = slab_sum(p.pri_out, p.pri_nsplit, p.RT, p.pri_pad, rt, ZD + lane, rr);
      p.prior_mu[((size_t)r * p.S + p.t) * ZD + lane] = mu;
      p.prior_var[((size_t)r * p.S + p.t) * ZD + lane] = expf(lv);
    }
  }
  __syncthreads();
  float W[9], ptr[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = sSH[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) ptr[c] = sSH[9 + c];
  const float wt[3] = {-ptr[0], -ptr[1], 0.f};

  float fbj[3] = {0.f, 0.f, 0.f};
  if constexpr (FB) {
    if (wave == 1) {       // (the whole wave: wave_sync is a wavefront barrier)
      const bool isj = lane < NJT;
      float T[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) T[i] = 0.f;
      if (isj) {
        // BodyModel takes axis-angle: rotation_matrix_to_angle_axis of the prediction, then smplx's Rodrigues formula
        float Rp[9], aa[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rp[i] = sROT[9 * lane + i];
        rotmat_to_aa(Rp, aa);
        rodrigues(aa, T);
#pragma unroll
        for (int c = 0; c < 3; ++c) T[9 + c] = fb_t[c];
      }
      // T_j = T_parent(j) [R'_j | J_j - J_parent(j)] by pointer jumping: round k absorbs the accumulated transform of the 2^k-th ancestor
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if (k < fb.nrounds) {
          if (isj) {
#pragma unroll
            for (int i = 0; i < 12; ++i) sCH[lane * 12 + i] = T[i];
          }
          wave_sync();
          const int a = (fb_anc >> (5 * k)) & 31;
          if (isj && a < NJT) {
            float A[12], Rn[9], tn[3];
#pragma unroll
            for (int i = 0; i < 12; ++i) A[i] = sCH[a * 12 + i];
            mat3_mul(A, T, Rn);
            mat3_vec(A, T + 9, tn);
#pragma unroll
            for (int i = 0; i < 9; ++i) T[i] = Rn[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) T[9 + c] = tn[c] + A[9 + c];
          }
          wave_sync();
        }
      }
      // Jtr = chain translation + trans (the local-frame prediction, as the body model is called with it)
#pragma unroll
      for (int c = 0; c < 3; ++c) fbj[c] = T[9 + c] + ptr[c];
    }
  }

  if (wave == 1 && lane < NJT) {
    const int j = lane;
    float q[3], o[3];
    // next input: W (pj + wt + t2j) - t2j ; W jv   (FB: the body model's joint in place of pj)
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (FB ? fbj[c] : s.pj[c]) + wt[c] + t2j[c];
    mat3_vec(W, q, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) XN[qoff(207 + 3 * j + c)] = o[c] - t2j[c];
    mat3_vec(W, s.jv, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) XN[qoff(273 + 3 * j + c)] = o[c];
    // world: G^T (pj + t2j) - t2j - gt ; G^T jv
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = s.pj[c] + t2j[c];
    mat3_tvec(G, q, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) WO[207 + 3 * j + c] = o[c] - t2j[c] - gt[c];
    mat3_tvec(G, s.jv, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) WO[273 + 3 * j + c] = o[c];
  }
  if (wave == 0 && lane == 0) {
    float q[3], o[3], M[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = s.ptrans[c] + wt[c];
    mat3_vec(W, q, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) XN[qoff(c)] = o[c];
    mat3_vec(W, s.ptvel, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) XN[qoff(3 + c)] = o[c];
    mat3_mul(W, s.pR, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) XN[qoff(6 + i)] = M[i];
    mat3_vec(W, s.prvel, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) XN[qoff(15 + c)] = o[c];
    // world
    float wtr[3];
    mat3_tvec(G, s.ptrans, wtr);
#pragma unroll
    for (int c = 0; c < 3; ++c) { wtr[c] -= gt[c]; WO[c] = wtr[c]; }
    mat3_tvec(G, s.ptvel, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) WO[3 + c] = o[c];
    mat3_tmul(G, s.pR, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) WO[6 + i] = M[i];
    mat3_tvec(G, s.prvel, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) WO[15 + c] = o[c];
    // accumulate the world transform
    mat3_mul(G, W, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) p.Gs_next[(size_t)r * 12 + i] = M[i];
    p.Gs_next[(size_t)r * 12 + 9] = -wtr[0];
    p.Gs_next[(size_t)r * 12 + 10] = -wtr[1];
    p.Gs_next[(size_t)r * 12 + 11] = 0.f;
  }
