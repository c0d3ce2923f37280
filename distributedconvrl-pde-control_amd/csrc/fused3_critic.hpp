// fused3_critic.hpp -- the critic pass of the fused 3-layer DDPG update:
//   a' = At(s'), qt = Ct([s'; a']), q = C([s; a]), loss statistics, dq, full critic backward (dW1, db1, dW2, db2, dW3, db3)
//   -> one slab of partial gradients per workgroup (summed by fused3_finish.hpp)
#pragma once
#include "fused3_layers.hpp"

namespace pdec {

// LDS map of the critic pass (float offsets).  Every weight block arrives by LDS-DMA in whole pieces (dma_even); the
// behaviour critic's small block is copied during the target phase into a region of its own, so the phase switch is one
// barrier + the issue of the next big copy.  Copies are waited for in issue order with literal vmcnt counts.
template <int MT, int MTA>
struct CriticLds {
  static constexpr int HP = 16 * MT, HPa = 16 * MTA;
  static constexpr int Wreg = 0;                                // [HP][LDW] big weight image / staging images
  static constexpr int sc = Wreg + wreg_floats(MT, MTA);        // target critic's small block
  static constexpr int sc2 = sc + small_floats(HP);             // behaviour critic's small block
  static constexpr int sa = sc2 + small_floats(HP);             // target actor's small block
  static constexpr int saW2 = sa + small_floats(HPa);           // target actor's W2 [HPa][LDWa]
  static constexpr int red = saW2 + big_floats(HPa);            // [8] block sums
  static constexpr int redA = red + 8;                          // [8][HP] pass A
  static constexpr int red5 = redA + 8 * HP;                    // [8][8] loss statistics
  static constexpr int end = red5 + 64;
  // the staging images that overlay Wreg: pass B's two [HP][LDP] (in wreg_floats), pass C's dz1 [HP][LDP128] + x [16][LDP128]
  static_assert(HP * LDP128 + 16 * LDP128 <= wreg_floats(MT, MTA), "pass C images do not fit the big LDS region");
};

template <int MT, int MTA>
__global__ __launch_bounds__(FTHREADS) __attribute__((amdgpu_num_vgpr(112))) void ddpg_critic_fused_kernel(FusedArgs g) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4;
  using Lds = CriticLds<MT, MTA>;
  constexpr int STATS = stats_chunk(MT);                // chunk of the loss statistics
  constexpr int HP = 16 * MT, HPa = 16 * MTA, LDW = HP + LDWPAD, LDWa = HPa + LDWPAD, NW = FTHREADS / 64;
  constexpr int NS = small_floats(HP), NSa = small_floats(HPa), NB = big_floats(HP), NBa = big_floats(HPa);
  float* Wreg = smem + Lds::Wreg;
  float* sc = smem + Lds::sc;
  float* sc2 = smem + Lds::sc2;
  float* sa = smem + Lds::sa;
  float* saW2 = smem + Lds::saW2;
  float* red = smem + Lds::red;
  const SmallLds SCt = carve_small(sc, HP), SC = carve_small(sc2, HP), SA = carve_small(sa, HPa);
  const int ns = g.ns, na = g.na, K0 = ns + na;
  const int col = blockIdx.x * FCOLS + w * 16 + lr;
  const bool valid = col < g.Bu;
  const LiveRows LAt = live_rows<MTA>(ns, g.At.H, g.full_rows), LC = live_rows<MT>(K0, g.C.H, g.full_rows);   // (Ct is C's shape)
  set_wave_prio(g.prio);

  // ---- phase T: target actor + target critic
  STAMP_RT(11);
  STAMP(0);
  // Copy schedule.  hipcc drains every LDS-DMA in flight (vmcnt(0)) at the first use of an ordinary global load and at every
  // __syncthreads(), so: the small blocks of the target nets are copied first, the per-column inputs are loaded and CONSUMED
  // (that wait covers the small copies, which are needed now anyway), and only then the long copies start -- the target
  // critic's W2 and the behaviour critic's small block -- which stay in flight across the raw barriers (lds_barrier) of the
  // target actor and layer 1.  No ordinary global load is used again before the last copy of the pass has been waited for.
  dma_even<NS, NW>(sc, g.Ct.w, w, l);
  dma_even<NSa, NW>(sa, g.At.w, w, l);
  dma_even<NBa, NW>(saW2, g.At.w + g.At.oW2, w, l);
  float xn[4], xq[4];                       // input rows 4t+q of s' and of [s; a]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = 4 * t + q;
    xn[t] = (valid && row < ns) ? g.sn[(size_t)col * ns + row] : 0.f;
    float v = 0.f;
    if (valid && row < ns) v = g.s[(size_t)col * ns + row];
    else if (valid && row < K0) v = g.a[(size_t)col * na + (row - ns)];
    xq[t] = v;
  }
  float rv = valid ? g.r[col] : 0.f;
  float tv = valid ? g.t[col] : 0.f;
  // mean reward for the reference's (1xBu).+(Bu) broadcast: every workgroup reduces all of r in the
  // same fixed order, so the value is identical everywhere
  float rsum = 0.f;
  if (g.quirk && g.rpart) {
    for (int i = tid; i < g.nrpart; i += FTHREADS) rsum += g.rpart[i];
  } else if (g.quirk && !g.rbar_dev) {   // 16-B loads, 8 in flight per lane: the L2 latency is paid per batch, not per element
    const int n4 = ((reinterpret_cast<uintptr_t>(g.r) & 15) == 0) ? g.Bu / 4 : 0;
    const f32x4* r4 = reinterpret_cast<const f32x4*>(g.r);
    int i = tid;
    for (; i + 7 * FTHREADS < n4; i += 8 * FTHREADS) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = r4[i + u * FTHREADS];
#pragma unroll
      for (int u = 0; u < 8; ++u) rsum += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
    }
    for (; i < n4; i += FTHREADS) { const f32x4 v = r4[i]; rsum += (v[0] + v[1]) + (v[2] + v[3]); }
    for (int k = 4 * n4 + tid; k < g.Bu; k += FTHREADS) rsum += g.r[k];
  }
  float rbar_in = g.rbar_dev ? g.rbar_dev[0] : 0.f;
  // every loaded value is consumed HERE (the compiler's wait for them lands in front of this statement)
  asm volatile("" : "+v"(xn[0]), "+v"(xn[1]), "+v"(xn[2]), "+v"(xn[3]), "+v"(xq[0]), "+v"(xq[1]), "+v"(xq[2]), "+v"(xq[3]),
               "+v"(rv), "+v"(tv), "+v"(rsum), "+v"(rbar_in));
  dma_wait();                                             // (the small copies; nothing else is outstanding)
  dma_even<NB, NW>(Wreg, g.Ct.w + g.Ct.oW2, w, l);
  dma_even<NS, NW>(sc2, g.C.w, w, l);
  constexpr int N_SC = dma_count<NS, NW>();
  float rbar = block_sum_lds(rsum, red, tid) / (float)g.Bu;   // raw barriers inside (small blocks visible afterwards)
  if (g.rbar_dev) rbar = rbar_in;
  STAMP(1);

  float x[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) x[t] = xn[t];
  float tgt;
  {
    f32x4 ha1[MTA], ha2[MTA];
    layer_in<MTA, 4>(ha1, x, SA, lr, q, LAt);
    layer_hh_live<MTA, MTA, true>(ha2, ha1, saW2, LDWa, SA.b2, lr, q, LAt.mo);
    relu_<MTA>(ha2);
    const float an = tanhf(head<MTA>(ha2, SA.w3, SA.b3[0], q));      // na == 1
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (4 * t + q == ns) x[t] = valid ? an : 0.f;
    f32x4 h1[MT], h2[MT];
    layer_in<MT, 4>(h1, x, SCt, lr, q, LC);
    dma_wait_but<N_SC>();                                 // the target critic's W2 has landed
    lds_barrier();
    layer_hh<MT, MT, true>(h2, h1, Wreg, LDW, SCt.b2, lr, q);
    relu_<MT>(h2);
    const float qt = head<MT>(h2, SCt.w3, SCt.b3[0], q);
    tgt = g.gamma * (1.f - tv) * qt;
  }
  dma_wait();                                             // the behaviour critic's small block (issued a phase ago)
  lds_barrier();                                        // every wave is done with Wreg; sc2 visible
  STAMP(2);
  // ---- phase Q: behaviour critic forward; its W2 lands behind layer 1
  dma_even<NB, NW>(Wreg, g.C.w + g.C.oW2, w, l);
  STAMP(3);
#pragma unroll
  for (int t = 0; t < 4; ++t) x[t] = xq[t];
  f32x4 h1[MT], h2[MT];
  layer_in<MT, 4>(h1, x, SC, lr, q, LC);
  dma_wait();
  lds_barrier();
  layer_hh<MT, MT, true>(h2, h1, Wreg, LDW, SC.b2, lr, q);
  relu_<MT>(h2);
  const float qv = head<MT>(h2, SC.w3, SC.b3[0], q);
  const float c = valid ? tgt - qv : 0.f;
  const float dq = valid ? -(2.f / (float)g.Bu) * ((g.quirk ? rbar : rv) + c) : 0.f;
  // loss statistics (one lane per column contributes)
  const bool rep = valid && q == 0;
  float sv[5] = {rep ? c : 0.f, rep ? c * c : 0.f, rep ? rv : 0.f, rep ? rv * rv : 0.f, rep ? (rv + c) * (rv + c) : 0.f};
  const int nslab = gridDim.x;
  float* Lm = Wreg;                 // staging images overlay the big weight region
  float* Rm = Wreg + HP * LDP;
  const int cw = (w & 3) * 16 + lr;

  // ---- pass A: dW3/db3 = dq x [h2; 1]^T.  A single output row: reduce dq*h2 over the 16 columns of each wave with DPP
  // row sums, then over the 8 waves through LDS (fixed order -> deterministic); no MFMA/staging round.  dz2 is taken from
  // h2 first and the row sums then overwrite h2 in place with no branch between them; the five loss statistics ride on the
  // same barrier.
  lds_barrier();
  STAMP(4);
  dma_even<NB, NW>(Wreg, g.C.w + g.C.oW2T, w, l);     // W2^T for the backward pass lands behind pass A
  f32x4 dz2[MT];
  head_bwd<MT>(dz2, h2, SC.w3, dq, q);
  float a_keep = 0.f;                 // this thread's element of dW3 / of the statistics (stored behind the next barrier)
  {
    float* redA = smem + Lds::redA;
    float* red5 = smem + Lds::red5;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * m + 4 * q + r;
        h2[m][r] = row_sum16((row == g.C.H ? 1.f : h2[m][r]) * dq);
      }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      for (int off = 32; off > 0; off >>= 1) sv[k] += __shfl_xor(sv[k], off);
    if (lr == 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) redA[w * HP + 16 * m + 4 * q + r] = h2[m][r];
    }
    if (l == 0)
      for (int k = 0; k < 5; ++k) red5[w * 8 + k] = sv[k];
    lds_barrier();
    if (tid < HP) {
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) a_keep += redA[ww * HP + tid];
    } else if (tid >= FTHREADS - 8) {          // the last eight lanes of the last wave: the statistics chunk
      if (tid - (FTHREADS - 8) < 5)
        for (int ww = 0; ww < NW; ++ww) a_keep += red5[ww * 8 + tid - (FTHREADS - 8)];
    }
  }
  // ---- dh1 = W2^T dz2, dz1
  STAMP(5);
  dma_wait();                         // W2^T (no store is outstanding yet: the slab stores of pass A follow the barrier)
  lds_barrier();
  STAMP(6);
  if (tid < HP)                       // slab position of element (row 0, column tid) of the [16][HP] product: tile tid/16, register 0, lane tid%16
    g.slab[((size_t)(4 * (tid >> 4)) * nslab + blockIdx.x) * 64 + (tid & 15)] = a_keep;
  else if (tid >= FTHREADS - 8)
    g.slab[((size_t)STATS * nslab + blockIdx.x) * 64 + (tid - (FTHREADS - 8))] = a_keep;
  f32x4 dz1[MT];
  layer_hh<MT, MT, false>(dz1, dz2, Wreg, LDW, nullptr, lr, q);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) dz1[m][r] = h1[m][r] > 0.f ? dz1[m][r] : 0.f;
  // ---- pass C first: dW1/db1 = dz1 x [x0; 1]^T in ONE staging round over all 128 columns (dz1 [HP][LDP128] +
  // x [16][LDP128] fill the big region exactly); dz1 is dead afterwards, which leaves pass B the registers for two
  // interleaved accumulation chains per wave
  STAMP(7);
  {
    float* Lc = Wreg;
    float* Rc = Wreg + HP * LDP128;
    const int cw128 = w * 16 + lr;
    f32x4 accC[((MT + 7) / 8 + 1) & ~1];
    zero_(accC);
    lds_barrier();
    stage_rows_ld<MT>(Lc, LDP128, dz1, cw128, q, -1);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = 4 * t + q;
      Rc[row * LDP128 + cw128] = row == K0 ? 1.f : x[t];
    }
    lds_barrier();
    gemm_pass_paired<((MT + 7) / 8 + 1) & ~1, 8>(accC, Lc, Rc, LDP128, MT, 1, w, lr, q);
    store_pass(accC, g.slab, nslab, MT + MT * MT, MT, 1, w, l);
  }
  // ---- pass B: dW2/db2 = dz2 x [h1; 1]^T, two 64-column halves
  STAMP(8);
  {
    f32x4 accB[(MT * MT + 7) / 8];
    zero_(accB);
    lds_barrier();
    if ((w >> 2) == 0) {
      stage_rows<MT>(Lm, dz2, cw, q, -1);
      stage_rows<MT>(Rm, h1, cw, q, g.C.H);
    }
    lds_barrier();
    gemm_pass_paired<(MT * MT + 7) / 8, 4>(accB, Lm, Rm, LDP, MT, MT, w, lr, q);
    lds_barrier();
    if ((w >> 2) == 1) {
      stage_rows<MT>(Lm, dz2, cw, q, -1);
      stage_rows<MT>(Rm, h1, cw, q, g.C.H);
    }
    lds_barrier();
    gemm_pass_paired_store<(MT * MT + 7) / 8, 4>(accB, Lm, Rm, LDP, MT, MT, w, lr, q, g.slab, nslab, MT, l);     // stores behind each tile pair
  }
  STAMP(9);
  STAMP(10);      // (read_stamps takes slot k + 1 - slot k for k = 0 .. 9, and slot 10 - slot 0)
  STAMP_RT(12);
}

}  // namespace pdec
