// fused3_actor.hpp -- the actor pass of the fused 3-layer DDPG update:
//   a = A(s), q = C([s; a]) with the UPDATED critic, -mean(q), backward through the critic to da, full actor backward
//   -> one slab of partial gradients per workgroup (summed by fused3_finish.hpp)
#pragma once
#include "fused3_layers.hpp"

namespace pdec {

// LDS map of the actor pass (float offsets).  The backward pass needs W2^T where the forward had W2: its first AX_ROWS rows
// (two output tiles) are copied into X during the forward, the rest into the big region at the switch, behind those two
// tiles (TWO; MT = 9).  A critic of at most AX_ROWS padded rows takes W2^T in one copy and has no X.
#define AX_ROWS 32
template <int MT, int MTA>
struct ActorLds {
  static constexpr int HP = 16 * MT, HPa = 16 * MTA, LDW = HP + LDWPAD;
  static constexpr bool TWO = HP > AX_ROWS && (AX_ROWS * LDW) % 256 == 0;     // W2^T in two parts (X + big region)
  static constexpr int NX = TWO ? AX_ROWS * LDW : 256;                        // floats of the first part (a DMA size: never 0)
  static constexpr int Wreg = 0;                                // [HP][LDW] big weight image / staging images
  static constexpr int sc = Wreg + wreg_floats(MT, MTA);        // critic's small block
  static constexpr int sa = sc + small_floats(HP);              // actor's small block
  static constexpr int saW2 = sa + small_floats(HPa);           // actor's W2 [HPa][LDWa]
  static constexpr int saW2T = saW2 + big_floats(HPa);          // actor's W2^T
  static constexpr int red = saW2T + big_floats(HPa);           // [8] block sums
  static constexpr int X = red + 8;                             // [AX_ROWS][LDW] (TWO only)
  static constexpr int end = X + (TWO ? NX : 0);
  static_assert(actor_stage_floats(MTA) <= wreg_floats(MT, MTA), "the actor's staging images do not fit the big LDS region");
};

template <int MT, int MTA>
__global__ __launch_bounds__(FTHREADS) __attribute__((amdgpu_num_vgpr(112))) void ddpg_actor_fused_kernel(FusedArgs g) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4;
  constexpr int HP = 16 * MT, HPa = 16 * MTA, LDW = HP + LDWPAD, LDWa = HPa + LDWPAD, NW = FTHREADS / 64;
  constexpr int NS = small_floats(HP), NSa = small_floats(HPa), NB = big_floats(HP), NBa = big_floats(HPa);
  using Lds = ActorLds<MT, MTA>;
  constexpr int STATS = stats_chunk(MTA);               // chunk of the pass's one statistic, sum q
  constexpr bool TWO = Lds::TWO;
  constexpr int NX = Lds::NX;
  float* Wreg = smem + Lds::Wreg;
  float* sc = smem + Lds::sc;
  float* sa = smem + Lds::sa;
  float* saW2 = smem + Lds::saW2;
  float* saW2T = smem + Lds::saW2T;
  float* red = smem + Lds::red;
  float* X = smem + Lds::X;
  const SmallLds SC = carve_small(sc, HP), SA = carve_small(sa, HPa);
  const int ns = g.ns;
  const int col = blockIdx.x * FCOLS + w * 16 + lr;
  const bool valid = col < g.Bu;
  const LiveRows LA = live_rows<MTA>(ns, g.A.H, g.full_rows), LC = live_rows<MT>(ns + g.na, g.C.H, g.full_rows);
  set_wave_prio(g.prio);

  // copy schedule as in the critic pass: small blocks, then the per-column input loaded AND consumed, then the long copy
  dma_even<NSa, NW>(sa, g.A.w, w, l);
  dma_even<NBa, NW>(saW2, g.A.w + g.A.oW2, w, l);
  dma_even<NBa, NW>(saW2T, g.A.w + g.A.oW2T, w, l);
  dma_even<NS, NW>(sc, g.C.w, w, l);
  float xs[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = 4 * t + q;
    xs[t] = (valid && row < ns) ? g.s[(size_t)col * ns + row] : 0.f;
  }
  asm volatile("" : "+v"(xs[0]), "+v"(xs[1]), "+v"(xs[2]), "+v"(xs[3]));
  dma_wait();
  dma_even<NB, NW>(Wreg, g.C.w + g.C.oW2, w, l);      // lands behind the actor forward and the critic's first layer
  lds_barrier();
  f32x4 ha1[MTA], ha2[MTA];
  layer_in<MTA, 4>(ha1, xs, SA, lr, q, LA);
  layer_hh_live<MTA, MTA, true>(ha2, ha1, saW2, LDWa, SA.b2, lr, q, LA.mo);
  relu_<MTA>(ha2);
  const float aout = tanhf(head<MTA>(ha2, SA.w3, SA.b3[0], q));
  float x[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) x[t] = (4 * t + q == ns) ? (valid ? aout : 0.f) : xs[t];
  f32x4 h1[MT], h2[MT];
  layer_in<MT, 4>(h1, x, SC, lr, q, LC);
  unsigned long long relu1 = 0;         // bit 4 m + r = [h1[m][r] > 0]: all the backward pass needs of h1
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) relu1 |= (unsigned long long)(h1[m][r] > 0.f) << (4 * m + r);
  dma_wait();
  lds_barrier();
  if constexpr (TWO) dma_even<NX, NW>(X, g.C.w + g.C.oW2T, w, l);      // rows 0 .. 31 of W2^T, behind the forward
  layer_hh<MT, MT, true>(h2, h1, Wreg, LDW, SC.b2, lr, q);
  relu_<MT>(h2);
  const float qv = head<MT>(h2, SC.w3, SC.b3[0], q);
  float st0 = (valid && q == 0) ? qv : 0.f;
  const float dq = valid ? -1.f / (float)g.Bu : 0.f;
  f32x4 dz2[MT];
  head_bwd<MT>(dz2, h2, SC.w3, dq, q);
  f32x4 dz1[MT];
  if constexpr (TWO) {
    dma_wait();
    lds_barrier();                                       // X visible; every wave is done with the big region
    dma_even<NB - NX, NW>(Wreg + NX, g.C.w + g.C.oW2T + NX, w, l);       // rows 32 .. of W2^T behind the first two tiles
    layer_hh_part<MT, MT, false, 0, AX_ROWS / 16>(dz1, dz2, X, LDW, nullptr, lr, q);
    dma_wait();
    lds_barrier();
    layer_hh_part<MT, MT, false, AX_ROWS / 16, MT>(dz1, dz2, Wreg, LDW, nullptr, lr, q);
  } else {
    lds_barrier();
    dma_even<NB, NW>(Wreg, g.C.w + g.C.oW2T, w, l);
    dma_wait();
    lds_barrier();
    layer_hh<MT, MT, false>(dz1, dz2, Wreg, LDW, nullptr, lr, q);
  }
  // da = sum_i W1[i][ns] * dz1[i]  (gradient w.r.t. the action input row of the critic)
  float da = 0.f;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * m + 4 * q + r;
      const float d = ((relu1 >> (4 * m + r)) & 1) ? dz1[m][r] : 0.f;
      da += SC.W1[row * LDW1 + ns] * d;
    }
  da += __shfl_xor(da, 16);
  da += __shfl_xor(da, 32);
  const float dza3 = da * (1.f - aout * aout);
  f32x4 dza2[MTA], dza1[MTA];
  head_bwd<MTA>(dza2, ha2, SA.w3, dza3, q);
  layer_hh_live<MTA, MTA, false>(dza1, dza2, saW2T, LDWa, nullptr, lr, q, LA.mo);
#pragma unroll
  for (int m = 0; m < MTA; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) dza1[m][r] = ha1[m][r] > 0.f ? dza1[m][r] : 0.f;
  // ---- weight gradients of the actor: three small column contractions over all 128 columns in ONE staging round, one output
  // tile per wave (2 + 4 + 2 tiles at MTA = 2); columns are contracted in ascending order.
  const int nslab = gridDim.x;
  constexpr int LDPA = LDP128;
  static_assert(slab_tiles(MTA) <= FTHREADS / 64, "one output tile per wave");
  float* I0 = Wreg;                       // DZ3 [16][LDPA]
  float* I1 = I0 + 16 * LDPA;             // HA2aug [HPa][LDPA]
  float* I2 = I1 + HPa * LDPA;            // DZA2 [HPa][LDPA]
  float* I3 = I2 + HPa * LDPA;            // HA1aug [HPa][LDPA]
  float* I4 = I3 + HPa * LDPA;            // DZA1 [HPa][LDPA]
  float* I5 = I4 + HPa * LDPA;            // Xaug [16][LDPA]
  const int cw = w * 16 + lr;
  lds_barrier();
  for (int i = tid; i < 16 * LDPA; i += FTHREADS) { I0[i] = 0.f; I5[i] = 0.f; }
  lds_barrier();
  if (q == 0) I0[cw] = dza3;
  stage_rows_ld<MTA>(I1, LDPA, ha2, cw, q, g.A.H);
  stage_rows_ld<MTA>(I2, LDPA, dza2, cw, q, -1);
  stage_rows_ld<MTA>(I3, LDPA, ha1, cw, q, g.A.H);
  stage_rows_ld<MTA>(I4, LDPA, dza1, cw, q, -1);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = 4 * t + q;
    I5[row * LDPA + cw] = row == ns ? 1.f : xs[t];
  }
  lds_barrier();
  {
    // tile numbering of the slab (store_pass): dW3a tiles 0 .. MTA-1, dW2a MTA .. MTA+MTA^2-1, dW1a the next MTA
    const float *Lp = nullptr, *Rp = nullptr;
    int T = -1;
    if (w < MTA) { Lp = I0; Rp = I1 + 16 * w * LDPA; T = w; }
    else if (w < MTA + MTA * MTA) { const int u = w - MTA, ti = u / MTA, tk = u - ti * MTA; Lp = I2 + 16 * ti * LDPA; Rp = I3 + 16 * tk * LDPA; T = w; }
    else if (w < 2 * MTA + MTA * MTA) { const int u = w - MTA - MTA * MTA; Lp = I4 + 16 * u * LDPA; Rp = I5; T = w; }
    if (T >= 0) {
      const float* lrow = Lp + lr * LDPA + 4 * q;
      const float* rrow = Rp + lr * LDPA + 4 * q;
      const f32x4 a = tile_chain<8>(f32x4{0.f, 0.f, 0.f, 0.f}, lrow, rrow);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        PDEC_SLAB_STORE(a[r], &g.slab[((size_t)(4 * T + r) * nslab + blockIdx.x) * 64 + l]);
    }
  }
  st0 = block_sum_lds(st0, red, tid);
  if (tid == 0) {
    float* st = g.slab + ((size_t)STATS * nslab + blockIdx.x) * 64;
    st[0] = st0;
    for (int i = 1; i < 8; ++i) st[i] = 0.f;
  }
}

}  // namespace pdec
