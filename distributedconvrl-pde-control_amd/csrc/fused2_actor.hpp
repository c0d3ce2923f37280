// fused2_actor.hpp -- the actor pass of the fused 2-layer DDPG update:
//   a = A(s), q = C([s; a]), -mean(q), backward through the critic to da, actor backward (dW1, db1, dW2, db2)
//   -> one slab of partial gradients per workgroup (summed by fused2_finish.hpp)
#pragma once
#include "fused2_layers.hpp"

namespace pdec {

// LDS map of the actor pass, stated as Critic2Lds is: float offsets of the two images, then the positions from `base` (the
// dynamic LDS in the kernel, 0 on the host) of the staging images and of what lies behind Saug, which grows with
// xrows = 16 nr_of(ns), the staged (padded) state rows, known at the launch.  KB is the CRITIC's k-block count: both images are
// built at its row stride.  Nothing overlays anything here.
template <int MT, int MTA, int KB>
struct Actor2Lds {
  static constexpr int HP = 16 * MT, HPa = 16 * MTA, LDK = 8 * KB + 4;
  static constexpr int SC = 0;                                  // critic image
  static constexpr int SA = SC + lds2_floats(HP, LDK);          // actor image
  template <class P>
  struct Behind {
    P Lm, Rm;    // staging: DZA1 [HPa][LDP], Saug [xrows][LDP]
    P redA;      // [8][HPa] row reduction of the output-row gradient
    P dacc;      // dW2a / db2a accumulator [HPa]
    P red;       // [8] block sum
    P end;
  };
  template <class P>
  __host__ __device__ __forceinline__ static Behind<P> behind(P base, int xrows) {
    Behind<P> b;
    b.Lm = base + SA + lds2_floats(HPa, LDK);
    b.Rm = b.Lm + HPa * LDP;
    b.redA = b.Rm + xrows * LDP;
    b.dacc = b.redA + 8 * HPa;
    b.red = b.dacc + HPa;
    b.end = b.red + 8;
    return b;
  }
};

template <int MT, int MTA, int KB>
__global__ __launch_bounds__(FTHREADS) void ddpg2_actor_kernel(Fused2Args g) {
  constexpr int LDK = 8 * KB + 4;
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4;
  constexpr int HP = 16 * MT, HPa = 16 * MTA;
  const int ns = g.ns, nRa = nr_of(ns);
  const int xrows = 16 * nRa;
  using Lds = Actor2Lds<MT, MTA, KB>;
  const Lds2 SC = carve2(smem + Lds::SC, HP, LDK), SA = carve2(smem + Lds::SA, HPa, LDK);
  const auto behind = Lds::behind(&smem[0], xrows);
  float *Lm = behind.Lm, *Rm = behind.Rm, *redA = behind.redA, *dacc = behind.dacc, *red = behind.red;
  const int nt = (g.Bu + 15) / 16, t0 = blockIdx.x * g.tpw, t1 = min(t0 + g.tpw, nt);     // wave tiles of this workgroup (critic pass)

  load_net2(SA, g.A, HPa, LDK, tid);
  load_net2(SC, g.C, HP, LDK, tid);
  for (int i = tid; i < HPa; i += FTHREADS) dacc[i] = 0.f;
  __syncthreads();
  f32x4 acc[1];
  zero_(acc);
  float st0 = 0.f;
  const int cw = (w & 3) * 16 + lr;
#pragma unroll 1
  for (int tb = t0; tb < t1; tb += 8) {
    const int live = min(8, t1 - tb);           // waves 0 .. live-1 hold columns (uniform over the workgroup)
    const int col = (tb + w) * 16 + lr;
    const bool valid = w < live && col < g.Bu;
    float xs[K2MAX][2];
    f32x4 ha[MTA];
    float dza2 = 0.f;
    if (w < live) {
      load_x2(xs, g.s, (size_t)col, ns, KB, q, valid);
      layer1_keep<MTA, KB>(ha, xs, SA, lr, q);
      const float aout = tanhf(head<MTA>(ha, SA.w2, SA.b2[0], q));
      float x[K2MAX][2];
#pragma unroll
      for (int blk = 0; blk < K2MAX; ++blk) { x[blk][0] = xs[blk][0]; x[blk][1] = xs[blk][1]; }
      set_row2(x, ns, valid ? aout : 0.f, q);
      // q = C([s; a]) and da = sum_i W1c[i][ns] * relu'(h1_i) * w2c_i * dq, tile by tile (nothing of h1 is kept)
      const float dq = valid ? -1.f / (float)g.Bu : 0.f;
      float qacc = 0.f, da = 0.f;
      layer1_head_da<MT, KB>(x, SC, ns, lr, q, qacc, da);
      qacc += __shfl_xor(qacc, 16);
      qacc += __shfl_xor(qacc, 32);
      da += __shfl_xor(da, 16);
      da += __shfl_xor(da, 32);
      if (valid && q == 0) st0 += qacc + SC.b2[0];
      dza2 = da * dq * (1.f - aout * aout);
    } else {                                    // a wave without columns in this chunk contributes zeros
#pragma unroll
      for (int blk = 0; blk < K2MAX; ++blk) { xs[blk][0] = 0.f; xs[blk][1] = 0.f; }
      zero_(ha);
    }
    __syncthreads();                            // the previous chunk's tiles have been consumed
    out_row_grad<MTA>(ha, dza2, g.A.H, redA, dacc, tid);
#pragma unroll
    for (int m = 0; m < MTA; ++m) {
      const float* wv = SA.w2 + 16 * m + 4 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r) ha[m][r] = ha[m][r] > 0.f ? wv[r] * dza2 : 0.f;
    }
    for (int half = 0; 4 * half < live; ++half) {
      __syncthreads();
      if ((w >> 2) == half) {
        stage_rows<MTA>(Lm, ha, cw, q, -1);
        stage_x2<LDP>(Rm, xs, xrows, cw, q, w < live ? ns : -1);
      }
      __syncthreads();
      gemm_cols<1, LDP, 4>(acc, Lm, Rm, MTA, nRa, w, lr, q);
    }
  }
  const int nslab = gridDim.x;
  store_pass(acc, g.slab, nslab, MTA, MTA, nRa, w, l);
  __syncthreads();
  store_row(dacc, HPa, g.slab, nslab, 0, tid);
  st0 = block_sum(st0, red, tid);
  if (tid == 0) {
    float* st = g.slab + ((size_t)stats2_chunk(MTA, nRa) * nslab + blockIdx.x) * 64;
    st[0] = st0;
    st[1] = st[2] = st[3] = st[4] = 0.f;
  }
}

}  // namespace pdec
