// fused2_critic.hpp -- the critic pass of the fused 2-layer DDPG update:
//   a' = At(s'), qt = Ct([s'; a']), q = C([s; a]), loss statistics, dq, critic backward (dW1, db1, dW2, db2)
//   -> one slab of partial gradients per workgroup (summed by fused2_finish.hpp)
#pragma once
#include "fused2_layers.hpp"

namespace pdec {

#ifndef CPWMAX             // column chunks one workgroup walks through: a shape constant of mlp_mfma2.hip (grid2_of deals by it)
#error "fused2_critic.hpp is part of the translation unit mlp_mfma2.hip, which defines CPWMAX ahead of it"
#endif

// LDS map of the critic pass.  The regions up to the staging images are fixed by the instantiation: float offsets into the
// dynamic LDS.  Those behind them move with xrows = 16 nr_of(ns + 1), the staged (padded) input rows, known at the launch:
// positions counted from `base`, which is the dynamic LDS (P = float*) in the kernel and 0 (P = int, float offsets) on the
// host, which takes the launch's byte count from behind(0, xrows).end.
template <int MT, int MTA, int KB>
struct Critic2Lds {
  static constexpr int HP = 16 * MT, HPa = 16 * MTA, LDK = 8 * KB + 4;
  static constexpr int SC = 0;                                  // critic image: the target critic's, then the behaviour critic's
  static constexpr int Lm = SC + lds2_floats(HP, LDK);          // staging: DZ1 [HP][LDQ] ...
  static constexpr int Rm = Lm + HP * LDQ;                      // ... and Xaug [xrows][LDQ]
  static constexpr int redA = Lm;                               // overlays the staging: [8][HP] row reduction of the output-row gradient
  static constexpr int red5 = Lm;                               // overlays it after the last chunk: [8][8] loss statistics
  // the staging region holds the larger of its tenants
  __host__ __device__ static int stage(int xrows) { const int gemm = HP * LDQ + xrows * LDQ, rows = 8 * HP; return gemm > rows ? gemm : rows; }
  template <class P>
  struct Behind {
    P SA;        // target actor's image
    P dacc;      // dW2 / db2 accumulator [HP]
    P end;
  };
  template <class P>
  __host__ __device__ __forceinline__ static Behind<P> behind(P base, int xrows) {
    Behind<P> b;
    b.SA = base + Lm + stage(xrows);
    b.dacc = b.SA + lds2_floats(HPa, LDK);
    b.end = b.dacc + HP;
    return b;
  }
};

template <int MT, int MTA, int KB>
__global__ __launch_bounds__(FTHREADS) void ddpg2_critic_kernel(Fused2Args g) {
  constexpr int LDK = 8 * KB + 4;
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4;
  constexpr int HP = 16 * MT, HPa = 16 * MTA;
  const int ns = g.ns, K0 = ns + 1, nR = nr_of(K0);
  const int xrows = 16 * nR;
  using Lds = Critic2Lds<MT, MTA, KB>;
  const Lds2 SC = carve2(smem + Lds::SC, HP, LDK);
  float *Lm = smem + Lds::Lm, *Rm = smem + Lds::Rm, *redA = smem + Lds::redA, *red5 = smem + Lds::red5;
  const auto behind = Lds::behind(&smem[0], xrows);
  const Lds2 SA = carve2(behind.SA, HPa, LDK);
  float* dacc = behind.dacc;
  // Columns in units of WAVE TILES (16 columns): workgroup b owns the tiles [t0, t1) and walks them in chunks of 8 (one per
  // wave).  The tiles are dealt evenly over the grid (grid2_of) instead of whole 128-column chunks strided over it -- config
  // C4's 784 chunks came as 196 workgroups x 4 chunks (60 CUs idle, x0.77); now 256 workgroups take 24.5 tiles each: three
  // full chunks and one with a single live wave, in which the other waves skip their forward passes and the dW1 GEMM skips the
  // column quarters that hold no live wave.
  const int nt = (g.Bu + 15) / 16, t0 = blockIdx.x * g.tpw, t1 = min(t0 + g.tpw, nt);

  load_net2(SA, g.At, HPa, LDK, tid);
  load_net2(SC, g.Ct, HP, LDK, tid);
  for (int i = tid; i < HP; i += FTHREADS) dacc[i] = 0.f;
  const float rbar = g.quirk ? g.rbar[0] : 0.f;
  __syncthreads();
  // ---- targets of every chunk: a' = At(s'), qt = Ct([s'; a'])
  float tgt[CPWMAX];
#pragma unroll
  for (int j = 0; j < CPWMAX; ++j) {
    const int tile = t0 + 8 * j + w;
    tgt[j] = 0.f;
    if (tile < t1) {
      const int col = tile * 16 + lr;
      const bool valid = col < g.Bu;
      float xn[K2MAX][2];
      load_x2(xn, g.sn, (size_t)col, ns, KB, q, valid);
      const float tv = valid ? g.t[col] : 0.f;
      f32x4 ha[MTA];
      layer1_keep<MTA, KB>(ha, xn, SA, lr, q);
      const float an = tanhf(head<MTA>(ha, SA.w2, SA.b2[0], q));
      set_row2(xn, ns, valid ? an : 0.f, q);
      const float qt = layer1_head<MT, KB>(xn, SC, lr, q);
      tgt[j] = g.gamma * (1.f - tv) * qt;
    }
  }
  __syncthreads();                              // every wave is done with the target critic's image
  load_net2(SC, g.C, HP, LDK, tid);
  __syncthreads();
  // ---- q = C([s; a]), dq, gradients, chunk by chunk
  constexpr int NACC = (MT * 3 + 7) / 8;
  f32x4 acc[NACC];
  zero_(acc);
  float sv[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const int cw = (w & 1) * 16 + lr;
#pragma unroll 1
  for (int j = 0; j < CPWMAX; ++j) {
    const int tb = t0 + 8 * j;                  // first tile of this chunk
    if (tb >= t1) break;
    const int live = min(8, t1 - tb);           // waves 0 .. live-1 hold columns (uniform over the workgroup)
    const float tgj = j == 0 ? tgt[0] : (j == 1 ? tgt[1] : (j == 2 ? tgt[2] : tgt[3]));
    const int col = (tb + w) * 16 + lr;
    const bool valid = w < live && col < g.Bu;
    float xq[K2MAX][2];
    f32x4 h1[MT];
    float dq = 0.f;
    if (w < live) {
      load_x2(xq, g.s, (size_t)col, ns, KB, q, valid);
      const float av = valid ? g.a[col] : 0.f, rv = valid ? g.r[col] : 0.f;
      set_row2(xq, ns, av, q);
      layer1_keep<MT, KB>(h1, xq, SC, lr, q);
      const float qv = head<MT>(h1, SC.w2, SC.b2[0], q);
      const float c = valid ? tgj - qv : 0.f;
      dq = valid ? -(2.f / (float)g.Bu) * ((g.quirk ? rbar : rv) + c) : 0.f;
      if (valid && q == 0) { sv[0] += c; sv[1] += c * c; sv[2] += rv; sv[3] += rv * rv; sv[4] += (rv + c) * (rv + c); }
    } else {                                    // a wave without columns in this chunk contributes zeros
#pragma unroll
      for (int blk = 0; blk < K2MAX; ++blk) { xq[blk][0] = 0.f; xq[blk][1] = 0.f; }
      zero_(h1);
    }
    __syncthreads();                            // the previous chunk's tiles have been consumed
    out_row_grad<MT>(h1, dq, g.C.H, redA, dacc, tid);      // dW2 / db2
    // dz1 in place; dW1 / db1 += dz1 x [x; 1]^T over the 128 columns (four 32-column quarters)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float* wv = SC.w2 + 16 * m + 4 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r) h1[m][r] = h1[m][r] > 0.f ? wv[r] * dq : 0.f;
    }
    for (int qq = 0; 2 * qq < live; ++qq) {     // (a quarter = the columns of waves 2 qq, 2 qq + 1)
      __syncthreads();
      if ((w >> 1) == qq) {
        stage_rows_ld<MT>(Lm, LDQ, h1, cw, q, -1);
        stage_x2<LDQ>(Rm, xq, xrows, cw, q, w < live ? K0 : -1);      // (no bias-gradient ones in a dead wave's columns)
      }
      __syncthreads();
      gemm_cols<NACC, LDQ, 2>(acc, Lm, Rm, MT, nR, w, lr, q);
    }
  }
  const int nslab = gridDim.x;
  store_pass(acc, g.slab, nslab, MT, MT, nR, w, l);
  __syncthreads();
  store_row(dacc, HP, g.slab, nslab, 0, tid);
  // ---- loss statistics
#pragma unroll
  for (int k = 0; k < 5; ++k)
    for (int off = 32; off > 0; off >>= 1) sv[k] += __shfl_xor(sv[k], off);
  if (l == 0)
    for (int k = 0; k < 5; ++k) red5[w * 8 + k] = sv[k];
  __syncthreads();
  if (tid < 8) {
    float* st = g.slab + ((size_t)stats2_chunk(MT, nR) * nslab + blockIdx.x) * 64;
    float a = 0.f;
    if (tid < 5)
      for (int ww = 0; ww < FTHREADS / 64; ++ww) a += red5[ww * 8 + tid];
    st[tid] = a;
  }
}

}  // namespace pdec
