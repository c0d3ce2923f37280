// fused2_layers.hpp -- what the fused 2-layer kernels share besides the image: the first-layer products, the input rows of a
// lane and their staging, the column GEMM of the weight gradients, the output row's gradient, the arguments of the two passes
// and the slab's tile numbering
#pragma once
#include "fused2_image.hpp"

namespace pdec {

#ifndef K2MAX              // k-blocks of 8 input rows: one of the family's shape constants, stated with the tile lists in mlp_mfma2.hip
#error "fused2_layers.hpp is part of the translation unit mlp_mfma2.hip, which defines K2MAX ahead of it"
#endif

#define LDQ 40             // leading dim of the 32-column staging images (8 mod 16 floats: conflict-free ds_read_b128)

// ---- the first layer out of the image, three forms.  Each repeats the bias load and the KB-block chain of one tile pair ON
// PURPOSE: every helper that was tried for the shared part changed the instruction streams of the passes ("The
// 2-layer family by subject", has the forms and what each changed), so a change to the chain is made three times.

// first layer: h = relu(W1 x + b1), tiles kept (D layout)
template <int MT, int KB>
__device__ __forceinline__ void layer1_keep(f32x4 (&h)[MT], const float (&x)[K2MAX][2], const Lds2& s, int lr, int q) {
  constexpr int ldk = 8 * KB + 4;
#pragma unroll
  for (int mo = 0; mo < MT; mo += 2) {
    const bool two = mo + 1 < MT;
    const float* b = s.b1 + 16 * mo + 4 * q;
    f32x4 a0 = {b[0], b[1], b[2], b[3]};
    f32x4 a1 = two ? f32x4{b[16], b[17], b[18], b[19]} : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* w0 = s.W1 + (16 * mo + lr) * ldk + 2 * q;
    const float* w1 = w0 + 16 * ldk;
#pragma unroll
    for (int blk = 0; blk < KB; ++blk) {
        const float2 wa = *reinterpret_cast<const float2*>(w0 + 8 * blk);
        a0 = mfma4(wa.x, x[blk][0], a0);
        if (two) {
          const float2 wb = *reinterpret_cast<const float2*>(w1 + 8 * blk);
          a1 = mfma4(wb.x, x[blk][0], a1);
          a0 = mfma4(wa.y, x[blk][1], a0);
          a1 = mfma4(wb.y, x[blk][1], a1);
        } else {
          a0 = mfma4(wa.y, x[blk][1], a0);
        }
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) a0[r] = fmaxf(a0[r], 0.f);
    h[mo] = a0;
    if (two) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a1[r] = fmaxf(a1[r], 0.f);
      h[mo + 1] = a1;
    }
  }
}

// first layer + output row without keeping the tiles: returns w2 . relu(W1 x + b1) + b2 (every lane of a column)
template <int MT, int KB>
__device__ __forceinline__ float layer1_head(const float (&x)[K2MAX][2], const Lds2& s, int lr, int q) {
  constexpr int ldk = 8 * KB + 4;
  float acc = 0.f;
#pragma unroll
  for (int mo = 0; mo < MT; mo += 2) {
    const bool two = mo + 1 < MT;
    const float* b = s.b1 + 16 * mo + 4 * q;
    f32x4 a0 = {b[0], b[1], b[2], b[3]};
    f32x4 a1 = two ? f32x4{b[16], b[17], b[18], b[19]} : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* w0 = s.W1 + (16 * mo + lr) * ldk + 2 * q;
    const float* w1 = w0 + 16 * ldk;
#pragma unroll
    for (int blk = 0; blk < KB; ++blk) {
        const float2 wa = *reinterpret_cast<const float2*>(w0 + 8 * blk);
        a0 = mfma4(wa.x, x[blk][0], a0);
        if (two) {
          const float2 wb = *reinterpret_cast<const float2*>(w1 + 8 * blk);
          a1 = mfma4(wb.x, x[blk][0], a1);
          a0 = mfma4(wa.y, x[blk][1], a0);
          a1 = mfma4(wb.y, x[blk][1], a1);
        } else {
          a0 = mfma4(wa.y, x[blk][1], a0);
        }
      }
    const float* wv = s.w2 + 16 * mo + 4 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc += wv[r] * fmaxf(a0[r], 0.f);
    if (two) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc += wv[16 + r] * fmaxf(a1[r], 0.f);
    }
  }
  acc += __shfl_xor(acc, 16);
  acc += __shfl_xor(acc, 32);
  return acc + s.b2[0];
}

// critic forward inside the actor pass: q partial = w2 . relu(W1 x + b1) and the input-gradient partial
// da = sum_i W1[i][ns] * relu'(z_i) * w2_i of this lane's rows, tile pair by tile pair (no tile is kept)
template <int MT, int KB>
__device__ __forceinline__ void layer1_head_da(const float (&x)[K2MAX][2], const Lds2& s, int ns, int lr, int q, float& qacc,
                                               float& da) {
  constexpr int ldk = 8 * KB + 4;
#pragma unroll
  for (int mo = 0; mo < MT; mo += 2) {
    const bool two = mo + 1 < MT;
    const float* b = s.b1 + 16 * mo + 4 * q;
    f32x4 a0 = {b[0], b[1], b[2], b[3]};
    f32x4 a1 = two ? f32x4{b[16], b[17], b[18], b[19]} : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* w0 = s.W1 + (16 * mo + lr) * ldk + 2 * q;
    const float* w1 = w0 + 16 * ldk;
#pragma unroll
    for (int blk = 0; blk < KB; ++blk) {
        const float2 wa = *reinterpret_cast<const float2*>(w0 + 8 * blk);
        a0 = mfma4(wa.x, x[blk][0], a0);
        if (two) {
          const float2 wb = *reinterpret_cast<const float2*>(w1 + 8 * blk);
          a1 = mfma4(wb.x, x[blk][0], a1);
          a0 = mfma4(wa.y, x[blk][1], a0);
          a1 = mfma4(wb.y, x[blk][1], a1);
        } else {
          a0 = mfma4(wa.y, x[blk][1], a0);
        }
      }
    {   // unconditional operand loads (a select, not a branch around the load)
      const int row0 = 16 * mo + 4 * q;
      const f32x4 wv = *reinterpret_cast<const f32x4*>(s.w2 + row0);
      const float* wc = s.W1 + row0 * ldk + ns;
      const float c0 = wc[0], c1 = wc[ldk], c2 = wc[2 * ldk], c3 = wc[3 * ldk];
      const float cc[4] = {c0, c1, c2, c3};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        qacc += wv[r] * fmaxf(a0[r], 0.f);
        const float t = cc[r] * wv[r];
        da += a0[r] > 0.f ? t : 0.f;
      }
      if (two) {
        const f32x4 wv1 = *reinterpret_cast<const f32x4*>(s.w2 + row0 + 16);
        const float* wc1 = wc + 16 * ldk;
        const float d0 = wc1[0], d1 = wc1[ldk], d2 = wc1[2 * ldk], d3 = wc1[3 * ldk];
        const float dd[4] = {d0, d1, d2, d3};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          qacc += wv1[r] * fmaxf(a1[r], 0.f);
          const float t = dd[r] * wv1[r];
          da += a1[r] > 0.f ? t : 0.f;
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the scheduler from hoisting every tile pair's operand loads (spills)
  }
}

// input rows of a lane: x[blk][t] = X[8 blk + 2 q + t][col]; rows < ns from `s`, 0 above (the action row is set by set_row2)
__device__ __forceinline__ void load_x2(float (&x)[K2MAX][2], const float* __restrict__ s, size_t col, int ns, int kb, int q,
                                        bool valid) {
#pragma unroll
  for (int blk = 0; blk < K2MAX; ++blk)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = 8 * blk + 2 * q + t;
      x[blk][t] = (valid && blk < kb && row < ns) ? s[col * ns + row] : 0.f;
    }
}
__device__ __forceinline__ void set_row2(float (&x)[K2MAX][2], int row, float v, int q) {
#pragma unroll
  for (int blk = 0; blk < K2MAX; ++blk)
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (8 * blk + 2 * q + t == row) x[blk][t] = v;
}
// write the lane's input rows into a [row][LD] staging image (row `ones_row` := 1: the bias gradient rides the GEMM)
template <int LD>
__device__ __forceinline__ void stage_x2(float* img, const float (&x)[K2MAX][2], int nrows, int cw, int q, int ones_row) {
#pragma unroll
  for (int blk = 0; blk < K2MAX; ++blk)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = 8 * blk + 2 * q + t;
      if (row < nrows) img[row * LD + cw] = row == ones_row ? 1.f : x[blk][t];
    }
}

// D[i][k] += sum over NC16 * 16 staged columns L[i][c] * R[k][c] (images [row][LD]); wave w takes tiles w, w+8, ...
template <int NACC, int LD, int NC16>
__device__ __forceinline__ void gemm_cols(f32x4 (&acc)[NACC], const float* L, const float* R, int nL, int nR, int w, int lr,
                                          int q) {
#pragma unroll
  for (int pp = 0; pp < NACC; ++pp) {
    const int p = w + 8 * pp;
    if (p < nL * nR) {
      const int ti = p / nR, tk = p - ti * nR;
      const float* lrow = L + (16 * ti + lr) * LD + 4 * q;
      const float* rrow = R + (16 * tk + lr) * LD + 4 * q;
      acc[pp] = tile_chain<NC16>(acc[pp], lrow, rrow);
    }
    // keep the scheduler from hoisting the next tiles' operand loads over this tile (register pressure: the activations are
    // live here); the partner wave on the SIMD hides the LDS latency
    __builtin_amdgcn_sched_barrier(0);
  }
}

// output-row gradient dW2/db2 += sum_cols g[col] * [h; 1]: DPP sum over a wave's 16 columns, LDS over the 8 waves,
// accumulated over the workgroup's chunks in dacc [HP] (fixed order -> deterministic)
template <int MT>
__device__ __forceinline__ void out_row_grad(const f32x4 (&h)[MT], float g, int H, float* redA, float* dacc, int tid) {
  const int w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4, HP = 16 * MT;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * m + 4 * q + r;
      const float v = row_sum16((row == H ? 1.f : h[m][r]) * g);
      if (lr == 0) redA[w * HP + row] = v;
    }
  __syncthreads();
  for (int i = tid; i < HP; i += FTHREADS) {
    float a = dacc[i];
#pragma unroll
    for (int ww = 0; ww < FTHREADS / 64; ++ww) a += redA[ww * HP + i];
    dacc[i] = a;
  }
}
__device__ __forceinline__ void store_row(const float* dacc, int HP, float* slab, int nslab, int T0, int tid) {
  for (int i = tid; i < HP; i += FTHREADS)
    slab[((size_t)(4 * (T0 + (i >> 4))) * nslab + blockIdx.x) * 64 + (i & 15)] = dacc[i];   // tile i/16, register 0, lane i%16
}

// One argument block serves both passes; a launch sets the fields its pass reads and leaves the rest zero:
//   critic pass: At, Ct, C | s, a, r, t, sn | Bu, ns, gamma, quirk, rbar (quirk only) | slab, tpw
//   actor pass:  A, C | s | Bu, ns | slab, tpw
struct Fused2Args {
  Net2 A, C, At, Ct;
  const float *s, *a, *r, *t, *sn;
  int Bu, ns;
  float gamma;
  int quirk;
  float* slab;
  const float* rbar;          // device scalar: mean reward (quirk) written by rmean_kernel
  int tpw;                    // wave tiles (16 columns) per workgroup: workgroup b owns tiles [b tpw, (b + 1) tpw) (grid2_of)
};

// Slab tiles of a 2-layer net with K0 inputs (chunk-major slab of store_pass, mfma_blocks.hpp): tiles [0, MT) are dW2 / db2 as a
// [16][HP] product of which row 0 is real (store_row), tiles MT + ti nR + tk the [HP][16 nR] product dW1 / db1 (column K0 is
// db1: the ones row of the staged inputs), then one chunk of loss statistics.  flat2_of_chunk (fused2_finish.hpp) is the inverse.
__host__ __device__ inline int nr_of(int K0) { return (K0 + 1 + 15) / 16; }
__host__ __device__ inline int slab2_tiles(int MT, int nR) { return MT + MT * nR; }
__host__ __device__ inline int stats2_chunk(int MT, int nR) { return 4 * slab2_tiles(MT, nR); }
static inline size_t slab2_floats(int MT, int nR, int nslab) { return ((size_t)stats2_chunk(MT, nR) + 1) * nslab * 64; }

}  // namespace pdec
