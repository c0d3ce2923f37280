// fused2_finish.hpp -- the finish launch of a fused 2-layer pass: deterministic sum of the per-workgroup slabs into the flat
// gradient buffer, loss finalisation and -- when it applies the update -- ADAM and Polyak on the flat parameters (the passes
// read those, so there is no image to refresh); and the apply launch behind an external all-reduce
#pragma once
#include "fused2_layers.hpp"

namespace pdec {

struct Finish2Args {
  const float* slabs;
  int nslab, K0, H, MT, nR;
  float* grads;
  float scale;
  int mode, Bu, quirk;
  float* loss_out;
  const float* loss_add;      // != null: device scalar added to the critic loss (reward groups, reward_group_route)
  int apply;
  float *p, *m, *v, *pt;
  double eta, b1, b2, eps, omb1p, omb2p;   // omb*p = 1 - beta^t: filled in by the kernels from `bp` (device resident)
  BpArgs bp;
  float rho, omr;
};

// Flux.Optimise.ADAM in Float64 (src/custom_nna.jl:23-24) and dest = rho dest + (1 - rho) src (src/PDEagent.jl:415-417);
// the same arithmetic, without FMA contraction, as adam_kernel / polyak_kernel (mlp.hip)
__device__ __forceinline__ void finish2_param(const Finish2Args& g, int i, float gi) {
#pragma clang fp contract(off)
  const double gd = (double)gi;
  const float mt = (float)(g.b1 * (double)g.m[i] + (1.0 - g.b1) * gd);
  const float vt = (float)(g.b2 * (double)g.v[i] + (1.0 - g.b2) * gd * gd);
  g.m[i] = mt;
  g.v[i] = vt;
  const float delta = (float)((double)mt / g.omb1p / (sqrt((double)vt / g.omb2p) + g.eps) * g.eta);
  const float pn = g.p[i] - delta;
  g.p[i] = pn;
  if (g.pt) g.pt[i] = g.rho * g.pt[i] + g.omr * pn;
}

// Flat parameter index of element `l` (lane order) of chunk (tile T, register r) of a slab, -1 for padding: tiles are numbered
// as slab2_tiles() lists them (fused2_layers.hpp), element (r, l) of a tile is row 4 (l >> 4) + r, column l & 15 (store_pass)
__device__ __forceinline__ int flat2_of_chunk(int K0, int H, int MT, int nR, int T, int r, int l) {
  const Flat2Offsets o = flat2_offsets(K0, H);
  const int q = l >> 4, lr = l & 15;
  int i = -1;
  if (T < MT) {                                  // dW2 / db2: only row 0 of the [16][HP] product is real
    const int row = 4 * q + r, col = 16 * T + lr;
    if (row == 0) i = col < H ? o.W2 + col : (col == H ? o.b2 : -1);
  } else {                                       // dW1 / db1
    const int u = T - MT, ti = u / nR, tk = u - ti * nR;
    const int row = 16 * ti + 4 * q + r, col = 16 * tk + lr;
    if (row < H) i = col < K0 ? row * K0 + col : (col == K0 ? o.b1 + row : -1);
  }
  return i;
}

// one block per chunk: 64 chunk elements x 16 slab groups, fixed-order combine -> deterministic
__global__ __launch_bounds__(1024) void finish2_kernel(Finish2Args g_in) {
  Finish2Args g = g_in;
  if (g.apply) {      // beta powers from device memory; one thread of the grid writes the advanced pair
    g.omb1p = 1.0 - g.bp.cur[0];
    g.omb2p = 1.0 - g.bp.cur[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) bp_advance(g.bp, g.b1, g.b2);
  }
  __shared__ float part[16][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int MT = g.MT, nR = g.nR;
  const int c = blockIdx.x, T = c >> 2, r = c & 3;
  const int i = flat2_of_chunk(g.K0, g.H, MT, nR, T, r, tx);   // this thread's chunk element (-1: padding)
  if (__syncthreads_or(i >= 0)) {
    float acc = 0.f;
    if (i >= 0) {
      const float* sp = g.slabs + (size_t)c * g.nslab * 64 + tx;
      int z = ty;
      for (; z + 240 < g.nslab; z += 256) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = sp[(size_t)(z + 16 * u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
      }
      for (; z < g.nslab; z += 16) acc += sp[(size_t)z * 64];
    }
    part[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && i >= 0) {
      float a = 0.f;
      for (int k = 0; k < 16; ++k) a += part[k][tx];
      a *= g.scale;
      g.grads[i] = a;
      if (g.apply) finish2_param(g, i, a);
    }
  }
  if (blockIdx.x == 0 && g.loss_out) {
    __shared__ double red[5][256];
    const int tid = threadIdx.x;
    const float* stc = g.slabs + (size_t)stats2_chunk(MT, nR) * g.nslab * 64;
    double st[5] = {0, 0, 0, 0, 0};
    if (tid < 256) {
      for (int z = tid; z < g.nslab; z += 256)
        for (int k = 0; k < 5; ++k) st[k] += (double)stc[(size_t)z * 64 + k];
      for (int k = 0; k < 5; ++k) red[k][tid] = st[k];
    }
    __syncthreads();
    for (int sft = 128; sft > 0; sft >>= 1) {
      if (tid < sft)
        for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + sft];
      __syncthreads();
    }
    if (tid == 0) {
      const double inv = 1.0 / g.Bu;
      if (g.mode == 0)
        *g.loss_out = (float)(g.quirk ? red[1][0] * inv + 2.0 * (red[0][0] * inv) * (red[2][0] * inv) + red[3][0] * inv
                                      : red[4][0] * inv + (g.loss_add ? (double)*g.loss_add : 0.0));
      else
        *g.loss_out = (float)(-red[0][0] * inv);
    }
  }
}

// ADAM + Polyak from the flat gradient buffer (after an external all-reduce): same arithmetic as the fused finish
__global__ void apply2_kernel(Finish2Args g_in, int n) {
  Finish2Args g = g_in;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  g.omb1p = 1.0 - g.bp.cur[0];
  g.omb2p = 1.0 - g.bp.cur[1];
  if (i == 0) bp_advance(g.bp, g.b1, g.b2);
  if (i < n) finish2_param(g, i, g.grads[i]);
}

}  // namespace pdec
