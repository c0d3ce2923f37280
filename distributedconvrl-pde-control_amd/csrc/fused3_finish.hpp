// fused3_finish.hpp -- the finish launch of a fused 3-layer pass: deterministic sum of the per-workgroup slabs into the flat
// gradient buffer (replicas stay bit-identical), loss finalisation, and -- when it applies the update -- ADAM, Polyak and the
// refresh of the padded images, all in one kernel
#pragma once
#include "fused3_layers.hpp"

namespace pdec {

struct FinishArgs {
  const float* slabs;          // chunk-major per-workgroup partial gradients (store_pass)
  int nslab, K0, H, MT;
  float* grads;                // flat gradient buffer (written when nslab > 0, read when nslab == 0)
  float scale;
  int mode, Bu, quirk;         // loss finalisation (mode 0 critic, 1 actor)
  float* loss_out;
  const float* loss_add;       // != null: device scalar added to the critic loss (reward groups, reward_group_route)
  int apply;                   // != 0: ADAM step on p, Polyak into pt, refresh the padded images
  float *p, *m, *v, *pt, *fw, *fwt;
  float* fwp;                  // published copy of the updated image (double-buffered: a concurrent acting kernel
                               // keeps reading the other copy), may be null
  FNet lay;
  double eta, b1, b2, eps, omb1p, omb2p;   // omb*p = 1 - beta^t: filled in by the kernel from `bp` (device resident)
  BpArgs bp;
  float rho, omr;
  int prio;                    // wave priority (the update chain is the critical path: same level as the passes)
};

// Flux.Optimise.ADAM (Float64 arithmetic, as the broadcast promotes; src/custom_nna.jl:23-24), then
// dest = rho dest + (1-rho) src (src/PDEagent.jl:415-417) for this one parameter, and its copies in the
// padded LDS images the fused passes stage from (so no separate prep launch is needed)
__device__ __forceinline__ void finish_param(const FinishArgs& g, int i, float gi, float p0, float m0, float v0, float pt0) {
  // no FMA contraction: Julia evaluates these broadcasts with separate multiplies and adds, and the two call
  // sites of this function (fused reduce+apply, apply after an all-reduce) must round identically
#pragma clang fp contract(off)
  const double gd = (double)gi;
  const float mt = (float)(g.b1 * (double)m0 + (1.0 - g.b1) * gd);
  const float vt = (float)(g.b2 * (double)v0 + (1.0 - g.b2) * gd * gd);
  g.m[i] = mt;
  g.v[i] = vt;
  const float delta = (float)((double)mt / g.omb1p / (sqrt((double)vt / g.omb2p) + g.eps) * g.eta);
  const float pn = p0 - delta;
  g.p[i] = pn;
  const ImagePos at = image_of_flat(g.lay, i);
  const int o1 = at.o1, o2 = at.o2;
  if (g.fw) { g.fw[o1] = pn; if (o2 >= 0) g.fw[o2] = pn; }
  if (g.fwp) { g.fwp[o1] = pn; if (o2 >= 0) g.fwp[o2] = pn; }
  if (g.pt) {
    const float tn = g.rho * pt0 + g.omr * pn;
    g.pt[i] = tn;
    if (g.fwt) {
      g.fwt[o1] = tn; if (o2 >= 0) g.fwt[o2] = tn;
    }
  }
}

// Flat parameter index of element `l` (lane order) of chunk (tile T, register r) of a slab, -1 for padding: tiles are
// numbered as slab_tiles() lists them, element (r, l) of a tile is row 4 (l >> 4) + r, column l & 15 (store_pass).
__device__ __forceinline__ int flat_of_chunk(int K0, int H, int MT, int T, int r, int l) {
  const FlatOffsets o = flat_offsets(K0, H);
  const int q = l >> 4, lr = l & 15;
  int i = -1;
  if (T < MT) {                                  // dW3 / db3: only row 0 of the [16][HP] product is real
    const int row = 4 * q + r, col = 16 * T + lr;
    if (row == 0) i = col < H ? o.W3 + col : (col == H ? o.b3 : -1);
  } else if (T < MT + MT * MT) {                 // dW2 / db2
    const int u = T - MT, ti = u / MT, tk = u - ti * MT;
    const int row = 16 * ti + 4 * q + r, col = 16 * tk + lr;
    if (row < H) i = col < H ? o.W2 + row * H + col : (col == H ? o.b2 + row : -1);
  } else {                                       // dW1 / db1
    const int ti = T - MT - MT * MT;
    const int row = 16 * ti + 4 * q + r, col = lr;
    if (row < H) i = col < K0 ? row * K0 + col : (col == K0 ? o.b1 + row : -1);
  }
  return i;
}

// the loss from the five sums of the statistics chunk over the batch: sum c, sum c^2, sum r, sum r^2, sum (r + c)^2 with
// c = target - q (critic pass); s0 = sum q (actor pass)
__device__ __forceinline__ float finish_loss(const FinishArgs& g, double s0, double s1, double s2, double s3, double s4) {
  const double inv = 1.0 / g.Bu;
  if (g.mode == 0)   // critic: quirk -> mean(c^2) + 2 mean(c) mean(r) + mean(r^2); else mean((r+c)^2)
    return (float)(g.quirk ? s1 * inv + 2.0 * (s0 * inv) * (s2 * inv) + s3 * inv
                           : s4 * inv + (g.loss_add ? (double)*g.loss_add : 0.0));
  return (float)(-s0 * inv);   // actor: -mean(q)
}

// The bit-identity reference of fused_finish_kernel below (PDEC_FINISH_REF=1 selects it; tests only): one block per chunk.
// grid: nslab > 0 -> one block per chunk (4 * slab_tiles(MT)); nslab == 0 -> ceil(n / 64) blocks (apply from grads).
// block = 64 chunk elements x 16 slab groups (1024 threads): each thread sums every 16th slab (16 loads in flight,
// a contiguous 256-B row each), then a fixed-order combine over the groups -> deterministic, so data-parallel
// replicas stay bit-identical.
__global__ __launch_bounds__(1024) void fused_finish_ref_kernel(FinishArgs g_in) {
  FinishArgs g = g_in;
  set_wave_prio(g.prio);
  if (g.apply) {      // the beta powers come from device memory; one thread of the grid writes the advanced pair
    g.omb1p = 1.0 - g.bp.cur[0];
    g.omb2p = 1.0 - g.bp.cur[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) bp_advance(g.bp, g.b1, g.b2);
  }
  __shared__ float part[16][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int K0 = g.K0, H = g.H, MT = g.MT;
  if (g.nslab > 0) {
    const int c = blockIdx.x, T = c >> 2, r = c & 3;
    const int i = flat_of_chunk(K0, H, MT, T, r, tx);   // this thread's chunk element (-1: padding)
    if (__syncthreads_or(i >= 0)) {
      float p0 = 0.f, m0 = 0.f, v0 = 0.f, pt0 = 0.f;
      if (g.apply && ty == 0 && i >= 0) {            // issue the parameter loads before the slab stream
        p0 = g.p[i]; m0 = g.m[i]; v0 = g.v[i];
        if (g.pt) pt0 = g.pt[i];
      }
      float acc = 0.f;
      if (i >= 0) {
        const float* sp = g.slabs + (size_t)c * g.nslab * 64 + tx;
        int z = ty;
        for (; z + 240 < g.nslab; z += 256) {
          float v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = PDEC_SLAB_LOAD(&sp[(size_t)(z + 16 * u) * 64]);
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
        if (g.apply) finish_param(g, i, a, p0, m0, v0, pt0);
      }
    }
  } else {
    const int i = blockIdx.x * 64 + tx;
    if (ty == 0 && i < flat_offsets(K0, H).n && g.apply) finish_param(g, i, g.grads[i], g.p[i], g.m[i], g.v[i], g.pt ? g.pt[i] : 0.f);
  }
  if (blockIdx.x == 0 && g.loss_out && g.nslab > 0) {   // block 0 also finalises the loss (fixed-order tree -> deterministic)
    __shared__ double red[5][256];
    const int tid = threadIdx.x;
    const float* stc = g.slabs + (size_t)stats_chunk(MT) * g.nslab * 64;
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
    if (tid == 0) *g.loss_out = finish_loss(g, red[0][0], red[1][0], red[2][0], red[3][0], red[4][0]);
  }
}

// Slab reduction + parameter update.  The summation tree of every gradient element is the one of the reference kernel above
// -- 16 partial sums over the slabs z = k, k + 16, k + 32, ... in that order, combined in the order k = 0 .. 15 -- so
// parameters are bit-identical to it; the work is cut differently (DESIGN.md 3.2 has the arithmetic):
//   * one block per HALF chunk (32 elements x nslab slabs = 128 contiguous bytes per slab row);
//   * 128 threads per block = 16 slab groups x 8 lanes, every lane loads 16 B (four elements of a slab row) and keeps
//     16 such loads in flight;
//   * all blocks of a grid are co-resident.
// grid: nslab > 0 -> 8 * slab_tiles(MT) blocks; nslab == 0 -> ceil(n / 128) blocks (apply from the gradient buffer).
#define FIN_THREADS 128
// the work of block `bx` of a finish grid with the launch arguments g_in
__device__ __forceinline__ void finish_block(const FinishArgs& g_in, const unsigned bx) {
  FinishArgs g = g_in;
  set_wave_prio(g.prio);
  if (g.apply) {      // the beta powers come from device memory; one thread of the grid writes the advanced pair
    g.omb1p = 1.0 - g.bp.cur[0];
    g.omb2p = 1.0 - g.bp.cur[1];
    if (bx == 0 && threadIdx.x == 0) bp_advance(g.bp, g.b1, g.b2);
  }
  __shared__ float part[16][36];
  const int tid = threadIdx.x;
  const int K0 = g.K0, H = g.H, MT = g.MT;
  if (g.nslab > 0) {
    const int c = bx >> 1, half = bx & 1, T = c >> 2, r = c & 3;
    // the chunk element this thread finishes (threads 0 .. 31; -1: padding)
    const int i = tid < 32 ? flat_of_chunk(K0, H, MT, T, r, 32 * half + tid) : -1;
    if (__syncthreads_or(i >= 0)) {
      float p0 = 0.f, m0 = 0.f, v0 = 0.f, pt0 = 0.f;
      if (g.apply && i >= 0) {                       // issue the parameter loads before the slab stream
        p0 = g.p[i]; m0 = g.m[i]; v0 = g.v[i];
        if (g.pt) pt0 = g.pt[i];
      }
      const int tx4 = tid & 7, ty = tid >> 3;        // 16-byte lane inside the 128-byte half row, slab group
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      {
        const f32x4* sp = reinterpret_cast<const f32x4*>(g.slabs + (size_t)c * g.nslab * 64 + 32 * half) + tx4;   // row stride: 16 float4
        int z = ty;
        for (; z + 240 < g.nslab; z += 256) {
          f32x4 v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = PDEC_SLAB_LOAD(&sp[(size_t)(z + 16 * u) * 16]);
#pragma unroll
          for (int u = 0; u < 16; ++u) acc += v[u];
        }
        for (; z < g.nslab; z += 16) acc += sp[(size_t)z * 16];
      }
      *reinterpret_cast<f32x4*>(&part[ty][4 * tx4]) = acc;
      __syncthreads();
      if (i >= 0) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) a += part[k][tid];
        a *= g.scale;
        g.grads[i] = a;
        if (g.apply) finish_param(g, i, a, p0, m0, v0, pt0);
      }
    }
  } else {
    const int i = bx * FIN_THREADS + tid;
    if (i < flat_offsets(K0, H).n && g.apply) finish_param(g, i, g.grads[i], g.p[i], g.m[i], g.v[i], g.pt ? g.pt[i] : 0.f);
  }
  if (bx == 0 && g.loss_out && g.nslab > 0) {   // block 0 also finalises the loss (fixed-order tree -> deterministic)
    // the reference kernel's tree: 256 strided partial sums, pairwise tree 128, 64, ..., 1 -- thread t owns partials t and t + 128
    // and starts with their sum (= the tree's first level)
    __shared__ double red[5][FIN_THREADS];
    const float* stc = g.slabs + (size_t)stats_chunk(MT) * g.nslab * 64;
    double st[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
    for (int hh = 0; hh < 2; ++hh)
      for (int z = tid + 128 * hh; z < g.nslab; z += 256)
        for (int k = 0; k < 5; ++k) st[hh][k] += (double)stc[(size_t)z * 64 + k];
    for (int k = 0; k < 5; ++k) red[k][tid] = st[0][k] + st[1][k];
    __syncthreads();
    for (int sft = 64; sft > 0; sft >>= 1) {
      if (tid < sft)
        for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + sft];
      __syncthreads();
    }
    if (tid == 0) *g.loss_out = finish_loss(g, red[0][0], red[1][0], red[2][0], red[3][0], red[4][0]);
  }
}

__global__ __launch_bounds__(FIN_THREADS) void fused_finish_kernel(FinishArgs g_in) {
  finish_block(g_in, blockIdx.x);
}

// Two finish grids in one launch: blocks [0, nc) are the grid of c, blocks [nc, gridDim.x) the grid of a, each block doing
// what it does in a launch of its own (block 0 of either grid finalises that grid's loss), so both nets end bit-identical to
// two launches.  For the critic's finish of update k + 1 and the actor's of update k under frozen targets, which touch
// disjoint memory.
__global__ __launch_bounds__(FIN_THREADS) void fused_finish_pair_kernel(FinishArgs c_in, FinishArgs a_in, int nc) {
  if ((int)blockIdx.x < nc) finish_block(c_in, blockIdx.x);
  else finish_block(a_in, blockIdx.x - nc);
}

}  // namespace pdec
