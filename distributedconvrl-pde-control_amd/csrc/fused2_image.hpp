// fused2_image.hpp -- the padded LDS image of one reference-shaped 2-layer net [K0, H, 1] that the fused 2-layer kernels build
// from the FLAT parameters (mlp_mfma2.hip is the translation unit; no padded copy is kept in HBM), and the ONE statement of the
// flat layout that the image loads and the finish kernel share.
#pragma once
#include "common.hpp"
#include "mfma_blocks.hpp"

namespace pdec {

struct Net2 {              // flat parameters [W1 [H][K0] row-major, b1 [H], W2 [1][H], b2 [1]]
  const float* p;
  int K0, H, kb;           // kb = ceil(K0 / 8) k-blocks are multiplied; the image row stride is a template constant
};

// the flat parameter (and gradient) layout [W1 [H][K0], b1 [H], W2 [1][H], b2]: where each array starts, and the count
struct Flat2Offsets {
  int b1, W2, b2, n;       // (W1 starts at 0)
};
__host__ __device__ __forceinline__ Flat2Offsets flat2_offsets(int K0, int H) {
  Flat2Offsets o;
  o.b1 = H * K0; o.W2 = o.b1 + H; o.b2 = o.W2 + H; o.n = o.b2 + 1;
  return o;
}

// LDS image of a net: W1 [HP][ldk] (ldk = 8 KB + 4: k-blocks of 8 and one pad slot), b1 [HP], w2 [HP], b2 [4]
struct Lds2 {
  float *W1, *b1, *w2, *b2;
};
__host__ __device__ constexpr int lds2_floats(int HP, int ldk) { return HP * ldk + 2 * HP + 4; }
__device__ __forceinline__ Lds2 carve2(float* base, int HP, int ldk) {
  Lds2 s;
  s.W1 = base; s.b1 = base + HP * ldk; s.w2 = s.b1 + HP; s.b2 = s.w2 + HP;
  return s;
}

// flat parameters -> padded LDS image: the H*K0 weights are streamed with 16-byte loads (8 in flight per lane) and
// scattered to their padded rows; the pad cells are zeroed by separate stores (disjoint addresses, no ordering needed)
__device__ __forceinline__ void load_net2(const Lds2& s, const Net2& n, int HP, int ldk, int tid) {
  const int K0 = n.K0, H = n.H;
  const Flat2Offsets o = flat2_offsets(K0, H);
  const int nw = o.b1;
  const int n4 = ((reinterpret_cast<uintptr_t>(n.p) & 15) == 0) ? nw / 4 : 0;
  const f32x4* w4 = reinterpret_cast<const f32x4*>(n.p);
  auto put = [&](int idx, float v) {
    const int r = idx / K0;
    s.W1[r * ldk + (idx - r * K0)] = v;
  };
  int i = tid;
  for (; i + 7 * FTHREADS < n4; i += 8 * FTHREADS) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = w4[i + u * FTHREADS];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) put(4 * (i + u * FTHREADS) + e, v[u][e]);
  }
  for (; i < n4; i += FTHREADS) {
    const f32x4 v = w4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) put(4 * i + e, v[e]);
  }
  for (int k = 4 * n4 + tid; k < nw; k += FTHREADS) put(k, n.p[k]);
  const int padc = ldk - K0;
  for (int k = tid; k < H * padc; k += FTHREADS) { const int r = k / padc; s.W1[r * ldk + K0 + (k - r * padc)] = 0.f; }
  for (int k = tid; k < (HP - H) * ldk; k += FTHREADS) s.W1[H * ldk + k] = 0.f;
  const float* b1 = n.p + (size_t)o.b1;      // W2 and b2 are indexed from b1: another form changes the passes' instruction streams
  for (int k = tid; k < HP; k += FTHREADS) {
    s.b1[k] = k < H ? b1[k] : 0.f;
    s.w2[k] = k < H ? b1[o.W2 - o.b1 + k] : 0.f;
  }
  if (tid == 0) s.b2[0] = b1[o.b2 - o.b1];
}

}  // namespace pdec
