// fused3_image.hpp -- the padded weight image of one 3-layer net [K0, H, H, 1] that the fused 3-layer kernels stage into LDS
// (mlp_mfma.hip is the translation unit), the ONE map between the flat parameters and the image, and the two kernels that
// walk the map in either direction.
#pragma once
#include "common.hpp"

namespace pdec {

#define LDWPAD 8           // weight-image row stride = HP + 8
#define LDW1 20            // LDS leading dim of W1 images
#ifndef KXP                // padded input rows: one of the family's shape constants, stated with the tile lists in mlp_mfma.hip
#error "fused3_image.hpp is part of the translation unit mlp_mfma.hip, which defines KXP ahead of it"
#endif

// The image is laid out exactly as the passes keep it in LDS: first the "small" block [W1 [HP][LDW1] | b1 [HP] | b2 [HP] |
// w3 [HP] | b3 [4]], then W2 [HP][LDW] and W2^T [HP][LDW], each block padded to a multiple of 256 floats, so that every block
// reaches LDS by asynchronous LDS-DMA in whole 1-KiB pieces (dma_even): no register round trip, no remainder.
struct FNet {
  const float* w;   // base
  int K0, H, HP, LDW;
  int oW1, ob1, ob2, ow3, ob3, oW2, oW2T, total;
  int nsmall, nbig;   // padded block sizes (floats, multiples of 256)
};
__host__ __device__ constexpr int pad256(int n) { return (n + 255) / 256 * 256; }
__host__ __device__ constexpr int small_floats(int HP) { return pad256(HP * LDW1 + 3 * HP + 4); }
__host__ __device__ constexpr int big_floats(int HP) { return pad256(HP * (HP + LDWPAD)); }

static FNet make_fnet_layout(int K0, int H) {
  FNet f{};
  f.K0 = K0; f.H = H;
  f.HP = (H + 1 + 15) / 16 * 16;
  f.LDW = f.HP + LDWPAD;
  f.nsmall = small_floats(f.HP); f.nbig = big_floats(f.HP);
  f.oW1 = 0;
  f.ob1 = f.HP * LDW1;
  f.ob2 = f.ob1 + f.HP;
  f.ow3 = f.ob2 + f.HP;
  f.ob3 = f.ow3 + f.HP;
  f.oW2 = f.nsmall;
  f.oW2T = f.oW2 + f.nbig;
  f.total = f.oW2T + f.nbig;
  return f;
}

// the internal flat parameter (and gradient) layout [W1 [H][K0], b1 [H], W2 [H][H], b2 [H], W3 [1][H], b3]: where each
// array starts, and the count
struct FlatOffsets {
  int b1, W2, b2, W3, b3, n;     // (W1 starts at 0)
};
__host__ __device__ __forceinline__ FlatOffsets flat_offsets(int K0, int H) {
  FlatOffsets o;
  o.b1 = H * K0; o.W2 = o.b1 + H; o.b2 = o.W2 + H * H; o.W3 = o.b2 + H; o.b3 = o.W3 + H; o.n = o.b3 + 1;
  return o;
}

// flat parameter index i (0 <= i < n) -> its offset in the image, and the offset of its twin in the W2^T block (-1: none)
struct ImagePos {
  int o1, o2;
};
__host__ __device__ __forceinline__ ImagePos image_of_flat(const FNet& f, int i) {
  const int K0 = f.K0, H = f.H;
  ImagePos p;
  p.o2 = -1;
  int j = i;
  if (j < H * K0) p.o1 = f.oW1 + (j / K0) * LDW1 + (j % K0);
  else if ((j -= H * K0) < H) p.o1 = f.ob1 + j;
  else if ((j -= H) < H * H) { p.o1 = f.oW2 + (j / H) * f.LDW + (j % H); p.o2 = f.oW2T + (j % H) * f.LDW + (j / H); }
  else if ((j -= H * H) < H) p.o1 = f.ob2 + j;
  else if ((j -= H) < H) p.o1 = f.ow3 + j;
  else p.o1 = f.ob3;
  return p;
}

// builds the padded image from the flat parameters: one thread per image float finds its parameter (the padding is written too)
__global__ void prep_fused_kernel(const float* __restrict__ p, float* __restrict__ out, FNet f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.total) return;
  const int K0 = f.K0, H = f.H;
  const FlatOffsets o = flat_offsets(K0, H);
  float v = 0.f;
  if (i < f.ob1) { const int r = i / LDW1, c = i % LDW1; if (r < H && c < K0) v = p[r * K0 + c]; }
  else if (i < f.ob2) { const int r = i - f.ob1; if (r < H) v = p[o.b1 + r]; }
  else if (i < f.ow3) { const int r = i - f.ob2; if (r < H) v = p[o.b2 + r]; }
  else if (i < f.ob3) { const int r = i - f.ow3; if (r < H) v = p[o.W3 + r]; }
  else if (i < f.oW2) { if (i == f.ob3) v = p[o.b3]; }
  else if (i < f.oW2T) { const int r = (i - f.oW2) / f.LDW, c = (i - f.oW2) % f.LDW; if (r < H && c < H) v = p[o.W2 + r * H + c]; }
  else { const int r = (i - f.oW2T) / f.LDW, c = (i - f.oW2T) % f.LDW; if (r < H && c < H) v = p[o.W2 + c * H + r]; }
  out[i] = v;
}

// the inverse: flat parameters out of a padded image (W2 from its row-major block); the episode ledger's snapshot of the
// image an acting kernel read (pdec_ledger_snapshot)
__global__ void unpack_fused_kernel(const float* __restrict__ img, float* __restrict__ p, FNet f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= flat_offsets(f.K0, f.H).n) return;
  p[i] = img[image_of_flat(f, i).o1];
}

// LDS image of the "small" part of a net: W1 [HP][LDW1], b1 [HP], b2 [HP], w3 [HP], b3 [4]
struct SmallLds {
  float *W1, *b1, *b2, *w3, *b3;
};
__device__ __forceinline__ SmallLds carve_small(float* base, int HP) {
  SmallLds s;
  s.W1 = base; s.b1 = s.W1 + HP * LDW1; s.b2 = s.b1 + HP; s.w3 = s.b2 + HP; s.b3 = s.w3 + HP;
  return s;
}

}  // namespace pdec
