// fused3_layers.hpp -- what the two passes and the acting kernel of the fused 3-layer family share on the device: LDS-DMA
// copies and raw LDS barriers, the live extents of a net, the layer products on weight images in LDS, the arguments of a
// pass, the phase stamps, and the slab's tile numbering.
#pragma once
#include "fused3_image.hpp"
#include "mfma_blocks.hpp"

namespace pdec {

// ---- the big LDS region of a pass: the padded W2 image (in whole DMA pieces), later overlaid by the staging images of the
// weight-gradient products.  LDP128: leading dimension of the images staged over all 128 columns (pass C of the critic, the
// actor's one round); 8 mod 16 floats like LDP, so the ds_read_b128 operand reads are conflict free.
#define LDP128 136
// the actor's staging images: DZ3 [16] | HA2aug, DZA2, HA1aug, DZA1 [HPa] each | Xaug [16] rows of LDP128
__host__ __device__ constexpr int actor_stage_floats(int MTA) { return (32 + 4 * 16 * MTA) * LDP128; }
__host__ __device__ constexpr int wreg_floats(int MT, int MTA) {
  const int HP = 16 * MT;
  int a = big_floats(HP), b = 2 * HP * LDP, c = actor_stage_floats(MTA);
  int m = a > b ? a : b;
  return m > c ? m : c;
}

// ---- tiles of a pass's slab, per workgroup: dW3 [16][HP] (MT tiles) | dW2 [HP][HP] (MT*MT) | dW1 [HP][16] (MT), four
// chunks each (mfma_blocks.hpp, store_pass); then ONE chunk of statistics (critic: the five loss sums, actor: sum of q)
__host__ __device__ constexpr int slab_tiles(int MT) { return MT + MT * MT + MT; }
__host__ __device__ constexpr int stats_chunk(int MT) { return 4 * slab_tiles(MT); }
static inline size_t slab_floats_total(int MT, int nslab) { return ((size_t)stats_chunk(MT) + 1) * nslab * 64; }

// ---- Asynchronous global -> LDS copy of NFL floats (a multiple of 256) by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave
// instruction, no VGPR round trip).  EVERY one of the NW waves issues the same number of instructions, dma_count<NFL, NW>()
// -- a wave whose turn falls beyond the last piece copies the last piece again (same bytes, harmless) -- so that a wave can
// wait for an older copy while younger ones are still in flight with a literal s_waitcnt vmcnt(N) (dma_wait_but<N>).
// The data may be read after that wait + a workgroup barrier.
template <int NFL, int NW>
__host__ __device__ constexpr int dma_count() { return (NFL / 256 + NW - 1) / NW; }
template <int NFL, int NW>
__device__ __forceinline__ void dma_even(float* dst_lds, const float* src, int w, int l) {
  static_assert(NFL % 256 == 0 && NFL > 0, "dma_even copies whole 1-KiB pieces");
  constexpr int NCH = NFL / 256;
#pragma unroll
  for (int j = 0; j < dma_count<NFL, NW>(); ++j) {
    int c = w + NW * j;
    c = c < NCH ? c : NCH - 1;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)c * 256 + l * 4),
                                     (__attribute__((address_space(3))) void*)(dst_lds + (size_t)c * 256), 16, 0, 0);
  }
}
template <int N>
__device__ __forceinline__ void dma_wait_but() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Workgroup barrier for LDS data only: every LDS operation of this wave is complete, then s_barrier.  Unlike __syncthreads()
// -- whose workgroup fence makes hipcc wait vmcnt(0), i.e. drain every LDS-DMA in flight -- it leaves vector-memory
// operations (the weight-image copies, slab stores) outstanding across the barrier.  The "memory" clobber keeps the
// compiler from moving LDS accesses across it.  Data a DMA wrote is visible after dma_wait*() + lds_barrier().
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// block-wide deterministic sum (the fixed tree of block_sum) on raw barriers
__device__ __forceinline__ float block_sum_lds(float v, float* red, int tid) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  lds_barrier();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  lds_barrier();
  float r = 0.f;
  for (int i = 0; i < FTHREADS / 64; ++i) r += red[i];
  lds_barrier();
  return r;
}

// ---- Live extents of a net inside its padded image (wave-uniform, computed once per kernel).  The image is zero outside
// [H][K0] and [H][H] (prep_fused_kernel writes 0 there, finish_param writes live elements only) and the activations are
// zero in the same rows, so an MFMA on a k-step or a tile beyond these counts adds exact zeros: it is not issued.
//   kt = ceil(K0 / 4) k-steps of the first layer hold an input row (the bias enters through the accumulator, not a ones row)
//   mo = ceil(H / 16) tiles hold a hidden unit; tiles(H) = ceil((H + 1) / 16) counts the bias / output-gradient row of the
//        GRADIENT image too, so mo is MT or MT - 1: only the LAST tile of a net can be dead (H a multiple of 16)
// full (PDEC_FUSED_FULL_ROWS=1, tests only): the padded extents, i.e. every MFMA on zero rows and tiles is issued as well --
// the bit-identity reference (tests/test_gpu_fused_live_rows.py).
struct LiveRows {
  int kt, mo;
};
template <int MT>
__device__ __forceinline__ LiveRows live_rows(int K0, int H, int full) {
  LiveRows v;
  v.kt = full ? KXP / 4 : (K0 + 3) >> 2;
  v.mo = full ? MT : (H + 15) >> 4;
  return v;
}

// h = relu(W1 x + b1): x given as KT register rows (lane holds x[4t+q][col]).  k-steps t >= lv.kt are skipped, a last tile
// at or beyond lv.mo is zero without an MFMA.  One uniform branch around a whole k-step for all tiles: the MFMAs of a k-step
// are independent of each other, and every accumulator still takes its k-steps in the order t = 0, 1, ...
template <int MT, int KT>
__device__ __forceinline__ void layer_in(f32x4 (&h)[MT], const float (&x)[KT], const SmallLds& s, int lr, int q, LiveRows lv) {
  const bool last = MT - 1 < lv.mo;           // the one tile that can be dead
#pragma unroll
  for (int mo = 0; mo < MT; ++mo) {
    const float* b = s.b1 + 16 * mo + 4 * q;
    h[mo] = f32x4{b[0], b[1], b[2], b[3]};
  }
  auto kstep = [&](int t) {
#pragma unroll
    for (int mo = 0; mo < MT - 1; ++mo) h[mo] = mfma4(s.W1[(16 * mo + lr) * LDW1 + 4 * t + q], x[t], h[mo]);
    if (last) h[MT - 1] = mfma4(s.W1[(16 * (MT - 1) + lr) * LDW1 + 4 * t + q], x[t], h[MT - 1]);
  };
  static_assert(KT == 4, "layer_in: four k-steps (KXP input rows)");
  kstep(0);                                   // K0 >= 1
  if (lv.kt > 1) {
    kstep(1);
    if (lv.kt > 2) {
      kstep(2);
      if (lv.kt > 3) kstep(3);
    }
  }
  if (!last) h[MT - 1] = f32x4{0.f, 0.f, 0.f, 0.f};
  relu_<MT>(h);
}

// out = W in (+ bias): W image row-major [..][ldw] in LDS, 4 consecutive k per ds_read_b128.
// Two output tiles are accumulated at a time with their MFMAs interleaved, so consecutive MFMAs of a wave are
// independent (issue interval 32 cycles instead of the 40-cycle dependent latency of v_mfma_f32_16x16x4_f32).
// Tiles MO0 .. MO1-1 of the output only: a weight image may live in two LDS regions (rows below / above a split), each
// handed in with a base pointer W such that row r of the image is at W + r * ldw.
template <int MTO, int MTI, bool BIAS, int MO0, int MO1>
__device__ __forceinline__ void layer_hh_part(f32x4 (&out)[MTO], const f32x4 (&in)[MTI], const float* W, int ldw,
                                              const float* bias, int lr, int q) {
#pragma unroll
  for (int mo = MO0; mo + 1 < MO1; mo += 2) {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (BIAS) {
      const float* b = bias + 16 * mo + 4 * q;
      acc0 = f32x4{b[0], b[1], b[2], b[3]};
      acc1 = f32x4{b[16], b[17], b[18], b[19]};
    }
    const float* wrow0 = W + (16 * mo + lr) * ldw + 4 * q;
    const float* wrow1 = wrow0 + 16 * ldw;
    // operand reads run ONE block ahead of the MFMAs that consume them (explicit double buffer): left to itself the
    // scheduler issues each pair of ds_read_b128 right before its 8 MFMAs and the wave eats the LDS latency every time
    f32x4 wa = *reinterpret_cast<const f32x4*>(wrow0);
    f32x4 wb = *reinterpret_cast<const f32x4*>(wrow1);
#pragma unroll
    for (int m = 0; m < MTI; ++m) {
      f32x4 wan = wa, wbn = wb;
      if (m + 1 < MTI) {
        wan = *reinterpret_cast<const f32x4*>(wrow0 + 16 * (m + 1));
        wbn = *reinterpret_cast<const f32x4*>(wrow1 + 16 * (m + 1));
      }
      __builtin_amdgcn_sched_barrier(0);
      mfma4x4_pair(wa, in[m], acc0, wb, in[m], acc1);
      __builtin_amdgcn_sched_barrier(0);
      wa = wan;
      wb = wbn;
    }
    out[mo] = acc0;
    out[mo + 1] = acc1;
  }
#pragma unroll
  for (int mo = MO0 + ((MO1 - MO0) & ~1); mo < MO1; ++mo) {      // the odd tile out
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (BIAS) {
      const float* b = bias + 16 * mo + 4 * q;
      acc = f32x4{b[0], b[1], b[2], b[3]};
    }
    const float* wrow = W + (16 * mo + lr) * ldw + 4 * q;
#pragma unroll
    for (int m = 0; m < MTI; ++m) acc = mfma4x4(*reinterpret_cast<const f32x4*>(wrow + 16 * m), in[m], acc);
    out[mo] = acc;
  }
}
template <int MTO, int MTI, bool BIAS>
__device__ __forceinline__ void layer_hh(f32x4 (&out)[MTO], const f32x4 (&in)[MTI], const float* W, int ldw,
                                         const float* bias, int lr, int q) {
  layer_hh_part<MTO, MTI, BIAS, 0, MTO>(out, in, W, ldw, bias, lr, q);
}
// layer_hh for the ACTOR-sized products (MTA x MTA tiles): output tiles and k-tiles at or beyond `live` = LiveRows::mo of that
// net are skipped, dead output tiles are zero.  With every tile live (and always at one tile) it is layer_hh itself, instruction
// for instruction; otherwise one chain per live tile over the live k-tiles, in layer_hh's order m = 0, 1, ...  The critic's
// MT x MT chains do not come through here.
template <int MTO, int MTI, bool BIAS>
__device__ __forceinline__ void layer_hh_live(f32x4 (&out)[MTO], const f32x4 (&in)[MTI], const float* W, int ldw,
                                              const float* bias, int lr, int q, int live) {
  static_assert(MTO == MTI, "layer_hh_live: square hidden layers");
  if (MTO == 1 || live >= MTO) {
    layer_hh<MTO, MTI, BIAS>(out, in, W, ldw, bias, lr, q);
    return;
  }
#pragma unroll
  for (int mo = 0; mo < MTO; ++mo) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (mo < live) {
      if (BIAS) {
        const float* b = bias + 16 * mo + 4 * q;
        acc = f32x4{b[0], b[1], b[2], b[3]};
      }
      const float* wrow = W + (16 * mo + lr) * ldw + 4 * q;
#pragma unroll
      for (int m = 0; m < MTI; ++m)
        if (m < live) acc = mfma4x4(*reinterpret_cast<const f32x4*>(wrow + 16 * m), in[m], acc);
    }
    out[mo] = acc;
  }
}

// ---- the arguments of a pass.  One struct for both kernels; each launch sets the fields its pass reads and leaves the
// rest zero:  critic pass: C, At, Ct | s, a, r, t, sn | gamma, quirk, rpart / nrpart / rbar_dev, stamps
//             actor pass:  A, C      | s
struct FusedArgs {
  FNet A, C, At, Ct;          // behaviour actor and critic, target actor and critic
  const float *s, *a, *r, *t, *sn;
  int Bu, ns, na;
  float gamma;
  int quirk;
  float* slab;                // chunk-major partial gradients, see store_pass
  const float* rpart;         // != null: per-workgroup reward sums of the producer, nrpart of them (sum / Bu = batch mean)
  int nrpart;
  const float* rbar_dev;      // != null: batch-mean reward already reduced by launch_rmean (batches beyond 32768 columns)
  int prio;                   // wave priority of the pass (PDEC_PRIO_MFMA)
  int full_rows;              // != 0 (PDEC_FUSED_FULL_ROWS=1, tests only): MFMAs over the padded extents, see LiveRows
  unsigned long long* stamps; // diagnostic only (PDEC_STAMPS=1): [gridDim.x][16] counter values at phase boundaries
};

// diagnostic phase stamps: wave 0 / lane 0 of each workgroup; a null pointer (the default) costs one scalar branch.
// STAMP: the shader clock (s_memtime); STAMP_RT: the constant 100 MHz counter (s_memrealtime), slots 11 / 12 at the start /
// end of the workgroup (shader clock = d s_memtime / d s_memrealtime x 100 MHz)
#define STAMP_AS(k, counter)                                                                  \
  do {                                                                                        \
    if (g.stamps && threadIdx.x == 0) g.stamps[(size_t)blockIdx.x * 16 + (k)] = counter();    \
  } while (0)
#define STAMP(k) STAMP_AS(k, __builtin_amdgcn_s_memtime)
#define STAMP_RT(k) STAMP_AS(k, __builtin_amdgcn_s_memrealtime)

}  // namespace pdec
