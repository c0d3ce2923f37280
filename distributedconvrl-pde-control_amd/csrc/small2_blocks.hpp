// small2_blocks.hpp -- the blocks the two register-resident kernels of the small DDPG update (ddpg_small2_kernel, small2.hpp;
// ddpg_small2f_kernel, small2f.hpp) are built from: the wave and row sums, the cross-wave exchange, the per-parameter ADAM step,
// the up-front minibatch staging, the load of a critic unit's registers, and the actor unit's gradient.
// NOT here, because as shared helpers they moved the kernels' register counts: the combining half of the exchange
// (s2_reduce2's, which ddpg_small2f_kernel spells out for its one-sided sums), the critic unit's write-back and the critic's
// TD-error / backward / ADAM block.  They stand in both kernels and must stay the same expressions for the two to agree bit for
// bit.
#pragma once
#include "small_args.hpp"

namespace pdec {

// sum over the 64 lanes of a wave, result in every lane: four DPP steps inside each row of 16 lanes, then the four row sums
// r0 .. r3 combined as (r0 + r1) + (r2 + r3) by two row broadcasts (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)
// and ONE v_readlane of lane 63 -- no LDS crossbar round trips (__shfl_xor = ds_bpermute_b32), a quarter of the VALU -> SGPR
// hazards of four readlanes.  (fp32 addition is commutative: r1 + r0 and (r3 + r2) + (r1 + r0) are the bits of the formula above.)
__device__ __forceinline__ float s2_wave_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // lane^1
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // lane^2
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));  // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));  // row_ror:8
  // rows outside the row mask receive `old` = 0: their values are not read again
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));  // row_bcast:15
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false));  // row_bcast:31
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// the four in-row steps of s2_wave_sum alone: every lane then holds the total of ITS row of 16 lanes (lane 16 r + 15 in exactly
// the order s2_wave_sum's row totals are formed in), for callers that sum four independent things per DPP chain, one per row
__device__ __forceinline__ float s2_row_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // lane^1
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // lane^2
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));  // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));  // row_ror:8
  return v;
}

// sum entries [0, n) and [H, H + n) of v (H = N / 2) over the workgroup; result in every thread.  buf: one of the two exchange
// buffers (S2_NW / S2_ROW, small_args.hpp; the caller alternates them); partial sums are added in wave order from 0.f, as before
template <int N>
__device__ __forceinline__ void s2_reduce2(float (&v)[N], int n, float* buf, int nw, int tid) {
  constexpr int H = N / 2;
  static_assert(N <= S2_ROW, "exchange row");
#pragma unroll
  for (int i = 0; i < N; ++i)
    if ((i < H ? i : i - H) < n) v[i] = s2_wave_sum(v[i]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) buf[(tid >> 6) * S2_ROW + i] = v[i];
  __syncthreads();
  float part[S2_NW][N];
#pragma unroll
  for (int w = 0; w < S2_NW; ++w)
#pragma unroll
    for (int i = 0; i < N; ++i) part[w][i] = buf[w * S2_ROW + i];       // rows >= nw: stale, never added
  float a[N];
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = 0.f;
#pragma unroll
  for (int w = 0; w < S2_NW; ++w)
    if (w < nw) {                                                         // (uniform)
#pragma unroll
      for (int i = 0; i < N; ++i) a[i] += part[w][i];
    }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (i < H ? i : i - H) < n ? a[i] : 0.f;
}

// Flux ADAM (fp64 arithmetic, no FMA contraction) + Polyak of one parameter held in registers.  The two bias-correction
// divisors 1 - beta^t are the same for every parameter of an update, so their reciprocals are taken once per update
// (i1, i2) and multiplied in: m * (1/c) instead of m / c differs from Flux's quotient by at most one fp64 ulp, far below
// the fp32 rounding of the stored step; it removes two of the three fp64 divisions per parameter.
__device__ __forceinline__ void s2_adam(float& p, float& m, float& v, float& pt, float gi, double eta, double b1, double b2,
                                        double eps, double i1, double i2, float rho, float omr, bool frozen) {
#pragma clang fp contract(off)
  const double gd = (double)gi;
  m = (float)(b1 * (double)m + (1.0 - b1) * gd);
  v = (float)(b2 * (double)v + (1.0 - b2) * gd * gd);
  const float delta = (float)((double)m * i1 / (sqrt((double)v * i2) + eps) * eta);
  p = p - delta;
  if (!frozen) pt = rho * pt + omr * p;      // frozen (rho == 1, uniform per launch): the target keeps its bits (see ddpg_small_kernel)
}

// The actor's gradient of -mean(C([s; A(s)])) for one actor unit: da[c] the critic's action gradient (summed over its units), ao[c]
// the actor's output tanh, ha[c] the unit's hidden activation; db2 is the same in every thread
template <int KA>
struct S2ActorGrad {
  float gb2, gw2, gb1, gw1[KA];
};
template <int KA, int BUT>
__device__ __forceinline__ S2ActorGrad<KA> s2_actor_grad(const float* da, const float* ao, const float* ha, float w2, const float* bs,
                                                         int Bu, int ns) {
  S2ActorGrad<KA> o;
  o.gw2 = 0.f; o.gb1 = 0.f; o.gb2 = 0.f;
#pragma unroll
  for (int k = 0; k < KA; ++k) o.gw1[k] = 0.f;
#pragma unroll
  for (int c = 0; c < BUT; ++c)
    if (c < Bu) {
      const float dz2 = da[c] * (1.f - ao[c] * ao[c]);      // tanh'
      o.gb2 += dz2;
      o.gw2 = fmaf(dz2, ha[c], o.gw2);
      const float dz = ha[c] > 0.f ? w2 * dz2 : 0.f;
      o.gb1 += dz;
#pragma unroll
      for (int k = 0; k < KA; ++k)
        if (k < ns) o.gw1[k] = fmaf(dz, bs[k * Bu + c], o.gw1[k]);
    }
  return o;
}

// the minibatches of ALL loops are fetched into LDS up front (pde_fetch!, src/PDEagent.jl:323-340): the replay traces
// do not change during the launch, so the two dependent global loads (slot index, then the row) are paid once.
// bstride floats per loop (Small2Lds / Small2fLds); the caller's next barrier orders the batches before their readers
__device__ __forceinline__ void s2_stage_batches(const SmallArgs& g, const SmSlots& sl, float* batch, int bstride, int ns, int Bu,
                                                 int tid, int nt) {
  for (int idx = tid; idx < g.loops * ns * Bu; idx += nt) {
    const int it = idx / (ns * Bu), rem = idx - it * (ns * Bu), k = rem / Bu, c = rem - k * Bu;
    batch[it * bstride + rem] = g.state[(size_t)sl.i_sn[it * Bu + c] * ns + k];
    batch[it * bstride + ns * Bu + rem] = g.state[(size_t)sl.i_s[it * Bu + c] * ns + k];
  }
  for (int idx = tid; idx < g.loops * Bu; idx += nt) {
    const int it = idx / Bu, c = idx - it * Bu;
    float* b = batch + it * bstride + 2 * ns * Bu;
    b[c] = g.action[sl.i_s[idx]];
    b[Bu + c] = g.reward[sl.i_rt[idx]];
    b[2 * Bu + c] = g.terminal[sl.i_rt[idx]];
  }
}

// critic unit `tid` (isC: there is one) of the 2-layer critic C with K0 = ns + 1 inputs, as its thread holds it for the launch:
// first-layer row w1 (KC >= K0 slots, the rest 0), bias b1 and output weight w2 at flat offsets ob1 / ow2, each with its ADAM
// moments (m, v) and its target copy (t)
template <int KC>
__device__ __forceinline__ void s2_load_critic_unit(const SmallNet& C, bool isC, int tid, int K0, int ob1, int ow2,
                                                    float (&w1)[KC], float (&w1m)[KC], float (&w1v)[KC], float (&w1t)[KC],
                                                    float& b1, float& b1m, float& b1v, float& b1t,
                                                    float& w2, float& w2m, float& w2v, float& w2t) {
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const bool ok = isC && k < K0;
    w1[k] = ok ? C.p[tid * K0 + k] : 0.f; w1m[k] = ok ? C.m[tid * K0 + k] : 0.f;
    w1v[k] = ok ? C.v[tid * K0 + k] : 0.f; w1t[k] = ok ? C.pt[tid * K0 + k] : 0.f;
  }
  if (isC) {
    b1 = C.p[ob1 + tid]; b1m = C.m[ob1 + tid]; b1v = C.v[ob1 + tid]; b1t = C.pt[ob1 + tid];
    w2 = C.p[ow2 + tid]; w2m = C.m[ow2 + tid]; w2v = C.v[ow2 + tid]; w2t = C.pt[ow2 + tid];
  }
}

}  // namespace pdec
