// fused3_act.hpp -- the fused acting kernel of a 3-layer actor on its published padded image
#pragma once
#include "fused3_layers.hpp"

namespace pdec {

// LDS map of the acting kernel (float offsets): the image's first two blocks as they sit in HBM
template <int MTA>
struct ActLds {
  static constexpr int sa = 0;                                  // small block
  static constexpr int saW2 = sa + small_floats(16 * MTA);      // W2 [HPa][LDWa]
  static constexpr int end = saW2 + big_floats(16 * MTA);
};

// actions = clamp(actor(state) + randn * act_noise, +-act_limit)  (src/PDEagent.jl:183-207) in ONE launch on the
// same MFMA building blocks as the update passes (16 columns per wave, layer outputs chained as B operands);
// exploration noise from the same Philox counter stream as pdec_randn (element index = column), so both
// paths draw identical numbers.  AN: what carries the amplitude -- the launch scalar, NoiseScale (pdec_mlp_set_noise_scale) or NoiseColor
// (pdec_mlp_set_noise_color).
#define ACT_THREADS 256
template <int MTA, class AN = float>
__global__ __launch_bounds__(ACT_THREADS) void policy_act_fused_kernel(FNet f, const float* __restrict__ state, int cols, int ns,
                                                                      AN act_noise, float lim, int learning, int tanh_out,
                                                                      uint64_t seed, uint64_t offset, float* __restrict__ out,
                                                                      const uint64_t* ctr_cur, uint64_t* ctr_next, uint64_t ctr_inc,
                                                                      int prio, int full_rows) {
  extern __shared__ __align__(16) float smem[];
  if (ctr_cur) {       // noise counter kept on the device (pdec_policy_act_rng_dev): read it, one thread writes the advanced value
    offset += *ctr_cur;
    if (blockIdx.x == 0 && threadIdx.x == 0) *ctr_next = offset + ctr_inc;
  }
  // wave priority: PDEC_PRIO_ACT (default 3: short and latency-critical when nothing else holds the PDE step back)
  set_wave_prio(prio);
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4;
  constexpr int HPa = 16 * MTA, LDWa = HPa + LDWPAD, NSa = small_floats(HPa), NBa = big_floats(HPa);
  float* sa = smem + ActLds<MTA>::sa;
  float* saW2 = smem + ActLds<MTA>::saW2;
  const SmallLds SA = carve_small(sa, HPa);
  const int c = blockIdx.x * (ACT_THREADS / 4) + w * 16 + lr;
  const bool valid = c < cols;
  float x[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = 4 * t + q;
    x[t] = (valid && row < ns) ? state[(size_t)c * ns + row] : 0.f;
  }
  dma_even<NSa, ACT_THREADS / 64>(sa, f.w, w, l);                 // the image is laid out as it sits in LDS: two copies
  dma_even<NBa, ACT_THREADS / 64>(saW2, f.w + f.oW2, w, l);
  dma_wait();
  __syncthreads();
  f32x4 h1[MTA], h2[MTA];
  const LiveRows LA = live_rows<MTA>(ns, f.H, full_rows);
  layer_in<MTA, 4>(h1, x, SA, lr, q, LA);
  layer_hh_live<MTA, MTA, true>(h2, h1, saW2, LDWa, SA.b2, lr, q, LA.mo);
  relu_<MTA>(h2);
  float o = head<MTA>(h2, SA.w3, SA.b3[0], q);
  if (!valid || q != 0) return;
  if (tanh_out) o = tanhf(o);
  if (learning) {
    const float z = noise_draw<float>(act_noise, noise_normal(seed, offset, c), c, c);
    o += z * noise_amp<float>(act_noise, c);
  }
  out[c] = fminf(fmaxf(o, -lim), lim);
}

}  // namespace pdec
