// fused2_act.hpp -- the fused acting kernel of a 2-layer actor on its flat parameters
#pragma once
#include "fused2_layers.hpp"

namespace pdec {

// LDS map of the acting kernel (float offsets): the actor's image at the row stride of its OWN k-block count
template <int MTA, int KB>
struct Act2Lds {
  static constexpr int SA = 0;
  static constexpr int end = SA + lds2_floats(16 * MTA, 8 * KB + 4);
};

// actions = clamp(actor(state) + randn * act_noise, +-act_limit)   (src/PDEagent.jl:183-207) in ONE launch: first layer
// on MFMA out of the padded LDS image, output row + tanh, exploration noise from the Philox stream of pdec_randn
// (element index = column: both paths draw identical numbers), clamp.  256 threads = 4 waves x 16 columns.  AN: what carries
// the amplitude -- the launch scalar, NoiseScale (pdec_mlp_set_noise_scale) or NoiseColor (pdec_mlp_set_noise_color).
template <int MTA, int KB, class AN = float>
__global__ __launch_bounds__(256) void policy_act2_kernel(Net2 n, const float* __restrict__ state, int cols, AN act_noise,
                                                          float lim, int learning, int tanh_out, uint64_t seed, uint64_t offset,
                                                          float* __restrict__ out, const uint64_t* ctr_cur, uint64_t* ctr_next,
                                                          uint64_t ctr_inc) {
  constexpr int LDK = 8 * KB + 4, HPa = 16 * MTA;
  extern __shared__ __align__(16) float smem[];
  if (ctr_cur) {       // device-resident noise counter (pdec_policy_act_rng_dev)
    offset += *ctr_cur;
    if (blockIdx.x == 0 && threadIdx.x == 0) *ctr_next = offset + ctr_inc;
  }
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, q = l >> 4;
  const Lds2 SA = carve2(smem + Act2Lds<MTA, KB>::SA, HPa, LDK);
  // image load with 256 threads (load_net2 assumes FTHREADS): plain row copy, the actor is small.  The offsets of b1 | W2 | b2
  // are those of flat2_offsets(n.K0, n.H), written out with H K0 as a 64-bit product: taken from flat2_offsets (32-bit) the
  // instruction stream of every instantiation changes ("The 2-layer family by subject")
  for (int i = tid; i < HPa * LDK; i += 256) {
    const int r = i / LDK, c = i - r * LDK;
    SA.W1[i] = (r < n.H && c < n.K0) ? n.p[(size_t)r * n.K0 + c] : 0.f;
  }
  const float* b1 = n.p + (size_t)n.H * n.K0;
  for (int i = tid; i < HPa; i += 256) { SA.b1[i] = i < n.H ? b1[i] : 0.f; SA.w2[i] = i < n.H ? b1[n.H + i] : 0.f; }
  if (tid == 0) SA.b2[0] = b1[2 * n.H];
  __syncthreads();
  const int c = blockIdx.x * 64 + w * 16 + lr;
  const bool valid = c < cols;
  float x[K2MAX][2];
  load_x2(x, state, (size_t)c, n.K0, KB, q, valid);
  f32x4 ha[MTA];
  layer1_keep<MTA, KB>(ha, x, SA, lr, q);
  float o = head<MTA>(ha, SA.w2, SA.b2[0], q);
  if (!valid || q != 0) return;
  if (tanh_out) o = tanhf(o);
  if (learning) {
    const float z = noise_draw<float>(act_noise, noise_normal(seed, offset, c), c, c);
    o += z * noise_amp<float>(act_noise, c);
  }
  out[c] = fminf(fmaxf(o, -lim), lim);
}

}  // namespace pdec
