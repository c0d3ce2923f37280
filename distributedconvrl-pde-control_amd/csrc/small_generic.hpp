// small_generic.hpp -- the reference's ACTUAL update shape (minibatch of `batch_size = 3` transitions, `update_loops = 20`
// updates per control step, src/PDEagent.jl:342-418, scripts/KS/setup/KSSetup.jl:66-71) in ONE launch, for nets of any depth up
// to SM_MAXL (the register kernels of small2.hpp / small2f.hpp serve the 2-layer shapes).
//
// At Bu = 3 every GEMM of the update is a few hundred multiply-adds; run as separate launches (the generic path) an
// update costs ~35 launches and a control step ~700, i.e. the step is pure launch latency (7 ms).  Here a single
// workgroup walks through all `loops` updates back to back: gather the minibatch from the device-resident replay traces
// (pde_fetch!, src/PDEagent.jl:323-340, indices drawn on the host exactly like pde_sample :317-321), target forward,
// critic forward/backward + ADAM, actor forward/backward through the updated critic + ADAM, Polyak -- with workgroup
// barriers between dependent layers.  Parameters, moments and gradients stay in global memory (L2-hot; a workgroup's
// waves share the CU's L1, so a barrier orders them), activations in LDS.  fp32 like the reference's networks, ADAM
// arithmetic in fp64 like Flux (see finish_param in fused3_finish.hpp).
#pragma once
#include "small_args.hpp"

namespace pdec {

__device__ __forceinline__ float sm_act(float z, int act) {
  return act == PDEC_ACT_RELU ? fmaxf(z, 0.f) : (act == PDEC_ACT_TANH ? tanhf(z) : z);
}
__device__ __forceinline__ float sm_dact(float a, int act) {   // derivative expressed through the activation value
  return act == PDEC_ACT_RELU ? (a > 0.f ? 1.f : 0.f) : (act == PDEC_ACT_TANH ? 1.f - a * a : 1.f);
}

// items x (sum over `len` terms): narrow reductions run one item per thread, wide ones (len >= 32, e.g. the critic's
// 140/340/1120-wide output layer) one item per wave with the terms spread over the lanes + a shuffle reduction, so no
// thread walks a long dependent chain of loads
template <class TermF, class StoreF>
__device__ __forceinline__ void sm_reduce(int items, int len, int tid, TermF term, StoreF store) {
  if (len >= 32) {
    const int wv = tid >> 6, lane = tid & 63;
    for (int it = wv; it < items; it += SM_THREADS / 64) {
      float acc = 0.f;
      for (int r = lane; r < len; r += 64) acc += term(it, r);
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
      if (lane == 0) store(it, acc);
    }
  } else {
    for (int it = tid; it < items; it += SM_THREADS) {
      float acc = 0.f;
      for (int r = 0; r < len; ++r) acc += term(it, r);
      store(it, acc);
    }
  }
}

// forward of one net: acts[0] = input [dims[0]][Bu] (already in LDS), acts[l] = layer outputs (feature-major)
__device__ void sm_forward(const SmallNet& n, const float* p, float* const* a, int Bu, int tid) {
  for (int l = 0; l < n.L; ++l) {
    const int in = n.dims[l], out = n.dims[l + 1], act = n.acts[l];
    const float* W = p + n.woff[l];
    const float* b = p + n.boff[l];
    const float* ain = a[l];
    float* aout = a[l + 1];
    sm_reduce(out * Bu, in, tid,
              [&](int idx, int k) { const int f = idx / Bu, c = idx - f * Bu; return W[f * in + k] * ain[k * Bu + c]; },
              [&](int idx, float z) { aout[idx] = sm_act(z + b[idx / Bu], act); });
    __syncthreads();
  }
}

// backward: dz0 holds dL/d(output activation) [dims[L]][Bu] on entry; writes gradients to n.g when want_dw;
// on return the buffer `*dx_out` holds dL/d(input) [dims[0]][Bu] when want_dx
__device__ void sm_backward(const SmallNet& n, const float* p, float* const* a, float* dz0, float* dz1, int Bu, int tid,
                            bool want_dw, bool want_dx, float** dx_out) {
  float *cur = dz0, *nxt = dz1;
  for (int l = n.L - 1; l >= 0; --l) {
    const int in = n.dims[l], out = n.dims[l + 1];
    // dz = dL/da * act'(a)
    for (int idx = tid; idx < out * Bu; idx += SM_THREADS) cur[idx] *= sm_dact(a[l + 1][idx], n.acts[l]);
    __syncthreads();
    if (want_dw) {
      float* gW = n.g + n.woff[l];
      float* gb = n.g + n.boff[l];
      for (int idx = tid; idx < out * in; idx += SM_THREADS) {
        const int f = idx / in, k = idx - f * in;
        float acc = 0.f;
        for (int c = 0; c < Bu; ++c) acc = fmaf(cur[f * Bu + c], a[l][k * Bu + c], acc);
        gW[idx] = acc;
      }
      for (int f = tid; f < out; f += SM_THREADS) {
        float acc = 0.f;
        for (int c = 0; c < Bu; ++c) acc += cur[f * Bu + c];
        gb[f] = acc;
      }
    }
    if (l > 0 || want_dx) {
      const float* W = p + n.woff[l];
      const float* dzc = cur;
      float* dxn = nxt;
      sm_reduce(in * Bu, out, tid,
                [&](int idx, int f) { const int k = idx / Bu, c = idx - k * Bu; return W[f * in + k] * dzc[f * Bu + c]; },
                [&](int idx, float v) { dxn[idx] = v; });
    }
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  if (dx_out) *dx_out = cur;
}

// Flux ADAM (fp64 arithmetic, no FMA contraction) + Polyak into the target
__device__ void sm_adam_polyak(const SmallNet& n, double eta, double b1, double b2, double eps, double omb1p, double omb2p,
                               float rho, float omr, int tid) {
#pragma clang fp contract(off)
  for (int i = tid; i < n.nparams; i += SM_THREADS) {
    const double gd = (double)n.g[i];
    const float mt = (float)(b1 * (double)n.m[i] + (1.0 - b1) * gd);
    const float vt = (float)(b2 * (double)n.v[i] + (1.0 - b2) * gd * gd);
    n.m[i] = mt;
    n.v[i] = vt;
    const float delta = (float)((double)mt / omb1p / (sqrt((double)vt / omb2p) + eps) * eta);
    n.p[i] = n.p[i] - delta;
  }
  __syncthreads();
}
__device__ void sm_polyak(const SmallNet& n, float rho, float omr, int tid) {
#pragma clang fp contract(off)
  for (int i = tid; i < n.nparams; i += SM_THREADS) n.pt[i] = rho * n.pt[i] + omr * n.p[i];
  __syncthreads();
}

__global__ __launch_bounds__(SM_THREADS) void ddpg_small_kernel(SmallArgs g_in) {
  SmallArgs g = g_in;
  if (g.pm && !sm_member_begin(g)) return;
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, Bu = g.Bu, ns = g.ns, na = g.na, K0 = ns + na;
  const int W = SmallLds::buf(g.maxw, Bu);           // floats per activation buffer
  // LDS carve (sized by SmallLds): actor activations aA[0..L], critic activations aC[0..L], two dz buffers, batch scalars
  float* aA[SM_MAXL + 1];
  float* aC[SM_MAXL + 1];
  float* q = sm;
  for (int l = 0; l <= g.A.L; ++l) { aA[l] = q; q += W; }
  for (int l = 0; l <= g.C.L; ++l) { aC[l] = q; q += W; }
  float* dz0 = q; q += W;
  float* dz1 = q; q += W;
  float* r = q; q += Bu;
  float* t = q; q += Bu;
  float* qt = q; q += Bu;
  float* red = q;                         // [SmallLds::RED]
  if (sm_halted(g, tid)) return;
  double bpa0 = g.bpA.cur[0], bpa1 = g.bpA.cur[1], bpc0 = g.bpC.cur[0], bpc1 = g.bpC.cur[1];
  const float omr = 1.0f - g.rho;
  const SmSlots sl = sm_slots(g, sm, tid, SM_THREADS);
  g.i_s = sl.i_s; g.i_rt = sl.i_rt; g.i_sn = sl.i_sn;
  // optional LDS residency of the learner state: [A.p | A.pt | A.m | A.v | A.g | C.p | C.pt | C.m | C.v | C.g]
  SmallNet gA = g.A, gC = g.C;     // global-memory views (written back at the end)
  if (g.lds_params) {
    float* base = red + SmallLds::RED;
    float* lp[10];
    const float* src[10] = {gA.p, gA.pt, gA.m, gA.v, nullptr, gC.p, gC.pt, gC.m, gC.v, nullptr};
    for (int k = 0; k < 10; ++k) {
      const int n = k < 5 ? gA.nparams : gC.nparams;
      lp[k] = base;
      base += SmallLds::pad(n);
      if (src[k])
        for (int i = tid; i < n; i += SM_THREADS) lp[k][i] = src[k][i];
    }
    g.A.p = lp[0]; g.A.pt = lp[1]; g.A.m = lp[2]; g.A.v = lp[3]; g.A.g = lp[4];
    g.C.p = lp[5]; g.C.pt = lp[6]; g.C.m = lp[7]; g.C.v = lp[8]; g.C.g = lp[9];
    __syncthreads();
  }
  for (int it = 0; it < g.loops; ++it) {
    const int* is = g.i_s + it * Bu;
    const int* irt = g.i_rt + it * Bu;
    const int* isn = g.i_sn + it * Bu;
    // ---- a' = At(s'), qt = Ct([s'; a'])                                        src/PDEagent.jl:385-386
    for (int idx = tid; idx < ns * Bu; idx += SM_THREADS) {
      const int k = idx / Bu, c = idx - k * Bu;
      const float v = g.state[(size_t)isn[c] * ns + k];
      aA[0][idx] = v;
      aC[0][idx] = v;
    }
    for (int c = tid; c < Bu; c += SM_THREADS) {
      r[c] = g.reward[irt[c]];
      t[c] = g.terminal[irt[c]];
    }
    __syncthreads();
    sm_forward(g.A, g.A.pt, aA, Bu, tid);
    for (int idx = tid; idx < na * Bu; idx += SM_THREADS) aC[0][ns * Bu + idx] = aA[g.A.L][idx];
    __syncthreads();
    sm_forward(g.C, g.C.pt, aC, Bu, tid);
    for (int c = tid; c < Bu; c += SM_THREADS) qt[c] = aC[g.C.L][c];
    __syncthreads();
    // ---- q = C([s; a])                                                           :392
    for (int idx = tid; idx < K0 * Bu; idx += SM_THREADS) {
      const int k = idx / Bu, c = idx - k * Bu;
      aC[0][idx] = k < ns ? g.state[(size_t)is[c] * ns + k] : g.action[(size_t)is[c] * na + (k - ns)];
    }
    __syncthreads();
    sm_forward(g.C, g.C.p, aC, Bu, tid);
    if (tid == 0) {   // loss and dq (tiny: Bu <= 16); quirk: r arrives 1 x Bu and broadcasts against the Bu-vector
      float rbar = 0.f;
      for (int c = 0; c < Bu; ++c) rbar += r[c];
      rbar /= (float)Bu;
      float loss = 0.f;
      for (int c = 0; c < Bu; ++c) {
        const float cc = g.gamma * (1.f - t[c]) * qt[c] - aC[g.C.L][c];
        if (g.quirk) {
          for (int j = 0; j < Bu; ++j) loss += (r[j] + cc) * (r[j] + cc);
        } else {
          loss += (r[c] + cc) * (r[c] + cc);
        }
        dz0[c] = -(2.f / (float)Bu) * ((g.quirk ? rbar : r[c]) + cc);
      }
      red[0] = g.quirk ? loss / (float)(Bu * Bu) : loss / (float)Bu;
    }
    __syncthreads();
    sm_backward(g.C, g.C.p, aC, dz0, dz1, Bu, tid, true, false, nullptr);         // :391-398
    sm_adam_polyak(g.C, g.eta_c, g.b1, g.b2, g.eps, 1.0 - bpc0, 1.0 - bpc1, g.rho, omr, tid);   // :400
    bpc0 *= g.b1;
    bpc1 *= g.b2;
    // ---- actor: -mean(C([s; A(s)])) with the updated critic                      :402-412
    for (int idx = tid; idx < ns * Bu; idx += SM_THREADS) {
      const int k = idx / Bu, c = idx - k * Bu;
      aA[0][idx] = g.state[(size_t)is[c] * ns + k];
    }
    __syncthreads();
    sm_forward(g.A, g.A.p, aA, Bu, tid);
    for (int idx = tid; idx < na * Bu; idx += SM_THREADS) aC[0][ns * Bu + idx] = aA[g.A.L][idx];
    __syncthreads();
    sm_forward(g.C, g.C.p, aC, Bu, tid);
    if (tid == 0) {
      float s = 0.f;
      for (int c = 0; c < Bu; ++c) s += aC[g.C.L][c];
      red[1] = -s / (float)Bu;
    }
    for (int c = tid; c < Bu; c += SM_THREADS) dz0[c] = -1.f / (float)Bu;
    __syncthreads();
    float* dx = nullptr;
    sm_backward(g.C, g.C.p, aC, dz0, dz1, Bu, tid, false, true, &dx);
    float* dA = dx == dz0 ? dz1 : dz0;    // the buffer not holding dx
    for (int idx = tid; idx < na * Bu; idx += SM_THREADS) dA[idx] = dx[ns * Bu + idx];
    __syncthreads();
    sm_backward(g.A, g.A.p, aA, dA, dx, Bu, tid, true, false, nullptr);
    sm_adam_polyak(g.A, g.eta_a, g.b1, g.b2, g.eps, 1.0 - bpa0, 1.0 - bpa1, g.rho, omr, tid);
    bpa0 *= g.b1;
    bpa1 *= g.b2;
    // rho == 1 (the reference as it runs: its Polyak loop iterates over an empty list, agent.py quirk_frozen_targets): the
    // targets are not touched at all, as in launch_finish / pdec_polyak -- dest = 1 * dest + 0 * src would rewrite them and
    // turn a non-finite behaviour parameter into a NaN target
    if (g.rho != 1.0f) {
      sm_polyak(g.A, g.rho, omr, tid);                                             // :415-417
      sm_polyak(g.C, g.rho, omr, tid);
    }
  }
  if (tid == 0 && g.losses) {
    g.losses[0] = red[0];
    g.losses[1] = red[1];
  }
  if (tid == 0) {
    g.bpA.next[0] = bpa0; g.bpA.next[1] = bpa1;
    g.bpC.next[0] = bpc0; g.bpC.next[1] = bpc1;
  }
  if (g.lds_params) {
    for (int i = tid; i < gA.nparams; i += SM_THREADS) { gA.p[i] = g.A.p[i]; gA.pt[i] = g.A.pt[i]; gA.m[i] = g.A.m[i]; gA.v[i] = g.A.v[i]; }
    for (int i = tid; i < gC.nparams; i += SM_THREADS) { gC.p[i] = g.C.p[i]; gC.pt[i] = g.C.pt[i]; gC.m[i] = g.C.m[i]; gC.v[i] = g.C.v[i]; }
  }
}

}  // namespace pdec
