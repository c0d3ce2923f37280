// mlp_small.hip -- the reference's ACTUAL update shape (minibatch of `batch_size = 3` transitions, `update_loops = 20`
// updates per control step, src/PDEagent.jl:342-418, scripts/KS/setup/KSSetup.jl:66-71) in ONE launch.
//
// At Bu = 3 every GEMM of the update is a few hundred multiply-adds; run as separate launches (the generic path) an
// update costs ~35 launches and a control step ~700, i.e. the step is pure launch latency (7 ms).  Here a single
// workgroup walks through all `loops` updates back to back: gather the minibatch from the device-resident replay traces
// (pde_fetch!, src/PDEagent.jl:323-340, indices drawn on the host exactly like pde_sample :317-321), target forward,
// critic forward/backward + ADAM, actor forward/backward through the updated critic + ADAM, Polyak -- with workgroup
// barriers between dependent layers.  Parameters, moments and gradients stay in global memory (L2-hot; a workgroup's
// waves share the CU's L1, so a barrier orders them), activations in LDS.  fp32 like the reference's networks, ADAM
// arithmetic in fp64 like Flux (see finish_param in mlp_mfma.hip).
#include "common.hpp"
#include "population.hpp"

namespace pdec {

#define SM_THREADS 256
#define SM_MAXL 4

struct SmallNet {
  float *p, *g, *m, *v;     // flat parameters / gradients / ADAM moments (internal layout: W_l row-major [out][in], b_l)
  float* pt;                // target parameters (Polyak destination) or null
  int L, nparams;
  int dims[SM_MAXL + 1], acts[SM_MAXL], woff[SM_MAXL], boff[SM_MAXL];
};

struct SmallArgs {
  SmallNet A, C;            // behaviour actor / critic (pt = target networks' parameters)
  const float *state, *action, *reward, *terminal;   // replay traces: [slot][ns], [slot][na], [slot], [slot]
  const int *i_s, *i_rt, *i_sn;                      // [loops][Bu] slots of s/a, r/t and s'
  int loops, Bu, ns, na, quirk, maxw;
  int lds_params;           // != 0: parameters, moments and gradients of all four networks are staged in LDS for the whole
                            // launch (the layer-to-layer dependency chain then pays LDS, not L2, latency)
  float gamma, rho;
  double eta_a, eta_c, b1, b2, eps;
  BpArgs bpA, bpC;          // device-resident ADAM beta powers of the actor / critic (read cur, thread 0 writes next)
  float* losses;            // [2]: critic loss, actor loss of the last loop
  const int* halt;          // != null and *halt != 0: the launch leaves the learner as it is (pdec_set_episode_halt on the critic)
  // pde_sample on the device (src/PDEagent.jl:317-321): when smp_on, the slots are not read from i_s / i_rt / i_sn but
  // drawn here from the Philox counter stream (seed, offset): draw k (= loop * Bu + column) is word k % 4 of counter
  // offset + k / 4, ind = (word * hi) >> 32 in [0, hi), logical index lg = base + ind,
  // slots (lg % cap1, lg % cap, (lg + stride) % cap1).  The slot table lives in LDS at float offset smp_lds.
  int smp_on, smp_lds;
  uint64_t smp_seed, smp_offset;
  uint32_t smp_hi;
  int64_t smp_base;
  int smp_cap, smp_cap1, smp_stride;
  // population (pdec_population_update): != null -> workgroup m updates member m (sm_member_begin)
  const PopMember* pm;
  long long* rows;
  long long m_after, m_freq, m_dsample;
  int m_hyper;              // != 0: gamma, rho and the two ADAM step sizes are the member's own (row slots enum PopHyperSlot)
};

// a row slot that holds the bit pattern of a double, as a wave-uniform value (every lane loads the same word; the halves go
// through the scalar registers the launch argument it replaces would sit in)
__device__ __forceinline__ double sm_row_double(const long long* row, int slot) {
  const long long b = row[slot];
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// population member blockIdx.x: Agent._maybe_update's trigger (agent.py) from the member's counters -- false: the member does not
// update at this step and the whole workgroup returns --, else its pointers, sampling bounds and beta-power slots into g as
// ddpg_update_small_impl sets them for its solo call; the row moves on as the host's counters do behind that call.  With
// m_hyper the member's own gamma, rho and step sizes replace the launch's: the doubles its solo call would pass, through the
// conversions small_args applies to them -- every kernel below reads them from its copy of g behind this prologue (omr, frz and
// the frozen kernel's up-front TD targets included), so the arithmetic is the solo call's.
// HYPER = false compiles that out: the launch's values are kernel arguments the compiler re-reads where it needs them, a
// member's own stay in registers for the whole launch, and the bounded register kernels (ddpg_small2_kernel, EXACT = false)
// have none left -- they would spill to scratch.  small_serves_member_hyper() tells the host which kernels serve it.
template <bool HYPER = true>
__device__ __forceinline__ bool sm_member_begin(SmallArgs& g) {
  const int mb = blockIdx.x;
  long long* row = g.rows + (size_t)mb * POP_ROW;
  const long long n_rt = row[POP_NRT], ustep = row[POP_USTEP], soff = row[POP_SAMPLE];
  const int sa = (int)row[POP_BPA], sc = (int)row[POP_BPC];
  const long long nv = n_rt < (long long)g.smp_cap ? n_rt : (long long)g.smp_cap;      // length(trajectory)
  if (row[POP_HALT] || !(nv > g.m_after) || ustep % g.m_freq != 0) return false;
  const PopMember& pm = g.pm[mb];
  g.A.p = pm.Ap; g.A.g = pm.Ag; g.A.m = pm.Am; g.A.v = pm.Av; g.A.pt = pm.Apt;
  g.C.p = pm.Cp; g.C.g = pm.Cg; g.C.m = pm.Cm; g.C.v = pm.Cv; g.C.pt = pm.Cpt;
  g.state = pm.ts; g.action = pm.ta; g.reward = pm.tr; g.terminal = pm.tt;
  g.bpA.cur = pm.bpA + 2 * sa; g.bpA.next = pm.bpA + 2 * (sa ^ 1);
  g.bpC.cur = pm.bpC + 2 * sc; g.bpC.next = pm.bpC + 2 * (sc ^ 1);
  g.losses = pm.losses;
  g.halt = nullptr;
  g.smp_seed = pm.sample_seed; g.smp_offset = (uint64_t)soff;
  g.smp_hi = (uint32_t)(nv - g.smp_stride);
  g.smp_base = n_rt > (long long)g.smp_cap ? n_rt - g.smp_cap : 0;
  if (HYPER && g.m_hyper) {
    g.gamma = (float)sm_row_double(row, POP_GAMMA); g.rho = (float)sm_row_double(row, POP_RHO);
    g.eta_a = sm_row_double(row, POP_ETA_A); g.eta_c = sm_row_double(row, POP_ETA_C);
  }
  __syncthreads();                    // every thread has read the row
  if (threadIdx.x == 0) {
    row[POP_SAMPLE] = soff + g.m_dsample;
    row[POP_BPA] = sa ^ 1;
    row[POP_BPC] = sc ^ 1;
  }
  return true;
}

// draw the [loops][Bu] slot tables into LDS (see SmallArgs); every thread then reads them after a barrier
__device__ __forceinline__ void sm_draw_slots(const SmallArgs& g, int* tab, int tid, int nt) {
  const int n = g.loops * g.Bu;
  for (int k = tid; k < n; k += nt) {
    const uint64_t ctr = g.smp_offset + (uint64_t)(k >> 2);
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32(c, (uint32_t)g.smp_seed, (uint32_t)(g.smp_seed >> 32));
    const uint32_t ind = (uint32_t)(((uint64_t)c[k & 3] * (uint64_t)g.smp_hi) >> 32);
    const int64_t lg = g.smp_base + (int64_t)ind;
    tab[k] = (int)(lg % g.smp_cap1);
    tab[n + k] = (int)(lg % g.smp_cap);
    tab[2 * n + k] = (int)((lg + g.smp_stride) % g.smp_cap1);
  }
}

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
  const int W = g.maxw * Bu;             // floats per activation buffer
  // LDS carve: actor activations aA[0..L], critic activations aC[0..L], two dz buffers, batch scalars
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
  float* red = q;                         // [4]
  double bpa0 = g.bpA.cur[0], bpa1 = g.bpA.cur[1], bpc0 = g.bpC.cur[0], bpc1 = g.bpC.cur[1];
  if (g.halt && *g.halt) {     // the episode ended before this step: only the beta powers move on to the slot the host flipped to
    if (tid == 0) { g.bpA.next[0] = bpa0; g.bpA.next[1] = bpa1; g.bpC.next[0] = bpc0; g.bpC.next[1] = bpc1; }
    return;
  }
  const float omr = 1.0f - g.rho;
  if (g.smp_on) {
    int* tab = reinterpret_cast<int*>(sm + g.smp_lds);
    sm_draw_slots(g, tab, tid, SM_THREADS);
    const int n = g.loops * Bu;
    g.i_s = tab; g.i_rt = tab + n; g.i_sn = tab + 2 * n;
    __syncthreads();
  }
  // optional LDS residency of the learner state: [A.p | A.pt | A.m | A.v | A.g | C.p | C.pt | C.m | C.v | C.g]
  SmallNet gA = g.A, gC = g.C;     // global-memory views (written back at the end)
  if (g.lds_params) {
    float* base = red + 4;
    float* lp[10];
    const float* src[10] = {gA.p, gA.pt, gA.m, gA.v, nullptr, gC.p, gC.pt, gC.m, gC.v, nullptr};
    for (int k = 0; k < 10; ++k) {
      const int n = k < 5 ? gA.nparams : gC.nparams;
      lp[k] = base;
      base += (n + 3) & ~3;
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


// ------------------------------------------------------------------------------------------------------------------
// 2-layer nets (the reference's `drop_middle_layer = true` shape, src/PDEagent.jl:30-41): one THREAD per hidden unit.
// A thread keeps its unit's weights (first-layer row, bias, output weight), their ADAM moments and the target copies in
// REGISTERS for all `loops` updates; forward, backward, ADAM and Polyak of a unit are thread-local, and only the
// output-layer sums cross threads (DPP inside a wave, one LDS exchange + one barrier across waves).  Three barriers
// per update instead of ~35, no weight traffic at all between the first load and the final write-back.
#define S2_BU 4            // most minibatch columns the register-resident kernel holds (reference: batch_size = 3)

struct Small2Args {
  SmallArgs g;
  int nC, nA;              // hidden widths
};

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

// Cross-wave exchange buffers: [2][S2_NW][S2_ROW] floats of LDS -- a row per wave, padded to 32 bytes, always eight rows (a
// workgroup has at most 512 threads) so that the combining reads below are unconditional vector reads issued together: one LDS
// round trip per exchange.  (Round 5 form: a loop over the waves with one load and one wait per partial, and the buffer picked
// through a two-pointer array that the compiler could no longer prove to be LDS -- 18 dependent FLAT loads per exchange, which
// was two thirds of the 4.6 us an update took.)
#define S2_NW 8
#define S2_ROW (2 * S2_BU)

// sum entries [0, n) and [H, H + n) of v (H = N / 2) over the workgroup; result in every thread.  buf: one of the two exchange
// buffers (the caller alternates them); partial sums are added in wave order from 0.f, as before
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

// EXACT: ns == KA and Bu == BUT are compile-time constants (the shipped experiments: (1,3) KS, (12,3) Keller-Segel,
// (9,3) fluid), so every column / input-row guard folds away; otherwise KA / BUT are upper bounds checked at run time
// OS > 0: the ADAM state of the actor's per-unit parameters lives ONE PARAMETER PER (lane, slot) of wave 0 -- flat parameter f in
// lane f % 64, slot f / 64, OS slots -- instead of ns + 2 parameters per unit thread: the actor's update is then OS fp64 ADAM chains
// per update (5 for the Keller-Segel actor's 280 parameters) where the 20 unit threads ran 14 one after the other while every other
// wave waited.  Gradients reach their owners and the new weights (and targets) their units through LDS, inside the wave (LDS
// operations of one wave execute in order: no barrier).  Same arithmetic per parameter.  Needs nA <= 64, (ns + 2) nA <= 64 OS.
template <int KC, int KA, int BUT, bool EXACT, int OS = 0>
__global__ __launch_bounds__(512) void ddpg_small2_kernel(Small2Args a_m) {
  Small2Args a_in = a_m;
  if (a_in.g.pm && !sm_member_begin<EXACT>(a_in.g)) return;
  const SmallArgs& g = a_in.g;
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
  if (g.halt && *g.halt) {     // the episode ended before this step (see ddpg_small_kernel)
    if (tid == 0) {
      g.bpA.next[0] = g.bpA.cur[0]; g.bpA.next[1] = g.bpA.cur[1];
      g.bpC.next[0] = g.bpC.cur[0]; g.bpC.next[1] = g.bpC.cur[1];
    }
    return;
  }
  const int Bu = EXACT ? BUT : g.Bu, ns = EXACT ? KA : g.ns, K0 = ns + 1, nC = a_in.nC, nA = a_in.nA;
  const bool isC = tid < nC, isA = tid < nA;
  // the minibatches of ALL loops are fetched into LDS up front (pde_fetch!, src/PDEagent.jl:323-340): the replay traces
  // do not change during the launch, so the two dependent global loads (slot index, then the row) are paid once
  const int bstride = (2 * ns + 3) * Bu;    // per loop: s' [ns][Bu], s [ns][Bu], a [Bu], r [Bu], t [Bu]
  float* batch = sm;
  float* red = batch + (size_t)g.loops * bstride;    // [2][S2_NW][S2_ROW]
  float* xg = red + 2 * S2_NW * S2_ROW;              // OS > 0: [3][64 OS] gradients / new parameters / new targets by flat index
  // three exchanges per update, two buffers: the parity flips from one update to the next, so an exchange never reuses
  // the buffer of the exchange right before it (a fast wave cannot overwrite partials a slow wave is still summing)
  int rp = 0;
  const int *i_s = g.i_s, *i_rt = g.i_rt, *i_sn = g.i_sn;
  if (g.smp_on) {
    int* tab = reinterpret_cast<int*>(sm + g.smp_lds);
    sm_draw_slots(g, tab, tid, nt);
    const int n = g.loops * g.Bu;
    i_s = tab; i_rt = tab + n; i_sn = tab + 2 * n;
    __syncthreads();
  }
  for (int idx = tid; idx < g.loops * ns * Bu; idx += nt) {
    const int it = idx / (ns * Bu), rem = idx - it * (ns * Bu), k = rem / Bu, c = rem - k * Bu;
    batch[it * bstride + rem] = g.state[(size_t)i_sn[it * Bu + c] * ns + k];
    batch[it * bstride + ns * Bu + rem] = g.state[(size_t)i_s[it * Bu + c] * ns + k];
  }
  for (int idx = tid; idx < g.loops * Bu; idx += nt) {
    const int it = idx / Bu, c = idx - it * Bu;
    float* b = batch + it * bstride + 2 * ns * Bu;
    b[c] = g.action[i_s[idx]];
    b[Bu + c] = g.reward[i_rt[idx]];
    b[2 * Bu + c] = g.terminal[i_rt[idx]];
  }
  // ---- this thread's unit: parameters p, moments m/v, target pt
  float cw1[KC], cw1m[KC], cw1v[KC], cw1t[KC], cb1 = 0, cb1m = 0, cb1v = 0, cb1t = 0, cw2 = 0, cw2m = 0, cw2v = 0, cw2t = 0;
  float aw1[KA], aw1m[KA], aw1v[KA], aw1t[KA], ab1 = 0, ab1m = 0, ab1v = 0, ab1t = 0, aw2 = 0, aw2m = 0, aw2v = 0, aw2t = 0;
  // output biases: replicated in every thread (identical arithmetic), written back by thread 0
  const int cob1 = nC * K0, cow2 = cob1 + nC, cob2 = cow2 + nC;
  const int aob1 = nA * ns, aow2 = aob1 + nA, aob2 = aow2 + nA;
  float cb2 = g.C.p[cob2], cb2m = g.C.m[cob2], cb2v = g.C.v[cob2], cb2t = g.C.pt[cob2];
  float ab2 = g.A.p[aob2], ab2m = g.A.m[aob2], ab2v = g.A.v[aob2], ab2t = g.A.pt[aob2];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const bool ok = isC && k < K0;
    cw1[k] = ok ? g.C.p[tid * K0 + k] : 0.f; cw1m[k] = ok ? g.C.m[tid * K0 + k] : 0.f;
    cw1v[k] = ok ? g.C.v[tid * K0 + k] : 0.f; cw1t[k] = ok ? g.C.pt[tid * K0 + k] : 0.f;
  }
  if (isC) {
    cb1 = g.C.p[cob1 + tid]; cb1m = g.C.m[cob1 + tid]; cb1v = g.C.v[cob1 + tid]; cb1t = g.C.pt[cob1 + tid];
    cw2 = g.C.p[cow2 + tid]; cw2m = g.C.m[cow2 + tid]; cw2v = g.C.v[cow2 + tid]; cw2t = g.C.pt[cow2 + tid];
  }
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const bool ok = isA && k < ns;
    aw1[k] = ok ? g.A.p[tid * ns + k] : 0.f; aw1m[k] = ok ? g.A.m[tid * ns + k] : 0.f;
    aw1v[k] = ok ? g.A.v[tid * ns + k] : 0.f; aw1t[k] = ok ? g.A.pt[tid * ns + k] : 0.f;
  }
  if (isA) {
    ab1 = g.A.p[aob1 + tid]; ab1m = g.A.m[aob1 + tid]; ab1v = g.A.v[aob1 + tid]; ab1t = g.A.pt[aob1 + tid];
    aw2 = g.A.p[aow2 + tid]; aw2m = g.A.m[aow2 + tid]; aw2v = g.A.v[aow2 + tid]; aw2t = g.A.pt[aow2 + tid];
  }
  constexpr int OSN = OS > 0 ? OS : 1;
  float op[OSN], om[OSN], ov[OSN], opt[OSN];
  const int nown = (ns + 2) * nA;                    // the actor's per-unit parameters = flat indices [0, nown)
  if constexpr (OS > 0) {
#pragma unroll
    for (int j = 0; j < OS; ++j) {
      const int f = j * 64 + tid;
      const bool own = tid < 64 && f < nown;
      op[j] = own ? g.A.p[f] : 0.f; om[j] = own ? g.A.m[f] : 0.f; ov[j] = own ? g.A.v[f] : 0.f; opt[j] = own ? g.A.pt[f] : 0.f;
    }
  }
  double bpa0 = g.bpA.cur[0], bpa1 = g.bpA.cur[1], bpc0 = g.bpC.cur[0], bpc1 = g.bpC.cur[1];
  const float omr = 1.0f - g.rho, invB = 1.f / (float)Bu;
  const bool frz = g.rho == 1.0f;
  float closs = 0.f, aloss = 0.f;
  for (int it = 0; it < g.loops; ++it) {
    const float* bsn = batch + it * bstride;
    const float* bs = bsn + ns * Bu;
    const float* ba = bs + ns * Bu;
    const float* br = ba + Bu;
    const float* bt = br + Bu;
    if (it == 0) __syncthreads();          // the batches are staged
    float v[2 * BUT];
    // Three exchanges per update: {a' = At(s'), A(s)} -> {qt = Ct([s'; a']), q = C([s; a])} -> critic update ->
    // {q of the updated critic on [s; A(s)], da}.  The behaviour actor's forward does not depend on the critic update, so
    // it shares the first exchange with the target actor's (src/PDEagent.jl:385 and :403).
    float ha[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) {
      float zt = ab1t, z = ab1;
#pragma unroll
      for (int k = 0; k < KA; ++k)
        if (k < ns) {
          zt += aw1t[k] * bsn[k * Bu + (c < Bu ? c : 0)];
          z += aw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
        }
      const bool on = isA && c < Bu;
      ha[c] = on ? fmaxf(z, 0.f) : 0.f;
      v[c] = on ? aw2t * fmaxf(zt, 0.f) : 0.f;
      v[BUT + c] = aw2 * ha[c];
    }
    s2_reduce2<2 * BUT>(v, Bu, red + rp * (S2_NW * S2_ROW), nw, tid);
    rp ^= 1;
    float an[BUT], ao[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) { an[c] = tanhf(v[c] + ab2t); ao[c] = tanhf(v[BUT + c] + ab2); }
    // ---- qt = Ct([s'; a'])  :386   and   q = C([s; a])  :392
    float h[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) {
      float zt = cb1t, z = cb1;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k < ns) {
          zt += cw1t[k] * bsn[k * Bu + (c < Bu ? c : 0)];
          z += cw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
        } else if (k == ns) {
          zt += cw1t[k] * an[c];
          z += cw1[k] * ba[c < Bu ? c : 0];
        }
      const bool on = isC && c < Bu;
      h[c] = on ? fmaxf(z, 0.f) : 0.f;
      v[c] = on ? cw2t * fmaxf(zt, 0.f) : 0.f;
      v[BUT + c] = cw2 * h[c];
    }
    s2_reduce2<2 * BUT>(v, Bu, red + rp * (S2_NW * S2_ROW), nw, tid);
    rp ^= 1;
    float qt[BUT];
#pragma unroll
    for (int c = 0; c < BUT; ++c) { qt[c] = v[c] + cb2t; v[c] = v[BUT + c]; }     // v[c] = q partial sum (without b2)
    float dq[BUT];
    {
      float rbar = 0.f;
      for (int c = 0; c < Bu; ++c) rbar += br[c];
      rbar *= invB;
      float loss = 0.f, gb2 = 0.f;
#pragma unroll
      for (int c = 0; c < BUT; ++c) {
        dq[c] = 0.f;
        if (c < Bu) {
          const float cc = g.gamma * (1.f - bt[c]) * qt[c] - (v[c] + cb2);
          if (g.quirk) {
            for (int j = 0; j < Bu; ++j) loss += (br[j] + cc) * (br[j] + cc);
          } else {
            loss += (br[c] + cc) * (br[c] + cc);
          }
          dq[c] = -(2.f * invB) * ((g.quirk ? rbar : br[c]) + cc);
          gb2 += dq[c];
        }
      }
      closs = g.quirk ? loss / (float)(Bu * Bu) : loss * invB;
      const double o1 = 1.0 / (1.0 - bpc0), o2 = 1.0 / (1.0 - bpc1);
      // thread-local backward of unit `tid`: dW2 = sum_c dq h, dz1 = relu'(h) w2 dq, db1 = sum_c dz1, dW1[k] = sum_c dz1 x[k]
      float gw2 = 0.f, gb1 = 0.f, gw1[KC];
#pragma unroll
      for (int k = 0; k < KC; ++k) gw1[k] = 0.f;
#pragma unroll
      for (int c = 0; c < BUT; ++c)
        if (c < Bu) {
          gw2 = fmaf(dq[c], h[c], gw2);
          const float dz = h[c] > 0.f ? cw2 * dq[c] : 0.f;
          gb1 += dz;
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k < ns) gw1[k] = fmaf(dz, bs[k * Bu + c], gw1[k]);
            else if (k == ns) gw1[k] = fmaf(dz, ba[c], gw1[k]);
        }
      if (isC) {
#pragma unroll
        for (int k = 0; k < KC; ++k)
          if (k < K0) s2_adam(cw1[k], cw1m[k], cw1v[k], cw1t[k], gw1[k], g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(cb1, cb1m, cb1v, cb1t, gb1, g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(cw2, cw2m, cw2v, cw2t, gw2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      }
      s2_adam(cb2, cb2m, cb2v, cb2t, gb2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      bpc0 *= g.b1;
      bpc1 *= g.b2;
    }
    // ---- actor: -mean(C([s; A(s)])) with the updated critic                     :402-412
    // critic forward on [s; A(s)]: q for the reported loss and da[c] = sum_f W1c[f][ns] relu'(h) w2 (-1/Bu) in ONE exchange
#pragma unroll
    for (int c = 0; c < BUT; ++c) {
      float z = cb1;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k < ns) z += cw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
        else if (k == ns) z += cw1[k] * ao[c];
      const bool on = isC && c < Bu;
      v[c] = on ? cw2 * fmaxf(z, 0.f) : 0.f;
      float wns = 0.f;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (k == ns) wns = cw1[k];
      v[BUT + c] = (on && z > 0.f) ? wns * cw2 * (-invB) : 0.f;
    }
    s2_reduce2<2 * BUT>(v, Bu, red + rp * (S2_NW * S2_ROW), nw, tid);
    rp ^= 1;
    {
      float s = 0.f;
      for (int c = 0; c < Bu; ++c) s += v[c] + cb2;
      aloss = -s * invB;
      const double o1 = 1.0 / (1.0 - bpa0), o2 = 1.0 / (1.0 - bpa1);
      float gw2 = 0.f, gb1 = 0.f, gb2 = 0.f, gw1[KA];
#pragma unroll
      for (int k = 0; k < KA; ++k) gw1[k] = 0.f;
#pragma unroll
      for (int c = 0; c < BUT; ++c)
        if (c < Bu) {
          const float dz2 = v[BUT + c] * (1.f - ao[c] * ao[c]);      // tanh'
          gb2 += dz2;
          gw2 = fmaf(dz2, ha[c], gw2);
          const float dz = ha[c] > 0.f ? aw2 * dz2 : 0.f;
          gb1 += dz;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) gw1[k] = fmaf(dz, bs[k * Bu + c], gw1[k]);
        }
      if constexpr (OS > 0) {
        if (tid < 64) {                    // wave 0: units -> owners -> units through LDS, in program order
          float* gA = xg;
          float* pA = xg + 64 * OS;
          float* ptA = pA + 64 * OS;
          if (isA) {
#pragma unroll
            for (int k = 0; k < KA; ++k)
              if (k < ns) gA[tid * ns + k] = gw1[k];
            gA[aob1 + tid] = gb1;
            gA[aow2 + tid] = gw2;
          }
#pragma unroll
          for (int j = 0; j < OS; ++j) {
            const int f = j * 64 + tid;
            if (f < nown) {
              s2_adam(op[j], om[j], ov[j], opt[j], gA[f], g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
              pA[f] = op[j];
              if (!frz) ptA[f] = opt[j];
            }
          }
          if (isA) {
#pragma unroll
            for (int k = 0; k < KA; ++k)
              if (k < ns) {
                aw1[k] = pA[tid * ns + k];
                if (!frz) aw1t[k] = ptA[tid * ns + k];
              }
            ab1 = pA[aob1 + tid]; aw2 = pA[aow2 + tid];
            if (!frz) { ab1t = ptA[aob1 + tid]; aw2t = ptA[aow2 + tid]; }
          }
        }
      } else if (isA) {
#pragma unroll
        for (int k = 0; k < KA; ++k)
          if (k < ns) s2_adam(aw1[k], aw1m[k], aw1v[k], aw1t[k], gw1[k], g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(ab1, ab1m, ab1v, ab1t, gb1, g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
        s2_adam(aw2, aw2m, aw2v, aw2t, gw2, g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      }
      s2_adam(ab2, ab2m, ab2v, ab2t, gb2, g.eta_a, g.b1, g.b2, g.eps, o1, o2, g.rho, omr, frz);
      bpa0 *= g.b1;
      bpa1 *= g.b2;
    }
  }
  // ---- write the learner state back
  if (isC) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k < K0) {
        g.C.p[tid * K0 + k] = cw1[k]; g.C.m[tid * K0 + k] = cw1m[k]; g.C.v[tid * K0 + k] = cw1v[k];
        if (!frz) g.C.pt[tid * K0 + k] = cw1t[k];
      }
    g.C.p[cob1 + tid] = cb1; g.C.m[cob1 + tid] = cb1m; g.C.v[cob1 + tid] = cb1v;
    if (!frz) g.C.pt[cob1 + tid] = cb1t;
    g.C.p[cow2 + tid] = cw2; g.C.m[cow2 + tid] = cw2m; g.C.v[cow2 + tid] = cw2v;
    if (!frz) g.C.pt[cow2 + tid] = cw2t;
  }
  if constexpr (OS > 0) {
#pragma unroll
    for (int j = 0; j < OS; ++j) {
      const int f = j * 64 + tid;
      if (tid < 64 && f < nown) {
        g.A.p[f] = op[j]; g.A.m[f] = om[j]; g.A.v[f] = ov[j];
        if (!frz) g.A.pt[f] = opt[j];
      }
    }
  } else if (isA) {
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (k < ns) {
        g.A.p[tid * ns + k] = aw1[k]; g.A.m[tid * ns + k] = aw1m[k]; g.A.v[tid * ns + k] = aw1v[k];
        if (!frz) g.A.pt[tid * ns + k] = aw1t[k];
      }
    g.A.p[aob1 + tid] = ab1; g.A.m[aob1 + tid] = ab1m; g.A.v[aob1 + tid] = ab1v;
    if (!frz) g.A.pt[aob1 + tid] = ab1t;
    g.A.p[aow2 + tid] = aw2; g.A.m[aow2 + tid] = aw2m; g.A.v[aow2 + tid] = aw2v;
    if (!frz) g.A.pt[aow2 + tid] = aw2t;
  }
  if (tid == 0) {
    g.C.p[cob2] = cb2; g.C.m[cob2] = cb2m; g.C.v[cob2] = cb2v;
    if (!frz) g.C.pt[cob2] = cb2t;
    g.A.p[aob2] = ab2; g.A.m[aob2] = ab2m; g.A.v[aob2] = ab2v;
    if (!frz) g.A.pt[aob2] = ab2t;
    if (g.losses) { g.losses[0] = closs; g.losses[1] = aloss; }
    g.bpA.next[0] = bpa0; g.bpA.next[1] = bpa1;
    g.bpC.next[0] = bpc0; g.bpC.next[1] = bpc1;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The same update for the reference's FROZEN target networks (rho == 1: the Polyak loop of src/PDEagent.jl:414-417 runs over an
// empty parameter list) -- the KS experiments' regime -- as TWO CHAINS SIDE BY SIDE.  With targets that never move
//   * the TD targets gamma (1 - t) Ct([s'; At(s')]) of all `loops` minibatches depend on nothing the launch changes: they are
//     computed once, up front, all columns at a time (one tanhf stream for all of them instead of three per update);
//   * a critic update reads the critic alone; an actor update reads the actor and the critic AFTER the critic update of the same
//     loop.  So the critic waves (one thread per critic unit, as above) run critic update i while ONE more wave, on the SIMD the
//     kernel above leaves idle, runs actor update i - 1 against the critic weights update i - 1 published in LDS (double
//     buffered): a lane of that wave holds the actor's unit `lane` and walks the critic's units lane, 64 + lane, ... for the
//     forward through the updated critic.  Two workgroup barriers per iteration (the critic's exchange, the hand-over), loops + 1
//     iterations; per iteration each wave issues about a third of what an update costs it above.
// Bit-identical to ddpg_small2_kernel at rho == 1: every sum is taken over the same lanes in the same order (the actor wave sums
// critic units r * 64 + lane by the wave tree and adds the rows r in order, which is what the cross-wave exchange above does), the
// expressions are the ones above (test_split_small_update_is_bit_identical).  Needs (KA + 2) nA + 1 <= 64 and nC <= 448; launched for the exact
// KS instantiation only (see the launch code).
// NWC: the number of critic waves, a compile-time constant (3 for the KS nets' 140 critic units): the row loop of the actor wave
// unrolls and its 18 wave sums interleave
template <int KC, int KA, int BUT, bool EXACT, int NWC>
__global__ __launch_bounds__(512) void ddpg_small2f_kernel(Small2Args a_m) {
  Small2Args a_in = a_m;
  if (a_in.g.pm && !sm_member_begin(a_in.g)) return;
  const SmallArgs& g = a_in.g;
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, nt = blockDim.x, nwc = NWC, wv = tid >> 6, lane = tid & 63;
  if (g.halt && *g.halt) {
    if (tid == 0) {
      g.bpA.next[0] = g.bpA.cur[0]; g.bpA.next[1] = g.bpA.cur[1];
      g.bpC.next[0] = g.bpC.cur[0]; g.bpC.next[1] = g.bpC.cur[1];
    }
    return;
  }
  const int Bu = EXACT ? BUT : g.Bu, ns = EXACT ? KA : g.ns, K0 = ns + 1, nC = a_in.nC, nA = a_in.nA;
  const bool actor_wave = wv == nwc;
  const bool isC = !actor_wave && tid < nC, isA = actor_wave && lane < nA;
  const int bstride = (2 * ns + 3) * Bu, ncol = g.loops * Bu, PUBN = nwc * 64, PUBS = (KC + 2) * PUBN + 4;
  float* batch = sm;
  float* red = batch + (size_t)g.loops * bstride;    // [2][S2_NW][S2_ROW]
  float* tq = red + 2 * S2_NW * S2_ROW;              // [ncol] Ct([s'; At(s')]) + b2t
  float* tan_ = tq + ncol;                           // [ncol] a' = tanh(At(s'))
  float* tpart = tan_ + ncol;                        // [S2_NW][ncol] wave sums of the target critic's output layer
  float* pub = tpart + S2_NW * ncol;                 // [2][PUBS]: W1 rows k (KC of them), b1, w2 by unit, then b2
  const int *i_s = g.i_s, *i_rt = g.i_rt, *i_sn = g.i_sn;
  if (g.smp_on) {
    int* tab = reinterpret_cast<int*>(sm + g.smp_lds);
    sm_draw_slots(g, tab, tid, nt);
    const int n = g.loops * g.Bu;
    i_s = tab; i_rt = tab + n; i_sn = tab + 2 * n;
    __syncthreads();
  }
  for (int idx = tid; idx < g.loops * ns * Bu; idx += nt) {
    const int it = idx / (ns * Bu), rem = idx - it * (ns * Bu), k = rem / Bu, c = rem - k * Bu;
    batch[it * bstride + rem] = g.state[(size_t)i_sn[it * Bu + c] * ns + k];
    batch[it * bstride + ns * Bu + rem] = g.state[(size_t)i_s[it * Bu + c] * ns + k];
  }
  for (int idx = tid; idx < g.loops * Bu; idx += nt) {
    const int it = idx / Bu, c = idx - it * Bu;
    float* b = batch + it * bstride + 2 * ns * Bu;
    b[c] = g.action[i_s[idx]];
    b[Bu + c] = g.reward[i_rt[idx]];
    b[2 * Bu + c] = g.terminal[i_rt[idx]];
  }
  // ---- this thread's unit (critic waves: critic unit tid; actor wave: actor unit lane)
  float cw1[KC], cw1m[KC], cw1v[KC], cw1t[KC], cb1 = 0, cb1m = 0, cb1v = 0, cb1t = 0, cw2 = 0, cw2m = 0, cw2v = 0, cw2t = 0;
  float aw1[KA], aw1t[KA], ab1 = 0, ab1t = 0, aw2 = 0, aw2t = 0;        // (the actor's moments: with their owner lanes, below)
  const int cob1 = nC * K0, cow2 = cob1 + nC, cob2 = cow2 + nC;
  const int aob1 = nA * ns, aow2 = aob1 + nA, aob2 = aow2 + nA;
  float cb2 = g.C.p[cob2], cb2m = g.C.m[cob2], cb2v = g.C.v[cob2], cb2t = g.C.pt[cob2];
  float ab2 = g.A.p[aob2], ab2t = g.A.pt[aob2];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const bool ok = isC && k < K0;
    cw1[k] = ok ? g.C.p[tid * K0 + k] : 0.f; cw1m[k] = ok ? g.C.m[tid * K0 + k] : 0.f;
    cw1v[k] = ok ? g.C.v[tid * K0 + k] : 0.f; cw1t[k] = ok ? g.C.pt[tid * K0 + k] : 0.f;
  }
  if (isC) {
    cb1 = g.C.p[cob1 + tid]; cb1m = g.C.m[cob1 + tid]; cb1v = g.C.v[cob1 + tid]; cb1t = g.C.pt[cob1 + tid];
    cw2 = g.C.p[cow2 + tid]; cw2m = g.C.m[cow2 + tid]; cw2v = g.C.v[cow2 + tid]; cw2t = g.C.pt[cow2 + tid];
  }
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const bool ok = isA && k < ns;
    aw1[k] = ok ? g.A.p[lane * ns + k] : 0.f;
    aw1t[k] = ok ? g.A.pt[lane * ns + k] : 0.f;
  }
  if (isA) {
    ab1 = g.A.p[aob1 + lane]; ab1t = g.A.pt[aob1 + lane];
    aw2 = g.A.p[aow2 + lane]; aw2t = g.A.pt[aow2 + lane];
  }
  // The actor's ADAM state lives ONE PARAMETER PER LANE of the actor wave: lane kind * nA + unit owns parameter `kind` (first-layer
  // weights 0 .. KA-1, then b1, then w2) of unit `unit`, lane (KA + 2) nA owns b2 -- (KA + 2) nA + 1 <= 64 lanes, one ADAM chain per
  // update instead of KA + 3 one after the other on nA lanes (the actor wave is the long pole of an iteration and ~45 % of its work
  // was these chains).  Gradients reach their owner and the new weights their unit by ds_bpermute; same arithmetic per parameter.
  constexpr int NP = KA + 2;
  const int okind = actor_wave ? lane / nA : 0, ounit = lane - okind * nA;
  const bool ownP = actor_wave && lane < NP * nA, ownB2 = actor_wave && lane == NP * nA;
  const int oidx = ownB2 ? aob2 : (okind < KA ? ounit * ns + okind : (okind == KA ? aob1 + ounit : aow2 + ounit));
  float op = 0.f, om = 0.f, ov = 0.f, opt_unused = 0.f;
  if ((ownP && (okind >= KA || okind < ns)) || ownB2) { op = g.A.p[oidx]; om = g.A.m[oidx]; ov = g.A.v[oidx]; }
  double bpa0 = g.bpA.cur[0], bpa1 = g.bpA.cur[1], bpc0 = g.bpC.cur[0], bpc1 = g.bpC.cur[1];
  const float invB = 1.f / (float)Bu;
  float closs = 0.f, aloss = 0.f;
  __syncthreads();                         // the batches are staged
  // ---- TD targets of every minibatch column, once.  a' = tanh(At(s')): actor wave, one tanhf stream over the columns.
  // Columns go four at a time: their wave sums are independent dependency chains (six DPP adds with hazard waits each) that
  // the scheduler interleaves inside one block -- one column per trip cost 15 us of the launch, a quarter of it.
  constexpr int PG = 4;
  if (actor_wave && nA <= 16) {
    // The actor's units fit one ROW of 16 lanes: a DPP chain then sums FOUR columns, one per row (unit lane & 15 of column ... + row;
    // the row totals at lanes 15 / 31 / 47 / 63 are formed exactly like the single row total of s2_wave_sum, whose two broadcast
    // steps only add the zeros of the empty rows) -- 16 columns per trip of four chains.
    const int ru = lane & 15, rr = lane >> 4;
    const bool isAr = ru < nA;
    float rw1[KA], rb1 = isAr ? g.A.pt[aob1 + ru] : 0.f, rw2 = isAr ? g.A.pt[aow2 + ru] : 0.f;
#pragma unroll
    for (int k = 0; k < KA; ++k) rw1[k] = (isAr && k < ns) ? g.A.pt[ru * ns + k] : 0.f;
    for (int col0 = 0; col0 < ncol; col0 += 64) {
      float mine = 0.f;
      const int nc = min(64, ncol - col0);
      for (int cc0 = 0; cc0 < nc; cc0 += 4 * PG) {
        float S[PG];
#pragma unroll
        for (int u = 0; u < PG; ++u) {
          const int col = min(col0 + cc0 + 4 * u + rr, ncol - 1), it = col / Bu, c = col - it * Bu;
          const float* bsn = batch + it * bstride;
          float zt = rb1;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) zt += rw1[k] * bsn[k * Bu + c];
          S[u] = s2_row_sum(isAr ? rw2 * fmaxf(zt, 0.f) : 0.f);
        }
#pragma unroll
        for (int u = 0; u < PG; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float T = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, S[u]), 16 * r + 15));
            if (lane == cc0 + 4 * u + r) mine = T;
          }
      }
      if (lane < nc) tan_[col0 + lane] = tanhf((0.f + mine) + ab2t);
    }
  } else if (actor_wave) {
    for (int col0 = 0; col0 < ncol; col0 += 64) {
      float mine = 0.f;
      const int nc = min(64, ncol - col0);
      for (int cc0 = 0; cc0 < nc; cc0 += PG) {
        float S[PG];
#pragma unroll
        for (int u = 0; u < PG; ++u) {
          const int col = min(col0 + cc0 + u, ncol - 1), it = col / Bu, c = col - it * Bu;
          const float* bsn = batch + it * bstride;
          float zt = ab1t;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) zt += aw1t[k] * bsn[k * Bu + c];
          S[u] = s2_wave_sum(isA ? aw2t * fmaxf(zt, 0.f) : 0.f);
        }
#pragma unroll
        for (int u = 0; u < PG; ++u)
          if (lane == cc0 + u) mine = S[u];
      }
      if (lane < nc) tan_[col0 + lane] = tanhf((0.f + mine) + ab2t);
    }
  }
  __syncthreads();
  // qt = Ct([s'; a']): critic waves (their threads hold the target critic's units), wave sums by column
  if (!actor_wave) {
    for (int col0 = 0; col0 < ncol; col0 += PG) {
      float S[PG];
#pragma unroll
      for (int u = 0; u < PG; ++u) {
        const int col = min(col0 + u, ncol - 1), it = col / Bu, c = col - it * Bu;
        const float* bsn = batch + it * bstride;
        const float an = tan_[col];
        float zt = cb1t;
#pragma unroll
        for (int k = 0; k < KC; ++k)
          if (k < ns) zt += cw1t[k] * bsn[k * Bu + c];
          else if (k == ns) zt += cw1t[k] * an;
        S[u] = s2_wave_sum(isC ? cw2t * fmaxf(zt, 0.f) : 0.f);
      }
      if (lane == 0)
#pragma unroll
        for (int u = 0; u < PG; ++u)
          if (col0 + u < ncol) tpart[wv * ncol + col0 + u] = S[u];
    }
  }
  __syncthreads();
  for (int col = tid; col < ncol; col += nt) {
    float a = 0.f;
    for (int w = 0; w < nwc; ++w) a += tpart[w * ncol + col];
    tq[col] = a + cb2t;
  }
  // (the first barrier of the loop below orders tq before its first reader)
  // ---- iteration i: critic update i (critic waves) beside actor update i - 1 (actor wave)
  for (int i = 0; i <= g.loops; ++i) {
    float* rb = red + (i & 1) * (S2_NW * S2_ROW);
    float* pw = pub + (i & 1) * PUBS;                 // the critic publishes update i here
    const float* pr = pub + ((i + 1) & 1) * PUBS;     // update i - 1, read by the actor wave
    if (!actor_wave) {
      if (i < g.loops) {
        const float* bs = batch + i * bstride + ns * Bu;
        const float* ba = bs + ns * Bu;
        const float* br = ba + Bu;
        const float* bt = br + Bu;
        // ---- q = C([s; a])  (src/PDEagent.jl:392)
        float h[BUT], v[BUT];
#pragma unroll
        for (int c = 0; c < BUT; ++c) {
          float z = cb1;
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k < ns) z += cw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
            else if (k == ns) z += cw1[k] * ba[c < Bu ? c : 0];
          const bool on = isC && c < Bu;
          h[c] = on ? fmaxf(z, 0.f) : 0.f;
          v[c] = cw2 * h[c];
        }
#pragma unroll
        for (int c = 0; c < BUT; ++c)
          if (c < Bu) v[c] = s2_wave_sum(v[c]);
        if (lane == 0)
#pragma unroll
          for (int c = 0; c < BUT; ++c) rb[wv * S2_ROW + c] = v[c];
        __syncthreads();                                 // barrier 1
        float part[S2_NW][BUT];
#pragma unroll
        for (int w = 0; w < S2_NW; ++w)
#pragma unroll
          for (int c = 0; c < BUT; ++c) part[w][c] = rb[w * S2_ROW + c];
#pragma unroll
        for (int c = 0; c < BUT; ++c) v[c] = 0.f;
#pragma unroll
        for (int w = 0; w < S2_NW; ++w)
          if (w < nwc) {
#pragma unroll
            for (int c = 0; c < BUT; ++c) v[c] += part[w][c];
          }
        float qt[BUT], dq[BUT];
#pragma unroll
        for (int c = 0; c < BUT; ++c) qt[c] = c < Bu ? tq[i * Bu + c] : 0.f;
        float rbar = 0.f;
        for (int c = 0; c < Bu; ++c) rbar += br[c];
        rbar *= invB;
        float loss = 0.f, gb2 = 0.f;
#pragma unroll
        for (int c = 0; c < BUT; ++c) {
          dq[c] = 0.f;
          if (c < Bu) {
            const float cc = g.gamma * (1.f - bt[c]) * qt[c] - (v[c] + cb2);
            if (g.quirk) {
              for (int j = 0; j < Bu; ++j) loss += (br[j] + cc) * (br[j] + cc);
            } else {
              loss += (br[c] + cc) * (br[c] + cc);
            }
            dq[c] = -(2.f * invB) * ((g.quirk ? rbar : br[c]) + cc);
            gb2 += dq[c];
          }
        }
        closs = g.quirk ? loss / (float)(Bu * Bu) : loss * invB;
        const double o1 = 1.0 / (1.0 - bpc0), o2 = 1.0 / (1.0 - bpc1);
        float gw2 = 0.f, gb1 = 0.f, gw1[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) gw1[k] = 0.f;
#pragma unroll
        for (int c = 0; c < BUT; ++c)
          if (c < Bu) {
            gw2 = fmaf(dq[c], h[c], gw2);
            const float dz = h[c] > 0.f ? cw2 * dq[c] : 0.f;
            gb1 += dz;
#pragma unroll
            for (int k = 0; k < KC; ++k)
              if (k < ns) gw1[k] = fmaf(dz, bs[k * Bu + c], gw1[k]);
              else if (k == ns) gw1[k] = fmaf(dz, ba[c], gw1[k]);
          }
        if (isC) {
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k < K0) s2_adam(cw1[k], cw1m[k], cw1v[k], cw1t[k], gw1[k], g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
          s2_adam(cb1, cb1m, cb1v, cb1t, gb1, g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
          s2_adam(cw2, cw2m, cw2v, cw2t, gw2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
        }
        s2_adam(cb2, cb2m, cb2v, cb2t, gb2, g.eta_c, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
        bpc0 *= g.b1;
        bpc1 *= g.b2;
        // publish the updated critic for the actor wave
#pragma unroll
        for (int k = 0; k < KC; ++k) pw[k * PUBN + tid] = cw1[k];
        pw[KC * PUBN + tid] = cb1;
        pw[(KC + 1) * PUBN + tid] = cw2;
        if (tid == 0) pw[(KC + 2) * PUBN] = cb2;
      } else {
        __syncthreads();                                 // barrier 1 of the last iteration (the actor wave's partner)
      }
    } else {
      __syncthreads();                                   // barrier 1: the critic's exchange
      if (i >= 1) {
        const int j = i - 1;
        const float* bs = batch + j * bstride + ns * Bu;
        // ---- A(s)  (src/PDEagent.jl:403)
        float ha[BUT], ao[BUT];
        float mine = 0.f;
#pragma unroll
        for (int c = 0; c < BUT; ++c) {
          float z = ab1;
#pragma unroll
          for (int k = 0; k < KA; ++k)
            if (k < ns) z += aw1[k] * bs[k * Bu + (c < Bu ? c : 0)];
          const bool on = isA && c < Bu;
          ha[c] = on ? fmaxf(z, 0.f) : 0.f;
          const float S = s2_wave_sum(aw2 * ha[c]);
          if (lane == c) mine = S;
        }
        {
          const float t = tanhf((0.f + mine) + ab2);      // lane c: tanh of column c -- one stream for the Bu columns
#pragma unroll
          for (int c = 0; c < BUT; ++c) ao[c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), c));
        }
        // ---- forward through the critic AFTER its update j: q on [s; A(s)] and da, rows r = units r * 64 + lane in order
        const float pcb2 = pr[(KC + 2) * PUBN];
        float vq[BUT], vd[BUT];
#pragma unroll
        for (int c = 0; c < BUT; ++c) vq[c] = vd[c] = 0.f;
#pragma unroll
        for (int r = 0; r < NWC; ++r) {
          const int u = r * 64 + lane;
          float w1[KC];
#pragma unroll
          for (int k = 0; k < KC; ++k) w1[k] = pr[k * PUBN + u];
          const float b1 = pr[KC * PUBN + u], w2 = pr[(KC + 1) * PUBN + u];
#pragma unroll
          for (int c = 0; c < BUT; ++c)
            if (c < Bu) {
              float z = b1;
#pragma unroll
              for (int k = 0; k < KC; ++k)
                if (k < ns) z += w1[k] * bs[k * Bu + c];
                else if (k == ns) z += w1[k] * ao[c];
              const bool on = u < nC;
              float wns = 0.f;
#pragma unroll
              for (int k = 0; k < KC; ++k)
                if (k == ns) wns = w1[k];
              vq[c] += s2_wave_sum(on ? w2 * fmaxf(z, 0.f) : 0.f);
              vd[c] += s2_wave_sum((on && z > 0.f) ? wns * w2 * (-invB) : 0.f);
            }
        }
        float sacc = 0.f;
        for (int c = 0; c < Bu; ++c) sacc += vq[c] + pcb2;
        aloss = -sacc * invB;
        const double o1 = 1.0 / (1.0 - bpa0), o2 = 1.0 / (1.0 - bpa1);
        float gw2 = 0.f, gb1 = 0.f, gb2 = 0.f, gw1[KA];
#pragma unroll
        for (int k = 0; k < KA; ++k) gw1[k] = 0.f;
#pragma unroll
        for (int c = 0; c < BUT; ++c)
          if (c < Bu) {
            const float dz2 = vd[c] * (1.f - ao[c] * ao[c]);      // tanh'
            gb2 += dz2;
            gw2 = fmaf(dz2, ha[c], gw2);
            const float dz = ha[c] > 0.f ? aw2 * dz2 : 0.f;
            gb1 += dz;
#pragma unroll
            for (int k = 0; k < KA; ++k)
              if (k < ns) gw1[k] = fmaf(dz, bs[k * Bu + c], gw1[k]);
          }
        {
          // gradients to their owner lanes (unit lanes hold gw1[k], gb1, gw2 of their unit; gb2 is the same in every lane)
          auto pull = [&](float x, int from) {
            return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from * 4, __builtin_bit_cast(int, x)));
          };
          float gown = gb2;
#pragma unroll
          for (int k = 0; k < KA; ++k) {
            const float t = pull(gw1[k], ounit);
            if (ownP && okind == k) gown = t;
          }
          {
            const float t1 = pull(gb1, ounit), t2 = pull(gw2, ounit);
            if (ownP && okind == KA) gown = t1;
            if (ownP && okind == KA + 1) gown = t2;
          }
          if ((ownP && (okind >= KA || okind < ns)) || ownB2)
            s2_adam(op, om, ov, opt_unused, gown, g.eta_a, g.b1, g.b2, g.eps, o1, o2, 1.f, 0.f, true);
          // the new weights back to their units
#pragma unroll
          for (int k = 0; k < KA; ++k) {
            const float t = pull(op, lane + k * nA);
            if (isA && k < ns) aw1[k] = t;
          }
          const float t1 = pull(op, lane + KA * nA), t2 = pull(op, lane + (KA + 1) * nA);
          if (isA) { ab1 = t1; aw2 = t2; }
          ab2 = pull(op, NP * nA);
        }
        bpa0 *= g.b1;
        bpa1 *= g.b2;
      }
    }
    __syncthreads();                                     // barrier 2: update i is published, update i - 1 has been read
  }
  // ---- write the learner state back (the targets keep their bits)
  if (isC) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k < K0) { g.C.p[tid * K0 + k] = cw1[k]; g.C.m[tid * K0 + k] = cw1m[k]; g.C.v[tid * K0 + k] = cw1v[k]; }
    g.C.p[cob1 + tid] = cb1; g.C.m[cob1 + tid] = cb1m; g.C.v[cob1 + tid] = cb1v;
    g.C.p[cow2 + tid] = cw2; g.C.m[cow2 + tid] = cw2m; g.C.v[cow2 + tid] = cw2v;
  }
  if ((ownP && (okind >= KA || okind < ns)) || ownB2) { g.A.p[oidx] = op; g.A.m[oidx] = om; g.A.v[oidx] = ov; }
  if (tid == 0) {
    g.C.p[cob2] = cb2; g.C.m[cob2] = cb2m; g.C.v[cob2] = cb2v;
    if (g.losses) g.losses[0] = closs;
    g.bpC.next[0] = bpc0; g.bpC.next[1] = bpc1;
  }
  if (actor_wave && lane == 0) {
    if (g.losses) g.losses[1] = aloss;
    g.bpA.next[0] = bpa0; g.bpA.next[1] = bpa1;
  }
}

// 2-layer relu/tanh actor [ns, h, 1] + relu/identity critic [ns+1, H, 1], H and h <= 512, ns <= 15, Bu <= S2_BU
static bool small2_ok(const Mlp* A, const Mlp* C, int Bu) {
  if (getenv("PDEC_SMALL_GENERIC")) return false;
  if (A->L != 2 || C->L != 2 || Bu > S2_BU) return false;
  if (A->dims[2] != 1 || C->dims[2] != 1 || C->dims[0] != A->dims[0] + 1 || A->dims[0] > 15) return false;
  if (A->acts[0] != PDEC_ACT_RELU || A->acts[1] != PDEC_ACT_TANH || C->acts[0] != PDEC_ACT_RELU || C->acts[1] != PDEC_ACT_IDENTITY)
    return false;
  return A->dims[1] <= 512 && C->dims[1] <= 512;
}

static int fill_net(SmallNet& n, Mlp* M, Mlp* T) {
  PDEC_REQUIRE(M->L <= SM_MAXL, "small update: at most %d layers", SM_MAXL);
  n.p = M->params.as<float>(); n.g = M->grads.as<float>(); n.m = M->m.as<float>(); n.v = M->v.as<float>();
  n.pt = T->params.as<float>();
  n.L = M->L; n.nparams = M->nparams;
  for (int l = 0; l <= M->L; ++l) n.dims[l] = M->dims[l];
  for (int l = 0; l < M->L; ++l) { n.acts[l] = M->acts[l]; n.woff[l] = (int)M->w_off[l]; n.boff[l] = (int)M->b_off[l]; }
  return PDEC_OK;
}

}  // namespace pdec

using namespace pdec;

struct SmallSampling {     // != null: draw the slots in the kernel (pdec_ddpg_update_small_rng)
  uint64_t seed, offset;
  int64_t n_valid, n_rt, capacity;
  int stride;
};

// Every register-kernel instantiation pdec_ddpg_update_small(_rng) and pdec_population_update can launch, X(id, reported name,
// kernel): the ONE list behind SmallKernelId, the names pdec_debug_small_update_kernel reports and the launch switch
// (small_launch).  small_plan() picks one; the launch sites and the query both go through it, so the query reports exactly
// what a call would launch.
#define SMALL2_KERNELS(X)                                                                       \
  X(S2F_2_1_3, "ddpg_small2f_kernel<2,1,3,1,3>", ddpg_small2f_kernel<2, 1, 3, true, 3>)         \
  X(S2_2_1_3, "ddpg_small2_kernel<2,1,3,1>", ddpg_small2_kernel<2, 1, 3, true>)                 \
  X(S2_13_12_3_OS5, "ddpg_small2_kernel<13,12,3,1,5>", ddpg_small2_kernel<13, 12, 3, true, 5>)  \
  X(S2_10_9_3_OS4, "ddpg_small2_kernel<10,9,3,1,4>", ddpg_small2_kernel<10, 9, 3, true, 4>)     \
  X(S2_13_12_3, "ddpg_small2_kernel<13,12,3,1>", ddpg_small2_kernel<13, 12, 3, true>)           \
  X(S2_10_9_3, "ddpg_small2_kernel<10,9,3,1>", ddpg_small2_kernel<10, 9, 3, true>)              \
  X(S2_4_3_4, "ddpg_small2_kernel<4,3,4,0>", ddpg_small2_kernel<4, 3, S2_BU, false>)            \
  X(S2_10_9_4, "ddpg_small2_kernel<10,9,4,0>", ddpg_small2_kernel<10, 9, S2_BU, false>)         \
  X(S2_13_12_4, "ddpg_small2_kernel<13,12,4,0>", ddpg_small2_kernel<13, 12, S2_BU, false>)      \
  X(S2_16_15_4, "ddpg_small2_kernel<16,15,4,0>", ddpg_small2_kernel<16, 15, S2_BU, false>)
static_assert(S2_BU == 4, "the reported names of the bounded instantiations spell S2_BU out");
enum SmallKernelId {
  SK_GENERIC,         // ddpg_small_kernel
#define X(ID, NAME, ...) SK_##ID,
  SMALL2_KERNELS(X)
#undef X
  SK_BATCHED,         // no kernel (not in the name table): reward groups that split the minibatch, served by the batched update
};
static const char* const small_kernel_names[] = {
    "ddpg_small_kernel",
#define X(ID, NAME, ...) NAME,
    SMALL2_KERNELS(X)
#undef X
};

struct SmallPlan {
  SmallKernelId id;
  int threads;              // block size
  size_t lds;               // dynamic LDS bytes of the launch (slot table included)
  int smp_lds;              // float offset of the slot table
  int lds_params;           // generic kernel: the learner state staged in LDS
  int maxw;                 // generic kernel: widest layer
};

// the kernel a call launches, its block and its dynamic LDS -- or the error the call raises.  Reads the env switches
// PDEC_SMALL_GENERIC / PDEC_SMALL_OWN / PDEC_SMALL_SPLIT per call (the identity tests switch them).  A broadcast target
// (quirk) whose reward groups (pdec_ddpg_set_reward_groups) split the minibatch -- 2 <= g, g L < Bu -- has no small kernel:
// SK_BATCHED, which the call refuses (the caller updates through pdec_ddpg_update_async); g = 1 is the diagonal target and
// g L >= Bu the whole-minibatch broadcast, both served by the small kernels as they are.
static int small_plan(const Mlp* A, const Mlp* C, int loops, int Bu, float rho, bool sampling, int quirk, SmallPlan* pl) {
  PDEC_REQUIRE(loops >= 1 && Bu >= 1 && Bu <= 16, "pdec_ddpg_update_small: needs 1 <= Bu <= 16 (got %d)", Bu);
  if (quirk && C->rg_g >= 2 && (int64_t)C->rg_g * C->rg_L < Bu) {
    *pl = SmallPlan{};
    pl->id = SK_BATCHED;
    return PDEC_OK;
  }
  PDEC_REQUIRE(A->L <= SM_MAXL && C->L <= SM_MAXL, "small update: at most %d layers", SM_MAXL);
  const int ns = A->dims[0];
  int maxw = 1;
  for (int l = 0; l <= A->L; ++l) maxw = std::max(maxw, A->dims[l]);
  for (int l = 0; l <= C->L; ++l) maxw = std::max(maxw, C->dims[l]);
  pl->maxw = maxw;
  size_t lds = ((size_t)(A->L + 1 + C->L + 1 + 2) * maxw * Bu + 3 * Bu + 4) * 4;
  PDEC_REQUIRE(lds <= 160 * 1024, "pdec_ddpg_update_small: layers too wide for the in-LDS activations (%zu B)", lds);
  const size_t lds_state = (size_t)5 * (((A->nparams + 3) & ~3) + ((C->nparams + 3) & ~3)) * 4;
  pl->lds_params = lds + lds_state <= 150 * 1024;
  if (pl->lds_params) lds += lds_state;
  const size_t tab_floats = sampling ? (size_t)3 * loops * Bu : 0;
  if (small2_ok(A, C, Bu) && (size_t)loops * (2 * ns + 3) * Bu * 4 <= 120 * 1024) {
    const int nC = C->dims[1], nA = A->dims[1];
    // the actor's ADAM state one parameter per lane of wave 0 (template OS slots) for the shipped moving-target shapes
    const char* noown = getenv("PDEC_SMALL_OWN");
    const int nown = (ns + 2) * nA;
    int os = 0;
    if (Bu == 3 && nA <= 64 && !(noown && noown[0] == '0')) {
      if (ns == 12 && nown <= 64 * 5) os = 5;             // Keller-Segel10_16: 14 x 20 parameters
      else if (ns == 9 && nown <= 64 * 4) os = 4;         // Fluid: 11 x 18
    }
    const size_t lds2f = (size_t)loops * (2 * ns + 3) * Bu + (size_t)2 * S2_NW * S2_ROW + (size_t)3 * 64 * os;   // + exchange buffers (+ owner rows)
    // frozen targets (the KS experiments' regime): the critic and the actor updates as two chains side by side (ddpg_small2f_kernel).
    // Only the exact KS instantiation (ns 1, batch 3, 129 - 192 critic units: KS22 / KS200 / KS500): there every guard folds at compile time and the
    // backend fuses multiplies and adds the same way in both kernels, which is what makes them agree bit for bit; the bounded
    // instantiations differ in the last place of the actor's gradient (a product fused into one kernel's sum and not the other's).
    const char* nosplit = getenv("PDEC_SMALL_SPLIT");
    const int nwc = (nC + 63) / 64;
    if (rho == 1.0f && Bu == 3 && ns == 1 && 3 * nA + 1 <= 64 && nwc == 3 && !(nosplit && nosplit[0] == '0')) {
      const int ncol = loops * Bu;
      const size_t ldsf = (size_t)loops * (2 * ns + 3) * Bu + (size_t)2 * S2_NW * S2_ROW + (size_t)ncol * (2 + S2_NW) +
                          (size_t)2 * ((2 + 2) * nwc * 64 + 4);
      if ((ldsf + tab_floats) * 4 <= 150 * 1024) {
        pl->id = SK_S2F_2_1_3; pl->threads = (nwc + 1) * 64; pl->smp_lds = (int)ldsf; pl->lds = (ldsf + tab_floats) * 4;
        return PDEC_OK;
      }
    }
    // the slot table sits behind the register kernel's LDS: it must fit in the workgroup's 160 KB, or the call takes the
    // generic kernel (which refuses cleanly when nothing fits)
    if ((lds2f + tab_floats) * 4 <= 160 * 1024) {
      pl->threads = (std::max(nC, nA) + 63) / 64 * 64;
      pl->smp_lds = (int)lds2f;
      pl->lds = (lds2f + tab_floats) * 4;
      if (Bu == 3 && ns == 1) pl->id = SK_S2_2_1_3;                      // KS22 / KS200 / KS500
      else if (Bu == 3 && ns == 12 && os == 5) pl->id = SK_S2_13_12_3_OS5;
      else if (Bu == 3 && ns == 9 && os == 4) pl->id = SK_S2_10_9_3_OS4;
      else if (Bu == 3 && ns == 12) pl->id = SK_S2_13_12_3;              // Keller-Segel10_16
      else if (Bu == 3 && ns == 9) pl->id = SK_S2_10_9_3;                // Fluid
      else if (ns <= 3) pl->id = SK_S2_4_3_4;
      else if (ns <= 9) pl->id = SK_S2_10_9_4;
      else if (ns <= 12) pl->id = SK_S2_13_12_4;
      else pl->id = SK_S2_16_15_4;
      return PDEC_OK;
    }
  }
  PDEC_REQUIRE(lds + tab_floats * 4 <= 160 * 1024, "pdec_ddpg_update_small: the slot table does not fit beside the learner state in LDS");
  pl->id = SK_GENERIC; pl->threads = SM_THREADS; pl->smp_lds = (int)(lds / 4); pl->lds = lds + tab_floats * 4;
  return PDEC_OK;
}

// do the kernels of this plan read a member's own gamma, rho and step sizes (sm_member_begin<HYPER>)?  All but the bounded
// instantiations of ddpg_small2_kernel
static bool small_serves_member_hyper(const SmallPlan& pl) {
  return !(pl.id == SK_S2_4_3_4 || pl.id == SK_S2_10_9_4 || pl.id == SK_S2_13_12_4 || pl.id == SK_S2_16_15_4);
}

// the shape checks of a small update on the four networks
static int small_nets(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, Mlp** pA, Mlp** pC, Mlp** pAt, Mlp** pCt) {
  Mlp* A = lookup_as<Mlp>(hA, Kind::Mlp);
  Mlp* C = lookup_as<Mlp>(hC, Kind::Mlp);
  Mlp* At = lookup_as<Mlp>(hAt, Kind::Mlp);
  Mlp* Ct = lookup_as<Mlp>(hCt, Kind::Mlp);
  if (!A || !C || !At || !Ct) { set_error("pdec_ddpg_update_small: bad network handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(A->dtype == PDEC_F32 && C->dtype == PDEC_F32 && At->dtype == PDEC_F32 && Ct->dtype == PDEC_F32,
               "pdec_ddpg_update_small: fp32 networks only (the reference's network dtype)");
  PDEC_REQUIRE(At->dims == A->dims && Ct->dims == C->dims, "ddpg: target networks must have the behaviour networks' shapes");
  const int ns = A->dims[0], na = A->dims[A->L];
  PDEC_REQUIRE(C->dims[0] == ns + na && C->dims[C->L] == 1, "ddpg: critic must map ns+na -> 1");
  PDEC_REQUIRE(A->stream == C->stream && At->stream == C->stream && Ct->stream == C->stream,
               "pdec_ddpg_update_small: the four networks must share one stream");
  *pA = A; *pC = C; *pAt = At; *pCt = Ct;
  return PDEC_OK;
}

// the fields of SmallArgs that a solo call and a population launch share; the caller adds its traces and slots, sampling
// bounds, beta-power slots and halt flag -- or the member table
static int small_args(SmallArgs& g, const SmallPlan& pl, Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, int loops, int Bu, double gamma,
                      double rho, int quirk, double eta_actor, double eta_critic) {
  int rc;
  if ((rc = fill_net(g.A, A, At)) || (rc = fill_net(g.C, C, Ct))) return rc;
  g.maxw = pl.maxw;
  g.lds_params = pl.lds_params;
  g.loops = loops; g.Bu = Bu; g.ns = A->dims[0]; g.na = A->dims[A->L];
  g.quirk = quirk && C->rg_g == 1 ? 0 : quirk;     // groups of one column: the diagonal target
  g.gamma = (float)gamma; g.rho = (float)rho;      // Float32 in the reference (y = 0.99f0, p = 0.995f0)
  g.eta_a = eta_actor; g.eta_c = eta_critic; g.b1 = 0.9; g.b2 = 0.999; g.eps = 1e-8;
  g.smp_lds = pl.smp_lds;
  return PDEC_OK;
}

// the plan's kernel on `grid` workgroups; allows the launch's dynamic LDS once per kernel (the register kernels ask for up to
// 160 KB)
static int small_launch(const SmallPlan& pl, dim3 grid, hipStream_t stream, const SmallArgs& g, int nA, int nC) {
  static size_t attr[SK_BATCHED] = {};
  auto go = [&](auto kern, int threads, size_t lds_attr, const auto& args) -> int {
    if (attr[pl.id] < lds_attr) {
      PDEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr));
      attr[pl.id] = lds_attr;
    }
    hipLaunchKernelGGL(kern, grid, dim3(threads), pl.lds, stream, args);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  };
  if (pl.id == SK_GENERIC) return go(ddpg_small_kernel, SM_THREADS, 160 * 1024, g);
  Small2Args a2{};
  a2.g = g;
  a2.g.lds_params = 0;
  a2.nC = nC; a2.nA = nA;
  switch (pl.id) {
#define X(ID, NAME, ...) case SK_##ID: return go(__VA_ARGS__, pl.threads, pl.lds, a2);
    SMALL2_KERNELS(X)
#undef X
    default: set_error("small update: no kernel for plan %d", (int)pl.id); return PDEC_E_INVALID;
  }
}

static int ddpg_update_small_impl(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* state_trace,
                                  const void* action_trace, const void* reward_trace, const void* terminal_trace,
                                  const int32_t* idx_s, const int32_t* idx_rt, const int32_t* idx_sn, int loops, int Bu,
                                  double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                                  void* losses_dev, const SmallSampling* smp) {
  Mlp *A, *C, *At, *Ct;
  int rc;
  if ((rc = small_nets(hA, hC, hAt, hCt, &A, &C, &At, &Ct))) return rc;
  PDEC_REQUIRE(state_trace && action_trace && reward_trace && terminal_trace && (smp || (idx_s && idx_rt && idx_sn)),
               "pdec_ddpg_update_small: null argument");
  SmallPlan pl{};
  if ((rc = small_plan(A, C, loops, Bu, (float)rho, smp != nullptr, quirk, &pl))) return rc;
  PDEC_REQUIRE(pl.id != SK_BATCHED,
               "pdec_ddpg_update_small: reward groups g = %d, L = %d split the minibatch of %d; update through pdec_ddpg_update_async",
               C->rg_g, C->rg_L, Bu);
  SmallArgs g{};
  if ((rc = small_args(g, pl, A, C, At, Ct, loops, Bu, gamma, rho, quirk, eta_actor, eta_critic))) return rc;
  g.state = (const float*)state_trace; g.action = (const float*)action_trace;
  g.reward = (const float*)reward_trace; g.terminal = (const float*)terminal_trace;
  g.i_s = idx_s; g.i_rt = idx_rt; g.i_sn = idx_sn;
  if (smp) {
    const int64_t hi = smp->n_valid - smp->stride;           // inds in 1:length(t)-number_actuators (src/PDEagent.jl:318)
    PDEC_REQUIRE(hi >= 1 && hi < ((int64_t)1 << 32) && smp->capacity >= 1 && smp->stride >= 0,
                 "pdec_ddpg_update_small_rng: nothing to sample (valid %lld, stride %d)", (long long)smp->n_valid, smp->stride);
    g.smp_on = 1;
    g.smp_seed = smp->seed; g.smp_offset = smp->offset; g.smp_hi = (uint32_t)hi;
    g.smp_base = smp->n_rt > smp->capacity ? smp->n_rt - smp->capacity : 0;      // logical index of the oldest entry
    g.smp_cap = (int)smp->capacity; g.smp_cap1 = (int)(smp->capacity + smp->stride); g.smp_stride = smp->stride;
  }
  if ((rc = bp_begin(A, g.b1, g.b2, &g.bpA)) || (rc = bp_begin(C, g.b1, g.b2, &g.bpC))) return rc;
  g.losses = (float*)losses_dev;
  g.halt = C->halt;
  ProfScope ps(C, "ddpg_small");
  if ((rc = small_launch(pl, dim3(1), C->stream, g, A->dims[1], C->dims[1]))) return rc;
  bp_done(A);
  bp_done(C);
  A->fw_dirty = C->fw_dirty = At->fw_dirty = Ct->fw_dirty = true;
  return PDEC_OK;
}

// one launch of M workgroups: member m's small update with device-side sampling where its own trigger fires (sm_member_begin)
extern "C" int pdec_population_update(pdec_handle pop) {
  GET_POP(P, pop);
  Mlp *A = P->A[0], *C = P->C[0];
  SmallPlan pl{};
  int rc;
  if ((rc = small_plan(A, C, P->loops, P->Bu, (float)P->rho, true, P->quirk, &pl))) return rc;
  PDEC_REQUIRE(pl.id != SK_BATCHED, "pdec_population_update: reward groups that split the minibatch are not served");
  SmallArgs g{};
  if ((rc = small_args(g, pl, A, C, P->At[0], P->Ct[0], P->loops, P->Bu, P->gamma, P->rho, P->quirk, P->eta_a, P->eta_c))) return rc;
  g.smp_on = 1;
  g.smp_cap = (int)P->cap; g.smp_cap1 = (int)P->cap1; g.smp_stride = P->stride;
  g.pm = P->tab.as<PopMember>(); g.rows = P->rows;
  g.m_after = P->after; g.m_freq = P->freq; g.m_dsample = ((long long)P->loops * P->Bu + 3) / 4;
  PDEC_REQUIRE(!P->member_hyper || small_serves_member_hyper(pl),
               "pdec_population_update: %s does not serve per-member hyper-parameters (pdec_population_set_member_hyper)",
               small_kernel_names[pl.id]);
  g.m_hyper = P->member_hyper;
  ProfScope ps(P, "population_update");
  return small_launch(pl, dim3(P->M), P->stream, g, A->dims[1], C->dims[1]);
}

extern "C" int pdec_population_set_member_hyper(pdec_handle pop, int on) {
  GET_POP(P, pop);
  if (on) {
    SmallPlan pl{};
    int rc;
    if ((rc = small_plan(P->A[0], P->C[0], P->loops, P->Bu, (float)P->rho, true, P->quirk, &pl))) return rc;
    PDEC_REQUIRE(pl.id != SK_BATCHED && small_serves_member_hyper(pl),
                 "pdec_population_set_member_hyper: the update kernel of these networks (%s) takes one gamma, rho and pair of step "
                 "sizes for the whole launch: members of this shape cannot differ in them",
                 pl.id == SK_BATCHED ? "reward groups" : small_kernel_names[pl.id]);
  }
  P->member_hyper = on ? 1 : 0;
  return PDEC_OK;
}

extern "C" int pdec_debug_small_update_kernel(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, int loops, int Bu,
                                              double rho, int sampling, char* name, int name_len, int64_t* lds_bytes) {
  Mlp *A, *C, *At, *Ct;
  int rc;
  PDEC_REQUIRE(name && name_len > 0 && lds_bytes, "pdec_debug_small_update_kernel: null argument");
  if ((rc = small_nets(hA, hC, hAt, hCt, &A, &C, &At, &Ct))) return rc;
  SmallPlan pl{};
  if ((rc = small_plan(A, C, loops, Bu, (float)rho, sampling != 0, 1, &pl))) return rc;   // as a broadcast-target call would
  if (pl.id == SK_BATCHED) snprintf(name, name_len, "generic_path/reward_groups");
  else if (pl.id == SK_GENERIC) snprintf(name, name_len, "ddpg_small_kernel/lds_params=%d", pl.lds_params);
  else snprintf(name, name_len, "%s", small_kernel_names[pl.id]);
  *lds_bytes = (int64_t)pl.lds;
  return PDEC_OK;
}

extern "C" int pdec_ddpg_update_small(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* state_trace,
                                      const void* action_trace, const void* reward_trace, const void* terminal_trace,
                                      const int32_t* idx_s, const int32_t* idx_rt, const int32_t* idx_sn, int loops, int Bu,
                                      double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                                      void* losses_dev) {
  return ddpg_update_small_impl(hA, hC, hAt, hCt, state_trace, action_trace, reward_trace, terminal_trace, idx_s, idx_rt, idx_sn,
                                loops, Bu, gamma, rho, quirk, eta_actor, eta_critic, losses_dev, nullptr);
}

extern "C" int pdec_ddpg_update_small_rng(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* state_trace,
                                          const void* action_trace, const void* reward_trace, const void* terminal_trace,
                                          int loops, int Bu, uint64_t seed, uint64_t offset, int64_t n_valid, int64_t n_rt,
                                          int64_t capacity, int stride, double gamma, double rho, int quirk, double eta_actor,
                                          double eta_critic, void* losses_dev) {
  SmallSampling smp{seed, offset, n_valid, n_rt, capacity, stride};
  return ddpg_update_small_impl(hA, hC, hAt, hCt, state_trace, action_trace, reward_trace, terminal_trace, nullptr, nullptr, nullptr,
                                loops, Bu, gamma, rho, quirk, eta_actor, eta_critic, losses_dev, &smp);
}
