// small_args.hpp -- what the three kernels of the small DDPG update (small_generic.hpp, small2.hpp, small2f.hpp) and their host
// code (mlp_small.hip) share: the launch arguments, the population member's prologue, the halt prologue, the slot table of the
// in-kernel sampler, and the dynamic-LDS layouts small_plan sizes the launches from (the register kernels carve from theirs).
#pragma once
#include "common.hpp"
#include "population.hpp"

namespace pdec {

#define SM_THREADS 256
#define SM_MAXL 4
#define S2_BU 4            // most minibatch columns the register-resident kernels hold (reference: batch_size = 3)

// Cross-wave exchange buffers of the register kernels: [2][S2_NW][S2_ROW] floats of LDS -- a row per wave, padded to 32 bytes,
// always eight rows (a workgroup has at most 512 threads) so that the combining reads (s2_reduce2) are unconditional vector reads
// issued together: one LDS round trip per exchange.  (Round 5 form: a loop over the waves with one load and one wait per partial,
// and the buffer picked through a two-pointer array that the compiler could no longer prove to be LDS -- 18 dependent FLAT loads
// per exchange, which was two thirds of the 4.6 us an update took.)
#define S2_NW 8
#define S2_ROW (2 * S2_BU)

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

struct Small2Args {
  SmallArgs g;
  int nC, nA;              // hidden widths
};

// ---- dynamic LDS, in floats from the start of the workgroup's allocation.  The register kernels carve their regions from their
// layout and small_plan takes the launch's bytes, the slot table's offset (`end`: the table sits behind everything else) and the
// 150 / 160 KB decisions from the same object, so the two sides cannot disagree.

// ddpg_small_kernel: actor activations aA[0 .. A.L], critic activations aC[0 .. C.L] and two dz buffers of buf(maxw, Bu) floats
// each, three batch scalars per column (r, t, qt), RED floats for the losses (end_act); behind them, when it is staged
// (lds_params), the learner state, five regions per network of pad(nparams) floats (end).  That kernel keeps walking a pointer
// over these regions -- its arrays of activation pointers live in scratch, and carved from offsets it took 4 more VGPRs
//  -- so the two sides share the terms (buf, RED, pad), not the sum: the order and the number of the regions are
// stated here for the host and by the walk for the kernel.
struct SmallLds {
  enum { RED = 4 };
  template <class T = int>      // (the kernel's int; the host sizes shapes that do not fit, in size_t)
  static __host__ __device__ constexpr T buf(int maxw, int Bu) { return (T)maxw * Bu; }                 // an activation buffer
  static __host__ __device__ constexpr int pad(int nparams) { return (nparams + 3) & ~3; }            // a state region: 16 bytes
  size_t end_act, end;
  SmallLds(int AL, int CL, int maxw, int Bu, int nparamsA, int nparamsC) {
    end_act = (size_t)(AL + 1 + CL + 1 + 2) * buf<size_t>(maxw, Bu) + 3 * Bu + RED;
    end = end_act + (size_t)5 * (pad(nparamsA) + pad(nparamsC));
  }
};

// ddpg_small2_kernel: the minibatches of all loops, the exchange buffers, and with OS > 0 the owner lanes' rows
struct Small2Lds {
  int bstride;              // per loop: s' [ns][Bu], s [ns][Bu], a [Bu], r [Bu], t [Bu]
  size_t batch, red, xg, end;
  __host__ __device__ Small2Lds(int loops, int ns, int Bu, int OS) {
    bstride = (2 * ns + 3) * Bu;
    batch = 0;
    red = batch + (size_t)loops * bstride;       // [2][S2_NW][S2_ROW]
    xg = red + 2 * S2_NW * S2_ROW;               // OS > 0: [3][64 OS] gradients / new parameters / new targets by flat index
    end = xg + (size_t)3 * 64 * OS;
  }
};

// ddpg_small2f_kernel: the same batches and exchange buffers, the up-front TD targets, and the critic the critic waves publish
// for the actor wave (KC first-layer rows, b1 and w2 by unit over nwc waves of units, then b2; double buffered)
struct Small2fLds {
  int bstride, ncol, pubn, pubs;
  size_t batch, red, tq, tan_, tpart, pub, end;
  __host__ __device__ Small2fLds(int loops, int ns, int Bu, int KC, int nwc) {
    bstride = (2 * ns + 3) * Bu;
    ncol = loops * Bu;
    pubn = nwc * 64;
    pubs = (KC + 2) * pubn + 4;
    batch = 0;
    red = batch + (size_t)loops * bstride;       // [2][S2_NW][S2_ROW]
    tq = red + 2 * S2_NW * S2_ROW;               // [ncol] Ct([s'; At(s')]) + b2t
    tan_ = tq + ncol;                            // [ncol] a' = tanh(At(s'))
    tpart = tan_ + ncol;                         // [S2_NW][ncol] wave sums of the target critic's output layer
    pub = tpart + (size_t)S2_NW * ncol;          // [2][pubs]: W1 rows k (KC of them), b1, w2 by unit, then b2
    end = pub + (size_t)2 * pubs;
  }
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
// conversions small_args applies to them -- every kernel reads them from its copy of g behind this prologue (omr, frz and
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

// the episode ended before this step: only the beta powers move on to the slot the host flipped to, and the workgroup returns
__device__ __forceinline__ bool sm_halted(const SmallArgs& g, int tid) {
  if (!(g.halt && *g.halt)) return false;
  if (tid == 0) {
    g.bpA.next[0] = g.bpA.cur[0]; g.bpA.next[1] = g.bpA.cur[1];
    g.bpC.next[0] = g.bpC.cur[0]; g.bpC.next[1] = g.bpC.cur[1];
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

// the launch's slot tables: the caller's, or (smp_on) drawn into the workgroup's LDS `sm` at g.smp_lds, behind a barrier
struct SmSlots {
  const int *i_s, *i_rt, *i_sn;
};
__device__ __forceinline__ SmSlots sm_slots(const SmallArgs& g, float* sm, int tid, int nt) {
  SmSlots s{g.i_s, g.i_rt, g.i_sn};
  if (g.smp_on) {
    int* tab = reinterpret_cast<int*>(sm + g.smp_lds);
    sm_draw_slots(g, tab, tid, nt);
    const int n = g.loops * g.Bu;
    s.i_s = tab; s.i_rt = tab + n; s.i_sn = tab + 2 * n;
    __syncthreads();
  }
  return s;
}

}  // namespace pdec
