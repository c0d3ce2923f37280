// env_sense.hpp -- device pieces every 1-D environment kernel shares: sensor dots, actuation, reward, featurize, block
// reductions and the terminal flags (ks_step.hip, ks_rollout.hip, kseg.hip, ksfd.hip, env.hip: sense_kernel)
#pragma once
#include "env.hpp"

namespace pdec {

// ------------------------------------------------------------------ shared device pieces
// sense_dots, reward_traj and reward_pair may be called with tid = SUM_IDLE_TID by threads that take no part in the sums (the
// second wave of the two-wave KS step, ks_step.hip): such a thread must do nothing but meet the barriers.  So in these three
// `tid` is only ever the start of a `for (i = tid; i < bound; i += nt)` loop or compared with 0 -- never scaled, never an index
// outside such a loop (the value leaves room for bounds up to 2^28 and for `tid + nt` without overflow).
constexpr int SUM_IDLE_TID = 1 << 28;

// dots[r][s] = sum_j Gs[j][s] * y_r[(sn0[s]+j) mod N] for r in {0,1}; yf(r,n) reads LDS.  Threads
// are split into groups that each cover a slice of the window; partials are combined via `part`.
template <class T, class YF>
__device__ __forceinline__ void sense_dots(const EnvDev<T>& e, YF yf, T* dots, T* part, int tid, int nt) {
  const int S = e.S, N = e.N, Wd = e.Wd;
  int ng = nt / S;
  if (ng < 1) ng = 1;
  if (ng > 8) ng = 8;
  const int chunk = (Wd + ng - 1) / ng;
  for (int idx = tid; idx < ng * S; idx += nt) {
    const int grp = idx / S, s = idx - grp * S;
    int j0 = grp * chunk, j1 = j0 + chunk;
    if (j1 > Wd) j1 = Wd;
    int n = e.sn0[s] + j0;
    if (n >= N) n -= N;
    // eight table rows in flight and four independent partial sums per trajectory: the loop used to be one load-to-use
    // latency per row (11 k cycles of the 77 k-cycle C2 step for a 90-row band)
    T p0[4] = {0, 0, 0, 0}, p1[4] = {0, 0, 0, 0};
    int j = j0;
    for (; j + 8 <= j1; j += 8) {
      T gk[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) gk[u] = e.Gs[(size_t)(j + u) * S + s];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int nn = n + u;
        nn = nn >= N ? nn - N : nn;
        p0[u & 3] += gk[u] * yf(0, nn);
        p1[u & 3] += gk[u] * yf(1, nn);
      }
      n += 8;
      if (n >= N) n -= N;
    }
    for (; j < j1; ++j) {
      const T gk = e.Gs[(size_t)j * S + s];
      p0[0] += gk * yf(0, n);
      p1[0] += gk * yf(1, n);
      if (++n == N) n = 0;
    }
    part[(grp * 2 + 0) * S + s] = (p0[0] + p0[1]) + (p0[2] + p0[3]);
    part[(grp * 2 + 1) * S + s] = (p1[0] + p1[1]) + (p1[2] + p1[3]);
  }
  __syncthreads();
  for (int idx = tid; idx < 2 * S; idx += nt) {
    T acc = 0;
    for (int grp = 0; grp < ng; ++grp) acc += part[grp * 2 * S + idx];
    dots[idx] = acc;
  }
  __syncthreads();
}

template <class T>
__device__ __forceinline__ T pow_abs(T d, T p) {
  d = d < 0 ? -d : d;
  if (p == (T)2) return d * d;
  if (p == (T)1) return d;
  return d == 0 ? (T)0 : (T)pow((double)d, (double)p);
}
template <>
__device__ __forceinline__ float pow_abs<float>(float d, float p) {
  d = fabsf(d);
  if (p == 2.0f) return d * d;
  if (p == 1.0f) return d;
  return d == 0.0f ? 0.0f : powf(d, p);
}

// reward_function for one trajectory: dots = <y, g_s> of the species the reward looks at
// (returns the sum of the rewards THIS thread wrote, for the optional per-workgroup reward sum)
template <class T>
__device__ __forceinline__ T reward_traj(const EnvDev<T>& e, const T* dots, const T* act, const T* actp,
                                         T* r_out, int tid, int nt) {
  T mine = 0;
  if (!e.mono) {
    for (int a = tid; a < e.A; a += nt) {
      const int s = e.a2s[a];
      const T d = e.r_in_scale * (dots[s] + e.r_offset * e.gsum[s]);
      const T da = act[a] - actp[a];
      const T r = -pow_abs<T>(d, e.r_power) / e.r_denom - e.a_pun * act[a] * act[a] - e.da_pun * da * da;
      r_out[a] = r;
      mine += r;
    }
  } else if (tid == 0) {
    T acc = 0;
    for (int a = 0; a < e.A; ++a) {
      const int s = e.a2s[a];
      const T d = e.r_in_scale * (dots[s] + e.r_offset * e.gsum[s]);
      const T da = act[a] - actp[a];
      acc += -pow_abs<T>(d, e.r_power) / e.r_denom - e.a_pun * act[a] * act[a] - e.da_pun * da * da;
    }
    r_out[0] = acc / (T)e.A;
    mine = acc / (T)e.A;
  }
  return mine;
}

// featurize for one trajectory.  dots: [n_species][S]; state/prev: [A][ns] (or [1][S] mono)
template <class T>
__device__ __forceinline__ void featurize_traj(const EnvDev<T>& e, const T* dots, const T* prev, T* state,
                                               int tid, int nt) {
  if (e.mono) {
    for (int s = tid; s < e.S; s += nt) state[s] = dots[s] * e.sensor_scale;
    return;
  }
  if (e.fmap) {                         // temporal_steps == 1: every row is fresh -- one gather through the map built at creation (the general
    const int tot = e.A * e.ns;         // path below spends ~40 instructions per element on divisions by run-time values)
    for (int idx = tid; idx < tot; idx += nt) state[idx] = dots[e.fmap[idx]] * e.sensor_scale;
    return;
  }
  const int w = e.window / 2;
  const int fresh = e.window * e.n_species;
  for (int idx = tid; idx < e.A * e.ns; idx += nt) {
    const int a = idx / e.ns, rr = idx - a * e.ns;
    T v;
    if (rr < fresh || prev == nullptr) {
      const int r0 = rr % fresh;
      const int sp = r0 / e.window, i = (r0 - sp * e.window) - w;
      int s = (e.a2s[a] - i) % e.S;
      if (s < 0) s += e.S;
      v = dots[sp * e.S + s] * e.sensor_scale;
    } else {
      v = prev[a * e.ns + (rr - fresh)];
    }
    state[idx] = v;
  }
}

// featurize with action memory (cfg.memory_size > 0; KSSetup.jl:190-229 with :216 and :220-226): columns are
// [fresh window rows | the previous state's rows minus its oldest block and its memory rows | memory rows], the memory rows =
// rows 1.. of the action just applied (actg [A][na]; null = reset form, featurize(y0) without env: zeros).  Kept apart from
// featurize_traj so that the fused step kernels stay what they were, instruction for instruction.
template <class T>
__device__ __forceinline__ void featurize_traj_mem(const EnvDev<T>& e, const T* dots, const T* prev, const T* actg, T* state,
                                                   int tid, int nt) {
  const int w = e.window / 2;
  const int fresh = e.window * e.n_species, body = e.ns - e.mem;
  for (int idx = tid; idx < e.A * e.ns; idx += nt) {
    const int a = idx / e.ns, rr = idx - a * e.ns;
    T v;
    if (rr >= body) {
      v = actg ? actg[(size_t)a * e.na + 1 + (rr - body)] : (T)0;
    } else if (rr < fresh || prev == nullptr) {
      const int r0 = rr % fresh;
      const int sp = r0 / e.window, i = (r0 - sp * e.window) - w;
      int sidx = (e.a2s[a] - i) % e.S;
      if (sidx < 0) sidx += e.S;
      v = dots[sp * e.S + sidx] * e.sensor_scale;
    } else {
      v = prev[(size_t)a * e.ns + (rr - fresh)];
    }
    state[idx] = v;
  }
}

// reward + featurize of the TWO trajectories of a workgroup in one pass each (per-actuator agents, temporal_steps == 1): the
// table loads (a2s, gsum, fmap) are shared and the two trajectories' load-to-use latencies overlap instead of following
// each other (3.6 k + 2.2 k cycles of the C2 step as four separate loops).  Same arithmetic per element as reward_traj /
// featurize_traj.  r1 / st1 null: single trajectory.
template <class T>
__device__ __forceinline__ T reward_pair(const EnvDev<T>& e, const T* dots0, const T* dots1, const T* act0, const T* act1,
                                         const T* actp0, const T* actp1, T* r0, T* r1, int tid, int nt) {
  T mine = 0;
  for (int a = tid; a < e.A; a += nt) {
    const int s = e.a2s[a];
    const T off = e.r_offset * e.gsum[s];
    const T d0 = e.r_in_scale * (dots0[s] + off);
    const T da0 = act0[a] - actp0[a];
    const T v0 = -pow_abs<T>(d0, e.r_power) / e.r_denom - e.a_pun * act0[a] * act0[a] - e.da_pun * da0 * da0;
    r0[a] = v0;
    mine += v0;
    if (r1) {
      const T d1 = e.r_in_scale * (dots1[s] + off);
      const T da1 = act1[a] - actp1[a];
      const T v1 = -pow_abs<T>(d1, e.r_power) / e.r_denom - e.a_pun * act1[a] * act1[a] - e.da_pun * da1 * da1;
      r1[a] = v1;
      mine += v1;
    }
  }
  return mine;
}
template <class T>
__device__ __forceinline__ void featurize_pair(const EnvDev<T>& e, const T* dots0, const T* dots1, T* st0, T* st1, int tid, int nt) {
  const int tot = e.A * e.ns;
  for (int idx = tid; idx < tot; idx += nt) {
    const int m = e.fmap[idx];
    st0[idx] = dots0[m] * e.sensor_scale;
    if (st1) st1[idx] = dots1[m] * e.sensor_scale;
  }
}

// p[n] = agent_power * sum_i act[(an0[n]+i) mod A] * GaC[i][n]
template <class T>
__device__ __forceinline__ T actuate_cell(const EnvDev<T>& e, const T* act, int n) {
  T acc = 0;
  int a = e.an0[n];
  for (int i = 0; i < e.Cnt; ++i) {
    acc += act[a] * e.GaC[(size_t)i * e.N + n];
    if (++a == e.A) a = 0;
  }
  return acc * e.agent_power;
}
// two trajectories at once (shared table loads)
template <class T>
__device__ __forceinline__ void actuate_cell2(const EnvDev<T>& e, const T* act0, const T* act1, int n, T& p0, T& p1) {
  T a0 = 0, a1 = 0;
  int a = e.an0[n];
  for (int i = 0; i < e.Cnt; ++i) {
    const T gk = e.GaC[(size_t)i * e.N + n];
    a0 += act0[a] * gk;
    a1 += act1[a] * gk;
    if (++a == e.A) a = 0;
  }
  p0 = a0 * e.agent_power;
  p1 = a1 * e.agent_power;
}

// the KS_MPT cells a lane owns at once: their table rows are independent loads (one per cell and table row in flight
// together, two rows unrolled) instead of one load-to-use latency per cell and row -- 5.4 k -> the C2 step's actuation;
// per cell the sum runs over the rows in the same order as actuate_cell2
template <class T, int M>
__device__ __forceinline__ void actuate_cells(const EnvDev<T>& e, const T* act0, const T* act1, const int (&n)[M], T (&p0)[M],
                                              T (&p1)[M]) {
  int a[M];
  bool ok[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    ok[j] = n[j] < e.N;
    a[j] = ok[j] ? e.an0[n[j]] : 0;
    p0[j] = 0; p1[j] = 0;
  }
#pragma unroll 2
  for (int i = 0; i < e.Cnt; ++i) {
    T gk[M];
#pragma unroll
    for (int j = 0; j < M; ++j) gk[j] = ok[j] ? e.GaC[(size_t)i * e.N + n[j]] : (T)0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      p0[j] += act0[a[j]] * gk[j];
      p1[j] += act1[a[j]] * gk[j];
      if (++a[j] == e.A) a[j] = 0;
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) { p0[j] *= e.agent_power; p1[j] *= e.agent_power; }
}

// All cells of both trajectories with FOUR CONSECUTIVE cells per lane: one 16/32-byte load per table row and lane (the rows
// of a lane's cells tid + 64 j are four separate 4-byte loads: 92 loads per lane at C2, 5 k cycles of load-to-use
// latency), results through an LDS scratch [2][N] from which every lane then takes the cells its transform owns.
// Per cell the sum runs over the rows in the order of actuate_cell2.  Needs N % 4 == 0.
template <class T>
__device__ __forceinline__ void actuate_consecutive(const EnvDev<T>& e, const T* act0, const T* act1, T* scratch, int tid, int nt) {
  typedef T T4 __attribute__((ext_vector_type(4)));
  const int N = e.N, A = e.A;
  for (int c0 = 4 * tid; c0 < N; c0 += 4 * nt) {
    int a[4];
    T p0[4] = {0, 0, 0, 0}, p1[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = e.an0[c0 + u];
#pragma unroll 4
    for (int i = 0; i < e.Cnt; ++i) {
      const T4 g = *reinterpret_cast<const T4*>(e.GaC + (size_t)i * N + c0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        p0[u] += act0[a[u]] * g[u];
        p1[u] += act1[a[u]] * g[u];
        if (++a[u] == A) a[u] = 0;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      scratch[c0 + u] = p0[u] * e.agent_power;
      scratch[N + c0 + u] = p1[u] * e.agent_power;
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ faults (pdec_env_set_faults), FLT instantiations only
// The two modifications of KSSetup.jl:190-245 are made on the ARRAYS the helpers above read, so the helpers themselves serve
// the healthy and the faulty kernels alike: the actuation reads the applied action gain[b][a] * action[a], featurize reads
// the sensor dots gain[b][s] * dot_s + bias[b][s] (indexed by the sensor, so a window row takes its own sensor's fault; the
// bias in units of the field, before sensor_scale).  The reward reads the commanded action and the true dots.
template <class T>
__device__ __forceinline__ T fault_action(const FaultDev<T>& f, int b, int A, int a, T v) {
  return f.act_gain ? f.act_gain[(size_t)b * A + a] * v : v;
}
template <class T>
__device__ __forceinline__ void fault_dots(const FaultDev<T>& f, int b, int S, const T* dots, T* out, int tid, int nt) {
  for (int s = tid; s < S; s += nt) {
    T v = dots[s];
    if (f.sens_gain) v = f.sens_gain[(size_t)b * S + s] * v;
    if (f.sens_bias) v = v + f.sens_bias[(size_t)b * S + s];
    out[s] = v;
  }
}

template <class T>
__device__ __forceinline__ T block_max(T v, T* red, int tid, int nt) {
  for (int off = 32; off > 0; off >>= 1) {
    T o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  T r = red[0];
  for (int i = 1; i < (nt + 63) / 64; ++i) r = red[i] > r ? red[i] : r;
  __syncthreads();
  return r;
}

// per-column terminal flags for the DDPG batch (every actuator column of a blown-up trajectory is terminal)
template <class T>
__device__ __forceinline__ void write_terminal(const EnvDev<T>& e, int b, bool flag, int tid, int nt) {
  if (!e.term_out) return;
  const int cpt = e.mono ? 1 : e.A;
  for (int a = tid; a < cpt; a += nt) e.term_out[(size_t)b * cpt + a] = flag ? (T)1 : (T)0;
}

// ------------------------------------------------------------------ the stand-alone closures of trajectory b
// MODE 0: prepare_action, 1: featurize, 2: reward.  The body of sense_kernel (env.hip) and of the episode clock's masked
// sensing launch (episode_clock.hip); both run 128 threads per trajectory -- sense_dots splits a sensor's window over nt / S
// groups, so the sums depend on that size -- with sense_lds_bytes of dynamic LDS.
#define PDEC_SENSE_THREADS 128
inline size_t sense_lds_bytes(const pdec_env_cfg& c) { return (2 * (size_t)c.N + 2 * c.A + 2 * c.S + 16 * c.S) * dtype_size(c.dtype); }

// FLT: prepare_action applies the actuator gains, featurize reads the dots through the sensor faults (without action memory)
template <class T, int MODE, bool FLT = false>
__device__ __forceinline__ void sense_traj(const EnvArg<T, FLT>& e, int b, const T* __restrict__ y, const T* __restrict__ action,
                                           const T* __restrict__ action_prev, const T* __restrict__ state_prev, T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = blockDim.x;
  T* sy = reinterpret_cast<T*>(smem_raw);  // [2][N]
  T* act = sy + 2 * N;
  T* actp = act + e.A;
  T* dots = actp + e.A;
  T* part = dots + 2 * e.S;
  if (MODE == 0 || MODE == 2) {     // row 0 of every action column (KSSetup.jl:176,241: action[1, i]); na = 1 without action memory
    for (int a = tid; a < e.A; a += nt) {
      act[a] = action[((size_t)b * e.A + a) * e.na];
      if constexpr (FLT && MODE == 0) act[a] = fault_action<T>(e.flt, b, e.A, a, act[a]);
      actp[a] = MODE == 2 ? action_prev[((size_t)b * e.A + a) * e.na] : (T)0;
    }
    __syncthreads();
  }
  if (MODE == 0) {
    for (int n = tid; n < N; n += nt) out[(size_t)b * N + n] = actuate_cell<T>(e, act, n);
    return;
  }
  const int sp = e.n_species;
  for (int i = tid; i < sp * N; i += nt) {
    // y[sp, N] column-major: (species, cell) at cell*sp + species
    const int n = i / sp, r = i - n * sp;
    sy[r * N + n] = y[(size_t)b * sp * N + i];
  }
  if (sp == 1)
    for (int n = tid; n < N; n += nt) sy[N + n] = 0;
  __syncthreads();
  sense_dots<T>(e, [&](int r, int n) { return sy[r * N + n]; }, dots, part, tid, nt);
  if (MODE == 1) {
    const size_t sw = e.mono ? (size_t)e.S : (size_t)e.A * e.ns;
    if constexpr (FLT) {        // `part` is free behind the dots
      fault_dots<T>(e.flt, b, e.S, dots, part, tid, nt);
      __syncthreads();
      featurize_traj<T>(e, part, state_prev ? state_prev + b * sw : nullptr, out + b * sw, tid, nt);
      return;
    }
    if (e.mem > 0)
      featurize_traj_mem<T>(e, dots, state_prev ? state_prev + b * sw : nullptr, action ? action + (size_t)b * e.A * e.na : nullptr,
                            out + b * sw, tid, nt);
    else
      featurize_traj<T>(e, dots, state_prev ? state_prev + b * sw : nullptr, out + b * sw, tid, nt);
  } else {
    const int rw = e.mono ? 1 : e.A;
    reward_traj<T>(e, dots, act, actp, out + (size_t)b * rw, tid, nt);
  }
}

}  // namespace pdec
