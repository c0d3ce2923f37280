// ksfd.hip -- the KS environment on RK4 + periodic finite differences: fused step in its LDS and one-wave forms, and the launch
#include "env_sense.hpp"

namespace pdec {

// ------------------------------------------------------------------ KS, RK4 + periodic 5-point finite differences
// The north-star variant u_t = -u u_x - u_xx - u_xxxx + p (+ the disturbance of KSSetup.jl:155) on the stencil table
// the reference defines but never uses (scripts/KS/setup/KSSetup.jl:55-59): d/dx = [0,-1/2,0,1/2,0]/dx,
// d2/dx2 = [0,1,-2,1,0]/dx^2, d4/dx4 = [1,-4,6,-4,1]/dx^4, classical RK4 (src/fluid_rk4.jl:122-132 form) with K
// sub-steps.  It is a DIFFERENT discretisation from the reference's CNAB2 step, so it is pinned by
// its own oracle (oracle/ks.py: rhs_fd / do_step_rk4_fd), not by the golden trajectories.
// One workgroup per trajectory, one cell per thread; neighbours through an LDS line with a periodic halo of 2.
template <class T>
__device__ __forceinline__ T ksfd_rhs(T u, T force, T* su, int n, int N, T i2dx, T idx2, T idx4, bool live) {
  __syncthreads();
  if (live) {
    su[n + 2] = u;
    if (n < 2) su[N + 2 + n] = u;        // right halo = cells 0, 1
    if (n >= N - 2) su[n - (N - 2)] = u; // left halo  = cells N-2, N-1
  }
  __syncthreads();
  T f = 0;
  if (live) {
    const T m2 = su[n], m1 = su[n + 1], p1 = su[n + 3], p2 = su[n + 4];
    const T ux = i2dx * (p1 - m1);
    const T uxx = idx2 * (m1 - (T)2 * u + p1);
    const T uxxxx = idx4 * (m2 - (T)4 * m1 + (T)6 * u - (T)4 * p1 + p2);
    f = -u * ux - uxx - uxxxx + force;
  }
  return f;
}

// per-workgroup reward sum of the RK4 + FD steps (one trajectory per workgroup), for the batch-mean reward of the DDPG update's
// reward broadcast -- the same hand-over as the CNAB2 step's (pdec_env_set_reward_partials_out): lanes by xor-shuffle, then the
// waves in order
template <class T>
__device__ __forceinline__ void ksfd_reward_partial(const EnvDev<T>& e, T rmine, T* red, int tid, int nt) {
  float v = (float)rmine;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if (nt <= 64) {
    if (tid == 0) e.rsum_out[blockIdx.x] = v;
    return;
  }
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = (T)v;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int i = 0; i < (nt + 63) / 64; ++i) tot += (float)red[i];
    e.rsum_out[blockIdx.x] = tot;
  }
}

// FLT (pdec_env_set_faults; MODE 0): per-trajectory actuator gains and sensor faults, instantiations of their own whose argument
// carries the three arrays (EnvDevF).  As in ks_step.hip: the applied action is staged in `act` for the actuation and the commanded
// one read again for the reward; featurize reads its dots from `part`
template <class T, int MODE, bool FLT = false>  // MODE 0: fused env step, 1: integrate only, 2: rhs only
__global__ void ksfd_env_step_kernel(EnvArg<T, FLT> e, const T* __restrict__ y_in, const T* __restrict__ p_in,
                                     const T* __restrict__ action, const T* __restrict__ action_prev,
                                     const T* __restrict__ state_prev, T* __restrict__ y_out, T* __restrict__ p_out,
                                     T* __restrict__ state_out, T* __restrict__ reward_out, int32_t* __restrict__ done) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x;
  T* su = reinterpret_cast<T*>(smem_raw);  // [2][N] (first N+4 used as the halo line; reused as sensing image)
  T* act = su + 2 * N + 4;                 // [A]
  T* actp = act + e.A;                     // [A]
  T* dots = actp + e.A;                    // [2][S]
  T* part = dots + 2 * e.S;                // [8][2][S]
  T* red = part + 16 * e.S;                // [16]
  const int n = tid;
  const bool live = n < N;
  const size_t yo = (size_t)b * N;
  T u = live ? y_in[yo + n] : (T)0;
  T p = 0;
  if (MODE == 0) {
    for (int a = tid; a < e.A; a += nt) {
      act[a] = action[(size_t)b * e.A + a];
      if constexpr (FLT) act[a] = fault_action<T>(e.flt, b, e.A, a, act[a]);
      actp[a] = action_prev[(size_t)b * e.A + a];
    }
    __syncthreads();
    if (live) {
      p = actuate_cell<T>(e, act, n);
      if (p_out) p_out[yo + n] = p;
    }
    if constexpr (FLT) {
      __syncthreads();
      for (int a = tid; a < e.A; a += nt) act[a] = action[(size_t)b * e.A + a];
    }
  } else if (live) {
    p = p_in[yo + n];
  }
  // forcing = actuation + disturbance mu cos(2 + pi + x/(Lx/2)), x = dx (n+1)   (KSSetup.jl:36,155)
  const T mu = e.mu_b ? e.mu_b[b] : e.dist_mu;      // pdec_env_set_disturbance: this trajectory's amplitude
  const T force = p + (live ? mu * (T)cos(2.0 + 3.14159265358979323846 + (double)e.dx * (n + 1) / ((double)e.dx * N / 2)) : (T)0);
  const T i2dx = (T)0.5 / e.dx, idx2 = (T)1 / (e.dx * e.dx), idx4 = idx2 * idx2;
  if (MODE == 2) {
    const T f = ksfd_rhs<T>(u, force, su, n, N, i2dx, idx2, idx4, live);
    if (live) y_out[yo + n] = f;
    return;
  }
  const T h = e.hstep;
  for (int it = 0; it < e.K; ++it) {
    const T k1 = ksfd_rhs<T>(u, force, su, n, N, i2dx, idx2, idx4, live);
    if (e.rk2) {     // PDEenv's built-in integrator (src/PDEenv.jl:208-214): explicit midpoint, `oversampling` sub-steps
      u = u + h * ksfd_rhs<T>(u + (T)0.5 * h * k1, force, su, n, N, i2dx, idx2, idx4, live);
      continue;
    }
    const T k2 = ksfd_rhs<T>(u + (T)0.5 * h * k1, force, su, n, N, i2dx, idx2, idx4, live);
    const T k3 = ksfd_rhs<T>(u + (T)0.5 * h * k2, force, su, n, N, i2dx, idx2, idx4, live);
    const T k4 = ksfd_rhs<T>(u + h * k3, force, su, n, N, i2dx, idx2, idx4, live);
    u = u + h / (T)6 * (k1 + (T)2 * (k2 + k3) + k4);
  }
  if (live) y_out[yo + n] = u;
  if (done) {
    T m = (live && !(fabs(u) <= e.max_value)) ? (T)1 : (T)0;
    m = block_max<T>(m, red, tid, nt);
    if (tid == 0) done[b] = (e.check_max == 1 && m > 0) ? 1 : 0;
    if (MODE == 0 && e.check_max != 2) write_terminal<T>(e, b, e.check_max == 1 && m > 0, tid, nt);
  }
  if (MODE != 0) return;
  __syncthreads();
  if (live) {
    su[n] = u;
    su[N + n] = 0;
  }
  __syncthreads();
  sense_dots<T>(e, [&](int r, int nn) { return su[r * N + nn]; }, dots, part, tid, nt);
  const int rw = e.mono ? 1 : e.A;
  const size_t sw = e.mono ? (size_t)e.S : (size_t)e.A * e.ns;
  const T rmine = reward_traj<T>(e, dots, act, actp, reward_out + (size_t)b * rw, tid, nt);
  const T* fd = dots;
  if constexpr (FLT) {
    fault_dots<T>(e.flt, b, e.S, dots, part, tid, nt);
    __syncthreads();
    fd = part;
  }
  featurize_traj<T>(e, fd, state_prev ? state_prev + b * sw : nullptr, state_out + b * sw, tid, nt);
  if (e.rsum_out) ksfd_reward_partial<T>(e, rmine, red, tid, nt);
  if (done && e.check_max == 2) {
    __syncthreads();
    if (tid == 0) {
      T m = 0;
      for (int a = 0; a < rw; ++a)
        if (!(fabs(reward_out[(size_t)b * rw + a]) <= e.max_value)) m = 1;
      done[b] = m > 0 ? 1 : 0;
      write_terminal<T>(e, b, m > 0, 0, 1);
    }
  }
}

// ---- the same step with ONE WAVE per trajectory (N = 64 CPL; used at N = 256, the grid of configs C1 / C2): lane l keeps the CPL consecutive
// cells CPL l .. CPL l + CPL - 1 in registers, the two neighbours on either side come from lanes l -+ 1 (periodic) by four
// lane exchanges per right-hand side -- no LDS line, no workgroup barrier inside the 4 K right-hand sides of a control step
// (the form above: two barriers each) -- and a 64-thread workgroup fits beside the update passes on every CU in one round
// (the 256-thread form: 72 VGPRs on all four SIMDs, one workgroup per CU at a time beside the passes, two rounds at B = 512).
// Same stencils and the same order of operations per cell as ksfd_rhs / the RK4 above.
// value of the same register in lane l - 1 (FROM_BELOW) or l + 1, periodic over the 64 lanes: one DPP wave rotate per 32-bit word
// (gfx9 wave_ror:1 / wave_rol:1) instead of a ds_bpermute round trip through the LDS crossbar
template <bool FROM_BELOW>
__device__ __forceinline__ float lane_neighbour(float x) {
  constexpr int ctrl = FROM_BELOW ? 0x13C : 0x134;      // DPP_WF_RR1 : DPP_WF_RL1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, 0xf, 0xf, false));
}
template <bool FROM_BELOW>
__device__ __forceinline__ double lane_neighbour(double x) {
  constexpr int ctrl = FROM_BELOW ? 0x13C : 0x134;
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, ctrl, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), ctrl, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <class T, int CPL>
__device__ __forceinline__ void ksfd_rhs_wave(const T (&w)[CPL], const T (&force)[CPL], T (&f)[CPL], int up, int dn, T i2dx, T idx2, T idx4) {
  T ext[CPL + 4];
  (void)up; (void)dn;
  ext[0] = lane_neighbour<true>(w[CPL - 2]);
  ext[1] = lane_neighbour<true>(w[CPL - 1]);
  ext[CPL + 2] = lane_neighbour<false>(w[0]);
  ext[CPL + 3] = lane_neighbour<false>(w[1]);
#pragma unroll
  for (int c = 0; c < CPL; ++c) ext[c + 2] = w[c];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const T m2 = ext[c], m1 = ext[c + 1], u = ext[c + 2], p1 = ext[c + 3], p2 = ext[c + 4];
    const T ux = i2dx * (p1 - m1);
    const T uxx = idx2 * (m1 - (T)2 * u + p1);
    const T uxxxx = idx4 * (m2 - (T)4 * m1 + (T)6 * u - (T)4 * p1 + p2);
    f[c] = -u * ux - uxx - uxxxx + force[c];
  }
}

template <class T, int CPL, bool FLT = false>
__global__ void __launch_bounds__(64) ksfd_wave_step_kernel(EnvArg<T, FLT> e, const T* __restrict__ y_in, const T* __restrict__ action,
                                                            const T* __restrict__ action_prev, const T* __restrict__ state_prev,
                                                            T* __restrict__ y_out, T* __restrict__ p_out, T* __restrict__ state_out,
                                                            T* __restrict__ reward_out, int32_t* __restrict__ done) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = 64, b = blockIdx.x;
  T* su = reinterpret_cast<T*>(smem_raw);  // [2][N] sensing image
  T* act = su + 2 * N + 4;                 // [A]
  T* actp = act + e.A;                     // [A]
  T* dots = actp + e.A;                    // [2][S]
  T* part = dots + 2 * e.S;                // [8][2][S]
  T* red = part + 16 * e.S;                // [16]
  set_wave_prio(e.prio);
  const size_t yo = (size_t)b * N;
  const int n0 = CPL * tid, up = (tid + 63) & 63, dn = (tid + 1) & 63;
  T u[CPL], force[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) u[c] = y_in[yo + n0 + c];
  for (int a = tid; a < e.A; a += nt) {
    act[a] = action[(size_t)b * e.A + a];
    if constexpr (FLT) act[a] = fault_action<T>(e.flt, b, e.A, a, act[a]);
    actp[a] = action_prev[(size_t)b * e.A + a];
  }
  __syncthreads();
  const T mu = e.mu_b ? e.mu_b[b] : e.dist_mu;      // pdec_env_set_disturbance: this trajectory's amplitude
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int n = n0 + c;
    const T p = actuate_cell<T>(e, act, n);
    if (p_out) p_out[yo + n] = p;
    // forcing = actuation + disturbance mu cos(2 + pi + x/(Lx/2)), x = dx (n+1)   (KSSetup.jl:36,155)
    force[c] = p + mu * (T)cos(2.0 + 3.14159265358979323846 + (double)e.dx * (n + 1) / ((double)e.dx * N / 2));
  }
  if constexpr (FLT) {
    __syncthreads();
    for (int a = tid; a < e.A; a += nt) act[a] = action[(size_t)b * e.A + a];
  }
  const T i2dx = (T)0.5 / e.dx, idx2 = (T)1 / (e.dx * e.dx), idx4 = idx2 * idx2, h = e.hstep;
  for (int it = 0; it < e.K; ++it) {
    T k1[CPL], k2[CPL], k3[CPL], k4[CPL], w[CPL];
    ksfd_rhs_wave<T, CPL>(u, force, k1, up, dn, i2dx, idx2, idx4);
#pragma unroll
    for (int c = 0; c < CPL; ++c) w[c] = u[c] + (T)0.5 * h * k1[c];
    ksfd_rhs_wave<T, CPL>(w, force, k2, up, dn, i2dx, idx2, idx4);
    if (e.rk2) {     // PDEenv's built-in integrator (src/PDEenv.jl:208-214): explicit midpoint, `oversampling` sub-steps
#pragma unroll
      for (int c = 0; c < CPL; ++c) u[c] = u[c] + h * k2[c];
      continue;
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) w[c] = u[c] + (T)0.5 * h * k2[c];
    ksfd_rhs_wave<T, CPL>(w, force, k3, up, dn, i2dx, idx2, idx4);
#pragma unroll
    for (int c = 0; c < CPL; ++c) w[c] = u[c] + h * k3[c];
    ksfd_rhs_wave<T, CPL>(w, force, k4, up, dn, i2dx, idx2, idx4);
#pragma unroll
    for (int c = 0; c < CPL; ++c) u[c] = u[c] + h / (T)6 * (k1[c] + (T)2 * (k2[c] + k3[c]) + k4[c]);
  }
  T m = 0;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    y_out[yo + n0 + c] = u[c];
    if (!(fabs(u[c]) <= e.max_value)) m = 1;
  }
  if (done) {
    m = block_max<T>(m, red, tid, nt);
    if (tid == 0) done[b] = (e.check_max == 1 && m > 0) ? 1 : 0;
    if (e.check_max != 2) write_terminal<T>(e, b, e.check_max == 1 && m > 0, tid, nt);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    su[n0 + c] = u[c];
    su[N + n0 + c] = 0;
  }
  __syncthreads();
  sense_dots<T>(e, [&](int r, int nn) { return su[r * N + nn]; }, dots, part, tid, nt);
  const int rw = e.mono ? 1 : e.A;
  const size_t sw = e.mono ? (size_t)e.S : (size_t)e.A * e.ns;
  const T rmine = reward_traj<T>(e, dots, act, actp, reward_out + (size_t)b * rw, tid, nt);
  const T* fd = dots;
  if constexpr (FLT) {
    fault_dots<T>(e.flt, b, e.S, dots, part, tid, nt);
    __syncthreads();
    fd = part;
  }
  featurize_traj<T>(e, fd, state_prev ? state_prev + b * sw : nullptr, state_out + b * sw, tid, nt);
  if (e.rsum_out) ksfd_reward_partial<T>(e, rmine, red, tid, nt);
  if (done && e.check_max == 2) {
    __syncthreads();
    if (tid == 0) {
      T mm = 0;
      for (int a = 0; a < rw; ++a)
        if (!(fabs(reward_out[(size_t)b * rw + a]) <= e.max_value)) mm = 1;
      done[b] = mm > 0 ? 1 : 0;
      write_terminal<T>(e, b, mm > 0, 0, 1);
    }
  }
}

// ------------------------------------------------------------------ host side
size_t ksfd_lds_bytes(const pdec_env_cfg& c) { return (2 * (size_t)c.N + 4 + 2 * c.A + 2 * c.S + 16 * c.S + 16) * dtype_size(c.dtype); }

int ksfd_launch_step(Env& E, int mode, const StepArgs& a) {
  const pdec_env_cfg& c = E.cfg;
  ProfScope ps(&E, mode == 0 ? "ksfd_env_step" : (mode == 1 ? "ksfd_pde_step" : "ksfd_rhs"));
  // fused step at N = 256: one wave per trajectory (ksfd_wave_step_kernel); PDEC_KSFD_LDS=1: the general form
  // (N = 1024 would need 168 VGPRs per wave: no room beside the passes)
  const bool wave = mode == 0 && c.N == 256 && getenv("PDEC_KSFD_LDS") == nullptr;
  by_dtype(c.dtype, [&](auto t) {
    using T = decltype(t);
    // one launch tail for the healthy and the fault-carrying kernels (pdec_env_set_faults: FLT, fused step only, argument EnvDevF)
    auto launch = [&](auto wave_kern, auto kern, const auto& e) {
      if (wave)
        hipLaunchKernelGGL(wave_kern, dim3(c.B), dim3(64), E.lds_bytes, E.stream, e, (const T*)a.y_in, (const T*)a.action,
                           (const T*)a.action_prev, (const T*)a.state_prev, (T*)a.y_out, (T*)a.p_out, (T*)a.state_out, (T*)a.reward_out, a.done);
      else
        hipLaunchKernelGGL(kern, dim3(c.B), dim3(E.nthreads), E.lds_bytes, E.stream, PDEC_STEP_KERNEL_ARGS(T, e, a));
    };
    if (mode == 0 && E.faults())
      launch(ksfd_wave_step_kernel<T, 4, true>, ksfd_env_step_kernel<T, 0, true>, make_dev_faults<T>(E));
    else
      launch(ksfd_wave_step_kernel<T, 4>, mode == 0 ? ksfd_env_step_kernel<T, 0> : (mode == 1 ? ksfd_env_step_kernel<T, 1> : ksfd_env_step_kernel<T, 2>),
             make_dev<T>(E));
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

}  // namespace pdec
