// kseg.hip -- the 1-D Keller-Segel environment: fused step (RK4 / explicit midpoint), persistent rollout and their launches
//
// Restates (from scratch, batched over independent trajectories):
//   (env::PDEenv)(action)              src/PDEenv.jl:195-241
//   Keller-Segel f + RK4               scripts/Keller-Segel/setup/KellerSegelSetup.jl:213-239
//   featurize / prepare_action / reward_function   KellerSegelSetup.jl:241-332
#include "env_sense.hpp"
#include "roll_actor.hpp"

namespace pdec {

// ------------------------------------------------------------------ Keller-Segel RK4 kernel
// One workgroup per trajectory, one cell per thread; u,v in registers, neighbours through
// LDS with the reference's zero-flux edge fix-up (KellerSegelSetup.jl:220-223).
template <class T>
__device__ __forceinline__ void kseg_rhs(T u, T v, T p, T* su, T* sv, int n, int N, T idx, T idx2, bool live,
                                         T& du, T& dv) {
  __syncthreads();
  if (live) {
    su[n + 1] = u;
    sv[n + 1] = v;
    if (n == 0) {
      su[0] = u;
      sv[0] = v;
    }
    if (n == N - 1) {
      su[N + 1] = u;
      sv[N + 1] = v;
    }
  }
  __syncthreads();
  if (live) {
    const T um = su[n], up = su[n + 2], vm = sv[n], vp = sv[n + 2];
    const T ux = (T)0.5 * idx * (up - um);
    const T uxx = idx2 * um - (T)2 * idx2 * u + idx2 * up;
    const T vx = (T)0.5 * idx * (vp - vm);
    const T vxx = idx2 * vm - (T)2 * idx2 * v + idx2 * vp;
    dv = vxx - v + u + p;
    du = uxx + u - (T)5.6 * ux * vx - (T)5.6 * u * vxx - u * u;
  }
}

template <class T, int MODE>  // MODE 0: fused env step, 1: integrate only, 2: rhs only
__global__ void kseg_env_step_kernel(EnvDev<T> e, const T* __restrict__ y_in, const T* __restrict__ p_in,
                                     const T* __restrict__ action, const T* __restrict__ action_prev,
                                     const T* __restrict__ state_prev, T* __restrict__ y_out,
                                     T* __restrict__ p_out, T* __restrict__ state_out,
                                     T* __restrict__ reward_out, int32_t* __restrict__ done) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x;
  T* su = reinterpret_cast<T*>(smem_raw);  // [N+2]
  T* sv = su + N + 2;                      // [N+2]
  T* act = sv + N + 2;                     // [A]
  T* actp = act + e.A;                     // [A]
  T* dots = actp + e.A;                    // [2][S]
  T* part = dots + 2 * e.S;                // [8][2][S]
  T* red = part + 16 * e.S;                // [16]
  const int n = tid;
  const bool live = n < N;
  // y[2, nx] Julia column-major: element (species, cell) at cell*2 + species
  const size_t yo = (size_t)b * 2 * N;
  T u = live ? y_in[yo + 2 * n] : (T)0, v = live ? y_in[yo + 2 * n + 1] : (T)0;
  T p = 0;
  if (MODE == 0) {
    for (int a = tid; a < e.A; a += nt) {
      act[a] = action[(size_t)b * e.A + a];
      actp[a] = action_prev[(size_t)b * e.A + a];
    }
    __syncthreads();
    if (live) {
      p = actuate_cell<T>(e, act, n);
      if (p_out) p_out[(size_t)b * N + n] = p;
    }
  } else if (live) {
    p = p_in[(size_t)b * N + n];
  }
  const T idx = (T)1 / e.dx, idx2 = (T)1 / (e.dx * e.dx);
  if (MODE == 2) {
    T du = 0, dv = 0;
    kseg_rhs<T>(u, v, p, su, sv, n, N, idx, idx2, live, du, dv);
    if (live) {
      y_out[yo + 2 * n] = du;
      y_out[yo + 2 * n + 1] = dv;
    }
    return;
  }
  const T h = e.hstep;
  for (int it = 0; it < e.K; ++it) {
    T k1u = 0, k1v = 0, k2u = 0, k2v = 0, k3u = 0, k3v = 0, k4u = 0, k4v = 0;
    kseg_rhs<T>(u, v, p, su, sv, n, N, idx, idx2, live, k1u, k1v);
    if (e.rk2) {     // PDEenv's built-in integrator (src/PDEenv.jl:208-214): explicit midpoint, `oversampling` sub-steps
      kseg_rhs<T>(u + (T)0.5 * h * k1u, v + (T)0.5 * h * k1v, p, su, sv, n, N, idx, idx2, live, k2u, k2v);
      u = u + h * k2u;
      v = v + h * k2v;
      continue;
    }
    kseg_rhs<T>(u + (T)0.5 * h * k1u, v + (T)0.5 * h * k1v, p, su, sv, n, N, idx, idx2, live, k2u, k2v);
    kseg_rhs<T>(u + (T)0.5 * h * k2u, v + (T)0.5 * h * k2v, p, su, sv, n, N, idx, idx2, live, k3u, k3v);
    kseg_rhs<T>(u + h * k3u, v + h * k3v, p, su, sv, n, N, idx, idx2, live, k4u, k4v);
    u = u + h / (T)6 * (k1u + (T)2 * (k2u + k3u) + k4u);
    v = v + h / (T)6 * (k1v + (T)2 * (k2v + k3v) + k4v);
  }
  if (live) {
    y_out[yo + 2 * n] = u;
    y_out[yo + 2 * n + 1] = v;
  }
  if (done) {
    T m = (live && !(fabs(u) <= e.max_value && fabs(v) <= e.max_value)) ? (T)1 : (T)0;
    m = block_max<T>(m, red, tid, nt);
    if (tid == 0) done[b] = (e.check_max == 1 && m > 0) ? 1 : 0;
    if (MODE == 0 && e.check_max != 2) write_terminal<T>(e, b, e.check_max == 1 && m > 0, tid, nt);
  }
  if (MODE != 0) return;
  __syncthreads();
  if (live) {
    su[n] = u;
    sv[n] = v;
  }
  __syncthreads();
  sense_dots<T>(e, [&](int r, int nn) { return r == 0 ? su[nn] : sv[nn]; }, dots, part, tid, nt);
  reward_traj<T>(e, dots, act, actp, reward_out + (size_t)b * e.A, tid, nt);
  const size_t sw = (size_t)e.A * e.ns;
  featurize_traj<T>(e, dots, state_prev ? state_prev + b * sw : nullptr, state_out + b * sw, tid, nt);
  if (done && e.check_max == 2) {
    __syncthreads();
    if (tid == 0) {
      T m = 0;
      for (int a = 0; a < e.A; ++a)
        if (!(fabs(reward_out[(size_t)b * e.A + a]) <= e.max_value)) m = 1;
      done[b] = m > 0 ? 1 : 0;
      write_terminal<T>(e, b, m > 0, 0, 1);
    }
  }
}

// ------------------------------------------------------------------ persistent Keller-Segel rollout (row F2)
// T control steps of  action = clamp(actor(state) + randn * act_noise);  (env::PDEenv)(action)  in ONE launch for the 1-D
// Keller-Segel environment (src/PDEagent.jl:175-209 + src/PDEenv.jl:195-241 with scripts/Keller-Segel/setup/KellerSegelSetup.jl:
// 213-332): the fields u, v stay in registers (one cell per thread, one workgroup per trajectory), state / action / reward rows
// in LDS, the actor (<= 3 Dense layers of <= RO_W units, 12 -> 20 -> 20 -> 1 in the shipped script) is evaluated in the kernel,
// one thread per (actuator, unit), and the exploration noise is the same Philox stream element for element (column c = b A + a
// of step t) as the acting kernel's, so the launch tracks the step-by-step loop to the actor's summation order.
// MEM: the member form -- trajectory b (one workgroup) takes the actor of member b / K from the table.  NT: the largest
// workgroup the instantiation is launched with (1024: any; the member form has a 256-thread instantiation, whose register
// budget holds the fp64 loop without spills).  AN = NoiseScale (pdec_mlp_set_noise_scale; solo form): the amplitude of each of
// the trajectory's A columns, entry (b A + a) / cols_per_entry of the array, is read into LDS once, behind the activations.
template <class T, bool MEM, int NT, class AN = T>
__global__ void __launch_bounds__(NT) kseg_rollout_kernel(EnvDev<T> e, RollActor actor, RollArgs<T, AN> g, RollMembers pm) {
  constexpr bool NS = std::is_same<AN, NoiseScale>::value;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x, A = e.A, ns = e.ns;
  T* su = reinterpret_cast<T*>(smem_raw);  // [N+2]
  T* sv = su + N + 2;                      // [N+2]
  T* act = sv + N + 2;                     // [A]
  T* actp = act + A;                       // [A]
  T* dots = actp + A;                      // [2][S]
  T* part = dots + 2 * e.S;                // [8][2][S]
  T* red = part + 16 * e.S;                // [16]
  T* stl = red + 16;                       // [2][A * ns]  state of the trajectory, ping-pong (temporal_steps > 1 shifts the old rows)
  T* stn = stl + A * ns;
  T* rsum = stn + A * ns;                  // [A]       accumulated reward
  T* rnow = rsum + A;                      // [A]       this step's reward
  const size_t wl_off = (size_t)(reinterpret_cast<unsigned char*>(rnow + A) - smem_raw + 15) & ~(size_t)15;
  T* wl = reinterpret_cast<T*>(smem_raw + wl_off);   // actor image, 16-byte aligned rows
  T* hb = wl + ((ro_image_elems(actor.dims, actor.L) + 3) & ~3);   // [2][A][RO_W] activations of the actor, ping-pong
  const int n = tid;
  const bool live = n < N;
  const size_t yo = (size_t)b * 2 * N, cols = (size_t)e.B * A;

  const void* params = actor.params;
  if constexpr (MEM) params = pm.params[b / pm.K];
  if (MEM && pm.f32 && sizeof(T) != sizeof(float)) ro_load_image<T, float>(actor, params, wl, tid, nt);
  else ro_load_image<T>(actor, params, wl, tid, nt);
  for (int i = tid; i < A * ns; i += nt) stl[i] = g.state[(size_t)b * A * ns + i];
  for (int a = tid; a < A; a += nt) {
    act[a] = g.action[(size_t)b * A + a];
    rsum[a] = 0;
  }
  if constexpr (NS) {                      // [A] behind the activations
    for (int a = tid; a < A; a += nt) hb[(size_t)2 * A * RO_W + a] = noise_amp<T>(g.act_noise, (size_t)b * A + a);
  }
  T u = live ? g.y[yo + 2 * n] : (T)0, v = live ? g.y[yo + 2 * n + 1] : (T)0;
  int flag = 0, first = -1;
  const T idx = (T)1 / e.dx, idx2 = (T)1 / (e.dx * e.dx), h = e.hstep;
  __syncthreads();

  for (int t = 0; t < g.steps; ++t) {
    // ---- policy (src/PDEagent.jl:183-207): the A actuator columns share the weights (per-actuator agents); one thread per
    // (actuator, output unit) and layer, k-ordered accumulation like the oracle's W * x + b
    const bool ctl = t >= g.control_from;     // pdec_env_set_control_from: zero action, no noise, no reward summed before it
    {
      const T* in = stl;
      int istride = ns, off = 0;
      for (int l = 0; ctl && l < actor.L; ++l) {
        const int din = actor.dims[l], dout = actor.dims[l + 1], fn = actor.acts[l];
        T* out = hb + (size_t)(l & 1) * A * RO_W;
        const T* Wt = wl + off;
        for (int id = tid; id < A * dout; id += nt) {
          const int a = id / dout, o = id - a * dout;
          T acc = Wt[din * RO_W + o];
          for (int k = 0; k < din; ++k) acc += Wt[k * RO_W + o] * in[a * istride + k];
          out[a * RO_W + o] = ro_act_fn<T>(acc, fn);
        }
        __syncthreads();
        in = out; istride = RO_W;
        off += (din + 1) * RO_W;
      }
      for (int a = tid; a < A; a += nt) {
        T o = ctl ? in[a * RO_W] : (T)0;
        if (!MEM && ctl && g.learning) {
          const uint64_t c = (uint64_t)b * A + a;                          // global column = element of the noise stream
          if constexpr (NS) o += (T)noise_normal(g.seed, g.offset + (uint64_t)t * ((cols + 3) / 4), c) * hb[(size_t)2 * A * RO_W + a];
          else o += (T)noise_normal(g.seed, g.offset + (uint64_t)t * ((cols + 3) / 4), c) * g.act_noise;
        }
        o = o < -g.act_limit ? -g.act_limit : (o > g.act_limit ? g.act_limit : o);
        actp[a] = act[a];
        act[a] = o;
      }
    }
    __syncthreads();
    if (g.log_action)
      for (int a = tid; a < A; a += nt) g.log_action[((size_t)t * e.B + b) * A + a] = act[a];
    // ---- prepare_action (KellerSegelSetup.jl:249-262), then the integrator of the step kernel (same order of operations)
    T p = 0;
    if (live) {
      p = actuate_cell<T>(e, act, n);
      if (g.log_p) g.log_p[((size_t)t * e.B + b) * N + n] = p;
    }
    for (int it = 0; it < e.K; ++it) {
      T k1u = 0, k1v = 0, k2u = 0, k2v = 0, k3u = 0, k3v = 0, k4u = 0, k4v = 0;
      kseg_rhs<T>(u, v, p, su, sv, n, N, idx, idx2, live, k1u, k1v);
      if (e.rk2) {
        kseg_rhs<T>(u + (T)0.5 * h * k1u, v + (T)0.5 * h * k1v, p, su, sv, n, N, idx, idx2, live, k2u, k2v);
        u = u + h * k2u;
        v = v + h * k2v;
        continue;
      }
      kseg_rhs<T>(u + (T)0.5 * h * k1u, v + (T)0.5 * h * k1v, p, su, sv, n, N, idx, idx2, live, k2u, k2v);
      kseg_rhs<T>(u + (T)0.5 * h * k2u, v + (T)0.5 * h * k2v, p, su, sv, n, N, idx, idx2, live, k3u, k3v);
      kseg_rhs<T>(u + h * k3u, v + h * k3v, p, su, sv, n, N, idx, idx2, live, k4u, k4v);
      u = u + h / (T)6 * (k1u + (T)2 * (k2u + k3u) + k4u);
      v = v + h / (T)6 * (k1v + (T)2 * (k2v + k3v) + k4v);
    }
    if (live && g.log_y) {
      g.log_y[((size_t)t * e.B + b) * 2 * N + 2 * n] = u;
      g.log_y[((size_t)t * e.B + b) * 2 * N + 2 * n + 1] = v;
    }
    if (e.check_max == 1) {
      T m = (live && !(fabs(u) <= e.max_value && fabs(v) <= e.max_value)) ? (T)1 : (T)0;
      m = block_max<T>(m, red, tid, nt);
      if (m > 0) { flag = 1; if (first < 0) first = t; }
    }
    // ---- reward and featurize from the sensor dots of the new fields
    __syncthreads();
    if (live) {
      su[n] = u;
      sv[n] = v;
    }
    __syncthreads();
    sense_dots<T>(e, [&](int r, int nn) { return r == 0 ? su[nn] : sv[nn]; }, dots, part, tid, nt);
    reward_traj<T>(e, dots, act, actp, rnow, tid, nt);
    featurize_traj<T>(e, dots, stl, stn, tid, nt);       // new rows on top, the previous state's rows shifted down (temporal stack)
    { T* sw = stl; stl = stn; stn = sw; }
    __syncthreads();
    for (int a = tid; a < A; a += nt) {
      if (ctl) rsum[a] += rnow[a];
      if (g.log_reward) g.log_reward[((size_t)t * e.B + b) * A + a] = rnow[a];
    }
    __syncthreads();
  }
  // ---- results back to HBM
  if (live) {
    g.y[yo + 2 * n] = u;
    g.y[yo + 2 * n + 1] = v;
  }
  for (int i = tid; i < A * ns; i += nt) g.state[(size_t)b * A * ns + i] = stl[i];
  for (int a = tid; a < A; a += nt) {
    g.action[(size_t)b * A + a] = act[a];
    if (g.reward_sum) g.reward_sum[(size_t)b * A + a] += rsum[a];
  }
  if (tid == 0) {
    if (g.done_any) g.done_any[b] = flag;
    if (g.done_step) g.done_step[b] = first;
  }
}

// ------------------------------------------------------------------ host side
size_t kseg_lds_bytes(const pdec_env_cfg& c) { return (2 * ((size_t)c.N + 2) + 2 * c.A + 2 * c.S + 16 * c.S + 16) * dtype_size(c.dtype); }

int kseg_launch_step(Env& E, int mode, const StepArgs& a) {
  ProfScope ps(&E, mode == 0 ? "kseg_env_step" : (mode == 1 ? "kseg_pde_step" : "kseg_rhs"));
  by_dtype(E.cfg.dtype, [&](auto t) {
    using T = decltype(t);
    const auto kern = mode == 0 ? kseg_env_step_kernel<T, 0> : (mode == 1 ? kseg_env_step_kernel<T, 1> : kseg_env_step_kernel<T, 2>);
    hipLaunchKernelGGL(kern, dim3(E.cfg.B), dim3(E.nthreads), E.lds_bytes, E.stream, PDEC_STEP_KERNEL_ARGS(T, make_dev<T>(E), a));
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

// ---- persistent rollout
bool kseg_rollout_supported(const Env& E, const Mlp& A, bool noise_tab) {
  return A.dtype == E.cfg.dtype && rollout_shape_ok(E, A, false, noise_tab);
}
int kseg_rollout_persistent(Env& E, const Mlp& A, const RollSpec& spec, const RollPtrs& ptrs, const RollMembers* pm) {
  const bool ntab = roll_noise_tab(spec, pm);
  if (!pm && !kseg_rollout_supported(E, A, ntab)) { set_error("kseg_rollout_persistent: configuration not covered"); return PDEC_E_INVALID; }
  const RollActor ra = make_roll_actor(A);
  const size_t lds = rollout_lds(E, A, false, ntab);
  const dim3 grid(E.cfg.B), block(E.nthreads);
  ProfScope ps(&E, pm ? "kseg_rollout_members" : "kseg_rollout");
  by_dtype(E.cfg.dtype, [&](auto t) {
    using T = decltype(t);
    const EnvDev<T> e = make_dev<T>(E);
    const RollArgs<T> g = make_roll_args<T>(spec, ptrs);
    if (ntab)
      hipLaunchKernelGGL((kseg_rollout_kernel<T, false, 1024, NoiseScale>), grid, block, lds, E.stream, e, ra,
                         (make_roll_args<T, NoiseScale>(spec, ptrs)), RollMembers{});
    else if (pm && E.nthreads <= 256) hipLaunchKernelGGL((kseg_rollout_kernel<T, true, 256>), grid, block, lds, E.stream, e, ra, g, *pm);
    else if (pm) hipLaunchKernelGGL((kseg_rollout_kernel<T, true, 1024>), grid, block, lds, E.stream, e, ra, g, *pm);
    else hipLaunchKernelGGL((kseg_rollout_kernel<T, false, 1024>), grid, block, lds, E.stream, e, ra, g, RollMembers{});
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

}  // namespace pdec
