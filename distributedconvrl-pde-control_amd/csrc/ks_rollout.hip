// ks_rollout.hip -- the persistent rollout of the spectral KS environment and its launch (pdec_rollout, pdec_rollout_members)
#include "env_sense.hpp"
#include "ks_engines.hpp"
#include "roll_actor.hpp"

namespace pdec {

// ------------------------------------------------------------------ persistent KS rollout (row F2)
// T control steps of  action = clamp(actor(state) + randn * act_noise);  (env::PDEenv)(action)  in ONE launch
// (src/PDEagent.jl:175-209 + src/PDEenv.jl:195-241 + the KS closures of KSSetup.jl:130-245): the two trajectories of a
// workgroup stay in registers between steps, their sensor dots / state / actions in LDS; nothing returns to HBM between
// steps but the optional log rows PDEhook records.  The actor (a chain of <= 3 Dense layers, widths <= RO_W, one output)
// is evaluated one column per lane on the vector unit from a copy of its parameters in LDS; exploration noise from the
// same Philox element numbering as pdec_policy_act_rng (element = global column, counter offset + t * ceil(cols / 4)).
// MEM: the member form -- workgroup w serves pair w % ceil(K/2) of member w / ceil(K/2), i.e. the trajectories
// m K + 2 pair (+ 1 while 2 pair + 1 < K): the pairing a solo launch on B = K trajectories makes, so both trajectories of a
// complex FFT (and of a thread's column pair) belong to ONE member and a member's arithmetic is that of its solo rollout.
// AN = NoiseScale (pdec_mlp_set_noise_scale; solo form): the amplitude of each of the workgroup's [2][A] columns, entry
// (b A + a) / cols_per_entry of the array, is read into LDS once, behind the activation planes.
// FLT (pdec_env_set_faults): the forcing is synthesised from gain * action, staged in `rnow` (free until this step's reward is
// written), and the state the policy reads next is featurized from gain * dot + bias, staged in `part` (free behind sense_dots):
// no LDS beyond the healthy kernel's, so the same configurations are served.  Instantiations of their own (argument EnvDevF).
template <class T, class ENG, bool MEM, class AN = T, bool FLT = false>
__global__ void __launch_bounds__(ENG::kThreads) ks_rollout_kernel(EnvArg<T, FLT> e, RollActor actor, RollArgs<T, AN> g, RollMembers pm) {
  constexpr bool NS = std::is_same<AN, NoiseScale>::value;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = blockDim.x, A = e.A, ns = e.ns;
  set_wave_prio(e.prio);
  ENG eng;
  eng.init(smem_raw, e, tid, nt);
  T* act = reinterpret_cast<T*>(reinterpret_cast<C2<T>*>(smem_raw) + ENG::lds_complex(N));  // [2][A] current
  T* actp = act + 2 * A;                  // [2][A] previous
  T* dots = actp + 2 * A;                 // [2][S]
  T* part = dots + 2 * e.S;               // [8][2][S]
  T* red = part + 16 * e.S;               // [16]
  T* stl = red + 16;                      // [2][A * ns]  state of both trajectories
  T* rsum = stl + 2 * A * ns;             // [2][A]       accumulated reward
  T* rnow = rsum + 2 * A;                 // [2][A]       this step's reward
  const size_t wl_off = (size_t)(reinterpret_cast<unsigned char*>(rnow + 2 * A) - smem_raw + 15) & ~(size_t)15;
  T* wl = reinterpret_cast<T*>(smem_raw + wl_off);   // actor image, 16-byte aligned rows
  using T2 = typename RoPair<T>::type;
  T2* hb = reinterpret_cast<T2*>(wl + ((ro_image_elems(actor.dims, actor.L) + 3) & ~3));   // [2][rows][nt] column pairs

  int bfirst = 2 * blockIdx.x;
  bool pair_full = bfirst + 1 < e.B;
  const void* params = actor.params;      // (the argument itself stays untouched: a modified copy would live in scratch)
  if constexpr (MEM) {
    const int hp = (pm.K + 1) / 2, m = blockIdx.x / hp, pr = blockIdx.x - m * hp;
    bfirst = m * pm.K + 2 * pr;
    pair_full = 2 * pr + 1 < pm.K;
    params = pm.params[m];
  }
  const int b0 = bfirst, b1 = b0 + 1;
  const bool has1 = pair_full;
  const size_t o0 = (size_t)b0 * N, o1 = (size_t)b1 * N;
  const size_t cols = (size_t)e.B * A;

  if (MEM && pm.f32 && sizeof(T) != sizeof(float)) ro_load_image<T, float>(actor, params, wl, tid, nt);
  else ro_load_image<T>(actor, params, wl, tid, nt);
  for (int i = tid; i < A * ns; i += nt) {
    stl[i] = g.state[(size_t)b0 * A * ns + i];
    stl[A * ns + i] = has1 ? g.state[(size_t)b1 * A * ns + i] : (T)0;
  }
  for (int a = tid; a < A; a += nt) {
    act[a] = g.action[(size_t)b0 * A + a];
    act[A + a] = has1 ? g.action[(size_t)b1 * A + a] : (T)0;
    rsum[a] = rsum[A + a] = 0;
  }
  T* namp = nullptr;                      // [2][A] (NS)
  if constexpr (NS) {
    namp = reinterpret_cast<T*>(hb + (size_t)2 * actor.rows * nt);
    for (int a = tid; a < A; a += nt) {
      namp[a] = noise_amp<T>(g.act_noise, (size_t)b0 * A + a);
      namp[A + a] = has1 ? noise_amp<T>(g.act_noise, (size_t)b1 * A + a) : (T)0;
    }
  }
  C2<T> U[KS_MPT], Nn[KS_MPT], Ck[KS_MPT], v[KS_MPT];
  T kc1[KS_MPT], kc2[KS_MPT], kc3[KS_MPT], kg[KS_MPT], kc4[KS_MPT];
  C2<T> kd[KS_MPT];      // (m0 + i m1) * dhat: the disturbance of both packed trajectories, each at its amplitude (ks_step.hip)
  const C2<T>* __restrict__ dtab = e.mu_b ? e.dhat1 : e.dhat;
  const T m0 = e.mu_b ? e.mu_b[b0] : (T)1, m1 = e.mu_b ? e.mu_b[has1 ? b1 : b0] : (T)1;
#pragma unroll
  for (int j = 0; j < KS_MPT; ++j) {      // per-mode constants (mode layout of the engine) and the initial fields
    const int k = eng.mode_index(j);
    const bool ok = k < N;
    kc1[j] = ok ? e.c1[k] : (T)0; kc2[j] = ok ? e.c2[k] : (T)0; kc3[j] = ok ? e.c3[k] : (T)0;
    kc4[j] = ok ? e.c4[k] : (T)0; kg[j] = ok ? e.g[k] : (T)0;
    const C2<T> d = ok ? dtab[k] : mk<T>(0, 0);
    kd[j] = mk<T>(m0 * d.x - m1 * d.y, m0 * d.y + m1 * d.x);
    const int n = eng.phys_index(j);
    U[j] = n < N ? mk<T>(g.y[o0 + n], has1 ? g.y[o1 + n] : (T)0) : mk<T>(0, 0);
  }
  int flag0 = 0, flag1 = 0, first0 = -1, first1 = -1;
  const T invN = (T)1 / (T)N;
  __syncthreads();

  for (int t = 0; t < g.steps; ++t) {
    // ---- policy (src/PDEagent.jl:183-207): one pair of adjacent columns of the [2][A] column space per thread.  Before step
    // control_from (pdec_env_set_control_from; plotting.jl:55-60) the action is zero: no actor, no noise, no reward summed
    const bool ctl = t >= g.control_from;
    for (int q0 = 0; q0 < A; q0 += nt) {
      const int q = q0 + tid;
      if (q < A) {
        const int idx0 = 2 * q;
        T2 o2 = T2{(T)0, (T)0};
        if (ctl) {
          for (int i = 0; i < ns; ++i) hb[(size_t)i * nt + tid] = T2{stl[(size_t)idx0 * ns + i], stl[(size_t)(idx0 + 1) * ns + i]};
          o2 = ro_actor_pair<T>(actor, wl, hb, tid, nt);
        }
        uint64_t cprev = ~0ull;
        double rad = 0, ang = 0;
        uint32_t ph[4];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int idx = idx0 + s, r = idx / A, a = idx - r * A;
          T o = s == 0 ? o2.x : o2.y;
          if (!MEM && ctl && g.learning && (r == 0 || has1)) {
            const uint64_t c = (uint64_t)(r == 0 ? b0 : b1) * A + a;          // global column = element of the noise stream
            if ((c >> 2) != cprev) {
              noise_block(ph, g.seed, g.offset + (uint64_t)t * ((cols + 3) / 4) + (c >> 2));
              cprev = c >> 2;
            }
            // the odd element shares the Box-Muller pair of its even neighbour
            if (s == 0 || (c & 1) == 0) noise_polar(ph, (int)((c >> 1) & 1), rad, ang);
            T amp;
            if constexpr (NS) amp = namp[idx];
            else amp = g.act_noise;
            o += (T)((c & 1) ? rad * sin(ang) : rad * cos(ang)) * amp;
          }
          o = o < -g.act_limit ? -g.act_limit : (o > g.act_limit ? g.act_limit : o);
          actp[idx] = act[idx];
          act[idx] = (r == 0 || has1) ? o : (T)0;
        }
      }
    }
    __syncthreads();
    if (g.log_action)
      for (int a = tid; a < A; a += nt) {
        g.log_action[((size_t)t * e.B + b0) * A + a] = act[a];
        if (has1) g.log_action[((size_t)t * e.B + b1) * A + a] = act[A + a];
      }
    // ---- prepare_action -> spectrum -> constant term of the CNAB2 update (KSSetup.jl:231-245, :155)
    T pa4[KS_MPT], pb4[KS_MPT];
    const T* ap = act;          // the action the actuators apply
    if constexpr (FLT) {
      for (int a = tid; a < A; a += nt) {
        rnow[a] = fault_action<T>(e.flt, b0, A, a, act[a]);
        rnow[A + a] = has1 ? fault_action<T>(e.flt, b1, A, a, act[A + a]) : (T)0;
      }
      __syncthreads();
      ap = rnow;
    }
    {
      int n4[KS_MPT];
#pragma unroll
      for (int j = 0; j < KS_MPT; ++j) n4[j] = eng.phys_index(j);
      if ((N & 3) == 0 && 2 * N <= 16 * e.S) {
        actuate_consecutive<T>(e, ap, ap + A, part, tid, nt);
#pragma unroll
        for (int j = 0; j < KS_MPT; ++j) {
          pa4[j] = n4[j] < N ? part[n4[j]] : (T)0;
          pb4[j] = n4[j] < N ? part[N + n4[j]] : (T)0;
        }
        __syncthreads();      // `part` is reused by the sensor dots of this step
      } else {
        actuate_cells<T, KS_MPT>(e, ap, ap + A, n4, pa4, pb4);
      }
    }
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) {
      const int n = eng.phys_index(j);
      T pa = 0, pb = 0;
      if (n < N) {
        pa = pa4[j]; pb = pb4[j];
        if (!has1) pb = 0;
        if (g.log_p) {
          g.log_p[((size_t)t * e.B + b0) * N + n] = pa;
          if (has1) g.log_p[((size_t)t * e.B + b1) * N + n] = pb;
        }
      }
      v[j] = mk<T>(pa, pb);
    }
    eng.template run<-1>(v);
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j)
      Ck[j] = mk<T>(kc4[j] * v[j].x + kd[j].x, kc4[j] * v[j].y + kd[j].y);
    // ---- do_step (KSSetup.jl:130-160): Nn = G fft(u^2), u_hat = fft(u), K CNAB2 sub-steps, y+ = real(ifft(u_hat))
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) v[j] = mk<T>(U[j].x * U[j].x, U[j].y * U[j].y);
    eng.template run<-1>(v);
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) Nn[j] = cscale(mul_i<+1, T>(v[j]), kg[j]);
    eng.template run<-1>(U);
    for (int it = 0; it < e.K; ++it) {
#pragma unroll
      for (int j = 0; j < KS_MPT; ++j) v[j] = U[j];
      eng.template run<+1>(v);
#pragma unroll
      for (int j = 0; j < KS_MPT; ++j) {
        const T wr = v[j].x * invN, wi = v[j].y * invN;
        v[j] = mk<T>(wr * wr, wi * wi);
      }
      eng.template run<-1>(v);
#pragma unroll
      for (int j = 0; j < KS_MPT; ++j) {
        const C2<T> nn1 = Nn[j];
        Nn[j] = cscale(mul_i<+1, T>(v[j]), kg[j]);
        U[j] = mk<T>(kc1[j] * U[j].x + kc2[j] * Nn[j].x - kc3[j] * nn1.x + Ck[j].x,
                     kc1[j] * U[j].y + kc2[j] * Nn[j].y - kc3[j] * nn1.y + Ck[j].y);
      }
    }
    eng.template run<+1>(U);
    T mx0 = 0, mx1 = 0;
#pragma unroll
    for (int j = 0; j < KS_MPT; ++j) {
      const int n = eng.phys_index(j);
      U[j] = mk<T>(U[j].x * invN, U[j].y * invN);
      if (n < N) {
        if (g.log_y) {
          g.log_y[((size_t)t * e.B + b0) * N + n] = U[j].x;
          if (has1) g.log_y[((size_t)t * e.B + b1) * N + n] = U[j].y;
        }
        if (!(fabs(U[j].x) <= e.max_value)) mx0 = 1;
        if (!(fabs(U[j].y) <= e.max_value)) mx1 = 1;
      }
    }
    if (e.check_max == 1) {
      mx0 = block_max<T>(mx0, red, tid, nt);
      mx1 = block_max<T>(mx1, red, tid, nt);
      if (mx0 > 0) { flag0 = 1; if (first0 < 0) first0 = t; }
      if (mx1 > 0) { flag1 = 1; if (first1 < 0) first1 = t; }
    }
    // ---- reward (KSSetup.jl:162-178) and featurize (:190-229) from the sensor dots of the new field
    const T* Rt = reinterpret_cast<const T*>(eng.publish(U));
    sense_dots<T>(e, [&](int r, int n) { return Rt[2 * n + r]; }, dots, part, tid, nt);
    const T* fd = dots;         // what featurize reads
    if constexpr (FLT) {
      fault_dots<T>(e.flt, b0, e.S, dots, part, tid, nt);
      if (has1) fault_dots<T>(e.flt, b1, e.S, dots + e.S, part + e.S, tid, nt);
      __syncthreads();
      fd = part;
    }
    if (e.fmap) {
      reward_pair<T>(e, dots, dots + e.S, act, act + A, actp, actp + A, rnow, has1 ? rnow + A : nullptr, tid, nt);
      featurize_pair<T>(e, fd, fd + e.S, stl, has1 ? stl + A * ns : nullptr, tid, nt);
    } else {
      reward_traj<T>(e, dots, act, actp, rnow, tid, nt);
      featurize_traj<T>(e, fd, nullptr, stl, tid, nt);
      if (has1) {
        reward_traj<T>(e, dots + e.S, act + A, actp + A, rnow + A, tid, nt);
        featurize_traj<T>(e, fd + e.S, nullptr, stl + A * ns, tid, nt);
      }
    }
    __syncthreads();
    for (int a = tid; a < A; a += nt) {
      if (ctl) {
        rsum[a] += rnow[a];
        rsum[A + a] += rnow[A + a];
      }
      if (g.log_reward) {
        g.log_reward[((size_t)t * e.B + b0) * A + a] = rnow[a];
        if (has1) g.log_reward[((size_t)t * e.B + b1) * A + a] = rnow[A + a];
      }
    }
    __syncthreads();
  }
  // ---- results back to HBM
#pragma unroll
  for (int j = 0; j < KS_MPT; ++j) {
    const int n = eng.phys_index(j);
    if (n < N) {
      g.y[o0 + n] = U[j].x;
      if (has1) g.y[o1 + n] = U[j].y;
    }
  }
  for (int i = tid; i < A * ns; i += nt) {
    g.state[(size_t)b0 * A * ns + i] = stl[i];
    if (has1) g.state[(size_t)b1 * A * ns + i] = stl[A * ns + i];
  }
  for (int a = tid; a < A; a += nt) {
    g.action[(size_t)b0 * A + a] = act[a];
    if (has1) g.action[(size_t)b1 * A + a] = act[A + a];
    if (g.reward_sum) {
      g.reward_sum[(size_t)b0 * A + a] += rsum[a];
      if (has1) g.reward_sum[(size_t)b1 * A + a] += rsum[A + a];
    }
  }
  if (tid == 0) {
    if (g.done_any) { g.done_any[b0] = flag0; if (has1) g.done_any[b1] = flag1; }
    if (g.done_step) { g.done_step[b0] = first0; if (has1) g.done_step[b1] = first1; }
  }
}

// ------------------------------------------------------------------ host side
bool ks_rollout_supported(const Env& E, const Mlp& A, bool noise_tab) {
  return A.dtype == E.cfg.dtype && rollout_shape_ok(E, A, true, noise_tab);
}

// pm = null: the solo form.  Member form: A is member 0's actor (the shape all members share), the grid M ceil(K / 2)
int ks_rollout_persistent(Env& E, const Mlp& A, const RollSpec& spec, const RollPtrs& ptrs, const RollMembers* pm) {
  const bool ntab = roll_noise_tab(spec, pm);
  if (!pm && !ks_rollout_supported(E, A, ntab)) { set_error("ks_rollout_persistent: configuration not covered"); return PDEC_E_INVALID; }
  const pdec_env_cfg& c = E.cfg;
  const RollActor ra = make_roll_actor(A);
  const size_t lds = rollout_lds(E, A, true, ntab);
  const dim3 grid(pm ? (c.B / pm->K) * ((pm->K + 1) / 2) : (c.B + 1) / 2), block(E.nthreads);
  ProfScope ps(&E, pm ? "ks_rollout_members" : "ks_rollout");
  by_dtype(c.dtype, [&](auto t) {
    using T = decltype(t);
    const RollArgs<T> g = make_roll_args<T>(spec, ptrs);
    with_ks_engine<T>(E.engine, [&](auto tag) {
      using ENG = typename decltype(tag)::type;
      // one launch tail for the healthy and the fault-carrying kernels (pdec_env_set_faults: FLT, argument EnvDevF)
      auto launch = [&](auto ntab_kern, auto member_kern, auto solo_kern, const auto& e) {
        if (ntab)
          hipLaunchKernelGGL(ntab_kern, grid, block, lds, E.stream, e, ra, (make_roll_args<T, NoiseScale>(spec, ptrs)), RollMembers{});
        else if (pm) hipLaunchKernelGGL(member_kern, grid, block, lds, E.stream, e, ra, g, *pm);
        else hipLaunchKernelGGL(solo_kern, grid, block, lds, E.stream, e, ra, g, RollMembers{});
      };
      if (E.faults())
        launch(ks_rollout_kernel<T, ENG, false, NoiseScale, true>, ks_rollout_kernel<T, ENG, true, T, true>,
               ks_rollout_kernel<T, ENG, false, T, true>, make_dev_faults<T>(E));
      else
        launch(ks_rollout_kernel<T, ENG, false, NoiseScale>, ks_rollout_kernel<T, ENG, true>, ks_rollout_kernel<T, ENG, false>, make_dev<T>(E));
    });
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

}  // namespace pdec
