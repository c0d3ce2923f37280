// ks_step.hip -- the spectral KS environment step (CNAB2) for gfx950: actuator synthesis, time integration, sensor
// read-out, reward, im2col featurize and blow-up flag fused in one launch (or the integrator alone), and its launch.
//
// Restates (from scratch, batched over independent trajectories):
//   (env::PDEenv)(action)              src/PDEenv.jl:195-241
//   KS do_step (CNAB2, spectral)       scripts/KS/setup/KSSetup.jl:115-160
//   featurize / prepare_action / reward_function   KSSetup.jl:162-245
//
// KS kernel design: one workgroup integrates TWO trajectories packed as the real and imaginary part of one complex sequence
// z = u_a + i u_b.  Every operator of the CNAB2 scheme is either a real diagonal in wave space (A_inv, B), multiplication by the
// purely imaginary diagonal G = -i alpha/2 (linear, so it acts on the packed spectrum directly) or the pointwise square in physical
// space, which acts on Re and Im separately -- so the pair never has to be separated and one complex FFT serves two trajectories.
// All 2K+3 FFTs of a control step run in registers / LDS (ks_engines.hpp); per-mode state lives in registers; HBM sees only the
// compulsory traffic (y, action in; y, state, reward, done out).
#include "env_sense.hpp"
#include "ks_engines.hpp"

namespace pdec {

// SHARE (pdec_env_set_simd_sharing; fp32 single-wave engine only): the 64-VGPR form of the kernel, see below
// SYNC (pdec_set_launch_sync; single-workgroup launches of the reference's own shapes): wait for the producer of the action
// before anything is read, signal behind the last store -- a separate instantiation, so that the batched kernels keep their code
// MU (pdec_env_set_disturbance): the disturbance amplitude per trajectory -- likewise instantiations of their own: in the one code
// path for both cases the register form of <float, FftWave256> took 98 VGPRs instead of 96 and its SIMD-sharing form spilled 20
// instead of 15, and those two budgets are what lets the step run beside the update passes
// FLT (pdec_env_set_faults; FUSED only): actuator gains and sensor faults per trajectory -- instantiations of their own for the
// same reason, with the three arrays behind the EnvDev argument (EnvDevF), so that the others keep their kernel arguments too.
// No LDS of its own: the applied action gain * action is staged in `act` for the actuation and the commanded action read again
// for the reward; the dots featurize reads stand in `part`, which is free behind sense_dots
template <class T, class ENG, bool FUSED, bool SHARE = false, bool SYNC = false, bool MU = false, bool FLT = false>
__global__ void __launch_bounds__(ENG::kThreads, SHARE ? 8 : 1) ks_env_step_kernel(EnvArg<T, FLT> e, const T* __restrict__ y_in, const T* __restrict__ p_in,
                                   const T* __restrict__ action, const T* __restrict__ action_prev,
                                   const T* __restrict__ state_prev, T* __restrict__ y_out,
                                   T* __restrict__ p_out, T* __restrict__ state_out,
                                   T* __restrict__ reward_out, int32_t* __restrict__ done) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int N = e.N, tid = threadIdx.x, nt = blockDim.x;
  constexpr int MPT = KsMpt<ENG>::value;        // modes / cells per thread: KS_MPT, two in the two-wave N = 256 engine
  // the sums (sensor dots: a window is split over nt / S groups; reward partial) keep the tree of the engine's one-wave form
  // where an engine names the threads that do them; the others take SUM_IDLE_TID (env_sense.hpp), pass the loops by and meet
  // the barriers
  constexpr int SUMT = KsSumThreads<ENG>::value;
  const int stid = SUMT ? (tid < SUMT ? tid : SUM_IDLE_TID) : tid, snt = SUMT ? SUMT : nt;
  if constexpr (SYNC) launch_sync_wait(e.sync);
  // This kernel is a long dependent chain (63 FFTs) issued by very few waves.  Beside the f32-MFMA update passes (which
  // execute on the vector unit) each of its instructions waits for an MFMA to drain (~2.7x slower), and their eight waves
  // per workgroup wait for each other at barriers; on its own it runs at priority 1, below the passes at 2 (r02f).
  // SHARE: in its register form (86 VGPRs) a wave of this kernel cannot share a SIMD with two waves of the 222-VGPR critic
  // pass (2 x 224 + 86 > 512): step and pass exclude each other per CU, and the step's tail delayed every workgroup of
  // the next pass (75 us in the pipeline against 63 alone, r02j).  The SHARE form keeps the per-mode constants, the
  // constant term and the previous nonlinear term in LDS (LDSC below), is bounded to 64 VGPRs (2 x 224 + 64 = 512) and
  // runs at priority 3: it is over before the next pass needs the registers, and the pass keeps its alone time (r02l:
  // 135 -> 125 us per control step).  Alone the SHARE form is slower (37 vs 29 us: four exposed LDS round trips per
  // sub-step), so only the two-stream training pipeline asks for it.
  set_wave_prio(e.prio);
  ENG eng;
  eng.init(smem_raw, e, tid, nt);
  T* act = reinterpret_cast<T*>(reinterpret_cast<C2<T>*>(smem_raw) + ENG::lds_complex(N));  // [2][A] current
  T* actp = act + 2 * e.A;                // [2][A] previous
  T* dots = actp + 2 * e.A;               // [2][S]
  T* part = dots + 2 * e.S;               // [8][2][S]
  T* red = part + 16 * e.S;               // [16]

  // member layout (pdec_env_set_member_layout): trajectory blockIdx.x alone, exactly the arithmetic of the B = 1 launch
  const int b0 = e.member ? (int)blockIdx.x : 2 * (int)blockIdx.x, b1 = b0 + 1;
  const bool has1 = !e.member && b1 < e.B;
  const size_t o0 = (size_t)b0 * N, o1 = (size_t)b1 * N;
  // disturbance (KSSetup.jl:155): cfg.mu, baked into the table dhat -- or, with pdec_env_set_disturbance, an amplitude per trajectory
  // on the table at mu = 1.  m0, m1 are uniform over the workgroup; a trajectory alone in it (the last of an odd batch, the member
  // layout) fills the empty slot with its own amplitude, as its B = 1 launch does with cfg.mu
  const C2<T>* __restrict__ dtab = MU ? e.dhat1 : e.dhat;
  T m0 = 1, m1 = 1;
  if constexpr (MU) { m0 = e.mu_b[b0]; m1 = e.mu_b[has1 ? b1 : b0]; }

  if (FUSED) {
    for (int a = tid; a < e.A; a += nt) {
      act[a] = action[(size_t)b0 * e.A + a];
      act[e.A + a] = has1 ? action[(size_t)b1 * e.A + a] : (T)0;
      actp[a] = action_prev[(size_t)b0 * e.A + a];
      actp[e.A + a] = has1 ? action_prev[(size_t)b1 * e.A + a] : (T)0;
      if constexpr (FLT) {
        act[a] = fault_action<T>(e.flt, b0, e.A, a, act[a]);
        if (has1) act[e.A + a] = fault_action<T>(e.flt, b1, e.A, a, act[e.A + a]);
      }
    }
  }
  __syncthreads();

  // LDSC: the per-mode constants, the constant term and the previous nonlinear term live in LDS (lane-private float4
  // slots) instead of 32 registers -- the kernel then fits in 64 VGPRs and a wave of it can share a SIMD with two waves
  // of the 222-VGPR critic pass (2 x 224 + 64 = 512), instead of waiting for / holding up a whole workgroup of it
  constexpr bool LDSC = SHARE;
  typedef T T4v __attribute__((ext_vector_type(4)));
  T4v* cst = reinterpret_cast<T4v*>(smem_raw + ((size_t)(reinterpret_cast<unsigned char*>(red + 16) - smem_raw + 15) & ~(size_t)15));
  C2<T> U[MPT], Nn[MPT], Ck[MPT], v[MPT];
  T kc1[MPT], kc2[MPT], kc3[MPT], kg[MPT];
  // forcing p (packed pair) -> spectrum -> constant term of the CNAB2 update
  T pa4[MPT], pb4[MPT];
  if (FUSED) {
    int n4[MPT];
#pragma unroll
    for (int j = 0; j < MPT; ++j) n4[j] = eng.phys_index(j);
    if ((N & 3) == 0 && 2 * N <= 16 * e.S) {     // `part` ([8][2][S], free until the sensor dots) holds the [2][N] scratch
      actuate_consecutive<T>(e, act, act + e.A, part, tid, nt);
#pragma unroll
      for (int j = 0; j < MPT; ++j) {
        pa4[j] = n4[j] < N ? part[n4[j]] : (T)0;
        pb4[j] = n4[j] < N ? part[N + n4[j]] : (T)0;
      }
    } else {
      actuate_cells<T, MPT>(e, act, act + e.A, n4, pa4, pb4);
    }
    if constexpr (FLT) {      // the forcing is made: back to the commanded action, which the reward punishes
      __syncthreads();
      for (int a = tid; a < e.A; a += nt) {
        act[a] = action[(size_t)b0 * e.A + a];
        if (has1) act[e.A + a] = action[(size_t)b1 * e.A + a];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MPT; ++j) {
    const int n = eng.phys_index(j);
    T pa = 0, pb = 0;
    if (n < N) {
      if (FUSED) {
        pa = pa4[j]; pb = pb4[j];
        if (!has1) pb = 0;
        if (p_out) {
          p_out[o0 + n] = pa;
          if (has1) p_out[o1 + n] = pb;
        }
      } else {
        pa = p_in[o0 + n];
        pb = has1 ? p_in[o1 + n] : (T)0;
      }
    }
    v[j] = mk<T>(pa, pb);
  }
  eng.template run<-1>(v);
#pragma unroll
  for (int j = 0; j < MPT; ++j) {
    const int k = eng.mode_index(j);
    if (k < N) {
      const C2<T> d = dtab[k];
      const T c4 = e.c4[k];
      // (1+i)*dhat: the same real disturbance enters both packed trajectories; MU: (m0 + i m1) * dhat1, each at its amplitude
      if constexpr (MU) Ck[j] = mk<T>(c4 * v[j].x + (m0 * d.x - m1 * d.y), c4 * v[j].y + (m0 * d.y + m1 * d.x));
      else Ck[j] = mk<T>(c4 * v[j].x + (d.x - d.y), c4 * v[j].y + (d.x + d.y));
      kc1[j] = e.c1[k];
      kc2[j] = e.c2[k];
      kc3[j] = e.c3[k];
      kg[j] = e.g[k];
    } else {
      Ck[j] = mk<T>(0, 0);
      kc1[j] = kc2[j] = kc3[j] = kg[j] = 0;
    }
    if constexpr (LDSC) cst[j * nt + tid] = T4v{kc1[j], kc2[j], kc3[j], kg[j]};
  }
  if constexpr (LDSC) {
    cst[4 * nt + tid] = T4v{Ck[0].x, Ck[0].y, Ck[1].x, Ck[1].y};
    cst[5 * nt + tid] = T4v{Ck[2].x, Ck[2].y, Ck[3].x, Ck[3].y};
  }
  // Nn = G * fft(u^2);  u_hat = fft(u)
#pragma unroll
  for (int j = 0; j < MPT; ++j) {
    const int n = eng.phys_index(j);
    U[j] = n < N ? mk<T>(y_in[o0 + n], has1 ? y_in[o1 + n] : (T)0) : mk<T>(0, 0);
    v[j] = mk<T>(U[j].x * U[j].x, U[j].y * U[j].y);
  }
  eng.template run<-1>(v);
#pragma unroll
  for (int j = 0; j < MPT; ++j) Nn[j] = cscale(mul_i<+1, T>(v[j]), kg[j]);   // G = i * (-alpha/2)
  if constexpr (LDSC) {
    cst[6 * nt + tid] = T4v{Nn[0].x, Nn[0].y, Nn[1].x, Nn[1].y};
    cst[7 * nt + tid] = T4v{Nn[2].x, Nn[2].y, Nn[3].x, Nn[3].y};
  }
  eng.template run<-1>(U);
  const T invN = (T)1 / (T)N;
  if constexpr (LDSC) {
    for (int it = 0; it < e.K; ++it) {
#pragma unroll
      for (int j = 0; j < MPT; ++j) v[j] = U[j];
      eng.template run<+1>(v);
#pragma unroll
      for (int j = 0; j < MPT; ++j) {
        const T wr = v[j].x * invN, wi = v[j].y * invN;
        v[j] = mk<T>(wr * wr, wi * wi);
      }
      eng.template run<-1>(v);
#pragma unroll
      for (int h = 0; h < 2; ++h) {          // modes 2h, 2h + 1
        const T4v nn = cst[(6 + h) * nt + tid], ck = cst[(4 + h) * nt + tid];
        T4v nw;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int j = 2 * h + u;
          const T4v c = cst[j * nt + tid];   // c1, c2, c3, g
          const C2<T> n1 = cscale(mul_i<+1, T>(v[j]), c[3]);
          U[j] = mk<T>(c[0] * U[j].x + c[1] * n1.x - c[2] * nn[2 * u] + ck[2 * u],
                       c[0] * U[j].y + c[1] * n1.y - c[2] * nn[2 * u + 1] + ck[2 * u + 1]);
          nw[2 * u] = n1.x; nw[2 * u + 1] = n1.y;
        }
        cst[(6 + h) * nt + tid] = nw;
      }
    }
  } else {
    for (int it = 0; it < e.K; ++it) {
#pragma unroll
      for (int j = 0; j < MPT; ++j) v[j] = U[j];
      eng.template run<+1>(v);
#pragma unroll
      for (int j = 0; j < MPT; ++j) {
        const T wr = v[j].x * invN, wi = v[j].y * invN;
        v[j] = mk<T>(wr * wr, wi * wi);
      }
      eng.template run<-1>(v);
#pragma unroll
      for (int j = 0; j < MPT; ++j) {
        const C2<T> nn1 = Nn[j];
        Nn[j] = cscale(mul_i<+1, T>(v[j]), kg[j]);
        U[j] = mk<T>(kc1[j] * U[j].x + kc2[j] * Nn[j].x - kc3[j] * nn1.x + Ck[j].x,
                     kc1[j] * U[j].y + kc2[j] * Nn[j].y - kc3[j] * nn1.y + Ck[j].y);
      }
    }
  }
  // y+ = real(ifft(u_hat))
  eng.template run<+1>(U);
  T mx0 = 0, mx1 = 0;
#pragma unroll
  for (int j = 0; j < MPT; ++j) {
    const int n = eng.phys_index(j);
    U[j] = mk<T>(U[j].x * invN, U[j].y * invN);
    if (n < N) {
      y_out[o0 + n] = U[j].x;
      if (has1) y_out[o1 + n] = U[j].y;
      // blow-up test max|y| > max_value (src/PDEenv.jl:227); a NaN also raises the flag
      // (deliberate deviation: Julia's `NaN > max_value` is false and the run would go on)
      if (!(fabs(U[j].x) <= e.max_value)) mx0 = 1;
      if (!(fabs(U[j].y) <= e.max_value)) mx1 = 1;
    }
  }
  if (done) {
    mx0 = block_max<T>(mx0, red, tid, nt);
    mx1 = block_max<T>(mx1, red, tid, nt);
    if (tid == 0) {
      const bool chk = e.check_max == 1;
      done[b0] = (chk && mx0 > 0) ? 1 : 0;
      if (has1) done[b1] = (chk && mx1 > 0) ? 1 : 0;
    }
    if (FUSED && e.check_max != 2) {
      write_terminal<T>(e, b0, e.check_max == 1 && mx0 > 0, tid, nt);
      if (has1) write_terminal<T>(e, b1, e.check_max == 1 && mx1 > 0, tid, nt);
    }
  }
  if (!FUSED) return;
  const T* Rt = reinterpret_cast<const T*>(eng.publish(U));
  sense_dots<T>(e, [&](int r, int n) { return Rt[2 * n + r]; }, dots, part, stid, snt);
  const int rw = e.mono ? 1 : e.A;             // reward entries per trajectory
  const int sw = e.mono ? e.S : e.A * e.ns;    // state entries per trajectory
  T rmine;
  const T* fd = dots;          // what featurize reads
  if constexpr (FLT) {
    fault_dots<T>(e.flt, b0, e.S, dots, part, tid, nt);
    if (has1) fault_dots<T>(e.flt, b1, e.S, dots + e.S, part + e.S, tid, nt);
    __syncthreads();
    fd = part;
  }
  if (e.fmap && !e.mono) {     // both trajectories in one pass each
    rmine = reward_pair<T>(e, dots, dots + e.S, act, act + e.A, actp, actp + e.A, reward_out + (size_t)b0 * rw,
                           has1 ? reward_out + (size_t)b1 * rw : nullptr, stid, snt);
    featurize_pair<T>(e, fd, fd + e.S, state_out + (size_t)b0 * sw, has1 ? state_out + (size_t)b1 * sw : nullptr, tid, nt);
  } else {
    rmine = reward_traj<T>(e, dots, act, actp, reward_out + (size_t)b0 * rw, stid, snt);
    featurize_traj<T>(e, fd, state_prev ? state_prev + (size_t)b0 * sw : nullptr, state_out + (size_t)b0 * sw, tid, nt);
    if (has1) {
      rmine += reward_traj<T>(e, dots + e.S, act + e.A, actp + e.A, reward_out + (size_t)b1 * rw, stid, snt);
      featurize_traj<T>(e, fd + e.S, state_prev ? state_prev + (size_t)b1 * sw : nullptr,
                        state_out + (size_t)b1 * sw, tid, nt);
    }
  }
  if (e.rsum_out) {
    // per-workgroup reward sum (fixed order: lanes by xor-shuffle, then waves in order) for the batch-mean reward of the
    // DDPG update's reward broadcast -- the critic pass then adds one partial per workgroup instead of re-reading all of r
    float v = (float)rmine;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = (T)v;
    __syncthreads();
    if (tid == 0) {
      float tot = 0.f;
      for (int i = 0; i < (nt + 63) / 64; ++i) tot += (float)red[i];
      e.rsum_out[blockIdx.x] = tot;
    }
  }
  if (done && e.check_max == 2) {
    // check_max_value == "reward" (src/PDEenv.jl:232-237): flag on max|reward|
    __syncthreads();
    if (tid == 0) {
      for (int t = 0; t < (has1 ? 2 : 1); ++t) {
        T m = 0;
        const T* r = reward_out + (size_t)(b0 + t) * rw;
        for (int a = 0; a < rw; ++a)
          if (!(fabs(r[a]) <= e.max_value)) m = 1;
        done[b0 + t] = m > 0 ? 1 : 0;
        write_terminal<T>(e, b0 + t, m > 0, 0, 1);
      }
    }
  }
  if constexpr (SYNC) launch_sync_done(e.sync);
}

// ------------------------------------------------------------------ host side
int ks_engine_threads(KsEngine k) {
  return with_ks_engine<float, true>(k, [](auto tag) { return (int)decltype(tag)::type::kThreads; });
}
size_t ks_lds_bytes(const pdec_env_cfg& c, KsEngine k) {      // the engine's buffers + act | actp | dots | part | red
  const size_t fft = with_ks_engine<float, true>(k, [&](auto tag) { return decltype(tag)::type::lds_complex(c.N); });
  return (fft * 2 + 4 * (size_t)c.A + 2 * c.S + 16 * c.S + 16) * dtype_size(c.dtype);
}

// The instantiation a launch takes.  FLT (pdec_env_set_faults) is a template argument -- its kernels take EnvDevF -- and exists for
// the fused forms only; SHARE: the 64-VGPR form (fp32 single-wave engine); SYNC: fp64 fixed plans (launch_step has checked the rest)
template <class T, class ENG, KsEngine KIND, bool FLT>
auto ks_step_kernel_for(bool fused, bool share, bool synced, bool mu) {
  auto kern = mu ? ks_env_step_kernel<T, ENG, true, false, false, true, FLT> : ks_env_step_kernel<T, ENG, true, false, false, false, FLT>;
  if constexpr (!FLT)
    if (!fused) kern = mu ? ks_env_step_kernel<T, ENG, false, false, false, true> : ks_env_step_kernel<T, ENG, false>;
  if constexpr (sizeof(T) == 4 && ks_is_single_wave(KIND))
    if (share) kern = mu ? ks_env_step_kernel<T, ENG, true, true, false, true, FLT> : ks_env_step_kernel<T, ENG, true, true, false, false, FLT>;
  if constexpr (!FLT && sizeof(T) == 8 && ks_is_fixed_plan(KIND))
    if (synced) kern = mu ? ks_env_step_kernel<T, ENG, true, false, true, true> : ks_env_step_kernel<T, ENG, true, false, true>;
  return kern;
}

int ks_launch_step(Env& E, bool fused, const StepArgs& a, const LaunchSync& sync) {
  const pdec_env_cfg& c = E.cfg;
  // pdec_env_set_two_wave_step: the engine of THIS launch (Env::engine, nthreads and lds_bytes stay those of the one-wave form)
  const KsEngine engine = ks_step_engine(E, fused);
  const bool two = engine != E.engine;
  const dim3 grid(E.member ? c.B : (c.B + 1) / 2), block(two ? ks_engine_threads(engine) : E.nthreads);
  const bool synced = sync.wait || sync.done;
  const bool mu = E.mu_b != nullptr;          // pdec_env_set_disturbance: the MU instantiation of whichever form is launched
  // SHARE: the 64-VGPR form + its lane-private constant slots (8 float4 per lane, 16-byte aligned)
  const bool share = fused && E.share_simd && c.dtype == PDEC_F32 && ks_is_single_wave(E.engine);
  const size_t lds = (two ? ks_lds_bytes(c, engine) : E.lds_bytes) + (share ? 16 + 8 * 16 * 64 : 0);
  // the training pipeline's form of the step, profiled in the pipeline (one launch per event pair): timed by the dispatch's own
  // timestamps (PDEC_TIMED_LAUNCH) so that the measurement puts no packets around the kernel
  const bool timed = c.dtype == PDEC_F32 && ks_is_single_wave(E.engine) && fused && E.prof && E.prof_reps == 1;
  by_dtype(c.dtype, [&](auto t) {
    using T = decltype(t);
    with_ks_engine<T, true>(engine, [&](auto tag) {
      using ENG = typename decltype(tag)::type;
      constexpr KsEngine KIND = decltype(tag)::kind;
      // one launch tail for the healthy and the fault-carrying kernels (their first argument differs: EnvDev / EnvDevF)
      auto launch = [&](auto kern, const auto& e) {
        if (timed) {
          PDEC_TIMED_LAUNCH(&E, "ks_env_step", kern, grid, block, lds, PDEC_STEP_KERNEL_ARGS(T, e, a));
          return;
        }
        // replay is safe when the step does not run in place (y_out != y_in)
        ProfScope ps(&E, fused ? "ks_env_step" : "ks_pde_step", !synced && a.y_out != a.y_in && a.state_out != a.state_prev);
        for (int rep = 0; rep < ps.reps; ++rep) hipLaunchKernelGGL(kern, grid, block, lds, E.stream, PDEC_STEP_KERNEL_ARGS(T, e, a));
      };
      if constexpr (KIND == KsEngine::Wave256x2) {      // ks_step_engine: fused, nothing opt-in set -- the one instantiation
        EnvDev<T> e = make_dev<T>(E);
        e.sync = sync;
        launch(ks_env_step_kernel<T, ENG, true>, e);
      } else if (fused && E.faults()) {              // pdec_env_set_faults (the integrator alone has neither side; a sync is refused before)
        launch(ks_step_kernel_for<T, ENG, KIND, true>(fused, share, synced, mu), make_dev_faults<T>(E));
      } else {
        EnvDev<T> e = make_dev<T>(E);
        e.sync = sync;
        launch(ks_step_kernel_for<T, ENG, KIND, false>(fused, share, synced, mu), e);
      }
    });
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

}  // namespace pdec
