// env.hip -- the 1-D PDE environments: creation, the stand-alone sensing closures, the composed env step and the C API.
// The kernels of the three PDEs live in ks_step.hip / ks_rollout.hip (spectral KS), kseg.hip (Keller-Segel) and ksfd.hip
// (finite-difference KS); the 2-D environments (fluid.hip, kseg2d.hip) answer the same entry points through Env's virtuals.
#include "env_sense.hpp"
#include "roll_actor.hpp"

namespace pdec {

// ------------------------------------------------------------------ stand-alone closures
// MODE 0: prepare_action, 1: featurize, 2: reward (env_sense.hpp: sense_traj)
// FLT (pdec_env_set_faults): prepare_action with the actuator gains, featurize through the sensor faults; reward is unchanged
template <class T, int MODE, bool FLT = false>
__global__ void sense_kernel(EnvArg<T, FLT> e, const T* __restrict__ y, const T* __restrict__ action,
                             const T* __restrict__ action_prev, const T* __restrict__ state_prev,
                             T* __restrict__ out) {
  sense_traj<T, MODE, FLT>(e, blockIdx.x, y, action, action_prev, state_prev, out);
}

// terminal flag per actuator column from the per-trajectory blow-up flags (composed env step; the fused kernels write it themselves)
template <class T>
__global__ void terminal_from_done_kernel(const int32_t* __restrict__ done, int B, int cpt, T* __restrict__ term) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * cpt) term[i] = (done[i / cpt] & 1) ? (T)1 : (T)0;
}

// ------------------------------------------------------------------ host side
// the step of the environment's PDE (mode 0: fused env step, 1: integrate only, 2: right-hand side only)
static int launch_step(Env& E, int mode, const StepArgs& a) {
  const pdec_env_cfg& c = E.cfg;
  const bool fused = mode == 0;
  const LaunchSync sync = E.sync;
  E.sync = LaunchSync{};
  if (sync.wait || sync.done) {        // served by the SYNC instantiations of the KS step, refused everywhere else
    const bool ok = c.pde_kind == PDEC_PDE_KS_CNAB2 && fused && c.B <= 2 && !E.member && c.dtype == PDEC_F64 && ks_is_fixed_plan(E.engine) &&
                    !(E.prof && E.prof_reps > 1);
    PDEC_REQUIRE(ok, "pdec_env_step: a launch sync is set (pdec_set_launch_sync) and this step is not the fused single-workgroup fp64 "
                     "KS step of 192 / 240 / 600 cells");
    PDEC_REQUIRE(!E.faults(), "pdec_env_step: a launch sync is set (pdec_set_launch_sync) and so are fault arrays (pdec_env_set_faults): "
                              "the synchronised step has no fault-carrying form");
  }
  switch (c.pde_kind) {
    case PDEC_PDE_KS_CNAB2: return ks_launch_step(E, fused, a, sync);
    case PDEC_PDE_KSEG_RK4: return kseg_launch_step(E, mode, a);
    case PDEC_PDE_KS_RK4_FD: return ksfd_launch_step(E, mode, a);
  }
  set_error("pde_kind %d not implemented", c.pde_kind);
  return PDEC_E_INVALID;
}

// ---- persistent rollout, member form (pdec_rollout_members): M actors of one shape, K trajectories each, greedy.  The actors'
// parameters may be Float32 under an fp64 environment (the reference's shape) or of the environment's dtype.  *served = 0 and
// nothing enqueued where the solo form would not serve an actor of this shape either.
bool rollout_members_supported(const Env& E, const std::vector<const Mlp*>& actors) {
  const Mlp& A = *actors[0];
  if (A.dtype != PDEC_F32 && A.dtype != E.cfg.dtype) return false;
  return rollout_shape_ok(E, A, true) || rollout_shape_ok(E, A, false);
}
// the members' pointer table: uploaded on the environment's stream from host memory this object owns.  It is rewritten only when
// the members change, and then behind everything the stream still has to do (an earlier upload may not have read it yet)
int roll_tab_upload(Env& E, const std::vector<const Mlp*>& actors) {
  const size_t M = actors.size();
  std::vector<const void*> tab(M);
  for (size_t m = 0; m < M; ++m) tab[m] = actors[m]->params.p;
  if (tab != E.roll_tab_host || !E.roll_tab.p) {
    PDEC_HIP(hipStreamSynchronize(E.stream));
    E.roll_tab_host = tab;
    if (E.roll_tab.bytes < sizeof(void*) * M) PDEC_HIP(E.roll_tab.alloc(sizeof(void*) * M));
    PDEC_HIP(hipMemcpyAsync(E.roll_tab.p, E.roll_tab_host.data(), sizeof(void*) * M, hipMemcpyHostToDevice, E.stream));
  }
  return PDEC_OK;
}
int rollout_members_persistent(Env& E, const std::vector<const Mlp*>& actors, int K, int T, double act_limit, const RollPtrs& ptrs) {
  const int M = (int)actors.size();
  const Mlp& A = *actors[0];
  if (!rollout_members_supported(E, actors)) { set_error("rollout_members_persistent: configuration not covered"); return PDEC_E_INVALID; }
  PDEC_REQUIRE(K >= 1 && (long long)M * K == E.cfg.B, "rollout_members_persistent: %d members x %d trajectories are not the environment's B = %d",
               M, K, E.cfg.B);
  const int rct = roll_tab_upload(E, actors);
  if (rct) return rct;
  const RollMembers pm{E.roll_tab.as<const void*>(), K, A.dtype == PDEC_F32 ? 1 : 0};
  const RollSpec greedy{T, 0, 0.0, act_limit, 0, 0, E.control_from};
  return E.cfg.pde_kind == PDEC_PDE_KS_CNAB2 ? ks_rollout_persistent(E, A, greedy, ptrs, &pm) : kseg_rollout_persistent(E, A, greedy, ptrs, &pm);
}

// the stand-alone closures (mode 0: prepare_action, 1: featurize, 2: reward)
static int launch_sense(Env& E, int mode, const void* y, const void* action, const void* action_prev, const void* state_prev, void* out) {
  ProfScope ps(&E, mode == 0 ? "actuate" : (mode == 1 ? "featurize" : "reward"));
  by_dtype(E.cfg.dtype, [&](auto t) {
    using T = decltype(t);
    if (mode != 2 && E.faults()) {
      const auto kf = mode == 0 ? sense_kernel<T, 0, true> : sense_kernel<T, 1, true>;
      hipLaunchKernelGGL(kf, dim3(E.cfg.B), dim3(PDEC_SENSE_THREADS),
                         sense_lds_bytes(E.cfg), E.stream, make_dev_faults<T>(E), (const T*)y, (const T*)action, (const T*)action_prev,
                         (const T*)state_prev, (T*)out);
      return;
    }
    const auto kern = mode == 0 ? sense_kernel<T, 0> : (mode == 1 ? sense_kernel<T, 1> : sense_kernel<T, 2>);
    hipLaunchKernelGGL(kern, dim3(E.cfg.B), dim3(PDEC_SENSE_THREADS), sense_lds_bytes(E.cfg), E.stream, make_dev<T>(E), (const T*)y, (const T*)action,
                       (const T*)action_prev, (const T*)state_prev, (T*)out);
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

// (env::PDEenv)(action) with action memory (cfg.memory_size > 0): the closures one after the other on the environment's
// stream -- prepare_action (row 0 of every action column), the integrator, reward (row 0), featurize (window rows, temporal
// stack, memory rows = rows 1.. of the action).  No shipped script sets memory_size, so this reference surface is served by
// four launches instead of one and the fused step kernels keep their register budgets.  src/PDEenv.jl:195-241.
static int env_step_composed(Env& E, const StepArgs& a) {
  const pdec_env_cfg& c = E.cfg;
  const size_t pbytes = (size_t)c.B * env_p_count(c) * dtype_size(c.dtype), need = pbytes + (size_t)c.B * sizeof(int32_t) + 64;
  if (E.mem_scratch.bytes < need) PDEC_HIP(E.mem_scratch.alloc(need));
  void* p = a.p_out ? a.p_out : E.mem_scratch.p;
  int32_t* flags = a.done ? a.done : reinterpret_cast<int32_t*>(E.mem_scratch.as<char>() + pbytes);
  int rc;
  if ((rc = launch_sense(E, 0, nullptr, a.action, nullptr, nullptr, p))) return rc;
  if ((rc = launch_step(E, 1, StepArgs{a.y_in, p, nullptr, nullptr, nullptr, a.y_out, nullptr, nullptr, nullptr, flags}))) return rc;
  if ((rc = launch_sense(E, 2, a.y_out, a.action, a.action_prev, nullptr, a.reward_out))) return rc;
  if ((rc = launch_sense(E, 1, a.y_out, a.action, nullptr, a.state_prev, a.state_out))) return rc;
  if (E.term_out) {
    const int n = c.B * c.A;
    by_dtype(c.dtype, [&](auto t) {
      hipLaunchKernelGGL((terminal_from_done_kernel<decltype(t)>), dim3((n + 255) / 256), dim3(256), 0, E.stream, flags, c.B, c.A,
                         (decltype(t)*)E.term_out);
    });
    PDEC_HIP(hipGetLastError());
  }
  return PDEC_OK;
}

// ---- the 1-D closures behind the C API
int Env::actuate(const void* action, void* p_out) { return launch_sense(*this, 0, nullptr, action, nullptr, nullptr, p_out); }
int Env::featurize(const void* y, const void* state_prev, void* state_out, const void* action) {
  return launch_sense(*this, 1, y, action, nullptr, state_prev, state_out);
}
int Env::reward(const void* y, const void* action, const void* action_prev, void* r_out) {
  return launch_sense(*this, 2, y, action, action_prev, nullptr, r_out);
}
int Env::pde_step(const void* y_in, const void* p, void* y_out, int32_t* done) {
  return launch_step(*this, 1, StepArgs{y_in, p, nullptr, nullptr, nullptr, y_out, nullptr, nullptr, nullptr, done});
}
int Env::rhs_eval(const void* y, const void* p, void* out) {
  return launch_step(*this, 2, StepArgs{y, p, nullptr, nullptr, nullptr, out, nullptr, nullptr, nullptr, nullptr});
}
int Env::env_step(const StepArgs& a) { return cfg.memory_size > 0 ? env_step_composed(*this, a) : launch_step(*this, 0, a); }

}  // namespace pdec

using namespace pdec;

extern "C" {

int pdec_env_create(pdec_handle* h, const pdec_env_cfg* cfg, const double* sensor_kernels,
                    const double* actuator_kernels, const int32_t* a2s) {
  PDEC_REQUIRE(h && cfg && sensor_kernels && actuator_kernels && a2s, "pdec_env_create: null argument");
  const pdec_env_cfg& c = *cfg;
  PDEC_REQUIRE(c.dtype == PDEC_F32 || c.dtype == PDEC_F64, "pdec_env_create: bad dtype %d", c.dtype);
  PDEC_REQUIRE(c.B >= 1 && c.N >= 4 && c.S >= 1 && c.A >= 1 && c.K >= 1, "pdec_env_create: bad sizes B=%d N=%d S=%d A=%d K=%d",
               c.B, c.N, c.S, c.A, c.K);
  PDEC_REQUIRE(c.window >= 1 && (c.window & 1) && c.temporal_steps >= 1, "pdec_env_create: window must be odd >= 1");
  PDEC_REQUIRE(c.window <= c.S || c.mono, "pdec_env_create: window %d larger than sensor count %d", c.window, c.S);
  PDEC_REQUIRE(c.Lx > 0 && c.dt > 0, "pdec_env_create: Lx and dt must be positive");
  PDEC_REQUIRE(c.integrator == 0 || (c.integrator == 1 && (c.pde_kind == PDEC_PDE_KSEG_RK4 || c.pde_kind == PDEC_PDE_KS_RK4_FD)),
               "pdec_env_create: integrator %d is not available for pde_kind %d", c.integrator, c.pde_kind);
  PDEC_REQUIRE(c.memory_size >= 0 && c.memory_size <= 64, "pdec_env_create: memory_size %d out of range", c.memory_size);
  PDEC_REQUIRE(c.memory_size == 0 || (!c.mono && c.check_max_value != 2),
               "pdec_env_create: action memory is built for the per-actuator environments with check_max_value 0 / 1 "
               "(KSSetup.jl:216-226); the global-agent form and the reward-based blow-up test are not");
  for (int a = 0; a < c.A; ++a) PDEC_REQUIRE(a2s[a] >= 0 && a2s[a] < c.S, "pdec_env_create: a2s[%d]=%d out of range", a, a2s[a]);
  auto E = std::make_unique<Env>();
  E->cfg = c;
  const int N = c.N;
  std::vector<int32_t> a2s_h(a2s, a2s + c.A);
  if (c.pde_kind == PDEC_PDE_KS_CNAB2) {
    PDEC_REQUIRE(c.n_species == 1, "KS has one species");
    PDEC_REQUIRE(N % 2 == 0, "KS CNAB2 needs even N (Nyquist slot, KSSetup.jl:115)");
    PDEC_REQUIRE(make_fft_plan(N, E->fft), "N=%d has a prime factor other than 2,3,5", N);
    int nt = ((N + 4 - 1) / 4 + 63) / 64 * 64;      // four modes / cells per thread (KS_MPT)
    PDEC_REQUIRE(nt <= 1024, "N=%d too large for the in-LDS KS kernel (max 4096)", N);
    E->engine = ks_pick_engine(N, getenv("PDEC_KS_GENERIC_FFT") != nullptr, getenv("PDEC_KS_LDS_FFT") != nullptr);
    // the fixed plans: one butterfly per thread and stage -> the largest N / radix, rounded up to whole waves
    E->nthreads = ks_is_fixed_plan(E->engine) ? ks_engine_threads(E->engine) : nt;
    E->lds_bytes = ks_lds_bytes(c, E->engine);
    PDEC_REQUIRE(E->lds_bytes <= 160 * 1024, "KS kernel needs %zu B of LDS (> 160 KiB)", E->lds_bytes);
    // per-mode constants, scripts/KS/setup/KSSetup.jl:115-123,131-135
    std::vector<double> c1(N), c2(N), c3(N), c4(N), g(N), dh(2 * N), dh1(2 * N), tw(2 * N), dist(N), dist1(N);
    const double hh = c.dt / c.K, dt2 = hh / 2, dt32 = 3 * hh / 2, dx = c.Lx / N;
    for (int k = 0; k < N; ++k) {
      double kx = k < N / 2 ? k : (k == N / 2 ? 0 : k - N);
      double al = 2 * M_PI * kx / c.Lx;
      double L = al * al - al * al * al * al;
      double Ainv = 1.0 / (1.0 - dt2 * L), Bc = 1.0 + dt2 * L;
      c1[k] = Ainv * Bc; c2[k] = Ainv * dt32; c3[k] = Ainv * dt2; c4[k] = Ainv * hh; g[k] = -0.5 * al;
      tw[2 * k] = cos(2 * M_PI * k / N);
      tw[2 * k + 1] = -sin(2 * M_PI * k / N);
      dist1[k] = cos(2 + M_PI + (dx * (k + 1)) / (c.Lx / 2));        // KSSetup.jl:155
      dist[k] = c.mu * dist1[k];
    }
    for (int k = 0; k < N; ++k) {  // O(N^2) host DFT, setup time only
      double re = 0, im = 0;
      if (c.mu != 0.0)
        for (int n = 0; n < N; ++n) {
          long long ph = ((long long)k * n) % N;
          re += dist[n] * tw[2 * ph];
          im += dist[n] * tw[2 * ph + 1];
        }
      dh[2 * k] = hh * re;
      dh[2 * k + 1] = hh * im;
      // the same spectrum at mu = 1, scaled per trajectory in the kernels (pdec_env_set_disturbance): made here, so that the
      // setter stores a pointer and nothing else
      double re1 = 0, im1 = 0;
      for (int n = 0; n < N; ++n) {
        long long ph = ((long long)k * n) % N;
        re1 += dist1[n] * tw[2 * ph];
        im1 += dist1[n] * tw[2 * ph + 1];
      }
      dh1[2 * k] = hh * re1;
      dh1[2 * k + 1] = hh * im1;
    }
    int rc;
    if ((rc = upload_converted(E->c1, c1.data(), N, c.dtype))) return rc;
    if ((rc = upload_converted(E->c2, c2.data(), N, c.dtype))) return rc;
    if ((rc = upload_converted(E->c3, c3.data(), N, c.dtype))) return rc;
    if ((rc = upload_converted(E->c4, c4.data(), N, c.dtype))) return rc;
    if ((rc = upload_converted(E->g, g.data(), N, c.dtype))) return rc;
    if ((rc = upload_converted(E->dhat, dh.data(), 2 * N, c.dtype))) return rc;
    if ((rc = upload_converted(E->dhat1, dh1.data(), 2 * N, c.dtype))) return rc;
    if ((rc = upload_converted(E->tw, tw.data(), 2 * N, c.dtype))) return rc;
  } else if (c.pde_kind == PDEC_PDE_KS_RK4_FD) {
    PDEC_REQUIRE(c.n_species == 1, "KS has one species");
    int nt = (N + 63) / 64 * 64;
    PDEC_REQUIRE(nt <= 1024, "N=%d too large for the one-cell-per-thread KS finite-difference kernel (max 1024)", N);
    E->nthreads = nt;
    E->lds_bytes = ksfd_lds_bytes(c);
  } else if (c.pde_kind == PDEC_PDE_KSEG_RK4) {
    PDEC_REQUIRE(c.n_species == 2, "Keller-Segel has two species");
    PDEC_REQUIRE(!c.mono, "Keller-Segel has no mono variant");
    int nt = (N + 63) / 64 * 64;
    PDEC_REQUIRE(nt <= 1024, "N=%d too large for the one-cell-per-thread K-S kernel (max 1024)", N);
    E->nthreads = nt;
    E->lds_bytes = kseg_lds_bytes(c);
  } else {
    set_error("pdec_env_create: pde_kind %d not implemented", c.pde_kind);
    return PDEC_E_INVALID;
  }
  PDEC_REQUIRE(sense_lds_bytes(c) <= 160 * 1024, "sensor kernels need too much LDS");
  // tables: circular band form of the dense kernels.  An entry counts as non-zero if it is non-zero
  // in the plan's dtype, so the band product equals the dense product term by term.
  auto nz = [&](double v) { return c.dtype == PDEC_F64 ? v != 0.0 : (float)v != 0.0f; };
  // window of a circular 0/1 pattern: start after the longest run of zeros
  auto window = [&](const std::vector<char>& m, int& start, int& len) {
    const int n = (int)m.size();
    int best = -1, bestpos = 0, run = 0;
    bool any = false;
    for (int i = 0; i < n; ++i) any |= m[i] != 0;
    if (!any) { start = 0; len = 0; return; }
    for (int i = 0; i < 2 * n; ++i) {       // longest zero run on the ring
      if (!m[i % n]) { if (++run > best && run <= n) { best = run; bestpos = i; } }
      else run = 0;
    }
    if (best <= 0) { start = 0; len = n; return; }
    start = (bestpos + 1) % n;
    len = n - best;
  };
  std::vector<double> gs(c.S, 0.0);
  std::vector<int32_t> sn0(c.S), slen(c.S), an0(N), alen(N);
  int Wd = 1, Cnt = 1;
  for (int s = 0; s < c.S; ++s) {
    std::vector<char> m(N);
    for (int n = 0; n < N; ++n) { m[n] = nz(sensor_kernels[(size_t)s * N + n]); gs[s] += sensor_kernels[(size_t)s * N + n]; }
    int st, ln; window(m, st, ln);
    sn0[s] = st; slen[s] = ln; Wd = std::max(Wd, ln);
  }
  for (int n = 0; n < N; ++n) {
    std::vector<char> m(c.A);
    for (int a = 0; a < c.A; ++a) m[a] = nz(actuator_kernels[(size_t)a * N + n]);
    int st, ln; window(m, st, ln);
    an0[n] = st; alen[n] = ln; Cnt = std::max(Cnt, ln);
  }
  std::vector<double> Gs((size_t)Wd * c.S, 0.0), GaC((size_t)Cnt * N, 0.0);
  for (int s = 0; s < c.S; ++s)
    for (int j = 0; j < slen[s]; ++j) Gs[(size_t)j * c.S + s] = sensor_kernels[(size_t)s * N + (sn0[s] + j) % N];
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < alen[n]; ++i) GaC[(size_t)i * N + n] = actuator_kernels[(size_t)((an0[n] + i) % c.A) * N + n];
  E->Wd = Wd; E->Cnt = Cnt;
  int rc;
  if ((rc = upload_converted(E->Gs, Gs.data(), Gs.size(), c.dtype))) return rc;
  if ((rc = upload_converted(E->GaC, GaC.data(), GaC.size(), c.dtype))) return rc;
  if ((rc = upload_converted(E->gsum, gs.data(), gs.size(), c.dtype))) return rc;
  PDEC_HIP(E->sn0.alloc(sizeof(int32_t) * c.S));
  PDEC_HIP(hipMemcpy(E->sn0.p, sn0.data(), sizeof(int32_t) * c.S, hipMemcpyHostToDevice));
  PDEC_HIP(E->an0.alloc(sizeof(int32_t) * N));
  PDEC_HIP(hipMemcpy(E->an0.p, an0.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
  PDEC_HIP(E->a2s.alloc(sizeof(int32_t) * c.A));
  PDEC_HIP(hipMemcpy(E->a2s.p, a2s_h.data(), sizeof(int32_t) * c.A, hipMemcpyHostToDevice));
  if (!c.mono && c.temporal_steps == 1 && c.memory_size == 0) {
    // featurize as one gather (KSSetup.jl:190-229 without temporal stacking): state[a][rr] = dots[sp][(a2s[a] - i) mod S]
    const int ns1 = c.window * c.n_species, w = c.window / 2;
    std::vector<int32_t> fm((size_t)c.A * ns1);
    for (int a = 0; a < c.A; ++a)
      for (int rr = 0; rr < ns1; ++rr) {
        const int sp = rr / c.window, i = (rr - sp * c.window) - w;
        int s = (a2s_h[a] - i) % c.S;
        if (s < 0) s += c.S;
        fm[(size_t)a * ns1 + rr] = sp * c.S + s;
      }
    PDEC_HIP(E->fmap.alloc(sizeof(int32_t) * fm.size()));
    PDEC_HIP(hipMemcpy(E->fmap.p, fm.data(), sizeof(int32_t) * fm.size(), hipMemcpyHostToDevice));
  }
  *h = register_object(std::move(E));
  return PDEC_OK;
}

#define GET_ENV(E, h)                              \
  Env* E = lookup_as<Env>(h, Kind::Env);           \
  if (!E) {                                        \
    set_error("%s: not an env handle", __func__);  \
    return PDEC_E_HANDLE;                          \
  }

int pdec_env_set_terminal_out(pdec_handle h, void* terminal_per_column) {
  GET_ENV(E, h);
  E->term_out = terminal_per_column;
  return PDEC_OK;
}

int pdec_env_set_simd_sharing(pdec_handle h, int on, int* effective) {
  GET_ENV(E, h);
  E->share_simd = on != 0;
  if (effective) *effective = (E->share_simd && E->cfg.pde_kind == PDEC_PDE_KS_CNAB2 && ks_is_single_wave(E->engine) && E->cfg.dtype == PDEC_F32) ? 1 : 0;
  return PDEC_OK;
}

int pdec_env_set_two_wave_step(pdec_handle h, int on, int* effective) {
  GET_ENV(E, h);
  E->two_wave = on != 0;
  if (effective) *effective = ks_step_engine(*E, true) == KsEngine::Wave256x2 ? 1 : 0;
  return PDEC_OK;
}

// Population (population.py): every trajectory of the batch is an independent member; the KS step runs one trajectory per
// workgroup instead of two per complex FFT, so each member's result is bit for bit its B = 1 step and a blown-up member's
// NaNs stay in its own workgroup.  The other 1-D kinds already run one trajectory per workgroup.
int pdec_env_set_member_layout(pdec_handle h, int on) {
  GET_ENV(E, h);
  const int k = E->cfg.pde_kind;
  PDEC_REQUIRE(!on || k == PDEC_PDE_KS_CNAB2 || k == PDEC_PDE_KSEG_RK4,
               "pdec_env_set_member_layout: the 1-D KS and Keller-Segel environments only (pde kind %d)", k);
  PDEC_REQUIRE(!on || !E->rsum_out, "pdec_env_set_member_layout: per-pair reward partials are set (pdec_env_set_reward_partials_out)");
  E->member = on != 0;
  return PDEC_OK;
}

int pdec_env_set_disturbance(pdec_handle h, const void* mu_per_trajectory) {
  GET_ENV(E, h);
  const pdec_env_cfg& c = E->cfg;
  if (mu_per_trajectory) {
    PDEC_REQUIRE(c.pde_kind != PDEC_PDE_FLUID_RK4, "pdec_env_set_disturbance: the fluid has no disturbance term (KS environments only)");
    PDEC_REQUIRE(c.pde_kind != PDEC_PDE_KSEG_RK4 && c.pde_kind != PDEC_PDE_KSEG2D_RK4,
                 "pdec_env_set_disturbance: Keller-Segel has no disturbance term (KS environments only)");
    PDEC_REQUIRE(c.pde_kind == PDEC_PDE_KS_CNAB2 || c.pde_kind == PDEC_PDE_KS_RK4_FD, "pdec_env_set_disturbance: pde kind %d is not a KS environment",
                 c.pde_kind);
    PDEC_REQUIRE(!c.mono, "pdec_env_set_disturbance: the global/mono agent's step has no disturbance term (KSglobalSetup.jl:167); "
                          "per-actuator agents only");
  }
  E->mu_b = mu_per_trajectory;
  return PDEC_OK;
}

int pdec_env_set_faults(pdec_handle h, const void* actuator_gain, const void* sensor_gain, const void* sensor_bias) {
  GET_ENV(E, h);
  const pdec_env_cfg& c = E->cfg;
  if (actuator_gain || sensor_gain || sensor_bias) {
    PDEC_REQUIRE(c.pde_kind != PDEC_PDE_FLUID_RK4, "pdec_env_set_faults: the fluid is not served (KS environments only)");
    PDEC_REQUIRE(c.pde_kind != PDEC_PDE_KSEG2D_RK4, "pdec_env_set_faults: the 2-D Keller-Segel grid is not served (KS environments only)");
    PDEC_REQUIRE(c.pde_kind != PDEC_PDE_KSEG_RK4, "pdec_env_set_faults: Keller-Segel is not served (KS environments only)");
    PDEC_REQUIRE(c.pde_kind == PDEC_PDE_KS_CNAB2 || c.pde_kind == PDEC_PDE_KS_RK4_FD, "pdec_env_set_faults: pde kind %d is not a KS environment",
                 c.pde_kind);
    PDEC_REQUIRE(!c.mono, "pdec_env_set_faults: the global/mono agent is not served; per-actuator agents only");
    PDEC_REQUIRE(c.memory_size == 0, "pdec_env_set_faults: memory_size %d > 0 (action memory) is not served", c.memory_size);
  }
  E->act_gain = actuator_gain; E->sens_gain = sensor_gain; E->sens_bias = sensor_bias;
  return PDEC_OK;
}

int pdec_env_set_control_from(pdec_handle h, int n0) {
  GET_ENV(E, h);
  PDEC_REQUIRE(n0 >= 0, "pdec_env_set_control_from: n0 = %d is negative", n0);
  E->control_from = n0;
  return PDEC_OK;
}

int pdec_env_set_reward_partials_out(pdec_handle h, void* partial_sums, int* n_partials) {
  GET_ENV(E, h);
  const bool ks = E->cfg.pde_kind == PDEC_PDE_KS_CNAB2, ksfd = E->cfg.pde_kind == PDEC_PDE_KS_RK4_FD;
  PDEC_REQUIRE(!E->member || partial_sums == nullptr, "pdec_env_set_reward_partials_out: the member layout is set");
  PDEC_REQUIRE(((ks || ksfd) && E->cfg.memory_size == 0) || partial_sums == nullptr,
               "pdec_env_set_reward_partials_out: provided by the fused KS steps only (use pdec_reward_mean elsewhere)");
  E->rsum_out = (float*)partial_sums;
  // CNAB2: one workgroup integrates two trajectories; RK4 + FD: one trajectory per workgroup
  if (n_partials) *n_partials = ks ? (E->cfg.B + 1) / 2 : E->cfg.B;
  return PDEC_OK;
}

int pdec_env_part_streams(pdec_handle h, int* n) {
  GET_ENV(E, h);
  PDEC_REQUIRE(n, "pdec_env_part_streams: null");
  *n = E->part_streams();
  return PDEC_OK;
}

int pdec_env_set_part_streams(pdec_handle h, void* const* hip_streams, int n) {
  GET_ENV(E, h);
  PDEC_REQUIRE(n >= 0 && (n == 0 || hip_streams), "pdec_env_set_part_streams: bad arguments");
  for (int i = 0; i < n; ++i) PDEC_REQUIRE(hip_streams[i], "pdec_env_set_part_streams: stream %d is null", i);
  return E->set_part_streams((const hipStream_t*)hip_streams, n);
}

int pdec_actuate(pdec_handle h, const void* action, void* p_out) {
  GET_ENV(E, h);
  PDEC_REQUIRE(action && p_out, "pdec_actuate: null");
  return E->actuate(action, p_out);
}

int pdec_featurize(pdec_handle h, const void* y, const void* prev_state, void* state_out) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y && state_out, "pdec_featurize: null");
  PDEC_REQUIRE(prev_state != state_out, "pdec_featurize: state_out must not alias prev_state");
  return E->featurize(y, prev_state, state_out);
}

int pdec_featurize_action(pdec_handle h, const void* y, const void* prev_state, const void* action, void* state_out) {
  GET_ENV(E, h);
  if (!action || E->cfg.memory_size == 0) return pdec_featurize(h, y, prev_state, state_out);
  PDEC_REQUIRE(y && state_out, "pdec_featurize_action: null");
  PDEC_REQUIRE(prev_state != state_out, "pdec_featurize_action: state_out must not alias prev_state");
  return E->featurize(y, prev_state, state_out, action);
}

int pdec_reward(pdec_handle h, const void* y, const void* action, const void* action_prev, void* r_out) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y && action && action_prev && r_out, "pdec_reward: null");
  return E->reward(y, action, action_prev, r_out);
}

int pdec_pde_step(pdec_handle h, const void* y_in, const void* p, void* y_out, int32_t* done) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y_in && p && y_out, "pdec_pde_step: null");
  return E->pde_step(y_in, p, y_out, done);
}

int pdec_rhs_eval(pdec_handle h, const void* y, const void* p, void* out) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y && p && out, "pdec_rhs_eval: null");
  PDEC_REQUIRE(E->cfg.pde_kind != PDEC_PDE_KS_CNAB2, "pdec_rhs_eval: only RK4-type PDE kinds expose an RHS");
  return E->rhs_eval(y, p, out);
}

int pdec_env_step(pdec_handle h, const void* y_in, const void* action, const void* action_prev,
                  const void* state_prev, void* y_out, void* p_out, void* state_out, void* reward_out,
                  int32_t* done) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y_in && action && action_prev && y_out && state_out && reward_out, "pdec_env_step: null");
  PDEC_REQUIRE(!(E->cfg.temporal_steps > 1 && state_prev == state_out),
               "pdec_env_step: state_out must not alias state_prev when temporal_steps > 1");
  return E->env_step(StepArgs{y_in, nullptr, action, action_prev, state_prev, y_out, p_out, state_out, reward_out, done});
}

// ---- host-pointer wrappers: stage through one plan-owned device arena, synchronous
static int env_stage(Env* E, size_t bytes) {
  if (E->stage.bytes < bytes) PDEC_HIP(E->stage.alloc(bytes));
  return PDEC_OK;
}

int pdec_pde_step_host(pdec_handle h, const void* y_in, const void* p, void* y_out, int32_t* done) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y_in && p && y_out, "pdec_pde_step_host: null");
  const pdec_env_cfg& c = E->cfg;
  const size_t ts = dtype_size(c.dtype);
  const size_t ny = (size_t)c.B * env_y_count(c) * ts, np = (size_t)c.B * env_p_count(c) * ts;
  int rc = env_stage(E, 2 * ny + np + c.B * sizeof(int32_t) + 64);
  if (rc) return rc;
  char* base = E->stage.as<char>();
  char *dy = base, *dp = base + ny, *dyo = dp + np, *dd = dyo + ny;
  PDEC_HIP(hipMemcpyAsync(dy, y_in, ny, hipMemcpyHostToDevice, E->stream));
  PDEC_HIP(hipMemcpyAsync(dp, p, np, hipMemcpyHostToDevice, E->stream));
  rc = pdec_pde_step(h, dy, dp, dyo, (int32_t*)dd);
  if (rc) return rc;
  PDEC_HIP(hipMemcpyAsync(y_out, dyo, ny, hipMemcpyDeviceToHost, E->stream));
  if (done) PDEC_HIP(hipMemcpyAsync(done, dd, c.B * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
  PDEC_HIP(hipStreamSynchronize(E->stream));
  return PDEC_OK;
}

int pdec_env_step_host(pdec_handle h, const void* y_in, const void* action, const void* action_prev,
                       const void* state_prev, void* y_out, void* p_out, void* state_out, void* reward_out,
                       int32_t* done) {
  GET_ENV(E, h);
  PDEC_REQUIRE(y_in && action && action_prev && y_out && state_out && reward_out, "pdec_env_step_host: null");
  const pdec_env_cfg& c = E->cfg;
  const size_t ts = dtype_size(c.dtype);
  const int ns = env_ns(c);
  const size_t ny = (size_t)c.B * env_y_count(c) * ts, np = (size_t)c.B * env_p_count(c) * ts, na = (size_t)c.B * c.A * env_na(c) * ts;
  const size_t nst = (size_t)c.B * (c.mono ? c.S : c.A * ns) * ts, nr = (size_t)c.B * (c.mono ? 1 : c.A) * ts;
  auto al = [](size_t x) { return (x + 63) / 64 * 64; };
  int rc = env_stage(E, 2 * al(ny) + al(np) + 2 * al(na) + 2 * al(nst) + al(nr) + al(c.B * sizeof(int32_t)));
  if (rc) return rc;
  char* q = E->stage.as<char>();
  char* dy = q; q += al(ny);
  char* dyo = q; q += al(ny);
  char* dp = q; q += al(np);
  char* da = q; q += al(na);
  char* dap = q; q += al(na);
  char* dsp = q; q += al(nst);
  char* dso = q; q += al(nst);
  char* dr = q; q += al(nr);
  char* dd = q;
  PDEC_HIP(hipMemcpyAsync(dy, y_in, ny, hipMemcpyHostToDevice, E->stream));
  PDEC_HIP(hipMemcpyAsync(da, action, na, hipMemcpyHostToDevice, E->stream));
  PDEC_HIP(hipMemcpyAsync(dap, action_prev, na, hipMemcpyHostToDevice, E->stream));
  if (state_prev) PDEC_HIP(hipMemcpyAsync(dsp, state_prev, nst, hipMemcpyHostToDevice, E->stream));
  rc = pdec_env_step(h, dy, da, dap, state_prev ? dsp : nullptr, dyo, dp, dso, dr, (int32_t*)dd);
  if (rc) return rc;
  PDEC_HIP(hipMemcpyAsync(y_out, dyo, ny, hipMemcpyDeviceToHost, E->stream));
  if (p_out) PDEC_HIP(hipMemcpyAsync(p_out, dp, np, hipMemcpyDeviceToHost, E->stream));
  PDEC_HIP(hipMemcpyAsync(state_out, dso, nst, hipMemcpyDeviceToHost, E->stream));
  PDEC_HIP(hipMemcpyAsync(reward_out, dr, nr, hipMemcpyDeviceToHost, E->stream));
  if (done) PDEC_HIP(hipMemcpyAsync(done, dd, c.B * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
  PDEC_HIP(hipStreamSynchronize(E->stream));
  return PDEC_OK;
}

}  // extern "C"
