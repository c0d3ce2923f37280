// fluid.hip -- batched 2-D pseudo-spectral vorticity environment for gfx950 (fp64; fp32 on the same kernels).
//
// Restates (from scratch, batched over independent trajectories):
//   rk4(f, p, dt)            src/fluid_rk4.jl:122-132      classical RK4, forcing frozen over the step
//   rhs(omghat, p)           src/fluid_rk4.jl:134-143      -nu k^2 w + advection(w) + p
//   advection(omghat)        src/fluid_rk4.jl:145-190      pseudo-spectral Jacobian, 3/2-rule de-aliasing
//   pad / chop               src/fluid_rk4.jl:192-229      index maps only (never materialised here)
//   do_step                  scripts/Fluid/setup/FluidSetup.jl:163-172   K = floor(16 nx dt) RK4 sub-steps
//   featurize / reward_function / prepare_action          FluidSetup.jl:188-261
//
// Design (HBM-bound path, so the point is to move fewer bytes than the reference's 5 padded
// 2-D FFTs per RHS):
//  * real(ifft(A)) = ifft(Herm(A)), Herm(A)[k] = (A[k] + conj(A[-k]))/2, so the four inverse
//    transforms of the reference (u, v, dw/dx, dw/dy; real part taken after each, :169-172)
//    become TWO complex transforms of Z1 = Herm(u^) + i Herm(v^), Z2 = Herm(wx^) + i Herm(wy^).
//    This is exact for any spectrum (Hermitian or not), including the +Nyquist modes the
//    reference keeps (FluidSetup.jl:106-107).
//  * the padded spectra are zero outside n (+1 mirror line) of the p = 3n/2 lines: the first
//    inverse pass only transforms those lines and the last forward pass only produces the n kept
//    ones (pruned 2-D FFT; pad()/chop() are index maps inside the kernels).
//  * the three slow-axis transforms (2 inverse, product, 1 forward) of a tile of columns happen
//    inside ONE kernel out of LDS: the physical-space fields never exist in HBM.  The forward
//    transform of the real product packs two columns as Re/Im of one complex line.
//  * RK4 stage updates and the linear term are fused into the last pass.
//  Per RHS and trajectory the HBM traffic is ~ (3 + 3) n p + 7 n^2 complex values (70 MB at n = 512)
//  instead of 5 * 2 * 2 * p^2 (189 MB) for un-fused library FFTs.
//
// Layout: Julia ComplexF64[ny, nx] column-major = memory [nx][ny] (y fastest); square box (nx = ny = n,
// Lx = Ly) as in every shipped script.  "fast axis" = y, "slow axis" = x.
//
// This file: the FluidEnv methods, the integrator of do_step and the env step on top of the right-hand sides, the split batch,
// creation, and the plan read-out.  The kernels and their launchers: fluid_lds.hip (LDS-tile family), fluid_wave.hip
// (one-line-per-wave family and the table of plans that dispatch reads), fluid_sense.hip (sensing, actuation, initialisers,
// error check); fluid.hpp has what they share.
#include "fluid.hpp"

namespace pdec {

// one right-hand side fused with an RK4 stage update (mode as in fluid_k3_kernel): on the environment's wave plan, else out of LDS
template <class T>
static int fluid_rhs_launch(FluidEnv& E, const void* omg_s, const void* phat, const void* f0, void* acc, void* out, int mode,
                            double ca, double cb) {
  if (E.wave) return E.wave->fns<T>().rhs(E, fluid_dev<T>(E), omg_s, phat, f0, acc, out, mode, ca, cb);
  return fluid_rhs_launch_lds(E, omg_s, phat, f0, acc, out, mode, ca, cb);
}

// (A HIP graph of the whole sub-step loop -- 8 K = 320 kernel nodes at the reference's own shape, one trajectory on the 128^2
// grid -- was measured and dropped: 232 against 260 env-steps/s eager.  That loop is not launch-bound: its kernels run
// 17-48 workgroups of ~10 us each on 256 CUs, HISTORY.md.)
// does fluid_integrate take the fused form (fluid_integrate_wave)?  Asked for by size or by PDEC_FLUID_FUSE, and served only where
// the environment's wave plan has a fused integrator (line pairs: n >= 256); a grid that asks and has none takes the plain loop.
static bool fluid_fused(const FluidEnv& E) {
  // measured (B = 16): n = 256: 650 -> 701 env-steps/s fused; n = 512: 76.6 -> 74.5 (the fused waves run six transforms
  // each and the stage's streaming phase no longer overlaps other waves' transforms) -> fused below 512 only
  static const char* fuse_env = getenv("PDEC_FLUID_FUSE");     // 1 / 0 force it on / off
  const bool fuse = fuse_env ? fuse_env[0] == '1' : (E.n >= 256 && E.n < 512);
  return fuse && E.n >= 256 && E.wave &&
         fluid_by_dtype(E, [&](auto t) { return E.wave->fns<decltype(t)>().integrate != nullptr; });
}

// do_step (FluidSetup.jl:163-172): K sub-steps of rk4 (src/fluid_rk4.jl:122-132), in place on f
template <class T>
static int fluid_integrate(FluidEnv& E, void* f, const void* phat) {
  if (fluid_fused(E)) return E.wave->fns<T>().integrate(E, fluid_dev<T>(E), f, phat);
  const double h = E.cfg.dt / E.cfg.K;
  void *fs = E.fs.p, *acc = E.acc.p;
  int rc;
  for (int it = 0; it < E.cfg.K; ++it) {
    if ((rc = fluid_rhs_launch<T>(E, f, phat, f, acc, fs, 1, 0.5 * h, h / 6.0))) return rc;
    if ((rc = fluid_rhs_launch<T>(E, fs, phat, f, acc, fs, 2, 0.5 * h, h / 3.0))) return rc;
    if ((rc = fluid_rhs_launch<T>(E, fs, phat, f, acc, fs, 2, h, h / 3.0))) return rc;
    if ((rc = fluid_rhs_launch<T>(E, fs, phat, f, acc, f, 4, 0.0, h / 6.0))) return rc;
  }
  return PDEC_OK;
}

int FluidEnv::actuate(const void* action, void* p_out) { return fluid_actuate(*this, action, p_out); }

int FluidEnv::featurize(const void* y, const void* state_prev, void* state_out, const void* action) {
  int rc = fluid_dots(*this, y);
  if (rc) return rc;
  // (action: the memory rows only)
  return fluid_feat_launch(*this, action, nullptr, state_prev, state_out, nullptr, nullptr);
}

int FluidEnv::reward(const void* y, const void* action, const void* action_prev, void* r_out) {
  int rc = fluid_dots(*this, y);
  if (rc) return rc;
  return fluid_feat_launch(*this, action, action_prev, nullptr, nullptr, r_out, nullptr);
}

int FluidEnv::rhs_eval(const void* y, const void* p, void* out) {
  return fluid_by_dtype(*this, [&](auto t) -> int {
    return fluid_rhs_launch<decltype(t)>(*this, y, p, nullptr, nullptr, out, 0, 0.0, 0.0);
  });
}

template <class T>
static int fluid_pde_step_t(FluidEnv& E, const void* y_in, const void* p, void* y_out, int32_t* done) {
  const size_t bytes = (size_t)E.cfg.B * E.n * E.n * sizeof(C2<T>);
  if (y_out != y_in) PDEC_HIP(hipMemcpyAsync(y_out, y_in, bytes, hipMemcpyDeviceToDevice, E.stream));
  int rc = fluid_integrate<T>(E, y_out, p);
  if (rc) return rc;
  if (done) {
    if (E.cfg.check_max_value == 1) return fluid_done_y(E, y_out, done);
    PDEC_HIP(hipMemsetAsync(done, 0, sizeof(int32_t) * E.cfg.B, E.stream));
  }
  return PDEC_OK;
}

int FluidEnv::pde_step(const void* y_in, const void* p, void* y_out, int32_t* done) {
  return fluid_by_dtype(*this, [&](auto t) -> int { return fluid_pde_step_t<decltype(t)>(*this, y_in, p, y_out, done); });
}

template <class T>
static int fluid_env_step_t(FluidEnv& E, const void* y_in, const void* action, const void* action_prev, const void* state_prev,
                            void* y_out, void* p_out, void* state_out, void* reward_out, int32_t* done) {
  void* ph = p_out ? p_out : E.phat.p;
  int rc;
  if ((rc = fluid_actuate(E, action, ph))) return rc;                                   // src/PDEenv.jl:199
  if ((rc = fluid_pde_step_t<T>(E, y_in, ph, y_out, nullptr))) return rc;               // :216-218
  if ((rc = fluid_dots(E, y_out))) return rc;
  // (terminal rows without a done array: check_max_value "y" leaves its flags in a slot of the environment's own)
  if (!done && E.term_out && E.cfg.check_max_value == 1) done = E.yflag.as<int32_t>();
  if (done && E.cfg.check_max_value != 2) {
    if (E.cfg.check_max_value == 1) { if ((rc = fluid_done_y(E, y_out, done))) return rc; }
    else PDEC_HIP(hipMemsetAsync(done, 0, sizeof(int32_t) * E.cfg.B, E.stream));
  }
  return fluid_feat_launch(E, action, action_prev, state_prev, state_out, reward_out, done, E.term_out);   // :220-222
}

int FluidEnv::env_step(const StepArgs& a) {
  FluidEnv& E = *this;
  if (E.nparts >= 2 && !E.prof) {
    // the parts of the batch side by side: every argument is batch-major, so a part is a pointer offset.  (Per-kernel
    // timing passes, pdec_prof_enable, take the whole batch on one stream.)
    const size_t nn = (size_t)E.n * E.n, A = E.cfg.A, ns = (size_t)env_ns(E.cfg), na = (size_t)env_na(E.cfg);
    const size_t ts = dtype_size(E.cfg.dtype);          // bytes of a real; a spectrum element is two
    auto off = [](const void* p, size_t bytes) -> const void* { return p ? (const char*)p + bytes : nullptr; };
    auto offm = [](void* p, size_t bytes) -> void* { return p ? (char*)p + bytes : nullptr; };
    {
      bool refused = false;
      PDEC_HIP(E.ps.ensure(E.stream, E.nparts, &refused));
      PDEC_REQUIRE(!refused, "fluid step: its %d part streams do not exist yet and cannot be made while the environment's stream is "
                   "being captured; run one step (or pdec_env_set_part_streams) before the capture, or PDEC_FLUID_SPLIT=0", E.nparts - 1);
    }
    {   // a fork that fails midway has already made some part streams wait: join them before returning
      const hipError_t ef = E.ps.fork(E.stream, E.nparts);
      if (ef != hipSuccess) { (void)E.ps.join(E.stream, E.nparts); PDEC_HIP(ef); }
    }
    int b0 = 0, rc_part = PDEC_OK;
    for (int hh = 0; hh < E.nparts; ++hh) {
      FluidEnv& H = *E.half[hh];
      H.stream = hh == 0 ? E.stream : E.ps.st[hh];
      H.term_out = E.term_out ? (char*)E.term_out + (size_t)b0 * A * ts : nullptr;
      const int rc = H.env_step(StepArgs{off(a.y_in, b0 * nn * 2 * ts), nullptr, off(a.action, b0 * A * na * ts),
                                         off(a.action_prev, b0 * A * na * ts), off(a.state_prev, b0 * A * ns * ts),
                                         offm(a.y_out, b0 * nn * 2 * ts), offm(a.p_out, b0 * nn * 2 * ts),
                                         offm(a.state_out, b0 * A * ns * ts), offm(a.reward_out, b0 * A * ts), a.done ? a.done + b0 : nullptr});
      if (rc) { rc_part = rc; break; }              // (the part streams are joined below on this path too)
      b0 += H.cfg.B;
    }
    const hipError_t ej = E.ps.join(E.stream, E.nparts);
    if (rc_part) return rc_part;
    PDEC_HIP(ej);
    return PDEC_OK;
  }
  return fluid_by_dtype(E, [&](auto t) -> int {
    return fluid_env_step_t<decltype(t)>(E, a.y_in, a.action, a.action_prev, a.state_prev, a.y_out, a.p_out, a.state_out,
                                         a.reward_out, a.done);
  });
}

}  // namespace pdec

using namespace pdec;

static int fluid_make(std::unique_ptr<FluidEnv>& out, const pdec_env_cfg& c, int BH, int BW, const double* sensor_boxes,
                      const int32_t* sensor_origin, const double* actuator_boxes, const int32_t* actuator_origin,
                      const int32_t* a2s) {
  PDEC_REQUIRE(c.pde_kind == PDEC_PDE_FLUID_RK4, "pdec_fluid_env_create: pde_kind must be PDEC_PDE_FLUID_RK4");
  PDEC_REQUIRE(c.dtype == PDEC_F64 || c.dtype == PDEC_F32, "pdec_fluid_env_create: bad dtype %d (ComplexF64 in the reference; "
               "ComplexF32 also served)", c.dtype);
  const int n = c.N;
  PDEC_REQUIRE(c.B >= 1 && n >= 8 && n % 4 == 0 && c.K >= 1, "pdec_fluid_env_create: bad sizes B=%d N=%d K=%d", c.B, n, c.K);
  PDEC_REQUIRE(c.S >= 1 && c.A >= 1 && c.sensors_per_axis >= 1 && c.sensors_per_axis * c.sensors_per_axis == c.S,
               "pdec_fluid_env_create: S must equal sensors_per_axis^2");
  // (a window wider than the sensor grid is served: circshift wraps any shift (FluidSetup.jl:219-224), and fluid_feat_kernel
  // reduces every offset modulo sensors_per_axis -- the window then visits a sensor more than once)
  PDEC_REQUIRE(c.window >= 1 && (c.window & 1) && c.temporal_steps >= 1 && !c.mono,
               "pdec_fluid_env_create: window must be odd; no mono variant");
  PDEC_REQUIRE(BH >= 1 && BW >= 1 && BH <= n && BW <= n, "pdec_fluid_env_create: bad box %dx%d", BH, BW);
  PDEC_REQUIRE(c.memory_size >= 0 && c.memory_size <= 64, "pdec_fluid_env_create: memory_size %d out of range", c.memory_size);
  PDEC_REQUIRE(c.Lx > 0 && c.dt > 0, "pdec_fluid_env_create: Lx and dt must be positive");
  for (int a = 0; a < c.A; ++a) PDEC_REQUIRE(a2s[a] >= 0 && a2s[a] < c.S, "pdec_fluid_env_create: a2s[%d] out of range", a);
  for (int s = 0; s < c.S; ++s)
    PDEC_REQUIRE(sensor_origin[2 * s] >= 0 && sensor_origin[2 * s] < n && sensor_origin[2 * s + 1] >= 0 &&
                     sensor_origin[2 * s + 1] < n, "pdec_fluid_env_create: sensor origin %d out of range", s);
  for (int a = 0; a < c.A; ++a)
    PDEC_REQUIRE(actuator_origin[2 * a] >= 0 && actuator_origin[2 * a] < n && actuator_origin[2 * a + 1] >= 0 &&
                     actuator_origin[2 * a + 1] < n, "pdec_fluid_env_create: actuator origin %d out of range", a);
  auto E = std::make_unique<FluidEnv>();
  E->cfg = c;
  E->n = n;
  E->p = c.ifpad ? n * 3 / 2 : n;
  E->nl = c.ifpad ? n + 1 : n;
  E->BH = BH; E->BW = BW;
  PDEC_REQUIRE(E->p <= 1536, "N=%d too large for the in-LDS line FFTs (max 1024 padded / 1536 un-padded)", n);
  PDEC_REQUIRE(make_fft_plan(E->p, E->plp) && make_fft_plan(n, E->pln), "N=%d: sizes must factor into 2,3,5", n);
  // one-line-per-wave register transforms where the plan table has a row for the padded length
  static const bool lds_fft = getenv("PDEC_FLUID_LDS_FFT") != nullptr;
  if (!lds_fft) E->wave = fluid_wave_plan(E->p);
  E->TL = pick_tile(E->p);
  E->TLn = pick_tile(n);
  PDEC_REQUIRE(E->TL >= 2, "internal: tile too small");
  const size_t ts = dtype_size(c.dtype), zs = 2 * ts;     // bytes of a real / of a complex element
  E->lds_p = ((size_t)2 * E->TL * (E->p + 2) + E->p) * zs;
  E->lds_n = ((size_t)2 * E->TLn * (n + 2) + n) * zs;
  PDEC_REQUIRE(E->lds_p <= 160 * 1024 && E->lds_n <= 160 * 1024, "fluid kernels need too much LDS");
  std::vector<double> k(n), twp(2 * (size_t)E->p), twn(2 * (size_t)n);
  for (int i = 0; i < n; ++i) k[i] = (i <= n / 2 ? i : i - n) / c.Lx * 2 * M_PI;     // FluidSetup.jl:106
  for (int m = 0; m < E->p; ++m) { twp[2 * m] = cos(2 * M_PI * m / E->p); twp[2 * m + 1] = -sin(2 * M_PI * m / E->p); }
  for (int m = 0; m < n; ++m) { twn[2 * m] = cos(2 * M_PI * m / n); twn[2 * m + 1] = -sin(2 * M_PI * m / n); }
  int rc;
  // (wavenumbers, twiddles and box tables: computed in fp64 and rounded once to the environment's dtype)
  if ((rc = upload_converted(E->k, k.data(), n, c.dtype))) return rc;
  if ((rc = upload_converted(E->twp, twp.data(), twp.size(), c.dtype))) return rc;
  if ((rc = upload_converted(E->twn, twn.data(), twn.size(), c.dtype))) return rc;
  if ((rc = upload_converted(E->sbox, sensor_boxes, (size_t)c.S * BH * BW, c.dtype))) return rc;
  if ((rc = upload_converted(E->abox, actuator_boxes, (size_t)c.A * BH * BW, c.dtype))) return rc;
  auto up_i = [](DevBuf& b, const int32_t* src, size_t cnt) -> int {
    PDEC_HIP(b.alloc(sizeof(int32_t) * (cnt ? cnt : 1)));
    if (cnt) PDEC_HIP(hipMemcpy(b.p, src, sizeof(int32_t) * cnt, hipMemcpyHostToDevice));
    return PDEC_OK;
  };
  if ((rc = up_i(E->sorg, sensor_origin, 2 * (size_t)c.S))) return rc;
  if ((rc = up_i(E->aorg, actuator_origin, 2 * (size_t)c.A))) return rc;
  if ((rc = up_i(E->a2s_d, a2s, c.A))) return rc;
  // candidate actuators per 16x16 block of cells
  E->nb1 = (n + 15) / 16;
  std::vector<int32_t> ptr(1, 0), idx;
  auto meets = [&](int o, int len, int c0) {   // ring interval [o, o+len) meets cells [c0, c0+16)
    for (int q = 0; q < 16 && c0 + q < n; ++q) {
      int dlt = c0 + q - o;
      if (dlt < 0) dlt += n;
      if (dlt < len) return true;
    }
    return false;
  };
  for (int bj = 0; bj < E->nb1; ++bj)
    for (int bi = 0; bi < E->nb1; ++bi) {
      for (int a = 0; a < c.A; ++a)
        if (meets(actuator_origin[2 * a], BW, bj * 16) && meets(actuator_origin[2 * a + 1], BH, bi * 16)) idx.push_back(a);
      ptr.push_back((int32_t)idx.size());
    }
  if ((rc = up_i(E->blkptr, ptr.data(), ptr.size()))) return rc;
  if ((rc = up_i(E->blkidx, idx.data(), idx.size()))) return rc;
  const size_t nn = (size_t)n * n, Bz = c.B;
  PDEC_HIP(E->W.alloc(Bz * 2 * E->nl * E->p * zs));
  PDEC_HIP(E->W2.alloc(Bz * n * E->p * zs));
  PDEC_HIP(E->fs.alloc(Bz * nn * zs));
  PDEC_HIP(E->acc.alloc(Bz * nn * zs));
  PDEC_HIP(E->tmpc.alloc(Bz * nn * zs));
  PDEC_HIP(E->phat.alloc(Bz * nn * zs));
  PDEC_HIP(E->yreal.alloc(Bz * nn * ts));
  PDEC_HIP(E->dots.alloc(Bz * c.S * ts));
  // pdec_fluid_error_detection's bits and the vortex table of ic(3) / ic(4) (50 vortices; a longer table grows it): made here, so
  // that the device entry points only enqueue
  PDEC_HIP(E->errbits.alloc(Bz * sizeof(int32_t)));
  PDEC_HIP(E->icv.alloc(Bz * 50 * 4 * ts));
  // the flag slot of the terminal rows under check_max_value "y" (every child of a split batch needs its own): made here too
  PDEC_HIP(E->yflag.alloc(Bz * sizeof(int32_t)));
  if ((rc = fluid_set_attrs(*E))) return rc;
  out = std::move(E);
  return PDEC_OK;
}

extern "C" int pdec_fluid_env_create(pdec_handle* h, const pdec_env_cfg* cfg, int BH, int BW, const double* sensor_boxes,
                                     const int32_t* sensor_origin, const double* actuator_boxes,
                                     const int32_t* actuator_origin, const int32_t* a2s) {
  PDEC_REQUIRE(h && cfg && sensor_boxes && sensor_origin && actuator_boxes && actuator_origin && a2s,
               "pdec_fluid_env_create: null argument");
  std::unique_ptr<FluidEnv> E;
  int rc = fluid_make(E, *cfg, BH, BW, sensor_boxes, sensor_origin, actuator_boxes, actuator_origin, a2s);
  if (rc) return rc;
  // pdec_fluid_ic_rng's table of doubles (50 vortices, ic(4)), on the environment the caller holds only -- the initialisers serve
  // a split batch from the parent's own arrays --: made here, so that the calls of a run only enqueue
  PDEC_HIP(E->icd.alloc((size_t)cfg->B * 50 * 4 * sizeof(double)));
  // part-batch children for the fused env step where a part still fills the chip (padded 512-point grids and up): two by
  // default; PDEC_FLUID_SPLIT=0 off, 1 / 2 two parts, 3 / 4 that many
  static const char* sp = getenv("PDEC_FLUID_SPLIT");
  int np = sp ? atoi(sp) : ((cfg->N >= 512 && cfg->B >= 8) ? 2 : 0);
  if (np == 1) np = 2;                                  // (PDEC_FLUID_SPLIT=1: on = two parts; 0: off; 3, 4: that many parts)
  np = std::min(std::min(np, (int)FluidEnv::MAXPART), cfg->B);
  if (np >= 2) {
    pdec_env_cfg ch = *cfg;
    int left = cfg->B;
    for (int i = 0; i < np; ++i) {
      ch.B = left / (np - i);
      left -= ch.B;
      if ((rc = fluid_make(E->half[i], ch, BH, BW, sensor_boxes, sensor_origin, actuator_boxes, actuator_origin, a2s))) return rc;
    }
    E->nparts = np;                                    // (streams and events: PartStreams::ensure at the first split step)
  }
  *h = register_object(std::move(E));
  return PDEC_OK;
}
// Unit-test entry: the dispatch decisions of this environment, by the host code that dispatches; see include/pdeconv_debug.h
extern "C" int pdec_debug_fluid_plan(pdec_handle h, int32_t* out12) {
  FluidEnv* Ep = fluid_handle(h, "pdec_debug_fluid_plan");
  if (!Ep) return PDEC_E_HANDLE;
  PDEC_REQUIRE(out12, "pdec_debug_fluid_plan: null out12");
  const FluidEnv& E = *Ep;
  const bool k2p = k2p_eligible(E);
  const FluidWavePlan* w = E.wave;
  const int32_t plan[12] = {E.p, E.nl, E.TL, E.TLn, w ? w->E : 0, w ? w->Q : 0, w ? w->LB : 0, w && E.n >= 256 ? 1 : 0,
                            k2p ? 1 : 0, fluid_fused(E) ? 1 : 0, E.nparts, k2p ? E.cfg.B * (E.p / 8) : 0};
  for (int i = 0; i < 12; ++i) out12[i] = plan[i];
  return PDEC_OK;
}
