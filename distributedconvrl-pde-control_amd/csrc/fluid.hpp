// fluid.hpp -- what the files of the 2-D fluid environment share: the device view FluidDev, the index maps of pad() / chop()
// (src/fluid_rk4.jl:192-229), the host object FluidEnv, the type of the wave-plan table, and the functions by which fluid.hip
// (host object, integrator, entry points), fluid_lds.hip (LDS-tile kernels), fluid_wave.hip (one-line-per-wave kernels and their
// plan table) and fluid_sense.hip (sensing, actuation, initialisers, error check) call each other.  fluid.hip has the design note.
//
// Every function declared here is a plain function of the environment: the dtype is resolved where a kernel template is named
// (fluid_by_dtype), never by the caller.
#pragma once
#include "env.hpp"
#include "mlp.hpp"
#include "wave_fft.hpp"

#include <type_traits>

namespace pdec {

#ifndef FL_NTH
#define FL_NTH 1024
#endif
#define FL_MAXE (3072 / FL_NTH)   // elements per thread of one tile: TL * p <= 3072
#ifndef FL_K2_TC
#define FL_K2_TC 4                // columns per workgroup of fluid_k2w_kernel
#endif

__host__ __device__ inline int fl_unpad(int ip, int n, int p) {   // chop(): padded index -> kept index or -1
  if (ip <= n / 2) return ip;
  if (ip >= p - n / 2 + 1) return ip - (p - n);
  return -1;
}
__host__ __device__ inline int fl_pad(int i, int n, int p) { return i <= n / 2 ? i : i + (p - n); }   // pad()
// the nl slow lines carried between the two inverse passes (n kept lines + the mirror of the Nyquist line)
__host__ __device__ inline int fl_line_jp(int s, int n, int p, int nl) { return s <= n / 2 ? s : s + p - nl; }
__host__ __device__ inline int fl_line_of(int jp, int n, int p, int nl) {
  if (jp <= n / 2) return jp;
  if (jp >= p - (nl - n / 2 - 1)) return jp - (p - nl);
  return -1;
}

template <class T>
struct FluidDev {
  int B, n, p, nl, TL, TLn, LS, LSn;
  int wtile;           // W between the two inverse passes is TILE-major, [b][f][p / 8][nl][8] (the persistent x-pass reads a
                       // tile as one contiguous block), instead of line-major [b][f][nl][p]
  T nu, inv2, scale_out, invn2;
  const T* k;          // [n] wavenumbers, [0..n/2, -n/2+1..-1] * 2 pi / L   (FluidSetup.jl:106-107)
  const C2<T>* twp;    // exp(-2 pi i m / p)
  const C2<T>* twn;    // exp(-2 pi i m / n)
  FftPlan plp, pln;
};

struct FluidEnv;

// One dtype's half of a row of the wave-plan table (fluid_wave.hip): the launchers of the WaveFft<T, E, Q, LB> instantiations
// that serve a padded length, each null where the instantiation is not built.
template <class T>
struct FluidWaveFns {
  // one right-hand side fused with an RK4 stage update, K1w + K2 + K3w (fluid_rhs_launch_wave)
  int (*rhs)(FluidEnv&, const FluidDev<T>&, const void* omg_s, const void* phat, const void* f0, void* acc, void* out, int mode,
             double ca, double cb);
  // the K sub-steps of a control step with K3 fused into the next K1 (fluid_integrate_wave)
  int (*integrate)(FluidEnv&, const FluidDev<T>&, void* f, const void* phat);
  // the persistent x-pass fluid_k2p_kernel, built for npw DMA pieces per wave and nsu output elements per thread (K2pGeom)
  int (*k2p)(FluidEnv&, const FluidDev<T>&);
  int k2p_npw, k2p_nsu;
  // wave_fft_debug_kernel on nlines lines (pdec_debug_wave_fft)
  void (*debug)(const void* in, void* out, const void* tw, int nlines, int sgn);
};
struct FluidWavePlan {
  int p, E, Q, LB;      // WaveFft<T, E, Q, LB> transforms lines of p points; LB 5: one line per HALF wave
  FluidWaveFns<double> f64;
  FluidWaveFns<float> f32;
  template <class T>
  const FluidWaveFns<T>& fns() const {
    if constexpr (std::is_same<T, float>::value) return f32;
    else return f64;
  }
};
// the row that serves padded length p, or null: fluid_make asks once per environment (and not at all under PDEC_FLUID_LDS_FFT)
const FluidWavePlan* fluid_wave_plan(int p);

struct FluidEnv : Env {
  int n = 0, p = 0, nl = 0, TL = 0, TLn = 0, BH = 0, BW = 0, nb1 = 0;
  FftPlan plp, pln;
  DevBuf k, twp, twn, sbox, sorg, abox, aorg, a2s_d, blkptr, blkidx;
  DevBuf W, W2, fs, acc, yreal, tmpc, dots, phat, icv, icd, errbits, yflag;
  size_t lds_p = 0, lds_n = 0;
  const FluidWavePlan* wave = nullptr;   // non-null: the one-line-per-wave transforms serve the padded length p
  // round 4: two child environments of B/2 trajectories each (own work arrays, own stream) that fluid_env_step runs side by
  // side -- trajectories are independent, and the kernels of a right-hand side differ in what bounds them (K1 / K2: fp64
  // issue, K3: HBM), so one half's K3 hides under the other half's transforms (n = 512, B = 16: 96.4 -> 100.8 env-steps/s)
  static constexpr int MAXPART = PartStreams::MAX;
  int nparts = 0;
  std::unique_ptr<FluidEnv> half[MAXPART];
  // round 5: the children's streams through the helper both split environments share (common.hpp PartStreams):
  // library-made streams are created at the first split step at the priority level of the environment's stream, as the 2-D
  // Keller-Segel environment does -- not at creation time at the lowest level, before pdec_set_stream had named that stream
  PartStreams ps;
  int part_streams() const override { return nparts >= 2 ? nparts - 1 : 0; }
  // the children exist since pdec_fluid_env_create: the caller's streams replace the library's one for one (all of them, or
  // PDEC_E_INVALID -- a child without a stream of its own would serialise behind another)
  int set_part_streams(const hipStream_t* s, int n) override {
    if (nparts < 2) return PDEC_OK;
    PDEC_REQUIRE(n >= nparts - 1, "pdec_env_set_part_streams: this environment runs %d parts and needs %d streams, got %d", nparts,
                 nparts - 1, n);
    PDEC_HIP(ps.give(s, nparts - 1));
    return PDEC_OK;
  }
  ~FluidEnv() override {
    for (int i = 0; i < MAXPART; ++i) half[i].reset();
  }
  int actuate(const void* action, void* p_out) override;
  int featurize(const void* y, const void* state_prev, void* state_out, const void* action = nullptr) override;
  int reward(const void* y, const void* action, const void* action_prev, void* r_out) override;
  int pde_step(const void* y_in, const void* p, void* y_out, int32_t* done) override;
  int rhs_eval(const void* y, const void* p, void* out) override;
  int env_step(const StepArgs& a) override;
};

// f(float{}) or f(double{}), by the environment's dtype: the one place that asks
template <class F>
static auto fluid_by_dtype(const FluidEnv& E, F&& f) {
  return E.cfg.dtype == PDEC_F32 ? f(float{}) : f(double{});
}

// does the persistent x-pass (fluid_k2p_kernel) serve this environment?  (fluid_wave.hip)
bool k2p_eligible(const FluidEnv& E);

template <class T>
static FluidDev<T> fluid_dev(const FluidEnv& E) {
  FluidDev<T> d;
  d.wtile = k2p_eligible(E) ? 1 : 0;
  d.B = E.cfg.B; d.n = E.n; d.p = E.p; d.nl = E.nl; d.TL = E.TL; d.TLn = E.TLn;
  d.LS = E.p + 2; d.LSn = E.n + 2;
  d.nu = (T)E.cfg.nu;
  const double inv = 1.0 / ((double)E.p * E.p);
  d.inv2 = (T)(inv * inv);                            // (scalars: computed in fp64, rounded once)
  d.scale_out = (T)(E.cfg.ifpad ? 1.5 * 1.5 : 1.0);   // src/fluid_rk4.jl:176
  d.invn2 = (T)(1.0 / ((double)E.n * E.n));
  d.k = E.k.as<T>(); d.twp = E.twp.as<C2<T>>(); d.twn = E.twn.as<C2<T>>();
  d.plp = E.plp; d.pln = E.pln;
  return d;
}

// ---- fluid_lds.hip
int pick_tile(int len);                       // lines per LDS tile of a transform of this length
int fluid_set_attrs(const FluidEnv& E);       // the dynamic-LDS limits of the LDS-tile kernels, at creation
// one right-hand side fused with an RK4 stage update on the LDS-tile kernels (mode as in fluid_k3_kernel)
int fluid_rhs_launch_lds(FluidEnv& E, const void* omg_s, const void* phat, const void* f0, void* acc, void* out, int mode, double ca,
                         double cb);
// the n x n transform pair: spec = fft2(real) (un-scaled), and E.yreal = real(ifft2(y))
int fluid_fft2_of_real(FluidEnv& E, const void* real, void* spec);
int fluid_to_physical(FluidEnv& E, const void* y);

// ---- fluid_sense.hip
FluidEnv* fluid_handle(pdec_handle h, const char* who);   // the fluid environment behind a handle, or null with the error set
int fluid_actuate(FluidEnv& E, const void* action, void* p_out);
int fluid_dots(FluidEnv& E, const void* y);
int fluid_feat_launch(FluidEnv& E, const void* action, const void* action_prev, const void* state_prev, void* state_out,
                      void* reward_out, int32_t* done, void* term_out = nullptr);
int fluid_done_y(FluidEnv& E, const void* y, int32_t* done);

}  // namespace pdec
