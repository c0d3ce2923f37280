// env.hpp -- the environment object shared by the 1-D environments (env.hip: creation, sensing and the C API; ks_step.hip,
// ks_rollout.hip, kseg.hip, ksfd.hip: their kernels) and the 2-D ones (fluid.hip, kseg2d.hip).
#pragma once
#include "common.hpp"
#include "fft_lds.hpp"
#include <type_traits>

namespace pdec {

template <class T>
struct EnvDev {
  int B, N, S, A, ns, window, temporal, mono, K, check_max, n_species, rk2, prio;
  int mem, na;           // action memory rows (cfg.memory_size) and rows per action column, na = 1 + mem: action [B][A][na]
  T sensor_scale, agent_power, r_in_scale, r_offset, r_power, r_denom, a_pun, da_pun, max_value;
  T dx, hstep, dist_mu;  // cell size, RK4 sub-step, KS disturbance amplitude (RK4-FD variant)
  // sensor / actuator kernels as circular BAND tables (exact: every non-zero entry of the dense
  // [S][N] / [A][N] matrices is kept; a kernel whose support is the whole domain gives Wd = N)
  const T* Gs;           // [Wd][S]   Gs[j][s] = g_s[(sn0[s] + j) mod N]     (coalesced over s)
  const int* sn0;        // [S]       first cell of sensor s's window
  const T* GaC;          // [Cnt][N]  GaC[i][n] = ga_{(an0[n]+i) mod A}[n]   (coalesced over n)
  const int* an0;        // [N]       first actuator reaching cell n
  int Wd, Cnt;
  float* rsum_out;       // optional [ceil(B/2)]: per-workgroup sum of the rewards it wrote (pdec_env_set_reward_partials_out)
  T* term_out;           // optional [B][cols per trajectory]: 1.0 where the trajectory blew up (pdec_env_set_terminal_out)
  const T* gsum;         // [S]     sum of each sensor kernel (reward offset term)
  const int* a2s;        // [A]
  const int* fmap;       // [A * ns] or null: state[idx] = dots[fmap[idx]] * sensor_scale (featurize without index arithmetic)
  // KS CNAB2 per-mode constants
  const T *c1, *c2, *c3, *c4, *g;
  const C2<T>* dhat;     // h * fft(mu cos(...))
  const C2<T>* dhat1;    // the same table at mu = 1 (pdec_env_set_disturbance: scaled per trajectory by mu_b)
  const T* mu_b;         // optional [B]: per-trajectory disturbance amplitude in the place of cfg.mu (pdec_env_set_disturbance)
  const C2<T>* tw;       // exp(-2 pi i k/N)
  FftPlan fft;
  LaunchSync sync;       // pdec_set_launch_sync (SYNC instantiations of the fused KS step only)
  int member = 0;        // pdec_env_set_member_layout: the KS step integrates ONE trajectory per workgroup (b0 = blockIdx.x)
};

// pdec_env_set_faults: per-trajectory actuator gains [B][A], sensor gains and biases [B][S] (each may be null: healthy).  The
// FLT instantiations of the KS kernels take EnvDevF, EnvDev with these three pointers behind it; every other kernel keeps
// EnvDev as its argument, and with it its kernel arguments and its code
template <class T>
struct FaultDev {
  const T *act_gain, *sens_gain, *sens_bias;
};
template <class T>
struct EnvDevF : EnvDev<T> {
  FaultDev<T> flt;
};
template <class T, bool FLT>
using EnvArg = std::conditional_t<FLT, EnvDevF<T>, EnvDev<T>>;

// The FFT engine of the spectral KS kernels (csrc/ks_engines.hpp: with_ks_engine maps an enumerator to its engine type).
enum class KsEngine {
  Wave256,      // N = 256: one wave, register-resident radix-4 (FftWave256)
  Wave1024,     // N = 1024: four waves x the same + one cross-wave stage through LDS (FftWave1024)
  LdsR4_256,    // N = 256 / 1024: radix-4 Stockham through LDS (FftR4<T, 4 / 5>), PDEC_KS_LDS_FFT=1 only
  LdsR4_1024,
  Fixed192,     // compile-time plans for the grids of the shipped experiments KS22 / KS200 / KS500 (FftFixed)
  Fixed240,
  Fixed600,
  Generic,      // any N = 2^a 3^b 5^c: mixed-radix Stockham through LDS (FftGeneric); every N under PDEC_KS_GENERIC_FFT=1
  Wave256x2,    // N = 256, fp32: the Wave256 transform over two waves (FftWave256x2); never Env::engine, see ks_step_engine
};
constexpr bool ks_is_single_wave(KsEngine k) { return k == KsEngine::Wave256; }
constexpr bool ks_is_fixed_plan(KsEngine k) { return k == KsEngine::Fixed192 || k == KsEngine::Fixed240 || k == KsEngine::Fixed600; }
// the engine of an N-cell grid under the two switches (read by pdec_env_create)
inline KsEngine ks_pick_engine(int N, bool force_generic, bool lds_fft) {
  if (force_generic) return KsEngine::Generic;
  if (N == 256) return lds_fft ? KsEngine::LdsR4_256 : KsEngine::Wave256;
  if (N == 1024) return lds_fft ? KsEngine::LdsR4_1024 : KsEngine::Wave1024;
  return N == 192 ? KsEngine::Fixed192 : N == 240 ? KsEngine::Fixed240 : N == 600 ? KsEngine::Fixed600 : KsEngine::Generic;
}
int ks_engine_threads(KsEngine k);      // ks_step.hip: ENG::kThreads

// the ten arrays of a step as they cross the C ABI, in the order the step kernels take them
struct StepArgs {
  const void *y_in, *p, *action, *action_prev, *state_prev;
  void *y_out, *p_out, *state_out, *reward_out;
  int32_t* done;
};

struct Env : Object {
  pdec_env_cfg cfg;
  DevBuf Gs, sn0, GaC, an0, gsum, a2s, fmap, c1, c2, c3, c4, g, dhat, dhat1, tw;
  int Wd = 0, Cnt = 0;
  DevBuf stage;  // staging for the _host wrappers
  DevBuf roll;   // ping-pong buffers of pdec_rollout
  DevBuf roll_tab;                          // pdec_rollout_members: the members' parameter pointers on the device ...
  std::vector<const void*> roll_tab_host;   // ... and the host image they were uploaded from (lives as long as the object)
  DevBuf mem_scratch;   // forcing field + flags of the composed env step (cfg.memory_size > 0)
  void* term_out = nullptr;
  float* rsum_out = nullptr;
  bool share_simd = false;   // pdec_env_set_simd_sharing: launch the 64-VGPR form of the fused KS step
  bool two_wave = false;     // pdec_env_set_two_wave_step: the fused fp32 N = 256 step on two waves per trajectory pair (ks_step_engine)
  bool member = false;       // pdec_env_set_member_layout: one KS trajectory per workgroup, the B = 1 launch's arithmetic
  const void* mu_b = nullptr;   // pdec_env_set_disturbance: caller-owned device array [B] of the environment's dtype
  int control_from = 0;         // pdec_env_set_control_from: the rollouts act from this step on (zero action before it)
  // pdec_env_set_faults: caller-owned device arrays of the environment's dtype, [B][A], [B][S], [B][S]; each may be null
  const void *act_gain = nullptr, *sens_gain = nullptr, *sens_bias = nullptr;
  bool faults() const { return act_gain || sens_gain || sens_bias; }
  FftPlan fft;
  int nthreads = 64;
  KsEngine engine = KsEngine::Generic;   // PDEC_PDE_KS_CNAB2 only
  size_t lds_bytes = 0;
  Env() : Object(Kind::Env) {}
  // environments that run parts of their batch on streams of their own (fluid.hip, kseg2d.hip): how many such streams the
  // step uses besides the environment's, and the caller's streams to use instead of the library's (pdec_env_set_part_streams)
  virtual int part_streams() const { return 0; }
  virtual int set_part_streams(const hipStream_t*, int) { return PDEC_OK; }
  // the closures behind pdec_actuate / pdec_featurize(_action) / pdec_reward / pdec_pde_step / pdec_rhs_eval / pdec_env_step,
  // called with checked arguments.  Here: the 1-D paths (env.hip); FluidEnv and Kseg2dEnv override them.
  virtual int actuate(const void* action, void* p_out);
  virtual int featurize(const void* y, const void* state_prev, void* state_out, const void* action = nullptr);
  virtual int reward(const void* y, const void* action, const void* action_prev, void* r_out);
  virtual int pde_step(const void* y_in, const void* p, void* y_out, int32_t* done);
  virtual int rhs_eval(const void* y, const void* p, void* out);
  virtual int env_step(const StepArgs& a);
};

// The engine a step launch takes: Env::engine, except that the fused step of an fp32 N = 256 CNAB2 environment with nothing
// opt-in set (no disturbance array, no faults, not the SIMD-sharing form, not the member layout) runs FftWave256x2 once pdec_env_set_two_wave_step asked
// for it.  The ONE statement of that rule: the launch (ks_launch_step) and the setter's `effective` both read it.
inline KsEngine ks_step_engine(const Env& E, bool fused) {
  const bool two = E.two_wave && fused && E.cfg.pde_kind == PDEC_PDE_KS_CNAB2 && E.engine == KsEngine::Wave256 &&
                   E.cfg.dtype == PDEC_F32 && !E.share_simd && !E.member && !E.mu_b && !E.faults();
  return two ? KsEngine::Wave256x2 : E.engine;
}

// ---- host pieces shared by the translation units of the 1-D environments: the kernels' view of an Env, the dtype dispatch
// and the step launches of the three PDEs
template <class T>
EnvDev<T> make_dev(const Env& E) {
  const pdec_env_cfg& c = E.cfg;
  EnvDev<T> e;
  e.B = c.B; e.N = c.N; e.S = c.S; e.A = c.A; e.window = c.window; e.temporal = c.temporal_steps;
  e.mono = c.mono; e.K = c.K; e.check_max = c.check_max_value; e.n_species = c.n_species;
  e.mem = c.memory_size; e.na = 1 + c.memory_size;      // (action memory: stand-alone closures + the composed env step only)
  e.ns = c.mono ? c.S : c.window * c.n_species * c.temporal_steps + c.memory_size;
  e.sensor_scale = (T)c.sensor_scale; e.agent_power = (T)c.agent_power;
  e.r_in_scale = (T)c.reward_in_scale; e.r_offset = (T)c.reward_offset; e.r_power = (T)c.reward_power;
  e.r_denom = (T)c.reward_denom; e.a_pun = (T)c.action_punish; e.da_pun = (T)c.delta_action_punish;
  e.max_value = (T)c.max_value;
  e.dx = (T)(c.Lx / c.N);
  e.hstep = (T)(c.dt / c.K);
  e.rk2 = c.integrator == 1;
  e.prio = env_prio("PDEC_PRIO_KS", (E.share_simd && ks_is_single_wave(E.engine) && c.dtype == PDEC_F32) ? 3 : 1);
  e.dist_mu = (T)c.mu;
  e.Gs = E.Gs.as<T>(); e.sn0 = E.sn0.as<int>(); e.GaC = E.GaC.as<T>(); e.an0 = E.an0.as<int>();
  e.Wd = E.Wd; e.Cnt = E.Cnt;
  e.gsum = E.gsum.as<T>(); e.a2s = E.a2s.as<int>();
  e.fmap = E.fmap.p ? E.fmap.as<int>() : nullptr;
  e.term_out = static_cast<T*>(E.term_out);
  e.rsum_out = E.rsum_out;
  e.c1 = E.c1.as<T>(); e.c2 = E.c2.as<T>(); e.c3 = E.c3.as<T>(); e.c4 = E.c4.as<T>(); e.g = E.g.as<T>();
  e.dhat = E.dhat.as<C2<T>>(); e.tw = E.tw.as<C2<T>>();
  e.dhat1 = E.dhat1.as<C2<T>>(); e.mu_b = static_cast<const T*>(E.mu_b);
  e.fft = E.fft;
  e.member = E.member ? 1 : 0;
  return e;
}

// the argument of the FLT instantiations (E.faults())
template <class T>
EnvDevF<T> make_dev_faults(const Env& E) {
  EnvDevF<T> e;
  static_cast<EnvDev<T>&>(e) = make_dev<T>(E);
  e.flt = FaultDev<T>{static_cast<const T*>(E.act_gain), static_cast<const T*>(E.sens_gain), static_cast<const T*>(E.sens_bias)};
  return e;
}

// f(T{}) with T = double or float by a PDEC_F64 / PDEC_F32 dtype: `by_dtype(dt, [&](auto t) { return g<decltype(t)>(...); })`
template <class F>
auto by_dtype(int dtype, F&& f) {
  return dtype == PDEC_F64 ? f(double{}) : f(float{});
}

// the arguments of a step kernel (the three PDEs share one list) from the untyped arrays
#define PDEC_STEP_KERNEL_ARGS(T, e, a)                                                                                      \
  e, (const T*)(a).y_in, (const T*)(a).p, (const T*)(a).action, (const T*)(a).action_prev, (const T*)(a).state_prev, \
      (T*)(a).y_out, (T*)(a).p_out, (T*)(a).state_out, (T*)(a).reward_out, (a).done

// The step of each PDE.  fused: the whole env step (else the integrator alone, on the forcing a.p); mode 0: fused env step,
// 1: integrate only, 2: right-hand side only.  sync (KS): a launch sync that launch_step has found servable.
int ks_launch_step(Env& E, bool fused, const StepArgs& a, const LaunchSync& sync);
int kseg_launch_step(Env& E, int mode, const StepArgs& a);
int ksfd_launch_step(Env& E, int mode, const StepArgs& a);
// dynamic LDS of the step kernels (Env::lds_bytes)
size_t ks_lds_bytes(const pdec_env_cfg& c, KsEngine k);
size_t kseg_lds_bytes(const pdec_env_cfg& c);
size_t ksfd_lds_bytes(const pdec_env_cfg& c);

// The persistent rollouts: T acting + env steps in ONE launch (ks_rollout.hip: ks_rollout_kernel, kseg.hip:
// kseg_rollout_kernel).  *_supported: the configuration is covered (else the caller loops per step); *_persistent returns
// PDEC_E_INVALID without touching anything when it is not.
struct Mlp;
struct RollMembers;
struct RollSpec {       // what the launch does
  int steps, learning;
  double act_noise, act_limit;
  uint64_t seed, offset;
  int control_from = 0;
  const double* noise_scale = nullptr;      // pdec_mlp_set_noise_scale on the actor, for a learning launch (null: act_noise)
  int noise_cpe = 1;
};
struct RollPtrs {       // its arrays as they cross the C ABI (pdec_rollout)
  void *y, *state, *action, *reward_sum, *log_y, *log_p, *log_action, *log_reward;
  int32_t *done_any, *done_step;
};
bool ks_rollout_supported(const Env& E, const Mlp& A, bool noise_tab = false);     // noise_tab: rollout_lds (roll_actor.hpp)
bool kseg_rollout_supported(const Env& E, const Mlp& A, bool noise_tab = false);
// pm != null: the member form (A = member 0's actor, the shape all members share; the caller has checked the shape)
int ks_rollout_persistent(Env& E, const Mlp& A, const RollSpec& spec, const RollPtrs& ptrs, const RollMembers* pm = nullptr);
int kseg_rollout_persistent(Env& E, const Mlp& A, const RollSpec& spec, const RollPtrs& ptrs, const RollMembers* pm = nullptr);
// the member form of the two launches above (pdec_rollout_members): actors[m] drives trajectories m K .. m K + K - 1
bool rollout_members_supported(const Env& E, const std::vector<const Mlp*>& actors);
int rollout_members_persistent(Env& E, const std::vector<const Mlp*>& actors, int K, int T, double act_limit, const RollPtrs& ptrs);

// E.roll_tab = the actors' parameter pointers, on E's stream (re-uploaded only when the members change)
int roll_tab_upload(Env& E, const std::vector<const Mlp*>& actors);
// act_members.hip: the acting step of M actors on one state matrix [M C][ns] in ONE launch (pdec_policy_act_members): the tile
// plan, whether the member form equals M solo pdec_policy_act_rng calls bit for bit, and the launch on E's stream
struct ActMembersPlan {
  int tile_cols = 0, tiles = 0;      // columns per workgroup (a multiple of 64; 0: one tile of 64 does not fit), tiles per member
  size_t lds = 0;                    // dynamic LDS of a workgroup
};
ActMembersPlan act_members_plan(const Mlp& A, int state_dtype, int cols_per_member);
bool act_members_served(int state_dtype, const std::vector<const Mlp*>& actors, int cols_per_member);
int act_members_launch(Env& E, const std::vector<const Mlp*>& actors, const void* state, int cols_per_member, double act_limit,
                       void* actions_out);

// element counts per trajectory of the arrays that cross the C ABI
inline size_t env_y_count(const pdec_env_cfg& c) {
  if (c.pde_kind == PDEC_PDE_FLUID_RK4) return (size_t)c.N * c.N * 2;
  if (c.pde_kind == PDEC_PDE_KSEG2D_RK4) return (size_t)c.N * c.Ny * 2;
  return (size_t)c.n_species * c.N;
}
inline size_t env_p_count(const pdec_env_cfg& c) {
  if (c.pde_kind == PDEC_PDE_FLUID_RK4) return (size_t)c.N * c.N * 2;
  if (c.pde_kind == PDEC_PDE_KSEG2D_RK4) return (size_t)c.N * c.Ny;
  return (size_t)c.N;
}
inline int env_ns(const pdec_env_cfg& c) {
  if (c.mono) return c.S;
  if (c.pde_kind == PDEC_PDE_FLUID_RK4) return c.window * c.window * c.temporal_steps + c.memory_size;
  if (c.pde_kind == PDEC_PDE_KSEG2D_RK4) return 2 * c.window * c.window * c.temporal_steps;
  return c.window * c.n_species * c.temporal_steps + c.memory_size;
}
inline int env_na(const pdec_env_cfg& c) { return 1 + c.memory_size; }

}  // namespace pdec
