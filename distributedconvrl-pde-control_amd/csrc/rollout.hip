// rollout.hip -- T control steps without the host in the loop.
//
// The reference's run loop (ReinforcementLearning.jl `run`, driven through src/PDEagent.jl:175-209 and
// src/PDEenv.jl:195-241) returns to the host after every control step; for evaluation / data-collection rollouts
// (`testrun`, PDEhook's bestDF logging, src/PDEhook.jl:51-63) nothing on the host depends on the step's result, so
// pdec_rollout enqueues all T steps -- actor forward + exploration noise + clamp, then the fused environment step --
// on the environment's stream in one call, ping-ponging the state buffers, accumulating the rewards and appending
// the per-step log rows on the device.  The caller synchronises once at the end (pdec_sync).
#include "env.hpp"
#include "mlp.hpp"

namespace pdec {

template <class T>
__global__ void rollout_accum_kernel(size_t n, const T* __restrict__ r, T* __restrict__ sum) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) sum[i] += r[i];
}
__global__ void rollout_or_kernel(int n, const int32_t* __restrict__ d, int32_t* __restrict__ acc, int32_t* __restrict__ first,
                                  int step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && d[i]) {
    acc[i] |= d[i];
    if (first && first[i] < 0) first[i] = step;
  }
}

}  // namespace pdec

using namespace pdec;

// The per-step form of a rollout, shared by pdec_rollout and the batched route of pdec_rollout_members: T times act(t, state,
// action_out) -- the caller's acting launch(es) on the environment's stream -- then the fused environment step, the reward sum,
// the done flags and the log rows, ping-ponging y / state / action between the caller's buffers and the environment's scratch.
template <class Act>
static int rollout_step_loop(pdec_handle henv, Env* E, int T, void* y, void* state, void* action, void* reward_sum, void* log_y,
                             void* log_p, void* log_action, void* log_reward, int32_t* done_any, int32_t* done_step, Act&& act) {
  const pdec_env_cfg& c = E->cfg;
  const size_t ts = dtype_size(c.dtype);
  const int ns = env_ns(c);
  const size_t ny = (size_t)c.B * env_y_count(c) * ts, np = (size_t)c.B * env_p_count(c) * ts, nact = (size_t)c.B * c.A * env_na(c) * ts;
  const size_t nst = (size_t)c.B * (c.mono ? c.S : (size_t)c.A * ns) * ts, nr = (size_t)c.B * (c.mono ? 1 : c.A) * ts;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  // scratch: second y / state / action buffers, p, reward, done
  const size_t need = al(ny) + al(nst) + al(nact) + al(np) + al(nr) + al(sizeof(int32_t) * c.B);
  if (E->roll.bytes < need) PDEC_HIP(E->roll.alloc(need));
  char* q = E->roll.as<char>();
  char* yb[2] = {(char*)y, q}; q += al(ny);
  char* sb[2] = {(char*)state, q}; q += al(nst);
  char* ab[2] = {(char*)action, q}; q += al(nact);      // ab[cur] = previous action, ab[cur ^ 1] receives the new one
  char* pb = q; q += al(np);
  char* rb = q; q += al(nr);
  int32_t* db = (int32_t*)q;
  if (done_any) PDEC_HIP(hipMemsetAsync(done_any, 0, sizeof(int32_t) * c.B, E->stream));
  if (done_step) PDEC_HIP(hipMemsetAsync(done_step, 0xFF, sizeof(int32_t) * c.B, E->stream));
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    // before step control_from (pdec_env_set_control_from) the zero action in the place of the acting call, unrewarded
    const bool ctl = t >= E->control_from;
    int rc = PDEC_OK;
    if (ctl) rc = act(t, (const void*)sb[cur], (void*)ab[cur ^ 1]);
    else PDEC_HIP(hipMemsetAsync(ab[cur ^ 1], 0, nact, E->stream));
    if (rc) return rc;
    rc = pdec_env_step(henv, yb[cur], ab[cur ^ 1], ab[cur], sb[cur], yb[cur ^ 1], pb, sb[cur ^ 1], rb, db);
    if (rc) return rc;
    cur ^= 1;
    const size_t nrew = nr / ts;
    if (reward_sum && ctl) {
      if (c.dtype == PDEC_F64)
        hipLaunchKernelGGL(rollout_accum_kernel<double>, dim3((unsigned)((nrew + 255) / 256)), dim3(256), 0, E->stream, nrew,
                           (const double*)rb, (double*)reward_sum);
      else
        hipLaunchKernelGGL(rollout_accum_kernel<float>, dim3((unsigned)((nrew + 255) / 256)), dim3(256), 0, E->stream, nrew,
                           (const float*)rb, (float*)reward_sum);
    }
    if (done_any)
      hipLaunchKernelGGL(rollout_or_kernel, dim3((c.B + 255) / 256), dim3(256), 0, E->stream, c.B, db, done_any, done_step, t);
    // PDEhook's per-step rows (src/PDEhook.jl:54-62), appended on the device
    if (log_y) PDEC_HIP(hipMemcpyAsync((char*)log_y + (size_t)t * ny, yb[cur], ny, hipMemcpyDeviceToDevice, E->stream));
    if (log_p) PDEC_HIP(hipMemcpyAsync((char*)log_p + (size_t)t * np, pb, np, hipMemcpyDeviceToDevice, E->stream));
    if (log_action) PDEC_HIP(hipMemcpyAsync((char*)log_action + (size_t)t * nact, ab[cur], nact, hipMemcpyDeviceToDevice, E->stream));
    if (log_reward) PDEC_HIP(hipMemcpyAsync((char*)log_reward + (size_t)t * nr, rb, nr, hipMemcpyDeviceToDevice, E->stream));
  }
  PDEC_HIP(hipGetLastError());
  if (cur == 1) {      // results back into the caller's buffers
    PDEC_HIP(hipMemcpyAsync(y, yb[1], ny, hipMemcpyDeviceToDevice, E->stream));
    PDEC_HIP(hipMemcpyAsync(state, sb[1], nst, hipMemcpyDeviceToDevice, E->stream));
    PDEC_HIP(hipMemcpyAsync(action, ab[1], nact, hipMemcpyDeviceToDevice, E->stream));
  }
  return PDEC_OK;
}

extern "C" int pdec_rollout(pdec_handle henv, pdec_handle hactor, int T, void* y, void* state, void* action,
                            double act_noise, double act_limit, int learning, uint64_t seed, uint64_t offset,
                            void* reward_sum, void* log_y, void* log_p, void* log_action, void* log_reward,
                            int32_t* done_any, int32_t* done_step) {
  Env* E = lookup_as<Env>(henv, Kind::Env);
  Mlp* A = lookup_as<Mlp>(hactor, Kind::Mlp);
  if (!E || !A) { set_error("pdec_rollout: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(T >= 1 && y && state && action, "pdec_rollout: null/empty argument");
  const pdec_env_cfg& c = E->cfg;
  PDEC_REQUIRE(A->dtype == c.dtype, "pdec_rollout: the actor and the environment must share one dtype");
  PDEC_REQUIRE(A->stream == E->stream, "pdec_rollout: the actor and the environment must share one stream");
  const int ns = env_ns(c), cols = c.B * (c.mono ? 1 : c.A), na = A->dims[A->L];
  PDEC_REQUIRE(A->dims[0] == (c.mono ? c.S : ns) && cols * na == c.B * c.A * env_na(c),
               "pdec_rollout: actor shape %d -> %d does not match the state/action matrices", A->dims[0], na);
  if (learning) PDEC_REFUSE_NOISE_COLOR(A, "pdec_rollout", "an exploring rollout does not advance its state: act step by step");
  const bool ntab = learning && A->noise_scale;
  if (ntab) PDEC_REQUIRE_NOISE_COLS(A, cols, "pdec_rollout");
  const RollSpec spec{T, learning, act_noise, act_limit, seed, offset, E->control_from, ntab ? A->noise_scale : nullptr, A->noise_scale_cpe};
  const RollPtrs ptrs{y, state, action, reward_sum, log_y, log_p, log_action, log_reward, done_any, done_step};
  // KS: the whole loop in ONE persistent launch -- the trajectories stay in registers / LDS between steps and the actor is
  // evaluated in the kernel (csrc/ks_rollout.hip: ks_rollout_kernel); reward_sum accumulates, the logs are written per step
  if (ks_rollout_supported(*E, *A, ntab)) return ks_rollout_persistent(*E, *A, spec, ptrs);
  // 1-D Keller-Segel: likewise one launch (csrc/kseg.hip: kseg_rollout_kernel)
  if (kseg_rollout_supported(*E, *A, ntab)) return kseg_rollout_persistent(*E, *A, spec, ptrs);
  return rollout_step_loop(henv, E, T, y, state, action, reward_sum, log_y, log_p, log_action, log_reward, done_any, done_step,
                           [&](int t, const void* s, void* a) {
                             return pdec_policy_act_rng(hactor, s, cols, act_noise, act_limit, learning, seed,
                                                        offset + (uint64_t)t * (((uint64_t)cols * na + 3) / 4), a);
                           });
}

// M actors, each driving its own block of per_member trajectories of one environment (population.py: evaluate_actors): ONE
// persistent launch (*served = 1: KS, 1-D Keller-Segel) or one batched step loop (*served = 2: fluid, 2-D Keller-Segel).
// Greedy only: the Philox numbering of the solo launches is by global column, so a member's noise stream is not defined here.
extern "C" int pdec_rollout_members(pdec_handle henv, const pdec_handle* actors, int M, int per_member, int T, void* y, void* state,
                                    void* action, double act_limit, int learning, void* reward_sum, void* log_y, void* log_p,
                                    void* log_action, void* log_reward, int32_t* done_any, int32_t* done_step, int* served) {
  Env* E = lookup_as<Env>(henv, Kind::Env);
  if (!E) { set_error("pdec_rollout_members: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(served, "pdec_rollout_members: served is null");
  *served = 0;
  PDEC_REQUIRE(actors && M >= 1 && per_member >= 1 && T >= 1 && y && state && action, "pdec_rollout_members: null/empty argument");
  PDEC_REQUIRE(learning == 0, "pdec_rollout_members: learning = 1 is not served (greedy evaluation only: the exploration noise is "
                              "numbered by global column, not per member)");
  const pdec_env_cfg& c = E->cfg;
  PDEC_REQUIRE((long long)M * per_member == c.B, "pdec_rollout_members: %d members x %d trajectories are not the environment's B = %d",
               M, per_member, c.B);
  std::vector<const Mlp*> nets(M);
  for (int m = 0; m < M; ++m) {
    nets[m] = lookup_as<Mlp>(actors[m], Kind::Mlp);
    if (!nets[m]) { set_error("pdec_rollout_members: bad actor handle (member %d)", m); return PDEC_E_HANDLE; }
    PDEC_REFUSE_NOISE_COLOR(nets[m], "pdec_rollout_members", "the member forms do not serve it");
  }
  for (int m = 1; m < M; ++m)
    if (nets[m]->dims != nets[0]->dims || nets[m]->acts != nets[0]->acts || nets[m]->dtype != nets[0]->dtype)
      return PDEC_OK;      // differing shapes: not served (the caller refuses or loops over solo rollouts)
  if (rollout_members_supported(*E, nets)) {
    int rc = rollout_members_persistent(*E, nets, per_member, T, act_limit,
                                        RollPtrs{y, state, action, reward_sum, log_y, log_p, log_action, log_reward, done_any, done_step});
    if (rc == PDEC_OK) *served = 1;
    return rc;
  }
  // the 2-D environments: no persistent launch, but ONE step loop for all members -- pdec_rollout's, with the member acting
  // kernel in the place of the solo acting call.  A trajectory's env step does not depend on B or on its place in the batch
  // there (grids (tiles, B), per-trajectory sensing; tests/test_gpu_act_members.py), so member m's rows are its solo rollout's.
  if (c.pde_kind != PDEC_PDE_FLUID_RK4 && c.pde_kind != PDEC_PDE_KSEG2D_RK4) return PDEC_OK;
  if (c.mono || c.memory_size > 0 || nets[0]->dims[0] != env_ns(c) || nets[0]->dims[nets[0]->L] != env_na(c)) return PDEC_OK;
  const int cols_per_member = per_member * c.A;
  if (!act_members_served(c.dtype, nets, cols_per_member)) return PDEC_OK;
  int rc = rollout_step_loop(henv, E, T, y, state, action, reward_sum, log_y, log_p, log_action, log_reward, done_any, done_step,
                             [&](int, const void* s, void* a) { return act_members_launch(*E, nets, s, cols_per_member, act_limit, a); });
  if (rc == PDEC_OK) *served = 2;
  return rc;
}
