// ledger.hip -- the episode bookkeeping of PDEhook (src/PDEhook.jl:51-97) for the batched training pipeline, on the device.
//
// The hook adds the batch-mean reward of every control step to a host accumulator, keeps the episode sums, and at the end
// of an episode whose number reaches min_best_episode copies the actor into bestNNA when its sum is >= every earlier one
// (:65-76).  The pipeline cannot read anything back per step (recorded steps, HIP graphs), so the ledger keeps all of it on
// the device and every launch's arguments depend only on buffers that the pipeline rotates with the step counter:
//   pdec_ledger_step      behind the env step: ret_b += (sum_a (double) r[b][a]) / R, the sum over a in index order;
//                         blew_b |= flags[b] != 0
//   pdec_ledger_snapshot  behind the acting kernel of an episode's last step: the actor parameters it read -> staging
//   pdec_ledger_close     at the episode's last step: row e mod cap <- (ret [B], blew [B], mean = (sum_b ret_b) / B summed
//                         in b order); the best decision of the hook, made on the device; the running sums back to 0.
// Greedy held-out evaluation (no counterpart in the hook, which knows the noisy training return only; it replaces the noise-free
// env.rollout on a fixed set of fields that tools/pipeline_learning_probe.py ran after a run): the pipeline rolls the snapshot out
// on an environment of K held-out fields and the ledger scores it.  Per trajectory b of that rollout's reward_sum [K][R] and
// done_step [K]:  ret_b = (sum_a (double) reward_sum[b][a]) / R in a order, blew_b = done_step[b] >= 0;  score = (sum_b ret_b) / K
// in b order, NaN when any blew_b is set or any ret_b is not finite (population.py: score_members' rule).
//   pdec_ledger_eval_load   training env stream, behind the snapshot: staging -> the evaluation actor's parameters
//   pdec_ledger_eval_close  evaluation stream, behind the rollout: row n mod cap <- (ret [K], blew [K], score, episode); the hook's
//                           rule on the scores; the evaluation actor's parameters -> the best-by-evaluation buffer when chosen.
// Nothing is read back until a host accessor is called.
#include <cmath>

#include "env.hpp"
#include "mlp.hpp"

namespace pdec {

struct LedgerState {
  double best_val;      // value of the best episode (PDEhook's initial bestreward: -1e6)
  double max_elig;      // largest non-NaN mean of an eligible episode so far (-inf: none)
  long long best_ep;    // 1-based number of the best episode (0: none yet), PDEhook.bestepisode
  long long pad;
};

struct Ledger : Object {
  pdec_handle env = 0, actor = 0;
  int B = 0, R = 0, env_dtype = PDEC_F32, cap = 0, nparams = 0, par_dtype = PDEC_F32;
  std::vector<int> dims;
  DevBuf run_ret, run_blew;     // double [B], int32 [B]
  DevBuf rows_ret, rows_blew;   // double [cap][B], int32 [cap][B]
  DevBuf rows_mean;             // double [cap]
  DevBuf st;                    // LedgerState
  DevBuf staging, best;         // flat parameters of the actor's dtype
  bool snapped = false;
  // greedy held-out evaluation (pdec_ledger_eval_attach)
  pdec_handle ev_env = 0, ev_actor = 0;
  int ev_K = 0, ev_R = 0, ev_dtype = PDEC_F32, ev_cap = 0, ev_par_dtype = PDEC_F32;
  DevBuf ev_ret, ev_blew;       // double [ev_cap][K], int32 [ev_cap][K]
  DevBuf ev_score, ev_ep;       // double [ev_cap], int64 [ev_cap]
  DevBuf ev_st;                 // LedgerState of the evaluation scores
  DevBuf ev_best;               // flat parameters of the evaluation actor's dtype
  bool staged = false;          // the staging buffer holds a snapshot (it survives the close that consumes `snapped`)
  Ledger() : Object(Kind::Ledger) {}
};

template <class T>
__global__ void ledger_step_kernel(const T* __restrict__ r, const int32_t* __restrict__ flags, int B, int R,
                                   double* __restrict__ ret, int32_t* __restrict__ blew) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int a = 0; a < R; ++a) s += (double)r[(size_t)b * R + a];
  ret[b] += s / (double)R;
  if (flags[b] != 0) blew[b] = 1;
}

// one workgroup.  snap_words: 32-bit words of the staging buffer copied to `best` when the episode is chosen (0: no tracking)
__global__ void ledger_close_kernel(double* __restrict__ ret, int32_t* __restrict__ blew, int B, double* __restrict__ rows_ret,
                                    int32_t* __restrict__ rows_blew, double* __restrict__ rows_mean, int row, LedgerState* st,
                                    long long ep1, int eligible, const uint32_t* __restrict__ staging, uint32_t* __restrict__ best,
                                    int snap_words) {
  __shared__ int choose;
  const int tid = threadIdx.x;
  for (int b = tid; b < B; b += blockDim.x) {
    rows_ret[(size_t)row * B + b] = ret[b];
    rows_blew[(size_t)row * B + b] = blew[b];
  }
  if (tid == 0) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += ret[b];
    const double mean = s / (double)B;
    rows_mean[row] = mean;
    int c = 0;
    // PDEhook.jl:66-71: an eligible episode whose value is >= every earlier eligible one becomes the best.  A NaN value is
    // never chosen and is left out of the comparison for later episodes (Julia's maximum would stay NaN from then on).
    if (snap_words > 0 && eligible && !isnan(mean)) {
      c = mean >= st->max_elig;
      if (c) {
        st->max_elig = mean;
        st->best_val = mean;
        st->best_ep = ep1;
      }
    }
    choose = c;
  }
  __syncthreads();
  if (choose)
    for (int i = tid; i < snap_words; i += blockDim.x) best[i] = staging[i];
  for (int b = tid; b < B; b += blockDim.x) {
    ret[b] = 0.0;
    blew[b] = 0;
  }
}

__global__ void ledger_zero_kernel(double* __restrict__ ret, int32_t* __restrict__ blew, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    ret[b] = 0.0;
    blew[b] = 0;
  }
}

// staging -> the evaluation actor's flat parameters (TS = TD: a copy; float -> double: an exact promotion)
template <class TS, class TD>
__global__ void ledger_eval_load_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (TD)src[i];
}

// one workgroup.  rsum [K][R], done_step [K]: the rollout's outputs; par -> best (par_words 32-bit words) when the evaluation is chosen
template <class T>
__global__ void ledger_eval_close_kernel(const T* __restrict__ rsum, const int32_t* __restrict__ done_step, int K, int R,
                                         double* __restrict__ rows_ret, int32_t* __restrict__ rows_blew,
                                         double* __restrict__ rows_score, long long* __restrict__ rows_ep, int row, LedgerState* st,
                                         long long ep1, int eligible, const uint32_t* __restrict__ par, uint32_t* __restrict__ best,
                                         int par_words) {
  __shared__ int choose;
  const int tid = threadIdx.x;
  double* ret = rows_ret + (size_t)row * K;
  int32_t* blew = rows_blew + (size_t)row * K;
  for (int b = tid; b < K; b += blockDim.x) {
    double s = 0.0;
    for (int a = 0; a < R; ++a) s += (double)rsum[(size_t)b * R + a];
    ret[b] = s / (double)R;
    blew[b] = done_step[b] >= 0 ? 1 : 0;
  }
  __syncthreads();      // (the row is this workgroup's own stores: visible to thread 0 behind the barrier)
  if (tid == 0) {
    double s = 0.0;
    int bad = 0;
    for (int b = 0; b < K; ++b) {
      s += ret[b];
      bad |= blew[b] != 0 || !isfinite(ret[b]);
    }
    const double score = bad ? (double)NAN : s / (double)K;
    rows_score[row] = score;
    rows_ep[row] = ep1;
    int c = 0;
    // the rule of ledger_close_kernel (PDEhook.jl:66-71) on the evaluation score
    if (eligible && !isnan(score)) {
      c = score >= st->max_elig;
      if (c) {
        st->max_elig = score;
        st->best_val = score;
        st->best_ep = ep1;
      }
    }
    choose = c;
  }
  __syncthreads();
  if (choose)
    for (int i = tid; i < par_words; i += blockDim.x) best[i] = par[i];
}

static Ledger* get_ledger(pdec_handle h, const char* fn, Env** E) {
  Ledger* L = lookup_as<Ledger>(h, Kind::Ledger);
  if (!L) {
    set_error("%s: not a ledger handle", fn);
    return nullptr;
  }
  if (E) {
    *E = lookup_as<Env>(L->env, Kind::Env);
    if (!*E) {
      set_error("%s: the ledger's environment has been destroyed", fn);
      return nullptr;
    }
  }
  return L;
}

// n flat parameters of dtype src_dtype (device) into D's parameters; differing dtypes: a host round trip, the values converted
// exactly as pdec_mlp_set_params converts (float <-> double casts).  The caller has drained the streams involved.
static int copy_params_converted(Mlp* D, const void* src, int src_dtype, size_t n) {
  if (D->dtype == src_dtype) {
    PDEC_HIP(hipMemcpy(D->params.p, src, n * dtype_size(D->dtype), hipMemcpyDeviceToDevice));
  } else {
    std::vector<double> h(n);
    std::vector<float> f(n);
    if (src_dtype == PDEC_F32) {
      PDEC_HIP(hipMemcpy(f.data(), src, n * 4, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) h[i] = f[i];
      PDEC_HIP(hipMemcpy(D->params.p, h.data(), n * 8, hipMemcpyHostToDevice));
    } else {
      PDEC_HIP(hipMemcpy(h.data(), src, n * 8, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) f[i] = (float)h[i];
      PDEC_HIP(hipMemcpy(D->params.p, f.data(), n * 4, hipMemcpyHostToDevice));
    }
  }
  return PDEC_OK;
}

}  // namespace pdec

using namespace pdec;

extern "C" {

int pdec_ledger_create(pdec_handle* out, pdec_handle env, pdec_handle actor, int capacity) {
  PDEC_REQUIRE(out && capacity >= 1, "pdec_ledger_create: null handle or capacity %d < 1", capacity);
  Env* E = lookup_as<Env>(env, Kind::Env);
  if (!E) { set_error("pdec_ledger_create: bad environment handle"); return PDEC_E_HANDLE; }
  auto L = std::make_unique<Ledger>();
  const pdec_env_cfg& c = E->cfg;
  L->env = env; L->B = c.B; L->R = c.mono ? 1 : c.A; L->env_dtype = c.dtype; L->cap = capacity;
  L->stream = E->stream;
  if (actor) {
    Mlp* M = lookup_as<Mlp>(actor, Kind::Mlp);
    if (!M) { set_error("pdec_ledger_create: bad actor handle"); return PDEC_E_HANDLE; }
    L->actor = actor; L->nparams = M->nparams; L->par_dtype = M->dtype; L->dims = M->dims;
    const size_t pb = (size_t)M->nparams * dtype_size(M->dtype);
    PDEC_HIP(L->staging.alloc(pb));
    PDEC_HIP(L->best.alloc(pb));
    PDEC_HIP(hipMemset(L->staging.p, 0, pb));
    PDEC_HIP(hipMemset(L->best.p, 0, pb));
  }
  const size_t B = (size_t)L->B, cap = (size_t)capacity;
  PDEC_HIP(L->run_ret.alloc(B * sizeof(double)));
  PDEC_HIP(L->run_blew.alloc(B * sizeof(int32_t)));
  PDEC_HIP(L->rows_ret.alloc(cap * B * sizeof(double)));
  PDEC_HIP(L->rows_blew.alloc(cap * B * sizeof(int32_t)));
  PDEC_HIP(L->rows_mean.alloc(cap * sizeof(double)));
  PDEC_HIP(L->st.alloc(sizeof(LedgerState)));
  PDEC_HIP(hipMemset(L->run_ret.p, 0, B * sizeof(double)));
  PDEC_HIP(hipMemset(L->run_blew.p, 0, B * sizeof(int32_t)));
  PDEC_HIP(hipMemset(L->rows_ret.p, 0, cap * B * sizeof(double)));
  PDEC_HIP(hipMemset(L->rows_blew.p, 0, cap * B * sizeof(int32_t)));
  PDEC_HIP(hipMemset(L->rows_mean.p, 0, cap * sizeof(double)));
  const LedgerState s0{-1000000.0, -INFINITY, 0, 0};
  PDEC_HIP(hipMemcpy(L->st.p, &s0, sizeof(s0), hipMemcpyHostToDevice));     // (blocking: ordered before every later launch)
  PDEC_HIP(hipDeviceSynchronize());
  *out = register_object(std::move(L));
  return PDEC_OK;
}

int pdec_ledger_step(pdec_handle ledger, const void* reward, const int32_t* flags) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_step", &E);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(reward && flags, "pdec_ledger_step: null argument");
  const dim3 grid((L->B + 255) / 256), block(256);
  if (L->env_dtype == PDEC_F64)
    hipLaunchKernelGGL(ledger_step_kernel<double>, grid, block, 0, E->stream, (const double*)reward, flags, L->B, L->R,
                       L->run_ret.as<double>(), L->run_blew.as<int32_t>());
  else
    hipLaunchKernelGGL(ledger_step_kernel<float>, grid, block, 0, E->stream, (const float*)reward, flags, L->B, L->R,
                       L->run_ret.as<double>(), L->run_blew.as<int32_t>());
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_ledger_snapshot(pdec_handle ledger) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_snapshot", &E);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(L->actor, "pdec_ledger_snapshot: the ledger was made without an actor");
  Mlp* M = lookup_as<Mlp>(L->actor, Kind::Mlp);
  if (!M) { set_error("pdec_ledger_snapshot: the actor has been destroyed"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(M->dims == L->dims && M->dtype == L->par_dtype, "pdec_ledger_snapshot: the actor changed shape");
  int yes = 0;
  int rc = pdec_mlp_acts_on_published_copy(L->actor, &yes);
  if (rc) return rc;
  if (yes) {
    // the fused 3-layer acting kernel read the published image fw_pub[pub]: unpack it (the flat parameters may already be
    // rewritten by the update running beside it on the other stream)
    rc = fused_unpack_published(M, L->staging.as<float>(), E->stream);
    if (rc) return rc;
  } else {
    // 2-layer / generic nets act on the flat parameters in place; the update's actor half waits for the acting kernel's
    // event, which the caller records behind this copy
    PDEC_HIP(hipMemcpyAsync(L->staging.p, M->params.p, (size_t)L->nparams * dtype_size(L->par_dtype), hipMemcpyDeviceToDevice,
                            E->stream));
  }
  L->snapped = true;
  L->staged = true;
  return PDEC_OK;
}

int pdec_ledger_close(pdec_handle ledger, int64_t episode, int64_t min_best_episode, int track_best) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_close", &E);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(episode >= 0, "pdec_ledger_close: episode %lld < 0", (long long)episode);
  int words = 0;
  if (track_best) {
    PDEC_REQUIRE(L->actor, "pdec_ledger_close: best tracking needs a ledger made with an actor");
    PDEC_REQUIRE(L->snapped, "pdec_ledger_close: no pdec_ledger_snapshot since the last close");
    words = (int)((size_t)L->nparams * dtype_size(L->par_dtype) / 4);
  }
  const int row = (int)(episode % L->cap);
  const int eligible = episode + 1 >= min_best_episode;
  hipLaunchKernelGGL(ledger_close_kernel, dim3(1), dim3(256), 0, E->stream, L->run_ret.as<double>(), L->run_blew.as<int32_t>(),
                     L->B, L->rows_ret.as<double>(), L->rows_blew.as<int32_t>(), L->rows_mean.as<double>(), row,
                     L->st.as<LedgerState>(), (long long)episode + 1, eligible, L->staging.as<uint32_t>(), L->best.as<uint32_t>(),
                     words);
  PDEC_HIP(hipGetLastError());
  L->snapped = false;
  return PDEC_OK;
}

int pdec_ledger_discard(pdec_handle ledger) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_discard", &E);
  if (!L) return PDEC_E_HANDLE;
  hipLaunchKernelGGL(ledger_zero_kernel, dim3((L->B + 255) / 256), dim3(256), 0, E->stream, L->run_ret.as<double>(),
                     L->run_blew.as<int32_t>(), L->B);
  PDEC_HIP(hipGetLastError());
  L->snapped = false;
  return PDEC_OK;
}

int pdec_ledger_read(pdec_handle ledger, double* returns, int32_t* blew_up, double* means) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_read", &E);
  if (!L) return PDEC_E_HANDLE;
  PDEC_HIP(hipStreamSynchronize(E->stream));
  const size_t n = (size_t)L->cap * L->B;
  if (returns) PDEC_HIP(hipMemcpy(returns, L->rows_ret.p, n * sizeof(double), hipMemcpyDeviceToHost));
  if (blew_up) PDEC_HIP(hipMemcpy(blew_up, L->rows_blew.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (means) PDEC_HIP(hipMemcpy(means, L->rows_mean.p, (size_t)L->cap * sizeof(double), hipMemcpyDeviceToHost));
  return PDEC_OK;
}

int pdec_ledger_best(pdec_handle ledger, double* value, int64_t* episode) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_best", &E);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(value && episode, "pdec_ledger_best: null");
  PDEC_HIP(hipStreamSynchronize(E->stream));
  LedgerState s;
  PDEC_HIP(hipMemcpy(&s, L->st.p, sizeof(s), hipMemcpyDeviceToHost));
  *value = s.best_val;
  *episode = s.best_ep;
  return PDEC_OK;
}

int pdec_ledger_best_params(pdec_handle ledger, pdec_handle mlp) {
  Env* E = nullptr;
  Ledger* L = get_ledger(ledger, "pdec_ledger_best_params", &E);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(L->actor, "pdec_ledger_best_params: the ledger was made without an actor");
  Mlp* D = lookup_as<Mlp>(mlp, Kind::Mlp);
  if (!D) { set_error("pdec_ledger_best_params: not an mlp handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(D->dims == L->dims, "pdec_ledger_best_params: the destination's layer sizes differ from the actor's");
  PDEC_HIP(hipStreamSynchronize(E->stream));
  PDEC_HIP(hipStreamSynchronize(D->stream));
  const int rc = copy_params_converted(D, L->best.p, L->par_dtype, (size_t)L->nparams);
  if (rc) return rc;
  D->fw_dirty = true;
  return PDEC_OK;
}

// ---- greedy held-out evaluation
static Ledger* get_eval(pdec_handle h, const char* fn, Env** EE, Mlp** EA) {
  Ledger* L = get_ledger(h, fn, nullptr);
  if (!L) return nullptr;
  if (!L->ev_env) {
    set_error("%s: no evaluation is attached to the ledger (pdec_ledger_eval_attach)", fn);
    return nullptr;
  }
  *EE = lookup_as<Env>(L->ev_env, Kind::Env);
  Mlp* A = lookup_as<Mlp>(L->ev_actor, Kind::Mlp);
  if (!*EE || !A) {
    set_error("%s: the evaluation environment or actor has been destroyed", fn);
    return nullptr;
  }
  if (EA) *EA = A;
  return L;
}

int pdec_ledger_eval_attach(pdec_handle ledger, pdec_handle eval_env, pdec_handle eval_actor, int capacity) {
  Ledger* L = get_ledger(ledger, "pdec_ledger_eval_attach", nullptr);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(capacity >= 1, "pdec_ledger_eval_attach: capacity %d < 1", capacity);
  PDEC_REQUIRE(L->actor, "pdec_ledger_eval_attach: the ledger was made without an actor (the evaluation rolls out its snapshot)");
  PDEC_REQUIRE(!L->ev_env, "pdec_ledger_eval_attach: an evaluation is already attached");
  Env* EE = lookup_as<Env>(eval_env, Kind::Env);
  Mlp* EA = lookup_as<Mlp>(eval_actor, Kind::Mlp);
  if (!EE || !EA) { set_error("pdec_ledger_eval_attach: bad environment or actor handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(eval_env != L->env && eval_actor != L->actor, "pdec_ledger_eval_attach: the evaluation needs an environment and an actor of its own");
  PDEC_REQUIRE(EA->dims == L->dims, "pdec_ledger_eval_attach: the evaluation actor's layer sizes differ from the actor's");
  PDEC_REQUIRE(EA->dtype == L->par_dtype || EA->dtype == PDEC_F64,
               "pdec_ledger_eval_attach: the staged parameters do not promote exactly to the evaluation actor's dtype");
  const pdec_env_cfg& c = EE->cfg;
  const size_t K = (size_t)c.B, cap = (size_t)capacity;
  const size_t pb = (size_t)L->nparams * dtype_size(EA->dtype);
  PDEC_HIP(L->ev_ret.alloc(cap * K * sizeof(double)));
  PDEC_HIP(L->ev_blew.alloc(cap * K * sizeof(int32_t)));
  PDEC_HIP(L->ev_score.alloc(cap * sizeof(double)));
  PDEC_HIP(L->ev_ep.alloc(cap * sizeof(long long)));
  PDEC_HIP(L->ev_st.alloc(sizeof(LedgerState)));
  PDEC_HIP(L->ev_best.alloc(pb));
  PDEC_HIP(hipMemset(L->ev_ret.p, 0, cap * K * sizeof(double)));
  PDEC_HIP(hipMemset(L->ev_blew.p, 0, cap * K * sizeof(int32_t)));
  PDEC_HIP(hipMemset(L->ev_score.p, 0, cap * sizeof(double)));
  PDEC_HIP(hipMemset(L->ev_ep.p, 0, cap * sizeof(long long)));
  PDEC_HIP(hipMemset(L->ev_best.p, 0, pb));
  const LedgerState s0{-1000000.0, -INFINITY, 0, 0};
  PDEC_HIP(hipMemcpy(L->ev_st.p, &s0, sizeof(s0), hipMemcpyHostToDevice));
  PDEC_HIP(hipDeviceSynchronize());
  L->ev_env = eval_env; L->ev_actor = eval_actor;
  L->ev_K = c.B; L->ev_R = c.mono ? 1 : c.A; L->ev_dtype = c.dtype; L->ev_cap = capacity; L->ev_par_dtype = EA->dtype;
  return PDEC_OK;
}

int pdec_ledger_eval_load(pdec_handle ledger) {
  Env* E = nullptr;
  Env* EE = nullptr;
  Mlp* EA = nullptr;
  if (!get_ledger(ledger, "pdec_ledger_eval_load", &E)) return PDEC_E_HANDLE;
  Ledger* L = get_eval(ledger, "pdec_ledger_eval_load", &EE, &EA);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(L->staged, "pdec_ledger_eval_load: no pdec_ledger_snapshot yet");
  PDEC_REQUIRE(EA->dims == L->dims && EA->dtype == L->ev_par_dtype && EA->nparams == L->nparams,
               "pdec_ledger_eval_load: the evaluation actor changed shape");
  const int n = L->nparams;
  const dim3 grid((n + 255) / 256), block(256);
  if (L->par_dtype == PDEC_F32 && L->ev_par_dtype == PDEC_F64)
    hipLaunchKernelGGL((ledger_eval_load_kernel<float, double>), grid, block, 0, E->stream, L->staging.as<float>(), EA->params.as<double>(), n);
  else if (L->par_dtype == PDEC_F32)
    hipLaunchKernelGGL((ledger_eval_load_kernel<float, float>), grid, block, 0, E->stream, L->staging.as<float>(), EA->params.as<float>(), n);
  else
    hipLaunchKernelGGL((ledger_eval_load_kernel<double, double>), grid, block, 0, E->stream, L->staging.as<double>(), EA->params.as<double>(), n);
  PDEC_HIP(hipGetLastError());
  EA->fw_dirty = true;      // the padded image of a fused 3-layer actor: rebuilt by its next acting call, on its own stream
  return PDEC_OK;
}

int pdec_ledger_eval_close(pdec_handle ledger, const void* reward_sum, const int32_t* done_step, int64_t n_eval, int64_t episode,
                           int64_t min_best_episode) {
  Env* EE = nullptr;
  Mlp* EA = nullptr;
  Ledger* L = get_eval(ledger, "pdec_ledger_eval_close", &EE, &EA);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(reward_sum && done_step && n_eval >= 0 && episode >= 1, "pdec_ledger_eval_close: null argument, n_eval < 0 or episode < 1");
  PDEC_REQUIRE(EA->dtype == L->ev_par_dtype && EA->nparams == L->nparams, "pdec_ledger_eval_close: the evaluation actor changed shape");
  const int row = (int)(n_eval % L->ev_cap);
  const int eligible = episode >= min_best_episode;
  const int words = (int)((size_t)L->nparams * dtype_size(L->ev_par_dtype) / 4);
  by_dtype(L->ev_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ledger_eval_close_kernel<T>, dim3(1), dim3(256), 0, EE->stream, (const T*)reward_sum, done_step, L->ev_K, L->ev_R,
                       L->ev_ret.as<double>(), L->ev_blew.as<int32_t>(), L->ev_score.as<double>(), L->ev_ep.as<long long>(), row,
                       L->ev_st.as<LedgerState>(), (long long)episode, eligible, EA->params.as<uint32_t>(), L->ev_best.as<uint32_t>(),
                       words);
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_ledger_eval_read(pdec_handle ledger, int64_t* episodes, double* returns, int32_t* blew_up, double* scores) {
  Env* EE = nullptr;
  Ledger* L = get_eval(ledger, "pdec_ledger_eval_read", &EE, nullptr);
  if (!L) return PDEC_E_HANDLE;
  PDEC_HIP(hipStreamSynchronize(EE->stream));
  const size_t cap = (size_t)L->ev_cap, n = cap * L->ev_K;
  if (episodes) PDEC_HIP(hipMemcpy(episodes, L->ev_ep.p, cap * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (returns) PDEC_HIP(hipMemcpy(returns, L->ev_ret.p, n * sizeof(double), hipMemcpyDeviceToHost));
  if (blew_up) PDEC_HIP(hipMemcpy(blew_up, L->ev_blew.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (scores) PDEC_HIP(hipMemcpy(scores, L->ev_score.p, cap * sizeof(double), hipMemcpyDeviceToHost));
  return PDEC_OK;
}

int pdec_ledger_eval_best(pdec_handle ledger, double* value, int64_t* episode) {
  Env* EE = nullptr;
  Ledger* L = get_eval(ledger, "pdec_ledger_eval_best", &EE, nullptr);
  if (!L) return PDEC_E_HANDLE;
  PDEC_REQUIRE(value && episode, "pdec_ledger_eval_best: null");
  PDEC_HIP(hipStreamSynchronize(EE->stream));
  LedgerState s;
  PDEC_HIP(hipMemcpy(&s, L->ev_st.p, sizeof(s), hipMemcpyDeviceToHost));
  *value = s.best_val;
  *episode = s.best_ep;
  return PDEC_OK;
}

int pdec_ledger_eval_best_params(pdec_handle ledger, pdec_handle mlp) {
  Env* EE = nullptr;
  Ledger* L = get_eval(ledger, "pdec_ledger_eval_best_params", &EE, nullptr);
  if (!L) return PDEC_E_HANDLE;
  Mlp* D = lookup_as<Mlp>(mlp, Kind::Mlp);
  if (!D) { set_error("pdec_ledger_eval_best_params: not an mlp handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(D->dims == L->dims, "pdec_ledger_eval_best_params: the destination's layer sizes differ from the actor's");
  PDEC_HIP(hipStreamSynchronize(EE->stream));
  PDEC_HIP(hipStreamSynchronize(D->stream));
  const int rc = copy_params_converted(D, L->ev_best.p, L->ev_par_dtype, (size_t)L->nparams);
  if (rc) return rc;
  D->fw_dirty = true;
  return PDEC_OK;
}

}  // extern "C"
