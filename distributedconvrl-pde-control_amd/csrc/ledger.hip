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
  const size_t n = (size_t)L->nparams;
  if (D->dtype == L->par_dtype) {
    PDEC_HIP(hipMemcpy(D->params.p, L->best.p, n * dtype_size(D->dtype), hipMemcpyDeviceToDevice));
  } else {
    // a host round trip: the values are converted exactly as pdec_mlp_set_params converts (float <-> double casts)
    std::vector<double> h(n);
    if (L->par_dtype == PDEC_F32) {
      std::vector<float> f(n);
      PDEC_HIP(hipMemcpy(f.data(), L->best.p, n * 4, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) h[i] = f[i];
      PDEC_HIP(hipMemcpy(D->params.p, h.data(), n * 8, hipMemcpyHostToDevice));
    } else {
      PDEC_HIP(hipMemcpy(h.data(), L->best.p, n * 8, hipMemcpyDeviceToHost));
      std::vector<float> f(n);
      for (size_t i = 0; i < n; ++i) f[i] = (float)h[i];
      PDEC_HIP(hipMemcpy(D->params.p, f.data(), n * 4, hipMemcpyHostToDevice));
    }
  }
  D->fw_dirty = true;
  return PDEC_OK;
}

}  // extern "C"
