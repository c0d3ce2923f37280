// nstep.hip -- n-step transitions of the batched training pipeline, assembled on the device.
//
// The pipeline's update of step k trains on one-step transitions (s_j, a_j, r_j, t_j, s_{j+1}) taken straight from its ring
// slots.  This object keeps the last n steps' rows -- state [cols][ns], action [cols][na], reward [cols], terminal [cols], in the
// ring slots' own layouts -- and one launch behind env step k emits, per column c, the transition that STARTS at step
// u = k - n + 1:
//   m        = the smallest i in [0, n-1] with t_{u+i}[c] != 0, or n - 1 if there is none
//   R[c]     = sum_{i=0..m} w_i r_{u+i}[c],  w_0 = 1, w_{i+1} = w_i gamma, in double, index order, no FMA contraction, rounded
//              once to the buffers' dtype
//   T[c]     = 1 if t_{u+m}[c] != 0 else 0
//   state    = s_in_u[c],  action = a_u[c]
// (next_state is the slot the one-step batch reads already: s_out_k.)  A window cut by a terminal has T = 1 and never bootstraps;
// every window that does bootstrap is full, so the update takes the one scalar gamma_n = w_n for all columns.
//
// One launch, one thread per element, coalesced along the columns: thread g stores element g of step k's state / action row into
// ring slot p = pos mod n and copies element g of the OLDEST slot (p + 1) mod n -- step u's -- to the output (n = 1: the input
// itself); threads g < cols store the reward / terminal of column g and walk the n - 1 older slots of that column, oldest first
// (n scalar loads per ring; the newest value is the thread's own input).  Slot p is written and slot (p + 1) mod n .. are read:
// no element is read by a thread other than the one that wrote it in this launch.
//
// The ring position lives on the device as a two-slot ping-pong, the way the acting kernel's noise counter does: a launch reads
// pos[sel] (every thread) and thread 0 writes pos[sel ^ 1] = pos + 1, a slot nobody reads in this launch; the host flips `sel`
// per call (flip(): replayed by pdec_graph_launch).  So the call's arguments are a function of the call's parity only and a
// recorded step / a captured chunk holds it.
#include "env.hpp"

namespace pdec {

#define NSTEP_MAX 32
#define NSTEP_THREADS 256

struct NStep : Object {
  int n = 1, cols = 0, ns = 0, na = 0, dtype = PDEC_F32;
  DevBuf S, A, R, T;         // [n][cols ns], [n][cols na], [n][cols], [n][cols]
  DevBuf pos;                // long long [2]
  int sel = 0;
  NStep() : Object(Kind::NStep) {}
};

template <class T>
struct NStepArgs {
  const T *s_in, *a_in, *r_in, *t_in;
  T *s_out, *a_out, *r_out, *t_out;
  T *S, *A, *R, *Tm;
  const long long* pos_in;
  long long* pos_out;
  double gamma;
  int n, cols, nS, nA;       // nS = cols ns, nA = cols na
};

// R and T of one column: rows oldest first, the newest (i = n - 1) is (r_new, t_new)
template <class T>
__device__ __forceinline__ void nstep_accumulate(const NStepArgs<T>& g, int c, int p, T r_new, T t_new, T* r_out, T* t_out) {
#pragma clang fp contract(off)
  double w = 1.0, acc = 0.0;
  T term = (T)0;
  int slot = p + 1 == g.n ? 0 : p + 1;
  for (int i = 0; i < g.n; ++i) {
    const bool newest = i == g.n - 1;
    const T r = newest ? r_new : g.R[(size_t)slot * g.cols + c];
    const T t = newest ? t_new : g.Tm[(size_t)slot * g.cols + c];
    const double wr = w * (double)r;
    acc = acc + wr;
    w = w * g.gamma;
    if (t != (T)0) {
      term = (T)1;
      break;
    }
    slot = slot + 1 == g.n ? 0 : slot + 1;
  }
  *r_out = (T)acc;
  *t_out = term;
}

template <class T>
__global__ void __launch_bounds__(NSTEP_THREADS) nstep_kernel(NStepArgs<T> g) {
  const int gid = blockIdx.x * NSTEP_THREADS + threadIdx.x;
  const long long pos = *g.pos_in;
  const int p = (int)(pos % g.n), old = p + 1 == g.n ? 0 : p + 1;
  if (gid < g.nS) {
    const T v = g.s_in[gid];
    g.S[(size_t)p * g.nS + gid] = v;
    g.s_out[gid] = g.n == 1 ? v : g.S[(size_t)old * g.nS + gid];
  }
  if (gid < g.nA) {
    const T v = g.a_in[gid];
    g.A[(size_t)p * g.nA + gid] = v;
    g.a_out[gid] = g.n == 1 ? v : g.A[(size_t)old * g.nA + gid];
  }
  if (gid < g.cols) {
    const T r = g.r_in[gid], t = g.t_in[gid];
    g.R[(size_t)p * g.cols + gid] = r;
    g.Tm[(size_t)p * g.cols + gid] = t;
    nstep_accumulate<T>(g, gid, p, r, t, g.r_out + gid, g.t_out + gid);
  }
  if (gid == 0) *g.pos_out = pos + 1;
}

static NStep* get_nstep(pdec_handle h, const char* fn) {
  NStep* N = lookup_as<NStep>(h, Kind::NStep);
  if (!N) set_error("%s: not an n-step handle", fn);
  return N;
}

}  // namespace pdec

using namespace pdec;

extern "C" {

int pdec_nstep_create(pdec_handle* out, int n_step, int cols, int ns, int na, int dtype) {
  PDEC_REQUIRE(out, "pdec_nstep_create: null handle");
  PDEC_REQUIRE(n_step >= 1 && n_step <= NSTEP_MAX, "pdec_nstep_create: n_step %d outside 1 .. %d", n_step, NSTEP_MAX);
  PDEC_REQUIRE(dtype == PDEC_F32 || dtype == PDEC_F64, "pdec_nstep_create: dtype %d", dtype);
  PDEC_REQUIRE(cols >= 1 && ns >= 1 && na >= 1, "pdec_nstep_create: cols %d, ns %d, na %d", cols, ns, na);
  const long long most = (long long)cols * (ns > na ? ns : na);
  PDEC_REQUIRE(most <= INT32_MAX - NSTEP_THREADS, "pdec_nstep_create: %lld elements per row exceed the kernel's 32-bit index", most);
  auto N = std::make_unique<NStep>();
  N->n = n_step; N->cols = cols; N->ns = ns; N->na = na; N->dtype = dtype;
  const size_t e = dtype_size(dtype), n = (size_t)n_step, c = (size_t)cols;
  DevBuf* bufs[] = {&N->S, &N->A, &N->R, &N->T, &N->pos};
  const size_t bytes[] = {n * c * ns * e, n * c * na * e, n * c * e, n * c * e, 2 * sizeof(long long)};
  for (int i = 0; i < 5; ++i) {
    PDEC_HIP(bufs[i]->alloc(bytes[i]));
    PDEC_HIP(hipMemset(bufs[i]->p, 0, bytes[i]));
  }
  PDEC_HIP(hipDeviceSynchronize());
  *out = register_object(std::move(N));
  return PDEC_OK;
}

int pdec_nstep_step(pdec_handle nstep, const void* s_in, const void* action, const void* reward, const void* terminal, double gamma,
                    void* state_out, void* action_out, void* reward_out, void* terminal_out) {
  NStep* N = get_nstep(nstep, "pdec_nstep_step");
  if (!N) return PDEC_E_HANDLE;
  PDEC_REQUIRE(s_in && action && reward && terminal && state_out && action_out && reward_out && terminal_out,
               "pdec_nstep_step: null argument");
  ProfScope ps(N, "nstep_step");
  const int nS = N->cols * N->ns, nA = N->cols * N->na;
  const int most = nS > nA ? nS : nA;      // (>= cols: ns, na >= 1)
  by_dtype(N->dtype, [&](auto t) {
    using T = decltype(t);
    NStepArgs<T> g{};
    g.s_in = (const T*)s_in; g.a_in = (const T*)action; g.r_in = (const T*)reward; g.t_in = (const T*)terminal;
    g.s_out = (T*)state_out; g.a_out = (T*)action_out; g.r_out = (T*)reward_out; g.t_out = (T*)terminal_out;
    g.S = N->S.as<T>(); g.A = N->A.as<T>(); g.R = N->R.as<T>(); g.Tm = N->T.as<T>();
    g.pos_in = N->pos.as<long long>() + N->sel; g.pos_out = N->pos.as<long long>() + (N->sel ^ 1);
    g.gamma = gamma; g.n = N->n; g.cols = N->cols; g.nS = nS; g.nA = nA;
    hipLaunchKernelGGL(nstep_kernel<T>, dim3((most + NSTEP_THREADS - 1) / NSTEP_THREADS), dim3(NSTEP_THREADS), 0, N->stream, g);
  });
  PDEC_HIP(hipGetLastError());
  flip(N->sel);
  return PDEC_OK;
}

int pdec_nstep_read(pdec_handle nstep, int64_t* position, void* states, void* actions, void* rewards, void* terminals) {
  NStep* N = get_nstep(nstep, "pdec_nstep_read");
  if (!N) return PDEC_E_HANDLE;
  PDEC_HIP(hipStreamSynchronize(N->stream));
  const size_t e = dtype_size(N->dtype), n = (size_t)N->n, c = (size_t)N->cols;
  if (position) PDEC_HIP(hipMemcpy(position, N->pos.as<long long>() + N->sel, sizeof(int64_t), hipMemcpyDeviceToHost));
  if (states) PDEC_HIP(hipMemcpy(states, N->S.p, n * c * N->ns * e, hipMemcpyDeviceToHost));
  if (actions) PDEC_HIP(hipMemcpy(actions, N->A.p, n * c * N->na * e, hipMemcpyDeviceToHost));
  if (rewards) PDEC_HIP(hipMemcpy(rewards, N->R.p, n * c * e, hipMemcpyDeviceToHost));
  if (terminals) PDEC_HIP(hipMemcpy(terminals, N->T.p, n * c * e, hipMemcpyDeviceToHost));
  return PDEC_OK;
}

}  // extern "C"
