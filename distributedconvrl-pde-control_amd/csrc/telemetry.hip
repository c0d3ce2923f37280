// telemetry.hip -- per-step facts of a training run, reduced and kept on the device.
//
// The batched training pipeline reports returns; what a run does inside -- the losses, how much of the batch sits on the action
// limit, how far the parameters move and the targets trail, when the first NaN appeared -- could be seen only by draining the
// streams every step.  This object keeps two rings of `capacity` rows of doubles and one launch per ring writes a row:
//   pdec_telemetry_step    (the object's stream: the env stream), behind everything that writes the rows of control step k:
//       step | reward_mean reward_min reward_max reward_nonfinite | action_mean action_abs_mean action_saturated |
//       state_abs_max state_nonfinite | blown_up | terminal                                                     (12 columns)
//   pdec_telemetry_update  (the critic's stream: the update stream), behind the last launch of the update:
//       update | critic_loss actor_loss | actor_norm2 critic_norm2 | actor_target_dist2 critic_target_dist2 |
//       actor_step2 critic_step2 | actor_abs_max critic_abs_max | actor_nonfinite critic_nonfinite               (13 columns)
// and a sticky pair (first_nonfinite_step, first_nonfinite_update), -1 until a row shows a non-finite value.
//
// Arithmetic: every input is promoted to double (exact), squares and sums are formed in double without FMA contraction, counts
// are doubles.  An entry that is not finite is left out of the sums and maxima and counted (a difference is left out when either
// of its two entries is not finite).
//
// Reduction: workgroup b of 256 threads owns the elements [b CHUNK, (b + 1) CHUNK); thread t takes t, t + 256, ... of them in index
// order, the wave combines by a fixed shuffle tree (offsets 32, 16, .., 1), thread 0 combines the four waves in wave order and
// stores the workgroup's partials.  The workgroup that draws the last ticket combines the partials: thread t takes workgroups t,
// t + 256, ... in index order, then the same tree.  Every order is a function of the shapes alone -- never of which workgroup
// arrives first -- and there is no floating-point atomic, so two runs of one program give bit-equal rows.  The hand-over is the
// counter form with written-through partials: agent-scope stores, a wait for them, a relaxed agent-scope ticket add; the last
// arriver reads every partial with agent-scope loads (the workgroups may sit on different XCDs, whose L2s are not coherent with
// each other).  The last arriver zeroes the ticket for the next launch.
//
// The row counters live on the device and are read and advanced by ONE thread -- thread 0 of the combining workgroup, the only
// reader of anything the launch's other workgroups wrote -- so they need no second slot and no host-side selector: the arguments
// of a call are the same at every step, and a recorded step or a captured chunk carries it whatever the number of calls it holds
// (with telemetry_every = 2 or 6 a six-step chunk holds an odd number of update calls, which a two-slot counter whose selector is
// baked into the graph would not survive).
#include <cmath>

#include "env.hpp"
#include "mlp.hpp"

namespace pdec {

#define TEL_THREADS 256
#define TEL_WAVES (TEL_THREADS / 64)
#define TEL_STEP_CHUNK 1024      // elements of one workgroup of the step launch
#define TEL_UPD_CHUNK 4096       // parameters of one workgroup of the update launch
#define TEL_STEP_COLS 12
#define TEL_UPD_COLS 13

enum { TEL_SUM = 0, TEL_MIN = 1, TEL_MAX = 2 };

// partials of one workgroup of the step launch
enum { TS_RSUM, TS_RMIN, TS_RMAX, TS_RNF, TS_ASUM, TS_AABS, TS_ASAT, TS_SMAX, TS_SNF, TS_BLOWN, TS_TERM, TS_K };
struct StepOps {
  static constexpr int K = TS_K;
  __device__ static constexpr int of(int k) { return k == TS_RMIN ? TEL_MIN : (k == TS_RMAX || k == TS_SMAX) ? TEL_MAX : TEL_SUM; }
  __device__ static constexpr double identity(int k) { return k == TS_RMIN ? INFINITY : k == TS_RMAX ? -INFINITY : 0.0; }
};
// partials of one workgroup of the update launch (one network), and the pair (actor, critic) the last arriver combines
enum { TU_NORM2, TU_TDIST2, TU_STEP2, TU_AMAX, TU_NF, TU_K };
template <int NETS>
struct UpdOps {          // (the identity of both operations is 0: |x| >= 0)
  static constexpr int K = NETS * TU_K;
  __device__ static constexpr int of(int k) { return k % TU_K == TU_AMAX ? TEL_MAX : TEL_SUM; }
};

struct Telemetry : Object {
  int cap = 0, B = 0, cols = 0, ns = 0, na = 0, env_dtype = PDEC_F32, par_dtype = PDEC_F32;
  int nA = 0, nC = 0;                 // flat parameters of the actor / the critic
  int nb_step = 0, nb_a = 0, nb_c = 0;
  hipStream_t upd_stream = nullptr;   // where the last pdec_telemetry_update ran
  DevBuf step_ring, upd_ring;         // double [cap][12], [cap][13]
  DevBuf step_part, upd_part;         // double [nb_step][TS_K], [nb_a + nb_c][TU_K]
  DevBuf prev_a, prev_c;              // the parameters at the previous update call, in their own dtype
  DevBuf ctl;                         // long long [4]: step calls, update calls, first_nonfinite_step, first_nonfinite_update
  DevBuf tickets;                     // unsigned [2]
  Telemetry() : Object(Kind::Telemetry) {}
  // pdec_destroy drains the object's own stream; an update launch still queued on the critic's stream reads the buffers freed here
  ~Telemetry() override {
    if (upd_stream != stream) (void)hipStreamSynchronize(upd_stream);
  }
};

__device__ __forceinline__ double tel_comb(int op, double a, double b) {
#pragma clang fp contract(off)
  return op == TEL_SUM ? a + b : op == TEL_MIN ? fmin(a, b) : fmax(a, b);
}

// v[k] of thread 0 <- the workgroup's combination, by the fixed tree.  lds: TEL_WAVES * K doubles.
template <class Ops>
__device__ __forceinline__ void tel_block_reduce(double (&v)[Ops::K], double* lds) {
  constexpr int K = Ops::K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
    for (int off = 32; off > 0; off >>= 1) x = tel_comb(Ops::of(k), x, __shfl_down(x, off, 64));
    if (lane == 0) lds[wave * K + k] = x;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double x = lds[k];
      for (int w = 1; w < TEL_WAVES; ++w) x = tel_comb(Ops::of(k), x, lds[w * K + k]);
      v[k] = x;
    }
  }
  __syncthreads();
}

// The partials cross workgroups -- possibly XCDs, whose L2s are not coherent with each other -- through agent-scope accesses
// only: written through by tel_store, read past the L2 by tel_load (every load of them).  That needs no release / acquire fence
// pair, i.e. no write-back and no invalidation of a whole L2 under the update passes that run next.
__device__ __forceinline__ void tel_store(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double tel_load(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Thread 0 has stored this workgroup's partials with tel_store: wait until they have left, then draw a ticket.  True in every
// thread of the workgroup that drew the last one (a launch of one workgroup draws none).  flag: one LDS word of the launch's array.
__device__ __forceinline__ bool tel_last_arriver(unsigned* ticket, double* flag) {
  if (gridDim.x == 1) return true;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = t == gridDim.x - 1 ? 1.0 : 0.0;
  }
  __syncthreads();
  return *flag != 0.0;
}

template <class T>
struct TelStepArgs {
  const T *s, *a, *r, *t;
  const int32_t* flags;
  double limit;
  int nS, cols, na, B, cap;
  double *part, *ring;
  unsigned* ticket;
  long long* ctl;
};

template <class T>
__global__ void __launch_bounds__(TEL_THREADS) telemetry_step_kernel(TelStepArgs<T> g) {
#pragma clang fp contract(off)
  __shared__ double lds[TEL_WAVES * TS_K + 1];
  const int tid = threadIdx.x, nb = (int)gridDim.x;
  double v[TS_K];
#pragma unroll
  for (int k = 0; k < TS_K; ++k) v[k] = StepOps::identity(k);
  const int base = blockIdx.x * TEL_STEP_CHUNK;
  for (int q = 0; q < TEL_STEP_CHUNK / TEL_THREADS; ++q) {
    const int i = base + q * TEL_THREADS + tid;
    if (i < g.nS) {
      const double x = (double)g.s[i];
      if (isfinite(x)) v[TS_SMAX] = fmax(v[TS_SMAX], fabs(x));
      else v[TS_SNF] = v[TS_SNF] + 1.0;
    }
    if (i < g.cols) {
      const double r = (double)g.r[i];
      if (isfinite(r)) {
        v[TS_RSUM] = v[TS_RSUM] + r;
        v[TS_RMIN] = fmin(v[TS_RMIN], r);
        v[TS_RMAX] = fmax(v[TS_RMAX], r);
      } else {
        v[TS_RNF] = v[TS_RNF] + 1.0;
      }
      const double a = (double)g.a[(size_t)i * g.na];
      v[TS_ASUM] = v[TS_ASUM] + a;
      v[TS_AABS] = v[TS_AABS] + fabs(a);
      if (fabs(a) >= g.limit) v[TS_ASAT] = v[TS_ASAT] + 1.0;
      if (g.t[i] != (T)0) v[TS_TERM] = v[TS_TERM] + 1.0;
    }
    if (i < g.B && g.flags[i] != 0) v[TS_BLOWN] = v[TS_BLOWN] + 1.0;
  }
  tel_block_reduce<StepOps>(v, lds);
  if (tid == 0)
    for (int k = 0; k < TS_K; ++k) tel_store(g.part + (size_t)blockIdx.x * TS_K + k, v[k]);
  if (!tel_last_arriver(g.ticket, lds + TEL_WAVES * TS_K)) return;
#pragma unroll
  for (int k = 0; k < TS_K; ++k) v[k] = StepOps::identity(k);
  for (int b = tid; b < nb; b += TEL_THREADS)
#pragma unroll
    for (int k = 0; k < TS_K; ++k) v[k] = tel_comb(StepOps::of(k), v[k], tel_load(g.part + (size_t)b * TS_K + k));
  tel_block_reduce<StepOps>(v, lds);
  if (tid == 0) {
    const long long pos = g.ctl[0];
    double* row = g.ring + (size_t)(pos % g.cap) * TEL_STEP_COLS;
    const double n = (double)g.cols, nfin = n - v[TS_RNF];
    const bool any = nfin > 0.0;
    row[0] = (double)pos;
    row[1] = any ? v[TS_RSUM] / nfin : (double)NAN;
    row[2] = any ? v[TS_RMIN] : (double)NAN;
    row[3] = any ? v[TS_RMAX] : (double)NAN;
    row[4] = v[TS_RNF];
    row[5] = v[TS_ASUM] / n;
    row[6] = v[TS_AABS] / n;
    row[7] = v[TS_ASAT];
    row[8] = v[TS_SMAX];
    row[9] = v[TS_SNF];
    row[10] = v[TS_BLOWN];
    row[11] = v[TS_TERM];
    if (v[TS_RNF] + v[TS_SNF] > 0.0 && g.ctl[2] < 0) g.ctl[2] = pos;
    g.ctl[0] = pos + 1;
    if (nb > 1) *g.ticket = 0u;
  }
}

template <class T>
struct TelUpdArgs {
  const T *p[2], *pt[2];       // [0] actor, [1] critic: parameters, target parameters
  T* prev[2];
  const T* losses;             // [critic, actor]
  int n[2], nb_a, cap;
  double *part, *ring;
  unsigned* ticket;
  long long* ctl;
};

template <class T>
__global__ void __launch_bounds__(TEL_THREADS) telemetry_update_kernel(TelUpdArgs<T> g) {
#pragma clang fp contract(off)
  __shared__ double lds[TEL_WAVES * 2 * TU_K + 1];
  const int tid = threadIdx.x, nb = (int)gridDim.x;
  const int net = (int)blockIdx.x >= g.nb_a ? 1 : 0;
  const int base = ((int)blockIdx.x - (net ? g.nb_a : 0)) * TEL_UPD_CHUNK, n = g.n[net];
  const T *p = g.p[net], *pt = g.pt[net];
  T* prev = g.prev[net];
  {
    double v[TU_K];
#pragma unroll
    for (int k = 0; k < TU_K; ++k) v[k] = 0.0;
    for (int q = 0; q < TEL_UPD_CHUNK / TEL_THREADS; ++q) {
      const int i = base + q * TEL_THREADS + tid;
      if (i < n) {
        const T raw = p[i];
        const double x = (double)raw, xt = (double)pt[i], xp = (double)prev[i];
        prev[i] = raw;
        if (isfinite(x)) {
          const double xx = x * x;
          v[TU_NORM2] = v[TU_NORM2] + xx;
          v[TU_AMAX] = fmax(v[TU_AMAX], fabs(x));
          if (isfinite(xt)) {
            const double d = x - xt, dd = d * d;
            v[TU_TDIST2] = v[TU_TDIST2] + dd;
          }
          if (isfinite(xp)) {
            const double d = x - xp, dd = d * d;
            v[TU_STEP2] = v[TU_STEP2] + dd;
          }
        } else {
          v[TU_NF] = v[TU_NF] + 1.0;
        }
      }
    }
    tel_block_reduce<UpdOps<1>>(v, lds);
    if (tid == 0)
      for (int k = 0; k < TU_K; ++k) tel_store(g.part + (size_t)blockIdx.x * TU_K + k, v[k]);
  }
  if (!tel_last_arriver(g.ticket, lds + TEL_WAVES * 2 * TU_K)) return;
  double v[2 * TU_K];
#pragma unroll
  for (int k = 0; k < 2 * TU_K; ++k) v[k] = 0.0;
  for (int b = tid; b < nb; b += TEL_THREADS) {
    const bool critic = b >= g.nb_a;
#pragma unroll
    for (int k = 0; k < TU_K; ++k) {
      const double x = tel_load(g.part + (size_t)b * TU_K + k);
      // (0 is the identity: the network workgroup b does not belong to is left as it is)
      v[k] = tel_comb(UpdOps<2>::of(k), v[k], critic ? 0.0 : x);
      v[TU_K + k] = tel_comb(UpdOps<2>::of(k), v[TU_K + k], critic ? x : 0.0);
    }
  }
  tel_block_reduce<UpdOps<2>>(v, lds);
  if (tid == 0) {
    const long long pos = g.ctl[1];
    double* row = g.ring + (size_t)(pos % g.cap) * TEL_UPD_COLS;
    const double lc = (double)g.losses[0], la = (double)g.losses[1];
    const bool first = pos == 0;
    row[0] = (double)pos;
    row[1] = lc;
    row[2] = la;
    row[3] = v[TU_NORM2];
    row[4] = v[TU_K + TU_NORM2];
    row[5] = v[TU_TDIST2];
    row[6] = v[TU_K + TU_TDIST2];
    row[7] = first ? 0.0 : v[TU_STEP2];
    row[8] = first ? 0.0 : v[TU_K + TU_STEP2];
    row[9] = v[TU_AMAX];
    row[10] = v[TU_K + TU_AMAX];
    row[11] = v[TU_NF];
    row[12] = v[TU_K + TU_NF];
    if ((!isfinite(lc) || !isfinite(la) || v[TU_NF] + v[TU_K + TU_NF] > 0.0) && g.ctl[3] < 0) g.ctl[3] = pos;
    g.ctl[1] = pos + 1;
    if (nb > 1) *g.ticket = 0u;
  }
}

static Telemetry* get_telemetry(pdec_handle h, const char* fn) {
  Telemetry* T = lookup_as<Telemetry>(h, Kind::Telemetry);
  if (!T) set_error("%s: not a telemetry handle", fn);
  return T;
}

// rings, counters, tickets and the previous parameters to their initial values; the caller has drained the streams
static int telemetry_clear(Telemetry* T) {
  DevBuf* zero[] = {&T->step_ring, &T->upd_ring, &T->step_part, &T->upd_part, &T->prev_a, &T->prev_c, &T->tickets};
  for (DevBuf* b : zero) PDEC_HIP(hipMemset(b->p, 0, b->bytes));
  const long long ctl0[4] = {0, 0, -1, -1};
  PDEC_HIP(hipMemcpy(T->ctl.p, ctl0, sizeof(ctl0), hipMemcpyHostToDevice));
  PDEC_HIP(hipDeviceSynchronize());
  return PDEC_OK;
}

}  // namespace pdec

using namespace pdec;

extern "C" {

int pdec_telemetry_create(pdec_handle* out, int capacity, int B, int cols, int ns, int na, int env_dtype, pdec_handle actor,
                          pdec_handle critic) {
  PDEC_REQUIRE(out, "pdec_telemetry_create: null handle");
  PDEC_REQUIRE(capacity >= 1, "pdec_telemetry_create: capacity %d < 1", capacity);
  PDEC_REQUIRE(env_dtype == PDEC_F32 || env_dtype == PDEC_F64, "pdec_telemetry_create: dtype %d", env_dtype);
  PDEC_REQUIRE(B >= 1 && cols >= B && ns >= 1 && na >= 1, "pdec_telemetry_create: B %d, cols %d, ns %d, na %d", B, cols, ns, na);
  const long long most = (long long)cols * (ns > na ? ns : na);
  PDEC_REQUIRE(most <= INT32_MAX - TEL_STEP_CHUNK, "pdec_telemetry_create: %lld elements per row exceed the kernel's 32-bit index", most);
  Mlp* A = lookup_as<Mlp>(actor, Kind::Mlp);
  Mlp* Cr = lookup_as<Mlp>(critic, Kind::Mlp);
  if (!A || !Cr) { set_error("pdec_telemetry_create: bad actor or critic handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(A->dtype == Cr->dtype, "pdec_telemetry_create: the actor and the critic must have one dtype");
  PDEC_REQUIRE(A->nparams >= 1 && Cr->nparams >= 1 && A->nparams <= INT32_MAX - TEL_UPD_CHUNK && Cr->nparams <= INT32_MAX - TEL_UPD_CHUNK,
               "pdec_telemetry_create: %d and %d parameters", A->nparams, Cr->nparams);
  auto T = std::make_unique<Telemetry>();
  T->cap = capacity; T->B = B; T->cols = cols; T->ns = ns; T->na = na; T->env_dtype = env_dtype; T->par_dtype = A->dtype;
  T->nA = A->nparams; T->nC = Cr->nparams;
  T->nb_step = (int)(((long long)cols * ns + TEL_STEP_CHUNK - 1) / TEL_STEP_CHUNK);
  T->nb_a = (T->nA + TEL_UPD_CHUNK - 1) / TEL_UPD_CHUNK;
  T->nb_c = (T->nC + TEL_UPD_CHUNK - 1) / TEL_UPD_CHUNK;
  const size_t e = dtype_size(T->par_dtype), cap = (size_t)capacity;
  PDEC_HIP(T->step_ring.alloc(cap * TEL_STEP_COLS * sizeof(double)));
  PDEC_HIP(T->upd_ring.alloc(cap * TEL_UPD_COLS * sizeof(double)));
  PDEC_HIP(T->step_part.alloc((size_t)T->nb_step * TS_K * sizeof(double)));
  PDEC_HIP(T->upd_part.alloc((size_t)(T->nb_a + T->nb_c) * TU_K * sizeof(double)));
  PDEC_HIP(T->prev_a.alloc((size_t)T->nA * e));
  PDEC_HIP(T->prev_c.alloc((size_t)T->nC * e));
  PDEC_HIP(T->ctl.alloc(4 * sizeof(long long)));
  PDEC_HIP(T->tickets.alloc(2 * sizeof(unsigned)));
  const int rc = telemetry_clear(T.get());
  if (rc) return rc;
  *out = register_object(std::move(T));
  return PDEC_OK;
}

int pdec_telemetry_step(pdec_handle telemetry, const void* s_out, const void* action, const void* reward, const void* terminal,
                        const int32_t* flags, double act_limit) {
  Telemetry* T = get_telemetry(telemetry, "pdec_telemetry_step");
  if (!T) return PDEC_E_HANDLE;
  PDEC_REQUIRE(s_out && action && reward && terminal && flags, "pdec_telemetry_step: null argument");
  ProfScope ps(T, "telemetry_step");
  by_dtype(T->env_dtype, [&](auto t) {
    using V = decltype(t);
    TelStepArgs<V> g{};
    g.s = (const V*)s_out; g.a = (const V*)action; g.r = (const V*)reward; g.t = (const V*)terminal; g.flags = flags;
    g.limit = act_limit; g.nS = T->cols * T->ns; g.cols = T->cols; g.na = T->na; g.B = T->B; g.cap = T->cap;
    g.part = T->step_part.as<double>(); g.ring = T->step_ring.as<double>();
    g.ticket = T->tickets.as<unsigned>(); g.ctl = T->ctl.as<long long>();
    hipLaunchKernelGGL(telemetry_step_kernel<V>, dim3(T->nb_step), dim3(TEL_THREADS), 0, T->stream, g);
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_telemetry_update(pdec_handle telemetry, pdec_handle actor, pdec_handle critic, pdec_handle actor_target,
                          pdec_handle critic_target, const void* losses) {
  Telemetry* T = get_telemetry(telemetry, "pdec_telemetry_update");
  if (!T) return PDEC_E_HANDLE;
  PDEC_REQUIRE(losses, "pdec_telemetry_update: null losses");
  Mlp* M[4] = {lookup_as<Mlp>(actor, Kind::Mlp), lookup_as<Mlp>(critic, Kind::Mlp), lookup_as<Mlp>(actor_target, Kind::Mlp),
               lookup_as<Mlp>(critic_target, Kind::Mlp)};
  for (int i = 0; i < 4; ++i) {
    if (!M[i]) { set_error("pdec_telemetry_update: bad network handle (argument %d)", i + 1); return PDEC_E_HANDLE; }
    PDEC_REQUIRE(M[i]->dtype == T->par_dtype && M[i]->nparams == (i % 2 ? T->nC : T->nA),
                 "pdec_telemetry_update: network %d differs in dtype or size from the one the object was made for", i + 1);
  }
  T->upd_stream = M[1]->stream;
  ProfScope ps(M[1], "telemetry_update");      // (timed through the critic's handle: the launch runs on its stream)
  by_dtype(T->par_dtype, [&](auto t) {
    using V = decltype(t);
    TelUpdArgs<V> g{};
    g.p[0] = M[0]->params.as<V>(); g.p[1] = M[1]->params.as<V>(); g.pt[0] = M[2]->params.as<V>(); g.pt[1] = M[3]->params.as<V>();
    g.prev[0] = T->prev_a.as<V>(); g.prev[1] = T->prev_c.as<V>();
    g.losses = (const V*)losses; g.n[0] = T->nA; g.n[1] = T->nC; g.nb_a = T->nb_a; g.cap = T->cap;
    g.part = T->upd_part.as<double>(); g.ring = T->upd_ring.as<double>();
    g.ticket = T->tickets.as<unsigned>() + 1; g.ctl = T->ctl.as<long long>();
    hipLaunchKernelGGL(telemetry_update_kernel<V>, dim3(T->nb_a + T->nb_c), dim3(TEL_THREADS), 0, T->upd_stream, g);
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_telemetry_read(pdec_handle telemetry, double* step_rows, int64_t* n_step_calls, double* update_rows, int64_t* n_update_calls,
                        int64_t* sentinel) {
  Telemetry* T = get_telemetry(telemetry, "pdec_telemetry_read");
  if (!T) return PDEC_E_HANDLE;
  PDEC_HIP(hipStreamSynchronize(T->stream));
  if (T->upd_stream != T->stream) PDEC_HIP(hipStreamSynchronize(T->upd_stream));
  long long ctl[4];
  PDEC_HIP(hipMemcpy(ctl, T->ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
  if (step_rows) PDEC_HIP(hipMemcpy(step_rows, T->step_ring.p, T->step_ring.bytes, hipMemcpyDeviceToHost));
  if (update_rows) PDEC_HIP(hipMemcpy(update_rows, T->upd_ring.p, T->upd_ring.bytes, hipMemcpyDeviceToHost));
  if (n_step_calls) *n_step_calls = ctl[0];
  if (n_update_calls) *n_update_calls = ctl[1];
  if (sentinel) { sentinel[0] = ctl[2]; sentinel[1] = ctl[3]; }
  return PDEC_OK;
}

int pdec_telemetry_reset(pdec_handle telemetry) {
  Telemetry* T = get_telemetry(telemetry, "pdec_telemetry_reset");
  if (!T) return PDEC_E_HANDLE;
  PDEC_HIP(hipStreamSynchronize(T->stream));
  if (T->upd_stream != T->stream) PDEC_HIP(hipStreamSynchronize(T->upd_stream));
  return telemetry_clear(T);
}

}  // extern "C"
