// episode_clock.hip -- per-trajectory episodes of the batched training pipeline, decided on the device.
//
// The lock-stepped pipeline ends every episode on the host: all B trajectories start together and time out together, and a
// trajectory that blows up in between is integrated on to the common end.  The episode clock gives every trajectory b its own
// clock; one boundary launch behind env step k decides per trajectory, from that step's blow-up flag and the clock, whether
// the episode ends IN this step, and restarts it there.  Rule per trajectory b, in this order (E: episode_steps, C: capacity,
// R = A reward columns):
//   1. blew = flags[b] != 0; where blew, non-finite entries of reward row b become 0 (autoreset_kernel's rule); other rows
//      are not touched
//   2. ret[b] += (sum_a (double) r[b][a]) / R, summed in a order (ledger_step_kernel's arithmetic, on the sanitised row)
//   3. clock[b]++, len[b]++, total[b]++; ends = blew || clock[b] == E
//   4. not ended: action_prev_next[b][:] = action[b][:], nothing else of b is written
//   5. ended: terminal row b = 1 (a time-out is terminal); log slot count[b] % C <- (ret[b], len[b], blew, total[b]);
//      count[b]++; ret[b] = 0; clock[b] = len[b] = 0; action_prev_next[b][:] = 0; y_next[b] <- the new field;
//      state_next[b] <- featurize(y_next[b]) in reset form (no previous state)
// The new field: row b of (y0, state0) -- or, with random initial fields, row b of what pdec_env_random_init(env, seed, off)
// draws at off = (n W + r) B ceil(nc / 4), n = count[b] after the increment and (r, W) the rank split: the field the
// lock-stepped pipeline's _draw_init gives trajectory b in its episode n.
//
// Two launches, both one workgroup per trajectory, a workgroup writing its own trajectory's rows only:
//   epclock_boundary_kernel  256 threads: rules 1 - 5 up to the new field (random_init_row reduces over its 256 threads, as
//                            random_init_kernel does), and ended[b] for the second launch
//   epclock_sense_kernel     128 threads, where ended[b]: sense_traj<T, 1> of y_next[b], the body of pdec_featurize's kernel
//                            at its workgroup size, so the state row equals pdec_featurize's bit for bit (with a fixed pair
//                            the row is copied from state0 in the first launch and this one is not issued)
// Every argument other than the ring pointers is fixed at creation and every counter lives on the device, so recorded steps
// and captured graphs hold the launches.
#include "env_sense.hpp"
#include "random_init.hpp"

namespace pdec {

struct EpisodeClock : Object {
  pdec_handle env = 0;
  int B = 0, R = 0, E = 0, cap = 0, random_init = 0, rank = 0, world = 1;
  uint64_t seed = 0;
  RandomInitSpec ri{};
  DevBuf clock, len, ended;       // int32 [B]
  DevBuf count, total;            // int64 [B]
  DevBuf ret;                     // double [B]
  DevBuf log_ret;                 // double [B][cap]
  DevBuf log_len, log_blew;       // int32 [B][cap]
  DevBuf log_end;                 // int64 [B][cap]
  EpisodeClock() : Object(Kind::EpisodeClock) {}
};

template <class T>
struct ClockArgs {
  T* reward;                  // [B][R]
  const int32_t* flags;       // [B]
  T* terminal;                // [B][R]
  const T* action;            // [B][arow]
  T* aprev_next;              // [B][arow]
  T* y_next;                  // [B][yrow]
  T* state_next;              // [B][srow]
  const T *y0, *state0;       // the fixed pair (null with random initial fields)
  int32_t *clock, *len, *ended;
  long long *count, *total;
  double* ret;
  double* log_ret;
  int32_t *log_len, *log_blew;
  long long* log_end;
  int R, E, cap, arow, yrow, srow, random_init, B;
  RandomInitSpec ri;
  uint64_t seed, rank, world;
};

template <class T>
__global__ void __launch_bounds__(RI_THREADS) epclock_boundary_kernel(ClockArgs<T> g) {
  __shared__ double a[RI_MAXC];
  __shared__ double red[RI_THREADS];
  __shared__ int s_ends;
  __shared__ long long s_n;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const bool blew = g.flags[b] != 0;
  T* r = g.reward + (size_t)b * g.R;
  if (blew)
    for (int i = tid; i < g.R; i += nt)
      if (!isfinite(r[i])) r[i] = (T)0;
  __syncthreads();      // (the row is this workgroup's own stores: visible to thread 0 behind the barrier)
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < g.R; ++i) s += (double)r[i];
    double ret = g.ret[b];
    ret += s / (double)g.R;
    const int c = g.clock[b] + 1, l = g.len[b] + 1;
    const long long t = g.total[b] + 1;
    g.total[b] = t;
    const int ends = blew || c == g.E;
    if (!ends) {
      g.ret[b] = ret;
      g.clock[b] = c;
      g.len[b] = l;
    } else {
      const long long n = g.count[b];
      const size_t slot = (size_t)b * g.cap + (size_t)(n % g.cap);
      g.log_ret[slot] = ret;
      g.log_len[slot] = l;
      g.log_blew[slot] = blew ? 1 : 0;
      g.log_end[slot] = t;
      g.count[b] = n + 1;
      g.ret[b] = 0.0;
      g.clock[b] = 0;
      g.len[b] = 0;
      s_n = n + 1;
    }
    g.ended[b] = ends;
    s_ends = ends;
  }
  __syncthreads();
  T* ap = g.aprev_next + (size_t)b * g.arow;
  if (!s_ends) {
    const T* ac = g.action + (size_t)b * g.arow;
    for (int i = tid; i < g.arow; i += nt) ap[i] = ac[i];
    return;
  }
  T* term = g.terminal + (size_t)b * g.R;
  for (int i = tid; i < g.R; i += nt) term[i] = (T)1;
  for (int i = tid; i < g.arow; i += nt) ap[i] = (T)0;
  if (!g.random_init) {
    const T* ys = g.y0 + (size_t)b * g.yrow;
    T* yd = g.y_next + (size_t)b * g.yrow;
    for (int i = tid; i < g.yrow; i += nt) yd[i] = ys[i];
    const T* ss = g.state0 + (size_t)b * g.srow;
    T* sd = g.state_next + (size_t)b * g.srow;
    for (int i = tid; i < g.srow; i += nt) sd[i] = ss[i];
    return;
  }
  // episode n of rank r of W: the draw of pdec_env_random_init(seed, (n W + r) B nblk), of which trajectory b takes the blocks
  // from b nblk on
  const uint64_t nblk = (uint64_t)((g.ri.nsp * g.ri.nsin + 3) / 4);
  const uint64_t off = ((uint64_t)s_n * g.world + g.rank) * (uint64_t)g.B * nblk;
  random_init_row<T>(g.y_next, b, g.ri.N, g.ri.nsp, g.ri.nsin, g.ri.dx, g.ri.fdiv, g.ri.base, g.ri.l2, g.seed, off + (uint64_t)b * nblk, a,
                     red);
}

// the features of the restarted trajectories' new fields (random initial fields only)
// FLT (pdec_env_set_faults): through the restarted trajectory's own sensor faults, as the step would have written the state
template <class T, bool FLT = false>
__global__ void __launch_bounds__(PDEC_SENSE_THREADS) epclock_sense_kernel(EnvArg<T, FLT> e, const int32_t* __restrict__ ended,
                                                                          const T* __restrict__ y_next, T* __restrict__ state_next) {
  const int b = blockIdx.x;
  if (ended[b] == 0) return;
  sense_traj<T, 1, FLT>(e, b, y_next, nullptr, nullptr, nullptr, state_next);
}

static EpisodeClock* get_clock(pdec_handle h, const char* fn, Env** E) {
  EpisodeClock* K = lookup_as<EpisodeClock>(h, Kind::EpisodeClock);
  if (!K) {
    set_error("%s: not an episode clock handle", fn);
    return nullptr;
  }
  if (E) {
    *E = lookup_as<Env>(K->env, Kind::Env);
    if (!*E) {
      set_error("%s: the clock's environment has been destroyed", fn);
      return nullptr;
    }
  }
  return K;
}

}  // namespace pdec

using namespace pdec;

extern "C" {

int pdec_epclock_create(pdec_handle* out, pdec_handle env, int episode_steps, int capacity, int random_init, uint64_t seed, int rank,
                        int world) {
  PDEC_REQUIRE(out, "pdec_epclock_create: null handle");
  Env* E = lookup_as<Env>(env, Kind::Env);
  if (!E) { set_error("pdec_epclock_create: bad environment handle"); return PDEC_E_HANDLE; }
  const pdec_env_cfg& c = E->cfg;
  PDEC_REQUIRE(c.pde_kind == PDEC_PDE_KS_CNAB2 || c.pde_kind == PDEC_PDE_KS_RK4_FD || c.pde_kind == PDEC_PDE_KSEG_RK4,
               "pdec_epclock_create: the 1-D environments only (KS, finite-difference KS, Keller-Segel)");
  PDEC_REQUIRE(!c.mono, "pdec_epclock_create: per-actuator agents only (mono)");
  PDEC_REQUIRE(c.memory_size == 0, "pdec_epclock_create: memory_size %d > 0 is not covered", c.memory_size);
  PDEC_REQUIRE(episode_steps >= 1, "pdec_epclock_create: episode_steps %d < 1", episode_steps);
  PDEC_REQUIRE(capacity >= 1, "pdec_epclock_create: capacity %d < 1", capacity);
  PDEC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "pdec_epclock_create: rank %d of %d", rank, world);
  auto K = std::make_unique<EpisodeClock>();
  K->env = env; K->B = c.B; K->R = c.A; K->E = episode_steps; K->cap = capacity; K->random_init = random_init ? 1 : 0;
  K->seed = seed; K->rank = rank; K->world = world;
  K->stream = E->stream;
  if (K->random_init) {
    PDEC_REQUIRE(random_init_spec(c, &K->ri), "pdec_epclock_create: the environment has no device initialiser");
    PDEC_REQUIRE(K->ri.nsp * K->ri.nsin <= RI_MAXC, "pdec_epclock_create: %d sine coefficients exceed the kernel's table",
                 K->ri.nsp * K->ri.nsin);
  }
  const size_t B = (size_t)c.B, n = B * (size_t)capacity;
  DevBuf* bufs[] = {&K->clock, &K->len, &K->ended, &K->count, &K->total, &K->ret, &K->log_ret, &K->log_len, &K->log_blew, &K->log_end};
  const size_t bytes[] = {B * 4, B * 4, B * 4, B * 8, B * 8, B * 8, n * 8, n * 4, n * 4, n * 8};
  for (int i = 0; i < 10; ++i) {
    PDEC_HIP(bufs[i]->alloc(bytes[i]));
    PDEC_HIP(hipMemset(bufs[i]->p, 0, bytes[i]));
  }
  PDEC_HIP(hipDeviceSynchronize());
  *out = register_object(std::move(K));
  return PDEC_OK;
}

int pdec_epclock_set(pdec_handle clock, const int32_t* clock0) {
  Env* E = nullptr;
  EpisodeClock* K = get_clock(clock, "pdec_epclock_set", &E);
  if (!K) return PDEC_E_HANDLE;
  const size_t B = (size_t)K->B;
  if (clock0)
    for (size_t b = 0; b < B; ++b)
      PDEC_REQUIRE(clock0[b] >= 0 && clock0[b] < K->E, "pdec_epclock_set: clock0[%zu] = %d outside 0 .. %d", b, clock0[b], K->E - 1);
  // a rare call (construction, reset_from): behind everything the stream still holds, blocking copies
  PDEC_HIP(hipStreamSynchronize(E->stream));
  if (clock0)
    PDEC_HIP(hipMemcpy(K->clock.p, clock0, B * sizeof(int32_t), hipMemcpyHostToDevice));
  else
    PDEC_HIP(hipMemset(K->clock.p, 0, B * sizeof(int32_t)));
  PDEC_HIP(hipMemset(K->len.p, 0, B * sizeof(int32_t)));
  PDEC_HIP(hipMemset(K->ret.p, 0, B * sizeof(double)));
  PDEC_HIP(hipDeviceSynchronize());
  return PDEC_OK;
}

int pdec_epclock_step(pdec_handle clock, void* reward, const int32_t* flags, void* terminal, const void* action, void* action_prev_next,
                      void* y_next, void* state_next, const void* y0, const void* state0) {
  Env* E = nullptr;
  EpisodeClock* K = get_clock(clock, "pdec_epclock_step", &E);
  if (!K) return PDEC_E_HANDLE;
  PDEC_REQUIRE(reward && flags && terminal && action && action_prev_next && y_next && state_next, "pdec_epclock_step: null argument");
  PDEC_REQUIRE(K->random_init || (y0 && state0), "pdec_epclock_step: a clock without random initial fields needs y0 and state0");
  PDEC_REQUIRE(action != action_prev_next, "pdec_epclock_step: action_prev_next must not alias action");
  const pdec_env_cfg& c = E->cfg;
  ProfScope ps(E, "epclock_step");
  by_dtype(c.dtype, [&](auto t) {
    using T = decltype(t);
    ClockArgs<T> g{};
    g.reward = (T*)reward; g.flags = flags; g.terminal = (T*)terminal; g.action = (const T*)action; g.aprev_next = (T*)action_prev_next;
    g.y_next = (T*)y_next; g.state_next = (T*)state_next; g.y0 = (const T*)y0; g.state0 = (const T*)state0;
    g.clock = K->clock.as<int32_t>(); g.len = K->len.as<int32_t>(); g.ended = K->ended.as<int32_t>();
    g.count = K->count.as<long long>(); g.total = K->total.as<long long>(); g.ret = K->ret.as<double>();
    g.log_ret = K->log_ret.as<double>(); g.log_len = K->log_len.as<int32_t>(); g.log_blew = K->log_blew.as<int32_t>();
    g.log_end = K->log_end.as<long long>();
    g.R = K->R; g.E = K->E; g.cap = K->cap; g.arow = c.A * env_na(c); g.yrow = (int)env_y_count(c); g.srow = c.A * env_ns(c);
    g.random_init = K->random_init; g.B = K->B; g.ri = K->ri; g.seed = K->seed; g.rank = (uint64_t)K->rank; g.world = (uint64_t)K->world;
    hipLaunchKernelGGL(epclock_boundary_kernel<T>, dim3(K->B), dim3(RI_THREADS), 0, E->stream, g);
    if (K->random_init && E->faults())
      hipLaunchKernelGGL((epclock_sense_kernel<T, true>), dim3(K->B), dim3(PDEC_SENSE_THREADS), sense_lds_bytes(c), E->stream,
                         make_dev_faults<T>(*E), (const int32_t*)K->ended.as<int32_t>(), (const T*)y_next, (T*)state_next);
    else if (K->random_init)
      hipLaunchKernelGGL(epclock_sense_kernel<T>, dim3(K->B), dim3(PDEC_SENSE_THREADS), sense_lds_bytes(c), E->stream, make_dev<T>(*E),
                         (const int32_t*)K->ended.as<int32_t>(), (const T*)y_next, (T*)state_next);
  });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_epclock_read(pdec_handle clock, int64_t* counts, double* returns, int32_t* lengths, int32_t* blew_up, int64_t* end_steps) {
  Env* E = nullptr;
  EpisodeClock* K = get_clock(clock, "pdec_epclock_read", &E);
  if (!K) return PDEC_E_HANDLE;
  PDEC_HIP(hipStreamSynchronize(E->stream));
  const size_t B = (size_t)K->B, n = B * (size_t)K->cap;
  if (counts) PDEC_HIP(hipMemcpy(counts, K->count.p, B * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (returns) PDEC_HIP(hipMemcpy(returns, K->log_ret.p, n * sizeof(double), hipMemcpyDeviceToHost));
  if (lengths) PDEC_HIP(hipMemcpy(lengths, K->log_len.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (blew_up) PDEC_HIP(hipMemcpy(blew_up, K->log_blew.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (end_steps) PDEC_HIP(hipMemcpy(end_steps, K->log_end.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return PDEC_OK;
}

}  // extern "C"
