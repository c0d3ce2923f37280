// act.hip -- agent(env) (src/PDEagent.jl:175-209): the routing of an acting call to a fused family, the few-column kernel or the
// generic sequence; the few-column acting kernel; the glue between two control steps, solo and for populations; the device
// noise counter.
#include "common.hpp"
#include "population.hpp"

using namespace pdec;

// ---- acting for FEW columns in one launch (the reference's own shape: one trajectory, A columns; src/PDEagent.jl:175-209)
// The generic path is pack + one GEMM launch per layer + randn + noise / clamp -- and, when the environment computes in fp64
// while the networks are Float32 (as in the reference), a promoted copy of the parameters first: seven launches of ~5.5 us for
// a few hundred multiply-adds.  This kernel does the same arithmetic in ONE workgroup: parameters of type TP promoted to T on
// the fly (exact), activations [feature][column] in LDS, per element acc = sum_k w x in ascending k from zero, then + bias and
// the activation -- the order of gemm_kernel's epilogue --, the Philox / Box-Muller draw of randn_kernel for element
// column * outputs + row, then v += noise * act_noise and the clamp of act_noise_clamp_kernel.
// (SMALL_ACT_MAXL: mlp.hpp)
// AN: what carries the amplitude -- the launch scalar, NoiseScale (pdec_mlp_set_noise_scale; a kernel family of its own, so
// that the scalar kernels keep their arguments and their code) or NoiseColor (pdec_mlp_set_noise_color; likewise)
template <class AN>
struct SmallActArgsT {
  int L, cols, maxw, learning, nrows;
  int dims[SMALL_ACT_MAXL + 1], acts[SMALL_ACT_MAXL], woff[SMALL_ACT_MAXL], boff[SMALL_ACT_MAXL];
  const void* p;
  AN act_noise;
  double lim;
  uint64_t seed, offset;
  const uint64_t* ctr_cur;
  uint64_t* ctr_next;
  uint64_t ctr_inc;
};
using SmallActArgs = SmallActArgsT<double>;
// the kernel's body; returns the LDS buffer that holds the finished actions as element i = column * outputs + row (what `out`
// receives), for a caller that goes on with them inside the same launch (step_glue_kernel)
template <class T, class TP, class AN>
__device__ __forceinline__ T* small_act_body(const SmallActArgsT<AN>& g, const T* __restrict__ state, T* __restrict__ out,
                                             unsigned char* smem) {
  T* X0 = reinterpret_cast<T*>(smem);
  T* X1 = X0 + (size_t)g.maxw * g.cols;
  const TP* p = static_cast<const TP*>(g.p);
  const int tid = threadIdx.x, cols = g.cols;
  uint64_t offset = g.offset;
  if (g.ctr_cur) {       // device-resident noise counter (pdec_policy_act_rng_dev)
    offset += *g.ctr_cur;
    if (tid == 0) *g.ctr_next = offset + g.ctr_inc;
  }
  const int ns = g.dims[0];
  for (int i = tid; i < ns * cols; i += 256) {
    const int c = i / ns, k = i - c * ns;
    X0[k * cols + c] = state[i];
  }
  __syncthreads();
  T* xin = X0;
  T* xout = X1;
  for (int l = 0; l < g.L; ++l) {
    const int in = g.dims[l], on = g.dims[l + 1];
    const TP* W = p + g.woff[l];
    const TP* b = p + g.boff[l];
    for (int i = tid; i < on * cols; i += 256) {
      const int j = i / cols, c = i - j * cols;
      T acc = 0;
      for (int k = 0; k < in; ++k) acc += (T)W[j * in + k] * xin[k * cols + c];
      xout[j * cols + c] = apply_act<T>(acc + (T)b[j], g.acts[l]);
    }
    __syncthreads();
    T* t = xin; xin = xout; xout = t;
  }
  const int no = g.dims[g.L];
  constexpr bool NS = noise_per_column<AN>;
  T an = 0;
  if constexpr (!NS) an = (T)g.act_noise;
  const T lim = (T)g.lim;
  for (int i = tid; i < no * cols; i += 256) {       // i = column * outputs + row: the element index of the noise stream
    const int c = i / no, f = i - c * no;
    T v = xin[f * cols + c];
    if (g.learning && f < g.nrows) {
      const T z = noise_draw<T>(g.act_noise, noise_normal(g.seed, offset, i), c, i);
      if constexpr (NS) an = noise_amp<T>(g.act_noise, c);
      v += z * an;
    }
    v = v < -lim ? -lim : (v > lim ? lim : v);
    out[i] = v;
    xout[i] = v;
  }
  return xout;
}
template <class T, class TP, class AN = double>
__global__ __launch_bounds__(256) void small_act_kernel(SmallActArgsT<AN> g, const T* __restrict__ state, T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char small_act_smem[];
  (void)small_act_body<T, TP>(g, state, out, small_act_smem);
}

// ---- the glue between two control steps of a single-trajectory training loop, ONE launch instead of three (round 6):
//   POST_ACT push of the step that just ran (reward, terminal; src/PDEagent.jl:276-289; raises the episode halt flag when that
//   step ended the episode -- replay_push_rt_kernel), agent(env) for the next step (small_act_kernel; or the zero action of the
//   start policy), PRE_ACT push of the next step's (state, action) (:254-274; replay_push2_kernel: skipped once the episode has
//   ended).  Same arithmetic and the same stores as the three launches; each of them was ~5 us of launch latency on the chain
//   act -> push -> update / env step -> push of the reference-shaped loop.
template <class AN>
struct StepGlueArgsT {
  float *tr, *tt;              // POST_ACT push: reward / terminal traces, capacity cap_rt, first slot start_rt, n_rt values (0: none)
  const void* r;
  const int32_t* done;
  int cols_per_traj, force;
  long long cap_rt, start_rt, n_rt;
  int act_mode;                // 0: no acting, 1: the actor, 2: the zero action
  SmallActArgsT<AN> act;
  const void* state;           // [cols][ns] of the environment's type: acting input and the PRE_ACT push's state rows
  void* out;                   // [cols][na]
  float *ts, *ta;              // PRE_ACT push: state / action traces, capacity cap_sa rows, first row start_sa, n_sa rows (0: none)
  int ns, na;
  long long cap_sa, start_sa, n_sa;
  int* halt;
  LaunchSync sync;             // pdec_set_launch_sync on the actor's handle: wait before the first read, signal behind the last store
  // population (pdec_population_glue): != null -> workgroup m serves member m, with its pointers from pm[m], its counters from
  // rows[m] and its slices of r / done / state / out (r_bytes, s_bytes, o_bytes apart); phase 0: a control step, 1: the
  // time-out push of the last step, 2: the POST_EPISODE push of the final state (active members, halt ignored)
  const PopMember* pm;
  long long* rows;
  int phase;
  long long d_noise, start_steps;
  size_t r_bytes, s_bytes, o_bytes;
};
using StepGlueArgs = StepGlueArgsT<double>;
template <class T, class TP, class AN = double>
__global__ __launch_bounds__(256) void step_glue_kernel(StepGlueArgsT<AN> g_in) {
  extern __shared__ __align__(16) unsigned char small_act_smem[];
  const int tid = threadIdx.x;
  StepGlueArgsT<AN> g = g_in;
  long long* mrow = nullptr;
  bool macting = false;
  if (g.pm) {                         // population member blockIdx.x: the solo call's arguments from its table entries
    const int mb = blockIdx.x;
    const PopMember& pm = g.pm[mb];
    mrow = g.rows + (size_t)mb * POP_ROW;
    g.tr = pm.tr; g.tt = pm.tt; g.ts = pm.ts; g.ta = pm.ta;
    g.act.p = pm.actor_p; g.act.seed = pm.noise_seed; g.act.offset = (uint64_t)mrow[POP_NOISE];
    if constexpr (std::is_same<AN, double>::value) g.act.act_noise = __longlong_as_double(mrow[POP_NOISE_AMP]);   // (members: scalar only)
    g.act.lim = __longlong_as_double(mrow[POP_LIMIT]);
    g.start_rt = mrow[POP_NRT] % g.cap_rt;
    g.start_sa = mrow[POP_NSA] % g.cap_sa;
    if (g.r) g.r = static_cast<const char*>(g.r) + mb * g.r_bytes;
    if (g.done) g.done += mb;
    if (g.state) g.state = static_cast<const char*>(g.state) + mb * g.s_bytes;
    if (g.out) g.out = static_cast<char*>(g.out) + mb * g.o_bytes;
    if (g.phase == 0) {               // acting = update_step > start_steps, with this step's update_step (run.py)
      macting = mrow[POP_USTEP] + 1 > g.start_steps;
      g.act_mode = macting ? 1 : 2;
    }
    if (g.phase == 2) {
      g.halt = nullptr;
      if (!mrow[POP_ACTIVE]) g.n_sa = 0;
    } else {
      g.halt = reinterpret_cast<int*>(mrow + POP_HALT);
    }
  }
  launch_sync_wait(g.sync);           // (the env step that wrote reward / done / state, on another stream)
  const bool was = g.halt && *g.halt;
  const bool ended = was || (g.halt && g.n_rt && g.done && g.done[0] != 0);
  if (g.n_rt && !was) {
    const T* r = static_cast<const T*>(g.r);
    for (long long i = tid; i < g.n_rt; i += 256) {
      const long long slot = (g.start_rt + i) % g.cap_rt;
      g.tr[slot] = (float)r[i];
      g.tt[slot] = (g.force || (g.done && g.done[i / g.cols_per_traj] != 0)) ? 1.f : 0.f;
    }
  }
  __syncthreads();                    // every thread has read *halt before one of them writes it
  if (tid == 0 && g.halt && !was && ended) *g.halt = 1;
  const T* state = static_cast<const T*>(g.state);
  T* out = static_cast<T*>(g.out);
  const T* acts = nullptr;            // the actions of this launch in LDS, element row * na + c
  if (g.act_mode == 1) {
    acts = small_act_body<T, TP>(g.act, state, out, small_act_smem);
  } else if (g.act_mode == 2) {
    for (long long i = tid; i < (long long)g.act.cols * g.na; i += 256) out[i] = (T)0;
  }
  if (g.n_sa && !ended) {
    __syncthreads();                  // the actions are in LDS
    const long long na_ = g.n_sa * g.ns, nb_ = g.n_sa * g.na;
    for (long long i = tid; i < na_ + nb_; i += 256) {
      if (i < na_) {
        const long long row = i / g.ns, c = i - row * g.ns;
        g.ts[((g.start_sa + row) % g.cap_sa) * g.ns + c] = (float)state[i];
      } else {
        const long long j = i - na_, row = j / g.na, c = j - row * g.na;
        g.ta[((g.start_sa + row) % g.cap_sa) * g.na + c] = acts ? (float)acts[j] : 0.f;
      }
    }
  }
  // the member's counters move as run.py settles the solo run's: the push of the step that ends the episode counts, the rest of
  // that step does not; nothing moves once the halt flag is up (every thread read the row before the barrier above)
  if (mrow && tid == 0 && g.phase != 2 && !was) {
    if (g.n_rt) mrow[POP_NRT] += g.n_rt;
    if (g.phase == 0 && !ended) {
      mrow[POP_USTEP] += 1;
      mrow[POP_NSA] += g.n_sa;
      if (macting) mrow[POP_NOISE] += g.d_noise;
    }
  }
  launch_sync_done(g.sync);
}

int pdec::mlp_maxw(const Mlp* M) {
  int maxw = 1;
  for (int l = 0; l <= M->L; ++l) maxw = std::max(maxw, M->dims[l]);
  return maxw;
}
// dynamic LDS of the acting body: two activation buffers [widest layer][cols] of the state's type
static size_t small_act_lds(const Mlp* M, int dtype, int cols) { return (size_t)2 * mlp_maxw(M) * cols * dtype_size(dtype); }

// does the single-launch form serve this actor at `cols` columns of type `dtype`?  (the fused MFMA acting kernels keep fp32
// actors at fp32 states; PDEC_SMALL_ACT=0: the generic launch sequence, for A/B tests)
static bool small_act_ok(const Mlp* M, int dtype, int cols) {
  static const bool off = [] { const char* e = getenv("PDEC_SMALL_ACT"); return e && e[0] == '0'; }();
  if (off || M->L > SMALL_ACT_MAXL || cols < 1) return false;
  if (!(M->dtype == dtype || (M->dtype == PDEC_F32 && dtype == PDEC_F64))) return false;
  return small_act_lds(M, dtype, cols) <= SMALL_ACT_LDS;
}

// the fields of SmallActArgs that depend on the network
template <class AN = double>
static SmallActArgsT<AN> small_act_args(const Mlp* M, int cols) {
  SmallActArgsT<AN> g{};
  g.L = M->L; g.cols = cols;
  g.maxw = mlp_maxw(M);
  for (int l = 0; l <= M->L; ++l) g.dims[l] = M->dims[l];
  for (int l = 0; l < M->L; ++l) { g.acts[l] = M->acts[l]; g.woff[l] = (int)M->w_off[l]; g.boff[l] = (int)M->b_off[l]; }
  g.nrows = M->noise_rows < 0 ? M->dims[M->L] : M->noise_rows;
  return g;
}

template <class AN>
static int small_act_launch(Mlp* M, int dtype, const void* state, int cols, AN act_noise, double act_limit, int learning,
                            uint64_t seed, uint64_t offset, void* actions_out, const uint64_t* ctr_cur, uint64_t* ctr_next,
                            uint64_t ctr_inc) {
  SmallActArgsT<AN> g = small_act_args<AN>(M, cols);
  g.learning = learning;
  g.p = M->params.p;
  g.act_noise = act_noise; g.lim = act_limit; g.seed = seed; g.offset = offset;
  g.ctr_cur = ctr_cur; g.ctr_next = ctr_next; g.ctr_inc = ctr_inc;
  const size_t lds = small_act_lds(M, dtype, cols);
  ProfScope ps(M, "small_act");
  if (dtype == PDEC_F64 && M->dtype == PDEC_F32)
    hipLaunchKernelGGL((small_act_kernel<double, float, AN>), dim3(1), dim3(256), lds, M->stream, g, (const double*)state, (double*)actions_out);
  else if (dtype == PDEC_F64)
    hipLaunchKernelGGL((small_act_kernel<double, double, AN>), dim3(1), dim3(256), lds, M->stream, g, (const double*)state, (double*)actions_out);
  else
    hipLaunchKernelGGL((small_act_kernel<float, float, AN>), dim3(1), dim3(256), lds, M->stream, g, (const float*)state, (float*)actions_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}
static int small_act(Mlp* M, int dtype, const void* state, int cols, double act_noise, double act_limit, int learning, uint64_t seed,
                     uint64_t offset, void* actions_out, const uint64_t* ctr_cur, uint64_t* ctr_next, uint64_t ctr_inc) {
  if (learning && M->noise_color)
    return small_act_launch(M, dtype, state, cols, noise_color_of(M, act_noise), act_limit, learning, seed, offset, actions_out,
                            ctr_cur, ctr_next, ctr_inc);
  if (M->noise_scale)
    return small_act_launch(M, dtype, state, cols, noise_scale_of(M), act_limit, learning, seed, offset, actions_out, ctr_cur,
                            ctr_next, ctr_inc);
  return small_act_launch(M, dtype, state, cols, act_noise, act_limit, learning, seed, offset, actions_out, ctr_cur, ctr_next, ctr_inc);
}

// launch(step_glue_kernel<T, TP>) of the (state dtype, parameter dtype) pair; the caller brings its own launch call
template <class AN = double, class F>
static void step_glue_dispatch(int state_dtype, int param_dtype, F&& launch) {
  if (state_dtype == PDEC_F64 && param_dtype == PDEC_F32) launch(step_glue_kernel<double, float, AN>);
  else if (state_dtype == PDEC_F64) launch(step_glue_kernel<double, double, AN>);
  else launch(step_glue_kernel<float, float, AN>);
}

ActRoute pdec::act_route(const Mlp* M, int cols) { return small_act_ok(M, M->dtype, cols) ? ACT_SMALL : ACT_GENERIC; }

// does pdec_step_glue serve this case (see there)?
bool pdec::step_glue_served(const Mlp* M, const Object* o, int dtype, int act_mode, int cols, int64_t n_rt) {
  return o->stream == M->stream && n_rt <= 256 && !(act_mode == 1 && (!small_act_ok(M, dtype, cols) || M->dtype == dtype));
}

extern "C" {

static int policy_act_rng_impl(pdec_handle actor, Mlp* M, const void* state, int cols, double act_noise, double act_limit,
                               int learning, uint64_t seed, uint64_t offset, void* actions_out, const uint64_t* ctr_cur,
                               uint64_t* ctr_next, uint64_t ctr_inc) {
  if (learning) PDEC_REQUIRE_NOISE_COLS(M, cols, "pdec_policy_act_rng");
  if (const FusedFamily* fam = fused_family_of_act(M, cols))
    return fam->policy_act(M, state, cols, act_noise, act_limit, learning, seed, offset, actions_out, ctr_cur, ctr_next, ctr_inc);
  if (act_route(M, cols) == ACT_SMALL)
    return small_act(M, M->dtype, state, cols, act_noise, act_limit, learning, seed, offset, actions_out, ctr_cur, ctr_next, ctr_inc);
  void* noise = nullptr;
  const size_t n = (size_t)cols * M->dims[M->L];
  const int zdtype = learning && M->noise_color ? PDEC_F64 : M->dtype;   // (the recurrence takes z as the double it is drawn as)
  if (learning || ctr_cur) {
    if (M->noise.bytes < n * dtype_size(zdtype)) PDEC_HIP(M->noise.alloc(n * dtype_size(zdtype)));
    ProfScope ps(M, "randn");
    int rc = launch_randn(M, M->noise.p, n, zdtype, seed, offset, ctr_cur, ctr_next, ctr_inc);
    if (rc) return rc;
    if (learning) noise = M->noise.p;
  }
  return policy_act_noise(M, state, noise, zdtype, cols, act_noise, act_limit, actions_out, "pdec_policy_act_rng");
}

int pdec_policy_act_rng(pdec_handle actor, const void* state, int cols, double act_noise, double act_limit,
                        int learning, uint64_t seed, uint64_t offset, void* actions_out) {
  GET_MLP(M, actor);
  PDEC_REQUIRE(state && actions_out && cols >= 1, "pdec_policy_act_rng: null/empty");
  return policy_act_rng_impl(actor, M, state, cols, act_noise, act_limit, learning, seed, offset, actions_out, nullptr, nullptr, 0);
}

// agent(env) for an environment that computes in `state_dtype` with an actor of another parameter type (the reference: fp64
// fields, Float32 networks) WITHOUT a promoted copy of the actor: *served = 1 and the action is enqueued when the single-launch
// form covers the case, *served = 0 (nothing enqueued) otherwise -- the caller then acts through a promoted clone.
int pdec_policy_act_rng_as(pdec_handle actor, int state_dtype, const void* state, int cols, double act_noise, double act_limit,
                           int learning, uint64_t seed, uint64_t offset, void* actions_out, int* served) {
  GET_MLP(M, actor);
  PDEC_REQUIRE(served, "pdec_policy_act_rng_as: null");
  PDEC_REQUIRE(state_dtype == PDEC_F32 || state_dtype == PDEC_F64, "pdec_policy_act_rng_as: bad dtype %d", state_dtype);
  *served = 0;
  if (!small_act_ok(M, state_dtype, cols) || M->dtype == state_dtype) return PDEC_OK;
  PDEC_REQUIRE(state && actions_out, "pdec_policy_act_rng_as: null");
  if (learning) PDEC_REQUIRE_NOISE_COLS(M, cols, "pdec_policy_act_rng_as");
  *served = 1;
  return small_act(M, state_dtype, state, cols, act_noise, act_limit, learning, seed, offset, actions_out, nullptr, nullptr, 0);
}

int pdec_step_glue_served(pdec_handle actor, pdec_handle trajectory_handle, int dtype, int act_mode, int cols, int64_t n_rt, int* served) {
  GET_MLP(M, actor);
  Object* o = lookup(trajectory_handle);
  if (!o) { set_error("pdec_step_glue_served: bad trajectory handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(served && (dtype == PDEC_F32 || dtype == PDEC_F64), "pdec_step_glue_served: bad argument");
  *served = step_glue_served(M, o, dtype, act_mode, cols, n_rt) ? 1 : 0;
  return PDEC_OK;
}

int pdec_step_glue(pdec_handle actor, pdec_handle trajectory_handle, int dtype, const void* reward, const int32_t* done_flags,
                   int cols_per_traj, int force_terminal, void* reward_trace, void* terminal_trace, int64_t capacity,
                   int64_t start_rt, int64_t n_rt, int act_mode, const void* state, int cols, double act_noise, double act_limit,
                   uint64_t seed, uint64_t offset, void* actions_out, void* state_trace, void* action_trace,
                   int64_t capacity_rows, int64_t start_sa, int64_t n_sa, pdec_handle done_event, int* served) {
  GET_MLP(M, actor);
  Object* o = lookup(trajectory_handle);
  if (!o) { set_error("pdec_step_glue: bad trajectory handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(served, "pdec_step_glue: null");
  PDEC_REQUIRE(dtype == PDEC_F32 || dtype == PDEC_F64, "pdec_step_glue: bad dtype %d", dtype);
  PDEC_REQUIRE(act_mode >= 0 && act_mode <= 2 && n_rt >= 0 && n_sa >= 0, "pdec_step_glue: bad argument");
  *served = 0;
  // served where the three launches it stands for would be the single-workgroup ones: the few-column acting kernel of
  // pdec_policy_act_rng_as (state of another type than the networks), single-block pushes, one stream
  if (!step_glue_served(M, o, dtype, act_mode, cols, n_rt)) {
    const bool had = M->sync.wait || M->sync.done;
    M->sync = LaunchSync{};
    PDEC_REQUIRE(!had, "pdec_step_glue: a launch sync is set (pdec_set_launch_sync) and this case is not served");
    return PDEC_OK;
  }
  PDEC_REQUIRE(!n_rt || (reward && reward_trace && terminal_trace && capacity >= 1 && n_rt <= capacity && cols_per_traj >= 1 && start_rt >= 0),
               "pdec_step_glue: bad POST_ACT push");
  PDEC_REQUIRE(!n_sa || (state && state_trace && action_trace && capacity_rows >= 1 && n_sa <= capacity_rows && start_sa >= 0),
               "pdec_step_glue: bad PRE_ACT push");
  PDEC_REQUIRE(act_mode == 0 || (actions_out && (act_mode == 2 || (state && cols >= 1))), "pdec_step_glue: bad acting arguments");
  PDEC_REQUIRE(act_mode == 0 || !n_sa || n_sa == cols, "pdec_step_glue: the PRE_ACT push takes the acting call's columns");
  if (act_mode == 1) PDEC_REQUIRE_NOISE_COLS(M, cols, "pdec_step_glue");
  hipEvent_t ev = nullptr;
  if (done_event) {
    ev = pdec::event_native(done_event);
    PDEC_REQUIRE(ev, "pdec_step_glue: bad event handle");
  }
  *served = 1;
  ProfScope ps(M, "step_glue");
  // by what carries the amplitude: the call's scalar, or the arrays set on the actor (each a kernel family of its own)
  auto launch = [&](auto amp) -> int {
    using AN = decltype(amp);
    StepGlueArgsT<AN> g{};
    g.tr = (float*)reward_trace; g.tt = (float*)terminal_trace; g.r = reward; g.done = done_flags;
    g.cols_per_traj = cols_per_traj; g.force = force_terminal; g.cap_rt = capacity; g.start_rt = start_rt; g.n_rt = n_rt;
    g.act_mode = act_mode; g.state = state; g.out = actions_out;
    g.ts = (float*)state_trace; g.ta = (float*)action_trace; g.ns = M->dims[0]; g.na = M->dims[M->L];
    g.cap_sa = capacity_rows; g.start_sa = start_sa; g.n_sa = n_sa;
    g.halt = o->halt;
    g.sync = M->sync;
    M->sync = LaunchSync{};
    g.act = small_act_args<AN>(M, cols);
    g.act.learning = 1;
    g.act.p = M->params.p;
    g.act.act_noise = amp; g.act.lim = act_limit; g.act.seed = seed; g.act.offset = offset;
    const size_t lds = act_mode == 1 ? small_act_lds(M, dtype, cols) : 16;
    // (done_event rides on the launch as the completion event of its dispatch packet, like pdec_mlp_set_stop_event's)
    step_glue_dispatch<AN>(dtype, M->dtype, [&](auto kern) { hipExtLaunchKernelGGL(kern, dim3(1), dim3(256), lds, M->stream, nullptr, ev, 0, g); });
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  };
  if (act_mode == 1 && M->noise_color) return launch(noise_color_of(M, act_noise));
  return act_mode == 1 && M->noise_scale ? launch(noise_scale_of(M)) : launch(act_noise);
}

int pdec_population_glue(pdec_handle pop, int phase, const void* reward, const int32_t* done_flags, const void* state,
                         void* actions_out) {
  GET_POP(P, pop);
  PDEC_REQUIRE(phase >= 0 && phase <= 2, "pdec_population_glue: bad phase %d", phase);
  PDEC_REQUIRE(phase == 2 || !reward == !done_flags, "pdec_population_glue: reward and done flags go together");
  PDEC_REQUIRE(phase != 1 || reward, "pdec_population_glue: the time-out push needs the rewards");
  PDEC_REQUIRE(phase == 1 || state, "pdec_population_glue: null state");
  PDEC_REQUIRE(phase != 0 || actions_out, "pdec_population_glue: null actions");
  Mlp* M = P->A[0];
  const int cols = P->cols, ns = M->dims[0], na = M->dims[M->L];
  const size_t ts = dtype_size(P->dtype);
  StepGlueArgs g{};
  g.r = phase == 2 ? nullptr : reward; g.done = phase == 2 ? nullptr : done_flags;
  g.cols_per_traj = cols; g.force = phase == 1; g.cap_rt = P->cap; g.n_rt = g.r ? cols : 0;
  g.act_mode = 0; g.state = phase == 1 ? nullptr : state; g.out = phase == 0 ? actions_out : nullptr;
  g.ns = ns; g.na = na; g.cap_sa = P->cap1; g.n_sa = phase == 1 ? 0 : cols;
  g.pm = P->tab.as<PopMember>(); g.rows = P->rows; g.phase = phase;
  g.d_noise = ((long long)cols * na + 3) / 4; g.start_steps = P->start_steps;
  g.r_bytes = (size_t)cols * ts; g.s_bytes = (size_t)cols * ns * ts; g.o_bytes = (size_t)cols * na * ts;
  g.act = small_act_args(M, cols);
  g.act.learning = 1;
  const size_t lds = phase == 0 ? small_act_lds(M, P->dtype, cols) : 16;
  ProfScope ps(P, "population_glue");
  step_glue_dispatch(P->dtype, M->dtype, [&](auto kern) { hipLaunchKernelGGL(kern, dim3(P->M), dim3(256), lds, P->stream, g); });
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

static int ensure_noise_ctr(Mlp* M) {
  if (!M->noise_ctr.p) {
    PDEC_HIP(M->noise_ctr.alloc(2 * sizeof(uint64_t)));
    // blocking copy, NOT hipMemset: a memset is queued on the null stream and returns; the acting kernel runs on a
    // non-blocking stream that the null stream does not order, so on a busy device it could read the counter first
    const uint64_t zero[2] = {0, 0};
    PDEC_HIP(hipMemcpy(M->noise_ctr.p, zero, sizeof(zero), hipMemcpyHostToDevice));
    M->nc_sel = 0;
  }
  return PDEC_OK;
}

int pdec_policy_act_rng_dev(pdec_handle actor, const void* state, int cols, double act_noise, double act_limit,
                            int learning, uint64_t seed, void* actions_out) {
  GET_MLP(M, actor);
  PDEC_REQUIRE(state && actions_out && cols >= 1, "pdec_policy_act_rng_dev: null/empty");
  int rc = ensure_noise_ctr(M);
  if (rc) return rc;
  uint64_t* c = M->noise_ctr.as<uint64_t>();
  const uint64_t inc = learning ? ((uint64_t)cols * M->dims[M->L] + 3) / 4 : 0;   // counters one call consumes (4 normals each)
  rc = policy_act_rng_impl(actor, M, state, cols, act_noise, act_limit, learning, seed, 0, actions_out, c + M->nc_sel,
                           c + (M->nc_sel ^ 1), inc);
  if (rc) return rc;
  flip(M->nc_sel);
  return PDEC_OK;
}

int pdec_mlp_set_noise_scale(pdec_handle actor, const double* scale_dev, int64_t n, int cols_per_entry) {
  GET_MLP(M, actor);
  if (!scale_dev) {
    M->noise_scale = nullptr; M->noise_scale_n = 0; M->noise_scale_cpe = 1;
    return PDEC_OK;
  }
  PDEC_REQUIRE(n >= 1 && cols_per_entry >= 1 && n * cols_per_entry <= INT32_MAX, "pdec_mlp_set_noise_scale: %lld entries x %d columns",
               (long long)n, cols_per_entry);
  M->noise_scale = scale_dev; M->noise_scale_n = n; M->noise_scale_cpe = cols_per_entry;
  return PDEC_OK;
}

int pdec_mlp_set_noise_color(pdec_handle actor, double* state_dev, const double* ab_dev, int64_t n, int cols_per_entry) {
  GET_MLP(M, actor);
  if (!state_dev) {
    M->noise_color = nullptr; M->noise_color_ab = nullptr; M->noise_color_n = 0; M->noise_color_cpe = 1;
    return PDEC_OK;
  }
  PDEC_REQUIRE(n >= 1 && cols_per_entry >= 1 && n <= INT32_MAX / cols_per_entry &&
                   n * cols_per_entry <= INT32_MAX / M->dims[M->L],
               "pdec_mlp_set_noise_color: %lld entries x %d columns x %d outputs", (long long)n, cols_per_entry, M->dims[M->L]);
  PDEC_REQUIRE(ab_dev, "pdec_mlp_set_noise_color: null {a, b} array with a state array set");
  M->noise_color = state_dev; M->noise_color_ab = ab_dev; M->noise_color_n = n; M->noise_color_cpe = cols_per_entry;
  return PDEC_OK;
}

int pdec_mlp_set_noise_rows(pdec_handle actor, int rows) {
  GET_MLP(M, actor);
  PDEC_REQUIRE(rows == -1 || (rows >= 1 && rows <= M->dims[M->L]), "pdec_mlp_set_noise_rows: %d of %d outputs", rows, M->dims[M->L]);
  M->noise_rows = rows == M->dims[M->L] ? -1 : rows;
  return PDEC_OK;
}

int pdec_noise_counter_set(pdec_handle actor, uint64_t value) {
  GET_MLP(M, actor);
  int rc = ensure_noise_ctr(M);
  if (rc) return rc;
  PDEC_HIP(hipStreamSynchronize(M->stream));
  PDEC_HIP(hipMemcpy(M->noise_ctr.as<uint64_t>() + M->nc_sel, &value, sizeof(value), hipMemcpyHostToDevice));
  return PDEC_OK;
}

int pdec_noise_counter_get(pdec_handle actor, uint64_t* value) {
  GET_MLP(M, actor);
  PDEC_REQUIRE(value, "pdec_noise_counter_get: null");
  int rc = ensure_noise_ctr(M);
  if (rc) return rc;
  PDEC_HIP(hipStreamSynchronize(M->stream));
  PDEC_HIP(hipMemcpy(value, M->noise_ctr.as<uint64_t>() + M->nc_sel, sizeof(*value), hipMemcpyDeviceToHost));
  return PDEC_OK;
}

}  // extern "C"
