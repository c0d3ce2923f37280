// The episode boundary of a population on the device (include/pdeconv.h: pdec_population_episode_close,
// pdec_population_copy_best_rows; population.py: Population.run(stops, episodes_per_sync > 1)).
//
// Between two episodes of a member the host does a handful of scalar rules: PDEhook's POST_EPISODE bookkeeping
// (src/PDEhook.jl:65-97), the stop condition (src/StopCondition.jl:6-40), the agent's POST_EPISODE push and PRE_EPISODE pop
// (src/PDEagent.jl:215-252, :291-314).  Here they run on the member's book (enum PopBookSlot, population.hpp) and its counter row, so a
// block of episodes is enqueued without a read-back between them.
#include "common.hpp"
#include "population.hpp"

namespace pdec {

struct PopCloseArgs {
  long long *rows, *book, *elog;     // [M][POP_ROW], [M][POP_BOOK], this episode's [M][POP_ELOG]
  const int32_t* flags;              // [T][M] done flags of the episode's steps
  const double* means;               // [M][T] per-step means over the actuators of the rewards
  const double *log_y, *log_state;   // [T + 1][M][ysz], [T + 1][M][ssz]: slot n = behind n executed steps
  double *env_y, *env_state;         // [M][ysz], [M][ssz]
  long long ysz, ssz, cols;
  int32_t* which;                    // [M] for pdec_population_copy_actors
  int T, M, stride, reset_post, last;
};

// Phase 0, workgroup m = member m, behind the time-out push.  Thread 0 applies the scalar rules; all threads gather the final
// y and state.  Idle members (ACTIVE == 0) get a zero log entry and a zero mask, and nothing else of theirs is written.
__global__ __launch_bounds__(256) void pop_episode_close_kernel(PopCloseArgs g) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const long long* row = g.rows + (size_t)m * POP_ROW;
  long long* bk = g.book + (size_t)m * POP_BOOK;
  long long* el = g.elog + (size_t)m * POP_ELOG;
  __shared__ int n_sh;
  if (!row[POP_ACTIVE]) {            // (phase 0 writes no row, so every thread reads the same value)
    if (tid == 0) {
      el[PEL_REWARD] = 0; el[PEL_STEPS] = 0; el[PEL_NEW_BEST] = 0; el[PEL_RAN] = 0;
      bk[PBK_FIRED] = 0;
      g.which[m] = 0;
    }
    return;
  }
  if (tid == 0) {
    // run._executed_steps: up to and with the first flagged step; a flag at step T - 1 is the time-out
    int n = g.T;
    for (int t = 0; t + 1 < g.T; ++t)
      if (g.flags[(size_t)t * g.M + m] != 0) { n = t + 1; break; }
    n_sh = n;
    // run._add_episode_reward: the sequential fp64 sum of the first n means, added to hook.reward = 0.0
    const double* mu = g.means + (size_t)m * g.T;
    double acc = mu[0];
    for (int i = 1; i < n; ++i) acc = __dadd_rn(acc, mu[i]);
    const double v = __dadd_rn(0.0, acc);
    // PDEhook.end_episode (src/PDEhook.jl:65-97).  rewards_compare's maximum is Python's: max() keeps its first element
    // unless a later one compares greater, so a NaN that came first stays and nothing is >= it
    const long long ep = bk[PBK_EP];
    int new_best = 0;
    if (n == g.T && ep >= bk[PBK_MIN_BEST]) {
      double cmp = __longlong_as_double(bk[PBK_CMP]);
      if (!bk[PBK_CMP_HAS]) cmp = v;
      else if (v > cmp) cmp = v;
      bk[PBK_CMP_HAS] = 1;
      bk[PBK_CMP] = __double_as_longlong(cmp);
      if (bk[PBK_COLLECT_NNA] && v >= cmp) {
        new_best = 1;
        bk[PBK_BESTREWARD] = __double_as_longlong(v);
        bk[PBK_BESTEPISODE] = ep;
      }
    }
    bk[PBK_EP] = ep + 1;
    g.which[m] = new_best | (bk[PBK_COLLECT_NNA] ? 2 : 0);
    // run._stop_fired: the condition once per executed step, is_terminated true at the last one
    const long long cur = bk[PBK_STOP_CUR], lim = bk[PBK_STOP_LIMIT];
    int fired;
    if (bk[PBK_STOP_KIND] == 0) {    // StopAfterEpisode: cur += 1 at the end; cur >= episode at any call
      fired = cur + 1 >= lim;
      bk[PBK_STOP_CUR] = cur + 1;
    } else {                         // StopAfterEpisodeWithMinSteps (src/StopCondition.jl:31): cur >= step at the last call
      fired = cur + n - 1 >= lim;
      bk[PBK_STOP_CUR] = cur + n;
    }
    bk[PBK_FIRED] = fired;
    el[PEL_REWARD] = __double_as_longlong(v); el[PEL_STEPS] = n; el[PEL_NEW_BEST] = new_best; el[PEL_RAN] = 1;
  }
  __syncthreads();
  const size_t n = (size_t)n_sh;
  const double* sy = g.log_y + (n * g.M + m) * g.ysz;
  const double* ss = g.log_state + (n * g.M + m) * g.ssz;
  double* dy = g.env_y + (size_t)m * g.ysz;
  double* ds = g.env_state + (size_t)m * g.ssz;
  for (long long i = tid; i < g.ysz; i += 256) dy[i] = sy[i];
  for (long long i = tid; i < g.ssz; i += 256) ds[i] = ss[i];
}

// Phase 1, thread m = member m, behind the POST_EPISODE push (pdec_population_glue phase 2, which reads NSA and ACTIVE as the
// episode had them): the counters move as the host moves them at the boundary.
__global__ __launch_bounds__(256) void pop_episode_next_kernel(PopCloseArgs g) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= g.M) return;
  long long* row = g.rows + (size_t)m * POP_ROW;
  long long* bk = g.book + (size_t)m * POP_BOOK;
  if (!row[POP_ACTIVE]) return;
  row[POP_NSA] += g.cols;                                   // Agent.end_episode: the dummy (s, a) went in
  if (g.reset_post) row[POP_USTEP] = 0;
  if (bk[PBK_RANDOM_INIT]) bk[PBK_INIT_OFF] += bk[PBK_INIT_INC];   // the field this episode began from is consumed
  if (bk[PBK_FIRED]) {
    row[POP_ACTIVE] = 0;
    row[POP_HALT] = 1;
    return;
  }
  row[POP_HALT] = 0;
  // PRE_EPISODE of the next episode (src/PDEagent.jl:237-252); behind a block's last episode it is the host's
  if (!g.last && row[POP_NSA] > row[POP_NRT]) row[POP_NSA] -= g.stride;
}

// n rows of sz doubles: dst[t][c] = src[t * src_step + c], by the threads of grid row blockIdx.y; 16 bytes per access where
// the row length and both addresses allow
__device__ __forceinline__ void best_rows(double* __restrict__ dst, const double* __restrict__ src, long long n, long long sz,
                                          long long src_step) {
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, nt = (long long)gridDim.x * 256;
  const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst);
  if (((sz | src_step) & 1) == 0 && ((as | ad) & 15) == 0) {
    const long long h = sz >> 1, hs = src_step >> 1;
    const double2* s2 = reinterpret_cast<const double2*>(src);
    double2* d2 = reinterpret_cast<double2*>(dst);
    for (long long i = t0; i < n * h; i += nt) {
      const long long t = i / h, c = i - t * h;
      d2[i] = s2[t * hs + c];
    }
    return;
  }
  for (long long i = t0; i < n * sz; i += nt) {
    const long long t = i / sz, c = i - t * sz;
    dst[i] = src[t * src_step + c];
  }
}

struct PopBestArgs {
  const int32_t* which;
  const long long* elog;             // this episode's [M][POP_ELOG]
  const double *la, *lp, *ly, *lr;   // the episode's logs: action [T + 1][M][asz], p [T][M][psz], y [T + 1][M][ysz], reward [T][M][rsz]
  double *ba, *bp, *by, *br;         // best rows [M][T][...]
  long long asz, psz, ysz, rsz;
  int T, M;
};
// member blockIdx.y with a new best: the rows PDEhook logs for its n steps -- action[1..n], p[0..n-1], y[1..n], reward[0..n-1]
__global__ __launch_bounds__(256) void pop_copy_best_rows_kernel(PopBestArgs g) {
  const int m = blockIdx.y;
  if (!(g.which[m] & 1)) return;
  long long n = g.elog[(size_t)m * POP_ELOG + PEL_STEPS];
  n = n < 0 ? 0 : (n > g.T ? g.T : n);
  const size_t M = (size_t)g.M, T = (size_t)g.T;
  best_rows(g.ba + m * T * g.asz, g.la + (M + m) * g.asz, n, g.asz, M * g.asz);
  best_rows(g.bp + m * T * g.psz, g.lp + (size_t)m * g.psz, n, g.psz, M * g.psz);
  best_rows(g.by + m * T * g.ysz, g.ly + (M + m) * g.ysz, n, g.ysz, M * g.ysz);
  best_rows(g.br + m * T * g.rsz, g.lr + (size_t)m * g.rsz, n, g.rsz, M * g.rsz);
}

}  // namespace pdec

using namespace pdec;

extern "C" {

int pdec_population_episode_close(pdec_handle pop, int phase, int64_t* book, int64_t* elog, const int32_t* flags,
                                  const double* means, int T, const void* log_y, const void* log_state, void* env_y,
                                  void* env_state, int64_t y_elems, int64_t state_elems, int32_t* which, int reset_post, int last) {
  GET_POP(P, pop);
  PDEC_REQUIRE(phase == 0 || phase == 1, "pdec_population_episode_close: bad phase %d", phase);
  PDEC_REQUIRE(book, "pdec_population_episode_close: null book");
  PDEC_REQUIRE(P->dtype == PDEC_F64, "pdec_population_episode_close: fp64 environments only");
  PopCloseArgs g{};
  g.rows = P->rows; g.book = (long long*)book; g.M = P->M; g.cols = P->cols; g.stride = P->stride;
  g.reset_post = reset_post != 0; g.last = last != 0;
  if (phase == 1) {
    ProfScope ps(P, "population_episode_next");
    hipLaunchKernelGGL(pop_episode_next_kernel, dim3((unsigned)((P->M + 255) / 256)), dim3(256), 0, P->stream, g);
    PDEC_HIP(hipGetLastError());
    return PDEC_OK;
  }
  PDEC_REQUIRE(elog && flags && means && log_y && log_state && env_y && env_state && which,
               "pdec_population_episode_close: null argument");
  PDEC_REQUIRE(T >= 1 && y_elems >= 1 && state_elems >= 1, "pdec_population_episode_close: bad size (T %d, %lld, %lld)", T,
               (long long)y_elems, (long long)state_elems);
  g.elog = (long long*)elog; g.flags = flags; g.means = means; g.T = T;
  g.log_y = (const double*)log_y; g.log_state = (const double*)log_state;
  g.env_y = (double*)env_y; g.env_state = (double*)env_state; g.ysz = y_elems; g.ssz = state_elems; g.which = which;
  ProfScope ps(P, "population_episode_close");
  hipLaunchKernelGGL(pop_episode_close_kernel, dim3((unsigned)P->M), dim3(256), 0, P->stream, g);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_population_copy_best_rows(pdec_handle pop, const int32_t* which, const int64_t* elog, int T, const void* log_action,
                                   const void* log_p, const void* log_y, const void* log_reward, void* best_action, void* best_p,
                                   void* best_y, void* best_reward, int64_t action_elems, int64_t p_elems, int64_t y_elems,
                                   int64_t reward_elems) {
  GET_POP(P, pop);
  PDEC_REQUIRE(which && elog && log_action && log_p && log_y && log_reward && best_action && best_p && best_y && best_reward,
               "pdec_population_copy_best_rows: null argument");
  PDEC_REQUIRE(P->dtype == PDEC_F64, "pdec_population_copy_best_rows: fp64 environments only");
  PDEC_REQUIRE(T >= 1 && action_elems >= 1 && p_elems >= 1 && y_elems >= 1 && reward_elems >= 1,
               "pdec_population_copy_best_rows: bad size");
  PopBestArgs g{};
  g.which = which; g.elog = (const long long*)elog; g.T = T; g.M = P->M;
  g.la = (const double*)log_action; g.lp = (const double*)log_p; g.ly = (const double*)log_y; g.lr = (const double*)log_reward;
  g.ba = (double*)best_action; g.bp = (double*)best_p; g.by = (double*)best_y; g.br = (double*)best_reward;
  g.asz = action_elems; g.psz = p_elems; g.ysz = y_elems; g.rsz = reward_elems;
  // one 16-byte access per thread and trip over the longest array of a member, at most ~2048 workgroups in all
  const long long most = (long long)T * std::max(std::max(action_elems, p_elems), std::max(y_elems, reward_elems));
  const long long want = (most / 2 + 255) / 256, cap = std::max<long long>(1, 2048 / (long long)P->M);
  const dim3 grid((unsigned)std::max<long long>(1, std::min(want, cap)), (unsigned)P->M);
  ProfScope ps(P, "population_copy_best_rows");
  hipLaunchKernelGGL(pop_copy_best_rows_kernel, grid, dim3(256), 0, P->stream, g);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

}  // extern "C"
