// ddpg.hip -- the DDPG update of an actor / critic pair (RLBase.update!(policy, batch), src/PDEagent.jl:363-418): the generic
// critic and actor passes on the Mlp methods with their loss kernels, reward groups, and the routing of every pass, apply and
// report to the fused family that serves it (FusedFamily, mlp.hpp) or to the generic path.  Also the batch-mean reward as a
// launch of its own (rmean_kernel), which both fused families and the producer of r use.
#include "common.hpp"
#include "mlp.hpp"
#include "mfma_blocks.hpp"     // f32x4

namespace pdec {

// ---- DDPG loss statistics (single block; deterministic)
// stats[0..4] = mean(c), mean(c^2), mean(r), mean(r^2), mean(q) with c_i = gamma(1-t_i)qt_i - q_i
template <class T>
__global__ void ddpg_stats_kernel(const T* __restrict__ q, const T* __restrict__ qt, const T* __restrict__ r,
                                  const T* __restrict__ t, int n, T gamma, T* __restrict__ stats) {
  __shared__ double red[5][256];
  const int tid = threadIdx.x;
  double a[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += 256) {
    const T qi = q[i];
    a[4] += (double)qi;
    if (qt) {
      const T c = gamma * ((T)1 - t[i]) * qt[i] - qi;
      a[0] += (double)c;
      a[1] += (double)c * (double)c;
      a[2] += (double)r[i];
      a[3] += (double)r[i] * (double)r[i];
    }
  }
  for (int k = 0; k < 5; ++k) red[k][tid] = a[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid < 5) stats[tid] = (T)(red[tid][0] / n);
}

// critic: dq_i = -(2/Bu)(rr + c_i) * scale with rr = mean(r) (quirk) or r_i; writes dz of the
// (identity) output layer directly; loss -> *loss_out
template <class T>
__global__ void ddpg_critic_dq_kernel(const T* __restrict__ q, const T* __restrict__ qt, const T* __restrict__ r,
                                      const T* __restrict__ t, int n, T gamma, int quirk, const T* __restrict__ stats,
                                      T* __restrict__ dq, T* __restrict__ loss_out, const T* __restrict__ loss_add) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && loss_out) {
    // quirk: mean_ij (r_j + c_i)^2 = mean(c^2) + 2 mean(c) mean(r) + mean(r^2); loss_add: reward groups (reward_group_route)
    *loss_out = quirk ? stats[1] + (T)2 * stats[0] * stats[2] + stats[3] : stats[5] + (loss_add ? *loss_add : (T)0);
  }
  if (i >= n) return;
  const T c = gamma * ((T)1 - t[i]) * qt[i] - q[i];
  const T rr = quirk ? stats[2] : r[i];
  dq[i] = -((T)2 / (T)n) * (rr + c);
}
// diagonal loss needs mean((r_i + c_i)^2): stats[5]
template <class T>
__global__ void ddpg_diag_loss_kernel(const T* __restrict__ q, const T* __restrict__ qt, const T* __restrict__ r,
                                      const T* __restrict__ t, int n, T gamma, T* __restrict__ stats) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double a = 0;
  for (int i = tid; i < n; i += 256) {
    const T e = r[i] + gamma * ((T)1 - t[i]) * qt[i] - q[i];
    a += (double)e * (double)e;
  }
  red[tid] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) stats[5] = (T)(red[0] / n);
}
template <class T>
__global__ void fill_kernel(T* __restrict__ p, int n, T v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
template <class T>
__global__ void neg_copy_kernel(T* __restrict__ dst, const T* __restrict__ src) { *dst = -*src; }

// mean of r in a fixed order (one block): the batch-mean reward of the reference's (1xBu).+(Bu) broadcast
__global__ __launch_bounds__(1024) void rmean_kernel(const float* __restrict__ r, int n, float* __restrict__ out) {
  __builtin_amdgcn_s_setprio(3);      // one short block; beside the update passes (priority 2) it would otherwise starve
  __shared__ float part[1024];
  const int tid = threadIdx.x;
  float acc = 0.f;
  const int n4 = ((reinterpret_cast<uintptr_t>(r) & 15) == 0) ? n / 4 : 0;
  const f32x4* r4 = reinterpret_cast<const f32x4*>(r);
  int i = tid;
  for (; i + 7 * 1024 < n4; i += 8 * 1024) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = r4[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
  }
  for (; i < n4; i += 1024) { const f32x4 v = r4[i]; acc += (v[0] + v[1]) + (v[2] + v[3]); }
  for (int k = 4 * n4 + tid; k < n; k += 1024) acc += r[k];
  part[tid] = acc;
  __syncthreads();
  for (int sft = 512; sft > 0; sft >>= 1) {
    if (tid < sft) part[tid] += part[tid + sft];
    __syncthreads();
  }
  if (tid == 0) out[0] = part[0] / (float)n;
}

}  // namespace pdec

using namespace pdec;

// ------------------------------------------------------------------ DDPG
// Reward groups (pdec_ddpg_set_reward_groups): column c belongs to group (c / (g L)) L + c % L, whose members are the
// columns base + k L, k = 0 .. g-1, base = (c / (g L)) g L + c % L.  rg[c] = (sum over k in that order) / g -- every
// column of a group sums the same values in the same order, so all of them hold the same mean -- and
// corr = mean_c (r_c - rg[c])^2 (= mean(r^2) - mean(rg^2)): the per-block partials (fixed tree, double) are added in block
// order by the block that finishes last, which resets the counter for the next launch (graph replays included).
#define RG_THREADS 256
template <class T>
__global__ __launch_bounds__(RG_THREADS) void reward_group_mean_kernel(const T* __restrict__ r, int n, int g, int L,
                                                                        T* __restrict__ rg, double* __restrict__ part,
                                                                        unsigned* __restrict__ counter) {
  __shared__ double red[RG_THREADS];
  __shared__ bool last;
  const int tid = threadIdx.x, c = blockIdx.x * RG_THREADS + tid;
  double e = 0.0;
  if (c < n) {
    const int gl = g * L, base = (c / gl) * gl + c % L;
    T sum = r[base];
    for (int k = 1; k < g; ++k) sum += r[base + k * L];
    const T m = sum / (T)g;
    rg[c] = m;
    const T d = r[c] - m;
    e = (double)d * (double)d;
  }
  red[tid] = e;
  __syncthreads();
  for (int s = RG_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x] = red[0];
    __threadfence();
    last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  double a = 0.0;
  for (int b = tid; b < (int)gridDim.x; b += RG_THREADS) a += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  red[tid] = a;
  __syncthreads();
  for (int s = RG_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    rg[n] = (T)(red[0] / n);
    *counter = 0u;
  }
}

int pdec::reward_group_route(Mlp* C, const void* r, int Bu, int quirk, CriticRoute* out) {
  *out = CriticRoute{r, quirk, nullptr};
  const int g = C->rg_g, L = C->rg_L;
  if (!quirk || g == 0) return PDEC_OK;
  if (g == 1) {                                   // groups of one column: the diagonal TD target
    out->quirk = 0;
    return PDEC_OK;
  }
  if ((int64_t)g * L >= Bu) return PDEC_OK;        // one group spans the batch: the whole-batch broadcast
  PDEC_REQUIRE(Bu % (g * L) == 0,
               "reward groups: the batch of %d columns is not a whole number of g x L = %d x %d column blocks", Bu, g, L);
  const size_t ts = dtype_size(C->dtype);
  const int nblk = cdiv(Bu, RG_THREADS);
  if (C->rg_vals.bytes < (size_t)(Bu + 1) * ts) PDEC_HIP(C->rg_vals.alloc((size_t)(Bu + 1) * ts));
  const size_t work = (size_t)nblk * 8 + 8;
  if (C->rg_work.bytes < work) {
    PDEC_HIP(C->rg_work.alloc(work));
    PDEC_HIP(hipMemset(C->rg_work.p, 0, work));   // the last-block counter starts (and every launch leaves it) at zero
    PDEC_HIP(hipDeviceSynchronize());
  }
  double* part = C->rg_work.as<double>();
  unsigned* counter = (unsigned*)(C->rg_work.as<char>() + C->rg_work.bytes - 8);
  {
    ProfScope ps(C, "ddpg_reward_groups");
    if (C->dtype == PDEC_F64)
      hipLaunchKernelGGL((reward_group_mean_kernel<double>), dim3(nblk), dim3(RG_THREADS), 0, C->stream, (const double*)r, Bu, g,
                         L, C->rg_vals.as<double>(), part, counter);
    else
      hipLaunchKernelGGL((reward_group_mean_kernel<float>), dim3(nblk), dim3(RG_THREADS), 0, C->stream, (const float*)r, Bu, g, L,
                         C->rg_vals.as<float>(), part, counter);
    PDEC_HIP(hipGetLastError());
  }
  out->r = C->rg_vals.p;
  out->quirk = 0;
  out->loss_add = C->rg_vals.as<char>() + (size_t)Bu * ts;
  return PDEC_OK;
}

int pdec::launch_rmean(Mlp* C, const float* r, int n, float** out) {
  float* rb = C->scratch.as<float>() + 40;      // device scalar behind the generic path's statistics and losses
  ProfScope ps(C, "ddpg_rmean");
  hipLaunchKernelGGL(rmean_kernel, dim3(1), dim3(1024), 0, C->stream, r, n, rb);
  PDEC_HIP(hipGetLastError());
  *out = rb;
  return PDEC_OK;
}

template <class T>
static int critic_grads_t(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                          const void* snext, int Bu, double gamma, int quirk, double grad_scale, void* loss_dev,
                          const void* loss_add) {
  const int ns = At->dims[0], na = At->dims[At->L];
  PDEC_REQUIRE(C->dims[0] == ns + na && Ct->dims[0] == ns + na && C->dims[C->L] == 1 && Ct->dims[Ct->L] == 1,
               "ddpg: critic must map ns+na -> 1");
  int rc;
  // a' = At(s')                                              src/PDEagent.jl:385
  if ((rc = At->pack(snext, ns, 0, nullptr, 0, 0, Bu))) return rc;
  if ((rc = At->forward(Bu))) return rc;
  // qt = Ct(vcat(s', a'))                                    :386
  if (At->stream != Ct->stream) PDEC_HIP(hipStreamSynchronize(At->stream));
  if ((rc = Ct->pack(snext, ns, 0, At->H[At->L].p, na, 1, Bu))) return rc;
  if ((rc = Ct->forward(Bu))) return rc;
  // q = C(vcat(s, a))                                        :392
  if (Ct->stream != C->stream) PDEC_HIP(hipStreamSynchronize(Ct->stream));
  if ((rc = C->pack(s, ns, 0, a, na, 0, Bu))) return rc;
  if ((rc = C->forward(Bu))) return rc;
  T* stats = C->scratch.as<T>();
  const T* q = C->H[C->L].as<T>();
  const T* qt = Ct->H[Ct->L].as<T>();
  // gamma is Float32 in the reference (y = 0.99f0, KSSetup.jl:64)
  const T gm = (T)(float)gamma;
  {
    ProfScope ps(C, "ddpg_loss");
    hipLaunchKernelGGL((ddpg_stats_kernel<T>), dim3(1), dim3(256), 0, C->stream, q, qt, (const T*)r, (const T*)t, Bu, gm, stats);
    if (!quirk)
      hipLaunchKernelGGL((ddpg_diag_loss_kernel<T>), dim3(1), dim3(256), 0, C->stream, q, qt, (const T*)r, (const T*)t, Bu, gm, stats);
    // dq goes straight into dz of the identity output layer (feature-major [1][Bu])
    hipLaunchKernelGGL((ddpg_critic_dq_kernel<T>), dim3(cdiv(Bu, 256)), dim3(256), 0, C->stream, q, qt, (const T*)r, (const T*)t, Bu,
                       gm, quirk, stats, C->dy_buf<T>(Bu), (T*)loss_dev, (const T*)loss_add);
    PDEC_HIP(hipGetLastError());
  }
  return C->backward(C->dy_buf<T>(Bu), 1, Bu, true, false, grad_scale);
}

template <class T>
static int actor_grads_t(Mlp* A, Mlp* C, const void* s, int Bu, double grad_scale, void* loss_dev) {
  const int ns = A->dims[0], na = A->dims[A->L];
  int rc;
  if ((rc = A->pack(s, ns, 0, nullptr, 0, 0, Bu))) return rc;
  if ((rc = A->forward(Bu))) return rc;
  if (A->stream != C->stream) PDEC_HIP(hipStreamSynchronize(A->stream));
  if ((rc = C->pack(s, ns, 0, A->H[A->L].p, na, 1, Bu))) return rc;
  if ((rc = C->forward(Bu))) return rc;
  T* stats = C->scratch.as<T>();
  {
    ProfScope ps(C, "ddpg_loss");
    hipLaunchKernelGGL((ddpg_stats_kernel<T>), dim3(1), dim3(256), 0, C->stream, C->H[C->L].as<T>(), (const T*)nullptr,
                       (const T*)nullptr, (const T*)nullptr, Bu, (T)0, stats);
    if (loss_dev) hipLaunchKernelGGL((neg_copy_kernel<T>), dim3(1), dim3(1), 0, C->stream, (T*)loss_dev, stats + 4);
    hipLaunchKernelGGL((fill_kernel<T>), dim3(cdiv(Bu, 256)), dim3(256), 0, C->stream, C->dy_buf<T>(Bu), Bu, (T)(-1.0 / Bu));
    PDEC_HIP(hipGetLastError());
  }
  // d(-mean q)/d[s;a] through the critic, no critic weight gradients   :402-409
  if ((rc = C->backward(C->dy_buf<T>(Bu), 1, Bu, false, true, 1.0))) return rc;
  if (A->stream != C->stream) PDEC_HIP(hipStreamSynchronize(C->stream));
  const T* dA = C->dz[C->dx_index].as<T>() + (size_t)ns * Bu;  // rows ns.. of dX0 = gradient w.r.t. A(s)
  return A->backward(dA, 1, Bu, true, false, grad_scale);
}

// ---- the fused families (mlp.hpp).  They are disjoint (L == 3 / L == 2), so the order decides nothing; it is fixed all the same.
static const FusedFamily* const fused_families[] = {&fused3_family, &fused2_family};
const FusedFamily* pdec::fused_family_of_pair(const Mlp* A, const Mlp* C) {
  for (const FusedFamily* f : fused_families)
    if (f->pair_ok(A, C)) return f;
  return nullptr;
}
const FusedFamily* pdec::fused_family_of_net(const Mlp* M) {
  for (const FusedFamily* f : fused_families)
    if (f->net_ok(M)) return f;
  return nullptr;
}
const FusedFamily* pdec::fused_family_of_act(const Mlp* M, int cols) {
  for (const FusedFamily* f : fused_families)
    if (f->act_ok(M, cols)) return f;
  return nullptr;
}
// Which family serves the pass of a pair, or null: the generic fp32 / fp64 launch sequence.  one_stream: the networks the pass
// touches all run on the critic's stream.
static const FusedFamily* pass_family(const Mlp* A, const Mlp* C, bool one_stream) {
  return one_stream ? fused_family_of_pair(A, C) : nullptr;
}
// pdec_ddpg_update_async applies ADAM + Polyak inside the finish launch of a fused pass (4 launches); below the family's
// apply_min_bu columns the passes are the same kernels and ADAM / Polyak are launches of their own
static bool update_applies_in_finish(const FusedFamily* fam, int Bu) { return fam && Bu >= fam->apply_min_bu; }

// the critic pass on arguments reward_group_route has already settled (loss_add: its loss correction, or null)
static int critic_grads_routed(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                               const void* snext, int Bu, double gamma, int quirk, double grad_scale, void* critic_loss_dev,
                               const void* loss_add) {
  int rc;
  const FusedFamily* fam = pass_family(A, C, A->stream == C->stream && At->stream == C->stream && Ct->stream == C->stream);
  if (fam)
    rc = fam->critic_grads(A, C, At, Ct, s, a, r, t, snext, Bu, (double)(float)gamma, quirk, grad_scale, critic_loss_dev, nullptr,
                           loss_add);
  else
    rc = C->dtype == PDEC_F64
             ? critic_grads_t<double>(A, C, At, Ct, s, a, r, t, snext, Bu, gamma, quirk, grad_scale, critic_loss_dev, loss_add)
             : critic_grads_t<float>(A, C, At, Ct, s, a, r, t, snext, Bu, gamma, quirk, grad_scale, critic_loss_dev, loss_add);
  if (rc == PDEC_OK && C->reduce_event) {     // see pdec_ddpg_actor_grads
    PDEC_HIP(hipEventRecord(C->reduce_event, C->stream));
    C->reduce_event = nullptr;
  }
  return rc;
}

extern "C" {

int pdec_ddpg_critic_grads(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* s,
                           const void* a, const void* r, const void* t, const void* snext, int Bu, double gamma,
                           int quirk, double grad_scale, void* critic_loss_dev) {
  GET_MLP(A, hA);
  GET_MLP(C, hC);
  GET_MLP(At, hAt);
  GET_MLP(Ct, hCt);
  PDEC_REQUIRE(s && a && r && t && snext && Bu >= 1, "pdec_ddpg_critic_grads: null/empty batch");
  PDEC_REQUIRE(A->dtype == C->dtype && At->dtype == C->dtype && Ct->dtype == C->dtype, "ddpg: dtype mismatch");
  PDEC_REQUIRE(At->dims == A->dims && Ct->dims == C->dims, "ddpg: target networks must have the behaviour networks' shapes");
  CriticRoute rt;
  int rc = reward_group_route(C, r, Bu, quirk, &rt);
  if (rc) return rc;
  return critic_grads_routed(A, C, At, Ct, s, a, rt.r, t, snext, Bu, gamma, rt.quirk, grad_scale, critic_loss_dev, rt.loss_add);
}

int pdec_ddpg_set_reward_groups(pdec_handle critic, int g, int L) {
  GET_MLP(C, critic);
  PDEC_REQUIRE(g >= 0 && L >= 1, "pdec_ddpg_set_reward_groups: needs g >= 0 (0: off) and L >= 1 (got g = %d, L = %d)", g, L);
  C->rg_g = g;
  C->rg_L = g ? L : 1;
  return PDEC_OK;
}

// batch-mean reward as its own (fixed-order, one block) reduction on the caller's stream: the producer of r -- the env
// step -- reduces it beside the update, which then reads one scalar instead of every workgroup summing all of r
int pdec_reward_mean(pdec_handle any_handle, const void* r, int n, void* mean_out) {
  Object* o = lookup(any_handle);
  if (!o) { set_error("pdec_reward_mean: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(r && mean_out && n >= 1, "pdec_reward_mean: null/empty");
  ProfScope ps(o, "ddpg_rmean");
  hipLaunchKernelGGL(rmean_kernel, dim3(1), dim3(1024), 0, o->stream, (const float*)r, n, (float*)mean_out);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

int pdec_ddpg_set_reward_partials(pdec_handle critic, const void* partial_sums, int n) {
  Mlp* C = lookup_as<Mlp>(critic, Kind::Mlp);
  if (!C) { set_error("pdec_ddpg_set_reward_partials: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(C->dtype == PDEC_F32 && n >= 0, "pdec_ddpg_set_reward_partials: fp32 critics only");
  PDEC_REQUIRE(partial_sums == nullptr || fused_net_supported(C), "pdec_ddpg_set_reward_partials: 3-layer fused critics only");
  C->rpart_ext = (const float*)partial_sums;
  C->rpart_n = n;
  return PDEC_OK;
}

int pdec_ddpg_set_reward_mean(pdec_handle critic, const void* mean_dev) {
  Mlp* C = lookup_as<Mlp>(critic, Kind::Mlp);
  if (!C) { set_error("pdec_ddpg_set_reward_mean: bad handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(C->dtype == PDEC_F32, "pdec_ddpg_set_reward_mean: fp32 critics only");
  C->rbar_ext = mean_dev;
  return PDEC_OK;
}

int pdec_ddpg_actor_grads(pdec_handle hA, pdec_handle hC, const void* s, int Bu, double grad_scale, void* actor_loss_dev) {
  GET_MLP(A, hA);
  GET_MLP(C, hC);
  PDEC_REQUIRE(s && Bu >= 1, "pdec_ddpg_actor_grads: null/empty batch");
  PDEC_REQUIRE(A->dtype == C->dtype, "ddpg: dtype mismatch");
  int rc;
  const FusedFamily* fam = pass_family(A, C, A->stream == C->stream);
  if (fam) rc = fam->actor_grads(A, C, nullptr, s, Bu, grad_scale, actor_loss_dev, nullptr);
  else rc = C->dtype == PDEC_F64 ? actor_grads_t<double>(A, C, s, Bu, grad_scale, actor_loss_dev)
                                 : actor_grads_t<float>(A, C, s, Bu, grad_scale, actor_loss_dev);
  // a reduce event (pdec_mlp_set_reduce_event) that the path taken did not put on its reduction launch: recorded behind it
  if (rc == PDEC_OK && A->reduce_event) {
    PDEC_HIP(hipEventRecord(A->reduce_event, A->stream));
    A->reduce_event = nullptr;
  }
  return rc;
}

int pdec_ddpg_update(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* s, const void* a,
                     const void* r, const void* t, const void* snext, int Bu, double gamma, double rho, int quirk,
                     double eta_actor, double eta_critic, double* actor_loss, double* critic_loss) {
  GET_MLP(C, hC);
  GET_MLP(A, hA);
  const size_t ts = dtype_size(C->dtype);
  char* losses = C->scratch.as<char>() + 16 * ts;  // two device scalars behind the stats
  int rc = pdec_ddpg_critic_grads(hA, hC, hAt, hCt, s, a, r, t, snext, Bu, gamma, quirk, 1.0, losses);
  if (rc) return rc;
  if ((rc = pdec_adam_step(hC, eta_critic, 0.9, 0.999, 1e-8))) return rc;           // :400
  if ((rc = pdec_ddpg_actor_grads(hA, hC, s, Bu, 1.0, losses + ts))) return rc;
  if (A->stream != C->stream) PDEC_HIP(hipStreamSynchronize(C->stream));
  if ((rc = pdec_adam_step(hA, eta_actor, 0.9, 0.999, 1e-8))) return rc;            // :412
  if ((rc = pdec_polyak(hAt, hA, rho))) return rc;                                  // :415-417
  if ((rc = pdec_polyak(hCt, hC, rho))) return rc;
  if (actor_loss || critic_loss) {
    unsigned char buf[16];
    PDEC_HIP(hipStreamSynchronize(A->stream));
    PDEC_HIP(hipMemcpyAsync(buf, losses, 2 * ts, hipMemcpyDeviceToHost, C->stream));
    PDEC_HIP(hipStreamSynchronize(C->stream));
    if (C->dtype == PDEC_F64) {
      if (critic_loss) *critic_loss = ((double*)buf)[0];
      if (actor_loss) *actor_loss = ((double*)buf)[1];
    } else {
      if (critic_loss) *critic_loss = ((float*)buf)[0];
      if (actor_loss) *actor_loss = ((float*)buf)[1];
    }
  }
  return PDEC_OK;
}

int pdec_adam_polyak_step(pdec_handle h, pdec_handle h_target, double eta, double beta1, double beta2, double eps,
                          double rho) {
  GET_MLP(M, h);
  Mlp* T = lookup_as<Mlp>(h_target, Kind::Mlp);
  if (!T) { set_error("pdec_adam_polyak_step: bad target handle"); return PDEC_E_HANDLE; }
  PDEC_REQUIRE(T->dims == M->dims && T->dtype == M->dtype, "pdec_adam_polyak_step: shape/dtype mismatch");
  if (const FusedFamily* fam = M->stream == T->stream ? fused_family_of_net(M) : nullptr) {
    const AdamPolyak ap{eta, beta1, beta2, eps, rho};
    return fam->adam_polyak(M, T, ap);
  }
  int rc = pdec_adam_step(h, eta, beta1, beta2, eps);
  if (rc) return rc;
  if (M->stream != T->stream) PDEC_HIP(hipStreamSynchronize(M->stream));
  return pdec_polyak(h_target, h, rho);
}

// phase bit 0: critic half (critic pass, reduce + ADAM(C) + Polyak(Ct)); bit 1: actor half (actor pass with the
// updated critic, reduce + ADAM(A) + Polyak(At)).  The split lets a caller order the actor half behind a
// concurrent reader of the actor's weights (e.g. the acting kernel of the same control step on another stream).
static int ddpg_update_phases(int phase, pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* s,
                              const void* a, const void* r, const void* t, const void* snext, int Bu, double gamma,
                              double rho, int quirk, double eta_actor, double eta_critic, void* losses_dev) {
  GET_MLP(A, hA);
  GET_MLP(C, hC);
  GET_MLP(At, hAt);
  GET_MLP(Ct, hCt);
  PDEC_REQUIRE(s && Bu >= 1, "pdec_ddpg_update_async: null/empty batch");
  PDEC_REQUIRE(!(phase & 1) || (a && r && t && snext), "pdec_ddpg_update_async: null batch array");
  PDEC_REQUIRE(A->dtype == C->dtype && At->dtype == C->dtype && Ct->dtype == C->dtype, "ddpg: dtype mismatch");
  PDEC_REQUIRE(At->dims == A->dims && Ct->dims == C->dims, "ddpg: target networks must have the behaviour networks' shapes");
  const size_t ts = dtype_size(C->dtype);
  char* l0 = (char*)losses_dev;
  char* l1 = l0 ? l0 + ts : nullptr;
  const bool one_stream = A->stream == C->stream && At->stream == C->stream && Ct->stream == C->stream;
  int rc;
  const void* loss_add = nullptr;
  if (phase & 1) {          // reward groups: routed once here (the generic branch below hands the routed arguments on unchanged)
    CriticRoute rt;
    if ((rc = reward_group_route(C, r, Bu, quirk, &rt))) return rc;
    r = rt.r;
    quirk = rt.quirk;
    loss_add = rt.loss_add;
  }
  const FusedFamily* fam = pass_family(A, C, one_stream);
  if (update_applies_in_finish(fam, Bu)) {
    // 4 launches: critic pass, reduce+ADAM(C)+Polyak(Ct), actor pass (updated critic), reduce+ADAM(A)+Polyak(At)
    const AdamPolyak apc{eta_critic, 0.9, 0.999, 1e-8, rho}, apa{eta_actor, 0.9, 0.999, 1e-8, rho};
    if ((phase & 1) &&
        (rc = fam->critic_grads(A, C, At, Ct, s, a, r, t, snext, Bu, (double)(float)gamma, quirk, 1.0, l0, &apc, loss_add)))
      return rc;
    if (phase & 2) return fam->actor_grads(A, C, At, s, Bu, 1.0, l1, &apa);
    return PDEC_OK;
  }
  // ADAM + Polyak through pdec_adam_polyak_step, the entry the data-parallel split sequence calls behind its all-reduce: a
  // network that entry updates with the fused families' fp32 apply kernel (any fp32 2-layer net, a 3-layer net with an image)
  // is updated by the same kernel here, so one GPU and several leave the same bits on every shape (the generic pdec_adam_step
  // rounds once from double: a last-bit difference from the second step on)
  if (phase & 1) {
    if ((rc = critic_grads_routed(A, C, At, Ct, s, a, r, t, snext, Bu, gamma, quirk, 1.0, l0, loss_add))) return rc;
    if ((rc = pdec_adam_polyak_step(hC, hCt, eta_critic, 0.9, 0.999, 1e-8, rho))) return rc;      // :400, :415-417 (critic pair)
  }
  if (phase & 2) {
    if ((rc = pdec_ddpg_actor_grads(hA, hC, s, Bu, 1.0, l1))) return rc;
    if (A->stream != C->stream) PDEC_HIP(hipStreamSynchronize(C->stream));
    if ((rc = pdec_adam_polyak_step(hA, hAt, eta_actor, 0.9, 0.999, 1e-8, rho))) return rc;       // :412, :415-417 (actor pair)
  }
  return PDEC_OK;
}

int pdec_ddpg_update_async(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* s,
                           const void* a, const void* r, const void* t, const void* snext, int Bu, double gamma,
                           double rho, int quirk, double eta_actor, double eta_critic, void* losses_dev) {
  return ddpg_update_phases(3, hA, hC, hAt, hCt, s, a, r, t, snext, Bu, gamma, rho, quirk, eta_actor, eta_critic, losses_dev);
}
int pdec_ddpg_update_critic_async(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* s,
                                  const void* a, const void* r, const void* t, const void* snext, int Bu, double gamma,
                                  double rho, int quirk, double eta_critic, void* losses_dev) {
  return ddpg_update_phases(1, hA, hC, hAt, hCt, s, a, r, t, snext, Bu, gamma, rho, quirk, 0.0, eta_critic, losses_dev);
}
int pdec_ddpg_update_actor_async(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, const void* s, int Bu,
                                 double rho, double eta_actor, void* losses_dev) {
  return ddpg_update_phases(2, hA, hC, hAt, hCt, s, nullptr, nullptr, nullptr, nullptr, Bu, 0.0, rho, 0, eta_actor, 0.0,
                            losses_dev);
}

int pdec_ddpg_defer_actor_finish(pdec_handle hA, int on, double rho, int* armed) {
  GET_MLP(A, hA);
  // the fused 3-layer family only (its finish launch is what is deferred), and frozen targets only: with moving targets the
  // next critic pass reads the target actor that the actor's finish writes
  const bool ok = on && (&fused3_family)->net_ok(A) && (float)rho == 1.0f;
  if (!ok) {                           // switched off, or declined: nothing stays pending
    A->defer_finish = false;
    if (int rc = fused_flush_pending(A)) return rc;
  } else {
    A->defer_finish = true;
  }
  if (armed) *armed = ok ? 1 : 0;
  return PDEC_OK;
}

int pdec_ddpg_flush_actor_finish(pdec_handle hA) {
  GET_MLP(A, hA);
  return fused_flush_pending(A);
}

int pdec_debug_batched_update_route(pdec_handle hA, pdec_handle hC, pdec_handle hAt, pdec_handle hCt, int Bu, int which, char* name,
                                    int name_len, int64_t* lds_bytes) {
  PDEC_REQUIRE(name && name_len > 0 && lds_bytes, "pdec_debug_batched_update_route: null argument");
  PDEC_REQUIRE(which >= 0 && which <= 4 && Bu >= 1, "pdec_debug_batched_update_route: which = %d, Bu = %d", which, Bu);
  GET_MLP(A, hA);
  *lds_bytes = 0;
  if (which == 4) {                    // pdec_policy_act_rng on Bu states
    if (const FusedFamily* fam = fused_family_of_act(A, Bu)) return fam->act_describe(A, name, name_len, lds_bytes);
    snprintf(name, name_len, "%s", act_route(A, Bu) == ACT_SMALL ? "small_act_kernel" : "generic");
    return PDEC_OK;
  }
  GET_MLP(C, hC);
  const bool actor_pass = which == 1 || which == 3, all_four = !(which == 1);
  PDEC_REQUIRE(A->dtype == C->dtype, "ddpg: dtype mismatch");
  bool one_stream = A->stream == C->stream;
  if (all_four) {
    GET_MLP(At, hAt);
    GET_MLP(Ct, hCt);
    PDEC_REQUIRE(At->dtype == C->dtype && Ct->dtype == C->dtype, "ddpg: dtype mismatch");
    PDEC_REQUIRE(At->dims == A->dims && Ct->dims == C->dims, "ddpg: target networks must have the behaviour networks' shapes");
    one_stream = one_stream && At->stream == C->stream && Ct->stream == C->stream;
  }
  // inside the update's generic branch the actor pass is pdec_ddpg_actor_grads, which looks at A and C only
  const FusedFamily* full = pass_family(A, C, one_stream);
  const FusedFamily* rt = (which == 3 && !update_applies_in_finish(full, Bu)) ? pass_family(A, C, A->stream == C->stream) : full;
  int rc = PDEC_OK;
  if (rt) rc = rt->describe(A, C, actor_pass, name, name_len, lds_bytes);
  else snprintf(name, name_len, "generic");
  if (rc) return rc;
  if (which >= 2 && rt && !update_applies_in_finish(full, Bu)) {
    const size_t n = strlen(name);
    snprintf(name + n, (size_t)name_len > n ? name_len - n : 0, "/adam_apart");
  }
  return PDEC_OK;
}

int pdec_debug_fused_image(pdec_handle mlp, int which, float* out_host, int* nfloats, int* pub, int* pending, int* paired) {
  GET_MLP(M, mlp);
  PDEC_REQUIRE(which >= 0 && which <= 2, "pdec_debug_fused_image: which = %d", which);
  PDEC_REQUIRE(fused_net_supported(M), "pdec_debug_fused_image: not a fused 3-layer network");
  const DevBuf& img = which == 0 ? M->fw : M->fw_pub[which - 1];
  if (nfloats) *nfloats = (int)(img.bytes / 4);
  if (pub) *pub = M->pub;
  if (pending) *pending = M->pend.on ? 1 : 0;
  if (paired) *paired = M->n_paired;
  if (out_host) {
    PDEC_REQUIRE(img.bytes > 0, "pdec_debug_fused_image: the network has no image yet (no fused pass or acting call has run)");
    PDEC_HIP(hipStreamSynchronize(M->stream));
    PDEC_HIP(hipMemcpy(out_host, img.p, img.bytes, hipMemcpyDeviceToHost));
  }
  return PDEC_OK;
}

int pdec_debug_critic_stamps(pdec_handle critic, int arm, double* out13) {
  GET_MLP(M, critic);
  if (arm) { M->stamps_armed = true; return PDEC_OK; }
  PDEC_REQUIRE(out13, "pdec_debug_critic_stamps: null");
  PDEC_REQUIRE(!M->stamps_armed && M->stamps_last[12] > 0, "pdec_debug_critic_stamps: no fused critic pass has run on this network since it was armed");
  PDEC_HIP(hipStreamSynchronize(M->stream));
  for (int i = 0; i < 13; ++i) out13[i] = M->stamps_last[i];
  return PDEC_OK;
}

}  // extern "C"
