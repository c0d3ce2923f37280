// population.hip -- the population object (include/pdeconv.h, population.py): its creation from M learners' networks, traces and
// counter rows, the members' beta-power slots, the hooks' actor snapshots and exploit by clone.  Its per-step launches are
// pdec_population_glue (act.hip) and the members' update (pdec_population_update in mlp_small.hip, the kernels in small_generic.hpp /
// small2.hpp / small2f.hpp), its episode boundary pop_book.hip.
#include "common.hpp"
#include "population.hpp"

using namespace pdec;

extern "C" {

int pdec_population_create(pdec_handle* out, int M, const pdec_handle* actors, const pdec_handle* critics,
                           const pdec_handle* target_actors, const pdec_handle* target_critics, void* const* traces,
                           const uint64_t* seeds, void* const* losses, int env_dtype, int cols, int64_t capacity, int stride,
                           int loops, int Bu, double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                           int64_t update_after_rows, int64_t update_freq, int64_t start_steps, int64_t* rows) {
  PDEC_REQUIRE(out && M >= 1 && actors && critics && target_actors && target_critics && traces && seeds && losses && rows,
               "pdec_population_create: null argument");
  PDEC_REQUIRE(env_dtype == PDEC_F32 || env_dtype == PDEC_F64, "pdec_population_create: bad dtype %d", env_dtype);
  PDEC_REQUIRE(cols >= 1 && capacity >= 1 && stride >= 1 && loops >= 1 && Bu >= 1 && update_freq >= 1 && update_after_rows >= stride,
               "pdec_population_create: bad argument (cols %d, capacity %lld, stride %d, update_after rows %lld)", cols,
               (long long)capacity, stride, (long long)update_after_rows);
  auto P = std::make_unique<Population>();
  P->M = M; P->cols = cols; P->dtype = env_dtype; P->rows = (long long*)rows;
  P->cap = capacity; P->cap1 = capacity + stride; P->stride = stride; P->after = update_after_rows; P->freq = update_freq;
  P->start_steps = start_steps; P->loops = loops; P->Bu = Bu; P->quirk = quirk;
  P->gamma = gamma; P->rho = rho; P->eta_a = eta_actor; P->eta_c = eta_critic;
  std::vector<PopMember> tab(M);
  for (int m = 0; m < M; ++m) {
    Mlp* A = lookup_as<Mlp>(actors[m], Kind::Mlp);
    Mlp* C = lookup_as<Mlp>(critics[m], Kind::Mlp);
    Mlp* At = lookup_as<Mlp>(target_actors[m], Kind::Mlp);
    Mlp* Ct = lookup_as<Mlp>(target_critics[m], Kind::Mlp);
    if (!A || !C || !At || !Ct) { set_error("pdec_population_create: bad network handle of member %d", m); return PDEC_E_HANDLE; }
    PDEC_REQUIRE(A->dtype == PDEC_F32 && C->dtype == PDEC_F32 && At->dtype == PDEC_F32 && Ct->dtype == PDEC_F32,
                 "pdec_population_create: member %d: fp32 networks only", m);
    PDEC_REQUIRE(A->stream == C->stream && At->stream == C->stream && Ct->stream == C->stream,
                 "pdec_population_create: member %d: its four networks must share one stream", m);
    if (m > 0) {
      Mlp* A0 = P->A[0];
      Mlp* C0 = P->C[0];
      PDEC_REQUIRE(A->dims == A0->dims && A->acts == A0->acts && C->dims == C0->dims && C->acts == C0->acts &&
                   At->dims == A0->dims && Ct->dims == C0->dims,
                   "pdec_population_create: member %d: network shapes differ from member 0's", m);
      PDEC_REQUIRE(A->stream == A0->stream, "pdec_population_create: member %d: update stream differs from member 0's", m);
      PDEC_REQUIRE(A->noise_rows == A0->noise_rows, "pdec_population_create: member %d: noise rows differ", m);
    }
    PDEC_REQUIRE(!A->halt && !C->halt, "pdec_population_create: member %d: an episode halt flag is attached", m);
    PDEC_REQUIRE(!A->noise_scale, "pdec_population_create: member %d: a noise scale array is set on its actor "
                                  "(pdec_mlp_set_noise_scale); a member's amplitude is the act_noise of its row", m);
    PDEC_REQUIRE(!A->noise_color, "pdec_population_create: member %d: a noise color is set on its actor "
                                  "(pdec_mlp_set_noise_color); the member glue does not serve it", m);
    BpArgs bp{};
    int rc;
    if ((rc = bp_begin(A, 0.9, 0.999, &bp)) || (rc = bp_begin(C, 0.9, 0.999, &bp))) return rc;   // (uploads the powers once)
    PopMember& e = tab[m];
    e.actor_p = A->params.p;
    e.ts = (float*)traces[4 * m]; e.ta = (float*)traces[4 * m + 1]; e.tr = (float*)traces[4 * m + 2]; e.tt = (float*)traces[4 * m + 3];
    PDEC_REQUIRE(e.ts && e.ta && e.tr && e.tt && losses[m], "pdec_population_create: member %d: null trace or loss slot", m);
    e.noise_seed = seeds[2 * m]; e.sample_seed = seeds[2 * m + 1];
    e.Ap = A->params.as<float>(); e.Ag = A->grads.as<float>(); e.Am = A->m.as<float>(); e.Av = A->v.as<float>(); e.Apt = At->params.as<float>();
    e.Cp = C->params.as<float>(); e.Cg = C->grads.as<float>(); e.Cm = C->m.as<float>(); e.Cv = C->v.as<float>(); e.Cpt = Ct->params.as<float>();
    e.bpA = A->bpd.as<double>(); e.bpC = C->bpd.as<double>();
    e.losses = (float*)losses[m];
    P->A.push_back(A); P->C.push_back(C); P->At.push_back(At); P->Ct.push_back(Ct);
  }
  Mlp* A0 = P->A[0];
  PDEC_REQUIRE(step_glue_served(A0, A0, env_dtype, 1, cols, cols),
               "pdec_population_create: the single-launch glue does not serve these networks at %d columns of dtype %d", cols, env_dtype);
  PDEC_HIP(P->tab.alloc(sizeof(PopMember) * M));
  PDEC_HIP(hipMemcpy(P->tab.p, tab.data(), sizeof(PopMember) * M, hipMemcpyHostToDevice));
  P->stream = A0->stream;
  *out = register_object(std::move(P));
  return PDEC_OK;
}

// the members' beta-power slots: get = write each member's (actor, critic) bp_sel into rows_host[m][POP_BPA / POP_BPC];
// set = adopt them from there (and mark the networks' derived images stale after the updates of an episode)
int pdec_population_bp_sel(pdec_handle pop, int64_t* rows_host, int set) {
  GET_POP(P, pop);
  PDEC_REQUIRE(rows_host, "pdec_population_bp_sel: null");
  for (int m = 0; m < P->M; ++m) {
    int64_t* r = rows_host + (size_t)m * POP_ROW;
    if (set) {
      PDEC_REQUIRE((r[POP_BPA] == 0 || r[POP_BPA] == 1) && (r[POP_BPC] == 0 || r[POP_BPC] == 1), "pdec_population_bp_sel: bad slot");
      P->A[m]->bp_sel = (int)r[POP_BPA]; P->C[m]->bp_sel = (int)r[POP_BPC];
      P->A[m]->fw_dirty = P->C[m]->fw_dirty = P->At[m]->fw_dirty = P->Ct[m]->fw_dirty = true;
    } else {
      r[POP_BPA] = P->A[m]->bp_sel; r[POP_BPC] = P->C[m]->bp_sel;
    }
  }
  return PDEC_OK;
}

}  // extern "C"

// the hooks' actor snapshots at the end of an episode (PDEhook POST_EPISODE: bestNNA on a new best, currentNNA every episode)
// for all members in one launch: member m (blockIdx.y) copies its behaviour actor's parameters to snap[2m] when bit 0 of
// which[m] is set and to snap[2m + 1] when bit 1 is -- the bytes pdec_mlp_copy moves between two fp32 networks
__global__ __launch_bounds__(256) void pop_copy_actors_kernel(const PopMember* __restrict__ pm, float* const* __restrict__ snap,
                                                              const int32_t* __restrict__ which, int n) {
  const int m = blockIdx.y, w = which[m];
  float* d0 = (w & 1) ? snap[2 * m] : nullptr;
  float* d1 = (w & 2) ? snap[2 * m + 1] : nullptr;
  if (!d0 && !d1) return;
  const float* src = static_cast<const float*>(pm[m].actor_p);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float v = src[i];
    if (d0) d0[i] = v;
    if (d1) d1[i] = v;
  }
}

extern "C" {

int pdec_population_set_actor_copies(pdec_handle pop, const pdec_handle* best, const pdec_handle* current) {
  GET_POP(P, pop);
  PDEC_REQUIRE(best && current, "pdec_population_set_actor_copies: null");
  std::vector<float*> tab(2 * (size_t)P->M, nullptr);
  std::vector<Mlp*> nets;
  for (int m = 0; m < P->M; ++m) {
    const pdec_handle h2[2] = {best[m], current[m]};
    for (int k = 0; k < 2; ++k) {
      if (!h2[k]) continue;
      Mlp* D = lookup_as<Mlp>(h2[k], Kind::Mlp);
      if (!D) { set_error("pdec_population_set_actor_copies: bad network handle of member %d", m); return PDEC_E_HANDLE; }
      PDEC_REQUIRE(D->dims == P->A[m]->dims && D->dtype == PDEC_F32 && D->stream == P->stream,
                   "pdec_population_set_actor_copies: member %d: a snapshot must be an fp32 network of the actor's shape on its stream", m);
      tab[2 * m + k] = D->params.as<float>();
      nets.push_back(D);
    }
  }
  if (!P->snap.p) PDEC_HIP(P->snap.alloc(sizeof(float*) * 2 * P->M));
  PDEC_HIP(hipStreamSynchronize(P->stream));       // (an earlier copy launch may still read the table)
  PDEC_HIP(hipMemcpy(P->snap.p, tab.data(), sizeof(float*) * 2 * P->M, hipMemcpyHostToDevice));
  P->snap_nets = nets;
  return PDEC_OK;
}

int pdec_population_copy_actors(pdec_handle pop, const int32_t* which) {
  GET_POP(P, pop);
  PDEC_REQUIRE(which && P->snap.p, "pdec_population_copy_actors: null flags or no snapshot table (pdec_population_set_actor_copies)");
  const int n = P->A[0]->nparams;
  const dim3 grid((unsigned)std::min(cdiv(n, 256), 16), (unsigned)P->M);
  ProfScope ps(P, "population_copy_actors");
  hipLaunchKernelGGL(pop_copy_actors_kernel, grid, dim3(256), 0, P->stream, P->tab.as<PopMember>(), P->snap.as<float*>(), which, n);
  PDEC_HIP(hipGetLastError());
  for (Mlp* D : P->snap_nets) D->fw_dirty = true;
  return PDEC_OK;
}

}  // extern "C"

// n floats src -> dst by the threads of grid row blockIdx.y: 16-byte accesses where source and destination are both aligned
// (or reach alignment after the same scalar head), single floats for heads, tails and differently aligned pairs
__device__ __forceinline__ void clone_floats(float* __restrict__ dst, const float* __restrict__ src, long long n) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, nt = (long long)gridDim.x * 256;
  const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst);
  if (((as ^ ad) & 15) != 0 || (as & 3) != 0) {
    for (long long i = t; i < n; i += nt) dst[i] = src[i];
    return;
  }
  long long head = (long long)(((16 - (as & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long long nv = (n - head) >> 2, tail = head + 4 * nv;
  for (long long i = t; i < head; i += nt) dst[i] = src[i];
  const float4* s4 = reinterpret_cast<const float4*>(src + head);
  float4* d4 = reinterpret_cast<float4*>(dst + head);
  for (long long i = t; i < nv; i += nt) d4[i] = s4[i];
  for (long long i = tail + t; i < n; i += nt) dst[i] = src[i];
}

// pdec_population_clone: destination blockIdx.y of the table takes over its source's learner -- parameters and both ADAM moments
// of the behaviour actor and critic, the parameters of the two target networks, the source's CURRENT beta powers into the
// destination's CURRENT slot, the loss pair and, where asked, the filled prefix of the four replay traces (rows past it are not
// touched).  The gradient buffers are scratch of the update -- every small-update kernel writes a gradient before it reads it,
// and the register kernels never touch the buffers at all -- so they stay.  No member is both a source and a destination
// (the entry point refuses it), so no workgroup reads what another writes.
__global__ __launch_bounds__(256) void pop_clone_members_kernel(const PopMember* __restrict__ pm, const PopClone* __restrict__ tab,
                                                                int nA, int nC, int ns, int na) {
  const PopClone c = tab[blockIdx.y];
  const PopMember& S = pm[c.src];
  const PopMember& D = pm[c.dst];
  clone_floats(D.Ap, S.Ap, nA); clone_floats(D.Am, S.Am, nA); clone_floats(D.Av, S.Av, nA); clone_floats(D.Apt, S.Apt, nA);
  clone_floats(D.Cp, S.Cp, nC); clone_floats(D.Cm, S.Cm, nC); clone_floats(D.Cv, S.Cv, nC); clone_floats(D.Cpt, S.Cpt, nC);
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    const int k = threadIdx.x & 1;
    if (threadIdx.x < 2) D.bpA[2 * c.bpa_dst + k] = S.bpA[2 * c.bpa_src + k];
    else D.bpC[2 * c.bpc_dst + k] = S.bpC[2 * c.bpc_src + k];
  }
  clone_floats(D.losses, S.losses, 2);
  if (c.rows_sa) {
    clone_floats(D.ts, S.ts, c.rows_sa * ns);
    clone_floats(D.ta, S.ta, c.rows_sa * na);
  }
  if (c.rows_rt) {
    clone_floats(D.tr, S.tr, c.rows_rt);
    clone_floats(D.tt, S.tt, c.rows_rt);
  }
}

extern "C" {

int pdec_population_clone(pdec_handle pop, const int32_t* src, const int64_t* rows_sa, const int64_t* rows_rt) {
  GET_POP(P, pop);
  PDEC_REQUIRE(src && rows_sa && rows_rt, "pdec_population_clone: null");
  const int M = P->M;
  std::vector<char> is_src(M, 0);
  for (int d = 0; d < M; ++d) {
    PDEC_REQUIRE(src[d] >= 0 && src[d] < M, "pdec_population_clone: member %d: source %d is not one of the %d members", d, (int)src[d], M);
    if (src[d] != d) is_src[src[d]] = 1;
  }
  std::vector<PopClone> tab;
  long long most = std::max(P->A[0]->nparams, P->C[0]->nparams);
  const int ns = P->A[0]->dims[0], na = P->A[0]->dims[P->A[0]->L];
  for (int d = 0; d < M; ++d) {
    if (src[d] == d) continue;
    PDEC_REQUIRE(!is_src[d], "pdec_population_clone: member %d is both a source and a destination (one launch copies all pairs: "
                 "no member may be read and written)", d);
    PDEC_REQUIRE(rows_sa[d] >= 0 && rows_sa[d] <= P->cap1 && rows_rt[d] >= 0 && rows_rt[d] <= P->cap,
                 "pdec_population_clone: member %d: %lld / %lld replay rows exceed the traces (%lld / %lld)", d,
                 (long long)rows_sa[d], (long long)rows_rt[d], P->cap1, P->cap);
    const int s = src[d];
    PDEC_REQUIRE(P->A[s]->bp_init && P->C[s]->bp_init && P->A[d]->bp_init && P->C[d]->bp_init,
                 "pdec_population_clone: member %d or %d: beta powers not initialised", s, d);
    tab.push_back(PopClone{s, d, P->A[s]->bp_sel, P->C[s]->bp_sel, P->A[d]->bp_sel, P->C[d]->bp_sel, rows_sa[d], rows_rt[d]});
    most = std::max(most, std::max((long long)rows_sa[d] * std::max(ns, na), (long long)rows_rt[d]));
  }
  if (tab.empty()) return PDEC_OK;
  if (!P->clones.p) PDEC_HIP(P->clones.alloc(sizeof(PopClone) * M));
  PDEC_HIP(hipStreamSynchronize(P->stream));       // (an earlier clone launch may still read the table)
  PDEC_HIP(hipMemcpy(P->clones.p, tab.data(), sizeof(PopClone) * tab.size(), hipMemcpyHostToDevice));
  // one 16-byte access per thread and trip over the longest array, at most ~2048 workgroups in all
  const long long want = cdiv(cdiv(most, 4), 256), cap = std::max<long long>(1, 2048 / (long long)tab.size());
  const dim3 grid((unsigned)std::max<long long>(1, std::min(want, cap)), (unsigned)tab.size());
  ProfScope ps(P, "population_clone");
  hipLaunchKernelGGL(pop_clone_members_kernel, grid, dim3(256), 0, P->stream, P->tab.as<PopMember>(), P->clones.as<PopClone>(),
                     P->A[0]->nparams, P->C[0]->nparams, ns, na);
  PDEC_HIP(hipGetLastError());
  for (const PopClone& c : tab)
    P->A[c.dst]->fw_dirty = P->C[c.dst]->fw_dirty = P->At[c.dst]->fw_dirty = P->Ct[c.dst]->fw_dirty = true;
  return PDEC_OK;
}

}  // extern "C"
