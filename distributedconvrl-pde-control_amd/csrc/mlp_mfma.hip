// mlp_mfma.hip -- fused fp32 MFMA path of the DDPG update for 3-layer actor/critic pairs: src/PDEagent.jl:385-409 as a critic
// pass and an actor pass, each followed by a finish launch (slab sum, ADAM, Polyak, image refresh), and the fused acting kernel.
// This file is the family's one translation unit and its host layer: tile lists and visitors, predicates, ensure_prepped, the
// launches, the deferred finish, fused3_family.  The kernels are templates instantiated from the lists below, in headers:
//   fused3_image.hpp   the padded weight image (FNet), the flat <-> image index map, prep_fused_kernel / unpack_fused_kernel
//   fused3_layers.hpp  LDS-DMA and raw barriers, LiveRows, the layer products, FusedArgs, stamps, the slab's tile numbering
//   fused3_critic.hpp  ddpg_critic_fused_kernel, CriticLds      fused3_actor.hpp  ddpg_actor_fused_kernel, ActorLds
//   fused3_finish.hpp  the three finish kernels                 fused3_act.hpp    policy_act_fused_kernel, ActLds
// Design (gfx950): one workgroup = 8 waves = 128 columns, a wave owns 16 columns for the whole pass;
// v_mfma_f32_16x16x4_f32 (exact f32), a layer's output tile D[16 rows][16 cols] (4 VGPRs per lane: col = lane&15,
// row = 4*(lane>>4)+r) is fed straight back as the B operand of the next layer, the A operand (4 consecutive k of a weight
// row) is one ds_read_b128 from the padded image in LDS; backward-to-input uses the pre-transposed image the same way.  Weight
// gradients contract over columns through [feature][col] staging images in LDS, bias gradients ride as a row of ones.
#include "common.hpp"
#include "mlp.hpp"
// The family's shape constants are stated in this file (KXP here, the tile lists and FUSED3_ACT_MAX_H below), where
// tests/fused_shape_cases.py reads them.  KXP stands ahead of the headers because the image and the layers are built on it.
#define KXP 16             // padded input rows (ns+na+1 <= 16)
#include "fused3_critic.hpp"
#include "fused3_actor.hpp"
#include "fused3_finish.hpp"
#include "fused3_act.hpp"

namespace pdec {

// ------------------------------------------------------------------ host side
static int mt_of(int H) { return (H + 1 + 15) / 16; }

// The instantiations of the two passes, X(critic tiles MT, actor tiles MTA): the ONE list behind the predicate
// (fused_supported), the launches and the report of pdec_debug_batched_update_route
#define FUSED3_TILES(X) X(9, 2) X(9, 1) X(2, 2) X(2, 1)
// the acting kernel's, X(actor tiles MTA)
#define FUSED3_ACT_TILES(X) X(2) X(1)

// f(tile_c<MT>, tile_c<MTA>) of the pair's instantiation; PDEC_E_INVALID for a pair the list does not have
template <class F>
static int visit_tiles(int mt, int mta, F&& f) {
#define X(MT_, MTA_) if (mt == MT_ && mta == MTA_) return f(tile_c<MT_>{}, tile_c<MTA_>{});
  FUSED3_TILES(X)
#undef X
  set_error("fused 3-layer pass: no instantiation for %d critic / %d actor tiles", mt, mta);
  return PDEC_E_INVALID;
}
template <class F>
static int visit_act_tiles(int mta, F&& f) {
#define X(MTA_) if (mta == MTA_) return f(tile_c<MTA_>{});
  FUSED3_ACT_TILES(X)
#undef X
  set_error("fused act: no instantiation for %d actor tiles", mta);
  return PDEC_E_INVALID;
}

// tests only, read per launch: the passes and the acting kernel issue every MFMA of the padded extents (LiveRows; the
// bit-identity reference of the live-row form)
static int fused_full_rows() {
  const char* e = getenv("PDEC_FUSED_FULL_ROWS");
  return (e && e[0] == '1') ? 1 : 0;
}

static bool fused_disabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("PDEC_DISABLE_FUSED");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}

// one 3-layer fp32 net [K0, H, H, 1] relu/relu/(tanh|identity) whose padded image the fused kernels can stage
bool fused_net_supported(const Mlp* M) {
  if (fused_disabled() || M->dtype != PDEC_F32 || M->L != 3) return false;
  if (M->dims[1] != M->dims[2] || M->dims[0] + 1 > KXP || M->dims[3] != 1) return false;
  if (M->acts[0] != PDEC_ACT_RELU || M->acts[1] != PDEC_ACT_RELU) return false;
  const int mt = mt_of(M->dims[1]);
  return mt == 9 || mt == 2 || mt == 1;
}

// an actor / critic pair of such nets (so na == 1 and ns + na + 1 <= KXP through the critic): the critic takes [s; a], tanh
// actor and identity critic, and the tile pair is one of FUSED3_TILES
static bool fused_supported(const Mlp* A, const Mlp* C) {
  if (!fused_net_supported(A) || !fused_net_supported(C)) return false;
  if (C->dims[0] != A->dims[0] + A->dims[3]) return false;
  if (A->acts[2] != PDEC_ACT_TANH || C->acts[2] != PDEC_ACT_IDENTITY) return false;
  const int mt = mt_of(C->dims[1]), mta = mt_of(A->dims[1]);
  bool ok = false;
#define X(MT_, MTA_) ok = ok || (mt == MT_ && mta == MTA_);
  FUSED3_TILES(X)
#undef X
  return ok;
}

static int ensure_prepped(Mlp* M) {
  const FNet f = make_fnet_layout(M->dims[0], M->dims[1]);
  const size_t bytes = (size_t)f.total * 4;
  if (M->fw.bytes < bytes) {
    PDEC_HIP(M->fw.alloc(bytes));
    PDEC_HIP(M->fw_pub[0].alloc(bytes));
    PDEC_HIP(M->fw_pub[1].alloc(bytes));
    M->fw_dirty = true;
  }
  if (M->fw_dirty) {
    ProfScope ps(M, "fused_prep");
    hipLaunchKernelGGL(prep_fused_kernel, dim3((f.total + 255) / 256), dim3(256), 0, M->stream, M->params.as<float>(),
                       M->fw.as<float>(), f);
    PDEC_HIP(hipGetLastError());
    // both published copies (the images the acting kernel reads, see fused_policy_act) restart from the fresh image
    PDEC_HIP(hipMemcpyAsync(M->fw_pub[0].p, M->fw.p, bytes, hipMemcpyDeviceToDevice, M->stream));
    PDEC_HIP(hipMemcpyAsync(M->fw_pub[1].p, M->fw.p, bytes, hipMemcpyDeviceToDevice, M->stream));
    M->fw_dirty = false;
  }
  return PDEC_OK;
}

static FNet fnet_of(const Mlp* M) {
  FNet f = make_fnet_layout(M->dims[0], M->dims[1]);
  f.w = M->fw.as<float>();
  return f;
}

// dynamic LDS bytes of a pass: the end of its layout
template <int MT, int MTA>
static size_t lds_bytes(bool actor_pass) {
  return (size_t)(actor_pass ? ActorLds<MT, MTA>::end : CriticLds<MT, MTA>::end) * 4;
}

// Phase stamps of the critic pass (diagnostic; PDEC_STAMPS=1 prints them, pdec_debug_critic_stamps arms one launch and returns
// them): per-phase s_memtime deltas averaged over the workgroups, and the shader clock the pass ran at
static int read_stamps(Mlp* C, unsigned long long* dev, int grid, double* out13) {
  PDEC_HIP(hipStreamSynchronize(C->stream));
  std::vector<unsigned long long> h((size_t)grid * 16);
  PDEC_HIP(hipMemcpy(h.data(), dev, h.size() * 8, hipMemcpyDeviceToHost));
  double d[10] = {0}, clk = 0;
  for (int b = 0; b < grid; ++b) {
    for (int k = 0; k < 10; ++k) d[k] += (double)(h[b * 16 + k + 1] - h[b * 16 + k]);
    const double rt = (double)(h[b * 16 + 12] - h[b * 16 + 11]);          // 100 MHz ticks
    if (rt > 0) clk += (double)(h[b * 16 + 10] - h[b * 16]) / rt * 0.1;     // GHz
  }
  double tot = 0;
  for (int k = 0; k < 10; ++k) { out13[k] = d[k] / grid; tot += out13[k]; }
  out13[10] = tot;              // shader cycles per workgroup, first to last stamp
  out13[11] = clk / grid;       // shader clock in GHz during the pass (mean over workgroups)
  out13[12] = grid;
  return PDEC_OK;
}
static int dump_stamps(Mlp* C, unsigned long long* dev, int grid) {
  double o[13];
  int rc = read_stamps(C, dev, grid, o);
  if (rc) return rc;
  fprintf(stderr, "[pdec stamps] critic pass, mean shader cycles per phase over %d WGs:", grid);
  static const char* nm[10] = {"load+rbar", "target", "loadQ", "fwdQ", "passA", "loadW2T", "dz1", "passC", "passB", "stats"};
  for (int k = 0; k < 10; ++k) fprintf(stderr, " %s=%.0f", nm[k], o[k]);
  fprintf(stderr, " | total=%.0f cycles, clock=%.3f GHz\n", o[10], o[11]);
  return PDEC_OK;
}

// The passes are exact f32.  (HISTORY.md §3.2a keeps the record of the deleted bf16-split forms; a process that still sets
// PDEC_SPLIT gets an error, not a silent exact-f32 run.)
static int split_refused() {
  const char* e = getenv("PDEC_SPLIT");
  if (e && e[0] && e[0] != '0') {
    set_error("PDEC_SPLIT=%s: the experimental bf16-split passes no longer exist (HISTORY.md §3.2a); the passes are exact f32", e);
    return PDEC_E_INVALID;
  }
  return PDEC_OK;
}
// One pass launch, on C's stream object (its profiling labels).  An instantiation per kernel, so each keeps its own
// once-flag of the dynamic-LDS attribute.  The phase stamps are the critic pass's only.
template <bool ACTOR, int MT, int MTA>
static int launch_pass(Mlp* C, const FusedArgs& g, int grid) {
  if (int rc = split_refused()) return rc;
  const size_t lds = lds_bytes<MT, MTA>(ACTOR);
  auto kern = ACTOR ? ddpg_actor_fused_kernel<MT, MTA> : ddpg_critic_fused_kernel<MT, MTA>;
  const char* label = ACTOR ? "ddpg_actor_fused" : "ddpg_critic_fused";
  static bool attr_set = false;
  if (!attr_set) {
    PDEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  static const bool env_stamps = getenv("PDEC_STAMPS") != nullptr;
  const bool want_stamps = !ACTOR && (env_stamps || C->stamps_armed);
  FusedArgs ga = g;
  if (want_stamps) {
    if (C->stamps.bytes < (size_t)grid * 16 * 8) PDEC_HIP(C->stamps.alloc((size_t)grid * 16 * 8));
    ga.stamps = C->stamps.as<unsigned long long>();
  }
  if (C->prof && C->prof_reps == 1) {
    PDEC_TIMED_LAUNCH(C, label, kern, dim3(grid), dim3(FTHREADS), lds, ga);
  } else {
    ProfScope ps(C, label, true);
    for (int rep = 0; rep < ps.reps; ++rep)
      hipLaunchKernelGGL(kern, dim3(grid), dim3(FTHREADS), lds, C->stream, ga);
  }
  PDEC_HIP(hipGetLastError());
  if (want_stamps && C->stamps_armed) {          // pdec_debug_critic_stamps: keep the figures of this launch for the caller
    C->stamps_armed = false;
    return read_stamps(C, ga.stamps, grid, C->stamps_last);
  }
  if (want_stamps) return dump_stamps(C, ga.stamps, grid);
  return PDEC_OK;
}

static int ensure_slab(Mlp* M, size_t floats) {
  if (M->fslab.bytes < floats * 4) PDEC_HIP(M->fslab.alloc(floats * 4));
  return PDEC_OK;
}

// The arguments of a finish launch on M: slab reduction (nslab > 0) and/or the parameter update (ap): ADAM on M, Polyak into
// Mt, refresh of both padded images.  Takes the beta-power slots of M; finish_issued() follows the launch.
static int finish_args(Mlp* M, Mlp* Mt, const float* slabs, int nslab, int MT, double grad_scale, int mode, int Bu, int quirk,
                       void* loss_dev, const AdamPolyak* ap, const void* loss_add, FinishArgs* out) {
  FinishArgs g{};
  g.slabs = slabs; g.nslab = nslab; g.K0 = M->dims[0]; g.H = M->dims[1]; g.MT = MT;
  g.grads = M->grads.as<float>(); g.scale = (float)grad_scale; g.mode = mode; g.Bu = Bu; g.quirk = quirk;
  g.loss_out = (float*)loss_dev;
  g.loss_add = (const float*)loss_add;
  g.apply = ap != nullptr;
  g.prio = env_prio("PDEC_PRIO_MFMA", 2);
  if (ap) {
    int rcb = bp_begin(M, ap->b1, ap->b2, &g.bp);
    if (rcb) return rcb;
    g.p = M->params.as<float>(); g.m = M->m.as<float>(); g.v = M->v.as<float>();
    g.fw = M->fw.as<float>();
    g.fwp = M->fw_pub[M->pub ^ 1].as<float>();       // written now, read by acting kernels enqueued after this launch
    g.lay = make_fnet_layout(M->dims[0], M->dims[1]);
    g.eta = ap->eta; g.b1 = ap->b1; g.b2 = ap->b2; g.eps = ap->eps;
    // rho == 1 (the reference as it runs: its Polyak loop iterates over an empty parameter list, src/PDEagent.jl:415-417 with
    // src/custom_nna.jl:20 -- agent.py quirk_frozen_targets): the target network is not touched at all, as in the reference
    // (dest = 1 * dest + 0 * src would rewrite it with its own bits, and turn an Inf in src into a NaN in dest)
    if (Mt && (float)ap->rho != 1.0f) {
      g.pt = Mt->params.as<float>(); g.fwt = Mt->fw.as<float>();
      const float r = (float)ap->rho;   // the reference holds p = 0.995f0 and computes (1 - p) in Float32
      g.rho = r; g.omr = 1.0f - r;
    }
  }
  *out = g;
  return PDEC_OK;
}
// the host's half of a finish launch that applied the update: the selectors of the beta powers and of the published image
static void finish_issued(Mlp* M, const AdamPolyak* ap) {
  if (ap) {
    bp_done(M);
    flip(M->pub);
  }
}

// One finish launch on M's stream.
static int launch_finish(Mlp* M, Mlp* Mt, const float* slabs, int nslab, int MT, double grad_scale, int mode,
                         int Bu, int quirk, void* loss_dev, const AdamPolyak* ap, const void* loss_add = nullptr) {
  FinishArgs g;
  if (int rc = finish_args(M, Mt, slabs, nslab, MT, grad_scale, mode, Bu, quirk, loss_dev, ap, loss_add, &g)) return rc;
  const int n = M->nparams;
  {
    const char* label = ap ? (nslab > 0 ? "fused_finish" : "fused_apply") : "fused_reduce";
    const bool use_ref = getenv("PDEC_FINISH_REF") != nullptr;            // tests only: the bit-identity reference kernel
    // the one-shot completion event of this launch: the apply launch carries the stop event (parameters updated), a reduce-only
    // launch the reduce event (flat gradient ready: what an all-reduce on another stream waits for)
    hipEvent_t& slot = ap ? M->stop_event : M->reduce_event;
    const hipEvent_t ev = slot;
    if (use_ref) {
      const int nblk = nslab > 0 ? 4 * slab_tiles(MT) : (n + 63) / 64;
      hipLaunchKernelGGL(fused_finish_ref_kernel, dim3(nblk), dim3(1024), 0, M->stream, g);
      if (ev) (void)hipEventRecord(ev, M->stream);
    } else {
      const int nblk = nslab > 0 ? 8 * slab_tiles(MT) : (n + FIN_THREADS - 1) / FIN_THREADS;
      if (M->prof) {
        PDEC_TIMED_LAUNCH(M, label, fused_finish_kernel, dim3(nblk), dim3(FIN_THREADS), 0, g);
        if (ev) (void)hipEventRecord(ev, M->stream);
      } else if (ev) {
        // the event rides on this kernel's own dispatch packet (its completion signal): a hipEventRecord behind the
        // launch is a packet of its own that the next kernel of the stream has to wait for (~4.5 us of the update chain)
        hipExtLaunchKernelGGL(fused_finish_kernel, dim3(nblk), dim3(FIN_THREADS), 0, M->stream, nullptr, ev, 0, g);
      } else {
        hipLaunchKernelGGL(fused_finish_kernel, dim3(nblk), dim3(FIN_THREADS), 0, M->stream, g);
      }
    }
    slot = nullptr;     // consumed (the stop event only by a launch that applies the update, the reduce event only by a reduce-only one)
  }
  PDEC_HIP(hipGetLastError());
  finish_issued(M, ap);
  return PDEC_OK;
}

// ---- the deferred actor finish (pdec_ddpg_defer_actor_finish).  With frozen targets the critic half of update k + 1 reads
// nothing the actor's finish of update k writes, so that finish need not be a launch of the update chain: the actor pass leaves
// it pending, and the critic's finish launch of the next update takes its blocks along (fused_finish_pair_kernel).
int fused_flush_pending(Mlp* A) {
  PendingFinish& P = A->pend;
  if (!P.on) return PDEC_OK;
  P.on = false;
  if (P.stop) A->stop_event = P.stop;       // the plain launch carries it, as the launch it replaces would have
  P.stop = nullptr;
  return launch_finish(A, nullptr, P.slabs, P.nslab, P.mta, P.scale, 1, P.Bu, 0, P.loss, &P.ap);
}

// The critic's finish (always with its update: ap) and the pending finish of A in one launch on C's stream.  The launch carries
// C's stop event; a stop event that was set on A is recorded behind it.
static int launch_finish_pair(Mlp* C, Mlp* Ct, const float* slabs, int nslab, int MT, double grad_scale, int Bu, int quirk,
                              void* loss_dev, const AdamPolyak* ap, const void* loss_add, Mlp* A) {
  PendingFinish& P = A->pend;
  // the reference kernel (PDEC_FINISH_REF), a profiled launch and nets on two streams keep the two launches
  if (getenv("PDEC_FINISH_REF") != nullptr || C->prof || A->prof || A->stream != C->stream) {
    if (int rc = fused_flush_pending(A)) return rc;
    return launch_finish(C, Ct, slabs, nslab, MT, grad_scale, 0, Bu, quirk, loss_dev, ap, loss_add);
  }
  FinishArgs gc, ga;
  int rc;
  if ((rc = finish_args(C, Ct, slabs, nslab, MT, grad_scale, 0, Bu, quirk, loss_dev, ap, loss_add, &gc))) return rc;
  if ((rc = finish_args(A, nullptr, P.slabs, P.nslab, P.mta, P.scale, 1, P.Bu, 0, P.loss, &P.ap, nullptr, &ga))) return rc;
  const int nc = 8 * slab_tiles(MT), na = 8 * slab_tiles(P.mta);
  const hipEvent_t ev = C->stop_event, eva = P.stop;
  if (ev)
    hipExtLaunchKernelGGL(fused_finish_pair_kernel, dim3(nc + na), dim3(FIN_THREADS), 0, C->stream, nullptr, ev, 0, gc, ga, nc);
  else
    hipLaunchKernelGGL(fused_finish_pair_kernel, dim3(nc + na), dim3(FIN_THREADS), 0, C->stream, gc, ga, nc);
  C->stop_event = nullptr;
  P.on = false;
  P.stop = nullptr;
  ++A->n_paired;
  PDEC_HIP(hipGetLastError());
  if (eva) PDEC_HIP(hipEventRecord(eva, C->stream));
  finish_issued(C, ap);
  finish_issued(A, &P.ap);
  return PDEC_OK;
}

int fused_unpack_published(Mlp* A, float* flat_out, hipStream_t stream) {
  PDEC_REQUIRE(fused_net_supported(A), "fused_unpack_published: not a fused 3-layer network");
  PDEC_REQUIRE_NO_PENDING(A, "fused_unpack_published");
  int rc = ensure_prepped(A);
  if (rc) return rc;
  FNet f = make_fnet_layout(A->dims[0], A->dims[1]);
  PDEC_REQUIRE(A->nparams == flat_offsets(f.K0, f.H).n, "fused_unpack_published: parameter count");
  hipLaunchKernelGGL(unpack_fused_kernel, dim3((A->nparams + 255) / 256), dim3(256), 0, stream, A->fw_pub[A->pub].as<float>(),
                     flat_out, f);
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

// a 3-layer fp32 actor whose published image the fused acting kernel reads, at any number of columns
#define FUSED3_ACT_MAX_H 31
static bool fused_act_ok(const Mlp* M, int) {
  return fused_net_supported(M) && M->dims[M->L] == 1 && M->dims[1] <= FUSED3_ACT_MAX_H;
}

// tiles and dynamic LDS bytes (the end of ActLds) of the acting kernel of a fused 3-layer actor, or the refusal
static int fused_act_plan(const Mlp* A, int* mta, size_t* lds) {
  *mta = mt_of(A->dims[1]);
  *lds = 0;                        // no instantiation
#define X(MTA_) if (*mta == MTA_) *lds = (size_t)ActLds<MTA_>::end * 4;
  FUSED3_ACT_TILES(X)
#undef X
  PDEC_REQUIRE(A->acts[2] == PDEC_ACT_TANH || A->acts[2] == PDEC_ACT_IDENTITY, "fused act: unsupported output activation");
  PDEC_REQUIRE(*lds != 0 && *lds <= 64 * 1024, "fused act: hidden width %d too large", A->dims[1]);
  return PDEC_OK;
}

static int fused_policy_act(Mlp* A, const void* state, int cols, double act_noise, double act_limit, int learning, uint64_t seed,
                            uint64_t offset, void* actions_out, const uint64_t* ctr_cur, uint64_t* ctr_next, uint64_t ctr_inc) {
  PDEC_REQUIRE_NO_PENDING(A, "fused act");
  int rc = ensure_prepped(A);
  if (rc) return rc;
  FNet f = fnet_of(A);
  // Read the PUBLISHED copy of the image: the update's finish kernel writes the other copy (and the in-place image
  // of the update passes), so an acting kernel may run beside the actor half of the following update.  A copy is
  // rewritten two updates later; callers that overlap acting and updating on different streams must order update
  // t+1 behind the acting kernel of step t-1 (bench.py waits on that event at the start of each update).
  f.w = A->fw_pub[A->pub].as<float>();
  int mta = 0;
  size_t lds = 0;
  if ((rc = fused_act_plan(A, &mta, &lds))) return rc;
  const int tanh_out = A->acts[2] == PDEC_ACT_TANH;
  const int prio = env_prio("PDEC_PRIO_ACT", 3);
  const int full_rows = fused_full_rows();
  const dim3 grid((cols + 63) / 64), block(ACT_THREADS);
  rc = visit_act_tiles(mta, [&](auto MTA) {
#define ACT_ARGS(an) f, (const float*)state, cols, A->dims[0], an, (float)act_limit, learning, tanh_out, seed, offset, \
                     (float*)actions_out, ctr_cur, ctr_next, ctr_inc, prio, full_rows
    auto go = [&](auto kern, auto an) {
      if (A->prof) PDEC_TIMED_LAUNCH(A, "policy_act_fused", kern, grid, block, lds, ACT_ARGS(an));
      else hipLaunchKernelGGL(kern, grid, block, lds, A->stream, ACT_ARGS(an));
    };
    if (learning && A->noise_color) go(policy_act_fused_kernel<decltype(MTA)::value, NoiseColor>, noise_color_of(A, act_noise));
    else if (A->noise_scale) go(policy_act_fused_kernel<decltype(MTA)::value, NoiseScale>, noise_scale_of(A));
    else go(policy_act_fused_kernel<decltype(MTA)::value>, (float)act_noise);
#undef ACT_ARGS
    return (int)PDEC_OK;
  });
  if (rc) return rc;
  PDEC_HIP(hipGetLastError());
  return PDEC_OK;
}

static int fused_act_describe(const Mlp* A, char* name, int name_len, int64_t* lds_out) {
  int mta = 0;
  size_t lds = 0;
  if (int rc = fused_act_plan(A, &mta, &lds)) return rc;
  return visit_act_tiles(mta, [&](auto MTA) {
    snprintf(name, name_len, "policy_act_fused_kernel<%d>", decltype(MTA)::value);
    *lds_out = (int64_t)lds;
    return (int)PDEC_OK;
  });
}

// ADAM(M) + Polyak(Mt <- M) + image refresh from the gradient buffer (after an external all-reduce)
static int fused_adam_polyak(Mlp* M, Mlp* Mt, const AdamPolyak& ap) {
  int rc;
  PDEC_REQUIRE_NO_PENDING(M, "fused apply");
  if ((rc = ensure_prepped(M)) || (Mt && (rc = ensure_prepped(Mt)))) return rc;
  return launch_finish(M, Mt, nullptr, 0, mt_of(M->dims[1]), 1.0, 0, 1, 0, nullptr, &ap);
}

static int fused_critic_grads(Mlp* A, Mlp* C, Mlp* At, Mlp* Ct, const void* s, const void* a, const void* r, const void* t,
                              const void* sn, int Bu, double gamma, int quirk, double grad_scale, void* loss_dev,
                              const AdamPolyak* apply, const void* loss_add) {
  int rc;
  if ((rc = ensure_prepped(C)) || (rc = ensure_prepped(At)) || (rc = ensure_prepped(Ct))) return rc;
  const int mt = mt_of(C->dims[1]), mta = mt_of(A->dims[1]);
  const int grid = (Bu + FCOLS - 1) / FCOLS;
  if ((rc = ensure_slab(C, slab_floats_total(mt, grid)))) return rc;
  FusedArgs g{};
  g.C = fnet_of(C); g.At = fnet_of(At); g.Ct = fnet_of(Ct);
  g.s = (const float*)s; g.a = (const float*)a; g.r = (const float*)r; g.t = (const float*)t; g.sn = (const float*)sn;
  g.Bu = Bu; g.ns = A->dims[0]; g.na = 1; g.gamma = (float)gamma; g.quirk = quirk;
  g.slab = C->fslab.as<float>();
  g.prio = env_prio("PDEC_PRIO_MFMA", 2);
  g.full_rows = fused_full_rows();
  if (quirk && C->rpart_ext) {         // the producer of r left one partial sum per workgroup
    g.rpart = C->rpart_ext; g.nrpart = C->rpart_n;
  } else if (quirk && C->rbar_ext) {   // reduced by the producer of r on its own stream (pdec_reward_mean): nothing to sum here
    g.rbar_dev = (const float*)C->rbar_ext;
  } else if (quirk && Bu > 256 * FCOLS) {     // every workgroup summing all of r itself does not scale (C3: 131072 rewards): reduce once
    float* rb = nullptr;
    if ((rc = launch_rmean(C, (const float*)r, Bu, &rb))) return rc;
    g.rbar_dev = rb;
  }
  C->rbar_ext = nullptr;
  C->rpart_ext = nullptr;
  rc = visit_tiles(mt, mta, [&](auto MT, auto MTA) {
    return launch_pass<false, decltype(MT)::value, decltype(MTA)::value>(C, g, grid);
  });
  if (rc) return rc;
  if (A->pend.on) {
    // (a reduce-only critic finish has no place for the actor's update: the pending finish goes first, as a launch of its own)
    if (apply) return launch_finish_pair(C, Ct, C->fslab.as<float>(), grid, mt, grad_scale, Bu, quirk, loss_dev, apply, loss_add, A);
    if ((rc = fused_flush_pending(A))) return rc;
  }
  return launch_finish(C, apply ? Ct : nullptr, C->fslab.as<float>(), grid, mt, grad_scale, 0, Bu, quirk, loss_dev, apply,
                       loss_add);
}

// what fused_critic_grads / fused_actor_grads would launch for this pair (pdec_debug_batched_update_route): through the same
// visitor and the same lds_bytes<> as launch_pass
static int fused_describe(const Mlp* A, const Mlp* C, bool actor_pass, char* name, int name_len, int64_t* lds) {
  if (int rc = split_refused()) return rc;
  return visit_tiles(mt_of(C->dims[1]), mt_of(A->dims[1]), [&](auto MT, auto MTA) {
    constexpr int mt_ = decltype(MT)::value, mta_ = decltype(MTA)::value;
    snprintf(name, name_len, "%s<%d,%d>", actor_pass ? "ddpg_actor_fused_kernel" : "ddpg_critic_fused_kernel", mt_, mta_);
    *lds = (int64_t)lds_bytes<mt_, mta_>(actor_pass);
    return (int)PDEC_OK;
  });
}

static int fused_actor_grads(Mlp* A, Mlp* C, Mlp* At, const void* s, int Bu, double grad_scale, void* loss_dev,
                             const AdamPolyak* apply) {
  int rc;
  PDEC_REQUIRE_NO_PENDING(A, "fused actor pass");
  if ((rc = ensure_prepped(C)) || (rc = ensure_prepped(A)) || (apply && At && (rc = ensure_prepped(At)))) return rc;
  const int mt = mt_of(C->dims[1]), mta = mt_of(A->dims[1]);
  const int grid = (Bu + FCOLS - 1) / FCOLS;
  if ((rc = ensure_slab(A, slab_floats_total(mta, grid)))) return rc;
  FusedArgs g{};
  g.C = fnet_of(C); g.A = fnet_of(A);
  g.s = (const float*)s; g.Bu = Bu; g.ns = A->dims[0]; g.na = 1;
  g.slab = A->fslab.as<float>();
  g.prio = env_prio("PDEC_PRIO_MFMA", 2);
  g.full_rows = fused_full_rows();
  // the actor pass is launched on the critic's stream object for profiling labels but must follow
  // ADAM(C); both handles share one stream in every caller (checked by the dispatcher)
  rc = visit_tiles(mt, mta, [&](auto MT, auto MTA) {
    return launch_pass<true, decltype(MT)::value, decltype(MTA)::value>(C, g, grid);
  });
  if (rc) return rc;
  // armed (pdec_ddpg_defer_actor_finish) and the targets frozen: the finish stays pending for the next critic finish launch.
  // (Moving targets: that critic pass reads the target actor this finish writes, so the launch is made here as ever.)
  if (A->defer_finish && apply && (float)apply->rho == 1.0f) {
    PendingFinish& P = A->pend;
    P.on = true;
    P.slabs = A->fslab.as<float>(); P.nslab = grid; P.mta = mta; P.Bu = Bu; P.scale = grad_scale; P.loss = loss_dev; P.ap = *apply;
    P.stop = A->stop_event;
    A->stop_event = nullptr;
    return PDEC_OK;
  }
  return launch_finish(A, apply ? At : nullptr, A->fslab.as<float>(), grid, mta, grad_scale, 1, Bu, 0, loss_dev, apply);
}

// the finish launch of a pass applies ADAM + Polyak at every batch size.  (Host pass only: the device pass would emit a const
// table as a constant of the code object, and these are addresses of host functions.)
#ifndef __HIP_DEVICE_COMPILE__
const FusedFamily fused3_family = {fused_supported,    fused_net_supported, fused_act_ok,      0,
                                   fused_critic_grads, fused_actor_grads,   fused_adam_polyak, fused_policy_act,
                                   fused_describe,     fused_act_describe};
#endif

}  // namespace pdec
