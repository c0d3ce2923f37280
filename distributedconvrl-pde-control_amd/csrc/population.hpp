// population.hpp -- the device tables of a population and the object behind its handle, for the files that build, serve or read
// them: population.hip, act.hip (pdec_population_glue), mlp_small.hip with small_args.hpp (the members' update: pdec_population_update
// and the kernels' member prologue sm_member_begin), pop_book.hip (the episode boundary)
#pragma once
#include "mlp.hpp"

namespace pdec {

// ---- populations (pdec_population_create, population.py): M independent single-trajectory learners whose per-step launches
// are ONE launch of M workgroups each.  Workgroup m reads member m's pointers from a device table (PopMember) and its counters
// from row m of a device int64 table that the host writes once per episode and reads back once per episode.
#define POP_ROW 16
enum PopSlot {
  POP_USTEP = 0,    // policy.update_step
  POP_NSA,          // trajectory.n_sa
  POP_NRT,          // trajectory.n_rt
  POP_NOISE,        // policy._noise_off (Philox counters of the exploration noise)
  POP_SAMPLE,       // policy._sample_off (Philox counters of the minibatch draws)
  POP_HALT,         // the member's episode halt flag (low 32 bits; pdec_set_episode_halt's protocol)
  POP_ACTIVE,       // 1: the member runs this episode (0: its stop condition has fired)
  POP_BPA,          // slot of the actor's / critic's double-buffered ADAM beta powers (Mlp::bp_sel)
  POP_BPC,
  POP_NOISE_AMP,    // act_noise, act_limit (bit patterns of doubles)
  POP_LIMIT,
};
// a member's own hyper-parameters (bit patterns of doubles), read by the small update's prologue (sm_member_begin) when
// pdec_population_set_member_hyper is on; with it off the launch-wide values of pdec_population_create hold and the slots are
// not read.  Slot 15 stays free.
enum PopHyperSlot {
  POP_GAMMA = 11,   // policy.y
  POP_RHO,          // policy.rho_effective
  POP_ETA_A,        // behaviour actor's / critic's ADAM step size
  POP_ETA_C,
};
// ---- a member's book (pdec_population_episode_close, csrc/pop_book.hip): what its PDEhook and its stop condition hold between
// two episodes, so that the episode boundary needs no host.  A caller-owned device table int64 [M][POP_BOOK] beside the rows,
// doubles as bit patterns; population.py mirrors the names (tests/test_population_blocks_host.py compares them).
#define POP_BOOK 16
enum PopBookSlot {
  PBK_EP = 0,        // hook.ep: index of the episode that is running (the close increments it)
  PBK_MIN_BEST,      // hook.min_best_episode
  PBK_COLLECT_NNA,   // hook.collect_NNA (0 / 1)
  PBK_CMP_HAS,       // 1: rewards_compare is not empty
  PBK_CMP,           // Python's max(rewards_compare) (double): the first element unless a later one compared greater
  PBK_BESTREWARD,    // hook.bestreward (double)
  PBK_BESTEPISODE,   // hook.bestepisode
  PBK_STOP_KIND,     // 0: StopAfterEpisode, 1: StopAfterEpisodeWithMinSteps
  PBK_STOP_CUR,      // the stop object's cur
  PBK_STOP_LIMIT,    // its episode / step
  PBK_RANDOM_INIT,   // hook.use_random_init (0 / 1)
  PBK_INIT_SEED,     // hook.init_seed
  PBK_INIT_OFF,      // hook._init_off: Philox offset of the member's NEXT initial field
  PBK_INIT_INC,      // ceil(coefficients / 4): what one drawn field consumes
  PBK_FIRED,         // phase 0 -> phase 1 of one close: the stop condition fired in this episode
  PBK_SPARE,
};
// the episode log of a block, int64 [E][M][POP_ELOG]: one entry per member and episode
#define POP_ELOG 4
enum PopElogSlot {
  PEL_REWARD = 0,    // the episode reward (double)
  PEL_STEPS,         // executed control steps n (0: the member was idle)
  PEL_NEW_BEST,      // 1: the episode is the member's new best
  PEL_RAN,           // 1: the member ran this episode
};
struct PopMember {
  const void* actor_p;                         // behaviour actor parameters (acting)
  float *ts, *ta, *tr, *tt;                     // replay traces: state, action, reward, terminal
  uint64_t noise_seed, sample_seed;
  float *Ap, *Ag, *Am, *Av, *Apt, *Cp, *Cg, *Cm, *Cv, *Cpt;   // the small update's learner state
  double *bpA, *bpC;                            // [2][2] beta powers
  float* losses;                                // [2]
};
// one destination of pdec_population_clone: member `dst` takes over member `src`'s learner; bp*: the CURRENT beta-power slots
// (Mlp::bp_sel) of the two members' actors / critics, rows_*: the replay rows that go along (0: the destination keeps its replay)
struct PopClone {
  int src, dst, bpa_src, bpc_src, bpa_dst, bpc_dst;
  long long rows_sa, rows_rt;
};

struct Population : Object {
  int M = 0, cols = 0, dtype = PDEC_F64;
  std::vector<Mlp*> A, C, At, Ct;
  DevBuf tab;                        // PopMember [M]
  DevBuf clones;                     // PopClone [M] (pdec_population_clone)
  DevBuf snap;                       // float* [M][2]: the hooks' best / current actor parameters (pdec_population_set_actor_copies)
  std::vector<Mlp*> snap_nets;       // (their objects: a copy makes their derived images stale)
  long long* rows = nullptr;         // [M][POP_ROW] (the caller's device buffer)
  long long cap = 0, cap1 = 0, after = 0, freq = 1, start_steps = 0;
  int stride = 0, loops = 1, Bu = 1, quirk = 0;
  double gamma = 0.99, rho = 1.0, eta_a = 0, eta_c = 0;   // member 0's at creation: they select the kernel, and hold for
  int member_hyper = 0;                                    // every member unless member_hyper (pdec_population_set_member_hyper)
  Population() : Object(Kind::Population) {}
};

// does pdec_step_glue's single launch serve this case (act.hip)?  pdec_population_create requires it of member 0's actor
bool step_glue_served(const Mlp* M, const Object* o, int dtype, int act_mode, int cols, int64_t n_rt);

}  // namespace pdec

// the population behind handle h at an entry point (the GET_MLP of populations)
#define GET_POP(P, h)                                                           \
  pdec::Population* P = pdec::lookup_as<pdec::Population>(h, pdec::Kind::Population); \
  if (!P) {                                                                     \
    pdec::set_error("%s: bad handle", __func__);                                \
    return PDEC_E_HANDLE;                                                       \
  }
