/* pdeconv_debug.h -- unit-test and measurement entry points of libpdeconv.so that are NOT part of the drop-in surface
 * (include/pdeconv.h): none of them stands in for a callable of the reference.  Used by tests/, bench.py and tools/ only;
 * the Julia glue (the .jl files under julia/) binds nothing from this file. */
#ifndef PDECONV_DEBUG_H
#define PDECONV_DEBUG_H

#include "pdeconv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Unit-test entry of the register-resident wave FFT the fluid kernels are built on (csrc/wave_fft.hpp): nlines
 * lines of `len` complex doubles (device), natural order in and out, unnormalised forward (sgn < 0) / inverse
 * (sgn > 0) with FFTW's conventions (src/fluid_rk4.jl uses FFTW's fft / ifft).  len in {64,128,192,256,384,512,768}, the
 * padded lengths of the plan table (pdec_debug_fluid_wave_table). */
int pdec_debug_wave_fft(const void* in_dev, void* out_dev, int len, int nlines, int sgn);
/* The same for `len` complex floats (the transform of the fp32 fluid environment); twiddles computed in fp64 and rounded
 * once.  len in {64,128,192,256,384,512,768}. */
int pdec_debug_wave_fft_f32(const void* in_dev, void* out_dev, int len, int nlines, int sgn);

/* Measurement aid of bench.py (no reference counterpart): arm = 1 makes the NEXT fused critic pass launched on `critic`
 * (the behaviour critic of a 3-layer pair, src/PDEagent.jl:385-400) record s_memtime / s_memrealtime stamps at its phase
 * boundaries; arm = 0 copies the record of that launch to out13[13] (host): the mean shader cycles of the ten phases per
 * workgroup, their sum, the shader clock in GHz (d s_memtime / d s_memrealtime x 100 MHz) and the workgroup count.
 * Synchronises the stream of the pass. */
int pdec_debug_critic_stamps(pdec_handle critic, int arm, double* out13);
/* Measurement aid (no counterpart in the reference): the fp32 2-D Keller-Segel tile kernel on `nb` trajectories with `reps` RK4
 * sub-steps per launch on the tile held in registers (no halo refresh: timing only), `iters` launches between two events ->
 * microseconds per launch.  What a time-resident form of KellerSegelSetup.jl:213-239 x 32 could at best cost (HISTORY.md round 5). */
int pdec_debug_kseg2d_probe(pdec_handle env, int nb, int reps, int iters, double* us_per_launch);
/* (built only with -DPDEC_DEBUG_PROBES -- `make EXTRA=-DPDEC_DEBUG_PROBES OBJDIR=... OUT=...` --: the PROBE instantiation of the
 * tile kernel is not in the default library, where this entry returns PDEC_E_INVALID) */

/* Measurement aid of bench.py --emulate-ar-us (no reference counterpart): ONE workgroup of one wave that spins on the
 * constant-rate 100 MHz counter for `us` microseconds (<= 10 000) on `hip_stream` -- a stand-in for the latency of a
 * small-message collective on a box with one GPU.  The loop is bounded by the counter AND by an iteration cap. */
int pdec_debug_spin_us(void* hip_stream, double us);

/* Unit-test entry (no reference counterpart): the kernel pdec_ddpg_update_small (sampling = 0) / pdec_ddpg_update_small_rng
 * (sampling != 0) would launch for these four networks, `loops`, `Bu` and `rho`, with the env switches as they are now --
 * launches nothing.  Writes the instantiation's name (e.g. "ddpg_small2f_kernel<2,1,3,1,3>", "ddpg_small_kernel/lds_params=0")
 * to name[name_len] and the dynamic LDS bytes of the launch, slot table included, to *lds_bytes; or returns the error the call
 * would return.  Reported for a broadcast-target call (quirk = 1): "generic_path/reward_groups" (0 bytes) when the critic's
 * reward groups split the minibatch (pdec_ddpg_set_reward_groups, 2 <= g, g L < Bu) -- the call refuses that case and the
 * batched update (pdec_ddpg_update_async) serves it. */
int pdec_debug_small_update_kernel(pdec_handle actor, pdec_handle critic, pdec_handle target_actor, pdec_handle target_critic,
                                   int loops, int Bu, double rho, int sampling, char* name, int name_len, int64_t* lds_bytes);

/* Unit-test entry (no reference counterpart): what the batched DDPG update would launch for these four networks on Bu columns, with
 * the env switches and the networks' streams as they are now -- launches nothing.  which = 0: the critic pass of pdec_ddpg_critic_grads,
 * 1: the actor pass of pdec_ddpg_actor_grads (looks at actor and critic only), 2 / 3: the critic / actor pass of
 * pdec_ddpg_update_async, 4: the acting kernel of pdec_policy_act_rng on Bu states (looks at the actor only).  Writes the
 * instantiation's name -- "ddpg_critic_fused_kernel<9,2>", "ddpg2_actor_kernel<22,2,6>", "policy_act_fused_kernel<1>",
 * "policy_act2_kernel<1,5>", "small_act_kernel", or "generic" for the generic launch sequence -- to name[name_len] and the
 * dynamic LDS bytes of that launch (0 for the last two) to *lds_bytes; or returns the error the call would return.  For which = 2 / 3
 * the name carries the suffix "/adam_apart" where the update runs a fused pass but ADAM and Polyak as launches of their own
 * (2-layer pairs below 64 columns).  Computed by the host code that dispatches (the family selectors of csrc/ddpg.hip, act_route of
 * csrc/act.hip, the visitors and LDS layouts of csrc/mlp_mfma.hip / fused3_*.hpp and csrc/mlp_mfma2.hip / fused2_*.hpp). */
int pdec_debug_batched_update_route(pdec_handle actor, pdec_handle critic, pdec_handle target_actor, pdec_handle target_critic,
                                    int Bu, int which, char* name, int name_len, int64_t* lds_bytes);

/* Unit-test entry (no reference counterpart): the padded weight images of a fused 3-layer network as the device holds them.
 * which = 0: the image the update passes stage from, 1 / 2: the two published copies acting kernels read.  *nfloats = floats of
 * one image (out_host may be null to ask for it), *pub = the copy the next acting kernel reads (0 / 1), *pending = 1 while a
 * deferred finish of this net has not been issued (pdec_ddpg_defer_actor_finish), *paired = how many of its finish launches so
 * far were blocks of a critic's finish launch.  Any out pointer may be null.  Copying an image synchronises the net's stream. */
int pdec_debug_fused_image(pdec_handle mlp, int which, float* out_host, int* nfloats, int* pub, int* pending, int* paired);

/* Unit-test entry (no reference counterpart): the tile plan of pdec_policy_act_members for an actor of this shape under states of
 * `state_dtype` with cols_per_member columns per member -- launches nothing.  *tile_cols = columns per workgroup (the largest
 * multiple of 64 whose two activation buffers [widest layer][tile_cols] fit 48 KB, capped at cols_per_member rounded up to 64;
 * 0: not even 64 fit, the call is not served), *tiles = workgroups per member, *lds_bytes = dynamic LDS of a workgroup. */
int pdec_debug_act_members_plan(pdec_handle actor, int state_dtype, int cols_per_member, int* tile_cols, int* tiles,
                                int64_t* lds_bytes);

/* Unit-test entry (no reference counterpart): the dispatch decisions of a fluid environment (pdec_fluid_env_create), with the env
 * switches as the process read them -- host code only, launches nothing.  out12 = { p (padded line length), nl (lines between the
 * two inverse passes), TL, TLn (lines per LDS tile of the padded / the n x n passes), wave_E, wave_Q, wave_LB (the one-line-per-wave
 * plan WaveFft<E, Q, LB> serving p; 0, 0, 0: the LDS-tile kernels serve it), pair (fluid_k1w_kernel takes a line and its mirror
 * per wave), k2p (the persistent x-pass fluid_k2p_kernel, W tile-major), fused (do_step takes fluid_integrate_wave), nparts (parts
 * the fused env step splits the batch into; 0: unsplit), x-pass tiles (B p / 8 workgroup tiles of fluid_k2p_kernel; 0 without it) }.
 * Computed by the host code that dispatches (csrc/fluid.hip fluid_make and fluid_fused, csrc/fluid_wave.hip k2p_eligible, all
 * three from the environment's row of the plan table below). */
int pdec_debug_fluid_plan(pdec_handle env, int32_t* out12);

/* Unit-test entry (no reference counterpart): the table of one-line-per-wave plans of the fluid environment (csrc/fluid_wave.hip
 * fluid_wave_table), the one place that says which WaveFft<E, Q, LB> serves a padded length and which instantiations exist for
 * it -- host code only: needs no device and no handle.  *nrows = rows of the table; out, where cap >= 14 * *nrows (else
 * PDEC_E_INVALID with *nrows set), receives per row { p, E, Q, LB, then for fp64 and again for fp32: rhs (the un-fused right-hand
 * side is built: 1 / 0), fused (fluid_integrate_wave with fluid_k31w_kernel), k2p (fluid_k2p_kernel), NPW, NSU (the DMA pieces per
 * wave and output elements per thread that instantiation was built for; 0, 0 without one) }. */
int pdec_debug_fluid_wave_table(int32_t* out, int cap, int* nrows);

#ifdef __cplusplus
}
#endif
#endif /* PDECONV_DEBUG_H */
