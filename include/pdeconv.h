/* pdeconv.h -- C ABI of libpdeconv.so: MI355X (gfx950) hot path of
 * janstenner/DistributedConvRL-PDE-Control, hand-written HIP behind plain C.
 *
 * The reference has NO FFI (pure Julia); the seam this library replaces is the set of
 * Julia callables that `PDEenv` / `CustomDDPGPolicy` invoke.  Each entry
 * point below cites the reference callable (file:line, relative to the reference repo) it
 * stands in for.  The Julia `ccall` bindings a maintainer would add are in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns int: 0 = OK, <0 = error (PDEC_E_*); text via pdec_last_error()
 *    (thread-local).  No exceptions cross the boundary.  Blow-up of the PDE is NOT an error:
 *    it sets the per-trajectory `done` flag (src/PDEenv.jl:226-237).
 *  - handles are opaque uint64_t created/destroyed in pairs; a handle is not re-entrant,
 *    distinct handles may be used from distinct threads.
 *  - array arguments of compute calls are DEVICE pointers (pdec_malloc, or any HIP
 *    allocation such as a torch tensor's data_ptr); calls are asynchronous on the handle's
 *    stream (pdec_set_stream; default = the null stream).  The `_host` wrappers take HOST
 *    pointers, stage through plan-owned buffers and return after completion -- these are
 *    what a Julia `do_step(env)` closure binds.
 *  - arrays are dense, batch-major `[B][...Julia column-major...]`: a Julia matrix
 *    `state[ns, A]` of trajectory b starts at `state + b*ns*A` and element (r,a) is at
 *    `a*ns + r`.  dtype (PDEC_F32 / PDEC_F64) is fixed at plan creation; setup-time tables
 *    (sensor kernels, weights in set/get) are passed as documented per call.
 */
#ifndef PDECONV_H
#define PDECONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t pdec_handle;

enum { PDEC_F32 = 0, PDEC_F64 = 1 };

enum {
  PDEC_OK = 0,
  PDEC_E_INVALID = -1,   /* bad argument / unsupported size */
  PDEC_E_HIP = -2,       /* HIP runtime error */
  PDEC_E_HANDLE = -3,    /* unknown / wrong-kind handle */
  PDEC_E_NOGPU = -4,     /* no usable gfx950 device */
  PDEC_E_COMM = -5       /* RCCL error */
};

/* PDE right-hand side / integrator kinds */
enum {
  PDEC_PDE_KS_CNAB2 = 0,     /* scripts/KS/setup/KSSetup.jl:130-160 (what the reference runs) */
  PDEC_PDE_KSEG_RK4 = 1,     /* scripts/Keller-Segel/setup/KellerSegelSetup.jl:213-239 with fixed RK4 */
  PDEC_PDE_KS_RK4_FD = 2,    /* north-star variant: RK4 + periodic 5-point FD (KSSetup.jl:55-59 table) */
  PDEC_PDE_FLUID_RK4 = 3,    /* src/fluid_rk4.jl:122-190 + scripts/Fluid/setup/FluidSetup.jl:163-172 */
  PDEC_PDE_KSEG2D_RK4 = 4    /* BASELINE.json configs[3]: the Keller-Segel rules (KellerSegelSetup.jl:63-66,213-239)
                                along both axes of a 2-D grid; no reference counterpart */
};

enum { PDEC_ACT_IDENTITY = 0, PDEC_ACT_RELU = 1, PDEC_ACT_TANH = 2 };

/* ---------------------------------------------------------------- runtime ------------ */
int pdec_init(int device_ordinal);            /* selects the device, checks gfx950 */
int pdec_shutdown(void);                      /* destroys every live handle */
const char* pdec_last_error(void);
int pdec_version(void);
int pdec_device_count(int* n);

int pdec_malloc(void** dptr, size_t bytes);
int pdec_free(void* dptr);
int pdec_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int pdec_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int pdec_memset(void* dptr, int value, size_t bytes);
int pdec_set_stream(pdec_handle h, void* hip_stream);   /* hipStream_t; NULL = null stream */
/* A non-blocking stream at an explicit priority LEVEL (-1 high, 0 normal, +1 low; clamped to the device's range), made together
 * with its hardware queue.  Why a library call: on this GPU a process's hardware queues are spread over FOUR compute pipes in
 * the order they are made, queue i on pipe i mod 4, and two BUSY queues on one pipe take turns instead of running side by
 * side (tools/c4_stream_matrix.sh, 21 creation orders: config C4 runs at 75 k env-steps/s when the env, update and two
 * part-batch streams sit on four pipes and at 40 - 46 k when two of them share one; HIP also lets at most four queues exist
 * per level and maps further streams of that level onto those).  So the streams that work at the same time -- env stream,
 * update stream, the part streams of pdec_env_set_part_streams -- are made BACK TO BACK by one caller, at most four of them,
 * and kept for the life of the process (queues made after others were destroyed take over the freed slots in an order of
 * their own: a fresh set per pipeline, the old one released, was measured worse than one set used again and again).  The
 * first call also makes the null stream's queue if nothing has yet, so that it cannot land between the caller's later.  A
 * framework's pooled streams give no such control (torch makes each pool stream at its first use).  hipGraph launches make
 * queues of their own for parallel branches; with all four pipes taken by busy streams they share one (C2: graph replay 190 -
 * 260 instead of 125 us per step -- eager issue, 110 us, is what the pipeline uses).  The reference has no counterpart
 * (single stream). */
int pdec_stream_create(void** hip_stream, int level);
int pdec_stream_destroy(void* hip_stream);
int pdec_sync(pdec_handle h);                           /* hipStreamSynchronize of h's stream */
int pdec_destroy(pdec_handle h);                        /* any handle kind */

/* Per-kernel timing with HIP events on the handle's stream (for bench.py's roofline):
 * when enabled every launch of the handle's kernels is bracketed by events. */
int pdec_prof_enable(pdec_handle h, int on);
int pdec_prof_reset(pdec_handle h);
/* name: kernel label, e.g. "ks_env_step", "ddpg_critic"; returns mean ms and launch count */
int pdec_prof_get(pdec_handle h, const char* name, double* mean_ms, int* count);

/* ---------------------------------------------------------------- environment -------- */
/* Configuration of one batched PDE environment = the globals of a reference setup file
 * (scripts/KS/setup/KSSetup.jl:20-77, scripts/Keller-Segel/setup/KellerSegelSetup.jl:26-84)
 * plus the build's batch size. */
typedef struct pdec_env_cfg {
  int pde_kind;            /* PDEC_PDE_* */
  int dtype;               /* PDEC_F32 / PDEC_F64 */
  int B;                   /* trajectories in the batch (reference: 1) */
  int N;                   /* nx: cells per species */
  int n_species;           /* 1 (KS) or 2 (Keller-Segel: rows u,v of y[2,nx]) */
  int S;                   /* number of sensors */
  int A;                   /* number of actuators (columns of state/action) */
  int window;              /* window_size (odd; rows per species = window) */
  int temporal_steps;      /* KellerSegelSetup.jl:48 */
  int mono;                /* 1: global agent (KSglobalSetup.jl): state [S,1], reward [1] */
  int K;                   /* oversampling: CNAB2 sub-steps / fixed RK4 sub-steps per control step */
  int check_max_value;     /* 0 none, 1 "y", 2 "reward" (src/PDEenv.jl:226-240) */
  double Lx;               /* domain length */
  double dt;               /* control interval */
  double mu;               /* KS disturbance amplitude (KSSetup.jl:155); 0 for mono */
  double max_value;        /* blow-up threshold */
  double sensor_scale;     /* sensors = <y,g> * sensor_scale  (1/max_value KS; 1/4 K-S) */
  double agent_power;      /* p = sum_i agent_power * action[i] * kernel_i */
  double reward_in_scale;  /* d = reward_in_scale * (<y,g> + reward_offset*sum(g)) */
  double reward_offset;    /* KS 0; K-S -1 (y-1) */
  double reward_power;     /* r = -|d|^reward_power / reward_denom - ... */
  double reward_denom;
  double action_punish;
  double delta_action_punish;
  /* 2-D fluid (PDEC_PDE_FLUID_RK4) only; ignored by the 1-D kinds.  Square periodic box: N = nx = ny,
   * Lx = Ly; y is the vorticity SPECTRUM, Julia ComplexF64[ny, nx] -> memory [B][nx][ny][re,im]. */
  int ifpad;               /* 1: 3/2-rule de-aliasing (scripts/Fluid/setup/FluidSetup.jl:101) */
  int sensors_per_axis;    /* sensors on a spa x spa grid, S = spa^2 (FluidSetup.jl:61) */
  double nu;               /* viscosity (FluidSetup.jl:28) */
  /* 2-D Keller-Segel (PDEC_PDE_KSEG2D_RK4) only: rows of the grid; N = nx (multiple of 4), square cells dx = Lx/nx */
  int Ny;
  /* time integrator of the right-hand-side kinds (PDEC_PDE_KSEG_RK4, PDEC_PDE_KS_RK4_FD): 0 = classical RK4 (what the
   * setups' do_step use), 1 = PDEenv's built-in explicit midpoint rule, K = `oversampling` sub-steps
   * (src/PDEenv.jl:208-214, taken when no do_step closure is supplied) */
  int integrator;
  /* action memory (scripts/KS/setup/KSSetup.jl:39,48,216-226; src/PDEagent.jl:201; 0 in every shipped script): the actor has
   * 1 + memory_size outputs per actuator; row 0 drives the PDE and the reward, rows 1.. come back as the LAST memory_size rows
   * of the next state (zeros at a reset).  action arrays become [B][A][1 + memory_size], state columns grow by memory_size.
   * Per-actuator kinds of the reference (KS CNAB2, KS RK4+FD, Keller-Segel, fluid); PDEC_E_INVALID for the global agent
 * (mono) and the 2-D Keller-Segel grid. */
  int memory_size;
} pdec_env_cfg;

/* sensor_kernels [S][N], actuator_kernels [A][N] (host, double, row = one kernel: the
 * `gaussians` / `gaussians_actuators` arrays, KSSetup.jl:111-113); a2s [A] 0-based index
 * of the sensor under each actuator (`actuators_to_sensors`).  Replaces the closures built
 * in KSSetup.jl:82-245 / KellerSegelSetup.jl:112-332. */
int pdec_env_create(pdec_handle* h, const pdec_env_cfg* cfg, const double* sensor_kernels,
                    const double* actuator_kernels, const int32_t* a2s);

/* 2-D fluid environment (src/fluid_rk4.jl:122-229 + scripts/Fluid/setup/FluidSetup.jl:139-261).
 * The sensor / actuator kernels are the thresholded Taylor-vortex bumps the reference keeps
 * `sparse` (FluidSetup.jl:139-161); each is passed as the dense BW x BH box around its periodic
 * support: boxes [S][BW][BH] (element (dj, di) at dj*BH + di; di runs along y = the fast axis of
 * the Julia array), origin [S][2] = {j0 (first x column), i0 (first y row)}, 0-based, wrapping
 * periodically; likewise for the A actuators.  The compute calls below then take
 *   y, p   : [B][nx][ny][2]  (spectra; p = fft(forcing), what prepare_action returns, :260)
 *   state  : [B][A][9*temporal_steps], reward [B][A], action [B][A]. */
int pdec_fluid_env_create(pdec_handle* h, const pdec_env_cfg* cfg, int BH, int BW,
                          const double* sensor_boxes, const int32_t* sensor_origin,
                          const double* actuator_boxes, const int32_t* actuator_origin,
                          const int32_t* a2s);

/* 2-D Keller-Segel environment (BASELINE.json configs[3]).  Sensors sit on the tensor grid
 * sensor_y[Sy] x sensor_x[Sx] (0-based cell indices of the box centres; sensor s = iy*Sx + ix), every sensor
 * and actuator kernel is the (2*half_window+1)^2 box of ones of KellerSegelSetup.jl:112-126, clipped at the
 * domain edge; a2s [A] as above (actuator boxes must not overlap).  cfg->N = nx, cfg->Ny = ny = the `ny` argument.
 *   y [B][ny][nx][2] (u,v interleaved; Julia y[2, nx, ny]), p [B][ny][nx], state [B][A][2*window^2*temporal_steps]
 * Feature rows: species u then v (:281-286), inside a species the (i,j) shifts of the 3x3 circular window in the
 * order of scripts/Fluid/setup/FluidSetup.jl:219-223, then the temporal stack (:297-303). */
int pdec_kseg2d_env_create(pdec_handle* h, const pdec_env_cfg* cfg, int ny, int Sx, int Sy,
                           const int32_t* sensor_x, const int32_t* sensor_y, int half_window,
                           const int32_t* a2s);

/* Fluid episode initialiser ic(caseno) (src/fluid_rk4.jl:72-120; taylorvtx :54-69) on the device: y_out[B][nx][ny][2]
 * = fft2 of the sum over nv vortices (9 periodic images each).  vortices: HOST [B][nv][4] = (x0, y0, a0, U_max), the
 * random draws of ic(3)/ic(4) made by the caller (scripts/Fluid/setup/FluidSetup.jl:386-394 generate_random_init). */
int pdec_fluid_ic(pdec_handle h, const double* vortices, int nv, void* y_out);
/* The same with the table already in DEVICE memory (doubles, [B][nv][4]): the launches of pdec_fluid_ic on the
 * environment's stream, no host copy and no synchronisation, so it can stand between two episodes that are enqueued in
 * one go.  An fp32 environment rounds the table once on the device.  y_out is bit for bit what pdec_fluid_ic writes for
 * the same table.  The table must stay valid until the stream has passed the call. */
int pdec_fluid_ic_dev(pdec_handle h, const double* vortices_dev, int nv, void* y_out);
/* ic(3) (caseno 3: nv = 30, training) / ic(4) (caseno 4: nv = 50, evaluation) with the random draws made on the device from
 * the library's Philox4x32-10 stream (seed, offset) instead of by the caller; any other caseno is refused.  One kernel, one
 * thread per (trajectory b, vortex v): counter offset + b nv + v, its four words w0..w3, u_i = (w_i + 0.5) 2^-32 in double
 * (pdec_env_random_init's convention); table row (x0, y0, a0, U) = (u0 Lx, u1 Ly, a0, 2 u3 - 1) with a0 = Lx / 20 (case 3)
 * or (Lx / 20) (0.5 + u2) (case 4).  One call consumes B nv counters, so W environments of B trajectories at offsets
 * o + r B nv draw what one of W B draws at o.  The table [B][nv][4] of doubles lives in a device buffer allocated with the
 * environment (no allocation, host copy or synchronisation in the call) and is also copied to vortices_out when that is not
 * NULL (DEVICE pointer); then the launches of pdec_fluid_ic_dev on the environment's stream (an fp32 environment rounds the
 * table once on the device): y_out is bit for bit pdec_fluid_ic_dev of that table. */
int pdec_fluid_ic_rng(pdec_handle h, uint64_t seed, uint64_t offset, int caseno, double* vortices_out, void* y_out);

/* error_detection of the fluid script (scripts/Fluid/setup/FluidSetup.jl:263-273) per trajectory, on the device:
 * w = real(ifft2(y[b])) through the library's own inverse passes (the sensing's), then errored_out[b] (device, int32 [B])
 * = 1 when the maximum over all cells of |w[i][j] - w[i-1][j]| and |w[i][j] - w[i][j-1]| (periodic along both axes)
 * exceeds 10, else 0.  The maximum propagates NaN, as the host function's does: errored_out[b] = 1 exactly when some
 * difference is above 10 (+inf included) and no difference is NaN.  A spectrum with a non-finite entry therefore yields 0
 * (its w is NaN wherever the entry reaches, and NaN > 10 is false).
 * Runs on the environment's stream and uses the environment's work arrays (the ones featurize and the step's sensing
 * use), so it must not overlap a step, featurize, reward or initialiser call of the same environment on another stream;
 * y itself is only read.  An environment that steps its batch in parts serves the whole batch here from its own arrays. */
int pdec_fluid_error_detection(pdec_handle h, const void* y, int32_t* errored_out);

/* prepare_action(; env): p[B][N] from action[B][A]      (KSSetup.jl:231-245) */
int pdec_actuate(pdec_handle h, const void* action, void* p_out);
/* do_step(env): y_out[B][n_species*N] from y_in, p[B][N]; done[B] int32 (bit0 = blow-up,
 * only when check_max_value==1)                           (KSSetup.jl:130-160, PDEenv.jl:216-228) */
int pdec_pde_step(pdec_handle h, const void* y_in, const void* p, void* y_out, int32_t* done);
/* featurize(; env): state_out[B][A][ns] from y and the previous state (temporal_steps>1;
 * may be NULL = constructor/reset form, KSSetup.jl:190-229, KellerSegelSetup.jl:265-316) */
int pdec_featurize(pdec_handle h, const void* y, const void* prev_state, void* state_out);
/* the same with the action the environment holds (cfg.memory_size > 0: rows 1.. of `action` [B][A][1 + memory_size] become the
 * last memory_size rows of every state column, KSSetup.jl:220-226; action NULL = pdec_featurize = the reset form: zeros) */
int pdec_featurize_action(pdec_handle h, const void* y, const void* prev_state, const void* action, void* state_out);
/* reward_function(env): r_out[B][A] (or [B][1] mono)      (KSSetup.jl:162-178) */
int pdec_reward(pdec_handle h, const void* y, const void* action, const void* action_prev,
                void* r_out);
/* (env::PDEenv)(action), src/PDEenv.jl:195-241, in ONE launch: delta_action, prepare_action,
 * integrator, reward, featurize, blow-up flag.  y_out may alias y_in; state_out must not
 * alias state_prev when temporal_steps>1.  p_out may be NULL. */
int pdec_env_step(pdec_handle h, const void* y_in, const void* action, const void* action_prev,
                  const void* state_prev, void* y_out, void* p_out, void* state_out,
                  void* reward_out, int32_t* done);
/* Optional extra output of pdec_env_step for the batched DDPG update: terminal_per_column
 * [B][A] (mono: [B][1]) of the plan's dtype, 1.0 on every actuator column of a trajectory that
 * blew up in this step (the `terminal` trace RL.jl fills per actuator, src/PDEagent.jl:284-288),
 * 0.0 otherwise.  NULL (default) disables it.  The pointer is read at each later pdec_env_step.
 * The fluid environment writes the rows in its sensing launch (no further launch): the flag of check_max_value 2 as that
 * launch reduces it, the flag of check_max_value 1 as the spectrum test left it (in a slot of the environment's own when
 * done is NULL), zeros when the test is off; a batch stepped in parts writes each part's slice.  The rows go out with the
 * rewards: pdec_env_step refuses a NULL reward_out, so every accepted step writes them. */
int pdec_env_set_terminal_out(pdec_handle h, void* terminal_per_column);
/* RHS evaluation for known-answer tests: out = f(y, p)    (KellerSegelSetup.jl:213-232) */
int pdec_rhs_eval(pdec_handle h, const void* y, const void* p, void* out);

/* Host-pointer forms (synchronous) -- what Julia's do_step/featurize closures bind. */
int pdec_pde_step_host(pdec_handle h, const void* y_in, const void* p, void* y_out, int32_t* done);
int pdec_env_step_host(pdec_handle h, const void* y_in, const void* action, const void* action_prev,
                       const void* state_prev, void* y_out, void* p_out, void* state_out,
                       void* reward_out, int32_t* done);

/* ---------------------------------------------------------------- networks ----------- */
/* Chain(Dense...) with weights shared across columns (src/PDEagent.jl:14-56).
 * dims[n_layers+1], acts[n_layers].  params_host: Flux.params order W1,b1,W2,b2,... each W
 * in Julia column-major [out,in] (element (o,i) at i*out+o), dtype = the plan's dtype; NULL
 * = zeros.  max_cols = largest number of columns any later call will pass. */
int pdec_mlp_create(pdec_handle* h, int dtype, int n_layers, const int32_t* dims,
                    const int32_t* acts, const void* params_host, int max_cols);
int pdec_mlp_num_params(pdec_handle h, int* n);
int pdec_mlp_set_params(pdec_handle h, const void* params_host);   /* Flux.loadparams!  (custom_nna.jl:26-27) */
int pdec_mlp_get_params(pdec_handle h, void* params_host);         /* Flux.params -> host (checkpoint)      */
int pdec_mlp_copy(pdec_handle dst, pdec_handle src);               /* copyto!(dst, src)  (custom_nna.jl:26)  */
/* app(x): x [cols][in] (= Julia [in, cols]), y_out [cols][out]    (custom_nna.jl:13) */
int pdec_mlp_forward(pdec_handle h, const void* x, int cols, void* y_out);
/* forward + backward of sum(dy .* app(x)): grads_out (device, layout of get_params, may be
 * NULL -> only the internal gradient buffer is filled), dx_out [cols][in] may be NULL */
int pdec_mlp_backward(pdec_handle h, const void* x, const void* dy, int cols, void* dx_out,
                      void* grads_out);
/* device pointer + length of the internal flat gradient buffer (for an external all-reduce) */
int pdec_mlp_grad_buffer(pdec_handle h, void** dptr, int* n);
/* update!(app, gs) with Flux.Optimise.ADAM semantics (custom_nna.jl:23-24); uses the
 * internal gradient buffer */
int pdec_adam_step(pdec_handle h, double eta, double beta1, double beta2, double eps);
int pdec_adam_get_state(pdec_handle h, void* m_host, void* v_host, double* beta_pow2);
int pdec_adam_set_state(pdec_handle h, const void* m_host, const void* v_host, const double* beta_pow2);
/* dest .= rho .* dest .+ (1-rho) .* src                          (src/PDEagent.jl:415-417)
 * Every `rho` of this header: the reference's loop runs over Flux.params([At, Ct]), which is empty (src/custom_nna.jl:20 defines a
 * functor of its own), so its targets never move; a caller reproduces the reference AS IT RUNS with rho = 1 (dest = 1*dest +
 * 0*src, exact) and the loop as written with rho = policy.p. */
int pdec_polyak(pdec_handle dst, pdec_handle src, double rho);

/* update!(app, gs) immediately followed by the Polyak step of the app's target network
 * (src/custom_nna.jl:23-24 + src/PDEagent.jl:415-417 for one network pair) in ONE launch; gradients are
 * taken from the internal gradient buffer (e.g. after pdec_allreduce_grads).  Polyak of a target only
 * depends on its own behaviour network, so doing it right after that network's ADAM step is equivalent
 * to the reference's order. */
int pdec_adam_polyak_step(pdec_handle h, pdec_handle h_target, double eta, double beta1, double beta2,
                          double eps, double rho);

/* T control steps in one call, no host round trip per step: for t = 0..T-1
 *   action_t = clamp(actor(state_t) + randn * act_noise, +-act_limit)   (src/PDEagent.jl:183-207, pdec_policy_act_rng
 *              with noise offset `offset + t * ceil(cols*na/4)`; learning = 0 -> no noise)
 *   (y, state, reward, done) = (env::PDEenv)(action_t)                  (src/PDEenv.jl:195-241, pdec_env_step)
 * all enqueued on the environment's stream (the actor handle must use the same stream and dtype).  In/out device
 * arrays: y, state, action (in: the previous action, for delta_action; out: the last one).  Optional outputs (NULL to
 * skip): reward_sum [B][A] += every step's reward; log_y / log_p / log_action / log_reward: [T][...] rows of the
 * trajectory (what PDEhook logs per step, src/PDEhook.jl:54-62); done_any [B] = OR of the step flags, done_step [B] =
 * first step that raised a flag (-1: none).  The reference stops an episode at `done`; a rollout keeps integrating
 * (blown-up trajectories saturate to inf/NaN) and reports the step, the caller discards what follows it.
 * KS (CNAB2, per-actuator agents, temporal_steps = 1, actor of <= 3 Dense layers no wider than 32 with one output):
 * ONE persistent launch for all T steps -- a workgroup keeps its two trajectories in registers and their state / actions
 * in LDS between steps and evaluates the actor itself on the vector unit (k-ordered sums like the oracle; not the
 * summation order of the MFMA acting kernel, so fp32 actions agree with the per-step loop to ~1e-6, not bit for bit).
 * 1-D Keller-Segel (per-actuator agents, any temporal_steps, same actor limits; scripts/Keller-Segel/setup/
 * KellerSegelSetup.jl:213-332): likewise one launch, one workgroup per trajectory.
 * PDEC_ROLLOUT_PERSISTENT=0 selects the per-step form, which every other configuration uses (same kernels as the loop
 * pdec_policy_act_rng -> pdec_env_step, bit-identical to it). */
int pdec_rollout(pdec_handle env, pdec_handle actor, int T, void* y, void* state, void* action,
                 double act_noise, double act_limit, int learning, uint64_t seed, uint64_t offset,
                 void* reward_sum, void* log_y, void* log_p, void* log_action, void* log_reward,
                 int32_t* done_any, int32_t* done_step);
/* The same for M actors at once (population.py: evaluate_actors): the environment's batch is B = M * per_member trajectories,
 * trajectory b is driven by actors[b / per_member], and the whole call is ONE persistent launch in which every workgroup takes
 * its actor from a device table.  Array shapes and the in / out contract are pdec_rollout's.  Greedy only: learning must be 0
 * (the exploration noise of pdec_rollout is numbered by global column, not per member; learning = 1 is an error).  Unlike
 * pdec_rollout the actors may live on another stream -- the caller orders the streams -- and in another dtype: Float32
 * parameters under an fp64 environment (the reference's shape) are promoted while a workgroup fills its LDS image, which is
 * exactly the image a promoted copy of the actor (pdec_mlp_copy into an fp64 network) would load.  KS: a workgroup's two
 * trajectories belong to one member (workgroup w: member w / ceil(per_member / 2), trajectories 2 (w % ceil(per_member / 2))
 * and the next of that member, if it has one) -- the pairing of a solo launch on per_member trajectories, so every member's
 * results are bit for bit those of pdec_rollout on its block alone.
 * Fluid and 2-D Keller-Segel (no persistent launch): *served = 2, "batched step loop" -- the T control steps of pdec_rollout's
 * per-step form enqueued ONCE on the B = M * per_member environment, with pdec_policy_act_members on per_member * A columns per
 * member in the place of the acting call (same pdec_env_step, reward sums, flags, log rows and copy-back).  A trajectory's
 * step does not depend on B or on its place in the batch in those environments, so here too every member's results are bit
 * for bit those of pdec_rollout on its block alone.  Served when pdec_policy_act_members serves the actors (see there); not
 * with the global agent or memory_size > 0.
 * *served = 0 and nothing is enqueued when the environment / actor shape is not one the persistent launches of pdec_rollout
 * or the batched step loop cover, when the actors differ in shape or dtype, when their parameters are neither Float32 nor of
 * the environment's dtype, or -- KS and 1-D Keller-Segel -- with PDEC_ROLLOUT_PERSISTENT=0: the caller then loops over
 * pdec_rollout. */
int pdec_rollout_members(pdec_handle env, const pdec_handle* actors, int M, int per_member, int T, void* y, void* state,
                         void* action, double act_limit, int learning, void* reward_sum, void* log_y, void* log_p,
                         void* log_action, void* log_reward, int32_t* done_any, int32_t* done_step, int* served);

/* policy act: actions[cols][na] = clamp(actor(state) + noise*act_noise, +-act_limit)
 * (src/PDEagent.jl:183-207).  noise [cols][na] device standard normals or NULL (-> no noise,
 * `learning=false`). */
int pdec_policy_act(pdec_handle actor, const void* state, const void* noise, int cols,
                    double act_noise, double act_limit, void* actions_out);
/* the same with the exploration noise drawn inside the kernel from the counter-based generator of
 * pdec_randn (identical numbers: element i of the stream (seed, offset) belongs to column i);
 * learning = 0 -> no noise (`learning=false`, src/PDEagent.jl:199).  One launch for 3-layer fp32 actors. */
/* exploration noise on the first `rows` outputs of the actor only (-1 = all, the default): with action memory the reference
 * adds noise to the driving row and leaves the memory rows as the actor produced them (src/PDEagent.jl:201:
 * actions[1:end-memory_size, :] += randn * act_noise); the clamp applies to every row.  Philox element numbering unchanged
 * (element = column * outputs + row; the memory rows' draws are skipped). */
int pdec_mlp_set_noise_rows(pdec_handle actor, int rows);
/* exploration amplitude per trajectory instead of one per call (src/PDEagent.jl:199-201 adds randn * act_noise with the agent's
 * one act_noise; a batch of trajectories explores at a ladder of levels): scale_dev is a device array of n doubles that the
 * caller keeps alive -- the pointer is stored, nothing is copied or synchronised, so a value written into the array on the acting
 * stream serves the next launch, a recorded call and a captured graph alike.  NULL returns to the scalar.  With an array set,
 * column c of an acting call adds z * (T)scale[c / cols_per_entry] (T: the type the kernel computes in) where it added
 * z * (T)act_noise: an array of equal values is the scalar call bit for bit.  The call's act_noise is not read; learning = 0 still
 * means no noise; noise rows, the clamp and the Philox element numbering are unchanged.  Served by pdec_policy_act (with noise),
 * pdec_policy_act_rng, _rng_as, _rng_dev, pdec_step_glue and pdec_rollout with learning = 1 (in a persistent launch the global
 * column is b A + a; the workgroup keeps its columns' amplitudes in LDS, and a configuration which that pushes over the 64 KB
 * bound takes the step loop).  A call whose cols is not n * cols_per_entry is refused (PDEC_E_INVALID).  Not served:
 * pdec_population_create refuses a member whose actor has an array set (members carry their amplitude in the row table); the
 * member forms (pdec_rollout_members, pdec_policy_act_members) are greedy and do not read it. */
int pdec_mlp_set_noise_scale(pdec_handle actor, const double* scale_dev, int64_t n, int cols_per_entry);
/* temporally correlated (Ornstein-Uhlenbeck / AR(1)) exploration noise in the place of the white draw (src/PDEagent.jl:201 adds
 * randn * act_noise, fresh at every control step; an integrator low-pass filters that away within a few steps).  Every noise
 * element i = column * outputs + row keeps a state x[i], a double whatever the kernel's type.  An acting call with learning = 1
 * draws z = the normal the white call draws for element i (stream numbering and the device counter unchanged) and computes, in
 * double,  x[i] = a_e x[i] + b_e z  with e = column / cols_per_entry, stores it back, and adds (T)x[i] * amp_c where the white
 * call added (T)z * amp_c; amp_c is the call's act_noise, or entry e of the array of pdec_mlp_set_noise_scale when one is set
 * (the two cols_per_entry must then be equal: refused by the acting call otherwise).  a_e in [0, 1) is the step-to-step
 * correlation and b_e = sqrt(1 - a_e^2) keeps the stationary variance at 1, so act_noise and the scale array mean what they
 * meant; a = 0, b = 1 gives x = z exactly and the white call bit for bit.  Rows >= the noise rows are neither read nor written,
 * and a call with learning = 0 touches nothing.
 *   state_dev [n * cols_per_entry * outputs] doubles, ab_dev [n][2] doubles {a, b}: device arrays the caller keeps alive and
 * zeroes (or fills) at an episode's start.  The pointers are stored, nothing is copied or synchronised: values written into
 * either array on the acting stream between launches serve the next launch, a recorded call and a captured graph alike.
 * state_dev = NULL switches it off.  Refused (PDEC_E_INVALID): n < 1, cols_per_entry < 1, a product n * cols_per_entry * outputs
 * beyond 2^31 - 1, ab_dev NULL with a state set; and by every acting call, a column count that is not n * cols_per_entry.
 *   Served by pdec_policy_act (with noise: the caller's noise[] is z), pdec_policy_act_rng, _rng_as, _rng_dev and pdec_step_glue,
 * on every kernel these reach; which kernel a shape reaches does not depend on it (pdec_debug_batched_update_route).  Refused
 * by name while a state is set: pdec_rollout with learning = 1 (the persistent and the host-enqueued exploring rollouts), the
 * member forms pdec_policy_act_members and pdec_rollout_members, and pdec_population_create, hence the member glue
 * (pdec_population_glue).  In Python, Population refuses such a member and TrainPipeline(episodes="per_trajectory") the option:
 * a restarted trajectory would have to zero its rows inside the boundary launch. */
int pdec_mlp_set_noise_color(pdec_handle actor, double* state_dev, const double* ab_dev, int64_t n, int cols_per_entry);
int pdec_policy_act_rng(pdec_handle actor, const void* state, int cols, double act_noise, double act_limit,
                        int learning, uint64_t seed, uint64_t offset, void* actions_out);
/* agent(env) where the environment computes in `state_dtype` and the actor keeps parameters of another type -- the reference's
 * case: fp64 fields, Float32 networks (src/PDEagent.jl:183-207 promotes in the broadcast) -- without a promoted copy of the
 * actor: when the single-launch acting kernel for few columns covers the case (<= 4 layers, activations of both buffers within
 * 48 KB of LDS) the action is enqueued and *served = 1; otherwise nothing is enqueued, *served = 0, and the caller acts through a
 * clone of the actor in `state_dtype` (pdec_mlp_copy + pdec_policy_act_rng).  Same arithmetic, bit for bit, either way. */
int pdec_policy_act_rng_as(pdec_handle actor, int state_dtype, const void* state, int cols, double act_noise, double act_limit,
                           int learning, uint64_t seed, uint64_t offset, void* actions_out, int* served);
/* agent(env), greedy, of M actors of one shape on ONE state matrix in one launch (act_members_kernel): state [M * cols_per_member][ns]
 * and actions_out [M * cols_per_member][na] of the environment's dtype, member m owns columns m * cols_per_member ... and is
 * driven by actors[m] (Float32 parameters, promoted on the fly, or parameters of the environment's dtype; any stream -- the
 * caller orders them).  Runs on the environment's stream; the environment owns the device table of parameter pointers.  The
 * arithmetic is pdec_policy_act_rng's with learning = 0 on each block alone, bit for bit.  No noise path: the exploration stream
 * is numbered by global column.  *served = 0 and nothing is enqueued when the actors' shapes, activations or dtypes differ, when
 * the parameter dtype is neither Float32 nor the environment's, with more than 4 layers or a widest layer of which a tile of
 * 64 columns does not fit 48 KB of LDS, or when pdec_policy_act_rng on cols_per_member states of an actor of the
 * environment's dtype would take a fused MFMA acting kernel (fp32 environments only; those kernels sum in another order). */
int pdec_policy_act_members(pdec_handle env, const pdec_handle* actors, int M, const void* state, int cols_per_member,
                            double act_limit, void* actions_out, int* served);
/* The glue between two control steps of a single-trajectory training loop in ONE launch (src/PDEagent.jl:276-289, :175-209,
 * :254-274 in the order RL.jl's run loop calls them): pdec_replay_push_rt of the step that just ran (n_rt == 0: none), then
 * agent(env) for the next step -- act_mode 1: pdec_policy_act_rng_as on `state` [cols][ns] of type `dtype` with learning = 1;
 * 2: the zero action of the start policy; 0: none --, then pdec_replay_push_sa of (state, that action) (n_sa == 0: none; the
 * action rows are zero when act_mode == 0).  The episode halt flag of `trajectory_handle` (pdec_set_episode_halt) is honoured
 * and raised as by the three calls.  *served = 0 and nothing enqueued when the case is not the single-workgroup one (the caller
 * then makes the three calls): the actor's and the trajectory handle's streams differ, the acting call would not be served by
 * pdec_policy_act_rng_as, or a push does not fit one block.  Same stores, bit for bit.  done_event (0: none): an event of
 * pdec_event_create that the launch carries as its own completion event -- what pdec_event_record right behind the call would
 * give, without the record's packet in the stream (cf. pdec_mlp_set_stop_event). */
int pdec_step_glue(pdec_handle actor, pdec_handle trajectory_handle, int dtype, const void* reward, const int32_t* done_flags,
                   int cols_per_traj, int force_terminal, void* reward_trace, void* terminal_trace, int64_t capacity,
                   int64_t start_rt, int64_t n_rt, int act_mode, const void* state, int cols, double act_noise, double act_limit,
                   uint64_t seed, uint64_t offset, void* actions_out, void* state_trace, void* action_trace,
                   int64_t capacity_rows, int64_t start_sa, int64_t n_sa, pdec_handle done_event, int* served);
/* would pdec_step_glue serve (act_mode, cols columns of type dtype, a POST_ACT push of n_rt values)?  Nothing is enqueued. */
int pdec_step_glue_served(pdec_handle actor, pdec_handle trajectory_handle, int dtype, int act_mode, int cols, int64_t n_rt, int* served);
/* the same with the noise counter kept ON THE DEVICE (one per actor handle): the kernel reads the current counter and
 * one of its threads stores the advanced value (+ ceil(cols*na/4) when learning), so no launch argument depends on how
 * many calls came before -- the form a captured HIP graph of the control step replays (pdec_capture_begin).
 * pdec_noise_counter_set / _get move the counter (they synchronise the actor's stream). */
int pdec_policy_act_rng_dev(pdec_handle actor, const void* state, int cols, double act_noise, double act_limit,
                            int learning, uint64_t seed, void* actions_out);
/* 1 when the acting kernels of this actor read a PUBLISHED, double-buffered copy of its weights that a concurrent
 * update does not write (fp32 3-layer actors on the fused path); 0 when they read the parameters in place -- a caller that
 * overlaps acting and updating must then order the update's actor half behind the acting kernel. */
int pdec_mlp_acts_on_published_copy(pdec_handle actor, int* yes);
int pdec_noise_counter_set(pdec_handle actor, uint64_t value);
int pdec_noise_counter_get(pdec_handle actor, uint64_t* value);
/* fill dst[n] with standard normals from a counter-based generator (replaces randn(rng),
 * src/PDEagent.jl:201) */
int pdec_randn(pdec_handle any_handle, void* dst, size_t n, int dtype, uint64_t seed, uint64_t offset);

/* DDPG update (src/PDEagent.jl:363-418) split at the points where a data-parallel run
 * all-reduces gradients.  s,snext [Bu][ns]; a [Bu][na]; r [Bu]; t [Bu] (same dtype; 0/1).
 * quirk=1 reproduces the reference's (1xBu).+(Bu) broadcast of the reward,
 * quirk=0 is the diagonal TD target.  grad_scale multiplies the gradients (1/world_size for
 * a data-parallel mean).  Losses are written to device scalars (dtype of the plan). */
int pdec_ddpg_critic_grads(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                           const void* s, const void* a, const void* r, const void* t,
                           const void* snext, int Bu, double gamma, int quirk, double grad_scale,
                           void* critic_loss_dev);
int pdec_ddpg_actor_grads(pdec_handle A, pdec_handle C, const void* s, int Bu, double grad_scale,
                          void* actor_loss_dev);
/* whole update on one device: critic grads, ADAM(C), actor grads, ADAM(A), Polyak x2;
 * losses returned to host (synchronises). */
int pdec_ddpg_update(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                     const void* s, const void* a, const void* r, const void* t, const void* snext,
                     int Bu, double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                     double* actor_loss, double* critic_loss);

/* whole update on one device WITHOUT host synchronisation: losses_dev[0] = critic loss, [1] = actor loss
 * (device scalars of the plan's dtype, may be NULL).  For 3-layer fp32 nets this is 4 launches: critic
 * pass, slab-reduce + ADAM(C) + Polyak(Ct), actor pass, slab-reduce + ADAM(A) + Polyak(At). */
int pdec_ddpg_update_async(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                           const void* s, const void* a, const void* r, const void* t, const void* snext,
                           int Bu, double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                           void* losses_dev);

/* The reference's actual update shape -- `update_loops` updates per control step on minibatches of `batch_size`
 * transitions (src/PDEagent.jl:342-418; KSSetup.jl:66-71: 20 x 3) -- in ONE launch: minibatch gather from the
 * device-resident replay traces (pde_fetch!, :323-340), the whole update, repeated `loops` times by one workgroup.
 * Traces (fp32, as RL.jl keeps them, :112-117): state [slots][ns], action [slots][na], reward [slots],
 * terminal [slots] (0/1).  idx_s / idx_rt / idx_sn: device int32 [loops][Bu] slots of (s,a), (r,t) and s',
 * drawn by the host as pde_sample does (:317-321).  fp32 networks of up to 4 layers, 1 <= Bu <= 16.
 * losses_dev (may be NULL): [critic, actor] loss of the last loop.  No host synchronisation. */
int pdec_ddpg_update_small(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                           const void* state_trace, const void* action_trace, const void* reward_trace,
                           const void* terminal_trace, const int32_t* idx_s, const int32_t* idx_rt,
                           const int32_t* idx_sn, int loops, int Bu, double gamma, double rho, int quirk,
                           double eta_actor, double eta_critic, void* losses_dev);

/* The batch-mean reward of the reference's (1 x Bu) .+ (Bu) broadcast (quirk = 1) reduced AHEAD of the
 * update: pdec_reward_mean(h, r, n, mean_out) sums the fp32 rewards r [n] in a fixed order on h's stream (the producer of
 * r -- the env step -- does it beside the running update) and pdec_ddpg_set_reward_mean hands the device scalar to the
 * NEXT critic pass of `critic`, which then does not read r for the mean (one hand-over per update; fp32 fused paths). */
int pdec_reward_mean(pdec_handle any_handle, const void* r, int n, void* mean_out);
/* For callers that run the fused KS step beside the f32-MFMA update passes on a second stream (the two-stream training
 * step): launch the step in the form that needs <= 64 VGPRs -- per-mode constants in LDS instead of registers -- so that a
 * wave of it can share a SIMD with two waves of the 222-VGPR critic pass instead of excluding a whole workgroup of it
 * (and being excluded by it) per CU; that form also runs at wave priority 3.  Alone it is slower (37 vs 29 us at C2), so
 * it is off by default.  *effective = 1 when the environment has such a form (KS CNAB2, N = 256, fp32), else 0. */
int pdec_env_set_simd_sharing(pdec_handle env, int on, int* effective);
/* For the same callers: launch the fused KS step with one trajectory pair spread over TWO waves (128-thread workgroups, two
 * points per lane, FftWave256x2), which puts 0.6 of the one-wave step's vector instructions on each SIMD it touches; the results are bit
 * for bit those of the one-wave step.  *effective = 1 when the next fused step takes that form (KS CNAB2, N = 256, fp32,
 * register-resident engine, no disturbance array, no faults, not the SIMD-sharing form, not the member layout), else 0; the launch re-reads the rule,
 * so an array set later returns the step to its one-wave kernel.  Off by default: alone it is 1.3 us slower; beside the update passes the training step measured 1.9 % shorter. */
int pdec_env_set_two_wave_step(pdec_handle env, int on, int* effective);
/* the same without any extra launch for the fused KS steps + 3-layer fused critic: every later pdec_env_step also writes the
 * sum of the rewards of each of its workgroups (CNAB2: two trajectories each, RK4 + FD: one) to partial_sums [*n_partials]
 * (fp32; NULL switches it off), and pdec_ddpg_set_reward_partials hands them to the next critic pass, which adds them in a
 * fixed order. */
int pdec_env_set_reward_partials_out(pdec_handle env, void* partial_sums, int* n_partials);
/* Environments that run parts of their batch on streams of their own (2-D Keller-Segel: the RK4 sub-steps of C4 in three
 * parts; fluid: child environments) make those streams themselves by default.  pdec_env_part_streams tells how many the step
 * uses besides the environment's own; pdec_env_set_part_streams hands over the caller's instead (made back to back with its
 * pipeline streams, see pdec_stream_create; the library's are released, the caller's are never destroyed by the library).
 * Fewer than asked for: 2-D Keller-Segel runs that many parts + 1 (0: unsplit), fluid refuses (PDEC_E_INVALID).  Environments
 * without parts accept and ignore the call.  Same results bit for bit either way.
 * The library's own part streams (and their events) are made at the FIRST split step, not at environment creation -- by then
 * the environment's stream, whose priority level they take, is known.  Nothing can be created while a stream is being
 * captured, so a caller that opens pdec_capture_begin before any eager step must either run one step first or hand over its
 * own streams with pdec_env_set_part_streams; otherwise the captured step returns PDEC_E_INVALID naming this. */
int pdec_env_part_streams(pdec_handle env, int* n);
int pdec_env_set_part_streams(pdec_handle env, void* const* hip_streams, int n);
int pdec_ddpg_set_reward_partials(pdec_handle critic, const void* partial_sums, int n);
int pdec_ddpg_set_reward_mean(pdec_handle critic, const void* mean_dev);

/* Reward groups: the reference's broadcast target (quirk = 1) read at batch scale.  The reference updates on minibatches of
 * g = batch_size transitions (KSSetup.jl:66: 3); an update of Bu columns is taken as the mean of Bu / g such minibatch losses.
 * Column c belongs to group (c / (g L)) L + c % L -- with interleave L = A (columns c = b A + a of B trajectories of A
 * actuators) group members are actuator a of g consecutive trajectories, with L = 1 g consecutive columns.  With r_bar(c)
 * the mean reward of c's group (summed in member order, the same in every group) and d_c = gamma (1 - t_c) q'_c - q_c:
 *   dL/dq_c = -(2 / Bu) (r_bar(c) + d_c),   loss = mean(d^2) + 2 mean_c(d_c r_bar(c)) + mean(r^2),
 * the mean over groups of the reference's per-group loss mean_ij (r_j + d_i)^2.  Bu % (g L) == 0 is required
 * (PDEC_E_INVALID otherwise).  g = 1 is the diagonal target (quirk = 0) and g L >= Bu the whole-batch broadcast: both run
 * the existing passes unchanged.  Otherwise one extra launch ahead of the critic pass, on the critic's stream, writes the
 * per-column group means and the loss term mean_c (r_c - r_bar(c))^2, and the pass runs as the diagonal target on those
 * means; the whole-batch hand-overs (pdec_ddpg_set_reward_mean / _partials) are not read.  Sticky on the critic handle,
 * g = 0 switches it off; it applies to pdec_ddpg_critic_grads, pdec_ddpg_update(_async), the critic half and the split
 * multi-rank sequence, with fp32 and fp64 critics.  pdec_ddpg_update_small(_rng) serve g = 1 and g L >= Bu and refuse the
 * rest.  Groups that never span ranks (B_local % g == 0 with L = A) make N ranks compute one rank's gradient on the
 * concatenated batch. */
int pdec_ddpg_set_reward_groups(pdec_handle critic, int g, int L);

/* the same with pde_sample (src/PDEagent.jl:317-321) INSIDE the kernel: draw k = loop * Bu + column is word k % 4 of the
 * Philox block (seed; counter offset + k / 4), ind = (word * (n_valid - stride)) >> 32, logical index
 * max(0, n_rt - capacity) + ind, slots (lg mod (capacity + stride), lg mod capacity, (lg + stride) mod (capacity + stride)).
 * n_valid = length(trajectory) = min(n_rt, capacity), n_rt = entries ever pushed to the reward / terminal traces,
 * stride = number of columns one control step pushes (number_actuators x batch).  The host passes a seed and an
 * offset, no index arrays. */
int pdec_ddpg_update_small_rng(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                               const void* state_trace, const void* action_trace, const void* reward_trace,
                               const void* terminal_trace, int loops, int Bu, uint64_t seed, uint64_t offset,
                               int64_t n_valid, int64_t n_rt, int64_t capacity, int stride, double gamma, double rho,
                               int quirk, double eta_actor, double eta_critic, void* losses_dev);

/* the two halves of pdec_ddpg_update_async as separate calls (critic half: critic pass + ADAM(C) + Polyak(Ct);
 * actor half: actor pass with the updated critic + ADAM(A) + Polyak(At)), so that a caller can order the
 * actor half behind a concurrent reader of the actor's weights on another stream.  losses_dev as above. */
int pdec_ddpg_update_critic_async(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                                  const void* s, const void* a, const void* r, const void* t, const void* snext,
                                  int Bu, double gamma, double rho, int quirk, double eta_critic, void* losses_dev);
int pdec_ddpg_update_actor_async(pdec_handle A, pdec_handle C, pdec_handle At, pdec_handle Ct,
                                 const void* s, int Bu, double rho, double eta_actor, void* losses_dev);
/* Frozen targets (rho == 1), fused 3-layer family: the finish launch of the actor half (slab reduction + ADAM + image
 * refresh) need not be a launch of its own.  While armed, pdec_ddpg_update_actor_async(.., rho = 1, ..) launches the pass and
 * leaves the finish PENDING, and the next pdec_ddpg_update_critic_async issues it as extra blocks of the critic's own finish
 * launch (the critic half reads nothing it writes): three launches per update instead of four, the same bits in every buffer.
 * While a finish is pending, calls that read what it writes (acting, another actor pass, pdec_adam_polyak_step on the actor)
 * are refused; the caller keeps the order critic half -> acting.  on = 0 disarms and flushes.  *armed: 1 when armed; 0 when
 * declined (another family, rho != 1) -- then, as with a later call that passes rho != 1, the sequence is the plain one.
 * A stop event set on the actor (pdec_mlp_set_stop_event) stays with the pending finish: a flush carries it on its launch,
 * the paired launch records it behind itself (and carries the critic's). */
int pdec_ddpg_defer_actor_finish(pdec_handle A, int on, double rho, int* armed);
/* the pending finish as a launch of its own on the actor's stream; no-op when nothing is pending */
int pdec_ddpg_flush_actor_finish(pdec_handle A);

/* ---------------------------------------------------------------- replay ---- */
/* The trajectory glue of src/PDEagent.jl:237-340 on device-resident traces (fp32, as RL.jl keeps them, :112-117):
 * state [capacity + stride][ns], action [capacity + stride][na], reward [capacity], terminal [capacity].  The host
 * keeps only the two entry counters (pop of the dummy (s, a) of an episode end, :237-252, is a counter decrement).
 * PRE_ACT push of one (s, a) column per actuator (:254-274): rows start .. start+n-1 (mod capacity_rows) of both traces
 * from s [n][ns], a [n][na] of `dtype`; a == NULL pushes zero actions (the POST_EPISODE dummy, :291-314).  One launch. */
int pdec_replay_push_sa(pdec_handle any_handle, void* state_trace, void* action_trace, int64_t capacity_rows, int ns, int na,
                        int64_t start, const void* s, const void* a, int64_t n, int dtype);
/* POST_ACT push of (r, terminal) (:276-289): r [n] of `dtype`; terminal of column i = done_flags[i / cols_per_traj] != 0
 * (the env step's per-trajectory flags), or 1 everywhere when force_terminal (time-out, src/PDEenv.jl:227).  One launch. */
int pdec_replay_push_rt(pdec_handle any_handle, void* reward_trace, void* terminal_trace, int64_t capacity_rows, int64_t start,
                        const void* r, const int32_t* done_flags, int cols_per_traj, int force_terminal, int64_t n, int dtype);
/* pde_sample + pde_fetch! (:317-340) for a batch of Bu transitions in one launch: indices from the Philox stream
 * (seed, offset) exactly as pdec_ddpg_update_small_rng draws them; outputs fp32 s, sn [Bu][ns], a [Bu][na], r, t [Bu];
 * slots_out (optional) int32 [3][Bu] = the slots used. */
int pdec_replay_sample(pdec_handle any_handle, const void* state_trace, const void* action_trace, const void* reward_trace,
                       const void* terminal_trace, int ns, int na, int64_t capacity, int stride, int64_t n_valid, int64_t n_rt,
                       uint64_t seed, uint64_t offset, int Bu, void* s_out, void* a_out, void* r_out, void* t_out,
                       void* sn_out, int32_t* slots_out);

/* Speculatively issued episodes (run.py: the control steps of a whole episode are enqueued without reading the environment's
 * `done` flag back after every step, src/PDEenv.jl:226-240 / RL.jl's `while !is_terminated(env)`).  `flag` is a device int32,
 * zero at the episode's start.  Attached to a handle, it makes the launches issued THROUGH that handle that change persistent
 * learner state no-ops once it is raised: pdec_replay_push_sa / pdec_replay_push_rt (the handle passed as any_handle) and
 * pdec_ddpg_update_small(_rng) (the behaviour critic's handle; the ADAM beta powers move on unchanged).  pdec_replay_push_rt
 * raises it after pushing a transition whose done_flags[0] != 0 (B = 1: the step that ends the episode is pushed, nothing
 * after it).  Everything else a later step writes goes to per-step buffers the host ignores.  NULL detaches. */
int pdec_set_episode_halt(pdec_handle any_handle, int32_t* flag);

/* Batched environments (B > 1; the reference has B = 1 and ends the episode at the first blow-up, src/PDEenv.jl:226-240):
 * same-step reset of every trajectory whose done flag is raised -- y, state and action rows are overwritten by their
 * initial images (reset!, :183-193), a non-finite reward becomes 0 -- so that a blown-up trajectory cannot feed inf/NaN
 * states into the learner for the rest of the lock-stepped episode.  state/state0, action/action0, reward may be NULL. */
int pdec_env_autoreset(pdec_handle env, const int32_t* done, void* y, const void* y0, void* state, const void* state0,
                       void* action, const void* action0, void* reward);
/* generate_random_init() of the 1-D setups (scripts/KS/setup/KSSetup.jl:288-298,
 * scripts/Keller-Segel/setup/KellerSegelSetup.jl:373-384) and of the 2-D Keller-Segel setup (the same sine sums along x and
 * along y, both species: n_coefficients = 2 (ceil(Lx / 3) + ceil(Ly / 3)), memory [ny][nx][2]) on the device, one workgroup
 * per trajectory: y0_out [B][...] in the environment's layout and dtype; uniforms from the Philox stream (seed, offset)
 * (Julia's global RNG cannot be reproduced, only the distribution; oracle/rng.py restates this stream).  Consumes
 * B * ceil(n_coefficients / 4) counters. */
int pdec_env_random_init(pdec_handle env, uint64_t seed, uint64_t offset, void* y0_out);
/* the same for the members of a population (the 1-D KS and Keller-Segel setups): trajectory b drawn from the stream
 * (seeds[b], offsets[b]) exactly as a B = 1 pdec_env_random_init(seeds[b], offsets[b]) draws it; seeds / offsets are DEVICE
 * arrays of B entries.  One launch. */
int pdec_env_random_init_members(pdec_handle env, const uint64_t* seeds, const uint64_t* offsets, void* y0_out);
/* Populations (population.py): every trajectory of the batch is an independent member.  on = 1: the KS step integrates one
 * trajectory per workgroup instead of two per complex FFT, so trajectory b's outputs are bit for bit those of a B = 1 step
 * on its inputs, whatever the other trajectories hold (the 1-D Keller-Segel step already runs one per workgroup). */
int pdec_env_set_member_layout(pdec_handle env, int on);
/* Robustness runs (scripts/KS/KS200_disturbed/KS200_disturbed.jl:16: an agent trained at mu = 0, evaluated at mu = 0.02): the
 * amplitude of the KS disturbance mu cos(2 + pi + x / (Lx / 2)) (KSSetup.jl:155) per trajectory instead of the creation-time
 * scalar cfg.mu.  mu_per_trajectory: a device array [B] of the environment's dtype, owned by the caller and read by every later
 * step or rollout launch on the environment's stream (the call itself stores the pointer and neither copies nor synchronises,
 * so launches recorded or captured afterwards follow later writes to the array); NULL returns to cfg.mu.  Trajectory b then steps
 * as an environment created with cfg.mu = mu[b] steps it: CNAB2 adds mu[b] h fft(cos(...)) -- the table at mu = 1, made at
 * creation, scaled per packed pair -- and the finite-difference steps add mu[b] cos(...) to the forcing, where an array of equal
 * values is bit for bit the scalar.  It belongs to the batch slot, not to the episode: pdec_env_autoreset leaves it alone.
 * Served for the KS environments with per-actuator agents (PDEC_PDE_KS_CNAB2 with every FFT engine, both step forms, the member
 * layout and the persistent rollouts; PDEC_PDE_KS_RK4_FD with both integrators).  Refused for the global/mono agent
 * (KSglobalSetup.jl:167 has no such term), for 1-D and 2-D Keller-Segel and for the fluid.  The acting-only closures
 * (pdec_actuate, pdec_featurize, pdec_reward) do not depend on it. */
int pdec_env_set_disturbance(pdec_handle env, const void* mu_per_trajectory);
/* Fault-tolerance runs: per-trajectory actuator and sensor faults of the KS environments, read by the kernels the way the
 * disturbance amplitude is.  Modifies the closures prepare_action and featurize (KSSetup.jl:190-245); reward_function and the
 * blow-up test stay what they are.  Three device arrays of the environment's dtype, owned by the caller; each may be NULL
 * (healthy), all NULL returns to the healthy environment.  The call stores the pointers and neither copies nor synchronises, so
 * launches recorded or captured afterwards follow later writes to the arrays.
 *   actuator_gain [B][A]: the forcing of trajectory b is synthesised from gain[b][a] * action[b][a] (0: dead, -1: reversed).
 *     The commanded action is unchanged everywhere else: the reward's action_punish / delta_action_punish terms, action_prev,
 *     the rollouts' action logs.  p_out and the p logs hold the forcing actually applied.
 *   sensor_gain, sensor_bias [B][S]: featurize writes (gain[b][s] * dot_s + bias[b][s]) * sensor_scale for sensor s -- indexed
 *     by the sensor, so a window row that reads a neighbouring sensor takes that sensor's fault; the bias is in units of the
 *     field.  Rows copied from the previous state (temporal_steps > 1) keep their values.  The reward reads the true dots.
 * The arrays belong to the batch slot, not to the episode: resets and the episode clock leave them alone, and the clock
 * re-featurizes a restarted trajectory through its own sensor faults.  Ones and zeros give, bit for bit, the healthy run (on
 * fields that are not identically zero: -0 * 1 + 0 is +0).
 * Served for PDEC_PDE_KS_CNAB2 (fused step in both forms, member layout, persistent rollouts, with or without a disturbance
 * array) and PDEC_PDE_KS_RK4_FD (both integrators), pdec_actuate and pdec_featurize, with per-actuator agents and
 * memory_size = 0.  Refused for the global/mono agent, memory_size > 0, 1-D and 2-D Keller-Segel and the fluid.  The fault-carrying
 * step has no synchronised form: pdec_env_step with a launch sync pending (pdec_set_launch_sync) and arrays set is refused by name;
 * a caller that hands over between streams by device flags uses events for such an environment (run.py does). */
int pdec_env_set_faults(pdec_handle env, const void* actuator_gain, const void* sensor_gain, const void* sensor_bias);
/* Delayed control (src/plotting.jl:55-60, plot_heat(p_t_action = ...): uncontrolled until t = p_t_action, then the actor
 * engages), a sticky setting read by pdec_rollout and pdec_rollout_members in all their forms; n0 = 0 (the default) is off.
 * For the steps t < n0 the action is exactly zero -- no actor evaluation, no exploration noise -- and reward_sum adds only the
 * steps t >= n0 (the uncontrolled prefix is the same whatever the actor).  The noise numbering per step is unchanged, so the
 * steps t >= n0 draw what they draw with n0 = 0; the log rows, done_any and done_step cover all T steps. */
int pdec_env_set_control_from(pdec_handle env, int n0);

/* ---------------------------------------------------------------- populations of single-trajectory learners
 * M independent reference-shaped DDPG learners (B = 1, small-batch update with device-side sampling, glue launch) whose
 * per-step launches are ONE launch of M workgroups each.  Member m: its four networks (fp32, one stream shared by all
 * members), traces[4m .. 4m+3] = its replay's state / action / reward / terminal traces (capacity + stride rows for s / a,
 * capacity for r / t), seeds[2m], seeds[2m+1] = its noise / sample seeds, losses[m] = its fp32 loss pair.  rows = a DEVICE
 * int64 [M][16] table of per-member counters in the order update_step, n_sa, n_rt, noise offset, sample offset, halt flag,
 * active, actor / critic beta-power slot, act_noise, act_limit (the last two as bit patterns of doubles); the caller writes
 * it before an episode, the launches below advance it as the solo run's host counters advance, and the caller reads it back
 * after the episode.  The members' slices of the per-step buffers lie cols * width * dtype-size bytes apart. */
int pdec_population_create(pdec_handle* out, int M, const pdec_handle* actors, const pdec_handle* critics,
                           const pdec_handle* target_actors, const pdec_handle* target_critics, void* const* traces,
                           const uint64_t* seeds, void* const* losses, int env_dtype, int cols, int64_t capacity, int stride,
                           int loops, int Bu, double gamma, double rho, int quirk, double eta_actor, double eta_critic,
                           int64_t update_after_rows, int64_t update_freq, int64_t start_steps, int64_t* rows);
/* phase 0: pdec_step_glue of one control step for every member (reward / done_flags of the previous step or both NULL,
 * state [M][cols][ns], actions_out [M][cols][na]); phase 1: the time-out push of the last step's rewards; phase 2: the
 * POST_EPISODE push of the final state with a zero action for the active members.  One launch of M workgroups. */
int pdec_population_glue(pdec_handle pop, int phase, const void* reward, const int32_t* done_flags, const void* state,
                         void* actions_out);
/* pdec_ddpg_update_small_rng for every member whose own trigger fires (min(n_rt, capacity) > update_after_rows,
 * update_step % update_freq == 0, not halted); one launch of M workgroups */
int pdec_population_update(pdec_handle pop);
/* set = 0: write each member's beta-power slots into rows_host[m][7], [m][8]; set = 1: adopt them from there */
int pdec_population_bp_sel(pdec_handle pop, int64_t* rows_host, int set);
/* the members' hooks' actor snapshots (best[m], current[m]: fp32 networks of the actor's shape on the networks' stream, 0 =
 * none); pdec_population_copy_actors then copies member m's behaviour actor parameters into best[m] where bit 0 of which[m]
 * is set and into current[m] where bit 1 is (which: DEVICE int32 [M]), for all members in one launch */
int pdec_population_set_actor_copies(pdec_handle pop, const pdec_handle* best, const pdec_handle* current);
int pdec_population_copy_actors(pdec_handle pop, const int32_t* which);
/* Per-member hyper-parameters.  on = 1: the update launch takes member m's gamma, Polyak rho and actor / critic ADAM step
 * sizes from rows[m][11], [12], [13], [14] (bit patterns of doubles: the values a solo pdec_ddpg_update_small_rng call of that
 * member would be given, converted as that call converts them) instead of pdec_population_create's; the caller writes them
 * with the rest of the row.  Off (the default) the slots are not read and the launch-wide values hold.  The kernel is
 * selected from pdec_population_create's rho for the whole launch: either every member's rho is 1 (frozen targets) or none's
 * is.  act_noise and act_limit (slots 9, 10) are per member either way.  Slot 15 is free.  Refused (on = 1) for networks
 * whose update takes a bounded instantiation of the register kernel (pdec_debug_small_update_kernel reports a name that ends
 * in ",0>"): those have no register left for a member's own values. */
int pdec_population_set_member_hyper(pdec_handle pop, int on);
/* Member d takes over the learner of member src[d] (src: HOST int32 [M]; src[d] == d: d stays as it is), all pairs in ONE
 * launch on the population's stream: parameters and ADAM moments of the behaviour actor and critic, the parameters of the two
 * target networks, the source's current beta powers (into the destination's current slot), the loss pair and the first
 * rows_sa[d] rows of the state / action traces and rows_rt[d] rows of the reward / terminal traces (HOST int64 [M]; 0: the
 * destination keeps its replay; rows past the prefix are not touched).  Counters, seeds and offsets are the caller's.  Refuses
 * a source out of range and a member that is both a source and a destination. */
int pdec_population_clone(pdec_handle pop, const int32_t* src, const int64_t* rows_sa, const int64_t* rows_rt);
/* The episode boundary of every member on the device, so that several episodes can be enqueued per read-back.  `book`: DEVICE
 * int64 [M][16], the caller's, beside the rows -- per member (doubles as bit patterns) 0 hook.ep, 1 min_best_episode,
 * 2 collect_NNA, 3 / 4 whether rewards_compare is non-empty and its maximum as Python's max() leaves it (the first element
 * unless a later one compared greater: a leading NaN stays), 5 bestreward, 6 bestepisode, 7 stop kind (0 StopAfterEpisode,
 * 1 StopAfterEpisodeWithMinSteps), 8 its cur, 9 its episode / step, 10 use_random_init, 11 init seed, 12 init offset of the
 * next field, 13 counters one field consumes, 14 scratch (the stop fired), 15 free.
 * phase 0 (behind pdec_population_glue phase 1; one workgroup per member): for members whose row has ACTIVE set, n = the
 * executed steps from flags [T][M] (up to and with the first flagged step; a flag at step T - 1 is the time-out), episode
 * reward = 0.0 + the sequential fp64 sum of means[m][0 .. n) (src/PDEhook.jl:52, :92), env_y[m] / env_state[m] = slot n of
 * log_y / log_state ([T + 1][M][y_elems / state_elems] doubles), then src/PDEhook.jl:65-97 on the book -- eligible:
 * n == T and ep >= min_best_episode; new best: collect_NNA and reward >= maximum, false for NaN --, which[m] = new best |
 * collect_NNA << 1 for pdec_population_copy_actors, src/StopCondition.jl:6-40 called once per executed step with
 * is_terminated true at the last, and elog[m] = {reward, n, new best, 1} (DEVICE int64 [M][4]).  Idle members: elog[m] = 0,
 * which[m] = 0, nothing else.
 * phase 1 (behind pdec_population_glue phase 2, which still reads the episode's n_sa and ACTIVE; only book, reset_post and last
 * are read): the counters of the active members move as src/PDEagent.jl:215-224, :291-314 and :237-252 move them --
 * n_sa += cols, update_step = 0 with reset_post, the init offset past the consumed field; where the stop fired ACTIVE = 0 and
 * HALT = 1, else HALT = 0 and, unless `last` (the block's last episode: the host's PRE_EPISODE follows), n_sa -= stride if
 * n_sa > n_rt. */
int pdec_population_episode_close(pdec_handle pop, int phase, int64_t* book, int64_t* elog, const int32_t* flags,
                                  const double* means, int T, const void* log_y, const void* log_state, void* env_y,
                                  void* env_state, int64_t y_elems, int64_t state_elems, int32_t* which, int reset_post, int last);
/* Where bit 0 of which[m] is set: the rows src/PDEhook.jl:54-62 logs for the n = elog[m][1] steps of this episode -- action
 * slots 1..n, p slots 0..n-1, y slots 1..n, reward slots 0..n-1 of the episode's logs ([slots][M][elems] doubles) -- into the
 * member's best rows best_* [M][T][elems] (src/PDEhook.jl:72-74).  One launch, grid (chunks, M). */
int pdec_population_copy_best_rows(pdec_handle pop, const int32_t* which, const int64_t* elog, int T, const void* log_action,
                                   const void* log_p, const void* log_y, const void* log_reward, void* best_action, void* best_p,
                                   void* best_y, void* best_reward, int64_t action_elems, int64_t p_elems, int64_t y_elems,
                                   int64_t reward_elems);

/* ---------------------------------------------------------------- episode ledger (PDEhook's bookkeeping, src/PDEhook.jl:51-97) */
/* The episode returns, blow-up bits and best actor of a batched training run, kept on the device: no launch argument depends
 * on anything but the caller's ring buffers, so pdec_ledger_step can be part of a recorded step or a captured graph.  All
 * launches go to the environment's stream.  `actor` (0: none) is the behaviour actor whose parameters the best-episode
 * snapshot keeps; `capacity` rows of logged episodes are kept (row = episode mod capacity). */
int pdec_ledger_create(pdec_handle* ledger, pdec_handle env, pdec_handle actor, int capacity);
/* behind the env step: ret_b += (sum_a (double) reward[b][a]) / R (sum in a order), blew_b |= flags[b] != 0.  reward [B][R] in
 * the environment's dtype, flags [B] (the env step's outputs) */
int pdec_ledger_step(pdec_handle ledger, const void* reward, const int32_t* flags);
/* behind the acting kernel of an episode's last step, before anything may rewrite what it read: copies the parameters that
 * kernel read (the published image of a fused 3-layer actor, unpacked; the flat parameters otherwise) to the staging buffer */
int pdec_ledger_snapshot(pdec_handle ledger);
/* at the episode's last step (0-based `episode`): row episode mod capacity <- returns [B] (fp64), blow-up bits [B] and the
 * batch mean (sum_b ret_b) / B in b order.  track_best: an episode with episode + 1 >= min_best_episode whose mean is >= every
 * earlier such mean becomes the best (its snapshot is kept); a NaN mean is never chosen and does not take part in later
 * comparisons.  The running sums restart from 0.  Nothing is read back. */
int pdec_ledger_close(pdec_handle ledger, int64_t episode, int64_t min_best_episode, int track_best);
/* the running sums restart from 0 without a row (an episode cut short) */
int pdec_ledger_discard(pdec_handle ledger);
/* host accessors (synchronise the environment's stream): all rows [capacity][B] / [capacity] (any pointer may be NULL), the
 * best value (-1e6 before any choice) and 1-based episode number (0: none), the best parameters into an MLP of the actor's
 * layer sizes (PDEC_E_INVALID otherwise; converted when its dtype differs) */
int pdec_ledger_read(pdec_handle ledger, double* returns, int32_t* blew_up, double* means);
int pdec_ledger_best(pdec_handle ledger, double* value, int64_t* episode);
int pdec_ledger_best_params(pdec_handle ledger, pdec_handle mlp);

/* Greedy held-out evaluation of the training actor, scored on the device (replaces the noise-free env.rollout on a fixed set of
 * fields that tools/pipeline_learning_probe.py ran after a training run, and PDEhook's choice of bestNNA by the noisy training
 * return, src/PDEhook.jl:65-76, by one made on the evaluation score).  The numbers, per evaluated trajectory b of the K the
 * evaluation environment holds, from a rollout's reward_sum [K][R] (environment's dtype) and done_step [K]:
 *   ret_b  = (sum_a (double) reward_sum[b][a]) / R, summed in a order;   blew_b = done_step[b] >= 0
 *   score  = (sum_b ret_b) / K, summed in b order; NaN when any blew_b is set or any ret_b is not finite
 * (population.py: score_members' rule, so a population's evaluate() and the pipeline rank alike).
 * pdec_ledger_eval_attach: ties an evaluation environment (B = K, any stream), an evaluation actor of the ledger's actor's layer
 * sizes (any dtype the staged parameters promote to exactly: the actor's own, or PDEC_F64) and `capacity` rows to a ledger made
 * with an actor; allocates rows [capacity][K] fp64 / int32, [capacity] scores and episode numbers, the evaluation state and the
 * best-by-evaluation parameter buffer.  Once per ledger. */
int pdec_ledger_eval_attach(pdec_handle ledger, pdec_handle eval_env, pdec_handle eval_actor, int capacity);
/* on the TRAINING environment's stream, behind pdec_ledger_snapshot of the same step: the staged parameters -> the evaluation
 * actor's flat parameters (Float32 -> fp64 is an exact promotion), one device kernel, no host copy, no synchronisation; the
 * images the acting kernels derive from them are rebuilt by the evaluation actor's next acting call on its own stream.  The
 * caller orders the streams: this call behind the previous evaluation's close, the evaluation's rollout behind this call. */
int pdec_ledger_eval_load(pdec_handle ledger);
/* on the EVALUATION environment's stream, behind the rollout that filled reward_sum / done_step (device): one workgroup writes
 * row `n_eval mod capacity` (returns, bits, score, 1-based `episode`) as defined above and applies PDEhook's rule to the score --
 * an evaluation with episode >= min_best_episode whose score is not NaN and >= every earlier such score becomes the best; its
 * parameters are copied from the EVALUATION ACTOR (the staging buffer may already hold a later snapshot).  Nothing is read back. */
int pdec_ledger_eval_close(pdec_handle ledger, const void* reward_sum, const int32_t* done_step, int64_t n_eval, int64_t episode,
                           int64_t min_best_episode);
/* host accessors (synchronise the evaluation environment's stream): all rows (any pointer may be NULL) -- episodes [capacity],
 * returns / blew_up [capacity][K], scores [capacity] --, the best score (-1e6 before any choice) and its 1-based episode (0:
 * none), the best parameters into an MLP of the actor's layer sizes (converted when its dtype differs) */
int pdec_ledger_eval_read(pdec_handle ledger, int64_t* episodes, double* returns, int32_t* blew_up, double* scores);
int pdec_ledger_eval_best(pdec_handle ledger, double* value, int64_t* episode);
int pdec_ledger_eval_best_params(pdec_handle ledger, pdec_handle mlp);

/* ---------------------------------------------------------------- episode clock (per-trajectory episodes on the device) */
/* A clock per trajectory of a batched 1-D environment (KS, finite-difference KS, Keller-Segel; per-actuator agents,
 * memory_size = 0): pdec_epclock_step behind env step k decides per trajectory whether its episode ends IN this step -- its
 * blow-up flag is raised, or its clock reaches episode_steps -- and restarts it there.  Per trajectory b, in this order:
 *   1. blew = flags[b] != 0; where blew, non-finite entries of reward row b become 0; other rows are not touched
 *   2. ret[b] += (sum_a (double) reward[b][a]) / R, summed in a order (pdec_ledger_step's arithmetic, on the sanitised row)
 *   3. clock[b]++, len[b]++, total[b]++; ends = blew || clock[b] == episode_steps
 *   4. not ended: action_prev_next[b][:] = action[b][:]; nothing else of b is written
 *   5. ended: terminal row b = 1; log slot count[b] % capacity <- (ret[b], len[b], blew, total[b]); count[b]++; ret[b] = 0;
 *      clock[b] = len[b] = 0; action_prev_next[b][:] = 0; y_next[b] <- the new field; state_next[b] <- its pdec_featurize row
 *      in reset form (no previous state)
 * The new field: row b of (y0, state0), or with random_init row b of what pdec_env_random_init(env, seed, off) draws at
 * off = (n world + rank) B ceil(nc / 4), n = count[b] after the increment, nc the sine coefficients per trajectory -- bit for
 * bit that call's row, and the state row bit for bit pdec_featurize's.  All counters live on the device and every argument
 * besides the arrays is fixed at creation, so the call can be part of a recorded step or a captured graph; one or two
 * launches on the environment's stream, one workgroup per trajectory, each writing its own trajectory's rows only.
 * Arrays in the environment's dtype: reward / terminal [B][A], action / action_prev_next [B][A][1], y_next [B][...], state_next
 * [B][A][ns]; flags [B] as the env step leaves them; y0 / state0 may be NULL with random_init.  Released with pdec_destroy. */
int pdec_epclock_create(pdec_handle* clock, pdec_handle env, int episode_steps, int capacity, int random_init, uint64_t seed,
                        int rank, int world);
/* clock[b] = clock0[b] (host array [B], values 0 .. episode_steps - 1; NULL: zeros), len = 0, ret = 0: the running episodes
 * are cut without a log entry; count, total and the logs stay.  Synchronises the environment's stream. */
int pdec_epclock_set(pdec_handle clock, const int32_t* clock0);
int pdec_epclock_step(pdec_handle clock, void* reward, const int32_t* flags, void* terminal, const void* action,
                      void* action_prev_next, void* y_next, void* state_next, const void* y0, const void* state0);
/* host accessor (synchronises the environment's stream; any pointer may be NULL): counts [B] episodes finished, and the log
 * rings [B][capacity] -- episode e of trajectory b sits in slot e mod capacity: its return, its length in steps, its blow-up
 * bit and the 1-based number of the pdec_epclock_step call that ended it */
int pdec_epclock_read(pdec_handle clock, int64_t* counts, double* returns, int32_t* lengths, int32_t* blew_up, int64_t* end_steps);

/* ---------------------------------------------------------------- n-step transitions, assembled on the device */
/* An object that keeps the last n_step rows of a batched control loop -- state [cols][ns], action [cols][na], reward [cols],
 * terminal [cols] in `dtype` (PDEC_F32 / PDEC_F64) -- on its own stream (pdec_set_stream).  1 <= n_step <= 32.  It knows no
 * environment: it reads the rows it is handed.  Released with pdec_destroy. */
int pdec_nstep_create(pdec_handle* nstep, int n_step, int cols, int ns, int na, int dtype);
/* Call number k (0-based) stores the row (s_in, action, reward, terminal) of step k and emits, per column c, the transition
 * that STARTS at step u = k - n + 1 (n = n_step):
 *   m             = the smallest i in [0, n-1] with terminal_{u+i}[c] != 0, or n - 1 if there is none
 *   reward_out[c] = sum_{i=0..m} w_i reward_{u+i}[c],  w_0 = 1, w_{i+1} = w_i gamma: in double, summed in index order without
 *                   FMA contraction, rounded once to dtype
 *   terminal_out[c] = 1 if terminal_{u+m}[c] != 0 else 0
 *   state_out[c]  = s_in_u[c],  action_out[c] = action_u[c]
 * The next state of that transition is the caller's own: the state that followed step k.  A window cut short by a terminal has
 * terminal_out = 1, so its bootstrap term gamma (1 - terminal) q' vanishes whatever the discount; every window that bootstraps
 * is full, and the update of the emitted batch takes the scalar w_n (the same repeated product) in the place of gamma for every
 * column.  Every call emits cols transitions, each transition start exactly once; the first n - 1 calls emit windows that reach
 * back before call 0 (rows of zeros) and are the caller's to ignore.  A non-finite reward reaches exactly the windows that hold
 * it at an index <= m.
 * One launch on the object's stream, one thread per element, every access coalesced along the columns; the ring position is a
 * device counter (read by pdec_nstep_read), so the arguments do not depend on k and the call can be part of a recorded step or a
 * captured graph.  No output may alias an input. */
int pdec_nstep_step(pdec_handle nstep, const void* s_in, const void* action, const void* reward, const void* terminal, double gamma,
                    void* state_out, void* action_out, void* reward_out, void* terminal_out);
/* host accessor (synchronises the object's stream; any pointer may be NULL): position = calls so far -- call k wrote ring slot
 * k mod n_step --, and the rings states [n_step][cols][ns], actions [n_step][cols][na], rewards / terminals [n_step][cols] */
int pdec_nstep_read(pdec_handle nstep, int64_t* position, void* states, void* actions, void* rewards, void* terminals);

/* ---------------------------------------------------------------- per-step training telemetry, kept on the device */
/* An object with two rings of `capacity` rows of doubles -- one row per control step, one per update -- and a sticky pair
 * (first_nonfinite_step, first_nonfinite_update).  It is made for rows of B trajectories and cols >= B columns -- state
 * [cols][ns], action [cols][na], reward / terminal [cols] in env_dtype, flags [B] -- and for an actor and a critic (mlp handles of
 * one dtype) whose flat parameter counts it keeps a copy of.  Nothing is read back until pdec_telemetry_read.  Every value is
 * promoted to double (exact); squares and sums are formed in double without FMA contraction; an entry that is not finite is left
 * out of sums and maxima and counted; partial sums are combined in an order that depends on the shapes only (no floating-point
 * atomics), so two runs of one program give bit-equal rows.  The row counters live on the device and no argument depends on the
 * call number, so both calls can be part of a recorded step or a captured graph.  Released with pdec_destroy. */
int pdec_telemetry_create(pdec_handle* telemetry, int capacity, int B, int cols, int ns, int na, int env_dtype, pdec_handle actor,
                          pdec_handle critic);
/* One launch on the object's stream (pdec_set_stream) writes step row n mod capacity, n the number of earlier step calls:
 *   step | reward_mean reward_min reward_max (over the finite rewards; NaN when there is none) reward_nonfinite |
 *   action_mean action_abs_mean (row 0 of every action column) action_saturated (columns with |a[c][0]| >= act_limit) |
 *   state_abs_max (over the finite entries, 0 when there is none) state_nonfinite | blown_up (flags[b] != 0) |
 *   terminal (terminal[c] != 0)                                                          -- 12 columns, counts as doubles.
 * first_nonfinite_step <- n when it is still -1 and reward_nonfinite + state_nonfinite > 0. */
int pdec_telemetry_step(pdec_handle telemetry, const void* s_out, const void* action, const void* reward, const void* terminal,
                        const int32_t* flags, double act_limit);
/* One launch on the stream of `critic` writes update row n mod capacity, n the number of earlier update calls, from the flat
 * parameters of the four networks (sizes and dtype as at creation) and losses = [critic, actor] in the networks' dtype:
 *   update | critic_loss actor_loss | actor_norm2 critic_norm2 (sum theta^2) | actor_target_dist2 critic_target_dist2
 *   (sum (theta - theta_target)^2) | actor_step2 critic_step2 (sum (theta - theta_prev)^2) | actor_abs_max critic_abs_max |
 *   actor_nonfinite critic_nonfinite                                                     -- 13 columns.
 * theta_prev is the object's copy of the parameters at the previous call, rewritten by this launch; step2 = 0 for the first call
 * after creation or reset.  A difference is left out when either entry is not finite.  first_nonfinite_update <- n when it is
 * still -1 and a loss or a parameter is not finite. */
int pdec_telemetry_update(pdec_handle telemetry, pdec_handle actor, pdec_handle critic, pdec_handle actor_target,
                          pdec_handle critic_target, const void* losses);
/* host accessor (synchronises both streams; any pointer may be NULL): the rings [capacity][12] and [capacity][13] -- call n sits
 * in row n mod capacity --, the numbers of calls so far, and sentinel[2] = (first_nonfinite_step, first_nonfinite_update) */
int pdec_telemetry_read(pdec_handle telemetry, double* step_rows, int64_t* n_step_calls, double* update_rows, int64_t* n_update_calls,
                        int64_t* sentinel);
/* rings, counters, the sentinel and theta_prev back to their state at creation.  Synchronises both streams. */
int pdec_telemetry_reset(pdec_handle telemetry);

/* ---------------------------------------------------------------- HIP graphs -- */
/* Record everything enqueued on the stream of `origin` (pdec_set_stream; not the null stream) -- library calls, and any
 * other stream that forks from it and joins it again through events -- between _begin and _end into one HIP graph;
 * pdec_graph_launch replays it with one host call.  Calls that keep their per-step state on the device
 * (pdec_policy_act_rng_dev, every ADAM step) replay correctly: the slot selectors of their double-buffered device
 * state, which the captured calls flipped on the host, are flipped again by every pdec_graph_launch after the first
 * (capturing records the work without running it, so the first launch is the execution the capture stands for).
 * A graph must be replayed at a step whose buffers are those of the captured one (same ring phase).
 * Precondition for environments that step their batch in parts (fluid, 2-D Keller-Segel): their part streams exist -- one
 * eager step or pdec_env_set_part_streams before the capture (see pdec_env_part_streams).
 * The graph handle is released with pdec_destroy. */
int pdec_capture_begin(pdec_handle origin);
int pdec_capture_end(pdec_handle origin, pdec_handle* graph);
int pdec_graph_launch(pdec_handle graph, void* hip_stream);      /* NULL = the stream it was captured on */
int pdec_graph_num_nodes(pdec_handle graph, int* n);
/* One-shot: the next slab-reduction / ADAM launch issued on `mlp` (the second kernel of pdec_ddpg_update_critic_async /
 * pdec_ddpg_update_actor_async on the fused 3-layer path) carries `event` as the completion event of its own dispatch
 * packet: what pdec_event_record(event, stream) right behind that call would give, without the record's own packet in the
 * stream (each costs the update chain ~4.5 us).  PDEC_E_INVALID for networks outside that path. */
int pdec_mlp_set_stop_event(pdec_handle mlp, pdec_handle event);
/* The same for the next reduce-ONLY launch on `mlp` (the second kernel of pdec_ddpg_actor_grads / pdec_ddpg_critic_grads on the
 * fused 3-layer path: the flat gradient buffer is complete when it ends) -- the event an all-reduce issued on ANOTHER stream
 * waits for, so that the collective leaves the update chain (pipeline.py).  A launch that applies the update never consumes
 * it, a reduce-only launch never consumes the stop event, and pdec_ddpg_actor_grads / _critic_grads record it behind their
 * last launch when the path they took has no such launch (so a waiter never sees a stale event). */
int pdec_mlp_set_reduce_event(pdec_handle mlp, pdec_handle event);
/* records a still pending stop event on the net's stream (the update took a path that does not consume it); else no-op */
int pdec_mlp_flush_stop_event(pdec_handle mlp);
/* Device-scope events for the hand-offs between two streams of one device (no system-scope cache fence, unlike a
 * default HIP event): record on one stream, make another stream wait.  Released with pdec_destroy. */
int pdec_event_create(pdec_handle* ev);
int pdec_event_record(pdec_handle ev, void* hip_stream);
int pdec_stream_wait_event(void* hip_stream, pdec_handle ev);

/* A device-side hand-over between two single-workgroup launches on DIFFERENT streams, for the NEXT launch through `handle`
 * that supports it -- pdec_step_glue (the actor's handle) and the fused fp64 KS step of one trajectory with 192 / 240 / 600 cells
 * in pdec_env_step (the environment's handle), the two launches that alternate on the chain of the reference-shaped training loop
 * (src/PDEenv.jl:195-241 and src/PDEagent.jl:175-289 in RL.jl's run order): the launch waits inside the kernel until
 * *wait_flag >= wait_value before it reads anything (NULL: no wait; the wait gives up after 0.3 s and counts a timeout) and
 * stores done_value to *done_flag behind its last store (NULL: no signal).  Flags: device int64, zeroed by the caller, values
 * increasing.  One-shot: cleared by the launch.  PDEC_E_INVALID from a launch that cannot honour a pending one. */
int pdec_set_launch_sync(pdec_handle handle, const int64_t* wait_flag, int64_t wait_value, int64_t* done_flag, int64_t done_value);
/* Do launches on the two streams run side by side?  HIP maps streams onto a few hardware queues; two streams that share one run
 * in issue order, and a pdec_set_launch_sync wait for a launch queued behind the waiter on the same hardware queue would wait for
 * nothing.  A caller checks its pair of streams with this once (a 20-ms bounded probe; synchronises both) before it uses
 * pdec_set_launch_sync across them.  *yes = 1: side by side. */
int pdec_streams_run_side_by_side(void* stream_a, void* stream_b, int* yes);
/* waits that gave up since the library was loaded (synchronous read) */
int pdec_launch_sync_timeouts(int* n);

/* ---------------------------------------------------------------- multi-GPU ---------- */
/* One RCCL communicator per process (one process per GPU).  unique_id: 128 bytes from
 * pdec_comm_unique_id on rank 0, broadcast by the host (the reference has no collective;
 * this is the build's data-parallel addition). */
int pdec_comm_unique_id(void* id128);
int pdec_comm_create(pdec_handle* c, int nranks, int rank, const void* id128);
/* the same with a bounded wait: RCCL's rendezvous blocks until every rank has arrived, so one missing rank would park the
 * others for ever; past timeout_ms (> 0) this returns PDEC_E_COMM instead and the caller can agree on another path
 * (bench.py: torch.distributed).  timeout_ms <= 0 = pdec_comm_create. */
int pdec_comm_create_timeout(pdec_handle* c, int nranks, int rank, const void* id128, int timeout_ms);
/* sum-all-reduce the internal gradient buffer of an MLP in place (fp32/fp64), on the network's stream ... */
int pdec_allreduce_grads(pdec_handle comm, pdec_handle mlp);
/* ... or on `hip_stream` (NULL = the network's): the caller orders it against the launch that leaves the gradient
 * (pdec_mlp_set_reduce_event) and the one that consumes it (pdec_stream_wait_event before pdec_adam_polyak_step) */
int pdec_allreduce_grads_on(pdec_handle comm, pdec_handle mlp, void* hip_stream);
int pdec_allreduce(pdec_handle comm, void* dptr, size_t n, int dtype, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* PDECONV_H */
