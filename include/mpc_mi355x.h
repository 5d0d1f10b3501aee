/*
 * mpc_mi355x.h - C ABI of the MI355X (gfx950) batched nonlinear-MPC solve engine.
 *
 * Drop-in boundary for the hot path of SaeedRahmani/MPC-RL_for_AVs:
 *   PureMPC_Agent._solve()   reference agents/pure_mpc.py:80-318   (one NLP per call, CasADi -> IPOPT)
 *   PureMPC_Agent.predict()  reference agents/pure_mpc.py:68-78
 * The reference has no FFI for this path (it is a plain Python method that builds a CasADi graph and
 * calls `ca.nlpsol('solver','ipopt',...)`, agents/pure_mpc.py:285-300); the entry points below are what a
 * binding for it binds instead: plain pointers and sizes, no Python or torch types.  INTEGRATION.md shows
 * the ctypes stub that replaces the body of `_solve`.
 *
 * Conventions
 *   - all floating-point data is IEEE double; indices are int32; flags uint8 / uint32
 *   - arrays are dense row-major with the batch index slowest: state[B][4], vref[B][N+1], ...
 *   - every call returns 0 on success or a negative MPC_ERR_* code; mpc_last_error() gives the text
 *   - no exceptions cross this boundary; per-instance solver outcomes go to status[] / iters[]
 *   - a handle belongs to one (process, device); calls on one handle must not overlap, and neither may the work they
 *     enqueue (MPC_FLAG_NO_SYNC) on different streams - the handle owns scratch such as the batch's launch order and the
 *     per-environment records - with one exception: mpc_solve_batch with MPC_FLAG_THROUGHPUT, made for batches in flight
 */
#ifndef MPC_MI355X_H
#define MPC_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_ABI_VERSION 8
#define MPC_MAX_HORIZON 64
#define MPC_MAX_OTHERS 16

/* error codes (return values) */
#define MPC_OK 0
#define MPC_ERR_INVALID_ARG (-1)
#define MPC_ERR_NO_DEVICE (-2)   /* no HIP device / HIP runtime error: the engine has no CPU fallback */
#define MPC_ERR_HIP (-3)
#define MPC_ERR_NO_REFERENCE (-4) /* mpc_set_reference() has not been called */

/* mpc_solve_batch flags */
#define MPC_FLAG_COLLISION_COST 1u /* add the distance/collision terms of agents/archive/pure_mpc.py:189-206 */
#define MPC_FLAG_DEVICE_PTRS 2u    /* all data pointers are device memory (else host memory, copied internally) */
#define MPC_FLAG_NO_SYNC 4u        /* with DEVICE_PTRS: enqueue only, do not synchronise the stream */
#define MPC_FLAG_WARM_START 8u     /* NOT in the reference (which cold-starts every solve, agents/pure_mpc.py:240-246):
                                      start from given controls instead of zeros.  They are clamped 0.1 % inside their
                                      bounds; if their rollout leaves the state bounds the cold start is used.  Changes
                                      the iterates (fewer of them), not the KKT point aimed at.
                                      mpc_solve_batch: U (required) holds the initial controls on entry;
                                      mpc_predict_batch: each environment starts from its previous solution advanced by
                                      one stage (kept in the handle, forgotten by the reset calls);
                                      mpc_reset_env_mask: forget only that memory, keep the detector state */

/* mpc_predict_batch only: the reference's call sequence _parse_obs -> _check_collision -> _solve as separate calls
 * (agents/pure_mpc.py:68-78).  Without either flag one call does all of it. */
#define MPC_FLAG_DETECT_ONLY 16u   /* _check_collision alone (agents/pure_mpc.py:552-676): advance the detector records of
                                      the B environments for this observation, solve nothing (weights, act may be NULL);
                                      mpc_get_env_state then serves is_collide, conflict_index, ... */
#define MPC_FLAG_DETECTED 32u      /* _solve after such a call for the SAME observation: the records are not advanced
                                      again; ego index, speed profile (agents/pure_mpc.py:678-724) and the solve only */

#define MPC_FLAG_THROUGHPUT 64u     /* the caller keeps several batches in flight on different streams: launch the build of the
                                      solve kernel for four resident waves per SIMD whatever the batch size.  By default the
                                      engine picks the build by how deep ONE batch fills the SIMDs (B <= 4 waves per SIMD, 4096
                                      on an MI355X: the latency build, 218 registers, two resident waves; else the 128-register
                                      one), which is the faster choice when batches run one at a time and the slower one when
                                      six of them share the GPU. */

#define MPC_FLAG_STRICT_DISCONTINUITY 128u /* reference-strict reading of the d = 1 discontinuity of the collision cost
                                      (agents/archive/pure_mpc.py:189-196): an instance that ends on it - MPC_STATUS_CONVERGED_ON_KINK
                                      or MPC_STATUS_ACCEPTABLE_ON_KINK - is reported as MPC_STATUS_KINK_UNSOLVED, i.e. NOT solved,
                                      with the last iterate as the result: what the reference's IPOPT reports for a point no
                                      smooth method accepts (solver.stats()['success'] false, the last iterate is used,
                                      agents/pure_mpc.py:303-305).  The iterates OF THAT SOLVE are the same with and without the flag; with
                                      MPC_FLAG_WARM_START the next closed-loop step differs (a solve reported unsolved does not seed it). */

/* per-instance solver status written to status[] */
#define MPC_STATUS_CONVERGED 0
#define MPC_STATUS_MAX_ITER 1       /* last iterate returned, like the reference (agents/pure_mpc.py:303-305) */
#define MPC_STATUS_FACTORIZATION 2
#define MPC_STATUS_INFEASIBLE_START 3 /* the initial state violates the state bounds of agents/pure_mpc.py:272-274 */
#define MPC_STATUS_STALLED 4          /* no acceptable step in 3 consecutive iterations, or (mpc_config.stall_window) no
                                         halving of the KKT error within the window; last iterate returned */
#define MPC_STATUS_CONVERGED_ON_KINK 5 /* converged, with the collision cost on, to a point that holds a vehicle exactly at
                                         the d = 1 m discontinuity of that cost (agents/archive/pure_mpc.py:189-196:
                                         100/d^2 outside, 1000/d^2 inside): a KKT point of the outer branch with
                                         |p - o|^2 >= 1 as a constraint, i.e. a local minimiser of the discontinuous
                                         objective.  IPOPT has no such notion.  Observed with the restatement of its
                                         algorithm at the reference's settings on the 148 such instances of BASELINE
                                         config 3 (profiles/r03_parity_vs_ipopt.txt, part b): 99 end without success
                                         (70 with steps below alpha_min, where IPOPT proper would try its restoration
                                         phase; 29 at max_iter 1000, half of them within 1e-3 of d = 1) and the reference
                                         would act on that last iterate (agents/pure_mpc.py:303-305); 49 converge to a
                                         smooth minimiser on one side of the jump (26 inside d < 1, 23 outside), a
                                         different action than this status returns in 35 of them. */

#define MPC_STATUS_ACCEPTABLE 6        /* IPOPT's "Solved To Acceptable Level" with IPOPT's defaults, which are live in the
                                         reference (it sets only max_iter, tol and print options, agents/pure_mpc.py:291-296):
                                         the scaled KKT error was at most acceptable_tol = 1e-6 in acceptable_iter = 15
                                         consecutive iterations while mpc_config.tol is tighter.  casadi reports it as success
                                         like "Solve Succeeded".  Never returned when tol >= 1e-6 (the reference's own tol). */
#define MPC_STATUS_ACCEPTABLE_ON_KINK 7 /* the same with a vehicle held at the d = 1 discontinuity (see status 5) */
#define MPC_STATUS_KINK_UNSOLVED 8     /* MPC_FLAG_STRICT_DISCONTINUITY only: would be status 5 or 7; counted as not solved */
/* solved, as a caller should count it: status 0, 5, 6, 7 */
#define MPC_STATUS_IS_SOLVED(st) ((st) == 0 || ((st) >= 5 && (st) <= 7))

typedef struct mpc_handle mpc_handle;

typedef struct mpc_config {
    int32_t struct_size; /* sizeof(mpc_config), for ABI evolution */
    int32_t horizon;     /* N; reference cfg key `horizon` (config/cfg.yaml:90 default 16, BASELINE uses 20) */
    double dt;           /* 1 / policy_frequency (agents/base_agent.py:43), 0.1 */
    int32_t max_iter;    /* interior-point iteration cap (reference: ipopt.max_iter 1000, agents/pure_mpc.py:294) */
    int32_t device;      /* HIP device ordinal */
    double tol;          /* scaled KKT tolerance (reference: ipopt.tol 1e-6, agents/pure_mpc.py:295); default 1e-8 */
    double w_distance;   /* cfg key weight_distance  (config/cfg.yaml:105), used with MPC_FLAG_COLLISION_COST */
    double w_collision;  /* cfg key weight_collision (config/cfg.yaml:106), used with MPC_FLAG_COLLISION_COST */
    int32_t ltv_passes;  /* iterative-linear agent: linearisation passes per call, the trip count of the loop at
                            agents/pure_mpc_linear.py:189 (`for _ in range(1)`); default 1 */
    int32_t stall_window; /* 0 (default) = off.  W > 0: a solve whose scaled KKT error has not halved within W consecutive
                            iterations ends with MPC_STATUS_STALLED instead of running on to max_iter - what makes the
                            reference's max_iter 1000 affordable in a batch, whose time is that of its slowest instance
                            (profiles/r03_tail.txt: one instance in a thousand never converges and costs 40 ms).  64
                            gives up on 2 - 6 of 4096 BASELINE-config-3 instances that would converge after 100 - 440
                            iterations.  Not an IPOPT option; the reference runs such instances to max_iter. */
} mpc_config;

/* ABI version of the loaded library (MPC_ABI_VERSION it was built with). */
int mpc_version(void);

/* Text of the last error raised on the calling thread ("" if none). */
const char *mpc_last_error(void);

/* Fill *cfg with the defaults (horizon 20, dt 0.1, max_iter 100, tol 1e-8, weights 10 / 1, device 0).
 * Writes sizeof(mpc_config) bytes of THIS header's layout: only for callers compiled against this header. */
void mpc_default_config(mpc_config *cfg);

/* The same for bindings that declare the struct themselves (ctypes, cgo, ...): `size` is the size of the caller's
 * object.  Nothing is written and MPC_ERR_INVALID_ARG is returned unless it equals the library's sizeof(mpc_config),
 * so a binding built for an older layout fails loudly instead of being overrun. */
int mpc_default_config_sized(mpc_config *cfg, int32_t size);

/* Create an engine bound to cfg->device.  Replaces PureMPC_Agent.__init__ (agents/pure_mpc.py:24-63). */
int mpc_create(const mpc_config *cfg, mpc_handle **out);

void mpc_destroy(mpc_handle *h);

/* Upload the global reference path: ref[M][4] = x, y, v, heading (host pointer).
 * Replaces the `reference_states` property (agents/base_agent.py:118-154), M = 85 there. */
int mpc_set_reference(mpc_handle *h, const double *ref, int32_t M);

/*
 * Solve B independent MPC instances (replaces B calls of PureMPC_Agent._solve, agents/pure_mpc.py:80-318).
 *   state      [B][4]    x, y, theta, v of the ego vehicle               (agents/pure_mpc.py:233-238)
 *   ego_index  [B]       index of the nearest reference point            (agents/pure_mpc.py:106-109)
 *   vref       [B][N+1]  reference speed of stage k = ref[min(ego_index+k, M-1)][2] after
 *                        update_reference_states (agents/pure_mpc.py:678-724); NULL = speeds of the table
 *   weights    [B][3]    weight_speed, weight_control, weight_input_diff (agents/pure_mpc.py:96-104)
 *   is_collide [B]       1: speed weight forced to 100 (agents/pure_mpc.py:143-147) and, with
 *                        MPC_FLAG_COLLISION_COST, the 3000 v^2 term is active
 *   others     [B][V][4] x, y, speed, heading of the other vehicles (constant-velocity model,
 *                        agents/base_agent.py:172-174); read only with MPC_FLAG_COLLISION_COST; may be NULL
 * outputs (u0 required, the rest optional = NULL):
 *   u0     [B][2]      first control (acceleration, steer) = MPC_Action    (agents/pure_mpc.py:311-318)
 *   U      [B][N][2]   full control sequence;  X [B][N+1][4] state trajectory
 *   status [B], iters [B]
 *   Where status is MPC_STATUS_INFEASIBLE_START nothing was iterated: U holds the controls of the start and, when U, X and
 *   status are all asked for, X their trajectory with every node written, outside the bounds as it is (without one of the
 *   three, X behind its first node outside the bounds is left as it was).
 *   stream: hipStream_t to enqueue on (NULL = the null stream)
 */
int mpc_solve_batch(mpc_handle *h, int32_t B, const double *state, const int32_t *ego_index, const double *vref,
                    const double *weights, const uint8_t *is_collide, const double *others, int32_t V,
                    uint32_t flags, double *u0, double *U, double *X, int32_t *status, int32_t *iters,
                    void *stream);

/*
 * Observation-level entry: everything PureMPC_Agent.predict() does (agents/pure_mpc.py:68-78) for B parallel
 * environments, on the device: observation parsing (agents/base_agent.py:81-116), the path-crossing collision
 * detector with its 10-step memory (agents/pure_mpc.py:552-676), the rewrite of the reference speed profile
 * (agents/pure_mpc.py:678-724) and the solve.  Environment b of the call owns state record b inside the handle
 * (records are created fresh on first use and persist across calls; see mpc_reset_env_state).
 *   obs            [B][vehicles_count][8] float32: presence, x, y, vx, vy, heading, sin_h, cos_h, absolute values,
 *                  row 0 = ego (config/config.py:4-26); present rows are contiguous (agents/base_agent.py:106-114)
 *   vehicles_count rows per observation, 1..MPC_MAX_OTHERS+1 (cfg `observation.vehicles_count`, 10)
 *   weights        [B][3] weight_speed, weight_control, weight_input_diff (RL action or the cfg defaults)
 *   ref_speed      [B] RL reference-speed override (agents/pure_mpc.py:683-688) or NULL
 *   flags          MPC_FLAG_COLLISION_COST: distance/collision terms over the observed vehicles; MPC_FLAG_DEVICE_PTRS,
 *                  MPC_FLAG_NO_SYNC as for mpc_solve_batch; MPC_FLAG_DETECT_ONLY / MPC_FLAG_DETECTED (above)
 *   act            [B][2] acceleration, steer;  status/iters [B] optional
 */
int mpc_predict_batch(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, const double *weights,
                      const double *ref_speed, uint32_t flags, double *act, int32_t *status, int32_t *iters,
                      void *stream);

/*
 * mpc_predict_batch_plan (an addition within ABI 8: old clients never call it, nothing else changes) - mpc_predict_batch that
 * also hands out the plan the solve ended with; mpc_predict_batch is this entry with U = X = NULL (one body).  Arguments,
 * flags and staging are those of mpc_predict_batch; with MPC_FLAG_DEVICE_PTRS U and X are device pointers, otherwise host
 * pointers, copied back like act.  Each is optional.
 *   U  [B][N][2]    the control sequence (acceleration, steer per stage), U[b][0] == act[b]
 *   X  [B][N+1][4]  the state trajectory x, y, theta, v (the state order of mpc_solve_batch); X[b][0] is the parsed state
 * Both hold the last iterate when the solve is not MPC_STATUS_IS_SOLVED, as in mpc_solve_batch.  The launches, and every bit
 * of act / status / iters, are those of mpc_predict_batch, and nothing is allocated.  With MPC_FLAG_WARM_START the kernel
 * writes its controls to the handle's warm-start memory as before and U is a device-to-device copy of that memory, enqueued
 * after the solve (capturable): the memory and the next step's iterates are exactly what they are without U.  With
 * MPC_FLAG_DETECT_ONLY nothing is solved and U and X are not written.  The two entries share one body, so the text of
 * mpc_last_error after a refusal names mpc_predict_batch whichever of them was called (likewise mpc_ltv_predict_batch below).
 */
int mpc_predict_batch_plan(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, const double *weights,
                           const double *ref_speed, uint32_t flags, double *act, double *U, double *X, int32_t *status,
                           int32_t *iters, void *stream);

/*
 * Iterative-linear MPC: B calls of IterativeLinearMPC_Agent._solve (agents/pure_mpc_linear.py:153-203): nearest
 * reference point (:38-60), forward simulation of the stored control profile (predict_motion, :84-110), linearisation
 * about it (linear_model_matrix, :62-82) and the QP of _linear_mpc_control (:205-257), which the reference gives to
 * cvxpy/ECOS and this engine solves with a Riccati-based primal-dual interior-point method.
 *   state  [B][4]     x, y, v, yaw of the ego vehicle - the state order of that agent (:23, :198)
 *   U      [B][N][2]  in: the stored profile (oa, od), zeros for a first call (:190-192); out: the new profile where
 *                     status is 0, unchanged elsewhere (:193-196).  Required.
 *   u0     [B][2]     acceleration, steer = U[b][0] where status is 0, else (0, 0) (:195)
 *   X      [B][N+1][4] optional: states of the linear model under the new controls (x, y, v, yaw)
 *   status [B]        MPC_STATUS_CONVERGED / MAX_ITER / FACTORIZATION, or MPC_STATUS_INFEASIBLE_START when the ego
 *                     speed is outside [0, 40/3.6] (the QP then has no feasible point: x[2,0] == v0, :252-256)
 *   target_index [B]  optional: index of the nearest reference point
 *   flags: MPC_FLAG_DEVICE_PTRS, MPC_FLAG_NO_SYNC.  cfg.horizon, dt, max_iter apply; the weights and bounds are the
 *   module constants of the reference (:27-37).
 */
int mpc_ltv_solve_batch(mpc_handle *h, int32_t B, const double *state, uint32_t flags, double *u0, double *U, double *X,
                        int32_t *status, int32_t *iters, int32_t *target_index, void *stream);

/* Observation-level entry of the same agent: Agent.predict (agents/base_agent.py:54-73) = _parse_obs + _solve for B
 * parallel environments.  Environment b owns a stored profile inside the handle (zeros until its first solve, kept
 * across calls, forgotten by mpc_reset_env_state / mpc_reset_env_mask).  obs, vehicles_count, act, status, iters as
 * for mpc_predict_batch. */
int mpc_ltv_predict_batch(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, uint32_t flags, double *act,
                          int32_t *status, int32_t *iters, void *stream);

/*
 * mpc_ltv_predict_batch_plan (an addition within ABI 8) - mpc_ltv_predict_batch that also hands out the plan;
 * mpc_ltv_predict_batch is this entry with U = X = NULL (one body, the same launch, the same bits).  U and X are optional,
 * device pointers with MPC_FLAG_DEVICE_PTRS, else host pointers.
 *   U  [B][N][2]    a device-to-device copy, enqueued after the solve, of the environment's stored profile (oa, od): the new
 *                   profile where status is 0 (then U[b][0] == act[b]), the profile the call started from elsewhere
 *   X  [B][N+1][4]  the states of the linear model under the profile of the last pass, x, y, v, yaw (the state order of
 *                   mpc_ltv_solve_batch).  Where status is MPC_STATUS_INFEASIBLE_START the kernel writes no X: those rows
 *                   are left as they were (with host pointers X is therefore copied in as well as out).
 */
int mpc_ltv_predict_batch_plan(mpc_handle *h, int32_t B, const float *obs, int32_t vehicles_count, uint32_t flags, double *act,
                               double *U, double *X, int32_t *status, int32_t *iters, void *stream);

/* Episode boundaries: forget collision memory / stop point of the listed environments (host array of n ids);
 * env_ids == NULL or n < 0 resets all.  Replaces constructing a new PureMPC_Agent (agents/pure_mpc.py:38-43,63). */
int mpc_reset_env_state(mpc_handle *h, const int32_t *env_ids, int32_t n, void *stream);

/* Same, from a done-mask: environment b is reset where done[b] != 0 (device pointer with MPC_FLAG_DEVICE_PTRS;
 * with MPC_FLAG_NO_SYNC the reset is only enqueued). */
int mpc_reset_env_mask(mpc_handle *h, int32_t B, const uint8_t *done, uint32_t flags, void *stream);

/* Detector state of environments 0..B-1 after the last mpc_predict_batch (host arrays, any may be NULL; synchronises):
 * is_collide, ego_index, collision_memory, stop_index (-1 = none) [B]; conflict_index [B][MPC_MAX_OTHERS] (-1 = none);
 * conflict_points [B][MPC_MAX_OTHERS][2] (NaN = none): where the predicted paths cross.
 * Serves the attributes callers / plots read from the agent (agents/pure_mpc.py:38-43, 589-593: is_collide,
 * conflict_points, conflict_index, agent_collide, stop_point). */
int mpc_get_env_state(mpc_handle *h, int32_t B, int32_t *is_collide, int32_t *ego_index, int32_t *collision_memory,
                      int32_t *stop_index, int32_t *conflict_index, double *conflict_points);

/* Checkpoint / resume of the per-environment detector records (the reference never saves them: its agent state is lost
 * with the process, agents/pure_mpc.py:38-43).  mpc_env_state_bytes(): size of one opaque record;
 * mpc_save_env_state copies records 0..B-1 to a host buffer of B * that size; mpc_set_env_state puts them back (into
 * this or another handle of the same library version), growing the handle's capacity if needed (not while a captured
 * hipGraph still addresses the old buffers: size the handle with mpc_reserve_envs first).  Every record is validated
 * (counts, indices against the reference table) and a bad one refuses the whole call; the restored environments lose
 * their warm-start controls and stored LTV profile (those belong to the episode that was running).  Both synchronise. */
int64_t mpc_env_state_bytes(void);
int mpc_save_env_state(mpc_handle *h, int32_t B, void *records);
int mpc_set_env_state(mpc_handle *h, int32_t B, const void *records);

/* Size the per-environment buffers (detector records, warm-start controls) for B environments now.  They otherwise grow
 * on demand, which frees the old buffers: not allowed inside a stream capture (a captured graph holds the addresses)
 * and it waits for the device to go idle.  Call this once before capturing a step into a hipGraph. */
int mpc_reserve_envs(mpc_handle *h, int32_t B);

/* Problem data the last mpc_predict_batch derived from the observations (host arrays, any may be NULL; synchronises):
 * state [B][4], ego_index [B], vref [B][N+1], is_collide [B], others [B][max(vehicles_count-1,1)][4], nveh [B].
 * Diagnostics / tests: these are exactly the arguments mpc_solve_batch would take. */
int mpc_get_last_inputs(mpc_handle *h, int32_t B, double *state, int32_t *ego_index, double *vref,
                        uint8_t *is_collide, double *others, int32_t *nveh);

/* Diagnostics / tests: the launch order of the last ORDERED solve of B instances on this handle (a batch of more than one wave
 * per SIMD without MPC_FLAG_THROUGHPUT) - order [B]: workgroup p solved instance order[p]; tier [B]: the tier of each
 * instance, 0 = the seat tier, 1..4 (host arrays, either may be NULL; synchronises).  What a launch that was not ordered
 * leaves there is unspecified. */
int mpc_get_launch_order(mpc_handle *h, int32_t B, int32_t *order, int32_t *tier);

/* Diagnostics for parity tests: with on != 0 every following mpc_predict_batch also keeps the polylines its detector
 * worked on.  mpc_get_last_paths then returns (host arrays, any may be NULL; synchronises), for environments 0..B-1 of that
 * call: ego_path [B][31][2] and ego_len [B] - what predict_ego_future_positions returns (agents/pure_mpc.py:459-527; 0
 * points where the environment replayed its collision memory, :558-563, and predicted nothing) - and agent_paths
 * [B][max(vehicles_count-1,1)][31][2] float32 - predict_future_positions per observed vehicle (:529-550; zeros for
 * absent vehicles).  Costs one memset and B * (500 + 248 V) bytes per call; off by default. */
int mpc_set_diagnostics(mpc_handle *h, int32_t on);
int mpc_get_last_paths(mpc_handle *h, int32_t B, double *ego_path, int32_t *ego_len, float *agent_paths);

/*
 * Synthetic intersection environment for MPC-in-the-loop rollouts (BASELINE configs 4-5; highway-env, which the reference
 * steps at agents/ppo_mpc.py:430-432, is not available offline): ONE launch per policy step for B environments - vehicle
 * models, respawn, reward / termination shape of envs/intersection_env_Feb2025_v1.py:80-155, terminal observation,
 * auto-reset and the next observation in the layout of config/config.py:10-26 (csrc/mpc_synth_env.hpp).  All pointers are
 * DEVICE memory on `device`; the call only enqueues on `stream` (capturable in a hipGraph).  State arrays, updated in
 * place: ego [B][4] x, y, heading, speed; opos [B][K'][2], ospeed / ohead [B][K'] f64, oactive [B][K'] u8 with
 * K' = max(K, 1); t [B] steps of the episode; rng_counter [B] (zero-initialised; with `seed` and env_offset + b it keys a
 * counter-based generator, so shards of one job draw distinct streams).  action [B][2] acceleration, steer.
 * Outputs: obs [B][10][8] f32 what the policy sees next (after the auto-reset), terminal_obs the same before it, reward [B]
 * f32, done / truncated / crashed / arrived [B] u8.  reset_all != 0: start fresh episodes everywhere and write obs only.
 * Limits (sixteen lanes per environment): K <= 15 other vehicles, M <= 128 route points; MPC_ERR_INVALID_ARG beyond.
 */
int mpc_synth_env_step(int32_t device, int32_t B, int32_t K, double dt, double spawn_probability, uint64_t seed,
                       int32_t env_offset, const double *ref_xy, int32_t M, const double *action, double *ego, double *opos,
                       double *ospeed, double *ohead, uint8_t *oactive, int32_t *t, int64_t *rng_counter, float *obs,
                       float *terminal_obs, float *reward, uint8_t *done, uint8_t *truncated, uint8_t *crashed,
                       uint8_t *arrived, int32_t reset_all, void *stream);

/*
 * mpc_synth_env_step_idm (an addition within ABI 8: old clients never call it, nothing else changes) - the same step with
 * reactive traffic (csrc/mpc_synth_traffic.hpp): every other vehicle follows one of twelve routes through the junction (its
 * entry lane x straight / left / right), keeps its distance with the Intelligent Driver Model and brakes for whatever stands
 * in the 40 m x 4 m corridor in front of it, the ego included; a respawned or reset vehicle is placed only where it is 10 m
 * clear of the others.  The ego, the crash test, reward, termination and the observation are those of mpc_synth_env_step.
 * Arguments of mpc_synth_env_step plus three state arrays, DEVICE memory, updated in place: oroute [B][K'] i32 = 3 * entry +
 * turn (entry 0..3 the approach lane, turn 0 straight, 1 left, 2 right), oprog [B][K'] f64 arc length along the route, otarget
 * [B][K'] f64 desired speed.  opos / ohead are written from (oroute, oprog) every step.  Same limits and error returns as
 * mpc_synth_env_step (a NULL oroute / oprog / otarget is MPC_ERR_INVALID_ARG); enqueues on `stream` only and never
 * synchronises (capturable in a hipGraph).  The draws mpc_synth_env_step makes keep their slots; the turn is one more draw.
 */
int mpc_synth_env_step_idm(int32_t device, int32_t B, int32_t K, double dt, double spawn_probability, uint64_t seed,
                           int32_t env_offset, const double *ref_xy, int32_t M, const double *action, double *ego, double *opos,
                           double *ospeed, double *ohead, uint8_t *oactive, int32_t *oroute, double *oprog, double *otarget,
                           int32_t *t, int64_t *rng_counter, float *obs, float *terminal_obs, float *reward, uint8_t *done,
                           uint8_t *truncated, uint8_t *crashed, uint8_t *arrived, int32_t reset_all, void *stream);

/*
 * Rollout glue for the same configurations (csrc/mpc_rollout_glue.hpp): what a step of the reference's collect_rollouts does
 * besides the MPC call and env.step, as two launches per step instead of ~40 torch kernels, and one at the rollout's end.  Device pointers, enqueue only.
 *
 * mpc_policy_act: the SB3 MlpPolicy-shaped actor-critic of PPO_MPC / A2C_MPC (agents/ppo_mpc.py:390-394; 80 -> H -> H tanh
 * twice, Gaussian head) for B observations obs [B][80] f32: both towers as one 80 -> 2H -> 2H -> (A + 1) network with the
 * weights laid out as w1 [80][2H], b1 [2H], w2 [2H][2H] (block diagonal), b2 [2H], wh [2H][A + 1], bh [A + 1], std [A] =
 * exp(log_std), c0 [1] = sum(log_std) + A / 2 log(2 pi); noise [B][A] the sample's standard normal draws: with noise_step
 * == NULL read from the caller (its own generator), otherwise DRAWN here - counter-based, keyed by (noise_seed, env_offset + b,
 * noise_step[0], component), no generator state, replayable in a hipGraph - and left in `noise`.
 * Outputs: actions [B][A] = mean + std * noise, values [B], log_probs [B], and the MPC's inputs as the reference maps the
 * action: version_v1 == 0 -> mpc_ref_speed [B] f64 = action 0 (agents/ppo_mpc.py:410-414), else mpc_weights [B][3] f64 =
 * actions 0..2 (:416-420); clip != 0 clips to the Box(-1, 1) action space first (PPO, :399-407; A2C does not, a2c_mpc.py:138-144).
 *
 * mpc_policy_act_sde: the same step with gSDE exploration (stable-baselines3's StateDependentNoiseDistribution as
 * ActorCriticPolicy(use_sde=True) builds it, the PPO agents' default, agents/ppo_mpc.py:114-115).  Same network and weight layout,
 * but sde_std [H][A] = exp(log_std) replaces std / c0.  With latent = the H policy units after layer 2 and E = sde_std * Z the
 * environment's exploration matrix [H][A]: actions = mean + latent @ E, log_probs = Normal(mean, sqrt(latent^2 @ sde_std^2 +
 * 1e-6)).log_prob(actions) summed over the components.  Z: with sde_noise [B][H][A] given, read from the caller (sde_epoch NULL);
 * otherwise DRAWN - counter-based, keyed by (noise_seed, env_offset + b, epoch, h * A + a) with epoch = sde_epoch[0] +
 * (sde_sample_freq > 0 ? sde_step[0] / sde_sample_freq : 0) (sde_step NULL reads as 0), so one matrix serves a whole epoch and is
 * never stored.  The caller advances sde_epoch[0] at every rollout start (far enough to pass the epochs the last rollout used);
 * sde_step is the policy steps taken in the rollout (the buffer position mpc_rollout_record advances).  Clip and MPC inputs as
 * mpc_policy_act.
 *
 * mpc_rollout_record: row pos_dev[0] of the rollout buffer row [T][B][cols] = [obs 80 | action A | reward | episode_start |
 * value | log_prob | (terminal_obs 80 | truncated)] (rollout_buffer.add, agents/ppo_mpc.py:462-469) and of mpc_actions_buf
 * [T][B][2]; last_obs <- new_obs, last_starts <- done; counts [4] += finished / crashed / arrived episodes and solves whose
 * status is not solved (MPC_STATUS_IS_SOLVED); dones_out <- done; pos_dev[0] += 1 (ticket: one zero-initialised int32 of
 * scratch) and, if given, step_counter[0] += 1 (the policy steps taken so far: mpc_policy_act's noise_step).  T is the number
 * of rows of the buffer: a step taken with pos_dev[0] >= T (or < 0) writes NOTHING to row / mpc_actions_buf - the torch path it
 * replaces raises an index error there - and is counted in counts[4] instead (counts is [5]: finished, crashed, arrived,
 * unsolved, refused steps); the carry-over, the counters and the position still advance.
 *
 * mpc_rollout_finish: the end of a rollout of T steps (1 <= T <= 8192) over the same buffer (agents/ppo_mpc.py:471-476
 * `rollout_buffer.compute_returns_and_advantage`, stable-baselines3's arithmetic in float32, operation by operation): if
 * keep_terminal and terminal_values [T][B] (V of every step's terminal observation) is given, the reward column becomes
 * reward + gamma * terminal_values * truncated first (the PPO agents' truncation bootstrap, :451-461); then, with
 * last_values [B] = V(observation after the last step) and dones [B] = the last step ended an episode, per environment
 *   delta_t = r_t + gamma V_{t+1} (1 - start_{t+1}) - V_t,  A_t = delta_t + gamma lambda (1 - start_{t+1}) A_{t+1}
 * backwards from t = T - 1 (V_T = last_values, start_T = dones); advantages [T][B] = A, returns [T][B] = A + V.
 */
int mpc_policy_act(int32_t device, int32_t B, int32_t A, int32_t H2, const float *obs, const float *w1, const float *b1,
                   const float *w2, const float *b2, const float *wh, const float *bh, const float *std_, const float *c0,
                   float *noise, uint64_t noise_seed, int32_t env_offset, const int64_t *noise_step, int32_t version_v1,
                   int32_t clip, float *actions, float *values, float *log_probs, double *mpc_weights, double *mpc_ref_speed,
                   void *stream);
int mpc_policy_act_sde(int32_t device, int32_t B, int32_t A, int32_t H2, const float *obs, const float *w1, const float *b1,
                       const float *w2, const float *b2, const float *wh, const float *bh, const float *sde_std,
                       const float *sde_noise, uint64_t noise_seed, int32_t env_offset, const int64_t *sde_epoch,
                       const int64_t *sde_step, int32_t sde_sample_freq, int32_t version_v1, int32_t clip, float *actions,
                       float *values, float *log_probs, double *mpc_weights, double *mpc_ref_speed, void *stream);
int mpc_rollout_record(int32_t device, int32_t T, int32_t B, int32_t A, int32_t cols, int32_t keep_terminal, float *row,
                       double *mpc_actions_buf, int64_t *pos_dev, int32_t *ticket, float *last_obs, float *last_starts,
                       const float *actions, const float *values, const float *log_probs, const double *mpc_act,
                       const int32_t *mpc_status, const float *new_obs, const float *reward, const uint8_t *done,
                       const float *terminal_obs, const uint8_t *truncated, const uint8_t *crashed, const uint8_t *arrived,
                       int64_t *counts, uint8_t *dones_out, int64_t *step_counter, void *stream);
int mpc_rollout_finish(int32_t device, int32_t T, int32_t B, int32_t A, int32_t cols, int32_t keep_terminal, float *row,
                       const float *last_values, const uint8_t *dones, const float *terminal_values, double gamma,
                       double gae_lambda, float *advantages, float *returns, void *stream);

/*
 * mpc_policy_control (an addition within ABI 8: old clients never call it, nothing else changes) - the step of the end-to-end
 * baseline, the reference's fourth model (agents/ppo_agent.py: an SB3 MlpPolicy whose two outputs are the vehicle's controls,
 * no MPC in between).  The network, weight layout, noise and outputs of mpc_policy_act at A = 2 (Gaussian policies only; the
 * baseline does not use gSDE): actions [B][2] = mean + std * noise, values [B], log_probs [B] are bit for bit what
 * mpc_policy_act writes for the same inputs, and noise [B][2] is read (noise_step == NULL) or drawn and left there, keyed by
 * (noise_seed, env_offset + b, noise_step[0], component), exactly as there.  control [B][2] f64 is the action in physical
 * units, as highway-env's ContinuousAction maps it: clip to [-1, 1] (always: the clip belongs to the environment's action
 * type, not to the algorithm; `actions` stays unclipped), then acceleration = 5 * a0 m/s^2 and steering = pi / 4 * a1 rad
 * (acceleration_range / steering_range of config/config.py:27-32) - what mpc_synth_env_step takes as `action`.
 * Device pointers, enqueue only on `stream`, never synchronises (capturable in a hipGraph); no scratch, no atomics.  From
 * MPC_POLICY_CONTROL_TILE_FROM environments on, one workgroup serves MPC_POLICY_CONTROL_TILE consecutive environments (each
 * weight is loaded once per tile, not once per environment); below, where the tiles would leave most of the GPU idle, one
 * environment per workgroup as in mpc_policy_act.  The results do not depend on the tile.  DESIGN.md 5.2 has the measurement
 * behind both numbers.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, H2 odd, < 2 or > 256, a NULL pointer other than noise_step / stream.  B == 0: nothing
 * to do, no device call.
 *
 * mpc_policy_control_tile: the same launch with the tile chosen by the caller, tile = 1, 2, 4, 8 or 16 (anything else is
 * refused) - every tile computes the same bits; it exists so that tools/bench_policy_control.py can time them side by side.
 */
#define MPC_POLICY_CONTROL_TILE 4
#define MPC_POLICY_CONTROL_TILE_FROM 2048
int mpc_policy_control(int32_t device, int32_t B, int32_t H2, const float *obs, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *wh, const float *bh, const float *std_, const float *c0, float *noise,
                       uint64_t noise_seed, int32_t env_offset, const int64_t *noise_step, float *actions, float *values,
                       float *log_probs, double *control, void *stream);
int mpc_policy_control_tile(int32_t tile, int32_t device, int32_t B, int32_t H2, const float *obs, const float *w1,
                            const float *b1, const float *w2, const float *b2, const float *wh, const float *bh,
                            const float *std_, const float *c0, float *noise, uint64_t noise_seed, int32_t env_offset,
                            const int64_t *noise_step, float *actions, float *values, float *log_probs, double *control,
                            void *stream);

/*
 * mpc_episode_stats (an addition within ABI 8: old clients never call it, nothing else changes) - per-episode accounting of
 * a closed-loop evaluation of B environments (the reference's model comparison, main/model_comparison.py:40-100, with the
 * per-environment update in csrc/mpc_episode_stats.hpp).  Device pointers, enqueue only on `stream`, never synchronises
 * (capturable in a hipGraph); one thread per environment, no scratch.  One launch per policy step, after mpc_synth_env_step.
 *
 * Inputs of a step: done, truncated, crashed, arrived [B] u8 and reward [B] f32 (the environment's outputs), ego [B][4] f64
 * (x, y, heading, speed after the step and its auto-reset), status and iters [B] i32 (the step's MPC solve).
 * Running state, zero-initialised by a reset launch: state_i32 [5][B] = steps of the current episode, crashed on any step,
 * unsolved solves (not MPC_STATUS_IS_SOLVED: right for the NLP and the LTV statuses), largest iteration count, episode
 * ordinal j; state_f64 [3][B] = sum of the speeds before each step, return (f64 sum of the f32 rewards), carry_speed.
 * Records, one slot per (environment b, ordinal j < Q): rec_i32 [6][B][Q] = steps, success (arrived), collision (crashed on
 * any step of the episode; crash and arrival on one step set both, as in the reference), truncated, unsolved, max_iters;
 * rec_f64 [2][B][Q] = average speed (speed sum / steps), return.
 *
 * The speed summed at a step is the ego speed BEFORE it: every launch ends by storing ego[b][3] in carry_speed, the next one
 * adds it.  reset != 0 (issue it after the environments' reset; the step inputs may be NULL): initialise the running state and
 * carry_speed, and recorded[0] = 0.  Otherwise, for every environment: steps += 1, speed sum += carry_speed, return +=
 * reward, crashed |= crashed[b], unsolved += !solved, max_iters = max(max_iters, iters[b]); when done[b]: if j < Q write slot
 * [b][j] and recorded[0] += 1; then clear the running state and j += 1 (up to Q: an environment whose Q episodes are
 * recorded keeps stepping with the batch and writes nothing).  A fixed quota per environment keeps the evaluated episodes
 * independent of how long other environments' episodes last and of how the batch is sharded.
 * step_counter (optional, non-reset launches): step_counter[0] += 1 - mpc_policy_act's noise_step for a stochastic policy.
 * Errors: B < 0, Q < 1, a NULL state / record / recorded pointer, or a NULL step input of a non-reset launch.
 */
int mpc_episode_stats(int32_t device, int32_t B, int32_t Q, int32_t reset, const uint8_t *done, const uint8_t *truncated,
                      const uint8_t *crashed, const uint8_t *arrived, const float *reward, const double *ego,
                      const int32_t *status, const int32_t *iters, int32_t *state_i32, double *state_f64, int32_t *rec_i32,
                      double *rec_f64, int64_t *recorded, int64_t *step_counter, void *stream);

/*
 * mpc_drive_metrics (an addition within ABI 8: old clients never call it, nothing else changes) - safety and comfort metrics
 * of a closed-loop evaluation of B environments, per episode, beside mpc_episode_stats: how close the ego got, how long it
 * was on a collision course, how hard it braked and jerked, how well it kept its route (formulas, in evaluation order, and
 * the per-environment update in csrc/mpc_drive_metrics.hpp; the thresholds there are this project's).  Device pointers,
 * enqueue only on `stream`, never synchronises (capturable in a hipGraph); sixteen lanes per environment, no LDS, no scratch.
 * One launch per policy step, after mpc_synth_env_step (or any environment with the reference's observation layout: the
 * update reads observations and the action only).
 *
 * Inputs of a step: terminal_obs [B][R][8] f32 (the scene after the step, before the auto-reset: presence, x, y, vx, vy,
 * heading, sin_h, cos_h; row 0 the ego, rows 1 .. R-1 the other vehicles, counted when presence != 0), obs [B][R][8] f32 (what
 * the next step starts from), action [B][2] f64 (acceleration, steering as commanded), done [B] u8, ref_xy [M][2] f64 (the
 * ego's route), dt (step length, s).
 * Running state: state_i32 [5][B] = steps, ttc_steps (time to collision < 2 s), close_steps (box gap < 1 m),
 * hard_brake_steps (longitudinal acceleration < -3 m/s^2), episode ordinal j; state_f64 [17][B] = min centre gap, min box
 * gap, min ttc, max |a_lon|, max |a_lat|, sum of squared jerk, max jerk, max steering rate, sum of the cross-track error,
 * max cross-track error, then the carries vx, vy, cos_h, sin_h, ax, ay, steer.
 * Records, one slot per (environment b, ordinal j < Q), the slot mpc_episode_stats writes for the same episode:
 * rec_i32 [4][B][Q] = steps, ttc_steps, close_steps, hard_brake_steps; rec_f64 [10][B][Q] = min_centre_gap, min_box_gap,
 * min_ttc (+inf when no other vehicle was ever present / on a collision course), max_abs_alon, max_abs_alat, rms_jerk
 * (sqrt(sum / (steps - 1)), 0 when steps < 2), max_jerk, max_steer_rate, mean_xte, max_xte.
 *
 * reset != 0 (issue it after the environments' reset; terminal_obs, action and done may be NULL): initialise the running
 * state, and the carries from obs.  Otherwise update the running state; when done[b]: if j < Q write slot [b][j]; then clear
 * the running state and j += 1 (up to Q).  Every launch ends by storing the carries from obs row 0 and the step's ax, ay,
 * steer.  All arithmetic is f64 without contraction on + - * / sqrt fabs: the kernel, a host build of the header and the
 * evaluator's torch path agree bit for bit.
 * Errors: B < 0, Q < 1, R outside 1 .. MPC_MAX_OTHERS + 1, M outside 1 .. 128, dt <= 0, a NULL state / record / obs / ref_xy
 * pointer, or a NULL terminal_obs / action / done of a non-reset launch.
 */
int mpc_drive_metrics(int32_t device, int32_t B, int32_t R, int32_t Q, int32_t M, int32_t reset, double dt,
                      const float *terminal_obs, const float *obs, const double *action, const uint8_t *done,
                      const double *ref_xy, int32_t *state_i32, double *state_f64, int32_t *rec_i32, double *rec_f64,
                      void *stream);

/*
 * mpc_interaction_metrics (an addition within ABI 8: old clients never call it, nothing else changes) - interaction metrics
 * of a closed-loop evaluation of B environments with reactive traffic, per episode, beside mpc_episode_stats and
 * mpc_drive_metrics: what the ego does to the other vehicles - how often one yields to it, how hard it makes one brake, how
 * much speed that costs the traffic, and the post-encroachment time where a traffic route crosses the ego's (formulas, in
 * evaluation order, and the per-environment update in csrc/mpc_interaction.hpp; the 1.5 s threshold there is this project's).
 * Device pointers, enqueue only on `stream`, never synchronises (capturable in a hipGraph); sixteen lanes per environment, the
 * route staged in LDS, no atomics, no scratch.  One launch per policy step, after mpc_synth_env_step_idm: unlike
 * mpc_drive_metrics the update reads the simulator's slots, so it serves that environment only.
 *
 * Inputs of a step, all const: the state arrays of mpc_synth_env_step_idm after the step and its auto-reset (ego [B][4],
 * opos [B][K][2], ospeed, ohead, oprog, otarget [B][K] f64, oactive [B][K] u8, oroute [B][K] i32), done [B] u8, ref_xy [M][2]
 * f64 (the ego's route), conflict [12][2] f64 = per traffic route the arc length along ref_xy and along the route where the
 * two cross (the first < 0: no crossing conflict), dt (step length, s).
 * Running state: state_i32 [18][B] = steps, yield_steps, forced_brake_steps, forced_brake_events, conflicts, pet_critical,
 * ego_first, episode ordinal j, the previous state's mask of hard-braking vehicles, then 9 carried oroute (-1: empty slot);
 * state_f64 [34][B] = max_forced_decel, speed_deficit, min_pet, the carried arc length of the ego, then 12 pass times of the
 * ego (one per route), 9 pass times of the slots and 9 carried oprog.  A pass time that is not set is -1.
 * Records, one slot per (environment b, ordinal j < Q), the slot mpc_episode_stats writes for the same episode:
 * rec_i32 [7][B][Q] = steps, yield_steps (states in which a vehicle's leader is the ego), forced_brake_steps (... and it brakes
 * harder than 3 m/s^2), forced_brake_events (vehicles that begin to), conflicts (post-encroachment times evaluated),
 * pet_critical (below 1.5 s), ego_first; rec_f64 [3][B][Q] = max_forced_decel, speed_deficit (m/s: the acceleration each
 * yielding vehicle would have had without the ego minus the one it has, times dt, summed), min_pet (+inf when none).
 *
 * The states of an episode that are folded are those its decisions were made in, s_0 .. s_{T-1}; the terminal state is not.
 * reset != 0 (issue it after the environments' reset; done may be NULL): clear the running state and fold the fresh state.
 * Otherwise, when done[b]: if j < Q write slot [b][j] from the states folded so far, then clear and j += 1 (up to Q), and
 * fold the current (fresh) state as state 0 of the next episode; when not done: fold the current state.  f64 without
 * contraction; cos and sin are each build's own, so the kernel and a host build of the header agree to their rounding.
 * Errors: B < 0, Q < 1, K outside 1 .. 9, M outside 1 .. 128, dt <= 0, any NULL array, or a NULL done of a non-reset launch.
 */
int mpc_interaction_metrics(int32_t device, int32_t B, int32_t K, int32_t Q, int32_t M, int32_t reset, double dt,
                            const double *ego, const double *opos, const double *ospeed, const double *ohead,
                            const uint8_t *oactive, const int32_t *oroute, const double *oprog, const double *otarget,
                            const uint8_t *done, const double *ref_xy, const double *conflict, int32_t *state_i32,
                            double *state_f64, int32_t *rec_i32, double *rec_f64, void *stream);

/*
 * mpc_episode_trace (an addition within ABI 8: old clients never call it, nothing else changes) - the step-by-step record of
 * the episodes of a closed-loop evaluation of B environments that someone will look at, beside mpc_episode_stats: every
 * environment keeps the last W steps of its current episode in rings, and an episode that ends and is selected by its outcome
 * is copied in chronological order to the next free slot of a store with capacity C (the model, the layouts and the
 * per-environment append and commit in csrc/mpc_episode_trace.hpp).  Device pointers, enqueue only on `stream`, never
 * synchronises (capturable in a hipGraph); two launches per call - the claim, one workgroup that ranks the environments whose
 * episode ends with a wave ballot and hands out the slots in environment order, then one workgroup of four waves per
 * environment for the append and the copy, 16 bytes per lane; no atomics, no scratch.  One call per policy step, after the
 * environment's step and before the buffer the agent acted on is overwritten.
 *
 * Inputs of a step: terminal_obs [B][R][8] f32 (the scene after the step, before the auto-reset), obs [B][R][8] f32 (what the
 * next step starts from), seen [B][R][8] f32 or NULL (what the agent acted on at this step, with a perception model), action
 * [B][2] f64 as commanded, reward [B] f32, done, truncated, crashed, arrived [B] u8, status and iters [B] i32 (the step's
 * solve).  Q: the quota of mpc_episode_stats; only episodes of ordinal j < Q are traced.  keep: the outcomes that are kept, a
 * bit set of 1 collision (crashed on any step), 2 truncated, 4 success (arrived), 8 unsolved (a solve that is not
 * MPC_STATUS_IS_SOLVED), 16 all; an episode is selected when keep & 16 or outcome & keep & 15.
 * Running state: state_i32 [4][B] = steps of the current episode, crashed so far, unsolved so far, episode ordinal j.
 * Rings: ring_scene [B][W + 1][R][8] f32 (scene t of the episode at index t mod (W + 1)), ring_seen [B][W][R][8] f32 or NULL,
 * ring_act [B][W][2] f64, ring_reward [B][W] f32, ring_i32 [B][W][3] = status, iters, flags (bit 0 done, 1 truncated, 2
 * crashed, 3 arrived); frame t at index t mod W.  slot [B] i32: work array between the two launches (the slot of an episode
 * that ends on this step, else -1).  slot keeps these values until the next mpc_episode_trace call (mpc_plan_trace reads it).
 * Store: kept_scene [C][W + 1][R][8], kept_seen [C][W][R][8] or NULL, kept_act [C][W][2], kept_reward [C][W], kept_i32
 * [C][W][3]: of a kept episode of T steps the last L = min(T, W), first = T - L: kept frame i is step first + i (i < L), kept
 * scene i is s_{first + i} (i <= L); entries past L are not written.  index [C][6] i32 = environment b, ordinal j, steps T,
 * first, outcome, the launch the episode ended on (1-based since the reset launch).  counts [4] i64 = matched, kept, dropped
 * (selected, but the store was full), launches; matched = kept + dropped.  Selected episodes take slots 0, 1, .. ordered by
 * the launch on which they ended, then by environment index.
 *
 * reset != 0 (issue it after the environments' reset; only obs is required): clear the running state and the counts, write
 * obs as s_0 of every environment; the store is not touched.  Otherwise, for every environment with j < Q: append the frame
 * and the scene terminal_obs; when done[b]: if the episode is selected and has a slot, copy the rings out and write its index
 * row; then clear the running state, j += 1, and write obs[b] as s_0 of the next episode.  An environment with j == Q writes
 * nothing.  Every scene plane (terminal_obs, obs, seen, ring_scene, ring_seen, kept_scene, kept_seen) must be 16-byte aligned.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, R outside 1 .. MPC_MAX_OTHERS + 1, Q < 1, W outside 1 .. 4096, C < 1, keep outside
 * 1 .. 31, a NULL state / ring / slot / store / index / counts pointer, a NULL obs, a NULL step input of a non-reset launch,
 * seen, ring_seen and kept_seen not all given or all NULL (a reset launch needs no seen), a misaligned scene plane.  B == 0
 * is a no-op.
 */
int mpc_episode_trace(int32_t device, int32_t B, int32_t R, int32_t Q, int32_t W, int32_t C, int32_t keep, int32_t reset,
                      const float *terminal_obs, const float *obs, const float *seen, const double *action,
                      const float *reward, const uint8_t *done, const uint8_t *truncated, const uint8_t *crashed,
                      const uint8_t *arrived, const int32_t *status, const int32_t *iters, int32_t *state_i32,
                      float *ring_scene, float *ring_seen, double *ring_act, float *ring_reward, int32_t *ring_i32,
                      int32_t *slot, float *kept_scene, float *kept_seen, double *kept_act, float *kept_reward,
                      int32_t *kept_i32, int32_t *index, int64_t *counts, void *stream);

/*
 * mpc_plan_metrics (an addition within ABI 8: old clients never call it, nothing else changes) - the MPC's plan against what
 * happened in a closed-loop evaluation of B environments, per episode, beside mpc_drive_metrics: how close the planned path
 * comes to where the observed vehicles will be (planned clearance), how far the ego ended up from where earlier plans put it
 * (prediction error by lead) and how much a new plan's first control departs from what the previous plan intended for this
 * step (replanning jump).  Formulas, in evaluation order, and the per-environment update in csrc/mpc_plan.hpp.  Device
 * pointers, enqueue only on `stream`, never synchronises (capturable in a hipGraph); sixteen lanes per environment, no LDS, no
 * atomics, no scratch.  One launch per policy step after the environment's step, and one with reset != 0 before the first.
 *
 * Inputs of a step: plan_X [B][N+1][4], plan_U [B][N][2] f64 and status [B] i32 (the step's solve, from
 * mpc_predict_batch_plan / mpc_ltv_predict_batch_plan; a plan is valid iff MPC_STATUS_IS_SOLVED(status), an invalid one is
 * counted and skipped everywhere), order (0: x, y, theta, v; 1: x, y, v, yaw - only x, y are read), acted [B][R][8] f32 (the
 * observation the agent acted on), terminal_obs [B][R][8] f32 (the scene after the step, before the auto-reset), done [B] u8,
 * dt [s], gap [m], lead0 .. lead3 (each 1 .. N, or 0 for unused; Lmax = the largest).
 * Per step: c = the minimum over the stages k = 1 .. N and the rows j >= 1 of `acted` with presence != 0 of the distance
 * between X[k].xy and (x_j + k dt vx_j, y_j + k dt vy_j); for each used lead h <= t + 1 whose plan p = t + 1 - h was valid,
 * e = |terminal_obs row 0 xy - X_p[h].xy|; for t >= 1 with both plans valid |U_t[0] - U_{t-1}[min(1, N - 1)]| per channel.
 * Running state: state_i32 [10][B] = steps, plans_valid, conflict_steps (c < gap), prev_valid, episode ordinal j, lead_n[4],
 * replan_n; state_f64 [15][B] = min_plan_gap, replan_sum[2], replan_max[2], lead_sum[4], lead_max[4], prev_u[2]; ring_xy
 * [B][Lmax][4][2] f64 = X_t[lead_i].xy at index t mod Lmax, ring_valid [B][Lmax] i32.
 * Records, one slot per (environment b, ordinal j < Q), the slot mpc_episode_stats writes for the same episode: rec_i32
 * [8][B][Q] = steps, plans_valid, plan_conflict_steps, replan_n, lead_n[4]; rec_f64 [13][B][Q] = min_plan_gap (+inf when no
 * valid plan ever met a present vehicle), replan_accel_mean, replan_steer_mean, replan_accel_max, replan_steer_max,
 * lead_mean[4], lead_max[4] (a mean is sum / n, 0 when n == 0).
 *
 * reset != 0 (the step inputs may be NULL): the running state of every environment returns to its start, the ring's validity
 * is cleared.  Otherwise update; when done[b]: if j < Q write slot [b][j] and j += 1; then clear the running state and the
 * ring's validity.  An environment past its quota writes no record.  All arithmetic is f64 without contraction on + - * /
 * sqrt fabs: the kernel, a host build of the header and the evaluator's numpy path agree bit for bit.
 * Errors (MPC_ERR_INVALID_ARG), one per rule: B < 0, N outside 1 .. MPC_MAX_HORIZON, R outside 1 .. MPC_MAX_OTHERS + 1,
 * Q < 1, dt NaN or <= 0, gap NaN or < 0, a lead outside 0 .. N, no lead used, order outside 0 .. 1, a NULL state / ring /
 * record pointer, a NULL step input of a non-reset launch.  B == 0 is a no-op.
 */
int mpc_plan_metrics(int32_t device, int32_t B, int32_t N, int32_t R, int32_t Q, int32_t reset, int32_t order, double dt,
                     double gap, int32_t lead0, int32_t lead1, int32_t lead2, int32_t lead3, const double *plan_X,
                     const double *plan_U, const int32_t *status, const float *acted, const float *terminal_obs,
                     const uint8_t *done, int32_t *state_i32, double *state_f64, double *ring_xy, int32_t *ring_valid,
                     int32_t *rec_i32, double *rec_f64, void *stream);

/*
 * mpc_plan_trace (an addition within ABI 8) - the plan planes of the episodes mpc_episode_trace keeps: call it right after
 * mpc_episode_trace, on the same stream, for the same step, with that call's work array `slot` and the same B, Q, W, C and
 * done.  Device pointers, enqueue only, capturable; one workgroup of four waves per environment, no atomics, no LDS.
 * Every environment with ordinal j < Q appends plan_X [B][N+1][4] / plan_U [B][N][2] f64 to ring_X [B][W][N+1][4] / ring_U
 * [B][W][N][2] at t mod W; when done[b] and 0 <= slot[b] < C the last L = min(T, W) frames are copied chronologically to
 * kept_X [C][W][N+1][4] / kept_U [C][W][N][2] at slot[b]: kept frame i is the plan that produced the recorder's action frame
 * i.  state_i32 [2][B] = steps of the current episode, ordinal j (done advances it; j >= Q writes nothing).  reset != 0 clears
 * state_i32 (the step inputs may be NULL).  The order, the capacity and the selection are the recorder's.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, N outside 1 .. MPC_MAX_HORIZON, Q < 1, W outside 1 .. 4096, C < 1, a NULL state /
 * ring / store pointer, a NULL step input of a non-reset launch.  B == 0 is a no-op.
 */
int mpc_plan_trace(int32_t device, int32_t B, int32_t N, int32_t Q, int32_t W, int32_t C, int32_t reset, const double *plan_X,
                   const double *plan_U, const uint8_t *done, const int32_t *slot, int32_t *state_i32, double *ring_X,
                   double *ring_U, double *kept_X, double *kept_U, void *stream);

/*
 * mpc_perceive (an addition within ABI 8: old clients never call it, nothing else changes) - a perception model between the
 * environment and the agent of a closed-loop evaluation: obs_seen is what the ego sees of the true scene obs_true under a
 * limited range, occlusion by the other vehicles' 5 m x 2 m rectangles and by static convex quadrilaterals, random dropout
 * and bounded measurement noise (every formula, in evaluation order, in csrc/mpc_perception.hpp).  Device pointers, enqueue
 * only on `stream`, never synchronises (capturable in a hipGraph); sixteen lanes per environment, no LDS, no scratch.  One
 * launch per policy step, after the environment's step, and one with reset != 0 after the environments' reset.
 *
 * obs_true, obs_seen [B][R][8] f32 (presence, x, y, vx, vy, heading, sin_h, cos_h; row 0 the ego, copied); occluders
 * [S][4][2] f64, corners in order (NULL when S == 0); row_class [B][R] u8 or NULL: per INPUT row 0 absent, 1 seen, 2 out of
 * range, 3 occluded, 4 dropped; counts [5][B] i64 += rows >= 1 present, seen, out of range, occluded, dropped; ctr [B] i64:
 * the launch counter that keys the draws with (seed, env_offset + b), += 1.  The seen rows are compacted to rows 1, 2, ...
 * in input order, the rest is +0.0f.  reset != 0: ctr and the counts of every b start from 0, then the launch perceives
 * obs_true like any other.  With every parameter off (range +inf, occlusion 0, min_points 1, p_drop and the sigmas 0) obs_seen is obs_true bit for bit when the
 * input's present rows are contiguous.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, R outside 1 .. MPC_MAX_OTHERS + 1, S outside 0 .. 8 or S > 0 with NULL occluders, a
 * NULL params / obs_true / obs_seen / counts / ctr, obs_seen == obs_true, a wrong struct_size, min_points outside 1 .. 5,
 * p_drop outside [0, 1], a negative or NaN sigma, range NaN or <= 0.  B == 0 is a no-op.
 */
typedef struct mpc_perception {
    int32_t struct_size; /* sizeof(mpc_perception), checked like mpc_config.struct_size */
    int32_t occlusion;   /* 0 off, 1: vehicles and static occluders hide what is behind them */
    int32_t min_points;  /* 1..5: a row is seen when at least this many of centre + four corners are visible */
    int32_t env_offset;  /* global id of environment 0 of this batch (sharding) */
    double range;        /* m; +inf = off */
    double p_drop;       /* probability that a visible row is dropped, [0, 1] */
    double sigma_pos;    /* m */
    double sigma_vel;    /* m/s */
    double sigma_head;   /* rad */
    uint64_t seed;
} mpc_perception;

int mpc_perceive(int32_t device, int32_t B, int32_t R, int32_t S, int32_t reset, const mpc_perception *params,
                 const float *obs_true, const double *occluders, float *obs_seen, uint8_t *row_class, int64_t *counts,
                 int64_t *ctr, void *stream);

/*
 * mpc_track_rows (an addition within ABI 8: old clients never call it, nothing else changes) - a tracker between the
 * perception model (or the true observation) and the agent of a closed-loop evaluation: a vehicle that vanishes from the
 * observation for up to `coast` launches stays in obs_out, moved on with its last velocity; measurements are smoothed by the
 * gains alpha_pos and alpha_vel; every output row gets an identity, the track slot behind it (every formula, in evaluation
 * order, in csrc/mpc_tracker.hpp).  Device pointers, enqueue only on `stream`, never synchronises (capturable in a hipGraph);
 * sixteen lanes per environment, a lane both a row and a slot, no LDS, no atomics, no scratch.  One launch per policy step,
 * after mpc_perceive where there is one, and one with reset != 0 after the environments' reset.
 *
 * obs_meas, obs_out [B][R][8] f32 (presence, x, y, vx, vy, heading, sin_h, cos_h; row 0 the ego, copied; finite); done [B] u8
 * or NULL: the environments whose episode ended on this step.  State, 16 slots per environment whatever R is: track_f64
 * [B][16][7] = x, y, vx, vy, heading, sin_h, cos_h; track_i32 [B][16][3] = alive, age, miss.  A launch: reset != 0 or done[b]
 * clears the slots of b; every alive slot is predicted by dt; the present rows, in row order, each claim the nearest alive
 * unclaimed slot within `gate` metres (squared distances against gate * gate, a tie to the lowest slot) and update it; an
 * unclaimed slot coasts (miss += 1) and expires when miss > coast; an unassociated row is born into the next free slot, or,
 * when none is free, evicts the lowest coasting one.  obs_out: the alive slots ordered by their squared distance to the ego
 * (ties to the lowest slot), the first R - 1 of them as rows 1, 2, ... with presence 1.0f, the rest +0.0f.  row_slot [B][R]
 * u8 or NULL: the slot behind each output row, 255 for row 0 and for empty rows; row_miss [B][R] u8 or NULL: that slot's miss
 * (0: measured in this launch).  counts [7][B] i64 += measured, matched, born, coasted, expired, evicted, cut; reset != 0
 * zeroes them first.  With coast 0 and both gains 1 obs_out is the present rows of obs_meas bit for bit, in that order.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, R outside 1 .. MPC_MAX_OTHERS + 1, dt NaN or <= 0, gate NaN or < 0 (+inf is allowed),
 * coast outside 0 .. 200, alpha_pos or alpha_vel outside (0, 1], a NULL obs_meas / obs_out / track_f64 / track_i32 / counts,
 * obs_out == obs_meas.  B == 0 is a no-op.
 */
int mpc_track_rows(int32_t device, int32_t B, int32_t R, int32_t reset, double dt, double gate, int32_t coast,
                   double alpha_pos, double alpha_vel, const float *obs_meas, const uint8_t *done, float *obs_out,
                   uint8_t *row_slot, uint8_t *row_miss, double *track_f64, int32_t *track_i32, int64_t *counts,
                   void *stream);

/*
 * mpc_actuate (an addition within ABI 8: old clients never call it, nothing else changes) - an actuator model between the
 * agent and the plant of a closed-loop evaluation: `applied` is what the vehicle makes of the agent's `command` under a
 * transport delay of whole policy steps, lost commands (the previous one is held), calibration gain and offset, bounded noise,
 * a first-order lag, a rate limit and saturation (every formula, in evaluation order, in csrc/mpc_actuator.hpp).  Device
 * pointers, enqueue only on `stream`, never synchronises (capturable in a hipGraph); one lane per (environment, channel)
 * pair, 32 environments per wave, no LDS, no atomics, no scratch.  One launch per policy step between the agent's action and
 * the environment's step, and one with reset != 0 before the first.
 *
 * command, applied [B][2] f64 (acceleration m/s^2, steering rad; applied may be command); done_prev [B] u8 or NULL: the
 * environments whose episode ended on the previous step, so that this command is the first of a new episode (their delay
 * line, held command and lag state are cleared first).  State: state_f64 [10][B][2] = the last eight commands, what reached
 * the actuator last, what was applied last; age [B] i32 the commands of this episode; ctr [B] i64 the launch counter that
 * keys the draws with (seed, env_offset + b).  counts [5][B] i64 += steps, held, rate_limited, saturated, nonfinite (each at
 * most one per environment and launch; a NaN or infinite command is applied as 0.0 and counted); sums [2][B][2] f64: the sum
 * and the maximum of |applied - command|.  reset != 0: state, age, ctr, counts and sums of every environment become 0, no
 * command is read and no applied written (command, done_prev and applied may be NULL).  With every parameter off (delay 0,
 * p_hold 0, gain 1, offset 0, sigma 0, alpha 1, rate +inf, lo -inf, hi +inf) applied is command bit for bit for every finite
 * command.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, a NULL params / state_f64 / age / ctr / counts / sums, a NULL command / applied with
 * reset == 0, a wrong struct_size, delay outside 0 .. 7, dt NaN or <= 0, p_hold outside [0, 1], a gain or offset that is
 * not finite, a sigma that is negative or not finite, alpha outside (0, 1], rate NaN or <= 0 (+inf is allowed), lo > hi or
 * either NaN.  B == 0 is a no-op.
 */
typedef struct mpc_actuator {
    int32_t struct_size; /* sizeof(mpc_actuator), checked like mpc_config.struct_size */
    int32_t delay;       /* 0..7 whole policy steps between the command and its arrival at the actuator */
    int32_t env_offset;  /* global id of environment 0 of this batch (sharding) */
    int32_t reserved;    /* 0 */
    double dt;           /* s, the policy step: the rate limit per launch is rate * dt */
    double p_hold;       /* probability that a step's command is lost and the previous one held, [0, 1] */
    double gain[2];      /* per channel (0 acceleration, 1 steering); 1 = off */
    double offset[2];    /* 0 = off */
    double sigma[2];     /* standard deviation of the noise; 0 = off */
    double alpha[2];     /* lag: applied = prev + alpha (target - prev), (0, 1]; 1 = off; dt / (tau + dt) */
    double rate[2];      /* largest change per second; +inf = off */
    double lo[2];        /* saturation; -inf = off */
    double hi[2];        /* +inf = off */
    uint64_t seed;
} mpc_actuator;

int mpc_actuate(int32_t device, int32_t B, int32_t reset, const mpc_actuator *params, const double *command,
                const uint8_t *done_prev, double *applied, double *state_f64, int32_t *age, int64_t *ctr, int64_t *counts,
                double *sums, void *stream);

/*
 * mpc_compensate (an addition within ABI 8: old clients never call it, nothing else changes) - delay compensation in front of
 * an agent whose command takes effect `steps` policy steps after the scene it was computed from: `out` is the observation
 * predicted to that moment.  The compensator remembers the commands still in flight, rolls the ego through them with the
 * environment's own vehicle model behind the nominal actuator (first-order lag, rate limit, saturation; no gain, offset, noise
 * or hold: a compensator knows its nominal actuator, not its errors), and moves every other vehicle on with its observed
 * velocity, re-ordered by distance to the predicted ego (every formula, in evaluation order, in csrc/mpc_compensate.hpp).
 * Device pointers, enqueue only on `stream`, never synchronises (capturable in a hipGraph); sixteen lanes per environment, four
 * environments per wave, no LDS, no atomics, no scratch.  One launch per policy step after the scene has been sensed, with the
 * agent's command of the step that just ran, and one with reset != 0 on the first scene.  A deployment with a known latency
 * calls it in front of mpc_predict_batch.
 *
 * obs, out [B][R][8] f32 (presence, x, y, vx, vy, heading, sin_h, cos_h; row 0 the ego; finite; out must not be obs);
 * command [B][2] f64 (acceleration m/s^2, steering rad; a NaN or infinite one counts as 0.0); done [B] u8 or NULL: the
 * environments whose episode ended on this step, so that obs is the first scene of a new one (their memory is cleared and
 * their command is not read); pred [B][4] f64 or NULL: the predicted ego x, y, heading, speed.  State: ring [8][B][2] f64 the
 * last eight commands; prev [B][2] f64 the nominal applied action of the step that just ran; age [B] i32 the commands of this
 * episode; pring [8][B][2] f64 the predicted (x, y) of the last eight launches.  counts [B] i64 += the predictions scored
 * against the ego observed `steps` launches later; sums [2][B] f64: the sum and the maximum of that position error [m].
 * reset != 0: every environment starts anew, counts and sums become 0, command and done are not read (both may be NULL); obs is
 * compensated like any other scene, with no command in flight.  With steps == 0, out is obs bit for bit.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, R outside 1 .. 17, a NULL params / obs / out / ring / prev / age / pring / counts /
 * sums, a NULL command with reset == 0, out == obs, a wrong struct_size, steps outside 0 .. 7, dt NaN or <= 0, alpha outside
 * (0, 1], rate NaN or <= 0 (+inf is allowed), lo > hi or either NaN.  B == 0 is a no-op.
 */
typedef struct mpc_compensator {
    int32_t struct_size; /* sizeof(mpc_compensator), checked like mpc_config.struct_size */
    int32_t steps;       /* 0..7 whole policy steps to look ahead: the delay being compensated */
    double dt;           /* s, the policy step */
    double alpha[2];     /* nominal lag per channel (0 acceleration, 1 steering), (0, 1]; 1 = none; dt / (tau + dt) */
    double rate[2];      /* nominal largest change per second; +inf = none */
    double lo[2];        /* nominal saturation; -inf = none */
    double hi[2];        /* +inf = none */
} mpc_compensator;

int mpc_compensate(int32_t device, int32_t B, int32_t R, int32_t reset, const mpc_compensator *params, const float *obs,
                   const double *command, const uint8_t *done, float *out, double *pred, double *ring, double *prev,
                   int32_t *age, double *pring, int64_t *counts, double *sums, void *stream);

/*
 * mpc_compensate_stale (an addition within ABI 8: old clients never call it, nothing else changes) - mpc_compensate for a
 * scene that is itself `latency` policy steps old (mpc_delay_scene below, or a deployment's own sensing latency): the same
 * arguments, the same state, the same update, with the ego rolled through steps + min(latency, age) commands - the ones issued
 * since the scene shown and the ones still in flight - and the others moved on by as much.  prev is then the nominal applied
 * action of the step before the scene shown, and a prediction is scored against the ego that arrives steps + latency launches
 * later (csrc/mpc_compensate.hpp states every change; with latency == 0 it computes what mpc_compensate computes).
 * mpc_compensate stays and means latency 0; it launches a build of the kernel of its own.  A deployment that knows both its
 * sensing latency and its actuation delay calls this in front of mpc_predict_batch.  With steps + latency == 0, out is obs bit
 * for bit; with steps + latency > 0 every environment's out is written by the prediction's formulas, also while its own
 * look-ahead is still 0.
 * Errors (MPC_ERR_INVALID_ARG): those of mpc_compensate, and latency < 0 or steps + latency > 7.  B == 0 is a no-op.
 */
int mpc_compensate_stale(int32_t device, int32_t B, int32_t R, int32_t reset, const mpc_compensator *params, int32_t latency,
                         const float *obs, const double *command, const uint8_t *done, float *out, double *pred, double *ring,
                         double *prev, int32_t *age, double *pring, int64_t *counts, double *sums, void *stream);

/*
 * mpc_delay_scene (an addition within ABI 8: old clients never call it, nothing else changes) - sensing latency in front of the
 * agent's pipeline of a closed-loop evaluation: `out` is the true scene of `steps` policy steps ago, bit for bit, every row,
 * whatever its order (every statement, in evaluation order, in csrc/mpc_latency.hpp).  Launched in front of mpc_perceive and
 * mpc_track_rows, which then see the old frame from where the ego was then.  The first `steps` steps of an episode show the
 * episode's first scene, growing older: a frame of a finished episode is never shown in the next one.  Device pointers,
 * enqueue only on `stream`, never synchronises (capturable in a hipGraph); sixteen lanes per environment, four environments
 * per wave, no LDS, no atomics, no scratch.
 *
 * obs, out [B][R][8] f32 (out must not be obs); done [B] u8 or NULL: the environments whose episode ended on this step, so
 * that obs is the first scene of a new one; stale [B] i32 or NULL <- the age, in steps, of the frame handed out:
 * min(steps, frames of this episode before this one).  State: frames [8][B][R][8] f32 the last eight scenes; age [B] i32 the
 * frames pushed in this episode.  counts [B] i64 += 1 per launch; sums [3][B] f64: the sum of stale, the sum and the maximum
 * of the ego lag [m], the distance between row 0 of obs and row 0 of out.  reset != 0: every environment starts anew, counts
 * and sums become 0 before this launch is counted, done is not read.  With steps == 0, out is obs.
 * Errors (MPC_ERR_INVALID_ARG): B < 0, R outside 1 .. 17, steps outside 0 .. 7, a NULL obs / out / frames / age / counts /
 * sums, out == obs.  B == 0 is a no-op.
 */
int mpc_delay_scene(int32_t device, int32_t B, int32_t R, int32_t reset, int32_t steps, const float *obs, const uint8_t *done,
                    float *out, int32_t *stale, float *frames, int32_t *age, int64_t *counts, double *sums, void *stream);

/*
 * Diagnostics: the NLP's functions at GIVEN points, evaluated by the solve kernel's own code (csrc/mpc_wave.hpp:
 * Solver::evaluate - stage_terms / track / dist, which judge every line-search trial, and the model step of the rollouts),
 * so that f(z) and g(z) computed by the reference's statements (agents/pure_mpc.py:128-283; tests/golden/
 * reference_sequences.npz) pin the device directly and not only through solutions.  Host pointers, synchronous.
 * Problem data as for mpc_solve_batch (the ego state is X[b][0]); X [B][N+1][4], U [B][N][2] the point;
 * f [B] <- the objective, unscaled, terms of k = 0 .. N-1 (:128-212; with MPC_FLAG_COLLISION_COST plus the terms of
 * agents/archive/pure_mpc.py:189-206); x_next [B][N][4] <- the model's successor of (X[k], U[k]) (:220-257): the reference's
 * dynamics constraint is X[k+1] - x_next[k] = 0.
 */
int mpc_eval_nlp(mpc_handle *h, int32_t B, const int32_t *ego_index, const double *vref, const double *weights,
                 const uint8_t *is_collide, const double *others, int32_t V, uint32_t flags, const double *X, const double *U,
                 double *f, double *x_next);

/* LDS bytes one workgroup (= one wave = one instance) of the solve kernel uses with V other vehicles in the
 * collision-cost term (V = 0: term off): 13.5 KB at horizon 20 with 8 vehicles, the same in every build since round 5 (B is
 * accepted for compatibility and ignored).  The engine keeps no per-instance solver state in HBM.  (diagnostics / capacity
 * planning) */
int64_t mpc_workspace_bytes(const mpc_handle *h, int32_t B, int32_t V);

/* Do kernels on two streams of `device` run side by side?  *overlap <- 1 if a ~0.3 ms one-wave timer kernel enqueued on each
 * finishes in the time of one, 0 if they take the time of two: the HIP runtime multiplexes its streams onto a few hardware
 * queues (GPU_MAX_HW_QUEUES, 4 by default) and two streams that share one SERIALISE, whatever the kernels - which of a
 * process's streams share is decided when they are created (measured round 6: of torch's pool streams 0-7 two shared a
 * queue, 8-15 none; batches in flight on them gave 2.6 against 3.45 M solves/s).  A caller that keeps several independent
 * batches in flight (MPC_FLAG_THROUGHPUT; the reference's vectorised environments in groups, agents/a2c_mpc.py:111-180) picks
 * its streams with this probe (engine.concurrent_streams).  Synchronises both streams; not capturable. */
int mpc_streams_overlap(int32_t device, void *stream_a, void *stream_b, int32_t *overlap);

#ifdef __cplusplus
}
#endif
#endif /* MPC_MI355X_H */
