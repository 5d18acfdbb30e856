/*
 * include/cilqr.h -- C-ABI of the MI355X-native batched CILQR trajectory optimiser.
 *
 * Drop-in boundary for the reference's `planning::IlqrOptimizer`
 * (algorithm/ilqr/ilqr_optimizer.h:29-52) and its stages.  Plain pointers and sizes only; no
 * C++/torch types cross this boundary.  Every entry point returns 0 (CILQR_OK) or a negative
 * error code and never throws.
 *
 * The reference has no FFI/plugin layer; what each entry replaces:
 *   cilqr_default_config    IlqrConfig/Weights/VehicleParam default member initialisers
 *                           (algorithm/params/planner_config.h:45-73, vehicle_param.h:21-64),
 *                           RelaxBarrierFunction t/epsilon (algorithm/ilqr/barrier_function.h:144-145)
 *   cilqr_create/destroy    IlqrOptimizer::IlqrOptimizer / Init   (ilqr_optimizer.cc:13-51)
 *   cilqr_solve_batch       IlqrOptimizer::Plan + cost()          (ilqr_optimizer.cc:53-95, .h:50-52),
 *                           B independent problems per call
 *   cilqr_stage_*           the private stages of Optimize()      (ilqr_optimizer.cc:154-320):
 *       load            TransformGoals cc:141, ShrinkConstraints cc:438, NormalizeHalfPlane cc:475
 *       init_guess      iqr cc:793-842
 *       total_cost      TotalCost cc:417-436
 *       quadratize      DynamicsJacbian vehicle_model.cc:21 + CostJacbian cc:620 + CostHessian cc:638
 *       backward        Backward cc:334-390 (+ CalGradientNorm cc:322)
 *       forward         Forward cc:392-415
 *       nearest_lane    FindNeastLaneSegment cc:605-618 + LineSegment2d::DistanceTo (algorithm/math/line_segment2d.cpp:61-75)
 *   cilqr_open_loop_rollout ilqr::iLQR::OpenLoopRollout (algorithm/slover/ilqr.h:363-370) on
 *                           VehicleModel::Dynamics (vehicle_model.cc:88-121)
 *   cilqr_dp_plan           DpPlanner::Plan + ComputePathProfile (algorithm/planner/dp_planner.cpp:135-281), one scene
 *                           on the host; cilqr_dp_plan_batch: B scenes per call on the GPU
 *   cilqr_scene_points_batch  Environment::QueryStaticObstaclesPoints + QueryDynamicObstaclesPoints
 *                           (algorithm/utils/environment.cpp:133-182) at every knot's time, B scenes per call on the GPU
 *   cilqr_plan_scenes_batch   TrajectoryPlanner::Plan (algorithm/planner/trajectory_planner.cpp:28-162) for B scenes:
 *                           DP -> obstacle points -> corridors -> lane constraints -> solve -> result rows
 *   cilqr_resample_rows     DiscretizedTrajectory::EvaluateTime / EvaluateStation (algorithm/utils/discretized_trajectory.cpp:50-136,
 *                           math::slerp math_utils.h:208-225) for a list of queries, one trajectory on the host;
 *                           cilqr_resample_rows_batch: B trajectories per call on the GPU
 *   cilqr_frenet_rows       DiscretizedTrajectory::GetProjection (discretized_trajectory.cpp:138-190) of every row of a
 *                           trajectory onto the centre line, and cilqr_cartesian_points, its inverse GetCartesian
 *                           (cpp:192-196), on the host; cilqr_frenet_rows_batch / cilqr_cartesian_points_batch on the GPU
 *
 * Layout convention: every per-problem array is problem-major ("[B][...]"), IEEE fp64,
 * in host or device memory as flagged by `memory`.
 */
#ifndef CILQR_H_
#define CILQR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CILQR_ABI_VERSION 7

#define CILQR_NX 6  /* state  (x, y, theta, v, a, delta)   vehicle_model.h:11 */
#define CILQR_NU 2  /* control (jerk, delta_rate)           vehicle_model.h:12 */
#define CILQR_TRAJ_FIELDS 10 /* time,x,y,theta,v,a,delta,kappa,jerk,delta_rate  (cc:771-791) */
#define CILQR_COST_FIELDS 5  /* total,target,dynamic,corridor,lane_boundary     (h:14-27)    */
#define CILQR_LANE_FIELDS 7  /* a,b,c,start_x,start_y,end_x,end_y               (corridor.h:24-25) */
#define CILQR_MAX_DISCS 16
#define CILQR_MAX_LANE_SEGMENTS 256

/* error codes */
#define CILQR_OK 0
#define CILQR_ERR_NULL (-1)         /* null output / handle            (cc:64-66)  */
#define CILQR_ERR_CONSTRAINTS (-2)  /* empty corridor or lane list     (cc:68-73)  */
#define CILQR_ERR_KNOTS (-3)        /* n_knots != floor(horizon/dt+1)  (cc:75-78)  */
#define CILQR_ERR_CAPACITY (-4)     /* batch / cmax / lane segments above what create() sized */
#define CILQR_ERR_DEVICE (-5)       /* HIP runtime error or no gfx950 device */
#define CILQR_ERR_ARG (-6)          /* invalid argument value */
#define CILQR_ERR_STATE (-7)        /* stage called before the stage it depends on */
#define CILQR_ERR_NO_PATH (-8)      /* cilqr_dp_plan: every sampled path collides ("DP failed", trajectory_planner.cpp:32-35) */

/* per-problem termination status (exits of Optimize(), cc:154-320) */
#define CILQR_ST_RUNNING 0
#define CILQR_ST_CONVERGED_ABS 1 /* dcost < abs_cost_tol                  cc:281,287 */
#define CILQR_ST_CONVERGED_REL 2 /* dcost / cost_old < rel_cost_tol      cc:282     */
#define CILQR_ST_GNORM 3         /* gnorm < 1e-6 && lambda < 1e-5        cc:236     */
#define CILQR_ST_UNSOLVED 4      /* lambda > 1e11                        cc:302     */
#define CILQR_ST_MAX_ITER 5      /* iter == max_iter_num                 cc:312     */
#define CILQR_ST_NO_CORRIDOR 6   /* corridor_count < 0 at some knot: the corridor producer failed there
                                    (cilqr_build_corridors codes -2 ... -4), or the DP planner found no path for the
                                    scene (-5 at knot 0, written by cilqr_plan_scenes_batch); the reference aborts the whole Plan
                                    (corridor.cc:78-81, trajectory_planner.cpp:49-57).  The problem is not
                                    optimised: traj = the init guess, n_cost = 1, n_iter = 1 */

#define CILQR_INIT_IQR 0
#define CILQR_INIT_TRACKER 1

#define CILQR_MEM_HOST 0
#define CILQR_MEM_DEVICE 1

/* Live configuration fields only (dead ones -- IlqrConfig::t/t_rate/alpha/gamma/rho,
 * planner_config.h:60-61,68-70 -- are not carried). */
typedef struct cilqr_config {
  int32_t n_steps;       /* N; knots K = N+1 = floor(horizon/dt + 1)  (cc:22) */
  int32_t num_of_disc;   /* planner_config.h:58 */
  int32_t max_iter;      /* :63 */
  int32_t init_guess;    /* CILQR_INIT_IQR (0): iqr, what the reference runs (cc:169, 793-842); CILQR_INIT_TRACKER (1):
                            InitGuess through the closed-loop Tracker (cc:107-139, tracker.cc), the alternative the
                            reference keeps commented out at cc:168 and recommends in README.md:61-67 */
  double dt;             /* delta_t, :94 */
  double safe_margin;    /* :59 */
  double w_jerk, w_delta_rate, w_x, w_y, w_theta, w_v, w_a, w_delta; /* Weights :45-55 */
  double abs_cost_tol, rel_cost_tol;                                  /* :65-66 */
  double front_hang, wheel_base, rear_hang, width;                    /* vehicle_param.h:26-41 */
  double max_velocity, min_acceleration, max_acceleration;            /* :46-52 */
  double jerk_min, jerk_max, delta_min, delta_max, delta_rate_min, delta_rate_max; /* :57-64 */
  double barrier_t, barrier_eps;                                      /* barrier_function.h:144-145 */
} cilqr_config;

typedef struct cilqr_solver* cilqr_handle;

/* Inputs of IlqrOptimizer::Plan (ilqr_optimizer.h:41-48) for B problems. */
typedef struct cilqr_problem_batch {
  int32_t batch;                 /* B */
  int32_t n_knots;               /* K; must equal n_steps + 1 */
  int32_t cmax;                  /* planes stored per knot in `corridor` (<= create() cmax) */
  int32_t memory;                /* CILQR_MEM_* of start/coarse/corridor/corridor_count */
  const double* start;           /* [B][4]  x, y, theta, velocity  (cc:151) */
  const double* coarse;          /* [B][K][6]  x, y, theta, velocity, a, delta  (cc:148) */
  const double* corridor;        /* [B][K][cmax][3]  a, b, c with "a x + b y < c"  (corridor.h:19-21) */
  const int32_t* corridor_count; /* [B][K]  live planes per knot; negative = no corridor at that knot
                                    (the problem ends with CILQR_ST_NO_CORRIDOR) */
  int32_t n_left, n_right;       /* lane segments, shared by the whole batch */
  const double* left_lane;       /* [n_left][7]  HOST memory */
  const double* right_lane;      /* [n_right][7] HOST memory */
  /* Per-problem lane tables (every Plan call of the reference carries its own lane constraints,
   * ilqr_optimizer.h:41-48).  n_lane_groups = 0 or 1: the one table above serves the whole batch.  Otherwise the
   * problems come grouped by table: group g is problems [lane_group_start[g], lane_group_start[g + 1]) and uses the
   * next lane_group_left[g] rows of left_lane and lane_group_right[g] rows of right_lane (the tables lie back to
   * back; n_left / n_right are then ignored).  The groups are solved one after the other on the handle. */
  int32_t n_lane_groups;
  int32_t reserved1;
  const int32_t* lane_group_start;   /* [n_lane_groups + 1], HOST memory, lane_group_start[0] = 0, last = batch */
  const int32_t* lane_group_left;    /* [n_lane_groups] rows */
  const int32_t* lane_group_right;   /* [n_lane_groups] rows */
  /* CILQR_INIT_TRACKER only: stations of the coarse trajectory's points ([B][K], same memory as `coarse`; TrajectoryPoint::s,
   * which the tracker's projection interpolates along: discretized_trajectory.cpp:165-197).  NULL: the accumulated
   * chord length of the coarse points is used. */
  const double* coarse_station;
} cilqr_problem_batch;

/* Outputs of Plan + cost().  iter_trajs is optional (NULL to skip). */
typedef struct cilqr_solution_batch {
  int32_t memory;                /* CILQR_MEM_* of every pointer below */
  int32_t max_iter_trajs;        /* capacity per problem of iter_trajs */
  double* traj;                  /* [B][K][10] */
  double* cost_hist;             /* [B][max_iter+1][5]; rows >= n_cost[b]: zero (CILQR_MEM_HOST) or left
                                    untouched (CILQR_MEM_DEVICE) */
  int32_t* n_cost;               /* [B] */
  int32_t* status;               /* [B] CILQR_ST_* */
  int32_t* n_iter;               /* [B] iterations started */
  double* iter_trajs;            /* [B][max_iter_trajs][K][10]: init guess + accepted non-final iterates (cc:170,294);
                                    entries >= n_iter_trajs[b] are unspecified */
  int32_t* n_iter_trajs;         /* [B] number that would have been produced (may exceed the capacity) */
  int8_t* alpha_trace;           /* optional (NULL to skip) [B][max_iter]: per iteration of Optimize() the index
                                    into the step-size list (cc:197) that the line search accepted, -1 = all
                                    eleven rejected (cc:296-308), -2 = left before the line search
                                    (gradient-norm exit cc:235-241, or status 6), -3 = iteration not run */
} cilqr_solution_batch;

/* Per-solve kernel timing, filled when profiling is on (cilqr_set_profiling). */
typedef struct cilqr_profile {
  int32_t iterations;            /* outer iterations of the last solve (the slowest problem's count) */
  int32_t backward_launches;
  double backward_ms;            /* sum of HIP-event durations of the backward kernel */
  double quadratize_ms;
  double linesearch_ms;          /* forward + cost + reduce kernels */
  double other_ms;               /* load, init guess, update, export */
  double total_ms;               /* first kernel start -> last kernel end */
  int64_t backward_problem_steps;/* sum over launches of (active problems x N) */
  int32_t backward_full_launches;/* launches whose active set was the whole batch */
  int32_t tail_problems;         /* problems handed to the per-problem tail kernel (upper bound), 0 = not used */
  double backward_full_ms;       /* their summed duration */
  double tail_ms;                /* duration of the tail kernel (not part of the four phase sums above) */
} cilqr_profile;

int cilqr_abi_version(void);
/* first 32 hex digits of the SHA-256 over the library's sources (cilqr_amd/csrc/Makefile): which sources this binary was built from */
const char* cilqr_build_id(void);
int cilqr_default_config(cilqr_config* cfg, int32_t n_steps);

/* device: HIP ordinal.  batch_capacity/cmax/max_lane_segments size the HBM arena once. */
int cilqr_create(const cilqr_config* cfg, int32_t device, int32_t batch_capacity, int32_t cmax,
                 int32_t max_lane_segments, cilqr_handle* out);
/* waits for the solves that were submitted and not collected (cilqr_submit), then frees everything */
int cilqr_destroy(cilqr_handle h);
/* hipStream_t to launch on (NULL = the handle's own stream). */
int cilqr_set_stream(cilqr_handle h, void* hip_stream);
/* Tuning knobs that never change results.  CILQR_OPT_SPEC_THRESHOLD: lockstep iterations with at
 * most this many active problems evaluate all 11 line-search step sizes concurrently instead of
 * round by round (0 disables).  Default: 8192 for cilqr_solve_batch (the shortest solve when the GPU is the caller's
 * alone), 1024 for solves submitted with cilqr_submit / cilqr_pool_submit (eleven candidates where two or three
 * would do is throughput taken from the other solves in flight: +4 % on a pool of two); setting the option sets both. */
#define CILQR_OPT_SPEC_THRESHOLD 1
/* CILQR_OPT_SEQ_ROUNDS (default 4, 1..11): with more active problems than the threshold above, this
 * many step sizes are tried round by round; the problems that rejected all of them evaluate the
 * remaining ones concurrently.  11 = fully sequential. */
#define CILQR_OPT_SEQ_ROUNDS 3
/* CILQR_OPT_COMPACTION (default 1): re-pack the surviving problems into dense slots whenever they
 * fill at most 75 % of the occupied slots, so later iterations keep reading coalesced rows.
 * 0 = never, 2..100 = re-pack at that occupancy percentage. */
#define CILQR_OPT_COMPACTION 2
/* CILQR_OPT_TEAM_THRESHOLD (default 4096): backward passes over at most this many problems spread each
 * problem over eight lanes (column-wise) instead of one, which shortens the chain of dependent
 * steps a small launch waits on; 0 = always one lane per problem.  Bit-identical results. */
#define CILQR_OPT_TEAM_THRESHOLD 4
/* CILQR_OPT_ROUND_GROUP (default 2; 1, 2 or 4): step sizes costed together in one sequential round.  The candidates
 * of a problem sit in neighbouring lanes and share its corridor / goal reads; a round may cost a candidate the
 * sequential loop would not have reached, the first passing index still wins.  Bit-identical results. */
#define CILQR_OPT_ROUND_GROUP 7
/* CILQR_OPT_WAVE_THRESHOLD (default 3072): backward passes over at most this many problems give every problem a
 * whole wavefront (operands in LDS, one output element per lane): the shortest chain of dependent work per step.
 * 0 = never.  Bit-identical results. */
#define CILQR_OPT_WAVE_THRESHOLD 6
/* CILQR_OPT_TAIL_THRESHOLD (default 1024 for cilqr_solve_batch, 128 for solves submitted with cilqr_submit /
 * cilqr_pool_submit -- beside other solves the tail's workgroups take CUs from the neighbours' bulk kernels; setting the
 * option sets both; at most 8192): once at most this many problems are still iterating they
 * leave the lockstep loop; one workgroup per problem runs all its remaining iterations in a single launch
 * (kernels_tail.hip), so the stragglers of a batch no longer cost nine launches per iteration.  0 = lockstep to
 * the end.  Bit-identical results. */
#define CILQR_OPT_TAIL_THRESHOLD 5
/* CILQR_OPT_FINISH_THRESHOLD (default min(batch capacity, 8192), which is also the most): once at most this many
 * problems are still iterating, the survivors move into a small finishing arena of the handle and the main arena is free:
 * with cilqr_submit, the next solve starts there while this one's stragglers finish on a second stream.  0 = never
 * (a submitted solve then runs start to end before the next begins).  Bit-identical results. */
#define CILQR_OPT_FINISH_THRESHOLD 8
/* CILQR_OPT_EXACT_LANE_TIES (default 1; 0 or 1) -- the one option that CAN change results.  FindNeastLaneSegment
 * (ilqr_optimizer.cc:605-618) keeps the first segment whose DistanceTo (line_segment2d.cpp:61-75: hypot to an end
 * point, |cross| to the foot) is strictly smaller.  The kernels compare squared distances, which order the same way
 * except on strips ~1e-7 m wide along the normals through segment end points, where two squares one or two ulp apart
 * have the same root: the reference sees a tie and keeps the earlier segment, a search on squares alone keeps the
 * strictly nearer one.  With 1 (the default: the reference's rule), whenever the two best squared distances are within
 * 1e-13 (relative) of each other the pair is decided by the reference's own distance values (libm-identical hypot)
 * and its strict '<', out of line, after the search loop; candidates that share an end point (the wedge outside every
 * joint) are the same distance in any arithmetic and are not re-examined.  0 = squares only: the opt-in fast rule,
 * 3 % more throughput on a pool of two handles, 6 % on a single solve; the step-replay tests then need the `lane_tie`
 * excuse (tests/parity_util.py). */
#define CILQR_OPT_EXACT_LANE_TIES 9
/* CILQR_OPT_SCENE_CHUNK (default 0): scenes whose obstacle points cilqr_plan_scenes_batch holds at a time.  0 = as many
 * as fit into 1 GiB of points; a positive value = that many (a test hook: a scene's result does not depend on the chunk
 * it falls into).  Bit-identical results. */
#define CILQR_OPT_SCENE_CHUNK 10
/* CILQR_OPT_TAIL_LDS_LIMIT (default 0): dynamic LDS, in bytes, that a tail launch of this handle may plan with.  The tail
 * kernel keeps as many of a problem's 14 tensors in LDS as fit beside its fixed block (lane tables, the backward pass's
 * operands) and leaves the rest in a private arena in global memory; which ones fit depends on the horizon, the plane
 * capacity, the lane tables and on what the device grants a workgroup.  0 = what the device grants; a positive value =
 * min(grant, value) in its place (it never raises anything above the grant, and it does not touch the fixed block: a limit
 * too small for that block and its margin leaves every tensor in the arena).  65536 gives the placement of a device that
 * grants no more than the default 64 KiB.  A test hook, like CILQR_OPT_SCENE_CHUNK: every placement computes the same
 * numbers.  Bit-identical results. */
#define CILQR_OPT_TAIL_LDS_LIMIT 11
/* CILQR_OPT_TAIL_PLAN (read-only: cilqr_set_option returns CILQR_ERR_ARG; cilqr_get_option returns CILQR_ERR_STATE unless
 * cilqr_stage_load has loaded a problem batch): the placement a tail launch takes for the loaded problem under the limit in
 * force, from the function the launch itself calls.  *value:
 *   bits 0..13   the tensor is in LDS: X, U, goals, corridor planes, plane counts, lin, term, gains, Xs, Us, parts,
 *                candidate totals, the scalars, the integers (bit 0 = X ... bit 13 = the integers)
 *   bits 16..20  the phases that address their tensors as LDS: backward pass, the rollouts' loads, the rollouts' stores,
 *                quadratisation, knot costs
 *   bit 21       the quadratisation runs in its split form
 *   bit 24       the tail kernel is available for this problem (its fixed block fits); otherwise solves stay in lockstep
 * *value_submitted: dynamic LDS bytes of the launch. */
#define CILQR_OPT_TAIL_PLAN 12
int cilqr_set_option(cilqr_handle h, int32_t option, int64_t value);
/* the value in force (for the options with two defaults -- CILQR_OPT_SPEC_THRESHOLD, CILQR_OPT_TAIL_THRESHOLD -- the one of
 * cilqr_solve_batch in *value and, if value_submitted is not NULL, the one of submitted solves there) */
int cilqr_get_option(cilqr_handle h, int32_t option, int64_t* value, int64_t* value_submitted);
/* enable = 1: HIP events around every phase of every lockstep iteration (cilqr_profile complete; about 4 %
 * slower: ~800 event records per solve); enable = 2: around the backward launches only (backward_* fields;
 * under 1 %); 0: none. */
int cilqr_set_profiling(cilqr_handle h, int32_t enable);
int cilqr_get_profile(cilqr_handle h, cilqr_profile* out);
/* bytes of device memory held by the handle */
int64_t cilqr_device_bytes(cilqr_handle h);

int cilqr_solve_batch(cilqr_handle h, const cilqr_problem_batch* in, cilqr_solution_batch* out);

/* ---- warm start: the first iterate from control sequences the caller already has ----
 * Every solve above starts from the handle's configured init guess, built from the coarse trajectory alone.  The batches
 * of a stream are rarely unrelated (the same scenes with new obstacle predictions, variants of one scene around a nominal
 * solution), and the previous solution lies in device memory in the layout of cilqr_solution_batch::traj.  A warm start
 * hands its controls to the solver.  For problem b with s = shift[b] (a NULL shift array: 0 for every problem):
 *   s <  0   the problem is not warm-started: it takes the handle's configured init guess, and all its outputs are
 *            bit-identical to the same batch solved without a warm start;
 *   s >= 0   for every step i < N, with r = i + s:  U_i = the two control columns of row r of the problem's warm rows if
 *            r < N (the bits are copied: not clamped, not angle-wrapped), U_i = (0, 0) otherwise (s >= N is compared
 *            before anything is added: s = 2^31 - 1 is valid and gives all zeros);
 *            X_0 = goals_[0] = (start.x, start.y, start.theta, start.v, 0, 0), X_{i+1} = Dynamics(X_i, U_i) with the
 *            arithmetic of cilqr_open_loop_rollout, bit for bit.
 * From there Optimize() runs unchanged: iter_trajs[0] is this pair and cost row 0 its TotalCost.  Knot 0 stays goals_[0]
 * with a = delta = 0, because Forward restarts every rollout there (cc:392-415); `shift` only spares a caller who has
 * advanced the problems in time the repacking of the controls.  Non-finite warm rows are no error: the arithmetic decides,
 * and every other problem of the batch is unaffected.  Any shift value is valid.
 *   layout   CILQR_ROWS_TRAJ      rows [B][K][CILQR_TRAJ_FIELDS], controls in columns 8 and 9
 *            CILQR_ROWS_PLAN      rows [B][K][CILQR_PLAN_FIELDS], controls in columns 9 and 10
 *            CILQR_ROWS_CONTROLS  rows [B][N][2]
 * (K rows per problem are addressed, the first N are read; no alignment beyond that of a double is assumed.)
 * With warm == NULL every call below is exactly its plain counterpart.  Checked before anything is launched, the handle
 * staying usable: CILQR_ERR_NULL for NULL rows; CILQR_ERR_ARG for an unknown layout or CILQR_ROWS_COARSE (which carries
 * no controls), and for a `memory` that is not a CILQR_MEM_* value or differs from in->memory.  The arrays of a submitted
 * solve must stay valid until its wait, like the other inputs.  cilqr_stage_load_warm arms cilqr_stage_init_guess, which then
 * produces this first iterate (readable as CILQR_T_X / CILQR_T_U). */
#define CILQR_ROWS_CONTROLS 3   /* [N][2] jerk, delta_rate (beside CILQR_ROWS_TRAJ / _PLAN / _COARSE below) */
typedef struct cilqr_warm_start {
  int32_t memory;        /* CILQR_MEM_*; must equal in->memory */
  int32_t layout;        /* CILQR_ROWS_TRAJ, CILQR_ROWS_PLAN or CILQR_ROWS_CONTROLS */
  const double*  rows;   /* [B][K][10] | [B][K][11] | [B][N][2] */
  const int32_t* shift;  /* [B], optional (NULL: 0 for all); < 0: cold */
} cilqr_warm_start;
int cilqr_solve_batch_warm(cilqr_handle h, const cilqr_problem_batch* in, const cilqr_warm_start* warm,
                           cilqr_solution_batch* out);

/* TrackerConfig / LateralTrackerConfig / LongitudinalTrackerConfig (algorithm/params/planner_config.h:18-43) for
 * CILQR_INIT_TRACKER; cilqr_create starts from the reference's defaults. */
typedef struct cilqr_tracker_config {
  double weight_l, weight_theta, weight_delta, weight_delta_rate, preview_time;   /* lateral  :18-25 */
  double weight_s, weight_v, weight_a, weight_j;                                  /* longitudinal :27-34 */
  double sumulation_dt, dt, tolerance;                                            /* :37-39 */
  int32_t max_num_iteration;                                                      /* :40 */
  int32_t reserved0;
} cilqr_tracker_config;
/* Limits of one tracker launch (every problem runs n_steps * dt / sumulation_dt simulation steps, each with a DARE loop of up
 * to max_num_iteration rounds; the reference's defaults are 150 iterations and 10 steps per knot). */
#define CILQR_TRACKER_MAX_ITERATIONS 1000  /* largest max_num_iteration */
#define CILQR_TRACKER_MAX_SIM_STEPS 32768  /* largest n_steps * dt / sumulation_dt (n_steps, dt of cilqr_create); also the
                                              most simulation rounds of one "track" call below, whatever its time column */
void cilqr_default_tracker_config(cilqr_tracker_config* cfg);
/* CILQR_ERR_NULL: null handle.  CILQR_ERR_ARG, the handle keeping the configuration it had: a null config; a field that is
 * not finite; sumulation_dt <= 0, dt <= 0, tolerance < 0; max_num_iteration outside 1 ... CILQR_TRACKER_MAX_ITERATIONS; more
 * than CILQR_TRACKER_MAX_SIM_STEPS simulation steps over the handle's horizon; a sumulation_dt whose clock
 * (t = 0, sumulation_dt, 2 sumulation_dt, ... summed in doubles, tracker.cc:186-203) does not pass every knot time i * dt
 * up to the last -- where the reference's tracker gives up ("tacker failed", cc:205-208): e.g. 0.03 or 0.25 for n_steps = 50,
 * dt = 0.1.  The stations a load brought (cilqr_problem_batch.coarse_station) are not touched. */
int cilqr_set_tracker_config(cilqr_handle h, const cilqr_tracker_config* cfg);

/* Asynchronous form of cilqr_solve_batch: submit returns at once (the structs are copied, the
 * arrays they point to -- inputs and outputs -- must stay valid and distinct per solve until its wait),
 * wait blocks for the result code of the OLDEST submitted solve.  A handle accepts up to THREE solves before the
 * oldest is collected (a fourth submit returns CILQR_ERR_STATE): TWO are in flight -- the handle iterates the bulk of
 * solve i+1 in its main arena while the last few thousand problems of solve i (the latency-bound part of a solve: lockstep
 * iterations over few problems, then the per-problem tail kernel) finish in a small second arena on a second stream
 * (CILQR_OPT_FINISH_THRESHOLD) -- and the third is queued behind them.  Keep the handle fed:
 *     submit(A); submit(B); submit(C); wait(); submit(D); wait(); submit(E); ...
 * Host arrays (CILQR_MEM_HOST) of more than 4 MB take a path of their own on a submitted solve: the inputs of the queued
 * solve are uploaded on a separate stream while the solve in front of it iterates (which is what the third place is for:
 * an upload is as long as most of a solve); the results come back on another one -- trajectories straight into the caller's
 * array, the LIVE Cost rows packed (24 MB instead of the dense 527 MB on the bench workload) and scattered into the
 * caller's dense cost_hist on the host, whose other rows the library clears.  Pinned or pageable memory alike (57 / 51 GB/s
 * measured); from the moment of the submit until the wait returns the library reads the inputs and writes the outputs.
 * Results are bit-identical to cilqr_solve_batch.  cilqr_get_profile reports the solve the last wait
 * collected.  A handle is not re-entrant: between a submit and the wait that collects it, call only
 * cilqr_submit / cilqr_wait on it (cilqr_solve_batch and cilqr_stage_load return CILQR_ERR_STATE). */
int cilqr_submit(cilqr_handle h, const cilqr_problem_batch* in, cilqr_solution_batch* out);
int cilqr_wait(cilqr_handle h);

/* cilqr_submit with a warm start (see cilqr_solve_batch_warm) */
int cilqr_submit_warm(cilqr_handle h, const cilqr_problem_batch* in, const cilqr_warm_start* warm, cilqr_solution_batch* out);

/* ---- stage entry points (operate on the handle's device state, whole batch) ----
 * A cilqr_solve_batch / cilqr_submit on the same handle invalidates the staged state: call
 * cilqr_stage_load again afterwards (CILQR_ERR_STATE otherwise). */
int cilqr_stage_load(cilqr_handle h, const cilqr_problem_batch* in);
/* the load of a warm-started solve: the cilqr_stage_init_guess that follows produces the warm first iterate */
int cilqr_stage_load_warm(cilqr_handle h, const cilqr_problem_batch* in, const cilqr_warm_start* warm);
int cilqr_stage_init_guess(cilqr_handle h);
/* overwrite the current iterate: X [B][K][6], U [B][N][2] */
int cilqr_stage_set_trajectory(cilqr_handle h, const double* X, const double* U, int32_t memory);
/* cost of the current iterate: cost5 [B][5] */
int cilqr_stage_total_cost(cilqr_handle h, double* cost5, int32_t memory);
int cilqr_stage_quadratize(cilqr_handle h);
/* lambda: [B] regularisation per problem, or NULL to use the solver state */
int cilqr_stage_backward(cilqr_handle h, const double* lambda, int32_t memory);
/* roll out with step alpha into the candidate buffers */
int cilqr_stage_forward(cilqr_handle h, double alpha);

/* tensors readable with cilqr_stage_read, all returned problem-major fp64 */
#define CILQR_T_GOALS 0      /* [B][K][6] */
#define CILQR_T_CORRIDOR 1   /* [B][K][cmax][3] shrunk + normalised (create() cmax) */
#define CILQR_T_LANES 2      /* [n_left+n_right][3] shrunk + normalised a,b,c (left rows first) */
#define CILQR_T_X 3          /* [B][K][6] current iterate */
#define CILQR_T_U 4          /* [B][N][2] */
#define CILQR_T_XCAND 5      /* [B][K][6] candidate of the last forward */
#define CILQR_T_UCAND 6      /* [B][N][2] */
#define CILQR_T_A 7          /* [B][N][6][6] */
#define CILQR_T_B 8          /* [B][N][6][2] */
#define CILQR_T_LX 9         /* [B][K][6] */
#define CILQR_T_LU 10        /* [B][N][2] */
#define CILQR_T_LXX 11       /* [B][K][6][6] */
#define CILQR_T_LUU 12       /* [B][N][2][2] */
#define CILQR_T_KFB 13       /* [B][N][2][6] feedback gains K */
#define CILQR_T_KFF 14       /* [B][N][2] feedforward k */
#define CILQR_T_DV 15        /* [B][2] delta_V_ */
#define CILQR_T_GNORM 16     /* [B] */
int cilqr_stage_read(cilqr_handle h, int32_t tensor, double* dst, int32_t memory);

/* ---- test door: the search state a solve starts with (no product path calls this) ----
 * Optimize() begins with cost_old = TotalCost(first iterate), lambda = dlambda = 1 and iteration 0 (cc:172, 180-186), so which
 * step size a solve accepts, which clause rejects the others and which exit it takes cannot be chosen from outside.  A seed
 * overwrites those four per-problem values of the NEXT solve on the handle (cilqr_solve_batch[_warm], or the next cilqr_submit
 * to begin), right after the first iterate's cost was committed; everything after that is the ordinary solve -- every line-search
 * schedule, compaction, the finishing arena, the tail kernel.  The first iterate itself is chosen with a warm start, shift 0.
 *   cost_old, lambda, dlambda  [batch] doubles, each may be NULL (that value keeps its start).  ANY bits are taken, non-finite
 *                              ones included: they are test cases.
 *   iter                       [batch], NULL or values in [0, max_iter): the iteration count the problem starts at, so that
 *                              iter = max_iter - n gives a solve of at most n iterations.  n_iter counts from it; alpha_trace
 *                              entries below it read -3 (not run).
 * Row 0 of cost_hist stays the TRUE cost of the first iterate, whatever cost_old was seeded; n_cost / n_iter_trajs start at 1.
 * The arrays are copied by the call (device arrays with a synchronous copy).  The seed is consumed by the solve that takes it,
 * whose batch must equal `batch` (CILQR_ERR_ARG from that solve otherwise).  A seed is for batches with one lane table: a batch with several lane groups is
 * refused while a seed is armed (CILQR_ERR_ARG, the seed disarmed).
 * seed == NULL disarms.  CILQR_ERR_NULL for a NULL handle; CILQR_ERR_ARG for batch < 1 or above the handle's capacity, an
 * unknown memory flag, an iter outside [0, max_iter); CILQR_ERR_STATE while solves are submitted on the handle. */
typedef struct cilqr_search_seed {
  int32_t memory;          /* CILQR_MEM_* of the four arrays */
  int32_t batch;
  const double*  cost_old; /* [batch] or NULL */
  const double*  lambda;   /* [batch] or NULL */
  const double*  dlambda;  /* [batch] or NULL */
  const int32_t* iter;     /* [batch] or NULL */
} cilqr_search_seed;
int cilqr_set_search_seed(cilqr_handle h, const cilqr_search_seed* seed);

/* FindNeastLaneSegment (cc:605-618) for n arbitrary points xy[n][2]: index of the nearest left /
 * right lane segment.  use_grid = 1: the accelerated lookup the solver uses; 0: the reference's
 * linear scan.  Both must agree everywhere (test hook). */
int cilqr_stage_nearest_lane(cilqr_handle h, int32_t n, const double* xy, int32_t* left, int32_t* right,
                             int32_t use_grid, int32_t memory);

/* ---- test hooks (no product path calls these) ----
 * cilqr_comm_create_loopback: a communicator for cilqr_gather_results whose `world` ranks are handles of ONE process on
 * ONE device, so that the paths of the gather that need more than one rank run on a machine with one GPU (RCCL refuses
 * two ranks on one device).  Handles that name the same `group` (any number; process-wide) form the communicator; every
 * rank is driven by a thread of its own.  The exchange is host-synchronous: a sender completes its stream and publishes
 * its buffer, the receiver copies it device-to-device on its own stream and completes that -- no stream waits for
 * another, so the order of work between streams that RCCL relies on is NOT exercised.  Every wait for a peer ends after
 * `timeout_ms` with CILQR_ERR_DEVICE; a send and a receive whose counts differ fail on both sides at once, also with
 * CILQR_ERR_DEVICE.  CILQR_ERR_ARG when the rank is taken or the group exists with another world.  Destroyed with
 * cilqr_comm_destroy, like any communicator. */
int cilqr_comm_create_loopback(cilqr_handle h, uint64_t group, int32_t rank, int32_t world, int32_t timeout_ms);

/* ---- corridor producer: the inputs of cilqr_problem_batch from obstacle points ---- */

/* CorridorConfig, algorithm/params/planner_config.h:75-86 */
typedef struct cilqr_corridor_config {
  double max_diff_x, max_diff_y;   /* obstacle points farther than this from the knot are ignored */
  double radius;                   /* sphere-flip radius */
  double max_axis_x, max_axis_y;   /* half extents of the box added around every knot */
  double lane_segment_length;      /* LaneBoundarySample spacing */
  int32_t is_multiple_sample;      /* 0: both ends of every box edge (8 points); 1: six samples per box edge (24
                                      points, corridor.cc:110-118) -- the caller then passes the obstacles' sample
                                      points (Polygon2d::sample_points, polygon2d.cpp:259-271) instead of their corners */
  int32_t reserved0;
} cilqr_corridor_config;
void cilqr_default_corridor_config(cilqr_corridor_config* cfg);

/* Corridor::BuildCorridorConstraints (algorithm/ilqr/corridor.cc:58-87) for `batch` trajectories of
 * `n_knots` knots: per knot AddCorridorPoints (cc:89-120) + BuildCorridor (cc:122-263), with
 * cv::convexHull replaced by an own float32 hull (see kernels_corridor.hip).
 *   knots          [batch][n_knots][3]              x, y, theta of the coarse trajectory point
 *   points         [batch][n_knots][max_points][2]  obstacle corner points valid at the knot's time
 *                                                   (Environment::Query{Static,Dynamic}ObstaclesPoints)
 *   point_count    [batch][n_knots]
 *   corridor       [batch][n_knots][cmax][3]        out: a, b, c with a x + b y <= c -- the layout of
 *   corridor_count [batch][n_knots]                 cilqr_problem_batch::corridor / corridor_count
 * A knot whose corridor cannot be built gets a negative count (-2: fewer than 4 usable points,
 * -3: more than cmax half-planes, -4: degenerate hull) and is counted in *n_failed; the reference
 * fails the whole Plan in that case (cc:78-81).  max_points + 8 (24 with is_multiple_sample) <= 320.  `memory`
 * applies to all arrays.
 *   polygons       [batch][n_knots][cmax][2]        optional out (NULL to skip): the vertices of each
 *                                                   corridor polygon (`convex_polygons`, cc:244-249),
 *                                                   vertex i being the start of half-plane i */
int cilqr_build_corridors(cilqr_handle h, const cilqr_corridor_config* cfg, int32_t batch, int32_t n_knots,
                          const double* knots, const double* points, const int32_t* point_count,
                          int32_t max_points, double* corridor, int32_t* corridor_count, int32_t cmax,
                          int32_t memory, int32_t* n_failed, double* polygons);

/* LaneBoundarySample (corridor.cc:298-311) + CalLeftLaneConstraints / CalRightLaneConstraints
 * (cc:265-296) + HalfPlaneConstraint (cc:313-321), host only: boundary [n][2] -> rows [.][7] in the
 * layout of cilqr_problem_batch::left_lane / right_lane.  Returns the number of rows (>= 1) or a
 * negative error code. */
int cilqr_lane_constraints(const double* boundary, int32_t n, double segment_length, int32_t is_left,
                           double* rows, int32_t max_rows);

/* Test hook for the kernels' own fp64 routines (host arrays of n doubles):
 * fn 0: log(x) for normal finite x > 0;  fn 1: 1 / x for normal finite x != 0;
 * fn 2: log(x) with mantissa and exponent handed over separately (the long-product path);
 * fn 3 / 4 / 5: sin / cos / tan(x) for |x| <= 1e5;  fn 6: NormalizeAngle(x) (math_utils.cpp:53-59);
 * fn 7 / 8: the device library's cos / sin as the corridor producer uses them for the box corners (corridor.cc:96-99);
 * fn 9: hypot(x, 1) by the libm-identical routine of the lane search and the constraint normalisation;
 * fn 10: NormalizeAngle(x) as the rollouts evaluate it (short paths as one straight line; the complete function for the
 *        wavefront when a lane's argument lies outside (-3 pi, 3 pi)) -- the same bits as fn 6 on every input. */
int cilqr_device_math(cilqr_handle h, int32_t fn, int32_t n, const double* in, double* out);

/* X[b][0] = x0[b]; X[b][i+1] = Dynamics(X[b][i], U[b][i]).  x0 [B][6], U [B][N][2], X [B][K][6] */
int cilqr_open_loop_rollout(cilqr_handle h, int32_t batch, const double* x0, const double* U,
                            double* X, int32_t memory);

/* ---- coarse trajectory: the producer of `coarse` / `start`; one scene on the host ----
 * DpPlanner::Plan (algorithm/planner/dp_planner.cpp:135-281): 5 x 7 x 10 (time, station, lateral) sampling DP in
 * the Frenet frame of the centre line with collision checks against the scene, then ComputePathProfile
 * (algorithm/utils/discrete_points_math.cc:27-176).  C++ callers use include/cilqr/dp_planner.hpp directly;
 * include/cilqr/trajectory_planner.hpp chains it with the corridor producer and the solve
 * (TrajectoryPlanner::Plan, algorithm/planner/trajectory_planner.cpp:28-162). */
#define CILQR_COARSE_FIELDS 9   /* time, s, x, y, theta, kappa, velocity, a, delta */
typedef struct cilqr_dp_config {   /* PlannerConfig planner_config.h:94-133 + VehicleParam vehicle_param.h:26-46 */
  double tf, delta_t;
  double dp_nominal_velocity, dp_w_obstacle, dp_w_lateral, dp_w_lateral_change, dp_w_lateral_velocity_change;
  double dp_w_longitudinal_velocity_bias, dp_w_longitudinal_velocity_change;
  double front_hang_length, wheel_base, rear_hang_length, width, max_velocity;
} cilqr_dp_config;
void cilqr_default_dp_config(cilqr_dp_config* cfg);
/* A scene in the vocabulary of the reference's messages (the files under msg/), flattened; HOST memory. */
typedef struct cilqr_scene {
  const double* center;                 /* [n_center][7]  CenterLinePoint: s x y theta kappa left_bound right_bound */
  int32_t n_center;
  int32_t n_static;
  const double* static_points;          /* [sum static_counts][2]  world-frame polygons, back to back (Obstacles.msg) */
  const int32_t* static_counts;         /* [n_static] */
  int32_t n_dynamic;
  int32_t reserved0;
  const double* dynamic_polygon_points;     /* [sum dynamic_polygon_counts][2]  body-frame polygons (DynamicObstacle.msg) */
  const int32_t* dynamic_polygon_counts;    /* [n_dynamic] */
  const double* dynamic_trajectories;       /* [sum dynamic_trajectory_counts][4]  time x y theta (DynamicTrajectoryPoint.msg) */
  const int32_t* dynamic_trajectory_counts; /* [n_dynamic] */
} cilqr_scene;
/* Environment::set_reference (algorithm/utils/environment.cpp:20-43), host only: the left / right road barriers -- the
 * centre line evaluated every 0.1 m of station and shifted by +left_bound / -right_bound along its normal -- that
 * Corridor::Plan samples its lane constraints from (corridor.cc:43-51; the `boundary` input of
 * cilqr_lane_constraints).  left / right [max_points][2]; returns the number of points or a negative error code. */
int cilqr_road_barriers(const double* center, int32_t n_center, double* left, double* right, int32_t max_points);
/* start3 = x, y, theta (dp_planner.cpp:135-141); coarse [n_knots][CILQR_COARSE_FIELDS], n_knots = tf / delta_t + 1.
 * Returns CILQR_OK, or CILQR_ERR_NO_PATH when every sampled path collides (coarse is filled all the same, as in
 * the reference, whose caller then stops: trajectory_planner.cpp:32-35). */
int cilqr_dp_plan(const cilqr_dp_config* cfg, const cilqr_scene* scene, const double* start3, double* coarse,
                  int32_t n_knots);

/* ---- which knots of a trajectory touch the scene: Environment::CheckOptimizationCollision(time, pose, collision_buffer)
 * (algorithm/utils/environment.cpp:92-111) for every knot; one scene on the host ----
 * The solver's constraints are barriers on a corridor: a trajectory it returns, converged or not, can still cut a polygon
 * or a road barrier.  This is the reference's own test for that, asked about every row of a trajectory.  Per knot, with
 * h = radius + collision_buffer and radius / the disc offsets derived from cfg as for the DP planner
 * (vehicle_param.h:76-95): the two vehicle discs, centres x + offset cos(theta), y + offset sin(theta), as axis-aligned
 * squares of half side h against
 *   - the static polygons (Polygon2d::HasOverlap(Box2d), polygon2d.cpp:150-164; Box2d::IsPointIn with its 1e-10);
 *   - the x-sorted road barrier points between two upper_bounds on x, plus the one predecessor (environment.cpp:54-80);
 *   - the dynamic polygons at the knot's time t.  An obstacle is absent when its vertex or sample count is < 1, when
 *     time[0] > t or when time[T-1] < t (no epsilon, cpp:117 -- not the rule of the Query...Points calls); otherwise its
 *     pose is the first sample with t < time[k], past the end the last one (the reference dereferences end() there),
 *     placed in Pose::transform order and boxed as Polygon2d::BuildFromPoints does.  Sample times are taken as
 *     non-decreasing.
 * All six tests are made, none is short-circuited; mask[k] != 0 is exactly the reference's bool.  Rear / front are the
 * geometric discs (offsets length / 4 - rear_hang and 3 length / 4 - rear_hang), not the reference's swapped variable
 * names.  Non-finite poses are no error: the arithmetic decides (in practice every comparison is false).
 * Only time, x, y and theta are read from a row: */
#define CILQR_ROWS_TRAJ 0     /* [K][CILQR_TRAJ_FIELDS]    time 0, x 1, y 2, theta 3 */
#define CILQR_ROWS_PLAN 1     /* [K][CILQR_PLAN_FIELDS]    time 0, x 2, y 3, theta 4 */
#define CILQR_ROWS_COARSE 2   /* [K][CILQR_COARSE_FIELDS]  time 0, x 2, y 3, theta 4 */
/* (every column of every CILQR_ROWS_* layout is stated once for the code: include/cilqr/row_layouts.hpp) */
#define CILQR_HIT_REAR_STATIC 1     /* mask bits: the rear disc against a static polygon, */
#define CILQR_HIT_REAR_BARRIER 2    /*            a road barrier point,                   */
#define CILQR_HIT_REAR_DYNAMIC 4    /*            a dynamic polygon;                      */
#define CILQR_HIT_FRONT_STATIC 8    /* the front disc likewise */
#define CILQR_HIT_FRONT_BARRIER 16
#define CILQR_HIT_FRONT_DYNAMIC 32
/* mask [n_knots] and n_hit are optional (NULL to skip); *first_hit = the first knot with a non-zero mask, -1 if there is
 * none; *n_hit = how many knots have one.  A static or dynamic slot with 0 vertices is unused.  CILQR_ERR_NULL;
 * CILQR_ERR_ARG for an unknown layout, n_knots < 1, a negative or non-finite collision_buffer, n_center < 2, a negative
 * count; CILQR_ERR_CAPACITY beyond the CILQR_DP_MAX_* limits below (the batched call accepts exactly the same scenes). */
int cilqr_check_collisions(const cilqr_dp_config* cfg, const cilqr_scene* scene, int32_t layout, const double* rows,
                           int32_t n_knots, double collision_buffer, uint8_t* mask, int32_t* first_hit, int32_t* n_hit);

/* ---- the same planner for B scenes per call, on the GPU (ABI 7) ----
 * One road (centre line) for the whole batch, as the lane tables of cilqr_problem_batch are; per scene a fixed number of
 * obstacle slots, every polygon stored with max_vertices vertices and every trajectory with max_samples samples
 * (cilqr_amd.scene_io.pack_scene_batch pads a list of scenes into this form).  A slot whose vertex count is 0 is unused.
 * Limits of the kernel's fixed-size storage (CILQR_ERR_CAPACITY beyond them): */
#define CILQR_DP_MAX_VERTICES 8      /* vertices per polygon */
#define CILQR_DP_MAX_STATIC 32       /* static obstacle slots per scene */
#define CILQR_DP_MAX_DYNAMIC 32      /* dynamic obstacle slots per scene */
#define CILQR_DP_MAX_SAMPLES 1024    /* trajectory samples per dynamic obstacle */
#define CILQR_DP_MAX_KNOTS 256       /* n_knots, and the path samples of the five layers together */
typedef struct cilqr_scene_batch {
  int32_t batch, memory;            /* CILQR_MEM_* of every per-problem array below */
  const double* center;             /* [n_center][7], HOST memory, ONE centre line for the batch */
  int32_t n_center;
  int32_t max_static, max_dynamic;  /* obstacle slots per scene (0: none, the arrays of that kind may be NULL) */
  int32_t max_vertices;             /* vertices stored per polygon */
  int32_t max_samples;              /* trajectory samples stored per dynamic obstacle */
  int32_t reserved0;
  const double*  static_points;     /* [B][max_static][max_vertices][2] world frame */
  const int32_t* static_counts;     /* [B][max_static] vertices; 0 = slot unused */
  const double*  dynamic_polygon_points;    /* [B][max_dynamic][max_vertices][2] body frame */
  const int32_t* dynamic_polygon_counts;    /* [B][max_dynamic]; 0 = slot unused */
  const double*  dynamic_trajectories;      /* [B][max_dynamic][max_samples][4] time x y theta */
  const int32_t* dynamic_trajectory_counts; /* [B][max_dynamic]; 0 samples: the obstacle is never there (as in cilqr_dp_plan) */
} cilqr_scene_batch;
/* cilqr_dp_plan for every scene of the batch, one workgroup per scene (kernels_dp.hip).  Per scene the semantics are
 * those of cilqr_dp_plan: the trajectory is filled whether or not a collision-free path exists (found[b] = 0 is its
 * CILQR_ERR_NO_PATH), a plan that stands still for a layer carries the same 0 / 0 = NaN curvature.  The lattice path,
 * every cost, the station and the time column are the host planner's bit for bit; x, y, the headings and what is
 * differenced from them go through the device's sin / cos / atan and agree to rounding.
 *   start3  [B][3] x y theta                         (memory as scenes->memory, like every array below)
 *   coarse9 [B][K][CILQR_COARSE_FIELDS]              optional (NULL to skip)
 *   coarse6 [B][K][6] x y theta velocity a delta     optional: cilqr_problem_batch::coarse
 *   knots3  [B][K][3] x y theta                      optional: the `knots` input of cilqr_build_corridors
 *   station [B][K]                                   optional: cilqr_problem_batch::coarse_station
 *   found   [B] 1 / 0;  *n_not_found (HOST, optional): how many are 0
 * Runs on the handle's stream and waits for that stream only (the count has to come back); its work space belongs to
 * the handle and grows to the largest call, nothing is allocated in steady state.  CILQR_ERR_STATE while solves are
 * submitted on the handle.  Checked before anything is launched: CILQR_ERR_NULL; CILQR_ERR_ARG for batch < 1,
 * n_center < 2, non-positive tf / delta_t, negative sizes, max_vertices < 1 with slots to fill and -- HOST arrays -- a
 * count that is negative or above its max_*; CILQR_ERR_KNOTS; CILQR_ERR_CAPACITY beyond the limits above.  With DEVICE arrays
 * the counts are checked in the kernel: such a scene is reported as not found, its rows are zero, the others are
 * unaffected.  Non-finite coordinates are no error: the arithmetic is the host planner's, the result deterministic. */
int cilqr_dp_plan_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                        const double* start3, int32_t n_knots, double* coarse9, double* coarse6, double* knots3,
                        double* station, int32_t* found, int32_t* n_not_found);

/* ---- obstacle points per knot for B scenes, on the GPU ----
 * What Corridor::BuildCorridorConstraints asks the Environment for once per knot (environment.cpp:133-182), for every
 * scene of a batch and every knot time of ONE time axis: the `points` / `point_count` inputs of cilqr_build_corridors,
 * in exactly that layout.  Per knot: the static polygons in slot order (slots with a count > 0; vertices copied bit for
 * bit), then the dynamic obstacles present at the knot's time t, in slot order.  An obstacle with T samples and m
 * vertices is absent when m < 1, T < 1, time[0] > t + 1e-10 or time[T-1] < t - 1e-10; otherwise its pose is sample k =
 * the first with t < time[k] + 1e-10 (std::upper_bound; past the end: the last) and its vertices are
 * x + rx c - ry s, y + rx s + ry c in that order, c / s the device library's cos / sin of the sample's heading
 * (cilqr_device_math fn 7 / 8).  is_multiple_sample = 1: every polygon contributes Polygon2d::sample_points
 * (polygon2d.cpp:259-271) instead of its corners -- reversed first if its signed area is negative, then six points per
 * edge at the accumulated ratios 0, 0.2, ..., each p (1 - ratio) + q ratio.
 *   knot_times  [n_knots], HOST memory
 *   points      [B][n_knots][max_points][2]   live points packed at the front of a knot's row; the rest of the row is
 *                                             left untouched (memory as scenes->memory, like the two arrays below)
 *   point_count [B][n_knots]
 *   scene_ok    [B] 1 / 0, optional (NULL to skip)
 * Checked before anything is launched: CILQR_ERR_NULL; CILQR_ERR_ARG for a bad batch, sizes or memory flag, HOST counts
 * that are negative or above their max_*, n_knots < 1 and max_points < (max_static + max_dynamic) * max_vertices * (6
 * with is_multiple_sample, else 1); CILQR_ERR_CAPACITY beyond the CILQR_DP_MAX_* limits; CILQR_ERR_STATE while solves
 * are submitted on the handle.  With DEVICE arrays the counts are checked in the kernel: such a scene gets point_count 0
 * at every knot and scene_ok 0, the others are unaffected.  Runs on the handle's stream and waits for that stream only;
 * its work space belongs to the handle and grows to the largest call. */
int cilqr_scene_points_batch(cilqr_handle h, const cilqr_scene_batch* scenes, int32_t n_knots, const double* knot_times,
                             int32_t is_multiple_sample, int32_t max_points, double* points, int32_t* point_count,
                             int32_t* scene_ok);

/* ---- cilqr_check_collisions for B scenes per call, on the GPU (kernels_collision.hip) ----
 * The audit behind cilqr_plan_scenes_batch: its `plan` rows (CILQR_ROWS_PLAN), the solver's traj (CILQR_ROWS_TRAJ) or
 * the DP planner's coarse9 (CILQR_ROWS_COARSE) against the scenes they were planned in, without leaving the device.  One
 * workgroup per scene; per knot the semantics are those of the host call above and the arithmetic is the DP kernels':
 * the vehicle heading goes through their sin / cos, the obstacle placement through the device library's cos / sin
 * (cilqr_device_math fn 7 / 8), so a verdict can differ from the host's only where a point lies within rounding of a
 * square's side or a polygon's edge.
 *   rows      [B][n_knots][fields of the layout]   (memory as scenes->memory, like the three arrays below)
 *   mask      [B][n_knots] CILQR_HIT_* bits, optional (NULL to skip)
 *   first_hit [B]  the first knot with a non-zero mask, -1: none
 *   n_hit     [B]  knots with a non-zero mask, optional
 *   *n_colliding (HOST, optional): the scenes with first_hit >= 0
 * Checked before anything is launched: CILQR_ERR_NULL; CILQR_ERR_ARG for a bad batch, sizes, layout or memory flag,
 * n_knots < 1, a negative or non-finite collision_buffer, n_center < 2 and HOST counts that are negative or above their
 * max_*; CILQR_ERR_CAPACITY beyond the CILQR_DP_MAX_* limits (n_knots included); CILQR_ERR_STATE while solves are submitted
 * on the handle.  With DEVICE arrays the counts are checked in the kernel: such a scene gets first_hit -2, n_hit 0 and a
 * zero mask row, the others are unaffected.  Runs on the handle's stream and waits for that stream only; DEVICE arrays
 * need no work space beyond the barrier table, HOST arrays are staged in blocks that belong to the handle and grow to
 * the largest call. */
int cilqr_check_collisions_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                                 int32_t layout, const double* rows, int32_t n_knots, double collision_buffer,
                                 uint8_t* mask, int32_t* first_hit, int32_t* n_hit, int32_t* n_colliding);

/* ---- resample: trajectory rows on another time or station axis (DiscretizedTrajectory::EvaluateTime / EvaluateStation,
 * algorithm/utils/discretized_trajectory.cpp:50-136; math::slerp, math_utils.h:208-225); one trajectory on the host ----
 * What the solver and the planners return are knot rows, delta_t apart; the reference's consumers read its result through
 * these two queries.  One trajectory is K >= 2 rows in one of the CILQR_ROWS_TRAJ / _PLAN / _COARSE layouts; `key` is its
 * time column (CILQR_KEY_TIME) or its station column (CILQR_KEY_STATION: _PLAN and _COARSE only, _TRAJ has none).  Keys are
 * taken as non-decreasing.  For a query q:
 *   bracket   (QueryLowerBound{Time,Station}Point, then Evaluate*)  if q >= key[K-1]: i = K-1; else if q < key[0]: i = 0;
 *             else i = std::lower_bound's halving written out,
 *                 first = 0, len = K;  while (len > 0) { half = len >> 1;
 *                     if (key[first + half] < q) { first += half + 1; len -= half + 1; } else len = half; }   i = first
 *             -- defined for any input, sorted or not.  If i == 0, i = 1.  p0 = row i-1, p1 = row i.  Outside the key
 *             range this extrapolates, as the reference does; a NaN query ends at i = 1 and the arithmetic decides.
 *   degenerate pair   |key1 - key0| < 1e-10 (strict; kMathEpsilon): the output row is p0 copied as bits, its key column
 *             included.
 *   otherwise w = (q - key0) / (key1 - key0), every operation rounded once (no fused multiply-add), and
 *             the key column      q itself;
 *             theta               slerp(p0.theta, key0, p1.theta, key1, q) with the reference's NormalizeAngle (slerp's own
 *                                 `<=` against 1e-10 stays as written);
 *             jerk, delta_rate    (where the layout has them) p0's bits: a control holds over its step;
 *             every other column  (1 - w) * p0 + w * p1 -- a and delta included, which the reference leaves at their
 *                                 default 0 and which are linear over a step in this model.
 * The output row has the layout of the input rows.  Non-finite rows and queries are no error: the arithmetic decides (a
 * result that is a NaN is a NaN in either call; which NaN is not part of the rule), the other queries are unaffected.
 *   rows [n_knots][fields], queries [n_queries], out [n_queries][fields]; HOST memory; no handle
 * CILQR_ERR_NULL; CILQR_ERR_ARG for n_knots < 2, n_queries < 1, an unknown layout or key, CILQR_KEY_STATION with
 * CILQR_ROWS_TRAJ, out == rows; CILQR_ERR_CAPACITY for n_knots > CILQR_DP_MAX_KNOTS.  C++ callers use
 * include/cilqr/trajectory_queries.hpp directly. */
#define CILQR_KEY_TIME 0
#define CILQR_KEY_STATION 1
int cilqr_resample_rows(int32_t layout, const double* rows, int32_t n_knots, int32_t key,
                        const double* queries, int32_t n_queries, double* out);
/* ---- the same for B trajectories per call, on the GPU (kernels_resample.hip; ABI 7) ----
 *   rows    [B][n_knots][fields]
 *   queries [n_queries], one axis for the whole batch (per_problem = 0), or [B][n_queries] (per_problem = 1)
 *   out     [B][n_queries][fields]
 * all three in `memory`; nothing beyond the alignment of a double is assumed.  Every element of `out` is the host call's
 * bit for bit (the kernel is built without contraction and wraps angles with the routine of cilqr_device_math fn 6).  Rows
 * resampled in CILQR_ROWS_PLAN layout feed cilqr_check_collisions_batch where they lie (up to CILQR_DP_MAX_KNOTS of them:
 * 51 knots at five times the rate are 251), and the next cycle's start state is the previous plan at the cycle time.
 * Runs on the handle's stream and waits for that stream only; DEVICE arrays need no work space, HOST arrays are staged in
 * blocks that belong to the handle and grow to the largest call.  Checked before anything is launched, the handle staying
 * usable: CILQR_ERR_NULL; CILQR_ERR_ARG for batch < 1, n_knots < 2, n_queries < 1, an unknown layout, key or memory flag,
 * CILQR_KEY_STATION with CILQR_ROWS_TRAJ, per_problem not 0 or 1, out == rows; CILQR_ERR_CAPACITY for n_knots >
 * CILQR_DP_MAX_KNOTS (n_queries has no limit beyond int32: sizes are computed in size_t); CILQR_ERR_STATE while solves are
 * submitted on the handle. */
int cilqr_resample_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                              int32_t key, const double* queries, int32_t n_queries, int32_t per_problem,
                              double* out, int32_t memory);

/* ---- frenet: points in the frame of the centre line (DiscretizedTrajectory::GetProjection / GetCartesian,
 * algorithm/utils/discretized_trajectory.cpp:138-196); host calls, no handle ----
 * The reference plans in the Frenet frame of the road: DpPlanner starts from GetProjection of the start state, Environment
 * builds its barriers with GetCartesian, and the bounds a trajectory has to respect are left_bound / right_bound at a
 * station.  `center` is [n_center][7] = s x y theta kappa left_bound right_bound (as in cilqr_scene_batch: HOST memory,
 * one line per call), n_center >= 2.  Every operation below is rounded once (no fused multiply-add).
 * Projection of a point (px, py):
 *   nearest   at = the FIRST index minimising dx*dx + dy*dy with dx = x_i - px, dy = y_i - py: a scan over all points
 *             with a strict `<`, starting from DBL_MAX at index 0 (QueryNearestPoint) -- if every distance is a NaN or
 *             >= DBL_MAX, at = 0.
 *   pair      i0 = max(0, at-1), i1 = min(n_center-1, at+1); the projected point starts as row `at`.  If i0 < i1 (always,
 *             for n_center >= 2): v0 = p - c[i0], v1 = c[i1] - c[i0], delta_s = (v0.v1) / sqrt(v1.v1), and the projected
 *             point is LinearInterpolateTrajectory(c[i0], c[i1], s_i0 + delta_s):
 *                 |s_i1 - s_i0| < 1e-10 (strict): row i0 as bits (not the nearest row);
 *                 otherwise w = (s - s_i0) / (s_i1 - s_i0), s the query station itself, theta by slerp with the reference's
 *                 NormalizeAngle (as under "resample"), x y kappa left_bound right_bound (1 - w) * a + w * b.
 *             It extrapolates past either end (w < 0, w > 1), as the reference does.  c[i0] and c[i1] coincident in x, y
 *             divide by zero: the arithmetic decides.
 *   lateral   copysign(hypot(nr_x, nr_y), nr_y * cos(theta) - nr_x * sin(theta)) with nr = p - projected point and theta
 *             the projected point's; positive to the left of the line.
 *   row       CILQR_FRENET_FIELDS doubles: station, lateral, then the projected point's x, y, theta, kappa, left_bound,
 *             right_bound.  The margins to the road edges are left_bound - lateral and lateral + right_bound.
 * Inverse, for a pair (station, lateral): ref = EvaluateStation(station) -- the bracket of "resample" on the station
 * column, interpolated as above -- and the output is [3]: ref.x - lateral * sin(ref.theta), ref.y + lateral * cos(ref.theta),
 * ref.theta.
 * Non-finite inputs are no error: the arithmetic decides.  A result that is a NaN is a NaN in every implementation; which
 * NaN is not part of the rule, and neither is the sign that a NaN cross product lends to `lateral`.
 * sin / cos in the host calls are the C library's sincos of the angle: what the reference's build (g++ -O2) makes of its
 * std::sin and std::cos of one argument; glibc's sincos is not its sin / cos in the last bit for every angle.
 *   rows [n_rows][fields] in one of CILQR_ROWS_TRAJ / _PLAN / _COARSE / _POINTS: only x and y are read.
 * CILQR_ERR_NULL; CILQR_ERR_ARG for n_center < 2, n_rows / n < 1, an unknown layout, an output that overlaps an input.
 * C++ callers use include/cilqr/trajectory_queries.hpp directly (project_point, project_rows, cartesian_point). */
#define CILQR_ROWS_POINTS 4      /* [K][2] x 0, y 1: the two projection calls only (resample and the audit refuse it) */
#define CILQR_FRENET_FIELDS 8    /* station, lateral, x, y, theta, kappa, left_bound, right_bound */
int cilqr_frenet_rows(const double* center, int32_t n_center, int32_t layout, const double* rows, int32_t n_rows,
                      double* frenet /* [n_rows][CILQR_FRENET_FIELDS] */);
int cilqr_cartesian_points(const double* center, int32_t n_center, const double* sl /* [n][2] station, lateral */, int32_t n,
                           double* xyt /* [n][3] x, y, theta */);
/* ---- the same for B trajectories of K knots / n pairs per call, on the GPU (kernels_frenet.hip; ABI 7) ----
 *   rows [B][n_knots][fields], frenet [B][n_knots][CILQR_FRENET_FIELDS]; sl [n][2], xyt [n][3]: in `memory`, nothing beyond
 *   the alignment of a double is assumed.  `center` is HOST memory in either case.
 * The nearest point is found by the full scan, unpruned, so `at` is the host call's.  Every element of `frenet` is the host
 * call's bit for bit, except the SIGN of lateral: the kernel takes sin / cos for the cross product from its own lean
 * routine (about an ulp off the C library's), so the sign can differ where |cross| is within rounding of 0 -- a point on
 * the line (the host's |cross| <= 1e-9 |nr|); |lateral| is the host's bits there too.  hypot follows the C library's
 * evaluation for components up to 2^511 whose larger one is 0 or at least 2^-459.  In `xyt`, theta is the host call's
 * bits; x and y use the device library's sin / cos (cilqr_device_math fn 8 / 7) in the host's expression.
 * Both calls run on the handle's stream and wait for that stream only.  DEVICE arrays need no work space beyond the
 * centre line's tables, which are kept in a block that belongs to the handle and grows to the largest call; HOST arrays
 * are staged in blocks of the same kind.  There is no limit on n_center, n_knots or n beyond int32: sizes are computed in
 * size_t.  Checked before anything is launched, the handle staying usable: CILQR_ERR_NULL; CILQR_ERR_ARG for n_center < 2,
 * batch / n_knots / n < 1, an unknown layout or memory flag, an output that overlaps an input; CILQR_ERR_STATE while solves
 * are submitted on the handle. */
int cilqr_frenet_rows_batch(cilqr_handle h, const double* center, int32_t n_center, int32_t batch, int32_t layout,
                            const double* rows, int32_t n_knots, double* frenet, int32_t memory);
int cilqr_cartesian_points_batch(cilqr_handle h, const double* center, int32_t n_center, int32_t n, const double* sl,
                                 double* xyt, int32_t memory);

/* ---- clearance: how close every knot of a trajectory comes to the obstacles of its scene (Polygon2d::DistanceTo(Vec2d),
 * algorithm/math/polygon2d.cpp:43-52, over LineSegment2d::DistanceTo, line_segment2d.cpp:38-75); one scene on the host ----
 * The audit above answers yes / no at one buffer, and with the reference's HasOverlap(Box2d): a polygon vertex in the disc's
 * square or a corner of the square in the polygon -- a long edge through the square is not seen.  This is the continuous
 * counterpart, the number a caller ranks plans by or chooses a collision_buffer from.  Per knot:
 *   disc centres   the audit's: rear x + r2x cos(theta), y + r2x sin(theta); front the same with f2x; radius, r2x, f2x from
 *                  cfg as for cilqr_check_collisions.
 *   polygon        n >= 1 vertices, normalised as Polygon2d::BuildFromPoints does (polygon2d.cpp:206-234):
 *                  area = sum over i = 1 .. n-1 of CrossProd(p0, p[i-1], p[i]) = (p[i-1] - p0) x (p[i] - p0); if area < 0 the
 *                  whole vertex array is reversed.  Edge i is (p[i], p[Next(i)]), Next(n-1) = 0: n = 1 gives one degenerate
 *                  edge, n = 2 two.  An edge carries the constructor's arithmetic: length = hypot(dx, dy), unit vector
 *                  (dx / length, dy / length), or (0, 0) when length <= 1e-10.
 *   distance       from a disc centre c to a polygon: d = 0.0 if IsPointIn(c) (the bounding box first, then the crossing
 *                  count, polygon2d.cpp:120-140).  Otherwise d starts at +inf and is updated edge by edge in order with
 *                  std::min(d, edge.DistanceTo(c)), that is (e < d) ? e : d -- a NaN is never taken.  edge.DistanceTo: with
 *                  x0, y0 = c - start: length <= 1e-10: hypot(x0, y0); proj = x0 ux + y0 uy; proj <= 0: hypot(x0, y0);
 *                  proj >= length: hypot(c - end); else |x0 uy - y0 ux|.  Every operation is rounded once (no fused
 *                  multiply-add), as the library is built.
 *   static column  the slots with a count >= 1 in slot order: best = +inf, slot = -1; a slot replaces them only when its
 *                  d < best (the first of equals wins).  Output: best - radius, one rounded subtraction (+inf stays +inf),
 *                  and the slot.
 *   dynamic column the same over the dynamic slots present at the knot's time.  Presence and the choice of the sample are
 *                  exactly those of cilqr_check_collisions (no epsilon; the first sample with t < time[k]; past the end the
 *                  last), the placement is in Pose::transform order; the placed polygon is then normalised and measured as
 *                  above.
 * Per trajectory: min_clearance = the smallest of the K x 4 values under the same strict `<` from +inf; min_knot = the first
 * knot whose row attains it, -1 if every value is +inf.  A negative clearance is a disc that reaches into (or, at -radius,
 * whose centre lies inside) a polygon.
 * The road barriers are deliberately not a column: they are a sampled point set, not an outline, and the margins to the
 * road edges are left_bound - lateral and lateral + right_bound of cilqr_frenet_rows[_batch].
 * Non-finite rows are no error: the arithmetic decides (a NaN centre is in no polygon and no NaN distance is taken, so its
 * values are +inf; a NaN vertex only ever removes its own polygon's edges from the minimum).
 *   rows [n_knots][fields] in CILQR_ROWS_TRAJ / _PLAN / _COARSE: only time, x, y, theta are read
 *   clearance [n_knots][CILQR_CLEARANCE_FIELDS]; nearest [n_knots][CILQR_CLEARANCE_FIELDS] slots, optional (NULL to skip)
 * CILQR_ERR_NULL; CILQR_ERR_ARG for an unknown layout (CILQR_ROWS_POINTS included: it has no time or heading), n_knots < 1,
 * n_center < 2, a negative count; CILQR_ERR_CAPACITY beyond the CILQR_DP_MAX_* limits -- the checks of
 * cilqr_check_collisions.  C++ callers use DpEnvironment::Clearance of include/cilqr/dp_planner.hpp directly. */
#define CILQR_CLEARANCE_FIELDS 4   /* rear_static, rear_dynamic, front_static, front_dynamic */
int cilqr_clearance_rows(const cilqr_dp_config* cfg, const cilqr_scene* scene, int32_t layout, const double* rows,
                         int32_t n_knots, double* clearance /* [K][4] */, int32_t* nearest /* [K][4], optional */,
                         double* min_clearance, int32_t* min_knot);
/* ---- the same for B scenes per call, on the GPU (kernels_clearance.hip; additive, ABI 7) ----
 * One workgroup per scene.  The arithmetic is the host call's except for the vehicle heading, which goes through the DP
 * kernels' sin / cos, and the obstacle placement, which goes through the device library's cos / sin (cilqr_device_math fn
 * 7 / 8): a distance differs from the host's by rounding of the centres and the placed vertices only (distance is
 * 1-Lipschitz in both), hypot follows the C library's evaluation for lengths in metres.  A scene's result does not depend
 * on the batch around it or on unused slots.
 *   rows          [B][n_knots][fields]             (memory as scenes->memory, like the four arrays below)
 *   clearance     [B][n_knots][4], optional;  nearest [B][n_knots][4], optional
 *   min_clearance [B];  min_knot [B]
 *   *n_below (HOST, optional): the scenes with min_clearance < threshold
 * Checked before anything is launched: the checks of cilqr_check_collisions_batch (CILQR_ERR_NULL, _ARG, _CAPACITY, _STATE),
 * and CILQR_ERR_ARG for a non-finite threshold with n_below given.  With DEVICE arrays the counts are checked in the
 * kernel: such a scene gets min_knot -2, a NaN min_clearance and NaN rows (nearest -1), the others are unaffected.  Runs on
 * the handle's stream and waits for that stream only; DEVICE arrays need no work space beyond the count, HOST arrays are
 * staged in blocks that belong to the handle and grow to the largest call. */
int cilqr_clearance_rows_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                               int32_t layout, const double* rows, int32_t n_knots,
                               double* clearance /* [B][K][4], optional */, int32_t* nearest /* [B][K][4], optional */,
                               double* min_clearance /* [B] */, int32_t* min_knot /* [B] */,
                               double threshold, int32_t* n_below /* HOST, optional */);

/* ---- constraint margins: how far a trajectory stays inside the constraints of its own solve (additive, ABI 7) ----
 * The solver enforces the corridor half-planes, the two lane tables and the state / control bounds as relaxed-log barriers
 * (quadratic for g > -barrier_eps, finite for g > 0), so a returned trajectory -- status 1 and 2 included, 4 and 5 the more
 * so -- may sit on the wrong side of a constraint.  These calls evaluate every constraint the solve was given on rows in
 * one of the CILQR_ROWS_TRAJ / _PLAN / _COARSE layouts (CILQR_ROWS_POINTS is refused) and reduce them per problem.
 * Every value is a MARGIN in physical units: >= 0 satisfied, < 0 violated.  Per knot i, D = cfg.num_of_disc; every
 * operation is rounded once (no fused multiply-add); hypot is the C library's evaluation for lengths in metres:
 *   disc centres   p_j = (x, y) + disc_off[j] (cos theta, sin theta), disc_off[j] = L (j - 0.5) - rear_hang,
 *                  L = (rear_hang + wheel_base + front_hang) / D   (cc:556-565).
 *   corridor plane the first n = max(0, min(corridor_count[i], in->cmax)) planes of the knot.  Each is shrunk and normalised
 *                  as the solver does it (cc:448, 479): c' = c - (disc_radius + safe_margin) (a a + b b) / hypot(a, b),
 *                  nrm = hypot(hypot(a, b), c'), (a_n, b_n, c_n) = (a, b, c') / nrm; if one of the three is not finite the
 *                  plane is (0, 0, -inf).  g = a_n px + b_n py - c_n, m = -g / hypot(a_n, b_n): metres, with exactly the
 *                  sign of the -g the cost sees.  A degenerate plane gives -inf.
 *   column 0       corridor: the minimum of m over the discs (outer loop) and the planes (inner loop), strict `<` from +inf:
 *                  the first of equals wins.  n = 0 gives +inf.
 *   columns 1, 2   left and right lane.  For every disc the segment FindNeastLaneSegment returns (cc:605-618:
 *                  LineSegment2d::DistanceTo, strict `<`, the first index; with exact lane ties off, the same cases compared
 *                  on squared distances alone, see CILQR_OPT_EXACT_LANE_TIES); its plane shrunk by disc_radius and
 *                  normalised in the same way (no rule for a non-finite result), the same m.  The column is the minimum
 *                  over the discs, the first of equals.
 *   columns 3 .. 7 velocity, acceleration, steering, jerk, steering rate: m = -g for the two g of the family as
 *                  DynamicsCost writes them (cc:523-528, 543-546): (-v, v - max_velocity), (a - max_acceleration,
 *                  min_acceleration - a), (delta - delta_max, delta_min - delta), (jerk - jerk_max, jerk_min - jerk),
 *                  (rate - delta_rate_max, delta_rate_min - rate); the smaller of the two, the first of equals.  Jerk and
 *                  steering rate are +inf at the last knot, and at every knot of a layout without control columns.
 *   NaN            a NaN margin is replaced by -inf before any comparison: a NaN pose never passes as feasible.
 *   columns read   CILQR_ROWS_TRAJ x 1 y 2 theta 3 v 4 a 5 delta 6 jerk 8 rate 9;  CILQR_ROWS_PLAN x 2 y 3 theta 4 v 6 a 7
 *                  delta 8 jerk 9 rate 10;  CILQR_ROWS_COARSE x 2 y 3 theta 4 v 6 a 7 delta 8, no controls.  (The code takes
 *                  these numbers from include/cilqr/row_layouts.hpp: state_columns.)
 *   which          (optional) [K][CILQR_MARGIN_WHICH_FIELDS]: the deciders -- corridor disc, corridor plane, left disc, left
 *                  segment, right disc, right segment (segments counted within the side's table of the problem's lane
 *                  group); -1 where the column is +inf.
 * Per problem: min_margin [8] = each column's minimum over the knots under the same strict `<`; min_knot [8] = the first
 * knot attaining it, -1 if the column is +inf throughout; violated = a bit mask, bit f (CILQR_MARGIN_BIT_*) set when
 * min_margin[f] < -tol[f].  tol [8]: HOST memory, optional (NULL: zeros), every entry finite and >= 0.  Per call:
 * *n_violating (HOST, optional) = the problems with a non-zero mask.
 * Of `in` the calls read batch, n_knots, cmax, memory, corridor, corridor_count and the lane tables with their groups (as
 * cilqr_solve_batch reads them); start, coarse and coarse_station are ignored and may be NULL.
 * cilqr_constraint_margins: the host call, in->memory == CILQR_MEM_HOST, any batch and any n_knots >= 1; the C library's cos
 * and sin; exact_lane_ties as CILQR_OPT_EXACT_LANE_TIES.  CILQR_ERR_NULL; CILQR_ERR_ARG for batch / n_knots < 1, an unknown
 * layout or memory flag, DEVICE memory, a tol entry that is negative or not finite, num_of_disc outside 1 .. CILQR_MAX_DISCS,
 * inconsistent lane groups; CILQR_ERR_CONSTRAINTS for missing corridor / lane arrays, cmax < 1 or an empty lane table, as a
 * solve.  C++ callers use include/cilqr/constraint_margins.hpp directly. */
#define CILQR_MARGIN_FIELDS 8
#define CILQR_MARGIN_WHICH_FIELDS 6
#define CILQR_MARGIN_BIT_CORRIDOR 0x01u
#define CILQR_MARGIN_BIT_LEFT_LANE 0x02u
#define CILQR_MARGIN_BIT_RIGHT_LANE 0x04u
#define CILQR_MARGIN_BIT_VELOCITY 0x08u
#define CILQR_MARGIN_BIT_ACCELERATION 0x10u
#define CILQR_MARGIN_BIT_STEERING 0x20u
#define CILQR_MARGIN_BIT_JERK 0x40u
#define CILQR_MARGIN_BIT_STEERING_RATE 0x80u
int cilqr_constraint_margins(const cilqr_config* cfg, int32_t exact_lane_ties, const cilqr_problem_batch* in, int32_t layout,
                             const double* rows, double* margins /* [B][K][8], optional */,
                             int32_t* which /* [B][K][6], optional */, double* min_margin /* [B][8] */,
                             int32_t* min_knot /* [B][8] */, const double* tol /* [8], optional */,
                             uint32_t* violated /* [B] */, int32_t* n_violating /* optional */);
/* ---- the same on the GPU (kernels_margins.hip) ----
 * One workgroup per problem reads the raw problem-major corridor where it lies.  rows and every per-problem output live in
 * in->memory.  The configuration, disc_off, the two shrink distances and the lane-tie rule are the handle's
 * (CILQR_OPT_EXACT_LANE_TIES as in force); in->n_knots and in->batch are NOT tied to the handle's n_steps or batch_capacity.
 * in->cmax above the handle's cmax, or a lane table above its max_lane_segments: CILQR_ERR_CAPACITY, as a solve.  The
 * arithmetic is the host call's except for the heading, which goes through the cost kernels' sin / cos (cilqr_device_math fn
 * 3 / 4): the bound columns are the host call's bits, the plane columns differ by the rounding of the disc centres only.
 * A problem's result does not depend on the batch around it.
 * Checked before anything is launched: the checks of the host call, and CILQR_ERR_STATE while solves are submitted on the
 * handle.  The call works in blocks of its own that belong to the handle and grow to the largest call; it touches neither
 * the staged nor the solver state (a cilqr_stage_* sequence around it sees nothing), runs on the handle's stream and waits for
 * that stream only. */
int cilqr_constraint_margins_batch(cilqr_handle h, const cilqr_problem_batch* in, int32_t layout, const double* rows,
                                   double* margins /* [B][K][8], optional */, int32_t* which /* [B][K][6], optional */,
                                   double* min_margin /* [B][8] */, int32_t* min_knot /* [B][8] */,
                                   const double* tol /* HOST [8], optional */, uint32_t* violated /* [B] */,
                                   int32_t* n_violating /* HOST, optional */);

/* ---- track: drive a vehicle along trajectory rows with the closed-loop Tracker (Tracker::Plan, algorithm/ilqr/tracker.cc:
 * 12-215); one trajectory on the host, no handle ----
 * The vehicle is simulated at sumulation_dt with RK4 under a lateral and a longitudinal LQR controller; it follows `rows`
 * from `start6`, which need not lie on them.  What CILQR_INIT_TRACKER runs inside a solve (kernels_tracker.hip), as a call of
 * its own: any time column, a full six-state start, any number of knots.
 *   followed   K = n_knots >= 2 rows in CILQR_ROWS_TRAJ / _PLAN / _COARSE; read: time, x, y, theta, v (and a, delta of row 0
 *              when start6 is NULL).  time is taken as non-decreasing; start_time = time[0], end_time = time[K-1].  station =
 *              the layout's station column (_PLAN, _COARSE); for _TRAJ the accumulated chord length s[0] = 0, s[k] = s[k-1] +
 *              hypot(x[k] - x[k-1], y[k] - y[k-1]), hypot as glibc 2.35 evaluates it without fused multiply-add.
 *   start      start6 = x y theta v a delta; NULL: x, y, theta, v, a, delta of row 0.
 *   gains      K = (R + B'PB)^-1 B'PA, P from P <- A'PA - A'PB (R + B'PB)^-1 B'PA + Q started at Q, while fewer than
 *              max_num_iteration rounds are done and |max coefficient of (P_next - P)| > tolerance; products accumulate in
 *              index order.  Longitudinal (once): A = I + [[0, dt, 0], [0, 0, -dt], 0], B = (0, 0, dt), Q = diag(weight_s,
 *              weight_v, weight_a), R = weight_j.  Lateral (every step): A = I + [[0, vm 0.1, 0], [0, 0, -vm / wheel_base 0.1],
 *              0] with vm = max(2, v) and 0.1 a literal, B = (0, 0, dt), Q = diag(weight_l, weight_theta, weight_delta), R =
 *              weight_delta_rate.
 *   clock      cur_time = start_time, i = 1; for (t = start_time; t < end_time + 1e-10; t += sumulation_dt), at most
 *              CILQR_TRACKER_MAX_SIM_STEPS rounds whatever the time column holds, and no further round once n_drive knots are
 *              recorded.  One round:
 *     preview     (x + cos(theta) v preview_time, y + sin(theta) v preview_time)
 *     projection  nearest followed point (first minimum of the squared distance over all K), its neighbours i0 = max(0, at -
 *                 1), i1 = min(K - 1, at + 1): st = s[i0] + (w . d) / |d| with d = p[i1] - p[i0], w = preview - p[i0]; if
 *                 |s[i1] - s[i0]| < 1e-10 the point is row i0, else x, y, v linear in station at st and theta by slerp
 *                 ("resample" above).
 *     lateral     (sin(pth) (x - px) - cos(pth) (y - py), NormalizeAngle(pth - theta), delta)
 *     match       the bracket of "resample" on the time column at cur_time: rows it - 1, it; if |t1 - t0| < 1e-10 station and
 *                 v of row it - 1, else linear in time
 *     longitud.   (match.s - st, match.v - v, a)
 *     controls    delta_rate = -K_lat . lateral, jerk = -K_lon . longitudinal, clamped to the vehicle's bounds
 *     RK4         one step of (x, y, theta, v, delta, a)' = (v cos theta, v sin theta, v tan(delta) / wheel_base, a,
 *                 delta_rate, jerk); then theta wrapped, v = max(0, v), delta clamped then wrapped, a clamped
 *     keep        cur_time = t (the clock BEFORE the step, as the reference has it); if i < K and cur_time > time[i] - 1e-10:
 *                 row i - 1 receives (jerk, delta_rate), the state is recorded as row i, i += 1
 *   n_drive    1 ... n_knots rows are recorded (row 0 is the start).  The projection still scans all n_knots and end_time is
 *              the last row's: rows 0 ... n_drive - 1 of a run with a larger n_drive are these rows bit for bit -- except the
 *              two control columns of row n_drive - 1, which belong to a step this run does not take and are 0.
 *   driven     [n_drive][CILQR_TRAJ_FIELDS]: time = cur_time when the row was recorded (row 0: start_time), x y theta v a
 *              delta, kappa = tan(delta) / wheel_base, jerk and delta_rate = the controls in force when the NEXT row was
 *              recorded; the last row's are 0, as the solver's export has them at its last knot.
 *   failure    fewer than n_drive rows recorded when the clock ends or the round limit is reached -- the reference's "tacker
 *              failed" (cc:205-208): CILQR_ERR_STATE, every row of `driven` zero.
 * Non-finite rows are no error: the arithmetic decides.  Every operation is rounded once; sin / cos (one sincos call where
 * the C library has it) and tan are the C library's.  CILQR_ERR_NULL; CILQR_ERR_ARG for an unknown layout (CILQR_ROWS_POINTS
 * included), n_knots < 2, n_drive outside 1 ... n_knots, a tracker configuration cilqr_set_tracker_config would refuse for
 * its values alone (non-finite, sumulation_dt or dt <= 0, tolerance < 0, max_num_iteration outside 1 ...
 * CILQR_TRACKER_MAX_ITERATIONS).  Of cfg only wheel_base and the five pairs of bounds are read.  C++ callers with the
 * reference's types use include/cilqr/tracker.hpp. */
int cilqr_track_rows(const cilqr_config* cfg, const cilqr_tracker_config* tcfg, int32_t layout, const double* rows,
                     int32_t n_knots, const double* start6 /* [6], optional */, int32_t n_drive,
                     double* driven /* [n_drive][CILQR_TRAJ_FIELDS] */);
/* ---- the same for B trajectories per call, on the GPU (kernels_track.hip; ABI 7) ----
 *   rows [B][n_knots][fields], start6 [B][6] (optional), driven [B][n_drive][CILQR_TRAJ_FIELDS], ok [B]: in `memory`;
 *   n_failed: HOST, optional.
 * The tracker configuration is the handle's (cilqr_set_tracker_config), wheel base and bounds those of cilqr_create; batch
 * and n_knots are not tied to the handle's, and no problem needs to be loaded.  ok[b] = 1: n_drive rows were recorded; 0:
 * the failure above, that problem's rows are all zero, the others are unaffected; *n_failed counts them.  A problem's rows do
 * not depend on the batch around it.  One lane per problem; sin, cos and tan are the device's (cilqr_device_math), so the
 * rows follow the host call closely but not bit for bit.  A pre-pass gathers the columns the rule reads into a
 * batch-fastest table in work space that belongs to the handle and grows to the largest call (48 bytes per followed row);
 * HOST arrays are staged in blocks of the handle likewise.  Driven rows in this layout feed cilqr_check_collisions_batch,
 * cilqr_clearance_rows_batch, cilqr_constraint_margins_batch, cilqr_resample_rows_batch and cilqr_solve_batch_warm where they
 * lie.  Runs on the handle's stream and waits for that stream only.  Checked before anything is launched, the handle staying
 * usable: CILQR_ERR_NULL (handle, rows, driven, ok); CILQR_ERR_ARG for batch < 1, an unknown layout, CILQR_ROWS_POINTS,
 * n_knots < 2, n_drive outside 1 ... n_knots, an unknown memory flag; CILQR_ERR_STATE while solves are submitted on the
 * handle. */
int cilqr_track_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                           const double* start6 /* [B][6], optional */, int32_t n_drive,
                           double* driven /* [B][n_drive][CILQR_TRAJ_FIELDS] */, int32_t* ok /* [B] */,
                           int32_t* n_failed /* HOST, optional */, int32_t memory);

/* ---- policy: the closed-loop law of a solve -- its feedback gains, and rollouts under them from starts the caller chooses
 * (additive, ABI 7) ----
 * Every iteration of a solve computes the gains K_i (2 x 6), k_i of the Riccati pass and applies them in Forward (cc:392-415)
 * as u_i = u*_i + K_i (x_i - x*_i) + alpha k_i.  Their curvature includes the corridor, lane and bound barriers.  The two calls
 * give that law to the caller: the gains about any batch of trajectories, and what the vehicle does under them when it does not
 * start where the plan assumed.
 *
 * cilqr_policy_gains_batch is the stage chain, bit for bit: cilqr_stage_load(in); the current iterate set to the state
 * columns of all K rows and the control columns of the first N rows of `rows` (the bits copied, on the device, wherever the
 * rows lie; every other column is not read); cilqr_stage_quadratize; cilqr_stage_backward(lambda); CILQR_T_KFB, CILQR_T_KFF
 * and CILQR_T_DV written problem-major as cilqr_stage_read writes them.  rows [B][K][fields], lambda [B] (NULL: 0 for every
 * problem), Kfb [B][N][2][6], kff [B][N][2], dV [B][2] (optional) and ok [B] (optional) lie in in->memory.  layout:
 * CILQR_ROWS_TRAJ or CILQR_ROWS_PLAN -- every other layout lacks the controls or the states: CILQR_ERR_ARG.  A problem with a
 * negative corridor_count at some knot (CILQR_ST_NO_CORRIDOR) gets ok = 0 and zeros in its K, k and dV; every other gets ok =
 * 1.  Backward has no failure exit in the reference (cc:363-371), so there is none here; a non-finite row poisons its own
 * problem only.  The checks are those of cilqr_stage_load -- among them CILQR_ERR_KNOTS unless in->n_knots is the handle's K,
 * CILQR_ERR_ARG for a batch with more than one lane group (solve such groups one call each), CILQR_ERR_STATE while solves
 * are submitted on the handle -- and CILQR_ERR_NULL for h, in, rows, Kfb, kff.  Afterwards the handle is in the staged state of
 * that chain: cilqr_stage_read and cilqr_stage_forward work on it. */
int cilqr_policy_gains_batch(cilqr_handle h, const cilqr_problem_batch* in, int32_t layout, const double* rows,
                             const double* lambda /* [B] or NULL = 0 for every problem */,
                             double* Kfb /* [B][N][2][6] */, double* kff /* [B][N][2] */, double* dV /* [B][2], optional */,
                             int32_t* ok /* [B], optional */);
/* cilqr_policy_rollout_batch (kernels_policy.hip): Forward from start6[s][b], for n_samples starts of every problem.
 * For sample s of problem b: x_0 = start6[s][b]; for every step i < n_out - 1
 *   difference  dx = x_i - x*_i component by component, x* the state columns of nominal row i.  theta is NOT wrapped, as at
 *               cc:407: a start on the other side of the +-pi cut from the nominal heading is the caller's business.
 *   control     for r = 0, 1: acc = K_i[r][0] dx_0; acc += K_i[r][1] dx_1; ... acc += K_i[r][5] dx_5;
 *               u_r = (u*_r + acc) + alpha k_i[r], u* the control columns of nominal row i; with kff == NULL u_r = u*_r + acc
 *               and alpha is not read.
 *   clamp       if clamp != 0: u_0 limited to [jerk_min, jerk_max], u_1 to [delta_rate_min, delta_rate_max] of the handle's
 *               configuration, as u < lo ? lo : (u > hi ? hi : u) -- a NaN passes.  n_clamped counts the steps at which a
 *               limit was applied to either control.
 *   step        u_1 = NormalizeAngle(u_1), x_{i+1} = Dynamics(x_i, u) (cc:408-410), the solve's own step.
 * Recorded row i (CILQR_ROWS_TRAJ): time i dt, the six states x_i, kappa = tan(delta) / wheel_base, the two controls applied
 * at step i; the last recorded row carries controls (0, 0), as the solver's export has them at its last knot.  max_dev =
 * sqrt(max_i ((x_i - x*_i)^2 + (y_i - y*_i)^2)) over the recorded rows (a NaN stays), end_dev the same at the last recorded
 * row.  dt, wheel_base and the bounds are the handle's; batch and n_knots are NOT tied to it (as for the margins), and no
 * problem needs to be loaded.
 *   rows [B][n_knots][fields] in CILQR_ROWS_TRAJ / _PLAN, Kfb [B][n_knots - 1][2][6], kff [B][n_knots - 1][2] or NULL,
 *   start6 [S][B][6], out_rows [S][B][n_out][CILQR_TRAJ_FIELDS], max_dev, end_dev, n_clamped [S][B]: all in `memory`; each
 *   output is optional, with out_rows == NULL only the summaries are produced (the cheap Monte-Carlo form).
 * Outputs are sample-major on purpose: slice s of out_rows is an ordinary batch of B CILQR_ROWS_TRAJ trajectories, which
 * cilqr_check_collisions_batch, cilqr_clearance_rows_batch, cilqr_constraint_margins_batch, cilqr_resample_rows_batch and a
 * warm start take where it lies, with the scenes or the problem batch of the nominal plans.  A chain's bits do not depend on
 * the batch, the samples or the chains around it.  Runs on the handle's stream and waits for that stream only; it touches
 * neither the staged nor the solver state.  Checked before anything is launched, the handle staying usable: CILQR_ERR_NULL
 * (h, rows, Kfb, start6; every output NULL); CILQR_ERR_ARG for an unknown memory flag, a layout other than _TRAJ / _PLAN,
 * batch < 1, n_knots < 2, n_out outside 1 ... n_knots, n_samples outside 1 ... CILQR_POLICY_MAX_SAMPLES, a non-finite alpha
 * with kff != NULL; CILQR_ERR_STATE while solves are submitted on the handle.  Process noise and random numbers are the
 * caller's: it supplies the starts. */
#define CILQR_POLICY_MAX_SAMPLES 256
int cilqr_policy_rollout_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows /* nominal [B][K][F] */,
                               int32_t n_knots, const double* Kfb /* [B][N][2][6] */, const double* kff /* [B][N][2] or NULL */,
                               double alpha, int32_t n_samples, const double* start6 /* [S][B][6] */, int32_t clamp,
                               int32_t n_out /* 1..K rows recorded; n_out - 1 steps are simulated */,
                               double* out_rows /* [S][B][n_out][CILQR_TRAJ_FIELDS] or NULL */,
                               double* max_dev /* [S][B] or NULL */, double* end_dev /* [S][B] or NULL */,
                               int32_t* n_clamped /* [S][B] or NULL */, int32_t memory);

/* ---- TrajectoryPlanner::Plan for B scenes per call (trajectory_planner.cpp:28-162) ----
 * scene batch -> cilqr_dp_plan_batch -> cilqr_scene_points_batch (at the time column the planner produced, with
 * corridor_cfg->is_multiple_sample and the worst-case max_points) -> cilqr_build_corridors (the cmax of the handle's
 * create call) -> cilqr_solve_batch with the lane tables of cilqr_road_barriers + cilqr_lane_constraints (built once per
 * call on the host from the batch's centre line and corridor_cfg->lane_segment_length) -> the rows of
 * trajectory_planner.cpp:101-125.  Only the scenes and the start states cross to the device: every intermediate lives in
 * the handle's work space (grown to the largest call), points and corridors are produced for CILQR_OPT_SCENE_CHUNK scenes at a
 * time, the corridors of the whole batch go into one solve.  The results are, bit for bit, those of the four calls made
 * one after the other (the solve is given the planner's station column as coarse_station).
 *   start4  [B][4] x y theta v       (memory as scenes->memory, like plan / coarse9 / outcome)
 *   out     the solver's own outputs, as for cilqr_solve_batch (its own `memory`)
 *   plan    [B][n_knots][CILQR_PLAN_FIELDS], optional: time s x y theta kappa velocity a delta jerk delta_rate; s is the
 *           running sum of hypot over the optimised x / y, every other column the bits of the trajectory's column
 *   coarse9 [B][n_knots][CILQR_COARSE_FIELDS], optional: the DP planner's trajectory
 *   outcome [B], optional: 0 planned; CILQR_PLAN_DP_FAILED ("DP failed", cpp:32-35); CILQR_PLAN_CORRIDOR_FAILED ("Corridor
 *           failed", cpp:49-57: a knot with corridor_count -2 ... -4).  Such a scene is not optimised: it ends with
 *           CILQR_ST_NO_CORRIDOR.  *n_dp_failed / *n_corridor_failed (HOST, optional): how many there are of each.
 * CILQR_ERR_CAPACITY when (max_static + max_dynamic) * max_vertices * (6 or 1) + 8 (24 with is_multiple_sample) exceeds
 * the corridor kernel's 320 points, when the batch exceeds the handle's capacity or the lane tables its
 * max_lane_segments; CILQR_ERR_KNOTS unless n_knots = tf / delta_t + 1 = the handle's n_steps + 1; the other checks are
 * those of the calls above, all made before anything is launched. */
#define CILQR_PLAN_FIELDS 11
#define CILQR_PLAN_DP_FAILED 1
#define CILQR_PLAN_CORRIDOR_FAILED 2
int cilqr_plan_scenes_batch(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                            const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots,
                            cilqr_solution_batch* out, double* plan, double* coarse9, int32_t* outcome,
                            int32_t* n_dp_failed, int32_t* n_corridor_failed);
/* ... with a warm start (see cilqr_solve_batch_warm): the pipeline of the second and every later planning cycle.  `warm` is
 * the cilqr_warm_start of the solve at the pipeline's end, for the B scenes in their order; warm->memory must equal
 * scenes->memory (HOST rows and shifts are staged into the pipeline's work space).  warm == NULL is exactly
 * cilqr_plan_scenes_batch.  The results are, bit for bit, those of the four calls made one after the other with
 * cilqr_solve_batch_warm last: a scene with shift < 0 has the bits of the cold pipeline, and one the pipeline does not
 * optimise (outcome != 0) ends with CILQR_ST_NO_CORRIDOR as there, its traj the first iterate.  The checks of cilqr_solve_batch_warm (CILQR_ERR_NULL for NULL rows, CILQR_ERR_ARG
 * for an unknown layout, CILQR_ROWS_COARSE, a bad or differing memory flag) are made with the others, before anything is
 * launched. */
int cilqr_plan_scenes_batch_warm(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                                 const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots,
                                 const cilqr_warm_start* warm, cilqr_solution_batch* out, double* plan, double* coarse9,
                                 int32_t* outcome, int32_t* n_dp_failed, int32_t* n_corridor_failed);

/* ---- scene window: a scene on the clock of a later planning cycle (additive, ABI 7) ----
 * Every scene call above reads a scene on the clock 0 ... tf, and a dynamic obstacle's samples carry absolute times.  To
 * plan again at scene time t0 the trajectories have to be on the clock t - t0, and of a long recording only the samples
 * the horizon can reach are wanted (CILQR_DP_MAX_SAMPLES holds for what the scene kernels read, not for what was recorded).
 * The window rule, for ONE dynamic obstacle with T samples time x y theta (times taken as non-decreasing, as everywhere in
 * the scene calls), a scene time t0, a span >= 0 and an output capacity out_samples; every operation is rounded once,
 * s[k] = time[k] - t0:
 *   T < 1:  count 0.  Otherwise
 *   L = the first k with !(s[k] < -1e-9), T if there is none;             lo = max(0, L - 1)
 *   H = the first k with (span + 1e-9) < s[k], T if there is none;        hi = min(T - 1, H)
 *       both searches are std::lower_bound's halving written out over the predicate, as in the resample rule,
 *           first = 0, len = T;  while (len > 0) { half = len >> 1;
 *               if (!pred(first + half)) { first += half + 1; len -= half + 1; } else len = half; }
 *       -- defined for any input, and L <= H on any input (the second predicate implies the first, so the two halvings
 *       probe the same samples until they part, the first going left); so count >= 1 whenever T >= 1;
 *   count = hi - lo + 1;  output sample j = (s[lo + j], then x, y, theta of sample lo + j copied as bits).
 *   count > out_samples: the obstacle OVERFLOWS.  Its count is written as -1, not as 0: the scene calls then refuse the
 *       scene (HOST arrays: CILQR_ERR_ARG; DEVICE arrays: the scene is reported invalid by the kernel that reads it) rather
 *       than plan it without that obstacle.  A source count that is negative or above the source's max_samples is treated
 *       the same way.  Nothing is written to the rows of such an obstacle.
 * Why the window is safe.  scene_core.hpp: scene_present / scene_sample_index choose the sample an obstacle shows at a
 * query time t, in a plain form (t < time[k]; present unless time[0] > t or time[T-1] < t) and in the 1e-10 form of the
 * Query...Points rule (t < time[k] + 1e-10; time[0] > t + 1e-10, time[T-1] < t - 1e-10).  Take any t in [0, span].
 *   - The chosen index is the first k with t < s[k] (+ 1e-10), T - 1 past the end.  Such a k has s[k] > -1e-10 (1 + 2^-52)
 *     > -1e-9, so !(s[k] < -1e-9) holds and k >= L >= lo.  If H < T, s[H] > span + 1e-9 > t, so the first such k is <= H;
 *     if H = T the index is at most T - 1.  Either way it is <= hi.
 *   - Every sample below lo has s < -1e-9, so neither form chooses it and the search over samples lo ... hi finds the same
 *     sample at index - lo; where the full search runs past the end (H = T) the window ends at T - 1 as well.
 *   - Presence.  If lo > 0, s[lo] < -1e-9 <= t: both `first sample later than t` tests are false on s[lo], and on s[0] <=
 *     s[lo] too.  If hi < T - 1, s[hi] > span + 1e-9 >= t + 1e-9: both `last sample earlier than t` tests are false on
 *     s[hi], and on s[T-1] >= s[hi] too.  Otherwise the window's end sample is the trajectory's.
 * So the window is not only close to the full shifted trajectory (time - t0, x, y, theta for all T samples): every scene
 * call returns the same bits on both, for knot and row times in [0, span].  The margins of 1e-9 against the rule's 1e-10
 * are what make this hold under rounding: a sum t + 1e-10 or s + 1e-10 is off by less than 1e-25 at these magnitudes.
 *
 * cilqr_window_scene: one scene on the host, no handle (C++ callers use include/cilqr/scene_window.hpp directly).  No limit
 * is placed on the source sample counts.
 *   trajectories [n_dynamic][out_samples][4], counts [n_dynamic]; rows past an obstacle's count are left untouched
 *   *n_overflow (optional): the obstacles that overflowed
 * CILQR_ERR_NULL; CILQR_ERR_ARG for a non-finite t0, a span that is non-finite or negative, out_samples < 1, n_dynamic < 0
 * and a negative count. */
int cilqr_window_scene(const cilqr_scene* scene, double t0, double span, int32_t out_samples,
                       double* trajectories /* [n_dynamic][out_samples][4] */, int32_t* counts /* [n_dynamic] */,
                       int32_t* n_overflow);
/* ---- the same for B scenes per call, each at its own t0, on the GPU (kernels_scene_window.hip) ----
 * The windows of a batch that is resident on the device: a cilqr_scene_batch with dynamic_trajectories = `trajectories`,
 * dynamic_trajectory_counts = `counts`, max_samples = out_samples and every other member as in `scenes` is the batch on the
 * clocks t - t0[b], and nothing but t0 crosses to the device per cycle.  scenes->max_samples may be any positive value:
 * this call alone does not hold the source to CILQR_DP_MAX_SAMPLES (CILQR_ERR_CAPACITY for out_samples beyond it).
 *   t0           [B]                                     (memory as scenes->memory, like the three arrays below)
 *   trajectories [B][max_dynamic][out_samples][4]        rows past a count are left untouched
 *   counts       [B][max_dynamic]
 *   ok           [B] 1 / 0, optional (NULL to skip): 0 where one of the scene's counts is -1
 *   *n_overflow  (HOST, optional): the scenes with ok = 0
 * One wavefront per (scene, slot); the two searches are made by the wave together (64 probes and one ballot per round)
 * and return what the halving returns on non-decreasing times (on times that decrease the wave's two searches can cross;
 * such an obstacle is refused with count -1).  Every element is the host call's bit for bit; a scene's windows do not depend
 * on the batch around it; no alignment beyond a double's is assumed.  Runs on the handle's stream and waits for that stream
 * only; DEVICE arrays need no work space beyond the count, HOST arrays are staged in blocks that belong to the handle and
 * grow to the largest call.  Checked before anything is launched, the handle staying usable: CILQR_ERR_NULL;
 * CILQR_ERR_ARG for a bad batch, sizes or memory flag, a span that is non-finite or negative, out_samples < 1 and -- HOST
 * arrays -- a non-finite t0[b] or a source count that is negative or above max_samples; CILQR_ERR_CAPACITY as above;
 * CILQR_ERR_STATE while solves are submitted on the handle.  With DEVICE arrays t0 and the counts are checked in the
 * kernel: a non-finite t0[b] or a bad source count gives every slot of that scene the count -1 and ok 0, the other scenes
 * are unaffected. */
int cilqr_window_scenes_batch(cilqr_handle h, const cilqr_scene_batch* scenes, const double* t0 /* [B] */, double span,
                              int32_t out_samples, double* trajectories /* [B][max_dynamic][out_samples][4] */,
                              int32_t* counts /* [B][max_dynamic] */, int32_t* ok /* [B], optional */,
                              int32_t* n_overflow /* HOST, optional */);

/* ---- scene prediction: a scene at t0 from what was observed by t0 (additive, ABI 7) ----
 * The window hands a cycle that starts at t0 the recording's future.  A caller with perception has the samples up to t0 and
 * nothing else; the prediction rule makes, from those alone, a trajectory on the clock 0 ... span in the layout the scene
 * calls read.  For ONE dynamic obstacle with T samples time x y theta (times taken as non-decreasing), a finite t0, a mode,
 * max_age >= 0, sample_dt > 0 and out_samples >= 2; every operation is rounded once, no product and sum are fused,
 * s[k] = time[k] - t0:
 *   T < 1:  count 0.  Otherwise
 *   J = the first k with 1e-9 < s[k], T if there is none (the window rule's halving over this predicate: defined for any input)
 *   J == 0: nothing has been observed yet.  count 0: the obstacle is unseen, and the scene calls treat it as never there.
 *   j = J - 1 is the latest observation, e = -s[j] its age (>= -1e-9).  e > max_age: count 0 -- the obstacle has left, or
 *       its recording ended before t0.
 *   CILQR_PREDICT_HOLD:               vx = vy = 0
 *   CILQR_PREDICT_CONSTANT_VELOCITY:  j >= 1 and h = time[j] - time[j-1] > 1e-10:  vx = (x[j] - x[j-1]) / h, vy likewise;
 *                                     otherwise vx = vy = 0 (a first sighting stands still)
 *   x0 = x[j] + vx * e,  y0 = y[j] + vy * e:  the position at t0
 *   output sample m = 0 ... out_samples - 1:  tm = (double)m * sample_dt;  (tm, x0 + vx * tm, y0 + vy * tm, theta[j] as bits)
 *       -- the heading is the observed one, never derived from the velocity;  count = out_samples.
 *   A source count that is negative (or, batched, above the source's max_samples) gives count -1, as in the window rule.
 *   Rows of a slot whose count is 0 or -1 are left untouched.  Non-finite samples are no error: the arithmetic decides.
 * The calls also take span and refuse (CILQR_ERR_ARG) unless (double)(out_samples - 1) * sample_dt >= span + 1e-9: the audit
 * calls an obstacle absent when time[T-1] < t, with no epsilon, and the Query...Points rule with its 1e-10.  With the last
 * sample at or past span + 1e-9 the window rule's argument (1e-9 against 1e-10) carries over unchanged: a predicted obstacle
 * is present at every t in [0, span].  (dt = 0.1 and a 5 s horizon: 51 samples do not suffice, 52 do.)
 *
 * cilqr_predict_scene: one scene on the host, no handle (C++ callers use include/cilqr/scene_predict.hpp directly).
 *   trajectories [n_dynamic][out_samples][4], counts [n_dynamic]
 *   *n_refused (optional): the obstacles with count -1 (a negative source count: the obstacle is refused, its neighbours
 *                          are predicted, and it takes no samples of the packed array)
 * CILQR_ERR_NULL; CILQR_ERR_ARG for a non-finite t0, a span that is non-finite or negative, n_dynamic < 0, an unknown mode,
 * a max_age that is negative or not finite, a sample_dt that is not positive or not finite, out_samples < 2 and the span
 * condition. */
#define CILQR_PREDICT_HOLD 0
#define CILQR_PREDICT_CONSTANT_VELOCITY 1
int cilqr_predict_scene(const cilqr_scene* scene, double t0, double span, int32_t mode, double max_age, double sample_dt,
                        int32_t out_samples, double* trajectories /* [n_dynamic][out_samples][4] */,
                        int32_t* counts /* [n_dynamic] */, int32_t* n_refused);
/* ---- the same for B scenes per call, each at its own t0, on the GPU (kernels_scene_predict.hip) ----
 * A cilqr_scene_batch with dynamic_trajectories = `trajectories`, dynamic_trajectory_counts = `counts`, max_samples =
 * out_samples and every other member as in `scenes` is the predicted batch; nothing but t0 crosses to the device per cycle.
 * scenes->max_samples may be any positive value (CILQR_ERR_CAPACITY for out_samples beyond CILQR_DP_MAX_SAMPLES).
 *   t0           [B]                                     (memory as scenes->memory, like the three arrays below)
 *   trajectories [B][max_dynamic][out_samples][4]        rows of a slot with count 0 or -1 are left untouched
 *   counts       [B][max_dynamic]                        out_samples, 0 or -1
 *   ok           [B] 1 / 0, optional (NULL to skip): 0 where one of the scene's counts is -1
 *   *n_refused   (HOST, optional): the scenes with ok = 0
 * One wavefront per (scene, slot); J comes from the wave's joint search (64 probes and one ballot per round), which returns
 * what the halving returns on non-decreasing times.  On times that decrease the wave's J may differ from the halving's and
 * the bits with it; every index read still lies in [0, T).  Otherwise every element is the host call's bit for bit; a
 * scene's prediction does not depend on the batch around it; no alignment beyond a double's is assumed.  Stream, work space
 * and checks as for cilqr_window_scenes_batch, plus the checks on mode, max_age, sample_dt, out_samples and span above:
 * HOST arrays with a non-finite t0[b] or a bad source count are refused with CILQR_ERR_ARG before anything is launched;
 * with DEVICE arrays they give every slot of that scene the count -1 and ok 0, the other scenes are unaffected. */
int cilqr_predict_scenes_batch(cilqr_handle h, const cilqr_scene_batch* scenes, const double* t0 /* [B] */, double span,
                               int32_t mode, double max_age, double sample_dt, int32_t out_samples,
                               double* trajectories /* [B][max_dynamic][out_samples][4] */,
                               int32_t* counts /* [B][max_dynamic] */, int32_t* ok /* [B], optional */,
                               int32_t* n_refused /* HOST, optional */);

/* ---- carry:the plan of the previous cycle as the coarse trajectory of the next (additive, ABI 7) ----
 * A later planning cycle need not search the lattice again: the plan of cycle n, read from the time the vehicle has reached,
 * is a coarse trajectory for cycle n + 1 as long as it still clears the obstacles on the new clock.  The carry rule makes that
 * coarse trajectory -- DiscretizedTrajectory::EvaluateTime at the knot times of the new cycle -- in the four forms
 * cilqr_dp_plan_batch returns.  For ONE trajectory of n_rows >= 2 rows in CILQR_ROWS_TRAJ / _PLAN / _COARSE, an `advance` in
 * seconds (the time driven since the rows' time[0]), max_advance, n_knots >= 1 and delta_t > 0; every operation is rounded
 * once (no fused multiply-add):
 *   state 1 (CILQR_CARRY_NOT_ASKED)   advance < 0.  Every output row is zero.
 *   state 2 (CILQR_CARRY_REFUSED)     advance is a NaN or above max_advance; or !(time[n_rows-1] - time[0] > 0) -- the all-zero
 *                                     rows a failed tracker leaves, NaN times --; or any coarse6 column of any row produced
 *                                     below is not finite.  Every output row is zero.
 *   state 0 (CILQR_CARRY_KEPT)        otherwise.  q_k = (time[0] + advance) + k * delta_t;  r_k = the resample rule above with
 *                                     CILQR_KEY_TIME at q_k (its extrapolation past the last row, its degenerate pair and its
 *                                     slerp included);  coarse9 row k = delta_t * k, s_k, r.x, r.y, r.theta, r.kappa,
 *                                     r.velocity, r.a, r.delta with s_0 = 0, s_k = s_{k-1} + hypot(x_k - x_{k-1}, y_k - y_{k-1})
 *                                     summed in knot order (the hypot of the `plan` rows of cilqr_plan_scenes_batch);
 *                                     coarse6, knots3 and station are the projections cilqr_dp_plan_batch writes.
 *   columns read   CILQR_ROWS_TRAJ x 1 y 2 theta 3 v 4 a 5 delta 6 kappa 7;  CILQR_ROWS_PLAN and _COARSE x 2 y 3 theta 4
 *                  kappa 5 v 6 a 7 delta 8.  (The code takes these numbers from include/cilqr/row_layouts.hpp through
 *                  trajectory_queries.hpp: carry_columns.)
 * cilqr_carry_rows: one trajectory on the host, no handle (C++ callers use include/cilqr/trajectory_queries.hpp: carry_rows).
 *   coarse9 [n_knots][CILQR_COARSE_FIELDS], coarse6 [n_knots][6], knots3 [n_knots][3], station [n_knots]: each optional
 * CILQR_ERR_NULL (rows, state); CILQR_ERR_ARG for an unknown layout, n_rows < 2, n_knots < 1, a delta_t that is not positive,
 * a max_advance that is negative or not finite; CILQR_ERR_CAPACITY for n_rows or n_knots > CILQR_DP_MAX_KNOTS. */
#define CILQR_CARRY_KEPT 0
#define CILQR_CARRY_NOT_ASKED 1
#define CILQR_CARRY_REFUSED 2
#define CILQR_CARRY_OFF_START 3   /* cilqr_plan_scenes_batch_carry only, like the next */
#define CILQR_CARRY_HIT 4
int cilqr_carry_rows(int32_t layout, const double* rows, int32_t n_rows, double advance, double max_advance,
                     int32_t n_knots, double delta_t, double* coarse9, double* coarse6, double* knots3, double* station,
                     int32_t* state);
/* ---- the same for B trajectories per call, each with its own advance, on the GPU (kernels_carry.hip) ----
 *   rows [B][n_rows][fields], advance [B], coarse9 / coarse6 / knots3 / station [B][n_knots][9 | 6 | 3 | 1] (each optional),
 *   state [B]: all in `memory`; *n_kept (HOST, optional): the trajectories with state 0
 * A workgroup takes a run of whole trajectories: their rows are staged in LDS once, the (trajectory, knot) pairs are spread
 * over the lanes, which bracket and interpolate there, the test for a non-finite value is one ballot per wavefront, the
 * running station one lane's sum per trajectory over chord lengths in LDS, and the four outputs leave as consecutive
 * doubles.  Every element is the host call's bit for bit (the kernel is built without
 * contraction, wraps angles with the routine of cilqr_device_math fn 6 and takes the hypot of fn 9); a trajectory's bits do
 * not depend on the batch around it; nothing beyond the alignment of a double is assumed.  Runs on the handle's stream and
 * waits for that stream only; DEVICE arrays need no work space beyond the count, HOST arrays are staged in blocks that belong
 * to the handle and grow to the largest call.  Checked before anything is launched, the handle staying usable:
 * CILQR_ERR_NULL (handle, rows, advance, state); CILQR_ERR_ARG for batch < 1, an unknown memory flag and what the host call
 * refuses; CILQR_ERR_CAPACITY as there; CILQR_ERR_STATE while solves are submitted on the handle. */
int cilqr_carry_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_rows,
                           const double* advance, double max_advance, int32_t n_knots, double delta_t, double* coarse9,
                           double* coarse6, double* knots3, double* station, int32_t* state, int32_t* n_kept,
                           int32_t memory);

/* ---- the pipeline of a later cycle: carried plans where they hold, the DP planner where they do not ----
 * cilqr_plan_scenes_batch_warm with the DP planner run for exactly the scenes that need it.
 *   1. carry    cilqr_carry_rows_batch on carry->rows / carry->advance with the planner's delta_t, for the path samples the
 *               planner fills (all n_knots rows with the default configuration; rows past them are zero, as the planner
 *               leaves them);
 *   2. audit    cilqr_check_collisions_batch (CILQR_ROWS_COARSE, the carried coarse9, carry->collision_buffer);
 *   3. select   source[b], first match wins: CILQR_CARRY_NOT_ASKED (state 1), CILQR_CARRY_REFUSED (state 2),
 *               CILQR_CARRY_OFF_START  !(hypot(start.x - row0.x, start.y - row0.y) <= carry->max_start_offset),
 *               CILQR_CARRY_HIT  first_hit[b] != -1 (the audit's -2 included), CILQR_CARRY_KEPT otherwise.  The scenes with
 *               a non-zero source are listed in ascending order (ballots, population counts and a prefix over wavefronts
 *               decide the positions, never an atomic);
 *   4. plan     cilqr_dp_plan_batch for the listed scenes alone: nothing for an empty list; the batch as it lies when all
 *               are listed; otherwise the listed scenes are gathered, CILQR_OPT_SCENE_CHUNK (or what fits a byte cap) at a
 *               time, planned, and their rows and `found` written over the carried ones.  A kept scene has found = 1;
 *   5. the rest as in cilqr_plan_scenes_batch_warm: obstacle points at the planner's time axis, corridors, outcome, the
 *               solve (`warm` may be NULL and is independent of `carry`), the plan rows.  coarse9 returns the merged coarse
 *               trajectories.
 * The results are, bit for bit, those of the public calls made one after the other: cilqr_carry_rows_batch,
 * cilqr_check_collisions_batch, the selection above, cilqr_dp_plan_batch on the listed scenes as a batch of their own with
 * the same max_*, the merge, cilqr_scene_points_batch, cilqr_build_corridors, cilqr_solve_batch_warm.  With carry == NULL or
 * every advance < 0 the call is cilqr_plan_scenes_batch_warm bit for bit.
 *   source [B], optional (memory as scenes->memory); *n_kept (HOST, optional): the scenes with source 0
 * Checked with the others, before anything is launched: CILQR_ERR_NULL for NULL rows or advance; CILQR_ERR_ARG for an unknown
 * layout, a memory flag that differs from scenes->memory, n_rows < 2, a max_advance, max_start_offset or collision_buffer
 * that is negative or not finite; CILQR_ERR_CAPACITY for n_rows > CILQR_DP_MAX_KNOTS. */
typedef struct cilqr_carry {   /* the previous cycle's rows, for the B scenes in their order */
  int32_t memory, layout;      /* memory must equal scenes->memory; CILQR_ROWS_TRAJ / _PLAN / _COARSE */
  int32_t n_rows, reserved0;
  const double* rows;          /* [B][n_rows][fields] */
  const double* advance;       /* [B] seconds driven since those rows' time[0]; < 0: plan this scene with the DP planner */
  double max_advance, max_start_offset, collision_buffer;
} cilqr_carry;
int cilqr_plan_scenes_batch_carry(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                                  const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots,
                                  const cilqr_carry* carry, const cilqr_warm_start* warm, cilqr_solution_batch* out,
                                  double* plan, double* coarse9, int32_t* outcome, int32_t* source /* [B], optional */,
                                  int32_t* n_dp_failed, int32_t* n_corridor_failed, int32_t* n_kept);

/* ---- stop: brake along a path that is already trusted (additive, ABI 7) ----
 * Where a cycle's plan is refused -- the audit calls it hit, the carried plan no longer clears, the planner found no path --
 * a caller keeps the path it has and takes the speed off it: the vehicle brakes along the path and comes to rest.  The stop
 * rule makes such rows for one trajectory and one braking profile; a caller orders its profiles gentlest first and takes the
 * first that stops clear (cilqr_stop_scenes_batch below).  Every operation is rounded once (no fused multiply-add).
 *   inputs      n_knots >= 2 rows in CILQR_ROWS_TRAJ / _PLAN / _COARSE; a profile (a_target, jerk), a_target <= 0, jerk < 0,
 *               both finite; delta_t > 0; n_out in 1 ... CILQR_DP_MAX_KNOTS; optionally start_va = (v0, a0), which replaces
 *               the velocity and a columns of row 0 (else v0, a0 are those columns).
 *   station key   _PLAN and _COARSE: the layout's station column.  _TRAJ (which has none): key_0 = 0, key_i = key_{i-1} +
 *               hypot(x_i - x_{i-1}, y_i - y_{i-1}) in knot order (the hypot of the `plan` rows and of "carry").
 *               s_end = key[n_knots-1].
 *   speed chain   (s_0, v_0, a_0) = (key_0, v0, a0); with jd = jerk * delta_t and hd = 0.5 * delta_t, step k -> k + 1:
 *               if v == 0:           s, v stay, a' = 0;
 *               otherwise            a' = max(a + jd, a_target) if a > a_target,  min(a - jd, a_target) if a < a_target,
 *                                    a_target else;      vn = v + hd * (a + a');
 *                   if !(vn > 0)     (the stop lies inside the step)  f = v / (v - vn);  s = s + (0.5 * v) * (f * delta_t);
 *                                    v = 0;  a = 0;
 *                   otherwise        s = s + hd * (v + vn);  v = vn;  a = a'.
 *   row k       always CILQR_ROWS_PLAN (11 columns), k = 0 ... n_out - 1:
 *               time       time[0] + delta_t * k;
 *               s          q_k = s_end if s_k > s_end, else s_k;
 *               x y theta kappa delta    the resample rule above with CILQR_KEY_STATION at q_k on the station key -- its
 *                          bracket, its degenerate pair (p0's bits) and its slerp included; delta is interpolated, never
 *                          recomputed from kappa, so no transcendental enters the rule;
 *               velocity, a    v_k, a_k;
 *               jerk       (a_{k+1} - a_k) / delta_t,   delta_rate  (delta_{k+1} - delta_k) / delta_t;  both 0 in the last row.
 *   status      first match wins:
 *               CILQR_STOP_REFUSED   v0 or a0 is not finite, v0 < 0, or any column of any row produced is not finite.  Every
 *                                    row is zero, stop_knot = -1, travel = 0.
 *               CILQR_STOP_OVERRUN   some s_k > s_end (the path is shorter than the stop).
 *               CILQR_STOP_MOVING    v_{n_out-1} > 0.
 *               CILQR_STOP_STOPPED   otherwise.
 *   stop_knot   the first k with v_k == 0, -1 if there is none;  travel = s_{n_out-1} - key_0, not clamped.
 * The rows are kinematic, like the DP planner's: the jump of a to 0 at the stop shows in jerk.  cilqr_track_rows_batch makes
 * them drivable, cilqr_constraint_margins_batch measures how far they overshoot the bounds.
 * cilqr_stop_rows: one trajectory and n_profiles profiles on the host, no handle (C++ callers use
 * include/cilqr/trajectory_queries.hpp: stop_rows).
 *   profiles [n_profiles][2] a_target, jerk;  start_va [2] or NULL;  out_rows [n_profiles][n_out][CILQR_PLAN_FIELDS],
 *   status / stop_knot / travel [n_profiles]: each output optional, not all of them
 * CILQR_ERR_NULL (rows, profiles); CILQR_ERR_ARG for an unknown layout, n_knots < 2, n_out < 1, n_profiles outside 1 ...
 * CILQR_STOP_MAX_PROFILES, a profile outside its domain, a delta_t that is not positive, every output NULL;
 * CILQR_ERR_CAPACITY for n_knots or n_out > CILQR_DP_MAX_KNOTS. */
#define CILQR_STOP_STOPPED 0
#define CILQR_STOP_MOVING 1
#define CILQR_STOP_OVERRUN 2
#define CILQR_STOP_REFUSED 3
#define CILQR_STOP_MAX_PROFILES 8
int cilqr_stop_rows(int32_t layout, const double* rows, int32_t n_knots, int32_t n_profiles, const double* profiles,
                    const double* start_va, double delta_t, int32_t n_out, double* out_rows, int32_t* status,
                    int32_t* stop_knot, double* travel);
/* ---- the same for B trajectories per call, on the GPU (kernels_stop.hip) ----
 *   rows [B][n_knots][fields], start_va [B][2] or NULL, in `memory`; profiles [n_profiles][2], HOST memory;
 *   out_rows [n_profiles][B][n_out][CILQR_PLAN_FIELDS], status / stop_knot / travel [n_profiles][B], in `memory`: each
 *   optional, not all of them
 * The outputs are profile-major on purpose: slice m is an ordinary batch of B CILQR_ROWS_PLAN trajectories and feeds
 * cilqr_check_collisions_batch, cilqr_clearance_rows_batch, cilqr_constraint_margins_batch, cilqr_resample_rows_batch,
 * cilqr_track_rows_batch and a warm start where it lies.  A workgroup takes a run of whole trajectories: their rows and
 * station keys are staged in LDS once and shared by all profiles, one lane per (trajectory, profile) runs the speed chain
 * into an LDS image of the rows, the (profile, knot) pairs are spread over the lanes, which bracket and interpolate there,
 * the controls are differenced from the neighbouring row of the image, the test for a non-finite value is one ballot per
 * wavefront, and the rows leave as consecutive doubles; an image that does not fit the workgroup's LDS is produced in chunks
 * of knots.  Every element is the host call's bit for bit (the kernel is built without contraction, wraps angles with the
 * routine of cilqr_device_math fn 6 and takes the hypot of fn 9); a chain's bits depend neither on the batch nor on the
 * profiles around it; nothing beyond the alignment of a double is assumed.  Runs on the handle's stream and waits for that
 * stream only; DEVICE arrays need no work space, HOST arrays are staged in blocks that belong to the handle and grow to the
 * largest call.  Checked before anything is launched, the handle staying usable: CILQR_ERR_NULL (handle, rows, profiles);
 * CILQR_ERR_ARG for batch < 1, an unknown memory flag and what the host call refuses; CILQR_ERR_CAPACITY as there;
 * CILQR_ERR_STATE while solves are submitted on the handle. */
int cilqr_stop_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                          int32_t n_profiles, const double* profiles, const double* start_va, double delta_t, int32_t n_out,
                          double* out_rows, int32_t* status, int32_t* stop_knot, double* travel, int32_t memory);
/* ---- the pipeline: for every scene the gentlest profile that stops clear ----
 *   1. stop     cilqr_stop_rows_batch for all n_profiles profiles, into the handle's work space;
 *   2. audit    cilqr_check_collisions_batch (CILQR_ROWS_PLAN, collision_buffer) on each slice;
 *   3. choose   choice[b] = the smallest m with status[m][b] == CILQR_STOP_STOPPED and first_hit[m][b] == -1; -1 if there is
 *               none (the caller orders the profiles gentlest first);
 *   4. gather   out_rows[b] = slice choice[b], or slice n_profiles - 1 where choice[b] is -1 (a small kernel, no atomics).
 * The results are, bit for bit, those of the public calls made one after the other.
 *   rows, start_va (optional), out_rows [B][n_out][CILQR_PLAN_FIELDS], choice [B], status / first_hit [n_profiles][B]
 *   (optional): memory as scenes->memory;  profiles: HOST memory;  *n_none (HOST, optional): the scenes with choice -1
 * The checks are those of the two calls, all made before anything is launched (out_rows and choice may not be NULL). */
int cilqr_stop_scenes_batch(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_scene_batch* scenes, int32_t layout,
                            const double* rows, int32_t n_knots, int32_t n_profiles, const double* profiles,
                            const double* start_va, double delta_t, int32_t n_out, double collision_buffer,
                            double* out_rows, int32_t* choice, int32_t* status, int32_t* first_hit, int32_t* n_none);

/* ---- several GPUs from ONE host process (the reference's caller is one process:
 * algorithm/planning_node.cc:9-31) ----
 * A multi handle owns one solver handle per listed device.  cilqr_multi_solve cuts the batch into contiguous shards
 * (the first batch % n shards hold one problem more), solves them concurrently -- each shard on its own device,
 * stream and host threads -- and every shard writes its results into the caller's arrays at its offset: problem order
 * is preserved, nothing is copied between devices, results are bit-identical to one cilqr_solve_batch over the whole
 * batch.  `devices` may list a device more than once (logical shards on one GPU).  The arrays of `in` / `out` must be
 * reachable from every listed device: host memory (CILQR_MEM_HOST), or device memory when all shards share the
 * device that holds it.  One lane table per call (n_lane_groups <= 1).  batch_capacity is for all shards together. */
typedef struct cilqr_multi* cilqr_multi_handle;
int cilqr_multi_create(const cilqr_config* cfg, const int32_t* devices, int32_t n_devices, int32_t batch_capacity,
                       int32_t cmax, int32_t max_lane_segments, cilqr_multi_handle* out);
int cilqr_multi_destroy(cilqr_multi_handle m);
int cilqr_multi_solve(cilqr_multi_handle m, const cilqr_problem_batch* in, cilqr_solution_batch* out);
/* ... with a warm start (see cilqr_solve_batch_warm); its arrays are cut into the same shards */
int cilqr_multi_solve_warm(cilqr_multi_handle m, const cilqr_problem_batch* in, const cilqr_warm_start* warm,
                           cilqr_solution_batch* out);
/* cilqr_set_option on every shard */
int cilqr_multi_set_option(cilqr_multi_handle m, int32_t option, int64_t value);
/* the split of a batch: first problem and device of every shard (arrays of max_shards entries, NULL to skip);
 * returns the number of shards */
int cilqr_multi_shards(cilqr_multi_handle m, int32_t batch, int32_t* first_problem, int32_t* device, int32_t max_shards);
int64_t cilqr_multi_device_bytes(cilqr_multi_handle m);

/* ---- a stream of batches on ONE GPU: several handles dealt out round-robin ----
 * cilqr_submit overlaps the latency-bound end of a solve with the bulk of the next one.  What stays idle then is inside
 * the bulk itself (a backward pass or a rollout is one lane per problem: N dependent steps on a fraction of the chip once
 * the active set has shrunk); other solves' cost kernels fit there.  A pool owns n_handles handles on one device
 * (n_handles x the memory of one; 1..16) and runs submitted solve s on handle s % n_handles: up to 3 x n_handles solves
 * submitted (two in flight and one queued per handle, see cilqr_submit), cilqr_pool_wait collects the OLDEST.  Keep it fed:
 *     for (i = 0; i < depth; ++i) submit(batch[i]);   then   wait(); submit(next); wait(); submit(next); ...
 * The rules of cilqr_submit hold per solve (structs copied, arrays valid and distinct until the wait that collects them; a
 * submit beyond the depth returns CILQR_ERR_STATE).  Results are bit-identical to cilqr_solve_batch.  Measured on the
 * bench workload (65536 problems per batch): 1.69-1.72 M solves/s with one handle, 1.94-1.99 M with two, 1.97-2.00 M with three.
 * cilqr_pool_set_option: cilqr_set_option on every handle (nothing in flight); cilqr_pool_get_profile: of the solve
 * the last wait collected; cilqr_pool_destroy waits for whatever is still in flight.  Solves may also be submitted to a
 * handle of the pool directly (cilqr_pool_handle_at) as long as the pool itself is empty meanwhile.  Like a handle, a pool
 * is driven by one host thread at a time (its handles run their own worker threads). */
typedef struct cilqr_pool* cilqr_pool_handle;
int cilqr_pool_create(const cilqr_config* cfg, int32_t device, int32_t n_handles, int32_t batch_capacity, int32_t cmax,
                      int32_t max_lane_segments, cilqr_pool_handle* out);
int cilqr_pool_destroy(cilqr_pool_handle p);
int cilqr_pool_submit(cilqr_pool_handle p, const cilqr_problem_batch* in, cilqr_solution_batch* out);
int cilqr_pool_submit_warm(cilqr_pool_handle p, const cilqr_problem_batch* in, const cilqr_warm_start* warm,
                           cilqr_solution_batch* out);   /* see cilqr_solve_batch_warm */
int cilqr_pool_wait(cilqr_pool_handle p);
int32_t cilqr_pool_depth(cilqr_pool_handle p);   /* 3 x n_handles */
/* handle k (0 <= k < n_handles) for what the pool has no call of its own for -- cilqr_set_profiling, cilqr_set_stream, a
 * synchronous cilqr_solve_batch, the stage entry points; NULL while solves are in flight on the pool.  Owned by the pool. */
cilqr_handle cilqr_pool_handle_at(cilqr_pool_handle p, int32_t k);
int cilqr_pool_set_option(cilqr_pool_handle p, int32_t option, int64_t value);
int cilqr_pool_get_profile(cilqr_pool_handle p, cilqr_profile* out);
int64_t cilqr_pool_device_bytes(cilqr_pool_handle p);

/* ---- multi-GPU (nothing in the single-process reference to replace) ----
 * One process per GPU.  Problems are independent: rank r solves a contiguous block of `batch` problems with
 * its own handle and no communication; ONE gather then moves the results to a root rank through RCCL
 * (grouped ncclSend / ncclRecv, point-to-point over xGMI).  librccl.so.1 is loaded on the first call --
 * libcilqr_hip.so does not link against it.
 *   rank 0:      cilqr_comm_unique_id(id)  ->  ship the 128 bytes to every rank (any transport)
 *   every rank:  cilqr_comm_create(h, id, rank, world)          (collective: ncclCommInitRank)
 *   every step:  cilqr_solve_batch(h, ...)  then  cilqr_gather_results(h, batch, &local, root, &gathered)
 * Travelling per rank: 8 of the 10 trajectory columns (time and kappa are rebuilt on the root with the
 * expressions of TransformToTrajectory, ilqr_optimizer.cc:771-791 -- bit-identical to a local export),
 * the LIVE Cost rows only (n_cost[b] of the max_iter + 1), n_cost, status, n_iter.
 * `local` and `gathered` must be CILQR_MEM_DEVICE; `gathered` (root only, NULL elsewhere) holds
 * world * batch problems in rank order: traj [world*batch][K][10], cost_hist [world*batch][max_iter+1][5]
 * (rows >= n_cost untouched), n_cost, status, n_iter (optional).  iter_trajs / alpha_trace do not travel.
 * Every rank passes the same `batch` and `root`.  The library checks the batch where every rank takes part in the
 * check: at a communicator's first gather, and at any gather for which every rank's batch differs from the batch last
 * agreed on (all ranks moving to another batch together) -- ranks that disagree there get CILQR_ERR_ARG on every rank,
 * nothing is written to `gathered`, and the communicator stays usable.  Beyond that, equal batches are a precondition:
 * one rank that alone changes its batch between gathers breaks it, and the outcome under RCCL is undefined. */
#define CILQR_UNIQUE_ID_BYTES 128
int cilqr_comm_unique_id(uint8_t* id /* [CILQR_UNIQUE_ID_BYTES] */);
int cilqr_comm_create(cilqr_handle h, const uint8_t* id, int32_t rank, int32_t world);
int cilqr_comm_destroy(cilqr_handle h);
int cilqr_comm_info(cilqr_handle h, int32_t* rank, int32_t* world);
int cilqr_gather_results(cilqr_handle h, int32_t batch, const cilqr_solution_batch* local, int32_t root,
                         cilqr_solution_batch* gathered);

const char* cilqr_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif /* CILQR_H_ */
