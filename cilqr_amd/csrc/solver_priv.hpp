// Private to cilqr_amd/csrc: the solver handle behind `cilqr_handle` (include/cilqr.h) and the
// error-reporting macro shared by the translation units that implement the C-ABI.
#pragma once
#include <atomic>

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/cilqr.h"
#include "hip_owned.hpp"
#include "solve_io.hpp"
#include "state.hpp"

extern thread_local char g_last_hip_error[256];

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      std::snprintf(g_last_hip_error, sizeof(g_last_hip_error), "%s -> %s", #expr, \
                    hipGetErrorString(e_));                                        \
      return CILQR_ERR_DEVICE;                                                     \
    }                                                                              \
  } while (0)

struct cilqr_comm;   // comm.hip: RCCL communicator + staging of cilqr_gather_results

// Entry points that create or destroy handles on SEVERAL devices (cilqr_multi_*, cilqr_pool_*) leave the calling thread's
// current HIP device as they found it.
struct cilqr_device_guard {
  int dev = -1;
  cilqr_device_guard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
  ~cilqr_device_guard() { if (dev >= 0) (void)hipSetDevice(dev); }
  cilqr_device_guard(const cilqr_device_guard&) = delete;
  cilqr_device_guard& operator=(const cilqr_device_guard&) = delete;
};

// What ONE solve in flight owns besides the arenas: the tensors indexed by PROBLEM (they outlive the hand-over of
// the survivors to the finishing arena and are read by the final export), the lane tables it was loaded with,
// its host-visible iteration counters and its events.  A handle has two of these, so that the finishing stage of
// solve i and the first stage of solve i+1 can be in flight together.
struct cilqr_job_set {
  double* hist = nullptr;
  int *iter = nullptr, *status = nullptr, *n_cost = nullptr, *n_iter_trajs = nullptr;
  signed char* atrace = nullptr;
  double* lanes = nullptr;
  unsigned char* lgrid = nullptr;
  double* lanes_raw = nullptr;      // device [2*smax][7]
  std::vector<double> lane_cache;   // the lane tables whose device image and grid are current (left rows, then right rows)
  int lane_cache_nl = -1, lane_cache_nr = -1;
  cilqr::pinned_mem h_count;        // int, mapped: written by k_update through h_count_dev
  int* h_count_dev = nullptr;
  int* tail_iter_dev = nullptr;     // largest iteration count reached inside the tail kernel
  // host arrays (CILQR_MEM_HOST) on the way out: the staging of ONE solve in flight (the way in: cilqr_in_buffer)
  cilqr::dev_mem out_stage;         // problem-major results on the device when the caller's buffers are host memory
  cilqr::pinned_mem out_pinned;     // small host batches: the staging block lands here in one copy
  cilqr::dev_mem row_off;           // long long [B + 1]: first packed Cost row of every problem, total (large host batches)
  cilqr::pinned_mem host_counts;    // n_cost | status | n_iter | n_iter_trajs of a large host batch
  cilqr::pinned_mem host_rows;      // its LIVE Cost rows, packed (scattered into the caller's dense array on the host)
  cilqr::hip_event exported;        // recorded on the solve's stream behind its last kernel (what the download stream waits for)
  std::vector<cilqr::hip_event> iter_ev;  // one per lockstep iteration (count read-back)
  std::vector<cilqr::hip_event> ev;       // profiling
  cilqr::hip_event handoff;         // survivors copied into the finishing arena (recorded on the first stage's stream)
  cilqr::hip_event sync_ev;         // what a relaxed host wait for a whole stream polls (solver.hip: wait_stream)
  // warm start: int [B], the shift of every problem of the load in force (0 where the caller gave no array), written by the
  // gather kernel for the init-guess launches behind it -- the caller's own array, staged, is given back with the load
  cilqr::dev_mem warm_shift;
};

struct cilqr_timer {  // event pairs around kernels / phases, resolved after the final sync
  cilqr_solver* h = nullptr;
  cilqr_job_set* js = nullptr;
  hipStream_t stream = nullptr;     // where the next events are recorded (changes at the hand-over)
  size_t next = 0;
  std::vector<int> kind;  // 0 quad, 1 backward, 2 linesearch, 3 other, 4 tail
  std::vector<char> full_flags, live_flags;  // per backward launch: covered the whole batch / had work
  bool open = false;   // the last begin() recorded an event, so the matching end() must too
  bool marked = false; // the last begin() opened a roctx range (CILQR_ROCTX=1), so the matching end() closes it
  bool on() const;
  bool wants(int k) const;
  int reserve();
  int begin(int k);
  int pair(int k, hipEvent_t* a, hipEvent_t* b);
  int end();
  void resolve(cilqr_profile* p);
};

// Host arrays on the way in: a problem-major copy of the caller's inputs on the device.  A buffer belongs to a solve from the
// start of its upload until its load kernels are enqueued; two of them, so that the arrays of the NEXT solve travel while this
// one iterates (solver.hip: worker_io_main).
struct cilqr_in_buffer {
  cilqr::dev_mem p;
  cilqr::hip_event ready;        // recorded on the upload stream behind the last input copy
  cilqr::hip_event loaded;       // recorded on the solve's stream behind the load kernels that read the buffer
  int state = 0;                 // 0 free; 1 owned by a solve; 2 given back: free once `loaded` has happened
};

// Solves a handle accepts before the oldest is collected: two in flight (first stage / finishing stage) and one more, queued,
// whose host arrays are uploaded meanwhile -- without it the main arena would sit idle for the length of an upload between
// two solves (26 ms of a 33 ms step on the bench workload, measured: 1.40 M solves/s from host arrays against 1.98 M).
constexpr int kJobRing = 3;

// One solve on its way through the handle: first stage (load, init guess, the lockstep iterations over the bulk of
// the batch, in the main arena), hand-over of the survivors, finishing stage (remaining lockstep iterations + the
// per-problem tail kernel in the small finishing arena, final export).
struct cilqr_job {
  cilqr_problem_batch in;
  cilqr_solution_batch out;
  cilqr_warm_start warm;    // has_warm only: the warm start of this solve (cilqr_submit_warm; copied like `in`)
  bool has_warm = false;
  int set = 0;              // the cilqr_job_set it runs on: taken when its first stage starts, given back when it is done
  int spec_threshold = 0;   // the threshold of this solve (cilqr_solver::spec_threshold or spec_threshold_submit)
  int tail_threshold = 0;   // likewise (cilqr_solver::tail_threshold or tail_threshold_submit)
  size_t tail_lds_limit = 0;   // cilqr_solver::tail_lds_limit when the solve was handed in
  int phase = 0;            // 0 free, 1 queued, 2 first stage, 3 waiting for the finishing stage, 4 finishing, 5 done
  int rc = CILQR_OK;
  char err_text[256] = "";  // what the worker thread's g_last_hip_error held when rc was set (that variable is thread-local)
  hipStream_t st1 = nullptr, st2 = nullptr;
  cilqr::DeviceState gmain;   // main arena with this job's problem-indexed tensors and lane tables
  cilqr::DeviceState d, o;    // the arena the active problems live in, and its twin
  int B = 0, it = 0, n_hint = 0, span = 0;
  bool handed = false;      // the survivors live in the finishing arena
  bool owns_fin = false;    // this solve holds the finishing arena / the tail workspace (cilqr_solver::fin_busy)
  bool tail_used = false;
  int tail_n = 0;
  bool first_quad = false;  // job_begin's fused pass has left lin / term of the first iterate in d: iteration 0 does not quadratise
  std::vector<int> bwd_iter;  // iteration index of every profiled backward launch
  cilqr_timer tm;
  cilqr_profile prof;
  // where the kernels write the results (the caller's device buffers, or the staging of the job set) and how they travel
  cilqr::solve_outputs res;
  bool relaxed_wait = false;  // the host waits of this solve poll and nap instead of spinning (solver.hip: wait_event)
  // Host inputs of a submitted solve travel ahead of it: the handle's transfer thread (solver.hip: worker_io_main) copies
  // them into the job set's staging on a stream of its own as soon as the solve is SUBMITTED, i.e. while the solve before it
  // still iterates; the first stage then only waits for the event behind the last copy.  upload: 0 = not delegated (device
  // inputs, a small batch, the synchronous call: staged inline by the solving thread), 1 = queued, 2 = being copied,
  // 3 = every copy enqueued and the event recorded, -1 = failed (upload_rc).
  int upload = 0;
  int upload_rc = CILQR_OK;
  cilqr::ProblemView pv;      // where the staged inputs lie (filled by whoever staged them)
  cilqr::WarmView wv;         // ... and the warm rows (rows == nullptr: none)
  bool past_load = false;     // its inputs are staged and its load kernels enqueued (or it failed before): the transfer thread may
                              // upload for the solve behind it
  int in_buf = -1;            // the cilqr_in_buffer they lie in (-1: the caller's own device arrays)
  bool io_busy = false;       // the transfer thread still works for this solve (upload, zero fill of the caller's cost_hist)
  bool io_taken = false;      // ... and has picked it up
  bool zero_by_io = false;    // large host outputs of a submitted solve: the transfer thread clears the caller's cost_hist
  bool zero_inline = false;   // large host outputs of a solve without the transfer thread: the solving thread clears cost_hist
};

struct cilqr_solver {
  cilqr_config cfg;
  int device = 0;
  int Bcap = 0, capacity = 0, cmax = 0, smax = 0;
  cilqr::DeviceState ds;      // arena A (also what the stage API works on)
  cilqr::DeviceState twin;    // arena B: only the fields k_compact moves are its own, the rest alias ds
  // finishing arena (capacity fin_cap slots) and its twin: where a solve continues once few enough problems are
  // left, so that the main arena is free for the next solve (cilqr_submit) while the stragglers finish
  cilqr::DeviceState fin, fin_twin;
  int fin_cap = 0;
  // first-knot cache of the main arena (DeviceState::knot0).  Kept out of `ds`, whose views the stage API uses: a solve's view
  // gets it in job_begin.  use_knot0 / fuse_first: test hooks, CILQR_NO_KNOT0_CACHE / CILQR_NO_FUSED_FIRST at cilqr_create.
  double2* knot0_main = nullptr;
  bool use_knot0 = true;
  bool fuse_first = true;
  int fin_threshold = 0;     // hand the survivors over at this active count (CILQR_OPT_FINISH_THRESHOLD); 0 = never
  bool compaction = true;
  int compact_percent = 75;  // re-pack when the survivors fill at most this share of the occupied slots
  // (the streams are declared before every other owner: the handle's memory and events are released first)
  cilqr::hip_stream own_stream;
  hipStream_t stream = nullptr;
  cilqr::hip_stream stream2;     // finishing stage of asynchronous solves (high priority: short, latency-bound kernels)
  cilqr::hip_stream stream_in;   // host arrays: uploads of submitted solves (the transfer thread), beside the solves' kernels
  cilqr::hip_stream stream_out;  // host arrays: downloads of finished solves, so that the next solve's kernels need not queue behind them
  std::vector<cilqr::dev_mem> allocs;   // the arenas and the job sets' tensors (cilqr_create)
  int64_t bytes = 0;
  // the lazily grown device blocks (staging, tail workspaces): their sizes belong to the thread that grows them; what another
  // thread may ask for at any time -- cilqr_device_bytes -- is this sum, kept by hip_mem::grow (found by the ThreadSanitizer
  // run of tools/tsan_run.sh: the sizes themselves used to be read there)
  std::atomic<int64_t> grown_bytes{0};
  cilqr::dev_mem in_small;          // small host batches: their device block (the large ones: in_bufs)
  cilqr::pinned_mem in_pinned;      // small host batches: the input arrays leave from here in one copy
  cilqr::hip_event in_pinned_ev;
  cilqr_job_set sets[2];
  bool set_busy[2] = {false, false};   // (under mu) a submitted solve runs on the set
  cilqr_in_buffer in_bufs[2];
  double* lambda_stage = nullptr;
  int B = 0;               // problems loaded
  int stage = 0;           // bit0 loaded, bit1 iterate, bit2 quadratized, bit3 gains
  bool stage_warm_all = false;   // ... without a shift array: every problem is warm-started, the init guess is not launched
  bool stage_warm = false; // the load in force was cilqr_stage_load_warm with a warm start: sets[0].warm_shift is current
  // test door (cilqr_set_search_seed), under mu: the seed the next job_begin takes -- host copies of the caller's arrays
  // (an empty vector: that value is not seeded) -- and the device block they are applied from
  bool seed_armed = false;
  int seed_batch = 0;
  std::vector<double> seed_cost_old, seed_lambda, seed_dlambda;
  std::vector<int> seed_iter;
  cilqr::dev_mem seed_dev;
  int spec_threshold = 8192;  // active sets up to this size evaluate all 11 step sizes at once (cilqr_solve_batch)
  // ... and for solves submitted with cilqr_submit: other solves share the GPU then, and eleven candidates per problem
  // where two or three would do is throughput taken from them (measured: pool of two 1.90 -> 1.98 M solves/s, one handle
  // with two solves in flight 1.67 -> 1.72 M; the sequential call loses 1 % at 2048, hence the two defaults).  Round 5, re-swept
  // beside the tail threshold below after the backward mappings had moved: 1024 with 128 there, pool of two 2.03-2.06 -> 2.07 M on two boxes
  int spec_threshold_submit = 1024;
  bool alone_on_device = false;   // a shard of cilqr_multi_*: its device is the caller's alone, submitted solves take spec_threshold
  int team_threshold = 4096;  // active sets up to this size run the backward pass with 8 lanes per problem
  int round_group = 2;        // step sizes costed per sequential round (1, 2 or 4)
  int wave_threshold = 3072;  // active sets up to this size run the backward pass with a wavefront per problem (1024 until
                              // round 5: re-swept after the wave form had become a third faster, tools/bwd_forms_sweep.py)
  int seq_rounds = 4;         // larger sets: this many round-by-round trials, then the rest at once
  // active sets up to this size leave the lockstep loop: one workgroup per problem (kernels_tail.hip).  Like the speculation
  // threshold it depends on company: a solve that has the GPU to itself (cilqr_solve_batch) is shortest when up to 1024 problems
  // finish there (the kernel then runs four rounds of workgroups: 1.27 -> 1.31 M solves/s); beside other solves those workgroups
  // hold a CU each for milliseconds and take it from the neighbours' bulk kernels (pool 1.97 -> 1.93 M), so submitted solves keep
  // fewer: 256 until round 5, 128 since (profiles/r05_cost_kernel_experiments.txt 6)
  int tail_threshold = 1024;
  int tail_threshold_submit = 128;
  size_t tail_lds_limit = 0;  // CILQR_OPT_TAIL_LDS_LIMIT: dynamic LDS a tail launch may plan with (0 = what the device grants; a test hook)
  cilqr::dev_mem tail_ws;     // private arenas of the tail's problems (lazily grown)
  cilqr::dev_mem tail_ws1;    // the same for a solve that reaches the tail without having been handed over (first stage)
  // asynchronous submit / wait: two jobs in flight, one worker thread per stage
  std::thread worker1, worker2, worker_io;
  std::mutex io_mu;           // creation of stream_in / stream_out (solver.hip: io_streams)
  std::mutex mu;
  std::condition_variable cv;
  bool workers_started = false, quit = false;
  bool fin_busy = false;      // the finishing arena holds a solve
  cilqr_job jobs[kJobRing];   // ring of submitted solves, oldest at job_head
  int job_head = 0;           // oldest job not yet collected by cilqr_wait
  int job_count = 0;          // submitted and not yet collected
  // profiling
  bool profiling = false;
  int profiling_level = 1;
  cilqr_profile prof;         // of the last solve that completed
  cilqr_comm* comm = nullptr;   // multi-GPU results gather (cilqr_comm_create)
  // The entry points that take HOST or DEVICE arrays (staging.hpp) have a set of blocks each: one of them calls another while
  // its own blocks hold live data (scene_pipeline.hip, carry_pipeline.hip).  What a call needs besides is named beside its set.
  cilqr::call_blocks cor;         // cilqr_build_corridors (corridor_batch.hip): the failure count alone -- its HOST arrays go
  cilqr::hip_event cor_done;      // through blocks of the call's own -- and the event a large call naps on
  cilqr::TrackerParams tracker;   // CILQR_INIT_TRACKER
  cilqr::call_blocks dp;          // cilqr_dp_plan_batch (planner_batch.hip): the road's tables
  cilqr::dev_mem dp_placed;       // ... and the placed dynamic polygons of a chunk of scenes
  // cilqr_scene_points_batch and cilqr_plan_scenes_batch (scene_pipeline.hip).  Both read the knot times from sp.tab, and
  // each sends them there its own way: the call through sp.tab_host like any table, the pipeline through sp_host, which
  // also lands its two outcome counts (upload_times), so sp.tab is as large as the larger of the two asks.  Then the
  // pipeline's intermediates (coarse trajectory, corridors, ..., HOST scenes and outputs) and the obstacle points of the
  // chunk of scenes in flight.
  cilqr::call_blocks sp;
  cilqr::pinned_mem sp_host;
  cilqr::dev_mem ps_work, ps_points;
  int scene_chunk = 0;            // CILQR_OPT_SCENE_CHUNK
  cilqr::call_blocks cc;          // cilqr_check_collisions_batch (collision_batch.hip): the barrier table
  cilqr::call_blocks rs;          // cilqr_resample_rows_batch (resample_batch.hip)
  cilqr::call_blocks fr;          // cilqr_frenet_rows_batch / cilqr_cartesian_points_batch (frenet_batch.hip): the centre line
  cilqr::call_blocks cl;          // cilqr_clearance_rows_batch (clearance_batch.hip)
  // cilqr_constraint_margins_batch (margins_batch.hip): the raw lane tables, the prepared lane rows behind them.  Nothing of
  // the staged or solver state is read or written by that call.
  cilqr::call_blocks mg;
  cilqr::call_blocks tk;          // cilqr_track_rows_batch (track_batch.hip)
  cilqr::dev_mem tk_work;         // ... and the follow table of the call (track.hpp)
  cilqr::call_blocks po;          // cilqr_policy_gains_batch / cilqr_policy_rollout_batch (policy_batch.hip)
  cilqr::call_blocks sw;          // cilqr_window_scenes_batch (scene_window_batch.hip)
  cilqr::call_blocks pr;          // cilqr_predict_scenes_batch (scene_predict_batch.hip)
  // cilqr_carry_rows_batch (carry_batch.hip); cilqr_plan_scenes_batch_carry (carry_pipeline.hip): the intermediates of its
  // coarse stage (states, hits, the list, HOST rows and advances), the gathered scenes and their plans, the list's length
  // on its way back
  cilqr::call_blocks cy;
  cilqr::pinned_mem cy_sel_host;
  cilqr::dev_mem cy_work, cy_chunk;
  // cilqr_stop_rows_batch (stop_batch.hip); cilqr_stop_scenes_batch (stop_pipeline.hip): its HOST arrays and the count, and
  // the slices of all profiles with their statuses and hits
  cilqr::call_blocks sr, ss;
  cilqr::dev_mem ss_work;
};

namespace cilqr {
// solver.hip (host waits): until `ev` has happened -- spinning in the runtime or, `relaxed`, with queries for `spin_us` and
// naps from then on
constexpr int kWaitSpinUs = 20;
int wait_event(hipEvent_t ev, bool relaxed, int spin_us = kWaitSpinUs);
}  // namespace cilqr

// The argument checks of a warm start against its problem batch (solver.hip; `in` not NULL): CILQR_OK for warm == NULL.
int cilqr_check_warm(const cilqr_problem_batch* in, const cilqr_warm_start* warm);

// cilqr_dp_plan_batch (planner_batch.hip); times_out (HOST, [n_knots], optional): the time column every planned scene gets
int cilqr_dp_plan_batch_impl(cilqr_solver* h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes, const double* start3,
                             int32_t n_knots, double* coarse9, double* coarse6, double* knots3, double* station,
                             int32_t* found, int32_t* n_not_found, double* times_out);
// the path samples of the five layers together: how many of a trajectory's n_knots rows k_dp_plan fills (the others stay
// zero); the checks on cfg are those of the call above (CILQR_ERR_ARG, CILQR_ERR_KNOTS, CILQR_ERR_CAPACITY)
int cilqr_dp_path_samples(const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes, int32_t n_knots, int32_t* n_samples);
