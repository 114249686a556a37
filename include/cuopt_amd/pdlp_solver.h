/*
 * C-ABI of the C++ host driver of the MI355X-native PDLP solver (cuopt_amd/csrc/pdlp_solver.cpp).
 *
 * This is the layer the libcuopt C API (cuopt_c.h -> cuOptSolve) sits on; it is exported so that
 * benches, the MIP-style warm-started re-solve loop and the parity tests can drive the solver
 * step by step.  It replaces, in the reference (cuOpt 25.08, LP/ = cpp/src/linear_programming/):
 *   cuoptamd_solver_create .... detail::problem_t ctor (cpp/src/mip/problem/problem.cu:53-136),
 *                               pdlp_solver_t ctor + the [init] block of run_solver
 *                               (LP/pdlp.cu:55-188, 984-1075)
 *   cuoptamd_solver_advance ... the while(true) loop of pdlp_solver_t::run_solver
 *                               (LP/pdlp.cu:1081-1185) incl. check_termination (:537-802) and
 *                               run_kkt_restart (LP/restart_strategy/pdlp_restart_strategy.cu:467-641)
 *   cuoptamd_hyper_preset ..... set_pdlp_solver_mode (LP/solve.cu:64-212)
 * All pointers are host pointers.  Functions return 0 or a negative code;
 * cuoptamd_last_error() holds the message.
 */
#ifndef CUOPT_AMD_PDLP_SOLVER_H
#define CUOPT_AMD_PDLP_SOLVER_H

#include <stdint.h>

#include "cuopt_amd/pdlp_device.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cuoptamd_solver cuoptamd_solver; /* opaque */

/* LP in the user's form: objective_sense * (c.x) + offset, lo <= A x <= hi, lb <= x <= ub */
typedef struct cuoptamd_lp {
  int32_t m, n;
  const int32_t* offsets; /* m+1 */
  const int32_t* indices; /* nnz */
  const double* values;   /* nnz */
  const double* c;        /* n */
  const double* lo;       /* m (may be -inf) */
  const double* hi;       /* m (may be +inf) */
  const double* lb;       /* n */
  const double* ub;       /* n */
  int32_t maximize;
  double objective_offset;
} cuoptamd_lp;

/* pdlp_hyper_params (cpp/include/cuopt/linear_programming/pdlp/pdlp_hyper_params.cuh:20-58) */
typedef struct cuoptamd_hyper {
  double initial_step_size_scaling;
  int32_t ruiz_iterations;
  int32_t do_pock_chambolle;
  int32_t do_ruiz;
  double alpha_pock_chambolle;
  double artificial_restart_threshold;
  int32_t compute_initial_step_size_before_scaling;
  int32_t compute_initial_primal_weight_before_scaling;
  double initial_primal_weight_c_scaling;
  double initial_primal_weight_b_scaling;
  int32_t major_iteration;
  int32_t min_iteration_restart;
  int32_t restart_strategy; /* 0 none, 1 KKT, 2 trust region (Methodical1) */
  int32_t never_restart_to_average;
  double reduction_exponent;
  double growth_exponent;
  double primal_weight_update_smoothing;
  double sufficient_reduction_for_restart;
  double necessary_reduction_for_restart;
  double primal_importance;
  double primal_distance_smoothing;
  double dual_distance_smoothing;
  int32_t compute_last_restart_before_new_primal_weight;
  int32_t artificial_restart_in_main_loop;
  int32_t rescale_for_restart;
  int32_t update_primal_weight_on_initial_solution;
  int32_t update_step_size_on_initial_solution;
  int32_t handle_some_primal_gradients_on_finite_bounds_as_residuals;
  int32_t project_initial_primal;
  /* ---- trailing fields, not in the reference (cuoptamd_hyper_preset fills them for every mode) ----
   * algorithm 0: PDHG with the adaptive step-size rule, running averages and KKT / trust-region restarts (the reference's; the four
   * cuOpt presets).  1: restarted reflected Halpern iteration with a constant step size (preset 4, docs/design/04d_halpern_mode.md):
   * eta = halpern_step_safety / sigma_max(scaled A), sigma_max by power iteration on A^T A until the estimate of sigma_max^2 moves by
   * at most halpern_power_tolerance relative or halpern_power_max_products products; restarts on the fixed-point error with
   * sufficient_ / necessary_reduction_for_restart and artificial_restart_threshold; primal_weight_update_smoothing at a restart. */
  int32_t algorithm;
  int32_t halpern_power_max_products;
  double halpern_step_safety;
  double halpern_power_tolerance;
} cuoptamd_hyper;

/* pdlp_solver_settings_t subset (pdlp/solver_settings.hpp:70-224) */
typedef struct cuoptamd_settings {
  double absolute_gap_tolerance, relative_gap_tolerance;
  double absolute_primal_tolerance, relative_primal_tolerance;
  double absolute_dual_tolerance, relative_dual_tolerance;
  int32_t iteration_limit; /* INT32_MAX: none */
  double time_limit;       /* seconds; +inf: none */
  int32_t per_constraint_residual;
  int32_t first_primal_feasible;
  /* warm start overrides (pdlp.cu:1014-1021); negative = not set */
  double initial_step_size;
  double initial_primal_weight;
  int32_t initial_k;
  int32_t use_graph; /* replay the PDHG attempt through hipGraphs (default 1) */
  /* infeasibility detection (pdlp/solver_settings.hpp: detect_infeasibility, strict_infeasibility;
   * tolerances default 1e-8, solver_settings.cu:83-84) */
  int32_t detect_infeasibility;
  int32_t strict_infeasibility;
  double primal_infeasible_tolerance;
  double dual_infeasible_tolerance;
  /* on a time / iteration limit return the best primal point seen at a major iteration instead of the last
   * iterate (pdlp.cu:264-331,390-466) */
  int32_t save_best_primal_so_far;
  /* iteration log (header + one line every 1000 iterations + summary, pdlp.cu:508-535,1077-1080): to stdout
   * and/or appended to log_file (NULL or "" = none) */
  int32_t log_to_console;
  const char* log_file;
  /* The reference's verdict kernel returns PrimalFeasible BEFORE it looks at the rays (termination_strategy.cu:190-226
   * vs :228-249), so its PDLP never reports an unbounded LP whose iterates are primal feasible: it runs until the
   * step-size arithmetic overflows (NumericalError).  Non-zero: a primal-feasible iterate whose normalised ray meets
   * the dual-infeasibility test is reported as DualInfeasible (needs detect_infeasibility; both iterates must agree
   * unless strict).  Default 0 = the reference's PDLP; cuOptSolve sets it for Concurrent / DualSimplex requests, where
   * the reference's simplex would return UNBOUNDED. */
  int32_t unbounded_from_feasible_iterates;
  /* A second, looser tolerance set (abs gap, rel gap, abs primal, rel primal, abs dual, rel dual).  When enabled, the
   * first iterate seen at a major iteration that is Optimal by THESE tolerances is kept; if the run then ends on an
   * iteration or time limit before the main tolerances are met, the kept iterate is returned with status Optimal
   * (cuoptamd_result::accepted_at_looser_tolerances = 1).  cuOptSolve uses it for Concurrent / DualSimplex requests
   * on small LPs: the main tolerances are simplex-grade (1e-8), the looser set is what the caller asked for, so the
   * caller's limits are honoured exactly as the reference's Concurrent mode would.  Ignored when
   * save_best_primal_so_far is set (same snapshot buffers). */
  int32_t accept_enabled;
  double accept_tolerance[6];
  /* set_relative_{primal,dual}_tolerance_factor (pdlp.cu:209-231): the norms ||b|| / ||c|| of the termination rule
   * (eps_abs + eps_rel * factor) replaced by the caller's values -- the MIP side keeps them fixed across re-solves.
   * Negative (default): computed from the problem. */
  double relative_primal_tolerance_factor, relative_dual_tolerance_factor;
  /* 0 (default), 2, 4, 8 or 16: the jagged layouts are built so that lockstep batches (cuoptamd_batch_create) of up to this many
   * clones can run on them -- a workgroup holds at most 16384 / batch_lanes rows, so that the row sums of every LP of the batch
   * fit its LDS.  Read when the solver is created (reset and clone ignore it; clones share the parent's layouts).  0: the layouts
   * of a solver that never batches, and cuoptamd_batch_create refuses a jagged parent with -7. */
  int32_t batch_lanes;
  /* Reflected Halpern mode (cuoptamd_hyper::algorithm == 1) only: non-zero lets an LP of resident size run the mode inside one
   * workgroup with the LP on chip (a whole period of steps in one launch, the evaluation of T(z^k) right behind it: two launches and
   * one synchronisation per period instead of four launches per step).  Read when the solver is created.  0 (default): the
   * multi-launch kernels, as before.  An LP that is not of resident size, or CUOPT_AMD_SMALL=0, silently takes the multi-launch
   * path (cuoptamd_solver_layout says which one runs); ignored when algorithm == 0.  A solver that runs on the resident path has
   * no clones: cuoptamd_solver_clone answers -7 for it, as for every resident solver (the multi-launch mode 4 can be cloned);
   * cuoptamd_batch_solve then solves the LPs independently, each in its own resident loop. */
  int32_t halpern_resident;
  /* Reflected Halpern mode on the resident path (algorithm == 1, halpern_resident != 0, an LP of resident size) only: non-zero lets
   * the solver be a member of a K-workgroup batch -- cuoptamd_batch_create accepts solvers that ALL have it set and run on the
   * resident path (any number, any matrices; -7 for a mix with other solvers), and cuoptamd_batch_solve takes that batch.  One launch
   * per resident tier in use, the evaluation of T(z^k) behind it and one synchronisation per period of the whole batch; every member
   * gets, bit for bit, what cuoptamd_solver_advance gives it on its own.  0 (default): refused / solved one after the other, as
   * before.  Ignored when algorithm == 0. */
  int32_t halpern_batch;
  /* Reflected Halpern mode on the multi-launch path (algorithm == 1, not the resident loop) only: non-zero lets the solver be a member
   * of a shared-matrix LOCKSTEP batch -- cuoptamd_batch_create accepts 2, 4, 8 or 16 such solvers over one matrix (a parent and its
   * clones) that ALL have it set, under the eligibility rules of the averaging lockstep batch (both matrices in the row-sum panels or
   * the CSR stream layout, no row beyond 128 entries; a jagged side is refused, with or without batch_lanes); -7, by name, for a mix of
   * members with and without it and for a mix of the two iterations.  The K LPs advance through four launches per step, the matrix
   * is streamed once for all of them; every member gets, bit for bit, what cuoptamd_solver_advance gives it on its own.
   * cuoptamd_batch_solve then groups LPs that share matrix and objective by 16 / 8 / 4 ("shared_matrix_halpern").  0 (default):
   * refused / solved one after the other, as before.  Ignored when algorithm == 0, and by a single solve. */
  int32_t halpern_lockstep;
  /* Reflected Halpern mode (algorithm == 1) only: non-zero switches infeasibility detection on.  At every major iteration whose
   * T(z^k) is not Optimal, the displacement of the period's last step, D = T(z^k) - z^k (unscaled: D_c dx, D_r dy), takes the
   * iterate's place in the infeasibility information: PrimalInfeasible iff dual_ray_linear_objective > 0 and
   * max_dual_ray_infeasibility / dual_ray_linear_objective <= primal_infeasible_tolerance, else DualInfeasible iff
   * primal_ray_linear_objective < 0 and max_primal_ray_infeasibility / -primal_ray_linear_objective <= dual_infeasible_tolerance --
   * whether or not T(z^k) is primal feasible.  The four *_ray_* fields of the result are filled, T(z^k) is what is returned, and
   * cuoptamd_solver_get_ray hands out the displacement itself.  Serves the multi-launch path (every layout), the resident loop
   * (halpern_resident) and the K-workgroup batch (halpern_batch); a lockstep batch (halpern_lockstep) refuses members that have it
   * set, with -7, unless every member also sets halpern_lockstep_rays (below).  0 (default): no certificate is looked for, as before (detect_infeasibility stays refused under algorithm == 1).
   * Ignored when algorithm == 0. */
  int32_t halpern_infeasibility;
  /* Reflected Halpern mode in a lockstep batch (halpern_lockstep) only: non-zero lets the batch take members that have
   * halpern_infeasibility set.  cuoptamd_batch_create then accepts such members iff EVERY member has this field set (-7, by name, for
   * a mix of members with and without it; members with and without halpern_infeasibility may be mixed), and cuoptamd_batch_advance
   * runs the ray pass for all members whose major iteration is due as ONE K-wide pass behind the attempts (pdlpdev_batch_halpern_rays:
   * two K-wide plain products in place of 2K single ones); the figures reach the host with each member's own evaluation read-back,
   * every member gets, bit for bit, what its own solver with halpern_infeasibility gives it, cuoptamd_solver_get_ray works on a member,
   * and a member that ends PrimalInfeasible / DualInfeasible rests while the others go on.  cuoptamd_batch_solve groups such LPs by
   * 16 / 8 / 4 ("shared_matrix_halpern") when both matrices are in the CSR stream layout; a side in the row-sum panels keeps them one
   * after the other ("shared_matrix"): the measured routing rule of docs/design/07_measurement.md, "Halpern mode".  0 (default): the refusal above stands, as before.  Ignored when algorithm == 0, and by a
   * single solve. */
  int32_t halpern_lockstep_rays;
  /* Reflected Halpern mode (algorithm == 1) only: non-zero lets cuoptamd_solver_create build a SHARDED solver (world >= 1 with a
   * communicator id) and cuoptamd_solve_sharded accept the mode: row blocks of A per rank, the owner-computes dataflow (the default
   * CUOPT_AMD_SHARD_DATAFLOW; allreduce and rsag are refused with -7, by name), over the collective transport (RCCL or the in-process
   * communicator, all-gathers or the halo exchange) or the direct peer stores (CUOPT_AMD_SHARD_TRANSPORT=p2p).  Every rank runs the
   * same major iterations on identical scalars.  Refused together with it, with -7 and by name: halpern_infeasibility,
   * halpern_resident, halpern_batch, membership of a lockstep batch and clones of a sharded solver, warm-start snapshots.  0
   * (default): a sharded solver in this mode is refused, as before.  Ignored when algorithm == 0. */
  int32_t halpern_sharded;
  /* Reflected Halpern mode (algorithm == 1) only: P = 1 .. 16 moves verdict and restart of a major iteration to the device and lets
   * cuoptamd_solver_advance enqueue BURSTS of up to P whole periods -- per period the steps to the period's target, the guarded
   * evaluation of T(z^k), one decision workgroup (the termination rule and the three restart tests on the scalars that are on the
   * device already), the guarded restart -- with no wait in between and ONE synchronisation per burst; the host then replays the
   * records the decisions left in pinned memory (counters, log lines, the result).  The device's verdict is the decision.  Every
   * figure, iterate and counter of the solve is, bit for bit, the one of P = 0; behind the period that stops a burst nothing that can
   * be read back changes.  Serves, with world == 1, the resident loop (halpern_resident and an LP of resident size) and the
   * multi-launch contexts the fused period path serves (both matrices in the panels, no per_constraint_residual); every other
   * context (stream, jagged, gather-free layouts; panels with per_constraint_residual) silently keeps the host-decided path
   * (cuoptamd_solver_halpern_device_major says which runs; cuOptAmdGetSolveInfo reports "halpern_device_major").  The time limit is looked at between bursts only: a
   * solve can overrun it by up to P periods, and the times in the iteration log are the burst's.  A step error, a budget that ends
   * inside a period and a period that is due at once go through the host-decided path.  Refused together with it, with -7 and by
   * name, at creation and at reset (a refused reset leaves the solver as it was): halpern_infeasibility, an enabled acceptance set
   * (accept_tolerance), halpern_sharded or any world > 1, halpern_batch, halpern_lockstep; cuoptamd_batch_create refuses a member that
   * has it set (a K-workgroup batch takes the option as a whole: cuoptamd_batch_set_halpern_device_major).  A value outside 0 .. 16 answers -1.  0 (default): the host decides after every period, as before.  Ignored when
   * algorithm == 0. */
  int32_t halpern_device_major;
} cuoptamd_settings;

/* additional_termination_information_t (pdlp/solver_solution.hpp:63-103) + run statistics */
typedef struct cuoptamd_result {
  int32_t status; /* pdlp_termination_status_t == CUOPT_TERIMINATION_STATUS_* ; 0 = still running */
  int32_t steps_taken;
  int32_t attempted_steps;
  int32_t returned_average;
  int32_t num_restarts;
  int32_t num_major_iterations;
  double primal_objective, dual_objective, gap, relative_gap;
  double l2_primal_residual, l2_dual_residual;
  double l2_relative_primal_residual, l2_relative_dual_residual;
  double max_primal_ray_infeasibility, max_dual_ray_infeasibility; /* filled when detect_infeasibility */
  double primal_ray_linear_objective, dual_ray_linear_objective;
  double initial_step_size, initial_primal_weight;
  double step_size, primal_weight;
  double norm_b, norm_c;
  double setup_seconds; /* transpose + upload + scaling + initial step/weight */
  double loop_seconds;  /* accumulated time inside cuoptamd_solver_advance */
  int32_t accepted_at_looser_tolerances; /* 1: the returned point is the one kept under settings.accept_tolerance */
  int32_t gpus;                          /* row blocks the LP was sharded into (1 = single GPU) */
} cuoptamd_result;

/* Row-block sharded solve inside ONE process: `gpus` host threads, one solver per visible device
 * (device g for rank g), row blocks balanced by nonzeros, RCCL all-reduce over xGMI (ncclCommInitRank from every thread
 * with one unique id).  Returns rank 0's statistics, the replicated primal solution / reduced costs and the GATHERED
 * dual solution (y has lp->m entries).  `soft_communicator` != 0 runs all ranks on device 0 through the in-process
 * communicator instead of RCCL (verification on a single-GPU box; not a production mode). */
int cuoptamd_solve_sharded(const cuoptamd_lp* lp, const cuoptamd_hyper* hyper, const cuoptamd_settings* settings,
                           int gpus, int soft_communicator, cuoptamd_result* result, double* x, double* y, double* rc);

/* pdlp_warm_start_data_t (cpp/include/cuopt/linear_programming/pdlp/pdlp_warm_start_data.hpp:31-90):
 * the complete solver state at a terminating major iteration.  Vectors are CALLER-allocated host arrays
 * (n entries for the primal ones, m for the dual ones).  As in the reference (pdlp.cu:468-489) the
 * current iterate and the average are in the user's UNSCALED space, A^T y, the running sums and the
 * last-restart anchors are in the solver's scaled space, so a snapshot is only meaningful for the SAME
 * constraint matrix and hyper-parameters (the reference's own restriction). */
typedef struct cuoptamd_warm_start {
  double* current_primal_solution;                  /* n */
  double* current_dual_solution;                    /* m */
  double* initial_primal_average;                   /* n */
  double* initial_dual_average;                     /* m */
  double* current_ATY;                              /* n */
  double* sum_primal_solutions;                     /* n */
  double* sum_dual_solutions;                       /* m */
  double* last_restart_duality_gap_primal_solution; /* n */
  double* last_restart_duality_gap_dual_solution;   /* m */
  /* optional (may be NULL): the current iterate in the solver's scaled space.  (x * D) / D is not x in the last
   * bit, so a restore from the unscaled iterate alone perturbs the trajectory; when these are present the
   * restore is bit-exact and its(full) == its(coarse) + its(warm) holds exactly. */
  double* current_primal_solution_scaled;           /* n */
  double* current_dual_solution_scaled;             /* m */
  double initial_primal_weight;
  double initial_step_size;
  int32_t total_pdlp_iterations;
  int32_t total_pdhg_iterations;
  double last_candidate_kkt_score;
  double last_restart_kkt_score;
  double sum_solution_weight;
  int32_t iterations_since_last_restart;
  /* sizes of the problem the snapshot was taken from (filled by get_warm_start; 0 = unknown): a snapshot of another
   * problem is refused by set_warm_start, like the reference (test_lp_solver.py:545-565) */
  int32_t n_variables, n_constraints;
} cuoptamd_warm_start;

/* The second engine (the reference's: cpp/src/dual_simplex, LP/solve.cu:295-347): an own bounded dual simplex (sparse LU of the
 * basis with product-form updates, dual steepest-edge pricing, Harris ratio test), host code like the reference's.  LPs of up to
 * 200 000 rows and 4e6 nonzeros (CUOPT_AMD_SIMPLEX_MAX_ROWS / CUOPT_AMD_SIMPLEX_MAX_NNZ move the limits).
 * *status: 1 optimal (x, y, rc, objective filled; y and rc in the convention rc = c - A^T y), 2 primal infeasible,
 * 3 unbounded, 5 iteration limit, 6 time limit, 7 numerical trouble / the engine abstains (a vertex on the box of the infinite
 * bounds whose ray costs less than any dual tolerance), 8 too large for this engine (nothing was done), 9 cancelled
 * (*cancel became non-zero: the other engine of a Concurrent solve finished first).  time_limit <= 0 / iteration_limit <= 0: none. */
int cuoptamd_dual_simplex(const cuoptamd_lp* lp, double time_limit, int32_t iteration_limit, const volatile int32_t* cancel,
                          int32_t* status, int32_t* iterations, double* objective, double* x, double* y, double* rc);
/* The same engine started from a basis guessed from the point x0 (n entries) and, optionally, the duals y0 (m entries, same
 * convention as y; NULL: none) -- e.g. PDLP's solution: the variables and rows that sit strictly between their bounds there form
 * the basis, then the ones on a bound with the smallest reduced cost at y0, completed / repaired with slacks.  This is the
 * crossover of a first-order solution to a vertex (the reference: crossover = true, LP/solve.cu:466-547). */
int cuoptamd_dual_simplex_from(const cuoptamd_lp* lp, const double* x0, const double* y0, double time_limit, int32_t iteration_limit,
                               const volatile int32_t* cancel, int32_t* status, int32_t* iterations, double* objective, double* x,
                               double* y, double* rc);

const char* cuoptamd_last_error(void);

/* presets, mode numbering as CUOPT_PDLP_SOLVER_MODE_* (0 Stable1, 1 Stable2, 2 Methodical1, 3 Fast1) and, beyond the reference's,
 * 4 = Halpern1 (CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1, cuopt_c_ext.h): Stable2's scaling and initial primal weight, algorithm = 1.  A
 * Halpern solver refuses, with a message that names the mode: sharded creation unless cuoptamd_settings::halpern_sharded is set
 * (then: the owner-computes dataflow, and none of halpern_infeasibility / _resident / _batch, clones or batches), warm-start snapshots,
 * detect_infeasibility, save_best_primal_so_far, first_primal_feasible; cuoptamd_batch_create answers -7 for it unless every member
 * is a resident Halpern solver with cuoptamd_settings::halpern_batch set (K workgroups of one launch), or every member is a
 * multi-launch Halpern solver over one matrix with cuoptamd_settings::halpern_lockstep set (the lockstep batch). */
void cuoptamd_hyper_preset(int mode, cuoptamd_hyper* h);
void cuoptamd_default_settings(cuoptamd_settings* s);

/* Builds A^T, slices this rank's row block (rank/world; world = 1: everything), uploads, scales,
 * computes the initial step size and primal weight.  `comm_id`: 128-byte RCCL id when world > 1
 * (or world == 1 and non-NULL to exercise the collective path), else NULL.
 * init_x / init_y: optional initial primal / dual solution in the user's (unscaled) space. */
int cuoptamd_solver_create(cuoptamd_solver** out, const cuoptamd_lp* lp, const cuoptamd_hyper* hyper,
                           const cuoptamd_settings* settings, const double* init_x,
                           const double* init_y, int device, int rank, int world,
                           const uint8_t* comm_id);
void cuoptamd_solver_destroy(cuoptamd_solver* s);

/* Persistent re-solve, the MIP heuristics' call pattern (get_relaxed_lp_solution / run_lp_with_vars_fixed,
 * cpp/src/mip/relaxed_lp/relaxed_lp.cu:53-175: same A and c, tightened or fixed bounds, previous primal/dual as the
 * initial point).  The reference constructs a new pdlp_solver_t per call (transpose, scaling, cuSPARSE set-up again);
 * here the solver keeps A, A^T, D_r, D_c and its kernels' layouts and only takes the new bounds.
 * lb / ub (n) and lo / hi (m_global): user-space host arrays, NULL = unchanged.  settings: NULL = unchanged.
 * init_x / init_y as in cuoptamd_solver_create.  Afterwards the solver behaves exactly (bit for bit) like a solver
 * freshly created on the modified LP: call cuoptamd_solver_advance. */
int cuoptamd_solver_reset(cuoptamd_solver* s, const double* lb, const double* ub, const double* lo, const double* hi,
                          const cuoptamd_settings* settings, const double* init_x, const double* init_y);

/* Persistent re-solve with a new OBJECTIVE vector, the feasibility pump's call pattern (linear_project_onto_polytope,
 * cpp/src/mip/local_search/feasibility_pump/feasibility_pump.cu:145-249: per round a distance objective to the rounded point, mixed
 * with alpha * c / ||c||, over the same constraints, warm-started from the previous point).  cuoptamd_solver_reset plus c (n doubles)
 * and objective_offset, both in the caller's terms exactly as at creation: c in the caller's column order and in the caller's sense
 * (a maximise solver negates it again; the sense itself cannot change), the offset as cuoptamd_lp::objective_offset.  c == NULL leaves
 * objective and offset unchanged: the call is cuoptamd_solver_reset.  Nothing of the matrix side is redone -- D_r, D_c, the initial
 * step, mode 4's sigma_max depend on A only; the scaled objective, ||c|| of the termination rule and the initial primal weight are
 * formed again by one kernel and one reduction (pdlpdev_set_objective), under the same overrides as ever (initial_primal_weight,
 * relative_dual_tolerance_factor).  Afterwards the solver is, bit for bit, a solver freshly created on the LP with that objective.
 * Every refusal of cuoptamd_solver_reset applies; an empty problem (m == 0) keeps its verdict.  -7, by name and with the solver left
 * exactly as it was, where the objective is not this solver's alone: a solver with live clones, a clone, a member of a lockstep
 * batch, a sharded solver.
 * Out of scope: per-member objectives for clones and lockstep shared-matrix batches (the objective would have to move into the part of
 * the device context an LP owns, and the K-wide kernels take K objectives); sharded solvers; changing the sense; the pump's auxiliary
 * variables for interior general integers, which change A. */
int cuoptamd_solver_reset_objective(cuoptamd_solver* s, const double* c, double objective_offset, const double* lb, const double* ub, const double* lo,
                                    const double* hi, const cuoptamd_settings* settings, const double* init_x, const double* init_y);

/* Runs the PDLP loop until a termination criterion fires or `max_new_iterations` further PDLP
 * iterations (accepted steps) have been taken, whichever is first.  result->status == 0 means
 * "budget exhausted, not terminated"; calling again continues exactly where it stopped. */
int cuoptamd_solver_advance(cuoptamd_solver* s, int32_t max_new_iterations, cuoptamd_result* result);

/* ---- shared-matrix batch (round 5): K LPs that differ in their bounds only are solved in lockstep, the matrix streamed once per
 * attempt for all of them (pdlpdev_batch_* in pdlp_device.h; the MIP heuristics' re-solve pattern, relaxed_lp.cu:53-127).
 * cuoptamd_solver_clone: a solver for the parent's LP with other bounds (NULL = the parent's CURRENT ones; settings NULL = the
 * parent's) that shares the parent's matrices on the device; behaves bit for bit like a solver freshly created on that LP.  Destroy
 * the clones before the parent (cuoptamd_solver_reset of either is fine while both exist).  -7: empty, resident or sharded parent.
 * cuoptamd_batch_create: K = 2, 4, 8 or 16 solvers over one matrix (a parent and its clones, none advanced by hand in between is NOT
 * required: a batch may be created over solvers in any state).  -7 when the layouts are not eligible (pdlp_device.h): the caller
 * falls back to cuoptamd_solver_advance per solver or to cuoptamd_batch_solve.
 * cuoptamd_batch_advance: every solver up to max_new_iterations further iterations or to its verdict; results[l] as
 * cuoptamd_solver_advance would fill it (loop_seconds: the wall time of the batch).  Solutions through the solvers' own getters.
 * cuoptamd_batch_destroy leaves the solvers alive. */
typedef struct cuoptamd_batch cuoptamd_batch;
int cuoptamd_solver_clone(cuoptamd_solver* parent, const double* lb, const double* ub, const double* lo, const double* hi,
                          const cuoptamd_settings* settings, cuoptamd_solver** out);
int cuoptamd_batch_create(cuoptamd_solver** solvers, int K, cuoptamd_batch** out);
int cuoptamd_batch_advance(cuoptamd_batch* batch, int32_t max_new_iterations, cuoptamd_result* results);
/* ---- small-LP batch (round 6): cuoptamd_batch_create over solvers on the resident small-LP path takes ANY number of them, whatever their
 * matrices -- one workgroup per LP, one launch per phase of the loop (pdlpdev_small_batch_* in pdlp_device.h; BASELINE config 5 at
 * branch-and-bound scale, cython_solve.cu:264-296 / relaxed_lp.cu:53-127).  Bit-identical to cuoptamd_solver_advance per solver.
 * cuoptamd_batch_reset: cuoptamd_solver_reset(lb[l], ub[l], NULL, NULL, NULL, init_x[l], init_y[l]) for every solver in one launch
 * (arrays and entries may be NULL); -7 when the batch is not a small-LP batch.
 * cuoptamd_batch_get_solutions: cuoptamd_solver_get_solution for every solver in one launch (any batch; arrays / entries may be NULL). */
int cuoptamd_batch_reset(cuoptamd_batch* batch, const double* const* lb, const double* const* ub, const double* const* init_x, const double* const* init_y);
int cuoptamd_batch_get_solutions(cuoptamd_batch* batch, double* const* x, double* const* y, double* const* rc);
/* cuoptamd_batch_branch: one branch-and-bound step per node in ONE launch -- the bounds of variable var[l] of solver l become
 * [lb[l], ub[l]] (var[l] < 0: none) and the solver starts again from the primal / dual its last solve returned, all on the device
 * (relaxed_lp.cu:74-108); bit for bit cuoptamd_solver_reset(full bounds, solution of cuoptamd_solver_get_solution).
 * cuoptamd_batch_solution_views: the solutions as pointers into the batch's pinned staging block (no copies; valid until the next
 * reset / branch / solutions call of the batch). */
int cuoptamd_batch_branch(cuoptamd_batch* batch, const int32_t* var, const double* lb, const double* ub);
int cuoptamd_batch_solution_views(cuoptamd_batch* batch, const double** x, const double** y, const double** rc);
/* cuoptamd_batch_reset_objectives: cuoptamd_solver_reset_objective(c[l], objective_offset[l], lb[l], ub[l], NULL, NULL, NULL, init_x[l],
 * init_y[l]) for every solver of a small-LP batch, with a number of launches that does not depend on K and the one synchronisation of
 * cuoptamd_batch_reset: the objectives are scaled, reduced and turned into the initial primal weights on the device, in front of the
 * reset kernel.  Arrays and entries may be NULL; c[l] == NULL keeps solver l's objective and offset (objective_offset == NULL: offsets
 * 0 for the solvers that get an objective).  warm_from_last != 0: every solver starts from the point its last solve returned, as in
 * cuoptamd_batch_branch (init_x and init_y must then be NULL).  -7 by name for a lockstep batch, whose members share one objective;
 * otherwise cuoptamd_batch_reset's refusals.
 * cuoptamd_batch_reset_stats: {kernel launches, synchronisations} of all reset / branch / reset_objectives calls of a small-LP batch. */
int cuoptamd_batch_reset_objectives(cuoptamd_batch* batch, const double* const* c, const double* objective_offset, const double* const* lb,
                                    const double* const* ub, const double* const* init_x, const double* const* init_y, int warm_from_last);
int cuoptamd_batch_reset_stats(cuoptamd_batch* batch, int64_t out[2]);
void cuoptamd_batch_destroy(cuoptamd_batch* batch);
/* counters of a small-LP batch (pdlpdev_small_batch_stats): {Halpern batch (0 / 1), resident tiers in use, loop launches, evaluation
 * launches behind the loop, runs (periods), restart rounds, resets, synchronisations}; restart rounds and resets are counted for a batch
 * in reflected Halpern mode, and an averaging batch counts the synchronisations of its runs only; -7: not a small-LP batch */
int cuoptamd_batch_stats(cuoptamd_batch* batch, int64_t out[8]);
/* ---- major iterations of a K-workgroup Halpern batch decided on the device (docs/design/04d_halpern_mode.md, "Bursts of a K-workgroup
 * batch").  An option of the BATCH, not a field of cuoptamd_settings: cuoptamd_batch_create keeps refusing a member that has
 * halpern_device_major set, and halpern_device_major + halpern_batch in the settings stays refused.
 * cuoptamd_batch_set_halpern_device_major(P), P = 1 .. 16: cuoptamd_batch_advance runs the batch in BURSTS -- up to P whole periods
 * for all members enqueued with no wait in between, each member's verdict and restart decided on the device
 * (pdlpdev_small_batch_run_halpern_burst), ONE synchronisation, then each member's records replayed on the host.  A round is a burst
 * when every member that is not done is burst-ready: its next target is a period's end, it is past min_iteration_restart, at least
 * one whole period fits its budget, no step error is pending and nothing waits to be prepared; the burst runs the fewest periods any
 * member allows.  Any other round is the host-decided one, for all members.  Every member gets, bit for bit, what its own
 * cuoptamd_solver_advance with halpern_device_major = 0 gives it.  The time limit is looked at between bursts.  P = 0: back to the
 * host-decided round.  -1: P outside 0 .. 16 or a null batch.  -7, by name: a batch that is no K-workgroup Halpern batch (an
 * averaging small-LP batch, either lockstep batch), a member with halpern_infeasibility, a member with an enabled acceptance set;
 * a refused call leaves the batch as it was.  cuoptamd_batch_reset and cuoptamd_batch_branch keep the option.
 * cuoptamd_batch_solve has nowhere to carry P and keeps the host-decided round.
 * cuoptamd_batch_halpern_device_major: the P the batch runs with.
 * cuoptamd_batch_halpern_burst_stats: out = {bursts, periods enqueued, records written, member-periods enqueued behind a member's
 * stop}; cuoptamd_batch_stats counts one synchronisation per burst and the bursts' loop and evaluation launches. */
int cuoptamd_batch_set_halpern_device_major(cuoptamd_batch* batch, int32_t P);
int cuoptamd_batch_halpern_device_major(cuoptamd_batch* batch);
int cuoptamd_batch_halpern_burst_stats(cuoptamd_batch* batch, int64_t out[4]);
/* the device-layer batch behind it (pdlpdev_batch_time_kernels) */
struct pdlpdev_batch* cuoptamd_batch_device(cuoptamd_batch* batch);

/* Fills *ws (get_filled_warmed_start_data, pdlp.cu:468-489) from a solver whose last advance terminated.
 * Single-GPU solvers only. */
int cuoptamd_solver_get_warm_start(cuoptamd_solver* s, cuoptamd_warm_start* ws);
/* Restores a snapshot into a freshly created solver (before its first advance), pdlp.cu:131-181:
 * iteration counts keep running from the snapshot (its(1e-2 from scratch) == its(1e-1) + its(1e-2 warm),
 * the reference's warm-start test, pdlp_test.cu:803-854). */
int cuoptamd_solver_set_warm_start(cuoptamd_solver* s, const cuoptamd_warm_start* ws);

/* set_pdlp_warm_start_data(data, var_mapping, constraint_mapping) of the reference (LP/solver_settings.cu:92-240): a
 * snapshot of an n_old x m_old problem for a problem with n_mapping variables / m_mapping constraints (0 = that side is
 * unchanged).  Shorter: new[map[i]] = old[i] for i < new size (the map must be a permutation of 0..new size-1), the
 * rest is dropped; longer: the old entries, then zeros (the map's values are not read, as in the reference).  `out`'s
 * vectors are caller-allocated at the new sizes; the scaled iterate is dropped when a size changes.  Host only. */
int cuoptamd_warm_start_remap(const cuoptamd_warm_start* in, const int32_t* var_mapping, int32_t n_mapping,
                              const int32_t* constraint_mapping, int32_t m_mapping, cuoptamd_warm_start* out);

/* x (n), y (m_global), reduced cost (n) of the returned iterate, unscaled, in the internal min-form
 * sign convention of the reference (any pointer may be NULL). Valid after a terminating advance. */
int cuoptamd_solver_get_solution(cuoptamd_solver* s, double* x, double* y, double* rc);
/* Reflected Halpern mode with cuoptamd_settings::halpern_infeasibility: the certificate of the last ray evaluation -- the unscaled
 * displacement dx (n) = D_c (x' - x^k), dy (m) = D_r (y' - y^k) of the period's last step, in the caller's order (either pointer may
 * be NULL).  For PrimalInfeasible dy is the Farkas certificate, for DualInfeasible dx the unbounded direction.  -7 when the option is
 * off or no ray has been evaluated at the solver's present step count. */
int cuoptamd_solver_get_ray(cuoptamd_solver* s, double* dx, double* dy);

/* Batch solve (call_batch_solve, LP/utilities/cython_solve.cu:264-296: independent LPs solved concurrently on
 * one GPU, one host thread + one stream each, at most `max_threads` at a time; <= 0: one per available core,
 * capped at 16).  results[i] is filled for every LP; x[i] / y[i] / rc[i] (each may be NULL, as may the arrays)
 * receive the solutions.  Returns 0 if every solve ran (look at results[i].status), else the first error. */
int cuoptamd_batch_solve(int32_t count, const cuoptamd_lp* lps, const cuoptamd_hyper* hyper,
                         const cuoptamd_settings* settings, int device, int max_threads,
                         cuoptamd_result* results, double** x, double** y, double** rc);
/* which way the last cuoptamd_batch_solve of this thread took (a static string; "" before the first call): "small" -- the K-workgroup
 * batch of resident LPs --, "small_halpern" -- the same in reflected Halpern mode (cuoptamd_settings::halpern_batch) --,
 * "shared_matrix" -- one set-up, clones, lockstep batches (reflected Halpern mode without halpern_lockstep: the clones one after the
 * other) --, "shared_matrix_halpern" -- the same with at least one group advanced by the Halpern lockstep batch
 * (cuoptamd_settings::halpern_lockstep) --, "independent" -- a solver per LP on worker threads.  The answers do
 * not tell the ways apart: every one gives each LP the result of its own solve. */
const char* cuoptamd_batch_solve_last_path(void);

/* the device context (for kernel timing and buffer downloads in benches/tests) */
pdlpdev_ctx* cuoptamd_solver_device(cuoptamd_solver* s);
/* cuoptamd_settings::halpern_device_major as this solver runs it: P when its major iterations are decided on the device in bursts of
 * up to P periods, 0 when the host decides them (the option is off, the averaging iteration, a context without the burst) */
int cuoptamd_solver_halpern_device_major(cuoptamd_solver* s);
/* rows [row_begin, row_end) of A held by this rank (of the matrix in the DEVICE's order when the set-up reordered it) */
int cuoptamd_solver_row_range(cuoptamd_solver* s, int32_t* row_begin, int32_t* row_end);
/* Set-up reordering (pdlp_device.h "device-side set-up"): info = pdlpdev_analysis_info's ten numbers (info[0] = 1: the device works
 * on P A Q; info[1]: 1 breadth-first levels, 2 seeded cells); row_new2old[m] / col_new2old[n] (either may be NULL) receive the maps
 * when the LP was reordered.  Returns 1 when reordered, 0 when the device holds the LP as given.  Everything that crosses this
 * interface -- bounds, initial iterates, solutions, warm starts -- stays in the CALLER's order either way. */
int cuoptamd_solver_reorder_info(cuoptamd_solver* s, int32_t info[10], int32_t* row_new2old, int32_t* col_new2old);

/* contiguous row-block partition balanced by nonzeros: fills bounds[0..world] */
void cuoptamd_partition_rows(int32_t m, const int32_t* offsets, int world, int32_t* bounds);
/* CSR transpose (stable: rows ascending inside each column), host, O(nnz) */
void cuoptamd_csr_transpose(int32_t m, int32_t n, const int32_t* offsets, const int32_t* indices,
                            const double* values, int32_t* t_offsets, int32_t* t_indices,
                            double* t_values);

#ifdef __cplusplus
}
#endif
#endif
