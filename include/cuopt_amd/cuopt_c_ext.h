/* Extensions of this library to the libcuopt C API (include/cuopt/linear_programming/cuopt_c.h mirrors the reference's
 * 41 functions unchanged; nothing here exists in NVIDIA/cuopt).
 *
 * Extra parameters accepted by cuOptSetIntegerParameter / cuOptGetIntegerParameter:
 *   CUOPT_AMD_NUM_GPUS       row blocks of one solve, one GPU each, inside the calling process (RCCL over xGMI).
 *                            0 (default) = the CUOPT_AMD_NUM_GPUS environment variable, else 1.
 *   CUOPT_AMD_SIMPLEX_GRADE  1 / 0: serve Concurrent / DualSimplex requests on small LPs (<= 1e5 nonzeros) at
 *                            simplex-grade tolerances (1e-8) with the requested tolerances as acceptance set
 *                            (cuoptamd_settings::accept_tolerance).  -1 (default) = the key simplex_grade of the
 *                            CUOPT_AMD_TUNE environment string (CUOPT_AMD_TUNE=simplex_grade=0), else on.
 *   CUOPT_AMD_HALPERN_RESIDENT  1 / 0 (default 0): under CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1 an LP of resident size (m, n <= 2048,
 *                            nnz <= 4096 ... 8192) runs a whole period of steps inside one workgroup with the LP on chip
 *                            (cuoptamd_settings::halpern_resident).  Larger LPs, and every LP under CUOPT_AMD_SMALL=0, take the
 *                            multi-launch kernels; ignored by the other solver modes.  cuOptAmdGetSolveInfo says what ran.
 *   CUOPT_AMD_HALPERN_BATCH  1 / 0 (default 0): with CUOPT_AMD_HALPERN_RESIDENT, the solvers of this call may be members of a
 *                            K-workgroup batch (cuoptamd_settings::halpern_batch): where several LPs are solved at once
 *                            (cuoptamd_batch_solve, cuoptamd_batch_create) K of them run in K workgroups of one launch, each
 *                            bit for bit as on its own.  A single solve is not changed by it; ignored by the other solver modes.
 *   CUOPT_AMD_HALPERN_LOCKSTEP  1 / 0 (default 0): under CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1 on the multi-launch path, LPs that share
 *                            matrix and objective advance as shared-matrix lockstep batches of 16 / 8 / 4
 *                            (cuoptamd_settings::halpern_lockstep; cuoptamd_batch_solve, cuoptamd_batch_create), each bit for bit
 *                            as on its own.  A single cuOptSolve is not changed by it; ignored by the other solver modes.
 *   CUOPT_AMD_HALPERN_INFEASIBILITY  1 / 0 (default 0): under CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1, infeasibility detection on the
 *                            displacement of a step (cuoptamd_settings::halpern_infeasibility): an infeasible LP ends as
 *                            PrimalInfeasible, an unbounded one as DualInfeasible, at CUOPT_PRIMAL_INFEASIBLE_TOLERANCE /
 *                            CUOPT_DUAL_INFEASIBLE_TOLERANCE, instead of at its iteration or time limit.  CUOPT_INFEASIBILITY_DETECTION
 *                            (the averaging iteration's) stays a validation error under that mode; ignored by the other modes.
 *   CUOPT_AMD_HALPERN_LOCKSTEP_RAYS  1 / 0 (default 0): with CUOPT_AMD_HALPERN_LOCKSTEP and CUOPT_AMD_HALPERN_INFEASIBILITY, the
 *                            lockstep batches take LPs that detect infeasibility (cuoptamd_settings::halpern_lockstep_rays): the
 *                            ray passes of a batch's members run as one K-wide pass, each member bit for bit as on its own; without
 *                            it such LPs are solved one after the other, as before.  A single cuOptSolve is not changed by it
 *                            (cuOptAmdGetSolveInfo reports "halpern_lockstep_rays"); ignored by the other solver modes.
 *   CUOPT_AMD_HALPERN_SHARDED  1 / 0 (default 0): under CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1 with CUOPT_AMD_NUM_GPUS > 1, the solve is
 *                            sharded by row blocks on the owner-computes dataflow (cuoptamd_settings::halpern_sharded), over
 *                            collectives or the direct peer stores; without it such a request stays a validation error.
 *                            CUOPT_AMD_HALPERN_INFEASIBILITY, _RESIDENT and _BATCH are validation errors together with it
 *                            (cuOptAmdGetSolveInfo reports "halpern_sharded"); ignored by the other solver modes.
 *   CUOPT_AMD_HALPERN_DEVICE_MAJOR  0 (default) .. 16: under CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1 on one GPU, P > 0 lets the device decide
 *                            verdict and restart of a major iteration itself and enqueues up to P periods per host
 *                            synchronisation (cuoptamd_settings::halpern_device_major); the answer is, bit for bit, the one of P = 0.
 *                            A time limit can be overrun by up to P periods.  CUOPT_AMD_HALPERN_INFEASIBILITY, _SHARDED, _BATCH and
 *                            _LOCKSTEP are validation errors together with it; where the simplex-grade emulation has switched the
 *                            acceptance set on, the parameter is dropped.  cuOptAmdGetSolveInfo reports "halpern_device_major": the
 *                            P that ran, 0 where the host decided (a layout without the burst, a dropped parameter); ignored by
 *                            the other solver modes.
 * Extra value of CUOPT_PDLP_SOLVER_MODE (constants.h stops at CUOPT_PDLP_SOLVER_MODE_FAST1 = 3):
 *   CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1 = 4: the restarted reflected Halpern iteration with a constant step size
 *                            (cuoptamd_hyper_preset(4), docs/design/04d_halpern_mode.md).  One GPU unless CUOPT_AMD_HALPERN_SHARDED is set (below); CUOPT_INFEASIBILITY_DETECTION,
 *                            save_best_primal_so_far and first_primal_feasible are refused with a validation error, and the
 *                            simplex-grade emulation leaves the infeasibility detection it would switch on off.
 */
#ifndef CUOPT_AMD_CUOPT_C_EXT_H
#define CUOPT_AMD_CUOPT_C_EXT_H

#include "cuopt/linear_programming/cuopt_c.h"
#include "cuopt_amd/pdlp_solver.h"

#define CUOPT_AMD_NUM_GPUS "amd_num_gpus"
#define CUOPT_AMD_SIMPLEX_GRADE "amd_simplex_grade"
#define CUOPT_AMD_HALPERN_RESIDENT "amd_halpern_resident"
#define CUOPT_AMD_HALPERN_BATCH "amd_halpern_batch"
#define CUOPT_AMD_HALPERN_LOCKSTEP "amd_halpern_lockstep"
#define CUOPT_AMD_HALPERN_INFEASIBILITY "amd_halpern_infeasibility"
#define CUOPT_AMD_HALPERN_LOCKSTEP_RAYS "amd_halpern_lockstep_rays"
#define CUOPT_AMD_HALPERN_SHARDED "amd_halpern_sharded"
#define CUOPT_AMD_HALPERN_DEVICE_MAJOR "amd_halpern_device_major"
#define CUOPT_AMD_PDLP_SOLVER_MODE_HALPERN1 4

#ifdef __cplusplus
extern "C" {
#endif

/* full PDLP statistics of an LP solution (the reference exposes additional_termination_information_t through its
 * C++ / Python API only: cpp/include/cuopt/linear_programming/pdlp/solver_solution.hpp:63-103) */
cuopt_int_t cuOptAmdGetPdlpStats(cuOptSolution solution, cuoptamd_result* stats);

/* which engine / attempt answered the request, as one JSON object (also "pdlp_algorithm": "pdhg_average" | "reflected_halpern"):
 * {"engine": "pdlp" | "dual_simplex", "requested_method": "Concurrent|DualSimplex|PDLP", "crossover_requested": bool,
 *  "simplex_grade_emulation": bool, "dual_simplex_consulted": bool, "dual_simplex_status": 1..9 (cuoptamd_dual_simplex),
 *  "crossover": "none" | "dual_simplex_from_the_pdlp_point" | "not_done_..." | "not_needed_vertex_from_the_dual_simplex",
 *  "answered_by": "...", "gpus": N, "iterations": K, "simplex_grade_attempt_iterations": K0,
 *  "halpern_resident": 0 | 1 (the PDLP solver of this call ran the reflected Halpern mode on the resident small-LP path)}
 * (the reference runs its dual simplex / crossover for such requests, LP/solve.cu:383-443,467-547; here an own simplex code on
 * the host -- cuoptamd_dual_simplex[_from], LPs of up to 200 000 rows -- answers DualSimplex requests, races PDLP under
 * Concurrent and crosses PDLP's point over to a vertex; beyond its limits PDLP serves the request, and the call says so
 * instead of pretending) */
cuopt_int_t cuOptAmdGetSolveInfo(cuOptSolution solution, char* buffer, cuopt_int_t buffer_size);

/* name of variable (kind 0) / constraint row (kind 1) `index` of a problem that came from cuOptReadProblem
 * (CUOPT_INVALID_ARGUMENT when the problem carries no names) */
cuopt_int_t cuOptAmdGetName(cuOptOptimizationProblem problem, cuopt_int_t kind, cuopt_int_t index, char* buffer,
                            cuopt_int_t buffer_size);

/* reads a .sol file (CUOPT_SOLUTION_FILE output, or MIPLIB style) into the variable order of `problem` (which must carry
 * variable names, i.e. come from cuOptReadProblem); objective_value / status may be NULL.  Mirrors
 * cpp/src/math_optimization/solution_reader.cu:57-145.  CUOPT_MPS_FILE_ERROR: cannot open; CUOPT_VALIDATION_ERROR: a
 * variable of the problem is not in the file. */
cuopt_int_t cuOptAmdReadSolutionFile(cuOptOptimizationProblem problem, const char* filename, cuopt_float_t* values,
                                     cuopt_float_t* objective_value, char* status, cuopt_int_t status_size);

#ifdef __cplusplus
}
#endif
#endif
