/*
 * russell_hipmf.h -- C-ABI of the MI355X-native sparse direct solver backend ("HIPMF": HIP
 * multifrontal LU) that plugs in behind russell_sparse's solver boundary.
 *
 * The entry points are what russell_sparse's FFI for this path binds.  They keep the shape of the
 * reference's existing GPU plug-in (c_code/interface_cudss.cu) and of the UMFPACK shim
 * (c_code/interface_umfpack.c): an opaque handle, new/drop, and the three phases
 * initialize (once) / factorize (values only, repeatable) / solve.  All sizes, indices, enums and
 * booleans are int32_t; matrices are 0-based CSR with f64 values; host pointers are borrowed for
 * the duration of a call and never retained (ownership rules of SURVEY.md section 8b).
 *
 * Reference interface each declaration replaces (paths relative to /root/reference):
 *   solver_hipmf_new         russell_sparse/c_code/interface_cudss.cu:62-123   (solver_cudss_new)
 *   solver_hipmf_drop        russell_sparse/c_code/interface_cudss.cu:126-171  (solver_cudss_drop)
 *   solver_hipmf_initialize  russell_sparse/c_code/interface_cudss.cu:190-396  (solver_cudss_initialize)
 *                            and interface_umfpack.c:82-124 (ordering, scaling arguments)
 *   solver_hipmf_factorize   russell_sparse/c_code/interface_cudss.cu:406-501  (solver_cudss_factorize)
 *                            and interface_umfpack.c:141-200 (rcond, determinant outputs)
 *   solver_hipmf_solve       russell_sparse/c_code/interface_cudss.cu:510-566  (solver_cudss_solve)
 * Rust side that calls them: russell_sparse/src/solver_cudss.rs:25-52,194-360.
 *
 * Status codes: 0 = success; the shared 100000..700000 codes are those of
 * russell_sparse/c_code/constants.h:5-12 verbatim; 1 = "Matrix is singular" is the value UMFPACK
 * returns (russell_sparse/src/solver_umfpack.rs:492); the 100..1000 block is this backend's
 * analogue of the cuDSS block (constants.h:22-36).
 */
#ifndef RUSSELL_HIPMF_H
#define RUSSELL_HIPMF_H

#include <inttypes.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C_BOOL int32_t

#define SUCCESSFUL_EXIT 0
#define ERROR_NULL_POINTER 100000
#define ERROR_MALLOC 200000
#define ERROR_VERSION 300000
#define ERROR_NOT_AVAILABLE 400000
#define ERROR_NEED_INITIALIZATION 500000
#define ERROR_NEED_FACTORIZATION 600000
#define ERROR_ALREADY_INITIALIZED 700000

#define HIPMF_WARNING_SINGULAR_MATRIX 1
#define HIPMF_WARNING_NOT_CONVERGED 2 /* the solve_updated and solve_extra_precise forms only: the tolerance was not reached; x holds the best iterate */
#define ERROR_HIP_MALLOC 100
#define ERROR_HIP_MEMCPY 200
#define ERROR_HIP_SYNCHRONIZE 300
#define ERROR_HIP_LAUNCH 350
#define ERROR_HIPMF_INVALID_MATRIX 600
#define ERROR_HIPMF_SYMBOLIC 700
#define ERROR_HIPMF_INVALID_VALUE 803
#define ERROR_HIPMF_COMM 900 /* an RCCL call failed */
#define ERROR_HIPMF_NO_DEVICE 1000

/* ordering argument of solver_hipmf_initialize */
#define HIPMF_ORDERING_DEFAULT 0            /* nested dissection */
#define HIPMF_ORDERING_NESTED_DISSECTION 1
#define HIPMF_ORDERING_NONE 2               /* natural order (Ordering::No) */
#define HIPMF_ORDERING_AMD 3                /* approximate minimum degree on A + A^T (Ordering::Amd / Amf / Qamd; own implementation of the
                                               published method, symbolic.cpp) -- the better choice for patterns without small separators */
#define HIPMF_ORDERING_BEST 4               /* both orderings, the one whose factorisation needs fewer flops is kept (Ordering::Best, UMFPACK's
                                               meaning of the word); the effective ordering reports which one that was */
/* scaling argument (same numbering as UMFPACK_SCALE_*) */
#define HIPMF_SCALE_NONE 0
#define HIPMF_SCALE_SUM 1
#define HIPMF_SCALE_MAX 2

struct InterfaceHIPMF;

/* Allocates a solver bound to the calling thread's current HIP device.  Returns NULL on failure. */
struct InterfaceHIPMF *solver_hipmf_new(void);

/* Frees every host and device resource.  NULL-safe. */
void solver_hipmf_drop(struct InterfaceHIPMF *solver);

/* Phase 1 (once): ordering + symbolic analysis on the host, device allocation, structure upload.
 * pivot_epsilon < 0 and refinement_nstep < 0 select the defaults (1e-13 relative, 2 steps).
 * general_symmetric: the CSR holds the LOWER triangle of a symmetric matrix (Sym::YesLower).
 * values may be NULL.  When given (the reference hands the numbers to the analysis phase as well:
 * umfpack_di_symbolic(Ap, Ai, Ax) at interface_umfpack.c:109, cudssExecute(ANALYSIS) at interface_cudss.cu:361)
 * and the diagonal is weak (missing, zero or < 1 % of the row's largest entry somewhere), general-storage matrices
 * get a maximum-product matching + row/column scaling pre-permutation, which stays in force for every later
 * factorisation with this handle.  A symmetric-lower matrix with such a diagonal (indefinite: the Lagrange rows of
 * CooMatrix::put_lagrange_block, coo_matrix.rs:823-857) is mirrored to general storage inside the handle and takes the same
 * path (HIPMF_COUNTER_SYM_EXPANDED); the caller keeps passing lower-triangle values and lower-triangle value maps.  Round 4: a
 * symmetric-lower handle initialised WITHOUT values makes that decision at its first solver_hipmf_factorize (one more analysis inside
 * that call when the diagonal is weak; handles with a value map installed keep the L D L^T path). */
int32_t solver_hipmf_initialize(struct InterfaceHIPMF *solver,
                                int32_t ordering,
                                int32_t scaling,
                                double pivot_epsilon,
                                int32_t refinement_nstep,
                                C_BOOL verbose,
                                C_BOOL general_symmetric,
                                C_BOOL positive_definite,
                                int32_t ndim,
                                const int32_t *row_pointers,
                                const int32_t *col_indices,
                                const double *values);

/* Phase 2 (repeatable): numeric multifrontal LU of the same structure with new values.
 * Returns 0, or 1 when an exactly-zero pivot was met ("Matrix is singular").
 * Pivot order: static (nested dissection + the matching of initialize).  Every factorize checks the diagonal of the system it is
 * about to factorise; when THESE values call for another maximum-product matching (general storage: initialize had no values, or
 * the values changed a lot) the matching is recomputed from them and the analysis redone inside this call (cost of an initialize;
 * HIPMF_COUNTER_REMATCH counts it).  UMFPACK pivots dynamically in every numeric phase (interface_umfpack.c:167). */
int32_t solver_hipmf_factorize(struct InterfaceHIPMF *solver,
                               int32_t *effective_ordering,
                               int32_t *effective_scaling,
                               int32_t *num_perturbed_pivots,
                               double *rcond_estimate,
                               double *determinant_coefficient,
                               double *determinant_exponent,
                               C_BOOL compute_determinant,
                               C_BOOL verbose,
                               const double *values);

/* Phase 3: x = A^{-1} rhs (forward/backward level-set solves + iterative refinement). */
int32_t solver_hipmf_solve(struct InterfaceHIPMF *solver, double *x, const double *rhs, C_BOOL verbose);

/* ---- extensions that the reference's single-RHS boundary lacks ---------- */

/* nrhs right-hand sides, column-major with leading dimension ld >= ndim (host pointers) */
int32_t solver_hipmf_solve_many(struct InterfaceHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld,
                                C_BOOL verbose);

/* Optional, any time after initialize: allocates and touches the block buffers of a later solve_many / solve_device / solve_many_sharded with
 * up to `nrhs` right-hand sides (a few GB at config 4's size; the FIRST blocked solve of a handle otherwise pays for them: 0.4 s there).
 * A rank that waits for the factor of another rank (solver_hipmf_broadcast_factor) calls it while the root factorises.  nrhs < 2: no-op. */
int32_t solver_hipmf_prepare_solve_many(struct InterfaceHIPMF *solver, int32_t nrhs);

/* the same two phases with operands already resident in HBM (device pointers) */
int32_t solver_hipmf_factorize_device(struct InterfaceHIPMF *solver, const double *d_values);
int32_t solver_hipmf_solve_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld);

/* Transposed solves A^T x = b with the factor of A: no second analysis or factorisation (UMFPACK's UMFPACK_At system of umfpack_di_solve,
 * which interface_umfpack.c:229 calls with UMFPACK_A; MUMPS's ICNTL(9) in the job-3 call of interface_mumps.c:243-277).  Refined by the rule
 * of solver_hipmf_solve (residual of A^T), Krylov-rescued after a factorisation that replaced pivots.  L D L^T / symmetric storage: the
 * ordinary solve.  _device: nrhs columns, leading dimension ld >= ndim; it remains the ONE-AT-A-TIME form (every column reads the whole
 * factor): many columns belong to solver_hipmf_solve_transpose_many / _many_device below.  Status codes as solver_hipmf_solve;
 * ERROR_HIPMF_INVALID_VALUE for nrhs < 1 or ld < ndim. */
int32_t solver_hipmf_solve_transpose(struct InterfaceHIPMF *solver, double *x, const double *rhs, C_BOOL verbose);
int32_t solver_hipmf_solve_transpose_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld);
/* nrhs right-hand sides of A^T X = B, column-major, leading dimension ld >= ndim; blocks of 16 columns travel through the transposed
 * level launches together (each factor entry is read once per block).  Refinement, Krylov rescue and status codes per column as
 * solver_hipmf_solve_transpose; L D L^T / symmetric storage: solver_hipmf_solve_many / _solve_device.  ERROR_HIPMF_INVALID_VALUE for
 * nrhs < 1 or ld < ndim.  A column's result does not depend on the block or the position it travels in; blocked and one-at-a-time
 * solves agree to rounding, not bit for bit (nrhs == 1 IS the one-at-a-time solve).  d_x may be d_rhs.  Without memory for the block
 * buffers (about 64 ndim + 16 x the solve workspace doubles) the columns are solved one at a time. */
int32_t solver_hipmf_solve_transpose_many(struct InterfaceHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld, C_BOOL verbose);
int32_t solver_hipmf_solve_transpose_many_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld);

/* Sparse right-hand sides and selected solution rows (MUMPS's ICNTL(20); cuDSS and PARDISO have partial solves):
 *   x_sel(k, c) = (A^{-1} B)(sel_idx[k], c),  k < nsel, c < nrhs,  column-major with ldx >= nsel
 * for B (ndim x nrhs) in compressed-column form: column c holds the rows rhs_idx[e] with values rhs_val[e], rhs_ptr[c] <= e < rhs_ptr[c + 1];
 * row indices 0-based and strictly ascending within a column; an empty column gives a zero column.  sel_idx == NULL: all ndim rows
 * (nsel is ignored, ldx >= ndim).  Duplicates in sel_idx are allowed.
 * Blocks of 16 columns travel through level-synchronous launches over the MARKED fronts of the elimination tree only: a non-zero touches
 * the fronts on the path from its front to the root in the forward pass, a wanted row the fronts on the path from the root to its front in
 * the backward pass; every other front would compute exact zeros or values nobody reads.
 * ACCURACY: one UNREFINED pass pair per column -- no iterative refinement and no Krylov rescue: both need the full residual, which reads
 * all of x and A and would undo the pruning (MUMPS treats ICNTL(20) / ICNTL(30) the same way).  The rows returned for a selection are bit
 * for bit the rows of the sel_idx == NULL result of the same columns.
 * The ordinary solve runs instead -- solver_hipmf_solve_device on the expanded columns, refined and rescued as the handle is set up,
 * followed by the selection -- for every block of a handle whose last factorisation replaced pivots (num_perturbed_pivots > 0), and for a
 * block whose marked fronts would read more than the share HIPMF_PRUNE_MAX_SHARE (environment, read per call; default 0.25) of the factor
 * entries a full pass pair reads, and for a block of one column when a full pass pair reads less than HIPMF_PRUNE_MIN_BYTES (default 2e9;
 * a share of 1 or more switches both rules off).  HIPMF_COUNTER_PRUNED_BLOCKS tells how many blocks of the last call ran pruned; dstats[8] is the time
 * between HIP events around the call's uploads, launches and copies (solver_hipmf_inverse_entries: summed over its blocks).
 * _device: every array is a device pointer (the index arrays are read back once: the marking runs on the host).
 * ERROR_HIPMF_INVALID_VALUE: nrhs < 1, an index out of range, decreasing rhs_ptr, unsorted or duplicate rows in a column, nsel < 1 with a
 * non-NULL sel_idx, ldx too small.  ERROR_NEED_INITIALIZATION / ERROR_NEED_FACTORIZATION before the respective phase. */
int32_t solver_hipmf_solve_sparse(struct InterfaceHIPMF *solver, double *x_sel, int32_t ldx, int32_t nrhs, const int32_t *rhs_ptr,
                                  const int32_t *rhs_idx, const double *rhs_val, int32_t nsel, const int32_t *sel_idx, C_BOOL verbose);
int32_t solver_hipmf_solve_sparse_device(struct InterfaceHIPMF *solver, double *d_x_sel, int32_t ldx, int32_t nrhs, const int32_t *d_rhs_ptr,
                                         const int32_t *d_rhs_idx, const double *d_rhs_val, int32_t nsel, const int32_t *d_sel_idx, C_BOOL verbose);
/* values[e] = (A^{-1})(rows[e], cols[e]), e < nent (MUMPS's ICNTL(30)); host arrays, any order, duplicates allowed.  A layer over
 * solver_hipmf_solve_sparse: the distinct columns are sorted by their position in the elimination order, taken 16 at a time as unit
 * vectors, and the rows asked for in a block are its selection.  Accuracy, fallbacks and status codes as solver_hipmf_solve_sparse
 * (ERROR_HIPMF_INVALID_VALUE: nent < 1 or an index out of range); HIPMF_COUNTER_PRUNED_BLOCKS sums over the blocks. */
int32_t solver_hipmf_inverse_entries(struct InterfaceHIPMF *solver, int32_t nent, const int32_t *rows, const int32_t *cols, double *values, C_BOOL verbose);
/* The same for the transposed system (adjoint right-hand sides, rows of the inverse):
 *   x_sel(k, c) = (A^{-T} B)(sel_idx[k], c)
 * Arguments, argument rules, status codes and their order exactly as solver_hipmf_solve_sparse / _device.  The blocks travel through the
 * level-synchronous launches of the blocked transposed solve (solver_hipmf_solve_transpose_many) restricted to the marked fronts; the
 * non-zeros enter through the column permutation and scaling, the wanted rows leave through the row ones.
 * ACCURACY: one UNREFINED transposed pass pair per column, as above; the rows returned for a selection are bit for bit the rows of the
 * sel_idx == NULL result of the same columns.
 * FALLBACKS: the rules of solver_hipmf_solve_sparse (num_perturbed_pivots > 0, HIPMF_PRUNE_MAX_SHARE, HIPMF_PRUNE_MIN_BYTES); the block is
 * then expanded and solved by solver_hipmf_solve_transpose_many_device -- refined and rescued as the handle is set up -- and the rows are
 * selected.  The two thresholds were measured for the ordinary path only (profiles/r09_sparse_rhs.txt); they have NOT been measured for A^T.
 * L D L^T / symmetric storage (A^T = A): solver_hipmf_solve_sparse itself, bit for bit.  HIPMF_COUNTER_PRUNED_* as there;
 * HIPMF_COUNTER_PRUNED_TRANSPOSED_BLOCKS counts the blocks that ran the transposed pruned launches.  Speed against the blocked transposed
 * solve on the expanded block (tools/sparse_rhs.py --transpose, profiles/r16_sparse_rhs_transpose.txt: one run per matrix on one MI355X,
 * wall-clock medians): 1M-DOF 2D matrix, 1 column / 1 row 0.861 against 1.140 ms, 16 columns / 16 rows 0.968 against 3.405 ms; 100^3
 * matrix, 1.943 against 4.884 ms and 2.378 against 10.888 ms. */
int32_t solver_hipmf_solve_sparse_transpose(struct InterfaceHIPMF *solver, double *x_sel, int32_t ldx, int32_t nrhs, const int32_t *rhs_ptr,
                                            const int32_t *rhs_idx, const double *rhs_val, int32_t nsel, const int32_t *sel_idx, C_BOOL verbose);
int32_t solver_hipmf_solve_sparse_transpose_device(struct InterfaceHIPMF *solver, double *d_x_sel, int32_t ldx, int32_t nrhs, const int32_t *d_rhs_ptr,
                                                   const int32_t *d_rhs_idx, const double *d_rhs_val, int32_t nsel, const int32_t *d_sel_idx, C_BOOL verbose);
/* values[e] = (A^{-1})(rows[e], cols[e]) = (A^{-T})(cols[e], rows[e]) through the transposed system: the distinct ROWS are sorted by the
 * position their unit vector enters the transposed elimination at, taken 16 at a time as unit right-hand sides of
 * solver_hipmf_solve_sparse_transpose, and the columns asked for in a block are its selection -- one block per 16 rows of the inverse, where
 * solver_hipmf_inverse_entries needs one per 16 columns.  Arguments, accuracy, fallbacks and status codes as solver_hipmf_inverse_entries. */
int32_t solver_hipmf_inverse_entries_by_rows(struct InterfaceHIPMF *solver, int32_t nent, const int32_t *rows, const int32_t *cols, double *values, C_BOOL verbose);

/* Solve with NEW matrix values on the KEPT factor (MKL PARDISO's "CGS/CG with the LU of a previous step", iparm[3]): solves
 *   A_new x = rhs,  A_new = the structure given to initialize with the `values` given here,
 * by right-preconditioned flexible GMRES started from x = 0, with the factor M of the last factorize as preconditioner.  For callers that
 * change the values often and by little (a new step size scales the shift of gamma M - J, a Jacobian moved in a few rows) and would
 * otherwise call solver_hipmf_factorize again.
 *   mapped = 0: `values` in the CSR order of initialize, as for solver_hipmf_factorize (a symmetric-lower handle: its lower triangle);
 *   mapped = 1: `values` hold the nnz_in numbers of solver_hipmf_set_value_map, as for solver_hipmf_factorize_mapped
 *               (ERROR_HIPMF_INVALID_VALUE without a map).
 *   rel_tol <= 0 selects 1e-12; max_steps <= 0 selects 4 x restart; steps and relres may be NULL.
 * The values pass through the staging of a factorize (value-map gather, mirroring of an expanded symmetric-lower handle) into a buffer of
 * their own: the values that iterative refinement and solver_hipmf_mat_vec_mul read, the factor and every statistic and counter of the
 * ordinary solves (HIPMF_COUNTER_KRYLOV_ITERATIONS, istats[10], the timers) are the same before and after the call.
 * Per step: z = M^{-1} v by ONE unrefined pass pair, w = A_new z by the streaming SpMV, classical Gram-Schmidt applied twice; V, Z and
 * every vector of length ndim live on the device (HIPMF_COUNTER_UPDATED_BASIS_BYTES), the host reads 2 k + 4 doubles per step and solves
 * the Hessenberg least-squares problem by Givens rotations.  Restart length 30, or HIPMF_UPDATED_RESTART (environment, 4 ... 200, read
 * per call); when the bases do not fit in device memory the restart length is halved down to 4, then ERROR_HIP_MALLOC.
 * After every cycle the TRUE residual b - A_new x is recomputed on the device: the call returns 0 once |r|_2 <= rel_tol |b|_2, and
 * HIPMF_WARNING_NOT_CONVERGED when max_steps are used up or a cycle brought no gain (x: the best iterate).  *relres is always that
 * recomputed residual over |b|_2, never the rotation estimate; *steps counts pass pairs.  rhs = 0 gives x = 0, 0 steps, status 0.
 * Every real handle kind is served: general LU, matched / scaled, symmetric-lower L D L^T, symmetric-lower expanded, factors with
 * replaced pivots (a perturbed factor is only a weaker preconditioner).  The complex twin has a form of its own, in complex arithmetic
 * (complex_solver_hipmf_solve_updated, further down).  Several right-hand sides per call: solver_hipmf_solve_updated_many below.  Results are bit-reproducible from call to call (no floating-point atomics).
 * WHEN IT PAYS: NOT MEASURED yet -- no step time and no break-even against solver_hipmf_factorize_device + solver_hipmf_solve_device has been
 * taken on an MI355X; tools/solve_updated.py produces the table (profiles/r10_solve_updated.txt).  No speed-up is claimed until it exists.
 * _device: x, rhs and values are device pointers and no vector crosses the host link.  ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION,
 * ERROR_NEED_FACTORIZATION in this order; ERROR_HIPMF_INVALID_VALUE for a non-finite rel_tol. */
int32_t solver_hipmf_solve_updated(struct InterfaceHIPMF *solver, double *x, const double *rhs, const double *values, int32_t mapped, double rel_tol,
                                   int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose);
int32_t solver_hipmf_solve_updated_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, const double *d_values, int32_t mapped,
                                          double rel_tol, int32_t max_steps, int32_t *steps, double *relres);

/* The same for nrhs right-hand sides: x and rhs are column-major ld x nrhs with ld >= ndim, as for solver_hipmf_solve_many; entries
 * ndim ... ld-1 of every column of x are not written.  values, mapped, rel_tol and max_steps mean what they mean above, max_steps is a
 * limit per column; HIPMF_UPDATED_RESTART and HIPMF_UPDATED_TIMING apply unchanged.  steps and relres: nrhs entries each, or NULL.
 * Every column gets the contract of the single form: relres[c] is the recomputed true residual over |b_c|_2, steps[c] counts the pass
 * pairs in which column c was still iterating, b_c = 0 gives x_c = 0, 0 steps and relres 0, a non-finite |b_c| gives x_c = 0 and relres
 * NaN.  Returns 0 when every column reached the tolerance, HIPMF_WARNING_NOT_CONVERGED when at least one did not (its x_c is its best
 * iterate; relres tells which).  nrhs == 1 is the single form, bit for bit.
 * Method: blocks of 16 columns (the last may be narrower).  Inside a block every column runs its OWN flexible GMRES -- own bases, own
 * Hessenberg matrix and rotations: no Krylov space is shared and no sum is ever formed across columns -- and the columns advance in
 * lockstep: per block step ONE blocked pass pair (the factor is read once for the block), ONE pass over the matrix values and indices,
 * Gram-Schmidt and normalisation batched over the columns, ONE host read of 16 (2 k + 4) doubles.  A column that converged, broke down
 * or used up its steps is masked out of every kernel and rides through the pass pair as zeros; the block goes on until its last column is
 * finished (blocks are neither compacted nor refilled).  The bases of the block form are its own, 61 x 16 x ndim doubles at restart 30
 * (HIPMF_COUNTER_UPDATED_BLOCK_BASIS_BYTES): 7.8 GB at 1M unknowns; halved restart length down to 4 when they do not fit, then
 * ERROR_HIP_MALLOC.  The guarantee of the single form holds: refinement's values, the factor, every statistic and counter of the ordinary
 * solves and the results of later solves are what they were.  Bit-reproducible from call to call.
 * WHEN IT PAYS: see DESIGN.md section 13 (tools/solve_updated.py --nrhs N, profiles/r11_solve_updated_many.txt).
 * ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION in this order; ERROR_HIPMF_INVALID_VALUE for nrhs < 1,
 * ld < ndim, a non-finite rel_tol, or mapped without a map. */
int32_t solver_hipmf_solve_updated_many(struct InterfaceHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld, const double *values,
                                        int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose);
int32_t solver_hipmf_solve_updated_many_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld,
                                               const double *d_values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres);

/* The TRANSPOSED forms: A_new^T x = rhs on the kept factor, for the adjoint systems of the callers above (discrete adjoints and
 * sensitivities of a step with a lagged Jacobian, adjoint right-hand sides after a coefficient update, condition estimates of the updated
 * matrix) without a new factorisation.  Arguments, values / mapped, rel_tol, max_steps, steps, relres, the per-column arrays, the return
 * codes, the argument checks and their order are exactly those of solver_hipmf_solve_updated / _device / _many / _many_device.
 * Method: the same right-preconditioned flexible GMRES from x = 0 (one core serves both; HIPMF_UPDATED_RESTART and HIPMF_UPDATED_TIMING
 * apply) with A_new^T as operator -- products and 2-norm residuals over the rows of A^T, long rows (dense columns of A) summed by a whole
 * workgroup, every sum in a fixed order: bit-reproducible from call to call -- and the UNREFINED transposed pass pair of the kept factor as
 * preconditioner (single: the kernels of solver_hipmf_solve_transpose; blocks of 16: those of solver_hipmf_solve_transpose_many, whose
 * buffers the first call allocates; without memory for them the columns go through the single form one at a time).  A cycle that does not
 * lower the true residual is taken back, non-finite records end a cycle, as above.  After a factorisation that replaced pivots the
 * preconditioner is merely weaker; there is no rescue inside.  L D L^T fronts, symmetric storage or a symmetric matrix expanded inside the
 * handle (A^T = A): the non-transposed form, its bits.
 * NO SIDE EFFECTS: a later solver_hipmf_solve / _solve_transpose and every counter of the ordinary and of the transposed solves
 * (HIPMF_COUNTER_TRANSPOSED_SOLVES, _TRANSPOSED_BLOCKS, _TRANSPOSED_KRYLOV_ITERATIONS, the refinement statistics, the timers) are what they
 * would have been without the call; HIPMF_COUNTER_UPDATED_* report the call as for the non-transposed forms.
 * WHEN IT PAYS (tools/solve_updated.py --transpose, one MI355X, profiles/r17_solve_updated_transpose.txt; DESIGN.md section 13 "The
 * transposed form"): at 1M unknowns a transposed step costs 1.25 ms (the transposed pass pair 1.12) against 0.56 ms for a plain step and
 * 8.4 ms for factorize_device + solve_transpose_device: the single form wins below seven steps and loses to refactorising beyond (15.0
 * against 8.45 ms at 12 steps).  The block form costs 0.213 ms per column and step, 4 - 6 times less than the loop of single calls, but
 * 16 or 64 columns share one refactorisation: it lost to factorize_device + solve_transpose_many_device in every case measured (1.60
 * against 0.83 ms per column at six steps and 16 columns). */
int32_t solver_hipmf_solve_updated_transpose(struct InterfaceHIPMF *solver, double *x, const double *rhs, const double *values, int32_t mapped,
                                             double rel_tol, int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose);
int32_t solver_hipmf_solve_updated_transpose_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, const double *d_values, int32_t mapped,
                                                    double rel_tol, int32_t max_steps, int32_t *steps, double *relres);
int32_t solver_hipmf_solve_updated_transpose_many(struct InterfaceHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld,
                                                  const double *values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres,
                                                  C_BOOL verbose);
int32_t solver_hipmf_solve_updated_transpose_many_device(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld,
                                                         const double *d_values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps,
                                                         double *relres);

/* EXTRA-PRECISE iterative refinement with forward error bounds (Demmel, Hida, Kahan, Li, Mukherjee & Riedy 2006; the scheme of LAPACK's
 * xGERFSX).  solver_hipmf_solve refines on a residual in working precision and stops on the backward error: its x is backward stable, its
 * forward error about cond(A) eps.  Here r = b - A (x + tail) is accumulated in twice the working precision (every product by an FMA,
 * every sum by TwoSum, rounded once) and the iteration watches the corrections: while cond(A) eps < 1 the forward error reaches the order of
 * eps, normwise and componentwise.  A: the values of the last factorize.  Per column, in the user's space:
 *   x <- one unrefined pass pair of b, tail <- 0; per step r as above, dx <- one unrefined pass pair of r,
 *   dn = |dx|_inf / |x|_inf, dc = max_i |dx_i| / |x_i| (0 / 0 counts 0, nonzero / 0 +infinity), rho = dn / dn of the step before;
 *   dn > dn of the step before (or a dx that is not finite): the step is NOT applied, state "no progress".  Else x <- x + dx -- with a
 *   tail (x, tail) <- the renormalised TwoSum of x + dx + tail -- and: dn <= dx_tol converged; not the first step and dn > dn_prev / 2
 *   "no progress"; max_steps steps "step limit".
 * dx_tol <= 0 selects eps, max_steps <= 0 selects 10.  x_tail (NULL allowed): the solution is kept as the unevaluated sum x + x_tail,
 * x the nearest double, and the residual includes the tail -- the error of x + x_tail goes below eps (order cond eps^2); its columns are laid
 * out as those of x.  rhs = 0 gives x = 0 (and tail = 0) in zero steps with every info entry 0.
 * info, 8 doubles per column on the host (info_len_8 of the single forms; NULL allowed):
 *   [0] steps taken (pass pairs after the first)  [1] dn of the last applied step  [2] normwise forward error bound dn / (1 - rho_max)
 *   [3] dc of the last applied step  [4] componentwise bound dc / (1 - rho_max)  [5] rho_max, the largest rho over the applied steps (0 when
 *   there was one)  [6] state: 0 converged, 1 no progress, 2 step limit  [7] 1 when a tail was carried.
 *   Without a tail both bounds are floored by max(10, sqrt(n)) eps; with no applied step or rho_max >= 1 they are +infinity.
 * Returns 0 when every column converged, HIPMF_WARNING_NOT_CONVERGED otherwise (x: the best iterate).
 * _many / _device: column-major ld x nrhs, ld >= ndim (entries ndim .. ld - 1 of a column are not touched), blocks of 16 columns: ONE
 * blocked pass pair, ONE pass over the matrix and ONE update launch per block step, ONE host read of the measures; a finished column is
 * masked out and rides through the pass pairs as zeros.  _device: x, x_tail and rhs are device pointers, info stays on the host.
 * HIPMF_COUNTER_EXTRA_PRECISE_STEPS / _BLOCKS report the last call.  Bit-reproducible from call to call (no floating-point atomics).
 * NO SIDE EFFECTS on the factor, the values, the refinement statistics, any counter, statistic or timer of the ordinary solves, or the
 * bits of a later solve.  After a factorisation that replaced pivots the pass pair is a weaker approximate inverse: the iteration then
 * needs more steps or ends as "no progress"; there is no Krylov rescue inside.
 * WHAT IT COSTS (tools/extra_precise.py, one MI355X, profiles/r18_extra_precise.txt): the start pass pair plus per
 * step one pass pair, one pass over the matrix and one update launch -- at 1M unknowns 0.459 + 0.035 + 0.018 ms -- and a host round
 * trip: 1.51 ms against 0.93 ms for solver_hipmf_solve_device at default refinement (two steps), 7.06 against 4.60 ms for 16 columns; on a
 * shifted Laplacian of 90 000 unknowns with cond 4e10 1.26 against 0.66 ms (four steps).  Host-pointer calls are not yet timed.
 * ERROR_NULL_POINTER (solver, x, rhs), ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION in this order; ERROR_HIPMF_INVALID_VALUE for
 * nrhs < 1 or ld < ndim. */
int32_t solver_hipmf_solve_extra_precise(struct InterfaceHIPMF *solver, double *x, double *x_tail, const double *rhs, double dx_tol, int32_t max_steps,
                                         double *info_len_8, C_BOOL verbose);
int32_t solver_hipmf_solve_extra_precise_many(struct InterfaceHIPMF *solver, double *x, double *x_tail, const double *rhs, int32_t nrhs, int32_t ld,
                                              double dx_tol, int32_t max_steps, double *info, C_BOOL verbose);
int32_t solver_hipmf_solve_extra_precise_device(struct InterfaceHIPMF *solver, double *d_x, double *d_x_tail, const double *d_rhs, int32_t nrhs, int32_t ld,
                                                double dx_tol, int32_t max_steps, double *info);

/* BORDERED SYSTEMS on the kept factor: block elimination, refined on the whole system.
 *     [ A   B ] [x]   [f]      A: the factorised ndim x ndim matrix (the values of the last factorize)
 *     [ C^T D ] [z] = [g]      B, C: ndim x k dense, D: k x k dense, 1 <= k <= HIPMF_BORDER_MAX
 * -- the bordering branch of russell_nonlin's arc-length continuation (k = 1), mean-value and periodicity constraints, fold and
 * branch-point systems, a few Lagrange multipliers, and rank-k changes outside A's pattern: (A + U V^T) x = b is the bordered system with
 * B = U, C = V, D = -I, g = 0 (Woodbury), called as set_border(k, U, V, -I) and solve_bordered(x, NULL, b, NULL, ...).  A symmetric-lower
 * handle keeps its L D L^T factor, which assembling the augmented matrix would give up.
 * solver_hipmf_set_border: B, C column-major ndim x k (ldb, ldc >= ndim; border ROW i of the system is COLUMN i of C), D column-major
 * k x k (ldd >= k).  Copies them to the device, computes W = A^{-1} B with the handle's ordinary blocked refined solve (16 columns per
 * block), S = D - C^T W on the device and the LU of S with partial pivoting in one workgroup; B, C, D, W, LU(S) and the pivots stay in
 * device memory.  border_info (NULL allowed): [0] min |u_ii| / max |u_ii| of S's LU  [1] mantissa and [2] base-10 exponent of det S
 * (the form of solver_hipmf_factorize's determinant: det [A B; C^T D] = det A det S, and [1] x 10^[2] is the arc-length loop's
 * "denominator" for k = 1)  [3] bytes of device memory held for the border.  An exactly zero pivot of S returns
 * HIPMF_WARNING_SINGULAR_MATRIX and leaves NO border set.  k = 0 drops the border and frees its memory (the pointers may be NULL).
 * The border belongs to ONE factorisation: every factorize*, initialize and adopt_factor drops it.
 * solver_hipmf_solve_bordered: x, f column-major ldx x nrhs (ldx >= ndim), z, g column-major ldz x nrhs (ldz >= k); entries beyond
 * ndim (k) of a column are not touched; g NULL means g = 0, z NULL means z is not returned.  Per block of up to 16 columns
 *   y <- one unrefined blocked pass pair of f, t <- g - C^T y, z <- S^{-1} t, x <- y - W z,
 * then iterative refinement on the bordered system: r_f = f - A x - B z, r_g = g - C^T x - D z, the componentwise backward error omega
 * over all ndim + k rows as solver_hipmf_solve defines it (denominators |A||x| + |B||z| + |f| and |C|^T|x| + |D||z| + |g|), (r_f, r_g)
 * through the same four lines, the correction added.  Stop by solve's rule: omega <= eps, or the step did not halve omega (a step that
 * did not lower it is taken back), or after max_steps steps (<= 0 selects 4).  Two separately refined solves with A are NOT backward
 * stable for the bordered system when A is ill-conditioned -- near a fold, where bordering is used; this refinement is (DESIGN.md
 * section 15).  A that is singular to rounding converges slowly or not at all (deflated block elimination is not implemented).
 * info (NULL allowed), 4 doubles per column on the host: [0] steps taken  [1] the last omega  [2] omega before the first step
 * [3] state: 0 converged, 1 no progress, 2 step limit.  Returns 0 whatever the state, as solver_hipmf_solve does after refinement.
 * Per block step ONE blocked pass pair, ONE pass over A, ONE launch per border product, ONE host read of the omegas; a finished column
 * rides on masked out.  Bit-reproducible from call to call (no floating-point atomics).  NO SIDE EFFECTS on the factor, the values, any
 * counter, statistic or timer of the ordinary solves, or the bits of a later solve; no Krylov rescue inside (after a factorisation that
 * replaced pivots the iteration needs more steps or ends as "no progress").
 * _device: B, C, D (x, z, f, g) are device pointers; border_info / info stay on the host.  The host and _device forms give the same bits.
 * HIPMF_COUNTER_BORDER_COLUMNS / _BORDERED_STEPS / _BORDERED_BLOCKS report the border in force and the last call.
 * The residual of a step is accumulated beyond twice the working precision and rounded once (the error-free sums of
 * solver_hipmf_solve_extra_precise): omega <= eps sits at the noise of a residual evaluated in working precision, which would decide by
 * chance between "converged" and "no progress"; with it a refined (x, z) is the exact solution rounded.
 * WHAT IT COSTS (tools/bordered.py, one MI355X, 1M unknowns, profiles/r19_bordered.txt; one step after the start in every case):
 * set_border_device 2.2 / 6.2 / 26.8 ms for k = 1 / 16 / 64; solve_bordered_device, one column: 1.90 / 2.35 / 4.87 ms against 0.92 ms
 * for solver_hipmf_solve_device; 16 columns: 7.4 / 12.5 / 38.7 ms against 6.5 ms -- a wide border is dear, the compensated residual and
 * not the pass pairs is then what is paid for.  k = 1 on host vectors: 2.47 ms against 5.57 ms for two solve calls, two inner products
 * and the combination by hand, and against 6.6 ms per solve (after 472 + 241 ms of analysis and factorisation) for the assembled matrix.
 * ERROR_NULL_POINTER (solver; B, C, D when k > 0; x, f), ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION in this order; then
 * ERROR_HIPMF_INVALID_VALUE for k outside 0 .. HIPMF_BORDER_MAX, a leading dimension that is too small, nrhs < 1, or no border in force
 * (none set, dropped with k = 0, or dropped by a later factorisation). */
#define HIPMF_BORDER_MAX 64
int32_t solver_hipmf_set_border(struct InterfaceHIPMF *solver, int32_t k, const double *B, int32_t ldb, const double *C, int32_t ldc, const double *D, int32_t ldd,
                                double *border_info_len_4, C_BOOL verbose);
int32_t solver_hipmf_set_border_device(struct InterfaceHIPMF *solver, int32_t k, const double *d_B, int32_t ldb, const double *d_C, int32_t ldc, const double *d_D,
                                       int32_t ldd, double *border_info_len_4, C_BOOL verbose);
int32_t solver_hipmf_solve_bordered(struct InterfaceHIPMF *solver, double *x, double *z, const double *f, const double *g, int32_t nrhs, int32_t ldx, int32_t ldz,
                                    int32_t max_steps, double *info, C_BOOL verbose);
int32_t solver_hipmf_solve_bordered_device(struct InterfaceHIPMF *solver, double *d_x, double *d_z, const double *d_f, const double *d_g, int32_t nrhs, int32_t ldx,
                                           int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose);

/* THE TRANSPOSED BORDERED SYSTEM with the border that solver_hipmf_set_border put in force:
 *     [ A^T  C   ] [y]   [p]
 *     [ B^T  D^T ] [w] = [q]      M^T of the system above
 * -- the left vector of fold and branch-point continuation with bordering (M v = e and M^T w = e in every step; the derivatives of the
 * test function are then ONE solver_hipmf_values_outer call, -w^T A_alpha v), and the discrete adjoint of anything computed with
 * solver_hipmf_solve_bordered: M^T [lambda; mu] = [dJ/dx; dJ/dz] (solver_hipmf_solve_adjoint covers A alone).
 * The arguments, info (4 doubles per column: steps, omega, omega before the first step, state), max_steps <= 0 -> 4, w == NULL /
 * q == NULL and the status codes are exactly those of solver_hipmf_solve_bordered.  Per block of up to 16 columns
 *   y0 <- one unrefined blocked TRANSPOSED pass pair of p, t <- q - B^T y0, w <- S^{-T} t, y <- y0 - V w,   V = A^{-T} C,
 * with the SAME S = D - C^T A^{-1} B (S^T = D^T - B^T V): its kept LU is solved transposed.  Then the same refinement on all ndim + k
 * rows of M^T, the residual accumulated beyond twice the working precision and rounded once, the same stopping rule column by column.
 * V and a packed D^T are built at the FIRST transposed call after a set_border (k refined transposed solves, 16 per block) and kept
 * until the border is dropped; a handle that never makes the call allocates and launches nothing for it.  A symmetric-lower handle
 * keeps its L D L^T factor here too (there A^T = A, but M^T != M unless B = C and D = D^T).
 * NO SIDE EFFECTS on any counter, statistic or timer of the other solves (HIPMF_COUNTER_BORDERED_STEPS / _BLOCKS included) or the bits
 * of a later solve; bit-reproducible; the host and _device forms give the same bits.
 * HIPMF_COUNTER_BORDERED_TRANSPOSED_STEPS / _BLOCKS report the last call, HIPMF_COUNTER_BORDER_TRANSPOSED_BYTES the device memory held
 * for V and D^T (0 until the first call).
 * WHAT IT COSTS (tools/bordered_transpose.py, one MI355X, 1M unknowns, profiles/r22_bordered_transpose.txt; one step after the start):
 * one column 3.30 / 3.72 / 6.05 ms for k = 1 / 16 / 64 (the first call after a set_border 6.4 / 11.9 / 40.2 ms); 16 columns 9.3 / 10.1 /
 * 18.7 ms against 7.3 / 12.4 / 37.2 ms for solver_hipmf_solve_bordered_device -- the residual of the transposed form takes the block's
 * columns four at a time.  k = 1 on host vectors: 3.89 ms against 6.76 ms for two solve_transpose calls, two inner products and the
 * combination by hand.  A symmetric-lower handle costs what the plain form costs. */
int32_t solver_hipmf_solve_bordered_transpose(struct InterfaceHIPMF *solver, double *y, double *w, const double *p, const double *q, int32_t nrhs, int32_t ldx,
                                              int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose);
int32_t solver_hipmf_solve_bordered_transpose_device(struct InterfaceHIPMF *solver, double *d_y, double *d_w, const double *d_p, const double *d_q, int32_t nrhs,
                                                     int32_t ldx, int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose);

/* SENSITIVITIES of the solve with respect to the matrix VALUES: tangent (forward) and adjoint (reverse) mode.
 * For J = J(x) with A x = b:  forward,  dx = A^{-1} (db - dA x);  reverse, with g = dJ/dx:  lambda = A^{-T} g = dJ/db  and
 *   dJ/da_ij = -lambda_i x_j  on the sparsity pattern, summed over the right-hand sides,
 * and the two agree: <g, dx> = <grad_values, dvalues> + <lambda, db>.  The transposed solves above give lambda; these calls add the
 * product restricted to the pattern, delivered IN THE ORDER OF THE CALLER'S VALUES, and the product with values other than the
 * factorised ones that the tangent needs.  `mapped` chooses that order as for solver_hipmf_solve_updated:
 *   mapped = 0: the array handed to solver_hipmf_factorize -- the CSR order of initialize; a symmetric-lower handle: its lower triangle,
 *               ONE entry for the two positions (i, j) and (j, i): its gradient is dJ/da_ij + dJ/da_ji, so that <grad, dvalues> is dJ --
 *               also when the handle expanded the matrix to general storage inside (HIPMF_COUNTER_SYM_EXPANDED);
 *   mapped = 1: the nnz_in inputs handed to solver_hipmf_factorize_mapped: input t receives the sum of the gradients of every CSR entry
 *               whose segment lists t (duplicate triplets all receive the entry's gradient).  ERROR_HIPMF_INVALID_VALUE without a map.
 * solver_hipmf_values_outer -- the primitive (needs initialize only; no factor is involved, so it combines with
 * solver_hipmf_solve_updated_transpose as well):
 *   grad[k] = beta grad[k] + alpha sum_{c < ncols} u[i_k + c ldu] w[j_k + c ldw]     for every value k = (i_k, j_k) of the caller,
 *   u, w column-major with ldu, ldw >= ndim; beta == 0: grad is not read (it may hold anything, NaN included).
 *   One lane per stored entry (kernels_sensitivity.hpp); the sum over the columns is ONE chain of fused multiply-adds in ascending c per
 *   entry (symmetric-lower off-diagonals: u_i w_j + u_j w_i of a column first, then the chain; several slots per input: summed in
 *   ascending slot order): the result does not depend on the launch geometry or the device, host and _device forms and repeated calls
 *   give the same bits, and there are no floating-point atomics.  Error per value: at most ncols eps sum_c |u_i w_j| (both products of a
 *   symmetric entry and every slot of an input counted, plus eps of the sum per extra addition; alpha other than +-1 and beta != 0 add
 *   one rounding each).
 * solver_hipmf_solve_tangent: dx = A^{-1} (db - dA x), dA the matrix `dvalues` describe (any values of the handle's structure), db NULL =
 *   zero; x, db, dx column-major ld x nrhs, ld >= ndim, entries ndim .. ld - 1 of a column of dx are not written; dx may be x or db.
 *   dvalues pass through the staging of a factorize into the operator's buffer of the solve_updated forms, the right-hand sides are
 *   formed by their blocked residual kernel, the solve is solver_hipmf_solve_device's, refined and rescued as the handle is set up.
 * solver_hipmf_solve_adjoint: lambda = A^{-T} g by solver_hipmf_solve_transpose_many's path (its refinement and rescue; L D L^T /
 *   symmetric matrices: the ordinary solve), then grad_values = beta grad_values - sum_c lambda_c x_c^T restricted to the pattern, by
 *   ONE outer product over all nrhs columns (the blocks of 16 of the solve do not cut the chain).  lambda = dJ/db; lambda may be g;
 *   grad_values NULL: the solve alone (x may then be NULL).
 * NO SIDE EFFECTS on the factor, the values refinement reads, the determinant, the statistics, the counters of the ordinary and of the
 * transposed solves, or the bits of later solves.  HIPMF_COUNTER_SENS_OUTER_COLUMNS sums the columns of all outer products of the handle,
 * HIPMF_COUNTER_SENS_OUTER_US is the HIP-event time of the outer and scatter kernels of the last one.
 * WHAT IT COSTS (tools/sensitivity.py, one MI355X, one run, 1M unknowns, 5M entries, device-resident operands, profiles/r21_sensitivity.txt;
 * DESIGN.md section 16): the outer kernel 0.021 ms for one column and 0.136 ms for 16 (repeated calls: the operands of one column stay in
 * the last-level cache), 0.095 ms more through a value map in random order; solver_hipmf_solve_adjoint_device 2.44 ms against 2.40 ms for
 * solver_hipmf_solve_transpose_many_device alone, 7.56 against 7.42 ms for 16 columns; the same gradient by hand (lambda and x to the
 * host, a NumPy gather, the gradient back) 21.8 and 293.5 ms.  The host-pointer forms, solve_tangent and the complex calls are not timed.
 * ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION (the two solves) in this order, then
 * ERROR_HIPMF_INVALID_VALUE for ncols / nrhs < 1, a leading dimension below ndim, or mapped = 1 without a map; the solves pass on the
 * status of the solve they wrap.  _device: every array is a device pointer. */
int32_t solver_hipmf_values_outer(struct InterfaceHIPMF *solver, double *grad, const double *u, const double *w, int32_t ncols, int32_t ldu, int32_t ldw,
                                  double alpha, double beta, int32_t mapped);
int32_t solver_hipmf_values_outer_device(struct InterfaceHIPMF *solver, double *d_grad, const double *d_u, const double *d_w, int32_t ncols, int32_t ldu,
                                         int32_t ldw, double alpha, double beta, int32_t mapped);
int32_t solver_hipmf_solve_tangent(struct InterfaceHIPMF *solver, double *dx, const double *x, const double *dvalues, const double *db, int32_t nrhs, int32_t ld,
                                   int32_t mapped);
int32_t solver_hipmf_solve_tangent_device(struct InterfaceHIPMF *solver, double *d_dx, const double *d_x, const double *d_dvalues, const double *d_db, int32_t nrhs,
                                          int32_t ld, int32_t mapped);
int32_t solver_hipmf_solve_adjoint(struct InterfaceHIPMF *solver, double *lambda, double *grad_values, const double *x, const double *g, int32_t nrhs, int32_t ld,
                                   double beta, int32_t mapped);
int32_t solver_hipmf_solve_adjoint_device(struct InterfaceHIPMF *solver, double *d_lambda, double *d_grad_values, const double *d_x, const double *d_g, int32_t nrhs,
                                          int32_t ld, double beta, int32_t mapped);

/* THE INERTIA of the factorised matrix: how many of its eigenvalues are positive, negative and zero, from the signs of the pivots D of
 * L D L^T (Sylvester's law of inertia).  For a handle that factorised K - sigma M with M positive definite, n_negative is the number of
 * eigenvalues of K x = lambda M x below sigma -- the direct solver's own count, and the certificate that a Lanczos run missed none.
 * The symmetric scaling S A S and the symmetric fill-reducing permutation are congruences: they leave the inertia alone.  The signs are
 * counted on the device (integer counts in per-workgroup slots, added in slot order; kernels_eigs.hpp); any of the three outputs may
 * be NULL.  Status codes in this order: ERROR_NULL_POINTER (solver), ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION,
 * ERROR_NOT_AVAILABLE -- for a general handle, for a symmetric-lower handle that was expanded to general storage
 * (HIPMF_COUNTER_SYM_EXPANDED: an LU with a matching) and for HIPMF_COUNTER_SYMMETRIC_LDLT == 0.  The tiled fronts of a symmetric
 * handle take pivot c from row c: their pivots are D.  The fronts of at most 64 rows that one wavefront factorises in LDS search their
 * pivot block on every handle; on diagonally dominant and on most definite matrices the search keeps the diagonal (ties go to it) and
 * their pivots are D as well.  Where it moved a row (indefinite matrices), the signs of that front's pivots say nothing -- but the
 * inertia of the matrix is the sum over the fronts of the inertia of their pivot blocks whatever the order inside them, so such a
 * front's block is multiplied out from its factors and counted by a Bunch-Kaufman elimination in LDS, one wavefront per front
 * (k_eig_inertia_small).  Replaced pivots (num_perturbed_pivots > 0) and zero pivots are reported in
 * n_zero, the other two counts cover the rest, and the call returns HIPMF_WARNING_SINGULAR_MATRIX: the counts are then those of a nearby
 * matrix.  ONE EXCEPTION: a replaced pivot inside a front that was multiplied out again cannot be told from the others any more; it is
 * counted by the sign the perturbed block gives it, not in n_zero, and only the warning status tells.  No side effects on the factor, the statistics or the counters. */
int32_t solver_hipmf_get_inertia(struct InterfaceHIPMF *solver, int64_t *n_positive, int64_t *n_negative, int64_t *n_zero);

/* EIGENPAIRS NEAREST A SHIFT on the kept factor: shift-invert Lanczos (what ARPACK's mode 3 does with any direct solver), with the whole
 * iteration on the device.  The handle holds the factor of A = K - sigma M, which the caller assembled and factorised; the call returns
 * the nev eigenvalues lambda_i of K x = lambda M x with the smallest |lambda_i - sigma|, ordered by that distance, and their eigenvectors.
 * M is given as VALUES ON THE HANDLE'S PATTERN, as solver_hipmf_solve_updated takes `values`: mapped = 0 the CSR order of initialize (a
 * symmetric-lower handle: its lower triangle), mapped = 1 the nnz_in inputs of the value map; m_values NULL: M = I.  They pass through
 * the staging of a factorize into the operator's buffer of the solve_updated forms, not the one refinement and mat_vec_mul read.  M must
 * be symmetric positive definite (a diagonal M is in the pattern); v^T M v <= 0 or not finite at any normalisation returns
 * ERROR_HIPMF_INVALID_VALUE.  The handle must have been initialised from a symmetric lower triangle -- kept as L D L^T or expanded to
 * general storage, Lanczos needs a symmetric operator, not a particular factor --; any other handle returns ERROR_NOT_AVAILABLE.
 * X: column-major ldx x nev, ldx >= ndim, M-orthonormal, the entry of largest modulus of every column (the first on ties) positive.
 * backward_error[i] (NULL allowed) = |A x_i - mu_i M x_i|_inf / ((|A|_inf + |mu_i| |M|_inf) |x_i|_inf) with mu_i = lambda_i - sigma, the
 * TRUE residual recomputed on the device at the end, never the Lanczos estimate.  lambda, backward_error (nev doubles), nconv, steps
 * (NULL allowed): on the host in both forms.
 * Method (Solver::eigs_near_shift, kernels_eigs.hpp): thick-restart Lanczos (Wu & Simon) on A^{-1} M in the M-inner product with full
 * reorthogonalisation.  One step: p = M v_j (the stream SpMV; skipped for M = I), w = A^{-1} p by the path of solver_hipmf_solve_device
 * WITH its refinement, classical Gram-Schmidt twice in the M-inner product against the whole basis with the fixed-order reductions of
 * the solve_updated forms, M w recomputed by SpMV (no second basis), v_{j+1} = w / sqrt(w^T M w).  The host reads 2 (j + 1) + 1 doubles
 * per step and keeps the projected matrix, diagonalised by a cyclic Jacobi method (on the HOST, at every step up to 32 basis vectors
 * and every fourth beyond: near ncv = 128 one such look is of the order of 1e8 flops and is expected to cost more than the step's
 * solve -- there the host, not the device, is the limit; not measured above ncv = 40).  Pair i has converged when
 * |beta s_i| <= tol |theta_i| (ARPACK's rule on the operator, theta_i = 1 / mu_i).  A full basis restarts with
 * k = nev + (ncv - nev) / 2 Ritz vectors (at most ncv - 1), formed in place on the FP64 MFMA (k_eig_rotate).  A breakdown (beta at the
 * rounding level) continues with the next vector of the start sequence, M-orthogonalised; a basis that spans the whole space ends the
 * call with what was found.  v0: the caller's start vector (normalised inside) or NULL: entry i of the vector of sequence number s is
 * (h + 0.5) / 2^31 - 1 with the 32-bit hash h = i 0x9e3779b1 + s 0x85ebca77 + 0x165667b1; h ^= h >> 16; h *= 0x7feb352d;
 * h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16 (wrap-around arithmetic), s = 0 first, the breakdown path takes the following ones
 * (with v0 given it starts at s = 0).  No rand, no clock.
 * Limits and defaults: 1 <= nev <= 64, nev < ndim, nev < ncv <= min(ndim, 128); ncv <= 0 selects min(ndim, max(2 nev + 8, 24)); tol <= 0
 * selects 1e-10; max_steps <= 0 selects 20 ncv.  A basis that does not fit in device memory is halved down to nev + 2 vectors, then
 * ERROR_HIP_MALLOC.  Returns 0 when nev pairs have converged, HIPMF_WARNING_NOT_CONVERGED when max_steps operator applications are
 * used up: the arrays hold the nev Ritz pairs NEAREST the shift (largest |theta|) and no others, the converged ones of them first, and
 * *nconv counts the converged among them -- a pair further away that has converged never takes a place or counts.  *steps counts operator applications.
 * Status codes in this order: ERROR_NULL_POINTER (solver, lambda, X), ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION,
 * ERROR_NOT_AVAILABLE, ERROR_HIPMF_INVALID_VALUE (nev, ncv, ldx < ndim, a non-finite tol or sigma, mapped = 1 without a map).
 * NO SIDE EFFECTS on the factor, the border in force, the values refinement reads, the timers, statistics and existing counters, or the
 * bits of later solves.  BIT-REPRODUCIBLE from call to call and between the two forms: no floating-point atomics.
 * HIPMF_COUNTER_EIGS_STEPS / _RESTARTS / _CONVERGED / _BASIS_BYTES describe the last call; _SOLVE_US / _SPMV_US / _ORTH_US / _ROTATE_US
 * are the HIP-event times of its phases.  The complex handle has no such call.
 * WHAT IT COSTS (tools/eigs.py, one MI355X, one run, 1M unknowns as a lower triangle, profiles/r25_eigs.txt):
 * sigma = 0, M = I, nev = 1 / 6 / 16: 14.9 / 34.8 / 95.5 ms on device vectors (12 / 28 / 72 steps), 15.4 / 40.8 / 112.6 ms on host vectors,
 * against 286 / 620 / 1258 ms for scipy's eigsh driving solver_hipmf_solve on the same handle; a step = the refined solve (1.03 ms;
 * 1.5 ms at an indefinite shift) + 0.08 - 0.18 ms of Gram-Schmidt + 0.13 ms for the three SpMVs with M. */
int32_t solver_hipmf_eigs_near_shift(struct InterfaceHIPMF *solver, int32_t nev, int32_t ncv, double sigma, const double *m_values, int32_t mapped, const double *v0,
                                     double tol, int32_t max_steps, double *lambda, double *X, int32_t ldx, double *backward_error, int32_t *nconv, int32_t *steps,
                                     C_BOOL verbose);
int32_t solver_hipmf_eigs_near_shift_device(struct InterfaceHIPMF *solver, int32_t nev, int32_t ncv, double sigma, const double *d_m_values, int32_t mapped,
                                            const double *d_v0, double tol, int32_t max_steps, double *lambda, double *d_X, int32_t ldx, double *backward_error,
                                            int32_t *nconv, int32_t *steps);

/* Solves exactly as solver_hipmf_solve (the same x, bit for bit), then analyses x against A and b as MUMPS does with
 * ICNTL(11) (the argument shape of solver_mumps_solve, interface_mumps.c:243-247; its RINFOG(4..11) are copied out at
 * interface_mumps.c:266-275 and read by solver_mumps.rs:249-253,415-422).  error_analysis_option: 0 none (array untouched),
 * 1 all eight entries, 2 entries 0 - 4.  With a_i = sum_j |a_ij|, N_A = max a_i, N_x = |x|_inf, r = b - A x, d_i = (|A||x|)_i + |b_i|,
 * I1 = {i : d_i > 1000 n eps (a_i N_x + |b_i|)}, I2 the rest:
 *   [0] N_A  [1] N_x  [2] |r|_inf / (N_A N_x)  [3] omega1 = max_I1 |r_i| / d_i  [4] omega2 = max_I2 |r_i| / ((|A||x|)_i + a_i N_x)
 *   [5] omega1 cond1 + omega2 cond2  [6] cond1  [7] cond2  (Arioli, Demmel & Duff 1989; cond by Hager / Higham's estimator with A^{-1}
 *   and A^{-T}: at most 22 unrefined pass pairs, HIPMF_COUNTER_ANALYSIS_SOLVES).  The statistics of the solve are left as it set them.
 * ERROR_HIPMF_INVALID_VALUE for an option other than 0, 1, 2. */
int32_t solver_hipmf_solve_with_error_analysis(struct InterfaceHIPMF *solver, double *x, const double *rhs, double *error_analysis_array_len_8,
                                               int32_t error_analysis_option, C_BOOL verbose);

/* v = alpha * A * u on the device with the values of the last factorize (host pointers);
 * the CSR SpMV of russell_sparse/src/csr_matrix.rs:709-729 */
int32_t solver_hipmf_mat_vec_mul(struct InterfaceHIPMF *solver, double *v, double alpha, const double *u);

/* perm[new] = old: the fill-reducing permutation applied to rows and columns (ndim entries) */
/* Value refresh through a map (extension for the repeat-factorise callers, SURVEY.md 8f-2: Radau5 / Newton iterations call
 * LinSolTrait::factorize with the same structure and new values every step, radau5.rs:264-303; the reference converts
 * COO -> CSC/CSR on the host each time, csc_matrix.rs:365-505).  After solver_hipmf_initialize:
 *   solver_hipmf_set_value_map: CSR entry j (the order given to initialize) is the sum of the caller's entries
 *     input[seg_idx[q]], seg_ptr[j] <= q < seg_ptr[j+1]  (seg_ptr has nnz+1 entries, seg_ptr[nnz] = nnz_in; e.g. the COO
 *     triplets with their duplicates);
 *   solver_hipmf_factorize_mapped / _device: numeric factorisation from nnz_in caller-ordered values (host / device pointer):
 *     one gather kernel replaces the host conversion. */
int32_t solver_hipmf_set_value_map(struct InterfaceHIPMF *solver, int32_t nnz_in, const int32_t *seg_ptr, const int32_t *seg_idx);
int32_t solver_hipmf_factorize_mapped(struct InterfaceHIPMF *solver, int32_t *effective_ordering, int32_t *effective_scaling,
                                      int32_t *num_perturbed_pivots, double *rcond_estimate, double *determinant_coefficient,
                                      double *determinant_exponent, C_BOOL compute_determinant, C_BOOL verbose,
                                      const double *input_values);
int32_t solver_hipmf_factorize_mapped_device(struct InterfaceHIPMF *solver, const double *d_input_values);

int32_t solver_hipmf_get_permutation(struct InterfaceHIPMF *solver, int32_t *perm);

/* Host-only helper (no device needed): the maximum-product matching + scaling of an n x n CSR matrix that
 * solver_hipmf_initialize applies to weak-diagonal matrices.  matched_row[j] = row matched to column j;
 * |row_scale[i] * a_ij * col_scale[j]| <= 1 with equality on the matched entries.  Returns 0, or
 * ERROR_HIPMF_INVALID_MATRIX when the matrix is structurally singular. */
int32_t hipmf_max_product_matching(int32_t ndim, const int32_t *row_pointers, const int32_t *col_indices, const double *values,
                                   int32_t *matched_row, double *row_scale, double *col_scale);
/* The same for the REAL-EQUIVALENT form (order ndim2 = 2 n: rows / columns 2 k, 2 k + 1 = real and imaginary part of complex row /
 * column k, entry a + i b -> [a -b; b a]) of a complex matrix, as the complex twin applies it (round 4): the matching runs on the
 * moduli of the complex entries, a pair of rows moves as a whole (matched_row[2 k + 1] = matched_row[2 k] + 1) and shares its scales. */
int32_t hipmf_paired_matching(int32_t ndim2, const int32_t *row_pointers, const int32_t *col_indices, const double *values, int32_t *matched_row,
                              double *row_scale, double *col_scale);

/* istats[16]: 0 ndim, 1 nnz(A), 2 nsuper, 3 nlevels, 4 nnz(L) strict, 5 nnz(U) incl. diag, 6 max front,
 *             7 max pivots, 8 perturbed pivots, 9 zero pivots, 10 refinement steps, 11 factor launches,
 *             12 solve launches, 13 pool bytes (persistent factor + arena of working blocks), 14 maximum-product matching in
 *             force (0/1), 15 solves that fell back from the dependency-driven to the level-set launches (hand-off timeout)
 * dstats[16]: 0 flops, 1 gemm flops, 2 ordering s, 3 symbolic total s, 4 assemble ms, 5 factor ms, 6 fwd ms,
 *             7 bwd ms, 8 solve total ms, 9 last residual inf-norm; accumulated since the last reset (HIP events on
 *             the solver's stream): 10 assemble ms, 11 factor ms, 12 #factorizations, 13 forward-solve ms,
 *             14 backward-solve ms, 15 #triangular passes */
int32_t solver_hipmf_get_stats(struct InterfaceHIPMF *solver, int64_t *istats, double *dstats);
int32_t solver_hipmf_reset_timers(struct InterfaceHIPMF *solver);
/* further counters (-1: unknown counter or handle not initialized) */
#define HIPMF_COUNTER_REMATCH 0            /* factorisations that recomputed the maximum-product matching + analysis for new values */
#define HIPMF_COUNTER_WEAK_DIAGONAL_ROWS 1 /* rows with a weak diagonal under the pivot order, values of the last factorize */
#define HIPMF_COUNTER_FUSED_FALLBACKS 2    /* = istats[15] */
#define HIPMF_COUNTER_PERSISTENT_BYTES 3   /* pool: the factor proper (small fronts, E / E' panels) */
#define HIPMF_COUNTER_ARENA_BYTES 4        /* pool: arena of the tiled fronts' working blocks */
#define HIPMF_COUNTER_SYMMETRIC_LDLT 5     /* 1: the tiled fronts are factorised as L D L^T */
#define HIPMF_COUNTER_SYM_EXPANDED 6       /* 1: symmetric-lower input with a weak diagonal (indefinite / saddle-point): mirrored to general
                                            * storage at initialize, factorised by LU with the maximum-product matching; the caller keeps
                                            * handing over lower-triangle values */
#define HIPMF_COUNTER_MID_FRONTS 8        /* fronts one workgroup factorises in one launch per level (k_front_lu: f > 64, at most 32 pivots and 192 off-diagonal rows, LU mode; k_front where switched on) */
#define HIPMF_COUNTER_CHAIN_FALLBACKS 7    /* factorisations repeated with one launch per tiled step after a hand-off of a chained launch timed out */
#define HIPMF_COUNTER_PLAN_DIGEST 9       /* diagnostic: digest of the row structures, pool layout and extend-add task lists of the last initialize
                                             (computed only when HIPMF_PLAN_DIGEST is set in the environment, else 0): equal for every thread count */
#define HIPMF_COUNTER_TAGGED_SOLVE 10     /* 1: the triangular solves of one right-hand side hand their vectors from front to front as data-tagged
                                             words above the wave-subtrees (no completion counters; HIPMF_TAG_SOLVE=0 or fronts of >= 2 048 rows: 0) */
#define HIPMF_COUNTER_GATE_WAITS 11       /* solves of this handle that found the device's gate held by another handle (dependency-driven
                                             launches of two handles are never resident together) */
#define HIPMF_COUNTER_WAVE_FRONTS 12      /* big fronts (f > 64) whose forward solve step is the work of one wavefront (at most 128 rows, 32 pivots) */
#define HIPMF_COUNTER_LEAF_FRONTS 13      /* leaves of the tree that the blocked (many-RHS) solves run in kernels of their own, sixteen columns per wavefront */
#define HIPMF_COUNTER_SPLIT_SLABS 14      /* backward slabs of the blocked solves whose dot products are split over several tasks (levels of few slabs near the root of a large factor) */
#define HIPMF_COUNTER_EVENT_FENCE_FREE 15  /* 1: the events that order this handle's streams are recorded without the system-scope fence (taken on gfx950 under a
                                             HIP 7 runtime only, where it was validated; HIPMF_EVENT_FENCE=1 or any other device / runtime: 0 = default flags) */
#define HIPMF_COUNTER_BLOCK_GROUPS 16      /* blocks of right-hand sides that travel through ONE dependency-driven launch together in the many-RHS solves
                                             (round 6: their latency chains overlap; 1 = one block per launch) -- value of the last blocked solve, 0 before */
#define HIPMF_COUNTER_SYM_WEAK_DIAGONAL 17 /* 1: a symmetric-lower handle that kept its L D L^T plan met a weak diagonal in the values of a factorize
                                             (HIPMF_OPTION_SYM_RECHECK off: nothing was re-analysed; see last_error / verbose) */
#define HIPMF_COUNTER_BCAST_SLICED_BYTES 18 /* bytes of factor that solver_hipmf_broadcast_factor moved as slices over all xGMI links (two point-to-point
                                             steps; three or more ranks, parts of >= 64 MB) instead of through ncclBroadcast, summed over the calls */
#define HIPMF_COUNTER_KRYLOV_ITERATIONS 19 /* steps of the Krylov rescue in the last solve: after a factorisation that PERTURBED pivots (static pivot order:
                                             what UMFPACK's dynamic pivoting, interface_umfpack.c:167, would have avoided) a column whose refined solution
                                             leaves |b - A x|_2 > 1e-13 |b|_2 is finished by flexible GMRES preconditioned with the factorisation
                                             (rank(E) + 1 steps in exact arithmetic); 0: not needed.  HIPMF_KRYLOV=0 switches it off */
#define HIPMF_COUNTER_TRANSPOSED_SOLVES 20 /* right-hand sides solved with A^T (solver_hipmf_solve_transpose / _device / _many / _many_device; the complex twin's A^T / A^H) */
#define HIPMF_COUNTER_ANALYSIS_SOLVES 21   /* pass pairs the condition estimates of the last solver_hipmf_solve_with_error_analysis (complex: _solve_with_error_analysis) took (at most 22) */
#define HIPMF_COUNTER_TRANSPOSED_KRYLOV_ITERATIONS 22 /* steps of the Krylov rescue (A^T as the operator, the transposed pass pair as the preconditioner)
                                                        in the last transposed solve; HIPMF_COUNTER_KRYLOV_ITERATIONS stays the last ordinary solve's */
#define HIPMF_COUNTER_TRANSPOSED_BLOCKS 23 /* 16-column blocks the last solver_hipmf_solve_transpose_many / _many_device ran through the blocked
                                              kernels (0: it fell back to the column loop, or A^T = A and the ordinary blocked solve ran) */
#define HIPMF_COUNTER_PRUNED_FWD_FRONTS 24 /* fronts the forward pass of the last pruned block of the last solver_hipmf_solve_sparse / _device /
                                              solver_hipmf_inverse_entries visited */
#define HIPMF_COUNTER_PRUNED_BWD_FRONTS 25 /* ... and its backward pass (sel_idx == NULL: every front) */
#define HIPMF_COUNTER_PRUNED_BLOCKS 26     /* 16-column blocks of the last such call that ran pruned (0: everything went through the ordinary solve) */
#define HIPMF_COUNTER_PRUNED_BYTES 27      /* bytes of factor entries (8 p f per front and pass) the marked fronts of the last pruned block hold, forward + backward */
#define HIPMF_COUNTER_UPDATED_STEPS 28       /* steps (pass pairs) of the last solver_hipmf_solve_updated / _device */
#define HIPMF_COUNTER_UPDATED_CYCLES 29      /* ... and its restart cycles */
#define HIPMF_COUNTER_UPDATED_BASIS_BYTES 30 /* device bytes held for the bases V and Z of those calls (0 before the first) */
#define HIPMF_COUNTER_UPDATED_PRECOND_US 31  /* HIPMF_UPDATED_TIMING=1 (environment, read per call; else 0): microseconds between HIP events around the pass pairs of the last such call ... */
#define HIPMF_COUNTER_UPDATED_SPMV_US 32     /* ... its SpMVs ... */
#define HIPMF_COUNTER_UPDATED_ARNOLDI_US 33  /* ... and its Gram-Schmidt / normalisation kernels (tools/solve_updated.py) */
#define HIPMF_COUNTER_UPDATED_BLOCKS 34             /* 16-column blocks of the last solver_hipmf_solve_updated_many / _device (0: it was handed to the single form) */
#define HIPMF_COUNTER_UPDATED_COLUMN_STEPS 35       /* sum of steps[c] of that call; with UPDATED_STEPS (there: blocked pass pairs, summed over blocks) it says how full they were */
#define HIPMF_COUNTER_UPDATED_BLOCK_BASIS_BYTES 36  /* device bytes held for the block bases of those calls (UPDATED_BASIS_BYTES stays the single form's) */
#define HIPMF_COUNTER_UPDATED_COMPLEX_ARITHMETIC 37 /* complex handle: 1 when its last solve_updated / _device orthogonalised in complex arithmetic (0 before the first) */
#define HIPMF_COUNTER_PRUNED_TRANSPOSED_BLOCKS 38   /* blocks of the last solver_hipmf_solve_sparse_transpose / _device / solver_hipmf_inverse_entries_by_rows (complex: trans = 1, 2) that ran the transposed pruned launches (0: A^T = A or everything fell back) */
#define HIPMF_COUNTER_EXTRA_PRECISE_STEPS 39        /* pass pairs after the first of the last solver_hipmf_solve_extra_precise / _many / _device (complex: _solve_extra_precise), summed over its block steps */
#define HIPMF_COUNTER_EXTRA_PRECISE_BLOCKS 40       /* 16-column blocks of that call */
#define HIPMF_COUNTER_EXTRA_PRECISE_RESIDUAL_US 41  /* HIPMF_EXTRA_TIMING=1 (environment, read per call; else 0): microseconds between HIP events around the doubled residuals of that call ... */
#define HIPMF_COUNTER_EXTRA_PRECISE_PRECOND_US 42   /* ... its correction pass pairs ... */
#define HIPMF_COUNTER_EXTRA_PRECISE_UPDATE_US 43    /* ... and its update launches (tools/extra_precise.py) */
#define HIPMF_COUNTER_BORDER_COLUMNS 44             /* k of the border in force (solver_hipmf_set_border), 0 when none */
#define HIPMF_COUNTER_BORDERED_STEPS 45             /* refinement steps of the last solver_hipmf_solve_bordered / _device, summed over its blocks */
#define HIPMF_COUNTER_BORDERED_BLOCKS 46            /* 16-column blocks of that call */
#define HIPMF_COUNTER_SENS_OUTER_COLUMNS 47         /* columns summed by the pattern-restricted outer products of this handle (solver_hipmf_values_outer / _device, the gradients of solver_hipmf_solve_adjoint / _device; the complex twin's calls), over all calls */
#define HIPMF_COUNTER_SENS_OUTER_US 48              /* microseconds between HIP events around the outer and scatter kernels of the last such call */
#define HIPMF_COUNTER_BORDERED_TRANSPOSED_STEPS 49  /* refinement steps of the last solver_hipmf_solve_bordered_transpose / _device, summed over its blocks */
#define HIPMF_COUNTER_BORDERED_TRANSPOSED_BLOCKS 50 /* 16-column blocks of that call */
#define HIPMF_COUNTER_BORDER_TRANSPOSED_BYTES 51    /* device bytes held for the transposed side of the border (V = A^{-T} C, D^T): 0 until the first transposed call */
#define HIPMF_COUNTER_COMPLEX_BORDER_COLUMNS 52             /* complex twin: k of the border in force (complex_solver_hipmf_set_border), 0 when none */
#define HIPMF_COUNTER_COMPLEX_BORDERED_STEPS 53             /* complex twin: refinement steps of the last complex_solver_hipmf_solve_bordered / _device, summed over its blocks */
#define HIPMF_COUNTER_COMPLEX_BORDERED_BLOCKS 54            /* 16-column blocks of that call */
#define HIPMF_COUNTER_COMPLEX_BORDERED_TRANSPOSED_STEPS 55  /* complex twin: refinement steps of the last complex_solver_hipmf_solve_bordered_transpose / _device */
#define HIPMF_COUNTER_COMPLEX_BORDERED_TRANSPOSED_BLOCKS 56 /* 16-column blocks of that call */
#define HIPMF_COUNTER_COMPLEX_BORDER_TRANSPOSED_BYTES 57    /* complex twin: device bytes held for V = A^{-H} conj(C) and D^H: 0 until the first transposed call */
#define HIPMF_COUNTER_EIGS_STEPS 58       /* operator applications (refined solves) of the last solver_hipmf_eigs_near_shift / _device */
#define HIPMF_COUNTER_EIGS_RESTARTS 59    /* ... its thick restarts */
#define HIPMF_COUNTER_EIGS_CONVERGED 60   /* ... and the pairs that had converged when it returned (*nconv) */
#define HIPMF_COUNTER_EIGS_BASIS_BYTES 61 /* device bytes held for the Lanczos basis of those calls (0 before the first) */
#define HIPMF_COUNTER_EIGS_SOLVE_US 62    /* microseconds between HIP events around the solves of the last such call ... */
#define HIPMF_COUNTER_EIGS_SPMV_US 63     /* ... its SpMVs with M ... */
#define HIPMF_COUNTER_EIGS_ORTH_US 64     /* ... its Gram-Schmidt, norm and scaling kernels ... */
#define HIPMF_COUNTER_EIGS_ROTATE_US 65   /* ... and its basis rotations (tools/eigs.py) */
int64_t solver_hipmf_get_counter(struct InterfaceHIPMF *solver, int32_t which);

/* Options of LinSolParams that the initialize signature (kept in the shape of interface_cudss.cu:190-203 minus the cuDSS-only
 * arguments) does not carry: set them BEFORE solver_hipmf_initialize (ERROR_ALREADY_INITIALIZED afterwards).
 *   HIPMF_OPTION_MATCHING            lin_sol_params.rs:13 / enums.rs Matching: 0 = None (never), 1 = Auto (default: when values are
 *                                    handed to initialize and the diagonal is weak), 2 = always; every reference variant other than
 *                                    None / Auto selects THE matching this backend has (maximum product + scaling, MC64 job 5)
 *   HIPMF_OPTION_PIVOTING            lin_sol_params.rs:16 / enums.rs Pivoting as an integer (0 Auto, 1 None, 2 GlobalCol, 3 GlobalRow, 4 Diagonal,
 *                                    5 LocalBlock): a REQUEST, as in the cuDSS shim, which reads the effective strategy back after
 *                                    factorize (interface_cudss.cu:485-491).  Every value is accepted (round 6; rounds 1 - 5 refused all but
 *                                    Auto / LocalBlock); the kernels have ONE strategy, readable as HIPMF_OPTION_EFFECTIVE_PIVOTING = 5
 *                                    (LocalBlock): partial pivoting inside the pivot block of a small front / the 32-row diagonal tile of a
 *                                    tiled one; a pivot below pivot_epsilon max|a| is replaced by +-sqrt(machine eps) max|a| and counted;
 *                                    solves after such a factorisation are finished by a Krylov rescue when refinement is not enough
 *                                    (HIPMF_COUNTER_KRYLOV_ITERATIONS), and an exactly zero pivot means status 1 ("singular") only when a
 *                                    probe solve confirms it
 *   HIPMF_OPTION_HYBRID_MEMORY       lin_sol_params.rs:39 (cuDSS hybrid memory, factor 0.01 .. 0.99; interface_cudss.cu:347-380: the factor spills
 *                                    to host memory, factor x total is the device share).  Accepted, range-checked and kept (get_option
 *                                    returns it), and WITHOUT effect on what fits: this backend has no out-of-core path, the factor +
 *                                    working arena live in HBM (288 GB), so the option can neither let a larger matrix through nor --
 *                                    since round 5 -- refuse one that fits the device (rounds 3 - 4 applied factor x total as a cap,
 *                                    which refused matrices the reference accepts).  A matrix that does not fit the free device memory
 *                                    is refused by initialize with the "Not enough memory" string the reference's harness recognises
 *                                    (stats_lin_sol.rs:334-340); the message names the option when it was set
 *   HIPMF_OPTION_SYM_RECHECK         (no reference counterpart) 1: a symmetric-lower handle initialised WITHOUT values looks at the diagonal
 *                                    of the first values it is asked to factorise (solver_hipmf_factorize or _factorize_device) and, when
 *                                    it is weak, redoes the analysis on the mirrored matrix with the matching inside that call (what
 *                                    initialize does when it is handed values).  0 (default since round 5): it keeps its L D L^T plan --
 *                                    the re-analysis changes the plan of this handle only, so peers waiting for its factor
 *                                    (solver_hipmf_broadcast_factor) would be refused and a permutation fetched earlier goes stale
 *   HIPMF_OPTION_ERROR_ESTIMATES     lin_sol_params.rs:50: the componentwise backward error omega of the last solve is always kept
 *   HIPMF_OPTION_CONDITION_NUMBERS   lin_sol_params.rs:55: min|u_ii| / max|u_ii| is always reported by factorize (rcond_estimate)
 * (both readable with solver_hipmf_get_option after solve / factorize: the value, not the flag). */
#define HIPMF_OPTION_MATCHING 0
#define HIPMF_OPTION_PIVOTING 1
#define HIPMF_OPTION_HYBRID_MEMORY 2
#define HIPMF_OPTION_ERROR_ESTIMATES 3
#define HIPMF_OPTION_CONDITION_NUMBERS 4
#define HIPMF_OPTION_SYM_RECHECK 5
#define HIPMF_OPTION_EFFECTIVE_PIVOTING 6 /* get_option only */
int32_t solver_hipmf_set_option(struct InterfaceHIPMF *solver, int32_t option, double value);
int32_t solver_hipmf_get_option(struct InterfaceHIPMF *solver, int32_t option, double *value);

/* ---- many right-hand sides over the GPUs of one node (the reference has no counterpart: lin_solver.rs:51,
 * interface_cudss.cu:275,281 create b and x with ONE column).  One process (or thread) per GPU, every rank runs
 * solver_hipmf_initialize on the same structure (the analysis is deterministic), ONE rank factorises, the factor travels over
 * RCCL / xGMI, every rank solves its block of columns.
 *
 * The numeric factor of a handle = 4 device buffers (solver_hipmf_factor_parts): [0] the persistent part of the front pool (small
 * fronts, E / E' panels), [1] row interchanges (int32 x n), [2] scaling (f64 x n), [3] pivots (f64 x n).  A peer that ran
 * initialize on the same structure may be handed their contents by any transport and then calls solver_hipmf_adopt_factor.
 * solver_hipmf_broadcast_factor does it with ncclBroadcast in 256 MB messages on the solver's stream (plus the matrix values for the
 * refinement SpMV), every rank of `comm` calls it; `comm` is an ncclComm_t -- the caller's own, or one made by
 * hipmf_comm_unique_id (rank 0; send the 128 bytes to the others by any means) + hipmf_comm_init_rank (every rank), so that a host
 * language needs no RCCL binding of its own.  RCCL is loaded on first use (dlopen). */
#define HIPMF_COMM_ID_BYTES 128
int32_t solver_hipmf_factor_parts(struct InterfaceHIPMF *solver, int32_t max_parts, void **d_ptrs, int64_t *bytes); /* returns 4 */
int32_t hipmf_comm_unique_id(void *id128);
int32_t hipmf_comm_init_rank(void **comm, int32_t nranks, const void *id128, int32_t rank);
void hipmf_comm_destroy(void *comm);
int32_t solver_hipmf_broadcast_factor(struct InterfaceHIPMF *solver, void *comm, int32_t root, int32_t rank, double *seconds,
                                      int64_t *bytes_sent);
/* This rank's block of the nrhs_total columns (contiguous blocks, sizes differ by at most one): solves columns
 * [first, first + count) of the n x nrhs_total device arrays d_rhs -> d_x (column-major, leading dimension ld) in place. */
int32_t solver_hipmf_solve_many_sharded(struct InterfaceHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs_total, int32_t ld,
                                        int32_t nranks, int32_t rank, int32_t *first_column, int32_t *num_columns);
int32_t solver_hipmf_adopt_factor(struct InterfaceHIPMF *solver, const double *d_values);

const char *solver_hipmf_last_error(struct InterfaceHIPMF *solver);

/* ---- complex (Complex64) twin ----------------------------------------------------------------------------------------------
 * Replaces russell_sparse/c_code/interface_complex_umfpack.c:40-248 (complex_solver_umfpack_new / _drop / _initialize / _factorize /
 * _solve) behind the Rust ComplexLinSolTrait (russell_sparse/src/complex_lin_solver.rs:12-104, complex_solver_umfpack.rs); Radau5
 * holds one of these next to the real solver (russell_ode/src/radau5.rs:48-51,264-301).  `values`, `x`, `rhs` are interleaved
 * (re, im) pairs: COMPLEX64 of c_code/constants.h:18 = double[2].  0-based CSR of the n x n complex matrix; general_symmetric: the
 * LOWER triangle of a complex SYMMETRIC (not Hermitian) matrix.  The system is solved in its real-equivalent form of order 2 n on
 * the same device path as real matrices; the expansion of the values happens on the device.  Round 4: the pivot searches take the two rows of a
 * complex row together (a complex LU with partial pivoting in real arithmetic), so the determinant IS available: determinant_coefficient_real /
 * _imag / _exponent as umfpack_zi_get_determinant returns them to interface_complex_umfpack.c:143-155,187-200 (det = (re + i im) x 10^exponent;
 * zeros when compute_determinant = 0).  set_value_map / factorize_mapped: as for the real solver, with the
 * caller's complex COO triplets as input (Radau5's K_comp = (alpha + i beta) M - J keeps its structure over the whole run). */
struct InterfaceComplexHIPMF;
struct InterfaceComplexHIPMF *complex_solver_hipmf_new(void);
void complex_solver_hipmf_drop(struct InterfaceComplexHIPMF *solver);
int32_t complex_solver_hipmf_initialize(struct InterfaceComplexHIPMF *solver, int32_t ordering, int32_t scaling, double pivot_epsilon,
                                        int32_t refinement_nstep, C_BOOL verbose, C_BOOL general_symmetric, int32_t ndim,
                                        const int32_t *row_pointers, const int32_t *col_indices, const double *values);
int32_t complex_solver_hipmf_factorize(struct InterfaceComplexHIPMF *solver, int32_t *effective_ordering, int32_t *effective_scaling,
                                       int32_t *num_perturbed_pivots, double *rcond_estimate, double *determinant_coefficient_real,
                                       double *determinant_coefficient_imag, double *determinant_exponent, C_BOOL compute_determinant, C_BOOL verbose,
                                       const double *values);
int32_t complex_solver_hipmf_get_determinant(struct InterfaceComplexHIPMF *solver, double *determinant_coefficient_real,
                                             double *determinant_coefficient_imag, double *determinant_exponent);
int32_t complex_solver_hipmf_solve(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, C_BOOL verbose);
/* nrhs right-hand sides per call, 16 columns per pass pair over the real-equivalent factor: solver_hipmf_solve_many / solver_hipmf_solve_device
 * for the complex handle.  x, rhs: column-major ld x nrhs COMPLEX arrays, interleaved (re, im); ld counts complex elements, ld >= n, columns
 * are 2 ld doubles apart; entries n .. ld - 1 of every column of x are not written; rhs is not changed.  Blocks of 16 columns, refinement and
 * the Krylov rescue after replaced pivots as the handle is set up.  nrhs == 1 is complex_solver_hipmf_solve, bit for bit.  _device: device
 * pointers, 16-byte aligned.  HIPMF_COUNTER_BLOCK_GROUPS as for the real handle.
 * ERROR_NULL_POINTER, ERROR_NEED_FACTORIZATION in this order, then ERROR_HIPMF_INVALID_VALUE (nrhs < 1, ld < n). */
int32_t complex_solver_hipmf_solve_many(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_device(struct InterfaceComplexHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld);
/* conjugate: 1 -> A^H x = b, 0 -> A^T x = b (the real transposed solve of the real-equivalent system; umfpack_zi_solve's UMFPACK_Aat / UMFPACK_At) */
int32_t complex_solver_hipmf_solve_transpose(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, int32_t conjugate, C_BOOL verbose);
/* The same for nrhs columns, 16 per transposed pass pair: solver_hipmf_solve_transpose_many for the complex handle.  x, rhs: column-major
 * ld x nrhs COMPLEX arrays, interleaved; ld counts complex elements, ld >= n; entries n .. ld - 1 of every column of x are not written.
 * conjugate = 1: A^H X = B, the blocked transposed solve of the real-equivalent system; conjugate = 0: A^T X = B, the same solve with the
 * imaginary parts of every block's staged columns negated on entry and exit (one launch per block each way); refinement and the
 * transposed rescue per column run in between, on the A^H system.  nrhs == 1 is complex_solver_hipmf_solve_transpose, bit for bit;
 * HIPMF_TRANSPOSE_BLOCKED=0 or no memory for the block buffers: that call column by column.  HIPMF_COUNTER_TRANSPOSED_BLOCKS counts the
 * blocks.  _device: device pointers; d_x may alias d_rhs.  ERROR_NULL_POINTER, ERROR_NEED_FACTORIZATION in this order, then
 * ERROR_HIPMF_INVALID_VALUE (conjugate not 0 or 1, nrhs < 1, ld < n).  Measured (tools/transpose_many.py --complex, 500 x 500 complex grid,
 * default refinement, profiles/r17_complex_transpose_many.txt): 0.36 ms per column (A^T 0.37) against 2.55 for the column loop. */
int32_t complex_solver_hipmf_solve_transpose_many(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld,
                                                  int32_t conjugate, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_transpose_many_device(struct InterfaceComplexHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld,
                                                         int32_t conjugate);
/* Sparse right-hand sides and selected solution rows for the complex handle (host pointers):
 *   x_sel(k, c) = (op(A)^{-1} B)(sel_idx[k], c),   trans = 0: op(A) = A,  1: A^T,  2: A^H
 * B in compressed-column form as for solver_hipmf_solve_sparse with rhs_val interleaved (re, im) pairs, one per entry of rhs_idx; x_sel
 * interleaved, column-major, ldx counted in COMPLEX elements (ldx >= nsel, or >= n with sel_idx == NULL).  A complex column is one real
 * column of the real-equivalent system: a non-zero of row i is rows 2 i, 2 i + 1, a selected row k rows 2 k, 2 k + 1.  A^H is the
 * transposed real-equivalent system; A^T is A^H with the imaginary parts negated on the way in and out (on the device); a complex-symmetric
 * handle (lower triangle given) has A^T = A: trans = 1 is trans = 0 there.
 * ACCURACY: one UNREFINED pass pair per column, selection rows bit for bit those of the sel_idx == NULL result, as for the real handle.
 * FALLBACKS by the rules of solver_hipmf_solve_sparse (thresholds not measured for A^T / A^H): trans = 0 complex_solver_hipmf_solve_device on
 * the expanded block, trans = 1, 2 the solve of complex_solver_hipmf_solve_transpose column by column, then the selection.
 * Status codes and their order as solver_hipmf_solve_sparse; in addition ERROR_HIPMF_INVALID_VALUE for trans outside 0 .. 2.
 * complex_solver_hipmf_get_counter answers HIPMF_COUNTER_PRUNED_* (fronts of the real-equivalent tree). */
int32_t complex_solver_hipmf_solve_sparse(struct InterfaceComplexHIPMF *solver, double *x_sel, int32_t ldx, int32_t nrhs, const int32_t *rhs_ptr,
                                          const int32_t *rhs_idx, const double *rhs_val, int32_t nsel, const int32_t *sel_idx, int32_t trans, C_BOOL verbose);
/* values[2 e], values[2 e + 1] = re, im of (A^{-1})(rows[e], cols[e]), e < nent; host arrays, any order, duplicates allowed.  Unit column
 * cols[e] is real column 2 cols[e] alone, the rows asked for in a block of 16 columns are its selection.  Accuracy, fallbacks and status
 * codes as solver_hipmf_inverse_entries. */
int32_t complex_solver_hipmf_inverse_entries(struct InterfaceComplexHIPMF *solver, int32_t nent, const int32_t *rows, const int32_t *cols, double *values, C_BOOL verbose);
/* Solves exactly as complex_solver_hipmf_solve (the same x, bit for bit), then the error analysis of solver_hipmf_solve_with_error_analysis
 * for the complex system (the argument shape of complex_solver_mumps_solve; RINFOG(4..11) of zmumps_c, interface_complex_mumps.c:243-280,
 * read by complex_solver_mumps.rs:262-268,429-436).  x, rhs: interleaved complex vectors of length 2 n.  |.| is the complex MODULUS
 * (hypot), n the complex order; a complex-symmetric handle (lower triangle) is analysed with the full matrix.  With
 * a_i = sum_j |a_ij|, N_A = max a_i, N_x = max |x_i|, r = b - A x, d_i = (|A||x|)_i + |b_i|, tau_i = 1000 n eps (a_i N_x + |b_i|),
 * I1 = {i : d_i > tau_i}, I2 the rest, the real weights w1 = d on I1, w2 = (|A||x|) + a N_x on I2 (zeros elsewhere):
 *   [0] N_A  [1] N_x  [2] |r|_inf / (N_A N_x)  [3] omega1 = max_I1 |r_i| / d_i  [4] omega2 = max_I2 |r_i| / ((|A||x|)_i + a_i N_x)
 *   [5] omega1 cond1 + omega2 cond2  [6] cond1 = est| |A^{-1}| w1 |_inf / N_x  [7] cond2 = est| |A^{-1}| w2 |_inf / N_x
 *   (| |A^{-1}| w |_inf = |C|_1, C = diag(w) A^{-H}, by LAPACK zlacn2's iteration: complex signs z / |z| (1 where |z| <= DBL_MIN), no
 *   repeated-sign test, at most 5 iterations + the real alternating vector; the larger of two successive iterates is kept.  At most 22
 *   unrefined pass pairs of the real-equivalent system, HIPMF_COUNTER_ANALYSIS_SOLVES.)  The statistics of the solve are left as it set them.
 * error_analysis_option: 0 none (array untouched), 1 all eight entries, 2 entries 0 - 4; ERROR_HIPMF_INVALID_VALUE for any other. */
int32_t complex_solver_hipmf_solve_with_error_analysis(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, double *error_analysis_array_len_8,
                                                       int32_t error_analysis_option, C_BOOL verbose);
int32_t complex_solver_hipmf_set_value_map(struct InterfaceComplexHIPMF *solver, int32_t nnz_in, const int32_t *seg_ptr, const int32_t *seg_idx);
int32_t complex_solver_hipmf_factorize_mapped(struct InterfaceComplexHIPMF *solver, int32_t *effective_ordering, int32_t *effective_scaling,
                                              int32_t *num_perturbed_pivots, double *rcond_estimate, C_BOOL verbose, const double *input_values);
int32_t complex_solver_hipmf_get_stats(struct InterfaceComplexHIPMF *solver, int64_t *istats, double *dstats); /* istats[0..1]: complex n, nnz */
/* the HIPMF_COUNTER_* values of solver_hipmf_get_counter for the complex twin's handle (-1: unknown counter / not initialized) */
int64_t complex_solver_hipmf_get_counter(struct InterfaceComplexHIPMF *solver, int32_t which);
/* Solve with NEW complex values on the KEPT factor: solver_hipmf_solve_updated for the complex handle, with the same contract (rel_tol <= 0
 * selects 1e-12, max_steps <= 0 selects 4 x restart, HIPMF_UPDATED_RESTART, the halved restart length, *relres the recomputed true residual
 * over |b|_2, *steps the pass pairs, rhs = 0, non-finite |b|, status 0 / HIPMF_WARNING_NOT_CONVERGED, a cycle without gain taken back,
 * bit-reproducible, no floating-point atomics, no side effects on the factor, refinement's values, the determinant, the statistics and
 * counters of the ordinary solves or the bits of a later solve).  x, rhs: interleaved complex vectors (2 n doubles); values: interleaved
 * complex numbers,
 *   mapped = 0: the nnz stored entries in the CSR order of initialize (a complex-symmetric handle: its lower triangle);
 *   mapped = 1: the nnz_in triplets of the value map set for this handle.
 * The handle always carries a value map (identity or triplets) and this call does not swap it: mapped = 0 while the triplet map is
 * installed, or mapped = 1 without one, is ERROR_HIPMF_INVALID_VALUE (last_error says which).
 * Method: flexible GMRES in COMPLEX arithmetic on the interleaved vectors of the real-equivalent system.  Real GMRES on [a -b; b a] would
 * minimise over real coefficients only -- a subset of the complex Krylov space, so never fewer steps, and 20 - 40 % more on the shifted
 * matrices of Radau5 -- and every step is one pass pair over the real-equivalent factor.  Per step: one unrefined pass pair, the
 * real-equivalent streaming SpMV on the staged values, classical Gram-Schmidt twice with complex coefficients <v, w> = sum conj(v_i) w_i
 * (kernels_krylov_complex.hpp: two sums per basis vector, five basis vectors per pass), real norm and scaling; the host reads 4 k + 6
 * doubles per step and keeps a complex Hessenberg matrix with complex Givens rotations.  V and Z are those of the real form for order 2 n:
 * HIPMF_COUNTER_UPDATED_BASIS_BYTES = 61 x 2 n x 8 at restart 30.  HIPMF_COUNTER_UPDATED_STEPS / _CYCLES / _PRECOND_US / _SPMV_US /
 * _ARNOLDI_US as for the real form; HIPMF_COUNTER_UPDATED_COMPLEX_ARITHMETIC is 1 after a call.
 * Every complex handle kind is served: general, complex-symmetric lower, matched / scaled, HIPMF_COMPLEX_PAIRS=0 and factors with replaced
 * pivots (flexible GMRES only needs M^{-1} v to be some vector: a factor that is not exactly complex-linear is a weaker preconditioner).
 * Several right-hand sides per call: complex_solver_hipmf_solve_updated_many below.
 * WHEN IT PAYS (tools/solve_updated.py --complex, one MI355X, one run, profiles/r12_solve_updated_complex.txt): on the 500 x 500 complex
 * shifted grid a step costs 0.46 - 0.47 ms (pass pair 0.37, SpMV 0.03, Arnoldi kernels 0.04 - 0.05) and complex_solver_hipmf_factorize_mapped
 * + complex_solver_hipmf_solve on the same new values 8.1 ms: break-even at 17 steps.  h -> h/2 takes 11 steps and 5.2 ms per call,
 * h -> h/10 17 steps and 7.8 ms.
 * ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION in this order, then ERROR_HIPMF_INVALID_VALUE (a non-finite
 * rel_tol, a `mapped` that does not name the map in force). */
int32_t complex_solver_hipmf_solve_updated(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, const double *values, int32_t mapped,
                                           double rel_tol, int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_updated_device(struct InterfaceComplexHIPMF *solver, double *d_x, const double *d_rhs, const double *d_values,
                                                  int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres);
/* The same for nrhs right-hand sides: solver_hipmf_solve_updated_many for the complex handle, in COMPLEX arithmetic.  x, rhs: column-major
 * ld x nrhs complex arrays, interleaved, ld in complex elements, ld >= n (entries n .. ld - 1 of a column of x are not written); steps,
 * relres: nrhs entries on the host, or NULL.  Per column the contract is that of complex_solver_hipmf_solve_updated: rel_tol, max_steps,
 * HIPMF_UPDATED_RESTART and the halved restart length; relres[c] the recomputed true residual over |b_c|_2; steps[c] the pass pairs in which
 * column c was still iterating; a zero right-hand side gives a zero column, 0 steps, relres 0; a non-finite one a zero column and relres NaN;
 * bit-reproducible; no side effects on the factor, refinement's values, the determinant, the statistics or the bits of later solves;
 * `mapped` has to name the map in force.  Status 0 when every column converged, else HIPMF_WARNING_NOT_CONVERGED.
 * Method: that of solver_hipmf_solve_updated_many -- blocks of 16 columns, every column its own Krylov space (no sum across columns), its
 * own complex Hessenberg matrix and rotations on the host; per block step ONE blocked pass pair over the real-equivalent factor, ONE pass
 * over the matrix, classical Gram-Schmidt twice batched over the columns with complex coefficients (kernels_krylov_complex_blocked.hpp: per
 * column the sums of the single complex kernels in their order), ONE host read of C (4 k + 6) doubles; finished columns are masked out.
 * The step counts are those of the single complex form, not of real GMRES on the 2 n system.  nrhs == 1 is the single form, bit for bit.
 * Block bases: (2 m + 1) x min(nrhs, 16) x 2 n doubles, HIPMF_COUNTER_UPDATED_BLOCK_BASIS_BYTES; HIPMF_COUNTER_UPDATED_BLOCKS,
 * _UPDATED_COLUMN_STEPS, _UPDATED_STEPS (blocked pass pairs) and _UPDATED_CYCLES as for the real block form.
 * WHEN IT PAYS (tools/solve_updated.py --complex --nrhs N, one MI355X, one run per N, profiles/r13_solve_updated_complex_many.txt): 500 x 500
 * complex shifted grid, h -> h/2 (11 steps per column), medians per column: N = 16: (a) this call 1.396 ms, (b) N single
 * complex_solver_hipmf_solve_updated_device calls 5.141 ms, (c) complex_solver_hipmf_factorize_mapped + complex_solver_hipmf_solve_many
 * 0.823 ms; N = 64: (a) 1.400, (b) 4.995, (c) 0.418 ms.  The block form is 3.6 - 3.7 times faster than the loop of single calls; with 16 or
 * more columns and 11 steps the refactorisation, whose cost the columns share, is cheaper still: by these figures the call pays against
 * (c) for few columns or few steps (a block step of 16 columns costs 2.0 ms, (c) about 8 ms + 0.3 ms per column).
 * ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION in this order, then ERROR_HIPMF_INVALID_VALUE (nrhs < 1, ld < n,
 * a non-finite rel_tol, then a `mapped` that does not name the map in force). */
int32_t complex_solver_hipmf_solve_updated_many(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld,
                                                const double *values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres,
                                                C_BOOL verbose);
int32_t complex_solver_hipmf_solve_updated_many_device(struct InterfaceComplexHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld,
                                                       const double *d_values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps,
                                                       double *relres);
/* solver_hipmf_solve_extra_precise for the complex handle: the same iteration on the real-equivalent system, the residual in twice the
 * working precision per real component; x, x_tail (NULL allowed), rhs: interleaved complex vectors (2 n doubles).  The measures dn and dc
 * take the MODULI of the complex components, not their real and imaginary parts; the floor of the bounds is max(10, sqrt(n)) eps with
 * the complex order n.  info, the return codes and the argument checks as for the real handle. */
int32_t complex_solver_hipmf_solve_extra_precise(struct InterfaceComplexHIPMF *solver, double *x, double *x_tail, const double *rhs, double dx_tol,
                                                 int32_t max_steps, double *info_len_8, C_BOOL verbose);
/* The TRANSPOSED forms for the complex handle: A_new^H z = c (conjugate = 1) or A_new^T z = c (conjugate = 0) on the kept factor, as
 * solver_hipmf_solve_updated_transpose and its three siblings for the real handle, in the complex arithmetic of the forms above.
 * conjugate = 1 is the transposed real-equivalent system: operator A_new^H, preconditioner the unrefined transposed pass pair.
 * conjugate = 0 is the same iteration on conjugated data (A_new^T z = c <=> A_new^H conj(z) = conj(c)): the imaginary parts of c are
 * negated on entry (in a staging copy: c is not changed) and those of z on exit; steps and relres are those of the A^H iteration on
 * conj(c), and z equals conj of the conjugate = 1 result for conj(c) bit for bit.  A complex-symmetric handle (lower triangle given) has
 * A^T = A: conjugate = 0 is the non-transposed form there, its bits.  ld counts complex elements.  Checks and their order: those of the
 * non-transposed complex forms, with ERROR_HIPMF_INVALID_VALUE for a conjugate other than 0 or 1 right after ERROR_NEED_FACTORIZATION;
 * the map check comes last.  No side effects on the handle, as for the real forms.  Measured (tools/solve_updated.py --complex
 * --transpose, 500 x 500 complex shifted grid, conjugate = 1, profiles/r17_solve_updated_transpose.txt): 1.22 ms per step against 9.6 ms
 * for factorize_mapped + solve_transpose, break-even at eight steps (h -> h/2 takes 11: 13.4 ms, a loss); block form 2.27 ms per column
 * against 13.35 for the loop of single calls and 0.97 (16 columns) for factorize_mapped + solve_transpose_many. */
int32_t complex_solver_hipmf_solve_updated_transpose(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, const double *values, int32_t mapped,
                                                     double rel_tol, int32_t max_steps, int32_t *steps, double *relres, int32_t conjugate, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_updated_transpose_device(struct InterfaceComplexHIPMF *solver, double *d_x, const double *d_rhs, const double *d_values,
                                                            int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres, int32_t conjugate);
int32_t complex_solver_hipmf_solve_updated_transpose_many(struct InterfaceComplexHIPMF *solver, double *x, const double *rhs, int32_t nrhs, int32_t ld,
                                                          const double *values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps,
                                                          double *relres, int32_t conjugate, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_updated_transpose_many_device(struct InterfaceComplexHIPMF *solver, double *d_x, const double *d_rhs, int32_t nrhs,
                                                                 int32_t ld, const double *d_values, int32_t mapped, double rel_tol, int32_t max_steps,
                                                                 int32_t *steps, double *relres, int32_t conjugate);
/* The sensitivity calls for the complex handle (host pointers; u, w, x, g, dx, lambda interleaved complex columns, leading dimensions in
 * complex elements >= n; the gradient and dvalues interleaved complex numbers in the order of the values the handle is fed: mapped = 0 the
 * nnz stored entries of initialize -- a complex-symmetric handle: its lower triangle, an off-diagonal entry standing for both positions --,
 * mapped = 1 the nnz_in triplets of the value map; `mapped` has to name the map in force, as for complex_solver_hipmf_solve_updated).
 * complex_solver_hipmf_values_outer:  grad[k] = beta grad[k] + alpha sum_c u[i_k, c] op(w[j_k, c]),  op = conj with conjugate_w = 1,
 *   alpha and beta real; directly on the complex entries: per entry two chains of fused multiply-adds (real and imaginary part) in
 *   ascending c, the same bits from call to call.
 * complex_solver_hipmf_solve_tangent:  dx = A^{-1} (db - dA x), as solver_hipmf_solve_tangent on the real-equivalent system.
 * complex_solver_hipmf_solve_adjoint, for a REAL-valued J of the complex x, with g = dJ/dRe x + i dJ/dIm x (twice the Wirtinger
 *   derivative with respect to conj x), so that dJ = Re <g, dx>, <a, b> = sum conj(a_i) b_i.  From A dx = db - dA x,
 *     dJ = Re g^H A^{-1} (db - dA x) = Re lambda^H db - Re sum_ij conj(lambda_i) dA_ij x_j     with  lambda = A^{-H} g,
 *   and -conj(lambda_i) x_j = conj(-lambda_i conj(x_j)).  Hence
 *     lambda = A^{-H} g  (complex_solver_hipmf_solve_transpose_many's conjugate = 1 path),
 *     grad_k = beta grad_k - sum_c lambda[i_k, c] conj(x[j_k, c]),
 *     dJ = Re <grad, dA> + Re <lambda, db>:  Re grad is the derivative with respect to Re a_ij, Im grad with respect to Im a_ij.
 *   grad_values NULL: the solve alone; lambda may be g.
 * Status codes and their order as for the real handle (the map check comes last); ERROR_HIPMF_INVALID_VALUE also for a conjugate_w other
 * than 0 or 1.  No side effects on the handle, as for the real handle.  There are no _device forms yet. */
int32_t complex_solver_hipmf_values_outer(struct InterfaceComplexHIPMF *solver, double *grad, const double *u, const double *w, int32_t ncols, int32_t ldu,
                                          int32_t ldw, double alpha, double beta, int32_t mapped, int32_t conjugate_w);
int32_t complex_solver_hipmf_solve_tangent(struct InterfaceComplexHIPMF *solver, double *dx, const double *x, const double *dvalues, const double *db, int32_t nrhs,
                                           int32_t ld, int32_t mapped);
int32_t complex_solver_hipmf_solve_adjoint(struct InterfaceComplexHIPMF *solver, double *lambda, double *grad_values, const double *x, const double *g, int32_t nrhs,
                                           int32_t ld, double beta, int32_t mapped);
/* BORDERED SYSTEMS for the complex handle: solver_hipmf_set_border, _solve_bordered and _solve_bordered_transpose in complex arithmetic,
 *     [ A   B ] [x]   [f]      A: the factorised complex n x n matrix
 *     [ C^T D ] [z] = [g]      B, C: n x k complex dense, D: k x k complex dense, 1 <= k <= HIPMF_COMPLEX_BORDER_MAX
 * -- Hopf-point location and continuation ([J - i omega M, B; C^T, D] with k = 1 or 2, and the same system transposed or adjoint in every
 * Newton step), constrained complex-shifted systems (K + i omega C - omega^2 M with constraints or Lagrange multipliers), and rank-k
 * changes outside the pattern: (A + U V^T) x = b is the bordered system with B = U, C = V, D = -I, g = 0 (Woodbury; Radau5's complex
 * system with a Broyden-type correction of J).
 * C^T is the PLAIN transpose, not the Hermitian one: border row i of the system is column i of C, as for the real handle.  All arrays
 * are interleaved (re, im) doubles, column-major; leading dimensions count COMPLEX entries: ldb, ldc, ldx >= n; ldd, ldz >= k.
 * HIPMF_COMPLEX_BORDER_MAX = 32: the real-equivalent border then has at most HIPMF_BORDER_MAX = 64 columns, what the products of the
 * real form are built for.
 * complex_solver_hipmf_set_border computes W = A^{-1} B with k refined solves (16 per block), S = D - C^T W and its LU as a COMPLEX
 * k x k matrix, partial pivoting by modulus.  border_info (NULL allowed): [0] min |u_ii| / max |u_ii| of that LU  [1], [2] real and
 * imaginary mantissa and [3] base-10 exponent of det S, in the form of complex_solver_hipmf_get_determinant: det M = det A det S
 * [4] bytes of device memory held for the border.  An exactly zero pivot of S returns HIPMF_WARNING_SINGULAR_MATRIX and leaves NO border
 * set.  k = 0 drops the border (the pointers may be NULL); every factorize*, initialize and adopted factor drops it.
 * complex_solver_hipmf_solve_bordered: block elimination, then iterative refinement on the whole system exactly as the real form does
 * it.  The residual of all n + k complex rows is accumulated beyond twice the working precision and rounded once; omega is the
 * componentwise backward error per COMPLEX row on complex moduli, |r_i| / (sum_j |a_ij||x_j| + sum_j |b_ij||z_j| + |f_i|), not that of
 * the 2 n real rows taken separately.  z / g may be NULL (z not returned; g = 0).  max_steps <= 0 selects 4.  info (NULL allowed):
 * 4 doubles per column -- steps, last omega, omega before the first step, state 0 converged / 1 no progress / 2 step limit; the call
 * returns 0 whatever the state.  No Krylov rescue inside.
 * complex_solver_hipmf_solve_bordered_transpose: M^H [y; w] = [p; q] (conjugate = 1), M^H = [A^H conj(C); B^H D^H], or M^T [y; w] =
 * [p; q] (conjugate = 0), M^T = [A^T C; B^T D^T]; `conjugate` as in complex_solver_hipmf_solve_transpose.  V = A^{-H} conj(C) and D^H
 * and the LU of its own Schur complement D^H - B^H V are built at the FIRST transposed call after a set_border (k refined transposed
 * solves; an exactly zero pivot there returns HIPMF_WARNING_SINGULAR_MATRIX from that call) and serve both: conjugate = 0 runs the loop
 * of M^H on conjugated data (p and q conjugated in a staging copy on entry, y and w on exit).  A handle that never makes the call
 * allocates and launches nothing for it.
 * NO SIDE EFFECTS on the factor, the values, any counter, statistic or timer of another solve (the plain and the transposed form do not
 * move each other's counters) or the bits of a later solve; bit-reproducible; the host and _device forms give the same bits.
 * HIPMF_COUNTER_COMPLEX_BORDER_COLUMNS .. _COMPLEX_BORDER_TRANSPOSED_BYTES (52 - 57) report the border in force and the last calls.
 * WHAT IT COSTS (tools/bordered_complex.py, one MI355X, the 500 x 500 complex shifted grid of tools/solve_updated.py --complex,
 * profiles/r24_bordered_complex.txt; one step after the start in every case): set_border_device 2.0 / 4.8 / 8.5 ms for k = 1 / 16 / 32;
 * solve_bordered_device, one column: 1.51 / 1.93 / 2.65 ms against 0.77 ms for complex_solver_hipmf_solve_device; 16 columns: 7.4 /
 * 11.0 / 16.2 ms against 3.2 ms -- two to five times the plain solve, dearest on a wide border with many columns (the compensated
 * complex residual).  Transposed, conjugate = 1: 3.12 / 3.54 / 4.22 ms for one column (the first call after a set_border 6.1 / 8.3 /
 * 16.9 ms), 8.2 / 9.6 / 11.9 ms for 16 -- dearer than the plain form for one column, cheaper for 16 columns from k = 16 on; conjugate =
 * 0 costs 0.03 - 0.2 ms more.  k = 1 on host vectors: 1.78 ms against 3.36 ms for two complex_solver_hipmf_solve calls, two inner
 * products and the combination by hand.  The border holds three packed 2n x kp arrays (kp = 2k rounded up to 16), the transposed
 * side a fourth: 784 MB + 256 MB at k = 32 on 250 000 unknowns.
 * ERROR_NULL_POINTER, ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION in this order, then ERROR_HIPMF_INVALID_VALUE (k outside
 * 0 .. HIPMF_COMPLEX_BORDER_MAX, a leading dimension that is too small, nrhs < 1, a conjugate other than 0 or 1, no border in force). */
#define HIPMF_COMPLEX_BORDER_MAX 32
int32_t complex_solver_hipmf_set_border(struct InterfaceComplexHIPMF *solver, int32_t k, const double *B, int32_t ldb, const double *C, int32_t ldc, const double *D,
                                        int32_t ldd, double *border_info_len_5, C_BOOL verbose);
int32_t complex_solver_hipmf_set_border_device(struct InterfaceComplexHIPMF *solver, int32_t k, const double *d_B, int32_t ldb, const double *d_C, int32_t ldc,
                                               const double *d_D, int32_t ldd, double *border_info_len_5, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_bordered(struct InterfaceComplexHIPMF *solver, double *x, double *z, const double *f, const double *g, int32_t nrhs, int32_t ldx,
                                            int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_bordered_device(struct InterfaceComplexHIPMF *solver, double *d_x, double *d_z, const double *d_f, const double *d_g, int32_t nrhs,
                                                   int32_t ldx, int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_bordered_transpose(struct InterfaceComplexHIPMF *solver, double *y, double *w, const double *p, const double *q, int32_t nrhs,
                                                      int32_t ldx, int32_t ldz, int32_t conjugate, int32_t max_steps, double *info, C_BOOL verbose);
int32_t complex_solver_hipmf_solve_bordered_transpose_device(struct InterfaceComplexHIPMF *solver, double *d_y, double *d_w, const double *d_p, const double *d_q,
                                                             int32_t nrhs, int32_t ldx, int32_t ldz, int32_t conjugate, int32_t max_steps, double *info,
                                                             C_BOOL verbose);
const char *complex_solver_hipmf_last_error(struct InterfaceComplexHIPMF *solver);

/* plain device-memory helpers so that callers need no HIP binding of their own */
void *hipmf_device_malloc(size_t bytes);
void hipmf_device_free(void *ptr);
int32_t hipmf_memcpy_h2d(void *dst, const void *src, size_t bytes);
int32_t hipmf_memcpy_d2h(void *dst, const void *src, size_t bytes);
int32_t hipmf_device_synchronize(void);
int32_t hipmf_device_count(void);
int32_t hipmf_device_mem_info(size_t *free_bytes, size_t *total_bytes); /* hipMemGetInfo of the calling thread's device */
/* Measured device-to-device copy rate in GB/s (read + written bytes over HIP-event time, `bytes` per copy, best of `reps`):
 * the achievable-HBM denominator bench.py reports beside the 8 TB/s spec. */
int32_t hipmf_device_copy_bandwidth(int64_t bytes, int32_t reps, double *gb_per_s);
/* Measured rate of v_mfma_f64_16x16x4_f64 in TFLOP/s (back-to-back MFMAs on four independent accumulators per wave, operands in
 * registers, `workgroups` x 256 threads, best of two timed launches): the achievable-MFMA denominator bench.py reports beside the
 * 78.6 TFLOP/s spec. */
int32_t hipmf_device_mfma_rate(int32_t workgroups, int32_t iters, double *tflops);
int32_t hipmf_set_device(int32_t device); /* selects the device later solver_hipmf_new() calls of this thread bind to */

/* ---- finite-difference Laplacian assembled on the device -------------------------------------------------
 * Replaces, for callers that keep the matrix in HBM, Fdm2d::get_matrices_sps of russell_pde
 * (/root/reference/russell_pde/src/fdm_2d.rs:603-649; molecule :376-386; mirrored / wrapped neighbours :944-979; local numbering
 * russell_pde/src/equation_handler.rs:153-190): the COO triplets of K-bar (unknown x unknown) and K-check (unknown x prescribed)
 * in the reference's order -- unknown nodes ascending, per node CUR, LEF, RIG, BOT, TOP -- duplicates of mirrored ghost nodes kept.
 *   nz = 1: the reference's 2D operator; nz > 1: the 7-point analogue (two more molecule entries: the z neighbours)
 *   sym: 0 every entry (Sym::No / YesFull), 1 lower triangle (Sym::YesLower), 2 upper triangle (Sym::YesUpper)
 *   prescribed: HOST array of nx*ny*nz bytes, non-zero = node with an essential boundary condition (NULL: none)
 * hipmf_fdm_new returns NULL on invalid sizes or allocation failure.  The *_device calls write DEVICE arrays of the sizes reported by
 * hipmf_fdm_dims (the K-check pointers may be NULL when np = 0); indices are the local numbers iu / ip.  Values can be regenerated
 * for new coefficients without touching the structure and handed to solver_hipmf_factorize_mapped_device. */
void *hipmf_fdm_new(int32_t nx, int32_t ny, int32_t nz, int32_t periodic_x, int32_t periodic_y, int32_t periodic_z, int32_t sym,
                    const uint8_t *prescribed);
void hipmf_fdm_drop(void *fdm);
int32_t hipmf_fdm_dims(const void *fdm, int64_t *nu, int64_t *np, int64_t *nnz_bar, int64_t *nnz_check);
int32_t hipmf_fdm_structure_device(const void *fdm, int32_t *d_bar_i, int32_t *d_bar_j, int32_t *d_check_i, int32_t *d_check_j);
int32_t hipmf_fdm_values_device(const void *fdm, double dx, double dy, double dz, double kx, double ky, double kz, double alpha,
                                double *d_bar_values, double *d_check_values);
/* The Lagrange-multiplier form of the same operator: replaces Fdm2d::get_matrices_lmm (fdm_2d.rs:672-748) -- the augmented matrix
 *   M = [K C^T; C 0]  of order neq + nlag  (neq = nx*ny*nz: every node keeps its equation; nlag = prescribed nodes)
 * as COO triplets in the reference's order: the molecule of every node ascending (entries above / below the diagonal skipped for
 * lower / upper storage), then per prescribed node, ascending, the entry of C (row neq + ip, column m) and / or of C^T (lower storage
 * keeps C, upper C^T, general storage both, C first); global node numbers as indices.  The matrix is a saddle-point system: handed to
 * solver_hipmf_initialize WITH values (or to a symmetric-lower handle) it takes the matched path, no perturbed pivots.  The constraint
 * matrix C of the reference's second return value is the (row - neq, column) view of the C entries.  The first call builds the offsets. */
int32_t hipmf_fdm_lmm_dims(void *fdm, int64_t *neq, int64_t *nlag, int64_t *nnz);
int32_t hipmf_fdm_lmm_structure_device(void *fdm, int32_t *d_i, int32_t *d_j);
int32_t hipmf_fdm_lmm_values_device(void *fdm, double dx, double dy, double dz, double kx, double ky, double kz, double alpha, double *d_values);

#ifdef __cplusplus
}
#endif
#endif
