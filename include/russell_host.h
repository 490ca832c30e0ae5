/*
 * russell_host.h -- flat C API of the host-side mirror of russell_sparse's Rust layer
 * (russell_amd/csrc/host/russell_host.hpp).  It exists because this image has no Rust toolchain: the
 * layer ABOVE the solver C-ABI (include/russell_hipmf.h) -- CooMatrix / CscMatrix / CsrMatrix, LinSolParams,
 * Genie, LinSolver (LinSolTrait), VerifyLinSys, StatsLinSol, read_matrix_market -- is written in C++ with
 * the reference's names, argument meaning and error strings, and exported here for ctypes and other FFIs.
 * Functions that can fail return a static error string (NULL = Ok), the analogue of Rust's StrError.
 * Reference files mirrored: russell_sparse/src/{coo,csc,csr}_matrix.rs, lin_solver.rs, lin_sol_params.rs,
 * enums.rs, verify_lin_sys.rs, stats_lin_sol.rs, read_matrix_market.rs, solver_cudss.rs (template of SolverHIPMF).
 */
#ifndef RUSSELL_HOST_H
#define RUSSELL_HOST_H
#include <inttypes.h>
#ifdef __cplusplus
extern "C" {
#endif

/* enums.rs: Sym {No, YesFull, YesLower, YesUpper} = 0..3; Genie {Hipmf, Umfpack, Mumps, Cudss} = 0..3;
 * Ordering {Amd, Amf, Auto, Best, BtfColamd, Cholmod, Colamd, Metis, No, Pord, Qamd, Scotch} = 0..11;
 * Scaling {Auto, Column, Diagonal, Max, No, RowCol, RowColIter, RowColRig, Sum} = 0..8;
 * MMsym {LeaveAsLower, SwapToUpper, MakeItFull} = 0..2 */
struct RhParams { /* lin_sol_params.rs:5-107, the fields this backend honours */
    int32_t ordering, scaling;
    int32_t has_pivot_epsilon;
    double pivot_epsilon;
    int32_t has_refinement_nstep, refinement_nstep;
    int32_t positive_definite, compute_determinant, verbose;
    /* round 3 (appended): lin_sol_params.rs:13-16,39,50,55 */
    int32_t matching, pivoting; /* enums.rs Matching (0 None, 1 Auto, 2.. named variants), Pivoting (0 Auto, 1 None, 2 GlobalCol, 3 GlobalRow, 4 Diagonal, 5 LocalBlock) */
    int32_t has_hybrid_memory_factor;
    double hybrid_memory_factor;
    int32_t compute_error_estimates, compute_condition_numbers;
};

void rh_set_hipmf_library(const char *path);

void *rh_coo_new(int64_t nrow, int64_t ncol, int64_t max_nnz, int32_t sym, const char **err);
void rh_coo_free(void *coo);
const char *rh_coo_put(void *coo, int64_t i, int64_t j, double aij);
void rh_coo_reset(void *coo);
void rh_coo_info(void *coo, int64_t *nrow, int64_t *ncol, int64_t *nnz, int64_t *max_nnz, int32_t *sym);
void rh_coo_arrays(void *coo, const int32_t **ai, const int32_t **aj, const double **ax);
const char *rh_coo_mat_vec_mul(void *coo, double *v, int64_t nv, double alpha, const double *u, int64_t nu);

/* coo_matrix.rs:629 (v += alpha A u), :708 (v = alpha A^T u), :738 assign, :779 add, :823 put_lagrange_block, :468 to_dense
 * (row-major nrow x ncol), :872 get_actual_nnz */
/* coo_matrix.rs:246-291 (NumCooMatrix::from): a COO matrix from ready triplet arrays (copied) */
void *rh_coo_from(int64_t nrow, int64_t ncol, int64_t nnz, const int32_t *row_indices, const int32_t *col_indices, const double *values, int32_t sym,
                  const char **err);
const char *rh_coo_mat_vec_mul_update(void *coo, double *v, int64_t nv, double alpha, const double *u, int64_t nu);
const char *rh_coo_mat_t_vec_mul(void *coo, double *v, int64_t nv, double alpha, const double *u, int64_t nu);
const char *rh_coo_assign(void *coo, double alpha, void *other);
const char *rh_coo_add(void *coo, double alpha, void *other);
const char *rh_coo_put_lagrange_block(void *coo, void *bb);
const char *rh_coo_to_dense(void *coo, double *a_row_major, int64_t len);
int64_t rh_coo_actual_nnz(void *coo);
/* csc_matrix.rs:197-262 / csr_matrix.rs:193-257: validated constructors from ready arrays (np pointers, nv indices / values, copied);
 * csc_matrix.rs:702 / csr_matrix.rs:676: dense row-major copies */
void *rh_csc_new(int64_t nrow, int64_t ncol, const int32_t *col_pointers, int64_t np, const int32_t *row_indices, const double *values, int64_t nv,
                 int32_t sym, const char **err);
void *rh_csr_new(int64_t nrow, int64_t ncol, const int32_t *row_pointers, int64_t np, const int32_t *col_indices, const double *values, int64_t nv,
                 int32_t sym, const char **err);
const char *rh_csc_to_dense(void *csc, double *a_row_major, int64_t len);
const char *rh_csr_to_dense(void *csr, double *a_row_major, int64_t len);
/* csc_matrix.rs:508-584 / csr_matrix.rs:483-558 */
void *rh_csc_from_csr(void *csr, const char **err);
void *rh_csr_from_csc(void *csc, const char **err);

void *rh_csc_from_coo(void *coo, const char **err);
const char *rh_csc_update_from_coo(void *csc, void *coo);
void rh_csc_arrays(void *csc, const int32_t **col_pointers, const int32_t **row_indices, const double **values, int64_t *ncol, int64_t *nnz);
const char *rh_csc_mat_vec_mul(void *csc, double *v, int64_t nv, double alpha, const double *u, int64_t nu);
void rh_csc_free(void *csc);

void *rh_csr_from_coo(void *coo, const char **err);
const char *rh_csr_update_from_coo(void *csr, void *coo);
void rh_csr_arrays(void *csr, const int32_t **row_pointers, const int32_t **col_indices, const double **values, int64_t *nrow, int64_t *nnz);
const char *rh_csr_mat_vec_mul(void *csr, double *v, int64_t nv, double alpha, const double *u, int64_t nu);
void rh_csr_free(void *csr);

const char *rh_verify(void *coo, const double *x, int64_t nx, const double *rhs, int64_t nr, double *out4);
void *rh_read_matrix_market(const char *path, int32_t mmsym, const char **err);

/* complex twin (ComplexCooMatrix, ComplexLinSolTrait): complex numbers are (re, im) pairs of doubles, vectors interleaved;
 * solved through the real-equivalent system on the same device path (complex_lin_solver.rs:12-104) */
const char *rh_coo_put_many(void *coo, int64_t n, const int32_t *i, const int32_t *j, const double *aij);
const char *rh_ccoo_put_many(void *ccoo, int64_t n, const int32_t *i, const int32_t *j, const double *re_im);
void *rh_ccoo_new(int64_t nrow, int64_t ncol, int64_t max_nnz, int32_t sym, const char **err);
void rh_ccoo_free(void *ccoo);
const char *rh_ccoo_put(void *ccoo, int64_t i, int64_t j, double re, double im);
void rh_ccoo_reset(void *ccoo);
const char *rh_ccoo_mat_vec_mul(void *ccoo, double *v, int64_t nv, double alpha_re, double alpha_im, const double *u, int64_t nu);
void *rh_clinsolver_new(const char **err);
void rh_clinsolver_free(void *solver);
const char *rh_clinsolver_factorize(void *solver, void *ccoo, const struct RhParams *params_or_null);
const char *rh_clinsolver_solve(void *solver, double *x, int64_t nx, const double *rhs, int64_t nr, int32_t verbose);
/* A^T x = rhs (conjugate = 0) or A^H x = rhs (conjugate = 1) with the factor of A */
const char *rh_clinsolver_solve_transpose(void *solver, double *x, int64_t nx, const double *rhs, int64_t nr, int32_t conjugate, int32_t verbose);
/* extension of the HIPMF backend (complex_solver_hipmf_solve_updated of russell_hipmf.h): A_new x = rhs with the factor of the last factorize
 * as preconditioner of a flexible GMRES in complex arithmetic; ccoo: the factorised matrix's structure with new values; x, rhs interleaved;
 * "Error(2): ..." when the tolerance was not reached (x: best iterate) */
const char *rh_clinsolver_solve_updated(void *solver, double *x, int64_t nx, void *ccoo, const double *rhs, int64_t nr, double rel_tol, int32_t max_steps,
                                        int32_t *steps, double *relres, int32_t verbose);
/* extensions of the HIPMF backend for nrhs right-hand sides (complex_solver_hipmf_solve_many / complex_solver_hipmf_solve_updated_many of
 * russell_hipmf.h): x, rhs column-major n x nrhs complex arrays, interleaved (2 n nrhs doubles), 16 columns per pass pair; steps / relres
 * nrhs entries; "Error(2): ..." when any column did not reach the tolerance (x, steps and relres are written then too) */
const char *rh_clinsolver_solve_many(void *solver, double *x, const double *rhs, int64_t n, int64_t nrhs);
const char *rh_clinsolver_solve_updated_many(void *solver, double *x, void *ccoo, const double *rhs, int64_t n, int64_t nrhs, double rel_tol, int32_t max_steps,
                                             int32_t *steps, double *relres, int32_t verbose);
/* the transposed forms (complex_solver_hipmf_solve_updated_transpose / _many, complex_solver_hipmf_solve_transpose_many of russell_hipmf.h):
 * conjugate = 1 -> A^H, 0 -> A^T; everything else as the functions above */
const char *rh_clinsolver_solve_updated_transpose(void *solver, double *x, int64_t nx, void *ccoo, const double *rhs, int64_t nr, double rel_tol, int32_t max_steps,
                                                  int32_t *steps, double *relres, int32_t conjugate, int32_t verbose);
const char *rh_clinsolver_solve_updated_transpose_many(void *solver, double *x, void *ccoo, const double *rhs, int64_t n, int64_t nrhs, double rel_tol,
                                                       int32_t max_steps, int32_t *steps, double *relres, int32_t conjugate, int32_t verbose);
const char *rh_clinsolver_solve_transpose_many(void *solver, double *x, const double *rhs, int64_t n, int64_t nrhs, int32_t conjugate);
/* determinant = (det_re + i det_im) x 10^det_exp (LinSolParams.compute_determinant; complex_solver_umfpack.rs:411-414) */
void rh_clinsolver_outputs(void *solver, double *det_re, double *det_im, double *det_exp, double *rcond, int32_t *npert);
/* the eight values of mumps_stats (RINFOG(4..11)) of the last solve when LinSolParams.compute_error_estimates (entries 0 - 4) or
 * compute_condition_numbers (all eight) was set at factorize; zeros otherwise (complex_solver_mumps.rs:429-436) */
void rh_clinsolver_mumps_stats(void *solver, double *out);

void *rh_linsolver_new(int32_t genie, const char **err);
void rh_linsolver_free(void *solver);
const char *rh_linsolver_factorize(void *solver, void *coo, const struct RhParams *params_or_null);
const char *rh_linsolver_solve(void *solver, double *x, int64_t nx, const double *rhs, int64_t nr, int32_t verbose);
const char *rh_linsolver_solve_many(void *solver, double *x, const double *rhs, int64_t n, int64_t nrhs);
/* extensions of the HIPMF backend (solver_hipmf_solve_sparse / solver_hipmf_inverse_entries of russell_hipmf.h): right-hand sides in
 * compressed-column form (ptr: ncol + 1 entries), sel == NULL: all rows; x_sel column-major with nx = (nsel or ndim) * ncol entries */
const char *rh_linsolver_solve_sparse(void *solver, double *x_sel, int64_t nx, int64_t ncol, const int32_t *ptr, const int32_t *idx, const double *val,
                                      int64_t nsel, const int32_t *sel, int32_t verbose);
const char *rh_linsolver_inverse_entries(void *solver, double *values, int64_t nent, const int32_t *rows, const int32_t *cols, int32_t verbose);
/* the same through A^T (solver_hipmf_solve_sparse_transpose / solver_hipmf_inverse_entries_by_rows): rows of A^{-T} B; the entries of
 * A^{-1} with 16 distinct rows per block */
const char *rh_linsolver_solve_sparse_transpose(void *solver, double *x_sel, int64_t nx, int64_t ncol, const int32_t *ptr, const int32_t *idx, const double *val,
                                                int64_t nsel, const int32_t *sel, int32_t verbose);
const char *rh_linsolver_inverse_entries_by_rows(void *solver, double *values, int64_t nent, const int32_t *rows, const int32_t *cols, int32_t verbose);
/* extension of the HIPMF backend (solver_hipmf_solve_updated of russell_hipmf.h): A_new x = rhs with the factor of the last factorize as
 * preconditioner; coo: the factorised matrix's structure with new values; "Error(2): ..." when the tolerance was not reached (x: best iterate) */
const char *rh_linsolver_solve_updated(void *solver, double *x, int64_t nx, void *coo, const double *rhs, int64_t nr, double rel_tol, int32_t max_steps,
                                       int32_t *steps, double *relres, int32_t verbose);
/* the same for nrhs right-hand sides (solver_hipmf_solve_updated_many): x, rhs column-major n x nrhs, steps / relres nrhs entries;
 * "Error(2): ..." when any column did not reach the tolerance (x, steps and relres are written then too) */
const char *rh_linsolver_solve_updated_many(void *solver, double *x, void *coo, const double *rhs, int64_t n, int64_t nrhs, double rel_tol, int32_t max_steps,
                                            int32_t *steps, double *relres, int32_t verbose);
/* the transposed forms, A_new^T x = rhs (solver_hipmf_solve_updated_transpose / _many): the arguments of the two functions above */
const char *rh_linsolver_solve_updated_transpose(void *solver, double *x, int64_t nx, void *coo, const double *rhs, int64_t nr, double rel_tol, int32_t max_steps,
                                                 int32_t *steps, double *relres, int32_t verbose);
const char *rh_linsolver_solve_updated_transpose_many(void *solver, double *x, void *coo, const double *rhs, int64_t n, int64_t nrhs, double rel_tol,
                                                      int32_t max_steps, int32_t *steps, double *relres, int32_t verbose);
void rh_linsolver_times(void *solver, uint64_t *ns3);
void rh_linsolver_outputs(void *solver, double *det_coef, double *det_exp, double *rcond, int32_t *eff_ordering, int32_t *eff_scaling, int32_t *npert);
const char *rh_linsolver_stats_json(void *solver, void *coo, const char *name, const double *x, const double *rhs);

const char *rh_error_string(int32_t code);
/* russell_lab formatters.rs:60-95 ("2.5ms", "1h2m3s"); writes at most len-1 bytes + NUL into buf */
void rh_format_nanoseconds(uint64_t nanoseconds, char *buf, int32_t len);
/* stats_lin_sol.rs:334-340 */
int32_t rh_is_memory_error(const char *message);
/* read_matrix_market.rs:346-475 for real AND complex files: exactly one of *coo / *ccoo is set (the other is NULL);
 * the handles are those of rh_coo_* / rh_ccoo_* */
void rh_ccoo_info(void *ccoo, int64_t *nrow, int64_t *ncol, int64_t *nnz, int64_t *max_nnz, int32_t *sym);
void rh_ccoo_arrays(void *ccoo, const int32_t **ai, const int32_t **aj, const double **ax_interleaved);
const char *rh_read_matrix_market_any(const char *path, int32_t mmsym, void **coo, void **ccoo);
const char *rh_enum_name(int32_t which, int32_t value);
int32_t rh_genie_get_sym(int32_t genie, int32_t symmetric);

#ifdef __cplusplus
}
#endif
#endif
