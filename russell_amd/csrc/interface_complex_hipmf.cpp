// interface_complex_hipmf.cpp -- complex (Complex64) twin of the C-ABI: complex_solver_hipmf_{new,drop,initialize,factorize,solve}
// with the shape of the reference's complex shim (/root/reference/russell_sparse/c_code/interface_complex_umfpack.c:82-248;
// values are interleaved (re, im) pairs, COMPLEX64 of constants.h:18; Rust side: complex_solver_umfpack.rs, complex_lin_solver.rs:12-104).
//
// The numeric path is the real one: a complex system A z = c of order n is solved as its REAL-EQUIVALENT system of order 2n with the
// unknowns (Re z_k, Im z_k) interleaved,
//     a + i b at (i, j)   ->   [ a  -b ; b  a ]   at rows 2i, 2i+1 / columns 2j, 2j+1,
// so the interleaved complex vectors ARE the real vectors (no copy), and the caller's complex values are expanded ON THE DEVICE
// (signed value map + k_gather_values): a factorisation moves nnz x 16 bytes over PCIe, nothing is expanded on the host.
// A complex SYMMETRIC matrix handed over as its lower triangle has an unsymmetric real-equivalent form: the mirrored entries are
// written out in the pattern (general LU on the device).
// Round 4: the real path runs in its PAIRED mode (NumericOptions.complex_pairs): the ordering and the matching work on the graph / the
// moduli of the complex matrix and keep rows 2 k, 2 k + 1 together, and every pivot search takes a pair of rows at a time (the row with
// the largest real or imaginary part in the column, then its partner) -- a complex LU with partial pivoting carried out in real
// arithmetic, whose complex pivots give the determinant (the real pivots alone only give |det A|^2).  HIPMF_COMPLEX_PAIRS=0: the plain
// real-equivalent factorisation of rounds 2 - 3 (no determinant).
#include <hipmf_device_rt.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "numeric.hpp"
#include "../../include/russell_hipmf.h"

using namespace hipmf;

struct InterfaceComplexHIPMF {
    Solver solver;       // the real-equivalent system of order 2 n
    int32_t n = 0;
    int64_t nnz = 0;     // stored complex entries of the caller's CSR
    bool sym_lower = false;
    // real-equivalent CSR entry q <- (stored complex entry, code): 0 +re, 1 -im, 2 +im, 3 +re
    std::vector<int32_t> src_entry;
    std::vector<int8_t> src_code;
    int32_t effective_ordering = 0;
    bool triplet_map = false; // the installed map reads the caller's COO triplets (complex_solver_hipmf_set_value_map)
    int8_t pairs_state = 0;   // the pairing the complex error analysis relies on: 0 not checked yet, 1 holds, -1 broken
    // the sensitivity calls (kernels_sensitivity.hpp) work on the caller's complex entries: row and column of every stored entry, the
    // inverse of the triplet map (triplet -> stored entries, ascending; empty without one), and whether the solver holds both as they are
    std::vector<int32_t> zrow, zcol, tri_inv_ptr, tri_inv_idx;
    bool sens_uploaded = false;
};

// No C++ exception crosses the C boundary (the same rule as interface_hipmf.cpp): a failed host allocation comes back as ERROR_MALLOC
// with a message the reference's harness recognises as a memory error (stats_lin_sol.rs:334-340), anything else as ERROR_HIPMF_SYMBOLIC.
template <typename Fn> static int32_t guarded(struct InterfaceComplexHIPMF *h, Fn fn) {
    try {
        return fn();
    } catch (const std::bad_alloc &) {
        if (h) h->solver.last_error = "Not enough memory: a host allocation failed";
        return ERROR_MALLOC;
    } catch (const std::exception &e) {
        if (h) h->solver.last_error = std::string("internal error: ") + e.what();
        return ERROR_HIPMF_SYMBOLIC;
    }
}

namespace {
// builds the real-equivalent CSR pattern (rows 2i, 2i+1) of the complex CSR (mirroring the strict lower triangle when sym_lower) and,
// per real entry, where its value comes from
int32_t build_real_equivalent(InterfaceComplexHIPMF *h, const int32_t *rp, const int32_t *ci, std::vector<int32_t> &rp2, std::vector<int32_t> &ci2) {
    const int32_t n = h->n;
    // full pattern of the complex matrix: per row, (column, stored entry)
    std::vector<int64_t> cnt((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; i++)
        for (int32_t k = rp[i]; k < rp[i + 1]; k++) {
            const int32_t j = ci[k];
            if (j < 0 || j >= n) return ERROR_HIPMF_INVALID_MATRIX;
            if (h->sym_lower && j > i) return ERROR_HIPMF_INVALID_MATRIX; // lower storage promised
            cnt[(size_t)i + 1]++;
            if (h->sym_lower && j != i) cnt[(size_t)j + 1]++;
        }
    for (int32_t i = 0; i < n; i++) cnt[(size_t)i + 1] += cnt[i];
    if (4 * cnt[n] > 0x7fffffffLL) return ERROR_HIPMF_INVALID_MATRIX;
    std::vector<int32_t> fcol((size_t)cnt[n]), fsrc((size_t)cnt[n]);
    {
        std::vector<int64_t> w(cnt.begin(), cnt.end() - 1);
        // rows ascending, stored entries of a row ascending in column: the mirrored entries (j, i), i > j, arrive in ascending i after the
        // row's own entries (columns <= j), so every full row is ascending without a sort
        for (int32_t i = 0; i < n; i++)
            for (int32_t k = rp[i]; k < rp[i + 1]; k++) fcol[(size_t)w[i]] = ci[k], fsrc[(size_t)w[i]++] = k;
        if (h->sym_lower)
            for (int32_t i = 0; i < n; i++)
                for (int32_t k = rp[i]; k < rp[i + 1]; k++)
                    if (ci[k] != i) fcol[(size_t)w[ci[k]]] = i, fsrc[(size_t)w[ci[k]]++] = k;
    }
    rp2.assign((size_t)2 * n + 1, 0);
    ci2.resize((size_t)4 * cnt[n]);
    h->src_entry.resize(ci2.size());
    h->src_code.resize(ci2.size());
    int64_t q = 0;
    for (int32_t i = 0; i < n; i++)
        for (int half = 0; half < 2; half++) {
            rp2[(size_t)2 * i + half] = (int32_t)q;
            for (int64_t e = cnt[i]; e < cnt[(size_t)i + 1]; e++) {
                ci2[(size_t)q] = 2 * fcol[(size_t)e], h->src_entry[(size_t)q] = fsrc[(size_t)e], h->src_code[(size_t)q] = (int8_t)(half == 0 ? 0 : 2), q++;
                ci2[(size_t)q] = 2 * fcol[(size_t)e] + 1, h->src_entry[(size_t)q] = fsrc[(size_t)e], h->src_code[(size_t)q] = (int8_t)(half == 0 ? 1 : 3), q++;
            }
        }
    rp2[(size_t)2 * n] = (int32_t)q;
    return SUCCESSFUL_EXIT;
}

// signed value map of the real solver: real entry q = sum over the caller's inputs behind its complex entry.  tri_ptr / tri_idx
// (optional): complex CSR entry c = sum of the caller's triplets tri_idx[tri_ptr[c] .. tri_ptr[c+1]) (COO with duplicates);
// without them input k IS complex entry k.  Inputs are interleaved (re, im): value 2k / 2k+1.
int32_t install_map(InterfaceComplexHIPMF *h, int64_t nin_complex, const int32_t *tri_ptr, const int32_t *tri_idx) {
    const size_t nq = h->src_entry.size();
    std::vector<int32_t> seg_ptr(nq + 1, 0), seg_idx;
    seg_idx.reserve(tri_ptr ? 4 * (size_t)nin_complex : nq);
    for (size_t q = 0; q < nq; q++) {
        const int32_t c = h->src_entry[q];
        const int code = h->src_code[q];
        const int32_t t0 = tri_ptr ? tri_ptr[c] : c, t1 = tri_ptr ? tri_ptr[c + 1] : c + 1;
        for (int32_t t = t0; t < t1; t++) {
            const int32_t k = tri_ptr ? tri_idx[t] : t;
            const int32_t v = (code == 0 || code == 3) ? 2 * k : 2 * k + 1;
            seg_idx.push_back(code == 1 ? ~v : v);
        }
        if (seg_idx.size() > 0x7fffffffULL) return ERROR_HIPMF_INVALID_VALUE;
        seg_ptr[q + 1] = (int32_t)seg_idx.size();
    }
    return h->solver.set_value_map(2 * nin_complex, seg_ptr.data(), seg_idx.data(), true);
}
} // namespace

extern "C" {

struct InterfaceComplexHIPMF *complex_solver_hipmf_new(void) {
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return nullptr;
        return new (std::nothrow) InterfaceComplexHIPMF();
    } catch (...) {
        return nullptr;
    }
}

void complex_solver_hipmf_drop(struct InterfaceComplexHIPMF *h) {
    if (!h) return;
    try {
        h->solver.release();
    } catch (...) {
    }
    delete h;
}

static int32_t c_initialize_body(struct InterfaceComplexHIPMF *h, int32_t ordering, int32_t scaling, double pivot_epsilon,
                                        int32_t refinement_nstep, C_BOOL verbose, C_BOOL general_symmetric, int32_t ndim,
                                        const int32_t *row_pointers, const int32_t *col_indices, const double *values) {
    if (!h || !row_pointers || !col_indices) return ERROR_NULL_POINTER;
    if (h->solver.initialized) return ERROR_ALREADY_INITIALIZED;
    if (ndim < 1 || ndim > 0x3fffffff) return ERROR_HIPMF_INVALID_MATRIX;
    if (validate_csr(ndim, row_pointers, col_indices) != 0) return ERROR_HIPMF_INVALID_MATRIX;
    h->n = ndim;
    h->nnz = row_pointers[ndim];
    h->sym_lower = general_symmetric == 1;
    std::vector<int32_t> rp2, ci2;
    int32_t code = build_real_equivalent(h, row_pointers, col_indices, rp2, ci2);
    if (code != SUCCESSFUL_EXIT) return code;
    SymbolicOptions so;
    so.ordering = (ordering == HIPMF_ORDERING_NONE) ? ORDERING_NATURAL
                  : (ordering == HIPMF_ORDERING_AMD ? ORDERING_MIN_DEGREE : (ordering == HIPMF_ORDERING_BEST ? ORDERING_BEST : ORDERING_NESTED_DISSECTION));
    NumericOptions no;
    no.scaling = (scaling < 0 || scaling > 2) ? HIPMF_SCALE_SUM : scaling;
    if (pivot_epsilon >= 0.0) no.pivot_epsilon = pivot_epsilon;
    if (refinement_nstep >= 0) no.refinement_nstep = refinement_nstep;
    no.verbose = verbose == 1;
    no.complex_pairs = Tunables::now(&Tunables::complex_pairs);
    h->effective_ordering = (ordering == HIPMF_ORDERING_NONE || ordering == HIPMF_ORDERING_AMD || ordering == HIPMF_ORDERING_BEST) ? ordering : HIPMF_ORDERING_NESTED_DISSECTION; // (BEST: resolved once the analysis has chosen)
    // the values (when given) let the analysis apply the maximum-product matching to a weak diagonal, as for real matrices
    std::vector<double> v2;
    if (values) {
        v2.resize(ci2.size());
        for (size_t q = 0; q < v2.size(); q++) {
            const double re = values[2 * (size_t)h->src_entry[q]], im = values[2 * (size_t)h->src_entry[q] + 1];
            const int c = h->src_code[q];
            v2[q] = (c == 0 || c == 3) ? re : (c == 1 ? -im : im);
        }
    }
    code = h->solver.initialize(2 * ndim, rp2.data(), ci2.data(), false, so, no, values ? v2.data() : nullptr);
    if (code != SUCCESSFUL_EXIT) return code;
    h->zrow.resize((size_t)h->nnz), h->zcol.assign(col_indices, col_indices + h->nnz);
    for (int32_t i = 0; i < ndim; i++)
        for (int32_t k = row_pointers[i]; k < row_pointers[i + 1]; k++) h->zrow[(size_t)k] = i;
    h->tri_inv_ptr.clear(), h->tri_inv_idx.clear(), h->sens_uploaded = false;
    return install_map(h, h->nnz, nullptr, nullptr);
}

int32_t complex_solver_hipmf_initialize(struct InterfaceComplexHIPMF *h, int32_t ordering, int32_t scaling, double pivot_epsilon,
                                        int32_t refinement_nstep, C_BOOL verbose, C_BOOL general_symmetric, int32_t ndim,
                                        const int32_t *row_pointers, const int32_t *col_indices, const double *values) {
    return guarded(h, [&]() { return c_initialize_body(h, ordering, scaling, pivot_epsilon, refinement_nstep, verbose, general_symmetric, ndim, row_pointers, col_indices, values); });
}

static int32_t c_set_value_map_body(struct InterfaceComplexHIPMF *h, int32_t nnz_in, const int32_t *seg_ptr, const int32_t *seg_idx) {
    if (!h || !seg_ptr || !seg_idx) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (nnz_in < 1 || seg_ptr[0] != 0 || seg_ptr[h->nnz] != nnz_in) return ERROR_HIPMF_INVALID_VALUE;
    for (int64_t c = 0; c < h->nnz; c++)
        if (seg_ptr[c + 1] < seg_ptr[c]) return ERROR_HIPMF_INVALID_VALUE;
    for (int32_t t = 0; t < nnz_in; t++)
        if (seg_idx[t] < 0 || seg_idx[t] >= nnz_in) return ERROR_HIPMF_INVALID_VALUE;
    h->triplet_map = true;
    { // triplet t is read by the stored entries tri_inv_idx[tri_inv_ptr[t] .. tri_inv_ptr[t + 1]), ascending
        h->tri_inv_ptr.assign((size_t)nnz_in + 1, 0);
        for (int32_t q = 0; q < nnz_in; q++) h->tri_inv_ptr[(size_t)seg_idx[q] + 1]++;
        for (int32_t t = 0; t < nnz_in; t++) h->tri_inv_ptr[(size_t)t + 1] += h->tri_inv_ptr[(size_t)t];
        h->tri_inv_idx.resize((size_t)nnz_in);
        std::vector<int32_t> at(h->tri_inv_ptr.begin(), h->tri_inv_ptr.end() - 1);
        for (int64_t c = 0; c < h->nnz; c++)
            for (int32_t q = seg_ptr[c]; q < seg_ptr[c + 1]; q++) h->tri_inv_idx[(size_t)at[(size_t)seg_idx[q]]++] = (int32_t)c;
        h->sens_uploaded = false;
    }
    return install_map(h, nnz_in, seg_ptr, seg_idx);
}

int32_t complex_solver_hipmf_set_value_map(struct InterfaceComplexHIPMF *h, int32_t nnz_in, const int32_t *seg_ptr, const int32_t *seg_idx) {
    return guarded(h, [&]() { return c_set_value_map_body(h, nnz_in, seg_ptr, seg_idx); });
}

static int32_t finish(struct InterfaceComplexHIPMF *h, int32_t code, int32_t *effective_ordering, int32_t *effective_scaling, int32_t *num_perturbed,
                      double *rcond) {
    if (effective_ordering) {
        *effective_ordering = h->effective_ordering;
        if (h->effective_ordering == HIPMF_ORDERING_BEST) *effective_ordering = h->solver.S.best_chose_min_degree ? HIPMF_ORDERING_AMD : HIPMF_ORDERING_NESTED_DISSECTION;
    }
    if (effective_scaling) *effective_scaling = h->solver.opt.scaling;
    if (num_perturbed) *num_perturbed = h->solver.n_perturbed;
    if (rcond) {
        *rcond = 0.0;
        if (code == SUCCESSFUL_EXIT) (void)h->solver.rcond_estimate(rcond); // (estimate of the real-equivalent matrix)
    }
    return code;
}

// determinant_coefficient_real / _imag / _exponent: det A = (real + i imag) x 10^exponent, the triple umfpack_zi_get_determinant hands
// to interface_complex_umfpack.c:187-195 (zeros when compute_determinant = 0, as there: :196-200)
static int32_t determinant_out(struct InterfaceComplexHIPMF *h, int32_t code, C_BOOL compute_determinant, double *det_re, double *det_im, double *det_exp) {
    if (det_re) *det_re = 0.0;
    if (det_im) *det_im = 0.0;
    if (det_exp) *det_exp = 0.0;
    if (code != SUCCESSFUL_EXIT || compute_determinant != 1) return code;
    return h->solver.determinant_complex(det_re, det_im, det_exp, nullptr);
}

static int32_t c_factorize_body(struct InterfaceComplexHIPMF *h, int32_t *effective_ordering, int32_t *effective_scaling,
                                       int32_t *num_perturbed_pivots, double *rcond_estimate, double *det_re, double *det_im, double *det_exp,
                                       C_BOOL compute_determinant, C_BOOL verbose, const double *values) {
    if (!h || !values) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (compute_determinant == 1 && !h->solver.opt.complex_pairs) return ERROR_NOT_AVAILABLE; // det of the plain real-equivalent form is |det A|^2: the phase is lost
    if (h->triplet_map) { // a triplet map is installed: plain CSR values need the identity map back
        int32_t c = install_map(h, h->nnz, nullptr, nullptr);
        if (c != SUCCESSFUL_EXIT) return c;
        h->triplet_map = false;
        h->tri_inv_ptr.clear(), h->tri_inv_idx.clear(), h->sens_uploaded = false;
    }
    h->solver.opt.verbose = verbose == 1;
    const int32_t code = finish(h, h->solver.factorize_mapped(values, false), effective_ordering, effective_scaling, num_perturbed_pivots, rcond_estimate);
    return determinant_out(h, code, compute_determinant, det_re, det_im, det_exp);
}

int32_t complex_solver_hipmf_factorize(struct InterfaceComplexHIPMF *h, int32_t *effective_ordering, int32_t *effective_scaling,
                                       int32_t *num_perturbed_pivots, double *rcond_estimate, double *determinant_coefficient_real,
                                       double *determinant_coefficient_imag, double *determinant_exponent, C_BOOL compute_determinant, C_BOOL verbose,
                                       const double *values) {
    return guarded(h, [&]() {
        return c_factorize_body(h, effective_ordering, effective_scaling, num_perturbed_pivots, rcond_estimate, determinant_coefficient_real,
                                determinant_coefficient_imag, determinant_exponent, compute_determinant, verbose, values);
    });
}

static int32_t c_factorize_mapped_body(struct InterfaceComplexHIPMF *h, int32_t *effective_ordering, int32_t *effective_scaling,
                                              int32_t *num_perturbed_pivots, double *rcond_estimate, C_BOOL verbose, const double *input_values) {
    if (!h || !input_values) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    h->solver.opt.verbose = verbose == 1;
    return finish(h, h->solver.factorize_mapped(input_values, false), effective_ordering, effective_scaling, num_perturbed_pivots, rcond_estimate);
}

int32_t complex_solver_hipmf_factorize_mapped(struct InterfaceComplexHIPMF *h, int32_t *effective_ordering, int32_t *effective_scaling,
                                              int32_t *num_perturbed_pivots, double *rcond_estimate, C_BOOL verbose, const double *input_values) {
    return guarded(h, [&]() { return c_factorize_mapped_body(h, effective_ordering, effective_scaling, num_perturbed_pivots, rcond_estimate, verbose, input_values); });
}

// the determinant of the last factorisation (complex_solver_hipmf_factorize_mapped has no determinant arguments: Radau5 never asks)
int32_t complex_solver_hipmf_get_determinant(struct InterfaceComplexHIPMF *h, double *determinant_coefficient_real, double *determinant_coefficient_imag,
                                             double *determinant_exponent) {
    if (!h) return ERROR_NULL_POINTER;
    return guarded(h, [&]() { return h->solver.determinant_complex(determinant_coefficient_real, determinant_coefficient_imag, determinant_exponent, nullptr); });
}

static int32_t c_solve_body(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, C_BOOL verbose) {
    if (!h || !x || !rhs) return ERROR_NULL_POINTER;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    h->solver.opt.verbose = verbose == 1;
    return h->solver.solve(x, rhs, 1, 2 * (int64_t)h->n, false); // interleaved complex vectors = vectors of the real-equivalent system
}

int32_t complex_solver_hipmf_solve(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_body(h, x, rhs, verbose); });
}

// nrhs columns in blocks of 16 per pass pair (Solver::solve on the real-equivalent system: refinement and the Krylov rescue as the handle
// is set up).  x, rhs: column-major ld x nrhs complex arrays, interleaved: columns 2 ld doubles apart.  Status codes and their order:
// those of solver_hipmf_solve_many.
static int32_t c_solve_many_body(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld, C_BOOL verbose, bool on_device) {
    if (!h || !x || !rhs) return ERROR_NULL_POINTER;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    if (nrhs < 1 || ld < h->n) return ERROR_HIPMF_INVALID_VALUE;
    if (!on_device) h->solver.opt.verbose = verbose == 1;
    return h->solver.solve(x, rhs, nrhs, 2 * (int64_t)ld, on_device);
}

int32_t complex_solver_hipmf_solve_many(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld, C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_many_body(h, x, rhs, nrhs, ld, verbose, false); });
}

int32_t complex_solver_hipmf_solve_device(struct InterfaceComplexHIPMF *h, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld) {
    return guarded(h, [&]() { return c_solve_many_body(h, d_x, d_rhs, nrhs, ld, 0, true); });
}

// Solve with new matrix values on the kept factor in complex arithmetic (Solver::solve_updated_complex).  The handle always carries a
// signed value map -- identity after initialize / complex_solver_hipmf_factorize, the caller's triplets after set_value_map -- and this
// call must not swap it (that would change what a later factorize_mapped reads): `mapped` has to name the map in force.
// trans: 0 the system with A_new, 1 A_new^T (conjugated data around the A^H iteration; a complex-symmetric handle: A^T = A, the plain form),
// 2 A_new^H (the transposed real-equivalent system)
static int32_t c_solve_updated_body(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, const double *values, int32_t mapped, double rel_tol,
                                    int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose, bool on_device, const char *who, int32_t trans = 0) {
    if (!h || !x || !rhs || !values) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    if (trans < 0 || trans > 2) return ERROR_HIPMF_INVALID_VALUE;
    // the transposed entry points check rel_tol here, so that their map check comes last whatever the handle (a complex-symmetric one
    // included, which takes the plain core below); the plain entry points keep their order: the map, then rel_tol in the core
    if (trans != 0 && !std::isfinite(rel_tol)) return ERROR_HIPMF_INVALID_VALUE;
    if (trans == 1 && h->sym_lower) trans = 0;
    if ((mapped != 0) != h->triplet_map) {
        h->solver.last_error = mapped != 0 ? std::string(who) + ": mapped = 1 but no triplet map is installed (complex_solver_hipmf_set_value_map)"
                                           : std::string(who) + ": mapped = 0 but the triplet map of complex_solver_hipmf_set_value_map is installed";
        return ERROR_HIPMF_INVALID_VALUE;
    }
    h->solver.opt.verbose = verbose == 1;
    int32_t st = 0;
    double rel = 0.0;
    const int32_t code = h->solver.solve_updated_complex(x, rhs, values, rel_tol, max_steps, &st, &rel, on_device, trans != 0, trans == 1);
    if (steps) *steps = st;
    if (relres) *relres = rel;
    if (verbose == 1 && (code == SUCCESSFUL_EXIT || code == HIPMF_WARNING_NOT_CONVERGED))
        printf("%s: %s after %d step(s) in %lld cycle(s), |b - A x|_2 / |b|_2 = %.3e\n", who, code == SUCCESSFUL_EXIT ? "converged" : "NOT converged", st,
               (long long)h->solver.updated_cycles, rel);
    return code;
}

int32_t complex_solver_hipmf_solve_updated(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, const double *values, int32_t mapped, double rel_tol,
                                           int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_updated_body(h, x, rhs, values, mapped, rel_tol, max_steps, steps, relres, verbose, false, "complex_solver_hipmf_solve_updated"); });
}

int32_t complex_solver_hipmf_solve_updated_device(struct InterfaceComplexHIPMF *h, double *d_x, const double *d_rhs, const double *d_values, int32_t mapped,
                                                  double rel_tol, int32_t max_steps, int32_t *steps, double *relres) {
    return guarded(h, [&]() {
        return c_solve_updated_body(h, d_x, d_rhs, d_values, mapped, rel_tol, max_steps, steps, relres, 0, true, "complex_solver_hipmf_solve_updated_device");
    });
}

// The same for nrhs columns (Solver::solve_updated_many_complex): blocks of 16 columns, every column its own complex flexible GMRES, in
// lockstep.  ld counts complex elements.  The order of the status codes is that of solver_hipmf_solve_updated_many; the map check of the
// single complex form comes last.
static int32_t c_solve_updated_many_body(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld, const double *values,
                                         int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose, bool on_device,
                                         const char *who, int32_t trans = 0) {
    if (!h || !x || !rhs || !values) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    if (trans < 0 || trans > 2) return ERROR_HIPMF_INVALID_VALUE;
    if (trans == 1 && h->sym_lower) trans = 0;
    if (nrhs < 1 || ld < h->n || !std::isfinite(rel_tol)) return ERROR_HIPMF_INVALID_VALUE;
    if ((mapped != 0) != h->triplet_map) {
        h->solver.last_error = mapped != 0 ? std::string(who) + ": mapped = 1 but no triplet map is installed (complex_solver_hipmf_set_value_map)"
                                           : std::string(who) + ": mapped = 0 but the triplet map of complex_solver_hipmf_set_value_map is installed";
        return ERROR_HIPMF_INVALID_VALUE;
    }
    h->solver.opt.verbose = verbose == 1;
    const int32_t code = h->solver.solve_updated_many_complex(x, rhs, nrhs, 2 * (int64_t)ld, values, rel_tol, max_steps, steps, relres, on_device, trans != 0, trans == 1);
    if (verbose == 1 && (code == SUCCESSFUL_EXIT || code == HIPMF_WARNING_NOT_CONVERGED))
        printf("%s: %d column(s) %s: %lld column step(s) in %lld blocked pass pair(s), %lld cycle(s), %lld block(s)\n", who, nrhs,
               code == SUCCESSFUL_EXIT ? "converged" : "NOT all converged", (long long)h->solver.updated_column_steps, (long long)h->solver.updated_steps,
               (long long)h->solver.updated_cycles, (long long)h->solver.updated_blocks);
    return code;
}

int32_t complex_solver_hipmf_solve_updated_many(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld, const double *values,
                                                int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres, C_BOOL verbose) {
    return guarded(h, [&]() {
        return c_solve_updated_many_body(h, x, rhs, nrhs, ld, values, mapped, rel_tol, max_steps, steps, relres, verbose, false, "complex_solver_hipmf_solve_updated_many");
    });
}

int32_t complex_solver_hipmf_solve_updated_many_device(struct InterfaceComplexHIPMF *h, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld,
                                                       const double *d_values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres) {
    return guarded(h, [&]() {
        return c_solve_updated_many_body(h, d_x, d_rhs, nrhs, ld, d_values, mapped, rel_tol, max_steps, steps, relres, 0, true,
                                         "complex_solver_hipmf_solve_updated_many_device");
    });
}

// Extra-precise iterative refinement for the complex handle (Solver::solve_extra_precise in pairs mode: the loop of the real handle on the
// real-equivalent system, the measures on the moduli of the complex components).  Status codes in the order of the real entry point.
static int32_t c_solve_extra_precise_body(struct InterfaceComplexHIPMF *h, double *x, double *x_tail, const double *rhs, double dx_tol, int32_t max_steps,
                                          double *info, C_BOOL verbose) {
    if (!h || !x || !rhs) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    h->solver.opt.verbose = verbose == 1;
    const int32_t code = h->solver.solve_extra_precise(x, x_tail, rhs, 1, 2 * (int64_t)h->n, dx_tol, max_steps, info, false, true);
    if (verbose == 1 && (code == SUCCESSFUL_EXIT || code == HIPMF_WARNING_NOT_CONVERGED))
        printf("complex_solver_hipmf_solve_extra_precise: %s after %lld step(s)\n", code == SUCCESSFUL_EXIT ? "converged" : "NOT converged", (long long)h->solver.extra_steps);
    return code;
}

int32_t complex_solver_hipmf_solve_extra_precise(struct InterfaceComplexHIPMF *h, double *x, double *x_tail, const double *rhs, double dx_tol, int32_t max_steps,
                                                 double *info_len_8, C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_extra_precise_body(h, x, x_tail, rhs, dx_tol, max_steps, info_len_8, verbose); });
}

// A^T z = c (conjugate = 0) or A^H z = c (conjugate = 1): the transpose of the real-equivalent form [a -b; b a] is the real-equivalent form
// of A^H, so the real transposed solve of the 2n system IS the A^H solve; A^T is the same solve with the imaginary parts of c and z negated
// on the way in and out (a device kernel).  Reference: umfpack_zi_solve's UMFPACK_At / UMFPACK_Aat systems (the complex shim calls it with
// UMFPACK_A, interface_complex_umfpack.c:235).
int32_t complex_solver_hipmf_solve_transpose(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t conjugate, C_BOOL verbose) {
    return guarded(h, [&]() {
        if (!h || !x || !rhs) return (int32_t)ERROR_NULL_POINTER;
        if (!h->solver.factorized) return (int32_t)ERROR_NEED_FACTORIZATION;
        if (conjugate != 0 && conjugate != 1) return (int32_t)ERROR_HIPMF_INVALID_VALUE;
        h->solver.opt.verbose = verbose == 1;
        return h->solver.solve_transpose(x, rhs, 1, h->solver.S.n, false, conjugate == 0);
    });
}

// trans of the bodies above from the conjugate argument of the transposed forms: 1 -> A^H (2), 0 -> A^T (1), anything else is refused
static int32_t trans_of(int32_t conjugate) { return conjugate == 1 ? 2 : (conjugate == 0 ? 1 : -1); }

int32_t complex_solver_hipmf_solve_updated_transpose(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, const double *values, int32_t mapped,
                                                     double rel_tol, int32_t max_steps, int32_t *steps, double *relres, int32_t conjugate, C_BOOL verbose) {
    return guarded(h, [&]() {
        return c_solve_updated_body(h, x, rhs, values, mapped, rel_tol, max_steps, steps, relres, verbose, false, "complex_solver_hipmf_solve_updated_transpose",
                                    trans_of(conjugate));
    });
}

int32_t complex_solver_hipmf_solve_updated_transpose_device(struct InterfaceComplexHIPMF *h, double *d_x, const double *d_rhs, const double *d_values,
                                                            int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres, int32_t conjugate) {
    return guarded(h, [&]() {
        return c_solve_updated_body(h, d_x, d_rhs, d_values, mapped, rel_tol, max_steps, steps, relres, 0, true, "complex_solver_hipmf_solve_updated_transpose_device",
                                    trans_of(conjugate));
    });
}

int32_t complex_solver_hipmf_solve_updated_transpose_many(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld,
                                                          const double *values, int32_t mapped, double rel_tol, int32_t max_steps, int32_t *steps,
                                                          double *relres, int32_t conjugate, C_BOOL verbose) {
    return guarded(h, [&]() {
        return c_solve_updated_many_body(h, x, rhs, nrhs, ld, values, mapped, rel_tol, max_steps, steps, relres, verbose, false,
                                         "complex_solver_hipmf_solve_updated_transpose_many", trans_of(conjugate));
    });
}

int32_t complex_solver_hipmf_solve_updated_transpose_many_device(struct InterfaceComplexHIPMF *h, double *d_x, const double *d_rhs, int32_t nrhs,
                                                                 int32_t ld, const double *d_values, int32_t mapped, double rel_tol, int32_t max_steps,
                                                                 int32_t *steps, double *relres, int32_t conjugate) {
    return guarded(h, [&]() {
        return c_solve_updated_many_body(h, d_x, d_rhs, nrhs, ld, d_values, mapped, rel_tol, max_steps, steps, relres, 0, true,
                                         "complex_solver_hipmf_solve_updated_transpose_many_device", trans_of(conjugate));
    });
}

// Many columns of A^T Z = C / A^H Z = C, 16 per transposed pass pair (Solver::solve_transpose_many on the real-equivalent system; conjugate
// = 0: every block's staged columns conjugated on entry and exit); the statistics are those of column 0.
static int32_t c_solve_transpose_many_body(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld, int32_t conjugate, C_BOOL verbose,
                                           bool on_device) {
    if (!h || !x || !rhs) return ERROR_NULL_POINTER;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    if ((conjugate != 0 && conjugate != 1) || nrhs < 1 || ld < h->n) return ERROR_HIPMF_INVALID_VALUE;
    if (!on_device) h->solver.opt.verbose = verbose == 1;
    return h->solver.solve_transpose_many(x, rhs, nrhs, 2 * (int64_t)ld, on_device, conjugate == 0);
}

int32_t complex_solver_hipmf_solve_transpose_many(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, int32_t nrhs, int32_t ld, int32_t conjugate,
                                                  C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_transpose_many_body(h, x, rhs, nrhs, ld, conjugate, verbose, false); });
}

int32_t complex_solver_hipmf_solve_transpose_many_device(struct InterfaceComplexHIPMF *h, double *d_x, const double *d_rhs, int32_t nrhs, int32_t ld,
                                                         int32_t conjugate) {
    return guarded(h, [&]() { return c_solve_transpose_many_body(h, d_x, d_rhs, nrhs, ld, conjugate, 0, true); });
}

// Sparse right-hand sides / selected rows for the complex handle (Solver::solve_sparse on the real-equivalent system): a complex column
// is one real column -- the non-zero (re, im) of row i is rows 2 i, 2 i + 1 (the interleaved values ARE the real values, ascending order is
// kept), a selected row k rows 2 k, 2 k + 1, and the real x_sel with leading dimension 2 ldx is the interleaved complex result.
// trans = 2 (A^H) is the transposed real-equivalent system, trans = 1 (A^T) the same with the imaginary parts negated on the way in and
// out (conj_pairs); a complex-symmetric handle has A^T = A.  The checks come in the order of solver_hipmf_solve_sparse.
static int32_t c_solve_sparse_body(struct InterfaceComplexHIPMF *h, double *x_sel, int32_t ldx, int32_t nrhs, const int32_t *rhs_ptr, const int32_t *rhs_idx,
                                   const double *rhs_val, int32_t nsel, const int32_t *sel_idx, int32_t trans, C_BOOL verbose) {
    if (!h) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    if (!x_sel || !rhs_ptr) return ERROR_NULL_POINTER;
    const int32_t n = h->n;
    if (trans < 0 || trans > 2 || nrhs < 1 || (sel_idx && nsel < 1)) return ERROR_HIPMF_INVALID_VALUE;
    if (ldx < (sel_idx ? nsel : n)) return ERROR_HIPMF_INVALID_VALUE;
    if (rhs_ptr[0] < 0) return ERROR_HIPMF_INVALID_VALUE;
    for (int32_t c = 0; c < nrhs; c++)
        if (rhs_ptr[c + 1] < rhs_ptr[c]) return ERROR_HIPMF_INVALID_VALUE;
    const int64_t e0 = rhs_ptr[0], e1 = rhs_ptr[nrhs];
    if (e1 > e0 && (!rhs_idx || !rhs_val)) return ERROR_NULL_POINTER;
    if (2 * (e1 - e0) > 0x7fffffffLL) return ERROR_HIPMF_INVALID_VALUE;
    std::vector<int32_t> ptr2((size_t)nrhs + 1), idx2((size_t)(2 * (e1 - e0))), sel2;
    for (int32_t c = 0; c <= nrhs; c++) ptr2[(size_t)c] = (int32_t)(2 * (rhs_ptr[c] - e0));
    for (int64_t e = e0; e < e1; e++) {
        const int32_t i = rhs_idx[e];
        if (i < 0 || i >= n) return ERROR_HIPMF_INVALID_VALUE;
        idx2[(size_t)(2 * (e - e0))] = 2 * i, idx2[(size_t)(2 * (e - e0) + 1)] = 2 * i + 1;
    }
    if (sel_idx) {
        sel2.resize(2 * (size_t)nsel);
        for (int32_t k = 0; k < nsel; k++) {
            if (sel_idx[k] < 0 || sel_idx[k] >= n) return ERROR_HIPMF_INVALID_VALUE;
            sel2[2 * (size_t)k] = 2 * sel_idx[k], sel2[2 * (size_t)k + 1] = 2 * sel_idx[k] + 1;
        }
    }
    if (trans == 1 && h->sym_lower) trans = 0;
    h->solver.opt.verbose = verbose == 1;
    const int32_t code = h->solver.solve_sparse(x_sel, 2 * (int64_t)ldx, nrhs, ptr2.data(), idx2.data(), rhs_val ? rhs_val + 2 * e0 : nullptr, 2 * nsel,
                                                sel_idx ? sel2.data() : nullptr, false, false, trans != 0, trans == 1);
    if (verbose == 1 && code == SUCCESSFUL_EXIT)
        printf("complex_solver_hipmf_solve_sparse: Solution completed (%d column(s), trans = %d, %lld pruned block(s))\n", nrhs, trans, (long long)h->solver.pruned_blocks);
    return code;
}

int32_t complex_solver_hipmf_solve_sparse(struct InterfaceComplexHIPMF *h, double *x_sel, int32_t ldx, int32_t nrhs, const int32_t *rhs_ptr, const int32_t *rhs_idx,
                                          const double *rhs_val, int32_t nsel, const int32_t *sel_idx, int32_t trans, C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_sparse_body(h, x_sel, ldx, nrhs, rhs_ptr, rhs_idx, rhs_val, nsel, sel_idx, trans, verbose); });
}

// entries of the complex inverse: Solver::inverse_entries in its pairs form (unit column c = real column 2 c alone)
int32_t complex_solver_hipmf_inverse_entries(struct InterfaceComplexHIPMF *h, int32_t nent, const int32_t *rows, const int32_t *cols, double *values, C_BOOL verbose) {
    return guarded(h, [&]() {
        if (!h) return (int32_t)ERROR_NULL_POINTER;
        h->solver.opt.verbose = verbose == 1;
        return h->solver.inverse_entries(nent, rows, cols, values, false, true);
    });
}

// The complex error analysis (k_zea_rows) reads complex row i from row 2i of the real-equivalent CSR alone: stored entry (i, j) is the
// adjacent pair (column 2j: +Re a_ij, column 2j+1: -Im a_ij).  build_real_equivalent always writes both, even where Im a_ij = 0, and the
// solver keeps the pattern it was given; checked once per handle on the device's copy of the pattern and against the value map.
static int32_t check_pairs(struct InterfaceComplexHIPMF *h) {
    if (h->pairs_state == 0) {
        std::vector<int32_t> rp, ci;
        const int32_t code = h->solver.download_pattern(rp, ci);
        if (code != SUCCESSFUL_EXIT) return code;
        bool ok = rp.size() == (size_t)2 * h->n + 1 && ci.size() == h->src_code.size();
        for (int32_t i = 0; ok && i < h->n; i++)
            for (int32_t q = rp[(size_t)2 * i]; ok && q < rp[(size_t)2 * i + 1]; q += 2)
                ok = q + 1 < rp[(size_t)2 * i + 1] && (ci[(size_t)q] & 1) == 0 && ci[(size_t)q + 1] == ci[(size_t)q] + 1 && h->src_code[(size_t)q] == 0 &&
                     h->src_code[(size_t)q + 1] == 1 && h->src_entry[(size_t)q] == h->src_entry[(size_t)q + 1];
        h->pairs_state = ok ? 1 : -1;
    }
    if (h->pairs_state > 0) return SUCCESSFUL_EXIT;
    h->solver.last_error = "internal error: the real-equivalent rows 2i do not hold complex entries as adjacent (re, -im) pairs";
    return ERROR_HIPMF_SYMBOLIC;
}

// Solve exactly as complex_solver_hipmf_solve does (the same x, bit for bit), then analyse x against A and b with complex moduli
// (Solver::error_analysis_complex): the argument shape of complex_solver_mumps_solve, whose RINFOG(4..11) the reference copies out of
// zmumps_c (interface_complex_mumps.c:243-280, complex_solver_mumps.rs:429-436).  error_analysis_option: 0 none (the array is not
// touched), 1 all eight values, 2 entries 0 - 4.
int32_t complex_solver_hipmf_solve_with_error_analysis(struct InterfaceComplexHIPMF *h, double *x, const double *rhs, double *error_analysis_array_len_8,
                                                       int32_t error_analysis_option, C_BOOL verbose) {
    return guarded(h, [&]() {
        if (!h || !x || !rhs || !error_analysis_array_len_8) return (int32_t)ERROR_NULL_POINTER;
        if (!h->solver.factorized) return (int32_t)ERROR_NEED_FACTORIZATION;
        if (error_analysis_option < 0 || error_analysis_option > 2) return (int32_t)ERROR_HIPMF_INVALID_VALUE;
        int32_t code = error_analysis_option == 0 ? (int32_t)SUCCESSFUL_EXIT : check_pairs(h);
        if (code != SUCCESSFUL_EXIT) return code;
        code = c_solve_body(h, x, rhs, verbose);
        if (code != SUCCESSFUL_EXIT) return code;
        return h->solver.error_analysis_complex(x, rhs, error_analysis_array_len_8, error_analysis_option);
    });
}

// Sensitivities with respect to the complex matrix values (Solver::values_outer_complex, solve_tangent, solve_adjoint;
// kernels_sensitivity.hpp), host pointers.  The outer product runs on the caller's complex entries and their order -- the stored entries
// (a complex-symmetric handle: its lower triangle, an off-diagonal entry standing for both positions) or the triplets of the value map --;
// the two solves run on the real-equivalent system, whose vectors the interleaved columns are: A dx = db - dA x there, and A^H lambda = g
// as its transposed system.  `mapped` has to name the map in force, as for complex_solver_hipmf_solve_updated.
static int32_t c_sens_map_check(struct InterfaceComplexHIPMF *h, int32_t mapped, const char *who) {
    if ((mapped != 0) == h->triplet_map) return SUCCESSFUL_EXIT;
    h->solver.last_error = mapped != 0 ? std::string(who) + ": mapped = 1 but no triplet map is installed (complex_solver_hipmf_set_value_map)"
                                       : std::string(who) + ": mapped = 0 but the triplet map of complex_solver_hipmf_set_value_map is installed";
    return ERROR_HIPMF_INVALID_VALUE;
}

// ... and the pattern and the inverse triplet map of the outer product on the device
static int32_t c_sens_prepare(struct InterfaceComplexHIPMF *h, int32_t mapped, const char *who) {
    if (const int32_t c = c_sens_map_check(h, mapped, who); c != SUCCESSFUL_EXIT) return c;
    if (h->sens_uploaded && h->solver.complex_pattern_set()) return SUCCESSFUL_EXIT; // (a re-matching factorize drops the solver's copy)
    int32_t code = h->solver.set_complex_pattern(h->nnz, h->zrow, h->zcol, h->sym_lower);
    if (code == SUCCESSFUL_EXIT) code = h->solver.set_complex_value_map(h->triplet_map ? (int64_t)h->tri_inv_idx.size() : 0, h->tri_inv_ptr, h->tri_inv_idx);
    h->sens_uploaded = code == SUCCESSFUL_EXIT;
    return code;
}

int32_t complex_solver_hipmf_values_outer(struct InterfaceComplexHIPMF *h, double *grad, const double *u, const double *w, int32_t ncols, int32_t ldu, int32_t ldw,
                                          double alpha, double beta, int32_t mapped, int32_t conjugate_w) {
    return guarded(h, [&]() {
        if (!h || !grad || !u || !w) return (int32_t)ERROR_NULL_POINTER;
        if (!h->solver.initialized) return (int32_t)ERROR_NEED_INITIALIZATION;
        if (ncols < 1 || ldu < h->n || ldw < h->n || (conjugate_w != 0 && conjugate_w != 1)) return (int32_t)ERROR_HIPMF_INVALID_VALUE;
        const int32_t code = c_sens_prepare(h, mapped, "complex_solver_hipmf_values_outer");
        if (code != SUCCESSFUL_EXIT) return code;
        return h->solver.values_outer_complex(grad, u, w, ncols, ldu, ldw, alpha, beta, conjugate_w == 1);
    });
}

int32_t complex_solver_hipmf_solve_tangent(struct InterfaceComplexHIPMF *h, double *dx, const double *x, const double *dvalues, const double *db, int32_t nrhs,
                                           int32_t ld, int32_t mapped) {
    return guarded(h, [&]() {
        if (!h || !dx || !x || !dvalues) return (int32_t)ERROR_NULL_POINTER;
        if (!h->solver.initialized) return (int32_t)ERROR_NEED_INITIALIZATION;
        if (!h->solver.factorized) return (int32_t)ERROR_NEED_FACTORIZATION;
        if (nrhs < 1 || ld < h->n) return (int32_t)ERROR_HIPMF_INVALID_VALUE;
        const int32_t code = c_sens_map_check(h, mapped, "complex_solver_hipmf_solve_tangent"); // (the tangent needs no pattern of its own)
        if (code != SUCCESSFUL_EXIT) return code;
        return h->solver.solve_tangent(dx, x, dvalues, db, nrhs, 2 * (int64_t)ld, true, false); // (the handle always carries a value map)
    });
}

int32_t complex_solver_hipmf_solve_adjoint(struct InterfaceComplexHIPMF *h, double *lambda, double *grad_values, const double *x, const double *g, int32_t nrhs,
                                           int32_t ld, double beta, int32_t mapped) {
    return guarded(h, [&]() {
        if (!h || !lambda || !g || (grad_values && !x)) return (int32_t)ERROR_NULL_POINTER;
        if (!h->solver.initialized) return (int32_t)ERROR_NEED_INITIALIZATION;
        if (!h->solver.factorized) return (int32_t)ERROR_NEED_FACTORIZATION;
        if (nrhs < 1 || ld < h->n) return (int32_t)ERROR_HIPMF_INVALID_VALUE;
        int32_t code = grad_values ? c_sens_prepare(h, mapped, "complex_solver_hipmf_solve_adjoint") : (int32_t)SUCCESSFUL_EXIT;
        if (code != SUCCESSFUL_EXIT) return code;
        code = h->solver.solve_adjoint(lambda, nullptr, nullptr, g, nrhs, 2 * (int64_t)ld, 0.0, false, false); // lambda = A^{-H} g: the transposed real-equivalent system
        if (code != SUCCESSFUL_EXIT || !grad_values) return code;
        return h->solver.values_outer_complex(grad_values, lambda, x, nrhs, ld, ld, -1.0, beta, true); // grad_k = beta grad_k - sum_c lambda_i conj(x_j)
    });
}

// Bordered systems on the kept factor for the complex handle (Solver::set_border, Solver::solve_bordered, Solver::solve_bordered_transpose
// in their pairs mode; kernels_border_complex.hpp): the interleaved complex arrays are handed on as they are, leading dimensions doubled.
// Status codes in the order of the real entry points: ERROR_NULL_POINTER (the handle; B, C, D with k > 0; x, f),
// ERROR_NEED_INITIALIZATION, ERROR_NEED_FACTORIZATION, then ERROR_HIPMF_INVALID_VALUE.  The residual kernels read the moduli |a_ij| from
// the adjacent pairs of the rows 2i: check_pairs, once per handle.
static int32_t c_set_border_body(struct InterfaceComplexHIPMF *h, int32_t k, const double *B, int32_t ldb, const double *C, int32_t ldc, const double *D,
                                 int32_t ldd, double *border_info, C_BOOL verbose, bool on_device) {
    if (!h) return ERROR_NULL_POINTER;
    if (k > 0 && k <= HIPMF_COMPLEX_BORDER_MAX && (!B || !C || !D)) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    if (k > 0 && k <= HIPMF_COMPLEX_BORDER_MAX && (ldb < h->n || ldc < h->n || ldd < k)) return ERROR_HIPMF_INVALID_VALUE;
    if (k > 0 && k <= HIPMF_COMPLEX_BORDER_MAX)
        if (const int32_t code = check_pairs(h); code != SUCCESSFUL_EXIT) return code;
    h->solver.opt.verbose = verbose == 1;
    return h->solver.set_border(k, B, 2 * (int64_t)ldb, C, 2 * (int64_t)ldc, D, 2 * (int64_t)ldd, border_info, on_device, true);
}

int32_t complex_solver_hipmf_set_border(struct InterfaceComplexHIPMF *h, int32_t k, const double *B, int32_t ldb, const double *C, int32_t ldc, const double *D,
                                        int32_t ldd, double *border_info_len_5, C_BOOL verbose) {
    return guarded(h, [&]() { return c_set_border_body(h, k, B, ldb, C, ldc, D, ldd, border_info_len_5, verbose, false); });
}

int32_t complex_solver_hipmf_set_border_device(struct InterfaceComplexHIPMF *h, int32_t k, const double *d_B, int32_t ldb, const double *d_C, int32_t ldc,
                                               const double *d_D, int32_t ldd, double *border_info_len_5, C_BOOL verbose) {
    return guarded(h, [&]() { return c_set_border_body(h, k, d_B, ldb, d_C, ldc, d_D, ldd, border_info_len_5, verbose, true); });
}

// trans: 0 the system itself, 1 M^T (the loop of M^H on conjugated data), 2 M^H (the transposed real-equivalent system)
static int32_t c_solve_bordered_body(struct InterfaceComplexHIPMF *h, double *x, double *z, const double *f, const double *g, int32_t nrhs, int32_t ldx, int32_t ldz,
                                     int32_t max_steps, double *info, C_BOOL verbose, bool on_device, const char *who, int32_t trans) {
    if (!h || !x || !f) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    if (!h->solver.factorized) return ERROR_NEED_FACTORIZATION;
    Solver &s = h->solver;
    if (trans < 0 || !s.bd_pairs) return ERROR_HIPMF_INVALID_VALUE; // (a conjugate other than 0 or 1; no border of this handle's kind in force)
    s.opt.verbose = verbose == 1;
    const int32_t code = trans != 0 ? s.solve_bordered_transpose(x, z, f, g, nrhs, 2 * (int64_t)ldx, 2 * (int64_t)ldz, max_steps, info, on_device, trans == 1)
                                    : s.solve_bordered(x, z, f, g, nrhs, 2 * (int64_t)ldx, 2 * (int64_t)ldz, max_steps, info, on_device);
    if (verbose == 1 && code == SUCCESSFUL_EXIT)
        printf("%s: %d column(s), border of %d: %lld block step(s) in %lld block(s)\n", who, nrhs, s.bd_k / 2, (long long)(trans != 0 ? s.bordered_t_steps : s.bordered_steps),
               (long long)(trans != 0 ? s.bordered_t_blocks : s.bordered_blocks));
    return code;
}

int32_t complex_solver_hipmf_solve_bordered(struct InterfaceComplexHIPMF *h, double *x, double *z, const double *f, const double *g, int32_t nrhs, int32_t ldx,
                                            int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose) {
    return guarded(h, [&]() { return c_solve_bordered_body(h, x, z, f, g, nrhs, ldx, ldz, max_steps, info, verbose, false, "complex_solver_hipmf_solve_bordered", 0); });
}

int32_t complex_solver_hipmf_solve_bordered_device(struct InterfaceComplexHIPMF *h, double *d_x, double *d_z, const double *d_f, const double *d_g, int32_t nrhs,
                                                   int32_t ldx, int32_t ldz, int32_t max_steps, double *info, C_BOOL verbose) {
    return guarded(h, [&]() {
        return c_solve_bordered_body(h, d_x, d_z, d_f, d_g, nrhs, ldx, ldz, max_steps, info, verbose, true, "complex_solver_hipmf_solve_bordered_device", 0);
    });
}

int32_t complex_solver_hipmf_solve_bordered_transpose(struct InterfaceComplexHIPMF *h, double *y, double *w, const double *p, const double *q, int32_t nrhs,
                                                      int32_t ldx, int32_t ldz, int32_t conjugate, int32_t max_steps, double *info, C_BOOL verbose) {
    return guarded(h, [&]() {
        return c_solve_bordered_body(h, y, w, p, q, nrhs, ldx, ldz, max_steps, info, verbose, false, "complex_solver_hipmf_solve_bordered_transpose", trans_of(conjugate));
    });
}

int32_t complex_solver_hipmf_solve_bordered_transpose_device(struct InterfaceComplexHIPMF *h, double *d_y, double *d_w, const double *d_p, const double *d_q,
                                                             int32_t nrhs, int32_t ldx, int32_t ldz, int32_t conjugate, int32_t max_steps, double *info,
                                                             C_BOOL verbose) {
    return guarded(h, [&]() {
        return c_solve_bordered_body(h, d_y, d_w, d_p, d_q, nrhs, ldx, ldz, max_steps, info, verbose, true, "complex_solver_hipmf_solve_bordered_transpose_device",
                                     trans_of(conjugate));
    });
}

const char *complex_solver_hipmf_last_error(struct InterfaceComplexHIPMF *h) { return h ? h->solver.last_error.c_str() : "null solver"; }

static int32_t c_get_stats_body(struct InterfaceComplexHIPMF *h, int64_t *is, double *ds) {
    if (!h || !is || !ds) return ERROR_NULL_POINTER;
    if (!h->solver.initialized) return ERROR_NEED_INITIALIZATION;
    const Solver &s = h->solver;
    for (int i = 0; i < 16; i++) is[i] = 0, ds[i] = 0.0;
    is[0] = h->n, is[1] = h->nnz, is[2] = s.S.nsuper, is[3] = s.S.nlevels, is[4] = s.S.nnz_l, is[5] = s.S.nnz_u, is[6] = s.S.max_front;
    is[7] = s.S.max_pivots, is[8] = s.n_perturbed, is[9] = s.n_zero_pivot, is[10] = s.refinement_steps_done;
    is[11] = s.times.n_kernel_launches_factor, is[12] = s.times.n_kernel_launches_solve, is[13] = s.pool_doubles * 8, is[14] = s.matched ? 1 : 0;
    is[15] = s.fused_fallbacks;
    ds[0] = s.S.flops, ds[1] = s.S.flops_gemm, ds[2] = s.S.seconds_ordering, ds[3] = s.S.seconds_total, ds[4] = s.times.scale_assemble_ms;
    ds[5] = s.times.factor_ms, ds[6] = s.times.fwd_ms, ds[7] = s.times.bwd_ms, ds[8] = s.times.solve_total_ms, ds[9] = s.last_residual_inf;
    return SUCCESSFUL_EXIT;
}

int32_t complex_solver_hipmf_get_stats(struct InterfaceComplexHIPMF *h, int64_t *is, double *ds) {
    return guarded(h, [&]() { return c_get_stats_body(h, is, ds); });
}

int64_t complex_solver_hipmf_get_counter(struct InterfaceComplexHIPMF *h, int32_t which) {
    if (!h || !h->solver.initialized) return -1;
    const Solver &s = h->solver;
    switch (which) {
    case HIPMF_COUNTER_REMATCH: return s.rematch_count;
    case HIPMF_COUNTER_WEAK_DIAGONAL_ROWS: return s.n_weak_diag;
    case HIPMF_COUNTER_FUSED_FALLBACKS: return s.fused_fallbacks;
    case HIPMF_COUNTER_PERSISTENT_BYTES: return s.S.persist_doubles * 8;
    case HIPMF_COUNTER_ARENA_BYTES: return s.S.temp_doubles * 8;
    case HIPMF_COUNTER_SYMMETRIC_LDLT: return s.S.sym_mode ? 1 : 0;
    case HIPMF_COUNTER_CHAIN_FALLBACKS: return s.chain_fallbacks;
    case HIPMF_COUNTER_MID_FRONTS: return s.mid_front_count;
    case HIPMF_COUNTER_TAGGED_SOLVE: return s.tagged_solve() ? 1 : 0;
    case HIPMF_COUNTER_GATE_WAITS: return s.gate_waits;
    case HIPMF_COUNTER_WAVE_FRONTS: return s.wave_front_count;
    case HIPMF_COUNTER_LEAF_FRONTS: return s.leaf_front_count();
    case HIPMF_COUNTER_SPLIT_SLABS: return s.split_slab_count();
    case HIPMF_COUNTER_KRYLOV_ITERATIONS: return s.krylov_iterations;
    case HIPMF_COUNTER_TRANSPOSED_SOLVES: return s.transposed_solves;
    case HIPMF_COUNTER_ANALYSIS_SOLVES: return s.analysis_solves;
    case HIPMF_COUNTER_TRANSPOSED_KRYLOV_ITERATIONS: return s.krylov_iterations_t;
    case HIPMF_COUNTER_TRANSPOSED_BLOCKS: return s.transposed_blocks;
    case HIPMF_COUNTER_PRUNED_FWD_FRONTS: return s.pruned_fwd_fronts;
    case HIPMF_COUNTER_PRUNED_BWD_FRONTS: return s.pruned_bwd_fronts;
    case HIPMF_COUNTER_PRUNED_BLOCKS: return s.pruned_blocks;
    case HIPMF_COUNTER_PRUNED_BYTES: return s.pruned_bytes;
    case HIPMF_COUNTER_PRUNED_TRANSPOSED_BLOCKS: return s.pruned_transposed_blocks;
    case HIPMF_COUNTER_UPDATED_STEPS: return s.updated_steps;
    case HIPMF_COUNTER_UPDATED_CYCLES: return s.updated_cycles;
    case HIPMF_COUNTER_UPDATED_BASIS_BYTES: return s.updated_basis_bytes();
    case HIPMF_COUNTER_UPDATED_PRECOND_US: return (int64_t)(1e3 * s.updated_ms[0]);
    case HIPMF_COUNTER_UPDATED_SPMV_US: return (int64_t)(1e3 * s.updated_ms[1]);
    case HIPMF_COUNTER_UPDATED_ARNOLDI_US: return (int64_t)(1e3 * s.updated_ms[2]);
    case HIPMF_COUNTER_UPDATED_COMPLEX_ARITHMETIC: return s.updated_complex ? 1 : 0;
    case HIPMF_COUNTER_BLOCK_GROUPS: return s.block_groups_last;
    case HIPMF_COUNTER_UPDATED_BLOCKS: return s.updated_blocks;
    case HIPMF_COUNTER_UPDATED_COLUMN_STEPS: return s.updated_column_steps;
    case HIPMF_COUNTER_UPDATED_BLOCK_BASIS_BYTES: return s.updated_block_basis_bytes();
    case HIPMF_COUNTER_EXTRA_PRECISE_STEPS: return s.extra_steps;
    case HIPMF_COUNTER_EXTRA_PRECISE_BLOCKS: return s.extra_blocks;
    case HIPMF_COUNTER_EXTRA_PRECISE_RESIDUAL_US: return (int64_t)(1e3 * s.extra_ms[0]);
    case HIPMF_COUNTER_EXTRA_PRECISE_PRECOND_US: return (int64_t)(1e3 * s.extra_ms[1]);
    case HIPMF_COUNTER_EXTRA_PRECISE_UPDATE_US: return (int64_t)(1e3 * s.extra_ms[2]);
    case HIPMF_COUNTER_SENS_OUTER_COLUMNS: return s.sens_outer_columns;
    case HIPMF_COUNTER_SENS_OUTER_US: return (int64_t)(1e3 * s.sens_outer_ms);
    case HIPMF_COUNTER_COMPLEX_BORDER_COLUMNS: return s.bd_pairs ? s.bd_k / 2 : 0;
    case HIPMF_COUNTER_COMPLEX_BORDERED_STEPS: return s.bordered_steps;
    case HIPMF_COUNTER_COMPLEX_BORDERED_BLOCKS: return s.bordered_blocks;
    case HIPMF_COUNTER_COMPLEX_BORDERED_TRANSPOSED_STEPS: return s.bordered_t_steps;
    case HIPMF_COUNTER_COMPLEX_BORDERED_TRANSPOSED_BLOCKS: return s.bordered_t_blocks;
    case HIPMF_COUNTER_COMPLEX_BORDER_TRANSPOSED_BYTES: return s.bt_bytes;
    default: return -1;
    }
}

} // extern "C"
