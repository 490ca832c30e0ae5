// kernels_sensitivity.hpp -- sensitivities of the solve with respect to the matrix VALUES (solver_hipmf_values_outer / _solve_tangent /
// _solve_adjoint and the complex twin's three calls; Solver::values_outer, solve_tangent, solve_adjoint in numeric.cpp).
//
// With lambda = A^{-T} g the gradient of J with respect to the stored entry (i, j) is -lambda_i x_j, summed over the right-hand sides:
// an outer product RESTRICTED TO THE SPARSITY PATTERN.  The kernels here form it and carry it to the order of the caller's values.
//
// k_sens_outer     One lane per STORED entry k = (i_k, j_k), consecutive lanes on consecutive entries: the column indices are read and
//                  the results written as whole cache lines, the row comes from the per-entry row array (d_arow; 4 more bytes per
//                  entry, read the same way), u is uniform over the lanes of a row and w is gathered.  A row of 10^5 entries is 10^5
//                  lanes like any others: long rows and long columns (arrow matrices, constraint rows) need no path of their own.
//                      grad[k] = beta grad[k] + alpha sum_{c < ncols} u[i_k + c ldu] w[j_k + c ldw]
//                  The sum over the columns is ONE chain of fma in ascending c per entry, carried in a register of the lane that owns
//                  the entry; no sum is formed across lanes, workgroups or launches, so the result depends neither on the launch
//                  geometry nor on the device, and there are no floating-point atomics.  beta == 0: grad is not read.
//                  SYM (symmetric-lower storage): an off-diagonal stored entry stands for (i, j) and (j, i) and gets
//                  sum_c (u_i w_j + u_j w_i), the two products of a column added first (one fma), then added to the chain.
// k_sens_scatter   To the caller's value order when that is not the CSR order of the handle: input t receives the sum of the slot
//                  gradients of every CSR slot that reads it -- the two mirrored slots of a symmetric matrix expanded to general storage
//                  (set_expansion), the slots whose segment of the value map (set_value_map) lists t -- through the INVERSE map
//                  (input -> slots, built once on the host), summed in ascending slot order.  (Maps that subtract inputs, ~t, belong
//                  to the complex twin's real-equivalent system, which has k_zsens_scatter: values_outer refuses them.)
//                      out[t] = beta out[t] + sum_q slot[inv_idx[q]],  inv_ptr[t] <= q < inv_ptr[t + 1]
// k_zsens_outer    The complex outer product on interleaved (re, im) columns of order n, one lane per stored COMPLEX entry:
//                      grad[k] = beta grad[k] + alpha sum_c u[i_k, c] op(w[j_k, c]),  op = conj with CONJ, alpha and beta real;
//                  real and imaginary part are two chains of two fma per column, in ascending c.  SYM as above (complex-symmetric lower
//                  storage).  k_zsens_scatter: the same scatter on complex slots (the triplets of the complex value map).
// Algorithmic bytes of k_sens_outer per stored entry: 4 (column index) + 8 (result), + 8 when beta != 0, plus the gathers of w (8 per
// column, mostly from the cache: neighbouring entries read neighbouring w) and the row-uniform reads of u; the row array adds 4.
#pragma once
#include "kernels_common.hpp"

namespace hipmf {

constexpr int SENS_MAX_WG = 2048; // workgroups of a launch at most: 256 CUs x 8, the entries beyond are reached by the grid stride

template <bool SYM>
__global__ void __launch_bounds__(256) k_sens_outer(int64_t nnz, const int32_t *__restrict__ arow, const int32_t *__restrict__ ci, const double *__restrict__ u,
                                                    int64_t ldu, const double *__restrict__ w, int64_t ldw, int32_t ncols, double alpha, double beta,
                                                    double *__restrict__ grad) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) {
        const int32_t i = arow[k], j = ci[k];
        const double *ui = u + i, *wj = w + j;
        double acc = 0.0;
        if (SYM && i != j) {
            const double *uj = u + j, *wi = w + i;
#pragma unroll 4
            for (int32_t c = 0; c < ncols; c++) acc += fma(ui[(int64_t)c * ldu], wj[(int64_t)c * ldw], uj[(int64_t)c * ldu] * wi[(int64_t)c * ldw]);
        } else {
#pragma unroll 4
            for (int32_t c = 0; c < ncols; c++) acc = fma(ui[(int64_t)c * ldu], wj[(int64_t)c * ldw], acc);
        }
        const double r = alpha * acc;
        grad[k] = beta == 0.0 ? r : fma(beta, grad[k], r);
    }
}

__global__ void __launch_bounds__(256) k_sens_scatter(int64_t nin, const int32_t *__restrict__ inv_ptr, const int32_t *__restrict__ inv_idx,
                                                      const double *__restrict__ slot, double beta, double *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nin; t += (int64_t)gridDim.x * 256) {
        double acc = 0.0;
        for (int32_t q = inv_ptr[t]; q < inv_ptr[t + 1]; q++) acc += slot[inv_idx[q]];
        out[t] = beta == 0.0 ? acc : fma(beta, out[t], acc);
    }
}

// (a, b) += (ur + i ui) (wr + i wi): two fma per part
__device__ __forceinline__ void zsens_mac(double ur, double ui, double wr, double wi, double &a, double &b) {
    a = fma(-ui, wi, fma(ur, wr, a));
    b = fma(ui, wr, fma(ur, wi, b));
}

template <bool SYM, bool CONJ>
__global__ void __launch_bounds__(256) k_zsens_outer(int64_t nnz, const int32_t *__restrict__ zrow, const int32_t *__restrict__ zcol, const double *__restrict__ u,
                                                     int64_t ldu, const double *__restrict__ w, int64_t ldw, int32_t ncols, double alpha, double beta,
                                                     double *__restrict__ grad) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) {
        const int32_t i = zrow[k], j = zcol[k];
        const bool both = SYM && i != j;
        double a = 0.0, b = 0.0;
#pragma unroll 2
        for (int32_t c = 0; c < ncols; c++) {
            const double *uc = u + 2 * (int64_t)c * ldu, *wc = w + 2 * (int64_t)c * ldw;
            const double wjr = wc[2 * (int64_t)j], wji = CONJ ? -wc[2 * (int64_t)j + 1] : wc[2 * (int64_t)j + 1];
            if (both) { // the two products of a column first, then the chain
                double pa = 0.0, pb = 0.0;
                const double wir = wc[2 * (int64_t)i], wii = CONJ ? -wc[2 * (int64_t)i + 1] : wc[2 * (int64_t)i + 1];
                zsens_mac(uc[2 * (int64_t)j], uc[2 * (int64_t)j + 1], wir, wii, pa, pb);
                zsens_mac(uc[2 * (int64_t)i], uc[2 * (int64_t)i + 1], wjr, wji, pa, pb);
                a += pa, b += pb;
            } else {
                zsens_mac(uc[2 * (int64_t)i], uc[2 * (int64_t)i + 1], wjr, wji, a, b);
            }
        }
        const double ra = alpha * a, rb = alpha * b;
        grad[2 * k] = beta == 0.0 ? ra : fma(beta, grad[2 * k], ra);
        grad[2 * k + 1] = beta == 0.0 ? rb : fma(beta, grad[2 * k + 1], rb);
    }
}

__global__ void __launch_bounds__(256) k_zsens_scatter(int64_t nin, const int32_t *__restrict__ inv_ptr, const int32_t *__restrict__ inv_idx,
                                                       const double *__restrict__ slot, double beta, double *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nin; t += (int64_t)gridDim.x * 256) {
        double a = 0.0, b = 0.0;
        for (int32_t q = inv_ptr[t]; q < inv_ptr[t + 1]; q++) a += slot[2 * (int64_t)inv_idx[q]], b += slot[2 * (int64_t)inv_idx[q] + 1];
        out[2 * t] = beta == 0.0 ? a : fma(beta, out[2 * t], a);
        out[2 * t + 1] = beta == 0.0 ? b : fma(beta, out[2 * t + 1], b);
    }
}

} // namespace hipmf
