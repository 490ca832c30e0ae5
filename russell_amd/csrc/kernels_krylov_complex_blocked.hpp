// kernels_krylov_complex_blocked.hpp -- the Arnoldi processes of complex_solver_hipmf_solve_updated_many (Solver::solve_updated_many_complex,
// numeric.cpp): up to KRYB_COLS = 16 INDEPENDENT flexible GMRES iterations in COMPLEX arithmetic, one per right-hand side, on the vectors of
// the real-equivalent system.  The three kernels of kernels_krylov_complex.hpp with what kernels_krylov_blocked.hpp added to the real ones:
// blockIdx.y = column, the stride vstr = C n between the basis vectors of one column (layout V[(k C + c) n + i], n = 2 nc doubles), a bit
// mask of the columns that take part (workgroup-uniform: a workgroup of a masked column returns at once), partial-sum slots per column
// (column c at partial + c pcol; inside a column slot 2 j holds the real parts of basis vector j, slot 2 j + 1 the imaginary parts, the
// workgroups of a slot contiguous) and, in the combine, a column's own count of directions.  No kernel forms a sum across columns.
//
// Per column the tile, the two pairs per thread (each pair ONE complex element: n, c n, vstr and the tile base are all even), the
// ZKRY_PASSV = 5 basis vectors per pass and the order of every sum are those of the single kernels: a column gets the single form's bits.
// No floating-point atomics.  k_kryb_reduce over 2 nv sums per column leaves a column's nv complex coefficients interleaved; the
// normalisation, the SpMV and the residual are k_kryb_scale, k_kryb_spmv and k_kryb_residual as they are.
//
// As compiled for gfx950 (VGPRs / waves per SIMD / LDS bytes / scratch): see the table in DESIGN.md section 13, "The complex block form".
#pragma once
#include "kernels_krylov_blocked.hpp"
#include "kernels_krylov_complex.hpp"

namespace hipmf {

// partial[c pcol + (2 j + p) gridDim.x + blockIdx.x] = real (p = 0) and imaginary (p = 1) part of the sum over the workgroup's tile of
// conj(V_c(i, j)) W_c(i), j < nv.  W: column c at W + c n.
__global__ void __launch_bounds__(256) k_zkryb_dots(int64_t n, const double *__restrict__ W, const double *__restrict__ V, int64_t vstr, int32_t nv, uint32_t mask,
                                                    double *__restrict__ partial, int64_t pcol) {
    __shared__ double red[2 * ZKRY_PASSV][4];
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    const double *w = W + (int64_t)c * n;
    const double *Vc = V + (int64_t)c * n;
    double *pc = partial + (int64_t)c * pcol;
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double w0, w1, w2, w3;
    zkry_ld(w, i0, n, w0, w1);
    zkry_ld(w, i1, n, w2, w3);
    for (int j0 = 0; j0 < nv; j0 += ZKRY_PASSV) {
        double a[ZKRY_PASSV][4], acc[2 * ZKRY_PASSV];
#pragma unroll
        for (int q = 0; q < ZKRY_PASSV; q++) { // (clamped vector: unconditional loads, the surplus sums are not stored)
            const double *v = Vc + (int64_t)(j0 + q < nv ? j0 + q : nv - 1) * vstr;
            zkry_ld(v, i0, n, a[q][0], a[q][1]);
            zkry_ld(v, i1, n, a[q][2], a[q][3]);
        }
#pragma unroll
        for (int q = 0; q < ZKRY_PASSV; q++) { // conj(a) w = (ar wr + ai wi) + i (ar wi - ai wr)
            acc[2 * q] = wave_sum_f64(fma(a[q][3], w3, fma(a[q][2], w2, fma(a[q][1], w1, a[q][0] * w0))));
            acc[2 * q + 1] = wave_sum_f64(fma(-a[q][3], w2, fma(a[q][2], w3, fma(-a[q][1], w0, a[q][0] * w1))));
        }
        __syncthreads(); // (the sums of the pass before have been read)
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 2 * ZKRY_PASSV; q++) red[q][threadIdx.x >> 6] = acc[q];
        }
        __syncthreads();
        const int q = threadIdx.x;
        if (q < 2 * ZKRY_PASSV && j0 + (q >> 1) < nv) pc[(int64_t)(2 * j0 + q) * gridDim.x + blockIdx.x] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    }
}

// column c: w -= sum_j coef_j V_c(:, j) (SUB) or x += sum_j coef_j Z_c(:, j), j < nv ascending, coef_j complex (interleaved); NORM: partial
// sums of |w|^2 of the result
template <bool SUB, bool NORM>
__device__ __forceinline__ void zkryb_axpy_many(int64_t n, double *__restrict__ w, const double *__restrict__ Vc, int64_t vstr, int32_t nv, const double *__restrict__ coef,
                                                double *__restrict__ partial) {
    __shared__ double red[4];
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double w0, w1, w2, w3;
    zkry_ld(w, i0, n, w0, w1);
    zkry_ld(w, i1, n, w2, w3);
    for (int j0 = 0; j0 < nv; j0 += ZKRY_PASSV) {
        double a[ZKRY_PASSV][4], cr[ZKRY_PASSV], ci[ZKRY_PASSV];
#pragma unroll
        for (int q = 0; q < ZKRY_PASSV; q++)
            if (j0 + q < nv) { // (workgroup-uniform)
                const double *v = Vc + (int64_t)(j0 + q) * vstr;
                cr[q] = SUB ? -coef[2 * (j0 + q)] : coef[2 * (j0 + q)];
                ci[q] = SUB ? -coef[2 * (j0 + q) + 1] : coef[2 * (j0 + q) + 1];
                zkry_ld(v, i0, n, a[q][0], a[q][1]);
                zkry_ld(v, i1, n, a[q][2], a[q][3]);
            }
#pragma unroll
        for (int q = 0; q < ZKRY_PASSV; q++)
            if (j0 + q < nv) { // c a = (cr ar - ci ai) + i (cr ai + ci ar)
                w0 = fma(-ci[q], a[q][1], fma(cr[q], a[q][0], w0)), w1 = fma(ci[q], a[q][0], fma(cr[q], a[q][1], w1));
                w2 = fma(-ci[q], a[q][3], fma(cr[q], a[q][2], w2)), w3 = fma(ci[q], a[q][2], fma(cr[q], a[q][3], w3));
            }
    }
    zkry_st(w, i0, n, w0, w1);
    zkry_st(w, i1, n, w2, w3);
    if (NORM) { // (elements beyond n were loaded as zeros and stay zero)
        const double s = kry_block_sum(fma(w3, w3, fma(w2, w2, fma(w1, w1, w0 * w0))), red);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}
// one round of classical Gram-Schmidt for the active columns: W_c -= sum_j h_{c,j} V_c(:, j), complex h (column c at h + c hstr doubles),
// fused with the partial sums of |W_c|^2 (partial[c pcol + blockIdx.x])
__global__ void __launch_bounds__(256) k_zkryb_update(int64_t n, double *__restrict__ W, const double *__restrict__ V, int64_t vstr, int32_t nv, uint32_t mask,
                                                      const double *__restrict__ h, int64_t hstr, double *__restrict__ partial, int64_t pcol) {
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    zkryb_axpy_many<true, true>(n, W + (int64_t)c * n, V + (int64_t)c * n, vstr, nv, h + (int64_t)c * hstr, partial + (int64_t)c * pcol);
}
// X_c += sum_{j < cnt[c]} y_{c,j} Z_c(:, j), complex y (X: column c at X + c xstr; y: column c at y + c ystr doubles; a column's own count of
// directions)
__global__ void __launch_bounds__(256) k_zkryb_combine(int64_t n, double *__restrict__ X, int64_t xstr, const double *__restrict__ Z, int64_t vstr, uint32_t mask,
                                                       const int32_t *__restrict__ cnt, const double *__restrict__ y, int64_t ystr) {
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    zkryb_axpy_many<false, false>(n, X + (int64_t)c * xstr, Z + (int64_t)c * n, vstr, cnt[c], y + (int64_t)c * ystr, nullptr);
}

} // namespace hipmf
