// kernels_krylov_blocked.hpp -- the Arnoldi processes of solver_hipmf_solve_updated_many (Solver::solve_updated_many, numeric.cpp): up to
// KRYB_COLS = 16 INDEPENDENT flexible GMRES iterations, one per right-hand side, that advance in lockstep so that they share the blocked
// pass pair, one pass over the matrix and every launch of a step.  No Krylov space is shared: no kernel here forms a sum across columns,
// so a non-finite number in one column cannot reach another.
//
// Basis layout: V[(k C + c) n + i] (Z alike), C = columns of the block: the C vectors of step k are contiguous, column-major with leading
// dimension n -- the shape the blocked pass pair takes -- and the basis vectors of ONE column lie vstr = C n apart.
//
// The vector kernels are the kernels of kernels_krylov.hpp (same tile, same two pairs per thread, same KRY_PASSV vectors per pass, same
// order of every sum: per column the bits of the single form) with blockIdx.y = column, the stride between a column's basis vectors, a bit
// mask of the columns that take part (workgroup-uniform: a workgroup of a masked column returns at once) and partial-sum slots per column
// (column c at partial + c pcol).  The two matrix kernels keep their row block and walk the columns, as k_residual_cols does: the values
// and indices come from HBM once per row block, not once per column.
#pragma once
#include "kernels_krylov.hpp"

namespace hipmf {

constexpr int KRYB_COLS = 16; // columns of a block (the widest instance of the blocked pass pair)

// partial[c pcol + j gridDim.x + blockIdx.x] = sum over the workgroup's tile of W_c(i) V_c(i, j), j < nv.  W: column c at W + c n.
__global__ void __launch_bounds__(256) k_kryb_dots(int64_t n, const double *__restrict__ W, const double *__restrict__ V, int64_t vstr, int32_t nv, uint32_t mask,
                                                   double *__restrict__ partial, int64_t pcol) {
    __shared__ double red[KRY_PASSV][4];
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    const double *w = W + (int64_t)c * n;
    const double *Vc = V + (int64_t)c * n;
    double *pc = partial + (int64_t)c * pcol;
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double w0, w1, w2, w3;
    kry_ld2(w, i0, n, w0, w1);
    kry_ld2(w, i1, n, w2, w3);
    for (int j0 = 0; j0 < nv; j0 += KRY_PASSV) {
        double a[KRY_PASSV][4], acc[KRY_PASSV];
#pragma unroll
        for (int q = 0; q < KRY_PASSV; q++) { // (clamped vector: unconditional loads, the surplus sums are not stored)
            const double *v = Vc + (int64_t)(j0 + q < nv ? j0 + q : nv - 1) * vstr;
            kry_ld2(v, i0, n, a[q][0], a[q][1]);
            kry_ld2(v, i1, n, a[q][2], a[q][3]);
        }
#pragma unroll
        for (int q = 0; q < KRY_PASSV; q++) acc[q] = wave_sum_f64(fma(w3, a[q][3], fma(w2, a[q][2], fma(w1, a[q][1], w0 * a[q][0]))));
        __syncthreads(); // (the sums of the pass before have been read)
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < KRY_PASSV; q++) red[q][threadIdx.x >> 6] = acc[q];
        }
        __syncthreads();
        const int q = threadIdx.x;
        if (q < KRY_PASSV && j0 + q < nv) pc[(int64_t)(j0 + q) * gridDim.x + blockIdx.x] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    }
}

// out[c ostr + j] = sum over b < nblk of partial[c pcol + j nblk + b]; grid (sums per column, columns); the order of k_kry_reduce
__global__ void __launch_bounds__(256) k_kryb_reduce(const double *__restrict__ partial, int64_t pcol, int32_t nblk, uint32_t mask, double *__restrict__ out,
                                                     int64_t ostr) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    const double *p = partial + (int64_t)c * pcol + (int64_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += p[b];
    s = kry_block_sum(s, red);
    if (threadIdx.x == 0) out[(int64_t)c * ostr + blockIdx.x] = s;
}

// column c: w -= sum_j coef_j V_c(:, j) (SUB) or x += sum_j coef_j Z_c(:, j), j < nv ascending; NORM: partial sums of |w|^2 of the result
template <bool SUB, bool NORM>
__device__ __forceinline__ void kryb_axpy_many(int64_t n, double *__restrict__ w, const double *__restrict__ Vc, int64_t vstr, int32_t nv, const double *__restrict__ coef,
                                               double *__restrict__ partial) {
    __shared__ double red[4];
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double w0, w1, w2, w3;
    kry_ld2(w, i0, n, w0, w1);
    kry_ld2(w, i1, n, w2, w3);
    for (int j0 = 0; j0 < nv; j0 += KRY_PASSV) {
        double a[KRY_PASSV][4], cj[KRY_PASSV];
#pragma unroll
        for (int q = 0; q < KRY_PASSV; q++)
            if (j0 + q < nv) { // (workgroup-uniform)
                const double *v = Vc + (int64_t)(j0 + q) * vstr;
                cj[q] = SUB ? -coef[j0 + q] : coef[j0 + q];
                kry_ld2(v, i0, n, a[q][0], a[q][1]);
                kry_ld2(v, i1, n, a[q][2], a[q][3]);
            }
#pragma unroll
        for (int q = 0; q < KRY_PASSV; q++)
            if (j0 + q < nv) w0 = fma(cj[q], a[q][0], w0), w1 = fma(cj[q], a[q][1], w1), w2 = fma(cj[q], a[q][2], w2), w3 = fma(cj[q], a[q][3], w3);
    }
    kry_st2(w, i0, n, w0, w1);
    kry_st2(w, i1, n, w2, w3);
    if (NORM) { // (elements beyond n were loaded as zeros and stay zero)
        const double s = kry_block_sum(fma(w3, w3, fma(w2, w2, fma(w1, w1, w0 * w0))), red);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}
// one round of classical Gram-Schmidt for the active columns: W_c -= sum_j h_{c,j} V_c(:, j) (h: column c at h + c hstr), fused with the
// partial sums of |W_c|^2 (partial[c pcol + blockIdx.x])
__global__ void __launch_bounds__(256) k_kryb_update(int64_t n, double *__restrict__ W, const double *__restrict__ V, int64_t vstr, int32_t nv, uint32_t mask,
                                                     const double *__restrict__ h, int64_t hstr, double *__restrict__ partial, int64_t pcol) {
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    kryb_axpy_many<true, true>(n, W + (int64_t)c * n, V + (int64_t)c * n, vstr, nv, h + (int64_t)c * hstr, partial + (int64_t)c * pcol);
}
// X_c += sum_{j < cnt[c]} y_{c,j} Z_c(:, j) (X: column c at X + c xstr; y: column c at y + c ystr; a column's own count of directions)
__global__ void __launch_bounds__(256) k_kryb_combine(int64_t n, double *__restrict__ X, int64_t xstr, const double *__restrict__ Z, int64_t vstr, uint32_t mask,
                                                      const int32_t *__restrict__ cnt, const double *__restrict__ y, int64_t ystr) {
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    kryb_axpy_many<false, false>(n, X + (int64_t)c * xstr, Z + (int64_t)c * n, vstr, cnt[c], y + (int64_t)c * ystr, nullptr);
}

// columns of `scale`: V_c = S_c / sqrt(nrm2[c nstr]) (S: column c at S + c sstr; V: at V + c ostr); columns of `zero`: V_c = 0 (a parked
// column: the blocked pass pair reads all C columns and must never meet stale or non-finite data); every other column is left alone
__global__ void __launch_bounds__(256) k_kryb_scale(int64_t n, const double *__restrict__ S, int64_t sstr, const double *__restrict__ nrm2, int64_t nstr,
                                                    double *__restrict__ V, int64_t ostr, uint32_t scale, uint32_t zero) {
    const int c = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double *v = V + (int64_t)c * ostr;
    if ((scale >> c) & 1u) {
        const double *w = S + (int64_t)c * sstr;
        const double s = 1.0 / sqrt(nrm2[(int64_t)c * nstr]);
        double w0, w1, w2, w3;
        kry_ld2(w, i0, n, w0, w1);
        kry_ld2(w, i1, n, w2, w3);
        kry_st2(v, i0, n, w0 * s, w1 * s);
        kry_st2(v, i1, n, w2 * s, w3 * s);
    } else if ((zero >> c) & 1u) {
        kry_st2(v, i0, n, 0.0, 0.0);
        kry_st2(v, i1, n, 0.0, 0.0);
    }
}

// W_c = A X_c for the active columns on the row blocks of the stream SpMV (X, W: column c at + c n).  The workgroup keeps its row block:
// after the first column its values and indices come from the cache.  Mirrored entries of symmetric-lower storage: inside spmv_block.
__global__ void __launch_bounds__(256) k_kryb_spmv(const int32_t *__restrict__ row_blk, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                   const double *__restrict__ vals, const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                   const int32_t *__restrict__ arow, int64_t n, const double *__restrict__ X, double *__restrict__ W, int32_t ncols,
                                                   uint32_t mask) {
    __shared__ SpmvLds sh;
    for (int c = 0; c < ncols; c++) {
        if (!((mask >> c) & 1u)) continue;
        spmv_block<false>(sh, row_blk, rp, ci, vals, tptr, tidx, arow, 1.0, X + (int64_t)c * n, nullptr, W + (int64_t)c * n, nullptr);
        __syncthreads(); // (the LDS of the block is reused by the next column)
    }
}

// R_c = B_c - A X_c for the active columns, fused with the partial sums of |r_c|^2 (partial[c pcol + blockIdx.x]) and |b_c|^2
// (partial[c pcol + gridDim.x + blockIdx.x]); X, B: column c at + c xstr / + c bstr (the caller's leading dimension), R at + c n
__global__ void __launch_bounds__(256) k_kryb_residual(const int32_t *__restrict__ row_blk, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       const double *__restrict__ vals, const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                       const int32_t *__restrict__ arow, int64_t n, const double *__restrict__ X, int64_t xstr,
                                                       const double *__restrict__ B, int64_t bstr, double *R, int32_t ncols, uint32_t mask,
                                                       double *__restrict__ partial, int64_t pcol) {
    __shared__ SpmvLds sh;
    const int r0 = row_blk[blockIdx.x], r1 = row_blk[blockIdx.x + 1];
    for (int c = 0; c < ncols; c++) {
        if (!((mask >> c) & 1u)) continue;
        double *r = R + (int64_t)c * n;
        const double *b = B + (int64_t)c * bstr;
        spmv_block<false>(sh, row_blk, rp, ci, vals, tptr, tidx, arow, 1.0, X + (int64_t)c * xstr, nullptr, r, nullptr);
        __syncthreads(); // (the rows of this block were written by other threads of this workgroup)
        double rr = 0.0, bb = 0.0;
        for (int i = r0 + threadIdx.x; i < r1; i += 256) {
            const double bi = b[i], ri = bi - r[i];
            r[i] = ri;
            rr = fma(ri, ri, rr), bb = fma(bi, bi, bb);
        }
        rr = kry_block_sum(rr, sh.red);
        bb = kry_block_sum(bb, sh.red);
        if (threadIdx.x == 0) partial[(int64_t)c * pcol + blockIdx.x] = rr, partial[(int64_t)c * pcol + gridDim.x + blockIdx.x] = bb;
        __syncthreads(); // (sh.red is the staging of the next column's long-row sum)
    }
}

} // namespace hipmf
