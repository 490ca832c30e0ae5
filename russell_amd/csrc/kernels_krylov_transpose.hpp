// kernels_krylov_transpose.hpp -- the operator side of the TRANSPOSED solve_updated forms (Solver::solve_updated_core and
// solve_updated_many_core with the transposed operator, numeric.cpp): w = A_new^T z and r = b - A_new^T x with the two sums of the
// 2-norm residual, for one column and for a block of up to KRYB_COLS columns, and the conjugation of a block of interleaved complex
// columns.  A_new^T is read as the CSR form of A^T that tr_prepare() builds (tptr / trow / tmap: row i of A^T lists the rows of A with
// an entry in column i, ascending, and where each value sits in the handle's CSR order); the VALUES come from the operator's own buffer
// through tmap, so the kernels never see d_vals.
//
// Shape: the stream SpMV of kernels_vector.hpp on the rows of A^T.  tr_prepare() cuts them into blocks of at most KRYT_CAP stored
// entries (tblk); a workgroup streams its block -- lanes read CONSECUTIVE entries of tmap / trow (whole cache lines, four loads in flight
// per lane), gather the value and the element of x, and park the products in LDS -- and then sums the rows from LDS with L lanes per row
// (L: the power of two that fills the workgroup), entries in ascending order per lane, lanes by a fixed butterfly.  A row of A^T is a
// COLUMN of A and can be long whatever the rows of A look like (a dense column: an arrow matrix, a constraint): a row with more than
// KRYT_CAP entries is a block of its own and is summed in strides by the whole workgroup and a fixed tree, instead of serialising on the
// one lane k_tr_spmv would give it.  L, the cut and both trees depend on the pattern alone: same inputs, same bits, whatever the launch.
// The gather x[trow[k]] is as irregular as the column pattern of A (a stencil: neighbouring lanes read neighbouring rows); it is served
// by L2 / the Infinity Cache as the gather of the ordinary SpMV is.
//
// The block kernels keep the workgroup's rows and walk the columns, which lie n apart: the block's values (through the map) and row
// indices are read from HBM ONCE, parked in LDS (12 bytes per entry) and reused by every column; only the gathers and the results move
// per column.  No sum is formed across columns; a masked column is skipped, a launch without columns returns at once.
// The residual kernels leave their partial sums in the layout k_kry_reduce / k_kryb_reduce consume: |r|^2 at partial[blockIdx.x], |b|^2
// at partial[gridDim.x + blockIdx.x] (per column at + c pcol).  No floating-point atomics anywhere.
#pragma once
#include "kernels_krylov_blocked.hpp"

namespace hipmf {

constexpr int KRYT_CAP = 1024; // stored entries of a block of rows of A^T (a longer row stands alone)

struct KrytLds {
    double prod[KRYT_CAP];
    double red[256];
};
struct KrytStage { // a block's values and row indices, kept across the columns of a block call
    double a[KRYT_CAP];
    int32_t idx[KRYT_CAP];
};

// y_i = sum_k a_k x[trow_k] over the rows [r0, r1) of A^T with the entries [e0, e1).  STAGED: a_k and trow_k come from stg (filled by
// kryt_stage for a block within the cap), else from vals[tmap[k]] and trow[k].  Every thread of the workgroup must call it; the caller
// synchronises before the LDS is used again.
template <bool STAGED>
__device__ __forceinline__ void kryt_rows(KrytLds &sh, const KrytStage *stg, int r0, int r1, int e0, int e1, const int32_t *__restrict__ tptr,
                                          const int32_t *__restrict__ trow, const int32_t *__restrict__ tmap, const double *__restrict__ vals,
                                          const double *__restrict__ x, double *__restrict__ y) {
    const int tid = threadIdx.x;
    if (e1 - e0 > KRYT_CAP) {
        // one long row (r1 == r0 + 1): strided partial sums, fixed-order tree over the workgroup
        double acc = 0.0;
        for (int e = e0 + tid; e < e1; e += 256) acc += vals[tmap[e]] * x[trow[e]];
        sh.red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) sh.red[tid] += sh.red[tid + s];
            __syncthreads();
        }
        if (tid == 0) y[r0] = sh.red[0];
        return;
    }
    const int ne = e1 - e0;
    for (int k = tid; k < ne; k += 4 * 256) {
        double v[4], xv[4];
        int j[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = k + 256 * u;
            if (STAGED) {
                v[u] = kk < ne ? stg->a[kk] : 0.0;
                j[u] = kk < ne ? stg->idx[kk] : 0;
            } else {
                v[u] = kk < ne ? vals[tmap[e0 + kk]] : 0.0;
                j[u] = kk < ne ? trow[e0 + kk] : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) xv[u] = (k + 256 * u < ne) ? x[j[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (k + 256 * u < ne) sh.prod[k + 256 * u] = v[u] * xv[u];
    }
    __syncthreads();
    const int nr = r1 - r0;
    int lsh = 0; // log2(lanes per row)
    while (lsh < 6 && (nr << (lsh + 1)) <= 256) lsh++;
    const int L = 1 << lsh, sub = tid & (L - 1), rows_per_pass = 256 >> lsh;
    for (int rr = tid >> lsh; rr < ((nr + rows_per_pass - 1) / rows_per_pass) * rows_per_pass; rr += rows_per_pass) {
        double acc = 0.0;
        if (rr < nr)
            for (int e = tptr[r0 + rr] - e0 + sub; e < tptr[r0 + rr + 1] - e0; e += L) acc += sh.prod[e];
        for (int o = L >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o); // (every lane of the wavefront takes part: the trip count above is uniform)
        if (rr < nr && sub == 0) y[r0 + rr] = acc;
    }
}

// the block's values (through the map) and row indices into LDS; a long row is not staged (kryt_rows reads it from memory per column)
__device__ __forceinline__ void kryt_stage(KrytStage &stg, int e0, int e1, const int32_t *__restrict__ trow, const int32_t *__restrict__ tmap,
                                           const double *__restrict__ vals) {
    if (e1 - e0 > KRYT_CAP) return;
    for (int k = threadIdx.x; k < e1 - e0; k += 256) stg.a[k] = vals[tmap[e0 + k]], stg.idx[k] = trow[e0 + k];
    __syncthreads();
}

// the workgroup's rows of r hold A^T x: r = b - r there, and the two partial sums (the order of k_kry_residual)
__device__ __forceinline__ void kryt_residual_sums(KrytLds &sh, int r0, int r1, const double *__restrict__ b, double *r, double *__restrict__ partial) {
    __syncthreads(); // (the rows of this block were written by other threads of this workgroup)
    double rr = 0.0, bb = 0.0;
    for (int i = r0 + threadIdx.x; i < r1; i += 256) {
        const double bi = b[i], ri = bi - r[i];
        r[i] = ri;
        rr = fma(ri, ri, rr), bb = fma(bi, bi, bb);
    }
    rr = kry_block_sum(rr, sh.red);
    bb = kry_block_sum(bb, sh.red);
    if (threadIdx.x == 0) partial[blockIdx.x] = rr, partial[gridDim.x + blockIdx.x] = bb;
}

// w = A_new^T z
__global__ void __launch_bounds__(256) k_kry_spmv_t(const int32_t *__restrict__ tblk, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                    const int32_t *__restrict__ tmap, const double *__restrict__ vals, const double *__restrict__ z,
                                                    double *__restrict__ w) {
    __shared__ KrytLds sh;
    const int r0 = tblk[blockIdx.x], r1 = tblk[blockIdx.x + 1];
    kryt_rows<false>(sh, nullptr, r0, r1, tptr[r0], tptr[r1], tptr, trow, tmap, vals, z, w);
}

// r = b - A_new^T x, fused with the partial sums of |r|^2 (partial[blockIdx.x]) and |b|^2 (partial[gridDim.x + blockIdx.x])
__global__ void __launch_bounds__(256) k_kry_residual_t(const int32_t *__restrict__ tblk, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                        const int32_t *__restrict__ tmap, const double *__restrict__ vals, const double *__restrict__ x,
                                                        const double *__restrict__ b, double *r, double *__restrict__ partial) {
    __shared__ KrytLds sh;
    const int r0 = tblk[blockIdx.x], r1 = tblk[blockIdx.x + 1];
    kryt_rows<false>(sh, nullptr, r0, r1, tptr[r0], tptr[r1], tptr, trow, tmap, vals, x, r);
    kryt_residual_sums(sh, r0, r1, b, r, partial);
}

// W_c = A_new^T Z_c for the columns c < ncols of `mask` (Z, W: column c at + c n)
__global__ void __launch_bounds__(256) k_kryb_spmv_t(const int32_t *__restrict__ tblk, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                     const int32_t *__restrict__ tmap, const double *__restrict__ vals, int64_t n, const double *__restrict__ Z,
                                                     double *__restrict__ W, int32_t ncols, uint32_t mask) {
    __shared__ KrytLds sh;
    __shared__ KrytStage stg;
    if (ncols < 32) mask &= (1u << ncols) - 1u;
    if (!mask) return;
    const int r0 = tblk[blockIdx.x], r1 = tblk[blockIdx.x + 1], e0 = tptr[r0], e1 = tptr[r1];
    kryt_stage(stg, e0, e1, trow, tmap, vals);
    for (int c = 0; c < ncols; c++) {
        if (!((mask >> c) & 1u)) continue;
        kryt_rows<true>(sh, &stg, r0, r1, e0, e1, tptr, trow, tmap, vals, Z + (int64_t)c * n, W + (int64_t)c * n);
        __syncthreads(); // (the LDS of the block is reused by the next column)
    }
}

// R_c = B_c - A_new^T X_c for the columns of `mask`, fused with the partial sums of |r_c|^2 (partial[c pcol + blockIdx.x]) and |b_c|^2
// (partial[c pcol + gridDim.x + blockIdx.x]); X, B: column c at + c xstr / + c bstr, R at + c n
__global__ void __launch_bounds__(256) k_kryb_residual_t(const int32_t *__restrict__ tblk, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                         const int32_t *__restrict__ tmap, const double *__restrict__ vals, int64_t n, const double *__restrict__ X,
                                                         int64_t xstr, const double *__restrict__ B, int64_t bstr, double *R, int32_t ncols, uint32_t mask,
                                                         double *__restrict__ partial, int64_t pcol) {
    __shared__ KrytLds sh;
    __shared__ KrytStage stg;
    if (ncols < 32) mask &= (1u << ncols) - 1u;
    if (!mask) return;
    const int r0 = tblk[blockIdx.x], r1 = tblk[blockIdx.x + 1], e0 = tptr[r0], e1 = tptr[r1];
    kryt_stage(stg, e0, e1, trow, tmap, vals);
    for (int c = 0; c < ncols; c++) {
        if (!((mask >> c) & 1u)) continue;
        double *r = R + (int64_t)c * n;
        kryt_rows<true>(sh, &stg, r0, r1, e0, e1, tptr, trow, tmap, vals, X + (int64_t)c * xstr, r);
        kryt_residual_sums(sh, r0, r1, B + (int64_t)c * bstr, r, partial + (int64_t)c * pcol);
        __syncthreads(); // (the LDS of the block is reused by the next column)
    }
}

// V_c[2 k + 1] = -V_c[2 k + 1] for the columns c < ncols of `mask` (column c at + c stride; n doubles = n / 2 interleaved complex
// elements per column): the complex A^T forms run the A^H iteration on conjugated data.  grid (pairs / 256, columns), one thread per
// pair: unlike the column permutation kernels, which fetch a row's index and scale once for eight columns, a conjugation has nothing
// per row to share between columns, so carrying several columns per thread would only lengthen the thread.
__global__ void __launch_bounds__(256) k_tr_conj_cols(int32_t n, double *__restrict__ V, int64_t stride, uint32_t mask, int32_t ncols) {
    const int c = blockIdx.y;
    if (c >= ncols || !((mask >> c) & 1u)) return;
    const int64_t i = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x) + 1;
    if (i < n) V[(int64_t)c * stride + i] = -V[(int64_t)c * stride + i];
}

} // namespace hipmf
