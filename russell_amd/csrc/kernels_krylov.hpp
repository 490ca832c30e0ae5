// kernels_krylov.hpp -- the Arnoldi process of solver_hipmf_solve_updated (Solver::solve_updated, numeric.cpp) on device-resident bases:
// flexible GMRES whose operator is the matrix with NEW values and whose right preconditioner is the kept factor.  All kernels are
// HBM-bound vector kernels over n doubles; V ((m + 1) x n) and Z (m x n) are column-major with stride n.
//
// Shape shared by all of them: a workgroup of 256 threads owns KRY_TILE = 1024 consecutive elements, a thread two pairs of neighbours
// (16-byte loads from 8-byte aligned addresses: the columns of a basis start at multiples of n, which may be odd).  The thread keeps its
// four elements of w in registers and walks the basis vectors KRY_PASSV = 8 at a time: 32 independent loads in flight per thread, 8
// accumulators (16 VGPRs) + 32 loaded values (64 VGPRs) + w (8): as compiled 80 VGPRs (k_kry_dots, six waves per SIMD) and 94
// (k_kry_update, five); 16 vectors per pass would need about 170 and halve the occupancy for no more bytes in flight.  w is read from HBM
// ONCE whatever the number of basis vectors.
//
// Sums over n never use floating-point atomics: every workgroup writes its partial sums to a slot of its own (column-major: all
// workgroups' partials of one basis vector are contiguous), k_kry_reduce adds the slots of a column in a fixed order -- inside a
// workgroup the 16-lane rows by a DPP butterfly, rows, wavefronts and strides in index order.  Same inputs, same bits.
#pragma once
#include "kernels_vector.hpp"

namespace hipmf {

constexpr int KRY_TILE = 1024; // elements of a vector per workgroup
constexpr int KRY_PASSV = 8;   // basis vectors per pass over the registers that hold w

__device__ __forceinline__ void kry_ld2(const double *__restrict__ p, int64_t i, int64_t n, double &a, double &b) {
    if (i + 1 < n) {
        const f64x2 v = ld_f64x2(p + i);
        a = v.x, b = v.y;
    } else {
        a = i < n ? p[i] : 0.0, b = 0.0;
    }
}
__device__ __forceinline__ void kry_st2(double *__restrict__ p, int64_t i, int64_t n, double a, double b) {
    if (i + 1 < n) {
        f64x2 v;
        v.x = a, v.y = b;
        st_f64x2(p + i, v);
    } else if (i < n) {
        p[i] = a;
    }
}

// sum of v over the 256 threads of the workgroup, the same bits in every thread (every thread must call it; red: 4 doubles of LDS)
__device__ __forceinline__ double kry_block_sum(double v, double *red) {
    v = wave_sum_f64(v);
    __syncthreads(); // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[j * gridDim.x + blockIdx.x] = sum over the workgroup's tile of w_i V(i, j), j < nv.  One pass over w; ceil(nv / KRY_PASSV) passes
// over the registers.  Bytes: (nv + 1) 8 n read, 8 nv gridDim.x written.
__global__ void __launch_bounds__(256) k_kry_dots(int64_t n, const double *__restrict__ w, const double *__restrict__ V, int32_t nv, double *__restrict__ partial) {
    __shared__ double red[KRY_PASSV][4];
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double w0, w1, w2, w3;
    kry_ld2(w, i0, n, w0, w1);
    kry_ld2(w, i1, n, w2, w3);
    for (int j0 = 0; j0 < nv; j0 += KRY_PASSV) {
        double a[KRY_PASSV][4], acc[KRY_PASSV];
#pragma unroll
        for (int q = 0; q < KRY_PASSV; q++) { // (clamped vector: unconditional loads, the surplus sums are not stored)
            const double *v = V + (int64_t)(j0 + q < nv ? j0 + q : nv - 1) * n;
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
        if (q < KRY_PASSV && j0 + q < nv) partial[(int64_t)(j0 + q) * gridDim.x + blockIdx.x] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    }
}

// out[c] = sum over b < nblk of partial[c * nblk + b], one workgroup per column c: thread t adds the slots t, t + 256, ... in order,
// then the 256 sums are added as in kry_block_sum
__global__ void __launch_bounds__(256) k_kry_reduce(const double *__restrict__ partial, int32_t nblk, double *__restrict__ out) {
    __shared__ double red[4];
    const double *p = partial + (int64_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += p[b];
    s = kry_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// w -= sum_j c_j V(:, j) (SUB) or w += sum_j c_j V(:, j), j < nv in ascending order, coefficients in device memory; NORM: the partial
// sums of |w|^2 of the result go to partial[blockIdx.x].  Bytes: (nv + 2) 8 n.
template <bool SUB, bool NORM>
__device__ __forceinline__ void kry_axpy_many(int64_t n, double *__restrict__ w, const double *__restrict__ V, int32_t nv, const double *__restrict__ c,
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
                const double *v = V + (int64_t)(j0 + q) * n;
                cj[q] = SUB ? -c[j0 + q] : c[j0 + q];
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
// one round of classical Gram-Schmidt: w -= sum_j h_j v_j, fused with the partial sums of |w|^2
__global__ void __launch_bounds__(256) k_kry_update(int64_t n, double *__restrict__ w, const double *__restrict__ V, int32_t nv, const double *__restrict__ h,
                                                    double *__restrict__ partial) {
    kry_axpy_many<true, true>(n, w, V, nv, h, partial);
}
// x += sum_j y_j z_j
__global__ void __launch_bounds__(256) k_kry_combine(int64_t n, double *__restrict__ x, const double *__restrict__ Z, int32_t nv, const double *__restrict__ y) {
    kry_axpy_many<false, false>(n, x, Z, nv, y, nullptr);
}

// v = w / sqrt(*nrm2)  (the squared norm comes from k_kry_reduce: no host round trip between the update and the next basis vector)
__global__ void __launch_bounds__(256) k_kry_scale(int64_t n, const double *__restrict__ w, const double *__restrict__ nrm2, double *__restrict__ v) {
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    const double s = 1.0 / sqrt(nrm2[0]);
    double w0, w1, w2, w3;
    kry_ld2(w, i0, n, w0, w1);
    kry_ld2(w, i1, n, w2, w3);
    kry_st2(v, i0, n, w0 * s, w1 * s);
    kry_st2(v, i1, n, w2 * s, w3 * s);
}

// r = b - A x on the row blocks of the stream SpMV (spmv_block), fused with the partial sums of |r|^2 (partial[blockIdx.x]) and of |b|^2
// (partial[gridDim.x + blockIdx.x]).  The product is parked in r first; the workgroup then revisits its own rows.
__global__ void __launch_bounds__(256) k_kry_residual(const int32_t *__restrict__ row_blk, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                      const double *__restrict__ vals, const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                      const int32_t *__restrict__ arow, const double *__restrict__ x, const double *__restrict__ b,
                                                      double *r, double *__restrict__ partial) {
    __shared__ SpmvLds sh;
    spmv_block<false>(sh, row_blk, rp, ci, vals, tptr, tidx, arow, 1.0, x, nullptr, r, nullptr);
    __syncthreads(); // (the rows of this block were written by other threads of this workgroup)
    const int r0 = row_blk[blockIdx.x], r1 = row_blk[blockIdx.x + 1];
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

} // namespace hipmf
