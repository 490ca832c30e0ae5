// kernels_krylov_complex.hpp -- the Arnoldi process of complex_solver_hipmf_solve_updated (Solver::solve_updated_complex, numeric.cpp):
// the flexible GMRES of kernels_krylov.hpp in COMPLEX arithmetic on the vectors of the real-equivalent system.  A vector of nc complex
// numbers is n = 2 nc interleaved doubles (re, im); V ((m + 1) x n) and Z (m x n) are column-major with stride n, as in the real form.
//
// Shape: that of kernels_krylov.hpp -- a workgroup of 256 threads owns KRY_TILE = 1024 consecutive doubles (512 complex numbers), a
// thread two 16-byte pairs.  Each pair IS one complex element: the tile base 1024 blockIdx.x and 2 threadIdx.x are even, KRY_TILE / 2 is
// even, and every basis vector starts at a multiple of n = 2 nc doubles, so a pair never straddles two complex numbers and, n being
// even, never the end of the vector (a pair is inside or outside as a whole: no one-element tail).  The kernels rely on that; the
// caller checks that n is even.
//
// The inner product is <v, w> = sum conj(v_i) w_i: per basis vector TWO sums (real and imaginary part), twice the accumulators and LDS
// slots of the real kernels, and the update spends four fused multiply-adds per complex element on two coefficient registers.  A pass
// over the registers that hold w takes ZKRY_PASSV = 5 basis vectors: 20 independent 16-byte loads in flight per thread, and as compiled
// for gfx950 61 VGPRs (k_zkry_dots), 72 (k_zkry_update) and 70 (k_zkry_combine): seven waves per SIMD for all three.  4 vectors give 52 /
// 48 / 46 VGPRs and eight waves but fewer loads in flight per SIMD (8 x 16 against 7 x 20); 6 give 69 / 84 / 82 and drop the update to
// five waves, 8 (the real kernels' count) 85 / 108 / 106 and four.  No scratch in any of them.  w is read from HBM once whatever the
// number of vectors.
//
// Sums never use floating-point atomics: every workgroup writes its partial sums to slots of its own -- column 2 j holds the real
// parts of basis vector j, column 2 j + 1 the imaginary parts, the workgroups of a column contiguous -- and k_kry_reduce over 2 nv
// columns leaves the nv complex coefficients interleaved.  The squared norm of w is the plain sum over its n doubles (k_kry_reduce over
// one column), the normalisation a real scaling (k_kry_scale), the residual that of the real-equivalent system (k_kry_residual).
#pragma once
#include "kernels_krylov.hpp"

namespace hipmf {

constexpr int ZKRY_PASSV = 5; // basis vectors per pass over the registers that hold w

// the complex element at doubles i, i + 1 (i even, n even: inside or outside as a whole)
__device__ __forceinline__ void zkry_ld(const double *__restrict__ p, int64_t i, int64_t n, double &re, double &im) {
    if (i < n) {
        const f64x2 v = ld_f64x2(p + i);
        re = v.x, im = v.y;
    } else {
        re = 0.0, im = 0.0;
    }
}
__device__ __forceinline__ void zkry_st(double *__restrict__ p, int64_t i, int64_t n, double re, double im) {
    if (i < n) {
        f64x2 v;
        v.x = re, v.y = im;
        st_f64x2(p + i, v);
    }
}

// partial[(2 j + c) * gridDim.x + blockIdx.x] = real (c = 0) and imaginary (c = 1) part of the sum over the workgroup's tile of
// conj(V(i, j)) w_i, j < nv.  One pass over w; ceil(nv / ZKRY_PASSV) passes over the registers.  Bytes: (nv + 1) 8 n read,
// 16 nv gridDim.x written.
__global__ void __launch_bounds__(256) k_zkry_dots(int64_t n, const double *__restrict__ w, const double *__restrict__ V, int32_t nv, double *__restrict__ partial) {
    __shared__ double red[2 * ZKRY_PASSV][4];
    const int64_t i0 = (int64_t)blockIdx.x * KRY_TILE + 2 * (int)threadIdx.x, i1 = i0 + KRY_TILE / 2;
    double w0, w1, w2, w3;
    zkry_ld(w, i0, n, w0, w1);
    zkry_ld(w, i1, n, w2, w3);
    for (int j0 = 0; j0 < nv; j0 += ZKRY_PASSV) {
        double a[ZKRY_PASSV][4], acc[2 * ZKRY_PASSV];
#pragma unroll
        for (int q = 0; q < ZKRY_PASSV; q++) { // (clamped vector: unconditional loads, the surplus sums are not stored)
            const double *v = V + (int64_t)(j0 + q < nv ? j0 + q : nv - 1) * n;
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
        if (q < 2 * ZKRY_PASSV && j0 + (q >> 1) < nv) partial[(int64_t)(2 * j0 + q) * gridDim.x + blockIdx.x] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    }
}

// w -= sum_j c_j V(:, j) (SUB) or w += sum_j c_j V(:, j), j < nv in ascending order, c_j complex (interleaved, device memory); NORM: the
// partial sums of |w|^2 of the result go to partial[blockIdx.x].  Bytes: (nv + 2) 8 n.
template <bool SUB, bool NORM>
__device__ __forceinline__ void zkry_axpy_many(int64_t n, double *__restrict__ w, const double *__restrict__ V, int32_t nv, const double *__restrict__ c,
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
                const double *v = V + (int64_t)(j0 + q) * n;
                cr[q] = SUB ? -c[2 * (j0 + q)] : c[2 * (j0 + q)];
                ci[q] = SUB ? -c[2 * (j0 + q) + 1] : c[2 * (j0 + q) + 1];
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
// one round of classical Gram-Schmidt: w -= sum_j h_j v_j with complex h_j, fused with the partial sums of |w|^2
__global__ void __launch_bounds__(256) k_zkry_update(int64_t n, double *__restrict__ w, const double *__restrict__ V, int32_t nv, const double *__restrict__ h,
                                                     double *__restrict__ partial) {
    zkry_axpy_many<true, true>(n, w, V, nv, h, partial);
}
// x += sum_j y_j z_j, complex y_j
__global__ void __launch_bounds__(256) k_zkry_combine(int64_t n, double *__restrict__ x, const double *__restrict__ Z, int32_t nv, const double *__restrict__ y) {
    zkry_axpy_many<false, false>(n, x, Z, nv, y, nullptr);
}

} // namespace hipmf
