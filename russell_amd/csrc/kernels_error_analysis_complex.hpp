// kernels_error_analysis_complex.hpp -- the MUMPS-style error analysis of the complex twin (complex_solver_hipmf_solve_with_error_analysis):
// the quantities of the real analysis (kernels_solve_transpose.hpp, k_ea_*) with complex moduli |z| = hypot(Re z, Im z), on the
// interleaved vectors of the real-equivalent system of order 2 nc (unknown k of the complex system = entries 2k, 2k+1).
// Row 2i of the real-equivalent CSR holds complex row i as adjacent pairs: column 2j carries a, column 2j+1 carries -b for
// a_ij = a + i b (interface_complex_hipmf.cpp, build_real_equivalent; the caller checks the pairing once per handle), so one pass
// over the even rows reads every complex entry once.  Every reduction has a fixed order: a repeat call gives the same bits.
#pragma once
#include "kernels_solve_transpose.hpp"

namespace hipmf {

__device__ __forceinline__ double zea_abs(double re, double im) { return hypot(re, im); }

// One pass over the even rows of A (one thread per complex row i), fused with the residual: r_i = b_i - (A x)_i with its real and
// imaginary parts in two double-double accumulators (rounded once each), ax_i = (|A||x|)_i, arow_i = sum_j |a_ij|; block maxima
// (atomicMax on the bits) into sc: [0] N_A = max arow_i, [1] N_x = max |x_i|, [2] max |r_i|.  Entries in stored order per row.
// x, b, r: interleaved (2 nc doubles); ax, arow: nc doubles.
__global__ void __launch_bounds__(256) k_zea_rows(int32_t nc, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                  const double *__restrict__ vals, const double *__restrict__ x, const double *__restrict__ b,
                                                  double *__restrict__ r, double *__restrict__ ax, double *__restrict__ arow, unsigned long long *sc) {
    __shared__ double s0[256], s1[256], s2[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double na = 0.0, nx = 0.0, nr = 0.0;
    if (i < nc) {
        double rs = b[2 * i], rc = 0.0, is = b[2 * i + 1], ic = 0.0, d = 0.0, a = 0.0;
        for (int e = rp[2 * i]; e < rp[2 * i + 1]; e += 2) {
            const double va = vals[e], mb = vals[e + 1]; // a_ij = va - i mb
            const int j2 = ci[e];
            const double xr = x[j2], xi = x[j2 + 1];
            ea_dot2_sub(rs, rc, va, xr); // Re: a xr - b xi = va xr + mb xi
            ea_dot2_sub(rs, rc, mb, xi);
            ea_dot2_sub(is, ic, va, xi); // Im: a xi + b xr = va xi - mb xr
            ea_dot2_sub(is, ic, -mb, xr);
            const double m = zea_abs(va, mb);
            d += m * zea_abs(xr, xi), a += m;
        }
        const double rr = rs + rc, ri = is + ic;
        r[2 * i] = rr, r[2 * i + 1] = ri, ax[i] = d, arow[i] = a;
        na = a, nx = zea_abs(x[2 * i], x[2 * i + 1]), nr = zea_abs(rr, ri);
    }
    s0[threadIdx.x] = na, s1[threadIdx.x] = nx, s2[threadIdx.x] = nr;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s0[threadIdx.x] = fmax(s0[threadIdx.x], s0[threadIdx.x + s]);
            s1[threadIdx.x] = fmax(s1[threadIdx.x], s1[threadIdx.x + s]);
            s2[threadIdx.x] = fmax(s2[threadIdx.x], s2[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) tr_atomic_max(sc, s0[0]), tr_atomic_max(sc + 1, s1[0]), tr_atomic_max(sc + 2, s2[0]);
}

// The split into I1 = {d_i > tau_i} and I2 with the moduli of r and b, the backward errors and the real weights of the two condition
// numbers: sc[3] = omega1, sc[4] = omega2 (atomicMax on the bits), cnt[0] = |I2|.  r, b interleaved; ax, arow, w1, w2: nc doubles.
__global__ void __launch_bounds__(256) k_zea_split(int32_t nc, double tau_scale, double nx, const double *__restrict__ r, const double *__restrict__ ax,
                                                   const double *__restrict__ arow, const double *__restrict__ b, double *__restrict__ w1,
                                                   double *__restrict__ w2, unsigned long long *sc, int32_t *cnt) {
    __shared__ double s3[256], s4[256];
    __shared__ int c2[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double o1 = 0.0, o2 = 0.0;
    int in2 = 0;
    if (i < nc) {
        const double ab = zea_abs(b[2 * i], b[2 * i + 1]), ar = zea_abs(r[2 * i], r[2 * i + 1]);
        const double d = ax[i] + ab, tau = tau_scale * (arow[i] * nx + ab);
        if (d > tau) {
            o1 = ar / d;
            w1[i] = d, w2[i] = 0.0;
        } else {
            const double d2 = ax[i] + arow[i] * nx;
            o2 = ar == 0.0 ? 0.0 : ar / d2; // (0 / 0 counts as 0)
            w1[i] = 0.0, w2[i] = d2;
            in2 = 1;
        }
    }
    s3[threadIdx.x] = o1, s4[threadIdx.x] = o2, c2[threadIdx.x] = in2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s3[threadIdx.x] = fmax(s3[threadIdx.x], s3[threadIdx.x + s]);
            s4[threadIdx.x] = fmax(s4[threadIdx.x], s4[threadIdx.x + s]);
            c2[threadIdx.x] += c2[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tr_atomic_max(sc + 3, s3[0]), tr_atomic_max(sc + 4, s4[0]);
        if (c2[0]) atomicAdd(cnt, c2[0]);
    }
}

// y = w o v: real weights (nc) times a complex vector (interleaved)
__global__ void k_zea_hadamard(int32_t nc, const double *__restrict__ w, const double *__restrict__ v, double *__restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const double wi = w[i];
    y[2 * i] = wi * v[2 * i], y[2 * i + 1] = wi * v[2 * i + 1];
}

// v = e / nc (mode 0), the real alternating test vector (-1)^i (1 + i / (nc - 1)) (mode 1), e_j (mode 2); imaginary parts zero
__global__ void k_zea_fill(int32_t nc, int32_t mode, int32_t j, double *__restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    double re;
    if (mode == 0) re = 1.0 / (double)nc;
    else if (mode == 1) re = ((i & 1) ? -1.0 : 1.0) * (1.0 + (nc > 1 ? (double)i / (double)(nc - 1) : 0.0));
    else re = i == j ? 1.0 : 0.0;
    v[2 * i] = re, v[2 * i + 1] = 0.0;
}

// xi = y / |y|, or 1 where |y| <= DBL_MIN (zlacn2's complex sign; no record of the previous sign vector: zlacn2 has no repeat test)
__global__ void k_zea_sign(int32_t nc, const double *__restrict__ y, double *__restrict__ xi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const double yr = y[2 * i], yi = y[2 * i + 1], m = zea_abs(yr, yi);
    if (m > 2.2250738585072014e-308) xi[2 * i] = yr / m, xi[2 * i + 1] = yi / m;
    else xi[2 * i] = 1.0, xi[2 * i + 1] = 0.0;
}

// First stage of the fixed-order reductions over the moduli of a complex vector (EA_RED_WG workgroups, fixed strides, a fixed tree;
// k_ea_reduce2 combines the partials).  mode 0: sum |v_i|; mode 1: max |v_i| with the smallest index on ties.
__global__ void __launch_bounds__(256) k_zea_reduce1(int32_t nc, int32_t mode, const double *__restrict__ v, double *__restrict__ pv, int32_t *__restrict__ pi) {
    __shared__ double sv[256];
    __shared__ int si[256];
    double a = 0.0;
    int ai = 0x7fffffff;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nc; i += EA_RED_WG * 256) {
        const double t = zea_abs(v[2 * i], v[2 * i + 1]);
        if (mode == 0) a += t;
        else if (ai == 0x7fffffff || t > a) a = t, ai = i; // (ascending i: a tie keeps the smaller index)
    }
    sv[threadIdx.x] = a, si[threadIdx.x] = ai;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            if (mode == 0) sv[threadIdx.x] += sv[threadIdx.x + s];
            else {
                const double ov = sv[threadIdx.x + s];
                const int oi = si[threadIdx.x + s];
                if (oi != 0x7fffffff && (si[threadIdx.x] == 0x7fffffff || ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])))
                    sv[threadIdx.x] = ov, si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) pv[blockIdx.x] = sv[0], pi[blockIdx.x] = si[0];
}

// out[0] = |v_j| (the modulus zlacn2 compares with the new maximum, computed as the reduction computes it)
__global__ void k_zea_abs_at(const double *__restrict__ v, int32_t j, double *out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = zea_abs(v[2 * j], v[2 * j + 1]);
}

} // namespace hipmf
