// kernels_border_complex.hpp -- the complex form of the bordered systems on the kept factor (complex_solver_hipmf_set_border /
// complex_solver_hipmf_solve_bordered / complex_solver_hipmf_solve_bordered_transpose; Solver::set_border and Solver::bordered_core in
// their pairs mode, numeric.cpp):
//     [ A   B ] [x]   [f]      A the factorised complex n x n matrix, B, C n x k complex dense, D k x k complex dense, k <= ZBORDER_MAX
//     [ C^T D ] [z] = [g]      (C^T the plain transpose)
// The handle holds the REAL-EQUIVALENT system of order 2n on interleaved (re, im) vectors (interface_complex_hipmf.cpp): a + i b at (i, j)
// is [a -b; b a] at rows 2i, 2i+1 / columns 2j, 2j+1.  The border is kept in that form too, 2k real columns packed as kernels_border.hpp
// packs k: column 2j of a packed array is the interleaved complex column j, column 2j+1 the same column times i, every pair (re, im)
// rotated to (-im, re) (k_zborder_pack).  B and W = A^{-1} B are packed as they are; for C the packed array is the real-equivalent form
// of conj(C), whose transpose is the real-equivalent form of C^T.  With these operands the products of the elimination -- t = g - C^T y
// (k_border_gram, k_border_reduce) and x = y - W z (k_border_apply) -- ARE the real kernels of kernels_border.hpp on 2k columns, and a
// product C^T Y of interleaved columns comes out as interleaved complex numbers, column-major with kp doubles per column.
//
// What complex arithmetic needs is here:
// k_zborder_pack, k_zborder_unpack  interleaved complex columns into and out of the packed real-equivalent form
// k_zborder_adjoint  D^H of the small diagonal block (the transposed side)
// k_zborder_lu     S = D - C^T W as a COMPLEX k x k matrix in LDS, partial pivoting by modulus; the complex determinant as a mantissa
//                  pair of modulus in [1, 10) and a base-10 exponent (the form of Solver::determinant_complex), min and max |u_ii|, the
//                  flag of an exactly zero pivot.  Real and imaginary parts lie in two planes of 32 x 32 doubles (16 KB together): every
//                  LDS access is an 8-byte one with the strides of k_border_lu, instead of 16-byte elements whose two halves share banks.
// k_zborder_small_solve  dz = S^{-1} (g - G) from that LU, one wavefront per column.  The transposed side is M^H, the transposed
//                  real-equivalent system, with V = A^{-H} conj(C) and a Schur complement of its own, S_T = D^H - B^H V, factorised by
//                  the same kernel (why not S^{-H} from the LU of S: Solver::bt_prepare) -- so the same solve serves there.  M^H alone
//                  serves both transposed calls: M^T [y; w] = [p; q] is M^H [conj y; conj w] = [conj p; conj q], so the call with
//                  conjugate = 0 runs the loop of M^H on conjugated data (k_tr_conj_cols on the way in and out), with the same V.
// k_zborder_residual_n, k_zborder_residual_nt, k_zborder_rows_part, k_zborder_rows  the residual of all n + k COMPLEX rows, every real
//                  and imaginary part accumulated beyond twice the working precision and rounded once (a complex product is four real
//                  TwoProducts; why: kernels_border.hpp), and omega per complex row on complex moduli,
//                      |r_i| / (sum_j |a_ij| |x_j| + sum_j |b_ij| |z_j| + |f_i|),
//                  not on the 2n real rows taken separately.  One thread per complex row reads the real rows 2i and 2i+1 of the handle's
//                  CSR; the moduli |a_ij| come from row 2i, where stored entry (i, j) is the adjacent pair (Re a_ij, -Im a_ij) at columns
//                  2j, 2j+1 (build_real_equivalent writes both wherever it writes one; check_pairs of the interface).
// No floating-point atomics except the exact maxima; the order of every sum is fixed by n, k and the block alone.
#pragma once
#include "kernels_border.hpp"

namespace hipmf {

constexpr int ZBORDER_MAX = 32; // complex border rows / columns at most (HIPMF_COMPLEX_BORDER_MAX): 2 ZBORDER_MAX = BORDER_MAX real ones

// (a + i b) / (c + i d) without the overflow of c^2 + d^2 (Smith)
__device__ __forceinline__ void zb_div(double a, double b, double c, double d, double &re, double &im) {
    if (fabs(c) >= fabs(d)) {
        const double t = d / c, den = c + d * t;
        re = (a + b * t) / den, im = (b - a * t) / den;
    } else {
        const double t = c / d, den = c * t + d;
        re = (a * t + b) / den, im = (b * t - a) / den;
    }
}

// complex columns [j0, j0 + ncols) of the packed real-equivalent form (kp real columns per real row) from interleaved complex columns
// (nc complex rows, ld DOUBLES from column to column); conj != 0: the real-equivalent form of the conjugated columns
__global__ void __launch_bounds__(256) k_zborder_pack(int32_t nc, int32_t ncols, int32_t kp, int32_t j0, const double *__restrict__ src, int64_t ld, int32_t conj,
                                                      double *__restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = e / ncols;
    const int j = (int)(e - i * ncols);
    if (i >= nc) return;
    const double a = src[2 * i + (int64_t)j * ld], b0 = src[2 * i + 1 + (int64_t)j * ld], b = conj ? -b0 : b0;
    double *d0 = dst + 2 * i * kp + 2 * (j0 + j), *d1 = d0 + kp;
    d0[0] = a, d0[1] = -b; // row 2i:     ( re, -im)
    d1[0] = b, d1[1] = a;  // row 2i + 1: ( im,  re)
}

// k_zborder_pack backwards: the interleaved complex columns are the even columns of the packed form
__global__ void __launch_bounds__(256) k_zborder_unpack(int32_t nc, int32_t ncols, int32_t kp, int32_t j0, const double *__restrict__ src, double *__restrict__ dst,
                                                        int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = e / ncols;
    const int j = (int)(e - i * ncols);
    if (i >= nc) return;
    const double *s0 = src + 2 * i * kp + 2 * (j0 + j);
    dst[2 * i + (int64_t)j * ld] = s0[0], dst[2 * i + 1 + (int64_t)j * ld] = s0[kp];
}

// Dh = D^H, both column-major interleaved complex with kp doubles per column
__global__ void __launch_bounds__(256) k_zborder_adjoint(int32_t k, int32_t kp, const double *__restrict__ D, double *__restrict__ Dh) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= k * k) return;
    const int i = e % k, j = e / k;
    Dh[2 * i + (int64_t)j * kp] = D[2 * j + (int64_t)i * kp], Dh[2 * i + 1 + (int64_t)j * kp] = -D[2 * j + 1 + (int64_t)i * kp];
}

// One workgroup: complex LU of S = D - G with partial pivoting by modulus (D, G, LU: column-major interleaved complex, kp doubles per
// column).  piv[j]: the row exchanged with row j at step j.  rec: [0] min |u_ii|, [1] max |u_ii|, [2] and [5] real and imaginary mantissa
// of det S, [3] its base-10 exponent, [4] 1 for an exactly zero pivot, which ends the elimination (LU is then not to be used).
__global__ void __launch_bounds__(256) k_zborder_lu(int32_t k, int32_t kp, const double *__restrict__ D, const double *__restrict__ G, double *__restrict__ LU,
                                                    int32_t *__restrict__ piv, double *__restrict__ rec) {
    __shared__ double sr[ZBORDER_MAX * ZBORDER_MAX], si[ZBORDER_MAX * ZBORDER_MAX]; // column-major, leading dimension k
    __shared__ int prow;
    __shared__ int bad;
    const int tid = threadIdx.x;
    for (int e = tid; e < k * k; e += 256) {
        const int64_t at = 2 * (e % k) + (int64_t)(e / k) * kp;
        sr[e] = D[at] - G[at], si[e] = D[at + 1] - G[at + 1];
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    double mr = 1.0, mi = 0.0, expo = 0.0, umin = INFINITY, umax = 0.0; // (thread 0's)
    for (int j = 0; j < k; j++) {
        if (tid == 0) {
            int best = j;
            double vb = hypot(sr[j + j * k], si[j + j * k]);
            for (int i = j + 1; i < k; i++) { // (the first of equal candidates; a NaN is never chosen over a number)
                const double v = hypot(sr[i + j * k], si[i + j * k]);
                if (v > vb) vb = v, best = i;
            }
            prow = best, piv[j] = best;
            if (!(vb > 0.0)) bad = 1;
        }
        __syncthreads();
        if (bad) break; // (workgroup-uniform)
        const int r = prow;
        if (r != j)
            for (int c = tid; c < k; c += 256) {
                const double tr = sr[j + c * k], ti = si[j + c * k];
                sr[j + c * k] = sr[r + c * k], si[j + c * k] = si[r + c * k];
                sr[r + c * k] = tr, si[r + c * k] = ti;
            }
        __syncthreads();
        const double dr = sr[j + j * k], di = si[j + j * k];
        if (tid == 0) {
            if (r != j) mr = -mr, mi = -mi;
            const double tr = mr * dr - mi * di, ti = mr * di + mi * dr;
            mr = tr, mi = ti;
            double mm = hypot(mr, mi);
            while (mm >= 10.0 && mm <= 1.79769313486231570815e308) mr /= 10.0, mi /= 10.0, mm /= 10.0, expo += 1.0;
            while (mm < 1.0 && mm > 0.0) mr *= 10.0, mi *= 10.0, mm *= 10.0, expo -= 1.0;
            const double a = hypot(dr, di);
            umin = a < umin ? a : umin, umax = a > umax ? a : umax;
        }
        __syncthreads(); // (the pivot has been read by everyone before the column below it is scaled)
        for (int i = j + 1 + tid; i < k; i += 256) {
            double qr, qi;
            zb_div(sr[i + j * k], si[i + j * k], dr, di, qr, qi);
            sr[i + j * k] = qr, si[i + j * k] = qi;
        }
        __syncthreads();
        const int rem = k - j - 1;
        for (int e = tid; e < rem * rem; e += 256) {
            const int i = j + 1 + e % rem, c = j + 1 + e / rem;
            const double lr = sr[i + j * k], li = si[i + j * k], ur = sr[j + c * k], ui = si[j + c * k];
            sr[i + c * k] = fma(li, ui, fma(-lr, ur, sr[i + c * k]));
            si[i + c * k] = fma(-li, ur, fma(-lr, ui, si[i + c * k]));
        }
        __syncthreads();
    }
    for (int e = tid; e < k * k; e += 256) {
        const int64_t at = 2 * (e % k) + (int64_t)(e / k) * kp;
        LU[at] = sr[e], LU[at + 1] = si[e];
    }
    if (tid == 0) {
        rec[0] = umin, rec[1] = umax, rec[2] = bad ? 0.0 : mr, rec[3] = bad ? 0.0 : expo, rec[4] = bad ? 1.0 : 0.0, rec[5] = bad ? 0.0 : mi;
        for (int j = 6; j < BORDER_REC; j++) rec[j] = 0.0;
    }
}

// One wavefront per column c (grid m), lane j = complex row j: dz = S^{-1} (g - G) from the LU of k_zborder_lu (P S = L U).
// g, G, dz, z, zs: interleaved, kp doubles per column, the entries from 2k on zero.  zs, mask: as k_border_small_solve.
__global__ void __launch_bounds__(64) k_zborder_small_solve(int32_t k, int32_t kp, const double *__restrict__ LU, const int32_t *__restrict__ piv,
                                                            const double *__restrict__ g, const double *__restrict__ G, double *__restrict__ dz,
                                                            double *__restrict__ z, double *__restrict__ zs, uint32_t mask) {
    __shared__ double tr[ZBORDER_MAX], ti[ZBORDER_MAX];
    const int c = blockIdx.x, j = threadIdx.x;
    if (!((mask >> c) & 1u)) return;
    const int64_t col = (int64_t)c * kp;
    if (j < k) tr[j] = g[col + 2 * j] - G[col + 2 * j], ti[j] = g[col + 2 * j + 1] - G[col + 2 * j + 1];
    __syncthreads();
    if (j == 0)
        for (int q = 0; q < k; q++) {
            const int r = piv[q];
            if (r != q) {
                const double vr = tr[q], vi = ti[q];
                tr[q] = tr[r], ti[q] = ti[r], tr[r] = vr, ti[r] = vi;
            }
        }
    __syncthreads();
    for (int q = 0; q < k; q++) { // L y = P t, unit diagonal
        const double qr = tr[q], qi = ti[q];
        __syncthreads();
        if (j > q && j < k) {
            const double lr = LU[2 * j + (int64_t)q * kp], li = LU[2 * j + 1 + (int64_t)q * kp];
            tr[j] = fma(li, qi, fma(-lr, qr, tr[j])), ti[j] = fma(-li, qr, fma(-lr, qi, ti[j]));
        }
        __syncthreads();
    }
    for (int q = k - 1; q >= 0; q--) { // U dz = y
        if (j == q) {
            double vr, vi;
            zb_div(tr[q], ti[q], LU[2 * q + (int64_t)q * kp], LU[2 * q + 1 + (int64_t)q * kp], vr, vi);
            tr[q] = vr, ti[q] = vi;
        }
        __syncthreads();
        const double qr = tr[q], qi = ti[q];
        if (j < q) {
            const double ur = LU[2 * j + (int64_t)q * kp], ui = LU[2 * j + 1 + (int64_t)q * kp];
            tr[j] = fma(ui, qi, fma(-ur, qr, tr[j])), ti[j] = fma(-ui, qr, fma(-ur, qi, ti[j]));
        }
        __syncthreads();
    }
    if (2 * j < kp) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const double v = j < k ? (h ? ti[j] : tr[j]) : 0.0;
            const int64_t at = col + 2 * j + h;
            dz[at] = v;
            if (zs) {
                const double old = z[at];
                zs[at] = old, z[at] = old + v;
            } else {
                z[at] = v;
            }
        }
    }
}

// the quotient of a complex row's omega (0 / 0 counts 0, nonzero / 0 counts 1, as in spmv_block; a NaN never wins the maximum)
__device__ __forceinline__ double zb_quot(double rr, double ri, double den) {
    const double am = hypot(rr, ri), q = den > 0.0 ? am / den : (am > 0.0 ? 1.0 : 0.0);
    return q > 0.0 ? q : 0.0;
}

// the block maxima of a column's quotients into word 1 of the slots of kernels_vector.hpp (red: one double per wavefront)
__device__ __forceinline__ void zb_block_max(double *red, double qi, unsigned long long *nrm) {
    for (int off = 32; off > 0; off >>= 1) {
        const double other = __shfl_xor(qi, off);
        qi = other > qi ? other : qi;
    }
    __syncthreads(); // (the maxima of the column before have been read)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = qi;
    __syncthreads();
    if (threadIdx.x == 0) {
        double mx = red[0];
        for (int w = 1; w < 4; w++) mx = red[w] > mx ? red[w] : mx;
        atomicMax(nrm + (size_t)(blockIdx.x & (RES_SLOTS - 1)) * RES_SLOT_WORDS + 1, (unsigned long long)__double_as_longlong(mx));
    }
}

// complex rows of A: one thread per complex row i (nc of them), the columns of the block in turn.  r = f - A x - B z in the real rows
// 2i, 2i+1 (vals, Bp, Z, x, f, r: the real-equivalent arrays of k_border_residual_n; k complex border columns = 2k packed ones), den and
// omega on moduli (see the head of the file).  A column whose bit in `mask` is clear: r = 0, no omega.
__global__ void __launch_bounds__(256) k_zborder_residual_n(int32_t nc, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const double *__restrict__ vals,
                                                            int32_t k, int32_t kp, const double *__restrict__ Bp, const double *__restrict__ Z,
                                                            const double *__restrict__ x, int64_t xstr, const double *__restrict__ f, int64_t fstr,
                                                            double *__restrict__ r, int64_t rstr, unsigned long long *nrm, int32_t ncols, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < nc;
    const int e0 = in ? rp[2 * i] : 0, e1 = in ? rp[2 * i + 1] : 0, e2 = in ? rp[2 * i + 2] : 0;
    for (int c = 0; c < ncols; c++) { // (workgroup-uniform)
        if (!((mask >> c) & 1u)) {
            if (in) r[2 * i + c * rstr] = 0.0, r[2 * i + 1 + c * rstr] = 0.0;
            continue;
        }
        const double *xc = x + c * xstr, *zc = Z + (int64_t)c * kp;
        double qi = 0.0;
        if (in) {
            const double fr = f[2 * i + c * fstr], fi = f[2 * i + 1 + c * fstr];
            XrSum ar = {fr, 0.0, 0.0}, ai = {fi, 0.0, 0.0};
            double den = hypot(fr, fi);
            for (int e = e0; e + 1 < e1; e += 2) { // row 2i: the pairs (Re a, -Im a) at the columns 2j, 2j+1
                const double a0 = vals[e], a1 = vals[e + 1], x0 = xc[ci[e]], x1 = xc[ci[e + 1]];
                xr_dot_sub(ar, a0, x0);
                xr_dot_sub(ar, a1, x1);
                den += hypot(a0, a1) * hypot(x0, x1);
            }
            for (int e = e1; e < e2; e++) xr_dot_sub(ai, vals[e], xc[ci[e]]); // row 2i+1
            const double *b0 = Bp + (int64_t)2 * i * kp, *b1 = b0 + kp;
            for (int j = 0; j < k; j++) {
                const double p0 = b0[2 * j], p1 = b0[2 * j + 1], z0 = zc[2 * j], z1 = zc[2 * j + 1];
                xr_dot_sub(ar, p0, z0);
                xr_dot_sub(ar, p1, z1);
                xr_dot_sub(ai, b1[2 * j], z0);
                xr_dot_sub(ai, b1[2 * j + 1], z1);
                den += hypot(p0, p1) * hypot(z0, z1);
            }
            const double rr = xr_round(ar), ri = xr_round(ai);
            r[2 * i + c * rstr] = rr, r[2 * i + 1 + c * rstr] = ri;
            qi = zb_quot(rr, ri, den);
        }
        zb_block_max(red, qi, nrm + (size_t)c * RES_NORM_WORDS);
    }
}

// complex rows of A^H: one thread per complex row i, the columns of the block BORDER_RT at a time as k_border_residual_nt takes them.
// r = p - A^H y - conj(C) w through the real rows 2i, 2i+1 of the transposed real-equivalent matrix (tptr / trow / tmap): row 2i holds
// the pairs (Re a_ji, Im a_ji) in the rows 2j, 2j+1, adjacent because the rows of a column come out ascending.  Cp: the packed
// real-equivalent form of conj(C).  Within a column the additions come in the order p_i, the stored entries, j = 0 .. k - 1, whatever
// the tile holds.  A column whose bit in `mask` is clear: r = 0, no omega.
__global__ void __launch_bounds__(256) k_zborder_residual_nt(int32_t nc, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow, const int32_t *__restrict__ tmap,
                                                             const double *__restrict__ vals, int32_t k, int32_t kp, const double *__restrict__ Cp,
                                                             const double *__restrict__ W, const double *__restrict__ y, int64_t ystr, const double *__restrict__ p,
                                                             int64_t pstr, double *__restrict__ r, int64_t rstr, unsigned long long *nrm, int32_t ncols, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < nc;
    const int e0 = in ? tptr[2 * i] : 0, e1 = in ? tptr[2 * i + 1] : 0, e2 = in ? tptr[2 * i + 2] : 0;
    const double *c0p = Cp + (int64_t)2 * (in ? i : 0) * kp, *c1p = c0p + kp;
    for (int c0 = 0; c0 < ncols; c0 += BORDER_RT) { // (workgroup-uniform, as everything that depends on the mask alone)
        const int nt = ncols - c0 < BORDER_RT ? ncols - c0 : BORDER_RT;
        const uint32_t tm = (mask >> c0) & ((1u << nt) - 1u);
        if (in)
            for (int t = 0; t < nt; t++)
                if (!((tm >> t) & 1u)) r[2 * i + (int64_t)(c0 + t) * rstr] = 0.0, r[2 * i + 1 + (int64_t)(c0 + t) * rstr] = 0.0;
        if (!tm) continue;
        double qi[BORDER_RT] = {0.0, 0.0, 0.0, 0.0};
        if (in) {
            XrSum ar[BORDER_RT], ai[BORDER_RT];
            double den[BORDER_RT];
#pragma unroll
            for (int t = 0; t < BORDER_RT; t++) {
                const bool on = ((tm >> t) & 1u) != 0;
                const double pr = on ? p[2 * i + (int64_t)(c0 + t) * pstr] : 0.0, pi = on ? p[2 * i + 1 + (int64_t)(c0 + t) * pstr] : 0.0;
                ar[t].s = pr, ar[t].c = 0.0, ar[t].cc = 0.0, ai[t].s = pi, ai[t].c = 0.0, ai[t].cc = 0.0, den[t] = hypot(pr, pi);
            }
            for (int e = e0; e + 1 < e1; e += 2) { // row 2i
                const double a0 = vals[tmap[e]], a1 = vals[tmap[e + 1]], am = hypot(a0, a1);
                const double *y0 = y + trow[e], *y1 = y + trow[e + 1];
#pragma unroll
                for (int t = 0; t < BORDER_RT; t++)
                    if ((tm >> t) & 1u) {
                        const double v0 = y0[(int64_t)(c0 + t) * ystr], v1 = y1[(int64_t)(c0 + t) * ystr];
                        xr_dot_sub(ar[t], a0, v0);
                        xr_dot_sub(ar[t], a1, v1);
                        den[t] += am * hypot(v0, v1);
                    }
            }
            for (int e = e1; e < e2; e++) { // row 2i+1
                const double a = vals[tmap[e]];
                const double *yj = y + trow[e];
#pragma unroll
                for (int t = 0; t < BORDER_RT; t++)
                    if ((tm >> t) & 1u) xr_dot_sub(ai[t], a, yj[(int64_t)(c0 + t) * ystr]);
            }
            for (int j = 0; j < k; j++) {
                const double p0 = c0p[2 * j], p1 = c0p[2 * j + 1], q0 = c1p[2 * j], q1 = c1p[2 * j + 1], pm = hypot(p0, p1);
                const double *wj = W + (int64_t)c0 * kp + 2 * j;
#pragma unroll
                for (int t = 0; t < BORDER_RT; t++)
                    if ((tm >> t) & 1u) {
                        const double w0 = wj[(int64_t)t * kp], w1 = wj[(int64_t)t * kp + 1];
                        xr_dot_sub(ar[t], p0, w0);
                        xr_dot_sub(ar[t], p1, w1);
                        xr_dot_sub(ai[t], q0, w0);
                        xr_dot_sub(ai[t], q1, w1);
                        den[t] += pm * hypot(w0, w1);
                    }
            }
#pragma unroll
            for (int t = 0; t < BORDER_RT; t++)
                if ((tm >> t) & 1u) {
                    const double rr = xr_round(ar[t]), ri = xr_round(ai[t]);
                    r[2 * i + (int64_t)(c0 + t) * rstr] = rr, r[2 * i + 1 + (int64_t)(c0 + t) * rstr] = ri;
                    qi[t] = zb_quot(rr, ri, den[t]);
                }
        }
        for (int t = 0; t < nt; t++) // (workgroup-uniform)
            if ((tm >> t) & 1u) zb_block_max(red, qi[t], nrm + (size_t)(c0 + t) * RES_NORM_WORDS);
    }
}

// border rows, first half, as k_border_rows_part: grid (chunks of BORDER_CHUNK REAL rows, columns).  Thread (j, q) of a tile of sixteen
// packed columns takes the chunk's COMPLEX rows q, q + 16, ...: both real rows of each go into the unrounded triple of -C^T x (packed
// column j: a real or an imaginary part of a border row), and |c| |x| on moduli into the fourth word -- the same number in the two
// packed columns of a border row.
__global__ void __launch_bounds__(256) k_zborder_rows_part(int32_t n, int32_t kp, const double *__restrict__ Cp, const double *__restrict__ x, int64_t xstr,
                                                           uint32_t mask, double *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sh[BORDER_PART][16][17];
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * BORDER_CHUNK;
    const int64_t i1 = i0 + BORDER_CHUNK < n ? i0 + BORDER_CHUNK : n; // (both even)
    const double *xc = x + c * xstr;
    for (int jt = 0; jt < kp; jt += 16) {
        XrSum acc = {0.0, 0.0, 0.0};
        double den = 0.0;
        for (int64_t i = i0 + 2 * q; i + 1 < i1; i += 32) {
            const double a0 = Cp[i * kp + jt + j], a1 = Cp[(i + 1) * kp + jt + j], x0 = xc[i], x1 = xc[i + 1];
            xr_dot_sub(acc, a0, x0);
            xr_dot_sub(acc, a1, x1);
            den += hypot(a0, a1) * hypot(x0, x1);
        }
        __syncthreads(); // (the tile before has been written out)
        sh[0][q][j] = acc.s, sh[1][q][j] = acc.c, sh[2][q][j] = acc.cc, sh[3][q][j] = den;
        __syncthreads();
        for (int st = 8; st > 0; st >>= 1) {
            if (q < st) {
                XrSum m = {sh[0][q][j], sh[1][q][j], sh[2][q][j]};
                xr_merge(m, sh[0][q + st][j], sh[1][q + st][j], sh[2][q + st][j]);
                sh[0][q][j] = m.s, sh[1][q][j] = m.c, sh[2][q][j] = m.cc, sh[3][q][j] += sh[3][q + st][j];
            }
            __syncthreads();
        }
        if (q == 0) {
            double *dst = part + (((int64_t)blockIdx.x * BORDER_COLS + c) * kp + jt + j) * BORDER_PART;
            dst[0] = sh[0][0][j], dst[1] = sh[1][0][j], dst[2] = sh[2][0][j], dst[3] = sh[3][0][j];
        }
    }
}

// border rows, second half: one wavefront per column c (grid m), lane j = REAL row j of the border (complex row j / 2, its real part in
// the even lane).  The chunks' triples merged in chunk order onto g_j, then -D z with D complex (column-major interleaved, kp doubles
// per column): rg = g - C^T x - D z rounded once per part; den = |C|^T|x| + |D||z| + |g| and omega[c] = max |rg_j| / den_j over the
// complex rows, all on moduli, in index order.  A column whose bit in `mask` is clear: rg = 0, omega untouched.
__global__ void __launch_bounds__(64) k_zborder_rows(int32_t k, int32_t kp, int32_t nchunk, const double *__restrict__ D, const double *__restrict__ g,
                                                     const double *__restrict__ part, const double *__restrict__ z, double *__restrict__ rg,
                                                     double *__restrict__ omega, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double rs[BORDER_MAX], qs[ZBORDER_MAX];
    const int c = blockIdx.x, j = threadIdx.x, jc = j >> 1, h = j & 1;
    const int64_t col = (int64_t)c * kp;
    if (!((mask >> c) & 1u)) {
        if (j < kp) rg[col + j] = 0.0;
        return;
    }
    double den = 0.0, s = 0.0;
    if (j < 2 * k) {
        XrSum acc = {g[col + j], 0.0, 0.0};
        den = hypot(g[col + 2 * jc], g[col + 2 * jc + 1]);
        for (int ch = 0; ch < nchunk; ch++) {
            const double *p = part + (((int64_t)ch * BORDER_COLS + c) * kp + j) * BORDER_PART;
            xr_merge(acc, p[0], p[1], p[2]);
            den += p[3];
        }
        for (int i = 0; i < k; i++) {
            const double dr = D[2 * jc + (int64_t)i * kp], di = D[2 * jc + 1 + (int64_t)i * kp], z0 = z[col + 2 * i], z1 = z[col + 2 * i + 1];
            xr_dot_sub(acc, h ? di : dr, z0);
            xr_dot_sub(acc, h ? dr : -di, z1);
            den += hypot(dr, di) * hypot(z0, z1);
        }
        s = xr_round(acc);
        rg[col + j] = s;
    } else if (j < kp) {
        rg[col + j] = 0.0;
    }
    rs[j] = s;
    __syncthreads();
    if (h == 0 && jc < k) qs[jc] = zb_quot(rs[j], rs[j + 1], den);
    __syncthreads();
    if (j == 0) {
        double mx = 0.0;
        for (int i = 0; i < k; i++) mx = qs[i] > mx ? qs[i] : mx;
        omega[c] = mx;
    }
}

} // namespace hipmf
