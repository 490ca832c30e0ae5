// kernels_border.hpp -- bordered systems on the kept factor (solver_hipmf_set_border / solver_hipmf_solve_bordered; Solver::set_border,
// Solver::solve_bordered in numeric.cpp):
//     [ A   B ] [x]   [f]      A the factorised n x n matrix, B, C n x k dense, D k x k dense, k <= BORDER_MAX
//     [ C^T D ] [z] = [g]
// by block elimination with W = A^{-1} B and the Schur complement S = D - C^T W kept beside the factor, refined on the WHOLE system.
//
// Layouts.  The handle keeps B, C and W "packed": row-major n x kp, kp = k rounded up to a multiple of 16, the padding columns zero
// (k_border_pack) -- a quarter-wave then reads sixteen border entries of one row as one 128-byte segment in both products.  Vectors of
// the first n rows are column-major blocks of at most BORDER_COLS = 16 columns, as the blocked pass pair takes them; everything of
// order k (g, z, t, the Gram products, S and its LU) is column-major with leading dimension kp, padding rows zero.
//
// k_border_gram    G = P^T Y (k x n times n x m, m <= 16) on v_mfma_f64_16x16x4_f64 with the n rows as the contraction.  One wavefront
//                  per chunk of BORDER_CHUNK rows and per tile of 16 border rows; BORDER_CHUNK is a compile-time constant, so where a
//                  partial sum is cut depends on n alone, never on the grid or the device.  Rows past n are zeros.  The partial tiles
//                  go to a scratch array ...
// k_border_reduce  ... and are summed in chunk order: sixteen strided partial sums per entry, combined by a fixed tree (the scheme of
//                  k_kryb_dots / k_kryb_reduce).  No floating-point atomics anywhere in this file: two calls give the same bits.
// k_border_lu      S = D - G in LDS (64 x 64 doubles = 32 KB), one workgroup, partial pivoting; LU, pivots and a record: min and max
//                  |u_ii|, det S as mantissa and base-10 exponent (the form of Solver::determinant), a flag for an exactly zero pivot.
// k_border_small_solve  t = g - G, dz = S^{-1} t from the stored LU, one wavefront per column; optionally z <- z + dz, the old z kept.
// k_border_apply   OUT = Y - P Z (n x k times k x m) on the MFMA with k as the contraction, padded to a multiple of 4; one wavefront per
//                  tile of 16 rows.  The tile is formed transposed (Z^T P^T): the result then has sixteen consecutive ROWS of one column
//                  in sixteen consecutive lanes, and Y / OUT move in 128-byte segments.  With SAVE the result is a correction:
//                  SAVE = OUT, OUT = OUT + (Y - P Z).
// k_border_residual_n, k_border_rows_part, k_border_rows  the residual of all n + k rows, accumulated beyond twice the working
//                  precision and rounded once, with the denominators and the omegas of solve()'s stopping rule (see there).
// The transposed form (solver_hipmf_solve_bordered_transpose; Solver::solve_bordered_transpose): [A^T C; B^T D^T] [y; w] = [p; q] with
// V = A^{-T} C and the SAME S (S^T = D^T - B^T V), so the LU above serves.  The Gram, apply and border-row kernels are reused with the
// operands swapped (B for C, V for W, the packed D^T for D); what is new:
// k_border_unpack  column-major columns back out of a packed array (the right-hand sides of V = A^{-T} C)
// k_border_small_solve_t  t = q - G, dw = S^{-T} t from the same LU: U^T forward, L^T backward, the row exchanges undone in reverse
// k_border_residual_nt  the n rows of M^T through the rows of A^T (tptr / trow / tmap of the transposed solves), the block's columns
//                  BORDER_RT at a time: a thread reads its row of A^T and of C once per tile of columns instead of once per column
// Columns whose bit in `mask` is clear are finished: a residual column is zeros (it rides along through the next pass pair), a correction
// leaves x and z of such a column alone.
// Traffic per launch, in bytes: gram 8 n (kp + m); apply 8 n (kp + 2 m), with SAVE 8 n (kp + 4 m); the residual of the n rows one pass
// over A plus 8 n (kp + 3 m), that of the border rows 8 n (kp + m).
#pragma once
#include "kernels_common.hpp"
#include "kernels_vector.hpp"
#include "kernels_refine_extra.hpp"

namespace hipmf {

constexpr int BORDER_MAX = 64;     // border rows / columns at most (HIPMF_BORDER_MAX): S and its LU live in the LDS of one workgroup
constexpr int BORDER_COLS = 16;    // right-hand sides per block (one MFMA tile)
constexpr int BORDER_CHUNK = 1024; // rows per partial sum of k_border_gram
constexpr int BORDER_REC = 8;      // doubles of k_border_lu's record: min |u_ii|, max |u_ii|, mantissa, exponent, zero-pivot flag

// dst[i kp + j0 + j] = src[i + j ld], j < ncols: columns [j0, j0 + ncols) of the packed form (the other columns are left alone)
__global__ void __launch_bounds__(256) k_border_pack(int32_t n, int32_t ncols, int32_t kp, int32_t j0, const double *__restrict__ src, int64_t ld,
                                                     double *__restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = e / ncols;
    const int j = (int)(e - i * ncols);
    if (i < n) dst[i * kp + j0 + j] = src[i + (int64_t)j * ld];
}

// grid (chunks, kp / 16), one wavefront: part[chunk kp 16 + c kp + j] holds the chunk's share of G[c kp + j] = (P^T Y)(j, c)
__global__ void __launch_bounds__(64) k_border_gram(int32_t n, int32_t kp, const double *__restrict__ P, const double *__restrict__ Y, int64_t ystr, int32_t m,
                                                    double *__restrict__ part) {
    const int lane = threadIdx.x & 63, o = lane & 15, kk = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * BORDER_CHUNK;
    const int jt = blockIdx.y * 16;
    const double *Pj = P + jt + o;
    const double *Yc = Y + (int64_t)(o < m ? o : 0) * ystr;
    f64x4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int ib = 0; ib < BORDER_CHUNK; ib += 32) { // (wave-uniform trip count: every lane takes part in every MFMA)
        double a[8], b[8];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int64_t i = i0 + ib + 4 * s + kk;
            const bool in = i < n;
            a[s] = in ? Pj[i * kp] : 0.0;
            b[s] = (in && o < m) ? Yc[i] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 8; s++) acc[s & 1] = mfma_f64_16x16x4(a[s], b[s], acc[s & 1]);
    }
    const int64_t base = (int64_t)blockIdx.x * kp * 16 + (int64_t)o * kp + jt;
#pragma unroll
    for (int g = 0; g < 4; g++) part[base + kk + 4 * g] = acc[0][g] + acc[1][g];
}

// grid kp: out[e] = sum over the chunks of part[chunk kp 16 + e] for sixteen consecutive e per workgroup; thread (e, q) sums the
// chunks q, q + 16, ... in order, the sixteen sums of an entry are combined by a fixed tree
__global__ void __launch_bounds__(256) k_border_reduce(int32_t nchunk, int32_t kp, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double red[16][17];
    const int o = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int64_t e = (int64_t)blockIdx.x * 16 + o, tile = (int64_t)kp * 16;
    double s = 0.0;
    for (int ch = q; ch < nchunk; ch += 16) s += part[(int64_t)ch * tile + e];
    red[q][o] = s;
    __syncthreads();
    for (int st = 8; st > 0; st >>= 1) {
        if (q < st) red[q][o] += red[q + st][o];
        __syncthreads();
    }
    if (q == 0) out[e] = red[0][o];
}

// One workgroup: LU of S = D - G with partial pivoting (D, G, LU: column-major, leading dimension kp).  piv[j]: the row exchanged with
// row j at step j.  rec: see BORDER_REC; an exactly zero pivot sets rec[4] = 1 and ends the elimination (LU is then not to be used).
__global__ void __launch_bounds__(256) k_border_lu(int32_t k, int32_t kp, const double *__restrict__ D, const double *__restrict__ G, double *__restrict__ LU,
                                                   int32_t *__restrict__ piv, double *__restrict__ rec) {
    __shared__ double s[BORDER_MAX * BORDER_MAX]; // column-major, leading dimension k
    __shared__ int prow;
    __shared__ int bad;
    const int tid = threadIdx.x;
    for (int e = tid; e < k * k; e += 256) {
        const int i = e % k, j = e / k;
        s[e] = D[i + (int64_t)j * kp] - G[i + (int64_t)j * kp];
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    double mant = 1.0, expo = 0.0, umin = INFINITY, umax = 0.0; // (thread 0's)
    for (int j = 0; j < k; j++) {
        if (tid == 0) {
            int best = j;
            double vb = fabs(s[j + j * k]);
            for (int i = j + 1; i < k; i++) { // (the first of equal candidates; a NaN is never chosen over a number)
                const double v = fabs(s[i + j * k]);
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
                const double t = s[j + c * k];
                s[j + c * k] = s[r + c * k], s[r + c * k] = t;
            }
        __syncthreads();
        const double d = s[j + j * k];
        if (tid == 0) {
            if (r != j) mant = -mant;
            mant *= d;
            while (fabs(mant) >= 10.0 && fabs(mant) <= 1.79769313486231570815e308) mant /= 10.0, expo += 1.0;
            while (fabs(mant) < 1.0 && mant != 0.0) mant *= 10.0, expo -= 1.0;
            const double a = fabs(d);
            umin = a < umin ? a : umin, umax = a > umax ? a : umax;
        }
        __syncthreads(); // (the pivot has been read by everyone before the column below it is scaled)
        for (int i = j + 1 + tid; i < k; i += 256) s[i + j * k] = s[i + j * k] / d;
        __syncthreads();
        const int rem = k - j - 1;
        for (int e = tid; e < rem * rem; e += 256) {
            const int i = j + 1 + e % rem, c = j + 1 + e / rem;
            s[i + c * k] = fma(-s[i + j * k], s[j + c * k], s[i + c * k]);
        }
        __syncthreads();
    }
    for (int e = tid; e < k * k; e += 256) LU[e % k + (int64_t)(e / k) * kp] = s[e];
    if (tid == 0) {
        rec[0] = umin, rec[1] = umax, rec[2] = bad ? 0.0 : mant, rec[3] = bad ? 0.0 : expo, rec[4] = bad ? 1.0 : 0.0;
        for (int j = 5; j < BORDER_REC; j++) rec[j] = 0.0;
    }
}

// One wavefront per column c (grid m): dz = S^{-1} (g - G) from the LU of k_border_lu, entries k .. kp - 1 of dz zero.
// zs != nullptr: zs = z, z = z + dz (a correction); else z = dz.  Columns whose bit in `mask` is clear are left alone.
__global__ void __launch_bounds__(64) k_border_small_solve(int32_t k, int32_t kp, const double *__restrict__ LU, const int32_t *__restrict__ piv,
                                                           const double *__restrict__ g, const double *__restrict__ G, double *__restrict__ dz,
                                                           double *__restrict__ z, double *__restrict__ zs, uint32_t mask) {
    __shared__ double t[BORDER_MAX];
    const int c = blockIdx.x, j = threadIdx.x;
    if (!((mask >> c) & 1u)) return;
    const int64_t col = (int64_t)c * kp;
    if (j < k) t[j] = g[col + j] - G[col + j];
    __syncthreads();
    if (j == 0)
        for (int q = 0; q < k; q++) {
            const int r = piv[q];
            if (r != q) {
                const double v = t[q];
                t[q] = t[r], t[r] = v;
            }
        }
    __syncthreads();
    for (int q = 0; q < k; q++) { // L y = P t, unit diagonal
        const double tq = t[q];
        __syncthreads();
        if (j > q && j < k) t[j] = fma(-LU[j + (int64_t)q * kp], tq, t[j]);
        __syncthreads();
    }
    for (int q = k - 1; q >= 0; q--) { // U dz = y
        if (j == q) t[q] = t[q] / LU[q + (int64_t)q * kp];
        __syncthreads();
        const double tq = t[q];
        if (j < q) t[j] = fma(-LU[j + (int64_t)q * kp], tq, t[j]);
        __syncthreads();
    }
    if (j < kp) {
        const double v = j < k ? t[j] : 0.0;
        dz[col + j] = v;
        if (zs) {
            const double old = z[col + j];
            zs[col + j] = old, z[col + j] = old + v;
        } else {
            z[col + j] = v;
        }
    }
}

// grid ceil(n / 64), four wavefronts, one tile of 16 rows each.  Z: column-major kp x m.  See the head of the file.
// v = Y - P Z; save == nullptr: OUT = v (zeros in a column the mask leaves out); else save = OUT, OUT = OUT + v in the columns of the mask.
// Y and OUT may be the same array.
__global__ void __launch_bounds__(256) k_border_apply(int32_t n, int32_t k, int32_t kp, const double *__restrict__ P, const double *__restrict__ Z, int32_t m,
                                                      uint32_t mask, const double *Y, int64_t ystr, double *OUT, int64_t ostr, double *__restrict__ save, int64_t sstr) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, o = lane & 15, kk = lane >> 4;
    const int64_t i = (int64_t)blockIdx.x * 64 + wv * 16 + o;
    const bool in = i < n;
    const double *Pi = P + (in ? i : 0) * kp;
    const double *Zo = Z + (int64_t)(o < m ? o : 0) * kp;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < (k + 3) / 4; s++) { // (workgroup-uniform trip count)
        const double a = o < m ? Zo[4 * s + kk] : 0.0, b = in ? Pi[4 * s + kk] : 0.0;
        acc = mfma_f64_16x16x4(a, b, acc); // tile^T: rows = right-hand sides, columns = the tile's rows
    }
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int c = kk + 4 * g;
        if (c >= m || !in) continue;
        const bool on = ((mask >> c) & 1u) != 0;
        if (save) {
            if (!on) continue;
            const double v = Y[i + c * ystr] - acc[g], old = OUT[i + c * ostr];
            save[i + c * sstr] = old, OUT[i + c * ostr] = old + v;
        } else {
            OUT[i + c * ostr] = on ? Y[i + c * ystr] - acc[g] : 0.0;
        }
    }
}

// ---- the residual of the bordered system, every row accumulated beyond twice the working precision and rounded once ----
// The stop test omega <= eps sits at the level of the rounding errors of a residual evaluated in working precision: such a residual's
// noise, sqrt(p) eps den_i / 2 in a row of p entries, decides from column to column whether a solution that IS backward stable is seen
// as converged, and -- carried through the correction -- leaves a forward error anywhere between eps and cond eps.  So the three
// kernels below use the error-free sums of kernels_refine_extra.hpp (TwoProduct by FMA, TwoSum, the compensation's errors in a third
// word): the residual is exact up to its one rounding, omega is what it says, and the refined (x, z) is the exact solution rounded.
// The products of the elimination itself (k_border_gram, k_border_apply) need no such care: they only shape the approximate inverse.

// rows of A: one thread per row i, the columns of the block in turn.  r = f - A x - B z, den = |A||x| + |B||z| + |f|, and per column
// max_i |r_i| / den_i into word 1 of the slots of kernels_vector.hpp (atomicMax on the bits of non-negative doubles: an exact maximum,
// whatever the order).  A column whose bit in `mask` is clear: r = 0, no omega.
__global__ void __launch_bounds__(256) k_border_residual_n(int32_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const double *__restrict__ vals,
                                                           const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx, const int32_t *__restrict__ arow,
                                                           int32_t k, int32_t kp, const double *__restrict__ Bp, const double *__restrict__ Z,
                                                           const double *__restrict__ x, int64_t xstr, const double *__restrict__ f, int64_t fstr,
                                                           double *__restrict__ r, int64_t rstr, unsigned long long *nrm, int32_t ncols, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int e0 = in ? rp[i] : 0, e1 = in ? rp[i + 1] : 0;
    const int q0 = (in && tptr) ? tptr[i] : 0, q1 = (in && tptr) ? tptr[i + 1] : 0;
    for (int c = 0; c < ncols; c++) { // (workgroup-uniform)
        if (!((mask >> c) & 1u)) {
            if (in) r[i + c * rstr] = 0.0;
            continue;
        }
        const double *xc = x + c * xstr, *zc = Z + (int64_t)c * kp;
        double qi = 0.0;
        if (in) {
            const double fi = f[i + c * fstr];
            XrSum acc = {fi, 0.0, 0.0};
            double den = fabs(fi);
            for (int e = e0; e < e1; e++) {
                const double a = vals[e], xv = xc[ci[e]];
                xr_dot_sub(acc, a, xv);
                den += fabs(a * xv);
            }
            for (int q = q0; q < q1; q++) { // the mirrored entries of symmetric-lower storage
                const double a = vals[tidx[q]], xv = xc[arow[tidx[q]]];
                xr_dot_sub(acc, a, xv);
                den += fabs(a * xv);
            }
            const double *bi = Bp + (int64_t)i * kp;
            for (int j = 0; j < k; j++) {
                const double a = bi[j], zv = zc[j];
                xr_dot_sub(acc, a, zv);
                den += fabs(a * zv);
            }
            const double ri = xr_round(acc), ai = fabs(ri);
            r[i + c * rstr] = ri;
            qi = den > 0.0 ? ai / den : (ai > 0.0 ? 1.0 : 0.0);
            qi = qi > 0.0 ? qi : 0.0; // (a NaN never wins the maximum, as in spmv_block)
        }
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
            atomicMax(nrm + (size_t)c * RES_NORM_WORDS + (size_t)(blockIdx.x & (RES_SLOTS - 1)) * RES_SLOT_WORDS + 1, (unsigned long long)__double_as_longlong(mx));
        }
    }
}

// border rows, first half: grid (chunks, columns).  Per border row j the chunk's share of -C^T x as an unrounded (sum, compensation,
// compensation's errors) triple and its share of |C|^T |x|: part[((chunk BORDER_COLS + c) kp + j) 4 ...].  Thread (j, q) of a tile of
// sixteen border rows takes the chunk's rows q, q + 16, ...; the sixteen triples of a border row are merged by a fixed tree.
constexpr int BORDER_PART = 4; // doubles per partial sum of k_border_rows_part
__global__ void __launch_bounds__(256) k_border_rows_part(int32_t n, int32_t kp, const double *__restrict__ Cp, const double *__restrict__ x, int64_t xstr,
                                                          uint32_t mask, double *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sh[BORDER_PART][16][17];
    const int c = blockIdx.y;
    if (!((mask >> c) & 1u)) return;
    const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * BORDER_CHUNK;
    const int64_t i1 = i0 + BORDER_CHUNK < n ? i0 + BORDER_CHUNK : n;
    const double *xc = x + c * xstr;
    for (int jt = 0; jt < kp; jt += 16) {
        XrSum acc = {0.0, 0.0, 0.0};
        double den = 0.0;
        for (int64_t i = i0 + q; i < i1; i += 16) {
            const double a = Cp[i * kp + jt + j], xv = xc[i];
            xr_dot_sub(acc, a, xv);
            den += fabs(a * xv);
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

// border rows, second half: one wavefront per column c (grid m), lane j = border row j.  The chunks' triples merged in chunk order onto
// g_j, then -D z: rg = g - C^T x - D z rounded once, den = |C|^T|x| + |D||z| + |g|, omega[c] = max_j |rg_j| / den_j in index order
// (0 / 0 counts 0, nonzero / 0 counts 1, as in spmv_block).  A column whose bit in `mask` is clear: rg = 0, omega untouched.
__global__ void __launch_bounds__(64) k_border_rows(int32_t k, int32_t kp, int32_t nchunk, const double *__restrict__ D, const double *__restrict__ g,
                                                    const double *__restrict__ part, const double *__restrict__ z, double *__restrict__ rg,
                                                    double *__restrict__ omega, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double qs[BORDER_MAX];
    const int c = blockIdx.x, j = threadIdx.x;
    const int64_t col = (int64_t)c * kp;
    if (!((mask >> c) & 1u)) {
        if (j < kp) rg[col + j] = 0.0;
        return;
    }
    double qj = 0.0;
    if (j < k) {
        XrSum acc = {g[col + j], 0.0, 0.0};
        double den = fabs(g[col + j]);
        for (int ch = 0; ch < nchunk; ch++) {
            const double *p = part + (((int64_t)ch * BORDER_COLS + c) * kp + j) * BORDER_PART;
            xr_merge(acc, p[0], p[1], p[2]);
            den += p[3];
        }
        for (int i = 0; i < k; i++) {
            const double d = D[j + (int64_t)i * kp], zi = z[col + i];
            xr_dot_sub(acc, d, zi);
            den += fabs(d * zi);
        }
        const double s = xr_round(acc), ai = fabs(s);
        rg[col + j] = s;
        qj = den > 0.0 ? ai / den : (ai > 0.0 ? 1.0 : 0.0);
    } else if (j < kp) {
        rg[col + j] = 0.0;
    }
    qs[j] = qj > 0.0 ? qj : 0.0; // (a NaN never wins the maximum)
    __syncthreads();
    if (j == 0) {
        double mx = 0.0;
        for (int i = 0; i < k; i++) mx = qs[i] > mx ? qs[i] : mx;
        omega[c] = mx;
    }
}

// ---- the transposed form ----

// dst[i + j ld] = src[i kp + j0 + j], j < ncols: k_border_pack backwards
__global__ void __launch_bounds__(256) k_border_unpack(int32_t n, int32_t ncols, int32_t kp, int32_t j0, const double *__restrict__ src, double *__restrict__ dst,
                                                       int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = e / ncols;
    const int j = (int)(e - i * ncols);
    if (i < n) dst[i + (int64_t)j * ld] = src[i * kp + j0 + j];
}

// One wavefront per column c (grid m): dw = S^{-T} (q - G) from the LU of k_border_lu (P S = L U, so S^T = U^T L^T P): U^T forward, L^T
// backward with its unit diagonal, then the row exchanges undone in reverse order.  zs, mask and the zero padding: k_border_small_solve.
__global__ void __launch_bounds__(64) k_border_small_solve_t(int32_t k, int32_t kp, const double *__restrict__ LU, const int32_t *__restrict__ piv,
                                                             const double *__restrict__ g, const double *__restrict__ G, double *__restrict__ dz,
                                                             double *__restrict__ z, double *__restrict__ zs, uint32_t mask) {
    __shared__ double t[BORDER_MAX];
    const int c = blockIdx.x, j = threadIdx.x;
    if (!((mask >> c) & 1u)) return;
    const int64_t col = (int64_t)c * kp;
    if (j < k) t[j] = g[col + j] - G[col + j];
    __syncthreads();
    for (int q = 0; q < k; q++) { // U^T a = t: row q of U is column q of U^T
        if (j == q) t[q] = t[q] / LU[q + (int64_t)q * kp];
        __syncthreads();
        const double tq = t[q];
        if (j > q && j < k) t[j] = fma(-LU[q + (int64_t)j * kp], tq, t[j]);
        __syncthreads();
    }
    for (int q = k - 1; q > 0; q--) { // L^T b = a, unit diagonal
        const double tq = t[q];
        __syncthreads();
        if (j < q) t[j] = fma(-LU[q + (int64_t)j * kp], tq, t[j]);
        __syncthreads();
    }
    if (j == 0)
        for (int q = k - 1; q >= 0; q--) {
            const int r = piv[q];
            if (r != q) {
                const double v = t[q];
                t[q] = t[r], t[r] = v;
            }
        }
    __syncthreads();
    if (j < kp) {
        const double v = j < k ? t[j] : 0.0;
        dz[col + j] = v;
        if (zs) {
            const double old = z[col + j];
            zs[col + j] = old, z[col + j] = old + v;
        } else {
            z[col + j] = v;
        }
    }
}

// rows of A^T: one thread per row i, the columns of the block BORDER_RT at a time.  r = p - A^T y - C w, den = |A^T||y| + |C||w| + |p|,
// omega as k_border_residual_n.  Row i of A^T is column i of A: entries vals[tmap[e]] in the rows trow[e], e in [tptr[i], tptr[i + 1]).
// A tile of columns shares every load of the row -- value, map and row index of a stored entry, the k entries of the border row -- and
// keeps one (sum, denominator) pair per column; within a column the additions come in the order p_i, the stored entries, j = 0 .. k - 1,
// whatever the tile holds: the tiling changes no bit.  A column whose bit in `mask` is clear: r = 0, no omega.
constexpr int BORDER_RT = 4;
__global__ void __launch_bounds__(256) k_border_residual_nt(int32_t n, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow, const int32_t *__restrict__ tmap,
                                                            const double *__restrict__ vals, int32_t k, int32_t kp, const double *__restrict__ Cp,
                                                            const double *__restrict__ W, const double *__restrict__ y, int64_t ystr, const double *__restrict__ p,
                                                            int64_t pstr, double *__restrict__ r, int64_t rstr, unsigned long long *nrm, int32_t ncols, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double red[BORDER_RT][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int e0 = in ? tptr[i] : 0, e1 = in ? tptr[i + 1] : 0;
    const double *ci = Cp + (int64_t)(in ? i : 0) * kp;
    for (int c0 = 0; c0 < ncols; c0 += BORDER_RT) { // (workgroup-uniform, as everything that depends on the mask alone)
        const int nt = ncols - c0 < BORDER_RT ? ncols - c0 : BORDER_RT;
        const uint32_t tm = (mask >> c0) & ((1u << nt) - 1u);
        if (in)
            for (int t = 0; t < nt; t++)
                if (!((tm >> t) & 1u)) r[i + (int64_t)(c0 + t) * rstr] = 0.0;
        if (!tm) continue;
        double qi[BORDER_RT] = {0.0, 0.0, 0.0, 0.0};
        if (in) {
            XrSum acc[BORDER_RT];
            double den[BORDER_RT];
#pragma unroll
            for (int t = 0; t < BORDER_RT; t++) {
                const double pi = ((tm >> t) & 1u) ? p[i + (int64_t)(c0 + t) * pstr] : 0.0;
                acc[t].s = pi, acc[t].c = 0.0, acc[t].cc = 0.0, den[t] = fabs(pi);
            }
            for (int e = e0; e < e1; e++) {
                const double a = vals[tmap[e]];
                const double *yj = y + trow[e];
#pragma unroll
                for (int t = 0; t < BORDER_RT; t++)
                    if ((tm >> t) & 1u) {
                        const double yv = yj[(int64_t)(c0 + t) * ystr];
                        xr_dot_sub(acc[t], a, yv);
                        den[t] += fabs(a * yv);
                    }
            }
            for (int j = 0; j < k; j++) {
                const double a = ci[j];
                const double *wj = W + (int64_t)c0 * kp + j;
#pragma unroll
                for (int t = 0; t < BORDER_RT; t++)
                    if ((tm >> t) & 1u) {
                        const double wv = wj[(int64_t)t * kp];
                        xr_dot_sub(acc[t], a, wv);
                        den[t] += fabs(a * wv);
                    }
            }
#pragma unroll
            for (int t = 0; t < BORDER_RT; t++)
                if ((tm >> t) & 1u) {
                    const double ri = xr_round(acc[t]), ai = fabs(ri);
                    r[i + (int64_t)(c0 + t) * rstr] = ri;
                    const double q = den[t] > 0.0 ? ai / den[t] : (ai > 0.0 ? 1.0 : 0.0);
                    qi[t] = q > 0.0 ? q : 0.0; // (a NaN never wins the maximum, as in spmv_block)
                }
        }
#pragma unroll
        for (int t = 0; t < BORDER_RT; t++)
            for (int off = 32; off > 0; off >>= 1) {
                const double other = __shfl_xor(qi[t], off);
                qi[t] = other > qi[t] ? other : qi[t];
            }
        __syncthreads(); // (the maxima of the tile before have been read)
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int t = 0; t < BORDER_RT; t++) red[t][threadIdx.x >> 6] = qi[t];
        }
        __syncthreads();
        if (threadIdx.x < BORDER_RT && ((tm >> threadIdx.x) & 1u)) {
            const int t = threadIdx.x;
            double mx = red[t][0];
            for (int w = 1; w < 4; w++) mx = red[t][w] > mx ? red[t][w] : mx;
            atomicMax(nrm + (size_t)(c0 + t) * RES_NORM_WORDS + (size_t)(blockIdx.x & (RES_SLOTS - 1)) * RES_SLOT_WORDS + 1, (unsigned long long)__double_as_longlong(mx));
        }
    }
}

} // namespace hipmf
