// kernels_eigs.hpp -- eigenpairs nearest a shift on the kept factor (solver_hipmf_eigs_near_shift; Solver::eigs_near_shift in numeric.cpp)
// and the inertia of the factor (solver_hipmf_get_inertia; Solver::inertia).  Thick-restart Lanczos on A^{-1} M in the M-inner product:
// the dots, the updates, the scaling and the SpMV of a step are those of kernels_krylov.hpp / kernels_vector.hpp; what is new is here.
//
// k_eig_rotate     DST(:, 0:k) = V(:, 0:m) Y, Y m x k column-major (leading dimension m), on v_mfma_f64_16x16x4_f64.  DST may be V itself
//                  (the restart) or the caller's X.  A wavefront owns 16 rows: it loads all m inputs of its rows into registers (one
//                  double per lane and K-step of 4, EIG_MMAX / 4 = 32 at most) BEFORE its first store, and no other wavefront reads or
//                  writes those rows -- that is what makes the in-place form safe.  The tile is formed transposed (Y^T V^T), as in
//                  k_border_apply: sixteen consecutive lanes then hold sixteen consecutive ROWS of one output column, so V and DST move in
//                  128-byte segments; every access is one 8-byte double, so odd column starts (multiples of an odd n) need no care.  Y
//                  comes through LDS sixteen output columns at a time, zero-padded to EIG_MMAX rows: the K loop of a tile runs over
//                  ceil(m / 4) steps in ascending order whatever the grid, the padding contributes exact zeros.  Bytes: (m + k) 8 n.
// k_eig_residuals  R = A X - M X diag(mu) for all columns in one launch, EIG_RT columns at a time (a thread reads its row of A and of M
//                  once per tile of columns, as k_border_residual_nt does): per workgroup and column max_i |r_i| and max_i |x_i| in
//                  slots of their own, combined by k_eig_max.  M's values on A's pattern; mvals == nullptr: M = I.
// k_eig_rownorm    per-workgroup max_i sum_j |a_ij| (the mirrored entries of symmetric-lower storage included): |A|_inf and |M|_inf.
// k_eig_max        out[c] = max over the slots of column c (a maximum does not depend on the order; the slots keep atomics out).
// k_eig_start      the start vector of sequence number seq: entry i = eig_hash(i, seq) mapped into (-1, 1).  No state, no rand().
// k_eig_absmax, k_eig_sign, k_eig_flip   the entry of largest modulus of every column (the FIRST on ties) is made positive.
// k_eig_inertia, k_eig_inertia_small, k_eig_inertia_sum   the inertia: signs of the pivots of the tiled fronts; per small front the
//                  signs of its pivots or, where its pivot search moved a row, the inertia of its pivot block multiplied out again;
//                  integer counts in per-workgroup slots, added by one workgroup.
// No floating-point atomics in this file.
#pragma once
#include "kernels_krylov.hpp"

namespace hipmf {

constexpr int EIG_MMAX = 128;   // basis vectors at most (ncv)
constexpr int EIG_NEV_MAX = 64; // eigenpairs per call at most
constexpr int EIG_RT = 4;       // columns per tile of k_eig_residuals
constexpr int EIG_INERTIA_WG = 64;

// The documented integer hash of (i, seq): two odd multipliers, then the finaliser "lowbias32" (xor-shift 16, times 0x7feb352d,
// xor-shift 15, times 0x846ca68b, xor-shift 16), all in 32-bit wrap-around arithmetic.  The value is (h + 0.5) / 2^31 - 1: 2^32
// equidistant numbers strictly inside (-1, 1), each exactly representable.
__host__ __device__ __forceinline__ double eig_hash(uint32_t i, uint32_t seq) {
    uint32_t h = i * 0x9e3779b1u + seq * 0x85ebca77u + 0x165667b1u;
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return ((double)h + 0.5) * (1.0 / 2147483648.0) - 1.0;
}

__global__ void __launch_bounds__(256) k_eig_start(int32_t n, uint32_t seq, double *__restrict__ v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = eig_hash((uint32_t)i, seq);
}

// grid ceil(n / 64), four wavefronts of 16 rows each.  See the head of the file.
__global__ void __launch_bounds__(256) k_eig_rotate(int32_t n, int32_t m, int32_t k, const double *V, const double *__restrict__ Y, double *DST, int64_t ldd) {
    __shared__ double Yt[EIG_MMAX * 16]; // Yt[r * 16 + c] = Y(r, c0 + c), zeros beyond m and k
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, o = lane & 15, kk = lane >> 4;
    const int64_t i = (int64_t)blockIdx.x * 64 + wv * 16 + o;
    const bool in = i < n;
    const int ms = (m + 3) / 4;
    double v[EIG_MMAX / 4];
#pragma unroll
    for (int s = 0; s < EIG_MMAX / 4; s++) { // every input of this wavefront's rows, before anything is stored
        const int j = 4 * s + kk;
        v[s] = (s < ms && in && j < m) ? V[i + (int64_t)j * n] : 0.0;
    }
    for (int c0 = 0; c0 < k; c0 += 16) { // (workgroup-uniform)
        __syncthreads();                 // (the tile before has been read)
        for (int e = threadIdx.x; e < EIG_MMAX * 16; e += 256) {
            const int r = e >> 4, c = e & 15;
            Yt[e] = (r < m && c0 + c < k) ? Y[r + (int64_t)(c0 + c) * m] : 0.0;
        }
        __syncthreads();
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < EIG_MMAX / 4; s++)
            if (s < ms) acc = mfma_f64_16x16x4(Yt[(4 * s + kk) * 16 + o], v[s], acc); // tile^T: rows = output columns, columns = the rows of V
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c = c0 + kk + 4 * g;
            if (in && c < k) DST[i + (int64_t)c * ldd] = acc[g];
        }
    }
}

// max over the workgroup of a non-negative v (a NaN never wins); the same value in every thread.  red: 4 doubles of LDS
__device__ __forceinline__ double eig_block_max(double v, double *red) {
    v = v > 0.0 ? v : 0.0;
    for (int off = 32; off > 0; off >>= 1) {
        const double other = __shfl_xor(v, off);
        v = other > v ? other : v;
    }
    __syncthreads(); // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double mx = red[0];
    for (int w = 1; w < 4; w++) mx = red[w] > mx ? red[w] : mx;
    return mx;
}

// one thread per row; part[c * gridDim.x + b] = max |r_i| of column c in workgroup b, part[(ncols + c) * gridDim.x + b] = max |x_i|.
// Within a column the additions of a row come in the order: stored entries of A, mirrored entries of A, then the same of -mu M (or
// -mu x_i), whatever the tile holds.
__global__ void __launch_bounds__(256) k_eig_residuals(int32_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const double *__restrict__ avals,
                                                       const double *__restrict__ mvals, const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                       const int32_t *__restrict__ arow, const double *__restrict__ X, int64_t ldx, const double *__restrict__ mu,
                                                       int32_t ncols, double *__restrict__ part) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int e0 = in ? rp[i] : 0, e1 = in ? rp[i + 1] : 0;
    const int q0 = (in && tptr) ? tptr[i] : 0, q1 = (in && tptr) ? tptr[i + 1] : 0;
    for (int c0 = 0; c0 < ncols; c0 += EIG_RT) { // (workgroup-uniform)
        const int nt = ncols - c0 < EIG_RT ? ncols - c0 : EIG_RT;
        double ra[EIG_RT] = {0.0, 0.0, 0.0, 0.0}, rm[EIG_RT] = {0.0, 0.0, 0.0, 0.0}, xa[EIG_RT] = {0.0, 0.0, 0.0, 0.0};
        if (in) {
            for (int e = e0; e < e1; e++) {
                const double a = avals[e], b = mvals ? mvals[e] : 0.0;
                const double *xj = X + ci[e];
#pragma unroll
                for (int t = 0; t < EIG_RT; t++)
                    if (t < nt) {
                        const double xv = xj[(int64_t)(c0 + t) * ldx];
                        ra[t] = fma(a, xv, ra[t]), rm[t] = fma(b, xv, rm[t]);
                    }
            }
            for (int q = q0; q < q1; q++) { // the mirrored entries of symmetric-lower storage
                const double a = avals[tidx[q]], b = mvals ? mvals[tidx[q]] : 0.0;
                const double *xj = X + arow[tidx[q]];
#pragma unroll
                for (int t = 0; t < EIG_RT; t++)
                    if (t < nt) {
                        const double xv = xj[(int64_t)(c0 + t) * ldx];
                        ra[t] = fma(a, xv, ra[t]), rm[t] = fma(b, xv, rm[t]);
                    }
            }
#pragma unroll
            for (int t = 0; t < EIG_RT; t++)
                if (t < nt) {
                    const double xi = X[i + (int64_t)(c0 + t) * ldx];
                    ra[t] = fabs(fma(-mu[c0 + t], mvals ? rm[t] : xi, ra[t]));
                    xa[t] = fabs(xi);
                }
        }
#pragma unroll
        for (int t = 0; t < EIG_RT; t++) {
            const double r = eig_block_max(ra[t], red), x = eig_block_max(xa[t], red);
            if (threadIdx.x == 0 && t < nt) part[(int64_t)(c0 + t) * gridDim.x + blockIdx.x] = r, part[(int64_t)(ncols + c0 + t) * gridDim.x + blockIdx.x] = x;
        }
    }
}

// part[blockIdx.x] = max over the workgroup's rows of sum_j |a_ij|
__global__ void __launch_bounds__(256) k_eig_rownorm(int32_t n, const int32_t *__restrict__ rp, const double *__restrict__ vals, const int32_t *__restrict__ tptr,
                                                     const int32_t *__restrict__ tidx, double *__restrict__ part) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (i < n) {
        for (int e = rp[i]; e < rp[i + 1]; e++) s += fabs(vals[e]);
        if (tptr)
            for (int q = tptr[i]; q < tptr[i + 1]; q++) s += fabs(vals[tidx[q]]);
    }
    s = eig_block_max(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup per column c: out[c] = max_b part[c * nblk + b]
__global__ void __launch_bounds__(256) k_eig_max(const double *__restrict__ part, int32_t nblk, double *__restrict__ out) {
    __shared__ double red[4];
    const double *p = part + (int64_t)blockIdx.x * nblk;
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) v = p[b] > v ? p[b] : v;
    v = eig_block_max(v, red);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// The last normalisation of the eigenvectors: x_c^T q_c (q_c = M x_c) as a compensated dot product (TwoProduct by FMA, TwoSum; Ogita,
// Rump & Oishi's Dot2), so that |x|_M = 1 holds to a few units of the last place whatever n is -- the plain sums of the iteration leave
// log2(n) of them.  grid (ceil(n / 256), ncols): the workgroup's (sum, compensation) to hi / lo [c gridDim.x + b], merged by a fixed tree.
__device__ __forceinline__ void eig_two_sum(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__global__ void __launch_bounds__(256) k_eig_dot2(int32_t n, const double *__restrict__ X, int64_t ldx, const double *__restrict__ Q, int64_t ldq, double *__restrict__ hi,
                                                  double *__restrict__ lo) {
#pragma clang fp contract(off)
    __shared__ double sh[256], sl[256];
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const double x = i < n ? X[i + (int64_t)c * ldx] : 0.0, q = i < n ? Q[i + (int64_t)c * ldq] : 0.0;
    const double pr = x * q;
    sh[threadIdx.x] = pr, sl[threadIdx.x] = fma(x, q, -pr);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            double t, e;
            eig_two_sum(sh[threadIdx.x], sh[threadIdx.x + s], t, e);
            sh[threadIdx.x] = t, sl[threadIdx.x] = (sl[threadIdx.x] + sl[threadIdx.x + s]) + e;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) hi[(int64_t)c * gridDim.x + blockIdx.x] = sh[0], lo[(int64_t)c * gridDim.x + blockIdx.x] = sl[0];
}
// one workgroup per column: the slots in slot order, out[c] = the rounded sum
__global__ void __launch_bounds__(64) k_eig_dot2_sum(int32_t nblk, const double *__restrict__ hi, const double *__restrict__ lo, double *__restrict__ out) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    double s = 0.0, comp = 0.0;
    for (int b = 0; b < nblk; b++) {
        double t, e;
        eig_two_sum(s, hi[(int64_t)c * nblk + b], t, e);
        s = t, comp += lo[(int64_t)c * nblk + b] + e;
    }
    out[c] = s + comp;
}
// x_c <- x_c / sqrt(nrm2[c]) (a column whose norm is not positive and finite is left alone)
__global__ void __launch_bounds__(256) k_eig_scale_cols(int32_t n, double *__restrict__ X, int64_t ldx, const double *__restrict__ nrm2) {
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const double s = nrm2[c];
    if (i < n && s > 0.0 && s < INFINITY) X[i + (int64_t)c * ldx] = X[i + (int64_t)c * ldx] / sqrt(s);
}

// grid (nblk, ncols): per workgroup of 256 rows the largest |x_i| of the column and the first row that has it
__global__ void __launch_bounds__(256) k_eig_absmax(int32_t n, const double *__restrict__ X, int64_t ldx, double *__restrict__ pv, int32_t *__restrict__ pi) {
    __shared__ double sv[256];
    __shared__ int si[256];
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const double a = i < n ? fabs(X[i + (int64_t)c * ldx]) : -1.0;
    sv[threadIdx.x] = a == a ? a : -1.0, si[threadIdx.x] = i; // (a NaN never wins)
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { // (a tie goes to the smaller ROW: a slot may already hold a row from further up)
            const double vo = sv[threadIdx.x + s];
            const int io = si[threadIdx.x + s];
            if (vo > sv[threadIdx.x] || (vo == sv[threadIdx.x] && io < si[threadIdx.x])) sv[threadIdx.x] = vo, si[threadIdx.x] = io;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) pv[(int64_t)c * gridDim.x + blockIdx.x] = sv[0], pi[(int64_t)c * gridDim.x + blockIdx.x] = si[0];
}
// one workgroup per column: sign[c] = -1 when the first entry of largest modulus is negative, else +1 (slots in order, the first wins ties)
__global__ void __launch_bounds__(64) k_eig_sign(int32_t nblk, const double *__restrict__ X, int64_t ldx, const double *__restrict__ pv,
                                                 const int32_t *__restrict__ pi, double *__restrict__ sign) {
    const int c = blockIdx.x;
    if (threadIdx.x != 0) return;
    double best = -1.0;
    int at = 0;
    for (int b = 0; b < nblk; b++)
        if (pv[(int64_t)c * nblk + b] > best) best = pv[(int64_t)c * nblk + b], at = pi[(int64_t)c * nblk + b];
    sign[c] = (best > 0.0 && X[at + (int64_t)c * ldx] < 0.0) ? -1.0 : 1.0;
}
__global__ void __launch_bounds__(256) k_eig_flip(int32_t n, double *__restrict__ X, int64_t ldx, const double *__restrict__ sign) {
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i < n && sign[c] < 0.0) X[i + (int64_t)c * ldx] = -X[i + (int64_t)c * ldx];
}

// ---- the inertia of the factor ----
// A pivot counts as positive (0), negative (1) or neither (2): zero, not a number, or replaced -- |d| == rep exactly, the value a
// static replacement leaves (pivot_replacement, kernels_common.hpp).
__device__ __forceinline__ int eig_pivot_class(double v, double rep) {
    if (!(fabs(v) > 0.0) || fabs(v) == rep) return 2; // (a NaN fails the first test)
    return v > 0.0 ? 0 : 1;
}
__device__ __forceinline__ double eig_replacement(const unsigned long long *anorm_bits, double pivot_eps) {
    const double rep = pivot_replacement(pivot_eps, __longlong_as_double((long long)*anorm_bits));
    return rep > 0.0 ? rep : -1.0; // (no replacement value asked for: nothing compares equal)
}

// The pivots of the TILED fronts (small[i] < 0: position i belongs to one): these take pivot c from row c on a symmetric handle, D of
// L D L^T is in d.  part[4 b + 0 .. 2] = the counts of workgroup b's stride, part[4 b + 3] = 0.
__global__ void __launch_bounds__(256) k_eig_inertia(int32_t n, const double *__restrict__ d, const unsigned long long *__restrict__ anorm_bits, double pivot_eps,
                                                     const int32_t *__restrict__ small, int64_t *__restrict__ part) {
    __shared__ int cnt[3][256];
    int c[3] = {0, 0, 0};
    const double rep = eig_replacement(anorm_bits, pivot_eps);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        if (small[i] < 0) c[eig_pivot_class(d[i], rep)]++;
    for (int q = 0; q < 3; q++) cnt[q][threadIdx.x] = c[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int q = 0; q < 3; q++) cnt[q][threadIdx.x] += cnt[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 4) part[4 * (int64_t)blockIdx.x + threadIdx.x] = threadIdx.x < 3 ? cnt[threadIdx.x][0] : 0;
}

// The fronts of at most SMALL_F rows, one wavefront each (list: their supernodes).  k_small_factor searches the pivot block (rows
// c .. p - 1) on every handle.  Where it kept the diagonal -- lperm is the identity: diagonally dominant and most definite fronts,
// ties go to the diagonal -- its LU without interchanges IS L D L^T and the pivots' signs count.  Where it moved a row, P F11 = L11 U11
// is no congruence and the signs of U11 say nothing; but the Schur complement a front hands to its parent does not depend on the order
// inside the pivot block, so the inertia of the matrix is still the sum over the fronts of the inertia of their F11.  Such a front's
// F11 = P^T L11 U11 is multiplied out in LDS (its lower triangle taken as the symmetric matrix) and its inertia counted by a
// Bunch-Kaufman elimination: 1 x 1 pivots by their sign, 2 x 2 pivots by their determinant and trace.  part[4 b + 3] counts such fronts.
constexpr int EIG_LDG = SMALL_F + 1;
__global__ void __launch_bounds__(64) k_eig_inertia_small(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD, const double *__restrict__ pool,
                                                          const int32_t *__restrict__ lperm, const double *__restrict__ diag,
                                                          const unsigned long long *__restrict__ anorm_bits, double pivot_eps, int64_t *__restrict__ part) {
    __shared__ double G[SMALL_F * EIG_LDG];
    __shared__ double col[SMALL_F];
    __shared__ int cls[SMALL_F];
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, f = fd.p + fd.m, lane = threadIdx.x;
    const double rep = eig_replacement(anorm_bits, pivot_eps);
    const int my = lane < p ? lperm[fd.first + lane] : lane;
    cls[lane] = lane < p ? eig_pivot_class(diag[fd.first + lane], rep) : 3;
    col[lane] = (lane < p && my != lane) ? 1.0 : 0.0;
    __syncthreads();
    int c[3] = {0, 0, 0};
    bool moved = false;
    for (int i = 0; i < p; i++) moved = moved || col[i] != 0.0; // (every lane reads the same words: wave-uniform)
    if (!moved) {
        if (lane == 0) {
            for (int i = 0; i < p; i++) c[cls[i]]++;
            for (int q = 0; q < 3; q++) part[4 * (int64_t)blockIdx.x + q] = c[q];
            part[4 * (int64_t)blockIdx.x + 3] = 0;
        }
        return;
    }
    // row `lane` of L11 U11 is row my of F11; U11 of a front with a packed copy of its rows of U lives there (k_small_factor)
    const double *F = pool + fd.off;
    const bool split = fd.epoff >= 0;
    const double *U = split ? pool + fd.epoff : F;
    const int ldu = split ? p : f;
    if (lane < p)
        for (int cc = 0; cc < p; cc++) {
            const int kmax = lane < cc ? lane : cc;
            double s = 0.0;
            for (int k = 0; k <= kmax; k++) s = fma(k == lane ? 1.0 : F[lane + (int64_t)k * f], U[k + (int64_t)cc * ldu], s);
            G[my * EIG_LDG + cc] = s;
        }
    __syncthreads();
    if (lane < p)
        for (int j = lane + 1; j < p; j++) G[lane * EIG_LDG + j] = G[j * EIG_LDG + lane]; // the lower triangle, mirrored
    __syncthreads();
    // symmetric exchange of rows and columns a, b of the full matrix
    auto swap_rc = [&](int a, int b) {
        __syncthreads(); // (the words the decision read are about to move)
        if (lane < p) {
            const double t = G[a * EIG_LDG + lane];
            G[a * EIG_LDG + lane] = G[b * EIG_LDG + lane], G[b * EIG_LDG + lane] = t;
        }
        __syncthreads();
        if (lane < p) {
            const double t = G[lane * EIG_LDG + a];
            G[lane * EIG_LDG + a] = G[lane * EIG_LDG + b], G[lane * EIG_LDG + b] = t;
        }
        __syncthreads();
    };
    const double alpha = 0.6403882032022076; // (1 + sqrt 17) / 8
    int k = 0;
    while (k < p) { // (every decision below reads LDS words all lanes see alike: wave-uniform)
        const double akk = G[k * EIG_LDG + k];
        double lam = 0.0;
        int r = k;
        for (int i = k + 1; i < p; i++) {
            const double v = fabs(G[i * EIG_LDG + k]);
            if (v > lam) lam = v, r = i;
        }
        int step = 1;
        if (lam > 0.0 && fabs(akk) < alpha * lam) {
            double sigma = 0.0;
            for (int j = k; j < p; j++)
                if (j != r) {
                    const double v = fabs(G[r * EIG_LDG + j]);
                    sigma = v > sigma ? v : sigma;
                }
            if (fabs(akk) * sigma >= alpha * lam * lam) {
            } else if (fabs(G[r * EIG_LDG + r]) >= alpha * sigma) {
                swap_rc(k, r);
            } else {
                if (r != k + 1) swap_rc(k + 1, r);
                step = 2;
            }
        }
        __syncthreads(); // (every lane has taken the decision before a row changes)
        if (step == 1) {
            const double d = G[k * EIG_LDG + k];
            c[eig_pivot_class(d, -1.0)]++;
            if (lam > 0.0 && d != 0.0 && lane > k && lane < p) {
                const double l = G[lane * EIG_LDG + k] / d;
                for (int j = k + 1; j < p; j++) G[lane * EIG_LDG + j] = fma(-l, G[k * EIG_LDG + j], G[lane * EIG_LDG + j]);
            }
        } else {
            const double a = G[k * EIG_LDG + k], b = G[(k + 1) * EIG_LDG + k], d = G[(k + 1) * EIG_LDG + k + 1], det = a * d - b * b;
            if (det < 0.0) c[0]++, c[1]++;
            else if (det > 0.0) c[a > 0.0 ? 0 : 1] += 2;
            else c[2]++, c[eig_pivot_class(a + d, -1.0)]++;
            if (det != 0.0 && lane > k + 1 && lane < p) {
                const double g1 = G[lane * EIG_LDG + k], g2 = G[lane * EIG_LDG + k + 1];
                const double l1 = (g1 * d - g2 * b) / det, l2 = (g2 * a - g1 * b) / det;
                for (int j = k + 2; j < p; j++) G[lane * EIG_LDG + j] = fma(-l1, G[k * EIG_LDG + j], fma(-l2, G[(k + 1) * EIG_LDG + j], G[lane * EIG_LDG + j]));
            }
        }
        __syncthreads();
        k += step;
    }
    if (lane == 0) {
        for (int q = 0; q < 3; q++) part[4 * (int64_t)blockIdx.x + q] = c[q];
        part[4 * (int64_t)blockIdx.x + 3] = 1;
    }
}

// one workgroup: out[q] = sum over the slots (integers: exact in any order; thread t adds the slots t, t + 256, ... and a tree the rest)
__global__ void __launch_bounds__(256) k_eig_inertia_sum(int64_t nslot, const int64_t *__restrict__ part, int64_t *__restrict__ out) {
    __shared__ long long red[4][256];
    long long s[4] = {0, 0, 0, 0};
    for (int64_t b = threadIdx.x; b < nslot; b += 256)
        for (int q = 0; q < 4; q++) s[q] += part[4 * b + q];
    for (int q = 0; q < 4; q++) red[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int q = 0; q < 4; q++) red[q][threadIdx.x] += red[q][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 4) out[threadIdx.x] = red[threadIdx.x][0];
}

} // namespace hipmf
