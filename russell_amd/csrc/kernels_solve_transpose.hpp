// kernels_solve_transpose.hpp -- transposed triangular solves (A^T x = b) on the stored factor, the residual of A^T, and the vector
// kernels of the MUMPS-style error analysis (solver_hipmf_solve_with_error_analysis).
//
// The factor of the permuted, scaled matrix is A^ = P^T L U (P: the interchanges inside the pivot blocks).  A^T y = c is
//   forward, leaves to root, U^T:   w = [c1; 0] + sum_children u_c (same rel maps as the ordinary forward pass),
//                                   z1 = inv(U11)^T w1,  u = w2 - U12^T z1
//   backward, root to leaves, L^T:  t = inv(L11)^T (z1 - L21^T x2),  x1 = P^T t  (x1[lperm[i]] = t_i),  x2 gathered through `rows`
// Small fronts (f <= SMALL_F): one wavefront per front, everything in LDS (k_tr_fwd_small / k_tr_bwd_small; the panel is dynamic LDS
// sized to the largest small front of the level, as k_fwd / k_bwd do, so that levels of tiny fronts keep many wavefronts per CU).
// Big fronts: with E = [inv(L11) P; -L21 inv(L11) P] and E' = [inv(U11) | -inv(U11) U12] (both forms of kernels_common.hpp),
//   [z1; u - w2] = E'^T w1   and   x1 = E^T [z1; x2]:
// one dot product per STORED column of E' / E.  Those columns are contiguous: a wavefront reads a column with consecutive lanes
// (coalesced, the layout the factorisation left -- no transposed copy) against the front's vector, which one launch before has
// assembled into the workspace (k_tr_assemble / k_tr_gather) and which the dot products read from L2: nothing of the size of a
// front is staged in LDS, so fronts of any size are served (the top separators of 3D factors included).
// Known zeros are skipped: column c < p of E' (inv(U11), upper triangular) has rows < 32 (c / 32 + 1) only; column c of E (the pivot
// rows inv(L11) P are block lower triangular in 32-column blocks, not so in the FD_DENSE_TOP form) has rows >= 32 (c / 32) only.
// Scheduling: one launch per level and front class, level-synchronous -- no waits inside a launch, no counters, no tagged words.
// Every sum has a fixed order (children ascending, lanes in fixed strides, a fixed butterfly), so two solves give the same bits.
#pragma once
#include "kernels_common.hpp"

namespace hipmf {

constexpr int TR_ROWS = 1024; // rows of a front's vector per assembly / gather task
constexpr int TR_COLS = 16;   // stored columns of E / E' per GEMV task (four wavefronts, four columns each)

// forward (U^T) step of a small front: one wavefront
__global__ void __launch_bounds__(64) k_tr_fwd_small(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD,
                                                     const double *__restrict__ pool, const int32_t *__restrict__ child_idx,
                                                     const int32_t *__restrict__ rel, double *__restrict__ work, double *__restrict__ xp,
                                                     int32_t ldu) {
    HIPMF_DYN_SHARED(double, UL); // UL[t * ldu + j] = U(j, t), j < p, t < f  (ldu = the level's largest p, odd: fmax * ldu doubles)
    __shared__ double w[SMALL_F];
    const int tid = threadIdx.x;
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, f = fd.p + fd.m;
    // (the rows of U: the packed p x f copy when the front has one -- m > 0 --, else the front itself; as k_bwd)
    const double *Ub = fd.epoff >= 0 ? pool + fd.epoff : pool + fd.off;
    const int64_t us = fd.epoff >= 0 ? p : f;
    for (int e = tid; e < p * f; e += 64) {
        const int j = e % p, t = e / p;
        UL[t * ldu + j] = Ub[j + (int64_t)t * us];
    }
    w[tid] = (tid < p) ? xp[fd.first + tid] : 0.0;
    __syncthreads();
    for (int ci = fd.child_begin; ci < fd.child_end; ci++) {
        const FrontDesc cd = FD[child_idx[ci]];
        const double *uc = work + cd.woff + cd.p;
        const int32_t *relc = rel + cd.rowptr;
        for (int i = tid; i < cd.m; i += 64) w[relc[i]] += uc[i];
        __syncthreads();
    }
    double v = (tid < f) ? w[tid] : 0.0;
    for (int j = 0; j < p; j++) {
        if (tid == j) v = v / UL[j * ldu + j];
        const double zj = wave_bcast(v, j);
        if (tid > j && tid < f) v -= UL[tid * ldu + j] * zj;
    }
    if (tid < p) xp[fd.first + tid] = v;
    else if (tid < f) work[fd.woff + tid] = v;
}

// backward (L^T) step of a small front: one wavefront
__global__ void __launch_bounds__(64) k_tr_bwd_small(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD,
                                                     const double *__restrict__ pool, const int32_t *__restrict__ rows,
                                                     const int32_t *__restrict__ lperm, double *__restrict__ xp, int32_t ldl) {
    HIPMF_DYN_SHARED(double, LL); // LL[i * ldl + r] = L(r, i), r < f, i < p  (ldl = the level's largest f, odd: pmax * ldl doubles)
    __shared__ double xg[SMALL_F];
    const int tid = threadIdx.x;
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, m = fd.m, f = fd.p + fd.m;
    const double *F = pool + fd.off;
    for (int e = tid; e < p * f; e += 64) {
        const int r = e % f, i = e / f;
        LL[i * ldl + r] = F[r + (int64_t)i * f];
    }
    if (tid < m) xg[tid] = xp[rows[fd.rowptr + tid]];
    double v = (tid < p) ? xp[fd.first + tid] : 0.0;
    __syncthreads();
    if (tid < p) {
        double acc = 0.0;
        for (int r = 0; r < m; r++) acc += LL[tid * ldl + p + r] * xg[r];
        v -= acc;
    }
    for (int r = p - 1; r > 0; r--) { // unit lower L11: t_r is final once the rows below it are done
        const double tr = wave_bcast(v, r);
        if (tid < r) v -= LL[tid * ldl + r] * tr;
    }
    if (tid < p) xp[fd.first + lperm[fd.first + tid]] = v;
}

// forward, big fronts: w = [c1; 0] + children's updates into the workspace, rows [r0, r1) of the front per task
__global__ void __launch_bounds__(256) k_tr_assemble(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                     const int32_t *__restrict__ child_idx, const int32_t *__restrict__ rel,
                                                     double *__restrict__ work, const double *__restrict__ xp) {
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    const int p = fd.p, r0 = tk.r0, r1 = tk.r1;
    double *W = work + fd.woff;
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) W[r] = r < p ? xp[fd.first + r] : 0.0;
    __syncthreads();
    for (int ci = fd.child_begin; ci < fd.child_end; ci++) {
        const FrontDesc cd = FD[child_idx[ci]];
        const double *uc = work + cd.woff + cd.p;
        const int32_t *relc = rel + cd.rowptr;
        for (int i = threadIdx.x; i < cd.m; i += 256) { // (rel is injective within a child: no two threads of one child meet)
            const int r = relc[i];
            if (r >= r0 && r < r1) W[r] += uc[i];
        }
        __syncthreads();
    }
}

// backward, big fronts: v = [z1; x2] into the workspace, rows [r0, r1) per task
__global__ void __launch_bounds__(256) k_tr_gather(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                   const int32_t *__restrict__ rows, double *__restrict__ work, const double *__restrict__ xp) {
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    const int p = fd.p;
    double *V = work + fd.woff;
    for (int r = tk.r0 + (int)threadIdx.x; r < tk.r1; r += 256) V[r] = r < p ? xp[fd.first + r] : xp[rows[fd.rowptr + r - p]];
}

// dot product of one stored column (contiguous, rows [i0, i1)) with the front's vector, by one wavefront; the same bits in every lane
__device__ __forceinline__ double tr_col_dot(const double *__restrict__ col, const double *__restrict__ v, int i0, int i1, int lane) {
    double acc = 0.0;
    int i = i0 + lane;
    for (; i + 192 < i1; i += 256) {
        const double e0 = col[i], e1 = col[i + 64], e2 = col[i + 128], e3 = col[i + 192];
        const double v0 = v[i], v1 = v[i + 64], v2 = v[i + 128], v3 = v[i + 192];
        acc += e0 * v0;
        acc += e1 * v1;
        acc += e2 * v2;
        acc += e3 * v3;
    }
    for (; i < i1; i += 64) acc += col[i] * v[i];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// GEMV of a big front, columns [r0, r1) of the task (FWD: E'^T w1 over the f columns of E'; else E^T v over the p columns of E)
template <bool FWD>
__global__ void __launch_bounds__(256) k_tr_gemv(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                 const double *__restrict__ pool, double *__restrict__ work, double *__restrict__ xp) {
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    fd_resident(fd);
    const int p = fd.p, f = fd.p + fd.m;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *V = work + fd.woff;
    for (int c = tk.r0 + wv; c < tk.r1; c += 4) {
        if (FWD) {
            const int i1 = c < p ? ((c / NB + 1) * NB < p ? (c / NB + 1) * NB : p) : p;
            const double t = tr_col_dot(pool + fd.epoff + (int64_t)c * fd.ldp, V, 0, i1, lane);
            if (lane == 0) {
                if (c < p) xp[fd.first + c] = t;
                else V[c] += t; // u = w2 + (E'^T w1)[c]: only this lane reads or writes entry c
            }
        } else {
            const int i0 = (fd.flags & FD_DENSE_TOP) ? 0 : (c / NB) * NB;
            const double t = tr_col_dot(pool + fd.eoff + (int64_t)c * fd.ld, V, i0, f, lane);
            if (lane == 0) xp[fd.first + c] = t;
        }
    }
}

// entry of the transposed system: xp[j] = cs[perm[j]] * b[perm[j]] (cs == nullptr: no column scaling)
__global__ void k_tr_perm_in(int32_t n, const int32_t *__restrict__ perm, const double *__restrict__ cs, const double *__restrict__ b,
                             double *__restrict__ xp) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) {
        const int q = perm[j];
        xp[j] = cs ? cs[q] * b[q] : b[q];
    }
}

// v[2 k + 1] = -v[2 k + 1]: the interleaved complex pairs of the complex twin's A^T solve (through the real-equivalent A^H solve)
__global__ void k_tr_conj(int32_t n, double *__restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (i & 1)) v[i] = -v[i];
}

__device__ __forceinline__ void tr_atomic_max(unsigned long long *w, double v) { // non-negative doubles order like their bits
    atomicMax(w, (unsigned long long)__double_as_longlong(v));
}

// Rows of A^T (columns of A: tptr / trow / tmap, values through the map into the stored values), one thread per row, entries in order.
// b == nullptr: y = A^T x.  Else r = b - A^T x and, into nrm (zeroed before): nrm[0] = max |r_i|, nrm[1] = omega = max |r_i| / (|A^T||x| + |b|)_i.
__global__ void __launch_bounds__(256) k_tr_spmv(int32_t n, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                 const int32_t *__restrict__ tmap, const double *__restrict__ vals, const double *__restrict__ x,
                                                 const double *__restrict__ b, double *__restrict__ y, unsigned long long *nrm) {
    __shared__ double sr[256], so[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double a = 0.0, q = 0.0;
    if (i < n) {
        double acc = 0.0, d = 0.0;
        for (int k = tptr[i]; k < tptr[i + 1]; k++) {
            const double t = vals[tmap[k]] * x[trow[k]];
            acc += t;
            d += fabs(t);
        }
        if (b) {
            const double ri = b[i] - acc, di = d + fabs(b[i]);
            y[i] = ri;
            a = fabs(ri);
            q = di > 0.0 ? a / di : (a > 0.0 ? 1.0 : 0.0);
        } else {
            y[i] = acc;
        }
    }
    if (!b) return;
    sr[threadIdx.x] = a, so[threadIdx.x] = q;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sr[threadIdx.x] = fmax(sr[threadIdx.x], sr[threadIdx.x + s]);
            so[threadIdx.x] = fmax(so[threadIdx.x], so[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) tr_atomic_max(nrm, sr[0]), tr_atomic_max(nrm + 1, so[0]);
}

// ---- error analysis (Arioli, Demmel & Duff; the quantities of MUMPS's RINFOG(4..11)) ----

// s + c += -a x without rounding error in the product and the sum (TwoProduct by an FMA, TwoSum; Ogita, Rump & Oishi's Dot2):
// the residual of a solution that is accurate to rounding level is itself a few ulps of |A||x| -- in plain double arithmetic half of
// its digits would be the noise of the summation order.  (Contraction is off: a fused a * x + s would break the error-free steps.)
__device__ __forceinline__ void ea_dot2_sub(double &s, double &c, double a, double x) {
#pragma clang fp contract(off)
    const double p = -a * x, pe = fma(-a, x, -p);
    const double t = s + p, bb = t - s, e = (s - (t - bb)) + (p - bb);
    s = t;
    c += e + pe;
}

// One pass over A (CSR + the mirrored entries of symmetric-lower storage), fused with the residual: per row r_i = b_i - (A x)_i (in
// twice the working precision, rounded once), ax_i = (|A||x|)_i, arow_i = sum_j |a_ij|; maxima (atomicMax on the bits) into sc:
// [0] N_A = max arow_i, [1] N_x = max |x_i|, [2] max |r_i|.  Entries in stored order per row.
__global__ void __launch_bounds__(256) k_ea_rows(int32_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                 const double *__restrict__ vals, const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                 const int32_t *__restrict__ arow_of, const double *__restrict__ x, const double *__restrict__ b,
                                                 double *__restrict__ r, double *__restrict__ ax, double *__restrict__ arow,
                                                 unsigned long long *sc) {
    __shared__ double s0[256], s1[256], s2[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double na = 0.0, nx = 0.0, nr = 0.0;
    if (i < n) {
        double rs = b[i], rc = 0.0, d = 0.0, a = 0.0;
        for (int e = rp[i]; e < rp[i + 1]; e++) {
            const double av = vals[e], xv = x[ci[e]];
            ea_dot2_sub(rs, rc, av, xv);
            d += fabs(av * xv), a += fabs(av);
        }
        if (tptr)
            for (int q = tptr[i]; q < tptr[i + 1]; q++) {
                const double av = vals[tidx[q]], xv = x[arow_of[tidx[q]]];
                ea_dot2_sub(rs, rc, av, xv);
                d += fabs(av * xv), a += fabs(av);
            }
        const double ri = rs + rc;
        r[i] = ri, ax[i] = d, arow[i] = a;
        na = a, nx = fabs(x[i]), nr = fabs(ri);
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

// The split into I1 = {d_i > tau_i} and I2, the backward errors and the weights of the two condition numbers:
// sc[3] = omega1, sc[4] = omega2 (atomicMax on the bits), cnt[0] = |I2|.
__global__ void __launch_bounds__(256) k_ea_split(int32_t n, double tau_scale, double nx, const double *__restrict__ r, const double *__restrict__ ax,
                                                  const double *__restrict__ arow, const double *__restrict__ b, double *__restrict__ w1,
                                                  double *__restrict__ w2, unsigned long long *sc, int32_t *cnt) {
    __shared__ double s3[256], s4[256];
    __shared__ int c2[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double o1 = 0.0, o2 = 0.0;
    int in2 = 0;
    if (i < n) {
        const double ab = fabs(b[i]), ar = fabs(r[i]), d = ax[i] + ab, tau = tau_scale * (arow[i] * nx + ab);
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

// y = w o v
__global__ void k_ea_hadamard(int32_t n, const double *__restrict__ w, const double *__restrict__ v, double *__restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = w[i] * v[i];
}

// v = e / n (mode 0), the alternating test vector (-1)^i (1 + i / (n - 1)) (mode 1), e_j (mode 2)
__global__ void k_ea_fill(int32_t n, int32_t mode, int32_t j, double *__restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) v[i] = 1.0 / (double)n;
    else if (mode == 1) v[i] = ((i & 1) ? -1.0 : 1.0) * (1.0 + (n > 1 ? (double)i / (double)(n - 1) : 0.0));
    else v[i] = i == j ? 1.0 : 0.0;
}

// xi = sign(y) (+1 for y >= 0); flag[0] |= 1 where the sign differs from the previous xi
__global__ void k_ea_sign(int32_t n, const double *__restrict__ y, double *__restrict__ xi, int32_t *flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = y[i] >= 0.0 ? 1.0 : -1.0;
    if (s != xi[i]) atomicOr(flag, 1);
    xi[i] = s;
}

// Deterministic reductions in two launches: EA_RED_WG workgroups walk the vector in fixed strides and combine in a fixed tree, one
// workgroup combines their partials.  mode 0: sum |v_i| -> out[0]; mode 1: max |v_i| with the smallest index on ties -> out[0], index -> iout[0].
constexpr int EA_RED_WG = 256;
__global__ void __launch_bounds__(256) k_ea_reduce1(int32_t n, int32_t mode, const double *__restrict__ v, double *__restrict__ pv, int32_t *__restrict__ pi) {
    __shared__ double sv[256];
    __shared__ int si[256];
    double a = 0.0;
    int ai = 0x7fffffff;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += EA_RED_WG * 256) {
        const double t = fabs(v[i]);
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
__global__ void __launch_bounds__(256) k_ea_reduce2(int32_t mode, const double *__restrict__ pv, const int32_t *__restrict__ pi, double *out, int32_t *iout) {
    __shared__ double sv[EA_RED_WG];
    __shared__ int si[EA_RED_WG];
    sv[threadIdx.x] = pv[threadIdx.x], si[threadIdx.x] = pi[threadIdx.x];
    __syncthreads();
    for (int s = EA_RED_WG / 2; s > 0; s >>= 1) {
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
    if (threadIdx.x == 0) out[0] = sv[0], iout[0] = si[0];
}

} // namespace hipmf
