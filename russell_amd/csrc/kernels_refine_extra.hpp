// kernels_refine_extra.hpp -- extra-precise iterative refinement (solver_hipmf_solve_extra_precise; Demmel, Hida, Kahan, Li, Mukherjee
// & Riedy 2006, the scheme of LAPACK's xGERFSX): the residual r = b - A (x + tail) accumulated in more than twice the working
// precision and rounded once, and the update of (x, tail) fused with the three measures the stopping rule reads.
//
// Residual: the streaming structure of spmv_block (kernels_vector.hpp) -- row blocks of at most SPMV_CAP stored entries, the entries
// staged through LDS once, L lanes per row -- with every product split into (p, e), p + e = -a x exactly (TwoProduct by an FMA), and
// every sum a TwoSum into a (sum, compensation) pair (Ogita, Rump & Oishi's Dot2, as ea_dot2_sub of kernels_solve_transpose.hpp).
// The compensation's own additions are TwoSums as well, their errors summed in a third word (the authors' SumK with K = 3): the pair
// alone leaves a noise of a few eps^2 (|A||x|)_i in r_i, which the solve multiplies by up to cond(A) -- the floor of the form with a
// tail, and from matrix to matrix a matter of how that noise happens to lie (measured on the emulator, biharm300 in lower storage:
// 3.4e-25 with the pair against 1.3e-26 for the same Dot2 in another order, equal noise per row).  The third word costs a dozen
// flops per entry of a kernel that is bound by memory and removes that floor.
// The lanes of a row are combined by a butterfly of TwoSums: TwoSum's error term does not depend on the order of its operands, so both
// partners of an exchange hold the same words and the result has the same bits in every call.  With a tail the entry's second product
// -a tail goes through the same steps.  The mirrored entries of symmetric-lower storage are added by the row's first lane.
// LDS: four staged arrays (p, e of x and of the tail) + three reduction arrays = 4 x 8 KB + 6 KB = 38 KB per workgroup, against the
// 20 KB of SpmvLds: four workgroups per CU of the 160 KB (spmv_block: eight).
// Contraction is off wherever an error-free step is formed: a fused a * x + s would break it.
#pragma once
#include "kernels_common.hpp"
#include "kernels_vector.hpp"

namespace hipmf {

struct XrLds {
    double p[SPMV_CAP], e[SPMV_CAP];   // -a x = p + e
    double q[SPMV_CAP], f[SPMV_CAP];   // -a tail = q + f (TAIL only)
    double red[3][256];
};

// the running sum of a lane: s + c + cc, |c| of the order of eps |s|, cc the rounding errors of the additions into c
struct XrSum {
    double s, c, cc;
};

// a + b = t + err exactly (Knuth's TwoSum; err is the same whichever operand comes first)
__device__ __forceinline__ double xr_two_sum(double a, double b, double &err) {
#pragma clang fp contract(off)
    const double t = a + b, bb = t - a;
    err = (a - (t - bb)) + (b - bb);
    return t;
}
// acc += v, v of the order of acc.s: into the sum, the error into the compensation
__device__ __forceinline__ void xr_add(XrSum &a, double v) {
#pragma clang fp contract(off)
    double e1, e2;
    a.s = xr_two_sum(a.s, v, e1);
    a.c = xr_two_sum(a.c, e1, e2);
    a.cc += e2;
}
// acc += v, v of the order of eps acc.s (the error term of a product): into the compensation
__device__ __forceinline__ void xr_add_low(XrSum &a, double v) {
#pragma clang fp contract(off)
    double e2;
    a.c = xr_two_sum(a.c, v, e2);
    a.cc += e2;
}
// acc += the sum of another lane (symmetric in its operands)
__device__ __forceinline__ void xr_merge(XrSum &a, double s2, double c2, double cc2) {
#pragma clang fp contract(off)
    double e1, e2, e3;
    a.s = xr_two_sum(a.s, s2, e1);
    const double cs = xr_two_sum(a.c, c2, e2);
    a.c = xr_two_sum(cs, e1, e3);
    a.cc = (a.cc + cc2) + (e2 + e3);
}
// acc += -a x without rounding error in the product and the sum
__device__ __forceinline__ void xr_dot_sub(XrSum &acc, double a, double x) {
#pragma clang fp contract(off)
    const double p = -a * x, pe = fma(-a, x, -p);
    xr_add(acc, p);
    xr_add_low(acc, pe);
}
// the sum rounded once (s and c nearly cancel where the residual is small: their sum is split again before the low words join)
__device__ __forceinline__ double xr_round(const XrSum &a) {
#pragma clang fp contract(off)
    double lo;
    const double hi = xr_two_sum(a.s, a.c, lo);
    return hi + (lo + a.cc);
}

// one column: r = b - A (x + tail) on the workgroup's row block (tail == nullptr: r = b - A x); active == false: r = 0 on these rows
// (the column rides along as zeros through the next pass pair)
template <bool TAIL>
__device__ __forceinline__ void xr_residual_block(XrLds &sh, const int32_t *__restrict__ row_blk, const int32_t *__restrict__ rp,
                                                  const int32_t *__restrict__ ci, const double *__restrict__ vals,
                                                  const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                  const int32_t *__restrict__ arow, const double *__restrict__ x,
                                                  const double *__restrict__ tail, const double *__restrict__ b, double *__restrict__ r,
                                                  bool active) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int r0 = row_blk[blockIdx.x], r1 = row_blk[blockIdx.x + 1];
    if (!active) {
        for (int i = r0 + tid; i < r1; i += 256) r[i] = 0.0;
        return;
    }
    const int e0 = rp[r0], e1 = rp[r1];
    if (e1 - e0 > SPMV_CAP) {
        // one long row (r1 == r0 + 1): strided partial sums, fixed-order tree of merges over the workgroup
        XrSum acc = {tid == 0 ? b[r0] : 0.0, 0.0, 0.0};
        for (int e = e0 + tid; e < e1; e += 256) {
            const double av = vals[e];
            const int j = ci[e];
            xr_dot_sub(acc, av, x[j]);
            if (TAIL) xr_dot_sub(acc, av, tail[j]);
        }
        if (tptr)
            for (int q = tptr[r0] + tid; q < tptr[r0 + 1]; q += 256) {
                const double av = vals[tidx[q]];
                const int j = arow[tidx[q]];
                xr_dot_sub(acc, av, x[j]);
                if (TAIL) xr_dot_sub(acc, av, tail[j]);
            }
        sh.red[0][tid] = acc.s, sh.red[1][tid] = acc.c, sh.red[2][tid] = acc.cc;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) {
                XrSum m = {sh.red[0][tid], sh.red[1][tid], sh.red[2][tid]};
                xr_merge(m, sh.red[0][tid + st], sh.red[1][tid + st], sh.red[2][tid + st]);
                sh.red[0][tid] = m.s, sh.red[1][tid] = m.c, sh.red[2][tid] = m.cc;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const XrSum m = {sh.red[0][0], sh.red[1][0], sh.red[2][0]};
            r[r0] = xr_round(m);
        }
        return;
    }
    const int ne = e1 - e0;
    for (int k = tid; k < ne; k += 4 * 256) {
        double v[4];
        int cj[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = k + 256 * u;
            v[u] = kk < ne ? vals[e0 + kk] : 0.0;
            cj[u] = kk < ne ? ci[e0 + kk] : 0;
        }
        double xv[4], tv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            xv[u] = (k + 256 * u < ne) ? x[cj[u]] : 0.0;
            tv[u] = (TAIL && k + 256 * u < ne) ? tail[cj[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = k + 256 * u;
            if (kk < ne) {
                const double pp = -v[u] * xv[u];
                sh.p[kk] = pp, sh.e[kk] = fma(-v[u], xv[u], -pp);
                if (TAIL) {
                    const double qq = -v[u] * tv[u];
                    sh.q[kk] = qq, sh.f[kk] = fma(-v[u], tv[u], -qq);
                }
            }
        }
    }
    __syncthreads();
    const int nr = r1 - r0;
    int lsh = 0; // log2(lanes per row)
    while (lsh < 6 && (nr << (lsh + 1)) <= 256) lsh++;
    const int L = 1 << lsh, sub = tid & (L - 1);
    for (int rr = tid >> lsh; rr < ((nr + (256 >> lsh) - 1) / (256 >> lsh)) * (256 >> lsh); rr += 256 >> lsh) {
        const int i = r0 + rr;
        XrSum acc = {0.0, 0.0, 0.0};
        if (rr < nr) {
            if (sub == 0) acc.s = b[i];
            for (int e = rp[i] - e0 + sub; e < rp[i + 1] - e0; e += L) {
                xr_add(acc, sh.p[e]);
                xr_add_low(acc, sh.e[e]);
                if (TAIL) {
                    xr_add(acc, sh.q[e]);
                    xr_add_low(acc, sh.f[e]);
                }
            }
            if (tptr && sub == 0)
                for (int q = tptr[i]; q < tptr[i + 1]; q++) {
                    const double av = vals[tidx[q]];
                    const int j = arow[tidx[q]];
                    xr_dot_sub(acc, av, x[j]);
                    if (TAIL) xr_dot_sub(acc, av, tail[j]);
                }
        }
        for (int o = L >> 1; o > 0; o >>= 1) // (every lane of the wavefront takes part: the trip count above is uniform)
            xr_merge(acc, __shfl_xor(acc.s, o), __shfl_xor(acc.c, o), __shfl_xor(acc.cc, o));
        if (rr < nr && sub == 0) r[i] = xr_round(acc);
    }
}

// Residuals of a block of columns in one launch, as k_residual_cols: column k of x / tail / b at base + k * stride, of r at r + k * rstr;
// the workgroup keeps its row block and walks the columns.  Columns whose bit in `mask` is clear get r = 0.  ncols == 1: the single form.
template <bool TAIL>
__global__ void __launch_bounds__(256) k_xr_residual_cols(const int32_t *__restrict__ row_blk, const int32_t *__restrict__ rp,
                                                          const int32_t *__restrict__ ci, const double *__restrict__ vals,
                                                          const int32_t *__restrict__ tptr, const int32_t *__restrict__ tidx,
                                                          const int32_t *__restrict__ arow, const double *__restrict__ x,
                                                          const double *__restrict__ tail, int64_t xstr, const double *__restrict__ b, int64_t bstr,
                                                          double *__restrict__ r, int64_t rstr, int32_t ncols, uint32_t mask) {
    __shared__ XrLds sh;
    for (int k = 0; k < ncols; k++) {
        xr_residual_block<TAIL>(sh, row_blk, rp, ci, vals, tptr, tidx, arow, x + k * xstr, TAIL ? tail + k * xstr : nullptr, b + k * bstr, r + k * rstr,
                                ((mask >> k) & 1u) != 0);
        __syncthreads();
    }
}

// The measures of a step live in atomic-max-on-bits slots, the RES_SLOTS idiom of kernels_vector.hpp: per column XR_NORM_WORDS words,
// slot s at word s * RES_SLOT_WORDS: [0] max |dx_i|, [1] max |x_i|, [2] max |dx_i| / |x_i| (0 / 0 counts 0, nonzero / 0 +infinity),
// [3] 1.0 when a component of dx or x is not finite.  A NaN never wins a maximum; word 3 is how the host learns of one.
constexpr int XR_NORM_WORDS = RES_NORM_WORDS;

__device__ __forceinline__ void xr_block_max(double (&red)[4][256], double m0, double m1, double m2, double m3, unsigned long long *nrm) {
    const int tid = threadIdx.x;
    red[0][tid] = m0 > 0.0 ? m0 : 0.0, red[1][tid] = m1 > 0.0 ? m1 : 0.0, red[2][tid] = m2 > 0.0 ? m2 : 0.0, red[3][tid] = m3;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int w = 0; w < 4; w++)
                if (red[w][tid + s] > red[w][tid]) red[w][tid] = red[w][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        unsigned long long *slot = nrm + (size_t)(blockIdx.x & (RES_SLOTS - 1)) * RES_SLOT_WORDS;
        for (int w = 0; w < 4; w++) atomicMax(slot + w, (unsigned long long)__double_as_longlong(red[w][0]));
    }
}

// The update of a step and its measures, one launch for the columns of a block (blockIdx.y = column; columns whose bit in `mask` is
// clear are left alone): the measures of (x, dx) as they stand BEFORE the update, the old x (and tail) into xs (ts) -- a step the host
// rejects is taken back from there --, then x <- x + dx or, with a tail, (x, tail) <- the renormalised TwoSum of x + dx + tail.
// PAIRS: the vectors are interleaved complex numbers and the measures take the moduli of the complex components (n even).
// dx == nullptr: measures of x alone (word 1 and word 3; the call's first look at b), nothing is written.
template <bool PAIRS>
__global__ void __launch_bounds__(256) k_xr_update_cols(int32_t n, double *__restrict__ x, double *__restrict__ tail, int64_t xstr,
                                                        const double *__restrict__ dx, int64_t dstr, double *__restrict__ xs, double *__restrict__ ts,
                                                        int64_t sstr, unsigned long long *nrm, uint32_t mask) {
#pragma clang fp contract(off)
    __shared__ double red[4][256];
    const int k = blockIdx.y;
    if (!((mask >> k) & 1u)) return;
    double *const xk = x + k * xstr, *const tk = tail ? tail + k * xstr : nullptr;
    const double *const dk = dx ? dx + k * dstr : nullptr;
    double *const xsk = xs ? xs + k * sstr : nullptr, *const tsk = ts ? ts + k * sstr : nullptr;
    constexpr int W = PAIRS ? 2 : 1;
    const int items = n / W;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
        double xv[W], dv[W];
#pragma unroll
        for (int w = 0; w < W; w++) xv[w] = xk[W * it + w], dv[w] = dk ? dk[W * it + w] : 0.0;
        const double ax = PAIRS ? hypot(xv[0], xv[W - 1]) : fabs(xv[0]), ad = PAIRS ? hypot(dv[0], dv[W - 1]) : fabs(dv[0]);
        if (!(ax <= 1.79769313486231570815e308) || !(ad <= 1.79769313486231570815e308)) m3 = 1.0;
        const double q = ax > 0.0 ? ad / ax : (ad > 0.0 ? INFINITY : 0.0);
        m0 = ad > m0 ? ad : m0, m1 = ax > m1 ? ax : m1, m2 = q > m2 ? q : m2;
        if (!dk) continue;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const int i = W * it + w;
            xsk[i] = xv[w];
            if (tk) {
                const double tv = tk[i];
                tsk[i] = tv;
                double err;
                const double s = xr_two_sum(xv[w], dv[w], err);
                const double t = err + tv, hi = s + t;
                xk[i] = hi, tk[i] = t - (hi - s); // FastTwoSum(s, t): |t| <= |s| up to rounding
            } else {
                xk[i] = xv[w] + dv[w];
            }
        }
    }
    xr_block_max(red, m0, m1, m2, m3, nrm + (size_t)k * XR_NORM_WORDS);
}

} // namespace hipmf
