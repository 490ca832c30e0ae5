// kernels_solve_transpose_blocked.hpp -- the transposed solves of kernels_solve_transpose.hpp for a BLOCK of TR_KB = 16 right-hand
// sides (solver_hipmf_solve_transpose_many): the same level-synchronous launches, every stored entry of the factor read once per block.
//
// Layouts
//   block vectors (xp, x, b, r)  column-major, column c at base + c * stride (stride n for the solver's own buffers, ld for the caller's)
//   workspace                    the front's f x 16 values INTERLEAVED: entry (r, c) of front s at work[(woff + r) * TR_KB + c] -- the sixteen
//                                values of a row are one 128-byte line: the B operand of the MFMA (rows k .. k + 3, sixteen columns) is 512
//                                contiguous bytes, and a child's update row is added with one line per row
// A block always carries sixteen columns: the entry kernel zero-fills the columns a tail block lacks (and those a refinement step no
// longer corrects), the exit kernel masks them.  Every column's arithmetic is therefore the same in every block and at every position:
// the small fronts run the single-column recurrences on sixteen register values, and an MFMA output column depends on its own column of
// the B operand only.
// Small fronts (f <= SMALL_F): one wavefront per front, the p x f panel in dynamic LDS (loaded ONCE for the sixteen columns), the
// substitution steps loop over the columns with the column values in registers.
// Big fronts: [z1; u - w2] = E'^T W1 (f x 16) and X1 = E^T V (p x 16) on v_mfma_f64_16x16x4_f64.  A task is one tile of TR_COLS = 16
// stored columns (the task lists of the single-column GEMV serve); its four wavefronts deal the 64-row chunks of the contraction among
// themselves.  The stored columns are contiguous, the A operand wants lane l to hold column l & 15 at row l >> 4: a wavefront reads 64
// rows of each of its sixteen columns with consecutive lanes (512 contiguous bytes per load), parks them in LDS at a column stride of
// TR_LDT = 66 doubles and reads the operand back from there -- 66 = 2 mod 32: the two 32-lane halves of a ds_read_b64 (lanes of one half:
// column o, rows kk, kk + 1) fall on 32 different 8-byte banks, and the parking stores of consecutive lanes are consecutive.  Nothing of
// the size of a front is staged: 64 rows x 16 columns per wavefront.  Known zeros are skipped per tile at 32-row granularity, as
// k_tr_gemv does per column (a 16-column tile lies inside one 32-column block).
// Every sum has a fixed order: four partial tiles per wavefront (the MFMAs dealt to them in turn), added pairwise, then the four
// wavefronts' tiles added pairwise; children ascending; the residual's entries in stored order.  Two calls give the same bits.
#pragma once
#include "kernels_solve_transpose.hpp"
#include "kernels_vector.hpp"

namespace hipmf {

constexpr int TR_KB = 16;  // right-hand sides per block
constexpr int TR_LDT = 66; // LDS column stride of a wavefront's parked 64 x 16 piece of E / E'
static_assert(TR_KB == 16 && TR_COLS == 16, "the product kernel is written for 16 x 16 MFMA tiles");
static_assert(TR_KB % PERM_CW == 0, "the entry / exit kernels carry PERM_CW columns per thread");

// entry of a block: xp[j + c xstr] = cs[perm[j]] * b[perm[j] + c bstr] for the columns c < ncols whose bit in `mask` is set, zero for the
// other columns up to TR_KB (cs == nullptr: no column scaling).  blockIdx.y = chunk of PERM_CW columns (grid.y = TR_KB / PERM_CW).
__global__ void __launch_bounds__(256) k_tr_perm_in_cols(int32_t n, const int32_t *__restrict__ perm, const double *__restrict__ cs, const double *__restrict__ b,
                                                         int64_t bstr, double *__restrict__ xp, int64_t xstr, uint64_t mask, int32_t ncols) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, c0 = blockIdx.y * PERM_CW;
    if (j >= n) return;
    const uint32_t m = (uint32_t)((mask >> c0) & ((1u << PERM_CW) - 1u));
    const int q = perm[j];
    const double sc = cs ? cs[q] : 1.0;
    double v[PERM_CW];
#pragma unroll
    for (int k = 0; k < PERM_CW; k++) v[k] = (c0 + k < ncols && ((m >> k) & 1u)) ? b[q + (int64_t)(c0 + k) * bstr] : 0.0;
#pragma unroll
    for (int k = 0; k < PERM_CW; k++) xp[j + (int64_t)(c0 + k) * xstr] = (c0 + k < ncols && ((m >> k) & 1u)) ? (cs ? sc * v[k] : v[k]) : 0.0;
}

// forward (U^T) step of a small front for sixteen columns: one wavefront
__global__ void __launch_bounds__(64) k_tr_fwd_small_blk(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD,
                                                         const double *__restrict__ pool, const int32_t *__restrict__ child_idx,
                                                         const int32_t *__restrict__ rel, double *__restrict__ work, double *__restrict__ xp,
                                                         int64_t xstr, int32_t ldu) {
    HIPMF_DYN_SHARED(double, UL); // UL[t * ldu + j] = U(j, t), as k_tr_fwd_small
    __shared__ double w[TR_KB * SMALL_F]; // w[c * SMALL_F + r]
    const int tid = threadIdx.x;
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, f = fd.p + fd.m;
    const double *Ub = fd.epoff >= 0 ? pool + fd.epoff : pool + fd.off;
    const int64_t us = fd.epoff >= 0 ? p : f;
    for (int e = tid; e < p * f; e += 64) {
        const int j = e % p, t = e / p;
        UL[t * ldu + j] = Ub[j + (int64_t)t * us];
    }
#pragma unroll
    for (int c = 0; c < TR_KB; c++) w[c * SMALL_F + tid] = (tid < p) ? xp[fd.first + tid + (int64_t)c * xstr] : 0.0;
    __syncthreads();
    for (int ci = fd.child_begin; ci < fd.child_end; ci++) {
        const FrontDesc cd = FD[child_idx[ci]];
        const double *uc = work + (cd.woff + cd.p) * TR_KB;
        const int32_t *relc = rel + cd.rowptr;
        for (int i = tid; i < cd.m; i += 64) {
            const int r = relc[i];
#pragma unroll
            for (int c = 0; c < TR_KB; c++) w[c * SMALL_F + r] += uc[(int64_t)i * TR_KB + c];
        }
        __syncthreads();
    }
    double v[TR_KB];
#pragma unroll
    for (int c = 0; c < TR_KB; c++) v[c] = (tid < f) ? w[c * SMALL_F + tid] : 0.0;
    for (int j = 0; j < p; j++) {
        const double ujj = UL[j * ldu + j];
        const bool below = tid > j && tid < f;
        const double utj = below ? UL[tid * ldu + j] : 0.0;
#pragma unroll
        for (int c = 0; c < TR_KB; c++) {
            if (tid == j) v[c] = v[c] / ujj;
            const double zj = wave_bcast(v[c], j);
            if (below) v[c] -= utj * zj;
        }
    }
    if (tid < p) {
#pragma unroll
        for (int c = 0; c < TR_KB; c++) xp[fd.first + tid + (int64_t)c * xstr] = v[c];
    } else if (tid < f) {
        double *wo = work + (fd.woff + tid) * TR_KB;
#pragma unroll
        for (int c = 0; c < TR_KB; c++) wo[c] = v[c];
    }
}

// backward (L^T) step of a small front for sixteen columns: one wavefront
__global__ void __launch_bounds__(64) k_tr_bwd_small_blk(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD,
                                                         const double *__restrict__ pool, const int32_t *__restrict__ rows,
                                                         const int32_t *__restrict__ lperm, double *__restrict__ xp, int64_t xstr, int32_t ldl) {
    HIPMF_DYN_SHARED(double, LL); // LL[i * ldl + r] = L(r, i), as k_tr_bwd_small
    __shared__ double xg[TR_KB * SMALL_F]; // xg[c * SMALL_F + r]
    const int tid = threadIdx.x;
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, m = fd.m, f = fd.p + fd.m;
    const double *F = pool + fd.off;
    for (int e = tid; e < p * f; e += 64) {
        const int r = e % f, i = e / f;
        LL[i * ldl + r] = F[r + (int64_t)i * f];
    }
    if (tid < m) {
        const int g = rows[fd.rowptr + tid];
#pragma unroll
        for (int c = 0; c < TR_KB; c++) xg[c * SMALL_F + tid] = xp[g + (int64_t)c * xstr];
    }
    double v[TR_KB];
#pragma unroll
    for (int c = 0; c < TR_KB; c++) v[c] = (tid < p) ? xp[fd.first + tid + (int64_t)c * xstr] : 0.0;
    __syncthreads();
    if (tid < p) {
        double acc[TR_KB];
#pragma unroll
        for (int c = 0; c < TR_KB; c++) acc[c] = 0.0;
        for (int r = 0; r < m; r++) {
            const double l = LL[tid * ldl + p + r];
#pragma unroll
            for (int c = 0; c < TR_KB; c++) acc[c] += l * xg[c * SMALL_F + r];
        }
#pragma unroll
        for (int c = 0; c < TR_KB; c++) v[c] -= acc[c];
    }
    for (int r = p - 1; r > 0; r--) { // unit lower L11: t_r is final once the rows below it are done
        const double lr = (tid < r) ? LL[tid * ldl + r] : 0.0;
#pragma unroll
        for (int c = 0; c < TR_KB; c++) {
            const double tr = wave_bcast(v[c], r);
            if (tid < r) v[c] -= lr * tr;
        }
    }
    if (tid < p) {
        const int64_t d = fd.first + lperm[fd.first + tid];
#pragma unroll
        for (int c = 0; c < TR_KB; c++) xp[d + (int64_t)c * xstr] = v[c];
    }
}

// Rows [rb, rb + 64) of sixteen block columns into the interleaved workspace through an LDS tile: the columns are read along their rows
// (consecutive lanes, consecutive entries -- or the gathered entries of `idx`), the workspace is written a row at a time (128-byte lines).
// src(r) = the entry of xp that is row r of the front's vector, < 0: zero.  Called by all 256 threads.
template <class Src>
__device__ __forceinline__ void tr_rows_to_work(double *tile, double *__restrict__ W, const double *__restrict__ xp, int64_t xstr, int r0, int r1, Src src) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, cc = threadIdx.x & 15, rr = threadIdx.x >> 4;
    for (int rb = r0; rb < r1; rb += 64) {
        const int r = rb + lane;
        const int64_t at = r < r1 ? src(r) : -1;
#pragma unroll
        for (int k = 0; k < TR_KB / 4; k++) {
            const int c = wv + 4 * k;
            tile[c * 65 + lane] = at >= 0 ? xp[at + (int64_t)c * xstr] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int rl = rr + 16 * k;
            if (rb + rl < r1) W[(int64_t)(rb + rl) * TR_KB + cc] = tile[cc * 65 + rl];
        }
        __syncthreads();
    }
}

// forward, big fronts: W = [C1; 0] + children's updates into the workspace, rows [r0, r1) of the front per task, sixteen columns
__global__ void __launch_bounds__(256) k_tr_assemble_blk(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                         const int32_t *__restrict__ child_idx, const int32_t *__restrict__ rel,
                                                         double *__restrict__ work, const double *__restrict__ xp, int64_t xstr) {
    __shared__ double tile[TR_KB * 65];
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    const int p = fd.p, r0 = tk.r0, r1 = tk.r1;
    const int64_t first = fd.first;
    double *W = work + fd.woff * TR_KB;
    tr_rows_to_work(tile, W, xp, xstr, r0, r1, [=](int r) -> int64_t { return r < p ? first + r : -1; });
    const int cc = threadIdx.x & 15, rr = threadIdx.x >> 4;
    for (int ci = fd.child_begin; ci < fd.child_end; ci++) {
        const FrontDesc cd = FD[child_idx[ci]];
        const double *uc = work + (cd.woff + cd.p) * TR_KB;
        const int32_t *relc = rel + cd.rowptr;
        for (int i = rr; i < cd.m; i += 16) { // (rel is injective within a child: no two rows of one child meet)
            const int r = relc[i];
            if (r >= r0 && r < r1) W[(int64_t)r * TR_KB + cc] += uc[(int64_t)i * TR_KB + cc];
        }
        __syncthreads();
    }
}

// backward, big fronts: V = [Z1; X2] into the workspace, rows [r0, r1) per task, sixteen columns
__global__ void __launch_bounds__(256) k_tr_gather_blk(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                       const int32_t *__restrict__ rows, double *__restrict__ work, const double *__restrict__ xp,
                                                       int64_t xstr) {
    __shared__ double tile[TR_KB * 65];
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    const int p = fd.p;
    const int64_t first = fd.first;
    const int32_t *fr = rows + fd.rowptr;
    tr_rows_to_work(tile, work + fd.woff * TR_KB, xp, xstr, tk.r0, tk.r1, [=](int r) -> int64_t { return r < p ? first + r : (int64_t)fr[r - p]; });
}

// Product of a big front for the tile of stored columns [r0, r1) of the task (at most 16, r0 a multiple of 16) and sixteen right-hand
// sides.  FWD: E'^T W1 over the f columns of E' (columns < p give Z1 -> xp, the others are added to the update rows of the workspace);
// else E^T V over the p columns of E (-> xp).
template <bool FWD>
__global__ void __launch_bounds__(256) k_tr_gemm_blk(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                     const double *__restrict__ pool, double *__restrict__ work, double *__restrict__ xp,
                                                     int64_t xstr) {
    __shared__ double T[4 * TR_COLS * TR_LDT]; // per wavefront 16 columns x 64 rows at stride TR_LDT; afterwards the four partial tiles
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    fd_resident(fd);
    const int p = fd.p, f = fd.p + fd.m;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = lane & 15, kk = lane >> 4;
    const int c0 = tk.r0;
    double *V = work + fd.woff * TR_KB;
    const double *M;
    int64_t ldm;
    int i0, i1, ncol;
    if (FWD) { // column c < p of E' (inv(U11)) has rows < 32 (c / 32 + 1) only
        M = pool + fd.epoff, ldm = fd.ldp, ncol = f;
        i0 = 0;
        i1 = c0 < p ? ((c0 / NB + 1) * NB < p ? (c0 / NB + 1) * NB : p) : p;
    } else { // column c of E has rows >= 32 (c / 32) only, unless the pivot rows are a full block
        M = pool + fd.eoff, ldm = fd.ld, ncol = p;
        i0 = (fd.flags & FD_DENSE_TOP) ? 0 : (c0 / NB) * NB;
        i1 = f;
    }
    f64x4 part[4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    double *Tw = T + wv * TR_COLS * TR_LDT;
    for (int ib = i0 + 64 * wv; ib < i1; ib += 256) { // (wave-uniform trip count)
        double a[TR_COLS], b[16];
        const int ra = ib + lane;
#pragma unroll
        for (int u = 0; u < TR_COLS; u++) { // columns past the last one: the last one again, result discarded
            const int cu = c0 + u < ncol ? c0 + u : ncol - 1;
            a[u] = ra < i1 ? M[(int64_t)cu * ldm + ra] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 16; s++) { // rows ib + 4 s .. + 3 of V, sixteen columns: 512 contiguous bytes
            const int rb = ib + 4 * s + kk;
            b[s] = rb < i1 ? V[(int64_t)rb * TR_KB + o] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TR_COLS; u++) Tw[u * TR_LDT + lane] = a[u];
        wave_sync();
#pragma unroll
        for (int s = 0; s < 16; s++) part[s & 3] = mfma_f64_16x16x4(Tw[o * TR_LDT + 4 * s + kk], b[s], part[s & 3]);
        wave_sync();
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; g++) T[wv * 256 + (kk + 4 * g) * 16 + o] = (part[0][g] + part[1][g]) + (part[2][g] + part[3][g]); // [stored column][rhs]
    __syncthreads();
    const int oc = threadIdx.x & 15, j = threadIdx.x >> 4;
    const double t = (T[oc * 16 + j] + T[256 + oc * 16 + j]) + (T[512 + oc * 16 + j] + T[768 + oc * 16 + j]);
    const int c = c0 + oc;
    if (c < p) xp[fd.first + c + (int64_t)j * xstr] = t;
    else if (FWD && c < f) V[(int64_t)c * TR_KB + j] += t; // U = W2 + (E'^T W1): only this thread reads or writes the entry
}

// Residuals of a block in one pass over A^T (tptr / trow / tmap as k_tr_spmv, entries in order): for the columns c < ncols whose bit in
// `mask` is set, r_c = b_c - A^T x_c and, into nrm (zeroed before): nrm[2 c] = max |r_i|, nrm[2 c + 1] = omega_c = max |r_i| / (|A^T||x_c| + |b_c|)_i.
__global__ void __launch_bounds__(256) k_tr_residual_cols(int32_t n, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                          const int32_t *__restrict__ tmap, const double *__restrict__ vals, const double *__restrict__ x,
                                                          int64_t xstr, const double *__restrict__ b, int64_t bstr, double *__restrict__ r, int64_t rstr,
                                                          unsigned long long *nrm, int32_t ncols, uint64_t mask) {
    __shared__ double sr[4 * TR_KB], so[4 * TR_KB];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t m = (uint32_t)(mask & ((ncols < TR_KB ? (1ull << ncols) : (1ull << TR_KB)) - 1ull));
    double acc[TR_KB], d[TR_KB];
#pragma unroll
    for (int c = 0; c < TR_KB; c++) acc[c] = 0.0, d[c] = 0.0;
    if (i < n) {
        for (int k = tptr[i]; k < tptr[i + 1]; k++) {
            const double a = vals[tmap[k]];
            const int64_t j = trow[k];
#pragma unroll
            for (int c = 0; c < TR_KB; c++)
                if ((m >> c) & 1u) {
                    const double t = a * x[j + (int64_t)c * xstr];
                    acc[c] += t;
                    d[c] += fabs(t);
                }
        }
    }
#pragma unroll
    for (int c = 0; c < TR_KB; c++) {
        if (!((m >> c) & 1u)) continue; // (workgroup-uniform)
        double a = 0.0, q = 0.0;
        if (i < n) {
            const double bi = b[i + (int64_t)c * bstr];
            const double ri = bi - acc[c], di = d[c] + fabs(bi);
            r[i + (int64_t)c * rstr] = ri;
            a = fabs(ri);
            q = di > 0.0 ? a / di : (a > 0.0 ? 1.0 : 0.0);
        }
        for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off)), q = fmax(q, __shfl_xor(q, off));
        if (lane == 0) sr[wv * TR_KB + c] = a, so[wv * TR_KB + c] = q;
    }
    __syncthreads();
    if (threadIdx.x < TR_KB && ((m >> threadIdx.x) & 1u)) {
        const int c = threadIdx.x;
        tr_atomic_max(nrm + 2 * c, fmax(fmax(sr[c], sr[TR_KB + c]), fmax(sr[2 * TR_KB + c], sr[3 * TR_KB + c])));
        tr_atomic_max(nrm + 2 * c + 1, fmax(fmax(so[c], so[TR_KB + c]), fmax(so[2 * TR_KB + c], so[3 * TR_KB + c])));
    }
}

} // namespace hipmf
