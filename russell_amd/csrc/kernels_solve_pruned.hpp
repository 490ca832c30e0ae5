// kernels_solve_pruned.hpp -- the ordinary solve A x = b for a BLOCK of SP_KB = 16 SPARSE right-hand sides and / or a few wanted rows of
// x (solver_hipmf_solve_sparse / _device, solver_hipmf_inverse_entries): level-synchronous launches over the MARKED fronts only.
//
// A non-zero at permuted position j touches, in the forward pass, only the fronts on the path from j's front to the root; row i of the
// solution needs, in the backward pass, only the fronts on the path from the root down to i's front.  The host (Solver::solve_sparse,
// numeric.cpp) marks the two sets per block and hands the kernels per-level lists of the marked small fronts and SolveTasks of the
// marked big ones.  Everything outside the sets would compute exact zeros (forward) or values nobody reads (backward).
//
// Layouts (those of kernels_solve_transpose_blocked.hpp)
//   block vector xp   column-major n x 16, column c at xp + c * xstr
//   workspace         the front's f x 16 values interleaved: entry (r, c) of front s at work[(woff + r) * SP_KB + c]; a workspace of the
//                     pruned path's own -- the tagged words of the ordinary solve's workspace are never touched
// A block always carries sixteen columns: k_sp_begin zero-fills the pivot rows of every marked front for all sixteen, k_sp_scatter_in
// writes the non-zeros of the live columns, k_sp_gather_out reads the live columns only.
//
// Children.  A parent adds the update vectors of its MARKED children only (mark[child] == epoch, one word per front, written by
// k_sp_begin for the fronts of the block's forward set; the epoch grows with every block, so nothing is ever cleared): what an
// unmarked child's slot of the workspace holds -- from an earlier block, or nothing at all -- is never read.
//
// Small fronts (f <= SMALL_F): one wavefront per front, the recurrences of k_fwd / k_bwd (kernels_solve.hpp) on sixteen register values,
// the panel staged in dynamic LDS once for the sixteen columns.
// Big fronts: forward  [y1; u - w2] = E w1   (f x p times p x 16),   backward  x1 = E' [y1; x2]   (p x f times f x 16)
// on v_mfma_f64_16x16x4_f64.  E and E' are column-major and the products run along their ROWS: the A operand (lane l holds row l & 15 of
// the tile at contraction index l >> 4) is read straight from memory, sixteen consecutive rows of one stored column per quarter-wave =
// one 128-byte segment -- no transposition through LDS as the transposed kernels need.  The B operand (contraction index l >> 4,
// right-hand side l & 15) is 512 contiguous bytes of the interleaved workspace.  A task is a tile of SP_ROWS = 16 rows; its four
// wavefronts deal the 32-wide chunks of the contraction among themselves, two accumulators each, summed in a fixed order.
// Known zeros are skipped as k_fwd_big / k_bwd_big do: the pivot rows of E right of their own 32-column block (tiled form), the columns
// of inv(U11) left of the tile's 32-column block.
// L D L^T fronts (FD_SYM) have no E': x1 = E^T [D^{-1} y1; x2] is the transposed product k_tr_gemm_blk<false> of
// kernels_solve_transpose_blocked.hpp, launched UNCHANGED on the restricted task list after k_sp_gather_sym has divided the pivot rows by
// D.  k_tr_gather_blk (backward gather of the LU fronts) is reused unchanged as well.  The forward kernels are variants because of the
// marked-children test; the LU backward product is new because the transposed kernels multiply by E'^T, not E'.
// Every sum has a fixed order (marked children ascending, chunks dealt in turn, pairwise sums of the partial tiles): two calls give the
// same bits, and a front's arithmetic does not depend on which other fronts are marked -- the selected rows of a pruned backward pass are
// bit for bit the rows of the full one.
#pragma once
#include "kernels_solve_transpose_blocked.hpp"

namespace hipmf {

constexpr int SP_KB = TR_KB;  // right-hand sides per block
constexpr int SP_ROWS = 16;   // rows of E / E' per product task (one MFMA tile)
constexpr int SP_CHUNK = 32;  // contraction indices per wavefront and turn (eight MFMAs)
static_assert(SP_KB == 16, "the product kernel is written for 16 x 16 MFMA tiles");

// entry ranges of the block's columns in the compressed-column arrays (kernel argument: no device copy of the column pointers)
struct SpCols {
    int32_t ptr[SP_KB + 1];
};

// Start of a block: list[k] = s for a front of the forward set (its mark is set), ~s for a front of the backward set only; the pivot rows
// of either are zeroed in all sixteen columns (the forward pass starts from them, the backward pass reads y1 = 0 where nothing arrived).
__global__ void __launch_bounds__(256) k_sp_begin(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD, int32_t *__restrict__ mark,
                                                  int32_t epoch, double *__restrict__ xp, int64_t xstr) {
    const int e = list[blockIdx.x];
    const int s = e >= 0 ? e : ~e;
    const int p = FD[s].p;
    const int64_t first = FD[s].first;
    if (e >= 0 && threadIdx.x == 0) mark[s] = epoch;
    for (int c = 0; c < SP_KB; c++)
        for (int r = threadIdx.x; r < p; r += 256) xp[first + r + (int64_t)c * xstr] = 0.0;
}

// Compressed columns into the block, one thread per non-zero: xp[ipos[q] + c xstr] = rs[q] * val (q = the row index, c = its column in
// the block; ipos = inverse of the entry permutation, rs = the row scaling -- what k_perm_in does for a dense column).
// ipos == nullptr / rs == nullptr: identity / no scaling (the expansion to a dense block of the fallback).
__global__ void __launch_bounds__(256) k_sp_scatter_in(SpCols cols, int32_t ncols, const int32_t *__restrict__ idx, const double *__restrict__ val,
                                                       const int32_t *__restrict__ ipos, const double *__restrict__ rs, double *__restrict__ xp,
                                                       int64_t xstr) {
    const int e = cols.ptr[0] + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= cols.ptr[ncols]) return;
    int c = 0;
#pragma unroll
    for (int k = 1; k < SP_KB; k++) c += (k < ncols && e >= cols.ptr[k]) ? 1 : 0; // (empty columns share their successor's start)
    const int q = idx[e];
    const int64_t i = ipos ? ipos[q] : q;
    xp[i + (int64_t)c * xstr] = rs ? rs[q] * val[e] : val[e];
}

// Selected rows out of the block, one thread per row: out[k + c ostr] = cs[q] * xp[ipos[q] + c xstr], q = sel[k] (sel == nullptr: q = k);
// ipos = inverse of the exit permutation, cs = the column scaling (nullptr: none) -- the arithmetic of k_perm_out.  ipos == nullptr:
// identity (the row selection of the fallback).  Plain vector stores.
__global__ void __launch_bounds__(256) k_sp_gather_out(int32_t nrows, const int32_t *__restrict__ sel, const int32_t *__restrict__ ipos,
                                                       const double *__restrict__ cs, const double *__restrict__ xp, int64_t xstr,
                                                       double *__restrict__ out, int64_t ostr, int32_t ncols) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrows) return;
    const int q = sel ? sel[k] : k;
    const int64_t j = ipos ? ipos[q] : q;
    const double sc = cs ? cs[q] : 1.0;
    for (int c = 0; c < ncols; c++) {
        const double v = xp[j + (int64_t)c * xstr];
        out[k + (int64_t)c * ostr] = cs ? sc * v : v;
    }
}

// forward (L) step of a marked small front for sixteen columns: one wavefront.  Dynamic LDS: ldp * (the list's largest p) doubles.
__global__ void __launch_bounds__(64) k_sp_fwd_small(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD, const double *__restrict__ pool,
                                                     const int32_t *__restrict__ lperm, const int32_t *__restrict__ child_idx,
                                                     const int32_t *__restrict__ rel, const int32_t *__restrict__ mark, int32_t epoch,
                                                     double *__restrict__ work, double *__restrict__ xp, int64_t xstr, int32_t ldp) {
    HIPMF_DYN_SHARED(double, P); // P[i + j * ldp] = F(i, j), i < f, j < p  (L11 and L21), as k_fwd
    __shared__ double w[SP_KB * SMALL_F]; // w[c * SMALL_F + r]
    const int tid = threadIdx.x;
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, f = fd.p + fd.m;
    const double *F = pool + fd.off;
    if (tid < f)
        for (int j = 0; j < p; j++) P[tid + j * ldp] = F[tid + (int64_t)j * f];
#pragma unroll
    for (int c = 0; c < SP_KB; c++) w[c * SMALL_F + tid] = (tid < p) ? xp[fd.first + tid + (int64_t)c * xstr] : 0.0;
    __syncthreads();
    for (int ci = fd.child_begin; ci < fd.child_end; ci++) {
        const int ch = child_idx[ci];
        if (mark[ch] != epoch) continue; // (workgroup-uniform)
        const FrontDesc cd = FD[ch];
        const double *uc = work + (cd.woff + cd.p) * SP_KB;
        const int32_t *relc = rel + cd.rowptr;
        for (int i = tid; i < cd.m; i += 64) {
            const int r = relc[i];
#pragma unroll
            for (int c = 0; c < SP_KB; c++) w[c * SMALL_F + r] += uc[(int64_t)i * SP_KB + c];
        }
        __syncthreads();
    }
    // row interchanges of the pivot block, then y1 = L11^{-1} (P w1) column by column, u = w2 - L21 y1
    const int src = (tid < p) ? lperm[fd.first + tid] : tid;
    double v[SP_KB];
#pragma unroll
    for (int c = 0; c < SP_KB; c++) v[c] = (tid < f) ? w[c * SMALL_F + src] : 0.0;
    for (int j = 0; j < p; j++) {
        const bool below = tid > j && tid < f;
        const double lj = below ? P[tid + j * ldp] : 0.0;
#pragma unroll
        for (int c = 0; c < SP_KB; c++) {
            const double vj = wave_bcast(v[c], j);
            if (below) v[c] -= lj * vj;
        }
    }
    if (tid < p) {
#pragma unroll
        for (int c = 0; c < SP_KB; c++) xp[fd.first + tid + (int64_t)c * xstr] = v[c];
    } else if (tid < f) {
        double *wo = work + (fd.woff + tid) * SP_KB;
#pragma unroll
        for (int c = 0; c < SP_KB; c++) wo[c] = v[c];
    }
}

// backward (U) step of a marked small front for sixteen columns: one wavefront.  Dynamic LDS: ldu * (the list's largest f) doubles.
__global__ void __launch_bounds__(64) k_sp_bwd_small(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD, const double *__restrict__ pool,
                                                     const int32_t *__restrict__ rows, double *__restrict__ xp, int64_t xstr, int32_t ldu) {
    HIPMF_DYN_SHARED(double, UL); // UL[t * ldu + j] = U(j, t), j < p, t < f  ([U11 | U12], the packed copy when the front has one, as k_bwd)
    __shared__ double xg[SP_KB * SMALL_F]; // x2 gathered from the ancestors: xg[c * SMALL_F + r]
    const int tid = threadIdx.x;
    const FrontDesc fd = FD[list[blockIdx.x]];
    const int p = fd.p, m = fd.m, f = fd.p + fd.m;
    const double *Ub = fd.epoff >= 0 ? pool + fd.epoff : pool + fd.off;
    const int64_t us = fd.epoff >= 0 ? p : f;
    for (int e = tid; e < p * f; e += 64) {
        const int j = e % p, t = e / p;
        UL[t * ldu + j] = Ub[j + (int64_t)t * us];
    }
    if (tid < m) {
        const int g = rows[fd.rowptr + tid];
#pragma unroll
        for (int c = 0; c < SP_KB; c++) xg[c * SMALL_F + tid] = xp[g + (int64_t)c * xstr];
    }
    double v[SP_KB];
#pragma unroll
    for (int c = 0; c < SP_KB; c++) v[c] = (tid < p) ? xp[fd.first + tid + (int64_t)c * xstr] : 0.0;
    __syncthreads();
    if (tid < p) { // t = y1 - U12 x2, columns ascending
        double acc[SP_KB];
#pragma unroll
        for (int c = 0; c < SP_KB; c++) acc[c] = 0.0;
        for (int r = 0; r < m; r++) {
            const double u = UL[(p + r) * ldu + tid];
#pragma unroll
            for (int c = 0; c < SP_KB; c++) acc[c] += u * xg[c * SMALL_F + r];
        }
#pragma unroll
        for (int c = 0; c < SP_KB; c++) v[c] -= acc[c];
    }
    // x1 = U11^{-1} t: columns from right to left, the reciprocal of the lane's own pivot formed once (as k_bwd)
    const double inv_d = (tid < p) ? 1.0 / UL[tid * ldu + tid] : 1.0;
    for (int j = p - 1; j >= 0; j--) {
        const double uj = (tid < j) ? UL[j * ldu + tid] : 0.0;
#pragma unroll
        for (int c = 0; c < SP_KB; c++) {
            if (tid == j) v[c] *= inv_d;
            const double vj = wave_bcast(v[c], j);
            if (tid < j) v[c] -= uj * vj;
        }
    }
    if (tid < p) {
#pragma unroll
        for (int c = 0; c < SP_KB; c++) xp[fd.first + tid + (int64_t)c * xstr] = v[c];
    }
}

// forward, marked big fronts: W = [b1; 0] + the MARKED children's updates into the workspace, rows [r0, r1) of the front per task
// (k_tr_assemble_blk with the mark test)
__global__ void __launch_bounds__(256) k_sp_assemble(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                     const int32_t *__restrict__ child_idx, const int32_t *__restrict__ rel,
                                                     const int32_t *__restrict__ mark, int32_t epoch, double *__restrict__ work,
                                                     const double *__restrict__ xp, int64_t xstr) {
    __shared__ double tile[SP_KB * 65];
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    const int p = fd.p, r0 = tk.r0, r1 = tk.r1;
    const int64_t first = fd.first;
    double *W = work + fd.woff * SP_KB;
    tr_rows_to_work(tile, W, xp, xstr, r0, r1, [=](int r) -> int64_t { return r < p ? first + r : -1; });
    const int cc = threadIdx.x & 15, rr = threadIdx.x >> 4;
    for (int ci = fd.child_begin; ci < fd.child_end; ci++) {
        const int ch = child_idx[ci];
        if (mark[ch] != epoch) continue; // (workgroup-uniform)
        const FrontDesc cd = FD[ch];
        const double *uc = work + (cd.woff + cd.p) * SP_KB;
        const int32_t *relc = rel + cd.rowptr;
        for (int i = rr; i < cd.m; i += 16) { // (rel is injective within a child: no two rows of one child meet)
            const int r = relc[i];
            if (r >= r0 && r < r1) W[(int64_t)r * SP_KB + cc] += uc[(int64_t)i * SP_KB + cc];
        }
        __syncthreads();
    }
}

// backward, marked L D L^T fronts: V = [D^{-1} y1; x2] into the workspace, rows [r0, r1) per task (k_tr_gather_blk + the division)
__global__ void __launch_bounds__(256) k_sp_gather_sym(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
                                                       const int32_t *__restrict__ rows, const double *__restrict__ diag, double *__restrict__ work,
                                                       const double *__restrict__ xp, int64_t xstr) {
    __shared__ double tile[SP_KB * 65];
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    const int p = fd.p;
    const int64_t first = fd.first;
    const int32_t *fr = rows + fd.rowptr;
    double *V = work + fd.woff * SP_KB;
    tr_rows_to_work(tile, V, xp, xstr, tk.r0, tk.r1, [=](int r) -> int64_t { return r < p ? first + r : (int64_t)fr[r - p]; });
    const int cc = threadIdx.x & 15, rr = threadIdx.x >> 4;
    const int re = tk.r1 < p ? tk.r1 : p;
    for (int r = tk.r0 + rr; r < re; r += 16) V[(int64_t)r * SP_KB + cc] = V[(int64_t)r * SP_KB + cc] / diag[first + r];
}

// Product of a marked big front for the tile of rows [r0, r1) of the task (at most 16) and sixteen right-hand sides.
// FWD: E w1 over the p columns of E (rows < p give y1 -> xp, the others are added to the update rows of the workspace);
// else E' [y1; x2] over the f columns of E' (-> xp).
template <bool FWD>
__global__ void __launch_bounds__(256) k_sp_gemm(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD, const double *__restrict__ pool,
                                                 double *__restrict__ work, double *__restrict__ xp, int64_t xstr) {
    __shared__ double T[4 * 256]; // the four wavefronts' partial tiles, [row][rhs]
    const SolveTask tk = tasks[blockIdx.x];
    const FrontDesc fd = FD[tk.s];
    fd_resident(fd);
    const int p = fd.p, f = fd.p + fd.m;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = lane & 15, kk = lane >> 4;
    const int r0 = tk.r0, r1 = tk.r1;
    double *V = work + fd.woff * SP_KB;
    const double *M;
    int64_t ldm;
    int j0, j1;
    if (FWD) { // the pivot rows of E (inv(L11) P) are zero right of their own 32-column block, unless the block is full (k_front)
        M = pool + fd.eoff, ldm = fd.ld;
        j0 = 0, j1 = p;
        if (r1 <= p && !(fd.flags & FD_DENSE_TOP)) j1 = ((r1 - 1) / NB + 1) * NB < p ? ((r1 - 1) / NB + 1) * NB : p;
    } else { // the columns of inv(U11) left of the tile's 32-column block are zero
        M = pool + fd.epoff, ldm = fd.ldp;
        j0 = (r0 / NB) * NB, j1 = f;
    }
    const int row = r0 + o < r1 ? r0 + o : r1 - 1; // (rows past the tile: the last one again, result discarded)
    const double *Mr = M + row;
    f64x4 part[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int jb = j0 + SP_CHUNK * wv; jb < j1; jb += 4 * SP_CHUNK) { // (wave-uniform trip count)
        double a[SP_CHUNK / 4], b[SP_CHUNK / 4];
#pragma unroll
        for (int s = 0; s < SP_CHUNK / 4; s++) {
            const int j = jb + 4 * s + kk;
            const int jc = j < j1 ? j : j1 - 1;
            a[s] = Mr[(int64_t)jc * ldm];
            b[s] = j < j1 ? V[(int64_t)j * SP_KB + o] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < SP_CHUNK / 4; s++) part[s & 1] = mfma_f64_16x16x4(a[s], b[s], part[s & 1]);
    }
#pragma unroll
    for (int g = 0; g < 4; g++) T[wv * 256 + (kk + 4 * g) * 16 + o] = part[0][g] + part[1][g];
    __syncthreads();
    const int oc = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const double t = (T[rl * 16 + oc] + T[256 + rl * 16 + oc]) + (T[512 + rl * 16 + oc] + T[768 + rl * 16 + oc]);
    const int r = r0 + rl;
    if (r >= r1) return;
    if (r < p) xp[fd.first + r + (int64_t)oc * xstr] = t;
    else if (FWD) V[(int64_t)r * SP_KB + oc] += t; // u = w2 + (E w1): only this thread reads or writes the entry
}

} // namespace hipmf
