// kernels_solve_pruned_transpose.hpp -- the transposed solve A^T x = b for a BLOCK of SP_KB = 16 SPARSE right-hand sides and / or a few
// wanted rows of x (solver_hipmf_solve_sparse_transpose / _device, solver_hipmf_inverse_entries_by_rows, the complex twin's trans = 1, 2):
// the level-synchronous launches of kernels_solve_transpose_blocked.hpp over the MARKED fronts only.
//
// The tree is the same and so is the pruning argument of kernels_solve_pruned.hpp: the forward (U^T) pass does something only on the root
// paths of the fronts the non-zeros enter at, the backward (L^T) pass of a wanted row reads its front's ancestors only.  What swaps is the
// side the maps are taken from: a non-zero of row i enters at the inverse of the COLUMN permutation, scaled by cs (k_tr_perm_in_cols), a
// wanted row k leaves from the inverse of the ROW permutation, scaled by rs (k_perm_out_cols) -- k_sp_scatter_in / k_sp_gather_out with
// the other pair of arrays.
//
// Launches per level (Solver::run_pruned_transposed, numeric.cpp)
//   forward   k_spt_fwd_small, k_spt_assemble (new: the marked-children test), k_tr_gemm_blk<true> (E'^T W1, unchanged)
//   backward  k_tr_gather_blk, k_tr_gemm_blk<false> (E^T V), k_tr_bwd_small_blk -- all unchanged: they read ancestors only
// on the pruned path's own workspace and block vector (layouts of kernels_solve_pruned.hpp).  The product tasks of the forward pass are
// tiles of TR_COLS = 16 stored columns of E' over [0, f) that start at 0 (k_tr_gemm_blk wants r0 a multiple of 16), those of the backward
// pass tiles of 16 columns of E over [0, p).
// The sums keep the order of the blocked transposed solve (marked children ascending -- an unmarked child contributes exact zeros
// there --, the substitution as written, the products untouched): a front's arithmetic does not depend on which other fronts are marked.
// An unmarked child's slot of the workspace holds whatever an earlier block left there and is never read.
//
// Complex twin, A^T through the real-equivalent A^H: the imaginary parts (odd rows of the real-equivalent system) are negated on the way
// in and on the way out -- k_spt_conj_in on the block's compressed values before the scatter, k_spt_conj_out on the gathered rows.
// Negation is exact, so where it is applied relative to the scalings does not change a bit.
//
// Speed (profiles/r16_sparse_rhs_transpose.txt: one MI355X, one run per matrix, wall-clock medians) against
// solver_hipmf_solve_transpose_many_device on the expanded block.  1M-DOF 2D matrix: 1 unit column / 1 row 0.861 against 1.140 ms, 16
// columns in a leaf region / 16 rows nearby 0.968 against 3.405 ms, 256 diagonal entries of the inverse by rows 22.77 against 54.48 ms
// (16 x the 16-column solve).  100^3 matrix: 1.943 against 4.884 ms, 2.378 against 10.888 ms, 64.59 against 174.20 ms.  The
// fallback thresholds HIPMF_PRUNE_MAX_SHARE / HIPMF_PRUNE_MIN_BYTES were measured for the ordinary path only (profiles/r09_sparse_rhs.txt)
// and have NOT been measured for A^T.
#pragma once
#include "kernels_solve_pruned.hpp"

namespace hipmf {

// forward (U^T) step of a marked small front for sixteen columns: one wavefront (k_tr_fwd_small_blk with the marked-children test).
// Dynamic LDS: ldu * (the list's largest f) doubles, ldu = (the list's largest p) | 1.
__global__ void __launch_bounds__(64) k_spt_fwd_small(const int32_t *__restrict__ list, const FrontDesc *__restrict__ FD, const double *__restrict__ pool,
                                                      const int32_t *__restrict__ child_idx, const int32_t *__restrict__ rel,
                                                      const int32_t *__restrict__ mark, int32_t epoch, double *__restrict__ work, double *__restrict__ xp,
                                                      int64_t xstr, int32_t ldu) {
    HIPMF_DYN_SHARED(double, UL); // UL[t * ldu + j] = U(j, t), j < p, t < f, as k_tr_fwd_small_blk
    __shared__ double w[SP_KB * SMALL_F]; // w[c * SMALL_F + r]
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
    double v[SP_KB];
#pragma unroll
    for (int c = 0; c < SP_KB; c++) v[c] = (tid < f) ? w[c * SMALL_F + tid] : 0.0;
    for (int j = 0; j < p; j++) {
        const double ujj = UL[j * ldu + j];
        const bool below = tid > j && tid < f;
        const double utj = below ? UL[tid * ldu + j] : 0.0;
#pragma unroll
        for (int c = 0; c < SP_KB; c++) {
            if (tid == j) v[c] = v[c] / ujj;
            const double zj = wave_bcast(v[c], j);
            if (below) v[c] -= utj * zj;
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

// forward, marked big fronts: W = [C1; 0] + the MARKED children's updates into the workspace, rows [r0, r1) of the front per task
// (k_tr_assemble_blk with the mark test; rel is injective within a child: no atomics)
__global__ void __launch_bounds__(256) k_spt_assemble(const SolveTask *__restrict__ tasks, const FrontDesc *__restrict__ FD,
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
        for (int i = rr; i < cd.m; i += 16) {
            const int r = relc[i];
            if (r >= r0 && r < r1) W[(int64_t)r * SP_KB + cc] += uc[(int64_t)i * SP_KB + cc];
        }
        __syncthreads();
    }
}

// complex twin, entry: the values of the block's non-zeros in odd rows (imaginary parts) change sign in place, one thread per non-zero
__global__ void __launch_bounds__(256) k_spt_conj_in(int32_t e0, int32_t e1, const int32_t *__restrict__ idx, double *__restrict__ val) {
    const int e = e0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e < e1 && (idx[e] & 1)) val[e] = -val[e];
}

// complex twin, exit: the gathered rows k whose row index (sel[k], or k when sel == nullptr) is odd change sign, one thread per row
__global__ void __launch_bounds__(256) k_spt_conj_out(int32_t nrows, const int32_t *__restrict__ sel, double *__restrict__ out, int64_t ostr, int32_t ncols) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrows) return;
    const int q = sel ? sel[k] : k;
    if (!(q & 1)) return;
    for (int c = 0; c < ncols; c++) out[k + (int64_t)c * ostr] = -out[k + (int64_t)c * ostr];
}

} // namespace hipmf
