// numeric.hpp -- device-side state and drivers of the multifrontal LU backend (factorize / solve).
#pragma once
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "device_owner.hpp"
#include "symbolic.hpp"
#include "tunables.hpp"

namespace hipmf {

struct FrontDesc;
struct SmallDesc;
struct EaTask;
struct EaRange;
struct SolveTask;
struct SfTask;
struct WtHdr;
struct WtWave;
struct LeafRec;
struct ZeroTask;
struct FactorInfo;

// status codes shared with the reference's C shims (/root/reference/russell_sparse/c_code/constants.h:5-12)
enum : int32_t {
    SUCCESSFUL_EXIT = 0,
    ERROR_NULL_POINTER = 100000,
    ERROR_MALLOC = 200000,
    ERROR_VERSION = 300000,
    ERROR_NOT_AVAILABLE = 400000,
    ERROR_NEED_INITIALIZATION = 500000,
    ERROR_NEED_FACTORIZATION = 600000,
    ERROR_ALREADY_INITIALIZED = 700000,
    // HIP block, analogous to the cuDSS block of constants.h:22-36
    ERROR_HIP_MALLOC = 100,
    ERROR_HIP_MEMCPY = 200,
    ERROR_HIP_SYNCHRONIZE = 300,
    ERROR_HIP_LAUNCH = 350,
    ERROR_HIPMF_INVALID_MATRIX = 600,
    ERROR_HIPMF_SYMBOLIC = 700,
    ERROR_HIPMF_INVALID_VALUE = 803,
    ERROR_HIPMF_COMM = 900,
    ERROR_HIPMF_NO_DEVICE = 1000,
    // numerical status, same value UMFPACK uses for a singular matrix (solver_umfpack.rs:492)
    WARNING_SINGULAR_MATRIX = 1,
    WARNING_NOT_CONVERGED = 2, // solve_updated only: max_steps exhausted (or no further progress) above the tolerance
};

struct NumericOptions {
    int32_t scaling = 1;            // 0 none, 1 sum (UMFPACK_SCALE_SUM), 2 max
    double pivot_epsilon = 1e-13;   // relative to max|scaled a_ij| (cuDSS documents 1e-13 as its f64 default)
    int32_t refinement_nstep = 2;   // UMFPACK's default UMFPACK_IRSTEP is 2
    int32_t matching = 1;           // maximum-product matching + scaling at initialize: 0 never, 1 when the diagonal is weak, 2 always
    double device_memory_factor = 0.0; // > 0: the factor + arena may take at most this share of the device's TOTAL memory (the device limit the
                                    // reference derives from hybrid_memory_factor, interface_cudss.cu:364-372); there is no host spill here: a pool
                                    // beyond the limit is refused by initialize with the out-of-memory status
                                    // (needs the values at initialize; general storage only)
    bool complex_pairs = false;     // the system is the real-equivalent form of a complex matrix (rows / columns 2 k, 2 k + 1 = Re, Im of complex
                                    // row / column k; interface_complex_hipmf.cpp): ordering, matching and pivot searches keep the pairs together,
                                    // and the factorisation leaves the complex pivots for determinant_complex()
    bool verbose = false;
};

struct PhaseTimes {
    double scale_assemble_ms = 0, factor_ms = 0, fwd_ms = 0, bwd_ms = 0, solve_total_ms = 0;
    int64_t n_kernel_launches_factor = 0, n_kernel_launches_solve = 0;
    // accumulated over calls since the last reset (HIP events on the solver's own stream)
    double acc_factor_ms = 0, acc_assemble_ms = 0, acc_fwd_ms = 0, acc_bwd_ms = 0;
    int64_t acc_factor_count = 0, acc_tri_count = 0;
};

struct StepPlan {
    int32_t nactive = 0;
    int64_t pfx_panel = 0, pfx_update = 0; // offsets into d_tasks
    int32_t n_panel = 0, n_update = 0;
    int32_t nfollow = 0; // look-ahead pieces at the head of the update launch (HIPMF_UPD_LA_FIRST=0: none, each is the last task of its front)
    int32_t ppfx[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, upfx[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}; // prefix words of slots 1 .. 3 (kernel arguments of launches with at most four fronts)
    // a full step whose trailing update runs in two launches: the critical strips (first block column / row + look-ahead) on the main
    // stream, the other tiles on a side stream beside the next group's panel steps
    bool split = false;
    bool all_narrow = false; // every active front is inside a group of panels: the update only touches the next panel's strips
    int64_t pfx_crit = 0, pfx_rest = 0;
    int32_t n_crit = 0, n_rest = 0;
};
struct LevelPlan {
    int32_t small_off = 0, small_cnt = 0, small_ld = 0, small_pmax = 1; // fronts with f <= SMALL_F
    int32_t small_cnt_a = 0, small_ld_a = 1;                              // ... the first small_cnt_a of them have f <= small_split
    int32_t big_off = 0, big_cnt = 0;                   // tiled path, sorted by p descending
    int32_t bigfd_off = 0;                              // their descriptors in d_bigfd (slot order)
    int32_t ea_off = 0, ea_cnt = 0;
    int32_t mirror_off = 0, mirror_cnt = 0; // symmetric mode: tiled fronts of the level with a small parent (k_mirror_cb)
    int32_t zero_off = 0, zero_cnt = 0; // zero-fill tasks of the level's working blocks
    int32_t sc_off = 0, sc_cnt = 0;     // entries of A scattered into the level's working blocks
    int32_t fwd_off = 0, fwd_cnt = 0, bwd_off = 0, bwd_cnt = 0; // SolveTask ranges of the big fronts
    int32_t big_pmax = 0, big_fmax = 0;
    bool wide = false; // solve with 32-row slabs x 32 column groups (few large fronts)
    std::vector<StepPlan> steps;
    int64_t pfx_flush = 0;  // k_eflush: prefix of tasks per tiled front (into d_tasks), their total
    int32_t n_flush = 0;
    int32_t upd_ts = 64;    // edge of the trailing-update tiles on this level (32: k_update32, one wave per tile)
    // fronts of the middle of the tree that ONE workgroup carries through their whole partial factorisation (k_front,
    // kernels_factor_front.hpp): their descriptors follow the tiled ones in d_bigfd, grouped by size class
    int32_t mid_off = 0;                 // first of them in d_bigfd
    static constexpr int MID_CLASSES = 6;
    int32_t mid_cnt[MID_CLASSES] = {0, 0, 0, 0, 0, 0}; // fronts per class: 0 .. 2 k_front with 10 / 16 / 24 columns of F12 per wavefront; 3 .. 5 k_front_lu (at most 32 pivots) by the LDS a front needs: up to 40 KB (four workgroups per CU), 80 KB (two), more (one)
    int32_t mid_lds[MID_CLASSES] = {0, 0, 0, 0, 0, 0}; // dynamic LDS of the class's launch, in doubles (its largest front)
    int32_t mid_total() const {
        int32_t t = 0;
        for (int c = 0; c < MID_CLASSES; c++) t += mid_cnt[c];
        return t;
    }
    int64_t chain_off = 0;  // the level's tiled steps as ONE launch (k_chain): its tasks in d_chain, chain_cnt of them (0: one launch per step)
    int32_t chain_cnt = 0;
};

struct ChainTask;

// transposed solves (built at the first one): per level the small fronts and the tasks of the big ones, A^T as CSR through a
// map into d_vals, a workspace of its own (the tagged words of d_work stay as the ordinary pass pair left them)
struct SolverTransposed {
    struct TrLevel {
        int32_t small_off = 0, small_cnt = 0, asm_off = 0, asm_cnt = 0, gf_off = 0, gf_cnt = 0, ga_off = 0, ga_cnt = 0, gb_off = 0, gb_cnt = 0;
        int32_t small_pmax = 1, small_fmax = 1; // largest p / f of the level's small fronts (their LDS panels)
    };
    std::vector<TrLevel> tr_levels;
    bool tr_ready = false;
    DeviceArray<int32_t> d_tr_list, d_ttptr, d_ttrow, d_ttmap;
    // the transposed solve_updated forms (kernels_krylov_transpose.hpp): the rows of A^T cut into blocks of at most KRYT_CAP stored
    // entries, and the partial sums of their residual kernels (2 tt_blocks per column of a block of 16)
    DeviceArray<int32_t> d_ttblk;
    DeviceArray<double> d_tt_part;
    int32_t tt_blocks = 0;
    DeviceArray<SolveTask> d_tr_tasks;
    DeviceArray<double> d_work_t, d_tvec; // d_tvec: six n-vectors (b, x, xp, r, v, z)
    DeviceArray<double> d_anl;            // error analysis: twelve n-vectors + reduction words (allocated at its first option-1/2 call)
    DeviceArray<unsigned long long> d_tnrm;
    PinnedArray<double> h_tnrm;
    // blocked transposed solves (allocated at the first one): the interleaved workspace (16 values per row of every front), four
    // n x 16 block vectors (b, x, xp, r), the norm words of a block (|r|, omega per column)
    bool tr_blk_ready = false;
    DeviceArray<double> d_work_tb, d_tblk;
    DeviceArray<unsigned long long> d_tnrm_blk;
    PinnedArray<double> h_tnrm_blk;
};

// sparse right-hand sides / selected solution rows (built at the first solver_hipmf_solve_sparse; kernels_solve_pruned.hpp): the inverses
// of the entry and exit permutations on both sides, one mark word per front, the block vector and the interleaved workspace of the pruned
// pass pair (its own: the tagged words of d_work stay as the ordinary pass pair left them), and reusable buffers that only grow -- the
// per-level lists of a block, the caller's compressed columns and selection, the staged result, the dense block of the fallback
struct SolverPruned {
    struct SpLevel {
        int32_t small_off = 0, small_cnt = 0, pmax = 1, fmax = 1; // marked small fronts of the level (offsets in ints into the list buffer)
        int32_t va_off = 0, va_cnt = 0;                           // SolveTasks: the big fronts' vectors (assembly forward, gather backward)
        int32_t pr_off = 0, pr_cnt = 0;                           // SolveTasks: their products, SP_ROWS rows each
    };
    // what the product tasks of a list cover: rows [0, p) of E' (backward; also the 16-column tiles of E over [0, p) of the transposed
    // backward pass), rows [0, p) and [p, f) of E (forward: the tiles restart at p), or 16-column tiles of E' over [0, f) from 0
    // (transposed forward: k_tr_gemm_blk wants tile starts that are multiples of 16)
    enum SpShape { SP_BACKWARD = 0, SP_FORWARD = 1, SP_FORWARD_T = 2 };
    template <class T> struct Growing {
        DeviceArray<T> a;
        size_t cap = 0;
        hipError_t need(size_t count) { // (contents are not kept)
            if (count <= cap) return hipSuccess;
            const hipError_t e = a.alloc(count + count / 2 + 64);
            cap = e == hipSuccess ? count + count / 2 + 64 : 0;
            return e;
        }
    };
    bool sp_ready = false;
    std::vector<int32_t> sp_ipos_r, sp_ipos_c; // row q of b enters at permuted position sp_ipos_r[q]; row q of x leaves from sp_ipos_c[q]
    std::vector<int32_t> sp_stamp_f, sp_stamp_b; // per front: the epoch of the block (call) that last marked it forward (backward)
    int32_t sp_epoch = 0;
    double sp_total_pf = 0.0;                  // sum over the fronts of p f: what one pass reads, in entries
    DeviceArray<int32_t> d_sp_ipos_r, d_sp_ipos_c, d_sp_mark;
    DeviceArray<double> d_sp_xp, d_sp_work;
    Growing<int32_t> d_sp_fwd, d_sp_bwd, d_sp_idx, d_sp_sel;
    Growing<double> d_sp_val, d_sp_out, d_sp_dense;
    EventOwner sp_ev0, sp_ev1; // around a call's device work (its time goes to times.solve_total_ms, dstats[8])
};

// solver_hipmf_solve_updated (allocated at its first call; kernels_krylov.hpp): the operator's values (the staging of a factorize, into a
// buffer of their own: d_vals stays what the last factorize left), the two bases of the flexible GMRES, four n-vectors (w, r, x, b; the
// device form uses the caller's x and b), the per-workgroup partial sums, the small device record of a step (both coefficient sets of
// CGS2, the squared norms, the residual's two sums, y) and its pinned mirror
struct SolverUpdated {
    DeviceArray<double> d_up_vals, d_up_V, d_up_Z, d_up_vec, d_up_part, d_up_rec;
    PinnedArray<double> h_up;
    int32_t up_m = 0;       // restart length V and Z are allocated for (0: not allocated)
    int32_t up_rec_m = 0;   // ... and the partial sums, the record and its mirror (always sized for complex coefficients)
    EventOwner up_ev[4];    // HIPMF_UPDATED_TIMING=1: around the pass pair, the SpMV and the Arnoldi kernels of a step
    // solver_hipmf_solve_updated_many (kernels_krylov_blocked.hpp): bases of a block of columns, V[(k C + c) n + i], of their own -- the
    // single form's stay as they are --, four n x C blocks (W, R, X, B; the device form uses the caller's x and b), partial sums per column,
    // the step's record C (2 D k + 2 D + 2), the residuals' 2 C sums and the C D m coefficients of the combine with its pinned mirror, the
    // counts k_c; D = 1 (real coefficients) or 2 (complex_solver_hipmf_solve_updated_many, kernels_krylov_complex_blocked.hpp)
    DeviceArray<double> d_ub_V, d_ub_Z, d_ub_vec, d_ub_part, d_ub_rec;
    DeviceArray<int32_t> d_ub_cnt;
    PinnedArray<double> h_ub;
    PinnedArray<int32_t> h_ub_cnt;
    int32_t ub_m = 0, ub_cols = 0; // restart length and columns the block buffers are allocated for (0: not allocated)
    int32_t ub_d = 0;              // ... and the doubles per coefficient (1 real, 2 complex) the partial sums and the record are sized for
};

// solver_hipmf_solve_extra_precise (allocated at its first call, regrown for a wider block; kernels_refine_extra.hpp): seven n x C blocks
// -- the residual, the correction, the x and tail a step can be taken back from, and the staging of x, tail and b of a host-pointer
// call (the device form works on the caller's) --, the measure slots of a block step and their pinned mirror
struct SolverExtraPrecise {
    DeviceArray<double> d_xr_vec;
    DeviceArray<unsigned long long> d_xr_nrm;
    PinnedArray<double> h_xr_nrm;
    int32_t xr_cols = 0;  // columns the blocks are allocated for (0: not allocated)
    EventOwner xr_ev[4];  // HIPMF_EXTRA_TIMING=1: around the residual, the pass pair and the update of a step
};

// solver_hipmf_set_border / solver_hipmf_solve_bordered (kernels_border.hpp).  The border in force: B, C and W = A^{-1} B packed row-major
// n x kp (kp = k rounded up to a multiple of 16), D, the LU of S = D - C^T W (column-major, leading dimension kp) and its pivots, the
// scratch of the Gram products' partial tiles.  Allocated by set_border, freed by set_border(0) or with the handle; a factorisation
// only clears bd_k and bt_ready (forget_border).  The blocks of solve_bordered are allocated at its first call and regrown for a wider block: five n x C blocks -- the
// residual, the pass pair's result, the x a step can be taken back from, and the staging of x and f of a host-pointer call --, the vectors of order kp of a block, the omegas of a block step and their pinned mirror.
struct SolverBorder {
    int32_t bd_k = 0, bd_kp = 0;   // border columns in force (0: none), and what the arrays are padded to
    bool bd_pairs = false;         // the border of the complex twin (kernels_border_complex.hpp): bd_k = 2 k real-equivalent columns, S, D and the
                                   // vectors of order k interleaved complex numbers, the residual and its omegas on complex moduli
    int32_t bd_chunks = 0;         // partial sums per entry of a Gram product: ceil(n / BORDER_CHUNK)
    int64_t bd_bytes = 0;          // device memory held for the border
    DeviceArray<double> d_bd_B, d_bd_C, d_bd_W, d_bd_D, d_bd_LU, d_bd_part, d_bd_rec;
    DeviceArray<int32_t> d_bd_piv;
    DeviceArray<double> d_bd_vec, d_bd_small;
    DeviceArray<unsigned long long> d_bd_nrm;
    PinnedArray<double> h_bd_nrm;
    int32_t bd_cols = 0, bd_small_kp = 0; // columns and border width the blocks of solve_bordered are allocated for (0: not allocated)
    // The transposed side (solve_bordered_transpose), built at the first transposed call after a set_border and kept until the border
    // is dropped: V = A^{-T} C packed as W is, and D^T packed as D is.  A factorisation clears bt_ready with bd_k.
    DeviceArray<double> d_bt_V, d_bt_Dt;
    DeviceArray<double> d_bt_LU;    // pairs: the LU of S_T = D^H - B^H V, the Schur complement of M^H factorised on its own (bt_prepare) ...
    DeviceArray<int32_t> d_bt_piv;  // ... and its pivots
    bool bt_ready = false;
    int64_t bt_bytes = 0; // device memory held for the transposed side
};

// solver_hipmf_values_outer / _solve_tangent / _solve_adjoint (kernels_sensitivity.hpp).  The inverse maps input -> CSR slots (pointer and
// slot list) that carry a slot gradient to the caller's value order: one for the value map (built at the first mapped call from
// h_seg_ptr / h_seg_idx; set_value_map marks it stale), one for the expansion of a symmetric-lower matrix (from h_emap).  The complex
// twin's pattern (row and column of every stored complex entry) and the inverse of its triplet map come from its interface.  Staging
// that only grows: the slot gradients, the caller-ordered gradient and the operand columns of a host-pointer call, the right-hand
// sides and solutions of a tangent solve, the partial sums its residual kernel writes.
struct SolverSensitivity {
    bool sn_map_ready = false, sn_exp_ready = false;
    DeviceArray<int32_t> d_sn_map_ptr, d_sn_map_idx, d_sn_exp_ptr, d_sn_exp_idx;
    DeviceArray<int32_t> d_sn_zrow, d_sn_zcol, d_sn_zinv_ptr, d_sn_zinv_idx;
    int64_t sn_znnz = 0, sn_znin = 0; // stored complex entries; triplets of the complex value map (0: none installed)
    bool sn_zsym = false;
    SolverPruned::Growing<double> d_sn_slot, d_sn_out, d_sn_ops, d_sn_rhs, d_sn_part;
    EventOwner sn_ev0, sn_ev1; // around the outer and scatter kernels of a call
};

// solver_hipmf_eigs_near_shift / solver_hipmf_get_inertia (kernels_eigs.hpp), allocated at the first call.  The Lanczos basis V
// ((m + 1) x n, its own allocation: the bases of solve_updated stay as they are), three n-vectors (p = M v, w, a staging vector), the
// staged X of a host-pointer call, the per-workgroup slots of the residual, norm and sign kernels, the small device record (the
// coefficients of a step, Y of a rotation, mu, the norms) and its pinned mirror; for the inertia a word per pivot position (0 in a
// small front, -1 in a tiled one), the list of the small fronts and the integer slots of the count.  M's values are staged in d_up_vals.
struct SolverEigs {
    DeviceArray<double> d_eg_V, d_eg_vec, d_eg_X, d_eg_part, d_eg_rec;
    DeviceArray<int32_t> d_eg_idx, d_eg_local, d_eg_small;
    DeviceArray<int64_t> d_eg_cnt;
    PinnedArray<double> h_eg;
    int32_t eg_nsmall = 0;  // small fronts of the plan (entries of d_eg_small)
    int32_t eg_m = 0;       // basis vectors V is allocated for, less one (0: not allocated)
    int32_t eg_xcols = 0;   // columns d_eg_X is allocated for
    bool eg_small = false;  // the slots and the record exist
    EventOwner eg_ev[16];   // around the phases of a step
};

// Everything a Solver holds on the device, and the counts that describe it.  Assigning a fresh instance frees it all and resets the
// counts; members are assigned in declaration order: the transposed-solve state, device memory, pinned memory, the graph and the
// events, the streams.
struct SolverDevice : SolverTransposed, SolverPruned, SolverUpdated, SolverExtraPrecise, SolverBorder, SolverSensitivity, SolverEigs {
    // exported for the many-RHS / multi-GPU paths: the factor lives in [d_pool, d_pool + pool_doubles)
    DeviceArray<double> d_pool;
    DeviceArray<int32_t> d_lperm;
    DeviceArray<double> d_rs;
    DeviceArray<double> d_cs_matched;     // column scaling of the matching ...
    double *d_cs = nullptr;               // ... as the kernels read it (nullptr: none; == d_rs in symmetric mode)
    DeviceArray<int32_t> d_rperm_matched; // row of A that is row i of the permuted system, under a matching ...
    int32_t *d_rperm = nullptr;           // ... as the kernels read it (== d_perm without matching)
    DeviceArray<int32_t> d_dcol; // column of the (matched) diagonal entry of every row of A (nullptr: identity)
    DeviceArray<LeafRec> d_leaf;   // records of the leaves: forward part, then backward part (other panel offsets)
    int32_t leaf_cnt = 0;
    int64_t split_units = 0;       // 256-double units of the scratch of partial sums
    int64_t split_slabs = 0;
    DeviceArray<double> d_split_scr;
    DeviceArray<int32_t> d_split_cnt; // one arrival counter per unit (the first unit of a slab's group is used; reset by the last arriver)
    DeviceArray<SfTask> d_sfk;
    DeviceArray<int32_t> d_needk;
    DeviceArray<SfTask> d_sf3;   // tasks of the level-by-level launches of the dependency-driven kernels (fallback of L D L^T / very large fronts)
    DeviceArray<int32_t> d_need3;
    DeviceArray<FrontDesc> d_fd;
    DeviceArray<FrontDesc> d_bigfd; // copies of the tiled fronts' descriptors, level by level in slot order
    DeviceArray<EaTask> d_ea;
    DeviceArray<EaRange> d_ear;
    DeviceArray<double> d_dws; // factorised diagonal tiles of the current tiled step, one per active big front
    DeviceArray<SolveTask> d_st;
    DeviceArray<SfTask> d_sf; // dependency-driven solve (kernels_solve_fused.hpp): one launch per direction
    DeviceArray<WtHdr> d_wt_hdr;              // batch headers: forward part, then backward part
    DeviceArray<int32_t> d_wt_meta;           // meta blocks of the batches (records + index lists): forward part, then backward part
    DeviceArray<WtWave> d_wt_wave;            // batch range and first pivot column of every wave-subtree: forward part, then backward part
    int32_t wt_waves = 0, wt_recs = 0;        // wave-subtrees, fronts they hold
    DeviceArray<SfTask> d_sf2;                // tasks of the fronts above the wave-subtrees: forward, then backward
    int32_t sf2_fwd_cnt = 0, sf2_bwd_cnt = 0;
    DeviceArray<int32_t> d_rep_idx;           // per front: index of its "complete" replicas (tiled fronts of the top levels), else -1
    DeviceArray<int32_t> d_rep;               // the replicas: forward part, then backward part (zeroed before every pass)
    int64_t rep_words = 0;
    DeviceArray<int32_t> d_need2;             // completed-task counts of that list (the slabs are cut differently)
    DeviceArray<int32_t> d_need;              // completed-task counts that mark a front as done: [0, ns) forward, [ns, 2 ns) backward
    DeviceArray<int32_t> d_sync;              // 2 x (SF_SYNC_HEADER + ns) ints: ticket, error word, counters; zeroed before every pass
    DeviceArray<ChainTask> d_chain;           // ChainTask records of all chained levels
    DeviceArray<int32_t> d_chain_cnt;         // their counters (3 per front and step) + the error word (last); zeroed before every factorisation
    int64_t chain_words = 0;
    // fused assembly of the small fronts (k_small_factor) and zero-fill of the big ones only
    DeviceArray<int32_t> d_sa_ptr, d_sa_k;
    DeviceArray<uint16_t> d_sa_pos;
    DeviceArray<ZeroTask> d_zero;
    DeviceArray<double> d_vs, d_vs2; // scaled values (and the mirrored ones of symmetric-lower storage)
    int32_t zero_cnt = 0;
    DeviceArray<int32_t> d_seg_ptr, d_seg_idx; // value map (set_value_map)
    DeviceArray<int32_t> d_emap;      // expansion of symmetric-lower values to the analysed general storage (set_expansion)
    DeviceArray<double> d_vlow;       // staging of the caller's lower-triangle values
    int64_t nnz_low = 0;
    DeviceArray<double> d_vin;
    int64_t nnz_in = 0;
    DeviceArray<SmallDesc> d_sd;      // per position of d_lists: descriptor + entry range of a small front
    DeviceArray<double> d_blk, d_work_blk; // many-RHS blocks (allocated at the first multi-column solve)
    DeviceArray<unsigned long long> d_norms_blk; // norm slots of lane 0's blocked solves (block_cols * block_groups columns)
    int32_t block_cols = 0;    // columns per block of the many-RHS driver once its buffers exist (8 or 16; HIPMF_BLOCK_COLS forces one)
    int32_t block_groups = 0;  // blocks ("groups", kernels_solve_fused.hpp SfGroups) a dependency-driven launch of the many-RHS driver carries once its
                               // buffers exist (1 .. SF_GMAX); block_cols * block_groups columns travel together
    DeviceArray<unsigned long long> d_trace;  // HIPMF_SF_TRACE=<file>: device-clock stamps of the upper tasks (profiling aid)
    DeviceArray<FactorInfo> d_info;
    DeviceArray<unsigned long long> d_scalar; // [0] anorm bits, [4 ...] the norm slots of k_residual (lane 0)
    DeviceArray<double> d_work, d_vals, d_xp, d_r, d_den, d_b, d_x, d_du;
    DeviceArray<int32_t> d_rows, d_rel, d_child, d_lists, d_tasks;
    DeviceArray<int32_t> d_rp, d_ci, d_arow, d_tptr, d_tidx, d_perm;
    DeviceArray<int32_t> d_ea_sc;   // k_extend_add_lds: per task, the range of its entries of A in d_sc_k / d_sc_pos (cumulative, all levels)
    DeviceArray<uint16_t> d_sc_pos; // ... position inside the task's tile
    DeviceArray<int32_t> d_sc_k;    // scatter lists of the tiled fronts, by level: input entry k (or ~k: mirrored copy) ...
    DeviceArray<int64_t> d_sc_at;   // ... and the pool offset it goes to
    DeviceArray<double> d_diag;     // pivots in pivot order (determinant, rcond, D of the symmetric fronts)
    DeviceArray<int32_t> d_row_blk; // row blocks of the stream SpMV (k_spmv_stream)
    // further lanes of the solve driver (allocated at the first solve with more than one block): stream, block buffers, hand-off
    // words, norms; lane 0 is the solver's own stream and buffers
    struct LaneBuffers {
        StreamOwner stream;
        DeviceArray<double> blk, work;
        DeviceArray<int32_t> sync;
        DeviceArray<unsigned long long> norms;
    };
    std::vector<LaneBuffers> extra_lanes;
    PinnedArray<double> h_nrm;   // pinned: norms of every lane
    PinnedArray<double> h_stage; // pinned: rhs | x of a single host-pointer solve
#ifndef HIPMF_EMULATED
    GraphExecOwner factor_graph; // the launches of a factorisation's levels, captured once and replayed (use_graph)
#endif
    int64_t graph_launches = 0;
    EventOwner ev[8];
    EventOwner ev_fork, ev_join;
    EventOwner ev_pb, ev_rest;
    EventOwner ev_pre0, ev_pre1; // the work before the first level that only the big fronts need (zero-fill of E / E', identity blocks, diagonal check) runs on stream4 beside the levels of small fronts
    EventOwner ev_fork3, ev_join3;
    StreamOwner stream;
    StreamOwner stream2; // the small fronts of a level are factorised beside its tiled steps
    StreamOwner stream3; // ... and so are the fronts one workgroup factorises (k_front)
    StreamOwner stream4; // ... and the bulk of a split trailing update (HIPMF_UPD_SPLIT)
};

// The Tunables base is the EFFECTIVE set of knobs of the current analysis: initialize_impl() starts it from `requested` and adjusts it for
// the matrix (complex pairs, plan-dependent defaults); the run-time fallbacks (a hand-off time-out, a failed graph capture) write it
// alone, so they last for ONE analysis.  Like SolverDevice, assigning a fresh instance resets everything.
class Solver : public SolverDevice, public Tunables {
  public:
    Solver();
    Tunables requested; // what the environment asked for at the last initialize() call: assigned there and nowhere else
    ~Solver();
    int32_t initialize(int32_t n, const int32_t *rp, const int32_t *ci, bool sym_lower, const SymbolicOptions &sopt,
                       const NumericOptions &nopt, const double *values = nullptr);
    // values: nnz doubles in the CSR order given to initialize; on_device tells where they live
    int32_t factorize(const double *values, bool on_device);
    // value refresh through a map: CSR entry j = sum of input[seg_idx[seg_ptr[j] .. seg_ptr[j + 1])]
    // signed_map: seg_ptr[nnz] map entries (any number), an index ~k subtracts input[k]
    int32_t set_value_map(int64_t nnz_in, const int32_t *seg_ptr, const int32_t *seg_idx, bool signed_map = false);
    int32_t factorize_mapped(const double *input, bool on_device);
    int32_t solve(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device);
    int32_t solve_core(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device); // the driver of solve(): triangular passes + refinement
    // the operator pair of the Krylov rescue (host vectors): precond z = M^{-1} v, apply w = Op z; nullptr: the factorisation and A
    struct KrylovOps {
        std::function<int32_t(double *, const double *)> precond, apply;
    };
    int32_t krylov_rescue(double *x, const double *rhs, bool on_device, const KrylovOps *ops = nullptr); // see numeric.cpp
    // Transposed solves A^T x = b on the stored factor (level-synchronous launches, kernels_solve_transpose.hpp), refined and rescued by the
    // rules of solve(); conj_pairs: interleaved complex pairs whose imaginary parts are negated on the way in and out (the complex twin's
    // A^T through the real-equivalent A^H).  L D L^T / symmetric storage: A^T = A, the ordinary solve.
    int32_t solve_transpose(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device, bool conj_pairs = false);
    // The same for many columns, 16 at a time through the blocked kernels (kernels_solve_transpose_blocked.hpp): every factor entry is read
    // once per block.  One column, A^T = A or no memory for the block buffers: solve_transpose.
    // conj_pairs: as in solve_transpose, the staged columns of every block conjugated on entry and exit (k_tr_conj_cols)
    int32_t solve_transpose_many(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device, bool conj_pairs = false);
    int64_t transposed_blocks = 0;   // 16-column blocks the last solve_transpose_many ran through the blocked kernels (0: it went to solve_transpose)
    // MUMPS-style error analysis of a solution xbar of A x = b (host vectors; option 1: all eight values, 2: entries 0 - 4), see numeric.cpp
    int32_t error_analysis(const double *xbar, const double *rhs, double *out, int32_t option);
    // the same for the complex twin: this handle holds the real-equivalent system of order 2 nc, xbar / rhs are interleaved complex vectors
    // (kernels_error_analysis_complex.hpp; the caller has checked the pairing of the even rows), see numeric.cpp
    int32_t error_analysis_complex(const double *xbar, const double *rhs, double *out, int32_t option);
    int32_t download_pattern(std::vector<int32_t> &rp, std::vector<int32_t> &ci); // host copies of the stored CSR pattern of A
    // Sparse right-hand sides and selected rows: x_sel(k, c) = (A^{-1} B)(sel_idx[k], c) for B (n x nrhs) in compressed-column form, 16
    // columns per block through the pruned level-synchronous launches of kernels_solve_pruned.hpp -- one UNREFINED pass pair over the
    // marked fronts.  sel_idx == nullptr: all n rows.  Blocks whose marked fronts read more than HIPMF_PRUNE_MAX_SHARE of what a full pass
    // pair reads, and every block of a factor with replaced pivots, go through solve() on the expanded columns.  on_device: every array
    // but the handle's own lives on the device.  See numeric.cpp.
    // transposed: A^T in place of A through the pruned transposed launches of kernels_solve_pruned_transpose.hpp (L D L^T / symmetric
    // storage: A^T = A, the ordinary path and its bits); its fallback is solve_transpose_many on the expanded columns.  The two thresholds
    // were measured for the ordinary path only.  conj_pairs (with transposed, host arrays): interleaved complex pairs whose imaginary
    // parts -- the odd rows -- are negated on the way in and out (the complex twin's A^T through the real-equivalent A^H).
    int32_t solve_sparse(double *x_sel, int64_t ldx, int32_t nrhs, const int32_t *rhs_ptr, const int32_t *rhs_idx, const double *rhs_val, int32_t nsel,
                         const int32_t *sel_idx, bool on_device, bool accumulate = false, bool transposed = false, bool conj_pairs = false);
    // values[e] = (A^{-1})(rows[e], cols[e]) (host arrays): blocks of at most 16 distinct columns, neighbours in the elimination order together.
    // by_rows: blocks of at most 16 distinct ROWS as unit right-hand sides of the transposed pruned solve ((A^{-1})(r, c) = (A^{-T})(c, r)),
    // the columns asked for in a block its selection.  pairs: this handle holds the real-equivalent system of a complex matrix of order
    // n / 2; rows / cols index the complex matrix, values are interleaved (re, im) -- unit column c is real column 2 c, row r rows 2 r, 2 r + 1.
    int32_t inverse_entries(int32_t nent, const int32_t *rows, const int32_t *cols, double *values, bool by_rows = false, bool pairs = false);
    int64_t pruned_transposed_blocks = 0;                 // blocks of the last such call that ran the transposed pruned kernels
    int64_t pruned_fwd_fronts = 0, pruned_bwd_fronts = 0; // fronts the forward / backward pass of the last pruned block visited
    int64_t pruned_blocks = 0;                            // blocks of the last solve_sparse / inverse_entries that ran pruned
    int64_t pruned_bytes = 0;                             // 8 x the factor entries (p f per front and pass) those fronts hold
    double pruned_call_ms = 0.0;                          // HIP-event time of the last solve_sparse / inverse_entries (also times.solve_total_ms)
    double pruned_share_last = 0.0;                       // share of a full pass pair's factor entries the last block's marked fronts read
    // A x = rhs for the matrix with the structure of initialize and the values given HERE, by right-preconditioned flexible GMRES with
    // the kept factor as preconditioner; bases, Gram-Schmidt (CGS2) and residuals on the device, the Hessenberg least-squares problem on
    // the host.  values: CSR order of the caller (mapped = false) or the inputs of the installed value map (mapped = true); on_device:
    // x, rhs and values are device pointers.  Returns SUCCESSFUL_EXIT (converged) or WARNING_NOT_CONVERGED.  d_vals, the factor and the
    // statistics of the ordinary solves are left as they were.  See numeric.cpp.
    // transposed: A_new^T x = rhs -- the same iteration with A_new^T as operator (kernels_krylov_transpose.hpp) and the unrefined
    // transposed pass pair of the kept factor as preconditioner; the statistics of the transposed solves stay as they were too.  A^T = A
    // (L D L^T fronts, symmetric storage): the plain form and its bits.
    int32_t solve_updated(double *x, const double *rhs, const double *values, bool mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres,
                          bool on_device, bool transposed = false);
    int64_t updated_steps = 0, updated_cycles = 0; // of the last solve_updated
    int64_t updated_basis_bytes() const { return up_m > 0 ? (int64_t)(2 * (int64_t)up_m + 1) * S.n * 8 : 0; }
    double updated_ms[3] = {0.0, 0.0, 0.0}; // HIPMF_UPDATED_TIMING=1: HIP-event time of the last call's pass pairs, SpMVs, Arnoldi kernels
    // The same for nrhs columns (x, rhs: column-major ld x nrhs) in blocks of KRYB_COLS = 16: every column runs its own flexible GMRES, the
    // columns of a block share the blocked pass pair, one pass over the matrix and the launches of a step.  steps / relres: nrhs entries on
    // the host or nullptr.  SUCCESSFUL_EXIT when every column converged, else WARNING_NOT_CONVERGED.  nrhs == 1 is solve_updated.  After
    // the call updated_steps counts blocked pass pairs and updated_cycles the cycles, both summed over the blocks.
    int32_t solve_updated_many(double *x, const double *rhs, int32_t nrhs, int64_t ld, const double *values, bool mapped, double rel_tol, int32_t max_steps,
                               int32_t *steps, double *relres, bool on_device, bool transposed = false);
    // The single form for the real-equivalent system of a COMPLEX matrix (S.n = 2 nc, vectors of interleaved (re, im) pairs; the
    // complex C-ABI): the same iteration in complex arithmetic -- <v, w> = sum conj(v_i) w_i, complex Hessenberg matrix and rotations
    // (kernels_krylov_complex.hpp) -- on the same bases and vectors.  values: always the inputs of the installed (signed) value map.
    // transposed: the transposed real-equivalent system, A_new^H z = c; with conj_pairs A_new^T z = c -- the same iteration on conjugated
    // data (the imaginary parts of c negated on entry, those of z on exit; steps and relres are those of the A^H iteration on conj(c)).
    int32_t solve_updated_complex(double *x, const double *rhs, const double *values, double rel_tol, int32_t max_steps, int32_t *steps, double *relres,
                                  bool on_device, bool transposed = false, bool conj_pairs = false);
    bool updated_complex = false; // the last solve_updated_complex orthogonalised in complex arithmetic (false before the first)
    // solve_updated_many for that system (the complex C-ABI): x, rhs column-major with ld DOUBLES (even, >= S.n) between columns; every
    // column its own flexible GMRES in complex arithmetic (kernels_krylov_complex_blocked.hpp).  nrhs == 1 is solve_updated_complex.
    int32_t solve_updated_many_complex(double *x, const double *rhs, int32_t nrhs, int64_t ld, const double *values, double rel_tol, int32_t max_steps, int32_t *steps,
                                       double *relres, bool on_device, bool transposed = false, bool conj_pairs = false);
    int64_t updated_blocks = 0, updated_column_steps = 0; // of the last solve_updated_many: 16-column blocks (0: single form), sum of the columns' steps
    // Extra-precise iterative refinement of A x = rhs on the kept factor (A: the values of the last factorize): per column x <- one
    // unrefined pass pair, then steps r = b - A (x + tail) in twice the working precision (kernels_refine_extra.hpp), dx = one unrefined
    // pass pair of r, x (and tail) updated, until dn = |dx|_inf / |x|_inf <= dx_tol (<= 0: eps), a step fails to halve dn, or max_steps
    // (<= 0: 10).  x, tail (nullptr: none carried), rhs: column-major ld x nrhs, blocks of 16 columns per pass pair; pairs: interleaved
    // complex vectors, the measures on moduli.  info: 8 doubles per column on the host (nullptr allowed), see include/russell_hipmf.h.
    // SUCCESSFUL_EXIT when every column converged, else WARNING_NOT_CONVERGED (x: the best iterate).  The factor, d_vals and the
    // statistics of the ordinary solves are left as they were.  See numeric.cpp.
    int32_t solve_extra_precise(double *x, double *tail, const double *rhs, int32_t nrhs, int64_t ld, double dx_tol, int32_t max_steps, double *info, bool on_device,
                                bool pairs = false);
    int64_t extra_steps = 0, extra_blocks = 0; // of the last solve_extra_precise: pass pairs after the first summed over the block steps, 16-column blocks
    double extra_ms[3] = {0.0, 0.0, 0.0};      // HIPMF_EXTRA_TIMING=1: HIP-event time of the last call's residuals, correction pass pairs, updates
    // The bordered system [A B; C^T D] [x; z] = [f; g] on the kept factor (kernels_border.hpp; B, C: column-major n x k, D: k x k).
    // set_border copies the border to the device, computes W = A^{-1} B with solve() in blocks of 16 columns, S = D - C^T W and its LU
    // with partial pivoting in one workgroup; info (nullptr allowed): min / max |u_ii| of S, det S as mantissa and base-10 exponent,
    // bytes held.  k == 0 frees the border.  WARNING_SINGULAR_MATRIX for an exactly zero pivot of S: no border is left set.
    // Every factorisation drops the border (forget_border).
    // pairs (the complex twin, kernels_border_complex.hpp): this handle holds the real-equivalent system of a complex matrix; k counts
    // COMPLEX columns (<= ZBORDER_MAX), B, C, D are interleaved complex arrays with ldb, ldc, ldd in doubles, C^T is the plain transpose,
    // and info takes five doubles: min / max |u_ii| of the complex LU of S, real and imaginary mantissa and exponent of det S, bytes.
    int32_t set_border(int32_t k, const double *B, int64_t ldb, const double *C, int64_t ldc, const double *D, int64_t ldd, double *info, bool on_device,
                       bool pairs = false);
    // Block elimination refined on the whole system, per block of 16 columns: y = one unrefined pass pair of f, t = g - C^T y,
    // z = S^{-1} t, x = y - W z; then steps on the residual (f - A x - B z, g - C^T x - D z) by the stopping rule of solve() on the
    // componentwise backward error omega over all n + k rows, at most max_steps (<= 0: 4).  x, f: column-major ldx x nrhs; z, g:
    // ldz x nrhs (nullptr: z is not returned, g = 0).  info: 4 doubles per column on the host (steps, omega, omega before the first
    // step, state 0 converged / 1 no progress / 2 step limit).  The factor, d_vals and the statistics of the ordinary solves are
    // left as they were.  See numeric.cpp.
    int32_t solve_bordered(double *x, double *z, const double *f, const double *g, int32_t nrhs, int64_t ldx, int64_t ldz, int32_t max_steps, double *info,
                           bool on_device);
    // The transposed system [A^T C; B^T D^T] [y; w] = [p; q] with the border in force: the same loop with V = A^{-T} C for W, the
    // transposed pass pair for the plain one, S^T = D^T - B^T V through the LU of S (U^T, L^T, the exchanges backwards), and the
    // residual over the rows of M^T.  Arguments, info and status codes as solve_bordered.  V and the packed D^T are built at the first
    // call after a set_border (bt_prepare); counters 44 - 46 and the statistics of every other solve are left as they were.
    // With a border set in pairs mode the system is M^H [y; w] = [p; q], M^H = [A^H conj(C); B^H D^H] (the transposed real-equivalent
    // system); conj_pairs: M^T instead -- the same loop on conjugated data, staged on the device, conjugated back on the way out.
    int32_t solve_bordered_transpose(double *y, double *w, const double *p, const double *q, int32_t nrhs, int64_t ldx, int64_t ldz, int32_t max_steps, double *info,
                                     bool on_device, bool conj_pairs = false);
    void drop_border(); // frees the border's device memory
    void forget_border() { bd_k = 0, bt_ready = false; } // a new factor: the border and what was built from it are no longer valid
    int64_t bordered_steps = 0, bordered_blocks = 0; // of the last solve_bordered: block steps summed over the blocks, 16-column blocks
    int64_t bordered_t_steps = 0, bordered_t_blocks = 0; // the same of the last solve_bordered_transpose
    // Sensitivities with respect to the matrix values (kernels_sensitivity.hpp).  The pattern-restricted outer product
    //   grad = beta grad + alpha sum_c u_c w_c^T |pattern
    // in the order of the values the caller hands to factorize (mapped = false: its CSR order, a symmetric-lower handle its lower
    // triangle, also when the handle expanded it) or to factorize_mapped (mapped = true: the inputs of the value map).  u, w:
    // column-major ldu x ncols, ldw x ncols.  Needs initialize only.  One fixed chain of fma per entry: the same bits from host and
    // device pointers, from call to call and on every device.
    int32_t values_outer(double *grad, const double *u, const double *w, int32_t ncols, int64_t ldu, int64_t ldw, double alpha, double beta, bool mapped,
                         bool on_device);
    // dx = A^{-1} (db - dA x) for the matrix dA that dvalues describe (values / mapped as above; db nullptr: zero): dvalues are staged
    // in the operator's value buffer of the solve_updated forms, the right-hand sides come from their blocked residual kernel, the
    // solve is solve() with the handle's refinement.  d_vals, the factor and the statistics of the ordinary solves stay as they were.
    int32_t solve_tangent(double *dx, const double *x, const double *dvalues, const double *db, int32_t nrhs, int64_t ld, bool mapped, bool on_device);
    // lambda = A^{-T} g by solve_transpose_many (A^T = A: solve), then grad = beta grad - sum_c lambda_c x_c^T |pattern by ONE
    // values_outer over all nrhs columns (grad nullptr: only the solve).  lambda may be g.  symmetric_matrix: a symmetric matrix that
    // the interface expanded to general storage (A^T = A).  The statistics of the ordinary and of the transposed solves stay as they were.
    int32_t solve_adjoint(double *lambda, double *grad, const double *x, const double *g, int32_t nrhs, int64_t ld, double beta, bool mapped, bool on_device,
                          bool symmetric_matrix = false);
    // The complex twin (this handle holds the real-equivalent system of order 2 nc; host pointers, interleaved (re, im)):
    // set_complex_pattern: row and column of every stored complex entry (sym: the lower triangle of a complex-symmetric matrix);
    // set_complex_value_map: the inverse of the triplet map, triplet -> stored entries (nin = 0: none, the values are the stored entries)
    int32_t set_complex_pattern(int64_t nnzc, const std::vector<int32_t> &zrow, const std::vector<int32_t> &zcol, bool sym);
    int32_t set_complex_value_map(int64_t nin, const std::vector<int32_t> &inv_ptr, const std::vector<int32_t> &inv_idx);
    bool complex_pattern_set() const { return sn_znnz > 0; }
    // grad = beta grad + alpha sum_c u_c op(w_c)^T |pattern on complex entries, op = conj with conjugate_w; ldu, ldw in complex elements
    int32_t values_outer_complex(double *grad, const double *u, const double *w, int32_t ncols, int64_t ldu, int64_t ldw, double alpha, double beta,
                                 bool conjugate_w);
    // The inertia of the factorised matrix from the signs of the pivots (Sylvester's law; kernels_eigs.hpp).  Needs the L D L^T plan
    // (S.sym_mode; else ERROR_NOT_AVAILABLE).  The fronts one wavefront factorises in LDS (k_small_factor) search their pivot block also
    // on a symmetric handle: where one moved a row, the inertia of its pivot block is counted from the product of its factors instead
    // (inertia_fronts_recounted tells how many).  The symmetric scaling S A S and the symmetric permutation are congruences and leave
    // the inertia alone.  Replaced and zero pivots are counted in n_zero and make the call return WARNING_SINGULAR_MATRIX.
    int32_t inertia(int64_t *n_positive, int64_t *n_negative, int64_t *n_zero);
    int64_t inertia_fronts_recounted = 0; // small fronts of the last inertia() whose pivot search had moved a row
    // The nev eigenpairs of K x = lambda M x nearest sigma, the handle holding the factor of A = K - sigma M: thick-restart Lanczos on
    // A^{-1} M in the M-inner product, everything of length n on the device (kernels_eigs.hpp; see numeric.cpp).  m_values: M on the
    // handle's pattern as solve_updated takes values (nullptr: M = I); v0: start vector or nullptr; X: column-major ldx x nev;
    // lambda, backward_error (nev each), nconv, steps: on the host.  symmetric_matrix: the interface expanded a symmetric matrix to
    // general storage.  SUCCESSFUL_EXIT or WARNING_NOT_CONVERGED.  The factor, d_vals, the border and every statistic stay as they were.
    int32_t eigs_near_shift(int32_t nev, int32_t ncv, double sigma, const double *m_values, bool mapped, const double *v0, double tol, int32_t max_steps,
                            double *lambda, double *X, int64_t ldx, double *backward_error, int32_t *nconv, int32_t *steps, bool on_device,
                            bool symmetric_matrix = false);
    int64_t eigs_steps = 0, eigs_restarts = 0, eigs_converged = 0; // of the last eigs_near_shift: operator applications, restarts, converged pairs
    int64_t eigs_basis_bytes() const { return eg_m > 0 ? ((int64_t)eg_m + 1) * S.n * 8 : 0; }
    double eigs_ms[4] = {0.0, 0.0, 0.0, 0.0}; // HIP-event time of the last call's solves, SpMVs, orthogonalisation kernels, rotations
    int64_t sens_outer_columns = 0; // columns summed by the outer products of this handle, over all calls
    double sens_outer_ms = 0.0;     // HIP-event time of the outer and scatter kernels of the last such call
    int64_t updated_block_basis_bytes() const { return ub_m > 0 ? (int64_t)(2 * (int64_t)ub_m + 1) * ub_cols * S.n * 8 : 0; }
    int64_t transposed_solves = 0;   // solve_transpose calls that solved (columns)
    int64_t analysis_solves = 0;     // pass pairs of the last error analysis (condition estimates)
    int64_t krylov_iterations_t = 0; // FGMRES steps of the last transposed solve (krylov_iterations / krylov_last_relres stay the ordinary solve's)
    double last_omega_t = 0.0;       // omega of the last transposed solve (first column)
    int32_t refinement_steps_done_t = 0;
    int32_t singular_verdict();      // exactly zero pivots were met: singular (status 1), or only an unlucky static order (0)?  One probe solve decides
    int64_t zero_pivots_absorbed = 0; // exactly zero pivots of factorisations that the probe solve found NOT singular (summed)
    bool in_rescue = false;
    int32_t krylov_cycles = 4;       // restarts at most
    std::vector<double> col_omega;   // per column of the last solve: omega of its final solution as the refinement measured it
    int64_t krylov_iterations = 0;   // FGMRES steps of the last solve (0: no rescue ran or was needed)
    double krylov_last_relres = 0.0; // |b - A x|_2 / |b|_2 after the last rescue
    int32_t prepare_many(int32_t nrhs); // the block buffers of a later many-RHS solve, ahead of time
    int32_t spmv(double *y, const double *x, double alpha, bool on_device); // y = alpha A x with the factorize()d values
    int32_t determinant(double *mantissa, double *exponent, double *rcond);
    int32_t rcond_estimate(double *rcond); // min |u_ii| / max |u_ii| by a device reduction
    int32_t determinant_complex(double *mantissa_re, double *mantissa_im, double *exponent, double *rcond); // opt.complex_pairs: det of the COMPLEX matrix = (re + i im) x 10^exponent
    int32_t adopt_factor(const double *d_values); // factor buffers were filled by a peer (many-RHS multi-GPU path)
    // The caller's value arrays hold nnz_lower entries (the lower triangle it handed to the C-ABI) while the handle was analysed with
    // the mirrored general matrix: entry k of the handle's CSR is entry emap[k] of the caller's.  Every entry point that takes CSR
    // values expands them on the device.
    int32_t set_expansion(int64_t nnz_lower, const std::vector<int32_t> &emap);
    int64_t expansion_inputs() const { return nnz_low; }
    const std::vector<int32_t> &expansion_map() const { return h_emap; }
    void mark_factor_adopted(int32_t root_perturbed = 0) { n_perturbed = root_perturbed, n_zero_pivot = 0, factorized = true, forget_border(); } // ... including the matrix values; the root's count of replaced pivots decides about the Krylov rescue here too
    void *d_diag_ptr() const { return d_diag; }
    // FNV-1a over what two handles must share to exchange a factor: the fill-reducing permutation, the matching's row permutation, the
    // layout of the pool (computed at initialize / after a re-matching factorize)
    uint64_t plan_signature() const { return plan_sig; }
    uint64_t plan_sig = 0;
    int64_t plan_digest = 0; // HIPMF_PLAN_DIGEST set at initialize: digest of the row structures, pool layout and extend-add task lists (else 0)
    int64_t nnz_in_values() const { return nnz_in; } // inputs the installed value map reads (0: none)
    const std::vector<int32_t> &kept_row_pointers() const { return h_rp_keep; } // the caller's CSR structure as handed to initialize
    const std::vector<int32_t> &kept_col_indices() const { return h_ci_keep; }
    void *d_vals_ptr() const { return d_vals; }
    void release();

    Symbolic S;
    NumericOptions opt;
    PhaseTimes times;
    bool initialized = false, factorized = false;
    int32_t n_perturbed = 0, n_zero_pivot = 0;
    int32_t n_weak_diag = 0;   // rows with a weak diagonal under the current pivot order, for the values of the last factorize
    int64_t rematch_count = 0; // factorisations that recomputed the maximum-product matching (and the analysis) for new values
    int32_t refinement_steps_done = 0;
    int64_t fused_fallbacks = 0; // solves that fell back to the level-set launches after a hand-off timeout (never expected)
    int64_t mid_front_count = 0; // fronts of this plan that one workgroup factorises in one launch (k_front)
    int64_t wave_front_count = 0; // big fronts that are wave-front tasks in the forward pass of this plan (sf_fwd_wave)
    int32_t block_groups_last = 0;   // blocks of right-hand sides per dependency-driven launch in the last blocked solve (round 6)
    bool sym_diag_looked = false;    // the first values of a symmetric-lower handle were checked for a weak diagonal (once per initialize)
    bool sym_weak_diag_seen = false; // L D L^T plan kept although a factorize met a weak diagonal (HIPMF_OPTION_SYM_RECHECK off)
    bool event_fence_free = false; // the events between this handle's streams are recorded without the system-scope fence (gfx950 + HIP 7 only)
    int64_t gate_waits = 0;      // solves that waited for another handle's solve on the same device (device_gate, numeric.cpp)
    bool tagged_solve() const { return tag_active && use_fused; }
    int64_t leaf_front_count() const { return use_fused ? leaf_cnt : 0; }
    int64_t split_slab_count() const { return use_fused ? split_slabs : 0; }
    int64_t chain_fallbacks = 0; // factorisations repeated with one launch per tiled step after a hand-off timeout of a chained launch (never expected)
    int64_t persist_bytes() const { return S.persist_doubles * 8; }
    double last_residual_inf = 0.0, last_omega = 0.0;
    int device = 0;
    std::string last_error;
    std::mutex err_mutex; // (the planning thread of initialize and the calling thread both report through last_error)

    int64_t pool_doubles = 0;     // doubles of the factor in d_pool
    bool matched = false;         // a maximum-product matching pre-permutation is in force
    int32_t match_parity = 0;     // parity of its row permutation (for the determinant)

  private:
    int32_t initialize_impl(int32_t n, const int32_t *rp, const int32_t *ci, bool sym_lower, const SymbolicOptions &sopt,
                            const NumericOptions &nopt, const double *values);
    int32_t upload_plan(const std::function<int32_t()> &tail); // tail: what initialize runs after the descriptor uploads, beside the solve task lists
    int32_t rematch_and_factorize(); // the values in d_vals invalidate the pivot order: new matching + analysis, then factorize
    // what a re-analysis needs: the caller's structure and options, the value map
    std::vector<int32_t> h_rp_keep, h_ci_keep, h_seg_ptr, h_seg_idx;
    SymbolicOptions sopt_keep;
    bool sym_lower_keep = false, rematching = false;
    bool rematch_futile = false; // the last re-matching left a weak diagonal: no further attempts for this handle
    int32_t run_factor();
    // forward + backward on nk permuted, scaled vectors (column c at xp + c * xstr, its workspace at wrk + c * wstr)
    struct SolveLane;
    int32_t run_triangular(double *xp, int32_t nk, double *wrk, int64_t xstr, int64_t wstr, void *lane_stream, int32_t *lane_sync, bool timed, int32_t lane_id, uint32_t gmask = 0xffffffffu);
    void harvest_tri();
    int32_t build_level_tasks();
    int32_t sfk_fwd_cnt = 0, sfk_bwd_cnt = 0, sfk_fwd_band = 0, sfk_bwd_top = 0;
    bool tags_armed = false;                   // the tagged words of d_work hold the tag pattern (left by the last pass pair's k_wt_bwd)
    std::vector<int32_t> sfk_band_f, sfk_band_b; // task offsets of the band's levels in d_sfk (forward: levels ascending from task 0; backward: relative to
                                               // the first backward task, the band's levels descending) -- one PLAIN launch per level (round 6)
    std::vector<int32_t> sf3_lvl, sf3_lvl_b; // task offsets per level: forward (leaves first), backward (root first)
    bool tri_pending = false;
    std::vector<LevelPlan> levels;
    int64_t work_doubles = 0;
    int32_t allbig_off = 0, allbig_cnt = 0, dws_stride = 1;
    // dependency-driven solve (kernels_solve_fused.hpp): one launch per direction
    int32_t sf_fwd_cnt = 0, sf_bwd_cnt = 0; // forward tasks first, then the backward tasks
    int32_t sf_fwd_band = 0, sf_bwd_top = 0; // tasks of the all-small bottom band (forward: first; backward: after sf_bwd_top)
    int32_t sf_fwd_launch = 0;              // == sf_fwd_cnt unless the profiling knob HIPMF_SF_FWD_LEVELS cuts the pass short
    int32_t wt_hdr_fwd = 0, wt_hdr_bwd = 0; // batches of the forward / backward part
    int64_t wt_meta_fwd = 0;                // words of the forward part of d_wt_meta
    int32_t sf2_fwd_mid = 0, sf2_bwd_top = 0; // forward: tasks below the top levels come first; backward: the top levels' tasks come first
    bool tree_active = false;               // the plan above exists for this matrix
    const double *last_host_rhs = nullptr;
    double *last_host_x = nullptr;
    bool tag_active = false;                // the launches above the wave-subtrees run their TAG instances (kernels_solve_fused.hpp, sf_tag_wait)
    int64_t work_arm0 = 0;                  // ... of which the first work_arm0 doubles (the roots of the wave-subtrees) are not armed: k_wt_fwd writes them in a launch of its own
    int64_t work_up = 0;                    // doubles at the head of a solve workspace: the vectors of the fronts outside the wave-subtrees' interiors
                                            // (tag_active: followed by n doubles, the tagged shadow of x)
    bool is_mid_lu(int32_t s) const;
    bool is_mid(int32_t s) const;
    bool level_path_ok = true;              // false: some front is too large for the level-set solves' LDS staging
    int32_t update_group(int32_t f) const { return f >= upd_g16 ? 16 : (f >= upd_g8 ? 8 : (f >= upd_g4 ? 4 : 2)); }
    int32_t sf_err[2] = {0, 0};
    std::vector<int32_t> h_emap;
    // values (CSR order of the caller, or the inputs of the value map: mapped) -> dst, nnz doubles in the handle's CSR order
    int32_t stage_values(double *dst, const double *values, bool mapped, bool on_device);
    struct OpPlain;      // the operator policies of the solve_updated cores (numeric.cpp)
    struct OpTransposed;
    // the flexible GMRES of solve_updated and solve_updated_complex; P: the arithmetic (UpdatedReal, UpdatedComplex in numeric.cpp), O: the
    // operator (OpPlain: A_new, OpTransposed: A_new^T -- preconditioner call, product and residual); conj_pairs: rhs and x are conjugated
    // on the way in and out (interleaved complex pairs)
    template <class P, class O>
    int32_t solve_updated_core(double *x, const double *rhs, const double *values, bool mapped, double rel_tol, int32_t max_steps, int32_t *steps, double *relres, bool on_device,
                               bool conj_pairs);
    // the block driver of solve_updated_many and solve_updated_many_complex; P, O and conj_pairs as above
    template <class P, class O>
    int32_t solve_updated_many_core(double *x, const double *rhs, int32_t nrhs, int64_t ld, const double *values, bool mapped, double rel_tol, int32_t max_steps, int32_t *steps,
                                    double *relres, bool on_device, bool conj_pairs);
    // the loop of solve_extra_precise, single and blocked (one column is a block of one); P: the measures (ExtraReal, ExtraPairs in numeric.cpp)
    template <class P>
    int32_t solve_extra_precise_core(double *x, double *tail, const double *rhs, int32_t nrhs, int64_t ld, double dx_tol, int32_t max_steps, double *info, bool on_device);
    // the blocked transposed pass pair on C <= 16 contiguous columns (stride n): Z = A^{-T} V, unrefined (buffers of tr_prepare_blocked())
    int32_t tr_pass_blk(double *Z, const double *V, int32_t C);
    // the loop of solve_bordered (T false) and solve_bordered_transpose (T true): the operands and the four launches that differ
    template <bool T>
    int32_t bordered_core(double *x, double *z, const double *f, const double *g, int32_t nrhs, int64_t ldx, int64_t ldz, int32_t max_steps, double *info, bool on_device,
                          bool conj_pairs = false);
    int32_t bt_prepare(); // V = A^{-T} C and the packed D^T of the border in force, once per set_border
    // Z = A^{-T} V for C <= 16 columns at the strides zs, vs, unrefined: the blocked pass pair, tr_pass per column without its buffers
    // or with HIPMF_TRANSPOSE_BLOCKED=0, solve_core on a handle where A^T = A (vs == zs there)
    int32_t bt_pass(double *Z, int64_t zs, const double *V, int64_t vs, int32_t C);
    // the error analysis of both forms; P: what differs (EaReal, EaComplex in numeric.cpp)
    template <class P>
    int32_t error_analysis_core(const double *xbar, const double *rhs, double *out, int32_t option);
    int64_t n_lists = 0;            // entries of d_lists
    static constexpr int32_t MAX_SOLVE_LANES = 4;
    int32_t solve_lanes = 1;   // HIPMF_SOLVE_LANES (1..4).  One since late round 4: two launches full of workgroups that wait for each other's
                               // lower-numbered tasks no longer pay (0.304 against 0.307 - 0.313 ms per right-hand side at 1000^2 with 256
                               // right-hand sides, 0.307 against 0.365 with 64) and, concurrently resident, every few runs one of them ran
                               // into a hand-off time-out (3.7 s; profiles/r04_solve_lanes.txt)
    bool solve_lanes_auto = true; // no HIPMF_SOLVE_LANES given: one lane when the factor exceeds 64 GB (solve())
    bool prepare_only = false;     // solve() stops after its buffers exist (prepare_many)
    int32_t block_groups_plan = 1; // ... what initialize planned for (HIPMF_BLOCK_GROUPS, else by the size of the factor): the split-dot-product scratch is sized by it
    int64_t work_blk_doubles = 0;  // stride between the columns of a blocked solve workspace: work_doubles without the tagged shadow xt
    std::vector<int32_t> sf_host, sfk_host; // (kind, front) per task (single-column lists / blocked list), kept only when tracing
    bool ea_lds_active() const { return use_ea_lds; }
    bool ea_lu_active() const { return ea_lds_active() && use_ea_lu && !use_binv; }
    int32_t spmv_blocks = 0;
    int32_t tr_prepare();
    template <class P>
    int32_t run_transposed(double *xp); // both passes of A^T; P: one vector or a block of 16 (TrSingle, TrBlocked in numeric.cpp)
    // the refinement rule of solve() on nk transposed columns; P issues the launches (TrColumn, TrColumns in numeric.cpp)
    template <class P>
    int32_t tr_refine(const P &p, int32_t nk, int32_t nstep, double *omega, int32_t *steps);
    int32_t tr_core(double *x, const double *b, int32_t nstep, double *omega, int32_t *steps); // one column: tr_pass, then the rule
    int32_t tr_pass(double *y, const double *v); // y = A^{-T} v on the device, one unrefined pass pair
    int32_t tr_spmv(double *y, const double *x); // y = A^T x on the device
    int32_t tr_rescue(double *tx, const double *tb, bool first_column); // FGMRES on one transposed column (the preconditioner: tr_pass)
    int32_t tr_prepare_blocked();
    int32_t sp_prepare();
    // per-level lists of the fronts in `fronts` (any order) into `buf`, levels ascending: forward shapes (assembly + products over f rows),
    // backward shapes (gather + products over p rows) or transposed forward shapes (assembly + 16-column tiles over f columns)
    void sp_build_lists(const std::vector<int32_t> &fronts, SpShape shape, std::vector<int32_t> &buf, std::vector<SpLevel> &lv) const;
    int32_t run_pruned(double *XP, const std::vector<SpLevel> &fl, const std::vector<SpLevel> &bl);
    int32_t run_pruned_transposed(double *XP, const std::vector<SpLevel> &fl, const std::vector<SpLevel> &bl); // the same for A^T
};

} // namespace hipmf
