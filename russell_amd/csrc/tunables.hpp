// tunables.hpp -- every environment knob of the solver: one struct of fields with their defaults, one table of variables.
//
// None is needed in normal use; the tests use them to force schedules on small problems.  Solver::initialize() reads the table once
// (Tunables::from_env) and keeps the result for the life of that analysis, a re-analysis by a re-matching factorize included; the rows
// marked PER_CALL are read at the call that uses them (Tunables::now), PER_PROCESS ones once per process.  This is the only file of the
// sources that reads the environment.  It needs the standard library alone.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace hipmf {

// the one reader of the environment (nullptr: not set)
inline const char *env_text(const char *name) { return std::getenv(name); }

struct Tunables {
    static constexpr int32_t MID_MMAX_CAP = 192;   // == MID_MMAX (kernels_factor_front.hpp; checked in numeric.cpp)
    static constexpr int32_t BLOCK_GROUPS_CAP = 4; // == SF_GMAX (kernels_solve_fused.hpp; checked in numeric.cpp)

    // ---- analysis (handed to SymbolicOptions by initialize) ----
    bool sym_ldlt = true;          // HIPMF_SYM_LDLT=0: symmetric-lower input is factorised as LU of the mirrored matrix instead of L D L^T on the tiled fronts
    // fewer, fatter fronts: nested-dissection leaves of <= 16 vertices become single dense supernodes
    // (1000^2 Poisson: 503 796 -> 113 068 fronts, 29 -> 20 levels, nnz(L) +18 %); see DESIGN.md section 4
    int32_t nd_leaf = 16;          // HIPMF_ND_LEAF: leaf size (1..64); 0 = classic minimum-degree leaves of 64 (dense_leaves = false)
    bool dense_leaves = true;
    int32_t split_pivots = 4096;   // HIPMF_SPLIT_PIVOTS: chain links of the big supernodes (0: never split)
    double dense_row_factor = 10.0; // HIPMF_DENSE_ROWS: degree threshold factor of the hub vertices (0: off)
    int32_t nd_threads = 0;        // HIPMF_ND_THREADS: host threads of the ordering, the assembly lists and the extend-add task lists (same result for any
                                   // count); not given: min(16, hardware threads), the assembly lists at most 4
    int32_t par_min = 200000;      // HIPMF_PAR_MIN: below this order / entry count / tile count the threaded pieces of initialize run serially (tests: 0)
    int32_t par_chunk = 4096;      // HIPMF_PAR_CHUNK: smallest size bound of the subtrees handed to host threads (tests: several subtrees per thread on small matrices)
    int32_t relax_ncol[3] = {4, 16, 64};        // HIPMF_RELAX="n0,n1,n2,z0,z1,z2": relaxed amalgamation (columns of the merged supernode,
    double relax_zeros[3] = {0.8, 0.1, 0.05};   // share of explicit zeros it may hold); see symbolic.hpp, profiles/r04_relax_sweep.txt
    int32_t relax_big_front = 2048; // HIPMF_RELAX_BIG: the largest tier merges only into fronts of at least this many rows (0: any)
    bool arena_reuse = true;       // HIPMF_ARENA_REUSE=0: every working block of a tiled front keeps its own storage (same bits, used by a test)
    bool align_panels = true;      // HIPMF_ALIGN_PANELS=0: the strides of E / E' are not rounded up to 128-byte lines (round 5, profiles/r04_sptrsv_traffic.json)
    int32_t matching = 1;          // HIPMF_MATCHING: when given it replaces NumericOptions::matching (0 never, 1 weak diagonal, 2 always)
    double pool_limit_gb = 0.0;    // HIPMF_POOL_LIMIT_GB: when given the analysis refuses a pool above 0.95 x this (tests: force the refusal); else 95 % of the free memory
    bool want_digest = false;      // HIPMF_PLAN_DIGEST set (any value): initialize digests row structures, pool layout and task lists into plan_digest
    bool plan_thread = true;       // HIPMF_PLAN_THREAD=0: the solve task lists are built in line, for timing comparisons
    bool event_fence = false;      // HIPMF_EVENT_FENCE=1: the events between the handle's streams keep the system-scope fence of the default flags

    // ---- factorisation ----
    // the launches of a factorisation's levels, captured once and replayed (HIPMF_FACTOR_GRAPH=0: eager launches)
    bool use_graph = false;        // (measured: no gain at 1000 x 1000 -- the gaps at the level boundaries are the cross-stream edges themselves, not host latency)
    bool use_binv = false;         // HIPMF_BLOCK_INV=1: LU fronts of the tiled path take ONE launch per step (kernels_factor_binv.hpp) instead of k_panel + k_update; measured slower (profiles/r04_rejected_experiments.txt)
    int32_t upd_split_min = 0;     // HIPMF_UPD_SPLIT=n: full steps (two-launch form) with at least n update workgroups are split (0: never; measured: no gain)
    bool overlap_small = true;     // HIPMF_OVERLAP_SMALL=0: everything on one stream
    bool small_pair = false;       // HIPMF_SMALL_PAIR=1: the two k_small_factor launches of an all-small level side by side (third stream)
    // levels with few tiled steps (the middle of the tree): all steps of a level in one launch with in-launch hand-offs (kernels_factor_chain.hpp)
    bool use_chain = false;        // HIPMF_FACTOR_CHAIN=1 switches it on.  Off by default: measured at the end of round 3 it is neutral for LU at
                                   // 1000 x 1000 (7.35 -> 7.34 ms), -1.6 % for L D L^T there and +1 ... +3 % on smaller problems (profiles/r03_chain_check.txt)
    bool chain_fine = false;       // HIPMF_CHAIN_FINE=1: a panel waits only for the critical pieces of the update before (measured: no gain)
    int32_t chain_max_steps = 8;   // a level is chained when it has at most this many steps (HIPMF_CHAIN_MAX_STEPS) ...
    int32_t chain_max_update = 16384; // ... no step of it has more update workgroups than this (HIPMF_CHAIN_MAX_WGS: wide steps are bound by throughput, and
                                   //     the 8-byte agent-scope accesses of the chained form cost more per byte) ...
    int32_t chain_min_update = 0;  // ... and its widest step has at least this many (HIPMF_CHAIN_MIN_WGS)
    int32_t upd32_max_front = 256; // LU: levels whose largest tiled front has at most this many rows update with 32 x 32 tiles, one wave per tile
                                   // (HIPMF_UPD32_MAXF; 0: never).  Bit-identical to the 64 x 64 instance; 1000 x 1000: 7.30 -> 7.23 ms.  The L D L^T
                                   // fronts keep the 64 x 64 tiles (measured: 6.32 -> 6.35 ms with the small ones) unless the variable is given
    // LU mode: fronts with f > 64, at most 64 pivots and at most mid_mmax off-diagonal rows whose pivot rows + column panel fit the
    // LDS budget of k_front are factorised by one workgroup each, one launch per level and size class (HIPMF_MID_FRONT=0: off,
    // HIPMF_MID_MMAX: rows at most, <= 192)
    bool use_mid = true;
    int32_t mid_mmax = 0;          // HIPMF_MID_MMAX: k_front (eight wavefronts, up to 64 pivots) takes the fronts with at most this many off-diagonal rows that
                                   // k_front_lu does not take; off by default -- measured 7.13 ms with it (80 rows) against 7.10 without, 7.28 on tiled launches alone
    bool use_mid_lu = true;        // HIPMF_MID_LU=0: fronts with at most 32 pivots take k_front / the tiled path like the others
    int32_t mid_lu_mmax = 192;     // HIPMF_MID_LU_MMAX: off-diagonal rows of a k_front_lu front at most
    bool mid_lu_split = false;     // HIPMF_MID_LU_SPLIT=1: the k_front_lu fronts of a level in three launches by LDS class (two or four fronts per CU for the smaller ones); measured slower: 6.58 -> 6.95 ms
    int32_t diag0_min_panels = 512; // HIPMF_DIAG0_MIN: step 0 of a level: from this many panel workgroups the first diagonal tiles get their own launch (k_diag0)
    // Tiled path: fronts with at least upd_g4 (upd_g8, upd_g16) rows apply 4 (8, 16) panels per pass over the trailing matrix instead of 2:
    // the read-modify-write of the trailing matrix bounds the large fronts (HIPMF_UPD_G4 / HIPMF_UPD_G8 / HIPMF_UPD_G16)
    int32_t upd_g4 = 2048, upd_g8 = 4096, upd_g16 = 1 << 30;
    int32_t small_wide_max = 7000; // a k_small_factor launch with at most this many fronts uses four wavefronts per front (HIPMF_SMALL_WIDE, 0: never)
    int32_t small_split = 28;      // small fronts up to this size get their own launch per level (HIPMF_SMALL_SPLIT, 0: one launch)
    bool upd_la_first = true;      // HIPMF_UPD_LA_FIRST=0: the look-ahead piece of a front is the last workgroup of its range in a trailing-update launch (1: the look-ahead pieces lead the launch)
    bool upd_xcd = true;           // HIPMF_UPD_XCD=0: the tiles of a full trailing update in plain order (1: whole tile columns per XCD)
    bool use_ea_lds = true;        // HIPMF_EA_LDS=0: LU working blocks go back to k_zero + k_scatter + k_extend_add (read-modify-write per child) instead of k_extend_add_lds
    bool use_ea_lu = true;         // HIPMF_EA_LU=0: the first diagonal tiles go back to k_diag0 / the first panel launch

    // ---- solves ----
    bool use_fused = true;         // false: level-set launches (HIPMF_FUSED_SOLVE=0, or after a hand-off timeout)
    // bottom of the tree: one wavefront per subtree of small fronts (kernels_solve_tree.hpp); the tasks of everything above it
    // (single right-hand side; the blocked many-RHS instances keep the task lists above)
    bool use_tree = true;          // HIPMF_TREE_SOLVE=0: the round-2 schedule (all-small band + upper band)
    int32_t wt_max_fronts = 24;    // HIPMF_WT_FRONTS: fronts per wave-subtree at most
    int32_t wt_max_kb = 64;        // HIPMF_WT_KB: panel kilobytes per wave-subtree at most
    int32_t up_stage = 32;         // HIPMF_UP_STAGE: entries of E per thread of a TOP-level forward slab parked in LDS before the wait (multiple of 8; 0: no top launch)
    int32_t up_stage_bwd = 48;     // HIPMF_UP_STAGE_BWD: the same for E' in the backward pass (the dot products run over f, not p)
    int32_t up_stage_mid = 8;      // HIPMF_UP_STAGE_MID: the same for the backward slabs BELOW the top levels (0: none; not given: 0 with the tagged hand-offs)
    int32_t up_top_fronts = 40;    // HIPMF_UP_TOP_FRONTS: the top levels are those above which no level has more tiled fronts
    bool up_pair_xcd = true;       // HIPMF_UP_PAIR_XCD=0: the 8-row slabs of a top-level front in row order (1: neighbours eight tasks apart = same XCD)
    int32_t up_max_groups = 32;    // HIPMF_UP_MAX_GROUPS: column groups of a top-level slab at most (32: 8-row slabs; 16: 16-row slabs = whole 128-byte lines)
    bool use_rep = true;           // HIPMF_UP_REPLICAS=0: every waiter polls the front's counter
    bool use_tag = true;           // HIPMF_TAG_SOLVE=0: completion counters instead of data-tagged hand-offs above the wave-subtrees
    bool wave_fronts = true;       // HIPMF_WAVE_FRONTS=0: the big fronts of few rows / pivots right above the wave-subtrees stay 256-thread slab tasks in the forward pass
    bool wave_fronts_bwd = true;   // ... and of the backward pass (HIPMF_WAVE_FRONTS_BWD=0: slab tasks there)
    int32_t mid_bwd_len4 = 256, mid_bwd_len5 = 64; // backward slabs below the top levels, tagged hand-offs: 16 / 32 rows from these dot lengths on (HIPMF_MID_BWD_LEN4 / _LEN5)
    bool host_direct = true;       // host-pointer solves: buffers seen in the previous call are copied without the pinned staging buffer (HIPMF_HOST_DIRECT=0: always staged)
    int32_t sf_big_rows = 6, sf_big_front = 2048; // forward solve: fronts with at least sf_big_front rows use slabs of 2^sf_big_rows rows (HIPMF_SF_BIG_ROWS, 0: by dot length only; HIPMF_SF_BIG_FRONT)
    int32_t sf_asm_front = 2048;   // HIPMF_SF_ASM_FRONT: forward solve: fronts with at least this many rows assemble their vector once, in tasks of their own (0: never; then sf_big_rows applies)
    bool slab64 = false;           // HIPMF_SOLVE_SLAB64=1: same slab shape in both solve paths (bitwise comparable)
    int32_t sf_fwd_levels = 0;     // HIPMF_SF_FWD_LEVELS: when given the forward pass runs up to this level only (the result is then meaningless)
    std::string sf_trace;          // HIPMF_SF_TRACE=<file>: four device-clock stamps per task of the upper (mixed) launches of the last solve (tools/fused_trace.py)
    // optional task list of the blocked (many-RHS) instances with wider slabs (HIPMF_BLOCKED_SLABS=1).  Measured and NOT the default:
    // 64 / 128-row slabs re-read the vector block of a front less often, but lose more in parallelism -- 144^3, 64 right-hand sides:
    // 4.92 -> 7.06 ms per right-hand side; 200^3, 256 right-hand sides: 4.58 -> 6.86 s (profiles/r03_rejected_experiments.txt)
    bool blocked_slabs = false;    // (not given: on for factors whose largest front has >= 16 384 rows when several groups share a launch)
    // round 5: the leaves of the tree leave the task lists of the blocked (many-RHS) solves: one wavefront carries sixteen columns through
    // LEAF_PER_WAVE leaves (kernels_solve_leaf.hpp).  HIPMF_LEAF_KERNELS=0: every small front stays a task.
    bool leaf_kernels = true;
    // blocked instances, backward pass, levels of few slabs with long dot products (the top of a 3D factor): a slab's dot products are
    // split over Q consecutive tasks (k_bwd_fused); forward, the largest fronts of such levels get narrower slabs.  A level qualifies
    // below split_tasks slabs (HIPMF_SPLIT_TASKS, 0: never), a front from split_minlen rows on (HIPMF_SPLIT_MINLEN).
    int32_t split_tasks = 512, split_minlen = 2048; // (split_minlen: 2 048 x the planned block groups unless HIPMF_SPLIT_MINLEN says otherwise; small values: tests)
    bool rearm_tags = false;       // HIPMF_REARM_TAGS=1: k_wt_bwd re-arms the tagged words for the next pass pair instead of a memset before every pass pair
                                   // (built and measured in round 6: same bits, NOT faster -- pass pair 0.4037 - 0.4076 against 0.4012 - 0.4058 ms, solve
                                   // 0.94 - 0.95 against 0.91 ms, profiles/r06_rejected_experiments.txt; default off)
    bool plain_band = true;        // HIPMF_PLAIN_BAND=0: the all-small band of the blocked solves stays ONE dependency-driven launch per direction
    int32_t block_groups_ask = 0;     // HIPMF_BLOCK_GROUPS=1..4: blocks of right-hand sides per dependency-driven launch (not given: by the size of the factor)
    double block_groups_max_bytes = 1e18; // factors up to this many bytes carry SF_GMAX blocks per launch, larger ones one (HIPMF_BLOCK_GROUPS_BYTES; no limit by default: measured to pay up to config 4's 84 GB, profiles/r06_block_groups.txt)
    bool krylov_enabled = true;    // HIPMF_KRYLOV=0: no rescue (the refined solution is returned as it is)
    int32_t krylov_restart = 40;   // directions per cycle (HIPMF_KRYLOV_RESTART)
    double krylov_omega_ok = 1e-13; // a column whose refined solution has a componentwise backward error up to this is not looked at by the rescue (HIPMF_KRYLOV_OMEGA)
    double krylov_tol = 1e-13;     // |b - A x|_2 <= tol |b|_2 ends the rescue (and is what triggers it) (HIPMF_KRYLOV_TOL)

    // ---- read at the call that uses them, not at initialize (tests toggle them between calls on one handle) ----
    int32_t block_cols_ask = 0;      // HIPMF_BLOCK_COLS=8 or 16: columns per block of the many-RHS driver (else by the number of right-hand sides)
    int32_t updated_restart = 30;  // HIPMF_UPDATED_RESTART: restart length of solve_updated (4 .. 200; other values are ignored)
    bool updated_timing = false;   // HIPMF_UPDATED_TIMING=1: HIP-event time of a solve_updated call's pass pairs, SpMVs, Arnoldi kernels
    bool extra_timing = false;     // HIPMF_EXTRA_TIMING=1: HIP-event time of a solve_extra_precise call's residuals, correction pass pairs, updates
    bool transpose_blocked = true; // HIPMF_TRANSPOSE_BLOCKED=0: solve_transpose_many sends its columns through the column loop of solve_transpose
    double prune_max_share = 0.25; // HIPMF_PRUNE_MAX_SHARE: a sparse block whose marked fronts read more than this share of a full pass pair takes the ordinary solve
    double prune_min_bytes = 2e9;  // HIPMF_PRUNE_MIN_BYTES: a block of ONE sparse column takes the ordinary solve below this many bytes per pass pair
                                   // (both defaults from the measurement of profiles/r09_sparse_rhs.txt)
    bool sym_expand = true;        // HIPMF_SYM_EXPAND=0: symmetric-lower input with a weak diagonal stays L D L^T with static pivoting (1: mirrored, matched LU)
    bool bcast_slices = true;      // HIPMF_BCAST_SLICES=0: the factor travels by plain ncclBroadcast (1: as N slices in two point-to-point steps)
    double bcast_slice_min = 64.0 * 1048576; // HIPMF_BCAST_SLICE_MIN: bytes from which a part of the factor travels as slices (at least 4096)
    bool complex_pairs = true;     // HIPMF_COMPLEX_PAIRS=0: the complex solver factorises the plain real-equivalent system (no complex determinant)
    bool process_gate = true;      // HIPMF_PROCESS_GATE=0: the per-device gate of the dependency-driven solves orders this process' handles only

    // ---- the table ----
    enum Kind { FLAG, INT, REAL, TEXT, RELAX };
    enum When { INIT, PER_CALL, PER_PROCESS };
    enum Status { DEFAULT_PATH, TEST_AID, PROFILING_AID, REJECTED }; // REJECTED: a measured-and-rejected experiment, `note` names its profile
    struct Row {
        const char *name;
        Kind kind;
        When when;
        Status status;
        const char *note;           // profiles/ file of a rejected experiment ("": the measurement stands in the field's comment only)
        bool Tunables::*b;          // FLAG: atoi != 0
        int32_t Tunables::*i;       // INT: atoi, rounded down to a multiple of step, clamped to [lo, hi]
        double Tunables::*d;        // REAL: atof
        std::string Tunables::*s;   // TEXT
        int32_t lo, hi, step;
        void (*parse)(Tunables &, const char *); // a rule of its own instead of the kind's (the kind still says how the row prints)
    };
    using Parse = void (*)(Tunables &, const char *);
    static constexpr int32_t ANY = INT_MIN, MAX = INT_MAX;
    static Row flag(const char *n, bool Tunables::*f, When w, Status s, const char *note = "", Parse p = nullptr) { return {n, FLAG, w, s, note, f, nullptr, nullptr, nullptr, 0, 0, 1, p}; }
    static Row integer(const char *n, int32_t Tunables::*f, int32_t lo, int32_t hi, When w, Status s, const char *note = "", Parse p = nullptr, int32_t step = 1) {
        return {n, INT, w, s, note, nullptr, f, nullptr, nullptr, lo, hi, step, p};
    }
    static Row real(const char *n, double Tunables::*f, When w, Status s, const char *note = "", Parse p = nullptr) { return {n, REAL, w, s, note, nullptr, nullptr, f, nullptr, 0, 0, 1, p}; }

    static constexpr int MAX_ROWS = 128; // (bits of given_bits)
    static const Row *rows(int *count = nullptr) {
        using T = Tunables;
        static const Row R[] = {
            // analysis
            flag("HIPMF_SYM_LDLT", &T::sym_ldlt, INIT, DEFAULT_PATH),
            integer("HIPMF_ND_LEAF", &T::nd_leaf, 0, 64, INIT, DEFAULT_PATH, "",
                    [](T &t, const char *e) { const int v = atoi(e); t.dense_leaves = v > 0, t.nd_leaf = v > 0 ? std::min(v, 64) : 64; }),
            integer("HIPMF_SPLIT_PIVOTS", &T::split_pivots, 0, MAX, INIT, DEFAULT_PATH),
            real("HIPMF_DENSE_ROWS", &T::dense_row_factor, INIT, DEFAULT_PATH),
            integer("HIPMF_ND_THREADS", &T::nd_threads, 1, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_PAR_MIN", &T::par_min, 0, MAX, INIT, TEST_AID),
            integer("HIPMF_PAR_CHUNK", &T::par_chunk, 1, MAX, INIT, TEST_AID),
            {"HIPMF_RELAX", RELAX, INIT, DEFAULT_PATH, "", nullptr, nullptr, nullptr, nullptr, 0, 0, 1,
             [](T &t, const char *e) { // (a malformed string is ignored)
                 int a, b, c;
                 double x, y, z;
                 if (sscanf(e, "%d,%d,%d,%lf,%lf,%lf", &a, &b, &c, &x, &y, &z) == 6)
                     t.relax_ncol[0] = a, t.relax_ncol[1] = b, t.relax_ncol[2] = c, t.relax_zeros[0] = x, t.relax_zeros[1] = y, t.relax_zeros[2] = z;
             }},
            integer("HIPMF_RELAX_BIG", &T::relax_big_front, 0, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_ARENA_REUSE", &T::arena_reuse, INIT, TEST_AID),
            flag("HIPMF_ALIGN_PANELS", &T::align_panels, INIT, DEFAULT_PATH),
            integer("HIPMF_MATCHING", &T::matching, ANY, MAX, INIT, DEFAULT_PATH),
            real("HIPMF_POOL_LIMIT_GB", &T::pool_limit_gb, INIT, TEST_AID),
            flag("HIPMF_PLAN_DIGEST", &T::want_digest, INIT, TEST_AID, "", [](T &t, const char *) { t.want_digest = true; }),
            flag("HIPMF_PLAN_THREAD", &T::plan_thread, INIT, PROFILING_AID),
            flag("HIPMF_EVENT_FENCE", &T::event_fence, INIT, TEST_AID),
            // factorisation
            flag("HIPMF_FACTOR_GRAPH", &T::use_graph, INIT, REJECTED),
            flag("HIPMF_BLOCK_INV", &T::use_binv, INIT, REJECTED, "profiles/r04_rejected_experiments.txt"),
            integer("HIPMF_UPD_SPLIT", &T::upd_split_min, 0, MAX, INIT, REJECTED),
            flag("HIPMF_OVERLAP_SMALL", &T::overlap_small, INIT, DEFAULT_PATH),
            flag("HIPMF_SMALL_PAIR", &T::small_pair, INIT, REJECTED, "profiles/r04_knob_sweep.txt"),
            flag("HIPMF_FACTOR_CHAIN", &T::use_chain, INIT, REJECTED, "profiles/r03_chain_check.txt"),
            flag("HIPMF_CHAIN_FINE", &T::chain_fine, INIT, REJECTED),
            integer("HIPMF_CHAIN_MAX_STEPS", &T::chain_max_steps, 0, MAX, INIT, REJECTED, "profiles/r03_chain_check.txt"),
            integer("HIPMF_CHAIN_MAX_WGS", &T::chain_max_update, 0, MAX, INIT, REJECTED, "profiles/r03_chain_check.txt"),
            integer("HIPMF_CHAIN_MIN_WGS", &T::chain_min_update, 0, MAX, INIT, REJECTED, "profiles/r03_chain_check.txt"),
            integer("HIPMF_UPD32_MAXF", &T::upd32_max_front, 0, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_MID_FRONT", &T::use_mid, INIT, DEFAULT_PATH),
            integer("HIPMF_MID_MMAX", &T::mid_mmax, 0, MID_MMAX_CAP, INIT, REJECTED),
            flag("HIPMF_MID_LU", &T::use_mid_lu, INIT, DEFAULT_PATH),
            integer("HIPMF_MID_LU_MMAX", &T::mid_lu_mmax, 1, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_MID_LU_SPLIT", &T::mid_lu_split, INIT, REJECTED),
            integer("HIPMF_DIAG0_MIN", &T::diag0_min_panels, ANY, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_UPD_G4", &T::upd_g4, 65, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_UPD_G8", &T::upd_g8, 65, MAX, INIT, DEFAULT_PATH, "", [](T &t, const char *e) { t.upd_g8 = std::max(t.upd_g4, atoi(e)); }),
            integer("HIPMF_UPD_G16", &T::upd_g16, 65, MAX, INIT, DEFAULT_PATH, "", [](T &t, const char *e) { t.upd_g16 = std::max(t.upd_g8, atoi(e)); }),
            integer("HIPMF_SMALL_WIDE", &T::small_wide_max, ANY, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_SMALL_SPLIT", &T::small_split, ANY, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_UPD_LA_FIRST", &T::upd_la_first, INIT, DEFAULT_PATH),
            flag("HIPMF_UPD_XCD", &T::upd_xcd, INIT, DEFAULT_PATH),
            flag("HIPMF_EA_LDS", &T::use_ea_lds, INIT, DEFAULT_PATH),
            flag("HIPMF_EA_LU", &T::use_ea_lu, INIT, DEFAULT_PATH),
            // solves
            flag("HIPMF_FUSED_SOLVE", &T::use_fused, INIT, DEFAULT_PATH),
            flag("HIPMF_TREE_SOLVE", &T::use_tree, INIT, DEFAULT_PATH),
            integer("HIPMF_WT_FRONTS", &T::wt_max_fronts, 1, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_WT_KB", &T::wt_max_kb, 1, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_UP_STAGE", &T::up_stage, 0, 64, INIT, DEFAULT_PATH, "", nullptr, 8),
            integer("HIPMF_UP_STAGE_BWD", &T::up_stage_bwd, 8, 64, INIT, DEFAULT_PATH, "", nullptr, 8),
            integer("HIPMF_UP_STAGE_MID", &T::up_stage_mid, 0, 32, INIT, DEFAULT_PATH, "", nullptr, 8),
            integer("HIPMF_UP_TOP_FRONTS", &T::up_top_fronts, 1, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_UP_PAIR_XCD", &T::up_pair_xcd, INIT, DEFAULT_PATH),
            integer("HIPMF_UP_MAX_GROUPS", &T::up_max_groups, 2, 32, INIT, DEFAULT_PATH),
            flag("HIPMF_UP_REPLICAS", &T::use_rep, INIT, DEFAULT_PATH),
            flag("HIPMF_TAG_SOLVE", &T::use_tag, INIT, DEFAULT_PATH),
            flag("HIPMF_WAVE_FRONTS", &T::wave_fronts, INIT, DEFAULT_PATH),
            flag("HIPMF_WAVE_FRONTS_BWD", &T::wave_fronts_bwd, INIT, DEFAULT_PATH),
            integer("HIPMF_MID_BWD_LEN4", &T::mid_bwd_len4, 1, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_MID_BWD_LEN5", &T::mid_bwd_len5, 1, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_HOST_DIRECT", &T::host_direct, INIT, DEFAULT_PATH),
            integer("HIPMF_SF_BIG_ROWS", &T::sf_big_rows, 0, 7, INIT, DEFAULT_PATH),
            integer("HIPMF_SF_BIG_FRONT", &T::sf_big_front, 65, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_SF_ASM_FRONT", &T::sf_asm_front, ANY, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_SOLVE_SLAB64", &T::slab64, INIT, TEST_AID),
            integer("HIPMF_SF_FWD_LEVELS", &T::sf_fwd_levels, ANY, MAX, INIT, PROFILING_AID),
            {"HIPMF_SF_TRACE", TEXT, INIT, PROFILING_AID, "", nullptr, nullptr, nullptr, &T::sf_trace, 0, 0, 1, nullptr},
            flag("HIPMF_BLOCKED_SLABS", &T::blocked_slabs, INIT, DEFAULT_PATH, "profiles/r06_block_groups.txt"),
            flag("HIPMF_LEAF_KERNELS", &T::leaf_kernels, INIT, DEFAULT_PATH),
            integer("HIPMF_SPLIT_TASKS", &T::split_tasks, 0, MAX, INIT, DEFAULT_PATH),
            integer("HIPMF_SPLIT_MINLEN", &T::split_minlen, 64, MAX, INIT, DEFAULT_PATH),
            flag("HIPMF_REARM_TAGS", &T::rearm_tags, INIT, REJECTED, "profiles/r06_rejected_experiments.txt"),
            flag("HIPMF_PLAIN_BAND", &T::plain_band, INIT, DEFAULT_PATH),
            integer("HIPMF_BLOCK_GROUPS", &T::block_groups_ask, 1, BLOCK_GROUPS_CAP, INIT, DEFAULT_PATH),
            real("HIPMF_BLOCK_GROUPS_BYTES", &T::block_groups_max_bytes, INIT, DEFAULT_PATH),
            flag("HIPMF_KRYLOV", &T::krylov_enabled, INIT, DEFAULT_PATH),
            integer("HIPMF_KRYLOV_RESTART", &T::krylov_restart, 4, MAX, INIT, DEFAULT_PATH),
            real("HIPMF_KRYLOV_TOL", &T::krylov_tol, INIT, DEFAULT_PATH),
            real("HIPMF_KRYLOV_OMEGA", &T::krylov_omega_ok, INIT, DEFAULT_PATH),
            // per call, per process
            integer("HIPMF_BLOCK_COLS", &T::block_cols_ask, ANY, MAX, PER_CALL, TEST_AID),
            integer("HIPMF_UPDATED_RESTART", &T::updated_restart, 4, 200, PER_CALL, DEFAULT_PATH, "",
                    [](T &t, const char *e) { if (atoi(e) >= 4 && atoi(e) <= 200) t.updated_restart = atoi(e); }),
            flag("HIPMF_UPDATED_TIMING", &T::updated_timing, PER_CALL, PROFILING_AID),
            flag("HIPMF_EXTRA_TIMING", &T::extra_timing, PER_CALL, PROFILING_AID),
            flag("HIPMF_TRANSPOSE_BLOCKED", &T::transpose_blocked, PER_CALL, TEST_AID, "", [](T &t, const char *e) { t.transpose_blocked = e[0] != '0'; }),
            real("HIPMF_PRUNE_MAX_SHARE", &T::prune_max_share, PER_CALL, DEFAULT_PATH),
            real("HIPMF_PRUNE_MIN_BYTES", &T::prune_min_bytes, PER_CALL, DEFAULT_PATH),
            flag("HIPMF_SYM_EXPAND", &T::sym_expand, PER_CALL, DEFAULT_PATH),
            flag("HIPMF_BCAST_SLICES", &T::bcast_slices, PER_CALL, DEFAULT_PATH),
            real("HIPMF_BCAST_SLICE_MIN", &T::bcast_slice_min, PER_CALL, DEFAULT_PATH, "",
                 [](T &t, const char *e) { t.bcast_slice_min = (double)std::max<long long>(4096, atoll(e)); }),
            flag("HIPMF_COMPLEX_PAIRS", &T::complex_pairs, PER_CALL, DEFAULT_PATH),
            flag("HIPMF_PROCESS_GATE", &T::process_gate, PER_PROCESS, DEFAULT_PATH),
        };
        static_assert(sizeof R / sizeof R[0] <= MAX_ROWS, "given_bits is too short for the table");
        if (count) *count = (int)(sizeof R / sizeof R[0]);
        return R;
    }
    static int nrows() {
        int c;
        rows(&c);
        return c;
    }

    // ---- reading ----
    uint64_t given_bits[MAX_ROWS / 64] = {}; // bit r: the variable of row r was set when this instance was read

    void read_row(int r) {
        const Row &w = rows()[r];
        const char *e = env_text(w.name);
        if (!e) return;
        given_bits[r / 64] |= 1ull << (r % 64);
        if (w.parse) w.parse(*this, e);
        else if (w.kind == FLAG) this->*w.b = atoi(e) != 0;
        else if (w.kind == INT) this->*w.i = std::max(w.lo, std::min(w.hi, atoi(e) / w.step * w.step));
        else if (w.kind == REAL) this->*w.d = atof(e);
        else if (w.kind == TEXT) this->*w.s = e;
    }
    static Tunables from_env() { // one walk over the table, in its order (HIPMF_UPD_G8 / _G16 build on the row before)
        Tunables t;
        for (int r = 0, nr = nrows(); r < nr; r++) t.read_row(r);
        return t;
    }
    static bool is(const Row &w, bool Tunables::*f) { return w.b == f; }
    static bool is(const Row &w, int32_t Tunables::*f) { return w.i == f; }
    static bool is(const Row &w, double Tunables::*f) { return w.d == f; }
    static bool is(const Row &w, std::string Tunables::*f) { return w.s == f; }
    template <class F> static int row_of(F Tunables::*f) {
        for (int r = 0, nr = nrows(); r < nr; r++)
            if (is(rows()[r], f)) return r;
        return -1; // (no row: a programming error, caught by the first test that initializes)
    }
    // was the variable of this field set when the instance was read?  (sites whose default depends on the plan ask this)
    template <class F> bool given(F Tunables::*f) const {
        const int r = row_of(f);
        return r >= 0 && (given_bits[r / 64] >> (r % 64) & 1) != 0;
    }
    // the PER_CALL / PER_PROCESS rows: the field's value as the environment says NOW
    template <class F> static F now(F Tunables::*f) {
        Tunables t;
        const int r = row_of(f);
        if (r >= 0) t.read_row(r);
        return t.*f;
    }

    // "NAME=value when status[ note]\n" per row into buf (at most cap bytes, always terminated when cap > 0); returns the bytes needed
    int64_t dump(char *buf, int64_t cap) const {
        static const char *const WHEN[] = {"initialize", "per-call", "per-process"};
        static const char *const STATUS[] = {"default-path", "test-aid", "profiling-aid", "rejected"};
        std::string out;
        char val[160];
        for (int r = 0, nr = nrows(); r < nr; r++) {
            const Row &w = rows()[r];
            if (w.kind == FLAG) snprintf(val, sizeof val, "%d", this->*w.b ? 1 : 0);
            else if (w.kind == INT) snprintf(val, sizeof val, "%d", this->*w.i);
            else if (w.kind == REAL) snprintf(val, sizeof val, "%.10g", this->*w.d);
            else if (w.kind == TEXT) snprintf(val, sizeof val, "%.150s", (this->*w.s).c_str());
            else snprintf(val, sizeof val, "%d,%d,%d,%.10g,%.10g,%.10g", relax_ncol[0], relax_ncol[1], relax_ncol[2], relax_zeros[0], relax_zeros[1], relax_zeros[2]);
            out += std::string(w.name) + "=" + val + " " + WHEN[w.when] + " " + STATUS[w.status] + (w.note[0] ? " " : "") + w.note + "\n";
        }
        if (buf && cap > 0) {
            const size_t k = std::min<size_t>(out.size(), (size_t)cap - 1);
            out.copy(buf, k);
            buf[k] = 0;
        }
        return (int64_t)out.size() + 1;
    }
};

} // namespace hipmf
