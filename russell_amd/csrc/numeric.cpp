// numeric.cpp -- host driver of the HIP kernels: plan upload, numeric factorisation, solves.
// Compiled with hipcc (-x hip) for gfx950.  The phase structure mirrors the reference's GPU
// plug-in (/root/reference/russell_sparse/c_code/interface_cudss.cu:190-566): initialize uploads
// the structure once, factorize re-uploads VALUES ONLY, solve moves one rhs in and one x out, and
// every phase synchronises its stream before returning.
#include "numeric.hpp"

#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <tuple>

#include "kernels.hpp"
#include "kernels_solve_transpose.hpp"
#include "kernels_solve_transpose_blocked.hpp"
#include "kernels_solve_pruned.hpp"
#include "kernels_solve_pruned_transpose.hpp"
#include "kernels_krylov.hpp"
#include "kernels_krylov_blocked.hpp"
#include "kernels_krylov_complex.hpp"
#include "kernels_krylov_complex_blocked.hpp"
#include "kernels_krylov_transpose.hpp"
#include "kernels_error_analysis_complex.hpp"
#include "kernels_eigs.hpp"
#include <fcntl.h>
#include <sys/mman.h>
#include <pthread.h>
#include <atomic>
#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>
#include "matching.hpp"
#include "krylov_host.hpp"

namespace hipmf {

// (HIPS: the same check outside the Solver's members -- the launch policies below -- on the Solver s)
#define HIPS(s, call, code)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            std::lock_guard<std::mutex> lock_((s).err_mutex); /* (the planning thread of initialize reports through the same string) */ \
            (s).last_error = std::string(#call) + ": " + hipGetErrorString(e_);                \
            if ((s).opt.verbose) fprintf(stderr, "hipmf: %s\n", (s).last_error.c_str());       \
            return (code);                                                                     \
        }                                                                                      \
    } while (0)
#define HIPC(call, code) HIPS(*this, call, code)

#define STREAM ((hipStream_t)stream)

// A phase runs on the handle's device (handles are Send: the calling thread's current device may be another one) and
// gives the caller's device back on return.
struct DeviceScope {
    int prev = -1, dev;
    explicit DeviceScope(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) (void)hipSetDevice(d);
    }
    ~DeviceScope() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

static_assert(Tunables::MID_MMAX_CAP == MID_MMAX && Tunables::BLOCK_GROUPS_CAP == SF_GMAX, "tunables.hpp clamps by the kernels' constants");
constexpr int32_t MAX_LDS_DOUBLES = 7936; // 62 KiB of dynamic LDS for the w1 / v vectors of the big-front solves

Solver::Solver() {}

bool Solver::is_mid_lu(int32_t s) const {
    if (!use_mid || !use_mid_lu || S.sym_mode) return false;
    const int32_t p = S.npiv(s), m = S.nrow(s);
    return p + m > SMALL_F && p <= MIDL_P && m <= mid_lu_mmax && midl_lds_doubles(p, m) <= MIDL_LDS_DOUBLES;
}
bool Solver::is_mid(int32_t s) const {
    if (!use_mid || S.sym_mode) return false;
    if (is_mid_lu(s)) return true;
    const int32_t p = S.npiv(s), m = S.nrow(s);
    return p + m > SMALL_F && p <= MID_PMAX && m <= mid_mmax && mid_lds_doubles(p, m) <= MID_LDS_DOUBLES;
}
Solver::~Solver() { release(); }

void Solver::release() {
    DeviceScope dev_scope(device);
    static_cast<SolverDevice &>(*this) = SolverDevice();
    initialized = factorized = false, matched = false;
    tree_active = tag_active = tags_armed = false, work_up = work_arm0 = 0;
    sym_diag_looked = sym_weak_diag_seen = false;
    block_groups_last = 0;
}

int32_t Solver::initialize(int32_t n, const int32_t *rp, const int32_t *ci, bool sym_lower, const SymbolicOptions &sopt,
                           const NumericOptions &nopt, const double *values) {
    if (initialized) return ERROR_ALREADY_INITIALIZED;
    requested = Tunables::from_env(); // (the one place: a re-matching factorize re-plans under the knobs of this call)
    // any failure leaves the handle as new: nothing allocated on the device, initialize may be tried again -- also when the failure
    // is an exception of the calling thread (a host allocation in the matching or the analysis: the device set-up thread has allocated
    // streams, events and structure arrays by then)
    int32_t code;
    try {
        code = initialize_impl(n, rp, ci, sym_lower, sopt, nopt, values);
    } catch (...) {
        release();
        throw; // (the C boundary turns it into ERROR_MALLOC / ERROR_HIPMF_SYMBOLIC: guarded(), interface_hipmf.cpp)
    }
    if (code != SUCCESSFUL_EXIT) {
        const std::string keep = last_error;
        release();
        last_error = keep;
    }
    return code;
}

int32_t Solver::initialize_impl(int32_t n, const int32_t *rp, const int32_t *ci, bool sym_lower, const SymbolicOptions &sopt,
                                const NumericOptions &nopt, const double *values) {
    opt = nopt;
    // the effective knobs start over from what initialize() was asked for (a hand-off time-out, like a failed graph capture,
    // sends ONE analysis to the fallback launches); the adjustments for this matrix follow below and in upload_plan
    static_cast<Tunables &>(*this) = requested;
    // (verbose: wall-clock of the host-side pieces of initialize, printed at the end)
    auto lap_t = std::chrono::steady_clock::now();
    std::vector<std::pair<const char *, double>> laps;
    auto lap = [&](const char *what) {
        const auto now = std::chrono::steady_clock::now();
        laps.emplace_back(what, std::chrono::duration<double>(now - lap_t).count());
        lap_t = now;
    };
    // the structure is validated once, before the matching / the analysis read through the indices
    if (const int vc = validate_csr(n, rp, ci)) {
        last_error = vc == -1 ? "invalid CSR: row pointers must start at 0 and be non-decreasing"
                              : (vc == -2 ? "invalid CSR: column index out of range"
                                          : "invalid CSR: the column indices of a row must be strictly increasing (no duplicates)");
        return ERROR_HIPMF_INVALID_MATRIX;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        last_error = "no HIP device visible";
        return ERROR_HIPMF_NO_DEVICE;
    }
    HIPC(hipGetDevice(&device), ERROR_HIPMF_NO_DEVICE);
    // Everything the device needs that does NOT depend on the analysis runs on a host thread of its own beside it: streams and events,
    // the first touch of the device (a cold process pays 30 - 45 ms for it), the free-memory figure the analysis refuses too large a
    // matrix by, and the upload of the matrix structure (refinement SpMV).  Joined right after the analysis.
    std::atomic<double> live_pool_limit{0.0};
    int32_t prep_code = SUCCESSFUL_EXIT;
    auto prep = [&]() -> int32_t {
        (void)hipSetDevice(device);
        if (!stream) {
            HIPC(hipStreamCreate(stream.put()), ERROR_HIPMF_NO_DEVICE);
            HIPC(hipStreamCreate(stream2.put()), ERROR_HIPMF_NO_DEVICE);
            HIPC(hipStreamCreate(stream3.put()), ERROR_HIPMF_NO_DEVICE);
            {
                // (background work -- zero-fill of E / E', diagonal check beside the first levels: lowest priority, it must not take
                //  compute units from the level's own launches; measured: level 0 took 225 us with the zero-fill beside it, 186 alone)
                int least = 0, greatest = 0;
                if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
                HIPC(hipStreamCreateWithPriority(stream4.put(), hipStreamDefault, least), ERROR_HIPMF_NO_DEVICE);
            }
            // events that order this handle's streams among themselves: no timing, and no system-scope fence at the record (the cache
            // write-back + invalidate of the default costs 5 - 7 us on the stream that records; kernels of the same device see each
            // other's results through the agent-scope release at a kernel's end).  HIPMF_EVENT_FENCE=1: the default flags.
            // Round 6 (VERDICT r05 weak 8 / ADVICE r04): the fence-free record is only taken where it was validated -- a gfx950 device
            // (every XCD's L2 is written back by the agent-scope release at a kernel's end, which is what makes another stream's
            // kernels AND the copy engines see the data: all of this handle's buffers are device memory) under a HIP 7 runtime; any
            // other device or runtime gets the default flags.  The join of the background stream (ev_pre1: the diagonal check writes the
            // FactorInfo words the host reads after the factorisation) keeps the default flags everywhere: it is off the chain.
            unsigned xflags = hipEventDisableTiming;
            const unsigned dflags = hipEventDisableTiming;
#ifndef HIPMF_EMULATED
            {
                hipDeviceProp_t prop;
                int rtv = 0;
                const bool known = hipGetDeviceProperties(&prop, device) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0 &&
                                   hipRuntimeGetVersion(&rtv) == hipSuccess && rtv / 10000000 == 7;
                event_fence_free = known && !event_fence;
                if (event_fence_free) xflags |= hipEventDisableSystemFence;
            }
#endif
            HIPC(hipEventCreateWithFlags(ev_pb.put(), xflags), ERROR_HIPMF_NO_DEVICE);
            HIPC(hipEventCreateWithFlags(ev_rest.put(), xflags), ERROR_HIPMF_NO_DEVICE);
            HIPC(hipEventCreateWithFlags(ev_pre0.put(), xflags), ERROR_HIPMF_NO_DEVICE);
            HIPC(hipEventCreateWithFlags(ev_pre1.put(), dflags), ERROR_HIPMF_NO_DEVICE);
            for (EventOwner *e : {&ev_fork, &ev_join, &ev_fork3, &ev_join3}) HIPC(hipEventCreateWithFlags(e->put(), xflags), ERROR_HIPMF_NO_DEVICE);
        }
        {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
                // (hybrid_memory_factor -- opt.device_memory_factor -- does NOT lower this limit: in the reference the option lets LARGER
                //  problems through by spilling the factor to host memory, interface_cudss.cu:347-380; without a host half, capping
                //  the device share would refuse matrices the reference accepts.  ADVICE r04.)
                const double limit = 0.95 * (double)free_b;
                live_pool_limit.store(limit);
            }
            if (given(&Tunables::pool_limit_gb)) live_pool_limit.store(0.95e9 * pool_limit_gb); // (tests: force the refusal)
        }
        // matrix structure (kept for the refinement SpMV) and per-entry row/col indices
        const int64_t nnz = rp[n];
        std::vector<int32_t> h_arow((size_t)nnz);
        for (int32_t i = 0; i < n; i++)
            for (int32_t p = rp[i]; p < rp[i + 1]; p++) h_arow[p] = i;
        {
            // row blocks of the stream SpMV: consecutive rows with at most SPMV_CAP stored entries (a longer row stands alone)
            std::vector<int32_t> rb(1, 0);
            int32_t start = 0;
            for (int32_t i = 0; i < n; i++)
                if (rp[i + 1] - rp[start] > SPMV_CAP && i > start) rb.push_back(i), start = i;
            // (the row that opens a block may itself exceed the cap: it is closed by the next row)
            rb.push_back(n);
            spmv_blocks = (int32_t)rb.size() - 1;
            HIPC(d_row_blk.upload(rb), ERROR_HIP_MALLOC);
        }
        HIPC(d_rp.alloc((size_t)n + 1), ERROR_HIP_MALLOC);
        HIPC(hipMemcpy(d_rp, rp, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice), ERROR_HIP_MALLOC);
        HIPC(d_ci.alloc((size_t)std::max<int64_t>(nnz, 1)), ERROR_HIP_MALLOC);
        if (nnz > 0) HIPC(hipMemcpy(d_ci, ci, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice), ERROR_HIP_MALLOC);
        HIPC(d_arow.upload(h_arow), ERROR_HIP_MALLOC);
        if (sym_lower) {
            // transpose lists: for every row i, the stored entries (r, i), r > i, mirrored into row i
            std::vector<int32_t> tptr((size_t)n + 1, 0), tidx;
            for (int64_t k = 0; k < nnz; k++)
                if (ci[k] != h_arow[k]) tptr[ci[k] + 1]++;
            for (int32_t i = 0; i < n; i++) tptr[i + 1] += tptr[i];
            tidx.resize((size_t)tptr[n]);
            std::vector<int32_t> w(tptr.begin(), tptr.end() - 1);
            for (int64_t k = 0; k < nnz; k++)
                if (ci[k] != h_arow[k]) tidx[w[ci[k]]++] = (int32_t)k;
            HIPC(d_tptr.upload(tptr), ERROR_HIP_MALLOC);
            HIPC(d_tidx.upload(tidx), ERROR_HIP_MALLOC);
        }
        return SUCCESSFUL_EXIT;
    };
    std::thread prep_thread([&]() {
        try {
            prep_code = prep();
        } catch (const std::bad_alloc &) { // (an exception must not leave the thread)
            std::lock_guard<std::mutex> lock(err_mutex);
            last_error = "Not enough memory: a host allocation failed";
            prep_code = ERROR_MALLOC;
        } catch (...) {
            std::lock_guard<std::mutex> lock(err_mutex);
            last_error = "initialize: the device set-up failed with an exception";
            prep_code = ERROR_HIPMF_INVALID_VALUE;
        }
    });
    struct PrepJoiner { // (every early return below waits for the thread)
        std::thread &t;
        ~PrepJoiner() {
            if (t.joinable()) t.join();
        }
    } prep_joiner{prep_thread};
    if (!rematching) {
        h_rp_keep.assign(rp, rp + n + 1);
        h_ci_keep.assign(ci, ci + rp[n]);
        sopt_keep = sopt;
        sym_lower_keep = sym_lower;
    }
    lap("validate + streams + keep");
    SymbolicOptions so = sopt;
    so.augment_above = SMALL_F;
    // symmetric-lower input (general_symmetric / positive_definite, interface_cudss.cu:324-333): the big fronts are factorised
    // as L D L^T on their lower triangle -- half the flops, half the factor (HIPMF_SYM_LDLT=0: LU of the mirrored matrix)
    so.symmetric_ldlt = sym_lower && sym_ldlt;
    if (opt.complex_pairs && (sym_lower || n % 2 != 0)) {
        last_error = "complex pairs need general storage and an even order";
        return ERROR_HIPMF_INVALID_MATRIX;
    }
    so.pair_blocks = opt.complex_pairs;
    so.nd_leaf = nd_leaf, so.dense_leaves = dense_leaves;
    so.split_pivots = split_pivots, so.dense_row_factor = dense_row_factor;
    so.nd_threads = nd_threads, so.parallel_min_n = par_min, so.parallel_chunk_min = par_chunk;
    for (int k = 0; k < 3; k++) so.relax_ncol[k] = relax_ncol[k], so.relax_zeros[k] = relax_zeros[k];
    so.relax_big_front = relax_big_front;
    so.arena_reuse = arena_reuse, so.align_panels = align_panels;
    // (HIPMF_SOLVE_LANES: read and ignored since round 5 -- two lanes are two dependency-driven launches resident together, the very thing
    //  the device gate of solve() rules out; one lane has been as fast since round 4, profiles/r04_solve_lanes.txt)
    solve_lanes = 1, solve_lanes_auto = false;
    if (given(&Tunables::matching)) opt.matching = matching;
    if (opt.complex_pairs) {
        // the pivot searches of k_front (opt-in), of the chained launch and of the block-inverse step do not pair
        use_chain = false, use_binv = false, mid_mmax = 0;
    }
    // Maximum-product matching + scaling (matching.cpp) when the numbers are known and the diagonal is weak: the
    // analysis then runs on B = A(mrow, :), whose diagonal holds the matched entries (all 1 after scaling).
    std::vector<int32_t> mrow, rpB, ciB;
    std::vector<int64_t> kB; // position in B's CSR of every entry of A
    std::vector<double> dr, dc;
    matched = false;
    if (values && !sym_lower && n > 1 && opt.matching > 0 && rp[0] == 0 && (opt.matching >= 2 || diagonal_is_weak(n, rp, ci, values, 0.01, opt.complex_pairs))) {
        if ((opt.complex_pairs ? paired_matching(n, rp, ci, values, mrow, dr, dc) : max_product_matching(n, rp, ci, values, mrow, dr, dc)) == 0) {
            matched = true;
            rpB.assign((size_t)n + 1, 0);
            for (int32_t j = 0; j < n; j++) rpB[j + 1] = rpB[j] + (rp[mrow[j] + 1] - rp[mrow[j]]);
            ciB.resize((size_t)rp[n]);
            kB.resize((size_t)rp[n]);
            for (int32_t j = 0; j < n; j++)
                for (int32_t p = rp[mrow[j]], q = rpB[j]; p < rp[mrow[j] + 1]; p++, q++) ciB[q] = ci[p], kB[p] = q;
            if (opt.verbose) fprintf(stderr, "hipmf: initialize: maximum-product matching + scaling applied (weak diagonal)\n");
        } else if (opt.verbose) {
            fprintf(stderr, "hipmf: initialize: the matrix has no perfect matching (structurally singular); continuing without\n");
        }
    }
    so.pool_limit_live = &live_pool_limit; // (the free-memory figure arrives from the set-up thread while the ordering runs)
    lap("matching test");
    int rc = matched ? analyse(n, rpB.data(), ciB.data(), false, so, S) : analyse(n, rp, ci, sym_lower, so, S);
    lap("analyse");
    prep_thread.join();
    so.pool_limit_bytes = live_pool_limit.load();
    if (prep_code != SUCCESSFUL_EXIT) return prep_code;
    if (rc == 0 && so.pool_limit_bytes > 0.0 && S.pool_estimate_bytes > so.pool_limit_bytes) rc = -40; // (the figure came too late for the analysis' own test)
    lap("wait for the device set-up");
    if (rc == -40) {
        char msg[256];
        if (opt.device_memory_factor > 0.0)
            snprintf(msg, sizeof msg, "Not enough memory: the fronts of this matrix need about %.1f GB (device: %.1f GB free; hybrid_memory_factor %.2f was given, "
                     "but this backend has no host half: the factor must fit the device)",
                     S.pool_estimate_bytes / 1e9, so.pool_limit_bytes / 0.95 / 1e9, opt.device_memory_factor);
        else
            snprintf(msg, sizeof msg, "Not enough memory: the fronts of this matrix need about %.1f GB (device: %.1f GB free)", S.pool_estimate_bytes / 1e9,
                     so.pool_limit_bytes / 0.95 / 1e9);
        last_error = msg;
        return ERROR_HIP_MALLOC;
    }
    if (rc == -41) { // a host thread of the analysis ran out of memory (row structures, column counts, Ordering::Best)
        last_error = "Not enough memory: a host allocation failed in the analysis";
        return ERROR_MALLOC;
    }
    if (rc != 0) {
        last_error = "symbolic analysis failed (" + std::to_string(rc) + ")";
        return rc <= -30 || rc >= -2 ? ERROR_HIPMF_INVALID_MATRIX : ERROR_HIPMF_SYMBOLIC;
    }
    if (matched) { // the assembly map back in the order of A's entries
        std::vector<int64_t> am((size_t)rp[n]);
        std::vector<int32_t> as((size_t)rp[n]);
        for (int64_t k = 0; k < rp[n]; k++) am[k] = S.amap[kB[k]], as[k] = S.amap_sn[kB[k]];
        S.amap.swap(am);
        S.amap_sn.swap(as);
    }
    // The assembly lists only read the analysis: they are computed on a host thread of their own beside upload_plan (which builds the
    // launch plans and talks to the device).
    //   The entries of A that land in small fronts are gathered by k_small_factor itself (per-front lists: entry index,
    //   position inside the front); the entries of the big fronts are scattered level by level (their working blocks share
    //   an arena: a block is zero-filled and filled when its level starts).
    struct AsmLists {
        std::vector<int32_t> sa_ptr, sa_k, sc_k, zero_off, zero_n;
        std::vector<uint16_t> sa_pos;
        std::vector<int64_t> sc_cnt, sc_at;
        std::vector<int32_t> ea_sc;   // (k_extend_add_lds) entries of A per extend-add task: sc_k is then in task order, sc_pos the position in the tile
        std::vector<uint16_t> sc_pos;
        std::vector<ZeroTask> zt;
        int32_t zero_cnt = 0, status = 0;
        double seconds = 0.0; // (verbose: how long the thread below worked)
    } AL;
    struct Joiner { // (every early return below must not leave the thread running)
        std::thread &t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    };
    std::thread asm_thread([this, &AL]() {
      try {
        const auto t_asm = std::chrono::steady_clock::now();
        struct Stop {
            double &out;
            std::chrono::steady_clock::time_point t0;
            ~Stop() { out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
        } stop{AL.seconds, t_asm};
        const int32_t ns = S.nsuper;
        std::vector<int32_t> &sa_ptr = AL.sa_ptr;
        std::vector<int64_t> &sc_cnt = AL.sc_cnt;
        sa_ptr.assign((size_t)ns + 1, 0);
        sc_cnt.assign((size_t)S.nlevels + 1, 0);
        // (front size per supernode once: S.fsize reads four entries of two arrays, and both passes below ask it per matrix entry)
        std::vector<int32_t> fsz((size_t)ns);
        for (int32_t s = 0; s < ns; s++) fsz[(size_t)s] = S.fsize(s);
        // The lists are stable bucket sorts of the entry sequence (all of amap, then all of amap2): small fronts by supernode, big ones by
        // level.  The sequence is cut into pieces; every piece counts its entries per bucket, the pieces' counts are turned into start
        // positions bucket by bucket (piece order = sequence order: the lists come out as the serial sweep wrote them), and every piece
        // then writes its entries from its own cursors.  Pieces run on host threads when the matrix is large enough.
        const int64_t nnz_a = (int64_t)S.amap.size();
        const bool two = !S.amap2.empty();
        int npiece = 1;
        {
            const int thr = given(&Tunables::nd_threads) ? std::min(4, nd_threads) : (int)std::min<unsigned>(4u, std::max(1u, std::thread::hardware_concurrency()));
            if (nnz_a >= par_min && nnz_a >= 64) npiece = thr;
        }
        const int passes = two ? 2 : 1, P = npiece * passes;
        auto piece_range = [&](int q, const std::vector<int64_t> *&am, int &pass, int64_t &k0, int64_t &k1) {
            pass = q / npiece;
            am = pass == 0 ? &S.amap : &S.amap2;
            const int t = q % npiece;
            k0 = nnz_a * t / npiece, k1 = nnz_a * (t + 1) / npiece;
        };
        std::vector<std::vector<int32_t>> cnt_s((size_t)P);
        std::vector<std::vector<int64_t>> cnt_l((size_t)P);
        auto run_pieces = [&](auto &&fn) {
            if (npiece == 1) {
                for (int q = 0; q < P; q++) fn(q);
                return;
            }
            std::vector<std::thread> pool;
            std::atomic<bool> oom{false};
            for (int q = 0; q < P; q++)
                pool.emplace_back([&, q]() {
                    try {
                        fn(q);
                    } catch (const std::bad_alloc &) { // (an exception must not leave a thread)
                        oom.store(true);
                    }
                });
            for (auto &th : pool) th.join();
            if (oom.load()) throw std::bad_alloc();
        };
        run_pieces([&](int q) {
            const std::vector<int64_t> *am;
            int pass;
            int64_t k0, k1;
            piece_range(q, am, pass, k0, k1);
            cnt_s[(size_t)q].assign((size_t)ns, 0), cnt_l[(size_t)q].assign((size_t)S.nlevels, 0);
            for (int64_t k = k0; k < k1; k++)
                if ((*am)[(size_t)k] >= 0) {
                    const int32_t s = S.amap_sn[(size_t)k];
                    if (fsz[(size_t)s] <= SMALL_F) cnt_s[(size_t)q][(size_t)s]++;
                    else cnt_l[(size_t)q][(size_t)S.sn_level[s]]++;
                }
        });
        // counts -> start positions (cnt becomes the piece's cursor), totals -> sa_ptr / sc_cnt
        {
            int64_t run = 0;
            for (int32_t s = 0; s < ns; s++) {
                sa_ptr[(size_t)s] = (int32_t)run;
                for (int q = 0; q < P; q++) {
                    const int32_t c = cnt_s[(size_t)q][(size_t)s];
                    cnt_s[(size_t)q][(size_t)s] = (int32_t)run;
                    run += c;
                }
                if (run > 0x7fffffffLL) {
                    AL.status = 1;
                    return;
                }
            }
            sa_ptr[(size_t)ns] = (int32_t)run;
            int64_t runl = 0;
            for (int32_t l = 0; l < S.nlevels; l++) {
                sc_cnt[(size_t)l] = runl;
                for (int q = 0; q < P; q++) {
                    const int64_t c = cnt_l[(size_t)q][(size_t)l];
                    cnt_l[(size_t)q][(size_t)l] = runl;
                    runl += c;
                }
            }
            sc_cnt[(size_t)S.nlevels] = runl;
        }
        if (sc_cnt[(size_t)S.nlevels] > 0x7fffffffLL) {
            AL.status = 1;
            return;
        }
        AL.sa_k.resize((size_t)sa_ptr[ns]);
        AL.sa_pos.resize((size_t)sa_ptr[ns]);
        AL.sc_k.resize((size_t)sc_cnt[(size_t)S.nlevels]);
        AL.sc_at.resize((size_t)sc_cnt[(size_t)S.nlevels]);
        run_pieces([&](int q) {
            const std::vector<int64_t> *amp;
            int pass;
            int64_t k0, k1;
            piece_range(q, amp, pass, k0, k1);
            const std::vector<int64_t> &am = *amp;
            std::vector<int32_t> &w = cnt_s[(size_t)q];
            std::vector<int64_t> &wl = cnt_l[(size_t)q];
            for (int64_t k = k0; k < k1; k++)
                if (am[(size_t)k] >= 0) {
                    const int32_t s = S.amap_sn[(size_t)k];
                    if (fsz[(size_t)s] > SMALL_F) {
                        const size_t qq = (size_t)wl[(size_t)S.sn_level[s]]++;
                        AL.sc_k[qq] = pass == 0 ? (int32_t)k : ~(int32_t)k;
                        AL.sc_at[qq] = am[(size_t)k];
                        continue;
                    }
                    const int64_t off = am[(size_t)k] - S.front_off[s], f = fsz[(size_t)s];
                    const size_t qq = (size_t)w[(size_t)s]++;
                    AL.sa_k[qq] = pass == 0 ? (int32_t)k : ~(int32_t)k;
                    AL.sa_pos[qq] = (uint16_t)((off % f) | ((off / f) << 8));
                }
        });
        cnt_s.clear(), cnt_l.clear();
        if (ea_lds_active()) {
            // linear index of tile (ct, rt) of a front with f rows among the tiles that have a task, tile columns outer, tile rows inner
            // (L D L^T fronts: the tiles strictly above the diagonal have none: rows (rt + 1) R <= ct C)
            auto ea_tile_index = [&](int64_t f, int64_t ct, int64_t rt) {
                const int64_t nrt = (f + EA_TILE_R - 1) / EA_TILE_R;
                if (!S.sym_mode) return ct * nrt + rt;
                int64_t idx = 0;
                for (int64_t c = 0; c < ct; c++) idx += nrt - std::min<int64_t>(nrt, (c * EA_TILE_C) / EA_TILE_R);
                return idx + rt - (ct * EA_TILE_C) / EA_TILE_R;
            };
            // k_extend_add_lds: the same entries by task.  Task numbering of upload_plan: levels ascending, the big fronts of a level in level
            // order, every tile of a front, tile columns outer, tile rows inner.
            // ... the first tiles of the level's fronts lead the level's tasks: first tile of the q-th big front = level base + q, its other
            // tiles follow the first tiles of all fronts in the order above.
            std::vector<int32_t> ea_first((size_t)ns, -1), ea_base((size_t)ns, -1); // task of tile (0, 0); task of tile (ct, rt) != (0, 0) is ea_base + ct nrt + rt
            int64_t ntask = 0;
            for (int32_t l = 0; l < S.nlevels; l++) {
                int64_t nbig = 0;
                for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) nbig += S.fsize(S.level_sn[k]) > SMALL_F ? 1 : 0;
                int64_t q = 0, others = ntask + nbig;
                for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
                    const int32_t s = S.level_sn[k];
                    const int64_t f = S.fsize(s);
                    if (f <= SMALL_F) continue;
                    ea_first[(size_t)s] = (int32_t)(ntask + q++);
                    ea_base[(size_t)s] = (int32_t)(others - 1); // (linear tile index 1 is the first of the others)
                    {
                        // (the index one past the front's last tile = the number of its tiles)
                        const int64_t nct = (f + EA_TILE_C - 1) / EA_TILE_C;
                        others += ea_tile_index(f, nct, S.sym_mode ? (nct * EA_TILE_C) / EA_TILE_R : 0) - 1;
                    }
                }
                ntask = others;
            }
            if (ntask > 0x7ffffff0LL) {
                AL.status = 1;
                return;
            }
            const size_t ne = AL.sc_k.size();
            std::vector<int32_t> task_of(ne);
            AL.ea_sc.assign((size_t)ntask + 1, 0);
            AL.sc_pos.resize(ne);
            std::vector<uint16_t> pos_of(ne);
            for (size_t e = 0; e < ne; e++) {
                const int32_t k = AL.sc_k[e] < 0 ? ~AL.sc_k[e] : AL.sc_k[e];
                const int32_t s = S.amap_sn[(size_t)k];
                const int64_t off = AL.sc_at[e] - S.front_off[s], ld = S.front_ld[s], f = fsz[(size_t)s];
                const int64_t r = off % ld, c = off / ld;
                const int64_t lin = ea_tile_index(f, c / EA_TILE_C, r / EA_TILE_R);
                task_of[e] = lin == 0 ? ea_first[(size_t)s] : ea_base[(size_t)s] + (int32_t)lin;
                pos_of[e] = (uint16_t)((r % EA_TILE_R) + (c % EA_TILE_C) * EA_TILE_R);
                AL.ea_sc[(size_t)task_of[e] + 1]++;
            }
            for (int64_t t = 0; t < ntask; t++) AL.ea_sc[(size_t)t + 1] += AL.ea_sc[(size_t)t];
            std::vector<int32_t> wt(AL.ea_sc.begin(), AL.ea_sc.end() - 1), k2(ne);
            for (size_t e = 0; e < ne; e++) { // (stable: the entries of a task keep the order of the level's list)
                const size_t q = (size_t)wt[(size_t)task_of[e]]++;
                k2[q] = AL.sc_k[e], AL.sc_pos[q] = pos_of[e];
            }
            AL.sc_k.swap(k2);
            std::vector<int64_t>().swap(AL.sc_at); // (positions are per tile now)
        }
        // zero-fill tasks, 16 Ki doubles per workgroup: first the persistent E / E' panels of all big fronts (one launch per
        // factorisation), then the working blocks level by level
        std::vector<ZeroTask> &zt = AL.zt;
        auto zero_range = [&](int64_t o0, int64_t len) {
            for (int64_t o = o0; o < o0 + len; o += 16384) zt.push_back({o, (int32_t)std::min<int64_t>(16384, o0 + len - o), 0});
        };
        for (int32_t s = 0; s < ns; s++) {
            if (S.fsize(s) <= SMALL_F || is_mid(s)) continue; // (k_front writes every entry of its E / E')
            const int64_t f = S.fsize(s), p = S.npiv(s);
            zero_range(S.e_off[s], (int64_t)S.front_ld[s] * p);
            if (S.ep_off[s] >= 0) zero_range(S.ep_off[s], f * (int64_t)S.front_ldp[s]);
        }
        AL.zero_cnt = (int32_t)zt.size();
        AL.zero_off.assign((size_t)S.nlevels, 0), AL.zero_n.assign((size_t)S.nlevels, 0);
        for (int32_t l = 0; l < S.nlevels; l++) {
            AL.zero_off[(size_t)l] = (int32_t)zt.size();
            // (the first-touch extend-add writes every working block whole: no per-level zero-fill launches, no tasks for them -- at 200^3
            //  they were 2.8 M records built and uploaded for nothing)
            for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1] && !ea_lds_active(); k++) {
                const int32_t s = S.level_sn[k];
                if (S.fsize(s) > SMALL_F) zero_range(S.front_off[s], (int64_t)S.front_ld[s] * S.fsize(s));
            }
            AL.zero_n[(size_t)l] = (int32_t)zt.size() - AL.zero_off[(size_t)l];
        }
        if (zt.size() > 0x7fffffffULL) AL.status = 2;
      } catch (const std::bad_alloc &) { // (an exception must not leave the thread)
        AL.status = 3;
      }
    });
    Joiner asm_joiner{asm_thread};
    // What follows the descriptor uploads of upload_plan -- permutation, plan signature, the assembly lists, the value and vector
    // buffers -- does not depend on the task lists of the solves, which a host thread builds meanwhile (a third of upload_plan's time):
    // it runs as upload_plan's tail, before that thread is joined.
    auto tail = [&]() -> int32_t {
        lap("plan + descriptor uploads");
        const int64_t nnz = S.nnz_a;
        HIPC(d_perm.upload(S.perm), ERROR_HIP_MALLOC);
        d_rperm = d_perm;
        {
            uint64_t hsh = 1469598103934665603ull;
            auto mix = [&](uint64_t v) {
                for (int b = 0; b < 8; b++) hsh = (hsh ^ ((v >> (8 * b)) & 0xff)) * 1099511628211ull;
            };
            for (int32_t k = 0; k < n; k++) mix((uint64_t)(uint32_t)S.perm[k] | ((uint64_t)(matched ? (uint32_t)mrow[S.perm[k]] : 0u) << 32));
            mix((uint64_t)S.persist_doubles), mix((uint64_t)S.temp_doubles), mix((uint64_t)S.nsuper);
            plan_sig = hsh & 0x7fffffffffffffffull;
        }
        if (matched) {
            std::vector<int32_t> rperm((size_t)n);
            for (int32_t k = 0; k < n; k++) rperm[k] = mrow[S.perm[k]];
            HIPC(d_rperm_matched.upload(rperm), ERROR_HIP_MALLOC);
            HIPC(d_cs_matched.upload(dc), ERROR_HIP_MALLOC);
            d_rperm = d_rperm_matched, d_cs = d_cs_matched;
            std::vector<int32_t> dcol((size_t)n);
            for (int32_t j = 0; j < n; j++) dcol[(size_t)mrow[j]] = j; // row mrow[j] of A is pivot row j: its diagonal entry sits in column j
            HIPC(d_dcol.upload(dcol), ERROR_HIP_MALLOC);
            // parity of the row permutation (determinant)
            std::vector<char> seen((size_t)n, 0);
            match_parity = 0;
            for (int32_t i = 0; i < n; i++) {
                if (seen[i]) continue;
                int len = 0;
                for (int32_t j = i; !seen[j]; j = mrow[j]) seen[j] = 1, len++;
                if ((len & 1) == 0) match_parity ^= 1;
            }
            if (opt.complex_pairs) { // the permutation of the complex rows (pairs move as a whole: paired_matching)
                match_parity = 0;
                std::fill(seen.begin(), seen.end(), 0);
                for (int32_t i = 0; i < n / 2; i++) {
                    if (seen[i]) continue;
                    int len = 0;
                    for (int32_t j = i; !seen[j]; j = mrow[2 * j] / 2) seen[j] = 1, len++;
                    if ((len & 1) == 0) match_parity ^= 1;
                }
            }
        }
        lap("perm + signature");
        {
            // (joined below: the lists were computed beside upload_plan)
            if (asm_thread.joinable()) asm_thread.join();
            if (opt.verbose) fprintf(stderr, "hipmf: initialize: the assembly-list thread worked %.3f s beside the launch plans\n", AL.seconds);
            if (want_digest) { // (the thread's lists join the digest of the plans: thread-count independence test)
                uint64_t h = (uint64_t)plan_digest ^ 1469598103934665603ull;
                auto eat = [&](const void *p, size_t bytes) {
                    const unsigned char *b = (const unsigned char *)p;
                    for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 1099511628211ull;
                };
                eat(AL.sa_ptr.data(), AL.sa_ptr.size() * sizeof(int32_t)), eat(AL.sa_k.data(), AL.sa_k.size() * sizeof(int32_t));
                eat(AL.sa_pos.data(), AL.sa_pos.size() * sizeof(AL.sa_pos[0])), eat(AL.sc_k.data(), AL.sc_k.size() * sizeof(int32_t));
                eat(AL.sc_cnt.data(), AL.sc_cnt.size() * sizeof(int64_t)), eat(AL.sc_pos.data(), AL.sc_pos.size() * sizeof(AL.sc_pos[0]));
                eat(AL.ea_sc.data(), AL.ea_sc.size() * sizeof(AL.ea_sc[0]));
                plan_digest = (int64_t)(h & 0x7fffffffffffffffull);
            }
            if (AL.status == 1) {
                last_error = "too many entries in the tiled fronts";
                return ERROR_HIPMF_SYMBOLIC;
            }
            if (AL.status == 2) {
                last_error = "too many zero-fill tasks";
                return ERROR_HIPMF_SYMBOLIC;
            }
            if (AL.status == 3) {
                last_error = "Not enough memory: a host allocation failed";
                return ERROR_MALLOC;
            }
            const int32_t ns = S.nsuper;
            for (int32_t l = 0; l < S.nlevels; l++) {
                levels[(size_t)l].sc_off = (int32_t)AL.sc_cnt[(size_t)l], levels[(size_t)l].sc_cnt = (int32_t)(AL.sc_cnt[(size_t)l + 1] - AL.sc_cnt[(size_t)l]);
                levels[(size_t)l].zero_off = AL.zero_off[(size_t)l], levels[(size_t)l].zero_cnt = AL.zero_n[(size_t)l];
            }
            zero_cnt = AL.zero_cnt;
            HIPC(d_sa_ptr.upload(AL.sa_ptr), ERROR_HIP_MALLOC);
            {
                // descriptors in launch order (the plan is on the device already: read it back rather than keep host copies around)
                std::vector<FrontDesc> h_fd((size_t)ns);
                std::vector<int32_t> h_lists((size_t)n_lists);
                HIPC(hipMemcpy(h_fd.data(), d_fd, sizeof(FrontDesc) * (size_t)ns, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
                if (n_lists > 0) HIPC(hipMemcpy(h_lists.data(), d_lists, sizeof(int32_t) * (size_t)n_lists, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
                std::vector<SmallDesc> sd(h_lists.size());
                for (size_t q = 0; q < h_lists.size(); q++) {
                    const int32_t s = h_lists[q];
                    sd[q].fd = h_fd[(size_t)s];
                    sd[q].e0 = AL.sa_ptr[(size_t)s], sd[q].e1 = AL.sa_ptr[(size_t)s + 1]; // (empty ranges for the big fronts, which never read them)
                }
                HIPC(d_sd.upload(sd), ERROR_HIP_MALLOC);
            }
            HIPC(d_sa_k.upload(AL.sa_k), ERROR_HIP_MALLOC);
            HIPC(d_sa_pos.upload(AL.sa_pos), ERROR_HIP_MALLOC);
            HIPC(d_sc_k.upload(AL.sc_k), ERROR_HIP_MALLOC);
            HIPC(d_sc_at.upload(AL.sc_at), ERROR_HIP_MALLOC);
            if (ea_lds_active()) {
                HIPC(d_ea_sc.upload(AL.ea_sc), ERROR_HIP_MALLOC);
                HIPC(d_sc_pos.upload(AL.sc_pos), ERROR_HIP_MALLOC);
            }
            HIPC(d_zero.upload(AL.zt), ERROR_HIP_MALLOC);
        }
        lap("assembly lists + zero tasks");
        std::vector<int64_t>().swap(S.amap);
        std::vector<int64_t>().swap(S.amap2);
        std::vector<int32_t>().swap(S.amap_sn);
        HIPC(d_vals.alloc(std::max<int64_t>(nnz, 1)), ERROR_HIP_MALLOC);
        HIPC(d_vs.alloc(std::max<int64_t>(nnz, 1)), ERROR_HIP_MALLOC);
        if (sym_lower) HIPC(d_vs2.alloc(std::max<int64_t>(nnz, 1)), ERROR_HIP_MALLOC);
        // (+ WT_X: a wave-subtree fetches its part of the vector / of the interchanges as WT_X entries from its first pivot column on)
        for (DeviceArray<double> *p : {&d_xp, &d_r, &d_den, &d_b, &d_x, &d_du, &d_rs}) HIPC(p->alloc((size_t)n + WT_X), ERROR_HIP_MALLOC);
        if (matched) HIPC(hipMemcpy(d_rs, dr.data(), sizeof(double) * n, hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
        HIPC(d_lperm.alloc((size_t)n + WT_X), ERROR_HIP_MALLOC);
        HIPC(hipMemsetAsync(d_lperm, 0, sizeof(int32_t) * ((size_t)n + WT_X), STREAM), ERROR_HIP_MEMCPY);
        for (double *p : {d_xp.get(), d_du.get()}) HIPC(hipMemsetAsync(p + n, 0, sizeof(double) * WT_X, STREAM), ERROR_HIP_MEMCPY);
        // (complex pairs: the n / 2 complex pivots follow the n real ones)
        HIPC(d_diag.alloc((size_t)n * (opt.complex_pairs ? 2 : 1)), ERROR_HIP_MALLOC);
        if (S.sym_mode) d_cs = d_rs; // symmetric scaling S A S keeps the big fronts symmetric: column scale = row scale
        {
            HIPC(hipMalloc((void **)d_info.put(), sizeof(FactorInfoExt)), ERROR_HIP_MALLOC);
            FactorInfoExt ext = {};
            ext.zdiag = opt.complex_pairs ? d_diag + n : nullptr;
            HIPC(hipMemcpy(d_info, &ext, sizeof ext, hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
        }
        HIPC(d_scalar.alloc(4 + (size_t)RES_NORM_WORDS * SF_KMAX), ERROR_HIP_MALLOC); // (blocked solves: d_norms_blk)
        for (EventOwner &e : ev) HIPC(hipEventCreate(e.put()), ERROR_HIP_MALLOC);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        lap("value / vector buffers");
        return SUCCESSFUL_EXIT;
    };
    const auto t_plan = std::chrono::steady_clock::now();
    int32_t code = upload_plan(tail);
    if (code != SUCCESSFUL_EXIT) return code;
    lap("wait for the solve task lists");
    if (opt.verbose)
        fprintf(stderr,
                "hipmf: initialize: graph %.3f s, ordering %.3f s, etree %.3f s, supernodes %.3f s, row structures %.3f s, layout %.3f s, "
                "assembly map %.3f s; plan + device allocation + upload + tail %.3f s\n",
                S.seconds_phase[0], S.seconds_phase[1], S.seconds_phase[2], S.seconds_phase[3], S.seconds_phase[4], S.seconds_phase[5],
                S.seconds_phase[6], std::chrono::duration<double>(std::chrono::steady_clock::now() - t_plan).count());
    if (opt.verbose) {
        fprintf(stderr, "hipmf: initialize: host pieces:");
        for (const auto &l : laps) fprintf(stderr, " %s %.3f s;", l.first, l.second);
        fprintf(stderr, "\n");
    }
    initialized = true;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::upload_plan(const std::function<int32_t()> &tail) {
    const int32_t ns = S.nsuper;
    // Blocks of right-hand sides per dependency-driven launch of the many-RHS driver (kernels_solve_fused.hpp, SfGroups).  The upper levels
    // of a SMALL factor are a chain of hand-offs that leaves the device idle: several blocks per launch overlap their chains (1M-DOF
    // Poisson: 0.281 -> 0.221 ms per right-hand side, profiles/r06_block_groups.txt).  Large 3D factors gain less (144^3: 3.28 -> 2.97 ms per
    // right-hand side; config 4's 84 GB with its 32-column shard: 398 -> 381 ms) but still gain: no size limit by default; the block
    // buffers never take more than half of the free device memory (solve()).  HIPMF_BLOCK_GROUPS=1..4 overrides.
    block_groups_plan = 8.0 * (double)S.persist_doubles <= block_groups_max_bytes ? SF_GMAX : 1;
    if (given(&Tunables::block_groups_ask)) block_groups_plan = block_groups_ask;
    // (the split dot products of the blocked backward slabs were tuned with ONE block per launch; several groups per launch fill the levels
    //  of few slabs by themselves, and every split costs a scratch round trip: with four groups, fronts from 8 192 rows on instead of 2 048 --
    //  config 4's shard 0.318 -> 0.303 s, 144^3 2.97 -> 2.91, 100^3 0.80 -> 0.78 ms per right-hand side, profiles/r06_block_groups.txt)
    if (!given(&Tunables::split_minlen)) split_minlen = 2048 * block_groups_plan;
    // Wider slabs for the blocked instances (64 rows, 128 forward for long dot products: every slab stages the whole vector block of its
    // front, so wide slabs re-read it less often) lost with one block per launch (round 3: 144^3 4.92 -> 7.06 ms per right-hand side) and
    // win on the LARGE 3D factors once several groups share a launch -- config 4's shard 0.304 -> 0.290 s, 144^3 2.91 -> 2.79 ms per
    // right-hand side -- while the smaller ones lose (100^3 0.788 -> 0.822, the 1M-DOF 2D factor 0.217 -> 0.284): on from a largest front
    // of 16 384 rows (144^3: 20 736, 100^3: 10 000); HIPMF_BLOCKED_SLABS=0 / 1 overrides.  (profiles/r06_block_groups.txt)
    if (!given(&Tunables::blocked_slabs)) blocked_slabs = block_groups_plan > 1 && S.max_front >= 16384;
    auto pl_t = std::chrono::steady_clock::now();
    std::string pl_log;
    auto pl_lap = [&](const char *what) { // (verbose: where the plan + upload time of initialize goes)
        const auto now = std::chrono::steady_clock::now();
        char buf[96];
        snprintf(buf, sizeof buf, " %s %.3f s;", what, std::chrono::duration<double>(now - pl_t).count());
        pl_log += buf;
        pl_t = now;
    };
    // ---- bottom of the tree: one wavefront per subtree of small fronts (kernels_solve_tree.hpp) ----
    // A front is "closed" when it and all its descendants are small fronts and the subtree stays within the caps (fronts, panel
    // bytes, pivots = the part of x the wave keeps in LDS, LDS stack = sum of f over a root-to-leaf path of fronts with children);
    // the wave-subtrees are the maximal closed ones.  Planned here, before the descriptors: the fronts strictly inside a wave-subtree
    // never touch the global solve workspace on that path, which decides the layout of the workspace (below).
    struct WtPlan {
        bool ok_tree = false;
        std::vector<char> ok;
        std::vector<int32_t> cnt, roots;
        std::vector<int64_t> bytes;
    } WP;
    WP.ok_tree = use_tree && S.n >= 4;
    if (WP.ok_tree) {
        bool tree_ok = true;
        std::vector<char> &ok = WP.ok;
        std::vector<int32_t> &cnt = WP.cnt;
        std::vector<int64_t> &bytes = WP.bytes;
        ok.assign((size_t)ns, 0), cnt.assign((size_t)ns, 0), bytes.assign((size_t)ns, 0);
        std::vector<int32_t> dl((size_t)ns, 0), piv((size_t)ns, 0);
        for (int32_t s = 0; s < ns && tree_ok; s++) { // (supernodes are numbered in postorder: children first)
            const int32_t f = S.fsize(s), p = S.npiv(s);
            bool good = f <= SMALL_F && (int64_t)f * p <= WT_NCH * WT_CHUNK && S.nrow(s) <= WT_MI - 16 * WT_NREC;
            int32_t c = 1, d = 0, pv = p;
            int64_t b = (int64_t)f * p * 8;
            for (int32_t q = S.child_ptr[s]; q < S.child_ptr[s + 1]; q++) {
                const int32_t ch = S.child_idx[q];
                if (ch >= s) tree_ok = false;
                else good = good && ok[(size_t)ch], c += cnt[(size_t)ch], b += bytes[(size_t)ch], d = std::max(d, dl[(size_t)ch]), pv += piv[(size_t)ch];
            }
            if (S.child_ptr[s + 1] > S.child_ptr[s]) d += f;
            cnt[(size_t)s] = c, bytes[(size_t)s] = b, dl[(size_t)s] = d, piv[(size_t)s] = pv;
            ok[(size_t)s] = good && c <= wt_max_fronts && b <= (int64_t)wt_max_kb * 1024 && d <= WT_STACK && pv <= WT_X;
        }
        if (tree_ok) {
            for (int32_t s = 0; s < ns; s++)
                if (ok[(size_t)s] && (S.sn_parent[s] < 0 || !ok[(size_t)S.sn_parent[s]])) WP.roots.push_back(s);
            // the longest subtrees first: workgroups start in index order, the short ones fill the tail
            std::stable_sort(WP.roots.begin(), WP.roots.end(), [&](int32_t a, int32_t b) { return bytes[(size_t)a] > bytes[(size_t)b]; });
            // the subtree of root R is the supernode range [R - cnt + 1, R] (postorder numbering)
            for (size_t ri = 0; ri < WP.roots.size() && tree_ok; ri++) {
                const int32_t R = WP.roots[ri], lo = R - cnt[(size_t)R] + 1;
                for (int32_t s = lo; s < R; s++)
                    if (S.sn_parent[s] < lo || S.sn_parent[s] > R) tree_ok = false;
            }
        }
        WP.ok_tree = tree_ok;
    }
    // Layout of a solve workspace (one per right-hand side of a block): the f-vectors of the fronts that talk to other workgroups
    // through it first -- everything but the interiors of the wave-subtrees --, then (tagged hand-offs only) a shadow copy of x, then
    // the interiors' vectors (used by the schedules without wave-subtrees only).  The data-tagged instances of the solve kernels
    // (kernels_solve_fused.hpp, sf_tag_wait) arm the first two parts with ONE memset before a pass pair.
    // Tagged hand-offs need a task list without ASSEMBLE tasks: matrices with fronts of sf_asm_front rows or more (3D: bound by
    // bandwidth, not by the hand-offs) keep the completion counters.
    const bool tag_shape = WP.ok_tree && !WP.roots.empty() && (sf_asm_front <= 0 || S.max_front < sf_asm_front); // (what the tagged hand-offs need; HIPMF_TAG_SOLVE=0 keeps the task shapes)
    const bool tag_plan = use_tag && tag_shape;
    std::vector<char> interior((size_t)ns, 0);
    if (tag_plan)
        for (int32_t R : WP.roots)
            for (int32_t s = R - WP.cnt[(size_t)R] + 1; s < R; s++) interior[(size_t)s] = 1;
    std::vector<int64_t> woff_of((size_t)ns, 0);
    work_doubles = 0;
    // Round 6: [ interiors | roots of the wave-subtrees | the other fronts | xt ].  The interiors (used by the schedules
    // without wave-subtrees: the blocked instances, the fallbacks) come first and the shadow xt LAST, so that the columns of a blocked
    // workspace -- which never use xt -- sit at a stride that leaves it out (work_blk_doubles); the armed part [work_arm0, work_up + n)
    // stays one contiguous range.
    // (the roots: their vectors are written by k_wt_fwd, a launch of its own BEFORE the tagged launches start -- nothing to arm there)
    std::vector<char> is_root((size_t)ns, 0);
    if (tag_plan) {
        for (int32_t s = 0; s < ns; s++)
            if (interior[(size_t)s]) woff_of[(size_t)s] = work_doubles, work_doubles += S.fsize(s);
        for (int32_t R : WP.roots) is_root[(size_t)R] = 1, woff_of[(size_t)R] = work_doubles, work_doubles += S.fsize(R);
    }
    work_arm0 = work_doubles;
    for (int32_t s = 0; s < ns; s++)
        if (!interior[(size_t)s] && !is_root[(size_t)s]) woff_of[(size_t)s] = work_doubles, work_doubles += S.fsize(s);
    work_up = work_doubles;
    work_blk_doubles = work_doubles;
    if (tag_plan) work_doubles += S.n; // xt
    std::vector<FrontDesc> fd((size_t)ns);
    for (int32_t s = 0; s < ns; s++) {
        FrontDesc &d = fd[s];
        d.off = S.front_off[s];
        d.rowptr = S.sn_rowptr[s];
        d.woff = woff_of[(size_t)s];
        d.p = S.npiv(s);
        d.m = S.nrow(s);
        d.first = S.sn_first[s];
        d.child_begin = S.child_ptr[s];
        d.child_end = S.child_ptr[s + 1];
        d.parent = S.sn_parent[s];
        d.ld = S.front_ld[s];
        d.ugroup = update_group(S.fsize(s));
        d.eoff = S.e_off[s], d.epoff = S.ep_off[s];
        d.flags = S.fsize(s) > SMALL_F ? (FD_BIG | (S.sym_mode ? FD_SYM : 0) | (is_mid(s) ? FD_DENSE_TOP : 0)) : 0;
        d.ldp = S.front_ldp[s];
    }
    pool_doubles = S.persist_doubles + S.temp_doubles;

    // The task lists of the solves (wave-subtrees, slabs, blocked instances: a third of the time of this function) depend on the
    // analysis and on `fd` only: they are built and uploaded on a host thread of their own while this one builds the launch plans of
    // the factorisation (no other HIP call runs here until the join).
    // dependency-driven solve: tasks in level order (forward: leaves first; backward: root first); small fronts
    // four to a workgroup (one per wavefront), big fronts one workgroup per slab of 2^kind rows
    int32_t sp_code = SUCCESSFUL_EXIT;
    auto solve_plans = [&]() -> int32_t {
        const bool tracing = given(&Tunables::sf_trace); // (HIPMF_SF_TRACE: the task lists stay on the host for the dump of solve())
        std::vector<SfTask> sf;
        std::vector<int32_t> need((size_t)2 * ns, 1);
        // rows per slab by the length of the dot products (forward: p columns, backward: f columns): long ones get
        // narrow slabs, i.e. more column groups per workgroup and more workgroups per front
        std::vector<char> in_w((size_t)ns, 0); // fronts that belong to a wave-subtree (kernels_solve_tree.hpp)
        bool tree = false;                     // the task list being built is the one above the wave-subtrees
        bool blocked = false;                  // ... the one of the blocked (many-RHS) instances
        bool klist = false;                    // ... the blocked instances' own list (d_sfk)
        int32_t k_fwd_rows = 0;                // klist, per level: log2 of the forward slab rows of the largest fronts (0: sf_big_rows)
        int32_t k_bwd_groups = 0;              // klist, per level: backward slabs of the big fronts of the level
        int32_t top_level = S.nlevels;         // ... its levels >= top_level run in a launch of their own (LDS-staged slabs)
        auto kind_of = [&](int32_t s, bool forward) {
            const int32_t len = forward ? S.npiv(s) : S.fsize(s);
            // Blocked instances (K columns on MFMA tiles): every slab stages the WHOLE vector block of its front (len x K doubles) chunk by
            // chunk, so narrow slabs re-read it as often as there are slabs -- at K = 16 and 16-row slabs as many bytes as the factor
            // itself (config 4 on one GPU: 16 columns cost 1.9x what 8 cost).  64 rows (four 16-output tiles per workgroup, forward 128
            // for the long dot products) read it a quarter / an eighth as often.
            if (blocked) return forward ? (S.fsize(s) >= sf_big_front || len >= 512 ? 7 : 6) : 6;
            if (!forward && S.sym_mode) return 4; // transposed GEMV of the L D L^T fronts: 16 columns of E per workgroup
            // fronts of thousands of rows: every slab workgroup gathers ALL children's update vectors, so 16-row slabs (625 of them
            // for 10 000 rows) re-read them hundreds of times; 64-row slabs still give >= 32 workgroups per front
            // (3D 100^3: pass pair 3.44 -> 3.33 ms, 64 right-hand sides 182 -> 160 ms)
            if (forward && klist && k_fwd_rows > 0 && S.fsize(s) >= sf_big_front) return k_fwd_rows;
            if (forward && sf_big_rows > 0 && S.fsize(s) >= sf_big_front) return sf_big_rows;
            // above the wave-subtrees: a thread's share of its row of E / E' (len / G entries, G = 256 / rows column groups) is parked
            // in LDS / registers BEFORE the wait, so the slabs are cut for <= ~40 entries per thread
            // TOP levels above the wave-subtrees (few, large fronts: a chain of hand-offs): a thread's share of its row of E / E'
            // (len / G entries, G = 256 / rows column groups) is parked in LDS BEFORE the wait, so the slabs are cut for <= 32 entries
            // per thread where 8-row slabs (G = 32) allow it
            if (tree && !slab64 && S.sn_level[s] >= top_level) {
                int32_t G = 2;
                while (G < up_max_groups && len > 32 * G) G *= 2;
                return G == 32 ? 3 : (G == 16 ? 4 : (G == 8 ? 5 : (G == 4 ? 6 : 7)));
            }
            // backward slabs of the factors that qualify for the tagged hand-offs (a level is a hop of poll + dot products + store: shorter dot products per thread
            // are worth the extra tasks): 16 rows from 256 positions on, 32 rows from 64 on (C2: backward 210.6 -> 207.0 us)
            if (tree && tag_shape && !forward && !slab64) return len >= mid_bwd_len4 ? 4 : (len >= mid_bwd_len5 ? 5 : (len > 32 ? 6 : 7));
            return slab64 ? 6 : (len >= 512 ? 4 : (len >= 128 ? 5 : (len > 32 ? 6 : 7)));
        };
        bool skip_leaves = false;              // ... the one of the blocked instances when the leaves have kernels of their own
        auto is_leaf_front = [&](int32_t s) {
            const int64_t p = S.npiv(s), m = S.nrow(s), f = p + m;
            return S.child_ptr[s + 1] == S.child_ptr[s] && f <= SMALL_F && p >= 1 && p <= LEAF_PMAX && m <= LEAF_MMAX && f * p <= LEAF_PANEL;
        };
        auto emit_level = [&](int32_t l, bool forward) {
            std::vector<int32_t> small, wavef;
            if (klist) {
                // Levels of FEW tasks near the root of a large (3D) factor: one workgroup per compute unit streams its slab with ~32 KB in
                // flight and the memory system idles.  Forward: narrower slabs for the largest fronts (their vector block is assembled
                // once: a narrow slab re-reads it from L2, nothing else); backward: the slabs' dot products are split (k_bwd_fused).
                k_fwd_rows = 0, k_bwd_groups = 0;
                if (forward && sf_big_rows > 0 && split_tasks > 0) {
                    for (int32_t rows_log = sf_big_rows; rows_log >= 4; rows_log--) {
                        int64_t cnt = 0;
                        for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++)
                            if (S.fsize(S.level_sn[k]) >= sf_big_front) cnt += (S.fsize(S.level_sn[k]) + (1 << rows_log) - 1) >> rows_log;
                        k_fwd_rows = rows_log;
                        if (cnt == 0 || cnt >= split_tasks) break;
                    }
                    if (k_fwd_rows == sf_big_rows) k_fwd_rows = 0;
                }
                if (!forward)
                    for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
                        const int32_t s = S.level_sn[k];
                        if (S.fsize(s) > SMALL_F && !(skip_leaves && is_leaf_front(s))) k_bwd_groups += (S.npiv(s) + (1 << kind_of(s, false)) - 1) >> kind_of(s, false);
                    }
            }
            for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
                int32_t s = S.level_sn[k];
                if (tree && in_w[(size_t)s]) continue;
                if (skip_leaves && is_leaf_front(s)) {
                    need[(size_t)(forward ? 0 : ns) + s] = 0; // (done by a launch of its own before / after the tasks': nobody counts it)
                    continue;
                }
                if (S.fsize(s) <= SMALL_F) {
                    small.push_back(s);
                    continue;
                }
                // forward pass above the wave-subtrees: big fronts of few rows and pivots are the work of one wavefront each
                // (kind 2, sf_fwd_wave) instead of 256-thread slab tasks
                // (below the top levels only: a top-level front publishes through its replicas, sf_publish_front)
                if (tree && forward && wave_fronts && !slab64 && S.sn_level[s] < top_level && S.fsize(s) <= SF_WF_ROWS && S.npiv(s) <= SF_WF_PIV &&
                    S.child_ptr[s + 1] - S.child_ptr[s] <= 64) {
                    wavef.push_back(s);
                    need[(size_t)s] = 1;
                    wave_front_count++;
                    continue;
                }
                // ... and in the backward pass (LU fronts: x1 = E' [y1; x2], sf_bwd_wave)
                if (tree && !forward && wave_fronts && wave_fronts_bwd && !slab64 && !S.sym_mode && S.sn_level[s] < top_level && S.fsize(s) <= SF_WF_ROWS &&
                    S.npiv(s) <= SF_WF_PIV) {
                    wavef.push_back(s);
                    need[(size_t)ns + s] = 1;
                    continue;
                }
                const int32_t kind = kind_of(s, forward), rows = 1 << kind, ext = forward ? S.fsize(s) : S.npiv(s);
                // forward pass of the largest fronts: the front's vector (right-hand side + children's updates) is assembled ONCE by
                // tasks of their own, 512 rows each (the chunk the blocked instances stage in LDS); the slabs wait for those
                int32_t nasm = 0;
                if (forward && sf_asm_front > 0 && S.fsize(s) >= sf_asm_front && S.child_ptr[s + 1] > S.child_ptr[s] && !(tree && tag_plan)) {
                    for (int32_t q0 = 0; q0 < ext; q0 += SF_ASM_ROWS) sf.push_back({1, s, q0, std::min(ext, q0 + SF_ASM_ROWS), 0, 0}), nasm++;
                }
                need[(size_t)(forward ? 0 : ns) + s] = (ext + rows - 1) / rows + nasm;
                const size_t first_slab = sf.size();
                // (klist, backward, a level of few slabs, long dot products: Q parts per slab -- only the last one to arrive publishes)
                int32_t Q = 1;
                if (klist && !forward && split_tasks > 0 && k_bwd_groups < 8 * split_tasks && S.fsize(s) >= split_minlen && kind >= 4) {
                    // enough parts to fill the device when the level has few slabs; parts of ~2 split_minlen positions when the dot products
                    // are long (a level of 840 slabs of 450 us each runs as one full round of workgroups and one nearly empty one)
                    const int64_t q_cnt = k_bwd_groups < split_tasks ? (3 * (int64_t)split_tasks / 2 + k_bwd_groups - 1) / std::max(1, k_bwd_groups) : 1;
                    const int64_t q_len = S.fsize(s) / (2 * (int64_t)split_minlen);
                    Q = (int32_t)std::min<int64_t>(std::min<int64_t>(8, std::max(q_cnt, q_len)), S.fsize(s) / std::max(1, split_minlen / 4));
                }
                if (Q >= 2) {
                    for (int32_t r0 = 0; r0 < ext; r0 += rows) {
                        for (int32_t q = 0; q < Q; q++) sf.push_back({kind, s, r0, std::min(ext, r0 + rows), (int32_t)split_units, q | (Q << 8)});
                        split_units += (int64_t)Q * (rows / 16);
                        split_slabs++;
                    }
                } else
                    for (int32_t r0 = 0; r0 < ext; r0 += rows) sf.push_back({kind, s, r0, std::min(ext, r0 + rows), nasm, 0});
                // 8-row slabs read 64-byte segments of E / E': two neighbouring slabs share every 128-byte line, and a line is fetched once per
                // XCD that asks for it (tools/microbench/fetch_calib.hip: 64-byte segments move twice their bytes).  Workgroup b runs on XCD
                // b mod 8 (observed, MI355X_MICROARCH.md), so the slabs 2j and 2j + 1 are placed eight tasks apart: the second one finds
                // the line in its XCD's L2.  Speed only: any placement is correct.
                if (kind == 3 && up_pair_xcd) {
                    const size_t cnt = sf.size() - first_slab;
                    std::vector<SfTask> tmp(sf.begin() + (std::ptrdiff_t)first_slab, sf.end());
                    for (size_t g0 = 0; g0 + 16 <= cnt; g0 += 16)
                        for (size_t j = 0; j < 8; j++) sf[first_slab + g0 + j] = tmp[g0 + 2 * j], sf[first_slab + g0 + 8 + j] = tmp[g0 + 2 * j + 1];
                }
            }
            for (size_t k = 0; k < wavef.size(); k += 4) {
                SfTask t = {2, wavef[k], -1, -1, -1, 0};
                if (k + 1 < wavef.size()) t.b = wavef[k + 1];
                if (k + 2 < wavef.size()) t.c = wavef[k + 2];
                if (k + 3 < wavef.size()) t.d = wavef[k + 3];
                sf.push_back(t);
            }
            for (size_t k = 0; k < small.size(); k += 4) {
                SfTask t = {0, small[k], -1, -1, -1, 0};
                if (k + 1 < small.size()) t.b = small[k + 1];
                if (k + 2 < small.size()) t.c = small[k + 2];
                if (k + 3 < small.size()) t.d = small[k + 3];
                sf.push_back(t);
            }
        };
        // the all-small band at the bottom of the tree (levels below the first one with a big front) runs in a lean
        // instance of the kernels (fewer registers, more wavefronts per CU); it holds most of the tasks
        int32_t band = 0;
        while (band < S.nlevels) {
            bool all_small = true;
            for (int32_t k = S.level_ptr[band]; k < S.level_ptr[band + 1] && all_small; k++) all_small = S.fsize(S.level_sn[k]) <= SMALL_F;
            if (!all_small) break;
            band++;
        }
        int32_t fwd_limit = S.nlevels; // profiling knob: run the forward pass up to this level only (the result is then meaningless)
        if (given(&Tunables::sf_fwd_levels)) fwd_limit = std::max(1, std::min(S.nlevels, sf_fwd_levels));
        sf_fwd_launch = 0;
        sf_fwd_band = 0;
        for (int32_t l = 0; l < S.nlevels; l++) {
            emit_level(l, true);
            if (l + 1 == band) sf_fwd_band = (int32_t)sf.size();
            if (l + 1 == fwd_limit) sf_fwd_launch = (int32_t)sf.size();
        }
        sf_fwd_cnt = (int32_t)sf.size();
        sf_bwd_top = 0;
        for (int32_t l = S.nlevels - 1; l >= 0; l--) {
            if (l + 1 == band) sf_bwd_top = (int32_t)sf.size() - sf_fwd_cnt;
            emit_level(l, false);
        }
        if (band == 0) sf_bwd_top = (int32_t)sf.size() - sf_fwd_cnt;
        sf_bwd_cnt = (int32_t)sf.size() - sf_fwd_cnt;
        leaf_cnt = 0;
        if (leaf_kernels && use_fused) {
            std::vector<LeafRec> lf, lb;
            for (int32_t s = 0; s < ns; s++) {
                if (!is_leaf_front(s)) continue;
                LeafRec r;
                memset(&r, 0, sizeof r);
                r.off = fd[(size_t)s].off, r.woff = fd[(size_t)s].woff, r.rowptr = fd[(size_t)s].rowptr;
                r.first = fd[(size_t)s].first, r.p = fd[(size_t)s].p, r.m = fd[(size_t)s].m, r.s = s;
                lf.push_back(r);
                r.off = fd[(size_t)s].epoff >= 0 ? fd[(size_t)s].epoff : fd[(size_t)s].off; // (the rows of U: p x f, stride p; m = 0: the block itself)
                lb.push_back(r);
            }
            leaf_cnt = (int32_t)lf.size();
            if (leaf_cnt > 0) {
                lf.insert(lf.end(), lb.begin(), lb.end());
                HIPC(d_leaf.upload(lf), ERROR_HIP_MALLOC);
            }
        }
        if (blocked_slabs || leaf_cnt > 0) {
            // the same levels once more for the blocked instances: without the leaves (kernels_solve_leaf.hpp) and -- HIPMF_BLOCKED_SLABS=1 --
            // with wider slabs (the other small fronts' tasks are the same)
            std::vector<SfTask> keep;
            keep.swap(sf);
            std::vector<int32_t> need_keep = need;
            std::fill(need.begin(), need.end(), 1);
            blocked = blocked_slabs;
            skip_leaves = leaf_cnt > 0;
            klist = true;
            split_units = 0, split_slabs = 0;
            sfk_fwd_band = 0;
            sfk_band_f.assign(1, 0), sfk_band_b.clear();
            for (int32_t l = 0; l < S.nlevels; l++) {
                emit_level(l, true);
                if (l < band) sfk_band_f.push_back((int32_t)sf.size()); // (round 6: the all-small band runs one PLAIN launch per level)
                if (l + 1 == band) sfk_fwd_band = (int32_t)sf.size();
            }
            sfk_fwd_cnt = (int32_t)sf.size();
            sfk_bwd_top = 0;
            for (int32_t l = S.nlevels - 1; l >= 0; l--) {
                if (l + 1 == band) sfk_bwd_top = (int32_t)sf.size() - sfk_fwd_cnt;
                if (l < band) sfk_band_b.push_back((int32_t)sf.size() - sfk_fwd_cnt);
                emit_level(l, false);
            }
            if (band == 0) sfk_bwd_top = (int32_t)sf.size() - sfk_fwd_cnt;
            sfk_bwd_cnt = (int32_t)sf.size() - sfk_fwd_cnt;
            sfk_band_b.push_back(sfk_bwd_cnt);
            if (plain_band)
                // the fronts of the band complete in launches of their own before (forward) / after (backward) the dependency-driven
                // launch of the levels above: nobody counts them, like the leaves
                for (int32_t l = 0; l < band; l++)
                    for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) need[(size_t)S.level_sn[k]] = 0, need[(size_t)ns + S.level_sn[k]] = 0;
            blocked = false;
            skip_leaves = false;
            klist = false;
            if (split_units > 0) {
                if (split_units >= (int64_t)0x7fffffff) return ERROR_HIPMF_SYMBOLIC;
                // (one set per group of a blocked launch)
                HIPC(d_split_scr.alloc(256 * (size_t)split_units * (size_t)block_groups_plan), ERROR_HIP_MALLOC);
                HIPC(d_split_cnt.alloc((size_t)split_units * (size_t)block_groups_plan), ERROR_HIP_MALLOC);
                HIPC(hipMemset(d_split_cnt, 0, sizeof(int32_t) * (size_t)split_units * (size_t)block_groups_plan), ERROR_HIP_MALLOC);
            }
            sfk_host.clear();
            if (tracing)
                for (const SfTask &t : sf) sfk_host.push_back(t.kind), sfk_host.push_back(t.a);
            HIPC(d_sfk.upload(sf), ERROR_HIP_MALLOC);
            HIPC(d_needk.upload(need), ERROR_HIP_MALLOC);
            sf.swap(keep);
            need.swap(need_keep);
        }
        if (tracing) { // profiling aid: four device-clock stamps per task of the upper (mixed) launches
            const size_t ntr = (size_t)(sf_fwd_cnt - sf_fwd_band) + (size_t)sf_bwd_top;
            HIPC(d_trace.alloc(8 * std::max<size_t>(ntr, 1)), ERROR_HIP_MALLOC);
            HIPC(hipMemset(d_trace, 0, sizeof(unsigned long long) * 8 * std::max<size_t>(ntr, 1)), ERROR_HIP_MALLOC);
            sf_host.clear();
            for (const SfTask &t : sf) sf_host.push_back(t.kind), sf_host.push_back(t.a);
        }
        HIPC(d_sf.upload(sf), ERROR_HIP_MALLOC);
        // ---- bottom of the tree: one wavefront per subtree of small fronts (kernels_solve_tree.hpp) ----
        // A front is "closed" when it and all its descendants are small fronts and the subtree stays within the caps (fronts, panel
        // bytes, pivots = the part of x the wave keeps in LDS, LDS stack = sum of f over a root-to-leaf path of fronts with children);
        // the wave-subtrees are the maximal closed ones.
        wt_waves = wt_recs = 0;
        sf2_fwd_cnt = sf2_bwd_cnt = 0;
        wave_front_count = 0;
        bool tree_ok = WP.ok_tree; // (the wave-subtrees were planned before the descriptors: WtPlan above)
        if (tree_ok) {
            const std::vector<int32_t> &cnt = WP.cnt, &roots = WP.roots;
            {
                std::vector<WtHdr> hdr_f, hdr_b;
                std::vector<int32_t> meta_f, meta_b;
                std::vector<WtWave> wav_f, wav_b;
                std::vector<int32_t> off((size_t)ns, 0);
                for (size_t ri = 0; ri < roots.size() && tree_ok; ri++) {
                    const int32_t R = roots[ri], lo = R - cnt[(size_t)R] + 1;
                    // the subtree is the supernode range [lo, R] (postorder numbering); its pivot columns are one contiguous range
                    for (int32_t s = R; s >= lo; s--) {
                        if (s != R && (S.sn_parent[s] < lo || S.sn_parent[s] > R)) tree_ok = false;
                        if (s == R) off[(size_t)s] = 0;
                        for (int32_t q = S.child_ptr[s]; q < S.child_ptr[s + 1]; q++) off[(size_t)S.child_idx[q]] = off[(size_t)s] + S.fsize(s);
                    }
                    if (!tree_ok) break;
                    const int32_t xfirst = S.sn_first[lo];
                    for (int dir = 0; dir < 2; dir++) { // 0: forward (postorder = ascending), 1: backward (descending)
                        std::vector<WtHdr> &hdr = dir == 0 ? hdr_f : hdr_b;
                        std::vector<int32_t> &meta = dir == 0 ? meta_f : meta_b;
                        std::vector<WtWave> &wav = dir == 0 ? wav_f : wav_b;
                        WtWave w;
                        memset(&w, 0, sizeof w);
                        w.b0 = (int32_t)hdr.size(), w.xfirst = xfirst, w.npiv = S.sn_first[R + 1] - xfirst;
                        int32_t s = dir == 0 ? lo : R;
                        const int32_t send = dir == 0 ? R + 1 : lo - 1, step = dir == 0 ? 1 : -1;
                        while (s != send) {
                            // one batch: as many consecutive fronts as fit (records, 1 KB pieces, words of the meta block)
                            int32_t nrec = 0, nch = 0, words = 0, e = s;
                            while (e != send && nrec < WT_NREC) {
                                const int32_t ck = (int32_t)(((int64_t)S.fsize(e) * S.npiv(e) + WT_CHUNK - 1) / WT_CHUNK);
                                const bool lists = dir == 0 ? e != R : true; // (the forward root has no use for its relative indices)
                                const int32_t wk = lists ? S.nrow(e) : 0;
                                if (nrec > 0 && (nch + ck > WT_NCH || 16 * (nrec + 1) + words + wk > WT_MI)) break;
                                nrec++, nch += ck, words += wk, e += step;
                            }
                            WtHdr h;
                            memset(&h, 0, sizeof h);
                            h.nrec = nrec;
                            h.meta = (int64_t)meta.size();
                            const size_t m0 = meta.size();
                            meta.resize(m0 + (size_t)16 * nrec);
                            int32_t ci = 0, lst = 16 * nrec;
                            for (int32_t k = 0, t = s; k < nrec; k++, t += step) {
                                WtRec r;
                                memset(&r, 0, sizeof r);
                                const int32_t par = S.sn_parent[t], pp = S.npiv(t), mm = S.nrow(t), ff = pp + mm;
                                const bool has_children = S.child_ptr[t + 1] > S.child_ptr[t];
                                const bool packed = dir == 1 && fd[(size_t)t].epoff >= 0;
                                const int64_t src = dir == 0 ? fd[(size_t)t].off : (packed ? fd[(size_t)t].epoff : fd[(size_t)t].off);
                                const int32_t ck = (int32_t)(((int64_t)ff * pp + WT_CHUNK - 1) / WT_CHUNK);
                                r.pslot = WT_CHUNK * ci;
                                for (int32_t c = 0; c < ck; c++) h.src[ci++] = src + (int64_t)WT_CHUNK * c;
                                r.pm = pp | (mm << 16);
                                r.xoff = S.sn_first[t] - xfirst;
                                int32_t lds_self = has_children ? off[(size_t)t] + 1 : 0, lds_par = 0;
                                if (t != R) {
                                    lds_par = off[(size_t)par] + 1;
                                    r.pxoff = S.sn_first[par] - xfirst, r.ppf = S.npiv(par) | (S.fsize(par) << 16);
                                    if (S.child_idx[S.child_ptr[par]] == t) r.flags |= 1;
                                }
                                if (packed) r.flags |= 2;
                                if (fd[(size_t)t].epoff >= 0) r.flags |= 4;
                                r.lds = lds_self | (lds_par << 16);
                                r.first = S.sn_first[t], r.s = t, r.woff = fd[(size_t)t].woff;
                                const bool lists = dir == 0 ? t != R : true;
                                r.relo = lst;
                                if (lists && mm > 0) {
                                    const int32_t *src_idx = (t != R ? S.rel.data() : S.sn_rows.data()) + S.sn_rowptr[t];
                                    meta.insert(meta.end(), src_idx, src_idx + mm);
                                    lst += mm;
                                }
                                memcpy(meta.data() + m0 + (size_t)16 * k, &r, sizeof r);
                            }
                            for (int32_t c = ci; c < WT_NCH; c++) h.src[c] = h.src[0];
                            h.words = lst;
                            hdr.push_back(h);
                            s = e;
                        }
                        w.b1 = (int32_t)hdr.size();
                        if (w.b1 > w.b0) w.h0 = hdr[(size_t)w.b0]; // (the first batch's header rides in the wave's record)
                        wav.push_back(w);
                    }
                }
                if (tree_ok) {
                    for (size_t ri = 0; ri < roots.size(); ri++)
                        for (int32_t s = roots[ri] - cnt[(size_t)roots[ri]] + 1; s <= roots[ri]; s++) in_w[(size_t)s] = 1, wt_recs++;
                    wt_waves = (int32_t)roots.size();
                    {
                        WtWave none;
                        memset(&none, 0, sizeof none);
                        while (wav_f.size() % WT_WAVES != 0) wav_f.push_back(none), wav_b.push_back(none);
                    }
                    // one array each: forward part, then backward part (the backward headers / waves index their own parts)
                    wt_hdr_fwd = (int32_t)hdr_f.size(), wt_hdr_bwd = (int32_t)hdr_b.size(), wt_meta_fwd = (int64_t)meta_f.size();
                    hdr_f.insert(hdr_f.end(), hdr_b.begin(), hdr_b.end());
                    meta_f.insert(meta_f.end(), meta_b.begin(), meta_b.end());
                    meta_f.resize(meta_f.size() + WT_MI, 0); // (a batch's meta block is fetched as WT_MI words whatever it holds)
                    wav_f.insert(wav_f.end(), wav_b.begin(), wav_b.end());
                    HIPC(d_wt_hdr.upload(hdr_f), ERROR_HIP_MALLOC);
                    HIPC(d_wt_meta.upload(meta_f), ERROR_HIP_MALLOC);
                    HIPC(d_wt_wave.upload(wav_f), ERROR_HIP_MALLOC);
                }
            }
            if (tree_ok) {
                // the fronts above: the same task kinds as before, slabs cut for the LDS-staged instances
                std::vector<SfTask> keep;
                keep.swap(sf);
                std::vector<int32_t> need_keep = need;
                std::fill(need.begin(), need.end(), 1);
                tree = true;
                // the TOP levels: from the first level on above which no level has more than up_top_fronts tiled fronts
                top_level = S.nlevels;
                if (up_stage > 0) {
                    while (top_level > 0) {
                        int32_t nb = 0;
                        for (int32_t k = S.level_ptr[top_level - 1]; k < S.level_ptr[top_level]; k++) nb += S.fsize(S.level_sn[k]) > SMALL_F;
                        if (nb > up_top_fronts || nb == 0) break;
                        top_level--;
                    }
                }
                sf2_fwd_mid = 0;
                for (int32_t l = 0; l < S.nlevels; l++) {
                    if (l == top_level) sf2_fwd_mid = (int32_t)sf.size();
                    emit_level(l, true);
                }
                sf2_fwd_cnt = (int32_t)sf.size();
                if (top_level >= S.nlevels) sf2_fwd_mid = sf2_fwd_cnt;
                sf2_bwd_top = 0;
                for (int32_t l = S.nlevels - 1; l >= 0; l--) {
                    emit_level(l, false);
                    if (l == top_level) sf2_bwd_top = (int32_t)sf.size() - sf2_fwd_cnt;
                }
                sf2_bwd_cnt = (int32_t)sf.size() - sf2_fwd_cnt;
                tree = false;
                {
                    // "complete" replicas of the tiled fronts of the top levels (kernels_solve_fused.hpp, sf_wait_front)
                    std::vector<int32_t> ridx((size_t)ns, -1);
                    int32_t ntop = 0;
                    if (use_rep)
                        for (int32_t l = top_level; l < S.nlevels; l++)
                            for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++)
                                if (S.fsize(S.level_sn[k]) > SMALL_F) ridx[(size_t)S.level_sn[k]] = ntop++;
                    rep_words = (int64_t)ntop * SF_REP * 16;
                    if (ntop > 0) {
                        HIPC(d_rep_idx.upload(ridx), ERROR_HIP_MALLOC);
                        // (one set per solve lane: a lane clears and uses its own words whatever the other lanes are doing)
                        HIPC(d_rep.alloc(2 * (size_t)rep_words * MAX_SOLVE_LANES), ERROR_HIP_MALLOC);
                        HIPC(hipMemset(d_rep, 0, sizeof(int32_t) * 2 * (size_t)rep_words * MAX_SOLVE_LANES), ERROR_HIP_MALLOC);
                    }
                }
                HIPC(d_sf2.upload(sf), ERROR_HIP_MALLOC);
                HIPC(d_need2.upload(need), ERROR_HIP_MALLOC);
                if (d_trace) { // (profiling aid: the stamps of THIS list's tasks)
                    // (room for the stamps of the blocked instances' upper launches too: a blocked solve writes into the same buffer)
                    const size_t ntr2 = std::max<size_t>(std::max<size_t>(sf.size(), (size_t)(sfk_fwd_cnt - sfk_fwd_band) + (size_t)sfk_bwd_top), 1);
                    HIPC(d_trace.alloc(8 * ntr2), ERROR_HIP_MALLOC);
                    HIPC(hipMemset(d_trace, 0, sizeof(unsigned long long) * 8 * ntr2), ERROR_HIP_MALLOC);
                    sf_host.clear();
                    for (const SfTask &t : sf) sf_host.push_back(t.kind), sf_host.push_back(t.a);
                }
                sf.swap(keep);
                need.swap(need_keep);
                if (opt.verbose)
                    fprintf(stderr,
                            "hipmf: initialize: %d wave-subtrees hold %d of %d fronts in %d + %d batches; %d + %d tasks above them, of which %d + %d "
                            "on the top levels (%d..%d)\n",
                            wt_waves, wt_recs, ns, wt_hdr_fwd, wt_hdr_bwd, sf2_fwd_cnt, sf2_bwd_cnt, sf2_fwd_cnt - sf2_fwd_mid, sf2_bwd_top, top_level,
                            S.nlevels - 1);
            }
        }
        tree_active = tree_ok && (wt_waves > 0 || sf2_fwd_cnt > 0);
        tag_active = tree_active && tag_plan;
        // (the backward slabs below the top levels: with the tagged hand-offs the small parked share of E' no longer pays -- 217 against
        //  221 us per backward pass at 1000 x 1000, profiles/r05_solve_variants_c2.txt; an explicit HIPMF_UP_STAGE_MID is kept)
        if (tag_active && !given(&Tunables::up_stage_mid)) up_stage_mid = 0;
        if (tree_active && up_stage > 0) {
            HIPMF_ALLOW_LDS((k_fwd_fused<false, 1, true>), sizeof(double) * 256 * (size_t)up_stage);
            HIPMF_ALLOW_LDS((k_bwd_fused<false, 1, false, true>), sizeof(double) * 256 * (size_t)up_stage_bwd);
            HIPMF_ALLOW_LDS((k_fwd_fused<false, 1, true, true>), sizeof(double) * 256 * (size_t)up_stage);
            HIPMF_ALLOW_LDS((k_bwd_fused<false, 1, false, true, true>), sizeof(double) * 256 * (size_t)up_stage_bwd);
        }
        HIPC(d_need.upload(need), ERROR_HIP_MALLOC);
        // (per group of a blocked launch: forward counters | backward counters | one word -- group 0's is the sticky error word)
        HIPC(d_sync.alloc(SF_GMAX * (2 * (size_t)(SF_SYNC_HEADER + ns) + 1)), ERROR_HIP_MALLOC);
        HIPC(hipMemset(d_sync, 0, sizeof(int32_t) * SF_GMAX * (2 * (size_t)(SF_SYNC_HEADER + ns) + 1)), ERROR_HIP_MALLOC);
        return SUCCESSFUL_EXIT;
    };
    const bool sp_async = plan_thread; // (HIPMF_PLAN_THREAD=0: in line, for timing comparisons)
    if (!sp_async) sp_code = solve_plans();
    std::thread sp_thread([&]() {
        if (!sp_async) return;
        (void)hipSetDevice(device);
        try {
            sp_code = solve_plans();
        } catch (const std::bad_alloc &) { // (an exception must not leave the thread)
            std::lock_guard<std::mutex> lock(err_mutex);
            last_error = "Not enough memory: a host allocation failed";
            sp_code = ERROR_MALLOC;
        }
    });
    struct SpJoiner { // (every early return below waits for the thread)
        std::thread &t;
        ~SpJoiner() {
            if (t.joinable()) t.join();
        }
    } sp_joiner{sp_thread};

    std::vector<int32_t> lists, tasks, allbig;
    std::vector<ChainTask> chain;
    chain_words = 0;
    std::vector<FrontDesc> bigfd;
    std::vector<EaTask, NoInitAlloc<EaTask>> ea;
    std::vector<EaRange, NoInitAlloc<EaRange>> ear;
    std::vector<int32_t> tiled_slot((size_t)S.nsuper, -1); // s -> slot among the tiled fronts of its level
    int32_t max_big = 0;
    std::vector<SolveTask> stasks;
    levels.assign((size_t)S.nlevels, LevelPlan());
    mid_front_count = 0;
    for (int32_t l = 0; l < S.nlevels; l++) {
        LevelPlan &L = levels[l];
        std::vector<int32_t> small, big;
        int32_t fmax_small = 1;
        for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
            int32_t s = S.level_sn[k];
            if (S.fsize(s) <= SMALL_F) {
                small.push_back(s);
                fmax_small = std::max(fmax_small, S.fsize(s));
                L.small_pmax = std::max(L.small_pmax, S.npiv(s));
            } else {
                big.push_back(s);
            }
        }
        // the fronts one workgroup factorises in one launch (k_front) leave the tiled list; by size class, then by pivots
        std::vector<int32_t> mid;
        {
            std::vector<int32_t> tiled;
            for (int32_t a : big) (is_mid(a) ? mid : tiled).push_back(a);
            big.swap(tiled);
            // class 3: k_front_lu (at most 32 pivots); 0 .. 2: k_front by the columns of F12 per wavefront (10 / 16 / 24)
            // (k_front_lu: a launch reserves the LDS of its largest front for every workgroup -- one front of 32 x 192 (117 KB) in the launch and
            //  every front has a CU to itself; by LDS class the many smaller ones run two or four to a CU)
            auto cls = [&](int32_t a) {
                const int32_t m = S.nrow(a);
                if (!is_mid_lu(a)) return m <= 80 ? 0 : (m <= 128 ? 1 : 2);
                const int32_t w = midl_lds_doubles(S.npiv(a), m);
                return (mid_lu_split && w <= 5000) ? 3 : ((mid_lu_split && w <= 10000) ? 4 : 5);
            };
            // (within a class: by the work of the front, largest first -- the workgroups that run longest start first)
            std::stable_sort(mid.begin(), mid.end(), [&](int32_t a, int32_t b) {
                return cls(a) != cls(b) ? cls(a) < cls(b) : (int64_t)S.npiv(a) * S.fsize(a) * S.fsize(a) > (int64_t)S.npiv(b) * S.fsize(b) * S.fsize(b);
            });
            mid_front_count += (int64_t)mid.size();
            for (int32_t a : mid) {
                const int c = cls(a);
                L.mid_cnt[c]++;
                L.mid_lds[c] = std::max(L.mid_lds[c], c >= 3 ? midl_lds_doubles(S.npiv(a), S.nrow(a)) : mid_lds_doubles(S.npiv(a), S.nrow(a)));
            }
        }
        std::stable_sort(big.begin(), big.end(), [&](int32_t a, int32_t b) { return S.npiv(a) > S.npiv(b); });
        // symmetric mode: the tiled fronts of this level whose parent is a small front (it pulls a FULL contribution block)
        std::vector<int32_t> mirror;
        if (S.sym_mode)
            for (int32_t a : big)
                if (S.sn_parent[a] >= 0 && S.nrow(a) > 0 && S.fsize(S.sn_parent[a]) <= SMALL_F) mirror.push_back(a);
        // the small fronts of a level go in two launches by size: the LDS a workgroup reserves is that of the largest front of
        // its launch, and the assembly phases of k_small_factor are latency-bound, i.e. they live on the number of resident waves
        std::stable_partition(small.begin(), small.end(), [&](int32_t a) { return S.fsize(a) <= small_split; });
        L.small_cnt_a = 0;
        int32_t fmax_a = 1;
        for (int32_t a : small)
            if (S.fsize(a) <= small_split) L.small_cnt_a++, fmax_a = std::max(fmax_a, S.fsize(a));
        if (L.small_cnt_a < 2048 || (int32_t)small.size() - L.small_cnt_a < 2048) L.small_cnt_a = 0; // not worth a second launch
        L.small_ld_a = fmax_a | 1;
        L.small_off = (int32_t)lists.size();
        L.small_cnt = (int32_t)small.size();
        L.small_ld = fmax_small | 1;
        lists.insert(lists.end(), small.begin(), small.end());
        L.big_off = (int32_t)lists.size();
        L.big_cnt = (int32_t)big.size();
        lists.insert(lists.end(), big.begin(), big.end());
        L.mirror_off = (int32_t)lists.size();
        L.mirror_cnt = (int32_t)mirror.size();
        lists.insert(lists.end(), mirror.begin(), mirror.end());
        L.bigfd_off = (int32_t)bigfd.size();
        for (int32_t a : big) bigfd.push_back(fd[(size_t)a]);
        L.mid_off = (int32_t)bigfd.size();
        for (int32_t a : mid) bigfd.push_back(fd[(size_t)a]);
        allbig.insert(allbig.end(), big.begin(), big.end()); // (k_set_identity: the tiled fronts only)
        max_big = std::max(max_big, L.big_cnt);
        // tiled steps over the augmented fronts: the active range of step k0 has f indices per dimension
        int32_t pmax = big.empty() ? 0 : S.npiv(big[0]);
        {
            int32_t fmax_big = 0;
            for (int32_t a : big) fmax_big = std::max(fmax_big, S.fsize(a));
            const bool forced = given(&Tunables::upd32_max_front); // (an explicit setting also applies to the symmetric fronts)
            L.upd_ts = (!big.empty() && fmax_big <= upd32_max_front && (!S.sym_mode || forced)) ? UPD_T_SMALL : UPD_T;
        }
        const int64_t UT = L.upd_ts;
        for (int32_t k0 = 0; k0 < pmax; k0 += NB) {
            StepPlan st;
            while (st.nactive < L.big_cnt && S.npiv(big[st.nactive]) > k0) st.nactive++;
            st.pfx_panel = (int64_t)tasks.size();
            int64_t acc = 0;
            for (int32_t a = 0; a < st.nactive; a++) {
                tasks.push_back((int32_t)acc);
                if (a >= 1 && a <= 3) st.ppfx[a - 1] = (int32_t)acc;
                acc += 2 * ((S.fsize(big[a]) + PANEL_T - 1) / PANEL_T);
            }
            tasks.push_back((int32_t)acc);
            st.n_panel = (int32_t)acc;
            st.pfx_update = (int64_t)tasks.size();
            acc = 0;
            // The look-ahead pieces lead the launch (update_task, kernels_factor.hpp): the prefix then counts tiles only.  The fronts are
            // sorted by pivots, so the ones another step follows are a prefix of the slots.  (k_bstep / k_bstep32 of the opt-in
            // block-inverse step read the same prefix and carry a look-ahead piece of the same kind: they keep the old order -- measured
            // slower than the two-launch step and off by default, a reorder would want a measurement of its own.)
            const bool la_first = upd_la_first && (S.sym_mode || !use_binv);
            int32_t nfollow_all = 0;
            while (nfollow_all < st.nactive && S.npiv(big[nfollow_all]) > k0 + NB) nfollow_all++;
            for (int32_t a = nfollow_all; a < st.nactive; a++)
                if (S.npiv(big[a]) > k0 + NB) return ERROR_HIPMF_SYMBOLIC; // (not a prefix: the level's fronts are not sorted)
            st.nfollow = la_first ? nfollow_all : 0;
            const int64_t la_own = la_first ? 0 : 1; // the look-ahead piece as the last task of its front's range
            for (int32_t a = 0; a < st.nactive; a++) {
                tasks.push_back((int32_t)acc);
                if (a >= 1 && a <= 3) st.upfx[a - 1] = (int32_t)acc;
                // tiles per dimension of k_update at this step: [base, f) and [f, f + base) are tiled separately (base = k0 + nb)
                const int64_t fa = S.fsize(big[a]), nba = std::min<int64_t>(NB, S.npiv(big[a]) - k0), basea = k0 + nba;
                const int64_t ntF = (fa - basea + UT - 1) / UT, ntE = (basea + UT - 1) / UT;
                int64_t nt = ntF + ntE;
                const bool follow = S.npiv(big[a]) > k0 + NB;  // another step follows: look-ahead workgroup
                const int32_t G = update_group(S.fsize(big[a]));
                const bool narrow = follow && ((k0 / NB) % G) != G - 1; // not the last step of a group: block column + block row only
                // (symmetric fronts enumerate only the tiles with live entries: lower triangle of F, rows of F x columns of E)
                if (S.sym_mode) acc += (narrow ? nt : ntF * (ntF + 1) / 2 + ntF * ntE) + (follow ? la_own : 0);
                else acc += (narrow ? 2 * nt : nt * nt) + (follow ? la_own : 0);
            }
            tasks.push_back((int32_t)acc);
            if (acc + st.nfollow > 0x7fffffffLL) return ERROR_HIPMF_SYMBOLIC;
            st.n_update = (int32_t)acc + st.nfollow;
            // Split this step's update?  LU, 64 x 64 tiles, no active front in a narrow step (the group's last step: every front applies the
            // whole rank-64 update), some front goes on afterwards (there is a panel chain to run beside the bulk), enough workgroups
            // for the bulk to be worth a stream of its own.
            bool any_narrow = false, any_follow = false, any_full = false;
            for (int32_t a = 0; a < st.nactive; a++) {
                const bool follow = S.npiv(big[a]) > k0 + NB;
                const int32_t G = update_group(S.fsize(big[a]));
                const bool nar = follow && ((k0 / NB) % G) != G - 1;
                any_narrow |= nar, any_follow |= follow, any_full |= !nar;
            }
            st.all_narrow = !any_full;
            if (!S.sym_mode && UT == UPD_T && upd_split_min > 0 && st.n_update >= upd_split_min && !use_chain) {
                if (!any_narrow && any_follow) {
                    st.split = true;
                    for (int part = 1; part <= 2; part++) {
                        (part == 1 ? st.pfx_crit : st.pfx_rest) = (int64_t)tasks.size();
                        int64_t acc2 = 0;
                        for (int32_t a = 0; a < st.nactive; a++) {
                            tasks.push_back((int32_t)acc2);
                            const int64_t fa = S.fsize(big[a]), nba = std::min<int64_t>(NB, S.npiv(big[a]) - k0), basea = k0 + nba;
                            const int64_t nt = (fa - basea + UT - 1) / UT + (basea + UT - 1) / UT;
                            const bool follow = S.npiv(big[a]) > k0 + NB;
                            acc2 += part == 1 ? (2 * nt - 1) + (follow ? la_own : 0) : (nt - 1) * (nt - 1);
                        }
                        tasks.push_back((int32_t)acc2);
                        (part == 1 ? st.n_crit : st.n_rest) = (int32_t)acc2 + (part == 1 ? st.nfollow : 0);
                    }
                }
            }
            L.steps.push_back(st);
        }
        // k_eflush (one-launch steps, LU): per tiled front (block columns) x (tiles of 64 rows of its p rows of E')
        L.pfx_flush = (int64_t)tasks.size();
        {
            int64_t accf = 0;
            for (int32_t a : big) {
                tasks.push_back((int32_t)accf);
                const int64_t pa = S.npiv(a);
                if (pa > NB) accf += ((pa + NB - 1) / NB) * ((pa + 63) / 64);
            }
            tasks.push_back((int32_t)accf);
            L.n_flush = S.sym_mode ? 0 : (int32_t)accf;
        }
        // the same steps as tasks of ONE launch (k_chain) for the levels near the root: panel tiles and update pieces in the order of the
        // launches, each with the counters it waits for and the ones it bumps (kernels_factor_chain.hpp)
        {
            int64_t maxu = 0;
            for (const StepPlan &st : L.steps) maxu = std::max<int64_t>(maxu, st.n_update);
            if (use_chain && L.upd_ts == UPD_T && !L.steps.empty() && maxu <= chain_max_update && maxu >= chain_min_update && (int32_t)L.steps.size() <= chain_max_steps) {
                const int32_t nsteps = (int32_t)L.steps.size();
                const int64_t cbase = chain_words;
                auto cidx = [&](int32_t a, int32_t si, int32_t j) { return (int32_t)(cbase + ((int64_t)a * nsteps + si) * 3 + j); };
                chain_words += (int64_t)L.big_cnt * nsteps * 3;
                std::vector<int32_t> prevC((size_t)L.big_cnt, 0), prevU((size_t)L.big_cnt, 0);
                L.chain_off = (int64_t)chain.size();
                for (int32_t si = 0; si < nsteps; si++) {
                    const StepPlan &st = L.steps[(size_t)si];
                    const int32_t k0 = si * NB;
                    for (int32_t a = 0; a < st.nactive; a++) {
                        const int32_t npan = 2 * ((S.fsize(big[a]) + PANEL_T - 1) / PANEL_T);
                        for (int32_t t = 0; t < npan; t++) {
                            ChainTask c{};
                            c.slot = a, c.k0 = k0, c.t = t, c.kind = 0;
                            c.w0 = si > 0 ? cidx(a, si - 1, chain_fine ? 1 : 2) : -1, c.n0 = si > 0 ? (chain_fine ? prevC[a] : prevU[a]) : 0;
                            c.w1 = -1, c.n1 = 0, c.pub0 = cidx(a, si, 0), c.pub1 = -1;
                            chain.push_back(c);
                        }
                    }
                    for (int32_t a = 0; a < st.nactive; a++) {
                        const int32_t npan = 2 * ((S.fsize(big[a]) + PANEL_T - 1) / PANEL_T);
                        const int64_t fa = S.fsize(big[a]), nba = std::min<int64_t>(NB, S.npiv(big[a]) - k0), basea = k0 + nba;
                        const int32_t ntF = (int32_t)((fa - basea + UPD_T - 1) / UPD_T), ntE = (int32_t)((basea + UPD_T - 1) / UPD_T), nt = ntF + ntE;
                        const bool follow = S.npiv(big[a]) > k0 + NB;
                        const int32_t G = update_group(S.fsize(big[a]));
                        const bool narrow = follow && ((k0 / NB) % G) != G - 1;
                        const int32_t ntri = ntF * (ntF + 1) / 2;
                        const int32_t ntiles = S.sym_mode ? (narrow ? nt : ntri + ntF * ntE) : (narrow ? 2 * nt : nt * nt);
                        // critical pieces: the look-ahead piece and the tiles that hold the next panel's block column (first tile column)
                        // or block row (first tile row); a narrow step consists of them
                        auto critical = [&](int32_t t) {
                            if (t == ntiles || narrow) return true;
                            if (!S.sym_mode) return t % nt == 0 || t / nt == 0;
                            return t < ntF || (t >= ntri && (t - ntri) % ntF == 0);
                        };
                        int32_t nC = 0;
                        auto emit = [&](int32_t t) {
                            ChainTask c{};
                            c.slot = a, c.k0 = k0, c.t = t, c.kind = 1;
                            c.w0 = cidx(a, si, 0), c.n0 = npan;
                            c.w1 = si > 0 ? cidx(a, si - 1, 2) : -1, c.n1 = si > 0 ? prevU[a] : 0;
                            c.pub0 = cidx(a, si, 2), c.pub1 = critical(t) ? cidx(a, si, 1) : -1;
                            if (c.pub1 >= 0) nC++;
                            chain.push_back(c);
                        };
                        if (follow) emit(ntiles); // the look-ahead piece first: the longest serial piece of the step
                        for (int32_t t = 0; t < ntiles; t++)
                            if (critical(t)) emit(t);
                        for (int32_t t = 0; t < ntiles; t++)
                            if (!critical(t)) emit(t);
                        prevC[a] = nC, prevU[a] = ntiles + (follow ? 1 : 0);
                    }
                }
                L.chain_cnt = (int32_t)((int64_t)chain.size() - L.chain_off);
            }
        }
        for (size_t q = 0; q < big.size(); q++) tiled_slot[(size_t)big[q]] = (int32_t)q;
        // solve tasks of the big fronts: 64-row slabs of the f rows (forward) / of the p pivot rows (backward)
        L.fwd_off = (int32_t)stasks.size();
        int64_t nslab = 0;
        big.insert(big.end(), mid.begin(), mid.end()); // (the solves treat every front with f > 64 alike)
        for (int32_t s : big) {
            L.big_pmax = std::max(L.big_pmax, S.npiv(s));
            L.big_fmax = std::max(L.big_fmax, S.fsize(s));
            nslab += (S.fsize(s) + SOLVE_SLAB - 1) / SOLVE_SLAB;
        }
        // few, large fronts (the levels near the root): narrow slabs and 32 column groups per workgroup
        L.wide = !slab64 && nslab < 256 && L.big_pmax >= 128;
        const int32_t slab = L.wide ? SOLVE_SLAB_WIDE : SOLVE_SLAB;
        for (int32_t s : big) {
            int32_t f = S.fsize(s);
            for (int32_t r0 = 0; r0 < f; r0 += slab) stasks.push_back({s, r0, std::min(f, r0 + slab)});
        }
        L.fwd_cnt = (int32_t)stasks.size() - L.fwd_off;
        L.bwd_off = (int32_t)stasks.size();
        for (int32_t s : big) {
            int32_t p = S.npiv(s);
            for (int32_t r0 = 0; r0 < p; r0 += slab) stasks.push_back({s, r0, std::min(p, r0 + slab)});
        }
        L.bwd_cnt = (int32_t)stasks.size() - L.bwd_off;
        if (L.big_pmax > MAX_LDS_DOUBLES || L.big_fmax > MAX_LDS_DOUBLES) {
            // the level-set solve kernels stage a whole p- / f-vector in LDS; the dependency-driven ones work in chunks
            // (without in-launch hand-offs such a factor is solved by the same kernels launched level by level: run_triangular)
            level_path_ok = false;
        }
    }
    if (S.sym_mode && !allbig.empty()) level_path_ok = false; // the level-set solve kernels have no L D L^T instance: same remedy
    // ---- extend-add tasks of every level ---------------------------------------------------------------------------------------------
    // EA_TILE_C x EA_TILE_R tiles of the parent (k_extend_add_lds: every tile of every front above SMALL_F has a task, and the first tile of
    // a tiled LU front also factorises the front's first diagonal tile -- those tasks lead the level's list: they are the long ones); the
    // legacy kernel (k_extend_add) gets 32 x 256 tiles, only the ones a child reaches.  With the first-touch extend-add a 3D problem has
    // tens of millions of tiles (200^3: 22.6 M tasks + 30.4 M child pieces, 2.4 GB; built serially they were 1.7 of the 1.9 s of the launch
    // plans): the lists are laid out by a counting pass and filled by a second one, both spread over host threads front by front.  The
    // arrays do not depend on the number of threads (every front writes its own, precomputed ranges).
    {
        const bool all_tiles = ea_lds_active();
        struct EaParent {
            int32_t s, level;
            int64_t ntask, nhead, nrange; // tasks (nhead of them lead the level's list), child pieces
            int64_t head_pos, tail_pos, range_pos;
        };
        std::vector<EaParent> eap;
        for (int32_t l = 0; l < S.nlevels; l++)
            for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
                const int32_t s = S.level_sn[k];
                if (S.fsize(s) <= SMALL_F) continue; // small parents pull their children's blocks themselves (k_small_factor)
                bool any = false;
                for (int32_t c = S.child_ptr[s]; c < S.child_ptr[s + 1]; c++) any |= S.nrow(S.child_idx[c]) > 0;
                if (!any && !all_tiles) continue;
                eap.push_back({s, l, 0, 0, 0, 0, 0, 0});
            }
        struct EaScratch {
            std::vector<int32_t> ccut, rcut;
        };
        // one front: FILL = false counts (P.ntask / nhead / nrange), FILL = true writes the tasks at the positions of P
        auto ea_front = [&](EaParent &P, EaScratch &t, const bool FILL) {
            const int32_t s = P.s, f = S.fsize(s);
            const int32_t cstep = f <= 64 ? f : (all_tiles ? EA_TILE_C : 32), rstep = f <= 64 ? f : (all_tiles ? EA_TILE_R : 256);
            // where every child's (ascending) relative indices cross the tile boundaries: computed once per child, not per tile (a front of
            // 76 000 rows has 716 000 tiles; four binary searches per tile and child made `initialize` of such a matrix take minutes)
            const int32_t cb = S.child_ptr[s], nch_s = S.child_ptr[s + 1] - cb;
            const int32_t ncc = (f + cstep - 1) / cstep + 1, nrc = (f + rstep - 1) / rstep + 1;
            t.ccut.resize((size_t)nch_s * ncc), t.rcut.resize((size_t)nch_s * nrc);
            for (int32_t q = 0; q < nch_s; q++) {
                const int32_t ch = S.child_idx[cb + q];
                const int32_t *rb = S.rel.data() + S.sn_rowptr[ch], *re = S.rel.data() + S.sn_rowptr[ch + 1];
                for (int32_t k = 0; k < ncc; k++) t.ccut[(size_t)q * ncc + k] = (int32_t)(std::lower_bound(rb, re, std::min(f, k * cstep)) - rb);
                for (int32_t k = 0; k < nrc; k++) t.rcut[(size_t)q * nrc + k] = (int32_t)(std::lower_bound(rb, re, std::min(f, k * rstep)) - rb);
            }
            int64_t ntask = 0, nhead = 0, nrange = 0;
            int64_t tail_pos = P.tail_pos, range_pos = P.range_pos;
            for (int32_t c0 = 0; c0 < f; c0 += cstep)
                for (int32_t r0 = 0; r0 < f; r0 += rstep) {
                    const int32_t c1 = std::min(f, c0 + cstep), r1 = std::min(f, r0 + rstep);
                    if (S.sym_mode && r1 <= c0) continue; // tile strictly above the diagonal
                    const int64_t piece_begin = range_pos + nrange;
                    for (int32_t q = 0; q < nch_s; q++) {
                        const int32_t jlo = t.ccut[(size_t)q * ncc + c0 / cstep], jhi = t.ccut[(size_t)q * ncc + c0 / cstep + 1];
                        const int32_t ilo = t.rcut[(size_t)q * nrc + r0 / rstep], ihi = t.rcut[(size_t)q * nrc + r0 / rstep + 1];
                        if (jlo >= jhi || ilo >= ihi) continue;
                        if (FILL) {
                            const int32_t ch = S.child_idx[cb + q];
                            EaRange &rg = ear[(size_t)(range_pos + nrange)];
                            rg.jlo = jlo, rg.jhi = jhi, rg.ilo = ilo, rg.ihi = ihi;
                            rg.ldc = S.front_ld[ch];
                            rg.cb_off = S.front_off[ch] + S.npiv(ch) + (int64_t)S.npiv(ch) * rg.ldc;
                            rg.rel_off = S.sn_rowptr[ch];
                            rg.pad = 0;
                        }
                        nrange++;
                    }
                    const int64_t piece_end = range_pos + nrange;
                    if (!(piece_end > piece_begin || all_tiles)) continue;
                    const bool head = all_tiles && c0 == 0 && r0 == 0; // (first tile of its front: at the head of the level's list)
                    if (FILL) {
                        EaTask &tk = ea[(size_t)(head ? P.head_pos : tail_pos++)];
                        tk.f_off = S.front_off[s];
                        tk.ld = S.front_ld[s];
                        tk.piece_begin = (int32_t)piece_begin, tk.piece_end = (int32_t)piece_end;
                        tk.sym = S.sym_mode ? 1 : 0; // L D L^T parent: lower triangle only
                        tk.c0 = c0, tk.r0 = r0, tk.nc = c1 - c0, tk.nr = r1 - r0;
                        tk.lu_slot = -1, tk.lu_first = 0, tk.lu_nb = 0, tk.pad = head ? 1 : 0;
                        if (head && tiled_slot[(size_t)s] >= 0 && ea_lu_active())
                            tk.lu_slot = tiled_slot[(size_t)s], tk.lu_first = S.sn_first[s], tk.lu_nb = std::min<int32_t>(NB, S.npiv(s));
                    }
                    ntask++, nhead += head ? 1 : 0;
                }
            if (!FILL) P.ntask = ntask, P.nhead = nhead, P.nrange = nrange;
        };
        // the fronts are handed out one at a time, largest (the last levels) first
        std::atomic<bool> ea_oom{false};
        auto ea_pass = [&](const bool FILL, int nthreads) {
            std::atomic<size_t> next{0};
            auto body = [&]() {
                try {
                    EaScratch t;
                    for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < eap.size();) ea_front(eap[eap.size() - 1 - i], t, FILL);
                } catch (const std::bad_alloc &) { // (an exception must not leave a thread)
                    ea_oom.store(true);
                }
            };
            if (nthreads <= 1) {
                body();
                return;
            }
            std::vector<std::thread> pool;
            for (int i = 0; i < nthreads; i++) pool.emplace_back(body);
            for (auto &th : pool) th.join();
        };
        int64_t tiles_bound = 0;
        for (const EaParent &P : eap) {
            const int64_t f = S.fsize(P.s);
            tiles_bound += f <= 64 ? 1 : ((f + 31) / 32) * ((f + 63) / 64);
        }
        int ea_threads = given(&Tunables::nd_threads) ? nd_threads : (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
        if (tiles_bound < par_min) ea_threads = 1; // (not worth the thread start-up)
        ea_pass(false, ea_threads);
        if (ea_oom.load()) return ERROR_MALLOC;
        // layout: level by level, a level's first tiles (nhead) in front of its other tasks, both in the order of the level's fronts
        int64_t task_pos = 0, range_pos = 0;
        size_t i0 = 0;
        for (int32_t l = 0; l < S.nlevels; l++) {
            LevelPlan &L = levels[l];
            size_t i1 = i0;
            int64_t heads = 0, total = 0;
            while (i1 < eap.size() && eap[i1].level == l) heads += eap[i1].nhead, total += eap[i1].ntask, i1++;
            int64_t hp = task_pos, tp = task_pos + heads;
            for (size_t i = i0; i < i1; i++) {
                EaParent &P = eap[i];
                P.head_pos = hp, P.tail_pos = tp, P.range_pos = range_pos;
                hp += P.nhead, tp += P.ntask - P.nhead, range_pos += P.nrange;
            }
            if (task_pos + total > 0x7fffffffLL || range_pos > 0x7fffffffLL) return ERROR_HIPMF_SYMBOLIC;
            L.ea_off = (int32_t)task_pos, L.ea_cnt = (int32_t)total;
            task_pos += total;
            i0 = i1;
        }
        ea.resize((size_t)task_pos), ear.resize((size_t)range_pos);
        ea_pass(true, ea_threads);
        if (ea_oom.load()) return ERROR_MALLOC;
    }
    plan_digest = 0;
    if (want_digest) {
        // (diagnostic / tests: one number over what the threaded pieces of initialize produce -- row structures, relative indices, pool
        //  layout, extend-add task lists -- to compare thread counts and builds; a pass over gigabytes at 200^3, hence opt-in)
        uint64_t h = 1469598103934665603ull;
        auto eat = [&](const void *p, size_t bytes) {
            const unsigned char *b = (const unsigned char *)p;
            for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 1099511628211ull;
        };
        eat(S.sn_rowptr.data(), S.sn_rowptr.size() * sizeof(int64_t)), eat(S.sn_rows.data(), S.sn_rows.size() * sizeof(int32_t));
        eat(S.rel.data(), S.rel.size() * sizeof(int32_t)), eat(S.front_off.data(), S.front_off.size() * sizeof(int64_t));
        eat(ea.data(), ea.size() * sizeof(EaTask)), eat(ear.data(), ear.size() * sizeof(EaRange));
        for (const LevelPlan &L : levels) eat(&L.ea_off, sizeof L.ea_off), eat(&L.ea_cnt, sizeof L.ea_cnt);
        plan_digest = (int64_t)(h & 0x7fffffffffffffffull);
    }
    if (ea_lds_active()) {
        HIPMF_ALLOW_LDS(k_extend_add_lds<false>, sizeof(double) * EA_TILE_C * EA_TILE_R);
        HIPMF_ALLOW_LDS(k_extend_add_lds<true>, sizeof(double) * EA_TILE_C * EA_TILE_R);
    }
    if (use_mid && !S.sym_mode) { // (a front with 64 pivots stages 67 KB)
        HIPMF_ALLOW_LDS(k_front<10>, sizeof(double) * MID_LDS_DOUBLES);
        HIPMF_ALLOW_LDS(k_front<16>, sizeof(double) * MID_LDS_DOUBLES);
        HIPMF_ALLOW_LDS(k_front<24>, sizeof(double) * MID_LDS_DOUBLES);
        HIPMF_ALLOW_LDS(k_front_lu<false>, sizeof(double) * MIDL_LDS_DOUBLES);
        HIPMF_ALLOW_LDS(k_front_lu<true>, sizeof(double) * MIDL_LDS_DOUBLES);
    }
    pl_lap("factor launch plans");
    allbig_off = (int32_t)lists.size();
    allbig_cnt = (int32_t)allbig.size();
    lists.insert(lists.end(), allbig.begin(), allbig.end());
    HIPC(d_fd.upload(fd), ERROR_HIP_MALLOC);
    HIPC(d_bigfd.upload(bigfd), ERROR_HIP_MALLOC);
    HIPC(d_ea.upload(ea), ERROR_HIP_MALLOC);
    HIPC(d_ear.upload(ear), ERROR_HIP_MALLOC);
    dws_stride = std::max(max_big, 1);
    HIPC(d_dws.alloc(2 * NB * NB * (size_t)std::max(max_big, 1)), ERROR_HIP_MALLOC);
    HIPC(d_st.upload(stasks), ERROR_HIP_MALLOC);
    HIPC(d_lists.upload(lists), ERROR_HIP_MALLOC);
    n_lists = (int64_t)lists.size();
    HIPC(d_tasks.upload(tasks), ERROR_HIP_MALLOC);
    if (!chain.empty()) {
        HIPC(d_chain.upload(chain), ERROR_HIP_MALLOC);
        chain_words += 1; // the error word
        HIPC(d_chain_cnt.alloc((size_t)chain_words), ERROR_HIP_MALLOC);
    }
    HIPC(d_rows.upload(S.sn_rows), ERROR_HIP_MALLOC);
    {
        // (+ 64 entries: the solve kernels read relative indices and workspace entries from clamped addresses, unconditionally)
        // (no padded copy of the array on the host: at 200^3 it holds hundreds of megabytes)
        HIPC(d_rel.alloc(S.rel.size() + 64), ERROR_HIP_MALLOC);
        if (!S.rel.empty()) HIPC(hipMemcpy(d_rel, S.rel.data(), sizeof(int32_t) * S.rel.size(), hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
        HIPC(hipMemset(d_rel + S.rel.size(), 0, sizeof(int32_t) * 64), ERROR_HIP_MEMCPY);
    }
    HIPC(d_child.upload(S.child_idx), ERROR_HIP_MALLOC);
    pl_lap("descriptor / index uploads");
    // (+ WT_CHUNK: the wave-subtree kernels read the factor in whole 1 KB pieces)
    // (tried: these two allocations on a host thread of their own beside the planning -- the runtime serialises the plan uploads behind
    //  the large allocation, initialize of the 200^3 matrix 6.0 -> 6.9 s)
    HIPC(d_pool.alloc(std::max<int64_t>(pool_doubles, 1) + WT_CHUNK), ERROR_HIP_MALLOC);
    HIPC(d_work.alloc(std::max<int64_t>(work_doubles, 1) + 64), ERROR_HIP_MALLOC);
    pl_lap("pool + workspace allocation");
    if (tail) {
        const int32_t tcode = tail();
        if (tcode != SUCCESSFUL_EXIT) return tcode;
        pl_lap("tail (permutation, assembly lists, buffers)");
    }
    // (the task lists of the dependency-driven solves were built beside everything above: see solve_plans)
    if (sp_thread.joinable()) sp_thread.join();
    if (sp_code != SUCCESSFUL_EXIT) return sp_code;
    pl_lap("wait for the solve task lists + their uploads");
    if (opt.verbose) fprintf(stderr, "hipmf: initialize: plan pieces:%s\n", pl_log.c_str());
    return SUCCESSFUL_EXIT;
}

int32_t Solver::factorize(const double *values, bool on_device) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!values) return ERROR_NULL_POINTER;
    DeviceScope dev_scope(device);
    int32_t code = stage_values(d_vals, values, false, on_device);
    if (code != SUCCESSFUL_EXIT) return code;
    code = run_factor();
    if (code != SUCCESSFUL_EXIT) return code;
    if (n_weak_diag > 0 && !rematching && !rematch_futile) return rematch_and_factorize();
    factorized = true;
    return n_zero_pivot > 0 ? singular_verdict() : SUCCESSFUL_EXIT;
}

// The pivot order of a handle is static: nested dissection on the pattern, plus -- for a weak diagonal -- the maximum-product matching
// of the values seen at initialize.  UMFPACK pivots dynamically in every umfpack_di_numeric (interface_umfpack.c:167); here every
// factorize checks the diagonal of the system it is about to factorise (k_diag_check) and, when the values call for another
// matching (none was computed because initialize had no values, or the values changed a lot), computes it from THESE values and
// redoes the analysis: the price of an initialize, paid only when the diagonal really is weak.  The value map and all options survive.
int32_t Solver::rematch_and_factorize() {
    const int32_t n = S.n;
    const int64_t nnz = S.nnz_a;
    std::vector<double> hv((size_t)nnz);
    HIPC(hipMemcpy(hv.data(), d_vals, sizeof(double) * nnz, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    const NumericOptions nopt = opt;
    const std::vector<int32_t> seg_ptr = h_seg_ptr, seg_idx = h_seg_idx;
    const int64_t nin = nnz_in;
    const PhaseTimes keep_times = times;
    const int64_t keep_rematch = rematch_count, keep_fallbacks = fused_fallbacks;
    const std::vector<int32_t> keep_emap = h_emap;
    const int64_t keep_low = nnz_low;
    release();
    rematching = true;
    int32_t code = initialize_impl(n, h_rp_keep.data(), h_ci_keep.data(), sym_lower_keep, sopt_keep, nopt, hv.data());
    if (code == SUCCESSFUL_EXIT && nin > 0) code = set_value_map(nin, seg_ptr.data(), seg_idx.data(), true);
    const bool had_expansion = keep_low > 0;
    if (code != SUCCESSFUL_EXIT) {
        rematching = false;
        const std::string keep = last_error;
        release();
        last_error = "re-analysis after a change of the matching failed: " + keep;
        return code;
    }
    times = keep_times;
    rematch_count = keep_rematch + 1;
    fused_fallbacks = keep_fallbacks;
    // (hv holds the EXPANDED values of the handle's own CSR: they are factorised as they are, the expansion map comes back afterwards)
    code = factorize(hv.data(), false); // (rematching is still set: one re-analysis per call)
    if (had_expansion && initialized) {
        // (without the map the next factorize would read the caller's lower-triangle buffer as expanded values)
        const int32_t ecode = set_expansion(keep_low, keep_emap);
        if (ecode != SUCCESSFUL_EXIT) {
            rematching = false;
            const std::string keep = last_error;
            release();
            last_error = "re-analysis after a change of the matching failed: " + keep;
            return ecode;
        }
    }
    rematching = false;
    // a new matching that leaves the diagonal weak (structurally singular matrix, no perfect matching, the boundary case of the
    // criterion) cannot be improved by another one: later factorizes keep this order instead of redoing the analysis every time
    if (n_weak_diag > 0) rematch_futile = true;
    if (opt.verbose) fprintf(stderr, "hipmf: factorize: weak diagonal for these values: maximum-product matching recomputed, analysis redone\n");
    return code;
}

int32_t Solver::set_value_map(int64_t nin, const int32_t *seg_ptr, const int32_t *seg_idx, bool signed_map) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!seg_ptr || !seg_idx) return ERROR_NULL_POINTER;
    const int64_t nnz = S.nnz_a;
    // (seg_ptr[nnz] = number of map entries: nin for a plain triplet map; a signed map -- the real-equivalent form of a complex matrix,
    //  interface_complex_hipmf.cpp -- uses every input value twice and marks subtracted entries ~k)
    if (nin < 1 || nin > 0x7fffffffLL || seg_ptr[0] != 0 || (signed_map ? seg_ptr[nnz] < 1 : seg_ptr[nnz] != nin)) return ERROR_HIPMF_INVALID_VALUE;
    for (int64_t j = 0; j < nnz; j++)
        if (seg_ptr[j + 1] < seg_ptr[j]) return ERROR_HIPMF_INVALID_VALUE;
    const int64_t nmap = seg_ptr[nnz];
    for (int64_t q = 0; q < nmap; q++) {
        if (seg_idx[q] < 0 && !signed_map) return ERROR_HIPMF_INVALID_VALUE;
        const int64_t k = seg_idx[q] < 0 ? ~(int64_t)seg_idx[q] : (int64_t)seg_idx[q]; // (~k: subtracted entry)
        if (k >= nin) return ERROR_HIPMF_INVALID_VALUE;
    }
    DeviceScope dev_scope(device);
    HIPC(d_seg_ptr.alloc(nnz + 1), ERROR_HIP_MALLOC);
    HIPC(d_seg_idx.alloc(nmap), ERROR_HIP_MALLOC);
    HIPC(d_vin.alloc(nin), ERROR_HIP_MALLOC);
    HIPC(hipMemcpy(d_seg_ptr, seg_ptr, sizeof(int32_t) * (nnz + 1), hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpy(d_seg_idx, seg_idx, sizeof(int32_t) * nmap, hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
    nnz_in = nin;
    sn_map_ready = false; // (the inverse map of values_outer is rebuilt from this one at its next mapped call)
    if (h_seg_ptr.data() != seg_ptr) h_seg_ptr.assign(seg_ptr, seg_ptr + nnz + 1), h_seg_idx.assign(seg_idx, seg_idx + nmap);
    return SUCCESSFUL_EXIT;
}

int32_t Solver::factorize_mapped(const double *input, bool on_device) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!input) return ERROR_NULL_POINTER;
    if (nnz_in < 1) return ERROR_HIPMF_INVALID_VALUE; // no map set
    DeviceScope dev_scope(device);
    int32_t code = stage_values(d_vals, input, true, on_device);
    if (code == SUCCESSFUL_EXIT) code = run_factor();
    if (code != SUCCESSFUL_EXIT) return code;
    if (n_weak_diag > 0 && !rematching && !rematch_futile) return rematch_and_factorize();
    factorized = true;
    return n_zero_pivot > 0 ? singular_verdict() : SUCCESSFUL_EXIT;
}

// The dependency-driven launches are safe ONE AT A TIME on a device: a task waits for tasks with lower workgroup indices of its own
// launch, which the hardware has placed before it.  Two such launches resident together (two handles on two host threads: the real
// and the complex system of russell_ode's Radau5, radau5.rs:270-296) can fill the compute units with each other's waiting
// workgroups and stall until a wait gives up (seen in round 4 with two solve lanes of one handle, profiles/r04_solve_lanes.txt).
// One gate per device, process-wide: a solve holds it from its first launch to its last synchronisation, so at most one handle's
// dependency-driven launches are in flight on a device; the other handle's solve waits (a solve takes a millisecond).  Launches that wait
// for nothing inside themselves (factorisations, products, the level-set solves) are not gated: they cannot hold anything up.
// Round 6: the gate also orders PROCESSES that share a GPU (two ranks on one device, a notebook beside a job): behind the in-process
// mutex sits a process-shared ROBUST pthread mutex in a page of /dev/shm/russell_hipmf_gate_<PCI bus id of the device> -- uncontended, a
// lock / unlock pair is two atomic operations in user space (a first version used flock(): two system calls per pass pair cost 0.9 % of
// the headline on the sandboxed GPU boxes, profiles/r06_two_processes.txt); a process that dies with the lock held leaves it
// recoverable (EOWNERDEAD -> pthread_mutex_consistent).  The process that creates the file initialises the mutex and then publishes a
// magic word; one that finds the file waits for the word (a creator that died in between: no process gate for the late-comers).  Where
// the file cannot be opened or mapped the gate stays in-process; HIPMF_PROCESS_GATE=0 switches the shared part off.
struct SharedGatePage {
    std::atomic<uint32_t> magic;
    pthread_mutex_t mu;
};
struct DeviceGate {
    std::mutex mu;
    int state = -2; // -2: not tried yet, -1: no shared part, 0: shared page mapped
    SharedGatePage *page = nullptr;
    void open_shared(int device) {
        state = -1;
#ifndef HIPMF_EMULATED
        if (!Tunables::now(&Tunables::process_gate)) return;
        constexpr uint32_t MAGIC = 0x48504d47u; // "HPMG"
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) return;
        for (char *c = bus; *c; c++)
            if (*c == ':' || *c == '.' || *c == '/') *c = '_';
        char path[160];
        snprintf(path, sizeof path, "/dev/shm/russell_hipmf_gate_%s", bus);
        const mode_t old = umask(0);
        bool creator = true;
        int fd = ::open(path, O_CREAT | O_EXCL | O_RDWR | O_CLOEXEC, 0666);
        if (fd < 0 && errno == EEXIST) creator = false, fd = ::open(path, O_RDWR | O_CLOEXEC);
        umask(old);
        if (fd < 0) return;
        if (creator && ftruncate(fd, (off_t)sizeof(SharedGatePage)) != 0) {
            ::close(fd);
            return;
        }
        if (!creator) { // (the creator may not have sized the file yet)
            struct stat st;
            for (int spin = 0; spin < 2000; spin++) {
                if (fstat(fd, &st) == 0 && (size_t)st.st_size >= sizeof(SharedGatePage)) break;
                usleep(500);
            }
            if (fstat(fd, &st) != 0 || (size_t)st.st_size < sizeof(SharedGatePage)) {
                ::close(fd);
                return;
            }
        }
        void *m = mmap(nullptr, sizeof(SharedGatePage), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        ::close(fd);
        if (m == MAP_FAILED) return;
        SharedGatePage *pg = (SharedGatePage *)m;
        if (creator) {
            pthread_mutexattr_t at;
            bool ok = pthread_mutexattr_init(&at) == 0;
            ok = ok && pthread_mutexattr_setpshared(&at, PTHREAD_PROCESS_SHARED) == 0;
            ok = ok && pthread_mutexattr_setrobust(&at, PTHREAD_MUTEX_ROBUST) == 0;
            ok = ok && pthread_mutex_init(&pg->mu, &at) == 0;
            (void)pthread_mutexattr_destroy(&at);
            if (!ok) {
                munmap(m, sizeof(SharedGatePage));
                return;
            }
            pg->magic.store(MAGIC, std::memory_order_release);
        } else {
            bool ready = false;
            for (int spin = 0; spin < 2000 && !ready; spin++) { // <= 1 s
                ready = pg->magic.load(std::memory_order_acquire) == MAGIC;
                if (!ready) usleep(500);
            }
            if (!ready) {
                munmap(m, sizeof(SharedGatePage));
                return;
            }
        }
        page = pg;
        state = 0;
#else
        (void)device;
#endif
    }
    // (call with mu held) true: the shared lock was free
    bool file_lock(int device) {
        if (state == -2) open_shared(device);
        if (state != 0) return true;
        int r = pthread_mutex_trylock(&page->mu);
        bool free_ = r == 0 || r == EOWNERDEAD;
        if (r == EBUSY) r = pthread_mutex_lock(&page->mu);
        if (r == EOWNERDEAD) (void)pthread_mutex_consistent(&page->mu); // (the owner died inside a solve: the lock is ours now)
        if (r != 0 && r != EOWNERDEAD) state = -1;                      // (unusable: in-process only from now on)
        shared_held = state == 0;
        return free_;
    }
    void file_unlock() {
        if (shared_held) (void)pthread_mutex_unlock(&page->mu);
        shared_held = false;
    }
    bool shared_held = false;
};
static DeviceGate &device_gate(int device) {
    static DeviceGate gates[64];
    return gates[device >= 0 && device < 64 ? device : 0];
}
// what std::unique_lock<std::mutex> was to the in-process gate
struct GateLock {
    DeviceGate &g;
    int device;
    bool owned = false;
    GateLock(DeviceGate &gate, int dev) : g(gate), device(dev) {}
    ~GateLock() {
        if (owned) unlock();
    }
    bool owns_lock() const { return owned; }
    // true: nobody held the gate (neither another handle of this process nor another process)
    bool lock_counting() {
        bool free_ = g.mu.try_lock();
        if (!free_) g.mu.lock();
        if (!g.file_lock(device)) free_ = false;
        owned = true;
        return free_;
    }
    void lock() { (void)lock_counting(); }
    void unlock() {
        g.file_unlock();
        g.mu.unlock();
        owned = false;
    }
};

int32_t Solver::run_factor() {
    const int32_t n = S.n;
    const int64_t nnz = S.nnz_a;
    int64_t launches = 0;
    forget_border(); // (a border belongs to the factorisation it was set for: Solver::set_border)
    HIPC(hipEventRecord((hipEvent_t)ev[0], STREAM), ERROR_HIP_SYNCHRONIZE);
    // (with a matching in force the scalings dr, dc of initialize stay: the structure was chosen for them)
    if (!matched)
        hipLaunchKernelGGL(k_row_scale, dim3((n + 255) / 256), dim3(256), 0, STREAM, n, d_rp, d_vals, d_tptr, d_tidx, opt.scaling, S.sym_mode ? 1 : 0, d_rs);
    HIPC(hipMemsetAsync(d_scalar, 0, 4 * sizeof(unsigned long long), STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(d_info, 0, sizeof(FactorInfo), STREAM), ERROR_HIP_MEMCPY);
    const bool chained = use_chain && d_chain_cnt != nullptr;
    GateLock gate(device_gate(device), device); // (the chained tiled steps wait inside their launch: see device_gate)
    if (chained) gate.lock();
    const bool PZ = opt.complex_pairs; // the pivot searches keep the (real, imaginary) rows of a complex row together (tile_lu32_z)
    if (chained) HIPC(hipMemsetAsync(d_chain_cnt, 0, sizeof(int32_t) * (size_t)chain_words, STREAM), ERROR_HIP_MEMCPY);
    int gs = (int)std::min<int64_t>(2048, (nnz + 255) / 256);
    hipLaunchKernelGGL(k_absmax, dim3(gs), dim3(256), 0, STREAM, nnz, d_vals, d_arow, d_ci, d_rs, d_cs, d_vs, d_vs2, d_scalar, d_info);
    launches += 2;
    // What only the big fronts (or nobody before the end) need runs beside the first levels, which hold small fronts only: the diagonal
    // check and the zero-fill / identity blocks of E, E' -- 65 of the 128 us this phase took in front of the 1M-DOF factorisation.
    bool pre_forked = false;
#ifndef HIPMF_EMULATED
    pre_forked = overlap_small && !use_graph && !levels.empty() && levels[0].ea_cnt == 0 && levels[0].steps.empty();
#endif
    hipStream_t pst = STREAM;
    if (pre_forked) {
        HIPC(hipEventRecord((hipEvent_t)ev_pre0, STREAM), ERROR_HIP_SYNCHRONIZE);
        HIPC(hipStreamWaitEvent((hipStream_t)stream4, (hipEvent_t)ev_pre0, 0), ERROR_HIP_SYNCHRONIZE);
        pst = (hipStream_t)stream4;
    }
    // (symmetric-lower storage that kept its L D L^T plan -- ADVICE r05: the FIRST values such a handle sees get the same look, once, so that
    //  a saddle-point / KKT matrix does not pass unnoticed when HIPMF_OPTION_SYM_RECHECK is off; the stored half of a row under-states the
    //  row's largest entry, a zero or missing diagonal is caught for certain.  Nothing is re-analysed: HIPMF_COUNTER_SYM_WEAK_DIAGONAL tells)
    const bool sym_first_look = S.sym_lower && opt.matching > 0 && !sym_diag_looked;
    if ((!S.sym_lower && opt.matching > 0) || sym_first_look) { // (general storage: would a maximum-product matching be called for with these values?)
        hipLaunchKernelGGL(k_diag_check, dim3((n + 255) / 256), dim3(256), 0, pst, n, d_rp, d_ci, d_vs, d_dcol, 0.01, d_info, opt.complex_pairs ? 1 : 0);
        launches++;
    }
    if (zero_cnt > 0) { // the E / E' panels start as [I; 0] / [I, 0]
        hipLaunchKernelGGL(k_zero, dim3(zero_cnt), dim3(256), 0, pst, d_zero, d_pool);
        hipLaunchKernelGGL(k_set_identity, dim3(allbig_cnt), dim3(256), 0, pst, d_lists + allbig_off, d_fd, d_pool);
        launches += 2;
    }
    if (pre_forked) HIPC(hipEventRecord((hipEvent_t)ev_pre1, (hipStream_t)stream4), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipEventRecord((hipEvent_t)ev[1], STREAM), ERROR_HIP_SYNCHRONIZE);
    // The working blocks of a level take over storage other fronts have left: they are zero-filled and receive A's entries when the
    // level BEFORE has pulled its children's contribution blocks (the storage plan frees a block after its parent's level's
    // extend-add), on the side stream, beside that level's factorisation.
    auto fill_level = [&](const LevelPlan &L, hipStream_t st) {
        if (L.zero_cnt > 0) {
            hipLaunchKernelGGL(k_zero, dim3(L.zero_cnt), dim3(256), 0, st, d_zero + L.zero_off, d_pool);
            launches++;
        }
        if (L.sc_cnt > 0) {
            hipLaunchKernelGGL(k_scatter, dim3((unsigned)std::min<int64_t>(2048, ((int64_t)L.sc_cnt + 255) / 256)), dim3(256), 0, st, (int64_t)L.sc_cnt,
                               d_sc_k + L.sc_off, d_sc_at + L.sc_off, d_vs, d_vs2, d_pool);
            launches++;
        }
    };
    // Everything from here to the last level is a FIXED sequence of launches (grids, arguments and cross-stream edges are set by the
    // plan): it is captured once into a hipGraph and replayed by later factorisations -- the host-side event calls between the
    // streams cost 5 - 11 us of idle device at every level boundary when issued eagerly (profiles/r03_factor_sequence.txt: 214 us
    // of gaps in one factorisation of the 1M-DOF matrix).
    auto enqueue_levels = [&]() -> int32_t {
    const bool ea_lds = ea_lds_active(); // the working blocks are written whole by the extend-add: no zero-fill / scatter launches
    bool pre_pending = pre_forked;
    if (!levels.empty() && !ea_lds) fill_level(levels[0], STREAM);
    for (size_t li = 0; li < levels.size(); li++) {
        const LevelPlan &L = levels[li];
        const LevelPlan *Lnext = li + 1 < levels.size() ? &levels[li + 1] : nullptr;
        const bool fill_next = !ea_lds && Lnext && (Lnext->zero_cnt > 0 || Lnext->sc_cnt > 0);
        if (pre_pending && (L.ea_cnt > 0 || !L.steps.empty() || L.mid_total() > 0 || fill_next)) {
            HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_pre1, 0), ERROR_HIP_SYNCHRONIZE);
            pre_pending = false;
        }
        if (L.ea_cnt > 0) {
            if (ea_lds && S.sym_mode)
                hipLaunchKernelGGL(k_extend_add_lds<true>, dim3(L.ea_cnt), dim3(256), sizeof(double) * EA_TILE_C * EA_TILE_R, STREAM, d_ea + L.ea_off, d_ear, d_rel,
                                   d_pool, d_ea_sc + L.ea_off, d_sc_k, d_sc_pos, d_vs, d_vs2, d_dws, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag);
            else if (ea_lds)
                hipLaunchKernelGGL((PZ ? k_extend_add_lds<false, true> : k_extend_add_lds<false, false>), dim3(L.ea_cnt), dim3(256), sizeof(double) * EA_TILE_C * EA_TILE_R, STREAM, d_ea + L.ea_off, d_ear, d_rel,
                                   d_pool, d_ea_sc + L.ea_off, d_sc_k, d_sc_pos, d_vs, d_vs2, d_dws, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag);
            else if (S.sym_mode) hipLaunchKernelGGL(k_extend_add<true>, dim3(L.ea_cnt), dim3(256), 0, STREAM, d_ea + L.ea_off, d_ear, d_rel, d_pool);
            else hipLaunchKernelGGL(k_extend_add<false>, dim3(L.ea_cnt), dim3(256), 0, STREAM, d_ea + L.ea_off, d_ear, d_rel, d_pool);
            launches++;
        }
        // a level's small fronts and its big fronts are independent of each other (both only need the level's extend-add):
        // when the level has both, the small ones are factorised on a second stream beside the tiled steps
        const bool has_mid = L.mid_total() > 0;
        const bool forked = overlap_small && ((L.small_cnt > 0 && (!L.steps.empty() || has_mid)) || fill_next);
        if (L.small_cnt > 0) {
            size_t shmem = sizeof(double) * (size_t)L.small_ld * (size_t)L.small_ld;
            hipStream_t sst = STREAM;
            if (forked) {
                HIPC(hipEventRecord((hipEvent_t)ev_fork, STREAM), ERROR_HIP_SYNCHRONIZE);
                HIPC(hipStreamWaitEvent((hipStream_t)stream2, (hipEvent_t)ev_fork, 0), ERROR_HIP_SYNCHRONIZE);
                sst = (hipStream_t)stream2;
            }
            const SmallAsm sasm = {d_sd, d_sa_k, d_sa_pos, d_vs, d_vs2, d_child, d_rel, d_lists};
            // (HIPMF_SMALL_PAIR=1: the two launches of an all-small level side by side -- the first on the third stream)
            const bool pair = small_pair && L.small_cnt_a > 0 && !forked && !use_graph && L.steps.empty() && !has_mid;
            if (L.small_cnt_a > 0) {
                const size_t shmem_a = sizeof(double) * (size_t)L.small_ld_a * (size_t)L.small_ld_a;
                hipStream_t ast = sst;
                if (pair) {
                    HIPC(hipEventRecord((hipEvent_t)ev_fork3, STREAM), ERROR_HIP_SYNCHRONIZE);
                    HIPC(hipStreamWaitEvent((hipStream_t)stream3, (hipEvent_t)ev_fork3, 0), ERROR_HIP_SYNCHRONIZE);
                    ast = (hipStream_t)stream3;
                }
                hipLaunchKernelGGL((PZ ? k_small_factor<1, true> : k_small_factor<1, false>), dim3(L.small_cnt_a), dim3(64), shmem_a, ast, d_lists + L.small_off, d_fd, d_pool, d_lperm,
                                   d_scalar, opt.pivot_epsilon, d_info, L.small_ld_a, sasm, d_diag);
                launches++;
                if (pair) HIPC(hipEventRecord((hipEvent_t)ev_join3, (hipStream_t)stream3), ERROR_HIP_SYNCHRONIZE);
            }
            // few fronts in the launch: four wavefronts per front (the launch lasts as long as one front's LU)
            const int32_t cnt_b = L.small_cnt - L.small_cnt_a;
            if (cnt_b <= small_wide_max && L.small_ld > 33)
                hipLaunchKernelGGL((PZ ? k_small_factor<4, true> : k_small_factor<4, false>), dim3(cnt_b), dim3(256), shmem, sst, d_lists + L.small_off + L.small_cnt_a, d_fd, d_pool, d_lperm,
                                   d_scalar, opt.pivot_epsilon, d_info, L.small_ld, sasm, d_diag);
            else
                hipLaunchKernelGGL((PZ ? k_small_factor<1, true> : k_small_factor<1, false>), dim3(cnt_b), dim3(64), shmem, sst, d_lists + L.small_off + L.small_cnt_a, d_fd, d_pool, d_lperm,
                                   d_scalar, opt.pivot_epsilon, d_info, L.small_ld, sasm, d_diag);
            launches++;
            if (pair) HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_join3, 0), ERROR_HIP_SYNCHRONIZE);
        } else if (forked) {
            HIPC(hipEventRecord((hipEvent_t)ev_fork, STREAM), ERROR_HIP_SYNCHRONIZE);
            HIPC(hipStreamWaitEvent((hipStream_t)stream2, (hipEvent_t)ev_fork, 0), ERROR_HIP_SYNCHRONIZE);
        }
        if (fill_next) fill_level(*Lnext, forked ? (hipStream_t)stream2 : STREAM);
        if (forked) HIPC(hipEventRecord((hipEvent_t)ev_join, (hipStream_t)stream2), ERROR_HIP_SYNCHRONIZE);
        // the fronts of the middle of the tree: one workgroup per front, one launch per size class (kernels_factor_front.hpp)
        // beside the level's tiled steps (and its small fronts): all three only depend on the level's extend-add
        const bool mid_forked = overlap_small && has_mid && (!L.steps.empty() || forked);
        if (has_mid) {
            hipStream_t mst = STREAM;
            if (mid_forked) {
                // (one record serves both side streams: nothing went out on the main stream since the fork of the small fronts)
                if (forked) HIPC(hipStreamWaitEvent((hipStream_t)stream3, (hipEvent_t)ev_fork, 0), ERROR_HIP_SYNCHRONIZE);
                else {
                    HIPC(hipEventRecord((hipEvent_t)ev_fork3, STREAM), ERROR_HIP_SYNCHRONIZE);
                    HIPC(hipStreamWaitEvent((hipStream_t)stream3, (hipEvent_t)ev_fork3, 0), ERROR_HIP_SYNCHRONIZE);
                }
                mst = (hipStream_t)stream3;
            }
            int32_t moff = L.mid_off;
            for (int c = LevelPlan::MID_CLASSES - 1; c >= 0; c--) moff += L.mid_cnt[c]; // (the largest class goes first: its workgroups run longest)
            for (int c = LevelPlan::MID_CLASSES - 1; c >= 0; c--) {
                moff -= L.mid_cnt[c];
                if (L.mid_cnt[c] == 0) continue;
                const size_t dyn = sizeof(double) * (size_t)L.mid_lds[c];
                const FrontDesc *mfd = d_bigfd + moff;
                if (c >= 3) {
                    hipLaunchKernelGGL((PZ ? k_front_lu<true> : k_front_lu<false>), dim3(L.mid_cnt[c]), dim3(64 * MIDL_NW), dyn, mst, mfd, d_pool, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag);
                    launches++;
                    continue;
                }
#define HIPMF_LAUNCH_FRONT(CM) \
    hipLaunchKernelGGL(k_front<CM>, dim3(L.mid_cnt[c]), dim3(64 * MID_NW), dyn, mst, mfd, d_pool, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag)
                if (c == 0) HIPMF_LAUNCH_FRONT(10);
                else if (c == 1) HIPMF_LAUNCH_FRONT(16);
                else HIPMF_LAUNCH_FRONT(24);
#undef HIPMF_LAUNCH_FRONT
                launches++;
            }
            if (mid_forked) {
                // (... and one wait joins both: stream3 takes stream2's end along)
                if (forked) HIPC(hipStreamWaitEvent((hipStream_t)stream3, (hipEvent_t)ev_join, 0), ERROR_HIP_SYNCHRONIZE);
                HIPC(hipEventRecord((hipEvent_t)ev_join3, (hipStream_t)stream3), ERROR_HIP_SYNCHRONIZE);
            }
        }
        int32_t k0 = 0;
        if (chained && L.chain_cnt > 0) {
            // all tiled steps of the level in one launch (kernels_factor_chain.hpp)
            const FrontDesc *lfd = d_bigfd + L.bigfd_off;
            const StepPlan &st0 = L.steps[0];
            const int32_t pre_lu = 1; // (the first diagonal tiles always get their launch here: a panel task that factorises the tile itself is 10 us longer)
            if (pre_lu) {
                if (S.sym_mode) hipLaunchKernelGGL(k_diag0<true>, dim3(st0.nactive), dim3(64), 0, STREAM, lfd, d_pool, d_lperm, d_dws, d_scalar, opt.pivot_epsilon, d_info, d_diag);
                else hipLaunchKernelGGL((PZ ? k_diag0<false, true> : k_diag0<false, false>), dim3(st0.nactive), dim3(64), 0, STREAM, lfd, d_pool, d_lperm, d_dws, d_scalar, opt.pivot_epsilon, d_info, d_diag);
                launches++;
            }
            const ChainTask *ct = (const ChainTask *)d_chain + L.chain_off;
            if (S.sym_mode)
                hipLaunchKernelGGL(k_chain<true>, dim3(L.chain_cnt), dim3(256), 0, STREAM, ct, lfd, d_pool, d_lperm, d_dws, dws_stride, d_scalar,
                                   opt.pivot_epsilon, d_info, d_diag, pre_lu, d_chain_cnt, d_chain_cnt + (chain_words - 1));
            else
                hipLaunchKernelGGL(k_chain<false>, dim3(L.chain_cnt), dim3(256), 0, STREAM, ct, lfd, d_pool, d_lperm, d_dws, dws_stride, d_scalar,
                                   opt.pivot_epsilon, d_info, d_diag, pre_lu, d_chain_cnt, d_chain_cnt + (chain_words - 1));
            launches++;
        } else {
        bool rest_pending = false; // the bulk of a split update is in flight on stream4
        for (const StepPlan &st : L.steps) {
            const FrontDesc *lfd = d_bigfd + L.bigfd_off; // descriptors of the level's tiled fronts, in slot order
            // step 0 of a level with many tiled fronts: the first diagonal tiles are factorised once, by a launch of their own (k_diag0)
            const bool ea_lu = ea_lu_active(); // the first diagonal tiles were factorised by the extend-add (k_extend_add_lds)
            const int32_t pre_lu = (k0 == 0 && (ea_lu || (st.n_panel >= diag0_min_panels && (S.sym_mode || !use_binv)))) ? 1 : 0;
            if (pre_lu && !ea_lu) {
                if (S.sym_mode) hipLaunchKernelGGL(k_diag0<true>, dim3(st.nactive), dim3(64), 0, STREAM, lfd, d_pool, d_lperm, d_dws, d_scalar, opt.pivot_epsilon, d_info, d_diag);
                else hipLaunchKernelGGL((PZ ? k_diag0<false, true> : k_diag0<false, false>), dim3(st.nactive), dim3(64), 0, STREAM, lfd, d_pool, d_lperm, d_dws, d_scalar, opt.pivot_epsilon, d_info, d_diag);
                launches++;
            }
            if (S.sym_mode) {
                hipLaunchKernelGGL(k_panel<true>, dim3(st.n_panel), dim3(PANEL_T), 0, STREAM, d_tasks + st.pfx_panel, st.nactive, lfd, k0,
                                   d_pool, d_lperm, d_dws, dws_stride, d_scalar, opt.pivot_epsilon, d_info, d_diag, pre_lu, Pfx4{st.ppfx[0], st.ppfx[1], st.ppfx[2]});
                if (st.n_update > 0 && L.upd_ts == UPD_T)
                    hipLaunchKernelGGL(k_update<true>, dim3(st.n_update), dim3(256), 0, STREAM, d_tasks + st.pfx_update, st.nactive, lfd, k0,
                                       d_pool, d_dws, dws_stride, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag, 0, Pfx4{st.upfx[0], st.upfx[1], st.upfx[2]}, st.nfollow);
                else if (st.n_update > 0)
                    hipLaunchKernelGGL(k_update32<true>, dim3(st.n_update), dim3(64), 0, STREAM, d_tasks + st.pfx_update, st.nactive, lfd, k0,
                                       d_pool, d_dws, dws_stride, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag, Pfx4{st.upfx[0], st.upfx[1], st.upfx[2]}, st.nfollow);
            } else if (use_binv) {
                // one launch per step: every tile forms its own rows of W = A inv(D) (kernels_factor_binv.hpp)
                if (k0 == 0) {
                    hipLaunchKernelGGL(k_dinv0, dim3(st.nactive), dim3(64), 0, STREAM, lfd, d_pool, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag);
                    launches++;
                }
                if (L.upd_ts == UPD_T)
                    hipLaunchKernelGGL(k_bstep, dim3(st.n_update), dim3(256), 0, STREAM, d_tasks + st.pfx_update, st.nactive, lfd, k0, d_pool, d_lperm,
                                       d_scalar, opt.pivot_epsilon, d_info, d_diag);
                else
                    hipLaunchKernelGGL(k_bstep32, dim3(st.n_update), dim3(64), 0, STREAM, d_tasks + st.pfx_update, st.nactive, lfd, k0, d_pool, d_lperm,
                                       d_scalar, opt.pivot_epsilon, d_info, d_diag);
                launches--;
            } else {
                hipLaunchKernelGGL((PZ ? k_panel<false, true> : k_panel<false, false>), dim3(st.n_panel), dim3(PANEL_T), 0, STREAM, d_tasks + st.pfx_panel, st.nactive, lfd, k0,
                                   d_pool, d_lperm, d_dws, dws_stride, d_scalar, opt.pivot_epsilon, d_info, d_diag, pre_lu, Pfx4{st.ppfx[0], st.ppfx[1], st.ppfx[2]});
                if (L.upd_ts == UPD_T && st.split && st.n_rest > 0) {
                    // the bulk of the previous split step must be through before anything touches its tiles again
                    if (rest_pending) HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_rest, 0), ERROR_HIP_SYNCHRONIZE);
                    HIPC(hipEventRecord((hipEvent_t)ev_pb, STREAM), ERROR_HIP_SYNCHRONIZE);
                    HIPC(hipStreamWaitEvent((hipStream_t)stream4, (hipEvent_t)ev_pb, 0), ERROR_HIP_SYNCHRONIZE);
                    hipLaunchKernelGGL((PZ ? k_update<false, true> : k_update<false, false>), dim3(st.n_crit), dim3(256), 0, STREAM, d_tasks + st.pfx_crit, st.nactive, lfd, k0, d_pool, d_dws,
                                       dws_stride, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag, 1, Pfx4{-1, -1, -1}, st.nfollow);
                    hipLaunchKernelGGL((PZ ? k_update<false, true> : k_update<false, false>), dim3(st.n_rest), dim3(256), 0, (hipStream_t)stream4, d_tasks + st.pfx_rest, st.nactive, lfd, k0,
                                       d_pool, d_dws, dws_stride, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag, 2, Pfx4{-1, -1, -1}, 0);
                    HIPC(hipEventRecord((hipEvent_t)ev_rest, (hipStream_t)stream4), ERROR_HIP_SYNCHRONIZE);
                    rest_pending = true;
                    launches++;
                } else if (L.upd_ts == UPD_T) {
                    // (an unsplit update may touch any tile: the bulk of a split step before it has to be through)
                    if (rest_pending && !st.all_narrow) {
                        HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_rest, 0), ERROR_HIP_SYNCHRONIZE);
                        rest_pending = false;
                    }
                    hipLaunchKernelGGL((PZ ? k_update<false, true> : k_update<false, false>), dim3(st.n_update), dim3(256), 0, STREAM, d_tasks + st.pfx_update, st.nactive, lfd, k0,
                                       d_pool, d_dws, dws_stride, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag, upd_xcd ? 4 : 0, Pfx4{st.upfx[0], st.upfx[1], st.upfx[2]}, st.nfollow);
                } else
                    hipLaunchKernelGGL((PZ ? k_update32<false, true> : k_update32<false, false>), dim3(st.n_update), dim3(64), 0, STREAM, d_tasks + st.pfx_update, st.nactive, lfd, k0,
                                       d_pool, d_dws, dws_stride, d_lperm, d_scalar, opt.pivot_epsilon, d_info, d_diag, Pfx4{st.upfx[0], st.upfx[1], st.upfx[2]}, st.nfollow);
            }
            launches += 2;
            k0 += NB;
        }
        if (rest_pending) HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_rest, 0), ERROR_HIP_SYNCHRONIZE);
        if (use_binv && !S.sym_mode && L.n_flush > 0) {
            // E' above its diagonal blocks: A(:, k) -> A(:, k) inv(D_k) (kernels_factor_binv.hpp)
            hipLaunchKernelGGL(k_eflush, dim3(L.n_flush), dim3(64), 0, STREAM, d_tasks + L.pfx_flush, L.big_cnt, d_bigfd + L.bigfd_off, d_pool);
            launches++;
        }
        }
        if (L.mirror_cnt > 0) {
            hipLaunchKernelGGL(k_mirror_cb, dim3(L.mirror_cnt), dim3(256), 0, STREAM, d_lists + L.mirror_off, d_fd, d_pool);
            launches++;
        }
        if (mid_forked) HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_join3, 0), ERROR_HIP_SYNCHRONIZE);
        else if (forked) HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_join, 0), ERROR_HIP_SYNCHRONIZE);
    }
    if (pre_pending) HIPC(hipStreamWaitEvent(STREAM, (hipEvent_t)ev_pre1, 0), ERROR_HIP_SYNCHRONIZE);
    return SUCCESSFUL_EXIT;
    };
#ifndef HIPMF_EMULATED
    bool replayed = false;
    if (use_graph && !chained) {
        if (!factor_graph) {
            // capture (nothing runs), instantiate; any failure falls back to eager launches for good
            const int64_t before = launches;
            hipGraph_t g = nullptr;
            hipGraphExec_t ge = nullptr;
            bool ok = hipStreamBeginCapture(STREAM, hipStreamCaptureModeRelaxed) == hipSuccess;
            if (ok) {
                const int32_t ccode = enqueue_levels();
                const bool ended = hipStreamEndCapture(STREAM, &g) == hipSuccess && g != nullptr;
                ok = ccode == SUCCESSFUL_EXIT && ended && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess && ge != nullptr;
                if (g) (void)hipGraphDestroy(g);
            }
            (void)hipGetLastError();
            if (ok) factor_graph.reset(ge), graph_launches = launches - before;
            else use_graph = false;
            launches = before;
        }
        if (factor_graph) {
            HIPC(hipGraphLaunch(factor_graph, STREAM), ERROR_HIP_LAUNCH);
            launches += graph_launches;
            replayed = true;
        }
    }
    if (!replayed)
#endif
    {
        const int32_t lcode = enqueue_levels();
        if (lcode != SUCCESSFUL_EXIT) return lcode;
    }
    HIPC(hipEventRecord((hipEvent_t)ev[2], STREAM), ERROR_HIP_SYNCHRONIZE);
    FactorInfo hinfo;
    int32_t chain_err = 0;
    HIPC(hipMemcpyAsync(&hinfo, d_info, sizeof(FactorInfo), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    if (chained) HIPC(hipMemcpyAsync(&chain_err, d_chain_cnt + (chain_words - 1), sizeof(int32_t), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    if (chain_err != 0) {
        // a hand-off inside a chained launch timed out (workgroups not dispatched in index order?): the factor is incomplete.  The scaled
        // values are still there: this handle goes back to one launch per step, for this factorisation and all later ones.
        use_chain = false;
        chain_fallbacks++;
        if (opt.verbose) fprintf(stderr, "hipmf: factorize: a hand-off of the chained tiled steps timed out; repeating with one launch per step\n");
        if (gate.owns_lock()) gate.unlock();
        return run_factor();
    }
    n_perturbed = hinfo.n_perturbed;
    n_zero_pivot = hinfo.n_zero_pivot;
    n_weak_diag = hinfo.n_weak_diag;
    if (sym_first_look) {
        sym_diag_looked = true;
        if (n_weak_diag > 0) {
            sym_weak_diag_seen = true;
            last_error = "symmetric (lower) matrix with a weak or zero diagonal factorised as L D L^T without interchanges: hand the values to initialize "
                         "or set HIPMF_OPTION_SYM_RECHECK for the matched LU path";
            if (opt.verbose) fprintf(stderr, "hipmf: factorize: WARNING: %d row(s) of the symmetric matrix have a weak diagonal; %s\n", n_weak_diag, last_error.c_str());
        }
        n_weak_diag = 0; // (the L D L^T plan is kept: no re-matching for this handle)
    }
    if (hinfo.n_nonfinite > 0) {
        last_error = "the matrix values contain NaN or Inf";
        factorized = false;
        return ERROR_HIPMF_INVALID_VALUE;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, (hipEvent_t)ev[0], (hipEvent_t)ev[1]);
    times.scale_assemble_ms = ms;
    (void)hipEventElapsedTime(&ms, (hipEvent_t)ev[1], (hipEvent_t)ev[2]);
    times.factor_ms = ms;
    times.acc_assemble_ms += times.scale_assemble_ms;
    times.acc_factor_ms += times.factor_ms;
    times.acc_factor_count++;
    times.n_kernel_launches_factor = launches;
    if (opt.verbose)
        fprintf(stderr, "hipmf: factorize: assemble %.3f ms, factor %.3f ms, %lld launches, %d pivot(s) perturbed\n",
                times.scale_assemble_ms, times.factor_ms, (long long)launches, n_perturbed);
    return SUCCESSFUL_EXIT;
}

int32_t Solver::run_triangular(double *xp, int32_t nk, double *wrk, int64_t xstr, int64_t wstr, void *lane_stream, int32_t *lane_sync, bool timed, int32_t lane_id, uint32_t gmask) {
    int64_t launches = 0;
    if (use_fused) {
        const int32_t ns = S.nsuper;
        const hipStream_t LST = (hipStream_t)lane_stream;
        int32_t *sync_f = lane_sync, *sync_b = lane_sync + SF_SYNC_HEADER + ns, *sync_err = lane_sync + 2 * (SF_SYNC_HEADER + ns);
        // block groups of a blocked launch (kernels_solve_fused.hpp, SfGroups): group g's counters at lane_sync + g * sync_stride
        const int64_t sync_stride = 2 * (int64_t)(SF_SYNC_HEADER + ns) + 1;
        const int32_t ngrp = nk > SF_KMAX ? (nk + SF_KMAX - 1) / SF_KMAX : 1;
        if (ngrp > SF_GMAX) return ERROR_HIPMF_INVALID_VALUE;
        // (the tagged single-column pass pair touches no completion counter: the wave-subtrees publish nothing, the tasks above poll data)
        const bool counters_unused = tree_active && nk == 1 && tag_active;
        if (!counters_unused) HIPC(hipMemsetAsync(lane_sync, 0, sizeof(int32_t) * 2 * (size_t)(SF_SYNC_HEADER + ns), LST), ERROR_HIP_MEMCPY);
        if (ngrp > 1) HIPC(hipMemsetAsync(lane_sync + sync_stride, 0, sizeof(int32_t) * (size_t)sync_stride * (size_t)(ngrp - 1), LST), ERROR_HIP_MEMCPY);
        if (timed) HIPC(hipEventRecord((hipEvent_t)ev[3], LST), ERROR_HIP_SYNCHRONIZE);
        const SfGroups one_group = {1, 0, 1, 1u, 0, 0};
        if (tree_active && nk == 1) {
            // (inside the timed pass pair: arming the tagged words is part of what a pass pair costs)
            // (round 6: k_wt_bwd, the last kernel of a pass pair, re-arms the words for the next one -- the memset is for the first pass
            //  pair of a workspace, and for whatever follows a pass that did not end with k_wt_bwd)
            if (tag_active && !(rearm_tags && tags_armed && wrk == d_work))
                HIPC(hipMemsetAsync(wrk + work_arm0, 0xFF, sizeof(double) * (size_t)(work_up - work_arm0 + S.n), LST), ERROR_HIP_MEMCPY);
            else if (d_rep)
                HIPC(hipMemsetAsync(d_rep + 2 * (size_t)rep_words * (size_t)lane_id, 0, sizeof(int32_t) * 2 * (size_t)rep_words, LST), ERROR_HIP_MEMCPY);
        }
        if (tree_active && nk == 1) {
            int32_t *const d_rep = this->d_rep ? this->d_rep + 2 * (size_t)rep_words * (size_t)lane_id : nullptr; // this lane's replicas
            // data-tagged hand-offs (kernels_solve_fused.hpp, sf_tag_wait): the words the tasks above the wave-subtrees hand to each other --
            // the vectors of those fronts in `wrk` and the shadow copy xt of x behind them -- hold the tag when the launches start
            const bool tag = tag_active;
            double *const xt = wrk + work_up;
            // one wavefront per subtree of small fronts at the bottom (k_wt_fwd / k_wt_bwd), LDS-staged dependency-driven tasks above
            const int32_t wg = (wt_waves + WT_WAVES - 1) / WT_WAVES;
            const size_t dyn = sizeof(double) * 256 * (size_t)up_stage;
            unsigned long long *no_tr = (timed && d_trace) ? d_trace.get() : nullptr;
            const int32_t *const no_rep_idx = nullptr;
            int *const no_rep = nullptr;
            if (wg > 0)
                hipLaunchKernelGGL(k_wt_fwd, dim3(wg), dim3(64 * WT_WAVES), 0, LST, d_wt_wave, d_wt_hdr, d_wt_meta, d_pool, d_lperm, sync_f, wrk, xp, tag ? 0 : 1);
            // the fronts above the wave-subtrees: the many mid-level tasks at full occupancy, then the top levels (a chain of
            // hand-offs between few, large fronts) with their shares of E / E' parked in LDS before the wait
            const int32_t f_mid = sf2_fwd_mid, f_top = sf2_fwd_cnt - sf2_fwd_mid, b_top = sf2_bwd_top, b_mid = sf2_bwd_cnt - sf2_bwd_top;
#define HIPMF_TREE_FWD(STGV, TAGV, CNT, DYN, TASKS, TRACE, STAGE, RIDX, REP)                                                                  \
    hipLaunchKernelGGL((k_fwd_fused<false, 1, STGV, TAGV>), dim3(CNT), dim3(256), DYN, LST, TASKS, d_fd, d_pool, d_lperm, d_child, d_rel, d_need2, \
                       sync_f, sync_err, wrk, xp, 1, xstr, wstr, TRACE, STAGE, RIDX, REP, one_group)
#define HIPMF_TREE_BWD(SYMV, STGV, TAGV, CNT, DYN, TASKS, TRACE, STAGE, RIDX, REP)                                                            \
    hipLaunchKernelGGL((k_bwd_fused<false, 1, SYMV, STGV, TAGV>), dim3(CNT), dim3(256), DYN, LST, TASKS, d_fd, d_pool, d_rows, d_need2 + ns,   \
                       sync_b, sync_err, wrk, xp, 1, xstr, wstr, TRACE, d_diag, STAGE, RIDX, REP, TAGV ? xt : (double *)nullptr, (double *)nullptr, (int *)nullptr, one_group)
            unsigned long long *tr_top = no_tr ? no_tr + 8 * (size_t)f_mid : no_tr;
            if (f_mid > 0) {
                if (tag) HIPMF_TREE_FWD(false, true, f_mid, 0, d_sf2, no_tr, 0, no_rep_idx, no_rep);
                else HIPMF_TREE_FWD(false, false, f_mid, 0, d_sf2, no_tr, 0, no_rep_idx, no_rep);
            }
            if (f_top > 0) {
                if (tag) HIPMF_TREE_FWD(true, true, f_top, dyn, d_sf2 + f_mid, tr_top, up_stage, no_rep_idx, no_rep);
                else HIPMF_TREE_FWD(true, false, f_top, dyn, d_sf2 + f_mid, tr_top, up_stage, (const int32_t *)d_rep_idx, d_rep);
            }
            if (timed) HIPC(hipEventRecord((hipEvent_t)ev[4], LST), ERROR_HIP_SYNCHRONIZE);
            {
                const SfTask *tb = d_sf2 + sf2_fwd_cnt;
                unsigned long long *tr_b = no_tr ? no_tr + 8 * (size_t)sf2_fwd_cnt : nullptr;
                unsigned long long *tr_bm = tr_b ? tr_b + 8 * (size_t)b_top : tr_b;
                const size_t dyn_b = sizeof(double) * 256 * (size_t)up_stage_bwd, dyn_m = sizeof(double) * 256 * (size_t)up_stage_mid;
                if (S.sym_mode) {
                    if (sf2_bwd_cnt > 0) {
                        if (tag) HIPMF_TREE_BWD(true, false, true, sf2_bwd_cnt, 0, tb, tr_b, 0, no_rep_idx, no_rep);
                        else HIPMF_TREE_BWD(true, false, false, sf2_bwd_cnt, 0, tb, tr_b, 0, no_rep_idx, no_rep);
                    }
                } else {
                    if (b_top > 0) {
                        if (tag) HIPMF_TREE_BWD(false, true, true, b_top, dyn_b, tb, tr_b, up_stage_bwd, no_rep_idx, no_rep);
                        else HIPMF_TREE_BWD(false, true, false, b_top, dyn_b, tb, tr_b, up_stage_bwd, (const int32_t *)d_rep_idx, d_rep ? d_rep + rep_words : d_rep);
                    }
                    if (b_mid > 0 && up_stage_mid > 0) { // (the backward slabs have no register prefetch of E': a small parked share pays)
                        if (tag) HIPMF_TREE_BWD(false, true, true, b_mid, dyn_m, tb + b_top, tr_bm, up_stage_mid, no_rep_idx, no_rep);
                        else HIPMF_TREE_BWD(false, true, false, b_mid, dyn_m, tb + b_top, tr_bm, up_stage_mid, no_rep_idx, no_rep);
                    } else if (b_mid > 0) {
                        if (tag) HIPMF_TREE_BWD(false, false, true, b_mid, 0, tb + b_top, tr_bm, 0, no_rep_idx, no_rep);
                        else HIPMF_TREE_BWD(false, false, false, b_mid, 0, tb + b_top, tr_bm, 0, no_rep_idx, no_rep);
                    }
                }
            }
#undef HIPMF_TREE_FWD
#undef HIPMF_TREE_BWD
            const bool rearm = tag && rearm_tags && wg > 0 && wrk == d_work;
            if (wg > 0)
                hipLaunchKernelGGL(k_wt_bwd, dim3(wg), dim3(64 * WT_WAVES), 0, LST, d_wt_wave + (size_t)wg * WT_WAVES, d_wt_hdr + wt_hdr_fwd,
                                   d_wt_meta + wt_meta_fwd, d_pool, xp, rearm ? wrk + work_arm0 : (double *)nullptr,
                                   (long long)(work_up - work_arm0 + S.n));
            tags_armed = rearm;
            if (timed) HIPC(hipEventRecord((hipEvent_t)ev[5], LST), ERROR_HIP_SYNCHRONIZE);
            times.n_kernel_launches_solve = 2 * (wg > 0) + (f_mid > 0) + (f_top > 0) + (S.sym_mode ? (sf2_bwd_cnt > 0) : (b_top > 0) + (b_mid > 0));
            if (timed) tri_pending = true;
            return SUCCESSFUL_EXIT;
        }
        const bool use_k = nk > 1 && d_sfk != nullptr; // the blocked instances have their own task list (no leaves; optionally wider slabs)
        const bool leaves = use_k && leaf_cnt > 0;
        const int32_t leaf_wgs = (leaf_cnt + LEAF_WAVES * LEAF_PER_WAVE - 1) / (LEAF_WAVES * LEAF_PER_WAVE);
        if (ngrp > 1 && (!use_k || (split_units > 0 && ngrp > block_groups_plan))) return ERROR_HIPMF_INVALID_VALUE; // (solve() sizes its blocks by block_groups_plan)
        if (leaves) // the leaves first: nothing in them waits for anything (their parents are tasks of the launches below)
            hipLaunchKernelGGL(k_leaf_fwd, dim3(leaf_wgs, ngrp), dim3(64 * LEAF_WAVES), 0, LST, d_leaf, leaf_cnt, d_pool, d_lperm, xp, xstr, wrk, wstr, sync_f, nk, gmask);
        const SfTask *T = use_k ? d_sfk : d_sf;
        const int32_t *NEED = use_k ? d_needk : d_need;
        const int32_t t_fwd = use_k ? sfk_fwd_cnt : sf_fwd_cnt;
        const int32_t fa = use_k ? sfk_fwd_band : std::min(sf_fwd_band, sf_fwd_launch), fb = (use_k ? sfk_fwd_cnt : sf_fwd_launch) - fa;
        const int32_t bt = use_k ? sfk_bwd_top : sf_bwd_top, bb = (use_k ? sfk_bwd_cnt : sf_bwd_cnt) - bt;
        unsigned long long *no_trace = nullptr;
        // (ngrp > 1: the grid holds every task once per group, padded to whole sets of 8 ngrp workgroups -- see sf_group_of)
        auto groups_of = [&](int32_t cnt) { return SfGroups{ngrp, cnt, nk, gmask, sync_stride, split_units}; };
        auto grid_of = [&](int32_t cnt) { return ngrp > 1 ? (unsigned)(((cnt + 7) / 8) * 8 * ngrp) : (unsigned)cnt; };
#define HIPMF_FWD(SMALL, KK, CNT, TASKS, TRACE)                                                                                            \
    hipLaunchKernelGGL((k_fwd_fused<SMALL, KK>), dim3(grid_of(CNT)), dim3(256), 0, LST, TASKS, d_fd, d_pool, d_lperm, d_child, d_rel, NEED, sync_f, \
                       sync_err, wrk, xp, nk, xstr, wstr, TRACE, 0, (const int32_t *)nullptr, (int *)nullptr, groups_of(CNT))
#define HIPMF_BWD1(SMALL, KK, SYMM, CNT, TASKS, TRACE)                                                                                     \
    hipLaunchKernelGGL((k_bwd_fused<SMALL, KK, SYMM>), dim3(grid_of(CNT)), dim3(256), 0, LST, TASKS, d_fd, d_pool, d_rows, NEED + ns, sync_b,        \
                       sync_err, wrk, xp, nk, xstr, wstr, TRACE, d_diag, 0, (const int32_t *)nullptr, (int *)nullptr, (double *)nullptr, d_split_scr, d_split_cnt, groups_of(CNT))
#define HIPMF_BWD(SMALL, KK, CNT, TASKS, TRACE)                                                                                            \
    do {                                                                                                                                  \
        if (!SMALL && S.sym_mode) HIPMF_BWD1(false, KK, true, CNT, TASKS, TRACE);                                                          \
        else HIPMF_BWD1(SMALL, KK, false, CNT, TASKS, TRACE);                                                                              \
    } while (0)
        // (round 6, blocked instances: the all-small band as one PLAIN launch per level -- ordinary loads and stores, no counters)
        const bool band_plain = use_k && plain_band && (int32_t)sfk_band_f.size() >= 2 && sfk_band_f.back() == fa;
#define HIPMF_FWD_PLAIN(KK)                                                                                                                \
    for (size_t li = 0; li + 1 < sfk_band_f.size(); li++) {                                                                               \
        const int32_t c0 = sfk_band_f[li], cn = sfk_band_f[li + 1] - c0;                                                                  \
        if (cn > 0)                                                                                                                       \
            hipLaunchKernelGGL((k_fwd_fused<true, KK, false, false, true>), dim3(grid_of(cn)), dim3(256), 0, LST, T + c0, d_fd, d_pool, d_lperm, d_child, \
                               d_rel, NEED, sync_f, sync_err, wrk, xp, nk, xstr, wstr, no_trace, 0, (const int32_t *)nullptr, (int *)nullptr, groups_of(cn)); \
    }
        if (nk == 1) {
            if (fa > 0) HIPMF_FWD(true, 1, fa, T, no_trace);
            if (fb > 0) HIPMF_FWD(false, 1, fb, T + fa, timed ? d_trace : no_trace);
        } else if (nk <= SF_KMID) {
            if (band_plain) {
                HIPMF_FWD_PLAIN(SF_KMID)
            } else if (fa > 0)
                HIPMF_FWD(true, SF_KMID, fa, T, no_trace);
            if (fb > 0) HIPMF_FWD(false, SF_KMID, fb, T + fa, timed ? d_trace : no_trace);
        } else {
            if (band_plain) {
                HIPMF_FWD_PLAIN(SF_KMAX)
            } else if (fa > 0)
                HIPMF_FWD(true, SF_KMAX, fa, T, no_trace);
            if (fb > 0) HIPMF_FWD(false, SF_KMAX, fb, T + fa, timed ? d_trace : no_trace);
        }
#undef HIPMF_FWD_PLAIN
        if (timed) HIPC(hipEventRecord((hipEvent_t)ev[4], LST), ERROR_HIP_SYNCHRONIZE);
#define HIPMF_BWD_PLAIN(KK)                                                                                                                \
    for (size_t li = 0; li + 1 < sfk_band_b.size(); li++) {                                                                               \
        const int32_t c0 = sfk_band_b[li], cn = sfk_band_b[li + 1] - c0;                                                                  \
        if (cn > 0)                                                                                                                       \
            hipLaunchKernelGGL((k_bwd_fused<true, KK, false, false, false, true>), dim3(grid_of(cn)), dim3(256), 0, LST, T + t_fwd + c0, d_fd, d_pool, \
                               d_rows, NEED + ns, sync_b, sync_err, wrk, xp, nk, xstr, wstr, no_trace, d_diag, 0, (const int32_t *)nullptr, (int *)nullptr, \
                               (double *)nullptr, (double *)nullptr, (int *)nullptr, groups_of(cn));                                       \
    }
        if (nk == 1) {
            if (bt > 0) HIPMF_BWD(false, 1, bt, T + t_fwd, (timed && d_trace) ? d_trace + 8 * (size_t)fb : nullptr);
            if (bb > 0) HIPMF_BWD(true, 1, bb, T + t_fwd + bt, no_trace);
        } else if (nk <= SF_KMID) {
            if (bt > 0) HIPMF_BWD(false, SF_KMID, bt, T + t_fwd, (timed && d_trace) ? d_trace + 8 * (size_t)fb : nullptr);
            if (band_plain) {
                HIPMF_BWD_PLAIN(SF_KMID)
            } else if (bb > 0)
                HIPMF_BWD(true, SF_KMID, bb, T + t_fwd + bt, no_trace);
        } else {
            if (bt > 0) HIPMF_BWD(false, SF_KMAX, bt, T + t_fwd, (timed && d_trace) ? d_trace + 8 * (size_t)fb : nullptr);
            if (band_plain) {
                HIPMF_BWD_PLAIN(SF_KMAX)
            } else if (bb > 0)
                HIPMF_BWD(true, SF_KMAX, bb, T + t_fwd + bt, no_trace);
        }
#undef HIPMF_BWD_PLAIN
#undef HIPMF_FWD
#undef HIPMF_BWD
#undef HIPMF_BWD1
        if (leaves) // ... and last: every ancestor of a leaf is complete
            hipLaunchKernelGGL(k_leaf_bwd, dim3(leaf_wgs, ngrp), dim3(64 * LEAF_WAVES), 0, LST, d_leaf + leaf_cnt, leaf_cnt, d_pool, d_rows, xp, xstr, nk, gmask);
        if (timed) HIPC(hipEventRecord((hipEvent_t)ev[5], LST), ERROR_HIP_SYNCHRONIZE);
        times.n_kernel_launches_solve = (fa > 0) + (fb > 0) + (bt > 0) + (bb > 0) + 2 * (leaves ? 1 : 0);
        if (timed) tri_pending = true;
        return SUCCESSFUL_EXIT;
    }
    if (nk != 1 || wrk != d_work) return ERROR_HIPMF_INVALID_VALUE; // the level-set launches carry one right-hand side
    if (!level_path_ok) {
        // L D L^T fronts / fronts beyond the LDS staging of the level-set kernels: the dependency-driven kernels, ONE LAUNCH PER LEVEL.
        // A task then only depends on tasks of earlier launches (the list carries no assemble-once tasks): the in-launch hand-offs,
        // and with them the reliance on the order in which the hardware places workgroups, are gone; same arithmetic.
        int32_t code = build_level_tasks();
        if (code != SUCCESSFUL_EXIT) return code;
        const int32_t ns = S.nsuper;
        int32_t *sync_f = lane_sync, *sync_b = lane_sync + SF_SYNC_HEADER + ns, *sync_err = lane_sync + 2 * (SF_SYNC_HEADER + ns);
        HIPC(hipMemsetAsync(lane_sync, 0, sizeof(int32_t) * 2 * (size_t)(SF_SYNC_HEADER + ns), STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipEventRecord((hipEvent_t)ev[3], STREAM), ERROR_HIP_SYNCHRONIZE);
        unsigned long long *no_tr = nullptr;
        for (int32_t l = 0; l < S.nlevels; l++) {
            const int32_t t0 = sf3_lvl[(size_t)l], cnt = sf3_lvl[(size_t)l + 1] - t0;
            if (cnt <= 0) continue;
            hipLaunchKernelGGL((k_fwd_fused<false, 1, false>), dim3(cnt), dim3(256), 0, STREAM, d_sf3 + t0, d_fd, d_pool, d_lperm, d_child, d_rel, d_need3,
                               sync_f, sync_err, wrk, xp, 1, xstr, wstr, no_tr, 0, (const int32_t *)nullptr, (int *)nullptr, SfGroups{1, 0, 1, 1u, 0, 0});
            launches++;
        }
        HIPC(hipEventRecord((hipEvent_t)ev[4], STREAM), ERROR_HIP_SYNCHRONIZE);
        const int32_t nb0 = sf3_lvl[(size_t)S.nlevels];
        for (int32_t l = S.nlevels - 1; l >= 0; l--) {
            const int32_t t0 = nb0 + sf3_lvl_b[(size_t)(S.nlevels - 1 - l)], cnt = sf3_lvl_b[(size_t)(S.nlevels - l)] - sf3_lvl_b[(size_t)(S.nlevels - 1 - l)];
            if (cnt <= 0) continue;
            if (S.sym_mode)
                hipLaunchKernelGGL((k_bwd_fused<false, 1, true, false>), dim3(cnt), dim3(256), 0, STREAM, d_sf3 + t0, d_fd, d_pool, d_rows, d_need3 + ns,
                                   sync_b, sync_err, wrk, xp, 1, xstr, wstr, no_tr, d_diag, 0, (const int32_t *)nullptr, (int *)nullptr, (double *)nullptr, (double *)nullptr, (int *)nullptr, SfGroups{1, 0, 1, 1u, 0, 0});
            else
                hipLaunchKernelGGL((k_bwd_fused<false, 1, false, false>), dim3(cnt), dim3(256), 0, STREAM, d_sf3 + t0, d_fd, d_pool, d_rows, d_need3 + ns,
                                   sync_b, sync_err, wrk, xp, 1, xstr, wstr, no_tr, d_diag, 0, (const int32_t *)nullptr, (int *)nullptr, (double *)nullptr, (double *)nullptr, (int *)nullptr, SfGroups{1, 0, 1, 1u, 0, 0});
            launches++;
        }
        HIPC(hipEventRecord((hipEvent_t)ev[5], STREAM), ERROR_HIP_SYNCHRONIZE);
        times.n_kernel_launches_solve = launches;
        tri_pending = true;
        return SUCCESSFUL_EXIT;
    }
    HIPC(hipEventRecord((hipEvent_t)ev[3], STREAM), ERROR_HIP_SYNCHRONIZE);
    for (const LevelPlan &L : levels) {
        if (L.small_cnt > 0) {
            hipLaunchKernelGGL(k_fwd, dim3(L.small_cnt), dim3(64), sizeof(double) * (size_t)L.small_ld * (size_t)L.small_pmax, STREAM,
                               d_lists + L.small_off, d_fd, d_pool, d_lperm, d_child, d_rel, d_work, xp, L.small_ld);
            launches++;
        }
        if (L.fwd_cnt > 0) {
            if (L.wide)
                hipLaunchKernelGGL((k_fwd_big<SOLVE_SLAB_WIDE, 32>), dim3(L.fwd_cnt), dim3(SOLVE_SLAB_WIDE * 32), sizeof(double) * (size_t)L.big_pmax,
                                   STREAM, d_st + L.fwd_off, d_fd, d_pool, d_child, d_rel, d_work, xp);
            else
                hipLaunchKernelGGL((k_fwd_big<SOLVE_SLAB, 4>), dim3(L.fwd_cnt), dim3(SOLVE_SLAB * 4), sizeof(double) * (size_t)L.big_pmax, STREAM,
                                   d_st + L.fwd_off, d_fd, d_pool, d_child, d_rel, d_work, xp);
            launches++;
        }
    }
    HIPC(hipEventRecord((hipEvent_t)ev[4], STREAM), ERROR_HIP_SYNCHRONIZE);
    for (auto it = levels.rbegin(); it != levels.rend(); ++it) {
        const LevelPlan &L = *it;
        if (L.bwd_cnt > 0) {
            if (L.wide)
                hipLaunchKernelGGL((k_bwd_big<SOLVE_SLAB_WIDE, 32>), dim3(L.bwd_cnt), dim3(SOLVE_SLAB_WIDE * 32), sizeof(double) * (size_t)L.big_fmax,
                                   STREAM, d_st + L.bwd_off, d_fd, d_pool, d_rows, d_work, xp);
            else
                hipLaunchKernelGGL((k_bwd_big<SOLVE_SLAB, 4>), dim3(L.bwd_cnt), dim3(SOLVE_SLAB * 4), sizeof(double) * (size_t)L.big_fmax, STREAM,
                                   d_st + L.bwd_off, d_fd, d_pool, d_rows, d_work, xp);
            launches++;
        }
        if (L.small_cnt > 0) {
            hipLaunchKernelGGL(k_bwd, dim3(L.small_cnt), dim3(64), sizeof(double) * (size_t)L.small_ld * (size_t)L.small_pmax, STREAM,
                               d_lists + L.small_off, d_fd, d_pool, d_rows, d_work, xp, L.small_ld);
            launches++;
        }
    }
    HIPC(hipEventRecord((hipEvent_t)ev[5], STREAM), ERROR_HIP_SYNCHRONIZE);
    times.n_kernel_launches_solve = launches;
    tri_pending = true;
    return SUCCESSFUL_EXIT;
}

// Task list of the level-by-level launches of the dependency-driven kernels (built at the first solve that needs it): the tasks of
// level l are sf3[sf3_lvl[l], sf3_lvl[l + 1]) in the forward part, the backward part follows with the levels from the root down.
int32_t Solver::build_level_tasks() {
    if (d_sf3) return SUCCESSFUL_EXIT;
    const int32_t ns = S.nsuper;
    std::vector<SfTask> sf;
    std::vector<int32_t> need((size_t)2 * ns, 1);
    auto kind_of = [&](int32_t s, bool forward) {
        const int32_t len = forward ? S.npiv(s) : S.fsize(s);
        if (!forward && S.sym_mode) return 4; // transposed GEMV of the L D L^T fronts: 16 columns of E per workgroup
        if (forward && sf_big_rows > 0 && S.fsize(s) >= sf_big_front) return sf_big_rows;
        return slab64 ? 6 : (len >= 512 ? 4 : (len >= 128 ? 5 : (len > 32 ? 6 : 7)));
    };
    auto emit_level = [&](int32_t l, bool forward) {
        std::vector<int32_t> small;
        for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
            const int32_t s = S.level_sn[k];
            if (S.fsize(s) <= SMALL_F) {
                small.push_back(s);
                continue;
            }
            const int32_t kind = kind_of(s, forward), rows = 1 << kind, ext = forward ? S.fsize(s) : S.npiv(s);
            need[(size_t)(forward ? 0 : ns) + s] = (ext + rows - 1) / rows;
            for (int32_t r0 = 0; r0 < ext; r0 += rows) sf.push_back({kind, s, r0, std::min(ext, r0 + rows), 0, 0});
        }
        for (size_t k = 0; k < small.size(); k += 4) {
            SfTask t = {0, small[k], -1, -1, -1, 0};
            if (k + 1 < small.size()) t.b = small[k + 1];
            if (k + 2 < small.size()) t.c = small[k + 2];
            if (k + 3 < small.size()) t.d = small[k + 3];
            sf.push_back(t);
        }
    };
    sf3_lvl.assign(1, 0);
    for (int32_t l = 0; l < S.nlevels; l++) emit_level(l, true), sf3_lvl.push_back((int32_t)sf.size());
    const int32_t nf = (int32_t)sf.size();
    sf3_lvl_b.assign(1, 0);
    for (int32_t l = S.nlevels - 1; l >= 0; l--) emit_level(l, false), sf3_lvl_b.push_back((int32_t)sf.size() - nf);
    HIPC(d_sf3.upload(sf), ERROR_HIP_MALLOC);
    HIPC(d_need3.upload(need), ERROR_HIP_MALLOC);
    return SUCCESSFUL_EXIT;
}

// reads the forward/backward event pair of the last triangular pass (call after a stream sync)
void Solver::harvest_tri() {
    if (!tri_pending) return;
    tri_pending = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, (hipEvent_t)ev[3], (hipEvent_t)ev[4]) != hipSuccess) return;
    times.fwd_ms = ms;
    times.acc_fwd_ms += ms;
    if (hipEventElapsedTime(&ms, (hipEvent_t)ev[4], (hipEvent_t)ev[5]) != hipSuccess) return;
    times.bwd_ms = ms;
    times.acc_bwd_ms += ms;
    times.acc_tri_count++;
}

// One lane of the solve driver: a stream with its own block buffers and hand-off words.  A single right-hand side (or a single
// block) uses lane 0 = the solver's own stream and buffers; several blocks alternate between two lanes so that the
// latency-bound upper levels of one block's triangular passes overlap with the bandwidth-bound leaf band of the other's.
struct Solver::SolveLane {
    hipStream_t st = nullptr;
    double *XP = nullptr, *DU = nullptr, *RR = nullptr, *BB = nullptr, *XX = nullptr, *WRK = nullptr;
    int32_t *sync = nullptr;             // completion counters + error word of the dependency-driven kernels
    unsigned long long *norms = nullptr; // 2 words per column: |r|_inf bits, omega bits
    double *h_nrm = nullptr;             // pinned host copy of the norms (a pageable target would make the copy synchronous)
    bool timed = false;                  // records the forward / backward event pair (lane 0 only)
    int32_t id = 0;                      // index of the lane (its set of completion replicas)
    // the block in flight
    bool busy = false;
    int32_t j0 = 0, nk = 0, it = 0;
    int64_t cstr = 0; // stride between the block's columns of b and x
    double prev[SF_KMAX * SF_GMAX];
    bool active[SF_KMAX * SF_GMAX];
    const double *bj[SF_KMAX * SF_GMAX];
    double *xj[SF_KMAX * SF_GMAX];
};

// The buffers of a blocked solve of `nrhs` right-hand sides (six n x KS blocks, KS workspaces, norm slots, the pinned norm mirror) cost
// the FIRST solve_many of a handle a few tenths of a second at config 4's size (0.735 s against 0.34 s): this call allocates
// and touches them ahead of time -- any time after initialize, e.g. while another rank still factorises.  Same decisions as solve().
int32_t Solver::prepare_many(int32_t nrhs) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (nrhs < 2) return SUCCESSFUL_EXIT;
    static double dummy = 0.0;
    prepare_only = true;
    const int32_t code = solve_core(&dummy, &dummy, nrhs, S.n, true);
    prepare_only = false;
    return code;
}

// An exactly zero pivot under a STATIC pivot order means "singular, or the order was unlucky" (a dynamic-pivoting solver would have taken a
// row from further down); UMFPACK's status 1 means the former only (solver_umfpack.rs:492,624-630).  Round 6: the factorisation that
// met zero pivots (replaced like every other small pivot) is asked to solve ONE system with a pseudo-random right-hand side -- a generic
// vector has a component outside the range of a singular matrix, so its residual cannot be driven down, while for a non-singular matrix
// the refined + Krylov-rescued solve reaches rounding level.  A rare path (a handful of solves); HIPMF_KRYLOV=0 keeps the old verdict.
int32_t Solver::singular_verdict() {
    if (!krylov_enabled || in_rescue) return WARNING_SINGULAR_MATRIX;
    const int32_t n = S.n;
    std::vector<double> b((size_t)n), x((size_t)n, 0.0), ax((size_t)n);
    unsigned long long st = 0x9e3779b97f4a7c15ull;
    for (int32_t i = 0; i < n; i++) { // splitmix64 -> uniform in [-1, 1)
        unsigned long long z = (st += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull, z = (z ^ (z >> 27)) * 0x94d049bb133111ebull, z ^= z >> 31;
        b[(size_t)i] = (double)(long long)(z >> 11) / 4503599627370496.0 - 1.0;
    }
    const bool keep_verbose = opt.verbose;
    opt.verbose = false;
    int32_t code = solve(x.data(), b.data(), 1, n, false);
    if (code == SUCCESSFUL_EXIT) code = spmv(ax.data(), x.data(), 1.0, false);
    opt.verbose = keep_verbose;
    last_host_rhs = nullptr, last_host_x = nullptr; // (the probe's buffers are gone: nobody "comes back" with them)
    if (code != SUCCESSFUL_EXIT) return WARNING_SINGULAR_MATRIX;
    long double rr = 0.0L, bb = 0.0L;
    bool finite = true;
    for (int32_t i = 0; i < n; i++) {
        const double d = b[(size_t)i] - ax[(size_t)i];
        finite = finite && std::isfinite(d);
        rr += (long double)d * d, bb += (long double)b[(size_t)i] * b[(size_t)i];
    }
    const bool solved = finite && rr <= 1e-16L * bb; // |r|_2 <= 1e-8 |b|_2: far below what a singular matrix allows for a generic b
    if (opt.verbose)
        fprintf(stderr, "hipmf: factorize: %d exactly zero pivot(s) under the static order; probe solve |r|/|b| = %.2e -> %s\n", n_zero_pivot,
                (double)sqrtl(rr / (bb > 0.0L ? bb : 1.0L)), solved ? "not singular" : "singular");
    if (solved) {
        zero_pivots_absorbed += n_zero_pivot;
        return SUCCESSFUL_EXIT;
    }
    return WARNING_SINGULAR_MATRIX;
}

// ---- Krylov rescue (round 6) ----
// The pivot order is static: fill-reducing ordering + maximum-product matching, interchanges inside a pivot block only.  What that cannot
// fix -- a pivot block none of whose rows offers a usable pivot (UMFPACK would take a row from further down, interface_umfpack.c:167) --
// is factorised with the pivot replaced by +-eps max|a| (counted: n_perturbed).  The factors are then the exact LU of A + E with E of rank
// <= n_perturbed, but (A + E)^{-1} E is not small, so plain iterative refinement stalls or diverges (tools: the random +-1 family of
// tests/test_matrix_zoo_gpu.py: forward error 1e5).  (A + E)^{-1} A = I - (A + E)^{-1} E is the identity plus a matrix of that rank:
// GMRES with the factorisation as RIGHT preconditioner converges in about n_perturbed + 1 steps.  Flexible form (the directions
// z_k = M^{-1} v_k are kept, w_k = A z_k is formed with the true matrix): the near-singular solves with M only need to give USEFUL
// directions, not accurate ones.  Host-side vectors (a rare path: only after a factorisation that perturbed pivots, and only for columns
// whose refined solution is not accurate): M^{-1} v = one unrefined pass pair through the device kernels, A z = the device SpMV.
int32_t Solver::krylov_rescue(double *x, const double *rhs, bool on_device, const KrylovOps *ops) {
    const int32_t n = S.n;
    const size_t nb = sizeof(double) * (size_t)n;
    std::vector<double> xh((size_t)n), bh((size_t)n), r((size_t)n), w((size_t)n);
    if (on_device) {
        HIPC(hipMemcpy(xh.data(), x, nb, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
        HIPC(hipMemcpy(bh.data(), rhs, nb, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    } else {
        memcpy(xh.data(), x, nb), memcpy(bh.data(), rhs, nb);
    }
    auto nrm2 = [&](const std::vector<double> &v) {
        long double t = 0.0L;
        for (double e : v) t += (long double)e * e;
        return (double)sqrtl(t);
    };
    auto residual = [&]() -> int32_t { // r = b - A x
        int32_t c = ops ? ops->apply(w.data(), xh.data()) : spmv(w.data(), xh.data(), 1.0, false);
        if (c != SUCCESSFUL_EXIT) return c;
        for (int32_t i = 0; i < n; i++) r[(size_t)i] = bh[(size_t)i] - w[(size_t)i];
        return SUCCESSFUL_EXIT;
    };
    for (double e : xh)
        if (!std::isfinite(e)) { // (a refinement that blew up: start the Krylov iteration from zero)
            std::fill(xh.begin(), xh.end(), 0.0);
            break;
        }
    const double bnorm = std::max(nrm2(bh), 1e-300);
    int32_t code = residual();
    if (code != SUCCESSFUL_EXIT) return code;
    double rnorm = nrm2(r);
    krylov_last_relres = rnorm / bnorm;
    if (!(rnorm > krylov_tol * bnorm)) return SUCCESSFUL_EXIT; // the refined solution is fine
    const int32_t m = std::max(4, std::min(krylov_restart, n));
    const int32_t saved_nstep = opt.refinement_nstep;
    const bool saved_verbose = opt.verbose;
    opt.refinement_nstep = 0, opt.verbose = false;
    in_rescue = true;
    std::vector<std::vector<double>> V, Z;
    GivensLsq<double> lsq(m);
    std::vector<double> hcol((size_t)m), y((size_t)m);
    for (int32_t cycle = 0; cycle < krylov_cycles && code == SUCCESSFUL_EXIT; cycle++) {
        V.assign(1, r);
        Z.clear();
        for (double &e : V[0]) e /= rnorm;
        lsq.reset(rnorm);
        int32_t k = 0;
        for (; k < m; k++) {
            Z.emplace_back((size_t)n);
            code = ops ? ops->precond(Z[(size_t)k].data(), V[(size_t)k].data()) : solve_core(Z[(size_t)k].data(), V[(size_t)k].data(), 1, n, false); // z_k = M^{-1} v_k
            if (code != SUCCESSFUL_EXIT) break;
            bool finite = true;
            for (double e : Z[(size_t)k]) finite = finite && std::isfinite(e);
            if (!finite) { // (a direction the perturbed factor cannot give: leave the cycle with what there is)
                Z.pop_back();
                break;
            }
            code = ops ? ops->apply(w.data(), Z[(size_t)k].data()) : spmv(w.data(), Z[(size_t)k].data(), 1.0, false); // w = A z_k
            if (code != SUCCESSFUL_EXIT) break;
            krylov_iterations++;
            for (int32_t j = 0; j <= k; j++) { // modified Gram-Schmidt
                long double t = 0.0L;
                for (int32_t i = 0; i < n; i++) t += (long double)w[(size_t)i] * V[(size_t)j][(size_t)i];
                hcol[(size_t)j] = (double)t;
                for (int32_t i = 0; i < n; i++) w[(size_t)i] -= (double)t * V[(size_t)j][(size_t)i];
            }
            const double hn = nrm2(w);
            lsq.push(k, hcol.data(), hn);
            if (saved_verbose) fprintf(stderr, "hipmf: krylov rescue: cycle %d step %d: residual estimate %.3e (|b| = %.3e)\n", cycle, k + 1, fabs(lsq.g[(size_t)k + 1]), bnorm);
            if (fabs(lsq.g[(size_t)k + 1]) <= krylov_tol * bnorm || !(hn > 0.0)) {
                k++;
                break;
            }
            V.emplace_back(w);
            for (double &e : V.back()) e /= hn;
        }
        if (code != SUCCESSFUL_EXIT) break;
        const int32_t kk = std::min<int32_t>(k, (int32_t)Z.size());
        lsq.solve(kk, y.data()); // x += Z y
        for (int32_t j = 0; j < kk; j++)
            for (int32_t i = 0; i < n; i++) xh[(size_t)i] += y[(size_t)j] * Z[(size_t)j][(size_t)i];
        const double before = rnorm;
        code = residual();
        if (code != SUCCESSFUL_EXIT) break;
        rnorm = nrm2(r);
        if (saved_verbose) fprintf(stderr, "hipmf: krylov rescue: cycle %d: |r| %.3e -> %.3e\n", cycle, before, rnorm);
        if (!(rnorm > krylov_tol * bnorm) || !(rnorm < 0.5 * before) || kk == 0) break; // done, or no longer improving
    }
    in_rescue = false;
    opt.refinement_nstep = saved_nstep, opt.verbose = saved_verbose;
    if (code != SUCCESSFUL_EXIT) return code;
    krylov_last_relres = rnorm / bnorm;
    if (on_device) HIPC(hipMemcpy(x, xh.data(), nb, hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
    else memcpy(x, xh.data(), nb);
    return SUCCESSFUL_EXIT;
}

int32_t Solver::solve(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device) {
    const int32_t code = solve_core(x, rhs, nrhs, ldx, on_device);
    if (code != SUCCESSFUL_EXIT || prepare_only || in_rescue || !krylov_enabled || n_perturbed <= 0 || !factorized) return code;
    DeviceScope dev_scope(device);
    krylov_iterations = 0;
    for (int32_t j = 0; j < nrhs; j++) {
        // A column whose componentwise backward error the refinement brought to rounding level is DONE, whatever its residual is relative
        // to |b| (an ill-conditioned system: |A||x| >> |b|): a backward-stable solution is all a direct solver owes, and the rescue's
        // residual test would otherwise cost such columns dozens of extra solves after every factorisation that replaced a pivot.
        if ((size_t)j < col_omega.size() && col_omega[(size_t)j] <= krylov_omega_ok) continue;
        const int32_t c = krylov_rescue(x + (int64_t)j * ldx, rhs + (int64_t)j * ldx, on_device);
        if (c != SUCCESSFUL_EXIT) return c;
        // (a factorisation the rescue cannot repair -- e.g. a kept L D L^T plan on a saddle-point matrix, dozens of replaced pivots AND
        //  growth -- fails for every column alike: the other columns keep their refined solutions instead of paying 160 solves each)
        if (krylov_last_relres > 1e-6) break;
    }
    return SUCCESSFUL_EXIT;
}

int32_t Solver::solve_core(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device) {
    if (!factorized && !prepare_only) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs) return ERROR_NULL_POINTER;
    if (nrhs < 1 || ldx < S.n) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    // The device's gate (see device_gate) is held only while dependency-driven launches of this solve are in flight: from just before a
    // triangular pass pair is queued until the host has seen its stream drain (staging copies, the host's look at the norms
    // and the waits of a many-RHS loop between blocks are outside -- another handle's solve gets its turn there).  With several lanes
    // (opt-in) the gate stays held until every lane is idle.  The gate is process-wide: two PROCESSES sharing one GPU are not
    // serialised by it -- their waits stay bounded by the device-clock time-out and the level-set fallback.
    GateLock gate(device_gate(device), device);
    auto gate_acquire = [&]() {
        if (!use_fused || gate.owns_lock()) return;
        if (!gate.lock_counting()) gate_waits++;
    };
    const int32_t n = S.n;
    const dim3 g((n + 255) / 256), b(256);
    const double EPS = 2.220446049250313e-16;
    refinement_steps_done = 0;
    // (componentwise backward error of every column's final solution where the refinement measured it; infinity: not measured -- refinement
    //  switched off, or more steps asked for than a measurement follows)
    col_omega.assign((size_t)nrhs, opt.refinement_nstep > 0 ? 0.0 : INFINITY);
    // Blocks of KB right-hand sides go through the triangular solves together (the dependency-driven kernels read each
    // factor entry once per block); one right-hand side uses the single-column instances and buffers.
    // (blocks of 16 columns = one full MFMA tile per slab tile when there are enough of them and the block buffers fit; else 8)
    int32_t KB = (use_fused && nrhs > 1) ? (nrhs > SF_KMID + SF_KMID / 2 ? SF_KMAX : SF_KMID) : 1;
    // ... and GB such blocks ("groups") travel through ONE set of dependency-driven launches (kernels_solve_fused.hpp, SfGroups): KB * GB
    // columns are in flight together; the upper levels' chains of hand-offs of the groups overlap.  Sixteen-column blocks only.
    int32_t GB = (KB == SF_KMAX && d_sfk) ? std::max(1, std::min(block_groups_plan, (nrhs + SF_KMAX - 1) / SF_KMAX)) : 1;
    if (KB > 1 && block_cols >= KB && block_cols * block_groups >= KB * GB) KB = block_cols, GB = block_groups; // (the buffers exist and are wide enough: keep their shape)
    if (KB > 1 && block_cols > 0 && (block_cols < KB || block_cols * block_groups < KB * GB)) {
        // wider blocks than the buffers of an earlier call hold: let them go, they are allocated again below
        d_blk.reset(), d_work_blk.reset(), d_norms_blk.reset();
        extra_lanes.clear();
        block_cols = 0, block_groups = 0;
    }
    if (KB == SF_KMAX && !d_blk) {
        size_t free_b = 0, total_b = 0;
        auto need_b = [&](int32_t groups) {
            return 8.0 * ((double)n * 6 + (double)work_blk_doubles) * SF_KMAX * groups * std::max(1, std::min(solve_lanes, (nrhs + SF_KMAX * groups - 1) / (SF_KMAX * groups)));
        };
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            while (GB > 1 && need_b(GB) > 0.5 * (double)free_b) GB /= 2; // (groups are a speed-up for small factors: never at the price of half the free memory)
            if (need_b(1) > 0.9 * (double)free_b) KB = SF_KMID, GB = 1;
        }
    }
    if (const int v = Tunables::now(&Tunables::block_cols_ask); KB > 1 && block_cols == 0 && (v == SF_KMID || v == SF_KMAX)) KB = v;
    if (KB != SF_KMAX) GB = 1;
    if (KB > 1) block_cols = KB, block_groups = GB, block_groups_last = GB;
    const int32_t KS = KB * GB; // columns of a block of the driver below
    const int32_t nblocks = (nrhs + KS - 1) / KS;
    // (rounds 2 - 3: two blocks in flight hid the host round trips of the refinement behind the other block's kernels, worth 10 - 20 % while
    //  a pass lasted a millisecond.  With the kernels of round 4 one lane is as fast or faster and two concurrently resident
    //  dependency-driven launches time out every few runs: the default is one lane, HIPMF_SOLVE_LANES asks for more.)  When the factor is tens of gigabytes a pass lasts 0.1 s, the round trips vanish, and two
    // launches full of waiting workgroups only get in each other's way (200^3, 256 right-hand sides: 3.0 - 3.7 s on two lanes from run
    // to run, 3.3 s on one; each lane also holds its own block and workspace buffers, 25 GB there): one lane from 64 GB of factor on.
    const int32_t lanes_here = (solve_lanes_auto && 8.0 * (double)S.persist_doubles > 64e9) ? 1 : solve_lanes;
    const int32_t nlanes = KB > 1 ? std::max(1, std::min(lanes_here, nblocks)) : 1;
    const size_t sync_words = 2 * (size_t)(SF_SYNC_HEADER + S.nsuper) + 1; // (per group of a blocked launch; group 0's last word is the error word)
    const size_t lane_cols = (size_t)SF_KMAX * SF_GMAX;                      // columns a lane's norm buffers are sized for
    if (KB > 1 && !d_blk) {
        // xp | du | r | den | b | x: six n x KS blocks, plus KS solve workspaces (columns at the stride that leaves the tagged shadow out)
        HIPC(d_blk.alloc(6 * (size_t)n * KS), ERROR_HIP_MALLOC);
        HIPC(d_work_blk.alloc((size_t)std::max<int64_t>(work_blk_doubles, 1) * KS + 64), ERROR_HIP_MALLOC);
        HIPC(d_norms_blk.alloc((size_t)RES_NORM_WORDS * lane_cols), ERROR_HIP_MALLOC);
    }
    if (!h_nrm) HIPC(h_nrm.alloc(RES_NORM_WORDS * lane_cols * MAX_SOLVE_LANES), ERROR_HIP_MALLOC);
    while ((int32_t)extra_lanes.size() < nlanes - 1) {
        LaneBuffers &r = extra_lanes.emplace_back(); // (registered first: release() frees whatever a failed allocation leaves behind)
        HIPC(hipStreamCreate(r.stream.put()), ERROR_HIPMF_NO_DEVICE);
        HIPC(r.blk.alloc(6 * (size_t)n * KS), ERROR_HIP_MALLOC);
        HIPC(r.work.alloc((size_t)std::max<int64_t>(work_blk_doubles, 1) * KS + 64), ERROR_HIP_MALLOC);
        HIPC(r.sync.alloc(sync_words * SF_GMAX), ERROR_HIP_MALLOC);
        HIPC(hipMemset(r.sync, 0, sizeof(int32_t) * sync_words * SF_GMAX), ERROR_HIP_MALLOC);
        HIPC(r.norms.alloc((size_t)RES_NORM_WORDS * lane_cols), ERROR_HIP_MALLOC);
    }
    SolveLane lanes[MAX_SOLVE_LANES];
    {
        SolveLane &L = lanes[0];
        L.st = STREAM;
        L.XP = KB > 1 ? d_blk : d_xp, L.DU = KB > 1 ? d_blk + (size_t)n * KS : d_du, L.RR = KB > 1 ? d_blk + 2 * (size_t)n * KS : d_r;
        L.BB = KB > 1 ? d_blk + 4 * (size_t)n * KS : d_b, L.XX = KB > 1 ? d_blk + 5 * (size_t)n * KS : d_x, L.WRK = KB > 1 ? d_work_blk : d_work;
        L.sync = d_sync, L.norms = KB > 1 ? d_norms_blk : d_scalar + 4, L.h_nrm = h_nrm, L.timed = true;
    }
    for (int32_t l = 1; l < nlanes; l++) {
        SolveLane &L = lanes[l];
        L.id = l;
        const LaneBuffers &r = extra_lanes[(size_t)l - 1];
        L.st = (hipStream_t)r.stream;
        L.XP = r.blk, L.DU = r.blk + (size_t)n * KS, L.RR = r.blk + 2 * (size_t)n * KS, L.BB = r.blk + 4 * (size_t)n * KS;
        L.XX = r.blk + 5 * (size_t)n * KS, L.WRK = r.work;
        L.sync = r.sync, L.norms = r.norms, L.h_nrm = h_nrm + (size_t)RES_NORM_WORDS * lane_cols * l, L.timed = false;
    }
    const int64_t wstr = KB > 1 ? work_blk_doubles : work_doubles;
    if (prepare_only) { // (prepare_many: the buffers exist now; first touch, then back)
        if (KB > 1) {
            HIPC(hipMemsetAsync(d_blk, 0, sizeof(double) * 6 * (size_t)n * KS, STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipMemsetAsync(d_work_blk, 0, sizeof(double) * ((size_t)std::max<int64_t>(work_blk_doubles, 1) * KS + 64), STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipMemsetAsync(d_norms_blk, 0, (size_t)RES_NORM_WORDS * lane_cols * sizeof(unsigned long long), STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipMemcpyAsync(h_nrm, d_norms_blk, (size_t)RES_NORM_WORDS * std::min<size_t>(lane_cols, (size_t)KS) * sizeof(double), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        }
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        return SUCCESSFUL_EXIT;
    }
    // One right-hand side handed over in pageable host memory goes through a pinned staging buffer: a pageable hipMemcpy of n
    // doubles from / into pages the runtime has not seen can cost 10 - 20 ms (measured in round 2: 22.8 ms per host solve of the 1M-DOF
    // system against 1.3 ms on the device; round 5, tools/microbench/host_copy_rates.py: 12 - 23 ms now and then for a fresh buffer, the
    // rate of pinned memory for one that was copied before).  A caller that comes back with the SAME two buffers as in its last call
    // (russell's solvers keep their vectors) is copied directly: 0.5 ms less per solve of the 1M-DOF system.
    const bool seen = !on_device && nrhs == 1 && rhs == last_host_rhs && x == last_host_x && host_direct;
    const bool staged = !on_device && nrhs == 1 && !seen;
    if (!on_device && nrhs == 1) last_host_rhs = rhs, last_host_x = x;
    if (staged) {
        if (!h_stage) HIPC(h_stage.alloc(2 * (size_t)n), ERROR_HIP_MALLOC);
        memcpy(h_stage, rhs, sizeof(double) * (size_t)n);
    }
    HIPC(hipEventRecord((hipEvent_t)ev[6], STREAM), ERROR_HIP_SYNCHRONIZE);
    if (nlanes > 1) {
        // the other lanes start after whatever the caller queued on the solver's stream (e.g. the factorisation)
        HIPC(hipEventRecord((hipEvent_t)ev_fork, STREAM), ERROR_HIP_SYNCHRONIZE);
        for (int32_t l = 1; l < nlanes; l++) HIPC(hipStreamWaitEvent(lanes[l].st, (hipEvent_t)ev_fork, 0), ERROR_HIP_SYNCHRONIZE);
    }

    // residual + norms of the active columns of the lane's block, and their way to the host
    auto enqueue_norms = [&](SolveLane &L) -> int32_t {
        HIPC(hipMemsetAsync(L.norms, 0, (size_t)RES_NORM_WORDS * L.nk * sizeof(unsigned long long), L.st), ERROR_HIP_MEMCPY);
        if (L.nk == 1) {
            if (L.active[0])
                hipLaunchKernelGGL(k_spmv_stream<true>, dim3(spmv_blocks), b, 0, L.st, d_row_blk, d_rp, d_ci, d_vals, d_tptr, d_tidx, d_arow, 1.0, L.xj[0], L.bj[0],
                                   L.RR, L.norms);
        } else {
            uint64_t amask = 0;
            for (int32_t c = 0; c < L.nk; c++)
                if (L.active[c]) amask |= 1ull << c;
            if (amask)
                hipLaunchKernelGGL(k_residual_cols, dim3(spmv_blocks), b, 0, L.st, d_row_blk, d_rp, d_ci, d_vals, d_tptr, d_tidx, d_arow, L.xj[0], L.cstr, L.bj[0],
                                   L.cstr, L.RR, (int64_t)n, L.norms, L.nk, amask);
        }
        HIPC(hipMemcpyAsync(L.h_nrm, L.norms, (size_t)RES_NORM_WORDS * L.nk * sizeof(double), hipMemcpyDeviceToHost, L.st), ERROR_HIP_MEMCPY);
        return SUCCESSFUL_EXIT;
    };
    auto finish = [&](SolveLane &L) -> int32_t {
        if (!on_device)
            for (int32_t c = 0; c < L.nk; c++)
                HIPC(hipMemcpyAsync(staged ? h_stage + n : x + (int64_t)(L.j0 + c) * ldx, L.XX + (size_t)c * n, sizeof(double) * n,
                                    hipMemcpyDeviceToHost, L.st),
                     ERROR_HIP_MEMCPY);
        L.busy = false;
        return SUCCESSFUL_EXIT;
    };
    // first solve of the block that starts at column j0
    auto start = [&](SolveLane &L, int32_t j0) -> int32_t {
        L.j0 = j0, L.nk = std::min(KS, nrhs - j0), L.it = 0, L.busy = true;
        for (int32_t c = 0; c < L.nk; c++) {
            if (on_device) {
                L.bj[c] = rhs + (int64_t)(j0 + c) * ldx;
                L.xj[c] = x + (int64_t)(j0 + c) * ldx;
            } else {
                HIPC(hipMemcpyAsync(L.BB + (size_t)c * n, staged ? h_stage : rhs + (int64_t)(j0 + c) * ldx, sizeof(double) * n,
                                    hipMemcpyHostToDevice, L.st),
                     ERROR_HIP_MEMCPY);
                L.bj[c] = L.BB + (size_t)c * n;
                L.xj[c] = L.XX + (size_t)c * n;
            }
            if (L.nk == 1) hipLaunchKernelGGL(k_perm_in, g, b, 0, L.st, n, d_rperm, d_rs, L.bj[c], L.XP + (size_t)c * n);
        }
        // (the columns of a block sit at a regular stride -- ldx on the device, n in the staging block: one launch for all of them)
        L.cstr = on_device ? ldx : (int64_t)n;
        const uint64_t all = L.nk >= 64 ? ~0ull : ((1ull << L.nk) - 1ull);
        if (L.nk > 1) hipLaunchKernelGGL(k_perm_in_cols, dim3(g.x, (L.nk + PERM_CW - 1) / PERM_CW), b, 0, L.st, n, d_rperm, d_rs, L.bj[0], L.cstr, L.XP, (int64_t)n, all, L.nk);
        gate_acquire();
        int32_t code = run_triangular(L.XP, L.nk, L.WRK, n, wstr, L.st, L.sync, L.timed, L.id);
        if (code != SUCCESSFUL_EXIT) return code;
        if (L.nk == 1) hipLaunchKernelGGL(k_perm_out, g, b, 0, L.st, n, d_perm, d_cs, L.XP, L.xj[0], 0);
        else hipLaunchKernelGGL(k_perm_out_cols, dim3(g.x, (L.nk + PERM_CW - 1) / PERM_CW), b, 0, L.st, n, d_perm, d_cs, L.XP, (int64_t)n, L.xj[0], L.cstr, 0, all, L.nk);
        for (int32_t c = 0; c < L.nk; c++) L.prev[c] = INFINITY, L.active[c] = true;
        if (opt.refinement_nstep <= 0) return finish(L);
        return enqueue_norms(L);
    };
    // Iterative refinement on A x = b (UMFPACK refines inside umfpack_di_solve, interface_umfpack.c:229), one step of the
    // lane's block; called when the norms of its last residual have arrived.
    // Stopping rule per column on the sparse backward error omega = max_i |r_i| / (|A||x| + |b|)_i: stop when
    // omega <= eps, when a step fails to halve it, or after refinement_nstep steps; a step that makes omega worse is
    // taken back.  The correction solves of a block run together as long as any of its columns is still active.
    auto advance = [&](SolveLane &L) -> int32_t {
        if (L.timed) harvest_tri();
        bool any = false;
        for (int32_t c = 0; c < L.nk; c++) {
            if (!L.active[c]) continue;
            double rn = 0.0, omega = 0.0; // maxima over the slots of k_residual (non-negative doubles)
            for (int32_t sl = 0; sl < RES_SLOTS; sl++) {
                rn = std::max(rn, L.h_nrm[(size_t)RES_NORM_WORDS * c + (size_t)sl * RES_SLOT_WORDS]);
                omega = std::max(omega, L.h_nrm[(size_t)RES_NORM_WORDS * c + (size_t)sl * RES_SLOT_WORDS + 1]);
            }
            if (L.it > 0 && !(omega < L.prev[c])) {
                hipLaunchKernelGGL(k_perm_out, g, b, 0, L.st, n, d_perm, d_cs, L.DU + (size_t)c * n, L.xj[c], 2); // take the last correction back (rare: one launch per such column)
                L.active[c] = false;
                col_omega[(size_t)(L.j0 + c)] = L.prev[c]; // (the solution it goes back to)
                continue;
            }
            col_omega[(size_t)(L.j0 + c)] = omega; // backward error of the column's current solution (what the Krylov rescue looks at)
            if (L.j0 + c == 0) last_residual_inf = rn, last_omega = omega;
            if (opt.verbose && L.j0 + c == 0) fprintf(stderr, "hipmf: refinement step %d: |r|_inf = %.3e, omega = %.3e\n", L.it, rn, omega);
            if (omega <= EPS || L.it == opt.refinement_nstep || (L.it > 0 && omega > 0.5 * L.prev[c])) {
                L.active[c] = false;
                continue;
            }
            L.prev[c] = omega;
            any = true;
        }
        if (!any) return finish(L);
        uint64_t amask = 0;
        uint32_t gmask = 0; // groups of the launch that still hold an active column: the others' tasks return at once
        for (int32_t c = 0; c < L.nk; c++)
            if (L.active[c]) amask |= 1ull << c, gmask |= 1u << (c / SF_KMAX);
        if (L.nk <= SF_KMAX) gmask = 0xffffffffu;
        if (L.nk == 1) hipLaunchKernelGGL(k_perm_in, g, b, 0, L.st, n, d_rperm, d_rs, L.RR, L.DU);
        else hipLaunchKernelGGL(k_perm_in_cols, dim3(g.x, (L.nk + PERM_CW - 1) / PERM_CW), b, 0, L.st, n, d_rperm, d_rs, L.RR, (int64_t)n, L.DU, (int64_t)n, amask, L.nk); // finished columns ride along as zeros
        gate_acquire();
        int32_t code = run_triangular(L.DU, L.nk, L.WRK, n, wstr, L.st, L.sync, L.timed, L.id, gmask);
        if (code != SUCCESSFUL_EXIT) return code;
        if (L.nk == 1) hipLaunchKernelGGL(k_perm_out, g, b, 0, L.st, n, d_perm, d_cs, L.DU, L.xj[0], 1);
        else hipLaunchKernelGGL(k_perm_out_cols, dim3(g.x, (L.nk + PERM_CW - 1) / PERM_CW), b, 0, L.st, n, d_perm, d_cs, L.DU, (int64_t)n, L.xj[0], L.cstr, 1, amask, L.nk);
        if (L.j0 == 0 && L.active[0]) refinement_steps_done++;
        // a column whose backward error was already within 64 eps is done after this correction: no further residual /
        // norm / host round trip just to confirm it
        bool again = false;
        for (int32_t c = 0; c < L.nk; c++) {
            if (L.active[c] && L.prev[c] <= 64.0 * EPS) L.active[c] = false;
            again |= L.active[c];
        }
        L.it++;
        if (!again || L.it > opt.refinement_nstep) return finish(L);
        return enqueue_norms(L);
    };

    int32_t next = 0;
    for (;;) {
        bool progressed = false;
        for (int32_t l = 0; l < nlanes; l++)
            if (!lanes[l].busy && next < nblocks) {
                int32_t code = start(lanes[l], next * KS);
                if (code != SUCCESSFUL_EXIT) return code;
                next++;
                progressed = true;
            }
        for (int32_t l = 0; l < nlanes; l++)
            if (lanes[l].busy) {
                HIPC(hipStreamSynchronize(lanes[l].st), ERROR_HIP_SYNCHRONIZE);
                if (nlanes == 1 && gate.owns_lock()) gate.unlock(); // (nothing of this solve is resident: another handle may go)
                int32_t code = advance(lanes[l]);
                if (code != SUCCESSFUL_EXIT) return code;
                progressed = true;
            }
        if (!progressed) break;
    }
    for (int32_t l = 1; l < nlanes; l++) HIPC(hipStreamSynchronize(lanes[l].st), ERROR_HIP_SYNCHRONIZE); // (idle by now: every block is finished)
    HIPC(hipEventRecord((hipEvent_t)ev[7], STREAM), ERROR_HIP_SYNCHRONIZE);
    if (use_fused) {
        HIPC(hipMemcpyAsync(&sf_err[0], d_sync + sync_words - 1, sizeof(int32_t), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        sf_err[1] = 0;
        for (int32_t l = 1; l < nlanes; l++) {
            int32_t e = 0;
            HIPC(hipMemcpy(&e, lanes[l].sync + sync_words - 1, sizeof(int32_t), hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
            sf_err[1] |= e;
        }
    }
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    harvest_tri();
    if (use_fused && d_trace && (nrhs == 1 || !sfk_host.empty())) {
        // dump: one line per task of the two upper launches: direction, level, front, kind, p, f, four stamps (10 ns units)
        // (a blocked solve: the stamps of its last block, against the task list of the blocked instances)
        const bool tr_k = nrhs > 1, tr_tree = !tr_k && tree_active;
        const std::vector<int32_t> &host = tr_k ? sfk_host : sf_host;
        const int32_t band0 = tr_k ? sfk_fwd_band : sf_fwd_band, fwd_all = tr_k ? sfk_fwd_cnt : sf_fwd_cnt;
        const size_t nf = tr_tree ? (size_t)sf2_fwd_cnt : (size_t)((tr_k ? sfk_fwd_cnt : sf_fwd_launch) - std::min(band0, tr_k ? sfk_fwd_cnt : sf_fwd_launch));
        const size_t nb = tr_tree ? (size_t)sf2_bwd_cnt : (size_t)(tr_k ? sfk_bwd_top : sf_bwd_top);
        std::vector<unsigned long long> tr(8 * (nf + nb));
        (void)hipMemcpy(tr.data(), d_trace, sizeof(unsigned long long) * tr.size(), hipMemcpyDeviceToHost);
        if (FILE *fp = fopen(sf_trace.c_str(), "w")) {
            for (size_t k = 0; k < nf + nb; k++) {
                const size_t ti = tr_tree ? k : (k < nf ? (size_t)band0 + k : (size_t)fwd_all + (k - nf));
                if (2 * ti + 1 >= host.size()) break;
                const int32_t kind = host[2 * ti], a = host[2 * ti + 1];
                fprintf(fp, "%c %d %d %d %d %d %llu %llu %llu %llu %llu %llu\n", k < nf ? 'F' : 'B', S.sn_level[a], a, kind, S.npiv(a), S.fsize(a),
                        tr[8 * k], tr[8 * k + 1], tr[8 * k + 2], tr[8 * k + 3], tr[8 * k + 4], tr[8 * k + 5]);
            }
            fclose(fp);
        }
    }
    if (use_fused && (sf_err[0] != 0 || sf_err[1] != 0)) {
        // a hand-off wait timed out (never expected): the result is not trusted; redo with the level-set launches
        use_fused = false; // (level-set kernels, or -- L D L^T fronts, fronts beyond their LDS staging -- the same kernels level by level)
        fused_fallbacks++;
        sf_err[0] = sf_err[1] = 0;
        (void)hipMemset(d_sync + sync_words - 1, 0, sizeof(int32_t));
        for (LaneBuffers &lb : extra_lanes) (void)hipMemset(lb.sync + sync_words - 1, 0, sizeof(int32_t));
        last_error = "dependency-driven solve timed out; level-set path used instead";
        if (opt.verbose) fprintf(stderr, "hipmf: %s\n", last_error.c_str());
        if (gate.owns_lock()) gate.unlock();
        return solve_core(x, rhs, nrhs, ldx, on_device);
    }
    if (staged) memcpy(x, h_stage + n, sizeof(double) * (size_t)n);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, (hipEvent_t)ev[6], (hipEvent_t)ev[7]);
    times.solve_total_ms = ms;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::spmv(double *y, const double *x, double alpha, bool on_device) {
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !y) return ERROR_NULL_POINTER;
    DeviceScope dev_scope(device);
    const int32_t n = S.n;
    const double *xd = x;
    double *yd = y;
    if (!on_device) {
        HIPC(hipMemcpyAsync(d_b, x, sizeof(double) * n, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        xd = d_b;
        yd = d_x;
    }
    hipLaunchKernelGGL(k_spmv_stream<false>, dim3(spmv_blocks), dim3(256), 0, STREAM, d_row_blk, d_rp, d_ci, d_vals, d_tptr, d_tidx, d_arow, alpha, xd,
                       (const double *)nullptr, yd, (unsigned long long *)nullptr);
    if (!on_device) HIPC(hipMemcpyAsync(y, d_x, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    return SUCCESSFUL_EXIT;
}

// The matrix values a caller hands over, into dst (nnz doubles in the handle's CSR order; d_vals for a factorize, d_up_vals for the
// solve_updated forms): through the value map (mapped: its inputs), as they are, or expanded from a mirrored lower triangle.
int32_t Solver::stage_values(double *dst, const double *values, bool mapped, bool on_device) {
    const int64_t nnz = S.nnz_a;
    const dim3 gv((unsigned)std::min<int64_t>(4096, (nnz + 255) / 256)), b256(256);
    if (!mapped && !d_emap) {
        HIPC(hipMemcpyAsync(dst, values, sizeof(double) * nnz, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        return SUCCESSFUL_EXIT;
    }
    const double *src = values;
    if (!on_device) {
        double *const via = mapped ? d_vin : d_vlow;
        HIPC(hipMemcpyAsync(via, values, sizeof(double) * (mapped ? nnz_in : nnz_low), hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        src = via;
    }
    if (mapped) hipLaunchKernelGGL(k_gather_values, gv, b256, 0, STREAM, nnz, d_seg_ptr, d_seg_idx, src, dst);
    else hipLaunchKernelGGL(k_expand_values, gv, b256, 0, STREAM, nnz, d_emap, src, dst);
    return SUCCESSFUL_EXIT;
}

// ---- what the solve_updated forms share ----
namespace {

// tolerance (default 1e-12), restart length (HIPMF_UPDATED_RESTART, 4 .. 200, default 30), step limit (default: four cycles) and
// whether the phases of a step are timed (HIPMF_UPDATED_TIMING=1)
struct UpdatedParams {
    double tol;
    int32_t restart, step_limit;
    bool timing;
    UpdatedParams(double rel_tol, int32_t max_steps) : tol(rel_tol > 0.0 ? rel_tol : 1e-12) {
        restart = Tunables::now(&Tunables::updated_restart);
        step_limit = max_steps > 0 ? max_steps : 4 * restart;
        timing = Tunables::now(&Tunables::updated_timing);
    }
};

// The bases V ((m + 1) x per_step doubles) and Z (m x per_step) anew; when they do not fit the restart length is halved (down to 4).
// Returns the restart length they hold; 0: not even 4 fit, nothing is allocated.
int32_t grow_bases(DeviceArray<double> &V, DeviceArray<double> &Z, int32_t m, size_t per_step) {
    V.reset(), Z.reset();
    for (int32_t mm = m;; mm = std::max(4, mm / 2)) {
        if (V.alloc((size_t)(mm + 1) * per_step) == hipSuccess && Z.alloc((size_t)mm * per_step) == hipSuccess) return mm;
        V.reset(), Z.reset();
        (void)hipGetLastError();
        if (mm == 4) return 0;
    }
}

// HIPMF_UPDATED_TIMING=1: events around the pass pair, the SpMV and the Arnoldi kernels of a step, summed into updated_ms
struct StepTimer {
    EventOwner *ev;
    hipStream_t st;
    bool on;
    hipError_t create() const {
        hipError_t e = hipSuccess;
        for (int t = 0; on && t < 4 && e == hipSuccess; t++)
            if (!ev[t]) e = hipEventCreate(ev[t].put());
        return e;
    }
    void mark(int t) const {
        if (on) (void)hipEventRecord((hipEvent_t)ev[t], st);
    }
    void add(double *ms_sum) const { // (after the step's synchronisation)
        float ms = 0.0f;
        for (int t = 0; on && t < 3; t++)
            if (hipEventElapsedTime(&ms, (hipEvent_t)ev[t], (hipEvent_t)ev[t + 1]) == hipSuccess) ms_sum[t] += ms;
    }
};

// The pass pairs of a solve_updated form or of an error analysis are ordinary unrefined solves: the statistics they leave behind and
// the options they run under are put back when the guard goes.  (krylov_rescue PRODUCES the two krylov_ fields and does not use it.)
struct NestedSolveGuard {
    Solver &s;
    const bool verbose; // as the caller set it
    auto fields() const {
        return std::tie(s.times, s.opt.refinement_nstep, s.opt.verbose, s.refinement_steps_done, s.in_rescue, s.col_omega, s.block_groups_last, s.last_omega,
                        s.last_residual_inf, s.krylov_last_relres, s.krylov_iterations);
    }
    const std::tuple<PhaseTimes, int32_t, bool, int32_t, bool, std::vector<double>, int32_t, double, double, double, int64_t> kept;
    explicit NestedSolveGuard(Solver &s_) : s(s_), verbose(s_.opt.verbose), kept(fields()) {}
    ~NestedSolveGuard() { fields() = kept; }
    void unrefined_quiet() const { s.opt.refinement_nstep = 0, s.opt.verbose = false, s.in_rescue = true; } // (and no Krylov rescue inside)
};

// The arithmetic of the single-column core and of the block driver: the scalar of the host's least-squares problem, doubles per
// coefficient (and with them the restart bound), the labels of the verbose lines and the three launches that differ, single
// (kernels_krylov.hpp, kernels_krylov_complex.hpp) and blocked (kernels_krylov_blocked.hpp, kernels_krylov_complex_blocked.hpp).
struct UpdatedReal {
    typedef double scalar;
    static constexpr int32_t D = 1; // doubles per coefficient; the restart length is at most n / D
    static constexpr const char *label = "solve_updated";
    static void dots(dim3 g, hipStream_t st, int64_t n, const double *w, const double *V, int32_t nv, double *part) { hipLaunchKernelGGL(k_kry_dots, g, dim3(256), 0, st, n, w, V, nv, part); }
    static void update(dim3 g, hipStream_t st, int64_t n, double *w, const double *V, int32_t nv, const double *h, double *part) { hipLaunchKernelGGL(k_kry_update, g, dim3(256), 0, st, n, w, V, nv, h, part); }
    static void combine(dim3 g, hipStream_t st, int64_t n, double *x, const double *Z, int32_t nv, const double *y) { hipLaunchKernelGGL(k_kry_combine, g, dim3(256), 0, st, n, x, Z, nv, y); }
    static constexpr const char *label_many = "solve_updated_many";
    static void dots_blk(dim3 g, hipStream_t st, int64_t n, const double *W, const double *V, int64_t vstr, int32_t nv, uint32_t mask, double *part, int64_t pcol) {
        hipLaunchKernelGGL(k_kryb_dots, g, dim3(256), 0, st, n, W, V, vstr, nv, mask, part, pcol);
    }
    static void update_blk(dim3 g, hipStream_t st, int64_t n, double *W, const double *V, int64_t vstr, int32_t nv, uint32_t mask, const double *h, int64_t hstr, double *part, int64_t pcol) {
        hipLaunchKernelGGL(k_kryb_update, g, dim3(256), 0, st, n, W, V, vstr, nv, mask, h, hstr, part, pcol);
    }
    static void combine_blk(dim3 g, hipStream_t st, int64_t n, double *X, int64_t xstr, const double *Z, int64_t vstr, uint32_t mask, const int32_t *cnt, const double *y, int64_t ystr) {
        hipLaunchKernelGGL(k_kryb_combine, g, dim3(256), 0, st, n, X, xstr, Z, vstr, mask, cnt, y, ystr);
    }
};
struct UpdatedComplex {
    typedef std::complex<double> scalar;
    static constexpr int32_t D = 2; // (the Krylov space of an nc x nc complex matrix has at most nc = n / 2 dimensions)
    static constexpr const char *label = "solve_updated (complex)";
    static void dots(dim3 g, hipStream_t st, int64_t n, const double *w, const double *V, int32_t nv, double *part) { hipLaunchKernelGGL(k_zkry_dots, g, dim3(256), 0, st, n, w, V, nv, part); }
    static void update(dim3 g, hipStream_t st, int64_t n, double *w, const double *V, int32_t nv, const double *h, double *part) { hipLaunchKernelGGL(k_zkry_update, g, dim3(256), 0, st, n, w, V, nv, h, part); }
    static void combine(dim3 g, hipStream_t st, int64_t n, double *x, const double *Z, int32_t nv, const double *y) { hipLaunchKernelGGL(k_zkry_combine, g, dim3(256), 0, st, n, x, Z, nv, y); }
    static constexpr const char *label_many = "solve_updated_many (complex)";
    static void dots_blk(dim3 g, hipStream_t st, int64_t n, const double *W, const double *V, int64_t vstr, int32_t nv, uint32_t mask, double *part, int64_t pcol) {
        hipLaunchKernelGGL(k_zkryb_dots, g, dim3(256), 0, st, n, W, V, vstr, nv, mask, part, pcol);
    }
    static void update_blk(dim3 g, hipStream_t st, int64_t n, double *W, const double *V, int64_t vstr, int32_t nv, uint32_t mask, const double *h, int64_t hstr, double *part, int64_t pcol) {
        hipLaunchKernelGGL(k_zkryb_update, g, dim3(256), 0, st, n, W, V, vstr, nv, mask, h, hstr, part, pcol);
    }
    static void combine_blk(dim3 g, hipStream_t st, int64_t n, double *X, int64_t xstr, const double *Z, int64_t vstr, uint32_t mask, const int32_t *cnt, const double *y, int64_t ystr) {
        hipLaunchKernelGGL(k_zkryb_combine, g, dim3(256), 0, st, n, X, xstr, Z, vstr, mask, cnt, y, ystr);
    }
};

// The columns of a block form one at a time through its single form (no memory for the block buffers of the transposed pass pair):
// `one(c)` solves column c; the counters of the call are the sums over the columns, updated_blocks = 0.
template <class F>
int32_t updated_one_by_one(Solver &s, int32_t nrhs, F one) {
    bool all_converged = true;
    int64_t steps = 0, cycles = 0;
    for (int32_t c = 0; c < nrhs; c++) {
        const int32_t code = one(c);
        if (code != SUCCESSFUL_EXIT && code != WARNING_NOT_CONVERGED) return code;
        all_converged = all_converged && code == SUCCESSFUL_EXIT;
        steps += s.updated_steps, cycles += s.updated_cycles;
    }
    s.updated_steps = s.updated_column_steps = steps, s.updated_cycles = cycles, s.updated_blocks = 0;
    return all_converged ? SUCCESSFUL_EXIT : WARNING_NOT_CONVERGED;
}

// The transposed pass pair on one vector (kernels_solve_transpose.hpp) or on a block of TR_KB (kernels_solve_transpose_blocked.hpp): the
// six kernels, the workspace, and the column stride xs of the block, which the blocked kernels take right after the vector -- their last
// pointer (launch; the small-front kernels end with the leading dimension of their LDS panel: launch_ld).
struct TrSingle {
    static constexpr auto fwd_small = k_tr_fwd_small;
    static constexpr auto assemble = k_tr_assemble;
    static constexpr auto fwd = k_tr_gemv<true>, bwd = k_tr_gemv<false>;
    static constexpr auto gather = k_tr_gather;
    static constexpr auto bwd_small = k_tr_bwd_small;
    static double *work(Solver &s) { return s.d_work_t; }
    template <class K, class... A> static void launch(K k, dim3 g, hipStream_t st, int64_t, const A &...a) { hipLaunchKernelGGL(k, g, dim3(256), 0, st, a...); }
    template <class K, class... A> static void launch_ld(K k, dim3 g, size_t lds, hipStream_t st, int64_t, int32_t ld, const A &...a) { hipLaunchKernelGGL(k, g, dim3(64), lds, st, a..., ld); }
};
struct TrBlocked {
    static constexpr auto fwd_small = k_tr_fwd_small_blk;
    static constexpr auto assemble = k_tr_assemble_blk;
    static constexpr auto fwd = k_tr_gemm_blk<true>, bwd = k_tr_gemm_blk<false>;
    static constexpr auto gather = k_tr_gather_blk;
    static constexpr auto bwd_small = k_tr_bwd_small_blk;
    static double *work(Solver &s) { return s.d_work_tb; }
    template <class K, class... A> static void launch(K k, dim3 g, hipStream_t st, int64_t xs, const A &...a) { hipLaunchKernelGGL(k, g, dim3(256), 0, st, a..., xs); }
    template <class K, class... A> static void launch_ld(K k, dim3 g, size_t lds, hipStream_t st, int64_t xs, int32_t ld, const A &...a) { hipLaunchKernelGGL(k, g, dim3(64), lds, st, a..., xs, ld); }
};

// What Solver::tr_refine launches for the columns it refines: the residual with its norm words (|r|, omega per column: words on the
// device and their pinned mirror), the entry of the residuals into xp, the pass pair (Pass), the exit of xp into x (mode 1: x += the
// correction, 2: x -= it).  mask: the columns a launch works on.
struct TrColumn { // one column through the single kernels, on buffers tr_prepare() made: x, b, then r and xp in d_tvec
    typedef TrSingle Pass;
    static constexpr size_t words = 2;
    Solver &s;
    double *x;
    const double *b;
    const int32_t n = s.S.n;
    const dim3 g = dim3((n + 255) / 256);
    double *const xp = s.d_tvec + 2 * (size_t)n, *const r = s.d_tvec + 3 * (size_t)n; // (xp: after a correction step, the permuted correction)
    unsigned long long *d_nrm() const { return s.d_tnrm; }
    double *h_nrm() const { return s.h_tnrm; }
    void residual(hipStream_t st, uint64_t) const { hipLaunchKernelGGL(k_tr_spmv, g, dim3(256), 0, st, n, s.d_ttptr, s.d_ttrow, s.d_ttmap, s.d_vals, (const double *)x, b, r, d_nrm()); }
    void perm_in(hipStream_t st, uint64_t) const { hipLaunchKernelGGL(k_tr_perm_in, g, dim3(256), 0, st, n, s.d_perm, s.d_cs, (const double *)r, xp); }
    void perm_out(hipStream_t st, int32_t mode, uint64_t) const { hipLaunchKernelGGL(k_perm_out, g, dim3(256), 0, st, n, s.d_rperm, s.d_rs, (const double *)xp, x, mode); }
};
struct TrColumns { // nk columns of a block through the _cols kernels, on the buffers of tr_prepare_blocked(): r and xp in d_tblk
    typedef TrBlocked Pass;
    static constexpr size_t words = 2 * TR_KB;
    Solver &s;
    double *X;
    int64_t xs;
    const double *B;
    int64_t bs;
    int32_t nk;
    const int32_t n = s.S.n;
    const dim3 g = dim3((n + 255) / 256), gp = dim3((n + 255) / 256, TR_KB / PERM_CW);
    double *const xp = s.d_tblk + 2 * (size_t)n * TR_KB, *const r = s.d_tblk + 3 * (size_t)n * TR_KB;
    unsigned long long *d_nrm() const { return s.d_tnrm_blk; }
    double *h_nrm() const { return s.h_tnrm_blk; }
    void residual(hipStream_t st, uint64_t mask) const {
        hipLaunchKernelGGL(k_tr_residual_cols, g, dim3(256), 0, st, n, s.d_ttptr, s.d_ttrow, s.d_ttmap, s.d_vals, (const double *)X, xs, B, bs, r, (int64_t)n, d_nrm(), nk, mask);
    }
    void perm_in(hipStream_t st, uint64_t mask) const { hipLaunchKernelGGL(k_tr_perm_in_cols, gp, dim3(256), 0, st, n, s.d_perm, s.d_cs, (const double *)r, (int64_t)n, xp, (int64_t)n, mask, nk); }
    void perm_out(hipStream_t st, int32_t mode, uint64_t mask) const { hipLaunchKernelGGL(k_perm_out_cols, gp, dim3(256), 0, st, n, s.d_rperm, s.d_rs, (const double *)xp, (int64_t)n, X, xs, mode, mask, nk); }
};

// The buffers and sizes the launches of an error analysis share: ne elements per vector, their grid, the partial results of a reduction
// (values, indices), the eight scalar words (maxima as bits; [5], [6] the results of a reduction) and the integer words ([0] a count or
// an index, [1] the flag of the real sign kernel).
struct EaWork {
    hipStream_t st;
    int32_t ne;
    dim3 g;
    double *pv;
    int32_t *pi;
    unsigned long long *sc;
    int32_t *si;
};
// What differs between the error analysis of a real matrix (k_ea_*, kernels_solve_transpose.hpp) and of a complex one held as its
// real-equivalent system (k_zea_*, kernels_error_analysis_complex.hpp; |.| the modulus): the elements per vector, the launches, whether
// the ordinary pass pair also applies A^{-T}, and two steps of the 1-norm estimator (sign, reduce).
struct EaReal {
    static int32_t elements(int32_t n) { return n; }
    static bool own_transpose(const Solver &s) { return s.S.sym_mode || s.d_tptr; } // A^T = A (L D L^T fronts, symmetric storage)
    static void rows(const Solver &s, const EaWork &w, const double *X, const double *B, double *R, double *AX, double *AR) {
        hipLaunchKernelGGL(k_ea_rows, w.g, dim3(256), 0, w.st, w.ne, s.d_rp, s.d_ci, s.d_vals, s.d_tptr, s.d_tidx, s.d_arow, X, B, R, AX, AR, w.sc);
    }
    static void split(const EaWork &w, double tau_scale, double NX, const double *R, const double *AX, const double *AR, const double *B, double *W1, double *W2) {
        hipLaunchKernelGGL(k_ea_split, w.g, dim3(256), 0, w.st, w.ne, tau_scale, NX, R, AX, AR, B, W1, W2, w.sc, w.si);
    }
    static void hadamard(const EaWork &w, const double *d, const double *v, double *y) { hipLaunchKernelGGL(k_ea_hadamard, w.g, dim3(256), 0, w.st, w.ne, d, v, y); }
    static void fill(const EaWork &w, int32_t mode, int32_t j, double *v) { hipLaunchKernelGGL(k_ea_fill, w.g, dim3(256), 0, w.st, w.ne, mode, j, v); }
    // xi = sign(y); *go_on: the iteration continues.  dlacn2: not after a repeated sign vector (the kernel's flag, not looked at the first
    // time, when xi starts from zeros) and not without growth of the estimate
    static int32_t sign(Solver &s, const EaWork &w, const double *y, double *xi, bool first, bool grew, bool *go_on) {
        int32_t changed = 1;
        if (first) HIPS(s, hipMemsetAsync(xi, 0, sizeof(double) * (size_t)w.ne, w.st), ERROR_HIP_MEMCPY);
        else HIPS(s, hipMemsetAsync(w.si + 1, 0, sizeof(int32_t), w.st), ERROR_HIP_MEMCPY);
        hipLaunchKernelGGL(k_ea_sign, w.g, dim3(256), 0, w.st, w.ne, y, xi, w.si + 1);
        if (!first) {
            HIPS(s, hipMemcpyAsync(&changed, w.si + 1, sizeof(int32_t), hipMemcpyDeviceToHost, w.st), ERROR_HIP_MEMCPY);
            HIPS(s, hipStreamSynchronize(w.st), ERROR_HIP_SYNCHRONIZE);
        }
        *go_on = first || (changed && grew);
        return SUCCESSFUL_EXIT;
    }
    // sum |v_i| (mode 0) or max |v_i| and its first index (mode 1); with jprev >= 0 also v_jprev: a copy ahead of the launches, which the
    // synchronisation completes
    static int32_t reduce(Solver &s, const EaWork &w, const double *v, int32_t mode, double *val, int32_t *idx, int32_t jprev, double *vprev) {
        if (jprev >= 0) HIPS(s, hipMemcpyAsync(vprev, v + jprev, sizeof(double), hipMemcpyDeviceToHost, w.st), ERROR_HIP_MEMCPY);
        hipLaunchKernelGGL(k_ea_reduce1, dim3(EA_RED_WG), dim3(256), 0, w.st, w.ne, mode, v, w.pv, w.pi);
        hipLaunchKernelGGL(k_ea_reduce2, dim3(1), dim3(EA_RED_WG), 0, w.st, mode, (const double *)w.pv, (const int32_t *)w.pi, (double *)(w.sc + 5), w.si);
        HIPS(s, hipMemcpyAsync(val, w.sc + 5, sizeof(double), hipMemcpyDeviceToHost, w.st), ERROR_HIP_MEMCPY);
        HIPS(s, hipMemcpyAsync(idx, w.si, sizeof(int32_t), hipMemcpyDeviceToHost, w.st), ERROR_HIP_MEMCPY);
        HIPS(s, hipStreamSynchronize(w.st), ERROR_HIP_SYNCHRONIZE);
        return SUCCESSFUL_EXIT;
    }
};
struct EaComplex {
    static int32_t elements(int32_t n) { return n / 2; }
    static bool own_transpose(const Solver &) { return false; } // (the transposed pass pair of the 2 nc system applies A^{-H})
    static void rows(const Solver &s, const EaWork &w, const double *X, const double *B, double *R, double *AX, double *AR) {
        hipLaunchKernelGGL(k_zea_rows, w.g, dim3(256), 0, w.st, w.ne, s.d_rp, s.d_ci, s.d_vals, X, B, R, AX, AR, w.sc);
    }
    static void split(const EaWork &w, double tau_scale, double NX, const double *R, const double *AX, const double *AR, const double *B, double *W1, double *W2) {
        hipLaunchKernelGGL(k_zea_split, w.g, dim3(256), 0, w.st, w.ne, tau_scale, NX, R, AX, AR, B, W1, W2, w.sc, w.si);
    }
    static void hadamard(const EaWork &w, const double *d, const double *v, double *y) { hipLaunchKernelGGL(k_zea_hadamard, w.g, dim3(256), 0, w.st, w.ne, d, v, y); }
    static void fill(const EaWork &w, int32_t mode, int32_t j, double *v) { hipLaunchKernelGGL(k_zea_fill, w.g, dim3(256), 0, w.st, w.ne, mode, j, v); }
    // xi = y / |y|.  zlacn2 has no repeated-sign test: no flag, and nothing is launched once the estimate has stopped growing
    static int32_t sign(Solver &, const EaWork &w, const double *y, double *xi, bool first, bool grew, bool *go_on) {
        *go_on = first || grew;
        if (*go_on) hipLaunchKernelGGL(k_zea_sign, w.g, dim3(256), 0, w.st, w.ne, y, xi);
        return SUCCESSFUL_EXIT;
    }
    // the same over the moduli; |v_jprev| by a launch of its own behind the reduction (the same arithmetic), read with the result
    static int32_t reduce(Solver &s, const EaWork &w, const double *v, int32_t mode, double *val, int32_t *idx, int32_t jprev, double *vprev) {
        hipLaunchKernelGGL(k_zea_reduce1, dim3(EA_RED_WG), dim3(256), 0, w.st, w.ne, mode, v, w.pv, w.pi);
        hipLaunchKernelGGL(k_ea_reduce2, dim3(1), dim3(EA_RED_WG), 0, w.st, mode, (const double *)w.pv, (const int32_t *)w.pi, (double *)(w.sc + 5), w.si);
        if (jprev >= 0) hipLaunchKernelGGL(k_zea_abs_at, dim3(1), dim3(64), 0, w.st, v, jprev, (double *)(w.sc + 6));
        double t[2] = {0.0, 0.0};
        HIPS(s, hipMemcpyAsync(t, w.sc + 5, sizeof(double) * 2, hipMemcpyDeviceToHost, w.st), ERROR_HIP_MEMCPY);
        HIPS(s, hipMemcpyAsync(idx, w.si, sizeof(int32_t), hipMemcpyDeviceToHost, w.st), ERROR_HIP_MEMCPY);
        HIPS(s, hipStreamSynchronize(w.st), ERROR_HIP_SYNCHRONIZE);
        *val = t[0];
        if (jprev >= 0) *vprev = t[1];
        return SUCCESSFUL_EXIT;
    }
};

} // namespace

// The operator of the single-column core and of the block driver, next to the arithmetic: A_new (the stream SpMV on the row blocks of
// initialize, preconditioner solve_core) or A_new^T (kernels_krylov_transpose.hpp on the row blocks of A^T that tr_prepare() cuts,
// preconditioner the unrefined transposed pass pair: level-synchronous launches that wait for nothing and take no device gate).  An
// operator gives the preconditioner call on C contiguous columns, the product and the residual, single and blocked, and where the
// residual's partial sums go: `blocks` slots per sum, in the Krylov kernels' buffer (plain) or in d_tt_part.  Both read d_up_vals.
struct Solver::OpPlain {
    static constexpr const char *tag = "";
    static int32_t blocks(const Solver &s) { return s.spmv_blocks; }
    static double *part(Solver &, double *krylov_part) { return krylov_part; }
    static int64_t pcol(const Solver &, int64_t krylov_pcol) { return krylov_pcol; }
    static int32_t precond(Solver &s, double *z, const double *v, int32_t C) { return s.solve_core(z, v, C, s.S.n, true); }
    static void product(Solver &s, hipStream_t st, const double *z, double *w) {
        hipLaunchKernelGGL(k_spmv_stream<false>, dim3(s.spmv_blocks), dim3(256), 0, st, s.d_row_blk, s.d_rp, s.d_ci, s.d_up_vals, s.d_tptr, s.d_tidx, s.d_arow, 1.0, z,
                           (const double *)nullptr, w, (unsigned long long *)nullptr);
    }
    static void residual(Solver &s, hipStream_t st, const double *x, const double *b, double *r, double *part) {
        hipLaunchKernelGGL(k_kry_residual, dim3(s.spmv_blocks), dim3(256), 0, st, s.d_row_blk, s.d_rp, s.d_ci, s.d_up_vals, s.d_tptr, s.d_tidx, s.d_arow, x, b, r, part);
    }
    static void product_blk(Solver &s, hipStream_t st, int64_t n, const double *Z, double *W, int32_t C, uint32_t mask) {
        hipLaunchKernelGGL(k_kryb_spmv, dim3(s.spmv_blocks), dim3(256), 0, st, s.d_row_blk, s.d_rp, s.d_ci, s.d_up_vals, s.d_tptr, s.d_tidx, s.d_arow, n, Z, W, C, mask);
    }
    static void residual_blk(Solver &s, hipStream_t st, int64_t n, const double *X, int64_t xstr, const double *B, int64_t bstr, double *R, int32_t C, uint32_t mask,
                             double *part, int64_t pcol) {
        hipLaunchKernelGGL(k_kryb_residual, dim3(s.spmv_blocks), dim3(256), 0, st, s.d_row_blk, s.d_rp, s.d_ci, s.d_up_vals, s.d_tptr, s.d_tidx, s.d_arow, n, X, xstr, B, bstr,
                           R, C, mask, part, pcol);
    }
};
struct Solver::OpTransposed { // (after tr_prepare(); the blocked launches after tr_prepare_blocked())
    static constexpr const char *tag = " (transposed)";
    static int32_t blocks(const Solver &s) { return s.tt_blocks; }
    static double *part(Solver &s, double *) { return s.d_tt_part; }
    static int64_t pcol(const Solver &s, int64_t) { return 2 * (int64_t)s.tt_blocks; }
    static int32_t precond(Solver &s, double *z, const double *v, int32_t C) { return C == 1 ? s.tr_pass(z, v) : s.tr_pass_blk(z, v, C); }
    static void product(Solver &s, hipStream_t st, const double *z, double *w) {
        hipLaunchKernelGGL(k_kry_spmv_t, dim3(s.tt_blocks), dim3(256), 0, st, s.d_ttblk, s.d_ttptr, s.d_ttrow, s.d_ttmap, s.d_up_vals, z, w);
    }
    static void residual(Solver &s, hipStream_t st, const double *x, const double *b, double *r, double *part) {
        hipLaunchKernelGGL(k_kry_residual_t, dim3(s.tt_blocks), dim3(256), 0, st, s.d_ttblk, s.d_ttptr, s.d_ttrow, s.d_ttmap, s.d_up_vals, x, b, r, part);
    }
    static void product_blk(Solver &s, hipStream_t st, int64_t n, const double *Z, double *W, int32_t C, uint32_t mask) {
        hipLaunchKernelGGL(k_kryb_spmv_t, dim3(s.tt_blocks), dim3(256), 0, st, s.d_ttblk, s.d_ttptr, s.d_ttrow, s.d_ttmap, s.d_up_vals, n, Z, W, C, mask);
    }
    static void residual_blk(Solver &s, hipStream_t st, int64_t n, const double *X, int64_t xstr, const double *B, int64_t bstr, double *R, int32_t C, uint32_t mask,
                             double *part, int64_t pcol) {
        hipLaunchKernelGGL(k_kryb_residual_t, dim3(s.tt_blocks), dim3(256), 0, st, s.d_ttblk, s.d_ttptr, s.d_ttrow, s.d_ttmap, s.d_up_vals, n, X, xstr, B, bstr, R, C, mask,
                           part, pcol);
    }
};

// ---- solve with new matrix values on the kept factor (solver_hipmf_solve_updated, complex_solver_hipmf_solve_updated) ----
// The callers of this backend change the VALUES of the matrix often and by little (a new step size scales the shift of gamma M - J, a
// Jacobian moves in a few rows): instead of a factorisation the old factor M serves as RIGHT preconditioner of a flexible GMRES on
// A_new x = b, started from x = 0.  Unlike the Krylov rescue above (host vectors, rare path) everything of length n lives on the device:
// per step z_k = M^{-1} v_k (one unrefined pass pair: solve_core on device pointers, default schedule, the device gate as in any solve),
// w = A_new z_k (the stream SpMV on the operator's own value buffer), classical Gram-Schmidt twice (CGS2: dots + k_kry_reduce + update,
// two rounds; all coefficients stay on the device), v_{k+1} = w / |w| (k_kry_scale).  The host reads back ONE small record per step
// through pinned memory -- both coefficient sets (it adds them: the new Hessenberg column) and the two squared norms, 2 D (k + 1) + 2
// doubles --, pushes the column into the least-squares problem (GivensLsq, krylov_host.hpp), and per cycle uploads y for x += Z y
// (combine) and reads the two sums of the recomputed true residual (k_kry_residual).  Non-finite numbers in a step's record (a direction
// the factor cannot give) end the cycle with the directions before it, as in the rescue.  A cycle that does not lower the true residual
// is taken back and ends the call: x is the best iterate.
// One core serves both arithmetics; the policy P gives what differs.  In the COMPLEX form this Solver holds the real-equivalent form
// of order n = 2 nc of a complex matrix, its vectors are nc interleaved (re, im) pairs.  Real GMRES on that system minimises over real
// coefficients only and usually needs 20 - 40 % more pass pairs.  Pass pair, SpMV, |w|^2 (the real sum over n doubles), normalisation
// and residual are the real form's launches; the coefficients are complex, D = 2 doubles each: h_j = sum conj(v_j,i) w_i (k_zkry_dots:
// two sums per basis vector, k_kry_reduce over 2 nv columns leaves them interleaved), k_zkry_update, k_zkry_combine.  The preconditioner
// only has to give SOME vector: a factor that is not exactly complex-linear (HIPMF_COMPLEX_PAIRS=0, replaced pivots) is merely weaker.
// The operator is a second axis, O: OpPlain is the text above; OpTransposed solves A_new^T x = b with z_k = M^{-T} v_k (tr_pass) and
// w = A_new^T z_k, r = b - A_new^T x from kernels_krylov_transpose.hpp -- Arnoldi, CGS2, the records, the least-squares problem and
// the cycle logic are shared.  conj_pairs (complex A^T through the A^H iteration): b is conjugated into the staging vector on entry, x
// on exit.
template <class P, class O>
int32_t Solver::solve_updated_core(double *x, const double *rhs, const double *values, bool mapped, double rel_tol, int32_t max_steps, int32_t *steps_out,
                                   double *relres_out, bool on_device, bool conj_pairs) {
    typedef typename P::scalar T;
    constexpr int32_t D = P::D;
    DeviceScope dev_scope(device);
    const int32_t n = S.n;
    const UpdatedParams par(rel_tol, max_steps);
    const StepTimer timer{up_ev, STREAM, par.timing};
    updated_steps = updated_cycles = 0;
    updated_ms[0] = updated_ms[1] = updated_ms[2] = 0.0;
    if (steps_out) *steps_out = 0;
    if (relres_out) *relres_out = 0.0;

    // buffers: the bases grow with the restart length (a complex basis vector is one real vector of n doubles); the partial sums, the
    // record and its mirror are sized for D = 2 whichever form allocates them
    int32_t m = std::max(4, std::min(par.restart, n / D));
    if (up_m < m && (up_m = grow_bases(d_up_V, d_up_Z, m, (size_t)n)) == 0) {
        last_error = "solve_updated: no device memory for the Krylov bases";
        return ERROR_HIP_MALLOC;
    }
    m = std::min(m, up_m);
    const int32_t nblk = (int32_t)(((int64_t)n + KRY_TILE - 1) / KRY_TILE);
    const int32_t rec_m = std::max(up_m, 200);
    if (!d_up_vals) HIPC(d_up_vals.alloc((size_t)std::max<int64_t>(S.nnz_a, 1)), ERROR_HIP_MALLOC);
    if (!d_up_vec) HIPC(d_up_vec.alloc(4 * (size_t)n), ERROR_HIP_MALLOC);
    if (!d_up_part || up_rec_m < rec_m) {
        HIPC(d_up_part.alloc(std::max((size_t)(2 * rec_m + 1) * nblk, 2 * (size_t)std::max(spmv_blocks, 1))), ERROR_HIP_MALLOC);
        HIPC(d_up_rec.alloc(6 * (size_t)rec_m + 8), ERROR_HIP_MALLOC);
        HIPC(h_up.alloc(6 * (size_t)rec_m + 8), ERROR_HIP_MALLOC);
        up_rec_m = rec_m;
    }
    HIPC(timer.create(), ERROR_HIP_SYNCHRONIZE);
    // the record: [0, 2 D m + 2) both coefficient sets of the step, then the squared norms after the two rounds; |r|^2, |b|^2; y
    double *const d_h = d_up_rec, *const d_res = d_up_rec + 2 * D * (size_t)rec_m + 2, *const d_y = d_res + 2;
    double *const h_rec = h_up, *const h_res = h_up + 2 * D * (size_t)rec_m + 2, *const h_y = h_res + 2;
    double *const d_w = d_up_vec, *const d_r = d_up_vec + (size_t)n;
    double *const d_xx = on_device ? x : d_up_vec + 2 * (size_t)n;
    const double *d_bb = rhs;
    const size_t nb = sizeof(double) * (size_t)n;

    // the operator's values: the staging factorize gives its own, into d_up_vals
    int32_t code = stage_values(d_up_vals, values, mapped, on_device);
    if (code != SUCCESSFUL_EXIT) return code;
    const dim3 gk((unsigned)nblk), b256(256), gn((unsigned)((n + 255) / 256));
    if (!on_device || conj_pairs) { // (the caller's device vector is read where it is unless it has to be conjugated)
        HIPC(hipMemcpyAsync(d_up_vec + 3 * (size_t)n, rhs, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        if (conj_pairs) hipLaunchKernelGGL(k_tr_conj, gn, b256, 0, STREAM, n, d_up_vec + 3 * (size_t)n);
        d_bb = d_up_vec + 3 * (size_t)n;
    }
    HIPC(hipMemsetAsync(d_xx, 0, nb, STREAM), ERROR_HIP_MEMCPY);

    double *const d_rpart = O::part(*this, d_up_part); // the partial sums of the residual
    // r = b - A_new x with its two sums on the host (one synchronisation)
    auto residual = [&](double &rr, double &bb) -> int32_t {
        O::residual(*this, STREAM, d_xx, d_bb, d_r, d_rpart);
        hipLaunchKernelGGL(k_kry_reduce, dim3(2), b256, 0, STREAM, (const double *)d_rpart, O::blocks(*this), d_res);
        HIPC(hipMemcpyAsync(h_res, d_res, 2 * sizeof(double), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        rr = h_res[0], bb = h_res[1];
        return SUCCESSFUL_EXIT;
    };
    auto combine = [&](int32_t kk, double sign) -> int32_t { // x += sign Z y
        for (int32_t j = 0; j < D * kk; j++) h_y[j] = sign * h_y[j];
        HIPC(hipMemcpyAsync(d_y, h_y, sizeof(double) * D * kk, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        P::combine(gk, STREAM, (int64_t)n, d_xx, d_up_Z, kk, d_y);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE); // (h_y may be rewritten)
        return SUCCESSFUL_EXIT;
    };
    auto finish = [&](int32_t code, double relres) -> int32_t {
        if (steps_out) *steps_out = (int32_t)updated_steps;
        if (relres_out) *relres_out = relres;
        if (conj_pairs && updated_steps > 0) { // (no step: x is the zeros of the entry, kept +0.0 as the other forms return them)
            hipLaunchKernelGGL(k_tr_conj, gn, b256, 0, STREAM, n, d_xx);
            HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        }
        if (!on_device) HIPC(hipMemcpy(x, d_xx, nb, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
        HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
        return code;
    };

    double rr = 0.0, bb = 0.0;
    code = residual(rr, bb);
    if (code != SUCCESSFUL_EXIT) return code;
    if (bb == 0.0) return finish(SUCCESSFUL_EXIT, 0.0); // x = 0
    if (!std::isfinite(bb)) return finish(WARNING_NOT_CONVERGED, NAN);
    const double bnorm = sqrt(bb);
    double rnorm = sqrt(rr);
    {
        const NestedSolveGuard guard(*this);
        guard.unrefined_quiet();
        GivensLsq<T> lsq(m);
        std::vector<T> rec(2 * (size_t)m), hcol((size_t)m), y((size_t)m);
        while (rnorm > par.tol * bnorm && updated_steps < par.step_limit) {
            updated_cycles++;
            hipLaunchKernelGGL(k_kry_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)d_r, (const double *)d_res, (double *)d_up_V); // v_0 = r / |r|
            lsq.reset(rnorm);
            int32_t k = 0; // directions of this cycle that entered the least-squares problem
            while (k < m && updated_steps < par.step_limit) {
                double *const zk = d_up_Z + (size_t)k * n;
                const double *const vk = d_up_V + (size_t)k * n;
                timer.mark(0);
                code = O::precond(*this, zk, vk, 1); // z_k = M^{-1} v_k
                if (code != SUCCESSFUL_EXIT) break;
                timer.mark(1);
                O::product(*this, STREAM, zk, d_w); // w = A_new z_k
                timer.mark(2);
                const int32_t nv = k + 1;
                double *const d_nrm = d_h + 2 * D * (size_t)nv; // the squared norms after the two rounds
                for (int32_t round = 0; round < 2; round++) { // CGS2
                    double *const hr = d_h + (size_t)round * D * nv;
                    P::dots(gk, STREAM, (int64_t)n, d_w, d_up_V, nv, d_up_part);
                    hipLaunchKernelGGL(k_kry_reduce, dim3(D * nv), b256, 0, STREAM, (const double *)d_up_part, nblk, hr);
                    P::update(gk, STREAM, (int64_t)n, d_w, d_up_V, nv, hr, d_up_part);
                    hipLaunchKernelGGL(k_kry_reduce, dim3(1), b256, 0, STREAM, (const double *)d_up_part, nblk, d_nrm + round);
                }
                hipLaunchKernelGGL(k_kry_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)d_w, (const double *)(d_nrm + 1), d_up_V + (size_t)(k + 1) * n);
                timer.mark(3);
                const int32_t nrec = 2 * D * nv + 2;
                if (hipMemcpyAsync(h_rec, d_h, sizeof(double) * nrec, hipMemcpyDeviceToHost, STREAM) != hipSuccess) code = ERROR_HIP_MEMCPY;
                if (code == SUCCESSFUL_EXIT && hipStreamSynchronize(STREAM) != hipSuccess) code = ERROR_HIP_SYNCHRONIZE;
                if (code != SUCCESSFUL_EXIT) break;
                timer.add(updated_ms);
                bool finite = true;
                for (int32_t j = 0; j < nrec; j++) finite = finite && std::isfinite(h_rec[j]);
                if (!finite) break; // (leave the cycle with what there is)
                updated_steps++;
                memcpy(rec.data(), h_rec, sizeof(T) * 2 * nv); // the new Hessenberg column: the coefficients of the two rounds, added
                for (int32_t j = 0; j < nv; j++) hcol[(size_t)j] = rec[(size_t)j] + rec[(size_t)(nv + j)];
                const double hn = sqrt(h_rec[nrec - 1]);
                lsq.push(k, hcol.data(), hn);
                if (guard.verbose)
                    fprintf(stderr, "hipmf: %s%s: cycle %lld step %d: residual estimate %.3e (|b| = %.3e)\n", P::label, O::tag, (long long)updated_cycles, k + 1, std::abs(lsq.g[(size_t)k + 1]), bnorm);
                k++;
                if (std::abs(lsq.g[(size_t)k]) <= par.tol * bnorm || !(hn > 0.0)) break;
            }
            if (code != SUCCESSFUL_EXIT || k == 0) break;
            lsq.solve(k, y.data());
            memcpy(h_y, y.data(), sizeof(T) * (size_t)k);
            code = combine(k, 1.0);
            if (code != SUCCESSFUL_EXIT) break;
            const double before = rnorm;
            code = residual(rr, bb);
            if (code != SUCCESSFUL_EXIT) break;
            if (guard.verbose) fprintf(stderr, "hipmf: %s%s: cycle %lld: |r| %.3e -> %.3e\n", P::label, O::tag, (long long)updated_cycles, before, sqrt(rr));
            if (!(sqrt(rr) < before)) { // no gain (or not a number): the cycle is taken back, x is the best iterate
                code = combine(k, -1.0);
                if (code == SUCCESSFUL_EXIT) code = residual(rr, bb);
                if (code == SUCCESSFUL_EXIT) rnorm = sqrt(rr);
                break;
            }
            rnorm = sqrt(rr);
        }
    }
    if (code != SUCCESSFUL_EXIT) return code;
    return finish(rnorm <= par.tol * bnorm ? SUCCESSFUL_EXIT : WARNING_NOT_CONVERGED, rnorm / bnorm);
}

int32_t Solver::solve_updated(double *x, const double *rhs, const double *values, bool mapped, double rel_tol, int32_t max_steps, int32_t *steps_out,
                              double *relres_out, bool on_device, bool transposed) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs || !values) return ERROR_NULL_POINTER;
    if (!std::isfinite(rel_tol)) return ERROR_HIPMF_INVALID_VALUE;
    if (mapped && nnz_in < 1) return ERROR_HIPMF_INVALID_VALUE; // no map set
    if (!transposed || S.sym_mode || d_tptr) // (A^T = A: L D L^T fronts, symmetric storage)
        return solve_updated_core<UpdatedReal, OpPlain>(x, rhs, values, mapped, rel_tol, max_steps, steps_out, relres_out, on_device, false);
    DeviceScope dev_scope(device);
    const int32_t code = tr_prepare();
    if (code != SUCCESSFUL_EXIT) return code;
    return solve_updated_core<UpdatedReal, OpTransposed>(x, rhs, values, mapped, rel_tol, max_steps, steps_out, relres_out, on_device, false);
}

// values: always the inputs of the installed (signed) value map, gathered as factorize_mapped gathers them
int32_t Solver::solve_updated_complex(double *x, const double *rhs, const double *values, double rel_tol, int32_t max_steps, int32_t *steps_out,
                                      double *relres_out, bool on_device, bool transposed, bool conj_pairs) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs || !values) return ERROR_NULL_POINTER;
    if (!std::isfinite(rel_tol)) return ERROR_HIPMF_INVALID_VALUE;
    if (nnz_in < 1 || (S.n & 1) || d_emap) return ERROR_HIPMF_INVALID_VALUE; // the complex handle: a value map, pairs, a general pattern
    updated_complex = true;
    if (!transposed || S.sym_mode || d_tptr) // (a symmetric real-equivalent form: A^H = A)
        return solve_updated_core<UpdatedComplex, OpPlain>(x, rhs, values, true, rel_tol, max_steps, steps_out, relres_out, on_device, conj_pairs);
    DeviceScope dev_scope(device);
    const int32_t code = tr_prepare();
    if (code != SUCCESSFUL_EXIT) return code;
    return solve_updated_core<UpdatedComplex, OpTransposed>(x, rhs, values, true, rel_tol, max_steps, steps_out, relres_out, on_device, conj_pairs);
}

// ---- the same for a block of right-hand sides (solver_hipmf_solve_updated_many; kernels_krylov_blocked.hpp) ----
// Every column runs the flexible GMRES above on its own -- own basis, own Hessenberg matrix, rotations and g on the host -- and the
// columns of a block of KRYB_COLS advance in lockstep: per block step ONE blocked pass pair Z_k = M^{-1} V_k (solve_core on the C
// contiguous columns of step k), ONE pass over the matrix (k_kryb_spmv), CGS2 and the normalisation batched over the columns, ONE host
// read of the block's record, C (2 k + 4) doubles (complex coefficients: C (4 k + 6)).  A column that is done for the cycle (rotation estimate at the tolerance, hn not
// positive, a non-finite record, its step limit) is "parked": its bit leaves the mask every kernel takes and its column of V_{k+1} is
// zeros.  At the end of a cycle (k == m or every column parked) every column gets its own back substitution over its own count of
// directions, one combine and one residual launch serve the block; a column is finished for the call when its TRUE residual meets the
// tolerance, when the cycle brought no gain (taken back) or when its steps are used up.  The block goes on with the others.
// transposed: the block form also needs the buffers of the blocked transposed pass pair; without memory for them the columns go through
// the single transposed form one at a time, as solve_transpose_many does.
int32_t Solver::solve_updated_many(double *x, const double *rhs, int32_t nrhs, int64_t ld, const double *values, bool mapped, double rel_tol,
                                   int32_t max_steps, int32_t *steps_out, double *relres_out, bool on_device, bool transposed) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs || !values) return ERROR_NULL_POINTER;
    if (nrhs < 1 || ld < S.n || !std::isfinite(rel_tol)) return ERROR_HIPMF_INVALID_VALUE;
    if (mapped && nnz_in < 1) return ERROR_HIPMF_INVALID_VALUE; // no map set
    if (nrhs == 1) {
        const int32_t code = solve_updated(x, rhs, values, mapped, rel_tol, max_steps, steps_out, relres_out, on_device, transposed);
        updated_blocks = 0, updated_column_steps = updated_steps;
        return code;
    }
    if (!transposed || S.sym_mode || d_tptr)
        return solve_updated_many_core<UpdatedReal, OpPlain>(x, rhs, nrhs, ld, values, mapped, rel_tol, max_steps, steps_out, relres_out, on_device, false);
    DeviceScope dev_scope(device);
    const int32_t code = tr_prepare();
    if (code != SUCCESSFUL_EXIT) return code;
    if (tr_prepare_blocked() != SUCCESSFUL_EXIT)
        return updated_one_by_one(*this, nrhs, [&](int32_t c) {
            return solve_updated(x + (int64_t)c * ld, rhs + (int64_t)c * ld, values, mapped, rel_tol, max_steps, steps_out ? steps_out + c : nullptr,
                                 relres_out ? relres_out + c : nullptr, on_device, true);
        });
    return solve_updated_many_core<UpdatedReal, OpTransposed>(x, rhs, nrhs, ld, values, mapped, rel_tol, max_steps, steps_out, relres_out, on_device, false);
}

// The block form for the real-equivalent system of a COMPLEX matrix (complex_solver_hipmf_solve_updated_many): the same lockstep
// iteration with complex coefficients per column (kernels_krylov_complex_blocked.hpp), on the conditions of solve_updated_complex.
// ld counts doubles (twice the caller's complex leading dimension, so every column starts on a complex element).
int32_t Solver::solve_updated_many_complex(double *x, const double *rhs, int32_t nrhs, int64_t ld, const double *values, double rel_tol, int32_t max_steps,
                                           int32_t *steps_out, double *relres_out, bool on_device, bool transposed, bool conj_pairs) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs || !values) return ERROR_NULL_POINTER;
    if (nrhs < 1 || ld < S.n || (ld & 1) || !std::isfinite(rel_tol)) return ERROR_HIPMF_INVALID_VALUE;
    if (nnz_in < 1 || (S.n & 1) || d_emap) return ERROR_HIPMF_INVALID_VALUE; // the complex handle: a value map, pairs, a general pattern
    if (nrhs == 1) {
        const int32_t code = solve_updated_complex(x, rhs, values, rel_tol, max_steps, steps_out, relres_out, on_device, transposed, conj_pairs);
        updated_blocks = 0, updated_column_steps = updated_steps;
        return code;
    }
    updated_complex = true;
    if (!transposed || S.sym_mode || d_tptr)
        return solve_updated_many_core<UpdatedComplex, OpPlain>(x, rhs, nrhs, ld, values, true, rel_tol, max_steps, steps_out, relres_out, on_device, conj_pairs);
    DeviceScope dev_scope(device);
    const int32_t code = tr_prepare();
    if (code != SUCCESSFUL_EXIT) return code;
    if (tr_prepare_blocked() != SUCCESSFUL_EXIT)
        return updated_one_by_one(*this, nrhs, [&](int32_t c) {
            return solve_updated_complex(x + (int64_t)c * ld, rhs + (int64_t)c * ld, values, rel_tol, max_steps, steps_out ? steps_out + c : nullptr,
                                         relres_out ? relres_out + c : nullptr, on_device, true, conj_pairs);
        });
    return solve_updated_many_core<UpdatedComplex, OpTransposed>(x, rhs, nrhs, ld, values, true, rel_tol, max_steps, steps_out, relres_out, on_device, conj_pairs);
}

// One driver serves both arithmetics, as solve_updated_core does: the policy P gives the three blocked launches that differ and the
// doubles per coefficient D, which size the step's record (2 D nv + 2 doubles per column), the partial-sum slots (D (m + 1) nblk per
// column), the restart bound (n / D), y (D m doubles per column) and the scalar of the per-column least-squares problems.  With D = 1
// every launch, its order and its arguments are those of the real driver before the complex form existed.
// O is the operator axis of solve_updated_core: the blocked preconditioner call, product and residual.  conj_pairs: the block's
// right-hand sides are conjugated into the staging block on entry, its solutions on exit (k_tr_conj_cols).
template <class P, class O>
int32_t Solver::solve_updated_many_core(double *x, const double *rhs, int32_t nrhs, int64_t ld, const double *values, bool mapped, double rel_tol,
                                        int32_t max_steps, int32_t *steps_out, double *relres_out, bool on_device, bool conj_pairs) {
    typedef typename P::scalar T;
    constexpr int32_t D = P::D;
    DeviceScope dev_scope(device);
    const int32_t n = S.n;
    const UpdatedParams par(rel_tol, max_steps);
    const StepTimer timer{up_ev, STREAM, par.timing};
    updated_steps = updated_cycles = updated_blocks = updated_column_steps = 0;
    updated_ms[0] = updated_ms[1] = updated_ms[2] = 0.0;
    for (int32_t c = 0; c < nrhs; c++) {
        if (steps_out) steps_out[c] = 0;
        if (relres_out) relres_out[c] = 0.0;
    }

    // buffers: bases for min(nrhs, 16) columns, wider when a later call is; the restart length is halved (down to 4) when they do not fit
    const int32_t CW = std::min<int32_t>(nrhs, KRYB_COLS);
    const int32_t nblk = (int32_t)(((int64_t)n + KRY_TILE - 1) / KRY_TILE);
    int32_t m = std::max(4, std::min(par.restart, n / D));
    if (ub_m < m || ub_cols < CW || ub_d < D) {
        const int32_t cols = std::max(ub_cols, CW);
        ub_m = ub_cols = ub_d = 0;
        const int32_t mm = grow_bases(d_ub_V, d_ub_Z, m, (size_t)cols * n);
        if (mm == 0) {
            last_error = "solve_updated_many: no device memory for the Krylov bases";
            return ERROR_HIP_MALLOC;
        }
        const size_t pcol_new = std::max((size_t)D * (mm + 1) * nblk, 2 * (size_t)std::max(spmv_blocks, 1));
        const size_t rec_new = (size_t)cols * (3 * (size_t)D * mm + 4);
        if (d_ub_vec.alloc(4 * (size_t)cols * n) != hipSuccess || d_ub_part.alloc(pcol_new * cols) != hipSuccess || d_ub_rec.alloc(rec_new) != hipSuccess ||
            h_ub.alloc(rec_new) != hipSuccess || d_ub_cnt.alloc((size_t)cols) != hipSuccess || h_ub_cnt.alloc((size_t)cols) != hipSuccess) {
            d_ub_V.reset(), d_ub_Z.reset();
            (void)hipGetLastError();
            return ERROR_HIP_MALLOC;
        }
        ub_m = mm, ub_cols = cols, ub_d = D;
    }
    m = std::min(m, ub_m);
    if (!d_up_vals) HIPC(d_up_vals.alloc((size_t)std::max<int64_t>(S.nnz_a, 1)), ERROR_HIP_MALLOC);
    HIPC(timer.create(), ERROR_HIP_SYNCHRONIZE);
    const int64_t pcol = (int64_t)std::max((size_t)D * (ub_m + 1) * nblk, 2 * (size_t)std::max(spmv_blocks, 1)); // partial-sum slots of a column
    // device record and its pinned mirror: the step's record, C (2 D nv + 2) | the residuals' sums, 2 C | y, column c at c D m
    const size_t off_res = (size_t)ub_cols * (2 * (size_t)D * ub_m + 2), off_y = off_res + 2 * (size_t)ub_cols;
    double *const d_rec = d_ub_rec, *const d_res = d_ub_rec + off_res, *const d_y = d_ub_rec + off_y;
    double *const h_rec = h_ub, *const h_res = h_ub + off_res, *const h_y = h_ub + off_y;
    const size_t nb = sizeof(double) * (size_t)n;

    // the operator's values, once per call, exactly as in solve_updated
    const dim3 b256(256);
    int32_t code = stage_values(d_up_vals, values, mapped, on_device);
    if (code != SUCCESSFUL_EXIT) return code;

    bool all_converged = true;
    std::vector<GivensLsq<T>> lsq((size_t)KRYB_COLS, GivensLsq<T>(m)); // per column of a block
    std::vector<T> crec(2 * (size_t)m), hcol((size_t)m), y((size_t)m);
    const int64_t ystr = (int64_t)D * m; // between the coefficients y of two columns
    double *const d_rpart = O::part(*this, d_ub_part); // the partial sums of the residuals and their slots per column
    const int64_t rpcol = O::pcol(*this, pcol);
    const bool stage_b = !on_device || conj_pairs; // (the caller's device block is read where it is unless it has to be conjugated)
    {
        const NestedSolveGuard guard(*this);
        guard.unrefined_quiet();
        for (int32_t j0 = 0; j0 < nrhs && code == SUCCESSFUL_EXIT; j0 += KRYB_COLS) {
            const int32_t C = std::min<int32_t>(KRYB_COLS, nrhs - j0);
            const uint32_t all = (1u << C) - 1u;
            const int64_t vstr = (int64_t)C * n; // between two basis vectors of one column
            updated_blocks++;
            double *const d_w = d_ub_vec, *const d_r = d_ub_vec + (size_t)C * n;
            double *const d_xx = on_device ? x + (int64_t)j0 * ld : d_ub_vec + 2 * (size_t)ub_cols * n;
            const double *const d_bb = stage_b ? d_ub_vec + 3 * (size_t)ub_cols * n : rhs + (int64_t)j0 * ld;
            const int64_t xstr = on_device ? ld : (int64_t)n, bstr = stage_b ? (int64_t)n : ld;
            if (stage_b)
                for (int32_t c = 0; c < C && code == SUCCESSFUL_EXIT; c++)
                    if (hipMemcpyAsync(d_ub_vec + 3 * (size_t)ub_cols * n + (size_t)c * n, rhs + (int64_t)(j0 + c) * ld, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                       STREAM) != hipSuccess)
                        code = ERROR_HIP_MEMCPY;
            if (code != SUCCESSFUL_EXIT) break;
            const dim3 gk((unsigned)nblk, (unsigned)C), gconj((unsigned)((n / 2 + 255) / 256), (unsigned)C);
            if (conj_pairs) hipLaunchKernelGGL(k_tr_conj_cols, gconj, b256, 0, STREAM, n, d_ub_vec + 3 * (size_t)ub_cols * n, (int64_t)n, all, C);
            hipLaunchKernelGGL(k_kryb_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)nullptr, (int64_t)0, (const double *)nullptr, (int64_t)0, d_xx, xstr, 0u, all); // x = 0

            // R_c = B_c - A_new X_c and its two sums for the columns of `mask`, on the host after one synchronisation
            auto residual = [&](uint32_t mask) -> int32_t {
                O::residual_blk(*this, STREAM, (int64_t)n, (const double *)d_xx, xstr, d_bb, bstr, d_r, C, mask, d_rpart, rpcol);
                hipLaunchKernelGGL(k_kryb_reduce, dim3(2, (unsigned)C), b256, 0, STREAM, (const double *)d_rpart, rpcol, O::blocks(*this), mask, d_res, (int64_t)2);
                HIPC(hipMemcpyAsync(h_res, d_res, 2 * (size_t)C * sizeof(double), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
                HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
                return SUCCESSFUL_EXIT;
            };
            // X_c += Z_c y_c over the first kc[c] directions for the columns of `mask` (h_y, h_ub_cnt filled by the caller; no synchronisation:
            // the residual that follows brings it)
            auto combine = [&](uint32_t mask) -> int32_t {
                HIPC(hipMemcpyAsync(d_y, h_y, sizeof(double) * (size_t)C * ystr, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
                HIPC(hipMemcpyAsync(d_ub_cnt, h_ub_cnt, sizeof(int32_t) * (size_t)C, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
                P::combine_blk(gk, STREAM, (int64_t)n, d_xx, xstr, (const double *)d_ub_Z, vstr, mask, (const int32_t *)d_ub_cnt, (const double *)d_y, ystr);
                return SUCCESSFUL_EXIT;
            };

            // per column of the block
            double bnorm[KRYB_COLS], rnorm[KRYB_COLS];
            int32_t steps[KRYB_COLS], kc[KRYB_COLS];
            bool nan_rhs[KRYB_COLS];
            uint32_t done = 0; // finished for the rest of the call
            code = residual(all);
            if (code != SUCCESSFUL_EXIT) break;
            for (int32_t c = 0; c < C; c++) {
                const double rr = h_res[2 * c], bb = h_res[2 * c + 1];
                steps[c] = 0, nan_rhs[c] = false, bnorm[c] = 0.0, rnorm[c] = 0.0;
                if (bb == 0.0) done |= 1u << c; // x_c = 0
                else if (!std::isfinite(bb)) done |= 1u << c, nan_rhs[c] = true;
                else {
                    bnorm[c] = sqrt(bb), rnorm[c] = sqrt(rr);
                    if (!(rnorm[c] > par.tol * bnorm[c])) done |= 1u << c;
                }
            }
            while (done != all) {
                updated_cycles++;
                // v_0 = r / |r| for the columns still at work, zeros for the others (d_res holds |r_c|^2 of every such column's last residual)
                hipLaunchKernelGGL(k_kryb_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)d_r, (int64_t)n, (const double *)d_res, (int64_t)2, (double *)d_ub_V, (int64_t)n,
                                   all & ~done, done);
                uint32_t parked = done; // ... for the rest of this cycle
                for (int32_t c = 0; c < C; c++) {
                    kc[c] = 0;
                    if ((done >> c) & 1u) continue;
                    lsq[(size_t)c].reset(rnorm[c]);
                }
                for (int32_t k = 0; k < m && parked != all; k++) {
                    const uint32_t act = all & ~parked;
                    double *const zk = d_ub_Z + (size_t)k * vstr;
                    const double *const vk = d_ub_V + (size_t)k * vstr;
                    timer.mark(0);
                    code = O::precond(*this, zk, vk, C); // Z_k = M^{-1} V_k: one blocked pass pair
                    if (code != SUCCESSFUL_EXIT) break;
                    timer.mark(1);
                    O::product_blk(*this, STREAM, (int64_t)n, (const double *)zk, d_w, C, act); // W = A_new Z_k
                    timer.mark(2);
                    const int32_t nv = k + 1;
                    const int64_t rstr = 2 * (int64_t)D * nv + 2; // the step's record of a column: both coefficient sets, the two squared norms
                    double *const d_nrm = d_rec + 2 * (size_t)D * nv;
                    for (int32_t round = 0; round < 2; round++) { // CGS2
                        double *const hr = d_rec + (size_t)round * D * nv;
                        P::dots_blk(gk, STREAM, (int64_t)n, (const double *)d_w, (const double *)d_ub_V, vstr, nv, act, (double *)d_ub_part, pcol);
                        hipLaunchKernelGGL(k_kryb_reduce, dim3((unsigned)(D * nv), (unsigned)C), b256, 0, STREAM, (const double *)d_ub_part, pcol, nblk, act, hr, rstr);
                        P::update_blk(gk, STREAM, (int64_t)n, d_w, (const double *)d_ub_V, vstr, nv, act, (const double *)hr, rstr, (double *)d_ub_part, pcol);
                        hipLaunchKernelGGL(k_kryb_reduce, dim3(1, (unsigned)C), b256, 0, STREAM, (const double *)d_ub_part, pcol, nblk, act, d_nrm + round, rstr);
                    }
                    double *const vnext = d_ub_V + (size_t)(k + 1) * vstr;
                    hipLaunchKernelGGL(k_kryb_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)d_w, (int64_t)n, (const double *)(d_nrm + 1), rstr, vnext, (int64_t)n,
                                       act, parked);
                    timer.mark(3);
                    if (hipMemcpyAsync(h_rec, d_rec, sizeof(double) * (size_t)C * rstr, hipMemcpyDeviceToHost, STREAM) != hipSuccess) code = ERROR_HIP_MEMCPY;
                    if (code == SUCCESSFUL_EXIT && hipStreamSynchronize(STREAM) != hipSuccess) code = ERROR_HIP_SYNCHRONIZE;
                    if (code != SUCCESSFUL_EXIT) break;
                    timer.add(updated_ms);
                    uint32_t newly = 0;
                    bool counted = false;
                    for (int32_t c = 0; c < C; c++) {
                        if (!((act >> c) & 1u)) continue;
                        const double *const rec = h_rec + (size_t)c * rstr;
                        bool finite = true;
                        for (int32_t j = 0; j < rstr; j++) finite = finite && std::isfinite(rec[j]);
                        if (!finite) { // (the column leaves the cycle with the directions before this one; the step is not counted for it)
                            newly |= 1u << c;
                            continue;
                        }
                        steps[c]++, updated_column_steps++, counted = true;
                        memcpy(crec.data(), rec, sizeof(T) * 2 * nv); // the new Hessenberg column: the coefficients of the two rounds, added
                        for (int32_t j = 0; j < nv; j++) hcol[(size_t)j] = crec[(size_t)j] + crec[(size_t)(nv + j)];
                        const double hn = sqrt(rec[rstr - 1]);
                        lsq[(size_t)c].push(k, hcol.data(), hn);
                        const double est = std::abs(lsq[(size_t)c].g[(size_t)k + 1]);
                        if (guard.verbose)
                            fprintf(stderr, "hipmf: %s%s: column %d cycle %lld step %d: residual estimate %.3e (|b| = %.3e)\n", P::label_many, O::tag, j0 + c, (long long)updated_cycles, k + 1, est,
                                    bnorm[c]);
                        kc[c] = k + 1;
                        if (est <= par.tol * bnorm[c] || !(hn > 0.0) || steps[c] >= par.step_limit) newly |= 1u << c;
                    }
                    if (counted) updated_steps++;
                    parked |= newly;
                    // a column parked by this step: its next basis vector (written before the host knew) becomes zeros
                    if (newly && parked != all && k + 1 < m)
                        hipLaunchKernelGGL(k_kryb_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)nullptr, (int64_t)0, (const double *)nullptr, (int64_t)0, vnext, (int64_t)n, 0u, newly);
                }
                if (code != SUCCESSFUL_EXIT) break;
                // the end of the cycle: per column the back substitution over its own directions
                uint32_t moved = 0;
                for (int32_t c = 0; c < C; c++) {
                    h_ub_cnt[c] = 0;
                    if ((done >> c) & 1u) continue;
                    if (kc[c] == 0) { // (not one usable direction: the column ends with what it has)
                        done |= 1u << c;
                        continue;
                    }
                    lsq[(size_t)c].solve(kc[c], y.data());
                    memcpy(h_y + (size_t)c * ystr, y.data(), sizeof(T) * (size_t)kc[c]);
                    h_ub_cnt[c] = kc[c];
                    moved |= 1u << c;
                }
                if (!moved) continue;
                code = combine(moved);
                if (code == SUCCESSFUL_EXIT) code = residual(moved);
                if (code != SUCCESSFUL_EXIT) break;
                uint32_t back = 0;
                for (int32_t c = 0; c < C; c++) {
                    if (!((moved >> c) & 1u)) continue;
                    const double now = sqrt(h_res[2 * c]);
                    if (guard.verbose) fprintf(stderr, "hipmf: %s%s: column %d cycle %lld: |r| %.3e -> %.3e\n", P::label_many, O::tag, j0 + c, (long long)updated_cycles, rnorm[c], now);
                    if (!(now < rnorm[c])) { // no gain (or not a number): the column's cycle is taken back, x_c is the best iterate
                        back |= 1u << c, done |= 1u << c;
                        continue;
                    }
                    rnorm[c] = now;
                    if (!(rnorm[c] > par.tol * bnorm[c]) || steps[c] >= par.step_limit) done |= 1u << c;
                }
                if (back) {
                    for (int32_t c = 0; c < C; c++)
                        if ((back >> c) & 1u)
                            for (int32_t j = 0; j < D * kc[c]; j++) h_y[(size_t)c * ystr + j] = -h_y[(size_t)c * ystr + j];
                    code = combine(back);
                    if (code == SUCCESSFUL_EXIT) code = residual(back);
                    if (code != SUCCESSFUL_EXIT) break;
                    for (int32_t c = 0; c < C; c++)
                        if ((back >> c) & 1u) rnorm[c] = sqrt(h_res[2 * c]);
                }
            }
            if (code != SUCCESSFUL_EXIT) break;
            if (conj_pairs) { // (a column without a step is the zeros of the entry, kept +0.0 as the other forms return them)
                uint32_t stepped = 0;
                for (int32_t c = 0; c < C; c++)
                    if (steps[c] > 0) stepped |= 1u << c;
                if (stepped) hipLaunchKernelGGL(k_tr_conj_cols, gconj, b256, 0, STREAM, n, d_xx, xstr, stepped, C);
            }
            for (int32_t c = 0; c < C; c++) {
                const double rel = nan_rhs[c] ? NAN : (bnorm[c] > 0.0 ? rnorm[c] / bnorm[c] : 0.0);
                if (steps_out) steps_out[j0 + c] = steps[c];
                if (relres_out) relres_out[j0 + c] = rel;
                if (nan_rhs[c] || (bnorm[c] > 0.0 && !(rnorm[c] <= par.tol * bnorm[c]))) all_converged = false;
                if (!on_device && hipMemcpyAsync(x + (int64_t)(j0 + c) * ld, d_xx + (size_t)c * n, nb, hipMemcpyDeviceToHost, STREAM) != hipSuccess) code = ERROR_HIP_MEMCPY;
            }
            if (code == SUCCESSFUL_EXIT && hipStreamSynchronize(STREAM) != hipSuccess) code = ERROR_HIP_SYNCHRONIZE; // (the staging blocks are the next block's)
        }
    }
    if (code != SUCCESSFUL_EXIT) return code;
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    return all_converged ? SUCCESSFUL_EXIT : WARNING_NOT_CONVERGED;
}

// ---- extra-precise iterative refinement (solver_hipmf_solve_extra_precise; kernels_refine_extra.hpp) ----
// solve() refines on a residual computed in working precision and stops on the backward error: its x is backward stable, its forward
// error about cond(A) eps.  Here the residual is accumulated in twice the working precision and rounded once, and the iteration watches
// the corrections themselves (Demmel, Hida, Kahan, Li, Mukherjee & Riedy 2006; LAPACK's xGERFSX): while cond(A) eps < 1 the forward
// error goes to the order of eps, normwise and componentwise, and dn / (1 - rho_max) bounds it.  Per column, in the user's space:
//   x <- one unrefined pass pair of b (solve_core with no refinement: k_perm_in, run_triangular under the device gate, k_perm_out), tail <- 0
//   step: r <- b - A (x + tail) (k_xr_residual_cols), dx <- one unrefined pass pair of r, then ONE launch (k_xr_update_cols) that leaves
//         max |dx|, max |x|, max |dx_i / x_i| of the x BEFORE the update, keeps that x (and tail) and applies x <- x + dx, with a tail
//         (x, tail) <- the renormalised TwoSum of x + dx + tail; the host reads the measures once per block step:
//         dn = |dx|_inf / |x|_inf, dc = max_i |dx_i| / |x_i|, rho = dn / dn of the step before
//   dn > dn of the step before, or a component that is not finite: the step is taken back, "no progress"; else, with the step applied:
//   dn <= dx_tol converged; not the first step and dn > dn_prev / 2 "no progress"; max_steps steps "step limit".
// The columns of a block of XR_COLS share the pass pairs, the pass over the matrix and the update launch; a finished column leaves the
// mask: its residual column is zeros and it rides along through the pass pairs.  A column with b = 0 is x = 0 in no step.
// One core serves the real and the complex handle; P gives the update launch (the complex handle's measures take moduli of pairs).
namespace {
constexpr int32_t XR_COLS = 16;
struct ExtraReal {
    static constexpr auto update = k_xr_update_cols<false>;
    static constexpr int32_t W = 1; // doubles per component
    static constexpr const char *label = "solve_extra_precise";
};
struct ExtraPairs {
    static constexpr auto update = k_xr_update_cols<true>;
    static constexpr int32_t W = 2;
    static constexpr const char *label = "solve_extra_precise (complex)";
};
} // namespace

template <class P>
int32_t Solver::solve_extra_precise_core(double *x, double *tail, const double *rhs, int32_t nrhs, int64_t ld, double dx_tol, int32_t max_steps, double *info,
                                         bool on_device) {
    DeviceScope dev_scope(device);
    const int32_t n = S.n, items = n / P::W;
    const double EPS = 2.220446049250313e-16;
    const double tol = dx_tol > 0.0 ? dx_tol : EPS;
    const int32_t limit = max_steps > 0 ? max_steps : 10;
    const double bound_floor = tail ? 0.0 : std::max(10.0, sqrt((double)items)) * EPS; // (x alone cannot be nearer than its own rounding)
    const StepTimer timer{xr_ev, STREAM, Tunables::now(&Tunables::extra_timing)};
    extra_steps = extra_blocks = 0;
    extra_ms[0] = extra_ms[1] = extra_ms[2] = 0.0;
    if (info)
        for (int64_t k = 0; k < 8 * (int64_t)nrhs; k++) info[k] = 0.0;

    const int32_t C = std::min(nrhs, XR_COLS);
    if (xr_cols < C) {
        xr_cols = 0;
        HIPC(d_xr_vec.alloc(7 * (size_t)n * C), ERROR_HIP_MALLOC);
        HIPC(d_xr_nrm.alloc((size_t)XR_NORM_WORDS * C), ERROR_HIP_MALLOC);
        HIPC(h_xr_nrm.alloc((size_t)XR_NORM_WORDS * C), ERROR_HIP_MALLOC);
        xr_cols = C;
    }
    HIPC(timer.create(), ERROR_HIP_SYNCHRONIZE);
    const size_t blk = (size_t)n * xr_cols, nb = sizeof(double) * (size_t)n;
    double *const d_R = d_xr_vec, *const d_DX = d_xr_vec + blk, *const d_XS = d_xr_vec + 2 * blk, *const d_TS = d_xr_vec + 3 * blk;
    const dim3 b256(256), gu((unsigned)std::max(1, std::min((items + 255) / 256, 1024)));
    const int64_t stride = on_device ? ld : (int64_t)n;

    // the maxima over the slots of column c: word w of k_xr_update_cols
    auto slot_max = [&](int32_t c, int32_t w) {
        double m = 0.0;
        for (int32_t sl = 0; sl < RES_SLOTS; sl++) m = std::max(m, h_xr_nrm[(size_t)XR_NORM_WORDS * c + (size_t)sl * RES_SLOT_WORDS + w]);
        return m;
    };
    const NestedSolveGuard guard(*this);
    guard.unrefined_quiet();
    bool all_converged = true;
    for (int32_t j0 = 0; j0 < nrhs; j0 += XR_COLS) {
        const int32_t nk = std::min(XR_COLS, nrhs - j0);
        extra_blocks++;
        double *const xb = on_device ? x + (int64_t)j0 * ld : d_xr_vec + 4 * blk;
        double *const tb = !tail ? nullptr : (on_device ? tail + (int64_t)j0 * ld : d_xr_vec + 5 * blk);
        const double *bb = on_device ? rhs + (int64_t)j0 * ld : d_xr_vec + 6 * blk;
        if (!on_device)
            for (int32_t c = 0; c < nk; c++)
                HIPC(hipMemcpyAsync(d_xr_vec + 6 * blk + (size_t)c * n, rhs + (int64_t)(j0 + c) * ld, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        const uint32_t all = nk >= 32 ? ~0u : ((1u << nk) - 1u);
        const size_t nrm_bytes = (size_t)XR_NORM_WORDS * nk * sizeof(unsigned long long);
        // max |b_i| per column (measures only: nothing is written through the pointer)
        HIPC(hipMemsetAsync(d_xr_nrm, 0, nrm_bytes, STREAM), ERROR_HIP_MEMCPY);
        hipLaunchKernelGGL(P::update, dim3(gu.x, nk), b256, 0, STREAM, n, const_cast<double *>(bb), (double *)nullptr, stride, (const double *)nullptr, (int64_t)0,
                           (double *)nullptr, (double *)nullptr, (int64_t)0, (unsigned long long *)d_xr_nrm, all);
        HIPC(hipMemcpyAsync(h_xr_nrm, d_xr_nrm, nrm_bytes, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        int32_t code = solve_core(xb, bb, nk, stride, true); // the start (ends with the stream drained: the norms of b are here)
        if (code != SUCCESSFUL_EXIT) return code;
        struct Column {
            bool active = false;
            int32_t steps = 0, state = 0;
            double dn_prev = INFINITY, dn = 0.0, dc = 0.0, rho_max = 0.0;
            bool applied = false, zero = false;
        } col[XR_COLS];
        uint32_t mask = 0;
        for (int32_t c = 0; c < nk; c++) {
            if (tb) HIPC(hipMemsetAsync(tb + (int64_t)c * stride, 0, nb, STREAM), ERROR_HIP_MEMCPY);
            if (slot_max(c, 1) == 0.0 && slot_max(c, 3) == 0.0) { // b = 0: x = 0, no step
                col[c].zero = true;
                HIPC(hipMemsetAsync(xb + (int64_t)c * stride, 0, nb, STREAM), ERROR_HIP_MEMCPY);
            } else {
                col[c].active = true, mask |= 1u << c;
            }
        }
        for (int32_t it = 1; mask != 0; it++) {
            timer.mark(0);
            if (tb)
                hipLaunchKernelGGL(k_xr_residual_cols<true>, dim3(spmv_blocks), b256, 0, STREAM, d_row_blk, d_rp, d_ci, d_vals, d_tptr, d_tidx, d_arow, (const double *)xb,
                                   (const double *)tb, stride, bb, stride, d_R, (int64_t)n, nk, mask);
            else
                hipLaunchKernelGGL(k_xr_residual_cols<false>, dim3(spmv_blocks), b256, 0, STREAM, d_row_blk, d_rp, d_ci, d_vals, d_tptr, d_tidx, d_arow, (const double *)xb,
                                   (const double *)nullptr, stride, bb, stride, d_R, (int64_t)n, nk, mask);
            timer.mark(1);
            code = solve_core(d_DX, d_R, nk, n, true);
            if (code != SUCCESSFUL_EXIT) return code;
            timer.mark(2);
            HIPC(hipMemsetAsync(d_xr_nrm, 0, nrm_bytes, STREAM), ERROR_HIP_MEMCPY);
            hipLaunchKernelGGL(P::update, dim3(gu.x, nk), b256, 0, STREAM, n, xb, tb, stride, (const double *)d_DX, (int64_t)n, d_XS, tb ? d_TS : (double *)nullptr, (int64_t)n,
                               (unsigned long long *)d_xr_nrm, mask);
            timer.mark(3);
            HIPC(hipMemcpyAsync(h_xr_nrm, d_xr_nrm, nrm_bytes, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
            timer.add(extra_ms);
            extra_steps++;
            for (int32_t c = 0; c < nk; c++) {
                Column &k = col[c];
                if (!k.active) continue;
                k.steps = it;
                const double mdx = slot_max(c, 0), mx = slot_max(c, 1);
                const double dn = mdx == 0.0 ? 0.0 : (mx > 0.0 ? mdx / mx : INFINITY), dc = slot_max(c, 2);
                if (guard.verbose && j0 + c == 0) fprintf(stderr, "hipmf: %s: step %d: dn = %.3e, dc = %.3e\n", P::label, it, dn, dc);
                if (slot_max(c, 3) != 0.0 || dn > k.dn_prev) { // not a number somewhere, or a larger correction than the last: taken back
                    HIPC(hipMemcpyAsync(xb + (int64_t)c * stride, d_XS + (size_t)c * n, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
                    if (tb) HIPC(hipMemcpyAsync(tb + (int64_t)c * stride, d_TS + (size_t)c * n, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
                    k.state = 1, k.active = false;
                    continue;
                }
                if (k.applied) k.rho_max = std::max(k.rho_max, k.dn_prev > 0.0 ? dn / k.dn_prev : 0.0);
                k.dn = dn, k.dc = dc;
                if (dn <= tol) k.state = 0, k.active = false;
                else if (k.applied && dn > 0.5 * k.dn_prev) k.state = 1, k.active = false;
                else if (it >= limit) k.state = 2, k.active = false;
                k.applied = true, k.dn_prev = dn;
            }
            mask = 0;
            for (int32_t c = 0; c < nk; c++)
                if (col[c].active) mask |= 1u << c;
        }
        for (int32_t c = 0; c < nk; c++) {
            const Column &k = col[c];
            all_converged = all_converged && k.state == 0;
            if (info && !k.zero) {
                double *const o = info + 8 * (size_t)(j0 + c);
                // (no applied step, or corrections that do not contract: nothing bounds the error)
                const double scale = (k.applied && k.rho_max < 1.0) ? 1.0 / (1.0 - k.rho_max) : INFINITY;
                o[0] = k.steps, o[1] = k.dn, o[2] = std::max(k.dn * scale, bound_floor), o[3] = k.dc, o[4] = std::max(k.dc * scale, bound_floor);
                o[5] = k.rho_max, o[6] = k.state, o[7] = tail ? 1.0 : 0.0;
            }
            if (!on_device) {
                HIPC(hipMemcpyAsync(x + (int64_t)(j0 + c) * ld, xb + (size_t)c * n, nb, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
                if (tb) HIPC(hipMemcpyAsync(tail + (int64_t)(j0 + c) * ld, tb + (size_t)c * n, nb, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
            }
        }
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE); // (the staging blocks are the next block's)
    }
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    return all_converged ? SUCCESSFUL_EXIT : WARNING_NOT_CONVERGED;
}

int32_t Solver::solve_extra_precise(double *x, double *tail, const double *rhs, int32_t nrhs, int64_t ld, double dx_tol, int32_t max_steps, double *info, bool on_device,
                                    bool pairs) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs) return ERROR_NULL_POINTER;
    if (nrhs < 1 || ld < S.n || (pairs && (S.n & 1))) return ERROR_HIPMF_INVALID_VALUE;
    return pairs ? solve_extra_precise_core<ExtraPairs>(x, tail, rhs, nrhs, ld, dx_tol, max_steps, info, on_device)
                 : solve_extra_precise_core<ExtraReal>(x, tail, rhs, nrhs, ld, dx_tol, max_steps, info, on_device);
}

// ---- bordered systems on the kept factor (solver_hipmf_set_border, solver_hipmf_solve_bordered; kernels_border.hpp) ----
//     [ A   B ] [x]   [f]
//     [ C^T D ] [z] = [g]      B, C: n x k dense, D: k x k dense, k <= BORDER_MAX
// Block elimination with W = A^{-1} B and S = D - C^T W needs one pass pair per right-hand side, but with an ill-conditioned A (near a
// fold: the case bordering exists for) it loses cond(A) eps even when every solve with A is refined on its own.  Iterative refinement
// on the bordered system as a whole, with the elimination as the approximate inverse, repairs that (Govaerts & Pryce 1993; Govaerts,
// Numerical Methods for Bifurcations of Dynamical Equilibria, 2000, ch. 3).  Per block of BORDER_COLS columns, in the user's space:
//   eliminate(r_f, r_g): y <- one unrefined pass pair of r_f (solve_core without refinement under the nested solve guard),
//                        t <- r_g - C^T y (k_border_gram + k_border_reduce), dz <- S^{-1} t (k_border_small_solve), dx <- y - W dz (k_border_apply)
//   start: (x, z) <- eliminate(f, g)
//   measure: r_f = f - A x - B z with den = |A||x| + |B||z| + |f| (k_border_residual_n), r_g = g - C^T x - D z with den =
//            |C|^T|x| + |D||z| + |g| (k_border_rows_part, k_border_rows), every row accumulated beyond twice the working precision and
//            rounded once (why: kernels_border.hpp); ONE host read of the omegas of the block's columns, omega = the maximum over all n + k rows
//   the rule of solve() per column: omega <= eps converged; a step that did not lower omega is taken back, "no progress"; a step that
//   did not halve it stays, "no progress"; max_steps steps "step limit"; else (x, z) += eliminate(r_f, r_g), the old (x, z) kept.
// A finished column leaves the mask: its residual columns are zeros through the next pass pair, the correction leaves it alone.
namespace {
// the border in force is given up unless the call that sets it reaches its end
struct BorderUndo {
    Solver &s;
    bool keep = false;
    ~BorderUndo() {
        if (!keep) s.drop_border();
    }
};
} // namespace

void Solver::drop_border() {
    DeviceScope dev_scope(device);
    static_cast<SolverBorder &>(*this) = SolverBorder();
}

// pairs: the border of the complex twin (kernels_border_complex.hpp).  kc complex columns are k = 2 kc packed real-equivalent ones -- the
// interleaved column and its partner, every pair rotated --; C is packed conjugated, so that the Gram product with it is C^T; W = A^{-1} B
// takes kc solves of interleaved columns, not 2 kc; S = D - C^T W stays a complex kc x kc matrix and is factorised as one.
int32_t Solver::set_border(int32_t kc, const double *B, int64_t ldb, const double *C, int64_t ldc, const double *D, int64_t ldd, double *info, bool on_device,
                           bool pairs) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (kc < 0 || kc > (pairs ? ZBORDER_MAX : BORDER_MAX) || (pairs && (S.n & 1))) return ERROR_HIPMF_INVALID_VALUE;
    const int32_t k = pairs ? 2 * kc : kc; // real(-equivalent) border columns
    if (info) info[0] = info[1] = info[2] = info[3] = 0.0, info[pairs ? 4 : 3] = 0.0;
    if (k == 0) {
        drop_border();
        return SUCCESSFUL_EXIT;
    }
    if (!B || !C || !D) return ERROR_NULL_POINTER;
    const int32_t n = S.n;
    if (ldb < n || ldc < n || ldd < k) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    drop_border();
    BorderUndo undo{*this};
    const int32_t kp = (k + 15) / 16 * 16, nch = (n + BORDER_CHUNK - 1) / BORDER_CHUNK;
    const size_t npk = (size_t)n * kp, kk2 = (size_t)kp * kp, tile = (size_t)kp * BORDER_COLS, nb = sizeof(double) * (size_t)n;
    DeviceArray<double> d_cols, d_wcol, d_gs; // the border's columns as they came (C, then B), a block of W, C^T W
    HIPC(d_bd_B.alloc(npk), ERROR_HIP_MALLOC);
    HIPC(d_bd_C.alloc(npk), ERROR_HIP_MALLOC);
    HIPC(d_bd_W.alloc(npk), ERROR_HIP_MALLOC);
    HIPC(d_bd_D.alloc(kk2), ERROR_HIP_MALLOC);
    HIPC(d_bd_LU.alloc(kk2), ERROR_HIP_MALLOC);
    HIPC(d_bd_piv.alloc((size_t)kp), ERROR_HIP_MALLOC);
    HIPC(d_bd_rec.alloc(BORDER_REC), ERROR_HIP_MALLOC);
    HIPC(d_bd_part.alloc(BORDER_PART * (size_t)nch * tile), ERROR_HIP_MALLOC); // (the widest user: k_border_rows_part)
    HIPC(d_cols.alloc((size_t)n * kc), ERROR_HIP_MALLOC);
    HIPC(d_wcol.alloc((size_t)n * BORDER_COLS), ERROR_HIP_MALLOC);
    HIPC(d_gs.alloc(kk2), ERROR_HIP_MALLOC);
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const dim3 b256(256);
    HIPC(hipMemsetAsync(d_bd_B, 0, sizeof(double) * npk, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(d_bd_C, 0, sizeof(double) * npk, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(d_bd_W, 0, sizeof(double) * npk, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(d_bd_D, 0, sizeof(double) * kk2, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(d_bd_piv, 0, sizeof(int32_t) * (size_t)kp, STREAM), ERROR_HIP_MEMCPY);
    // columns [j0, j0 + nk) of `to` from the columns of `from` as they came: nk (complex) columns, n doubles apart
    auto pack = [&](const double *from, int32_t j0, int32_t nk, int32_t conj, double *to) {
        if (pairs)
            hipLaunchKernelGGL(k_zborder_pack, dim3((unsigned)(((int64_t)(n / 2) * nk + 255) / 256)), b256, 0, STREAM, n / 2, nk, kp, j0, from, (int64_t)n, conj, to);
        else
            hipLaunchKernelGGL(k_border_pack, dim3((unsigned)(((int64_t)n * nk + 255) / 256)), b256, 0, STREAM, n, nk, kp, j0, from, (int64_t)n, to);
    };
    for (int32_t j = 0; j < kc; j++) {
        HIPC(hipMemcpyAsync(d_cols + (size_t)j * n, C + (int64_t)j * ldc, nb, in, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipMemcpyAsync(d_bd_D + (size_t)j * kp, D + (int64_t)j * ldd, sizeof(double) * (size_t)k, in, STREAM), ERROR_HIP_MEMCPY);
    }
    pack(d_cols, 0, kc, 1, d_bd_C); // (pairs: conj(C), whose real-equivalent form transposed is that of C^T)
    for (int32_t j = 0; j < kc; j++) HIPC(hipMemcpyAsync(d_cols + (size_t)j * n, B + (int64_t)j * ldb, nb, in, STREAM), ERROR_HIP_MEMCPY);
    pack(d_cols, 0, kc, 0, d_bd_B);
    {
        const NestedSolveGuard guard(*this); // (W comes from ordinary refined solves: their statistics are not the caller's)
        for (int32_t j0 = 0; j0 < kc; j0 += BORDER_COLS) {
            const int32_t nk = std::min(BORDER_COLS, kc - j0);
            const int32_t code = solve(d_wcol, d_cols + (size_t)j0 * n, nk, n, true);
            if (code != SUCCESSFUL_EXIT) return code;
            pack(d_wcol, j0, nk, 0, d_bd_W);
            // (pairs: C^T W of nk interleaved columns comes out interleaved, kp doubles per complex column of S)
            hipLaunchKernelGGL(k_border_gram, dim3((unsigned)nch, (unsigned)(kp / 16)), dim3(64), 0, STREAM, n, kp, (const double *)d_bd_C, (const double *)d_wcol,
                               (int64_t)n, nk, (double *)d_bd_part);
            hipLaunchKernelGGL(k_border_reduce, dim3((unsigned)kp), b256, 0, STREAM, nch, kp, (const double *)d_bd_part, d_gs + (size_t)j0 * kp);
        }
    }
    if (pairs)
        hipLaunchKernelGGL(k_zborder_lu, dim3(1), b256, 0, STREAM, kc, kp, (const double *)d_bd_D, (const double *)d_gs, (double *)d_bd_LU, (int32_t *)d_bd_piv,
                           (double *)d_bd_rec);
    else
        hipLaunchKernelGGL(k_border_lu, dim3(1), b256, 0, STREAM, k, kp, (const double *)d_bd_D, (const double *)d_gs, (double *)d_bd_LU, (int32_t *)d_bd_piv,
                           (double *)d_bd_rec);
    double rec[BORDER_REC];
    HIPC(hipMemcpyAsync(rec, d_bd_rec, sizeof rec, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    if (rec[4] != 0.0) return WARNING_SINGULAR_MATRIX; // (an exactly zero pivot of S: no border is left set)
    bd_k = k, bd_kp = kp, bd_chunks = nch, bd_pairs = pairs;
    bd_bytes = (int64_t)(sizeof(double) * (3 * npk + 2 * kk2 + BORDER_PART * (size_t)nch * tile + BORDER_REC) + sizeof(int32_t) * (size_t)kp);
    if (info && pairs) info[0] = rec[1] > 0.0 ? rec[0] / rec[1] : 0.0, info[1] = rec[2], info[2] = rec[5], info[3] = rec[3], info[4] = (double)bd_bytes;
    if (info && !pairs) info[0] = rec[1] > 0.0 ? rec[0] / rec[1] : 0.0, info[1] = rec[2], info[2] = rec[3], info[3] = (double)bd_bytes;
    if (opt.verbose && pairs)
        fprintf(stderr, "hipmf: set_border (complex): k = %d, min / max |u_ii| of S = %.3e, det S = (%.6f %+.6f i) x 10^%.0f, %.1f MB on the device\n", kc,
                rec[1] > 0.0 ? rec[0] / rec[1] : 0.0, rec[2], rec[5], rec[3], 1e-6 * (double)bd_bytes);
    if (opt.verbose && !pairs)
        fprintf(stderr, "hipmf: set_border: k = %d, min / max |u_ii| of S = %.3e, det S = %.6f x 10^%.0f, %.1f MB on the device\n", k, rec[1] > 0.0 ? rec[0] / rec[1] : 0.0,
                rec[2], rec[3], 1e-6 * (double)bd_bytes);
    undo.keep = true;
    return SUCCESSFUL_EXIT;
}

// The transposed form, [A^T C; B^T D^T] [y; w] = [p; q] (T of bordered_core), is the same loop with the operands swapped: V = A^{-T} C for W
// and the transposed pass pair for the plain one (bt_pass), B for C in the Gram product and the border rows, S^T = D^T - B^T V through the
// LU of S (k_border_small_solve_t), the packed D^T for D, and the n rows of the residual through the rows of A^T, the block's columns four
// at a time (k_border_residual_nt; on a handle where A^T = A, k_border_residual_n with C for B).  V and D^T are built at the first
// transposed call after a set_border (bt_prepare).  With T false nothing is allocated or launched that the plain form did not before.
template <bool T>
int32_t Solver::bordered_core(double *x, double *z, const double *f, const double *g, int32_t nrhs, int64_t ldx, int64_t ldz, int32_t max_steps, double *info,
                              bool on_device, bool conj_pairs) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !f) return ERROR_NULL_POINTER;
    const int32_t n = S.n, k = bd_k, kp = bd_kp, nch = bd_chunks;
    if (k < 1 || nrhs < 1 || ldx < n || ((z || g) && ldz < k)) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    const double EPS = 2.220446049250313e-16;
    const int32_t limit = max_steps > 0 ? max_steps : 4;
    int64_t &steps_done = T ? bordered_t_steps : bordered_steps, &blocks_done = T ? bordered_t_blocks : bordered_blocks;
    steps_done = blocks_done = 0;
    if (info)
        for (int64_t q = 0; q < 4 * (int64_t)nrhs; q++) info[q] = 0.0;
    if (T) {
        const int32_t code = bt_prepare();
        if (code != SUCCESSFUL_EXIT) return code;
    }
    const bool a_is_at = S.sym_mode || d_tptr; // A^T = A: the plain pass pair and the plain rows serve the transposed form
    // what the elimination multiplies with (the Gram product and the border rows; the correction), and the small diagonal block
    const double *const d_gram = T ? (const double *)d_bd_B : (const double *)d_bd_C, *const d_corr = T ? (const double *)d_bt_V : (const double *)d_bd_W;
    const double *const d_diag = T ? (const double *)d_bt_Dt : (const double *)d_bd_D;
    const double *const d_side = T ? (const double *)d_bd_C : (const double *)d_bd_B; // the border columns in the first n rows
    // The border of the complex twin (bd_pairs; kernels_border_complex.hpp): the pass pairs, the Gram products and the corrections above
    // are those of the real-equivalent system with k = 2 kc packed columns; the small solve is complex (T: with the Schur complement of
    // M^H, the transposed real-equivalent system), the residual and its omegas run per complex row on moduli.  conj_pairs (T alone): M^T -- the
    // loop of M^H on conjugated data; right-hand sides and results of a device call are then staged as a host call's are.
    const bool Z = bd_pairs;
    if (conj_pairs && !(T && Z)) return ERROR_HIPMF_INVALID_VALUE;
    const bool staged = !on_device || conj_pairs;
    const int32_t C = std::min(nrhs, BORDER_COLS);
    const size_t tile = (size_t)kp * BORDER_COLS;
    if (bd_cols < C || bd_small_kp != kp) {
        bd_cols = 0;
        HIPC(d_bd_vec.alloc(5 * (size_t)n * C), ERROR_HIP_MALLOC);
        HIPC(d_bd_small.alloc(6 * tile), ERROR_HIP_MALLOC);
        HIPC(d_bd_nrm.alloc((size_t)RES_NORM_WORDS * C + BORDER_COLS), ERROR_HIP_MALLOC);
        HIPC(h_bd_nrm.alloc((size_t)RES_NORM_WORDS * C + BORDER_COLS), ERROR_HIP_MALLOC);
        bd_cols = C, bd_small_kp = kp;
    }
    const size_t blk = (size_t)n * bd_cols, nb = sizeof(double) * (size_t)n, kb = sizeof(double) * (size_t)k;
    double *const d_R = d_bd_vec, *const d_Y = d_bd_vec + blk, *const d_XS = d_bd_vec + 2 * blk;
    double *const d_GG = d_bd_small, *const d_Z = d_bd_small + tile, *const d_ZS = d_bd_small + 2 * tile, *const d_DZ = d_bd_small + 3 * tile;
    double *const d_RG = d_bd_small + 4 * tile, *const d_G = d_bd_small + 5 * tile;
    const dim3 b256(256), b64(64), gt((unsigned)((n + 63) / 64)), gg((unsigned)nch, (unsigned)(kp / 16));
    const int64_t stride = staged ? (int64_t)n : ldx;
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, out = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;

    const NestedSolveGuard guard(*this);
    guard.unrefined_quiet();
    for (int32_t j0 = 0; j0 < nrhs; j0 += BORDER_COLS) {
        const int32_t nk = std::min(BORDER_COLS, nrhs - j0);
        blocks_done++;
        double *const xb = staged ? d_bd_vec + 3 * blk : x + (int64_t)j0 * ldx;
        const double *const fb = staged ? d_bd_vec + 4 * blk : f + (int64_t)j0 * ldx;
        HIPC(hipMemsetAsync(d_bd_small, 0, sizeof(double) * 6 * tile, STREAM), ERROR_HIP_MEMCPY); // (the rows k .. kp - 1 stay zero: g = 0 without a g)
        for (int32_t c = 0; c < nk; c++) {
            if (staged) HIPC(hipMemcpyAsync(d_bd_vec + 4 * blk + (size_t)c * n, f + (int64_t)(j0 + c) * ldx, nb, in, STREAM), ERROR_HIP_MEMCPY);
            if (g) HIPC(hipMemcpyAsync(d_GG + (size_t)c * kp, g + (int64_t)(j0 + c) * ldz, kb, in, STREAM), ERROR_HIP_MEMCPY);
        }
        // conj_pairs: the imaginary parts of the block's n-vectors and of its vectors of order k negated (on the way in: p and q)
        auto conj_block = [&](double *vn, double *vk) {
            hipLaunchKernelGGL(k_tr_conj_cols, dim3((unsigned)((n / 2 + 255) / 256), (unsigned)nk), b256, 0, STREAM, n, vn, (int64_t)n, ~0u, nk);
            hipLaunchKernelGGL(k_tr_conj_cols, dim3(1, (unsigned)nk), b256, 0, STREAM, kp, vk, (int64_t)kp, ~0u, nk);
        };
        if (conj_pairs) conj_block(d_bd_vec + 4 * blk, d_GG);
        const size_t nrm_words = (size_t)RES_NORM_WORDS * nk + BORDER_COLS;
        unsigned long long *const d_nrm = d_bd_nrm;
        double *const d_omega_g = reinterpret_cast<double *>(d_nrm + (size_t)RES_NORM_WORDS * nk);
        const double *const h_omega_g = h_bd_nrm + (size_t)RES_NORM_WORDS * nk;
        uint32_t mask = nk >= 32 ? ~0u : ((1u << nk) - 1u);

        // (dx, dz) of the residual (rf, rg), dx = y - W dz with y left in ydst by the pass pair; fresh: (x, z) <- (dx, dz), else (x, z) += (dx, dz)
        auto eliminate = [&](double *ydst, int64_t ystr, const double *rf, const double *rg, bool fresh) -> int32_t {
            const int32_t code = T ? bt_pass(ydst, ystr, rf, ystr, nk) : solve_core(ydst, rf, nk, ystr, true);
            if (code != SUCCESSFUL_EXIT) return code;
            hipLaunchKernelGGL(k_border_gram, gg, b64, 0, STREAM, n, kp, d_gram, (const double *)ydst, ystr, nk, (double *)d_bd_part);
            hipLaunchKernelGGL(k_border_reduce, dim3((unsigned)kp), b256, 0, STREAM, nch, kp, (const double *)d_bd_part, d_G);
            if (Z) { // (T: the LU of S_T = D^H - B^H V, see bt_prepare)
                hipLaunchKernelGGL(k_zborder_small_solve, dim3((unsigned)nk), b64, 0, STREAM, k / 2, kp, T ? (const double *)d_bt_LU : (const double *)d_bd_LU,
                                   T ? (const int32_t *)d_bt_piv : (const int32_t *)d_bd_piv, rg, (const double *)d_G, d_DZ, d_Z, fresh ? (double *)nullptr : d_ZS, mask);
            } else if (T) {
                hipLaunchKernelGGL(k_border_small_solve_t, dim3((unsigned)nk), b64, 0, STREAM, k, kp, (const double *)d_bd_LU, (const int32_t *)d_bd_piv, rg,
                                   (const double *)d_G, d_DZ, d_Z, fresh ? (double *)nullptr : d_ZS, mask);
            } else {
                hipLaunchKernelGGL(k_border_small_solve, dim3((unsigned)nk), b64, 0, STREAM, k, kp, (const double *)d_bd_LU, (const int32_t *)d_bd_piv, rg,
                                   (const double *)d_G, d_DZ, d_Z, fresh ? (double *)nullptr : d_ZS, mask);
            }
            hipLaunchKernelGGL(k_border_apply, gt, b256, 0, STREAM, n, k, kp, d_corr, (const double *)d_DZ, nk, mask, (const double *)ydst, ystr, xb, stride,
                               fresh ? (double *)nullptr : d_XS, (int64_t)n);
            return SUCCESSFUL_EXIT;
        };
        // the residual of (x, z) over all n + k rows into (d_R, d_RG), the omegas of the columns of the mask to the host
        auto measure = [&]() -> int32_t {
            HIPC(hipMemsetAsync(d_nrm, 0, nrm_words * sizeof(unsigned long long), STREAM), ERROR_HIP_MEMCPY);
            if (Z) {
                const dim3 gz((unsigned)((n / 2 + 255) / 256));
                if (T)
                    hipLaunchKernelGGL(k_zborder_residual_nt, gz, b256, 0, STREAM, n / 2, d_ttptr, d_ttrow, d_ttmap, d_vals, k / 2, kp, d_side, (const double *)d_Z,
                                       (const double *)xb, stride, fb, stride, d_R, (int64_t)n, d_nrm, nk, mask);
                else
                    hipLaunchKernelGGL(k_zborder_residual_n, gz, b256, 0, STREAM, n / 2, d_rp, d_ci, d_vals, k / 2, kp, d_side, (const double *)d_Z, (const double *)xb,
                                       stride, fb, stride, d_R, (int64_t)n, d_nrm, nk, mask);
                hipLaunchKernelGGL(k_zborder_rows_part, dim3((unsigned)nch, (unsigned)nk), b256, 0, STREAM, n, kp, d_gram, (const double *)xb, stride, mask,
                                   (double *)d_bd_part);
                hipLaunchKernelGGL(k_zborder_rows, dim3((unsigned)nk), b64, 0, STREAM, k / 2, kp, nch, d_diag, (const double *)d_GG, (const double *)d_bd_part,
                                   (const double *)d_Z, d_RG, d_omega_g, mask);
                HIPC(hipMemcpyAsync(h_bd_nrm, d_nrm, nrm_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
                HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
                return SUCCESSFUL_EXIT;
            }
            if (T && !a_is_at) {
                hipLaunchKernelGGL(k_border_residual_nt, dim3((unsigned)((n + 255) / 256)), b256, 0, STREAM, n, d_ttptr, d_ttrow, d_ttmap, d_vals, k, kp, d_side,
                                   (const double *)d_Z, (const double *)xb, stride, fb, stride, d_R, (int64_t)n, d_nrm, nk, mask);
            } else {
                hipLaunchKernelGGL(k_border_residual_n, dim3((unsigned)((n + 255) / 256)), b256, 0, STREAM, n, d_rp, d_ci, d_vals, d_tptr, d_tidx, d_arow, k, kp, d_side,
                                   (const double *)d_Z, (const double *)xb, stride, fb, stride, d_R, (int64_t)n, d_nrm, nk, mask);
            }
            hipLaunchKernelGGL(k_border_rows_part, dim3((unsigned)nch, (unsigned)nk), b256, 0, STREAM, n, kp, d_gram, (const double *)xb, stride, mask, (double *)d_bd_part);
            hipLaunchKernelGGL(k_border_rows, dim3((unsigned)nk), b64, 0, STREAM, k, kp, nch, d_diag, (const double *)d_GG, (const double *)d_bd_part, (const double *)d_Z,
                               d_RG, d_omega_g, mask);
            HIPC(hipMemcpyAsync(h_bd_nrm, d_nrm, nrm_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
            return SUCCESSFUL_EXIT;
        };

        int32_t code = eliminate(xb, stride, fb, d_GG, true);
        if (code != SUCCESSFUL_EXIT) return code;
        struct Column {
            bool active = true;
            int32_t steps = 0, state = 0;
            double prev = INFINITY, omega = 0.0, omega0 = 0.0;
        } col[BORDER_COLS];
        for (int32_t it = 0; mask != 0; it++) {
            code = measure();
            if (code != SUCCESSFUL_EXIT) return code;
            for (int32_t c = 0; c < nk; c++) {
                Column &q = col[c];
                if (!q.active) continue;
                double omega = h_omega_g[c];
                for (int32_t sl = 0; sl < RES_SLOTS; sl++) omega = std::max(omega, h_bd_nrm[(size_t)RES_NORM_WORDS * c + (size_t)sl * RES_SLOT_WORDS + 1]);
                if (guard.verbose && j0 + c == 0) fprintf(stderr, "hipmf: %s: after %d step(s): omega = %.3e\n", T ? "solve_bordered_transpose" : "solve_bordered", it, omega);
                if (it == 0) q.omega0 = omega;
                if (it > 0 && !(omega < q.prev)) { // the step did not lower omega: taken back
                    HIPC(hipMemcpyAsync(xb + (int64_t)c * stride, d_XS + (size_t)c * n, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
                    HIPC(hipMemcpyAsync(d_Z + (size_t)c * kp, d_ZS + (size_t)c * kp, sizeof(double) * (size_t)kp, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
                    q.state = 1, q.active = false;
                    continue;
                }
                q.omega = omega;
                if (omega <= EPS) q.state = 0, q.active = false;
                else if (it > 0 && omega > 0.5 * q.prev) q.state = 1, q.active = false;
                else if (it >= limit) q.state = 2, q.active = false;
                else q.prev = omega;
            }
            mask = 0;
            for (int32_t c = 0; c < nk; c++)
                if (col[c].active) mask |= 1u << c, col[c].steps = it + 1;
            if (!mask) break;
            code = eliminate(d_Y, (int64_t)n, d_R, d_RG, false);
            if (code != SUCCESSFUL_EXIT) return code;
            steps_done++;
        }
        if (conj_pairs) conj_block(xb, d_Z); // (on the way out: y and w)
        for (int32_t c = 0; c < nk; c++) {
            const Column &q = col[c];
            if (info) {
                double *const o = info + 4 * (size_t)(j0 + c);
                o[0] = q.steps, o[1] = q.omega, o[2] = q.omega0, o[3] = q.state;
            }
            if (staged) HIPC(hipMemcpyAsync(x + (int64_t)(j0 + c) * ldx, xb + (size_t)c * n, nb, out, STREAM), ERROR_HIP_MEMCPY);
            if (z) HIPC(hipMemcpyAsync(z + (int64_t)(j0 + c) * ldz, d_Z + (size_t)c * kp, kb, out, STREAM), ERROR_HIP_MEMCPY);
        }
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE); // (the staging blocks are the next block's)
    }
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    return SUCCESSFUL_EXIT;
}

int32_t Solver::solve_bordered(double *x, double *z, const double *f, const double *g, int32_t nrhs, int64_t ldx, int64_t ldz, int32_t max_steps, double *info,
                               bool on_device) {
    return bordered_core<false>(x, z, f, g, nrhs, ldx, ldz, max_steps, info, on_device);
}

// ---- sensitivities with respect to the matrix values (kernels_sensitivity.hpp) ----
// J = J(x), A x = b: with lambda = A^{-T} dJ/dx the derivatives are dJ/db = lambda and dJ/da_ij = -lambda_i x_j on the pattern (adjoint,
// solve_adjoint); forward, dx = A^{-1} (db - dA x) (solve_tangent).  <dJ/dx, dx> = <grad, dvalues> + <lambda, db> ties the two together.
// The products are formed per STORED entry of the handle (values_outer) and carried to the order of the caller's values by the inverse
// of whatever staging a factorize applies to them (stage_values): the value map, the expansion of a mirrored lower triangle.
namespace {

// The inverse of a staging map.  Slot j of the handle's CSR reads the inputs idx[ptr[j] .. ptr[j + 1]) (ptr == nullptr: the one input
// idx[j]); input t is read by the slots inv_idx[inv_ptr[t] .. inv_ptr[t + 1]), ascending.  false: the map subtracts an input (~t: the
// real-equivalent form of a complex matrix, whose gradient is values_outer_complex's business).
bool invert_staging(int64_t nin, int64_t nslot, const int32_t *ptr, const int32_t *idx, std::vector<int32_t> &inv_ptr, std::vector<int32_t> &inv_idx) {
    const int64_t nmap = ptr ? ptr[nslot] : nslot;
    auto input = [&](int64_t q) { return idx[q]; };
    for (int64_t q = 0; q < nmap; q++)
        if (idx[q] < 0) return false;
    inv_ptr.assign((size_t)nin + 1, 0);
    for (int64_t q = 0; q < nmap; q++) inv_ptr[(size_t)input(q) + 1]++;
    for (int64_t t = 0; t < nin; t++) inv_ptr[(size_t)t + 1] += inv_ptr[(size_t)t];
    inv_idx.resize((size_t)nmap);
    std::vector<int32_t> at(inv_ptr.begin(), inv_ptr.end() - 1);
    for (int64_t j = 0; j < nslot; j++)
        for (int64_t q = ptr ? ptr[j] : j; q < (ptr ? ptr[j + 1] : j + 1); q++) inv_idx[(size_t)at[(size_t)input(q)]++] = (int32_t)j;
    return true;
}

// What a transposed solve leaves behind, put back when the guard goes (NestedSolveGuard keeps the ordinary solves' side)
struct TransposedStatsGuard {
    Solver &s;
    auto fields() const { return std::tie(s.transposed_solves, s.transposed_blocks, s.krylov_iterations_t, s.last_omega_t, s.refinement_steps_done_t); }
    const std::tuple<int64_t, int64_t, int64_t, double, int32_t> kept;
    explicit TransposedStatsGuard(Solver &s_) : s(s_), kept(fields()) {}
    ~TransposedStatsGuard() { fields() = kept; }
};

dim3 sens_grid(int64_t count) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(SENS_MAX_WG, (count + 255) / 256))); }

} // namespace

int32_t Solver::values_outer(double *grad, const double *u, const double *w, int32_t ncols, int64_t ldu, int64_t ldw, double alpha, double beta, bool mapped,
                             bool on_device) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!grad || !u || !w) return ERROR_NULL_POINTER;
    const int32_t n = S.n;
    const int64_t nnz = S.nnz_a;
    if (ncols < 1 || ldu < n || ldw < n || (mapped && nnz_in < 1)) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    // the way back to the caller's order: nothing (the CSR order), or an inverse map, built at its first use
    const int32_t *inv_ptr = nullptr, *inv_idx = nullptr;
    int64_t nout = nnz;
    if (mapped) {
        if (!sn_map_ready) {
            std::vector<int32_t> ip, ii;
            if (!invert_staging(nnz_in, nnz, h_seg_ptr.data(), h_seg_idx.data(), ip, ii)) return ERROR_HIPMF_INVALID_VALUE;
            HIPC(d_sn_map_ptr.upload(ip), ERROR_HIP_MALLOC);
            HIPC(d_sn_map_idx.upload(ii), ERROR_HIP_MALLOC);
            sn_map_ready = true;
        }
        inv_ptr = d_sn_map_ptr, inv_idx = d_sn_map_idx, nout = nnz_in;
    } else if (d_emap) {
        if (!sn_exp_ready) {
            std::vector<int32_t> ip, ii;
            (void)invert_staging(nnz_low, nnz, nullptr, h_emap.data(), ip, ii);
            HIPC(d_sn_exp_ptr.upload(ip), ERROR_HIP_MALLOC);
            HIPC(d_sn_exp_idx.upload(ii), ERROR_HIP_MALLOC);
            sn_exp_ready = true;
        }
        inv_ptr = d_sn_exp_ptr, inv_idx = d_sn_exp_idx, nout = nnz_low;
    }
    if (!sn_ev0) HIPC(hipEventCreate(sn_ev0.put()), ERROR_HIPMF_NO_DEVICE);
    if (!sn_ev1) HIPC(hipEventCreate(sn_ev1.put()), ERROR_HIPMF_NO_DEVICE);
    const double *du = u, *dw = w;
    double *dout = grad;
    if (!on_device) { // the operand columns packed (leading dimension n), the gradient in the caller's order
        const size_t nb = sizeof(double) * (size_t)n, blk = (size_t)n * ncols;
        HIPC(d_sn_ops.need(2 * blk), ERROR_HIP_MALLOC);
        HIPC(d_sn_out.need((size_t)std::max<int64_t>(nout, 1)), ERROR_HIP_MALLOC);
        for (int32_t c = 0; c < ncols; c++) {
            HIPC(hipMemcpyAsync(d_sn_ops.a + (size_t)c * n, u + (int64_t)c * ldu, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipMemcpyAsync(d_sn_ops.a + blk + (size_t)c * n, w + (int64_t)c * ldw, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        }
        if (beta != 0.0) HIPC(hipMemcpyAsync(d_sn_out.a, grad, sizeof(double) * (size_t)nout, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        du = d_sn_ops.a, dw = d_sn_ops.a + blk, ldu = ldw = n, dout = d_sn_out.a;
    }
    double *dslot = dout;
    if (inv_ptr) {
        HIPC(d_sn_slot.need((size_t)std::max<int64_t>(nnz, 1)), ERROR_HIP_MALLOC);
        dslot = d_sn_slot.a;
    }
    const double beta_outer = inv_ptr ? 0.0 : beta; // (through a map the caller's gradient enters in the scatter)
    HIPC(hipEventRecord((hipEvent_t)sn_ev0, STREAM), ERROR_HIP_SYNCHRONIZE);
    if (d_tptr) hipLaunchKernelGGL(k_sens_outer<true>, sens_grid(nnz), dim3(256), 0, STREAM, nnz, d_arow, d_ci, du, ldu, dw, ldw, ncols, alpha, beta_outer, dslot);
    else hipLaunchKernelGGL(k_sens_outer<false>, sens_grid(nnz), dim3(256), 0, STREAM, nnz, d_arow, d_ci, du, ldu, dw, ldw, ncols, alpha, beta_outer, dslot);
    if (inv_ptr) hipLaunchKernelGGL(k_sens_scatter, sens_grid(nout), dim3(256), 0, STREAM, nout, inv_ptr, inv_idx, (const double *)dslot, beta, dout);
    HIPC(hipEventRecord((hipEvent_t)sn_ev1, STREAM), ERROR_HIP_SYNCHRONIZE);
    if (!on_device) HIPC(hipMemcpyAsync(grad, dout, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, (hipEvent_t)sn_ev0, (hipEvent_t)sn_ev1);
    sens_outer_ms = ms;
    sens_outer_columns += ncols;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::solve_tangent(double *dx, const double *x, const double *dvalues, const double *db, int32_t nrhs, int64_t ld, bool mapped, bool on_device) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!dx || !x || !dvalues) return ERROR_NULL_POINTER;
    const int32_t n = S.n;
    if (nrhs < 1 || ld < n || (mapped && nnz_in < 1)) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    const size_t nb = sizeof(double) * (size_t)n, blk = (size_t)n * nrhs;
    // R = db - dA x and Y = A^{-1} R packed (leading dimension n), a zero vector for db == nullptr; x and db of a host-pointer call
    HIPC(d_sn_rhs.need((on_device ? 2 : 4) * blk + (size_t)n), ERROR_HIP_MALLOC);
    const int64_t pcol = 2 * (int64_t)std::max(spmv_blocks, 1);
    HIPC(d_sn_part.need((size_t)pcol * KRYB_COLS), ERROR_HIP_MALLOC);
    if (!d_up_vals) HIPC(d_up_vals.alloc((size_t)std::max<int64_t>(S.nnz_a, 1)), ERROR_HIP_MALLOC);
    double *const R = d_sn_rhs.a, *const Y = R + blk, *const zero = Y + blk, *const XS = zero + n, *const BS = XS + blk;
    int32_t code = stage_values(d_up_vals, dvalues, mapped, on_device);
    if (code != SUCCESSFUL_EXIT) return code;
    const double *X = x, *B = db;
    int64_t xstr = ld, bstr = ld;
    if (!on_device) {
        for (int32_t c = 0; c < nrhs; c++) {
            HIPC(hipMemcpyAsync(XS + (size_t)c * n, x + (int64_t)c * ld, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
            if (db) HIPC(hipMemcpyAsync(BS + (size_t)c * n, db + (int64_t)c * ld, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        }
        X = XS, B = BS, xstr = bstr = n;
    }
    if (!db) {
        HIPC(hipMemsetAsync(zero, 0, nb, STREAM), ERROR_HIP_MEMCPY);
        B = zero, bstr = 0; // (every column reads the same zeros)
    }
    for (int32_t j0 = 0; j0 < nrhs; j0 += KRYB_COLS) { // the right-hand sides: the blocked residual of the solve_updated forms on the staged dvalues
        const int32_t nk = std::min<int32_t>(KRYB_COLS, nrhs - j0);
        OpPlain::residual_blk(*this, STREAM, n, X + (int64_t)j0 * xstr, xstr, B + (int64_t)j0 * bstr, bstr, R + (size_t)j0 * n, nk, (1u << nk) - 1u, d_sn_part.a, pcol);
    }
    {
        const NestedSolveGuard guard(*this); // (refined as the handle is set up; the statistics of the ordinary solves stay the caller's)
        code = solve(Y, R, nrhs, n, true);
    }
    if (code != SUCCESSFUL_EXIT) return code;
    for (int32_t c = 0; c < nrhs; c++)
        HIPC(hipMemcpyAsync(dx + (int64_t)c * ld, Y + (size_t)c * n, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    return SUCCESSFUL_EXIT;
}

int32_t Solver::solve_adjoint(double *lambda, double *grad, const double *x, const double *g, int32_t nrhs, int64_t ld, double beta, bool mapped, bool on_device,
                              bool symmetric_matrix) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!lambda || !g || (grad && !x)) return ERROR_NULL_POINTER;
    const int32_t n = S.n;
    if (nrhs < 1 || ld < n || (grad && mapped && nnz_in < 1)) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    int32_t code;
    {
        const NestedSolveGuard guard(*this);
        const TransposedStatsGuard guard_t(*this);
        const bool plain = symmetric_matrix || S.sym_mode || d_tptr; // A^T = A: the ordinary solve, which reads its right-hand sides again while it refines
        const double *rhs = g;
        if (plain && on_device && lambda == g) {
            const size_t span = (size_t)(nrhs - 1) * (size_t)ld + (size_t)n;
            HIPC(d_sn_rhs.need(span), ERROR_HIP_MALLOC);
            HIPC(hipMemcpyAsync(d_sn_rhs.a, g, sizeof(double) * span, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
            rhs = d_sn_rhs.a;
        }
        code = plain ? solve(lambda, rhs, nrhs, ld, on_device) : solve_transpose_many(lambda, rhs, nrhs, ld, on_device);
    }
    if (code != SUCCESSFUL_EXIT || !grad) return code;
    return values_outer(grad, lambda, x, nrhs, ld, ld, -1.0, beta, mapped, on_device);
}

// ---- the inertia of the factor, and eigenpairs nearest the shift on the kept factor (kernels_eigs.hpp) ----

// Sylvester's law: A = L D L^T has as many positive / negative eigenvalues as D has positive / negative entries.  The symmetric scaling
// S A S and the symmetric fill-reducing permutation P A P^T are congruences: they leave the inertia alone, so the pivots in d_diag
// speak of the caller's matrix.  The tiled fronts of a symmetric handle take pivot c from row c by construction (kernels_factor.hpp,
// PIVOT = !SYM): their pivots are D.  The fronts that k_small_factor holds in LDS search the pivot block whatever the handle; where
// the search kept the diagonal their pivots are D as well, where it moved a row k_eig_inertia_small counts the inertia of the front's
// pivot block from the product of its factors (see there) -- the sum over the fronts is the inertia of the matrix either way.
int32_t Solver::inertia(int64_t *n_positive, int64_t *n_negative, int64_t *n_zero) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!S.sym_mode) return ERROR_NOT_AVAILABLE;
    DeviceScope dev_scope(device);
    const int32_t n = S.n;
    if (!d_eg_local) { // per pivot position: 0 in a small front, -1 in a tiled one; and the list of the small fronts
        std::vector<int32_t> local((size_t)n, -1), small;
        for (int32_t s = 0; s < S.nsuper; s++)
            if (S.fsize(s) <= SMALL_F) {
                small.push_back(s);
                for (int32_t i = 0; i < S.npiv(s); i++) local[(size_t)S.sn_first[s] + i] = 0;
            }
        eg_nsmall = (int32_t)small.size();
        HIPC(d_eg_small.upload(small), ERROR_HIP_MALLOC);
        HIPC(d_eg_cnt.alloc(4 * ((size_t)EIG_INERTIA_WG + small.size()) + 4), ERROR_HIP_MALLOC);
        HIPC(d_eg_local.upload(local), ERROR_HIP_MALLOC);
    }
    const int32_t nwg = (int32_t)std::min<int64_t>(EIG_INERTIA_WG, ((int64_t)n + 255) / 256);
    const int64_t nslot = (int64_t)nwg + eg_nsmall;
    int64_t *const d_sum = d_eg_cnt + 4 * ((size_t)EIG_INERTIA_WG + (size_t)eg_nsmall);
    hipLaunchKernelGGL(k_eig_inertia, dim3(nwg), dim3(256), 0, STREAM, n, (const double *)d_diag, (const unsigned long long *)d_scalar, opt.pivot_epsilon,
                       (const int32_t *)d_eg_local, (int64_t *)d_eg_cnt);
    if (eg_nsmall > 0)
        hipLaunchKernelGGL(k_eig_inertia_small, dim3((unsigned)eg_nsmall), dim3(64), 0, STREAM, (const int32_t *)d_eg_small, (const FrontDesc *)d_fd, (const double *)d_pool,
                           (const int32_t *)d_lperm, (const double *)d_diag, (const unsigned long long *)d_scalar, opt.pivot_epsilon, d_eg_cnt + 4 * (size_t)nwg);
    hipLaunchKernelGGL(k_eig_inertia_sum, dim3(1), dim3(256), 0, STREAM, nslot, (const int64_t *)d_eg_cnt, d_sum);
    int64_t got[4] = {0, 0, 0, 0};
    HIPC(hipMemcpyAsync(got, d_sum, sizeof got, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    inertia_fronts_recounted = got[3];
    if (n_positive) *n_positive = got[0];
    if (n_negative) *n_negative = got[1];
    if (n_zero) *n_zero = got[2];
    return (got[2] > 0 || n_perturbed > 0 || n_zero_pivot > 0) ? WARNING_SINGULAR_MATRIX : SUCCESSFUL_EXIT;
}

namespace {

// events around the phases of a Lanczos step (0 solve, 1 SpMV, 2 orthogonalisation, 3 rotation; -1: the end of the last phase), read
// after the step's synchronisation
struct EigTimer {
    EventOwner *ev;
    hipStream_t st;
    double *ms;
    int tag[16];
    int cnt = 0;
    void mark(int t) {
        if (cnt < 16 && hipEventRecord((hipEvent_t)ev[cnt], st) == hipSuccess) tag[cnt++] = t;
    }
    void flush() {
        float e = 0.0f;
        for (int i = 0; i + 1 < cnt; i++)
            if (tag[i] >= 0 && hipEventElapsedTime(&e, (hipEvent_t)ev[i], (hipEvent_t)ev[i + 1]) == hipSuccess) ms[tag[i]] += e;
        cnt = 0;
    }
};

} // namespace

// Shift-invert Lanczos with thick restart (Wu & Simon) on OP = A^{-1} M, which is symmetric in the M-inner product; A = K - sigma M is
// what the handle factorised, so an eigenvalue theta of OP is 1 / (lambda - sigma) and the wanted pairs are those of largest |theta|.
// One step with the basis v_0 .. v_j: p = M v_j (the stream SpMV on the staged values; M = I: nothing), w = A^{-1} p by solve() with
// the handle's refinement, CGS2 in the M-inner product -- h = V^T (M w) by k_kry_dots / k_kry_reduce, w -= V h by k_kry_update, twice,
// M w recomputed by SpMV each time (no second basis M V) --, beta^2 = w^T M w, v_{j+1} = w / beta (k_kry_scale).  The host reads the
// 2 (j + 1) coefficients and beta^2 and keeps the projected matrix T: alpha_j = h_j on the diagonal, beta_j beside it, after a restart
// the arrowhead beta s_i in row and column k.  T is diagonalised by cyclic Jacobi (krylov_host.hpp) when the basis is full and, before
// that, at every step up to 32 vectors and every fourth beyond: pair i has converged when |beta s_{q-1, i}| <= tol |theta_i| (ARPACK's
// rule).  A full basis restarts with the k = nev + (ncv - nev) / 2 (at most ncv - 1) Ritz vectors of largest |theta|, formed in place by
// k_eig_rotate, and v_k = v_ncv.  beta at the rounding level of |w| before Gram-Schmidt is a (lucky) breakdown: the next vector of the
// start sequence (k_eig_start) is M-orthogonalised against the basis and the iteration goes on with beta = 0; a basis that spans the
// whole space ends the call.  At the end X = V Y (k_eig_rotate into the caller's array), the sign of every column is fixed, and the
// TRUE residuals |A x - mu M x|_inf come from k_eig_residuals.
int32_t Solver::eigs_near_shift(int32_t nev, int32_t ncv, double sigma, const double *m_values, bool mapped, const double *v0, double tol, int32_t max_steps,
                                double *lambda, double *X, int64_t ldx, double *backward_error, int32_t *nconv_out, int32_t *steps_out, bool on_device,
                                bool symmetric_matrix) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!lambda || !X) return ERROR_NULL_POINTER;
    if (!(S.sym_lower || symmetric_matrix) || opt.complex_pairs) return ERROR_NOT_AVAILABLE;
    const int32_t n = S.n;
    if (nev < 1 || nev > EIG_NEV_MAX || nev >= n || ldx < n || !std::isfinite(tol) || !std::isfinite(sigma)) return ERROR_HIPMF_INVALID_VALUE;
    if (ncv <= 0) ncv = std::min(n, std::max(2 * nev + 8, 24));
    if (ncv <= nev || ncv > std::min<int32_t>(n, EIG_MMAX)) return ERROR_HIPMF_INVALID_VALUE;
    if (m_values && mapped && nnz_in < 1) return ERROR_HIPMF_INVALID_VALUE; // no map set
    if (!(tol > 0.0)) tol = 1e-10;
    DeviceScope dev_scope(device);
    eigs_steps = eigs_restarts = eigs_converged = 0;
    eigs_ms[0] = eigs_ms[1] = eigs_ms[2] = eigs_ms[3] = 0.0;
    if (nconv_out) *nconv_out = 0;
    if (steps_out) *steps_out = 0;

    // ---- buffers ----
    int32_t m = ncv;
    if (eg_m < m) {
        d_eg_V.reset(), eg_m = 0;
        for (int32_t mm = m;; mm = std::max(nev + 2, mm / 2)) {
            if (mm <= nev) break; // (ncv == nev + 1 did not fit)
            if (d_eg_V.alloc(((size_t)mm + 1) * (size_t)n) == hipSuccess) {
                eg_m = mm;
                break;
            }
            (void)hipGetLastError();
            if (mm <= nev + 2) break;
        }
        if (eg_m == 0) {
            last_error = "eigs_near_shift: no device memory for the Lanczos basis";
            return ERROR_HIP_MALLOC;
        }
    }
    m = std::min(m, eg_m);
    if (max_steps <= 0) max_steps = 20 * m;
    const int32_t nblk = (int32_t)(((int64_t)n + KRY_TILE - 1) / KRY_TILE), g256 = (n + 255) / 256;
    const size_t rec_h = 2 * ((size_t)EIG_MMAX + 1) + 4, rec_y = (size_t)EIG_MMAX * EIG_MMAX, rec_total = rec_h + rec_y + 4 * (size_t)EIG_NEV_MAX + 4;
    if (!eg_small) {
        HIPC(d_eg_vec.alloc(3 * (size_t)n), ERROR_HIP_MALLOC);
        HIPC(d_eg_part.alloc(((size_t)EIG_MMAX + 2) * nblk + (2 * (size_t)EIG_NEV_MAX + 1) * g256), ERROR_HIP_MALLOC);
        HIPC(d_eg_idx.alloc((size_t)EIG_NEV_MAX * g256), ERROR_HIP_MALLOC);
        HIPC(d_eg_rec.alloc(rec_total), ERROR_HIP_MALLOC);
        HIPC(h_eg.alloc(rec_total), ERROR_HIP_MALLOC);
        for (int t = 0; t < 16; t++) HIPC(hipEventCreate(eg_ev[t].put()), ERROR_HIP_SYNCHRONIZE);
        eg_small = true;
    }
    if (!on_device && eg_xcols < nev) {
        HIPC(d_eg_X.alloc((size_t)n * nev), ERROR_HIP_MALLOC);
        eg_xcols = nev;
    }
    const bool has_m = m_values != nullptr;
    if (has_m) {
        if (!d_up_vals) HIPC(d_up_vals.alloc((size_t)std::max<int64_t>(S.nnz_a, 1)), ERROR_HIP_MALLOC);
        const int32_t c = stage_values(d_up_vals, m_values, mapped, on_device);
        if (c != SUCCESSFUL_EXIT) return c;
    }
    double *const V = d_eg_V, *const d_p = d_eg_vec, *const d_w = d_eg_vec + (size_t)n, *const d_q = d_eg_vec + 2 * (size_t)n;
    double *const d_h = d_eg_rec, *const d_nrm = d_eg_rec + 2 * ((size_t)EIG_MMAX + 1), *const d_Y = d_eg_rec + rec_h, *const d_mu = d_Y + rec_y;
    double *const d_out = d_mu + EIG_NEV_MAX; // 2 nev maxima, then |A|, |M|; the signs behind them
    double *const d_sign = d_out + 2 * (size_t)EIG_NEV_MAX + 4;
    double *const h_h = h_eg, *const h_Y = h_eg + rec_h, *const h_mu = h_Y + rec_y, *const h_out = h_mu + EIG_NEV_MAX;
    double *const d_part = d_eg_part, *const d_part2 = d_eg_part + ((size_t)EIG_MMAX + 2) * nblk;
    double *const Xd = on_device ? X : (double *)d_eg_X;
    const int64_t ldxd = on_device ? ldx : n;
    const dim3 gk((unsigned)nblk), b256(256), gn((unsigned)g256);
    const size_t nb = sizeof(double) * (size_t)n;
    const double EPS = 2.220446049250313e-16;
    EigTimer timer{eg_ev, STREAM, eigs_ms};

    // y = M x on the staged values; M = I: x itself
    bool timed = true;
    auto times_m = [&](const double *x, double *y) -> const double * {
        if (!has_m) return x;
        if (timed) timer.mark(1);
        hipLaunchKernelGGL(k_spmv_stream<false>, dim3(spmv_blocks), b256, 0, STREAM, d_row_blk, d_rp, d_ci, d_up_vals, d_tptr, d_tidx, d_arow, 1.0, x, (const double *)nullptr, y,
                           (unsigned long long *)nullptr);
        return y;
    };
    // one round of Gram-Schmidt of w against v_0 .. v_{nv - 1} in the M-inner product, the coefficients to hr (device)
    auto gs_round = [&](int32_t nv, double *hr) {
        const double *mw = times_m(d_w, d_q);
        timer.mark(2);
        hipLaunchKernelGGL(k_kry_dots, gk, b256, 0, STREAM, (int64_t)n, mw, (const double *)V, nv, d_part);
        hipLaunchKernelGGL(k_kry_reduce, dim3(nv), b256, 0, STREAM, (const double *)d_part, nblk, hr);
        hipLaunchKernelGGL(k_kry_update, gk, b256, 0, STREAM, (int64_t)n, d_w, (const double *)V, nv, (const double *)hr, d_part);
    };
    // d_nrm[0] = w^T M w
    auto m_norm2 = [&]() {
        const double *mw = times_m(d_w, d_q);
        timer.mark(2);
        hipLaunchKernelGGL(k_kry_dots, gk, b256, 0, STREAM, (int64_t)n, mw, (const double *)d_w, 1, d_part);
        hipLaunchKernelGGL(k_kry_reduce, dim3(1), b256, 0, STREAM, (const double *)d_part, nblk, d_nrm);
    };
    // the record of a step on the host: cnt doubles from d_h, then the norm word
    auto read_record = [&](int32_t cnt) -> int32_t {
        timer.mark(-1);
        if (cnt > 0) HIPC(hipMemcpyAsync(h_h, d_h, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipMemcpyAsync(h_h + 2 * ((size_t)EIG_MMAX + 1), d_nrm, sizeof(double), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        timer.flush();
        return SUCCESSFUL_EXIT;
    };
    double &h_nrm = h_h[2 * ((size_t)EIG_MMAX + 1)];
    const auto invalid_m = [&]() {
        last_error = "eigs_near_shift: v^T M v is not positive (M must be symmetric positive definite)";
        return ERROR_HIPMF_INVALID_VALUE;
    };
    // v_dst = the vector of the start sequence number `seq`, M-orthogonalised against v_0 .. v_{nv - 1} and normalised; the norm must be
    // positive and finite.  *ok = false: the vector lies in the span of the basis to rounding (the caller tries the next one).
    uint32_t seq = 0;
    auto new_direction = [&](int32_t nv, double *v_dst, bool *ok) -> int32_t {
        *ok = false;
        m_norm2();
        int32_t c = read_record(0);
        if (c != SUCCESSFUL_EXIT) return c;
        const double before = h_nrm;
        if (!(before > 0.0) || !std::isfinite(before)) return invalid_m();
        if (nv > 0) {
            gs_round(nv, d_h), gs_round(nv, d_h + nv);
            m_norm2();
            c = read_record(0);
            if (c != SUCCESSFUL_EXIT) return c;
            if (!std::isfinite(h_nrm)) return invalid_m();
            if (!(h_nrm > 1e-8 * before)) return SUCCESSFUL_EXIT; // (half of the digits gone: not a direction of its own)
        }
        hipLaunchKernelGGL(k_kry_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)d_w, (const double *)d_nrm, v_dst);
        *ok = true;
        return SUCCESSFUL_EXIT;
    };

    const NestedSolveGuard guard(*this); // (the solves are refined as the handle is set up; the statistics of the ordinary solves stay the caller's)
    opt.verbose = false;
    int32_t code = SUCCESSFUL_EXIT;
    // ---- the start vector ----
    {
        if (v0) HIPC(hipMemcpyAsync(d_w, v0, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        else hipLaunchKernelGGL(k_eig_start, gn, b256, 0, STREAM, n, seq++, d_w);
        bool ok = false;
        code = new_direction(0, V, &ok);
        if (code != SUCCESSFUL_EXIT) return code;
    }
    std::vector<double> T((size_t)m * m, 0.0), theta, Z, Ysel;
    std::vector<int32_t> order;
    std::vector<char> conv;
    int32_t j = 0, q = 0, nconv = 0;
    double beta_last = 0.0;
    bool done = false, spans = false;
    while (!done) {
        // ---- one Lanczos step ----
        const double *vj = V + (size_t)j * n;
        const double *rhs = times_m(vj, d_p);
        timer.mark(0);
        code = solve(d_w, rhs, 1, n, true);
        if (code != SUCCESSFUL_EXIT) return code;
        eigs_steps++;
        const int32_t nv = j + 1;
        gs_round(nv, d_h), gs_round(nv, d_h + nv);
        m_norm2();
        code = read_record(2 * nv);
        if (code != SUCCESSFUL_EXIT) return code;
        double hsum2 = 0.0;
        bool finite = std::isfinite(h_nrm);
        for (int32_t i = 0; i < nv; i++) {
            const double hi = h_h[i] + h_h[nv + i];
            finite = finite && std::isfinite(hi);
            hsum2 += hi * hi;
        }
        if (!finite) return invalid_m();
        const double beta2 = h_nrm, wnorm2 = hsum2 + std::max(beta2, 0.0), level = 1024.0 * EPS;
        const bool breakdown = !(beta2 > level * level * wnorm2);
        if (breakdown && beta2 < -level * level * wnorm2) return invalid_m();
        T[(size_t)j * m + j] = h_h[j] + h_h[nv + j];
        q = j + 1;
        beta_last = breakdown ? 0.0 : sqrt(beta2);
        if (!breakdown) {
            hipLaunchKernelGGL(k_kry_scale, gk, b256, 0, STREAM, (int64_t)n, (const double *)d_w, (const double *)d_nrm, V + (size_t)q * n);
        } else if (q >= n) {
            spans = true;
        } else { // the next vector of the start sequence, against the whole basis
            bool ok = false;
            for (int attempt = 0; attempt < 4 && !ok; attempt++) {
                hipLaunchKernelGGL(k_eig_start, gn, b256, 0, STREAM, n, seq++, d_w);
                code = new_direction(q, V + (size_t)q * n, &ok);
                if (code != SUCCESSFUL_EXIT) return code;
            }
            if (!ok) spans = true; // (nothing new to be had: stop with what has been found)
        }
        if (q < m) T[(size_t)j * m + q] = T[(size_t)q * m + j] = beta_last;
        if (guard.verbose) fprintf(stderr, "hipmf: eigs_near_shift: step %lld, basis %d, beta %.3e%s\n", (long long)eigs_steps, q, beta_last, breakdown ? " (breakdown)" : "");
        const bool out_of_steps = eigs_steps >= max_steps;
        if (!(q == m || out_of_steps || spans || q <= 32 || (q & 3) == 0)) {
            j = q;
            continue;
        }
        // ---- the Ritz pairs of the basis so far ----
        jacobi_eigh(q, T.data(), m, theta, Z);
        order.resize((size_t)q);
        for (int32_t i = 0; i < q; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return std::fabs(theta[(size_t)a]) > std::fabs(theta[(size_t)b]); });
        conv.assign((size_t)q, 0);
        nconv = 0;
        for (int32_t i = 0; i < q; i++) {
            const int32_t e = order[(size_t)i];
            conv[(size_t)e] = std::fabs(beta_last * Z[(size_t)(q - 1) * q + e]) <= tol * std::fabs(theta[(size_t)e]);
            if (i < nev && conv[(size_t)e]) nconv++;
        }
        done = (q >= nev && nconv == nev) || out_of_steps || spans;
        if (done) break;
        if (q < m) {
            j = q;
            continue;
        }
        // ---- thick restart ----
        const int32_t k = std::min(nev + (m - nev) / 2, m - 1);
        for (int32_t c = 0; c < k; c++)
            for (int32_t r = 0; r < m; r++) h_Y[(size_t)c * m + r] = Z[(size_t)r * m + order[(size_t)c]];
        HIPC(hipMemcpyAsync(d_Y, h_Y, sizeof(double) * (size_t)m * k, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        timer.mark(3);
        hipLaunchKernelGGL(k_eig_rotate, dim3((unsigned)((n + 63) / 64)), b256, 0, STREAM, n, m, k, (const double *)V, (const double *)d_Y, V, (int64_t)n);
        timer.mark(-1);
        HIPC(hipMemcpyAsync(V + (size_t)k * n, V + (size_t)m * n, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE); // (h_Y may be rewritten)
        timer.flush();
        std::fill(T.begin(), T.end(), 0.0);
        for (int32_t c = 0; c < k; c++) {
            const int32_t e = order[(size_t)c];
            T[(size_t)c * m + c] = theta[(size_t)e];
            T[(size_t)c * m + k] = T[(size_t)k * m + c] = beta_last * Z[(size_t)(m - 1) * m + e];
        }
        eigs_restarts++;
        j = k;
    }

    // ---- the results: the nev Ritz pairs of largest |theta| and no others -- a pair further from the shift that happens to have
    // converged (an isolated one at the far end of the spectrum does so early) never displaces a nearer one --, the converged ones
    // of them first, each group by distance from the shift; nconv counts the converged among these
    const int32_t nout = std::min(nev, q);
    std::vector<int32_t> sel;
    for (int pass = 0; pass < 2; pass++)
        for (int32_t i = 0; i < nout; i++)
            if ((conv[(size_t)order[(size_t)i]] != 0) == (pass == 0)) sel.push_back(order[(size_t)i]);
    nconv = 0;
    for (int32_t c = 0; c < nout; c++) {
        const int32_t e = sel[(size_t)c];
        nconv += conv[(size_t)e] ? 1 : 0;
        h_mu[c] = 1.0 / theta[(size_t)e];
        lambda[c] = sigma + h_mu[c];
        for (int32_t r = 0; r < q; r++) h_Y[(size_t)c * q + r] = Z[(size_t)r * q + e];
    }
    for (int32_t c = nout; c < nev; c++) { // (fewer steps than pairs asked for: the rest is empty)
        lambda[c] = sigma;
        if (backward_error) backward_error[c] = 1.0;
        HIPC(hipMemsetAsync(Xd + (size_t)c * ldxd, 0, nb, STREAM), ERROR_HIP_MEMCPY);
    }
    HIPC(hipMemcpyAsync(d_Y, h_Y, sizeof(double) * (size_t)q * nout, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(d_mu, h_mu, sizeof(double) * (size_t)nout, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    timer.mark(3);
    hipLaunchKernelGGL(k_eig_rotate, dim3((unsigned)((n + 63) / 64)), b256, 0, STREAM, n, q, nout, (const double *)V, (const double *)d_Y, Xd, ldxd);
    timer.mark(-1);
    // |x_c|_M = 1 once more, from a compensated x_c^T M x_c (the norms of the iteration carry the rounding of plain sums over n)
    timed = false; // (the phases of the steps and the rotations are what the counters report)
    for (int32_t c = 0; c < nout; c++) {
        const double *xc = Xd + (size_t)c * ldxd;
        const double *mx = times_m(xc, d_q);
        hipLaunchKernelGGL(k_eig_dot2, gn, b256, 0, STREAM, n, xc, (int64_t)0, mx, (int64_t)0, d_part2 + (size_t)c * g256, d_part2 + ((size_t)nout + c) * g256);
    }
    hipLaunchKernelGGL(k_eig_dot2_sum, dim3((unsigned)nout), dim3(64), 0, STREAM, g256, (const double *)d_part2, (const double *)(d_part2 + (size_t)nout * g256), d_sign);
    hipLaunchKernelGGL(k_eig_scale_cols, dim3((unsigned)g256, (unsigned)nout), b256, 0, STREAM, n, Xd, ldxd, (const double *)d_sign);
    int32_t *const d_pi = d_eg_idx;
    hipLaunchKernelGGL(k_eig_absmax, dim3((unsigned)g256, (unsigned)nout), b256, 0, STREAM, n, (const double *)Xd, ldxd, d_part2, d_pi);
    hipLaunchKernelGGL(k_eig_sign, dim3((unsigned)nout), dim3(64), 0, STREAM, g256, (const double *)Xd, ldxd, (const double *)d_part2, (const int32_t *)d_pi, d_sign);
    hipLaunchKernelGGL(k_eig_flip, dim3((unsigned)g256, (unsigned)nout), b256, 0, STREAM, n, Xd, ldxd, (const double *)d_sign);
    // |A|_inf, |M|_inf once, then the true residuals of all columns in one pass over the values
    hipLaunchKernelGGL(k_eig_rownorm, gn, b256, 0, STREAM, n, (const int32_t *)d_rp, (const double *)d_vals, (const int32_t *)d_tptr, (const int32_t *)d_tidx, d_part2);
    hipLaunchKernelGGL(k_eig_max, dim3(1), b256, 0, STREAM, (const double *)d_part2, g256, d_out + 2 * (size_t)EIG_NEV_MAX);
    if (has_m) {
        hipLaunchKernelGGL(k_eig_rownorm, gn, b256, 0, STREAM, n, (const int32_t *)d_rp, (const double *)d_up_vals, (const int32_t *)d_tptr, (const int32_t *)d_tidx, d_part2);
        hipLaunchKernelGGL(k_eig_max, dim3(1), b256, 0, STREAM, (const double *)d_part2, g256, d_out + 2 * (size_t)EIG_NEV_MAX + 1);
    }
    hipLaunchKernelGGL(k_eig_residuals, gn, b256, 0, STREAM, n, (const int32_t *)d_rp, (const int32_t *)d_ci, (const double *)d_vals,
                       has_m ? (const double *)d_up_vals : (const double *)nullptr, (const int32_t *)d_tptr, (const int32_t *)d_tidx, (const int32_t *)d_arow, (const double *)Xd, ldxd,
                       (const double *)d_mu, nout, d_part2);
    hipLaunchKernelGGL(k_eig_max, dim3(2 * (unsigned)nout), b256, 0, STREAM, (const double *)d_part2, g256, d_out);
    HIPC(hipMemcpyAsync(h_out, d_out, sizeof(double) * (2 * (size_t)EIG_NEV_MAX + 2), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    if (!on_device)
        for (int32_t c = 0; c < nev; c++) HIPC(hipMemcpyAsync(X + (int64_t)c * ldx, Xd + (size_t)c * n, nb, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    timer.flush();
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    const double anorm = h_out[2 * (size_t)EIG_NEV_MAX], mnorm = has_m ? h_out[2 * (size_t)EIG_NEV_MAX + 1] : 1.0;
    for (int32_t c = 0; c < nout && backward_error; c++) {
        const double den = (anorm + std::fabs(h_mu[c]) * mnorm) * h_out[nout + c];
        backward_error[c] = den > 0.0 ? h_out[c] / den : (h_out[c] > 0.0 ? 1.0 : 0.0);
    }
    eigs_converged = nconv;
    if (nconv_out) *nconv_out = nconv;
    if (steps_out) *steps_out = (int32_t)eigs_steps;
    if (guard.verbose)
        fprintf(stderr, "hipmf: eigs_near_shift: %d of %d pair(s) converged after %lld step(s), %lld restart(s)\n", nconv, nev, (long long)eigs_steps, (long long)eigs_restarts);
    return nconv == nev ? SUCCESSFUL_EXIT : WARNING_NOT_CONVERGED;
}

// ---- the transposed bordered system (the loop: bordered_core above) ----

int32_t Solver::solve_bordered_transpose(double *y, double *w, const double *p, const double *q, int32_t nrhs, int64_t ldx, int64_t ldz, int32_t max_steps, double *info,
                                         bool on_device, bool conj_pairs) {
    return bordered_core<true>(y, w, p, q, nrhs, ldx, ldz, max_steps, info, on_device, conj_pairs);
}

// V = A^{-T} C by the handle's refined transposed solves, 16 columns per block, as W = A^{-1} B came from solve() -- nothing of the
// caller's statistics moves, plain or transposed --, packed as W is; D^T packed as D is (k_border_pack reads a column-major k x k array
// into a row-major one: the transpose).  Also the rows of A^T and the buffers of the transposed pass pair (tr_prepare,
// tr_prepare_blocked), which a handle where A^T = A does not need.
int32_t Solver::bt_prepare() {
    if (bt_ready) return SUCCESSFUL_EXIT;
    const int32_t n = S.n, k = bd_k, kp = bd_kp;
    const size_t npk = (size_t)n * kp, kk2 = (size_t)kp * kp;
    const dim3 b256(256);
    if (!(S.sym_mode || d_tptr)) {
        const int32_t code = tr_prepare();
        if (code != SUCCESSFUL_EXIT) return code;
        if (Tunables::now(&Tunables::transpose_blocked)) (void)tr_prepare_blocked(); // (without the block buffers: tr_pass per column, see bt_pass)
    }
    DeviceArray<double> d_cols, d_vcol, d_gs, d_rec; // a block of C's columns as they came, and of V; pairs: B^H V and the record of its LU
    HIPC(d_bt_V.alloc(npk), ERROR_HIP_MALLOC);
    HIPC(d_bt_Dt.alloc(kk2), ERROR_HIP_MALLOC);
    if (bd_pairs) {
        HIPC(d_bt_LU.alloc(kk2), ERROR_HIP_MALLOC);
        HIPC(d_bt_piv.alloc((size_t)kp), ERROR_HIP_MALLOC);
        HIPC(d_gs.alloc(kk2), ERROR_HIP_MALLOC);
        HIPC(d_rec.alloc(BORDER_REC), ERROR_HIP_MALLOC);
        HIPC(hipMemsetAsync(d_bt_piv, 0, sizeof(int32_t) * (size_t)kp, STREAM), ERROR_HIP_MEMCPY);
    }
    HIPC(d_cols.alloc((size_t)n * BORDER_COLS), ERROR_HIP_MALLOC);
    HIPC(d_vcol.alloc((size_t)n * BORDER_COLS), ERROR_HIP_MALLOC);
    HIPC(hipMemsetAsync(d_bt_V, 0, sizeof(double) * npk, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(d_bt_Dt, 0, sizeof(double) * kk2, STREAM), ERROR_HIP_MEMCPY);
    if (bd_pairs) // (D^H: the small block of the transposed real-equivalent system, M^H)
        hipLaunchKernelGGL(k_zborder_adjoint, dim3((unsigned)((k / 2 * (k / 2) + 255) / 256)), b256, 0, STREAM, k / 2, kp, (const double *)d_bd_D, (double *)d_bt_Dt);
    else
        hipLaunchKernelGGL(k_border_pack, dim3((unsigned)(((int64_t)k * k + 255) / 256)), b256, 0, STREAM, k, k, kp, 0, (const double *)d_bd_D, (int64_t)kp, (double *)d_bt_Dt);
    {
        const NestedSolveGuard guard(*this);
        const TransposedStatsGuard guard_t(*this);
        // (pairs: V = A^{-H} conj(C) from the k / 2 interleaved columns of conj(C), the even columns of the packed array; M^T is
        // served from the same V on conjugated data, see bordered_core)
        const int32_t kcols = bd_pairs ? k / 2 : k;
        for (int32_t j0 = 0; j0 < kcols; j0 += BORDER_COLS) {
            const int32_t nk = std::min(BORDER_COLS, kcols - j0);
            const dim3 gp((unsigned)(((int64_t)n * nk + 255) / 256)), gz((unsigned)(((int64_t)(n / 2) * nk + 255) / 256));
            if (bd_pairs)
                hipLaunchKernelGGL(k_zborder_unpack, gz, b256, 0, STREAM, n / 2, nk, kp, j0, (const double *)d_bd_C, (double *)d_cols, (int64_t)n);
            else
                hipLaunchKernelGGL(k_border_unpack, gp, b256, 0, STREAM, n, nk, kp, j0, (const double *)d_bd_C, (double *)d_cols, (int64_t)n);
            const int32_t code = solve_transpose_many(d_vcol, d_cols, nk, n, true);
            if (code != SUCCESSFUL_EXIT) return code;
            if (bd_pairs) {
                hipLaunchKernelGGL(k_zborder_pack, gz, b256, 0, STREAM, n / 2, nk, kp, j0, (const double *)d_vcol, (int64_t)n, 0, (double *)d_bt_V);
                hipLaunchKernelGGL(k_border_gram, dim3((unsigned)bd_chunks, (unsigned)(kp / 16)), dim3(64), 0, STREAM, n, kp, (const double *)d_bd_B, (const double *)d_vcol,
                                   (int64_t)n, nk, (double *)d_bd_part);
                hipLaunchKernelGGL(k_border_reduce, dim3((unsigned)kp), b256, 0, STREAM, bd_chunks, kp, (const double *)d_bd_part, d_gs + (size_t)j0 * kp);
            } else {
                hipLaunchKernelGGL(k_border_pack, gp, b256, 0, STREAM, n, nk, kp, j0, (const double *)d_vcol, (int64_t)n, (double *)d_bt_V);
            }
        }
    }
    if (bd_pairs) {
        // The complex twin factorises the Schur complement of M^H on its own, S_T = D^H - B^H V, instead of reaching for S^H through the LU
        // of S.  The real form may do that because W and V come from the SAME perturbed factor, (A + E)^{-1} B and (A + E)^{-T} C: then
        // D^T - B^T V is the transpose of S to rounding.  Here W and V are each built from k solves of the even real-equivalent columns,
        // the partners by rotation, and E does not have the structure of a complex matrix: rows and columns of the 2k x 2k real Schur
        // complement then give complex numbers that differ by cond(A)^2 eps -- 7e-7 relative at cond 7e10 (zhopf1e-10 of
        // tests/bordered_complex.py), which the border rows see in full as an omega of 1e-2 before the first step.  With S_T the
        // elimination of M^H is as consistent as that of M.  An exactly zero pivot of S_T: WARNING_SINGULAR_MATRIX, nothing is kept.
        hipLaunchKernelGGL(k_zborder_lu, dim3(1), b256, 0, STREAM, k / 2, kp, (const double *)d_bt_Dt, (const double *)d_gs, (double *)d_bt_LU, (int32_t *)d_bt_piv,
                           (double *)d_rec);
        double rec[BORDER_REC];
        HIPC(hipMemcpyAsync(rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        if (rec[4] != 0.0) return WARNING_SINGULAR_MATRIX;
    }
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE); // (the blocks go with this scope)
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    bt_bytes = (int64_t)(sizeof(double) * (npk + kk2));
    if (bd_pairs) bt_bytes += (int64_t)(sizeof(double) * kk2 + sizeof(int32_t) * (size_t)kp);
    bt_ready = true;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::bt_pass(double *Z, int64_t zs, const double *V, int64_t vs, int32_t C) {
    if (S.sym_mode || d_tptr) return solve_core(Z, V, C, zs, true);
    const int32_t n = S.n;
    if (C > 1 && tr_blk_ready && Tunables::now(&Tunables::transpose_blocked)) { // (one column: the single kernels, as solve_transpose_many sends it)
        const dim3 gp((n + 255) / 256, TR_KB / PERM_CW), b(256);
        const uint64_t all = (1ull << C) - 1ull;
        double *XP = d_tblk + 2 * (size_t)n * TR_KB;
        hipLaunchKernelGGL(k_tr_perm_in_cols, gp, b, 0, STREAM, n, d_perm, d_cs, V, vs, XP, (int64_t)n, all, C);
        const int32_t code = run_transposed<TrBlocked>(XP);
        if (code != SUCCESSFUL_EXIT) return code;
        hipLaunchKernelGGL(k_perm_out_cols, gp, b, 0, STREAM, n, d_rperm, d_rs, (const double *)XP, (int64_t)n, Z, zs, 0, all, C);
        return SUCCESSFUL_EXIT;
    }
    for (int32_t c = 0; c < C; c++) {
        const int32_t code = tr_pass(Z + (int64_t)c * zs, V + (int64_t)c * vs);
        if (code != SUCCESSFUL_EXIT) return code;
    }
    return SUCCESSFUL_EXIT;
}

int32_t Solver::set_complex_pattern(int64_t nnzc, const std::vector<int32_t> &zrow, const std::vector<int32_t> &zcol, bool sym) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (nnzc < 1 || (int64_t)zrow.size() != nnzc || (int64_t)zcol.size() != nnzc) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    sn_znnz = 0;
    HIPC(d_sn_zrow.upload(zrow), ERROR_HIP_MALLOC);
    HIPC(d_sn_zcol.upload(zcol), ERROR_HIP_MALLOC);
    sn_znnz = nnzc, sn_zsym = sym, sn_znin = 0;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::set_complex_value_map(int64_t nin, const std::vector<int32_t> &inv_ptr, const std::vector<int32_t> &inv_idx) {
    if (sn_znnz < 1) return ERROR_NEED_INITIALIZATION;
    sn_znin = 0;
    if (nin < 1) return SUCCESSFUL_EXIT;
    if ((int64_t)inv_ptr.size() != nin + 1) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    HIPC(d_sn_zinv_ptr.upload(inv_ptr), ERROR_HIP_MALLOC);
    HIPC(d_sn_zinv_idx.upload(inv_idx), ERROR_HIP_MALLOC);
    sn_znin = nin;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::values_outer_complex(double *grad, const double *u, const double *w, int32_t ncols, int64_t ldu, int64_t ldw, double alpha, double beta,
                                     bool conjugate_w) {
    if (!initialized || sn_znnz < 1) return ERROR_NEED_INITIALIZATION;
    if (!grad || !u || !w) return ERROR_NULL_POINTER;
    const int64_t nc = S.n / 2, nnzc = sn_znnz, nout = sn_znin > 0 ? sn_znin : nnzc;
    if (ncols < 1 || ldu < nc || ldw < nc) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    if (!sn_ev0) HIPC(hipEventCreate(sn_ev0.put()), ERROR_HIPMF_NO_DEVICE);
    if (!sn_ev1) HIPC(hipEventCreate(sn_ev1.put()), ERROR_HIPMF_NO_DEVICE);
    const size_t nb = sizeof(double) * 2 * (size_t)nc, blk = 2 * (size_t)nc * ncols;
    HIPC(d_sn_ops.need(2 * blk), ERROR_HIP_MALLOC);
    HIPC(d_sn_out.need(2 * (size_t)nout), ERROR_HIP_MALLOC);
    for (int32_t c = 0; c < ncols; c++) {
        HIPC(hipMemcpyAsync(d_sn_ops.a + 2 * (size_t)c * nc, u + 2 * (int64_t)c * ldu, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipMemcpyAsync(d_sn_ops.a + blk + 2 * (size_t)c * nc, w + 2 * (int64_t)c * ldw, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    }
    if (beta != 0.0) HIPC(hipMemcpyAsync(d_sn_out.a, grad, sizeof(double) * 2 * (size_t)nout, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    const double *du = d_sn_ops.a, *dw = d_sn_ops.a + blk;
    double *dout = d_sn_out.a, *dslot = dout;
    const bool via = sn_znin > 0;
    if (via) {
        HIPC(d_sn_slot.need(2 * (size_t)nnzc), ERROR_HIP_MALLOC);
        dslot = d_sn_slot.a;
    }
    const double beta_outer = via ? 0.0 : beta;
    const dim3 gz = sens_grid(nnzc), b256(256);
    HIPC(hipEventRecord((hipEvent_t)sn_ev0, STREAM), ERROR_HIP_SYNCHRONIZE);
    auto outer = [&](auto kernel) { hipLaunchKernelGGL(kernel, gz, b256, 0, STREAM, nnzc, (const int32_t *)d_sn_zrow, (const int32_t *)d_sn_zcol, du, nc, dw, nc, ncols, alpha, beta_outer, dslot); };
    if (sn_zsym) conjugate_w ? outer(k_zsens_outer<true, true>) : outer(k_zsens_outer<true, false>);
    else conjugate_w ? outer(k_zsens_outer<false, true>) : outer(k_zsens_outer<false, false>);
    if (via) hipLaunchKernelGGL(k_zsens_scatter, sens_grid(nout), b256, 0, STREAM, nout, (const int32_t *)d_sn_zinv_ptr, (const int32_t *)d_sn_zinv_idx, (const double *)dslot, beta, dout);
    HIPC(hipEventRecord((hipEvent_t)sn_ev1, STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipMemcpyAsync(grad, dout, sizeof(double) * 2 * (size_t)nout, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, (hipEvent_t)sn_ev0, (hipEvent_t)sn_ev1);
    sens_outer_ms = ms;
    sens_outer_columns += ncols;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::set_expansion(int64_t nnz_lower, const std::vector<int32_t> &emap) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (nnz_lower < 1 || (int64_t)emap.size() != S.nnz_a) return ERROR_HIPMF_INVALID_VALUE;
    DeviceScope dev_scope(device);
    HIPC(d_emap.upload(emap), ERROR_HIP_MALLOC);
    HIPC(d_vlow.alloc((size_t)nnz_lower), ERROR_HIP_MALLOC);
    nnz_low = nnz_lower;
    sn_exp_ready = false;
    if (&emap != &h_emap) h_emap = emap;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::adopt_factor(const double *d_values) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!d_values) return ERROR_NULL_POINTER;
    DeviceScope dev_scope(device);
    int32_t lc = stage_values(d_vals, d_values, false, true);
    if (lc != SUCCESSFUL_EXIT) return lc;
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    n_perturbed = n_zero_pivot = 0;
    factorized = true, forget_border();
    return SUCCESSFUL_EXIT;
}

// rcond estimate alone: a reduction over the pivots on the device (the determinant needs all of them on the host)
int32_t Solver::rcond_estimate(double *rcond) {
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!rcond) return ERROR_NULL_POINTER;
    DeviceScope dev_scope(device);
    const unsigned long long init[2] = {0x7ff0000000000000ull, 0ull};
    unsigned long long got[2];
    HIPC(hipMemcpyAsync(d_scalar + 2, init, sizeof init, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    hipLaunchKernelGGL(k_diag_minmax, dim3((unsigned)std::min<int64_t>(1024, (S.n + 255) / 256)), dim3(256), 0, STREAM, S.n, d_diag, d_scalar + 2);
    HIPC(hipMemcpyAsync(got, d_scalar + 2, sizeof got, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    double mn, mx;
    memcpy(&mn, &got[0], 8);
    memcpy(&mx, &got[1], 8);
    *rcond = (mx > 0.0 && std::isfinite(mn)) ? mn / mx : 0.0;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::determinant(double *mantissa, double *exponent, double *rcond) {
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    DeviceScope dev_scope(device);
    const int32_t n = S.n;
    std::vector<double> du((size_t)n), rs((size_t)n), cs;
    std::vector<int32_t> lp((size_t)n);
    const bool col_scaled = d_cs != nullptr; // matching, or the symmetric scaling S A S
    if (col_scaled) {
        cs.resize((size_t)n);
        HIPC(hipMemcpyAsync(cs.data(), d_cs, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    }
    HIPC(hipMemcpyAsync(du.data(), d_diag, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(rs.data(), d_rs, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(lp.data(), d_lperm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    // det(A) = sign * prod(u_ii) / prod(rs_i): the symmetric permutation contributes sign^2 = +1,
    // the row interchanges inside the pivot blocks contribute the parity of their cycles
    double m = 1.0, e = 0.0, umin = INFINITY, umax = 0.0;
    bool zero = false;
    for (int32_t i = 0; i < n; i++) {
        double d = col_scaled ? du[i] / rs[i] / cs[i] : du[i] / rs[i]; // (any pairing: only the products matter)
        umin = std::min(umin, std::fabs(du[i]));
        umax = std::max(umax, std::fabs(du[i]));
        if (d == 0.0 || !std::isfinite(d)) {
            zero = true;
            continue;
        }
        m *= d;
        while (std::fabs(m) >= 10.0) m /= 10.0, e += 1.0;
        while (std::fabs(m) < 1.0) m *= 10.0, e -= 1.0;
    }
    int parity = 0;
    std::vector<char> seen;
    for (int32_t s = 0; s < S.nsuper; s++) {
        int32_t first = S.sn_first[s], p = S.npiv(s);
        seen.assign((size_t)p, 0);
        for (int32_t i = 0; i < p; i++) {
            if (seen[i]) continue;
            int len = 0;
            for (int32_t j = i; !seen[j]; j = lp[first + j]) {
                seen[j] = 1;
                len++;
            }
            if ((len & 1) == 0) parity ^= 1;
        }
    }
    if (matched) parity ^= match_parity;
    if (parity) m = -m;
    if (zero || n_zero_pivot > 0) m = 0.0, e = 0.0;
    if (mantissa) *mantissa = m;
    if (exponent) *exponent = e;
    if (rcond) *rcond = (umax > 0.0 && std::isfinite(umin)) ? umin / umax : 0.0;
    return SUCCESSFUL_EXIT;
}

// Determinant of the COMPLEX matrix whose real-equivalent form was factorised with opt.complex_pairs (the coefficient / exponent pair
// umfpack_zi_get_determinant returns, /root/reference/russell_sparse/c_code/interface_complex_umfpack.c:187-195): the product of the
// complex pivots the paired pivot searches left (kernels_common.hpp, FactorInfoExt), over the scalings of the pairs, times the sign of
// the permutation of the complex rows (interchanges inside the pivot blocks, matching).
int32_t Solver::determinant_complex(double *mantissa_re, double *mantissa_im, double *exponent, double *rcond) {
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!opt.complex_pairs) return ERROR_NOT_AVAILABLE;
    DeviceScope dev_scope(device);
    const int32_t n = S.n, nc = n / 2;
    std::vector<double> zd((size_t)n), rs((size_t)n), cs;
    std::vector<int32_t> lp((size_t)n);
    const bool col_scaled = d_cs != nullptr;
    if (col_scaled) {
        cs.resize((size_t)n);
        HIPC(hipMemcpyAsync(cs.data(), d_cs, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    }
    HIPC(hipMemcpyAsync(zd.data(), d_diag + n, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(rs.data(), d_rs, sizeof(double) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(lp.data(), d_lperm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    double mr = 1.0, mi = 0.0, e = 0.0, zmin = INFINITY, zmax = 0.0;
    bool zero = false;
    for (int32_t k = 0; k < nc; k++) {
        // (the two rows of a pair carry the same scale up to rounding; any pairing of pivots and scales: only the products matter)
        double sc = std::sqrt(rs[2 * k] * rs[2 * k + 1]);
        if (col_scaled) sc *= std::sqrt(cs[2 * k] * cs[2 * k + 1]);
        const double a = zd[2 * k], b = zd[2 * k + 1], mod = std::hypot(a, b);
        zmin = std::min(zmin, mod), zmax = std::max(zmax, mod);
        const double zr = a / sc, zi = b / sc;
        if ((zr == 0.0 && zi == 0.0) || !std::isfinite(zr) || !std::isfinite(zi)) {
            zero = true;
            continue;
        }
        const double tr = mr * zr - mi * zi, ti = mr * zi + mi * zr;
        mr = tr, mi = ti;
        double mm = std::hypot(mr, mi);
        while (mm >= 10.0) mr /= 10.0, mi /= 10.0, mm /= 10.0, e += 1.0;
        while (mm < 1.0 && mm > 0.0) mr *= 10.0, mi *= 10.0, mm *= 10.0, e -= 1.0;
    }
    int parity = 0;
    std::vector<char> seen;
    for (int32_t s = 0; s < S.nsuper; s++) {
        const int32_t first = S.sn_first[s], pc = S.npiv(s) / 2;
        if ((first & 1) || (S.npiv(s) & 1)) return ERROR_HIPMF_SYMBOLIC; // (analyse with pair_blocks keeps the pairs inside one supernode)
        seen.assign((size_t)pc, 0);
        for (int32_t i = 0; i < pc; i++) {
            if (seen[i]) continue;
            int len = 0;
            for (int32_t j = i; !seen[j]; j = lp[first + 2 * j] >> 1) {
                if ((lp[first + 2 * j] >> 1) != (lp[first + 2 * j + 1] >> 1) || (lp[first + 2 * j] >> 1) >= pc) {
                    last_error = "internal error: a pivot pair was split";
                    return ERROR_HIPMF_SYMBOLIC;
                }
                seen[j] = 1;
                len++;
            }
            if ((len & 1) == 0) parity ^= 1;
        }
    }
    if (matched) parity ^= match_parity;
    if (parity) mr = -mr, mi = -mi;
    if (zero || n_zero_pivot > 0) mr = 0.0, mi = 0.0, e = 0.0;
    if (mantissa_re) *mantissa_re = mr;
    if (mantissa_im) *mantissa_im = mi;
    if (exponent) *exponent = e;
    if (rcond) *rcond = (zmax > 0.0 && std::isfinite(zmin)) ? zmin / zmax : 0.0;
    return SUCCESSFUL_EXIT;
}

// ---- transposed solves (A^T x = b) and the error analysis ----
// The plan (built at the first transposed solve of a factor): per level the small fronts (one wavefront each) and, for the big fronts,
// the assembly / gather tasks (TR_ROWS rows of the front's vector each) and the GEMV tasks (TR_COLS stored columns of E' resp. E each).
// A^T as CSR: for row i of A^T (column i of A) the rows of A holding an entry in that column, in ascending order, and where its value
// sits in d_vals -- values are read through the map, so refreshed values, factorize_mapped and adopt_factor need nothing here.
int32_t Solver::tr_prepare() {
    if (tr_ready) return SUCCESSFUL_EXIT;
    const int32_t n = S.n;
    std::vector<int32_t> list;
    std::vector<SolveTask> tasks;
    tr_levels.assign((size_t)S.nlevels, TrLevel());
    for (int32_t l = 0; l < S.nlevels; l++) {
        TrLevel &T = tr_levels[(size_t)l];
        std::vector<int32_t> big;
        T.small_off = (int32_t)list.size();
        for (int32_t k = S.level_ptr[l]; k < S.level_ptr[l + 1]; k++) {
            const int32_t s = S.level_sn[k];
            if (S.fsize(s) <= SMALL_F) {
                list.push_back(s);
                T.small_pmax = std::max(T.small_pmax, S.npiv(s)), T.small_fmax = std::max(T.small_fmax, S.fsize(s));
            } else {
                big.push_back(s);
            }
        }
        T.small_cnt = (int32_t)list.size() - T.small_off;
        auto emit = [&](int32_t &off, int32_t &cnt, bool rows_of_front, bool all_cols, int32_t step) {
            off = (int32_t)tasks.size();
            for (int32_t s : big) {
                const int32_t ext = (rows_of_front || all_cols) ? S.fsize(s) : S.npiv(s);
                for (int32_t r0 = 0; r0 < ext; r0 += step) tasks.push_back({s, r0, std::min(ext, r0 + step)});
            }
            cnt = (int32_t)tasks.size() - off;
        };
        emit(T.asm_off, T.asm_cnt, true, false, TR_ROWS);  // forward: the front's vector
        emit(T.gf_off, T.gf_cnt, false, true, TR_COLS);    // forward: the f columns of E'
        emit(T.ga_off, T.ga_cnt, true, false, TR_ROWS);    // backward: the front's vector
        emit(T.gb_off, T.gb_cnt, false, false, TR_COLS);   // backward: the p columns of E
    }
    HIPC(d_tr_list.upload(list), ERROR_HIP_MALLOC);
    HIPC(d_tr_tasks.upload(tasks), ERROR_HIP_MALLOC);
    // A^T by a counting pass over the stored pattern (rows ascending: the entries of a column of A come out in row order)
    const int64_t nnz = S.nnz_a;
    std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz);
    HIPC(hipMemcpy(rp.data(), d_rp, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpy(ci.data(), d_ci, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    std::vector<int32_t> tp((size_t)n + 1, 0), trow((size_t)nnz), tmap((size_t)nnz);
    for (int64_t k = 0; k < nnz; k++) tp[(size_t)ci[(size_t)k] + 1]++;
    for (int32_t i = 0; i < n; i++) tp[(size_t)i + 1] += tp[(size_t)i];
    std::vector<int32_t> fill(tp.begin(), tp.end() - 1);
    for (int32_t i = 0; i < n; i++)
        for (int32_t k = rp[(size_t)i]; k < rp[(size_t)i + 1]; k++) {
            const int32_t q = fill[(size_t)ci[(size_t)k]]++;
            trow[(size_t)q] = i, tmap[(size_t)q] = k;
        }
    HIPC(d_ttptr.upload(tp), ERROR_HIP_MALLOC);
    HIPC(d_ttrow.upload(trow), ERROR_HIP_MALLOC);
    HIPC(d_ttmap.upload(tmap), ERROR_HIP_MALLOC);
    {
        // the row blocks of the transposed solve_updated products: consecutive rows of A^T with at most KRYT_CAP stored entries (a
        // longer row -- a dense column of A -- stands alone, closed by the next row)
        std::vector<int32_t> tb(1, 0);
        int32_t start = 0;
        for (int32_t i = 0; i < n; i++)
            if (tp[(size_t)i + 1] - tp[(size_t)start] > KRYT_CAP && i > start) tb.push_back(i), start = i;
        tb.push_back(n);
        tt_blocks = (int32_t)tb.size() - 1;
        HIPC(d_ttblk.upload(tb), ERROR_HIP_MALLOC);
        HIPC(d_tt_part.alloc(2 * (size_t)std::max(tt_blocks, 1) * KRYB_COLS), ERROR_HIP_MALLOC);
    }
    HIPC(d_work_t.alloc((size_t)std::max<int64_t>(work_up, 1) + 64), ERROR_HIP_MALLOC);
    HIPC(d_tvec.alloc(6 * (size_t)n), ERROR_HIP_MALLOC);
    HIPC(d_tnrm.alloc(2), ERROR_HIP_MALLOC);
    HIPC(h_tnrm.alloc(2), ERROR_HIP_MALLOC);
    tr_ready = true;
    return SUCCESSFUL_EXIT;
}

// both passes of A^T on the permuted, scaled xp (in place), one launch per level and front class.  P: TrSingle (one vector) or
// TrBlocked (n x TR_KB at stride n)
template <class P>
int32_t Solver::run_transposed(double *xp) {
    const size_t nl = tr_levels.size();
    const int64_t xs = S.n;
    double *work = P::work(*this);
    for (size_t l = 0; l < nl; l++) {
        const TrLevel &T = tr_levels[l];
        const int32_t ldu = T.small_pmax | 1;
        if (T.small_cnt > 0)
            P::launch_ld(P::fwd_small, dim3(T.small_cnt), sizeof(double) * (size_t)T.small_fmax * (size_t)ldu, STREAM, xs, ldu, d_tr_list + T.small_off, d_fd, d_pool,
                         d_child, d_rel, work, xp);
        if (T.asm_cnt > 0) P::launch(P::assemble, dim3(T.asm_cnt), STREAM, xs, d_tr_tasks + T.asm_off, d_fd, d_child, d_rel, work, (const double *)xp);
        if (T.gf_cnt > 0) P::launch(P::fwd, dim3(T.gf_cnt), STREAM, xs, d_tr_tasks + T.gf_off, d_fd, d_pool, work, xp);
    }
    for (size_t l = nl; l-- > 0;) {
        const TrLevel &T = tr_levels[l];
        const int32_t ldl = T.small_fmax | 1;
        if (T.ga_cnt > 0) P::launch(P::gather, dim3(T.ga_cnt), STREAM, xs, d_tr_tasks + T.ga_off, d_fd, d_rows, work, (const double *)xp);
        if (T.gb_cnt > 0) P::launch(P::bwd, dim3(T.gb_cnt), STREAM, xs, d_tr_tasks + T.gb_off, d_fd, d_pool, work, xp);
        if (T.small_cnt > 0)
            P::launch_ld(P::bwd_small, dim3(T.small_cnt), sizeof(double) * (size_t)T.small_pmax * (size_t)ldl, STREAM, xs, ldl, d_tr_list + T.small_off, d_fd, d_pool,
                         d_rows, d_lperm, xp);
    }
    return SUCCESSFUL_EXIT;
}

// y = A^{-T} v (device vectors, y != v allowed to alias d_tvec slots other than xp): entry with the column permutation and scaling,
// exit with the row ones (A^ = Pr Rs A Cs Pc: b^_j = cs[cp_j] b[cp_j], x[rp_i] = rs[rp_i] y_i)
int32_t Solver::tr_pass(double *y, const double *v) {
    const int32_t n = S.n;
    const dim3 g((n + 255) / 256), b(256);
    double *xp = d_tvec + 2 * (size_t)n;
    hipLaunchKernelGGL(k_tr_perm_in, g, b, 0, STREAM, n, d_perm, d_cs, v, xp);
    int32_t code = run_transposed<TrSingle>(xp);
    if (code != SUCCESSFUL_EXIT) return code;
    hipLaunchKernelGGL(k_perm_out, g, b, 0, STREAM, n, d_rperm, d_rs, xp, y, 0);
    return SUCCESSFUL_EXIT;
}

// the same for C <= TR_KB contiguous columns at stride n through the blocked kernels (after tr_prepare_blocked(); the entry kernel fills
// the columns from C on with zeros)
int32_t Solver::tr_pass_blk(double *Z, const double *V, int32_t C) {
    const int32_t n = S.n;
    const dim3 gp((n + 255) / 256, TR_KB / PERM_CW), b(256);
    const uint64_t all = (1ull << C) - 1ull;
    double *XP = d_tblk + 2 * (size_t)n * TR_KB;
    hipLaunchKernelGGL(k_tr_perm_in_cols, gp, b, 0, STREAM, n, d_perm, d_cs, V, (int64_t)n, XP, (int64_t)n, all, C);
    const int32_t code = run_transposed<TrBlocked>(XP);
    if (code != SUCCESSFUL_EXIT) return code;
    hipLaunchKernelGGL(k_perm_out_cols, gp, b, 0, STREAM, n, d_rperm, d_rs, (const double *)XP, (int64_t)n, Z, (int64_t)n, 0, all, C);
    return SUCCESSFUL_EXIT;
}

int32_t Solver::tr_spmv(double *y, const double *x) {
    const int32_t n = S.n;
    hipLaunchKernelGGL(k_tr_spmv, dim3((n + 255) / 256), dim3(256), 0, STREAM, n, d_ttptr, d_ttrow, d_ttmap, d_vals, x, (const double *)nullptr, y,
                       (unsigned long long *)nullptr);
    return SUCCESSFUL_EXIT;
}

// The refinement rule of solve() for nk <= TR_KB transposed columns that one unrefined pass pair has solved, omega = max_i |r_i| /
// (|A^T||x| + |b|)_i per column: stop at omega <= eps, after nstep steps or when a step fails to halve omega; a step that makes omega
// worse is taken back; a column within 64 eps is done after its correction.  One residual launch and one host look at the omegas per
// step; columns that are done leave through the mask (they ride through the correcting passes as zeros and the exit kernel leaves them
// alone).  P issues the launches: TrColumn (nk = 1, the single kernels) or TrColumns (a block).
template <class P>
int32_t Solver::tr_refine(const P &p, int32_t nk, int32_t nstep, double *omega, int32_t *steps) {
    const double EPS = 2.220446049250313e-16;
    double prev[TR_KB];
    for (int c = 0; c < nk; c++) omega[c] = prev[c] = INFINITY, steps[c] = 0;
    uint64_t active = nstep > 0 ? (1ull << nk) - 1ull : 0;
    for (int32_t it = 0; active; it++) {
        HIPC(hipMemsetAsync(p.d_nrm(), 0, sizeof(unsigned long long) * P::words, STREAM), ERROR_HIP_MEMCPY);
        p.residual(STREAM, active);
        HIPC(hipMemcpyAsync(p.h_nrm(), p.d_nrm(), sizeof(double) * P::words, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        uint64_t back = 0, corr = 0;
        for (int c = 0; c < nk; c++) {
            if (!((active >> c) & 1ull)) continue;
            const double om = p.h_nrm()[2 * c + 1];
            if (it > 0 && !(om < prev[c])) {
                back |= 1ull << c, omega[c] = prev[c]; // take the last correction back
                continue;
            }
            omega[c] = om;
            if (om <= EPS || it == nstep || (it > 0 && om > 0.5 * prev[c])) continue;
            prev[c] = om, corr |= 1ull << c;
        }
        if (back) p.perm_out(STREAM, 2, back);
        if (!corr) break;
        p.perm_in(STREAM, corr);
        const int32_t code = run_transposed<typename P::Pass>(p.xp);
        if (code != SUCCESSFUL_EXIT) return code;
        p.perm_out(STREAM, 1, corr);
        active = 0;
        for (int c = 0; c < nk; c++)
            if ((corr >> c) & 1ull) {
                steps[c]++;
                if (!(prev[c] <= 64.0 * EPS || it + 1 > nstep)) active |= 1ull << c;
            }
    }
    return SUCCESSFUL_EXIT;
}

// one transposed solve of device vectors (not d_tvec slots 2 and 3): the pass pair, then the rule
int32_t Solver::tr_core(double *x, const double *bvec, int32_t nstep, double *omega, int32_t *steps) {
    *omega = INFINITY, *steps = 0;
    const int32_t code = tr_pass(x, bvec);
    return code != SUCCESSFUL_EXIT ? code : tr_refine(TrColumn{*this, x, bvec}, 1, nstep, omega, steps);
}

// FGMRES on one transposed column (device vectors tx, tb: not d_tvec slots 2 .. 5) with A^T as the operator and the transposed pass pair as the
// preconditioner (host vectors; d_tvec slots 4 and 5).  Its step count goes to krylov_iterations_t (first column only): krylov_iterations /
// krylov_last_relres stay what the last ordinary solve left.
int32_t Solver::tr_rescue(double *tx, const double *tb, bool first_column) {
    const size_t nb = sizeof(double) * (size_t)S.n;
    double *tv = d_tvec + 4 * (size_t)S.n, *tz = d_tvec + 5 * (size_t)S.n;
    KrylovOps ops;
    ops.precond = [&](double *z, const double *v) -> int32_t {
        HIPC(hipMemcpy(tv, v, nb, hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
        const int32_t c = tr_pass(tz, tv);
        if (c != SUCCESSFUL_EXIT) return c;
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        HIPC(hipMemcpy(z, tz, nb, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
        return SUCCESSFUL_EXIT;
    };
    ops.apply = [&](double *w, const double *z) -> int32_t {
        HIPC(hipMemcpy(tv, z, nb, hipMemcpyHostToDevice), ERROR_HIP_MEMCPY);
        tr_spmv(tz, tv);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        HIPC(hipMemcpy(w, tz, nb, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
        return SUCCESSFUL_EXIT;
    };
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    const int64_t keep_iter = krylov_iterations;
    const double keep_relres = krylov_last_relres;
    krylov_iterations = 0;
    const int32_t code = krylov_rescue(tx, tb, true, &ops);
    if (first_column) krylov_iterations_t = krylov_iterations;
    krylov_iterations = keep_iter, krylov_last_relres = keep_relres;
    return code;
}

int32_t Solver::solve_transpose(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device, bool conj_pairs) {
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs) return ERROR_NULL_POINTER;
    if (nrhs < 1 || ldx < S.n) return ERROR_HIPMF_INVALID_VALUE;
    if ((S.sym_mode || d_tptr) && !conj_pairs) { // A^T = A (L D L^T fronts, symmetric storage): the ordinary solve, its bits
        const int32_t code = solve(x, rhs, nrhs, ldx, on_device);
        if (code == SUCCESSFUL_EXIT) transposed_solves += nrhs, last_omega_t = last_omega, refinement_steps_done_t = refinement_steps_done;
        return code;
    }
    DeviceScope dev_scope(device);
    int32_t code = tr_prepare();
    if (code != SUCCESSFUL_EXIT) return code;
    const int32_t n = S.n;
    const size_t nb = sizeof(double) * (size_t)n;
    const dim3 g((n + 255) / 256), b(256);
    double *tb = d_tvec, *tx = d_tvec + (size_t)n;
    krylov_iterations_t = 0;
    for (int32_t j = 0; j < nrhs; j++) {
        const double *bj = rhs + (int64_t)j * ldx;
        double *xj = x + (int64_t)j * ldx;
        HIPC(hipMemcpyAsync(tb, bj, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        if (conj_pairs) hipLaunchKernelGGL(k_tr_conj, g, b, 0, STREAM, n, tb);
        double omega = INFINITY;
        int32_t steps = 0;
        code = tr_core(tx, tb, opt.refinement_nstep, &omega, &steps);
        if (code != SUCCESSFUL_EXIT) return code;
        if (krylov_enabled && !in_rescue && n_perturbed > 0 && !(omega <= krylov_omega_ok)) {
            code = tr_rescue(tx, tb, j == 0);
            if (code != SUCCESSFUL_EXIT) return code;
        }
        if (conj_pairs) hipLaunchKernelGGL(k_tr_conj, g, b, 0, STREAM, n, tx);
        HIPC(hipMemcpyAsync(xj, tx, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        if (j == 0) last_omega_t = omega, refinement_steps_done_t = steps;
    }
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    transposed_solves += nrhs;
    return SUCCESSFUL_EXIT;
}

// ---- blocked transposed solves: TR_KB columns per pass pair (kernels_solve_transpose_blocked.hpp) ----
// The buffers of the blocked path, allocated at its first call: the interleaved workspace (TR_KB values per row of every front, beside
// d_work and d_work_t), four n x TR_KB block vectors (b, x, xp, r), the norm words.  The launches run over the task lists tr_prepare
// built on tr_levels: TR_ROWS rows per assembly / gather task, and -- the product kernel's tile -- TR_COLS stored columns per product task.
int32_t Solver::tr_prepare_blocked() {
    if (tr_blk_ready) return SUCCESSFUL_EXIT;
    const size_t n = (size_t)S.n;
    if (d_work_tb.alloc(((size_t)std::max<int64_t>(work_up, 1) + 64) * TR_KB) != hipSuccess || d_tblk.alloc(4 * n * TR_KB) != hipSuccess ||
        d_tnrm_blk.alloc(2 * TR_KB) != hipSuccess || h_tnrm_blk.alloc(2 * TR_KB) != hipSuccess) {
        d_work_tb.reset(), d_tblk.reset(), d_tnrm_blk.reset(), h_tnrm_blk.reset();
        (void)hipGetLastError(); // (the caller runs the column loop instead: the failed allocation is not its error)
        return ERROR_HIP_MALLOC;
    }
    tr_blk_ready = true;
    return SUCCESSFUL_EXIT;
}

// nrhs columns of A^T X = B, TR_KB at a time.  Per block: entry (column permutation and scaling), the two passes, exit (row ones), then
// the refinement rule for the block's columns (tr_refine), then the transposed FGMRES rescue of solve_transpose for the columns that need
// it.  One column, A^T = A, HIPMF_TRANSPOSE_BLOCKED=0 or no memory for the block buffers: solve_transpose (transposed_blocks stays 0).
// conj_pairs (the complex twin's A^T through the A^H solve of the real-equivalent system): every block's right-hand sides are staged and
// conjugated on entry, its solutions on exit (k_tr_conj_cols); refinement and rescue run in between, on the A^H system.
int32_t Solver::solve_transpose_many(double *x, const double *rhs, int32_t nrhs, int64_t ldx, bool on_device, bool conj_pairs) {
    transposed_blocks = 0;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x || !rhs) return ERROR_NULL_POINTER;
    if (nrhs < 1 || ldx < S.n) return ERROR_HIPMF_INVALID_VALUE;
    if (nrhs == 1 || S.sym_mode || d_tptr) return solve_transpose(x, rhs, nrhs, ldx, on_device, conj_pairs);
    DeviceScope dev_scope(device);
    {
        const int32_t code = tr_prepare();
        if (code != SUCCESSFUL_EXIT) return code;
        if (!Tunables::now(&Tunables::transpose_blocked) || tr_prepare_blocked() != SUCCESSFUL_EXIT) return solve_transpose(x, rhs, nrhs, ldx, on_device, conj_pairs);
    }
    const int32_t n = S.n, nstep = opt.refinement_nstep;
    const size_t nb = sizeof(double) * (size_t)n, nz = (size_t)n;
    const dim3 gp((n + 255) / 256, TR_KB / PERM_CW), b(256);
    double *TB = d_tblk, *TX = TB + nz * TR_KB, *XP = TX + nz * TR_KB; // (then the residuals: TrColumns)
    const uintptr_t xa = (uintptr_t)x, ra = (uintptr_t)rhs, span = sizeof(double) * (size_t)nrhs * (size_t)ldx;
    const bool aliased = on_device && xa < ra + span && ra < xa + span; // (x written while rhs is still read: the block's columns are staged)
    krylov_iterations_t = 0;
    int64_t blocks = 0;
    for (int32_t j0 = 0; j0 < nrhs; j0 += TR_KB, blocks++) {
        const int32_t nk = std::min<int32_t>(TR_KB, nrhs - j0);
        const uint64_t all = (1ull << nk) - 1ull;
        const double *B = rhs + (int64_t)j0 * ldx;
        double *X = x + (int64_t)j0 * ldx;
        int64_t bs = ldx, xs = ldx;
        const dim3 gconj((unsigned)((n / 2 + 255) / 256), (unsigned)nk);
        if (!on_device || aliased || conj_pairs) {
            for (int32_t c = 0; c < nk; c++)
                HIPC(hipMemcpyAsync(TB + nz * c, B + (int64_t)c * ldx, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
            if (conj_pairs) hipLaunchKernelGGL(k_tr_conj_cols, gconj, b, 0, STREAM, n, TB, (int64_t)n, (uint32_t)all, nk);
            B = TB, bs = n;
        }
        if (!on_device) X = TX, xs = n;
        hipLaunchKernelGGL(k_tr_perm_in_cols, gp, b, 0, STREAM, n, d_perm, d_cs, B, bs, XP, (int64_t)n, all, nk);
        int32_t code = run_transposed<TrBlocked>(XP);
        if (code != SUCCESSFUL_EXIT) return code;
        hipLaunchKernelGGL(k_perm_out_cols, gp, b, 0, STREAM, n, d_rperm, d_rs, (const double *)XP, (int64_t)n, X, xs, 0, all, nk);
        double omega[TR_KB];
        int32_t steps[TR_KB];
        code = tr_refine(TrColumns{*this, X, xs, B, bs, nk}, nk, nstep, omega, steps);
        if (code != SUCCESSFUL_EXIT) return code;
        if (krylov_enabled && !in_rescue && n_perturbed > 0) {
            double *tb = d_tvec, *tx = d_tvec + nz;
            for (int c = 0; c < nk; c++) {
                if (omega[c] <= krylov_omega_ok) continue;
                HIPC(hipMemcpyAsync(tb, B + (int64_t)c * bs, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
                HIPC(hipMemcpyAsync(tx, X + (int64_t)c * xs, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
                code = tr_rescue(tx, tb, j0 + c == 0);
                if (code != SUCCESSFUL_EXIT) return code;
                HIPC(hipMemcpyAsync(X + (int64_t)c * xs, tx, nb, hipMemcpyDeviceToDevice, STREAM), ERROR_HIP_MEMCPY);
            }
        }
        if (conj_pairs) hipLaunchKernelGGL(k_tr_conj_cols, gconj, b, 0, STREAM, n, X, xs, (uint32_t)all, nk);
        if (!on_device)
            for (int32_t c = 0; c < nk; c++)
                HIPC(hipMemcpyAsync(x + (int64_t)(j0 + c) * ldx, TX + nz * c, nb, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
        if (j0 == 0) last_omega_t = omega[0], refinement_steps_done_t = steps[0];
    }
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    transposed_solves += nrhs;
    transposed_blocks = blocks;
    return SUCCESSFUL_EXIT;
}

// ---- sparse right-hand sides, selected solution rows, entries of the inverse (kernels_solve_pruned.hpp) ----
// Pruning the elimination tree is exact.  The forward pass of column c starts from zeros everywhere but at the permuted positions of its
// non-zeros: a front whose subtree holds none of them assembles zeros, eliminates zeros and hands zeros up -- only the fronts on the paths
// from those positions' fronts to the root do anything.  The backward pass computes x1 of a front from y1 and the entries of x of its
// ANCESTORS only: row i of x needs the fronts on the path from the root down to i's front and nothing else.
// The maps (built once): the inverses of the entry permutation (d_rperm: row of A at permuted position i; with a matching the matched
// one) and of the exit permutation (d_perm), read back from the device -- so whatever initialize or a re-matching factorize installed is
// what the maps invert --; the front of a position and the parent of a front are S.sn_of and S.sn_parent.
int32_t Solver::sp_prepare() {
    if (sp_ready) return SUCCESSFUL_EXIT;
    const size_t n = (size_t)S.n, ns = (size_t)S.nsuper;
    std::vector<int32_t> rp(n), cp(n);
    HIPC(hipMemcpy(rp.data(), d_rperm, sizeof(int32_t) * n, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpy(cp.data(), d_perm, sizeof(int32_t) * n, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    sp_ipos_r.assign(n, 0), sp_ipos_c.assign(n, 0);
    for (size_t i = 0; i < n; i++) sp_ipos_r[(size_t)rp[i]] = (int32_t)i, sp_ipos_c[(size_t)cp[i]] = (int32_t)i;
    HIPC(d_sp_ipos_r.upload(sp_ipos_r), ERROR_HIP_MALLOC);
    HIPC(d_sp_ipos_c.upload(sp_ipos_c), ERROR_HIP_MALLOC);
    HIPC(d_sp_mark.alloc(std::max<size_t>(ns, 1)), ERROR_HIP_MALLOC);
    HIPC(hipMemset(d_sp_mark, 0, sizeof(int32_t) * std::max<size_t>(ns, 1)), ERROR_HIP_MEMCPY);
    HIPC(d_sp_xp.alloc(n * SP_KB), ERROR_HIP_MALLOC);
    HIPC(d_sp_work.alloc(((size_t)std::max<int64_t>(work_up, 1) + 64) * SP_KB), ERROR_HIP_MALLOC);
    HIPC(hipEventCreate(sp_ev0.put()), ERROR_HIPMF_NO_DEVICE);
    HIPC(hipEventCreate(sp_ev1.put()), ERROR_HIPMF_NO_DEVICE);
    sp_stamp_f.assign(ns, 0), sp_stamp_b.assign(ns, 0);
    sp_epoch = 0;
    sp_total_pf = 0.0;
    for (int32_t s = 0; s < S.nsuper; s++) sp_total_pf += (double)S.npiv(s) * (double)S.fsize(s);
    sp_ready = true;
    return SUCCESSFUL_EXIT;
}

void Solver::sp_build_lists(const std::vector<int32_t> &fronts, SpShape shape, std::vector<int32_t> &buf, std::vector<SpLevel> &lv) const {
    const size_t nl = (size_t)S.nlevels;
    lv.assign(nl, SpLevel());
    buf.clear();
    // bucket by level (counting sort; fronts ascending within a level: the lists do not depend on the order the marking met them)
    std::vector<int32_t> cnt(nl + 1, 0), order(fronts.size());
    for (int32_t s : fronts) cnt[(size_t)S.sn_level[(size_t)s] + 1]++;
    for (size_t l = 0; l < nl; l++) cnt[l + 1] += cnt[l];
    {
        std::vector<int32_t> at(cnt.begin(), cnt.end() - 1);
        for (int32_t s : fronts) order[(size_t)at[(size_t)S.sn_level[(size_t)s]]++] = s;
    }
    for (size_t l = 0; l < nl; l++) {
        SpLevel &L = lv[l];
        int32_t *b = order.data() + cnt[l], *e = order.data() + cnt[l + 1];
        std::sort(b, e);
        L.small_off = (int32_t)buf.size();
        for (int32_t *q = b; q < e; q++)
            if (S.fsize(*q) <= SMALL_F) buf.push_back(*q), L.pmax = std::max(L.pmax, S.npiv(*q)), L.fmax = std::max(L.fmax, S.fsize(*q));
        L.small_cnt = (int32_t)buf.size() - L.small_off;
        auto task = [&](int32_t s, int32_t r0, int32_t r1) { buf.push_back(s), buf.push_back(r0), buf.push_back(r1); };
        L.va_off = (int32_t)buf.size();
        for (int32_t *q = b; q < e; q++)
            if (S.fsize(*q) > SMALL_F)
                for (int32_t r0 = 0; r0 < S.fsize(*q); r0 += TR_ROWS) task(*q, r0, std::min(S.fsize(*q), r0 + TR_ROWS)), L.va_cnt++;
        L.pr_off = (int32_t)buf.size();
        for (int32_t *q = b; q < e; q++)
            if (S.fsize(*q) > SMALL_F) {
                const int32_t p = S.npiv(*q), f = S.fsize(*q);
                if (shape == SP_FORWARD_T) { // (tiles of TR_COLS stored columns of E' over [0, f), every start a multiple of 16)
                    for (int32_t r0 = 0; r0 < f; r0 += TR_COLS) task(*q, r0, std::min(f, r0 + TR_COLS)), L.pr_cnt++;
                    continue;
                }
                for (int32_t r0 = 0; r0 < p; r0 += SP_ROWS) task(*q, r0, std::min(p, r0 + SP_ROWS)), L.pr_cnt++;
                if (shape == SP_FORWARD) // (the tiles of the update rows start at p: no tile straddles the pivot block, whose known zeros are skipped)
                    for (int32_t r0 = p; r0 < f; r0 += SP_ROWS) task(*q, r0, std::min(f, r0 + SP_ROWS)), L.pr_cnt++;
            }
    }
}

// both passes on the permuted, scaled block XP (n x SP_KB at stride n, in place) over the lists already on the device
int32_t Solver::run_pruned(double *XP, const std::vector<SpLevel> &fl, const std::vector<SpLevel> &bl) {
    const int64_t xs = S.n;
    const int32_t *FB = d_sp_fwd.a, *BB = d_sp_bwd.a;
    const int32_t ep = sp_epoch;
    auto tasks = [](const int32_t *base, int32_t off) { return reinterpret_cast<const SolveTask *>(base + off); };
    for (size_t l = 0; l < fl.size(); l++) {
        const SpLevel &L = fl[l];
        if (L.small_cnt > 0) {
            const int32_t ldp = L.fmax | 1;
            hipLaunchKernelGGL(k_sp_fwd_small, dim3(L.small_cnt), dim3(64), sizeof(double) * (size_t)ldp * (size_t)L.pmax, STREAM, FB + L.small_off, d_fd, d_pool,
                               d_lperm, d_child, d_rel, d_sp_mark, ep, d_sp_work, XP, xs, ldp);
        }
        if (L.va_cnt > 0)
            hipLaunchKernelGGL(k_sp_assemble, dim3(L.va_cnt), dim3(256), 0, STREAM, tasks(FB, L.va_off), d_fd, d_child, d_rel, d_sp_mark, ep, d_sp_work,
                               (const double *)XP, xs);
        if (L.pr_cnt > 0)
            hipLaunchKernelGGL(k_sp_gemm<true>, dim3(L.pr_cnt), dim3(256), 0, STREAM, tasks(FB, L.pr_off), d_fd, d_pool, d_sp_work, XP, xs);
    }
    for (size_t l = bl.size(); l-- > 0;) {
        const SpLevel &L = bl[l];
        if (L.va_cnt > 0) {
            if (S.sym_mode)
                hipLaunchKernelGGL(k_sp_gather_sym, dim3(L.va_cnt), dim3(256), 0, STREAM, tasks(BB, L.va_off), d_fd, d_rows, d_diag, d_sp_work, (const double *)XP, xs);
            else
                hipLaunchKernelGGL(k_tr_gather_blk, dim3(L.va_cnt), dim3(256), 0, STREAM, tasks(BB, L.va_off), d_fd, d_rows, d_sp_work, (const double *)XP, xs);
        }
        if (L.pr_cnt > 0) {
            if (S.sym_mode) // x1 = E^T [D^{-1} y1; x2]: the transposed product of the blocked transposed solves, sixteen columns of E per task
                hipLaunchKernelGGL(k_tr_gemm_blk<false>, dim3(L.pr_cnt), dim3(256), 0, STREAM, tasks(BB, L.pr_off), d_fd, d_pool, d_sp_work, XP, xs);
            else
                hipLaunchKernelGGL(k_sp_gemm<false>, dim3(L.pr_cnt), dim3(256), 0, STREAM, tasks(BB, L.pr_off), d_fd, d_pool, d_sp_work, XP, xs);
        }
        if (L.small_cnt > 0) {
            const int32_t ldu = L.pmax | 1;
            hipLaunchKernelGGL(k_sp_bwd_small, dim3(L.small_cnt), dim3(64), sizeof(double) * (size_t)ldu * (size_t)L.fmax, STREAM, BB + L.small_off, d_fd, d_pool,
                               d_rows, XP, xs, ldu);
        }
    }
    return SUCCESSFUL_EXIT;
}

// The same for A^T: the forward (U^T) pass over the lists of shape SP_FORWARD_T, the backward (L^T) pass over backward lists -- the
// blocked transposed kernels on the pruned path's workspace, the two forward kernels that add children's updates with the mark test
// (kernels_solve_pruned_transpose.hpp).  Nothing of the blocked transposed solve's own buffers (d_work_tb, d_tblk) is touched.
int32_t Solver::run_pruned_transposed(double *XP, const std::vector<SpLevel> &fl, const std::vector<SpLevel> &bl) {
    const int64_t xs = S.n;
    const int32_t *FB = d_sp_fwd.a, *BB = d_sp_bwd.a;
    const int32_t ep = sp_epoch;
    auto tasks = [](const int32_t *base, int32_t off) { return reinterpret_cast<const SolveTask *>(base + off); };
    for (size_t l = 0; l < fl.size(); l++) {
        const SpLevel &L = fl[l];
        if (L.small_cnt > 0) {
            const int32_t ldu = L.pmax | 1;
            hipLaunchKernelGGL(k_spt_fwd_small, dim3(L.small_cnt), dim3(64), sizeof(double) * (size_t)ldu * (size_t)L.fmax, STREAM, FB + L.small_off, d_fd, d_pool,
                               d_child, d_rel, d_sp_mark, ep, d_sp_work, XP, xs, ldu);
        }
        if (L.va_cnt > 0)
            hipLaunchKernelGGL(k_spt_assemble, dim3(L.va_cnt), dim3(256), 0, STREAM, tasks(FB, L.va_off), d_fd, d_child, d_rel, d_sp_mark, ep, d_sp_work,
                               (const double *)XP, xs);
        if (L.pr_cnt > 0)
            hipLaunchKernelGGL(k_tr_gemm_blk<true>, dim3(L.pr_cnt), dim3(256), 0, STREAM, tasks(FB, L.pr_off), d_fd, d_pool, d_sp_work, XP, xs);
    }
    for (size_t l = bl.size(); l-- > 0;) {
        const SpLevel &L = bl[l];
        if (L.va_cnt > 0)
            hipLaunchKernelGGL(k_tr_gather_blk, dim3(L.va_cnt), dim3(256), 0, STREAM, tasks(BB, L.va_off), d_fd, d_rows, d_sp_work, (const double *)XP, xs);
        if (L.pr_cnt > 0)
            hipLaunchKernelGGL(k_tr_gemm_blk<false>, dim3(L.pr_cnt), dim3(256), 0, STREAM, tasks(BB, L.pr_off), d_fd, d_pool, d_sp_work, XP, xs);
        if (L.small_cnt > 0) {
            const int32_t ldl = L.fmax | 1;
            hipLaunchKernelGGL(k_tr_bwd_small_blk, dim3(L.small_cnt), dim3(64), sizeof(double) * (size_t)ldl * (size_t)L.pmax, STREAM, BB + L.small_off, d_fd, d_pool,
                               d_rows, d_lperm, XP, xs, ldl);
        }
    }
    return SUCCESSFUL_EXIT;
}

// x_sel(k, c) = (A^{-1} B)(sel_idx[k], c), column-major with ldx >= the number of rows returned (nsel, or n when sel_idx == nullptr).
// Per block of up to SP_KB columns:
//   mark     forward set = union of the root paths of the fronts of the non-zeros' permuted positions, backward set (once per call) = the
//            same for the selected rows; a walk stops at the first front already marked: O(visited fronts)
//   decide   share = (sum of p f over the forward set + the same over the backward set) / (2 sum over all fronts): the factor entries the
//            pruned pass pair reads against a full one.  share > theta (HIPMF_PRUNE_MAX_SHARE, read per call; default 0.25 from the measured
//            crossover), a one-column block on a factor whose pass pair reads less than HIPMF_PRUNE_MIN_BYTES (2e9), or
//            a factor with replaced pivots: the columns are expanded into a dense block, solve() runs on it -- refinement and Krylov
//            rescue as the handle has them -- and the rows are selected
//   run      k_sp_begin (marks, zeros), k_sp_scatter_in (entry permutation and row scaling), the two passes, k_sp_gather_out (exit
//            permutation and column scaling).  One unrefined pass pair: a residual needs all of x and all of A, which is what pruning avoids
//            (MUMPS's ICNTL(20) / ICNTL(30) solves are unrefined too).
// accumulate: pruned_blocks continues to count (inverse_entries calls this once per block of columns).
// transposed (A^T X = B; a handle with A^T = A runs everything above unchanged): the maps swap roles.  b enters as k_tr_perm_in_cols has
// it, xp[j] = cs[perm[j]] b[perm[j]] -- a non-zero of row i at sp_ipos_c[i], scaled by cs, and the forward set is marked from there --;
// x leaves as k_perm_out_cols has it with d_rperm / d_rs -- row k from sp_ipos_r[k], scaled by rs, the backward set marked from there.
// The passes are run_pruned_transposed, the fallback (same rules; the thresholds have not been measured for A^T) is solve_transpose_many
// on the expanded block, or solve_transpose column by column for conj_pairs.  conj_pairs: k_spt_conj_in / k_spt_conj_out around a pruned block.
int32_t Solver::solve_sparse(double *x_sel, int64_t ldx, int32_t nrhs, const int32_t *rhs_ptr, const int32_t *rhs_idx, const double *rhs_val, int32_t nsel,
                             const int32_t *sel_idx, bool on_device, bool accumulate, bool transposed, bool conj_pairs) {
    if (!accumulate) pruned_blocks = 0, pruned_transposed_blocks = 0;
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!x_sel || !rhs_ptr) return ERROR_NULL_POINTER;
    const int32_t n = S.n;
    if (nrhs < 1 || (sel_idx && nsel < 1)) return ERROR_HIPMF_INVALID_VALUE;
    const int32_t nout = sel_idx ? nsel : n;
    if (ldx < nout) return ERROR_HIPMF_INVALID_VALUE;
    const bool tr = transposed && !(S.sym_mode || d_tptr);
    if (conj_pairs && (!tr || on_device)) return ERROR_HIPMF_INVALID_VALUE; // (the sign kernels work on the staged copies of a transposed block)
    DeviceScope dev_scope(device);
    // host copies of the index arrays (the marking runs on the host), validated before anything reads through them
    std::vector<int32_t> ptr_keep, idx_keep, sel_keep;
    const int32_t *hp = rhs_ptr, *hi = rhs_idx, *hs = sel_idx;
    if (on_device) {
        ptr_keep.resize((size_t)nrhs + 1);
        HIPC(hipMemcpy(ptr_keep.data(), rhs_ptr, sizeof(int32_t) * ((size_t)nrhs + 1), hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
        hp = ptr_keep.data();
    }
    if (hp[0] < 0) return ERROR_HIPMF_INVALID_VALUE;
    for (int32_t c = 0; c < nrhs; c++)
        if (hp[c + 1] < hp[c]) return ERROR_HIPMF_INVALID_VALUE;
    const int32_t e_first = hp[0], e_end = hp[nrhs];
    const size_t nnz_b = (size_t)(e_end - e_first);
    if (nnz_b > 0 && (!rhs_idx || !rhs_val)) return ERROR_NULL_POINTER;
    if (on_device) {
        idx_keep.resize(nnz_b);
        if (nnz_b) HIPC(hipMemcpy(idx_keep.data(), rhs_idx + e_first, sizeof(int32_t) * nnz_b, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
        hi = idx_keep.data() - e_first;
        if (sel_idx) {
            sel_keep.resize((size_t)nsel);
            HIPC(hipMemcpy(sel_keep.data(), sel_idx, sizeof(int32_t) * (size_t)nsel, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
            hs = sel_keep.data();
        }
    }
    for (int32_t c = 0; c < nrhs; c++)
        for (int32_t e = hp[c]; e < hp[c + 1]; e++)
            if (hi[e] < 0 || hi[e] >= n || (e > hp[c] && hi[e] <= hi[e - 1])) return ERROR_HIPMF_INVALID_VALUE;
    if (hs)
        for (int32_t k = 0; k < nsel; k++)
            if (hs[k] < 0 || hs[k] >= n) return ERROR_HIPMF_INVALID_VALUE;
    int32_t code = sp_prepare();
    if (code != SUCCESSFUL_EXIT) return code;
    HIPC(hipEventRecord((hipEvent_t)sp_ev0, STREAM), ERROR_HIP_SYNCHRONIZE);
    // the arrays as the kernels read them: the caller's on the device, else copies in the reusable buffers (entry e of the caller at e - e_first)
    const int32_t *d_idx = rhs_idx, *d_sel = sel_idx;
    const double *d_val = rhs_val;
    double *d_out = x_sel;
    int64_t ostr = ldx;
    int32_t shift = 0;
    if (!on_device) {
        HIPC(d_sp_idx.need(std::max<size_t>(nnz_b, 1)), ERROR_HIP_MALLOC);
        HIPC(d_sp_val.need(std::max<size_t>(nnz_b, 1)), ERROR_HIP_MALLOC);
        HIPC(d_sp_out.need((size_t)nout * (size_t)std::min<int32_t>(nrhs, SP_KB)), ERROR_HIP_MALLOC);
        if (nnz_b) {
            HIPC(hipMemcpyAsync(d_sp_idx.a, rhs_idx + e_first, sizeof(int32_t) * nnz_b, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
            HIPC(hipMemcpyAsync(d_sp_val.a, rhs_val + e_first, sizeof(double) * nnz_b, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        }
        d_idx = d_sp_idx.a, d_val = d_sp_val.a, shift = e_first;
        if (sel_idx) {
            HIPC(d_sp_sel.need((size_t)nsel), ERROR_HIP_MALLOC);
            HIPC(hipMemcpyAsync(d_sp_sel.a, sel_idx, sizeof(int32_t) * (size_t)nsel, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
            d_sel = d_sp_sel.a;
        }
        ostr = nout;
    }
    const double theta = Tunables::now(&Tunables::prune_max_share), min_bytes_1col = Tunables::now(&Tunables::prune_min_bytes);
    const bool never_pruned = n_perturbed > 0;
    const std::vector<int32_t> &pos_in = tr ? sp_ipos_c : sp_ipos_r, &pos_out = tr ? sp_ipos_r : sp_ipos_c; // where b enters, where x leaves
    const int32_t *const d_ipr = d_sp_ipos_r, *const d_ipc = d_sp_ipos_c;
    const double *const d_rsc = d_rs, *const d_csc = d_cs;
    const int32_t *d_pos_in = tr ? d_ipc : d_ipr, *d_pos_out = tr ? d_ipr : d_ipc;
    const double *d_sc_in = tr ? d_csc : d_rsc, *d_sc_out = tr ? d_rsc : d_csc;
    // the backward set and its lists: once per call
    std::vector<int32_t> bset, fset, bbuf, fbuf;
    std::vector<SpLevel> blv, flv;
    double b_pf = 0.0;
    bool bwd_ready = false;
    auto prepare_bwd = [&]() -> int32_t {
        if (bwd_ready) return SUCCESSFUL_EXIT;
        const int32_t be = ++sp_epoch;
        if (!hs) {
            bset.resize((size_t)S.nsuper);
            for (int32_t s = 0; s < S.nsuper; s++) bset[(size_t)s] = s, sp_stamp_b[(size_t)s] = be;
            b_pf = sp_total_pf;
        } else {
            for (int32_t k = 0; k < nsel; k++)
                for (int32_t s = S.sn_of[(size_t)pos_out[(size_t)hs[k]]]; s >= 0 && sp_stamp_b[(size_t)s] != be; s = S.sn_parent[(size_t)s])
                    sp_stamp_b[(size_t)s] = be, bset.push_back(s), b_pf += (double)S.npiv(s) * (double)S.fsize(s);
        }
        sp_build_lists(bset, SP_BACKWARD, bbuf, blv);
        HIPC(d_sp_bwd.need(std::max<size_t>(bbuf.size(), 1)), ERROR_HIP_MALLOC);
        if (!bbuf.empty()) HIPC(hipMemcpyAsync(d_sp_bwd.a, bbuf.data(), sizeof(int32_t) * bbuf.size(), hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
        bwd_ready = true;
        return SUCCESSFUL_EXIT;
    };
    const dim3 gsel((nout + 255) / 256), b256(256);
    for (int32_t j0 = 0; j0 < nrhs; j0 += SP_KB) {
        const int32_t nk = std::min<int32_t>(SP_KB, nrhs - j0);
        SpCols cols;
        for (int32_t c = 0; c <= SP_KB; c++) cols.ptr[c] = hp[j0 + std::min(c, nk)] - shift;
        const int32_t nz = cols.ptr[nk] - cols.ptr[0];
        double *out_blk = on_device ? d_out + (int64_t)j0 * ostr : d_sp_out.a;
        bool pruned = !never_pruned;
        double f_pf = 0.0;
        int32_t fe = 0;
        if (pruned) {
            code = prepare_bwd();
            if (code != SUCCESSFUL_EXIT) return code;
            fe = ++sp_epoch;
            fset.clear();
            for (int32_t e = hp[j0]; e < hp[j0 + nk]; e++)
                for (int32_t s = S.sn_of[(size_t)pos_in[(size_t)hi[e]]]; s >= 0 && sp_stamp_f[(size_t)s] != fe; s = S.sn_parent[(size_t)s])
                    sp_stamp_f[(size_t)s] = fe, fset.push_back(s), f_pf += (double)S.npiv(s) * (double)S.fsize(s);
            pruned_share_last = sp_total_pf > 0.0 ? (f_pf + b_pf) / (2.0 * sp_total_pf) : 0.0;
            if (pruned_share_last > theta) pruned = false;
            // a block of ONE column on a factor whose full pass pair reads little: the dependency-driven single-column solve is faster than
            // the pruned path's chain of level launches, however few fronts it visits (theta >= 1 asks for pruning regardless)
            if (theta < 1.0 && nk == 1 && 16.0 * sp_total_pf < min_bytes_1col) pruned = false;
        }
        if (pruned) {
            sp_build_lists(fset, tr ? SP_FORWARD_T : SP_FORWARD, fbuf, flv);
            // k_sp_begin's list behind the forward lists: the forward set (marked), then the fronts of the backward set alone (~s)
            const size_t begin_off = fbuf.size();
            for (int32_t s : fset) fbuf.push_back(s);
            for (int32_t s : bset)
                if (sp_stamp_f[(size_t)s] != fe) fbuf.push_back(~s);
            const size_t begin_cnt = fbuf.size() - begin_off;
            HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE); // (the previous block's launches read the buffer that is refilled now)
            HIPC(d_sp_fwd.need(fbuf.size()), ERROR_HIP_MALLOC);
            HIPC(hipMemcpyAsync(d_sp_fwd.a, fbuf.data(), sizeof(int32_t) * fbuf.size(), hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
            double *XP = d_sp_xp;
            hipLaunchKernelGGL(k_sp_begin, dim3((unsigned)begin_cnt), b256, 0, STREAM, d_sp_fwd.a + begin_off, d_fd, d_sp_mark, fe, XP, (int64_t)n);
            if (nz > 0 && conj_pairs) // (d_val is the staged copy: conj_pairs comes with host arrays)
                hipLaunchKernelGGL(k_spt_conj_in, dim3((nz + 255) / 256), b256, 0, STREAM, cols.ptr[0], cols.ptr[nk], d_idx, d_sp_val.a);
            if (nz > 0)
                hipLaunchKernelGGL(k_sp_scatter_in, dim3((nz + 255) / 256), b256, 0, STREAM, cols, nk, d_idx, d_val, d_pos_in, d_sc_in, XP, (int64_t)n);
            code = tr ? run_pruned_transposed(XP, flv, blv) : run_pruned(XP, flv, blv);
            if (code != SUCCESSFUL_EXIT) return code;
            hipLaunchKernelGGL(k_sp_gather_out, gsel, b256, 0, STREAM, nout, d_sel, d_pos_out, d_sc_out, (const double *)XP, (int64_t)n, out_blk, ostr, nk);
            if (conj_pairs) hipLaunchKernelGGL(k_spt_conj_out, gsel, b256, 0, STREAM, nout, d_sel, out_blk, ostr, nk);
            if (tr) pruned_transposed_blocks++;
            pruned_fwd_fronts = (int64_t)fset.size(), pruned_bwd_fronts = (int64_t)bset.size();
            pruned_bytes = (int64_t)(8.0 * (f_pf + b_pf));
            pruned_blocks++;
        } else {
            // the ordinary solve on the expanded block, then the selection
            HIPC(d_sp_dense.need(2 * (size_t)n * SP_KB), ERROR_HIP_MALLOC);
            double *B = d_sp_dense.a, *X = B + (size_t)n * SP_KB;
            HIPC(hipMemsetAsync(B, 0, sizeof(double) * (size_t)n * (size_t)nk, STREAM), ERROR_HIP_MEMCPY);
            if (nz > 0)
                hipLaunchKernelGGL(k_sp_scatter_in, dim3((nz + 255) / 256), b256, 0, STREAM, cols, nk, d_idx, d_val, (const int32_t *)nullptr, (const double *)nullptr, B,
                                   (int64_t)n);
            code = !tr ? solve(X, B, nk, n, true) : (conj_pairs ? solve_transpose(X, B, nk, n, true, true) : solve_transpose_many(X, B, nk, n, true));
            if (code != SUCCESSFUL_EXIT) return code;
            hipLaunchKernelGGL(k_sp_gather_out, gsel, b256, 0, STREAM, nout, d_sel, (const int32_t *)nullptr, (const double *)nullptr, (const double *)X, (int64_t)n, out_blk,
                               ostr, nk);
        }
        if (!on_device)
            for (int32_t c = 0; c < nk; c++)
                HIPC(hipMemcpyAsync(x_sel + (int64_t)(j0 + c) * ldx, d_sp_out.a + (size_t)c * (size_t)nout, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, STREAM),
                     ERROR_HIP_MEMCPY);
        HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    }
    HIPC(hipEventRecord((hipEvent_t)sp_ev1, STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, (hipEvent_t)sp_ev0, (hipEvent_t)sp_ev1);
    pruned_call_ms = accumulate ? pruned_call_ms + ms : ms;
    times.solve_total_ms = pruned_call_ms; // (HIP events around the call's uploads, launches and copies: dstats[8])
    return SUCCESSFUL_EXIT;
}

// values[e] = (A^{-1})(rows[e], cols[e]): the distinct columns sorted by the position their unit vector enters the elimination at
// (neighbours share most of their root paths), blocks of at most SP_KB of them, right-hand sides = unit vectors, selected rows = the union
// of the rows asked for in the block; one solve_sparse per block.
// by_rows: the mirror image through A^T -- (A^{-1})(r, c) = (A^{-T})(c, r): the distinct ROWS sorted by the position their unit vector
// enters the transposed elimination at (sp_ipos_c), sixteen of them per transposed pruned solve, the columns asked for its selection.
// pairs: indices of the complex matrix behind a real-equivalent handle (unit vector 2 u alone, rows 2 w and 2 w + 1, interleaved values).
int32_t Solver::inverse_entries(int32_t nent, const int32_t *rows, const int32_t *cols, double *values, bool by_rows, bool pairs) {
    pruned_blocks = 0, pruned_transposed_blocks = 0;
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    if (!factorized) return ERROR_NEED_FACTORIZATION;
    if (!rows || !cols || !values) return ERROR_NULL_POINTER;
    if (nent < 1) return ERROR_HIPMF_INVALID_VALUE;
    const int32_t n = pairs ? S.n / 2 : S.n, w = pairs ? 2 : 1;
    for (int32_t e = 0; e < nent; e++)
        if (rows[e] < 0 || rows[e] >= n || cols[e] < 0 || cols[e] >= n) return ERROR_HIPMF_INVALID_VALUE;
    {
        DeviceScope dev_scope(device);
        const int32_t code = sp_prepare();
        if (code != SUCCESSFUL_EXIT) return code;
    }
    std::vector<int32_t> ent((size_t)nent);
    for (int32_t e = 0; e < nent; e++) ent[(size_t)e] = e;
    const int32_t *unit = by_rows ? rows : cols, *want = by_rows ? cols : rows; // the unit right-hand sides, the rows of the solution asked for
    const std::vector<int32_t> &pos = (by_rows && !(S.sym_mode || d_tptr)) ? sp_ipos_c : sp_ipos_r;
    std::sort(ent.begin(), ent.end(), [&](int32_t a, int32_t b) {
        const int32_t pa = pos[(size_t)w * (size_t)unit[a]], pb = pos[(size_t)w * (size_t)unit[b]];
        return pa != pb ? pa < pb : (want[a] != want[b] ? want[a] < want[b] : a < b);
    });
    std::vector<int32_t> ptr, idx, sel;
    std::vector<double> val, out;
    pruned_call_ms = 0.0;
    for (size_t e0 = 0; e0 < ent.size();) {
        // entries [e0, e1): up to SP_KB distinct columns
        ptr.assign(1, 0), idx.clear(), sel.clear();
        size_t e1 = e0;
        while (e1 < ent.size()) {
            const int32_t c = w * unit[ent[e1]];
            if (idx.empty() || idx.back() != c) {
                if ((int32_t)idx.size() == SP_KB) break;
                idx.push_back(c), ptr.push_back((int32_t)idx.size());
            }
            for (int32_t h = 0; h < w; h++) sel.push_back(w * want[ent[e1]] + h);
            e1++;
        }
        std::sort(sel.begin(), sel.end());
        sel.erase(std::unique(sel.begin(), sel.end()), sel.end());
        const int32_t nk = (int32_t)idx.size(), ns = (int32_t)sel.size();
        val.assign((size_t)nk, 1.0);
        out.assign((size_t)nk * (size_t)ns, 0.0);
        const int32_t code = solve_sparse(out.data(), ns, nk, ptr.data(), idx.data(), val.data(), ns, sel.data(), false, true, by_rows);
        if (code != SUCCESSFUL_EXIT) return code;
        int32_t c = -1, last = -1;
        for (size_t e = e0; e < e1; e++) {
            const int32_t en = ent[e];
            if (unit[en] != last) last = unit[en], c++;
            const int32_t k = (int32_t)(std::lower_bound(sel.begin(), sel.end(), w * want[en]) - sel.begin());
            for (int32_t h = 0; h < w; h++) values[(size_t)w * (size_t)en + (size_t)h] = out[(size_t)c * (size_t)ns + (size_t)k + (size_t)h];
        }
        e0 = e1;
    }
    return SUCCESSFUL_EXIT;
}

// ---- error analysis of a solution xbar of A x = b (Arioli, Demmel & Duff 1989; MUMPS's RINFOG(4..11)) ----
//   a_i = sum_j |a_ij|, N_A = max a_i, N_x = |xbar|_inf, r = b - A xbar, d_i = (|A||xbar|)_i + |b_i|, tau_i = 1000 n eps (a_i N_x + |b_i|),
//   I1 = {i : d_i > tau_i}, I2 = the rest.
//   out[0] N_A, [1] N_x, [2] |r|_inf / (N_A N_x), [3] omega1 = max_{I1} |r_i| / d_i, [4] omega2 = max_{I2} |r_i| / ((|A||xbar|)_i + a_i N_x),
//   [5] omega1 cond1 + omega2 cond2, [6] cond1 = est| |A^{-1}| w1 |_inf / N_x, [7] cond2 = est| |A^{-1}| w2 |_inf / N_x
//   (w1 = d on I1, w2 = (|A||xbar|) + a N_x on I2, zeros elsewhere).
// | |A^{-1}| w |_inf = |C|_1 with C = diag(w) A^{-T} is estimated by Hager / Higham's algorithm (LAPACK dlacn2): C v = w o (A^{-T} v) is one
// transposed pass pair, C^T v = A^{-1} (w o v) one ordinary pass pair, both unrefined; at most 5 iterations + the alternating test vector,
// i.e. at most 11 pass pairs per estimate.  The vector steps run on the device (only scalars come to the host), every reduction has a
// fixed order: a repeat call gives the same bits.  (One liberty: the larger of two successive iterates' norms is kept -- both are lower
// bounds of |C|_1 -- where dlacn2 keeps the later one.)
// One core serves the real matrix and the complex twin; the policy P (EaReal, EaComplex) gives what differs.  In the COMPLEX form this
// handle holds the real-equivalent system of order n = 2 nc, xbar and rhs are nc interleaved pairs, n above is nc and |.| the complex
// modulus (include/russell_hipmf.h; the real analysis of the 2 nc system would sum |Re| + |Im| instead).  C = diag(w) A^{-H}: the
// transpose of the 2 nc system IS the real-equivalent form of A^H.  The iteration is zlacn2's: the complex sign z / |z| and no repeat
// test of the sign vector.
template <class P>
int32_t Solver::error_analysis_core(const double *xbar, const double *rhs, double *out, int32_t option) {
    const int32_t n = S.n, ne = P::elements(n);
    const size_t nb = sizeof(double) * (size_t)n;
    const bool sym = P::own_transpose(*this);
    // x | b | r | ax | arow | w1 | w2 | v | y | z | xi | t (vectors of n doubles, ax .. w2 of ne), partials, scalars
    // (kept per handle: a hipMalloc / hipFree pair of 12 n doubles per call would cost a device-wide synchronisation every time)
    if (!d_anl) HIPC(hipMalloc((void **)d_anl.put(), nb * 12 + sizeof(double) * (EA_RED_WG + 8) + sizeof(int32_t) * (EA_RED_WG + 8)), ERROR_HIP_MALLOC);
    double *X = d_anl, *B = X + n, *R = B + n, *AX = R + n, *AR = AX + ne, *W1 = AR + ne, *W2 = W1 + ne, *V = W2 + ne, *Y = V + n, *Z = Y + n,
           *XI = Z + n, *T = XI + n;
    double *pv = d_anl + 12 * (size_t)n, *sv = pv + EA_RED_WG;
    int32_t *pi = (int32_t *)(sv + 8);
    const EaWork w{STREAM, ne, dim3((ne + 255) / 256), pv, pi, (unsigned long long *)sv, pi + EA_RED_WG};
    HIPC(hipMemcpyAsync(X, xbar, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(B, rhs, nb, hipMemcpyHostToDevice, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemsetAsync(sv, 0, sizeof(double) * 8 + sizeof(int32_t) * (EA_RED_WG + 8), STREAM), ERROR_HIP_MEMCPY);
    P::rows(*this, w, X, B, R, AX, AR);
    double h[8];
    HIPC(hipMemcpyAsync(h, w.sc, sizeof(double) * 3, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    const double NA = h[0], NX = h[1], RN = h[2];
    const double tau_scale = 1000.0 * (double)ne * 2.220446049250313e-16;
    P::split(w, tau_scale, NX, R, AX, AR, B, W1, W2);
    int32_t n2 = 0;
    HIPC(hipMemcpyAsync(h + 3, w.sc + 3, sizeof(double) * 2, hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipMemcpyAsync(&n2, w.si, sizeof(int32_t), hipMemcpyDeviceToHost, STREAM), ERROR_HIP_MEMCPY);
    HIPC(hipStreamSynchronize(STREAM), ERROR_HIP_SYNCHRONIZE);
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    const double om1 = h[3], om2 = h[4];
    out[0] = NA, out[1] = NX, out[2] = (NA * NX > 0.0) ? RN / (NA * NX) : 0.0, out[3] = om1, out[4] = om2;
    analysis_solves = 0;
    if (option != 1) return SUCCESSFUL_EXIT;

    int32_t code = SUCCESSFUL_EXIT, jx = 0;
    auto reduce = [&](const double *v, int32_t mode, double *val, int32_t *idx, int32_t jprev, double *vprev) { return P::reduce(*this, w, v, mode, val, idx, jprev, vprev); };
    auto inv = [&](double *y, const double *v) -> int32_t { // y = A^{-1} v, one unrefined ordinary pass pair
        analysis_solves++;
        return solve_core(y, v, 1, n, true);
    };
    auto inv_t = [&](double *y, const double *v) -> int32_t { // y = A^{-T} v
        if (sym) return inv(y, v);
        analysis_solves++;
        return tr_pass(y, v);
    };
    // C v and C^T v of C = diag(w) A^{-T}
    auto cmul = [&](const double *d, double *y, const double *v) -> int32_t {
        const int32_t c = inv_t(T, v);
        if (c != SUCCESSFUL_EXIT) return c;
        P::hadamard(w, d, (const double *)T, y);
        return SUCCESSFUL_EXIT;
    };
    auto ctmul = [&](const double *d, double *z, const double *v) -> int32_t {
        P::hadamard(w, d, v, T);
        return inv(z, T);
    };
    auto estimate = [&](const double *d, double *est) -> int32_t {
        int32_t c;
        bool go_on = true;
        P::fill(w, 0, 0, V);
        if ((c = cmul(d, Y, V)) != SUCCESSFUL_EXIT) return c;
        if (ne == 1) return reduce(Y, 1, est, &jx, -1, nullptr);
        if ((c = reduce(Y, 0, est, &jx, -1, nullptr)) != SUCCESSFUL_EXIT) return c;
        if ((c = P::sign(*this, w, Y, XI, true, true, &go_on)) != SUCCESSFUL_EXIT) return c;
        if ((c = ctmul(d, Z, XI)) != SUCCESSFUL_EXIT) return c;
        double zmax = 0.0;
        int32_t j = 0;
        if ((c = reduce(Z, 1, &zmax, &j, -1, nullptr)) != SUCCESSFUL_EXIT) return c;
        for (int32_t iter = 2;; iter++) {
            P::fill(w, 2, j, V);
            if ((c = cmul(d, Y, V)) != SUCCESSFUL_EXIT) return c;
            const double estold = *est;
            double e = 0.0;
            if ((c = reduce(Y, 0, &e, &jx, -1, nullptr)) != SUCCESSFUL_EXIT) return c;
            *est = std::max(e, estold);
            if ((c = P::sign(*this, w, Y, XI, false, !(e <= estold), &go_on)) != SUCCESSFUL_EXIT) return c;
            if (!go_on) break;
            if ((c = ctmul(d, Z, XI)) != SUCCESSFUL_EXIT) return c;
            double zjlast = 0.0;
            if ((c = reduce(Z, 1, &zmax, &j, j, &zjlast)) != SUCCESSFUL_EXIT) return c;
            if (!(zjlast != zmax && iter < 5)) break;
        }
        P::fill(w, 1, 0, V);
        if ((c = cmul(d, Y, V)) != SUCCESSFUL_EXIT) return c;
        double e = 0.0;
        if ((c = reduce(Y, 0, &e, &jx, -1, nullptr)) != SUCCESSFUL_EXIT) return c;
        const double temp = 2.0 * (e / (3.0 * (double)ne));
        if (temp > *est) *est = temp;
        return SUCCESSFUL_EXIT;
    };
    double e1 = 0.0, e2 = 0.0;
    {
        const NestedSolveGuard guard(*this); // the statistics of the caller's solve stay as that solve left them
        guard.unrefined_quiet();
        if (ne - n2 > 0) code = estimate(W1, &e1);
        if (code == SUCCESSFUL_EXIT && n2 > 0) code = estimate(W2, &e2);
    }
    if (code != SUCCESSFUL_EXIT) return code;
    HIPC(hipGetLastError(), ERROR_HIP_LAUNCH);
    const double c1 = NX > 0.0 ? e1 / NX : 0.0, c2 = NX > 0.0 ? e2 / NX : 0.0;
    out[5] = om1 * c1 + om2 * c2, out[6] = c1, out[7] = c2;
    return SUCCESSFUL_EXIT;
}

int32_t Solver::error_analysis(const double *xbar, const double *rhs, double *out, int32_t option) {
    if (option == 0) return SUCCESSFUL_EXIT;
    DeviceScope dev_scope(device);
    const int32_t code = EaReal::own_transpose(*this) ? SUCCESSFUL_EXIT : tr_prepare(); // (A^T = A needs no transposed plan)
    return code != SUCCESSFUL_EXIT ? code : error_analysis_core<EaReal>(xbar, rhs, out, option);
}

// the complex twin (complex_solver_hipmf_solve_with_error_analysis)
int32_t Solver::error_analysis_complex(const double *xbar, const double *rhs, double *out, int32_t option) {
    if (option == 0) return SUCCESSFUL_EXIT;
    if (S.sym_mode || d_tptr || (S.n & 1)) return ERROR_HIPMF_INVALID_VALUE; // (not a real-equivalent handle)
    DeviceScope dev_scope(device);
    const int32_t code = tr_prepare();
    return code != SUCCESSFUL_EXIT ? code : error_analysis_core<EaComplex>(xbar, rhs, out, option);
}

int32_t Solver::download_pattern(std::vector<int32_t> &rp, std::vector<int32_t> &ci) {
    if (!initialized) return ERROR_NEED_INITIALIZATION;
    DeviceScope dev_scope(device);
    rp.resize((size_t)S.n + 1), ci.resize((size_t)S.nnz_a);
    HIPC(hipMemcpy(rp.data(), d_rp, sizeof(int32_t) * ((size_t)S.n + 1), hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    if (S.nnz_a > 0) HIPC(hipMemcpy(ci.data(), d_ci, sizeof(int32_t) * (size_t)S.nnz_a, hipMemcpyDeviceToHost), ERROR_HIP_MEMCPY);
    return SUCCESSFUL_EXIT;
}

} // namespace hipmf

// debug hook (tests, docs): "NAME=value when status\n" for every row of the knob table as the environment reads NOW; returns the bytes needed
extern "C" int64_t hipmf_debug_knobs(char *buf, int64_t cap) { return hipmf::Tunables::from_env().dump(buf, cap); }

#ifdef HIPMF_STAMPS
extern "C" int32_t hipmf_debug_read_stamps(unsigned long long *out, int64_t n) {
    if (n > 16 * 1024) n = 16 * 1024;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hipmf::hipmf_stamps), sizeof(unsigned long long) * (size_t)n) != hipSuccess) return 1;
    static unsigned long long zeros[16 * 1024];
    return hipMemcpyToSymbol(HIP_SYMBOL(hipmf::hipmf_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : 2;
}
#endif
