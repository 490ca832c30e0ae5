"""The substitution kernels that carry SIXTEEN right-hand sides through a front, WITHOUT refinement, on the hand-placed fronts of
tests/front_shapes.py: the blocked transposed solves (kernels_solve_transpose_blocked.hpp), the pruned pass pairs for sparse right-hand
sides (kernels_solve_pruned.hpp) and their transposed twins (kernels_solve_pruned_transpose.hpp), and the complex handle on the same kernels.

One case = one matrix of front_shapes (two_leaves_and_root with three leaves, chain, complex_two_leaves_and_root), factorised with
refinement_nstep = 0 in the natural order, and on it
  solve_transpose_many with 17 columns (a full block and a tail block), host and device form;
  solve_sparse with A and A^T under HIPMF_PRUNE_MAX_SHARE=1: 17 compressed columns whose non-zeros lie in the pivot rows of ONE leaf, every
    column against the dense column with zeros elsewhere, the empty columns exactly zero, a row selection bit for bit the rows of the
    full result;
  inverse_entries by columns and by rows against columns of A^{-1} / A^{-T};
  a stale workspace: after solve_many and a sparse solve that marks ANOTHER leaf, the sparse solve gives the bits of a fresh handle.
Every solution is judged by front_shapes.Reference.check unchanged (longdouble omega and forward error against C times unrefined LAPACK);
a handful of entries of the inverse cannot form a residual, so they take the forward-error half of the same rule, the same C.  No product
code in the reference path.  The shape lists and the emulator subset: tests/test_blocked_shapes_cpu.py; figures and the mutations the
subset catches: profiles/r23_blocked_shapes.txt."""
import ctypes as C

import numpy as np

import front_shapes as F

NRHS = 17  # one full block of sixteen columns and a tail block of one
TILED_ONLY = {"HIPMF_MID_FRONT": "0"}
PRUNE_ALWAYS = {"HIPMF_PRUNE_MAX_SHARE": "1"}  # (read per call: no block is sent to the ordinary solve because of its share)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def blocks(nrhs):
    return -(-nrhs // 16)


def counts(p):
    """non-zeros of the columns of a block, among p candidate rows: one, a few, none, ..., all"""
    return (1, 3, 0, 2, min(9, p), 1, p)


def sparse_columns(n, region, seed, ncols=NRHS, complex_values=False):
    """`ncols` compressed columns (ascending rows) with the counts of counts() in turn, non-zeros in the rows `region` only; the LAST column
    is full (all of `region`), so that a tail block is not an empty one.  Returns ptr, idx, val and the dense columns as rows."""
    rng = np.random.default_rng(seed)
    region = np.asarray(region)
    pat = counts(region.size)
    cnt = [min(pat[k % len(pat)], region.size) for k in range(ncols - 1)] + [region.size]
    ptr, idx, val = [0], [], []
    for k in cnt:
        idx += list(np.sort(rng.choice(region, size=k, replace=False)))
        v = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
        val += list(v * np.exp(1j * rng.uniform(-np.pi, np.pi, k)) if complex_values else v)
        ptr.append(len(idx))
    ptr, idx, val = np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, complex if complex_values else float)
    B = np.zeros((ncols, n), val.dtype)
    for c in range(ncols):
        B[c, idx[ptr[c]:ptr[c + 1]]] = val[ptr[c]:ptr[c + 1]]
    return ptr, idx, val, B


class Layout:
    """where a case puts things: `rhs` the rows the sparse non-zeros live in (the pivot rows of one leaf), `other` the pivot rows of another
    leaf (selected rows; the non-zeros of the call that dirties the workspace), `root` the root's rows, `fwd` the fronts on the root path
    of `rhs` (pruned_fwd_fronts), `regions` what the (row, column) pairs of inverse_entries are drawn from"""

    def __init__(self, rhs, other, root, fwd, regions, tag=""):
        self.rhs, self.other, self.root, self.fwd, self.regions, self.tag = np.asarray(rhs), np.asarray(other), np.asarray(root), fwd, regions, tag

    def select(self):
        return np.concatenate([self.other[:: max(1, self.other.size // 5)], self.root[:1], self.root[-1:]]).astype(np.int32)


def two_leaves_layout(p, m, leaves):
    leaf = [np.arange(g * p, (g + 1) * p) for g in range(leaves)]
    root = np.arange(leaves * p, leaves * p + m)
    return Layout(leaf[0], leaf[1], root, 2 if m else 1, leaf[:3] + ([root] if m else []))


def chain_layouts(p1, p2, m2):
    """(the non-zeros in the big leaf: leaf, middle front and root are marked), (in the one-pivot leaf under the root: the middle front and
    everything below it stay unmarked)"""
    under_mid, under_root, leaf = np.array([0]), np.array([1]), np.arange(2, 2 + p1)
    mid, root = np.arange(2 + p1, 2 + p1 + p2), np.arange(2 + p1 + p2, 2 + p1 + p2 + m2)
    regions = [leaf, mid, root, under_root]
    return (Layout(leaf, under_mid, root, 3, regions, " [big leaf]"), Layout(under_root, leaf, root, 2, regions, " [leaf under the root]"))


def entry_pairs(regions, seed, per_pair=2):
    """about twenty (row, column) pairs: every ordered pair of regions (leaf-leaf, leaf-root, root-leaf, root-root, a region with itself)
    `per_pair` times, a duplicate, in a shuffled order"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    k = len(regions)
    combos = [(a, b) for a in range(k) for b in range(k)]
    per = max(1, min(per_pair, 20 // len(combos)))
    for a, b in combos:
        for _ in range(per):
            rows.append(int(rng.choice(regions[a])))
            cols.append(int(rng.choice(regions[b])))
    rows.append(rows[0]), cols.append(cols[0])
    pi = rng.permutation(len(rows))
    return np.array(rows, np.int32)[pi], np.array(cols, np.int32)[pi]


def check_entries(ref, vals, at, unit, what, log):
    """vals[k] = x[at[k]] for op(A) x = e_unit.  A few entries of x form no residual: the forward-error half of Reference.check, the same C,
    the error taken over the entries that came back and measured against max |x_ref| as there"""
    e = np.zeros(ref.A.shape[0])
    e[unit] = 1.0
    x_ref, _, fe_l = ref.prepare(e)
    fe = float(np.max(np.abs(np.asarray(vals).astype(F.LD) - x_ref[at])) / np.max(np.abs(x_ref)))
    log.append("%-44s entries %d fe %.3e fe_lapack %.3e cond_inf %.3e" % (what, len(at), fe, fe_l, ref.cond))
    assert np.all(np.isfinite(vals)), what
    assert fe <= F.C * max(fe_l, F.EPS * ref.cond), (what, "forward error", fe, fe_l, ref.cond)


def _handle(lib, case, weak):
    from russell_amd.backend import Hipmf
    s = Hipmf(lib)
    try:
        if weak:  # (a maximum-product matching would put the +3 back on the diagonal: the interchanges are the point)
            assert s.set_option("matching", 0) == 0
        assert s.initialize(case.n, case.rp, case.ci, ordering=F.ORDERING_NONE, refinement_nstep=0, general_symmetric=case.symmetric) == 0
        assert s.factorize(case.v) == 0
        assert s.num_perturbed == 0 and s.counter("rematch") == 0
    except BaseException:
        s.close()
        raise
    return s


def _transpose_many_device(s, B):
    d_b, d_x = s.dev_alloc(B.nbytes), s.dev_alloc(B.nbytes)
    try:
        s.h2d(d_b, B)
        s.h2d(d_x, np.full(B.shape, np.nan))
        s.solve_transpose_many_device(d_x, d_b, B.shape[0])
        X = np.zeros(B.shape)
        s.d2h(X, d_x)
        return X
    finally:
        s.dev_free(d_b)
        s.dev_free(d_x)


def run_case(lib, case, expect, weak, env, log, name, layouts):
    """every call of the module's docstring on one real matrix; `layouts`: one Layout per placement of the sparse non-zeros"""
    n, sym = case.n, case.symmetric
    ref = F.Reference(case.A)
    ref_t = ref.transposed()
    refs = {False: ref, True: ref_t}
    rng = np.random.default_rng(5)
    B = rng.standard_normal((NRHS, n))
    with F.environment(dict(env, **PRUNE_ALWAYS)):
        s = _handle(lib, case, weak)
        fresh = None
        try:
            got = F.reached(s)
            nsuper = got["nsuper"]
            log.append("%-40s n %d asked %s reached %s" % (name, n, expect, got))
            for k, val in expect.items():
                assert got[k] == val, (name, k, got, expect)
            assert got["symmetric_ldlt"] == int(sym)

            # 1. solve_transpose_many, host and device form (A^T = A: the ordinary blocked solve, no transposed block)
            for form, X in (("host", s.solve_transpose_many(B)), ("device", _transpose_many_device(s, B))):
                assert s.counter("transposed_blocks") == (0 if sym else blocks(NRHS)), (name, form)
                for j in range(NRHS):
                    ref_t.check(X[j], B[j], "%s transpose_many (%s) col %d" % (name, form, j), log)

            for lay in layouts:
                tag = name + lay.tag
                ptr, idx, val, Bs = sparse_columns(n, lay.rhs, 7)
                sel = lay.select()
                # 2. sparse right-hand sides, A and A^T
                full = {}
                for tr in (False, True):
                    what = "%s sparse%s" % (tag, " transposed" if tr else "")
                    X = s.solve_sparse(ptr, idx, val, transpose=tr)
                    assert s.counter("pruned_blocks") == blocks(NRHS), what
                    assert s.counter("pruned_transposed_blocks") == (blocks(NRHS) if tr and not sym else 0), what
                    assert s.counter("pruned_fwd_fronts") == lay.fwd and lay.fwd < nsuper, (what, s.counter("pruned_fwd_fronts"), lay.fwd, nsuper)
                    assert s.counter("pruned_bwd_fronts") == nsuper, what
                    for j in range(NRHS):
                        if ptr[j + 1] == ptr[j]:
                            assert not X[j].any(), (what, "the empty column", j)
                        else:
                            refs[tr].check(X[j], Bs[j], "%s col %d" % (what, j), log)
                    Xs = s.solve_sparse(ptr, idx, val, select=sel, transpose=tr)
                    assert s.counter("pruned_blocks") == blocks(NRHS) and s.counter("pruned_bwd_fronts") < nsuper, (what, s.counter("pruned_bwd_fronts"), nsuper)
                    assert np.array_equal(bits(Xs), bits(X[:, sel])), (what, "selected rows")
                    full[tr] = X

                # 3. entries of the inverse, by columns (A x = e_col) and by rows (A^T y = e_row)
                rows, cols = entry_pairs(lay.regions, 11)
                for by_rows in (False, True):
                    what = "%s inverse_entries%s" % (tag, " by rows" if by_rows else "")
                    vals = s.inverse_entries(rows, cols, by_rows=by_rows)
                    unit, want = (rows, cols) if by_rows else (cols, rows)
                    assert s.counter("pruned_blocks") == blocks(np.unique(unit).size), what
                    assert s.counter("pruned_transposed_blocks") == (blocks(np.unique(unit).size) if by_rows and not sym else 0), what
                    for u in np.unique(unit):
                        k = np.flatnonzero(unit == u)
                        check_entries(refs[by_rows], vals[k], want[k], u, "%s unit %d" % (what, u), log)

                # 4. stale workspace: the ordinary blocked solve, a sparse solve that marks ANOTHER leaf, then the solve of 2. again
                if fresh is None:
                    fresh = _handle(lib, case, weak)
                optr, oidx, oval, _ = sparse_columns(n, lay.other, 9)
                for tr in (False, True):
                    what = "%s stale workspace%s" % (tag, " transposed" if tr else "")
                    Xf = fresh.solve_sparse(ptr, idx, val, transpose=tr)
                    s.solve_many(B)
                    s.solve_sparse(optr, oidx, oval, transpose=tr)
                    Xl = s.solve_sparse(ptr, idx, val, transpose=tr)
                    assert s.counter("pruned_fwd_fronts") == lay.fwd, what
                    assert np.array_equal(bits(Xl), bits(Xf)), (what, "against a fresh handle", float(np.max(np.abs(Xl - Xf))))
                    assert np.array_equal(bits(Xl), bits(full[tr])), (what, "against the first call")
                fresh.close()
                fresh = None  # (the next placement starts from a fresh handle again)
            assert s.num_perturbed == 0 and s.counter("rematch") == 0
            assert s.stats()["refinement_steps"] == 0 and s.counter("krylov_iterations") == 0
        finally:
            s.close()
            if fresh is not None:
                fresh.close()


# ---- the complex handle, through the raw C-ABI ------------------------------------------------------------------------------------------

COMPLEX_LEAVES = 3
OPS = {0: lambda Z: Z, 1: lambda Z: Z.T.copy(), 2: lambda Z: Z.conj().T.copy()}  # trans of complex_solver_hipmf_solve_sparse: A, A^T, A^H


def run_complex(lib_path, p, m, symmetric, log):
    """complex_solver_hipmf_solve_many (17 columns), _solve_transpose_many (conjugate 0, 1) and _solve_sparse (A, A^T, A^H) without
    refinement against the complex longdouble reference of Z, Z^T, Z^H; weak pivot blocks in general storage"""
    from russell_amd._capi import load
    from russell_amd.backend import Hipmf
    Z, rp, ci, zv = F.complex_two_leaves_and_root(p, m, 100 * p + m, weak=not symmetric, symmetric=symmetric, leaves=COMPLEX_LEAVES)
    n = Z.shape[0]
    name = "complex p=%d m=%d %s" % (p, m, "symmetric-lower" if symmetric else "general")
    lib = load(lib_path)
    rng = np.random.default_rng(5)
    B = rng.standard_normal((NRHS, n)) + 1j * rng.standard_normal((NRHS, n))
    refs = {t: F.ComplexReference(op(Z)) for t, op in OPS.items()}
    want = F.expect_two_leaves(2 * p, 2 * m, COMPLEX_LEAVES)  # the real-equivalent fronts: twice the complex pivots and rows
    lay = two_leaves_layout(p, m, COMPLEX_LEAVES)
    ptr, idx, val, Bs = sparse_columns(n, lay.rhs, 7, complex_values=True)
    sel = lay.select()
    flat = lambda a: np.ascontiguousarray(a, np.complex128).view(np.float64).reshape(-1)
    h = lib.complex_solver_hipmf_new()
    assert h
    try:
        with F.environment({"HIPMF_MATCHING": "0"}):  # (matching: see front_shapes.run_case)
            assert lib.complex_solver_hipmf_initialize(h, F.ORDERING_NONE, 1, -1.0, 0, 0, int(symmetric), n, rp, ci, None) == 0
        npert = C.c_int32()
        assert lib.complex_solver_hipmf_factorize(h, None, None, C.byref(npert), None, None, None, None, 0, 0, zv) == 0
        assert npert.value == 0
        ist, dst = np.zeros(16, np.int64), np.zeros(16)
        assert lib.complex_solver_hipmf_get_stats(h, ist, dst) == 0
        counter = lambda k: int(lib.complex_solver_hipmf_get_counter(h, Hipmf.COUNTERS[k]))
        got = {"nsuper": int(ist[2]), "max_front": int(ist[6]), "max_pivots": int(ist[7]), "mid_fronts": counter("mid_fronts")}
        nsuper = got["nsuper"]
        log.append("%-44s n %d asked %s reached %s" % (name, n, want, got))
        # (symmetric-lower complex storage is mirrored to general storage: the paired pivot searches are LU searches)
        assert got == want and counter("rematch") == 0 and counter("symmetric_ldlt") == 0, (name, got, want)

        X = np.zeros((NRHS, n), np.complex128)
        assert lib.complex_solver_hipmf_solve_many(h, flat(X), flat(B), NRHS, n, 0) == 0
        for j in range(NRHS):
            refs[0].check(X[j], B[j], "%s many col %d" % (name, j), log)
        for conjugate in (0, 1):
            X = np.zeros((NRHS, n), np.complex128)
            assert lib.complex_solver_hipmf_solve_transpose_many(h, flat(X), flat(B), NRHS, n, conjugate, 0) == 0
            assert counter("transposed_blocks") == blocks(NRHS), (name, conjugate)
            for j in range(NRHS):
                refs[1 + conjugate].check(X[j], B[j], "%s transpose_many conjugate %d col %d" % (name, conjugate, j), log)
        with F.environment(PRUNE_ALWAYS):
            for t in OPS:
                what = "%s sparse trans %d" % (name, t)
                X = np.zeros((NRHS, n), np.complex128)
                assert lib.complex_solver_hipmf_solve_sparse(h, flat(X), n, NRHS, ptr, idx, flat(val), 0, None, t, 0) == 0
                assert counter("pruned_blocks") == blocks(NRHS), what
                assert counter("pruned_transposed_blocks") == (blocks(NRHS) if t == 2 or (t == 1 and not symmetric) else 0), what
                assert counter("pruned_fwd_fronts") == lay.fwd and lay.fwd < nsuper and counter("pruned_bwd_fronts") == nsuper, what
                for j in range(NRHS):
                    if ptr[j + 1] == ptr[j]:
                        assert not X[j].any(), (what, "the empty column", j)
                    else:
                        refs[t].check(X[j], Bs[j], "%s col %d" % (what, j), log)
                Xs = np.zeros((NRHS, sel.size), np.complex128)
                assert lib.complex_solver_hipmf_solve_sparse(h, flat(Xs), sel.size, NRHS, ptr, idx, flat(val), sel.size, sel.ctypes.data, t, 0) == 0
                assert counter("pruned_bwd_fronts") < nsuper, what
                assert np.array_equal(bits(flat(Xs)), bits(flat(X[:, sel]))), (what, "selected rows")
        assert lib.complex_solver_hipmf_get_stats(h, ist, dst) == 0
        assert int(ist[10]) == 0 and counter("krylov_iterations") == 0
    finally:
        lib.complex_solver_hipmf_drop(h)
