"""Thin object wrapper over the C-ABI (include/russell_hipmf.h): one handle = one solver on one GPU.

This is plumbing for tests / bench / the Python mirror of the Rust host layer (russell_amd.sparse).
It adds no numerics of its own; every number comes out of the HIP library.
"""
import ctypes as C

import numpy as np

from . import _capi

ISTAT_NAMES = ["ndim", "nnz_a", "nsuper", "nlevels", "nnz_l", "nnz_u", "max_front", "max_pivots", "n_perturbed", "n_zero_pivot",
               "refinement_steps", "factor_launches", "solve_launches", "pool_bytes", "matched", "fused_fallbacks"]
DSTAT_NAMES = ["flops", "flops_gemm", "ordering_s", "symbolic_s", "assemble_ms", "factor_ms", "fwd_ms", "bwd_ms", "solve_total_ms",
               "residual_inf", "acc_assemble_ms", "acc_factor_ms", "acc_factor_count", "acc_fwd_ms", "acc_bwd_ms", "acc_tri_count"]


class HipmfError(RuntimeError):
    def __init__(self, code, where, detail=""):
        super().__init__("%s failed with status %d %s" % (where, code, detail))
        self.code = code


class Hipmf:
    def __init__(self, lib_path=None):
        self.lib = _capi.load(lib_path)
        self.h = self.lib.solver_hipmf_new()
        if not self.h:
            raise RuntimeError("solver_hipmf_new returned NULL: no HIP device visible (there is no CPU fallback)")
        self.n = 0
        self.nnz = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.solver_hipmf_drop(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _err(self, code, where):
        return HipmfError(code, where, (self.lib.solver_hipmf_last_error(self.h) or b"").decode())

    def initialize(self, n, row_pointers, col_indices, ordering=0, scaling=1, pivot_epsilon=-1.0, refinement_nstep=-1,
                   verbose=False, general_symmetric=False, positive_definite=False, values=None):
        """values (optional, as in the reference's shims, which hand the numbers to the analysis phase too): lets the
        analysis apply the maximum-product matching + scaling when the diagonal is weak."""
        rp = np.ascontiguousarray(row_pointers, dtype=np.int32)
        ci = np.ascontiguousarray(col_indices, dtype=np.int32)
        self.n, self.nnz = int(n), int(rp[n])
        vptr = None
        if values is not None:
            self._init_values = np.ascontiguousarray(values, dtype=np.float64)
            assert self._init_values.size >= self.nnz
            vptr = self._init_values.ctypes.data
        return self.lib.solver_hipmf_initialize(self.h, ordering, scaling, pivot_epsilon, refinement_nstep, int(verbose),
                                                int(general_symmetric), int(positive_definite), n, rp, ci, vptr)

    def factorize(self, values, compute_determinant=False, verbose=False):
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.size >= self.nnz
        eo, es, npv = C.c_int32(), C.c_int32(), C.c_int32()
        rc, dc, de = C.c_double(), C.c_double(), C.c_double()
        code = self.lib.solver_hipmf_factorize(self.h, C.byref(eo), C.byref(es), C.byref(npv), C.byref(rc), C.byref(dc), C.byref(de),
                                               int(compute_determinant), int(verbose), v)
        self.effective_ordering, self.effective_scaling, self.num_perturbed = eo.value, es.value, npv.value
        self.rcond, self.det_coefficient, self.det_exponent = rc.value, dc.value, de.value
        return code

    def set_value_map(self, seg_ptr, seg_idx):
        """CSR entry j <- sum of input[seg_idx[seg_ptr[j]:seg_ptr[j+1]]] (e.g. COO triplets with duplicates)."""
        sp = np.ascontiguousarray(seg_ptr, dtype=np.int32)
        si = np.ascontiguousarray(seg_idx, dtype=np.int32)
        self.nnz_in = int(si.size)
        return self.lib.solver_hipmf_set_value_map(self.h, self.nnz_in, sp, si)

    def factorize_mapped(self, input_values, compute_determinant=False, verbose=False):
        v = np.ascontiguousarray(input_values, dtype=np.float64)
        assert v.size >= self.nnz_in
        eo, es, npv = C.c_int32(), C.c_int32(), C.c_int32()
        rc, dc, de = C.c_double(), C.c_double(), C.c_double()
        code = self.lib.solver_hipmf_factorize_mapped(self.h, C.byref(eo), C.byref(es), C.byref(npv), C.byref(rc), C.byref(dc),
                                                      C.byref(de), int(compute_determinant), int(verbose), v)
        self.effective_ordering, self.effective_scaling, self.num_perturbed = eo.value, es.value, npv.value
        self.rcond, self.det_coefficient, self.det_exponent = rc.value, dc.value, de.value
        return code

    def solve(self, rhs, verbose=False):
        b = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros(self.n)
        code = self.lib.solver_hipmf_solve(self.h, x, b, int(verbose))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve")
        return x

    def solve_transpose(self, rhs, verbose=False):
        """x = A^{-T} rhs with the factor of A (L D L^T / symmetric storage: the ordinary solve)."""
        b = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros(self.n)
        code = self.lib.solver_hipmf_solve_transpose(self.h, x, b, int(verbose))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_transpose")
        return x

    def solve_with_error_analysis(self, rhs, option, verbose=False, array=None):
        """(x, the eight MUMPS-style values) -- x as solve() returns it; option 1: all eight, 2: entries 0 - 4, 0: none (array untouched)."""
        b = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros(self.n)
        ea = np.zeros(8) if array is None else array
        code = self.lib.solver_hipmf_solve_with_error_analysis(self.h, x, b, ea, int(option), int(verbose))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_with_error_analysis")
        return x, ea

    def solve_many(self, rhs_colmajor, ld=None):
        """rhs_colmajor: array of shape (nrhs, ld) whose rows hold the right-hand sides in their first n entries (= column-major
        ld x nrhs; ld defaults to n).  Returns x in the same layout: zeros where the library writes nothing, except that the
        ld - n padding entries of every row are those of rhs_colmajor."""
        b = np.ascontiguousarray(rhs_colmajor, dtype=np.float64)
        ld = self.n if ld is None else int(ld)
        if b.ndim != 2 or b.shape[1] != ld:
            raise ValueError("solve_many expects an array of shape (nrhs, ld) with ld = %d, got %r" % (ld, b.shape))
        nrhs = b.shape[0]
        x = np.zeros_like(b)
        x[:, self.n:] = b[:, self.n:]
        code = self.lib.solver_hipmf_solve_many(self.h, x, b, nrhs, ld, 0)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_many")
        return x

    def solve_transpose_many(self, rhs_colmajor, ld=None):
        """X = A^{-T} B for an array of shape (nrhs, ld) as solve_many takes and returns it; 16 columns per pass pair over the factor."""
        b = np.ascontiguousarray(rhs_colmajor, dtype=np.float64)
        ld = self.n if ld is None else int(ld)
        if b.ndim != 2 or b.shape[1] != ld:
            raise ValueError("solve_transpose_many expects an array of shape (nrhs, ld) with ld = %d, got %r" % (ld, b.shape))
        nrhs = b.shape[0]
        x = np.zeros_like(b)
        x[:, self.n:] = b[:, self.n:]
        code = self.lib.solver_hipmf_solve_transpose_many(self.h, x, b, nrhs, ld, 0)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_transpose_many")
        return x

    def solve_sparse(self, rhs_ptr, rhs_idx, rhs_val, select=None, ldx=None, verbose=False, transpose=False):
        """Rows `select` (None: all n) of A^{-1} B for B in compressed-column form (rhs_ptr of nrhs + 1 entries, 0-based row indices ascending
        within a column): an array of shape (nrhs, ldx) whose rows hold the columns' selected entries in their first nsel places (ldx
        defaults to nsel).  One unrefined pass pair over the marked fronts per block of 16 columns.  transpose: A^{-T} B
        (solver_hipmf_solve_sparse_transpose)."""
        name = "solver_hipmf_solve_sparse_transpose" if transpose else "solver_hipmf_solve_sparse"
        ptr = np.ascontiguousarray(rhs_ptr, dtype=np.int32)
        idx = np.ascontiguousarray(rhs_idx, dtype=np.int32)
        val = np.ascontiguousarray(rhs_val, dtype=np.float64)
        nrhs = int(ptr.size) - 1
        sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
        nsel = self.n if sel is None else int(sel.size)
        ldx = nsel if ldx is None else int(ldx)
        x = np.zeros((max(nrhs, 0), max(ldx, 0)))
        code = getattr(self.lib, name)(self.h, x, ldx, nrhs, ptr, idx, val, nsel, None if sel is None else sel.ctypes.data, int(verbose))
        if code != 0:
            raise self._err(code, name)
        return x

    def inverse_entries(self, rows, cols, verbose=False, by_rows=False):
        """(A^{-1})[rows[e], cols[e]] for every e (any order, duplicates allowed), 16 distinct columns per pruned pass pair; by_rows: 16
        distinct rows per transposed pruned pass pair (solver_hipmf_inverse_entries_by_rows)."""
        name = "solver_hipmf_inverse_entries_by_rows" if by_rows else "solver_hipmf_inverse_entries"
        r = np.ascontiguousarray(rows, dtype=np.int32)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        if r.shape != c.shape or r.ndim != 1:
            raise ValueError("inverse_entries expects two index vectors of equal length, got %r and %r" % (r.shape, c.shape))
        v = np.zeros(r.size)
        code = getattr(self.lib, name)(self.h, int(r.size), r, c, v, int(verbose))
        if code != 0:
            raise self._err(code, name)
        return v

    def solve_updated(self, rhs, values, mapped=False, rel_tol=0.0, max_steps=0, verbose=False, transpose=False):
        """A_new x = rhs for the matrix with the structure of initialize and the `values` given here (mapped: the inputs of the installed
        value map), by flexible GMRES on the device with the kept factor as right preconditioner; transpose: A_new^T x = rhs
        (solver_hipmf_solve_updated_transpose).  Returns (x, steps, relres, status):
        status 0 = converged, 2 = HIPMF_WARNING_NOT_CONVERGED (x is the best iterate); any other status raises."""
        name = "solver_hipmf_solve_updated_transpose" if transpose else "solver_hipmf_solve_updated"
        x = np.zeros(self.n)
        steps, relres = C.c_int32(0), C.c_double(0.0)
        code = getattr(self.lib, name)(self.h, x, np.ascontiguousarray(rhs, dtype=np.float64), np.ascontiguousarray(values, dtype=np.float64),
                                       int(bool(mapped)), float(rel_tol), int(max_steps), C.byref(steps), C.byref(relres), int(verbose))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, name)
        return x, int(steps.value), float(relres.value), code

    def solve_updated_many(self, rhs_colmajor, values, mapped=False, rel_tol=0.0, max_steps=0, ld=None, verbose=False, transpose=False):
        """solve_updated for the right-hand sides of an array of shape (nrhs, ld) as solve_many takes it, 16 columns per blocked pass pair,
        every column its own iteration; transpose: A_new^T X = B (solver_hipmf_solve_updated_transpose_many).  Returns (x, steps, relres,
        status): x in the layout of solve_many, steps and relres NumPy arrays
        of nrhs entries, status 0 = every column converged, 2 = at least one did not (relres tells which); any other status raises."""
        name = "solver_hipmf_solve_updated_transpose_many" if transpose else "solver_hipmf_solve_updated_many"
        b = np.ascontiguousarray(rhs_colmajor, dtype=np.float64)
        ld = self.n if ld is None else int(ld)
        if b.ndim != 2 or b.shape[1] != ld:
            raise ValueError("solve_updated_many expects an array of shape (nrhs, ld) with ld = %d, got %r" % (ld, b.shape))
        nrhs = b.shape[0]
        x = np.zeros_like(b)
        x[:, self.n:] = b[:, self.n:]
        steps, relres = np.zeros(nrhs, np.int32), np.zeros(nrhs)
        code = getattr(self.lib, name)(self.h, x, b, nrhs, ld, np.ascontiguousarray(values, dtype=np.float64), int(bool(mapped)), float(rel_tol),
                                       int(max_steps), steps.ctypes.data, relres.ctypes.data, int(verbose))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, name)
        return x, steps, relres, code

    def solve_extra_precise(self, rhs, tail=False, dx_tol=0.0, max_steps=0, verbose=False):
        """Extra-precise iterative refinement of A x = rhs (the residual in twice the working precision, solver_hipmf_solve_extra_precise).
        Returns (x, x_tail or None, info, status): info the eight values of include/russell_hipmf.h (steps, dn, normwise bound, dc,
        componentwise bound, rho_max, state, tail carried); tail=True keeps the solution as x + x_tail; status 0 = converged,
        2 = HIPMF_WARNING_NOT_CONVERGED (x is the best iterate); any other status raises."""
        x, info = np.zeros(self.n), np.zeros(8)
        t = np.zeros(self.n) if tail else None
        code = self.lib.solver_hipmf_solve_extra_precise(self.h, x, None if t is None else t.ctypes.data, np.ascontiguousarray(rhs, dtype=np.float64),
                                                         float(dx_tol), int(max_steps), info.ctypes.data, int(verbose))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, "solver_hipmf_solve_extra_precise")
        return x, t, info, code

    def solve_extra_precise_many(self, rhs_colmajor, tail=False, dx_tol=0.0, max_steps=0, ld=None, verbose=False, x=None, x_tail=None):
        """solve_extra_precise for the right-hand sides of an array of shape (nrhs, ld) as solve_many takes it, 16 columns per pass pair.
        Returns (x, x_tail or None, info, status) with x and x_tail in that layout and info of shape (nrhs, 8); x / x_tail: arrays of
        that shape to write into (their entries n .. ld - 1 of every row are left alone)."""
        b = np.ascontiguousarray(rhs_colmajor, dtype=np.float64)
        ld = self.n if ld is None else int(ld)
        if b.ndim != 2 or b.shape[1] != ld:
            raise ValueError("solve_extra_precise_many expects an array of shape (nrhs, ld) with ld = %d, got %r" % (ld, b.shape))
        nrhs = b.shape[0]
        x = np.zeros_like(b) if x is None else x
        t = (np.zeros_like(b) if x_tail is None else x_tail) if (tail or x_tail is not None) else None
        info = np.zeros((nrhs, 8))
        code = self.lib.solver_hipmf_solve_extra_precise_many(self.h, x, None if t is None else t.ctypes.data, b, nrhs, ld, float(dx_tol), int(max_steps),
                                                              info.ctypes.data, int(verbose))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, "solver_hipmf_solve_extra_precise_many")
        return x, t, info, code

    WARNING_SINGULAR_MATRIX = 1

    def set_border(self, B, C_, D, verbose=False):
        """The border of [A B; C^T D] on the kept factor (solver_hipmf_set_border): B, C_ of shape (n, k), D of shape (k, k); k = 0 (or
        B None) drops it.  Returns (border_info, status): min / max |u_ii| of S = D - C^T A^{-1} B, mantissa and base-10 exponent of
        det S, device bytes held; status 0 or WARNING_SINGULAR_MATRIX (an exactly zero pivot of S: no border is set); others raise."""
        info = np.zeros(4)
        if B is None or np.asarray(B).size == 0:
            code = self.lib.solver_hipmf_set_border(self.h, 0, None, 0, None, 0, None, 0, info.ctypes.data, int(verbose))
        else:
            Bf, Cf, Df = (np.asfortranarray(np.asarray(a, dtype=np.float64).reshape(np.shape(a)[0], -1)) for a in (B, C_, D))
            k = Bf.shape[1]
            if Bf.shape != (self.n, k) or Cf.shape != (self.n, k) or Df.shape != (k, k):
                raise ValueError("set_border expects B, C of shape (%d, k) and D of shape (k, k), got %r, %r, %r" % (self.n, Bf.shape, Cf.shape, Df.shape))
            code = self.lib.solver_hipmf_set_border(self.h, k, Bf.ctypes.data, self.n, Cf.ctypes.data, self.n, Df.ctypes.data, k, info.ctypes.data, int(verbose))
        if code not in (0, self.WARNING_SINGULAR_MATRIX):
            raise self._err(code, "solver_hipmf_set_border")
        return info, code

    def solve_bordered(self, f, g=None, want_z=True, max_steps=0, ldx=None, ldz=None, verbose=False, x=None, z=None):
        """[A B; C^T D] [x; z] = [f; g] with the border of set_border, refined on the whole system (solver_hipmf_solve_bordered).
        f: (n,) or (nrhs, ldx) as solve_many takes it; g: (k,) or (nrhs, ldz), None: g = 0; want_z False: z is not returned.
        x / z: arrays of those shapes to write into (their padding is left alone).  Returns (x, z or None, info of shape (nrhs, 4))."""
        return self._solve_bordered("solver_hipmf_solve_bordered", f, g, want_z, max_steps, ldx, ldz, verbose, x, z)

    def solve_bordered_transpose(self, p, q=None, want_w=True, max_steps=0, ldx=None, ldz=None, verbose=False, y=None, w=None):
        """[A^T C; B^T D^T] [y; w] = [p; q], the transpose of solve_bordered's system with the same border
        (solver_hipmf_solve_bordered_transpose).  Arguments and results as solve_bordered: returns (y, w or None, info)."""
        return self._solve_bordered("solver_hipmf_solve_bordered_transpose", p, q, want_w, max_steps, ldx, ldz, verbose, y, w)

    def _solve_bordered(self, entry, f, g, want_z, max_steps, ldx, ldz, verbose, x, z):
        k = self.counter("border_columns")
        fa = np.ascontiguousarray(f, dtype=np.float64)
        single = fa.ndim == 1
        fa = fa.reshape(1, -1) if single else fa
        nrhs = fa.shape[0]
        ldx = fa.shape[1] if ldx is None else int(ldx)
        ga = None if g is None else np.ascontiguousarray(g, dtype=np.float64).reshape(nrhs, -1)
        ldz = (k if ga is None else ga.shape[1]) if ldz is None else int(ldz)
        x = np.zeros((nrhs, ldx)) if x is None else x
        z = (np.zeros((nrhs, max(ldz, 1))) if z is None else z) if want_z else None
        info = np.zeros((nrhs, 4))
        code = getattr(self.lib, entry)(self.h, x.ctypes.data, None if z is None else z.ctypes.data, fa.ctypes.data, None if ga is None else ga.ctypes.data, nrhs, ldx,
                                        ldz, int(max_steps), info.ctypes.data, int(verbose))
        if code != 0:
            raise self._err(code, entry)
        if single:
            return x[0], (None if z is None else z[0]), info[0]
        return x, z, info

    ERROR_NOT_AVAILABLE = 400000

    def inertia(self):
        """(n_positive, n_negative, n_zero, status) of the factorised matrix from the signs of the pivots of L D L^T
        (solver_hipmf_get_inertia): status 0, or WARNING_SINGULAR_MATRIX when pivots were replaced or zero (they are counted in n_zero).
        Raises HipmfError with code ERROR_NOT_AVAILABLE where the factor is no L D L^T (a general or an expanded handle)."""
        pos, neg, zero = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        code = self.lib.solver_hipmf_get_inertia(self.h, C.addressof(pos), C.addressof(neg), C.addressof(zero))
        if code not in (0, self.WARNING_SINGULAR_MATRIX):
            raise self._err(code, "solver_hipmf_get_inertia")
        return int(pos.value), int(neg.value), int(zero.value), code

    def eigs_near_shift(self, nev, sigma, m_values=None, mapped=False, ncv=0, v0=None, tol=0.0, max_steps=0, ldx=None, verbose=False):
        """The nev eigenpairs of K x = lambda M x nearest sigma on a handle that holds the factor of K - sigma M
        (solver_hipmf_eigs_near_shift): m_values are M's values on the handle's pattern as solve_updated takes values (None: M = I),
        v0 a start vector or None.  Returns (lambda, X, backward_error, nconv, steps, status): lambda and backward_error of nev
        entries, X of shape (nev, ldx) whose rows hold the eigenvectors in their first n entries (= column-major ldx x nev);
        status 0 = nev pairs converged, 2 = HIPMF_WARNING_NOT_CONVERGED (the best nev Ritz pairs, converged first); others raise."""
        nev = int(nev)
        ldx = self.n if ldx is None else int(ldx)
        lam, be = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        X = np.zeros((max(nev, 1), max(ldx, 1)))
        mv = None if m_values is None else np.ascontiguousarray(m_values, dtype=np.float64)
        if mv is not None:
            assert mv.size >= self._value_count(mapped)
        v = None if v0 is None else np.ascontiguousarray(v0, dtype=np.float64)
        nconv, steps = C.c_int32(0), C.c_int32(0)
        code = self.lib.solver_hipmf_eigs_near_shift(self.h, nev, int(ncv), float(sigma), None if mv is None else mv.ctypes.data, int(bool(mapped)),
                                                     None if v is None else v.ctypes.data, float(tol), int(max_steps), lam.ctypes.data, X.ctypes.data, ldx,
                                                     be.ctypes.data, C.addressof(nconv), C.addressof(steps), int(verbose))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, "solver_hipmf_eigs_near_shift")
        return lam[:nev], X[:nev], be[:nev], int(nconv.value), int(steps.value), code

    def eigs_near_shift_device(self, nev, sigma, d_X, d_m_values=None, mapped=False, ncv=0, d_v0=None, tol=0.0, max_steps=0, ldx=None):
        """eigs_near_shift with M's values, the start vector and X (column-major ldx x nev) resident on the device; returns
        (lambda, backward_error, nconv, steps, status)"""
        nev = int(nev)
        lam, be = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        nconv, steps = C.c_int32(0), C.c_int32(0)
        code = self.lib.solver_hipmf_eigs_near_shift_device(self.h, nev, int(ncv), float(sigma), d_m_values, int(bool(mapped)), d_v0, float(tol), int(max_steps),
                                                            lam.ctypes.data, d_X, int(ldx or self.n), be.ctypes.data, C.addressof(nconv), C.addressof(steps))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, "solver_hipmf_eigs_near_shift_device")
        return lam[:nev], be[:nev], int(nconv.value), int(steps.value), code

    def _value_count(self, mapped):
        """entries of a value array of this handle: the inputs of the value map (mapped) or what factorize takes"""
        return int(self.nnz_in) if mapped else int(self.nnz)

    @staticmethod
    def _columns(a, n, what):
        """(array of shape (ncols, ld), single) from a vector of n entries or an array of shape (ncols, ld) as solve_many takes it"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        single = a.ndim == 1
        a = a.reshape(1, -1) if single else a
        if a.ndim != 2 or a.shape[1] < n:
            raise ValueError("%s expects a vector of %d entries or an array of shape (ncols, ld >= %d), got %r" % (what, n, n, a.shape))
        return a, single

    def values_outer(self, u, w, alpha=1.0, beta=0.0, grad=None, mapped=False):
        """grad = beta grad + alpha sum_c u_c w_c^T restricted to the pattern, in the order of the values handed to factorize (mapped: to
        factorize_mapped); solver_hipmf_values_outer.  u, w: vectors or arrays of shape (ncols, ld) as solve_many takes them.  grad: the
        array to update (beta = 0: it is not read), None: a new one.  Needs initialize only."""
        ua, _ = self._columns(u, self.n, "values_outer")
        wa, _ = self._columns(w, self.n, "values_outer")
        if ua.shape[0] != wa.shape[0]:
            raise ValueError("values_outer: u has %d columns, w %d" % (ua.shape[0], wa.shape[0]))
        g = np.zeros(self._value_count(mapped)) if grad is None else grad
        code = self.lib.solver_hipmf_values_outer(self.h, g.ctypes.data, ua.ctypes.data, wa.ctypes.data, ua.shape[0], ua.shape[1], wa.shape[1], float(alpha),
                                                  float(beta), int(bool(mapped)))
        if code != 0:
            raise self._err(code, "solver_hipmf_values_outer")
        return g

    def solve_tangent(self, x, dvalues, db=None, mapped=False, dx=None):
        """dx = A^{-1} (db - dA x) for the matrix dA that dvalues describe (solver_hipmf_solve_tangent); x, db (None: zero): vectors or
        arrays of shape (nrhs, ld); dx: an array of that shape to write into (its padding is left alone), None: a new one."""
        xa, single = self._columns(x, self.n, "solve_tangent")
        ba = None if db is None else self._columns(db, self.n, "solve_tangent")[0]
        if ba is not None and ba.shape != xa.shape:
            raise ValueError("solve_tangent: x has shape %r, db %r" % (xa.shape, ba.shape))
        out = np.zeros_like(xa) if dx is None else dx
        code = self.lib.solver_hipmf_solve_tangent(self.h, out.ctypes.data, xa.ctypes.data, np.ascontiguousarray(dvalues, dtype=np.float64).ctypes.data,
                                                   None if ba is None else ba.ctypes.data, xa.shape[0], xa.shape[1], int(bool(mapped)))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_tangent")
        return out.reshape(xa.shape)[0] if single and dx is None else out

    def solve_adjoint(self, g, x=None, beta=0.0, grad=None, mapped=False, want_grad=True, lam=None):
        """lambda = A^{-T} g and grad = beta grad - sum_c lambda_c x_c^T restricted to the pattern, in the caller's value order
        (solver_hipmf_solve_adjoint).  g, x: vectors or arrays of shape (nrhs, ld); lam: the array lambda is written into (it may be g),
        None: a new one; want_grad False: the solve alone.  Returns (lambda, grad or None)."""
        ga, single = self._columns(g, self.n, "solve_adjoint")
        xa = None if x is None else self._columns(x, self.n, "solve_adjoint")[0]
        if want_grad and (xa is None or xa.shape != ga.shape):
            raise ValueError("solve_adjoint: the gradient needs x in the shape of g")
        out = np.zeros_like(ga) if lam is None else lam
        gr = None if not want_grad else (np.zeros(self._value_count(mapped)) if grad is None else grad)
        code = self.lib.solver_hipmf_solve_adjoint(self.h, out.ctypes.data, None if gr is None else gr.ctypes.data, None if xa is None else xa.ctypes.data,
                                                   ga.ctypes.data, ga.shape[0], ga.shape[1], float(beta), int(bool(mapped)))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_adjoint")
        return (out.reshape(ga.shape)[0] if single and lam is None else out), gr

    def mat_vec_mul(self, u, alpha=1.0):
        v = np.zeros(self.n)
        code = self.lib.solver_hipmf_mat_vec_mul(self.h, v, alpha, np.ascontiguousarray(u, dtype=np.float64))
        if code != 0:
            raise self._err(code, "solver_hipmf_mat_vec_mul")
        return v

    def permutation(self):
        p = np.zeros(self.n, np.int32)
        code = self.lib.solver_hipmf_get_permutation(self.h, p)
        if code != 0:
            raise self._err(code, "solver_hipmf_get_permutation")
        return p

    def stats(self):
        i, d = np.zeros(16, np.int64), np.zeros(16)
        code = self.lib.solver_hipmf_get_stats(self.h, i, d)
        if code != 0:
            raise self._err(code, "solver_hipmf_get_stats")
        out = {k: int(v) for k, v in zip(ISTAT_NAMES, i)}
        out.update({k: float(v) for k, v in zip(DSTAT_NAMES, d)})
        return out

    COUNTERS = {"rematch": 0, "weak_diagonal_rows": 1, "fused_fallbacks": 2, "persistent_bytes": 3, "arena_bytes": 4, "symmetric_ldlt": 5, "sym_expanded": 6, "chain_fallbacks": 7, "mid_fronts": 8, "plan_digest": 9, "tagged_solve": 10, "gate_waits": 11, "wave_fronts": 12, "leaf_fronts": 13, "split_slabs": 14, "event_fence_free": 15, "block_groups": 16, "sym_weak_diagonal": 17, "bcast_sliced_bytes": 18, "krylov_iterations": 19, "transposed_solves": 20, "analysis_solves": 21, "transposed_krylov_iterations": 22, "transposed_blocks": 23, "pruned_fwd_fronts": 24, "pruned_bwd_fronts": 25, "pruned_blocks": 26, "pruned_bytes": 27, "updated_steps": 28, "updated_cycles": 29, "updated_basis_bytes": 30, "updated_precond_us": 31, "updated_spmv_us": 32, "updated_arnoldi_us": 33, "updated_blocks": 34, "updated_column_steps": 35, "updated_block_basis_bytes": 36, "pruned_transposed_blocks": 38, "extra_precise_steps": 39, "extra_precise_blocks": 40, "extra_precise_residual_us": 41, "extra_precise_precond_us": 42, "extra_precise_update_us": 43, "border_columns": 44, "bordered_steps": 45, "bordered_blocks": 46, "sens_outer_columns": 47, "sens_outer_us": 48, "bordered_transposed_steps": 49, "bordered_transposed_blocks": 50, "border_transposed_bytes": 51, "complex_border_columns": 52, "complex_bordered_steps": 53, "complex_bordered_blocks": 54, "complex_bordered_transposed_steps": 55, "complex_bordered_transposed_blocks": 56, "complex_border_transposed_bytes": 57, "eigs_steps": 58, "eigs_restarts": 59, "eigs_converged": 60, "eigs_basis_bytes": 61, "eigs_solve_us": 62, "eigs_spmv_us": 63, "eigs_orth_us": 64, "eigs_rotate_us": 65}

    WARNING_NOT_CONVERGED = 2

    OPTIONS = {"matching": 0, "pivoting": 1, "hybrid_memory": 2, "error_estimates": 3, "condition_numbers": 4, "sym_recheck": 5}

    def set_option(self, name, value):
        """solver_hipmf_set_option (before initialize): the LinSolParams fields the initialize signature does not carry."""
        return int(self.lib.solver_hipmf_set_option(self.h, self.OPTIONS[name], float(value)))

    def counter(self, name):
        return int(self.lib.solver_hipmf_get_counter(self.h, self.COUNTERS[name]))

    def reset_timers(self):
        self.lib.solver_hipmf_reset_timers(self.h)

    # ---- device-resident operands (bench / multi-GPU) -------------------------------------------
    def dev_alloc(self, nbytes):
        p = self.lib.hipmf_device_malloc(nbytes)
        if not p:
            raise MemoryError("hipmf_device_malloc(%d)" % nbytes)
        return p

    def dev_free(self, p):
        self.lib.hipmf_device_free(p)

    def h2d(self, dptr, arr):
        a = np.ascontiguousarray(arr)
        code = self.lib.hipmf_memcpy_h2d(dptr, a.ctypes.data_as(C.c_void_p), a.nbytes)
        if code != 0:
            raise self._err(code, "hipmf_memcpy_h2d")

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        code = self.lib.hipmf_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), dptr, arr.nbytes)
        if code != 0:
            raise self._err(code, "hipmf_memcpy_d2h")

    def factorize_device(self, d_values):
        return self.lib.solver_hipmf_factorize_device(self.h, d_values)

    def factorize_mapped_device(self, d_input_values):
        """Numeric factorisation from a DEVICE array of input values (e.g. COO triplets) through the installed value map."""
        return self.lib.solver_hipmf_factorize_mapped_device(self.h, d_input_values)

    def factor_buffers(self):
        """(pointer, bytes) of the device buffers that hold the numeric factor: persistent part of the front pool, local row
        interchanges, scaling, pivots.  A peer that ran `initialize` on the same structure can be handed their contents and then
        `adopt_factor`."""
        ptrs = (C.c_void_p * 4)()
        sizes = (C.c_int64 * 4)()
        k = self.lib.solver_hipmf_factor_parts(self.h, 4, ptrs, sizes)
        if k != 4:
            raise self._err(k, "solver_hipmf_factor_parts")
        return [(int(ptrs[i] or 0), int(sizes[i])) for i in range(4)]

    def broadcast_factor(self, comm, root, rank):
        """RCCL broadcast of the factor (and the matrix values) from `root`; returns (seconds, bytes)."""
        sec, nb = C.c_double(0.0), C.c_int64(0)
        code = self.lib.solver_hipmf_broadcast_factor(self.h, comm, root, rank, C.byref(sec), C.byref(nb))
        if code != 0:
            raise self._err(code, "solver_hipmf_broadcast_factor")
        return sec.value, nb.value

    def solve_many_sharded(self, d_x, d_rhs, nrhs_total, nranks, rank, ld=None):
        first, count = C.c_int32(0), C.c_int32(0)
        code = self.lib.solver_hipmf_solve_many_sharded(self.h, d_x, d_rhs, nrhs_total, ld or self.n, nranks, rank, C.byref(first), C.byref(count))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_many_sharded")
        return first.value, count.value

    def adopt_factor(self, d_values):
        """Declare the factor buffers (filled by a peer) valid; d_values: the matrix values on the device (refinement SpMV)."""
        return self.lib.solver_hipmf_adopt_factor(self.h, d_values)

    def prepare_solve_many(self, nrhs):
        """Allocate and touch the block buffers of a later many-RHS solve ahead of time (any time after initialize)."""
        code = self.lib.solver_hipmf_prepare_solve_many(self.h, int(nrhs))
        if code != 0:
            raise self._err(code, "solver_hipmf_prepare_solve_many")

    def solve_device(self, d_x, d_rhs, nrhs=1, ld=None):
        code = self.lib.solver_hipmf_solve_device(self.h, d_x, d_rhs, nrhs, ld or self.n)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_device")

    def solve_transpose_device(self, d_x, d_rhs, nrhs=1, ld=None):
        code = self.lib.solver_hipmf_solve_transpose_device(self.h, d_x, d_rhs, nrhs, ld or self.n)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_transpose_device")

    def solve_transpose_many_device(self, d_x, d_rhs, nrhs, ld=None):
        """device-resident columns of A^T X = B, 16 per pass pair over the factor (solve_transpose_device: one at a time)"""
        code = self.lib.solver_hipmf_solve_transpose_many_device(self.h, d_x, d_rhs, nrhs, ld or self.n)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_transpose_many_device")

    def solve_sparse_device(self, d_x_sel, ldx, nrhs, d_rhs_ptr, d_rhs_idx, d_rhs_val, nsel, d_sel_idx=None, transpose=False):
        """solve_sparse with every array resident on the device (d_sel_idx None: all n rows)"""
        name = "solver_hipmf_solve_sparse_transpose_device" if transpose else "solver_hipmf_solve_sparse_device"
        code = getattr(self.lib, name)(self.h, d_x_sel, int(ldx), int(nrhs), d_rhs_ptr, d_rhs_idx, d_rhs_val, int(nsel), d_sel_idx, 0)
        if code != 0:
            raise self._err(code, name)

    def solve_updated_device(self, d_x, d_rhs, d_values, mapped=False, rel_tol=0.0, max_steps=0, transpose=False):
        """solve_updated with x, rhs and values resident on the device; returns (steps, relres, status)"""
        name = "solver_hipmf_solve_updated_transpose_device" if transpose else "solver_hipmf_solve_updated_device"
        steps, relres = C.c_int32(0), C.c_double(0.0)
        code = getattr(self.lib, name)(self.h, d_x, d_rhs, d_values, int(bool(mapped)), float(rel_tol), int(max_steps), C.byref(steps), C.byref(relres))
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, name)
        return int(steps.value), float(relres.value), code

    def solve_extra_precise_device(self, d_x, d_x_tail, d_rhs, nrhs=1, dx_tol=0.0, max_steps=0, ld=None):
        """solve_extra_precise_many with x, x_tail (None: no tail) and rhs (column-major ld x nrhs) resident on the device; returns (info, status)"""
        nrhs = int(nrhs)
        info = np.zeros((max(nrhs, 1), 8))
        code = self.lib.solver_hipmf_solve_extra_precise_device(self.h, d_x, d_x_tail, d_rhs, nrhs, int(ld or self.n), float(dx_tol), int(max_steps),
                                                                info.ctypes.data)
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, "solver_hipmf_solve_extra_precise_device")
        return info[:nrhs], code

    def set_border_device(self, k, d_B, d_C, d_D, ldb=None, ldc=None, ldd=None):
        """set_border with B, C (column-major ld x k) and D (ldd x k) resident on the device; returns (border_info, status)"""
        info = np.zeros(4)
        code = self.lib.solver_hipmf_set_border_device(self.h, int(k), d_B, int(ldb or self.n), d_C, int(ldc or self.n), d_D, int(ldd or k), info.ctypes.data, 0)
        if code not in (0, self.WARNING_SINGULAR_MATRIX):
            raise self._err(code, "solver_hipmf_set_border_device")
        return info, code

    def solve_bordered_device(self, d_x, d_z, d_f, d_g, nrhs=1, max_steps=0, ldx=None, ldz=None):
        """solve_bordered with x, f (column-major ldx x nrhs) and z, g (ldz x nrhs; None allowed) resident on the device; returns info"""
        nrhs = int(nrhs)
        info = np.zeros((max(nrhs, 1), 4))
        code = self.lib.solver_hipmf_solve_bordered_device(self.h, d_x, d_z, d_f, d_g, nrhs, int(ldx or self.n), int(ldz or max(self.counter("border_columns"), 1)),
                                                           int(max_steps), info.ctypes.data, 0)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_bordered_device")
        return info[:nrhs]

    def solve_bordered_transpose_device(self, d_y, d_w, d_p, d_q, nrhs=1, max_steps=0, ldx=None, ldz=None):
        """solve_bordered_transpose with y, p (column-major ldx x nrhs) and w, q (ldz x nrhs; None allowed) resident on the device; returns info"""
        nrhs = int(nrhs)
        info = np.zeros((max(nrhs, 1), 4))
        code = self.lib.solver_hipmf_solve_bordered_transpose_device(self.h, d_y, d_w, d_p, d_q, nrhs, int(ldx or self.n),
                                                                     int(ldz or max(self.counter("border_columns"), 1)), int(max_steps), info.ctypes.data, 0)
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_bordered_transpose_device")
        return info[:nrhs]

    def values_outer_device(self, d_grad, d_u, d_w, ncols=1, alpha=1.0, beta=0.0, mapped=False, ldu=None, ldw=None):
        """values_outer with grad, u and w (column-major ldu x ncols, ldw x ncols) resident on the device"""
        code = self.lib.solver_hipmf_values_outer_device(self.h, d_grad, d_u, d_w, int(ncols), int(ldu or self.n), int(ldw or self.n), float(alpha), float(beta),
                                                         int(bool(mapped)))
        if code != 0:
            raise self._err(code, "solver_hipmf_values_outer_device")

    def solve_tangent_device(self, d_dx, d_x, d_dvalues, d_db=None, nrhs=1, mapped=False, ld=None):
        """solve_tangent with dx, x, db (column-major ld x nrhs; db None: zero) and dvalues resident on the device"""
        code = self.lib.solver_hipmf_solve_tangent_device(self.h, d_dx, d_x, d_dvalues, d_db, int(nrhs), int(ld or self.n), int(bool(mapped)))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_tangent_device")

    def solve_adjoint_device(self, d_lambda, d_grad, d_x, d_g, nrhs=1, beta=0.0, mapped=False, ld=None):
        """solve_adjoint with lambda, x, g (column-major ld x nrhs) and grad (None: the solve alone) resident on the device"""
        code = self.lib.solver_hipmf_solve_adjoint_device(self.h, d_lambda, d_grad, d_x, d_g, int(nrhs), int(ld or self.n), float(beta), int(bool(mapped)))
        if code != 0:
            raise self._err(code, "solver_hipmf_solve_adjoint_device")

    def solve_updated_many_device(self, d_x, d_rhs, nrhs, d_values, mapped=False, rel_tol=0.0, max_steps=0, ld=None, transpose=False):
        """solve_updated_many with x, rhs (column-major ld x nrhs) and values resident on the device; returns (steps, relres, status)"""
        name = "solver_hipmf_solve_updated_transpose_many_device" if transpose else "solver_hipmf_solve_updated_many_device"
        nrhs = int(nrhs)
        steps, relres = np.zeros(max(nrhs, 1), np.int32), np.zeros(max(nrhs, 1))
        code = getattr(self.lib, name)(self.h, d_x, d_rhs, nrhs, int(ld or self.n), d_values, int(bool(mapped)), float(rel_tol),
                                       int(max_steps), steps.ctypes.data, relres.ctypes.data)
        if code not in (0, self.WARNING_NOT_CONVERGED):
            raise self._err(code, name)
        return steps[:nrhs], relres[:nrhs], code


class ComplexHipmf:
    """The complex twin's handle (complex_solver_hipmf_*): life cycle, solve and the sensitivity calls.  Complex vectors and value arrays
    go in and out as NumPy complex128 arrays; the library sees them as interleaved (re, im) pairs."""

    def __init__(self, lib_path=None):
        self.lib = _capi.load(lib_path)
        self.h = self.lib.complex_solver_hipmf_new()
        if not self.h:
            raise RuntimeError("complex_solver_hipmf_new returned NULL: no HIP device visible (there is no CPU fallback)")
        self.n = self.nnz = self.nnz_in = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.complex_solver_hipmf_drop(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _err(self, code, where):
        return HipmfError(code, where, (self.lib.complex_solver_hipmf_last_error(self.h) or b"").decode())

    @staticmethod
    def _z(a):
        return np.ascontiguousarray(a, dtype=np.complex128)

    def initialize(self, n, row_pointers, col_indices, ordering=0, scaling=1, pivot_epsilon=-1.0, refinement_nstep=-1, verbose=False, general_symmetric=False,
                   values=None):
        rp = np.ascontiguousarray(row_pointers, dtype=np.int32)
        ci = np.ascontiguousarray(col_indices, dtype=np.int32)
        self.n, self.nnz = int(n), int(rp[n])
        self._init_values = None if values is None else self._z(values)
        return self.lib.complex_solver_hipmf_initialize(self.h, ordering, scaling, pivot_epsilon, refinement_nstep, int(verbose), int(general_symmetric), n, rp, ci,
                                                        None if values is None else self._init_values.ctypes.data)

    def factorize(self, values, verbose=False):
        """numeric factorisation from the nnz stored complex entries (drops a triplet map: the identity map is back in force)"""
        npv = C.c_int32()
        code = self.lib.complex_solver_hipmf_factorize(self.h, None, None, C.byref(npv), None, None, None, None, 0, int(verbose), self._z(values).view(np.float64))
        self.num_perturbed, self.nnz_in = npv.value, 0
        return code

    def set_value_map(self, seg_ptr, seg_idx):
        sp = np.ascontiguousarray(seg_ptr, dtype=np.int32)
        si = np.ascontiguousarray(seg_idx, dtype=np.int32)
        code = self.lib.complex_solver_hipmf_set_value_map(self.h, int(si.size), sp, si)
        if code == 0:
            self.nnz_in = int(si.size)
        return code

    def factorize_mapped(self, input_values, verbose=False):
        return self.lib.complex_solver_hipmf_factorize_mapped(self.h, None, None, None, None, int(verbose), self._z(input_values).view(np.float64))

    def solve(self, rhs, verbose=False):
        x = np.zeros(self.n, np.complex128)
        code = self.lib.complex_solver_hipmf_solve(self.h, x.view(np.float64), self._z(rhs).view(np.float64), int(verbose))
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_solve")
        return x

    def solve_transpose(self, rhs, conjugate=True, verbose=False):
        """x = A^{-H} rhs (conjugate) or A^{-T} rhs with the factor of A"""
        x = np.zeros(self.n, np.complex128)
        code = self.lib.complex_solver_hipmf_solve_transpose(self.h, x.view(np.float64), self._z(rhs).view(np.float64), int(bool(conjugate)), int(verbose))
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_solve_transpose")
        return x

    def determinant(self):
        """(real, imaginary, exponent): det A = (real + i imaginary) x 10^exponent, of the last factorisation"""
        g = (C.c_double(), C.c_double(), C.c_double())
        code = self.lib.complex_solver_hipmf_get_determinant(self.h, C.byref(g[0]), C.byref(g[1]), C.byref(g[2]))
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_get_determinant")
        return tuple(q.value for q in g)

    def counter(self, name):
        return int(self.lib.complex_solver_hipmf_get_counter(self.h, Hipmf.COUNTERS[name]))

    def _columns(self, a, what):
        a = self._z(a)
        single = a.ndim == 1
        a = a.reshape(1, -1) if single else a
        if a.ndim != 2 or a.shape[1] < self.n:
            raise ValueError("%s expects a vector of %d entries or an array of shape (ncols, ld >= %d), got %r" % (what, self.n, self.n, a.shape))
        return a, single

    def _value_count(self, mapped):
        return int(self.nnz_in) if mapped else int(self.nnz)

    def values_outer(self, u, w, alpha=1.0, beta=0.0, grad=None, mapped=False, conjugate_w=False):
        """grad = beta grad + alpha sum_c u_c op(w_c)^T restricted to the pattern, op = conj with conjugate_w, in the order of the complex
        values the handle is fed (mapped: the triplets of the value map); complex_solver_hipmf_values_outer."""
        ua, _ = self._columns(u, "values_outer")
        wa, _ = self._columns(w, "values_outer")
        if ua.shape[0] != wa.shape[0]:
            raise ValueError("values_outer: u has %d columns, w %d" % (ua.shape[0], wa.shape[0]))
        g = np.zeros(self._value_count(mapped), np.complex128) if grad is None else grad
        code = self.lib.complex_solver_hipmf_values_outer(self.h, g.ctypes.data, ua.ctypes.data, wa.ctypes.data, ua.shape[0], ua.shape[1], wa.shape[1], float(alpha),
                                                          float(beta), int(bool(mapped)), int(bool(conjugate_w)))
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_values_outer")
        return g

    def solve_tangent(self, x, dvalues, db=None, mapped=False, dx=None):
        """dx = A^{-1} (db - dA x) for the complex matrix dA that dvalues describe (complex_solver_hipmf_solve_tangent)"""
        xa, single = self._columns(x, "solve_tangent")
        ba = None if db is None else self._columns(db, "solve_tangent")[0]
        if ba is not None and ba.shape != xa.shape:
            raise ValueError("solve_tangent: x has shape %r, db %r" % (xa.shape, ba.shape))
        out = np.zeros_like(xa) if dx is None else dx
        code = self.lib.complex_solver_hipmf_solve_tangent(self.h, out.ctypes.data, xa.ctypes.data, self._z(dvalues).ctypes.data, None if ba is None else ba.ctypes.data,
                                                           xa.shape[0], xa.shape[1], int(bool(mapped)))
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_solve_tangent")
        return out.reshape(xa.shape)[0] if single and dx is None else out

    def solve_adjoint(self, g, x=None, beta=0.0, grad=None, mapped=False, want_grad=True, lam=None):
        """lambda = A^{-H} g and grad_k = beta grad_k - sum_c lambda_i conj(x_j) for a real-valued J with g = dJ/dRe x + i dJ/dIm x
        (complex_solver_hipmf_solve_adjoint): dJ = Re <grad, dA> + Re <lambda, db>.  Returns (lambda, grad or None)."""
        ga, single = self._columns(g, "solve_adjoint")
        xa = None if x is None else self._columns(x, "solve_adjoint")[0]
        if want_grad and (xa is None or xa.shape != ga.shape):
            raise ValueError("solve_adjoint: the gradient needs x in the shape of g")
        out = np.zeros_like(ga) if lam is None else lam
        gr = None if not want_grad else (np.zeros(self._value_count(mapped), np.complex128) if grad is None else grad)
        code = self.lib.complex_solver_hipmf_solve_adjoint(self.h, out.ctypes.data, None if gr is None else gr.ctypes.data, None if xa is None else xa.ctypes.data,
                                                           ga.ctypes.data, ga.shape[0], ga.shape[1], float(beta), int(bool(mapped)))
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_solve_adjoint")
        return (out.reshape(ga.shape)[0] if single and lam is None else out), gr

    # ---- bordered systems on the kept factor (complex_solver_hipmf_set_border / _solve_bordered / _solve_bordered_transpose) ----
    WARNING_SINGULAR_MATRIX = 1

    def set_border(self, B, C_, D, verbose=False):
        """The border of [A B; C^T D] on the kept factor, C^T the plain transpose: B, C_ complex of shape (n, k), D of shape (k, k); k = 0
        (or B None) drops it.  Returns (border_info, status): min / max |u_ii| of the complex LU of S = D - C^T A^{-1} B, real and
        imaginary mantissa and base-10 exponent of det S, device bytes held; status 0 or WARNING_SINGULAR_MATRIX; others raise."""
        info = np.zeros(5)
        if B is None or np.asarray(B).size == 0:
            code = self.lib.complex_solver_hipmf_set_border(self.h, 0, None, 0, None, 0, None, 0, info.ctypes.data, int(verbose))
        else:
            Bf, Cf, Df = (np.asfortranarray(np.asarray(a, dtype=np.complex128).reshape(np.shape(a)[0], -1)) for a in (B, C_, D))
            k = Bf.shape[1]
            if Bf.shape != (self.n, k) or Cf.shape != (self.n, k) or Df.shape != (k, k):
                raise ValueError("set_border expects B, C of shape (%d, k) and D of shape (k, k), got %r, %r, %r" % (self.n, Bf.shape, Cf.shape, Df.shape))
            code = self.lib.complex_solver_hipmf_set_border(self.h, k, Bf.ctypes.data, self.n, Cf.ctypes.data, self.n, Df.ctypes.data, k, info.ctypes.data, int(verbose))
        if code not in (0, self.WARNING_SINGULAR_MATRIX):
            raise self._err(code, "complex_solver_hipmf_set_border")
        return info, code

    def solve_bordered(self, f, g=None, want_z=True, max_steps=0, ldx=None, ldz=None, verbose=False, x=None, z=None):
        """[A B; C^T D] [x; z] = [f; g] with the border of set_border, refined on the whole system.  f: complex (n,) or (nrhs, ldx); g:
        (k,) or (nrhs, ldz), None: g = 0; want_z False: z is not returned.  x / z: complex arrays of those shapes to write into (their
        padding is left alone).  Returns (x, z or None, info of shape (nrhs, 4))."""
        return self._solve_bordered("complex_solver_hipmf_solve_bordered", None, f, g, want_z, max_steps, ldx, ldz, verbose, x, z)

    def solve_bordered_transpose(self, p, q=None, conjugate=True, want_w=True, max_steps=0, ldx=None, ldz=None, verbose=False, y=None, w=None):
        """M^H [y; w] = [p; q] (conjugate) or M^T [y; w] = [p; q] with M = [A B; C^T D] of set_border.  Arguments and results as
        solve_bordered: returns (y, w or None, info)."""
        return self._solve_bordered("complex_solver_hipmf_solve_bordered_transpose", int(bool(conjugate)), p, q, want_w, max_steps, ldx, ldz, verbose, y, w)

    def _solve_bordered(self, entry, conjugate, f, g, want_z, max_steps, ldx, ldz, verbose, x, z):
        k = self.counter("complex_border_columns")
        fa = self._z(f)
        single = fa.ndim == 1
        fa = fa.reshape(1, -1) if single else fa
        nrhs = fa.shape[0]
        ldx = fa.shape[1] if ldx is None else int(ldx)
        ga = None if g is None else self._z(g).reshape(nrhs, -1)
        ldz = (k if ga is None else ga.shape[1]) if ldz is None else int(ldz)
        x = np.zeros((nrhs, ldx), np.complex128) if x is None else x
        z = (np.zeros((nrhs, max(ldz, 1)), np.complex128) if z is None else z) if want_z else None
        info = np.zeros((nrhs, 4))
        head = (self.h, x.ctypes.data, None if z is None else z.ctypes.data, fa.ctypes.data, None if ga is None else ga.ctypes.data, nrhs, ldx, ldz)
        tail = (int(max_steps), info.ctypes.data, int(verbose))
        code = getattr(self.lib, entry)(*(head + (() if conjugate is None else (conjugate,)) + tail))
        if code != 0:
            raise self._err(code, entry)
        if single:
            return x[0], (None if z is None else z[0]), info[0]
        return x, z, info

    # device-resident operands: interleaved complex arrays, 16 bytes per entry
    def dev_alloc(self, nbytes):
        p = self.lib.hipmf_device_malloc(nbytes)
        if not p:
            raise MemoryError("hipmf_device_malloc(%d)" % nbytes)
        return p

    def dev_free(self, p):
        self.lib.hipmf_device_free(p)

    def h2d(self, dptr, arr):
        a = np.ascontiguousarray(arr)
        code = self.lib.hipmf_memcpy_h2d(dptr, a.ctypes.data_as(C.c_void_p), a.nbytes)
        if code != 0:
            raise self._err(code, "hipmf_memcpy_h2d")

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        code = self.lib.hipmf_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), dptr, arr.nbytes)
        if code != 0:
            raise self._err(code, "hipmf_memcpy_d2h")

    def set_border_device(self, k, d_B, d_C, d_D, ldb=None, ldc=None, ldd=None):
        """set_border with B, C (column-major ld x k complex) and D (ldd x k) resident on the device; returns (border_info, status)"""
        info = np.zeros(5)
        code = self.lib.complex_solver_hipmf_set_border_device(self.h, int(k), d_B, int(ldb or self.n), d_C, int(ldc or self.n), d_D, int(ldd or k), info.ctypes.data, 0)
        if code not in (0, self.WARNING_SINGULAR_MATRIX):
            raise self._err(code, "complex_solver_hipmf_set_border_device")
        return info, code

    def solve_bordered_device(self, d_x, d_z, d_f, d_g, nrhs=1, max_steps=0, ldx=None, ldz=None):
        """solve_bordered with x, f (column-major ldx x nrhs complex) and z, g (ldz x nrhs; None allowed) resident on the device; returns info"""
        nrhs = int(nrhs)
        info = np.zeros((max(nrhs, 1), 4))
        code = self.lib.complex_solver_hipmf_solve_bordered_device(self.h, d_x, d_z, d_f, d_g, nrhs, int(ldx or self.n),
                                                                   int(ldz or max(self.counter("complex_border_columns"), 1)), int(max_steps), info.ctypes.data, 0)
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_solve_bordered_device")
        return info[:nrhs]

    def solve_bordered_transpose_device(self, d_y, d_w, d_p, d_q, nrhs=1, conjugate=True, max_steps=0, ldx=None, ldz=None):
        """solve_bordered_transpose with y, p (column-major ldx x nrhs complex) and w, q (ldz x nrhs; None allowed) resident on the device; returns info"""
        nrhs = int(nrhs)
        info = np.zeros((max(nrhs, 1), 4))
        code = self.lib.complex_solver_hipmf_solve_bordered_transpose_device(self.h, d_y, d_w, d_p, d_q, nrhs, int(ldx or self.n),
                                                                             int(ldz or max(self.counter("complex_border_columns"), 1)), int(bool(conjugate)),
                                                                             int(max_steps), info.ctypes.data, 0)
        if code != 0:
            raise self._err(code, "complex_solver_hipmf_solve_bordered_transpose_device")
        return info[:nrhs]
