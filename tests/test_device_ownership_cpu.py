"""Every handle gives back what it took: live device allocations, pinned allocations, streams and events (counted by the CPU
emulator, tools/hipemu) return to their value from before the handle was made once it is closed -- after the paths that allocate lazily
(block buffers of the many-RHS solves, transposed solves, error analysis), re-analysis, value maps, a refused initialize, and the FDM
device handle.  The reference checks its C shims the same way under valgrind."""
import ctypes as C
import gc

import numpy as np
import scipy.sparse as sp

from russell_amd import problems as P
from russell_amd.backend import Hipmf
from russell_amd.pde import FdmDevice
from test_complex_error_analysis_cpu import ZHandle, shifted_convection_diffusion
from test_gpu_parity import _random_unsymmetric
from test_sym_indefinite_cpu import saddle_point


def _live(lib_path):
    f = C.CDLL(lib_path).hipemu_live_objects
    f.argtypes, f.restype = [C.c_void_p], None
    out = (C.c_longlong * 4)()

    def counts():
        f(out)
        return tuple(out)  # device allocations, pinned allocations, streams, events

    return counts


def _baseline(live):
    gc.collect()
    return live()


def _exercise(s, A, rng, transposed=True):
    n = A.shape[0]
    xs = rng.standard_normal(n)
    b = A @ xs
    assert np.max(np.abs(s.solve(b) - xs)) < 1e-8
    for nrhs in (2, 18, 40):  # (18: wider blocks than the 2-column call's: the block buffers are allocated again)
        XS = rng.standard_normal((nrhs, n))
        assert np.max(np.abs(s.solve_many(np.array([A @ XS[j] for j in range(nrhs)])) - XS)) < 1e-8
    if transposed:
        assert np.max(np.abs(s.solve_transpose(A.T @ xs) - xs)) < 1e-8
    for option in (1, 2):
        x, _ = s.solve_with_error_analysis(b, option)
        assert np.max(np.abs(x - xs)) < 1e-8


def test_lu_and_ldlt_handles_give_back_everything(emu_lib):
    live = _live(emu_lib)
    rng = np.random.default_rng(3)
    n, rp, ci, v = P.convection_diffusion2d(16, peclet=30.0, scale_decades=0.0)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    base = _baseline(live)
    s = Hipmf(emu_lib)
    assert s.initialize(n, rp, ci) == 0 and s.factorize(v) == 0
    assert live() != base
    _exercise(s, A, rng)
    s.close()
    assert live() == base
    # symmetric-lower storage, L D L^T fronts
    n, rp, ci, v = P.poisson2d(16, 14)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    lrp, lci, lv = P.lower_triangle(n, rp, ci, v)
    base = _baseline(live)
    s = Hipmf(emu_lib)
    assert s.initialize(n, lrp, lci, general_symmetric=True) == 0 and s.factorize(lv) == 0
    assert s.counter("symmetric_ldlt") == 1
    _exercise(s, A, rng)
    s.close()
    assert live() == base


def test_expanded_lower_triangle_with_value_maps_gives_back_everything(emu_lib):
    live = _live(emu_lib)
    A, L = saddle_point(8, 12)
    n = A.shape[0]
    rp, ci, v = L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)
    nnz = v.size
    base = _baseline(live)
    s = Hipmf(emu_lib)
    assert s.initialize(n, rp, ci, general_symmetric=True, values=v) == 0
    assert s.counter("sym_expanded") == 1
    for _ in range(2):  # (the second map replaces the first one's buffers)
        assert s.set_value_map(np.arange(nnz + 1), np.arange(nnz)) == 0
        assert s.factorize_mapped(v) == 0
    _exercise(s, A, np.random.default_rng(5), transposed=False)
    s.close()
    assert live() == base


def test_complex_twin_gives_back_everything(emu_lib):
    live = _live(emu_lib)
    A = shifted_convection_diffusion(12)
    rng = np.random.default_rng(7)
    b = A @ (rng.standard_normal(A.shape[0]) + 1j * rng.standard_normal(A.shape[0]))
    base = _baseline(live)
    z = ZHandle(emu_lib, A)
    z.solve(b)
    for option in (1, 2):
        z.solve_ea(b, option)
    z.close()
    assert live() == base


def test_rematching_factorize_gives_back_everything(emu_lib):
    live = _live(emu_lib)
    n = 400
    M, rng = _random_unsymmetric(n, 1e-3, 3)
    xs = rng.standard_normal(n)
    base = _baseline(live)
    s = Hipmf(emu_lib)
    assert s.initialize(n, M.indptr.astype(np.int32), M.indices.astype(np.int32)) == 0
    assert s.factorize(M.data) == 0 and s.counter("rematch") == 1
    assert np.max(np.abs(s.solve(M @ xs) - xs)) < 1e-6 * max(1.0, np.max(np.abs(xs)))
    s.close()
    assert live() == base


def test_refused_initialize_gives_back_everything_at_once(emu_lib, monkeypatch):
    live = _live(emu_lib)
    n, rp, ci, v = P.poisson2d(120, 110)
    monkeypatch.setenv("HIPMF_POOL_LIMIT_GB", "0.001")
    base = _baseline(live)
    s = Hipmf(emu_lib)
    assert s.initialize(n, rp, ci) != 0
    assert live() == base  # before close(): the refusal itself let go of the streams, events and structure arrays
    s.close()
    assert live() == base


def test_fdm_device_handle_gives_back_everything(emu_lib):
    live = _live(emu_lib)
    for lmm in (False, True):
        base = _baseline(live)
        mask = np.zeros(6 * 5, np.uint8)
        mask[:6] = 1
        g = FdmDevice(6, 5, prescribed=mask, lib_path=emu_lib)
        g.structure_device()
        if lmm:
            g.lmm_dims()
            g.lmm_structure_device()
        g.close()
        assert live() == base
