// krylov_host.hpp -- the host side of every flexible GMRES of numeric.cpp (Krylov rescue, solve_updated, solve_updated_many, the
// complex solve_updated): the least-squares problem min |g - H y| of a cycle, kept triangular by Givens rotations.  No HIP in here.
#pragma once
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

namespace hipmf {

// T = double or std::complex<double>.  H is (m + 1) x m with row stride m; rotation j is [c s; -conj(s) c] with real c.
template <class T>
struct GivensLsq {
    int32_t m;
    std::vector<T> H, sn, g;
    std::vector<double> cs;

    explicit GivensLsq(int32_t m_) : m(m_), H((size_t)(m_ + 1) * m_), sn((size_t)m_), g((size_t)m_ + 1), cs((size_t)m_) {}

    void reset(double rnorm) { // a new cycle: g = |r| e_0
        for (T &e : g) e = T(0.0);
        g[0] = rnorm;
    }
    // Column k of the Hessenberg matrix: hcol[0 .. k] and the subdiagonal entry hn >= 0.  Applies the rotations 0 .. k - 1, makes
    // rotation k and updates g: |g[k + 1]| is the residual estimate after k + 1 directions.
    void push(int32_t k, const T *hcol, double hn) {
        for (int32_t j = 0; j <= k; j++) H[(size_t)j * m + k] = hcol[j];
        H[(size_t)(k + 1) * m + k] = hn;
        for (int32_t j = 0; j < k; j++) {
            const T a = H[(size_t)j * m + k], b = H[(size_t)(j + 1) * m + k];
            H[(size_t)j * m + k] = cs[(size_t)j] * a + sn[(size_t)j] * b;
            H[(size_t)(j + 1) * m + k] = -conj_of(sn[(size_t)j]) * a + cs[(size_t)j] * b;
        }
        rotation(H[(size_t)k * m + k], hn, cs[(size_t)k], sn[(size_t)k]);
        H[(size_t)(k + 1) * m + k] = 0.0;
        g[(size_t)k + 1] = -conj_of(sn[(size_t)k]) * g[(size_t)k];
        g[(size_t)k] = cs[(size_t)k] * g[(size_t)k];
    }
    // y[0 .. k) of the triangular system over the first k directions (a zero pivot gives 0)
    void solve(int32_t k, T *y) const {
        for (int32_t i = k - 1; i >= 0; i--) {
            T t = g[(size_t)i];
            for (int32_t j = i + 1; j < k; j++) t -= H[(size_t)i * m + j] * y[j];
            y[i] = H[(size_t)i * m + i] != T(0.0) ? t / H[(size_t)i * m + i] : T(0.0);
        }
    }

  private:
    static double conj_of(double s) { return s; }
    static std::complex<double> conj_of(const std::complex<double> &s) { return std::conj(s); }
    // The rotation that takes (a, hn) to (diag, 0); diag replaces a.  Two overloads on purpose: the complex formula at a real a
    // differs from the real one in signs and rounding.
    static void rotation(double &a, double hn, double &c, double &s) {
        const double d = std::hypot(a, hn);
        c = d > 0.0 ? a / d : 1.0, s = d > 0.0 ? hn / d : 0.0;
        a = d;
    }
    // hn real and not negative: (a, hn) -> (a / |a| d, 0) with c = |a| / d, s = (a / |a|) hn / d
    static void rotation(std::complex<double> &a, double hn, double &c, std::complex<double> &s) {
        const double aa = std::abs(a), d = std::hypot(aa, hn);
        const std::complex<double> phase = aa > 0.0 ? a / aa : std::complex<double>(1.0, 0.0);
        c = d > 0.0 ? aa / d : 1.0, s = d > 0.0 ? phase * (hn / d) : std::complex<double>(0.0, 0.0);
        a = phase * d;
    }
};

// Eigenvalues w and orthonormal eigenvectors Z (row-major n x n, Z[r n + c] = component r of eigenvector c) of the symmetric matrix A
// (row-major, leading dimension lda; only read) by the cyclic Jacobi method -- the projected matrix of the thick-restart Lanczos
// (Solver::eigs_near_shift), n <= 128.  The textbook scheme: sweeps over the upper triangle by rows, the rotation that annihilates
// a_pq from t = sign(tau) / (|tau| + sqrt(1 + tau^2)), tau = (a_qq - a_pp) / (2 a_pq); after three sweeps an entry that no longer
// changes either diagonal neighbour in working precision is set to zero.  Small eigenvector components come out with small absolute
// errors relative to their own size, which the Lanczos stop test (the LAST row of Z) relies on.  Deterministic: no data-dependent order.
inline void jacobi_eigh(int32_t n, const double *A, int32_t lda, std::vector<double> &w, std::vector<double> &Z) {
    std::vector<double> a((size_t)n * n);
    for (int32_t i = 0; i < n; i++)
        for (int32_t j = 0; j < n; j++) a[(size_t)i * n + j] = i <= j ? A[(size_t)i * lda + j] : A[(size_t)j * lda + i];
    Z.assign((size_t)n * n, 0.0);
    for (int32_t i = 0; i < n; i++) Z[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 100; sweep++) {
        double off = 0.0;
        for (int32_t p = 0; p < n; p++)
            for (int32_t q = p + 1; q < n; q++) off += std::fabs(a[(size_t)p * n + q]);
        if (off == 0.0) break;
        for (int32_t p = 0; p < n - 1; p++)
            for (int32_t q = p + 1; q < n; q++) {
                const double apq = a[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q], g = 100.0 * std::fabs(apq);
                if (sweep > 2 && std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
                    continue;
                }
                const double tau = (aqq - app) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                a[(size_t)p * n + p] = app - t * apq, a[(size_t)q * n + q] = aqq + t * apq;
                a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
                for (int32_t r = 0; r < n; r++) {
                    if (r != p && r != q) {
                        const double arp = a[(size_t)r * n + p], arq = a[(size_t)r * n + q];
                        a[(size_t)r * n + p] = a[(size_t)p * n + r] = c * arp - s * arq;
                        a[(size_t)r * n + q] = a[(size_t)q * n + r] = s * arp + c * arq;
                    }
                    const double zrp = Z[(size_t)r * n + p], zrq = Z[(size_t)r * n + q];
                    Z[(size_t)r * n + p] = c * zrp - s * zrq, Z[(size_t)r * n + q] = s * zrp + c * zrq;
                }
            }
    }
    w.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) w[(size_t)i] = a[(size_t)i * n + i];
}

} // namespace hipmf
