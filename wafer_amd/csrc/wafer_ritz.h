// One Rayleigh-Ritz step on k <= WAFER_RITZ_MAX states (host side; the sums H_ij = <l_i|H|l_j> and S_ij = <l_i|l_j> come from
// wafer_k_ritz_sums, wafer_ritz.hip.h).  Plain C++, no HIP: wafer_ritz_solve() of the C ABI serves it without a GPU.
//
//   A = (H + H^T) / 2, B = (S + S^T) / 2        the sums are symmetric up to their rounding
//   B = L L^T                                   Cholesky; a pivot <= 0 or a non-finite value: the states are linearly dependent
//   At = L^-1 A L^-T                            the standard problem of the same eigenvalues
//   At = Q diag(evals) Q^T                      cyclic Jacobi, until the off-diagonal Frobenius norm is <= 2^-52 |At|_F
//   C = L^-T Q                                  C^T B C = I, C^T A C = diag(evals)
// Eigenvalues ascend, the lower Jacobi index first on exact ties; each column of C has its component of largest magnitude
// positive (the lowest index on ties), so that the result does not depend on which way a rotation happened to turn.
// Nothing is written on failure.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef WAFER_RITZ_MAX
#define WAFER_RITZ_MAX 8
#endif

enum { WAFER_RITZ_OK = 0, WAFER_RITZ_DEPENDENT = 1, WAFER_RITZ_NO_CONVERGENCE = 2 };
enum { WAFER_RITZ_SWEEPS = 64 };

// h, s: row-major k x k.  evals[k]; coef[j * k + a] = component of input state j in output state a.  1 <= k <= WAFER_RITZ_MAX.
static inline int wafer_ritz_solve_host(int k, const double *h, const double *s, double *evals, double *coef)
{
    constexpr int M = WAFER_RITZ_MAX;
    double A[M][M], L[M][M], Q[M][M];
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) {
            A[i][j] = 0.5 * (h[i * k + j] + h[j * k + i]);
            L[i][j] = 0.5 * (s[i * k + j] + s[j * k + i]);   // B, overwritten by its factor below
            if (!std::isfinite(A[i][j]) || !std::isfinite(L[i][j])) return WAFER_RITZ_DEPENDENT;
        }
    // Cholesky, lower triangle in place
    for (int j = 0; j < k; ++j) {
        double d = L[j][j];
        for (int p = 0; p < j; ++p) d -= L[j][p] * L[j][p];
        if (!(d > 0.0) || !std::isfinite(d)) return WAFER_RITZ_DEPENDENT;
        const double piv = std::sqrt(d);
        L[j][j] = piv;
        for (int i = j + 1; i < k; ++i) {
            double t = L[i][j];
            for (int p = 0; p < j; ++p) t -= L[i][p] * L[j][p];
            L[i][j] = t / piv;
        }
        for (int i = 0; i < j; ++i) L[i][j] = 0.0;
    }
    // X = L^-1 A (column by column), then At = X L^-T, i.e. L At^T = X^T (row by row of X)
    for (int c = 0; c < k; ++c)
        for (int i = 0; i < k; ++i) {
            double t = A[i][c];
            for (int p = 0; p < i; ++p) t -= L[i][p] * A[p][c];
            A[i][c] = t / L[i][i];
        }
    for (int r = 0; r < k; ++r)
        for (int i = 0; i < k; ++i) {
            double t = A[r][i];
            for (int p = 0; p < i; ++p) t -= L[i][p] * A[r][p];
            A[r][i] = t / L[i][i];
        }
    double fro2 = 0.0;
    for (int i = 0; i < k; ++i)
        for (int j = i; j < k; ++j) {
            const double m = 0.5 * (A[i][j] + A[j][i]);
            A[i][j] = A[j][i] = m;
            fro2 += (i == j ? 1.0 : 2.0) * m * m;
        }
    if (!std::isfinite(fro2)) return WAFER_RITZ_DEPENDENT;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) Q[i][j] = i == j ? 1.0 : 0.0;
    // cyclic Jacobi (row order); every rotation sets its pivot to an exact zero
    const double stop2 = fro2 * 0x1p-104;
    bool converged = false;
    for (int sweep = 0; sweep <= WAFER_RITZ_SWEEPS; ++sweep) {
        double off2 = 0.0;
        for (int p = 0; p < k; ++p)
            for (int q = p + 1; q < k; ++q) off2 += 2.0 * A[p][q] * A[p][q];
        if (off2 <= stop2) { converged = true; break; }
        if (sweep == WAFER_RITZ_SWEEPS) break;
        for (int p = 0; p < k; ++p)
            for (int q = p + 1; q < k; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = std::isinf(theta) ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int r = 0; r < k; ++r) {   // columns p, q
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = c * arp - sn * arq;
                    A[r][q] = sn * arp + c * arq;
                }
                for (int r = 0; r < k; ++r) {   // rows p, q
                    const double apr = A[p][r], aqr = A[q][r];
                    A[p][r] = c * apr - sn * aqr;
                    A[q][r] = sn * apr + c * aqr;
                }
                A[p][q] = A[q][p] = 0.0;
                for (int r = 0; r < k; ++r) {
                    const double qrp = Q[r][p], qrq = Q[r][q];
                    Q[r][p] = c * qrp - sn * qrq;
                    Q[r][q] = sn * qrp + c * qrq;
                }
            }
    }
    if (!converged) return WAFER_RITZ_NO_CONVERGENCE;
    // ascending, the lower index first on exact ties (insertion sort: stable)
    int order[M];
    for (int i = 0; i < k; ++i) {
        if (!std::isfinite(A[i][i])) return WAFER_RITZ_DEPENDENT;
        int at = i;
        while (at > 0 && A[order[at - 1]][order[at - 1]] > A[i][i]) { order[at] = order[at - 1]; --at; }
        order[at] = i;
    }
    // C = L^-T Q: back substitution per column, then the sign rule
    double Cm[M][M];
    for (int a = 0; a < k; ++a) {
        const int col = order[a];
        for (int i = k - 1; i >= 0; --i) {
            double t = Q[i][col];
            for (int p = i + 1; p < k; ++p) t -= L[p][i] * Cm[p][a];
            Cm[i][a] = t / L[i][i];
            if (!std::isfinite(Cm[i][a])) return WAFER_RITZ_DEPENDENT;
        }
        int big = 0;
        for (int i = 1; i < k; ++i)
            if (std::fabs(Cm[i][a]) > std::fabs(Cm[big][a])) big = i;
        if (Cm[big][a] < 0.0)
            for (int i = 0; i < k; ++i) Cm[i][a] = -Cm[i][a];
    }
    for (int a = 0; a < k; ++a) evals[a] = A[order[a]][order[a]];
    for (int j = 0; j < k; ++j)
        for (int a = 0; a < k; ++a) coef[j * k + a] = Cm[j][a];
    return WAFER_RITZ_OK;
}
