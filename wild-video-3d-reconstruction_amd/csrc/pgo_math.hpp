// pgo_math.hpp -- per-thread fp64 Sim3 algebra of the pose-graph optimiser
// (pgo.hip): the exact left Jacobian, a 7x7 inverse, the SE3 -> Sim3 lift.
#pragma once

#include "liegroups.hpp"

namespace dpvo {
namespace pgo {

using S3 = lie::Sim3<double>;

// ---------------------------------------------------------------------------
// 7x7 helpers
// ---------------------------------------------------------------------------
__device__ static void eye7(double A[7][7])
{
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) A[i][j] = (double)(i == j);
}

// exact left Jacobian of Sim3 at x (see the header comment)
__device__ static void exact_left_jacobian(const double* x, double J[7][7])
{
    double s = 0;
    for (int i = 0; i < 7; i++) s += fabs(x[i]);
    int m = 0;
    while (s > 0.25 && m < 60) { s *= 0.5; m++; }
    const double sc = ldexp(1.0, -m);
    double y[7], X[7][7], A[7][7];
    for (int i = 0; i < 7; i++) y[i] = x[i] * sc;
    S3::ad(y, X);
    // Horner: Jl = I + X/2 (I + X/3 (I + ...)), exp = I + X (I + X/2 (I + ...)); |X| <= 1/4, 13 terms
    eye7(J);
    eye7(A);
    for (int k = 13; k >= 1; k--) {
        lie::mmk<double, 7>(X, J, J);
        lie::mmk<double, 7>(X, A, A);
        const double cj = 1.0 / (double)(k + 1), ca = 1.0 / (double)k;
        for (int i = 0; i < 7; i++)
            for (int j = 0; j < 7; j++) {
                J[i][j] = (double)(i == j) + cj * J[i][j];
                A[i][j] = (double)(i == j) + ca * A[i][j];
            }
    }
    for (int d = 0; d < m; d++) {
        double H[7][7];
        for (int i = 0; i < 7; i++)
            for (int j = 0; j < 7; j++) H[i][j] = 0.5 * ((double)(i == j) + A[i][j]);
        lie::mmk<double, 7>(H, J, J);
        lie::mmk<double, 7>(A, A, A);
    }
}

// B = A^-1, Gauss-Jordan with partial pivoting (A is overwritten)
__device__ static void inv7(double A[7][7], double B[7][7])
{
    eye7(B);
    for (int c = 0; c < 7; c++) {
        int p = c;
        double best = fabs(A[c][c]);
        for (int r = c + 1; r < 7; r++)
            if (fabs(A[r][c]) > best) { best = fabs(A[r][c]); p = r; }
        if (p != c)
            for (int j = 0; j < 7; j++) {
                double t = A[c][j]; A[c][j] = A[p][j]; A[p][j] = t;
                t = B[c][j]; B[c][j] = B[p][j]; B[p][j] = t;
            }
        const double id = 1.0 / A[c][c];
        for (int j = 0; j < 7; j++) { A[c][j] *= id; B[c][j] *= id; }
        for (int r = 0; r < 7; r++) {
            if (r == c) continue;
            const double f = A[r][c];
            for (int j = 0; j < 7; j++) { A[r][j] -= f * A[c][j]; B[r][j] -= f * B[c][j]; }
        }
    }
}

__device__ static S3 se3_as_sim3_inv(const double* pose)  // Sim3([t, q, 1])^-1
{
    double d[8];
    for (int i = 0; i < 7; i++) d[i] = pose[i];
    d[7] = 1.0;
    return S3::load(d).inv();
}

// r = Log(M), M = C Exp(g_i) Exp(g_j)^-1
__device__ static S3 edge_residual(const S3& C, const double* gi, const double* gj, double* r)
{
    const S3 M = C.mul(S3::Exp(gi)).mul(S3::Exp(gj).inv());
    M.Log(r);
    return M;
}

// J_i = Jl^-1(r) Ad(C) Jl(g_i), J_j = -Jl^-1(r) Ad(M) Jl(g_j); jli / jlj: the
// exact Jl(g_i) / Jl(g_j), row-major 7x7 like the outputs
__device__ static void edge_jacobians(const S3& C, const S3& M, const double* r, const double* jli, const double* jlj,
                                      double* Ji, double* Jj)
{
    double Jr[7][7], Jinv[7][7], Ad[7][7], P[7][7], T[7][7];
    exact_left_jacobian(r, Jr);
    inv7(Jr, Jinv);
    C.Adj(Ad);
    for (int a = 0; a < 7; a++)
        for (int b = 0; b < 7; b++) P[a][b] = jli[a * 7 + b];
    lie::mmk<double, 7>(Ad, P, T);
    lie::mmk<double, 7>(Jinv, T, T);
    for (int a = 0; a < 7; a++)
        for (int b = 0; b < 7; b++) Ji[a * 7 + b] = T[a][b];
    M.Adj(Ad);
    for (int a = 0; a < 7; a++)
        for (int b = 0; b < 7; b++) P[a][b] = jlj[a * 7 + b];
    lie::mmk<double, 7>(Ad, P, T);
    lie::mmk<double, 7>(Jinv, T, T);
    for (int a = 0; a < 7; a++)
        for (int b = 0; b < 7; b++) Jj[a * 7 + b] = -T[a][b];
}

}  // namespace pgo
}  // namespace dpvo
