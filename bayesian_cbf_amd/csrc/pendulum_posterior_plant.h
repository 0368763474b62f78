// The pendulum's plant DRAWN FROM THE MODEL'S OWN POSTERIOR, and the rel-degree-2 condition on that draw (pendulum.hip's sampled
// plant kernel).  CBC2(x,u) = grad(L_f h)' (f + g u) + k_alpha[0] h + k_alpha[1] L_f h reads four columns of the posterior jet at x:
//     s = (f, g, df/dtheta, df/domega),   vec-covariance A (x) Sigma4,   mean = [Mk[:,0], Mk[:,1], Mj[:,(1+0)C], Mj[:,(1+1)C]]
// (after the task kernel has added the mean model), Sigma4 = rows / columns {0, 1, C, 2C} of Sigma6 = P6 - G with
// P6 = blockdiag(s2 Bm, kxx s2/ell_0^2 Bm, kxx s2/ell_1^2 Bm) -- the prior of the jet of a stationary kernel at x' = x, whose value /
// derivative cross blocks vanish -- and G = W6'W6 of the jets launch.  The marginal of a Gaussian is exact, so the g-derivative
// columns need not be drawn.  Everything in fp64 registers, every index a compile-time constant (no scratch).
#pragma once
#include "bcbf_common.h"

namespace bcbf {

// S = L L' of a positive-semidefinite N x N (lower triangle read): a pivot <= 0 leaves its column zero, so the draw stays in the
// range of S (the rule of psd_chol3, unicycle_task.h)
template <int N> __device__ inline void psd_chol(const double (&S)[N][N], double (&L)[N][N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int i = 0; i < N; ++i) L[i][j] = 0.0;
        double d = S[j][j];
#pragma unroll
        for (int p = 0; p < N; ++p) if (p < j) d -= L[j][p] * L[j][p];
        if (d > 0.0) {
            const double ljj = __builtin_sqrt(d);
            L[j][j] = ljj;
#pragma unroll
            for (int i = 0; i < N; ++i) if (i > j) {
                double v = S[i][j];
#pragma unroll
                for (int p = 0; p < N; ++p) if (p < j) v -= L[i][p] * L[j][p];
                L[i][j] = v / ljj;
            }
        }
    }
}

// Sigma4 (lower triangle; the upper is mirrored) from the step's workspace: Bk[2,2] = the top-left block as the jets wrote it,
// G[6,6], the prior's derivative variances kxx s2 / ell_d^2 Bm[0,0].  gp == 0 (no learned model, no prior): Sigma4 = 0.
template <typename T>
__device__ inline void pendulum_jet_covariance(int gp, const T* Bk, const T* G, T s2, T B00, const T* ell, double kxx,
                                               double (&S4)[4][4]) {
    constexpr int CT = 6;
    constexpr int ix[4] = {0, 1, 2, 4};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c <= a) {
            double v = 0.0;
            if (gp) {
                if (a < 2) v = (double)Bk[a * 2 + c];
                else {
                    v = -(double)G[ix[a] * CT + ix[c]];
                    if (a == c) {
                        const double l = (double)ell[a - 2];
                        v += kxx * (double)s2 / (l * l) * (double)B00;
                    }
                }
            }
            S4[a][c] = v;
            S4[c][a] = v;
        }
}

// S = mean + L_A Z L_S' for Z[2][4]: T[p][k] = sum_{q <= k} Z[p][q] L_S[k][q], then S[i][k] = mean[i][k] + sum_{p <= i} L_A[i][p] T[p][k]
__device__ inline void pendulum_jet_draw(const double (&mean)[2][4], const double (&LA)[2][2], const double (&LS)[4][4],
                                         const double (&Z)[2][4], double (&S)[2][4]) {
    double Tm[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q <= k) t += Z[p][q] * LS[k][q];
            Tm[p][k] = t;
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 2; ++p) if (p <= i) t += LA[i][p] * Tm[p][k];
            S[i][k] = mean[i][k] + t;
        }
}

// On the draw S = (f, g, df/dtheta, df/domega) and the control u: xd = f + g u,  lfh = gh' f,
// cbc2 = (Hh f + J' gh)' xd + k0 h + k1 lfh  with J[j][i] = d f_j / d x_i = S[j][2 + i]
__device__ inline void pendulum_cbc2_on(const double (&S)[2][4], double u, double h, const double (&gh)[2], const double (&Hh)[2][2],
                                        double k0, double k1, double (&xd)[2], double& lfh, double& cbc2) {
    xd[0] = S[0][0] + S[0][1] * u;
    xd[1] = S[1][0] + S[1][1] * u;
    lfh = gh[0] * S[0][0] + gh[1] * S[1][0];
    double gr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
        gr[i] = (Hh[i][0] * S[0][0] + Hh[i][1] * S[1][0]) + (S[0][2 + i] * gh[0] + S[1][2 + i] * gh[1]);
    cbc2 = (gr[0] * xd[0] + gr[1] * xd[1]) + k0 * h + k1 * lfh;
}

}  // namespace bcbf
