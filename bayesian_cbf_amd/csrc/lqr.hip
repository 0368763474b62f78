// The reference's LQR nominal controller (LQRController.control, controllers.py:64-115), batched: one lane per instance, the
// whole finite-horizon Riccati recursion in registers.  The reference hands (A, B, Q, R, s, z, T) to the external package
// `bdlqr`; the recursion here is the same author's in-tree statement of it, affine_backpropagation (ilqr.py:43-76), with the
// same cost u'Ru + 2 z'u + x'Qx + 2 s'x.  Parity with bdlqr's own iterates is not claimed.
//
// Inputs are the jets' layout (bcbf_posterior_jets*: Mk[Bt,n,C], Mj[Bt,n,C(1+n)], C = 1+m), so the entry composes with them
// without a repack:  g = Mk[b,:,1:],  Jf[i][d] = Mj[b,i,(1+d)C],  Jg_j[i][d] = Mj[b,i,(1+d)C+1+j].  (f = Mk[b,:,0] is not
// read: the reference's linear system has no drift term.)
//   B = g dt,  s = -Q x_goal,  z = 0
//   pass(A): P = Q, o = s; T times { G = R + B'PB;  K = G^-1 B'PA;  k = G^-1 B'o;  P <- Q + A'PA - A'PB K;  o <- s + A'o - K'B'o }
//            -> -K x - k of the LAST iteration (x itself, not x - x_goal)
//   u0 = pass(I + dt Jf),   u = pass(I + dt (Jf + sum_j Jg_j u0_j))
// Every instantiation carries P, o, K, k in fp64: the fp32 entry reads and writes fp32 only (a plain fp32 recursion is 1.9e-3
// off at dt = 0.001, T = 1000 on pendulum linearisations).  The cost (Q, R, s) is uniform and arrives by value.
// The pendulum step (pendulum.hip, nominal = 1) launches the SAME kernel instantiation through lqr_nominal_step_f64, with the
// epsilon-greedy draw and the clip applied to its result.
#include "bcbf_common.h"
#include "lqr.h"

namespace bcbf {

template <int n, int m>
struct LqrCost {
    double Q[n][n], R[m][m], s[n];
};

// What the pendulum step adds to the kernel's result (m = 1): EpsilonGreedyController's draw, then the clip
struct LqrExplore {
    const double* explore;      // [Bt,2] uniform draws (coin, action) or NULL
    double eps;
    int clip;
    double lo, hi;
};

// G X = Y for the m x m G (m <= 3) and the nc columns of Y, in place, by elimination without exchanges: G = R + B'PB is positive
// definite wherever the problem is well posed, and a pivot that is not > 0 is what status 1 reports
template <int m, int nc>
__device__ inline bool lqr_solve(double (&G)[m][m], double (&Y)[m][nc]) {
    // one reciprocal per pivot and multiplications (an fp64 division is a dozen dependent instructions, and one wave per SIMD
    // hides none of them: with a division per entry they were a third of the n = 2, m = 1 iteration)
    bool ok = true;
    double inv[m];
#pragma unroll
    for (int p = 0; p < m; ++p) {
        const double piv = G[p][p];
        ok = ok && piv > 0.0;
        inv[p] = 1.0 / piv;
#pragma unroll
        for (int r = p + 1; r < m; ++r) {
            const double f = G[r][p] * inv[p];
#pragma unroll
            for (int c = p + 1; c < m; ++c) G[r][c] -= f * G[p][c];
#pragma unroll
            for (int c = 0; c < nc; ++c) Y[r][c] -= f * Y[p][c];
        }
    }
#pragma unroll
    for (int p = m - 1; p >= 0; --p) {
#pragma unroll
        for (int c = 0; c < nc; ++c) {
            double v = Y[p][c];
#pragma unroll
            for (int r = p + 1; r < m; ++r) v -= G[p][r] * Y[r][c];
            Y[p][c] = v * inv[p];
        }
    }
    return ok;
}

// One backward pass of T iterations on (A, B) and the control -K x - k of the last one
template <int n, int m>
__device__ inline bool lqr_pass(const double (&A)[n][n], const double (&B)[n][m], const LqrCost<n, m>& c,
                                const double (&x)[n], int T, double (&u)[m]) {
    double P[n][n], o[n], Kk[m][n + 1];          // Kk = [K | k]
#pragma unroll
    for (int i = 0; i < n; ++i) {
        o[i] = c.s[i];
#pragma unroll
        for (int j = 0; j < n; ++j) P[i][j] = c.Q[i][j];
    }
    bool ok = true;
    for (int it = 0; it < T; ++it) {
        double PB[n][m], PA[n][n], G[m][m];
#pragma unroll
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int j = 0; j < m; ++j) {
                double v = 0.0;
#pragma unroll
                for (int l = 0; l < n; ++l) v += P[i][l] * B[l][j];
                PB[i][j] = v;
            }
#pragma unroll
            for (int j = 0; j < n; ++j) {
                double v = 0.0;
#pragma unroll
                for (int l = 0; l < n; ++l) v += P[i][l] * A[l][j];
                PA[i][j] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < m; ++i) {
#pragma unroll
            for (int j = 0; j < m; ++j) {
                double v = c.R[i][j];
#pragma unroll
                for (int l = 0; l < n; ++l) v += B[l][i] * PB[l][j];
                G[i][j] = v;
            }
#pragma unroll
            for (int j = 0; j < n; ++j) {
                double v = 0.0;
#pragma unroll
                for (int l = 0; l < n; ++l) v += B[l][i] * PA[l][j];
                Kk[i][j] = v;
            }
            double w = 0.0;                      // z + B'o, z = 0
#pragma unroll
            for (int l = 0; l < n; ++l) w += B[l][i] * o[l];
            Kk[i][n] = w;
        }
        double w[m];
#pragma unroll
        for (int i = 0; i < m; ++i) w[i] = Kk[i][n];
        if (!lqr_solve<m, n + 1>(G, Kk)) {
            ok = false;
            break;
        }
        double Pn[n][n], on[n];
#pragma unroll
        for (int i = 0; i < n; ++i) {
            double vo = c.s[i];
#pragma unroll
            for (int l = 0; l < n; ++l) vo += A[l][i] * o[l];
#pragma unroll
            for (int l = 0; l < m; ++l) vo -= Kk[l][i] * w[l];
            on[i] = vo;
#pragma unroll
            for (int j = 0; j < n; ++j) {
                double v = c.Q[i][j];
#pragma unroll
                for (int l = 0; l < n; ++l) v += A[l][i] * PA[l][j];
                Pn[i][j] = v;
            }
            double AtPB[m];
#pragma unroll
            for (int l = 0; l < m; ++l) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < n; ++r) v += A[r][i] * PB[r][l];
                AtPB[l] = v;
            }
#pragma unroll
            for (int j = 0; j < n; ++j) {
#pragma unroll
                for (int l = 0; l < m; ++l) Pn[i][j] -= AtPB[l] * Kk[l][j];
            }
        }
#pragma unroll
        for (int i = 0; i < n; ++i) {
            o[i] = on[i];
#pragma unroll
            for (int j = 0; j < n; ++j) P[i][j] = Pn[i][j];
        }
    }
#pragma unroll
    for (int i = 0; i < m; ++i) {
        double v = -Kk[i][n];
#pragma unroll
        for (int j = 0; j < n; ++j) v -= Kk[i][j] * x[j];
        u[i] = ok ? v : 0.0;
    }
    return ok;
}

template <typename T, int n, int m>
__global__ void __launch_bounds__(64)
lqr_nominal_kernel(const T* __restrict__ Mk, const T* __restrict__ Mj, const T* __restrict__ x, LqrCost<n, m> c, double dt,
                   int numSteps, int t, const int* __restrict__ t_dev, LqrExplore E, T* __restrict__ u, T* __restrict__ u0,
                   int* __restrict__ status, int Bt) {
    constexpr int C = 1 + m, CT = C * (1 + n);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    // the horizon: T = max(numSteps - t, 1); a counter read from the device is held to t >= 0, so T <= numSteps bounds the loop
    int tt = t;
    if (t_dev) {
        tt = t_dev[0];
        tt = tt < 0 ? 0 : tt;
    }
    int Th = numSteps - tt;
    Th = Th < 1 ? 1 : Th;
    const T* mk = Mk + (size_t)b * n * C;
    const T* mj = Mj + (size_t)b * n * CT;
    double B[n][m], Jf[n][n], A[n][n], xs[n], ua[m], ub[m];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        xs[i] = (double)x[(size_t)b * n + i];
#pragma unroll
        for (int j = 0; j < m; ++j) B[i][j] = (double)mk[i * C + 1 + j] * dt;
#pragma unroll
        for (int d = 0; d < n; ++d) {
            Jf[i][d] = (double)mj[i * CT + (1 + d) * C];
            A[i][d] = (i == d ? 1.0 : 0.0) + dt * Jf[i][d];
        }
    }
    bool ok = lqr_pass<n, m>(A, B, c, xs, Th, ua);
    if (ok) {
#pragma unroll
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int d = 0; d < n; ++d) {
                double v = Jf[i][d];
#pragma unroll
                for (int j = 0; j < m; ++j) v += (double)mj[i * CT + (1 + d) * C + 1 + j] * ua[j];
                A[i][d] = (i == d ? 1.0 : 0.0) + dt * v;
            }
        }
        ok = lqr_pass<n, m>(A, B, c, xs, Th, ub);
    }
#pragma unroll
    for (int j = 0; j < m; ++j) {
        double v = ok ? ub[j] : 0.0;
        if constexpr (m == 1) {
            // EpsilonGreedyController around this controller, then clip = max(min(u, hi), lo) -- pendulum_task_kernel's lines
            if (E.explore && E.explore[(size_t)b * 2] < E.eps) v = E.lo + E.explore[(size_t)b * 2 + 1] * (E.hi - E.lo);
            if (E.clip) {
                v = v > E.hi ? E.hi : v;
                v = v < E.lo ? E.lo : v;
            }
        }
        u[(size_t)b * m + j] = (T)v;
        if (u0) u0[(size_t)b * m + j] = (T)(ok ? ua[j] : 0.0);
    }
    status[b] = ok ? 0 : 1;
}

static int lqr_einval(const char* why) {
    set_error_message(why);
    return BCBF_EINVAL;
}

template <typename T, int n, int m>
static int lqr_launch(const T* Mk, const T* Mj, const T* x, const T* x_goal, const T* Q, const T* R, double dt, int numSteps,
                      int t, const int* t_dev, const LqrExplore& E, T* u, T* u0, int* status, int Bt, hipStream_t st) {
    LqrCost<n, m> c;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) c.Q[i][j] = (double)Q[i * n + j];
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) c.R[i][j] = (double)R[i * m + j];
    for (int i = 0; i < n; ++i) {                // s = -Q x_goal
        double v = 0.0;
        for (int j = 0; j < n; ++j) v += c.Q[i][j] * (double)x_goal[j];
        c.s[i] = -v;
    }
    hipLaunchKernelGGL((lqr_nominal_kernel<T, n, m>), dim3((Bt + 63) / 64), dim3(64), 0, st, Mk, Mj, x, c, dt, numSteps, t,
                       t_dev, E, u, u0, status, Bt);
    return check_launch("lqr_nominal");
}

template <typename T>
static int lqr_nominal(const T* Mk, const T* Mj, const T* x, const T* x_goal, const T* Q, const T* R, T dt, int numSteps, int t,
                       const int* t_dev, const LqrExplore& E, T* u, T* u0, int* status, int Bt, int n, int m, void* stream) {
    // ---- argument checks, before any HIP call
    if (Bt < 0) return lqr_einval("lqr_nominal: Bt < 0");
    if (n < 1 || n > 4 || m < 1 || m > 3) return lqr_einval("lqr_nominal: compiled for 1 <= n <= 4, 1 <= m <= 3");
    if (!Mk || !Mj || !x || !x_goal || !Q || !R || !u || !status) return lqr_einval("lqr_nominal: null required pointer");
    if (!(dt > T(0))) return lqr_einval("lqr_nominal: dt must be > 0");
    if (numSteps < 1) return lqr_einval("lqr_nominal: numSteps < 1");
    if (!t_dev && t < 0) return lqr_einval("lqr_nominal: t < 0 without t_dev");
    if (Bt == 0) return BCBF_OK;
    hipStream_t st = (hipStream_t)stream;
#define BCBF_LQR(NN, MM) \
    if (n == NN && m == MM) return lqr_launch<T, NN, MM>(Mk, Mj, x, x_goal, Q, R, (double)dt, numSteps, t, t_dev, E, u, u0, status, Bt, st);
    BCBF_LQR(1, 1) BCBF_LQR(1, 2) BCBF_LQR(1, 3)
    BCBF_LQR(2, 1) BCBF_LQR(2, 2) BCBF_LQR(2, 3)
    BCBF_LQR(3, 1) BCBF_LQR(3, 2) BCBF_LQR(3, 3)
    BCBF_LQR(4, 1) BCBF_LQR(4, 2) BCBF_LQR(4, 3)
#undef BCBF_LQR
    return lqr_einval("lqr_nominal: shape not compiled");
}

// the pendulum step's nominal control (n = 2, m = 1): the public entry's kernel with the explorer's draw and the clip
int lqr_nominal_step_f64(const double* Mk, const double* Mj, const double* x, const double* x_goal, const double* Q, double R,
                         double dt, int numSteps, int t, const int* t_dev, const double* explore, double eps, int clip,
                         double lo, double hi, double* u_ref, int* lstatus, int Bt, void* stream) {
    const LqrExplore E{explore, eps, clip, lo, hi};
    return lqr_nominal<double>(Mk, Mj, x, x_goal, Q, &R, dt, numSteps, t, t_dev, E, u_ref, nullptr, lstatus, Bt, 2, 1, stream);
}

}  // namespace bcbf

extern "C" {
#define BCBF_LQR_ENTRY(T, SUF)                                                                                              \
    int bcbf_lqr_nominal_##SUF(const T* Mk, const T* Mj, const T* x, const T* x_goal, const T* Q, const T* R, T dt,         \
                               int numSteps, int t, const int* t_dev, T* u, T* u0, int* status, int Bt, int n, int m,       \
                               void* stream) {                                                                              \
        return bcbf::lqr_nominal<T>(Mk, Mj, x, x_goal, Q, R, dt, numSteps, t, t_dev, bcbf::LqrExplore{}, u, u0, status, Bt, \
                                    n, m, stream);                                                                          \
    }
BCBF_LQR_ENTRY(float, f32)
BCBF_LQR_ENTRY(double, f64)
#undef BCBF_LQR_ENTRY
}
