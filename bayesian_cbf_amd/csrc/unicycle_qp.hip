// The unicycle's CLF-CBF quadratic program on the MEAN model (ControllerCLF, unicycle_move_to_pose.py:699-791): per step the
// control-Lyapunov row, relaxed by a free variable of linear weight w, the control box and one hard barrier row per obstacle,
//     minimise |u|^2 + w relax   subject to   lo <= u <= hi,   a_c.u + b_c - relax <= 0,   a_k.u + b_k >= 0   (k < Kob <= 3).
// Three entries: the program alone, one control evaluation for a batch of states, and the closed loop itself -- every step of a
// rollout inside ONE launch, one lane per instance, as pendulum_qp.hip does for the pendulum: planner, rows, program, statistics
// and plant step touch no memory, so state, parameters, control points and statistics stay in registers and only the optional
// recording stores.
//
// The program.  relax is free with a positive linear cost, so its row is tight, relax = a_c.u + b_c, and the objective becomes
// |u + (w/2) a_c|^2 + const: u* is the Euclidean projection of p = -(w/2) a_c onto the polygon {box} n {a_k.u + b_k >= 0},
// relax* = a_c.u* + b_c (it may be negative).  The optimum is unique, the box excludes unboundedness, the program is infeasible
// exactly when the polygon is empty.  The projection onto M = 4 + Kob <= 7 half-planes is found by enumerating the active sets
// of size <= 2 (clf_cbf_qp2_solve below): at most 1 + 7 + 21 = 29 candidates.  The reference hands the program to GUROBI through
// cvxpy; parity with its iterates is not claimed.
//
// Everything is compiled per Kob so that every index of the row arrays is a compile-time constant (a runtime-indexed register
// array goes to scratch).  No LDS, no inline assembly.
#include "bcbf_common.h"
#include "unicycle_task.h"       // unicycle_row_vals, ackermann_g, ackermann_euler, normalize_radians
#include <stdio.h>
#include <limits>

namespace bcbf {

template <typename T> struct UqpVec2;
template <> struct UqpVec2<float> { using type = float2; };
template <> struct UqpVec2<double> { using type = double2; };

// (not `v - v == 0`: with the compiler's default contraction, v = a * b turns that into fma(a, b, -(a * b)), the rounding error
// of the product, which is not 0)
template <typename T> __device__ inline bool uqp_finite(T v) { return fabs(v) <= std::numeric_limits<T>::max(); }

// The M = 4 + KOB half-planes a_i.u + b_i >= 0, in the order lo0, lo1, hi0, hi1, hard rows
template <typename T, int KOB>
struct Qp2Rows {
    T a[4 + KOB][2];
    T b[4 + KOB];
};

template <typename T, int KOB>
__device__ inline void qp2_box(Qp2Rows<T, KOB>& r, T lo0, T lo1, T hi0, T hi1) {
    r.a[0][0] = T(1);  r.a[0][1] = T(0);  r.b[0] = -lo0;
    r.a[1][0] = T(0);  r.a[1][1] = T(1);  r.b[1] = -lo1;
    r.a[2][0] = T(-1); r.a[2][1] = T(0);  r.b[2] = hi0;
    r.a[3][0] = T(0);  r.a[3][1] = T(-1); r.b[3] = hi1;
}

// Projection of p = -(w/2) a_c onto the polygon of `r`.  Candidates, in this order: p itself; the foot of p on each line, in row
// order (a row with zero normal is no candidate); each pairwise intersection, in lexicographic order (a pair whose determinant is
// exactly 0 is no candidate).  A candidate is admissible when every row NOT in its active set satisfies a_i.u + b_i >= -tol_i,
// tol_i = 64 eps (|a_i0 u0| + |a_i1 u1| + |b_i|) -- a zero-normal row thereby reduces to b_i >= -tol_i.  The answer is the
// admissible candidate nearest to p, ties to the first in the order (strict <).  No admissible candidate, or a non-finite row or
// result: status 1, nothing written.  `active`: bit i set for row i of the winning candidate's active set.
// No contraction into fused multiply-adds in here: the rule's exact tests (determinant == 0, strict <) are stated on the rounded
// products -- a contracted a d - b c of two parallel rows is the rounding error of b c, not 0.
template <typename T, int KOB>
__device__ inline int clf_cbf_qp2_solve(const Qp2Rows<T, KOB>& r, T ac0, T ac1, T bc, T w, T& u0, T& u1, T& relax, int& active) {
#pragma clang fp contract(off)
    constexpr int M = 4 + KOB;
    const T tol64 = T(64) * std::numeric_limits<T>::epsilon();
    bool fin = uqp_finite(ac0) && uqp_finite(ac1) && uqp_finite(bc);
#pragma unroll
    for (int i = 0; i < M; ++i) fin = fin && uqp_finite(r.a[i][0]) && uqp_finite(r.a[i][1]) && uqp_finite(r.b[i]);
    if (!fin) return 1;
    const T p0 = -(w / T(2)) * ac0, p1 = -(w / T(2)) * ac1;
    T best = std::numeric_limits<T>::infinity(), bu0 = T(0), bu1 = T(0);
    int bact = 0;
    bool found = false;
    // candidate (c0, c1) with active rows i, j (-1: none); `valid`: the candidate exists
    auto consider = [&](T c0, T c1, int i, int j, bool valid) __attribute__((always_inline)) {
#pragma clang fp contract(off)
        bool ok = valid;
#pragma unroll
        for (int q = 0; q < M; ++q) {
            if (q == i || q == j) continue;
            const T t0 = r.a[q][0] * c0, t1 = r.a[q][1] * c1;
            const T s = t0 + t1 + r.b[q];
            const T tol = tol64 * (fabs(t0) + fabs(t1) + fabs(r.b[q]));
            ok = ok && (s >= -tol);
        }
        const T d0 = c0 - p0, d1 = c1 - p1;
        const T d = d0 * d0 + d1 * d1;
        if (ok && d < best) {
            best = d; bu0 = c0; bu1 = c1; found = true;
            bact = (i >= 0 ? 1 << i : 0) | (j >= 0 ? 1 << j : 0);
        }
    };
    consider(p0, p1, -1, -1, true);
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const T n2 = r.a[i][0] * r.a[i][0] + r.a[i][1] * r.a[i][1];
        const bool valid = !(r.a[i][0] == T(0) && r.a[i][1] == T(0));
        const T tt = (r.a[i][0] * p0 + r.a[i][1] * p1 + r.b[i]) / n2;
        consider(p0 - r.a[i][0] * tt, p1 - r.a[i][1] * tt, i, -1, valid);
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = i + 1; j < M; ++j) {
            const T det = r.a[i][0] * r.a[j][1] - r.a[i][1] * r.a[j][0];
            const bool valid = det != T(0);
            const T c0 = (r.b[j] * r.a[i][1] - r.b[i] * r.a[j][1]) / det;
            const T c1 = (r.b[i] * r.a[j][0] - r.b[j] * r.a[i][0]) / det;
            consider(c0, c1, i, j, valid);
        }
    }
    if (!found) return 1;
    const T rl = ac0 * bu0 + ac1 * bu1 + bc;
    if (!(uqp_finite(bu0) && uqp_finite(bu1) && uqp_finite(rl))) return 1;
    u0 = bu0; u1 = bu1; relax = rl; active = bact;
    return 0;
}

// Host values of the task, passed by value
template <typename T>
struct UnicycleQpTask {
    T Kp[4], clf_gamma, relax_weight, lo[2], hi[2], tw[2], gam[3];
};

template <typename T, int KOB>
struct UnicycleQpObstacles {
    T cx[KOB + 1], cy[KOB + 1], rad[KOB + 1];         // (+1: no zero-length array for KOB = 0)
};

template <typename T, int KOB>
__device__ inline UnicycleQpObstacles<T, KOB> unicycle_qp_obstacles(const T* __restrict__ centers, const T* __restrict__ radii,
                                                                    int obs_stride, int b) {
    UnicycleQpObstacles<T, KOB> o;
#pragma unroll
    for (int k = 0; k < KOB; ++k) {
        const size_t at = (size_t)b * obs_stride * KOB + k;
        o.cx[k] = centers[at * 2];
        o.cy[k] = centers[at * 2 + 1];
        o.rad[k] = radii[at];
    }
    return o;
}

// The rows at x on the controller's model.  POLAR = false: CLFCartesian and ObstacleCBF on AckermannDrive(L) (f = 0): unicycle_row
// gives the gradient and the constant of each row, a_k = grad_k . g(x; L), b_k = cst_k.  POLAR = true (KOB = 0): CLFPolar on
// PolarDynamics through cartesian2polar (unicycle_move_to_pose.py:112-167, 442-497).  V and h_k: the CLF's and the barriers'
// values (V only where want_V: it is an output of the control entry alone).
template <typename T, int KOB, bool POLAR>
__device__ inline void unicycle_qp_rows(T px, T py, T th, const T (&plan)[3], const T (&dot_plan)[3], T L,
                                        const UnicycleQpTask<T>& p, const UnicycleQpObstacles<T, KOB>& o, bool want_V,
                                        T& ac0, T& ac1, T& bc, T& V, Qp2Rows<T, KOB>& r, T (&h)[KOB + 1]) {
    V = T(0);
    if (POLAR) {
        const T xd = plan[0] - px, yd = plan[1] - py;
        T rho = sqrt(xd * xd + yd * yd);
        if (!(rho > T(1e-6))) rho = std::numeric_limits<T>::quiet_NaN();      // the reference asserts here: refused (status 1)
        const T phi = atan2(yd, xd);
        const T alpha = normalize_radians(th - phi), beta = normalize_radians(plan[2] - phi);
        const T sa = sin(alpha), ca = cos(alpha), sb = sin(beta), sba = sin(beta - alpha);
        V = T(0.5) * p.Kp[0] * rho * rho + p.Kp[1] * (T(1) - ca) + p.Kp[2] * (T(1) - cos(beta))
            + p.Kp[3] * (T(1) - cos(beta - alpha));
        const T gv0 = p.Kp[0] * rho, gv1 = p.Kp[1] * sa - p.Kp[3] * sba, gv2 = p.Kp[2] * sb + p.Kp[3] * sba;
        const T sr = -sa / rho;
        ac0 = gv0 * (-ca) + gv1 * sr + gv2 * sr;
        ac1 = gv1;
        bc = p.clf_gamma * V;
    } else {
        T G[3][2];
        ackermann_g<T>(th, L, G);
        const T Kp3[3] = {p.Kp[0], p.Kp[1], p.Kp[2]};
        T g[3], cst;
        unicycle_row_vals<T>(0, px, py, th, plan, dot_plan, Kp3, p.clf_gamma, T(0), T(0), T(0), p.tw[0], p.tw[1], T(0), g, cst);
        ac0 = g[0] * G[0][0] + g[1] * G[1][0] + g[2] * G[2][0];
        ac1 = g[0] * G[0][1] + g[1] * G[1][1] + g[2] * G[2][1];
        bc = cst;
        if (want_V) {       // gamma = 1 on a resting plan: the constant of the row is V itself
            const T zero[3] = {T(0), T(0), T(0)};
            T g2[3];
            unicycle_row_vals<T>(0, px, py, th, plan, zero, Kp3, T(1), T(0), T(0), T(0), p.tw[0], p.tw[1], T(0), g2, V);
        }
#pragma unroll
        for (int k = 0; k < KOB; ++k) {
            T hk;       // gamma = 1: the constant of the row is h_k itself, and b_k = gamma_k h_k as unicycle_row forms it
            unicycle_row_vals<T>(1 + k, px, py, th, plan, dot_plan, Kp3, p.clf_gamma, o.cx[k], o.cy[k], o.rad[k], p.tw[0],
                                 p.tw[1], T(1), g, hk);
            h[k] = hk;
            r.a[4 + k][0] = g[0] * G[0][0] + g[1] * G[1][0] + g[2] * G[2][0];
            r.a[4 + k][1] = g[0] * G[0][1] + g[1] * G[1][1] + g[2] * G[2][1];
            r.b[4 + k] = p.gam[k] * hk;
        }
    }
}

// ---- the program alone
template <typename T, int KOB>
__global__ void __launch_bounds__(64)
clf_cbf_qp2_kernel(const T* __restrict__ a, const T* __restrict__ bv, T lo0, T lo1, T hi0, T hi1, T w, T* __restrict__ u,
                   T* __restrict__ relax, int* __restrict__ active, int* __restrict__ status, int Bt) {
    constexpr int K = 1 + KOB;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    const T* ab = a + (size_t)b * K * 2;
    const T* bb = bv + (size_t)b * K;
    Qp2Rows<T, KOB> r;
    qp2_box<T, KOB>(r, lo0, lo1, hi0, hi1);
#pragma unroll
    for (int k = 0; k < KOB; ++k) {
        r.a[4 + k][0] = ab[(1 + k) * 2];
        r.a[4 + k][1] = ab[(1 + k) * 2 + 1];
        r.b[4 + k] = bb[1 + k];
    }
    T u0 = T(0), u1 = T(0), rl = T(0);
    int act = 0;
    const int st = clf_cbf_qp2_solve<T, KOB>(r, ab[0], ab[1], bb[0], w, u0, u1, rl, act);
    if (status) status[b] = st;
    if (st == 0) {
        if (u) { u[(size_t)b * 2] = u0; u[(size_t)b * 2 + 1] = u1; }
        if (relax) relax[b] = rl;
        if (active) active[b] = act;
    }
}

// ---- one control evaluation
template <typename T, int KOB, bool POLAR>
__global__ void __launch_bounds__(64)
unicycle_clf_cbf_control_kernel(const T* __restrict__ x, const T* __restrict__ plan, const T* __restrict__ dot_plan,
                                UnicycleQpTask<T> p, const T* __restrict__ L_ctrl, int L_stride,
                                const T* __restrict__ centers, const T* __restrict__ radii, int obs_stride,
                                T* __restrict__ a, T* __restrict__ bv, T* __restrict__ values, T* __restrict__ u,
                                T* __restrict__ relax, int* __restrict__ active, int* __restrict__ status, int Bt) {
    constexpr int K = 1 + KOB;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    const T L = L_ctrl[(size_t)b * L_stride];
    const UnicycleQpObstacles<T, KOB> o = unicycle_qp_obstacles<T, KOB>(centers, radii, obs_stride, b);
    const T pl[3] = {plan[(size_t)b * 3], plan[(size_t)b * 3 + 1], plan[(size_t)b * 3 + 2]};
    const T dp[3] = {dot_plan[(size_t)b * 3], dot_plan[(size_t)b * 3 + 1], dot_plan[(size_t)b * 3 + 2]};
    Qp2Rows<T, KOB> r;
    qp2_box<T, KOB>(r, p.lo[0], p.lo[1], p.hi[0], p.hi[1]);
    T ac0, ac1, bc, V, h[KOB + 1];
    unicycle_qp_rows<T, KOB, POLAR>(x[(size_t)b * 3], x[(size_t)b * 3 + 1], x[(size_t)b * 3 + 2], pl, dp, L, p, o, true, ac0, ac1,
                                    bc, V, r, h);
    if (a) {
        a[(size_t)b * K * 2] = ac0; a[(size_t)b * K * 2 + 1] = ac1;
#pragma unroll
        for (int k = 0; k < KOB; ++k) {
            a[((size_t)b * K + 1 + k) * 2] = r.a[4 + k][0];
            a[((size_t)b * K + 1 + k) * 2 + 1] = r.a[4 + k][1];
        }
    }
    if (bv) {
        bv[(size_t)b * K] = bc;
#pragma unroll
        for (int k = 0; k < KOB; ++k) bv[(size_t)b * K + 1 + k] = r.b[4 + k];
    }
    if (values) {
        values[(size_t)b * K] = V;
#pragma unroll
        for (int k = 0; k < KOB; ++k) values[(size_t)b * K + 1 + k] = h[k];
    }
    T u0 = T(0), u1 = T(0), rl = T(0);
    int act = 0;
    const int st = clf_cbf_qp2_solve<T, KOB>(r, ac0, ac1, bc, p.relax_weight, u0, u1, rl, act);
    if (status) status[b] = st;
    if (st == 0) {
        if (u) { u[(size_t)b * 2] = u0; u[(size_t)b * 2 + 1] = u1; }
        if (relax) relax[b] = rl;
        if (active) active[b] = act;
    }
}

// PiecewiseLinearPlanner (planner.py:19-64): three control points in (x, y, cos, sin); the integers come from the host
struct UnicycleQpPlanner {
    int kind, t2, lookahead, numStepsPlan;
};

// ---- the closed loop, numSteps steps in one launch.  Per step, in sample_generator_trajectory's order: the convergence test
// (stop_rho), the plan at the global step, rows at x_t on the controller's model, the program, min_h and cost of x_t, the Euler
// step on the PLANT's wheelbase; no angle wrap (the reference applies none).  An instance whose program cannot be solved records
// the 1-based global step in status and freezes, state and statistics as before that step; one with rho(x_t, goal) < stop_rho
// records converged_at = the global step and stops, status 0.  Recording as pendulum_clf_cbf_rollout_kernel does it.
template <typename T, int KOB, bool POLAR>
__global__ void __launch_bounds__(64)
unicycle_clf_cbf_rollout_kernel(T* __restrict__ x, const T* __restrict__ goal, const T* __restrict__ x0_plan,
                                UnicycleQpPlanner pk, UnicycleQpTask<T> p, const T* __restrict__ L_ctrl, int Lc_stride,
                                const T* __restrict__ L_true, int Lt_stride, const T* __restrict__ centers,
                                const T* __restrict__ radii, int obs_stride, T dt, T stop_rho, T* __restrict__ min_h,
                                T* __restrict__ cost, int* __restrict__ status, int* __restrict__ converged_at,
                                T* __restrict__ traj, T* __restrict__ u_rec, int record_every, int t_offset, int numSteps,
                                int Bt) {
    using P2 = typename UqpVec2<T>::type;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    const T Lc = L_ctrl[(size_t)b * Lc_stride], Lt = L_true[(size_t)b * Lt_stride];
    const UnicycleQpObstacles<T, KOB> o = unicycle_qp_obstacles<T, KOB>(centers, radii, obs_stride, b);
    const T g0 = goal[(size_t)b * 3], g1 = goal[(size_t)b * 3 + 1], g2 = goal[(size_t)b * 3 + 2];
    // control points: c0 the start, c1 the goal's position with the heading of the straight line, c2 the goal
    T c0[4] = {T(0), T(0), T(0), T(0)}, c1[4] = {T(0), T(0), T(0), T(0)}, c2[4] = {T(0), T(0), T(0), T(0)};
    if (pk.kind == 1) {
        const T s0 = x0_plan[(size_t)b * 3], s1 = x0_plan[(size_t)b * 3 + 1], s2 = x0_plan[(size_t)b * 3 + 2];
        const T d0 = g0 - s0, d1 = g1 - s1;
        const T dn = sqrt(d0 * d0 + d1 * d1);
        c0[0] = s0; c0[1] = s1; c0[2] = cos(s2); c0[3] = sin(s2);
        c1[0] = g0; c1[1] = g1; c1[2] = d0 / dn; c1[3] = d1 / dn;
        c2[0] = g0; c2[1] = g1; c2[2] = cos(g2); c2[3] = sin(g2);
    }
    T px = x[(size_t)b * 3], py = x[(size_t)b * 3 + 1], th = x[(size_t)b * 3 + 2];
    T mh = KOB > 0 ? min_h[b] : T(0), cs = cost[b];
    int st = status[b], conv = converged_at ? converged_at[b] : -1;
    const bool rec = record_every > 0 && (traj || u_rec);
    int until = rec ? (record_every - t_offset % record_every) % record_every : -1;   // steps until the next recorded one
    size_t row = 0;
    Qp2Rows<T, KOB> r;
    qp2_box<T, KOB>(r, p.lo[0], p.lo[1], p.hi[0], p.hi[1]);
    for (int t = 0; t < numSteps; ++t) {
        T u0 = T(0), u1 = T(0);
        bool live = st == 0 && conv < 0;
        if (live) {
            const T xd = g0 - px, yd = g1 - py;
            if (sqrt(xd * xd + yd * yd) < stop_rho) {
                conv = t_offset + t;
                live = false;
            }
        }
        if (live) {
            T pl[3] = {g0, g1, g2}, dp[3] = {T(0), T(0), T(0)};
            if (pk.kind == 1) {
                const int tg = t_offset + t;
                const int tt = tg + pk.lookahead < pk.numStepsPlan ? tg + pk.lookahead : pk.numStepsPlan;
                const bool first = tt <= pk.t2;
                const int pt = first ? 0 : pk.t2, ct = first ? pk.t2 : pk.numStepsPlan;
                const T num = T(tt - pt), den = T(ct - pt), dend = den * dt;
                T xp[4], xv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const T from = first ? c0[i] : c1[i], to = first ? c1[i] : c2[i];
                    xp[i] = (to - from) * num / den + from;
                    xv[i] = (to - from) / dend;
                }
                pl[0] = xp[0]; pl[1] = xp[1]; pl[2] = atan2(xp[3], xp[2]);
                dp[0] = xv[0]; dp[1] = xv[1]; dp[2] = (xv[2] - xv[3]) / (xv[2] * xv[2] + xv[3] * xv[3]);
            }
            T ac0, ac1, bc, V, h[KOB + 1], rl = T(0);
            int act = 0;
            unicycle_qp_rows<T, KOB, POLAR>(px, py, th, pl, dp, Lc, p, o, false, ac0, ac1, bc, V, r, h);
            if (clf_cbf_qp2_solve<T, KOB>(r, ac0, ac1, bc, p.relax_weight, u0, u1, rl, act)) {
                st = t_offset + t + 1;
                u0 = T(0); u1 = T(0);
                live = false;
            } else {
#pragma unroll
                for (int k = 0; k < KOB; ++k) {
                    const T hv = uqp_finite(h[k]) ? h[k] : T(-INFINITY);   // a non-finite h never passes for "safe"
                    mh = hv < mh ? hv : mh;
                }
                cs += u0 * u0 + u1 * u1;
            }
        }
        if (until == 0) {
            if (traj) {
                T* tr = traj + (row * Bt + b) * 3;
                tr[0] = px; tr[1] = py; tr[2] = th;
            }
            if (u_rec) {
                P2 v;
                v.x = u0; v.y = u1;
                reinterpret_cast<P2*>(u_rec)[row * Bt + b] = v;
            }
            ++row;
            until = record_every;
        }
        --until;
        if (live) {
            T n0, n1, n2;
            ackermann_euler<T>(px, py, th, u0, u1, dt, Lt, n0, n1, n2);
            px = n0; py = n1; th = n2;
        }
    }
    x[(size_t)b * 3] = px; x[(size_t)b * 3 + 1] = py; x[(size_t)b * 3 + 2] = th;
    if (KOB > 0) min_h[b] = mh;
    cost[b] = cs;
    status[b] = st;
    if (converged_at) converged_at[b] = conv;
}

static int unicycle_qp_einval(const char* entry, const char* why) {
    char msg[240];
    snprintf(msg, sizeof(msg), "%s: %s", entry, why);
    set_error_message(msg);
    return BCBF_EINVAL;
}

template <typename T> static bool uqp_host_finite(T v) { return fabs(v) <= std::numeric_limits<T>::max(); }

template <typename T>
static const char* unicycle_qp_box(const T* lo, const T* hi, T relax_weight) {
    if (!lo || !hi) return "null lo or hi";
    for (int i = 0; i < 2; ++i)
        if (!uqp_host_finite(lo[i]) || !uqp_host_finite(hi[i])) return "lo and hi must be finite (the box excludes unboundedness)";
    if (!(relax_weight > T(0)) || !uqp_host_finite(relax_weight)) return "relax_weight must be > 0 and finite";
    return nullptr;
}

template <typename T>
static const char* unicycle_qp_task(const T* Kp, int clf_kind, T clf_gamma, T relax_weight, const T* lo, const T* hi,
                                    const T* L_ctrl, int L_stride, const T* centers, const T* radii, int obs_stride,
                                    const T* tw, const T* gammas, int Kob, UnicycleQpTask<T>& p) {
    if (Kob < 0 || Kob > 3) return "Kob must be 0..3";
    if (clf_kind != 0 && clf_kind != 1) return "clf_kind must be 0 (CLFCartesian) or 1 (CLFPolar)";
    if (clf_kind == 1 && Kob != 0) return "clf_kind 1 (CLFPolar) takes no obstacles: ObstacleCBF is stated in Cartesian coordinates";
    if (!Kp) return "null Kp";
    if (const char* why = unicycle_qp_box<T>(lo, hi, relax_weight)) return why;
    if (!uqp_host_finite(clf_gamma)) return "clf_gamma must be finite";
    if (!L_ctrl) return "null L_ctrl";
    if (L_stride != 0 && L_stride != 1) return "L_ctrl stride must be 0 (shared) or 1 (per instance)";
    if (Kob > 0 && (!centers || !radii || !tw || !gammas)) return "null centers, radii, tw or gammas with Kob > 0";
    if (obs_stride != 0 && obs_stride != 1) return "obstacle stride must be 0 (shared) or 1 (per instance)";
    for (int i = 0; i < 4; ++i) p.Kp[i] = Kp[i];
    p.clf_gamma = clf_gamma; p.relax_weight = relax_weight;
    for (int i = 0; i < 2; ++i) { p.lo[i] = lo[i]; p.hi[i] = hi[i]; p.tw[i] = Kob > 0 ? tw[i] : T(0); }
    for (int k = 0; k < 3; ++k) p.gam[k] = k < Kob ? gammas[k] : T(0);
    return nullptr;
}

template <typename T>
static int clf_cbf_qp2(const char* entry, const T* a, const T* b, const T* lo, const T* hi, T relax_weight, T* u, T* relax,
                       int* active, int* status, int Bt, int K, void* stream) {
    if (Bt <= 0) return unicycle_qp_einval(entry, "Bt <= 0");
    if (K < 1 || K > 4) return unicycle_qp_einval(entry, "K must be 1..4 (the relaxed row and up to three hard rows)");
    if (!a || !b) return unicycle_qp_einval(entry, "null a or b");
    if (const char* why = unicycle_qp_box<T>(lo, hi, relax_weight)) return unicycle_qp_einval(entry, why);
    const dim3 grid((Bt + 63) / 64), block(64);
    hipStream_t s = (hipStream_t)stream;
#define BCBF_UQP_QP2(KOB)                                                                                              \
    hipLaunchKernelGGL((clf_cbf_qp2_kernel<T, KOB>), grid, block, 0, s, a, b, lo[0], lo[1], hi[0], hi[1], relax_weight, u, \
                       relax, active, status, Bt)
    switch (K - 1) {
        case 0: BCBF_UQP_QP2(0); break;
        case 1: BCBF_UQP_QP2(1); break;
        case 2: BCBF_UQP_QP2(2); break;
        default: BCBF_UQP_QP2(3); break;
    }
#undef BCBF_UQP_QP2
    return check_launch(entry);
}

template <typename T>
static int unicycle_clf_cbf_control(const char* entry, const T* x, const T* plan, const T* dot_plan, const T* Kp, int clf_kind,
                                    T clf_gamma, T relax_weight, const T* lo, const T* hi, const T* L_ctrl, int L_stride,
                                    const T* centers, const T* radii, int obs_stride, const T* tw, const T* gammas, T* a, T* b,
                                    T* values, T* u, T* relax, int* active, int* status, int Bt, int Kob, void* stream) {
    if (Bt <= 0) return unicycle_qp_einval(entry, "Bt <= 0");
    if (!x || !plan || !dot_plan) return unicycle_qp_einval(entry, "null x, plan or dot_plan");
    UnicycleQpTask<T> p;
    if (const char* why = unicycle_qp_task<T>(Kp, clf_kind, clf_gamma, relax_weight, lo, hi, L_ctrl, L_stride, centers, radii,
                                              obs_stride, tw, gammas, Kob, p))
        return unicycle_qp_einval(entry, why);
    const dim3 grid((Bt + 63) / 64), block(64);
    hipStream_t s = (hipStream_t)stream;
#define BCBF_UQP_CTRL(KOB, POLAR)                                                                                       \
    hipLaunchKernelGGL((unicycle_clf_cbf_control_kernel<T, KOB, POLAR>), grid, block, 0, s, x, plan, dot_plan, p, L_ctrl, \
                       L_stride, centers, radii, obs_stride, a, b, values, u, relax, active, status, Bt)
    if (clf_kind == 1) BCBF_UQP_CTRL(0, true);
    else switch (Kob) {
        case 0: BCBF_UQP_CTRL(0, false); break;
        case 1: BCBF_UQP_CTRL(1, false); break;
        case 2: BCBF_UQP_CTRL(2, false); break;
        default: BCBF_UQP_CTRL(3, false); break;
    }
#undef BCBF_UQP_CTRL
    return check_launch(entry);
}

template <typename T>
static int unicycle_clf_cbf_rollout(const char* entry, T* x, const T* goal, const T* x0_plan, int planner_kind, int t2,
                                    int lookahead, int numStepsPlan, const T* Kp, int clf_kind, T clf_gamma, T relax_weight,
                                    const T* lo, const T* hi, const T* L_ctrl, int Lc_stride, const T* L_true, int Lt_stride,
                                    const T* centers, const T* radii, int obs_stride, const T* tw, const T* gammas, T dt,
                                    T stop_rho, T* min_h, T* cost, int* status, int* converged_at, T* traj, T* u_rec,
                                    int record_every, int t_offset, int numSteps, int Bt, int Kob, void* stream) {
    if (Bt <= 0) return unicycle_qp_einval(entry, "Bt <= 0");
    if (numSteps < 0) return unicycle_qp_einval(entry, "numSteps < 0");
    if (t_offset < 0 || (long long)t_offset + numSteps > 0x7ffffffeLL)
        return unicycle_qp_einval(entry, "t_offset < 0 or t_offset + numSteps overflows");
    if (!(dt > T(0)) || !uqp_host_finite(dt)) return unicycle_qp_einval(entry, "dt must be > 0");
    if (!(stop_rho >= T(0)) || !uqp_host_finite(stop_rho)) return unicycle_qp_einval(entry, "stop_rho must be >= 0 (0: never stop)");
    if (!x || !goal || !cost || !status) return unicycle_qp_einval(entry, "null x, goal, cost or status");
    if (Kob > 0 && !min_h) return unicycle_qp_einval(entry, "null min_h with Kob > 0");
    if (stop_rho > T(0) && !converged_at) return unicycle_qp_einval(entry, "stop_rho > 0 needs converged_at");
    if (planner_kind != 0 && planner_kind != 1) return unicycle_qp_einval(entry, "planner kind must be 0 (NoPlanner) or 1 (PiecewiseLinearPlanner)");
    if (planner_kind == 1) {
        if (!x0_plan) return unicycle_qp_einval(entry, "planner kind 1 needs x0_plan");
        if (numStepsPlan < 3 || t2 < 0 || t2 >= numStepsPlan || lookahead < 1 || lookahead > numStepsPlan)
            return unicycle_qp_einval(entry, "planner kind 1 needs numStepsPlan >= 3, 0 <= t2 < numStepsPlan, 1 <= lookahead <= numStepsPlan");
    }
    if (!L_true) return unicycle_qp_einval(entry, "null L_true");
    if (Lt_stride != 0 && Lt_stride != 1) return unicycle_qp_einval(entry, "L_true stride must be 0 (shared) or 1 (per instance)");
    if ((traj || u_rec) && record_every <= 0) return unicycle_qp_einval(entry, "recording pointers need record_every > 0");
    UnicycleQpTask<T> p;
    if (const char* why = unicycle_qp_task<T>(Kp, clf_kind, clf_gamma, relax_weight, lo, hi, L_ctrl, Lc_stride, centers, radii,
                                              obs_stride, tw, gammas, Kob, p))
        return unicycle_qp_einval(entry, why);
    UnicycleQpPlanner pk;
    pk.kind = planner_kind; pk.t2 = t2; pk.lookahead = lookahead; pk.numStepsPlan = numStepsPlan;
    const dim3 grid((Bt + 63) / 64), block(64);
    hipStream_t s = (hipStream_t)stream;
#define BCBF_UQP_ROLL(KOB, POLAR)                                                                                        \
    hipLaunchKernelGGL((unicycle_clf_cbf_rollout_kernel<T, KOB, POLAR>), grid, block, 0, s, x, goal, x0_plan, pk, p, L_ctrl, \
                       Lc_stride, L_true, Lt_stride, centers, radii, obs_stride, dt, stop_rho, min_h, cost, status,       \
                       converged_at, traj, u_rec, record_every, t_offset, numSteps, Bt)
    if (clf_kind == 1) BCBF_UQP_ROLL(0, true);
    else switch (Kob) {
        case 0: BCBF_UQP_ROLL(0, false); break;
        case 1: BCBF_UQP_ROLL(1, false); break;
        case 2: BCBF_UQP_ROLL(2, false); break;
        default: BCBF_UQP_ROLL(3, false); break;
    }
#undef BCBF_UQP_ROLL
    return check_launch(entry);
}

}  // namespace bcbf

extern "C" {
#define BCBF_UNI_QP(T, SUF)                                                                                                  \
    int bcbf_clf_cbf_qp2_##SUF(const T* a, const T* b, const T* lo, const T* hi, T relax_weight, T* u, T* relax, int* active, \
                               int* status, int Bt, int K, void* stream) {                                                   \
        return bcbf::clf_cbf_qp2<T>("bcbf_clf_cbf_qp2_" #SUF, a, b, lo, hi, relax_weight, u, relax, active, status, Bt, K,    \
                                    stream);                                                                                 \
    }                                                                                                                        \
    int bcbf_unicycle_clf_cbf_control_##SUF(const T* x, const T* plan, const T* dot_plan, const T* Kp, int clf_kind,          \
                                            T clf_gamma, T relax_weight, const T* lo, const T* hi, const T* L_ctrl,           \
                                            int L_stride, const T* centers, const T* radii, int obs_stride, const T* tw,      \
                                            const T* gammas, T* a, T* b, T* values, T* u, T* relax, int* active, int* status, \
                                            int Bt, int Kob, void* stream) {                                                 \
        return bcbf::unicycle_clf_cbf_control<T>("bcbf_unicycle_clf_cbf_control_" #SUF, x, plan, dot_plan, Kp, clf_kind,      \
                                                 clf_gamma, relax_weight, lo, hi, L_ctrl, L_stride, centers, radii,           \
                                                 obs_stride, tw, gammas, a, b, values, u, relax, active, status, Bt, Kob,     \
                                                 stream);                                                                    \
    }                                                                                                                        \
    int bcbf_unicycle_clf_cbf_rollout_##SUF(T* x, const T* goal, const T* x0_plan, int planner_kind, int t2, int lookahead,   \
                                            int numStepsPlan, const T* Kp, int clf_kind, T clf_gamma, T relax_weight,         \
                                            const T* lo, const T* hi, const T* L_ctrl, int Lc_stride, const T* L_true,        \
                                            int Lt_stride, const T* centers, const T* radii, int obs_stride, const T* tw,     \
                                            const T* gammas, T dt, T stop_rho, T* min_h, T* cost, int* status,                \
                                            int* converged_at, T* traj, T* u_rec, int record_every, int t_offset,             \
                                            int numSteps, int Bt, int Kob, void* stream) {                                   \
        return bcbf::unicycle_clf_cbf_rollout<T>("bcbf_unicycle_clf_cbf_rollout_" #SUF, x, goal, x0_plan, planner_kind, t2,   \
                                                 lookahead, numStepsPlan, Kp, clf_kind, clf_gamma, relax_weight, lo, hi,      \
                                                 L_ctrl, Lc_stride, L_true, Lt_stride, centers, radii, obs_stride, tw,        \
                                                 gammas, dt, stop_rho, min_h, cost, status, converged_at, traj, u_rec,        \
                                                 record_every, t_offset, numSteps, Bt, Kob, stream);                         \
    }
BCBF_UNI_QP(float, f32)
BCBF_UNI_QP(double, f64)
#undef BCBF_UNI_QP
}
