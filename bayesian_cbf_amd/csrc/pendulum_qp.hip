// The pendulum's CLF-CBF quadratic program on the KNOWN model (PendulumCBFCLFDirect / run_pendulum_control_cbf_clf,
// pendulum.py:530-640, 770-906, 1019-1024): per step two affine rows in the control -- the energy CLF, relaxed by a slack of
// weight w, and a radial barrier, hard -- and the program
//     minimise 1/2 (u^2 + w rho^2)   subject to   a0 u - rho <= b0,   a1 u <= b1.
// Two entries: one control evaluation for a batch of states, and the closed loop itself -- every step of a rollout inside ONE
// launch, one lane per instance.  The state is two numbers, the rows a handful of sin / cos, the program has a closed form:
// nothing of a step touches memory, so state, parameters and statistics stay in registers for the whole launch and only the
// optional recording stores.  (Every other loop of this library is driven one launch per step because its step streams a
// model; this one would spend its time on launches.)
//
// Rows.  The controller's model is (m, g, l), x = (theta, omega), d = theta - theta_c.
//   EnergyCLF:  V = l omega^2 / 2 + g (1 - cos theta);  the reference RETURNS the "abstract" values  A = grad V . g(x) =
//     omega / m  and  b = -grad V . f(x) - c V = -c V  (grad V = [g sin theta, l omega]: the two products of grad V . f cancel).
//     Its hand-written `direct = l omega` agrees with the returned omega / m only when m l = 1 -- for another model the
//     reference's own assert trips (pendulum.py:559-566); the returned value is what is built here.
//   RadialCBFRelDegree2 (cbf_kind 0):  h = cos Delta_c - cos d,  A = -sin d / (m l),
//     b = omega^2 cos d - (g/l) sin d sin theta + k0 h + k1 omega sin d                                  (pendulum.py:698-746)
//   RadialCBF (cbf_kind 1, rel-degree 1):  h = (cos Delta_c - cos d)(omega^2 + 1),  grad h = [sin d (omega^2 + 1),
//     2 omega (cos Delta_c - cos d)],  A = -grad h . g(x) = -2 omega (cos Delta_c - cos d) / (m l),  b = grad h . f(x) + gamma h
//                                                                                                       (pendulum.py:582-637)
// QP.  control_QP_cbf_clf with constraint_margin_weights = [w] (pendulum.py:800-864); the reference hands it to cvxopt, an
// interior-point method.  The objective is strictly convex, so the optimum is unique and is what is computed here, in closed
// form, by walking the four active sets (pendulum_qp_solve below); parity with cvxopt's iterates is not claimed.
#include "bcbf_common.h"
#include "pendulum_plant.h"      // pendulum_euler
#include <stdio.h>
#include <limits>

namespace bcbf {

template <typename T>
struct PendulumQpTask {
    T clf_c, k0, k1, theta_c, delta_c, cbf_gamma, slack_weight;
    int cbf_kind;
};

template <typename T>
struct PendulumQpRows {
    T a0, b0, a1, b1;     // CLF row (relaxed), CBF row (hard)
    T V, h;
};

// The two rows at x = (th, om) on the controller's model (m, g, l)
template <typename T>
__device__ inline PendulumQpRows<T> pendulum_qp_rows(T th, T om, T m, T g, T l, const PendulumQpTask<T>& p) {
    PendulumQpRows<T> r;
    const T sth = sin(th), cth = cos(th);
    r.V = l * om * om / T(2) + g * (T(1) - cth);
    r.a0 = om / m;
    r.b0 = -p.clf_c * r.V;
    const T d = th - p.theta_c;
    const T sd = sin(d), cd = cos(d);
    const T gap = cos(p.delta_c) - cd;
    if (p.cbf_kind == 0) {
        r.h = gap;
        r.a1 = -sd / (m * l);
        r.b1 = om * om * cd - (g / l) * sd * sth + p.k0 * r.h + p.k1 * om * sd;
    } else {
        const T w1 = om * om + T(1);
        const T gh0 = sd * w1, gh1 = T(2) * om * gap;
        r.h = gap * w1;
        r.a1 = -gh1 / (m * l);
        r.b1 = gh0 * om + gh1 * (-(g / l) * sth) + p.cbf_gamma * r.h;
    }
    return r;
}

// minimise 1/2 (u^2 + w rho^2)  s.t.  a0 u - rho <= b0 (multiplier l0),  a1 u <= b1 (multiplier l1).
// KKT: u + l0 a0 + l1 a1 = 0, w rho = l0.  The four active sets, each with its primal-feasibility and sign conditions:
//   {}     u = 0, rho = 0                                      needs b0 >= 0, b1 >= 0
//   {0}    l0 = -b0 / (a0^2 + 1/w), u = -l0 a0, rho = l0 / w   needs b0 < 0 (l0 > 0), a1 u <= b1
//   {1}    u = b1 / a1, rho = 0                                needs a0 u <= b0, l1 = -u / a1 >= 0
//   {0,1}  u = b1 / a1, rho = a0 u - b0 > 0                    needs l1 = -(u + w rho a0) / a1 >= 0
// Eliminating rho = max(0, a0 u - b0) leaves a convex function of u alone on the half line a1 u <= b1, so the sets are walked in
// an order that needs no multiplier test: the minimiser without row 1 ({} when b0 >= 0, else {0}) is the answer when it
// satisfies row 1; otherwise row 1 is active, u = b1 / a1, and row 0 is active there exactly when a0 u > b0.  (The sign
// conditions of {1} and {0,1} then hold by convexity.)  Row 1 cannot be met only when a1 == 0 and b1 < 0: status 1, nothing
// divided, u and rho left alone.  A non-finite row or result is reported the same way, so that no NaN is ever acted upon.
template <typename T>
__device__ inline int pendulum_qp_solve(T a0, T b0, T a1, T b1, T w, T& u, T& rho) {
    T uu = T(0);
    if (!(b0 >= T(0))) uu = a0 * b0 / (a0 * a0 + T(1) / w);       // {0}: -l0 a0
    if (!(a1 * uu <= b1)) {
        if (!(a1 != T(0))) return 1;                               // 0 <= b1 fails: infeasible
        uu = b1 / a1;                                              // {1} or {0,1}
    }
    const T s = a0 * uu - b0;
    const T rr = s > T(0) ? s : T(0);
    if (!(fabs(uu) <= std::numeric_limits<T>::max()) || !(fabs(s) <= std::numeric_limits<T>::max())) return 1;
    u = uu;
    rho = rr;
    return 0;
}

template <typename T>
__device__ inline void pendulum_qp_load(const T* __restrict__ params, int stride, int b, T& m, T& g, T& l) {
    const T* q = params + (size_t)b * stride;
    m = q[0]; g = q[1]; l = q[2];
}

template <typename T>
__global__ void __launch_bounds__(64)
pendulum_clf_cbf_control_kernel(const T* __restrict__ x, const T* __restrict__ ctrl_params, int ctrl_stride,
                                PendulumQpTask<T> p, T* __restrict__ A, T* __restrict__ bvec, T* __restrict__ values,
                                T* __restrict__ u, T* __restrict__ rho, int* __restrict__ status, int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    T m, g, l;
    pendulum_qp_load(ctrl_params, ctrl_stride, b, m, g, l);
    const PendulumQpRows<T> r = pendulum_qp_rows<T>(x[(size_t)b * 2], x[(size_t)b * 2 + 1], m, g, l, p);
    if (A) { A[(size_t)b * 2] = r.a0; A[(size_t)b * 2 + 1] = r.a1; }
    if (bvec) { bvec[(size_t)b * 2] = r.b0; bvec[(size_t)b * 2 + 1] = r.b1; }
    if (values) { values[(size_t)b * 2] = r.V; values[(size_t)b * 2 + 1] = r.h; }
    T uu = T(0), rr = T(0);
    const int st = pendulum_qp_solve<T>(r.a0, r.b0, r.a1, r.b1, p.slack_weight, uu, rr);
    if (status) status[b] = st;
    if (st == 0) {
        if (u) u[b] = uu;
        if (rho) rho[b] = rr;
    }
}

template <typename T> struct Pair;
template <> struct Pair<float> { using type = float2; };
template <> struct Pair<double> { using type = double2; };

// The closed loop, numSteps steps in one launch.  Per step, in sampling_pendulum's order (pendulum.py:199-226): rows at x_t,
// the program, min_h and damage of x_t, the Euler step on the PLANT's parameters, the theta wrap.  An instance whose program cannot
// be solved records the 1-based global step (t_offset + t + 1) in status and freezes: state, min_h and damage keep the values
// they had BEFORE that step (the reference's controller raises there, ahead of its damage bookkeeping of the step).  Global
// steps that are multiples of record_every are recorded, the launch's first at row 0: (x_t, u_t) before the step, one
// 16-byte (fp64) store per lane, contiguous across the wave; a frozen instance records its frozen state and u = 0.
template <typename T>
__global__ void __launch_bounds__(64)
pendulum_clf_cbf_rollout_kernel(T* __restrict__ x, const T* __restrict__ ctrl_params, int ctrl_stride,
                                const T* __restrict__ true_params, int true_stride, PendulumQpTask<T> p, T dt,
                                T* __restrict__ min_h, int* __restrict__ damage, int* __restrict__ status,
                                T* __restrict__ traj, T* __restrict__ u_rec, int record_every, int t_offset, int numSteps,
                                int Bt) {
    using P2 = typename Pair<T>::type;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    T m, g, l, pm, pg, pl;
    pendulum_qp_load(ctrl_params, ctrl_stride, b, m, g, l);
    pendulum_qp_load(true_params, true_stride, b, pm, pg, pl);
    const P2 x0 = reinterpret_cast<const P2*>(x)[b];
    T th = x0.x, om = x0.y;
    T mh = min_h[b];
    int dmg = damage[b], st = status[b];
    const T quarter_pi = T(M_PI) / T(4);
    const bool rec = record_every > 0 && (traj || u_rec);
    int until = rec ? (record_every - t_offset % record_every) % record_every : -1;   // steps until the next recorded one
    size_t row = 0;
    for (int t = 0; t < numSteps; ++t) {
        T uu = T(0), rr = T(0);
        if (st == 0) {
            const PendulumQpRows<T> r = pendulum_qp_rows<T>(th, om, m, g, l, p);
            if (pendulum_qp_solve<T>(r.a0, r.b0, r.a1, r.b1, p.slack_weight, uu, rr)) {
                st = t_offset + t + 1;
                uu = T(0);
            } else {
                T hv = r.h;
                if (!(hv == hv)) hv = -INFINITY;                  // a non-finite h never passes for "safe"
                mh = hv < mh ? hv : mh;
                dmg += (T(0) < th && th < quarter_pi) ? 1 : 0;
            }
        }
        if (until == 0) {
            if (traj) {
                P2 v;
                v.x = th; v.y = om;
                reinterpret_cast<P2*>(traj)[row * Bt + b] = v;
            }
            if (u_rec) u_rec[row * Bt + b] = uu;
            ++row;
            until = record_every;
        }
        --until;
        if (st == 0) pendulum_euler<T>(th, om, uu, pm, pg, pl, dt);
    }
    P2 xo;
    xo.x = th; xo.y = om;
    reinterpret_cast<P2*>(x)[b] = xo;
    min_h[b] = mh;
    damage[b] = dmg;
    status[b] = st;
}

static int pendulum_qp_einval(const char* entry, const char* why) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", entry, why);
    set_error_message(msg);
    return BCBF_EINVAL;
}

template <typename T>
static const char* pendulum_qp_task(T clf_c, const T* k_alpha, T theta_c, T delta_c, T cbf_gamma, int cbf_kind, T slack_weight,
                                    int ctrl_stride, PendulumQpTask<T>& p) {
    if (!k_alpha) return "null k_alpha";
    if (cbf_kind != 0 && cbf_kind != 1) return "cbf_kind must be 0 (RadialCBFRelDegree2) or 1 (RadialCBF)";
    if (!(slack_weight > T(0))) return "slack_weight must be > 0";
    if (ctrl_stride != 0 && ctrl_stride != 3) return "ctrl_stride must be 0 (one shared row) or 3 (per instance)";
    p.clf_c = clf_c; p.k0 = k_alpha[0]; p.k1 = k_alpha[1];
    p.theta_c = theta_c; p.delta_c = delta_c; p.cbf_gamma = cbf_gamma; p.slack_weight = slack_weight;
    p.cbf_kind = cbf_kind;
    return nullptr;
}

template <typename T>
static int pendulum_clf_cbf_control(const char* entry, const T* x, const T* ctrl_params, int ctrl_stride, T clf_c,
                                    const T* k_alpha, T theta_c, T delta_c, T cbf_gamma, int cbf_kind, T slack_weight, T* A,
                                    T* b, T* values, T* u, T* rho, int* status, int Bt, void* stream) {
    if (Bt <= 0) return pendulum_qp_einval(entry, "Bt <= 0");
    if (!x || !ctrl_params) return pendulum_qp_einval(entry, "null x or ctrl_params");
    PendulumQpTask<T> p;
    if (const char* why = pendulum_qp_task<T>(clf_c, k_alpha, theta_c, delta_c, cbf_gamma, cbf_kind, slack_weight, ctrl_stride, p))
        return pendulum_qp_einval(entry, why);
    hipLaunchKernelGGL((pendulum_clf_cbf_control_kernel<T>), dim3((Bt + 63) / 64), dim3(64), 0, (hipStream_t)stream, x,
                       ctrl_params, ctrl_stride, p, A, b, values, u, rho, status, Bt);
    return check_launch(entry);
}

template <typename T>
static int pendulum_clf_cbf_rollout(const char* entry, T* x, const T* ctrl_params, int ctrl_stride, const T* true_params,
                                    int true_stride, T clf_c, const T* k_alpha, T theta_c, T delta_c, T cbf_gamma,
                                    int cbf_kind, T slack_weight, T dt, T* min_h, int* damage, int* status, T* traj, T* u_rec,
                                    int record_every, int t_offset, int numSteps, int Bt, void* stream) {
    if (Bt <= 0) return pendulum_qp_einval(entry, "Bt <= 0");
    if (numSteps < 0) return pendulum_qp_einval(entry, "numSteps < 0");
    if (t_offset < 0 || (long long)t_offset + numSteps > 0x7ffffffeLL) return pendulum_qp_einval(entry, "t_offset < 0 or t_offset + numSteps overflows");
    if (!(dt > T(0))) return pendulum_qp_einval(entry, "dt must be > 0");
    if (!x || !ctrl_params || !true_params || !min_h || !damage || !status)
        return pendulum_qp_einval(entry, "null x, ctrl_params, true_params, min_h, damage or status");
    if (true_stride != 0 && true_stride != 3) return pendulum_qp_einval(entry, "true_stride must be 0 (one shared row) or 3 (per instance)");
    if ((traj || u_rec) && record_every <= 0) return pendulum_qp_einval(entry, "recording pointers need record_every > 0");
    PendulumQpTask<T> p;
    if (const char* why = pendulum_qp_task<T>(clf_c, k_alpha, theta_c, delta_c, cbf_gamma, cbf_kind, slack_weight, ctrl_stride, p))
        return pendulum_qp_einval(entry, why);
    hipLaunchKernelGGL((pendulum_clf_cbf_rollout_kernel<T>), dim3((Bt + 63) / 64), dim3(64), 0, (hipStream_t)stream, x,
                       ctrl_params, ctrl_stride, true_params, true_stride, p, dt, min_h, damage, status, traj, u_rec,
                       record_every, t_offset, numSteps, Bt);
    return check_launch(entry);
}

}  // namespace bcbf

extern "C" {
#define BCBF_PEND_QP(T, SUF)                                                                                                \
    int bcbf_pendulum_clf_cbf_control_##SUF(const T* x, const T* ctrl_params, int ctrl_stride, T clf_c, const T* k_alpha,    \
                                            T theta_c, T delta_c, T cbf_gamma, int cbf_kind, T slack_weight, T* A, T* b,     \
                                            T* values, T* u, T* rho, int* status, int Bt, void* stream) {                   \
        return bcbf::pendulum_clf_cbf_control<T>("bcbf_pendulum_clf_cbf_control_" #SUF, x, ctrl_params, ctrl_stride, clf_c,  \
                                                 k_alpha, theta_c, delta_c, cbf_gamma, cbf_kind, slack_weight, A, b, values, \
                                                 u, rho, status, Bt, stream);                                               \
    }                                                                                                                       \
    int bcbf_pendulum_clf_cbf_rollout_##SUF(T* x, const T* ctrl_params, int ctrl_stride, const T* true_params,              \
                                            int true_stride, T clf_c, const T* k_alpha, T theta_c, T delta_c, T cbf_gamma,   \
                                            int cbf_kind, T slack_weight, T dt, T* min_h, int* damage, int* status, T* traj, \
                                            T* u_rec, int record_every, int t_offset, int numSteps, int Bt, void* stream) { \
        return bcbf::pendulum_clf_cbf_rollout<T>("bcbf_pendulum_clf_cbf_rollout_" #SUF, x, ctrl_params, ctrl_stride,         \
                                                 true_params, true_stride, clf_c, k_alpha, theta_c, delta_c, cbf_gamma,      \
                                                 cbf_kind, slack_weight, dt, min_h, damage, status, traj, u_rec,             \
                                                 record_every, t_offset, numSteps, Bt, stream);                             \
    }
BCBF_PEND_QP(float, f32)
BCBF_PEND_QP(double, f64)
#undef BCBF_PEND_QP
}
