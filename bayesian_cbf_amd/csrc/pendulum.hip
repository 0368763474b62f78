// The pendulum's rel-degree-2 safety loop (SOCPController with cbfs = [RadialCBFRelDegree2], controllers.py:569-591;
// pendulum.py:643-746), batched: one host call per control step that sequences the existing launchers
//   jets -> task rows -> cbc2 terms -> pack -> controller cones -> coneqp -> plant step
// on the caller's stream, as control_step.hip does for the unicycle.  The two kernels of this file are elementwise
// (one lane per instance); the jets launch dominates the step.
//
// Task kernel: the deterministic mean model (a pendulum, or none = ZeroDynamicsModel) is added to the jets' posterior
// factors exactly as cbc2.reldeg2_quadratic_terms does on the host (Mk += [fhat | ghat], Mj[:, :, (1+i) C] += J[:, :, i]);
// the radial barrier h = cos(delta) - cos(theta - theta_c) with its gradient and Hessian; the nominal control of
// controllers.GreedyController (controllers.py:174-213) on the shifted posterior mean; the objective q = e_0, P = 0.
// Plant kernel: u = y[2:] where the program was solved, u_ref elsewhere (SOCPController.control on a batch); the safety
// bookkeeping (min_h over h(x_t) before the step, failed programs); x += (f + g u) dt on the true pendulum with the theta
// wrap of PendulumDynamicsModel.step.
// The observing entry (bcbf_pendulum_control_step_observe_f64) instantiates both kernels with Learn = true: the task
// kernel can write the GP prior of a regressor with no data and wraps the greedy u_ref in the epsilon-greedy explorer
// (EpsilonGreedyController, controllers.py:269-285); the plant kernel writes the step's observation row
// (MeanAdjustedModel.train, controllers.py:320-378).  The Learn = false instantiations are the plain entry's.
// The sampled entry (bcbf_pendulum_control_step_sampled_f64) runs the observing entry's launches with a third plant kernel: the
// jet columns the rel-degree-2 condition reads are drawn from the model's own posterior, the state advances on the draw and the
// condition is evaluated on it (pendulum_posterior_plant.h) -- the instrument that measures what risk the loop actually holds.
#include "bcbf_common.h"
#include "pendulum_plant.h"      // pendulum_euler, pendulum_advance
#include "pendulum_posterior_plant.h"      // the sampled plant kernel's draw
#include "lqr.h"                 // lqr_nominal_step_f64: the LQR nominal control (nominal = 1)

namespace bcbf {

template <typename T>
struct PendulumParams {
    int has_gp, has_mean, has_uref;
    T mean_mass, mean_gravity, mean_length;     // deterministic mean model (has_mean)
    T theta_c, delta_c;                         // RadialCBFRelDegree2: cbf_col_theta, cbf_col_delta
    T xg[2], Qg[4], R, dt;                      // GreedyController: x_goal, Q (x_quad_goal_cost), R (u_quad_cost), dt
};

// What the observing entry adds (read only by the Learn = true instantiations)
template <typename T>
struct PendulumLearn {
    int prior;                                  // no GP: write the prior of a regressor with no data (needs M0, s2, Bm)
    const T *M0, *s2, *Bm;                      // M0[Bt,C,n], s2[Bt], Bm[Bt,C,C]
    const T* explore;                           // [Bt,2] uniform draws (coin, action) or NULL
    T eps;                                      // exploration probability of this step
    int clip;                                   // clip u_ref to [lo, hi]
    T lo, hi;
    T *obs_x, *obs_uh, *obs_y;                  // observation row at b * obs_ld (all three or none)
    int obs_ld;
    int has_mean;                               // the mean model the targets subtract (as PendulumParams)
    T mean_mass, mean_gravity, mean_length;
};

template <typename T, bool Learn>
__global__ void __launch_bounds__(256)
pendulum_task_kernel(const T* __restrict__ x, T* __restrict__ Mk, T* __restrict__ Bk, T* __restrict__ G,
                     T* __restrict__ Mj, T* __restrict__ h, T* __restrict__ gh, T* __restrict__ Hh,
                     const T* __restrict__ u_ref_in, T* __restrict__ u_ref, double* __restrict__ P,
                     double* __restrict__ q, PendulumParams<T> p, PendulumLearn<T> L, int Bt) {
    constexpr int n = 2, C = 2, CT = C * (1 + n);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    const T th = x[b * n], om = x[b * n + 1];
    T* mk = Mk + (size_t)b * n * C;
    T* mj = Mj + (size_t)b * n * CT;
    if (Learn && !p.has_gp && L.prior) {
        // a regressor with no data (cbc2.posterior_for, control_affine_model.py:495-506): Mk = M0', Bk = s2 Bm, G = Mj = 0
        const T* m0 = L.M0 + (size_t)b * C * n;
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < C; ++c) mk[i * C + c] = m0[c * n + i];
        for (int i = 0; i < n * CT; ++i) mj[i] = T(0);
        for (int i = 0; i < C * C; ++i) Bk[(size_t)b * C * C + i] = L.s2[b] * L.Bm[(size_t)b * C * C + i];
        for (int i = 0; i < CT * CT; ++i) G[(size_t)b * CT * CT + i] = T(0);
    } else if (!p.has_gp) {       // no learned model: the mean model is the whole model, every variance term is 0
        for (int i = 0; i < n * C; ++i) mk[i] = T(0);
        for (int i = 0; i < n * CT; ++i) mj[i] = T(0);
        for (int i = 0; i < C * C; ++i) Bk[(size_t)b * C * C + i] = T(0);
        for (int i = 0; i < CT * CT; ++i) G[(size_t)b * CT * CT + i] = T(0);
    }
    if (p.has_mean) {
        const T c = -(p.mean_gravity / p.mean_length);
        mk[0 * C + 0] += om;                                 // fhat = [omega, -(g/l) sin theta]
        mk[1 * C + 0] += c * sin(th);
        mk[1 * C + 1] += T(1) / (p.mean_mass * p.mean_length);      // ghat = [0, 1/(m l)]'
        // J[j][i] = d fhat_j / d x_i = [[0, 1], [-(g/l) cos theta, 0]] into column (1+i) C (its zeros add nothing)
        mj[0 * CT + 2 * C] += T(1);
        mj[1 * CT + 1 * C] += c * cos(th);
    }
    const T d = th - p.theta_c;
    h[b] = cos(p.delta_c) - cos(d);
    gh[b * n] = sin(d);
    gh[b * n + 1] = T(0);
    Hh[b * 4 + 0] = cos(d);
    Hh[b * 4 + 1] = Hh[b * 4 + 2] = Hh[b * 4 + 3] = T(0);
    T u0;
    if (p.has_uref) {
        u0 = u_ref_in[b];
    } else {                     // u = (lam R dt + (1-lam) G'P G)^-1 (1-lam) G'P (x_g - x - f dt),  G = g dt, lam = 1/2
        const T lam = T(0.5);
        const T f0 = p.dt * mk[0], f1 = p.dt * mk[C];
        const T g0 = p.dt * mk[1], g1 = p.dt * mk[C + 1];
        const T PG0 = g0 * p.Qg[0] + g1 * p.Qg[2], PG1 = g0 * p.Qg[1] + g1 * p.Qg[3];      // (G'P)_j
        const T Q = lam * (p.R * p.dt) + (T(1) - lam) * (PG0 * g0 + PG1 * g1);
        const T r0 = p.xg[0] - th - f0, r1 = p.xg[1] - om - f1;
        const T cc = (T(1) - lam) * (g0 * (p.Qg[0] * r0 + p.Qg[1] * r1) + g1 * (p.Qg[2] * r0 + p.Qg[3] * r1));
        u0 = cc / Q;
    }
    if constexpr (Learn) {
        // EpsilonGreedyController: the uniform action lo + a (hi - lo) when the coin falls below eps, then
        // clip = max(min(u, hi), lo) (misc.py:287-288; a NaN stays NaN, as torch.min / torch.max keep it)
        if (L.explore && L.explore[(size_t)b * 2] < L.eps) u0 = L.lo + L.explore[(size_t)b * 2 + 1] * (L.hi - L.lo);
        if (L.clip) {
            u0 = u0 > L.hi ? L.hi : u0;
            u0 = u0 < L.lo ? L.lo : u0;
        }
    }
    u_ref[b] = u0;
    for (int i = 0; i < 9; ++i) P[(size_t)b * 9 + i] = 0.0;                  // min y_1: P = 0, q = e_0 (controllers.py:575)
    q[(size_t)b * 3] = 1.0;
    q[(size_t)b * 3 + 1] = q[(size_t)b * 3 + 2] = 0.0;
}

// bcbf_cbc2_terms writes (mean_A, mean_b, Q, p, r, mean(u0), var(u0)); bcbf_controller_cones reads the first five
template <typename T>
__global__ void __launch_bounds__(256) pendulum_pack_terms_kernel(const T* __restrict__ t2, T* __restrict__ t, int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    for (int i = 0; i < 5; ++i) t[(size_t)b * 5 + i] = t2[(size_t)b * 7 + i];
}

// What both plant kernels do first: status, the applied control u = y[2] where the program was solved and u_ref elsewhere, and the
// safety bookkeeping on h(x_t)
template <typename T>
__device__ inline T pendulum_choose_control(int b, const double* __restrict__ y, const int* __restrict__ sstatus,
                                            const int* __restrict__ cstatus, const int* __restrict__ tstatus,
                                            const T* __restrict__ u_ref, const T* __restrict__ h, T* __restrict__ u,
                                            int* __restrict__ status, T* __restrict__ min_h, int* __restrict__ fails, int& st) {
    st = tstatus[b] == 1 ? BCBF_PENDULUM_BADHESSIAN : cstatus[b] != 0 ? BCBF_SOCP_BADCONE : sstatus[b];
    status[b] = st;
    const T ub = st == 0 ? (T)y[(size_t)b * 3 + 2] : u_ref[b];
    u[b] = ub;
    if (min_h) {
        T hv = h[b];
        if (!(hv == hv)) hv = -INFINITY;          // a non-finite h never passes for "safe"
        min_h[b] = hv < min_h[b] ? hv : min_h[b];
        fails[b] += st != 0;
    }
    return ub;
}

// The observation row of pendulum_plant_kernel<T, true>, for the sampled plant kernel: x still holds x_t, (th, om) = x_{t+1}.
// (That kernel keeps its own copy of these lines: calling this function from it swaps two of its instructions, and the kernels of
// the two earlier entries are held instruction-identical.)
template <typename T>
__device__ inline void pendulum_observation_row(const PendulumLearn<T>& L, int b, const T* __restrict__ x, T ub, T th, T om, T dt) {
    if (L.obs_x) {
        const T t0 = x[b * 2], w0 = x[b * 2 + 1];
        T m0 = T(0), m1 = T(0);
        if (L.has_mean) {
            m0 = w0 + T(0) * ub;
            m1 = -(L.mean_gravity / L.mean_length) * sin(t0) + T(1) / (L.mean_mass * L.mean_length) * ub;
        }
        const size_t r = (size_t)b * L.obs_ld * 2;
        L.obs_x[r] = t0;
        L.obs_x[r + 1] = w0;
        L.obs_uh[r] = T(1);
        L.obs_uh[r + 1] = ub;
        L.obs_y[r] = (th - t0) / dt - m0;
        L.obs_y[r + 1] = (om - w0) / dt - m1;
    }
}

template <typename T, bool Learn>
__global__ void __launch_bounds__(256)
pendulum_plant_kernel(T* __restrict__ x, const double* __restrict__ y, const int* __restrict__ sstatus,
                      const int* __restrict__ cstatus, const int* __restrict__ tstatus, const T* __restrict__ u_ref,
                      const T* __restrict__ h, T* __restrict__ u, int* __restrict__ status, T* __restrict__ min_h,
                      int* __restrict__ fails, T mass, T gravity, T length, T dt, PendulumLearn<T> L, int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    int st;
    const T ub = pendulum_choose_control<T>(b, y, sstatus, cstatus, tstatus, u_ref, h, u, status, min_h, fails, st);
    T th = x[b * 2], om = x[b * 2 + 1];
    pendulum_euler<T>(th, om, ub, mass, gravity, length, dt);
    if constexpr (Learn) {
        // the buffered row (MeanAdjustedModel._train): X = x_t, UH = (1, u_t), Y = (x_{t+1} - x_t) / dt - (f + g u)(x_t) of
        // the mean model, from the STORED states -- theta_{t+1} is wrapped, so a step across +-pi gives a target ~ 2 pi / dt
        if (L.obs_x) {
            const T t0 = x[b * 2], w0 = x[b * 2 + 1];
            T m0 = T(0), m1 = T(0);
            if (L.has_mean) {
                m0 = w0 + T(0) * ub;
                m1 = -(L.mean_gravity / L.mean_length) * sin(t0) + T(1) / (L.mean_mass * L.mean_length) * ub;
            }
            const size_t r = (size_t)b * L.obs_ld * 2;
            L.obs_x[r] = t0;
            L.obs_x[r + 1] = w0;
            L.obs_uh[r] = T(1);
            L.obs_uh[r + 1] = ub;
            L.obs_y[r] = (th - t0) / dt - m0;
            L.obs_y[r + 1] = (om - w0) / dt - m1;
        }
    }
    x[b * 2] = th;
    x[b * 2 + 1] = om;
}

// What the sampled entry adds: the caller's standard normals, the outputs on the draw, and what Sigma4 is made of
template <typename T>
struct PendulumDraw {
    const T* z;                                 // [Bt,2,4]
    T *xdot_s, *cbc_s;                          // [Bt,2] each, or NULL
    int *relaxed, *viol_relaxed;                // [Bt] counters (both or neither)
    T rho_tol;
    int gp;                                     // 0: no learned model and no prior (Sigma4 = 0)
    int kernel_kind;
    const T *Mk, *Bk, *G, *Mj, *A, *Bm, *ell, *s2, *gh, *Hh, *kalpha;
};

// The plant kernel of the sampled entry: the jet columns CBC2 reads are DRAWN from the model's posterior at x_t
// (pendulum_posterior_plant.h), the state advances on the draw -- true_* plays no part -- and the condition is evaluated on the
// same draw at the applied control.  Bookkeeping and observation rows as pendulum_plant_kernel<T, true>.
template <typename T>
__global__ void __launch_bounds__(256)
pendulum_sampled_plant_kernel(T* __restrict__ x, const double* __restrict__ y, const int* __restrict__ sstatus,
                              const int* __restrict__ cstatus, const int* __restrict__ tstatus, const T* __restrict__ u_ref,
                              const T* __restrict__ h, T* __restrict__ u, int* __restrict__ status, T* __restrict__ min_h,
                              int* __restrict__ fails, T dt, PendulumLearn<T> L, PendulumDraw<T> D, int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    int st;
    const T ub = pendulum_choose_control<T>(b, y, sstatus, cstatus, tstatus, u_ref, h, u, status, min_h, fails, st);
    double S4[4][4], LS[4][4], Ad[2][2], LA[2][2], mean[2][4], Z[2][4], S[2][4], gh[2], Hh[2][2];
    pendulum_jet_covariance<T>(D.gp, D.Bk + (size_t)b * 4, D.G + (size_t)b * 36, D.s2[b], D.Bm[(size_t)b * 4], D.ell + (size_t)b * 2,
                               kernel_kxx(D.kernel_kind), S4);
    psd_chol<4>(S4, LS);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            Ad[i][j] = (double)D.A[(size_t)b * 4 + i * 2 + j];
            Hh[i][j] = (double)D.Hh[(size_t)b * 4 + i * 2 + j];
        }
        gh[i] = (double)D.gh[(size_t)b * 2 + i];
        mean[i][0] = (double)D.Mk[(size_t)b * 4 + i * 2];
        mean[i][1] = (double)D.Mk[(size_t)b * 4 + i * 2 + 1];
        mean[i][2] = (double)D.Mj[(size_t)b * 12 + i * 6 + 2];
        mean[i][3] = (double)D.Mj[(size_t)b * 12 + i * 6 + 4];
#pragma unroll
        for (int k = 0; k < 4; ++k) Z[i][k] = (double)D.z[(size_t)b * 8 + i * 4 + k];
    }
    psd_chol<2>(Ad, LA);
    pendulum_jet_draw(mean, LA, LS, Z, S);
    double xd[2], lfh, cbc2;
    pendulum_cbc2_on(S, (double)ub, (double)h[b], gh, Hh, (double)D.kalpha[0], (double)D.kalpha[1], xd, lfh, cbc2);
    if (D.xdot_s) {
        D.xdot_s[(size_t)b * 2] = (T)xd[0];
        D.xdot_s[(size_t)b * 2 + 1] = (T)xd[1];
    }
    if (D.cbc_s) {
        D.cbc_s[(size_t)b * 2] = (T)lfh;
        D.cbc_s[(size_t)b * 2 + 1] = (T)cbc2;
    }
    if (D.relaxed) {      // the safety cone is soft: a step that bought slack (rho = y[1]) was never promised the risk
        const int rel = st == 0 && (T)y[(size_t)b * 3 + 1] > D.rho_tol;
        D.relaxed[b] += rel;
        D.viol_relaxed[b] += rel && !(cbc2 >= 0.0);
    }
    T th = x[b * 2], om = x[b * 2 + 1];
    pendulum_advance<T>(th, om, (T)xd[0], (T)xd[1], dt);
    pendulum_observation_row<T>(L, b, x, ub, th, om, dt);
    x[b * 2] = th;
    x[b * 2 + 1] = om;
}

template <typename T>
__global__ void __launch_bounds__(256)
pendulum_plant_step_kernel(T* __restrict__ x, const T* __restrict__ u, T mass, T gravity, T length, T dt, int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    T th = x[b * 2], om = x[b * 2 + 1];
    pendulum_euler<T>(th, om, u[b], mass, gravity, length, dt);
    x[b * 2] = th;
    x[b * 2 + 1] = om;
}

// What the nominal entry adds: which nominal controller, and the LQR's horizon (bcbf_lqr_nominal_f64's numSteps, t, t_dev, status)
struct PendulumNominal {
    int nominal, numSteps, t;
    const int* t_dev;
    int* lstatus;
};

static int pendulum_einval(const char* why) {
    set_error_message(why);
    return BCBF_EINVAL;
}

// The 56 arguments every control-step entry takes, then (Bt, n, m) and the stream triple: in ABI order (include/bcbf.h)
struct PendulumStepArgs {
    const double *Lop, *Vw, *X, *UHB, *ell, *s2, *Bm, *M0, *A;
    int N, shared, kernel_kind, mean_model;
    double mean_mass, mean_gravity, mean_length, theta_c, delta_c;
    const double *kalpha, *x_goal, *Q_goal;
    double R;
    const double* u_ref_in;
    double safety_factor, ctrl_reg, relax_weight;
    int hessian_mode, max_iters;
    double true_mass, true_gravity, true_length, dt;
    double *x, *Mk, *Bk, *G, *Mj, *h, *gh, *Hh, *u_ref, *terms2, *terms;
    int* tstatus;
    double *Gc, *hc;
    int* cstatus;
    double *P, *q, *y;
    int *sstatus, *iters;
    double* u;
    int* status;
    double* min_h;
    int* fails;
    int Bt, n, m;
    void *ev_start, *ev_stop, *stream;
};

// Lg: the observing entries' own arguments (pendulum_learn_args); D, Nm: NULL without the sampled / nominal group
template <bool Learn>
static int pendulum_control_step(const PendulumStepArgs& a, const PendulumLearn<double>& Lg, const PendulumDraw<double>* D = nullptr,
                                 const PendulumNominal* Nm = nullptr) {
    PendulumLearn<double> L = Lg;
    if (Learn) {      // what the Learn = true kernels read of the common arguments
        L.M0 = a.M0; L.s2 = a.s2; L.Bm = a.Bm;
        L.has_mean = a.mean_model != 0;
        L.mean_mass = a.mean_mass; L.mean_gravity = a.mean_gravity; L.mean_length = a.mean_length;
    }
    // ---- argument checks, before any HIP call
    if (a.Bt < 0) return pendulum_einval("pendulum_control_step: Bt < 0");
    if (a.n != 2 || a.m != 1) return pendulum_einval("pendulum_control_step: the pendulum has n = 2, m = 1");
    if (!a.x || !a.ell || !a.s2 || !a.Bm || !a.A || !a.kalpha || !a.x_goal || !a.Q_goal)
        return pendulum_einval("pendulum_control_step: null state / model / task buffer");
    if (!a.Mk || !a.Bk || !a.G || !a.Mj || !a.h || !a.gh || !a.Hh || !a.u_ref || !a.terms2 || !a.terms || !a.tstatus || !a.Gc ||
        !a.hc || !a.cstatus || !a.P || !a.q || !a.y || !a.sstatus || !a.u || !a.status)
        return pendulum_einval("pendulum_control_step: null workspace buffer");
    if (!a.min_h != !a.fails) return pendulum_einval("pendulum_control_step: min_h and fails go together");
    if (a.Lop && (!a.Vw || !a.X || !a.UHB || !a.M0 || a.N < 1)) return pendulum_einval("pendulum_control_step: incomplete GP");
    if (a.shared != 0 && a.shared != 1) return pendulum_einval("pendulum_control_step: shared must be 0 or 1");
    if (a.kernel_kind < 0 || a.kernel_kind >= BCBF_KINDS) return pendulum_einval("pendulum_control_step: bad kernel_kind");
    if (a.hessian_mode != 0 && a.hessian_mode != 1) return pendulum_einval("pendulum_control_step: bad hessian_mode");
    if (a.max_iters < 1) return pendulum_einval("pendulum_control_step: max_iters < 1");
    if (!(a.dt > 0.0) || !(a.R > 0.0)) return pendulum_einval("pendulum_control_step: dt and R must be > 0");
    if (a.mean_model && !(a.mean_mass * a.mean_length != 0.0)) return pendulum_einval("pendulum_control_step: mean model m l == 0");
    if (!(a.true_mass * a.true_length != 0.0)) return pendulum_einval("pendulum_control_step: true model m l == 0");
    if (!(a.safety_factor >= 0.0) || !(a.ctrl_reg > 0.0) || !(a.relax_weight > 0.0))
        return pendulum_einval("pendulum_control_step: safety factor, ctrl_reg, relax_weight");
    if (Learn) {
        if (L.prior != 0 && L.prior != 1) return pendulum_einval("pendulum_control_step_observe: prior must be 0 or 1");
        if (!a.Lop && L.prior && (!L.M0 || !L.s2 || !L.Bm))
            return pendulum_einval("pendulum_control_step_observe: the prior needs M0");
        if (!(L.eps >= 0.0 && L.eps <= 1.0)) return pendulum_einval("pendulum_control_step_observe: eps must lie in [0, 1]");
        if (L.explore && !L.clip) return pendulum_einval("pendulum_control_step_observe: explore needs ctrl_range");
        if (L.explore && a.u_ref_in) return pendulum_einval("pendulum_control_step_observe: explore wraps the greedy u_ref, not u_ref_in");
        if (L.clip && !(L.lo <= L.hi)) return pendulum_einval("pendulum_control_step_observe: ctrl_range needs lo <= hi");
        if ((L.obs_x || L.obs_uh || L.obs_y) && (!L.obs_x || !L.obs_uh || !L.obs_y))
            return pendulum_einval("pendulum_control_step_observe: obs_x, obs_uh, obs_y go together");
        if (L.obs_x && L.obs_ld < 1) return pendulum_einval("pendulum_control_step_observe: obs_ld < 1");
        if (L.has_mean && !(L.mean_mass * L.mean_length != 0.0))
            return pendulum_einval("pendulum_control_step_observe: mean model m l == 0");
    }
    if (D) {
        if (!D->z) return pendulum_einval("pendulum_control_step_sampled: null z");
        if (!D->relaxed != !D->viol_relaxed)
            return pendulum_einval("pendulum_control_step_sampled: relaxed and viol_relaxed go together");
        if (!(D->rho_tol >= 0.0)) return pendulum_einval("pendulum_control_step_sampled: rho_tol must be >= 0");
    }
    const bool lqr = Nm && Nm->nominal == 1;
    if (Nm) {
        if (Nm->nominal != 0 && Nm->nominal != 1) return pendulum_einval("pendulum_control_step_nominal: nominal must be 0 or 1");
        if (lqr && a.u_ref_in) return pendulum_einval("pendulum_control_step_nominal: the LQR nominal control excludes u_ref_in");
        if (lqr && !Nm->lstatus) return pendulum_einval("pendulum_control_step_nominal: the LQR nominal control needs lstatus");
        if (lqr && Nm->numSteps < 1) return pendulum_einval("pendulum_control_step_nominal: numSteps < 1");
        if (lqr && !Nm->t_dev && Nm->t < 0) return pendulum_einval("pendulum_control_step_nominal: t < 0 without t_dev");
    }
    if (a.Bt == 0) return BCBF_OK;
    hipStream_t st = (hipStream_t)a.stream;
    // 1. jets of the learned model at x (skipped without one: the task kernel writes the mean model alone)
    if (a.ev_start) (void)hipEventRecord((hipEvent_t)a.ev_start, st);
    int rc = BCBF_OK;
    if (a.Lop) {
        auto jets = a.kernel_kind == 0 ? bcbf_posterior_jets_f64 : a.kernel_kind == 1 ? bcbf_posterior_jets_matern52_f64
                                                                                  : bcbf_posterior_jets_rbfm52_f64;
        rc = jets(a.Lop, a.Vw, a.X, a.UHB, a.ell, a.s2, a.Bm, a.M0, a.x, a.Mk, a.Bk, a.G, a.Mj, nullptr, a.shared, a.Bt, a.N, 2, 1,
                  a.stream);
    }
    if (a.ev_stop) (void)hipEventRecord((hipEvent_t)a.ev_stop, st);
    if (rc) return rc;
    // 2. task kernel
    PendulumParams<double> p;
    p.has_gp = a.Lop != nullptr;
    p.has_mean = a.mean_model != 0;
    p.has_uref = a.u_ref_in != nullptr;
    p.mean_mass = a.mean_mass; p.mean_gravity = a.mean_gravity; p.mean_length = a.mean_length;
    p.theta_c = a.theta_c; p.delta_c = a.delta_c;
    p.xg[0] = a.x_goal[0]; p.xg[1] = a.x_goal[1];
    for (int i = 0; i < 4; ++i) p.Qg[i] = a.Q_goal[i];
    p.R = a.R; p.dt = a.dt;
    const dim3 grid((a.Bt + 255) / 256), block(256);
    hipLaunchKernelGGL((pendulum_task_kernel<double, Learn>), grid, block, 0, st, a.x, a.Mk, a.Bk, a.G, a.Mj, a.h, a.gh, a.Hh,
                       a.u_ref_in, a.u_ref, a.P, a.q, p, L, a.Bt);
    if ((rc = check_launch("pendulum_task"))) return rc;
    // 2b. LQRController in place of the task kernel's greedy u_ref, on the factors it has just shifted: bcbf_lqr_nominal_f64's
    // kernel, then the explorer's draw and the clip as the task kernel applies them
    if (lqr && (rc = lqr_nominal_step_f64(a.Mk, a.Mj, a.x, a.x_goal, a.Q_goal, a.R, a.dt, Nm->numSteps, Nm->t, Nm->t_dev, L.explore,
                                          L.eps, L.clip, L.lo, L.hi, a.u_ref, Nm->lstatus, a.Bt, a.stream)))
        return rc;
    // 3. rel-degree-2 terms (linearised at u_ref), 4. the program's rows (objective cone + safety cone of kind 1)
    if ((rc = bcbf_cbc2_terms_f64(a.Mk, a.Bk, a.G, a.Mj, a.A, a.Bm, a.ell, a.s2, a.h, a.gh, a.Hh, a.kalpha, a.u_ref, a.terms2,
                                  a.tstatus, a.Bt, 2, 1, a.hessian_mode, a.kernel_kind, a.stream)))
        return rc;
    hipLaunchKernelGGL((pendulum_pack_terms_kernel<double>), grid, block, 0, st, a.terms2, a.terms, a.Bt);
    if ((rc = check_launch("pendulum_pack_terms"))) return rc;
    const int kind = 1;
    if ((rc = bcbf_controller_cones_f64(a.terms, a.u_ref, &kind, &a.safety_factor, a.ctrl_reg, a.relax_weight, 2, 1, a.Gc, a.hc,
                                        a.cstatus, a.Bt, 1, 1, a.stream)))
        return rc;
    // 5. min y_1 over y = [y_1, rho, u] in Q^3 x Q^3
    const int qdims[2] = {3, 3};
    if ((rc = bcbf_coneqp_f64(a.P, a.q, a.Gc, a.hc, 3, 0, qdims, 2, a.y, a.sstatus, a.iters, a.Bt, a.max_iters, a.stream))) return rc;
    // 6. choose u, bookkeeping, plant step (the sampled entry: on a draw from the model's posterior at x_t)
    if (D) {
        PendulumDraw<double> d = *D;
        d.gp = a.Lop != nullptr || (Learn && L.prior);
        d.kernel_kind = a.kernel_kind;
        d.Mk = a.Mk; d.Bk = a.Bk; d.G = a.G; d.Mj = a.Mj; d.A = a.A; d.Bm = a.Bm; d.ell = a.ell; d.s2 = a.s2; d.gh = a.gh;
        d.Hh = a.Hh; d.kalpha = a.kalpha;
        hipLaunchKernelGGL((pendulum_sampled_plant_kernel<double>), grid, block, 0, st, a.x, a.y, a.sstatus, a.cstatus, a.tstatus,
                           a.u_ref, a.h, a.u, a.status, a.min_h, a.fails, a.dt, L, d, a.Bt);
        return check_launch("pendulum_sampled_plant");
    }
    hipLaunchKernelGGL((pendulum_plant_kernel<double, Learn>), grid, block, 0, st, a.x, a.y, a.sstatus, a.cstatus, a.tstatus, a.u_ref,
                       a.h, a.u, a.status, a.min_h, a.fails, a.true_mass, a.true_gravity, a.true_length, a.dt, L, a.Bt);
    return check_launch("pendulum_plant");
}

// the observing entries' own arguments as the kernels take them (pendulum_control_step adds what it reads of the common ones)
static PendulumLearn<double> pendulum_learn_args(int prior, const double* explore, double eps, const double* ctrl_range,
                                                 double* obs_x, double* obs_uh, double* obs_y, int obs_ld) {
    PendulumLearn<double> L{};
    L.prior = prior;
    L.explore = explore;
    L.eps = eps;
    L.clip = ctrl_range != nullptr;
    L.lo = ctrl_range ? ctrl_range[0] : 0.0;
    L.hi = ctrl_range ? ctrl_range[1] : 0.0;
    L.obs_x = obs_x; L.obs_uh = obs_uh; L.obs_y = obs_y; L.obs_ld = obs_ld;
    return L;
}

}  // namespace bcbf

extern "C" {
#define BCBF_PEND_PLANT(T, SUF)                                                                                       \
    int bcbf_pendulum_plant_step_##SUF(T* x, const T* u, T mass, T gravity, T length, T dt, int Bt, void* stream) {   \
        if (!x || !u || Bt < 0) return bcbf::pendulum_einval("pendulum_plant_step: null buffer or Bt < 0");          \
        if (!(mass * length != T(0)) || !(dt == dt)) return bcbf::pendulum_einval("pendulum_plant_step: m l == 0");  \
        if (Bt == 0) return BCBF_OK;                                                                                  \
        hipLaunchKernelGGL((bcbf::pendulum_plant_step_kernel<T>), dim3((Bt + 255) / 256), dim3(256), 0,               \
                           (hipStream_t)stream, x, u, mass, gravity, length, dt, Bt);                                 \
        return bcbf::check_launch("pendulum_plant_step");                                                             \
    }
BCBF_PEND_PLANT(float, f32)
BCBF_PEND_PLANT(double, f64)
#undef BCBF_PEND_PLANT

// the parameters of each argument group, in ABI order (include/bcbf.h), and the records they fill
#define BCBF_PEND_PARAMS                                                                                              \
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,     \
        const double* Bm, const double* M0, const double* A, int N, int shared, int kernel_kind, int mean_model,      \
        double mean_mass, double mean_gravity, double mean_length, double theta_c, double delta_c, const double* kalpha, \
        const double* x_goal, const double* Q_goal, double R, const double* u_ref_in, double safety_factor,           \
        double ctrl_reg, double relax_weight, int hessian_mode, int max_iters, double true_mass, double true_gravity, \
        double true_length, double dt, double* x, double* Mk, double* Bk, double* G, double* Mj, double* h, double* gh, \
        double* Hh, double* u_ref, double* terms2, double* terms, int* tstatus, double* Gc, double* hc, int* cstatus, \
        double* P, double* q, double* y, int* sstatus, int* iters, double* u, int* status, double* min_h, int* fails
#define BCBF_PEND_TAIL int Bt, int n, int m, void* ev_start, void* ev_stop, void* stream
#define BCBF_PEND_ARGS                                                                                                \
    bcbf::PendulumStepArgs {                                                                                          \
        Lop, Vw, X, UHB, ell, s2, Bm, M0, A, N, shared, kernel_kind, mean_model, mean_mass, mean_gravity, mean_length, theta_c, \
            delta_c, kalpha, x_goal, Q_goal, R, u_ref_in, safety_factor, ctrl_reg, relax_weight, hessian_mode, max_iters,  \
            true_mass, true_gravity, true_length, dt, x, Mk, Bk, G, Mj, h, gh, Hh, u_ref, terms2, terms, tstatus, Gc, hc,  \
            cstatus, P, q, y, sstatus, iters, u, status, min_h, fails, Bt, n, m, ev_start, ev_stop, stream            \
    }
#define BCBF_PEND_LEARN_PARAMS                                                                                        \
    int prior, const double* explore, double eps, const double* ctrl_range, double* obs_x, double* obs_uh, double* obs_y, int obs_ld
#define BCBF_PEND_LEARN_ARGS bcbf::pendulum_learn_args(prior, explore, eps, ctrl_range, obs_x, obs_uh, obs_y, obs_ld)
#define BCBF_PEND_DRAW_PARAMS const double* z, double* xdot_s, double* cbc_s, int* relaxed, int* viol_relaxed, double rho_tol
#define BCBF_PEND_DRAW_ARGS bcbf::PendulumDraw<double> { z, xdot_s, cbc_s, relaxed, viol_relaxed, rho_tol }

int bcbf_pendulum_control_step_f64(BCBF_PEND_PARAMS, BCBF_PEND_TAIL) {
    return bcbf::pendulum_control_step<false>(BCBF_PEND_ARGS, bcbf::PendulumLearn<double>{});
}

int bcbf_pendulum_control_step_observe_f64(BCBF_PEND_PARAMS, BCBF_PEND_LEARN_PARAMS, BCBF_PEND_TAIL) {
    return bcbf::pendulum_control_step<true>(BCBF_PEND_ARGS, BCBF_PEND_LEARN_ARGS);
}

int bcbf_pendulum_control_step_sampled_f64(BCBF_PEND_PARAMS, BCBF_PEND_LEARN_PARAMS, BCBF_PEND_DRAW_PARAMS, BCBF_PEND_TAIL) {
    const bcbf::PendulumDraw<double> D = BCBF_PEND_DRAW_ARGS;
    return bcbf::pendulum_control_step<true>(BCBF_PEND_ARGS, BCBF_PEND_LEARN_ARGS, &D);
}

// (no draws z: the observing entry's plant kernel)
int bcbf_pendulum_control_step_nominal_f64(BCBF_PEND_PARAMS, BCBF_PEND_LEARN_PARAMS, BCBF_PEND_DRAW_PARAMS, int nominal, int numSteps,
                                           int t, const int* t_dev, int* lstatus, BCBF_PEND_TAIL) {
    const bcbf::PendulumDraw<double> D = BCBF_PEND_DRAW_ARGS;
    const bcbf::PendulumNominal Nm{nominal, numSteps, t, t_dev, lstatus};
    return bcbf::pendulum_control_step<true>(BCBF_PEND_ARGS, BCBF_PEND_LEARN_ARGS, z ? &D : nullptr, &Nm);
}
}
