// One host call per control step: the whole unicycle hot path (task functions -> GP posterior ->
// chance-constraint terms + SOCP (one fused launch) -> plant Euler step) enqueued on one stream.  This is the entry
// point a reference-side `ControllerCLFBayesian.control` binds to (unicycle_move_to_pose.py:926-995);
// it only sequences the kernels of the other translation units.
#include "bcbf_common.h"
#include "unicycle_task.h"

namespace bcbf {
template <typename T>
int launch_unicycle_socp(const T* Mk, const T* Bk, const T* A, const T* sign, const T* w, const T* r, const T* relax_mask,
                         const T* rho, T* cones, int* cstatus, T* y, int* status, int* iters, int Bt, int max_iters,
                         const UnicycleTask<T>& task, void* stream);

// What the observing entries add: the step of a loop that LEARNS from itself (LearnedShiftInvariantDynamics,
// unicycle_move_to_pose.py:326-386).  The posterior is queried at `xq` (NULL: at x -- pass the shift-invariant input (0, 0, theta)
// of the current state) and the solve / plant launch also writes this step's observation row and the next query (UnicycleTask:
// obs_x, obs_uh, obs_y at row b * obs_ld; xq_next).  flags: bit 0 = shift-invariant regressor inputs, bit 1 = the planner's target
// advances with the step (plan += dot_plan dt).  The defaults are UnicycleTask's: the plain entries leave both groups at them.
template <typename T>
struct UnicycleObserveArgs {
    const T* xq = nullptr;
    T *obs_x = nullptr, *obs_uh = nullptr, *obs_y = nullptr;
    int obs_ld = 1;
    T* xq_next = nullptr;
    int flags = 1;
};

// What the sampled entries add: the plant DRAWN FROM THE MODEL'S OWN POSTERIOR (fu_func_gp(u), unicycle_move_to_pose.py:262-275,
// sampled as GaussianProcessBase.sample samples it, gp_algebra.py:33-34).  A solved instance advances by
//   xdot_s = fhat + ghat u + M_k ubar + sqrt(max(ubar' B_k ubar, 0)) L_A z,   A = L_A L_A',   ubar = (1, u)
// instead of by the true Ackermann drive (L_true is ignored); cbc_s[b,k] = sign_k (grad_k . xdot_s + cst_k) (cbc1.py:10-14) is row
// k's condition on the draw.  z[Bt,3]: the caller's standard normals; xdot_s[Bt,3], cbc_s[Bt,1+Kob]: optional.  The observation
// rows then record the SAMPLED plant; the solve launch is the kernel's sampled instantiation.
template <typename T>
struct UnicycleSampledArgs {
    const T* z = nullptr;
    T *xdot_s = nullptr, *cbc_s = nullptr;
};

// Every argument of a control step.  The 42 all entries share and the stream triple, in ABI order (include/bcbf.h); then what the
// entry says: the learned model's data kernel (0 = RBF, 1 = Matern-5/2, 2 = their product: which posterior launch runs), which
// checks apply, and the optional groups.
enum UnicycleStepForm { US_PLAIN, US_OBSERVE, US_SAMPLED };
template <typename T>
struct UnicycleStepArgs {
    const T *Lop, *Vw, *X, *UHB, *ell, *s2, *Bm, *M0, *A;
    T* x;
    const T *plan, *dot_plan, *Kp;
    T clf_gamma;
    const T *centers, *radii, *tw, *gammas;
    T L_mean;
    const T *w, *r, *sign, *relax_mask, *rho;
    T *grad, *cst, *fhat, *ghat, *Mk, *Bk, *cones;
    int* cstatus;
    T* y;
    int *status, *iters;
    T dt, L_true;
    int Bt, N, Kob, max_iters, shared_gp;
    void *ev_start, *ev_stop, *stream;
    int kernel_kind;
    UnicycleStepForm form = US_PLAIN;
    UnicycleObserveArgs<T> obs{};
    UnicycleSampledArgs<T> draw{};
};

// the posterior launches of a precision: the streaming kernel (RBF, one model per instance), and the query of each data kernel
template <typename T>
struct UnicyclePosterior;
#define BCBF_US_POSTERIOR(T, SUF)                                                                                      \
    template <>                                                                                                        \
    struct UnicyclePosterior<T> {                                                                                      \
        static constexpr auto step = bcbf_posterior_step_##SUF;                                                        \
        static constexpr decltype(&bcbf_posterior_query_##SUF) query[3] = {                                            \
            bcbf_posterior_query_##SUF, bcbf_posterior_query_matern52_##SUF, bcbf_posterior_query_rbfm52_##SUF};       \
    };
BCBF_US_POSTERIOR(float, f32)
BCBF_US_POSTERIOR(double, f64)
#undef BCBF_US_POSTERIOR

// Two launches per step: the posterior kernel, then ONE kernel that forms the task rows (CLC + obstacle CBCs) from the
// state, the chance-constraint terms and cones from (M_k, B_k), solves the SOCP and advances the plant.
template <typename T>
static int unicycle_control_step(const UnicycleStepArgs<T>& a) {
    const UnicycleObserveArgs<T>& o = a.obs;
    if (a.Bt <= 0) return BCBF_OK;
    // the refusals leave the error message alone.  The plain entries expose the rows; the others may, all four or none
    if (!a.x || a.Kob < 0 || a.Kob + 1 > BCBF_MAX_QUAD_CONSTRAINTS || a.kernel_kind < 0 || a.kernel_kind > 2) return BCBF_EINVAL;
    if ((a.form == US_PLAIN || a.grad) && (!a.grad || !a.cst || !a.fhat || !a.ghat)) return BCBF_EINVAL;
    if ((o.obs_x || o.obs_uh || o.obs_y) && (!o.obs_x || !o.obs_uh || !o.obs_y || o.obs_ld < 1 || !(a.dt > T(0)))) return BCBF_EINVAL;
    if (a.form == US_SAMPLED && !a.draw.z) return BCBF_EINVAL;
    hipStream_t st = (hipStream_t)a.stream;
    if (a.ev_start) (void)hipEventRecord((hipEvent_t)a.ev_start, st);
    // Lop == NULL: no learned model in the loop -- (Mk, Bk) are the caller's (fixed-kernel model: 0 and I)
    const T* q = o.xq ? o.xq : a.x;
    int rc = BCBF_OK;
    if (a.Lop && a.kernel_kind == 0 && !a.shared_gp)
        rc = UnicyclePosterior<T>::step(a.Lop, a.Vw, a.X, a.UHB, a.ell, a.s2, a.Bm, a.M0, q, nullptr, a.Mk, a.Bk, a.Bt, a.N, 3, 2,
                                        a.stream);
    else if (a.Lop)
        rc = UnicyclePosterior<T>::query[a.kernel_kind](a.Lop, a.Vw, a.X, a.UHB, a.ell, a.s2, a.Bm, a.M0, q, nullptr, a.Mk, a.Bk,
                                                        nullptr, a.shared_gp ? 1 : 0, a.Bt, a.N, 3, 2, a.stream);
    if (a.ev_stop) (void)hipEventRecord((hipEvent_t)a.ev_stop, st);
    if (rc) return rc;
    UnicycleTask<T> task;
    task.x = a.x; task.plan = a.plan; task.dot_plan = a.dot_plan; task.Kp = a.Kp; task.centers = a.centers;
    task.radii = a.radii; task.tw = a.tw; task.gammas = a.gammas; task.clf_gamma = a.clf_gamma; task.L_mean = a.L_mean;
    task.dt = a.dt; task.L_true = a.L_true; task.grad = a.grad; task.cst = a.cst; task.fhat = a.fhat; task.ghat = a.ghat;
    task.Kob = a.Kob; task.obs_x = o.obs_x; task.obs_uh = o.obs_uh; task.obs_y = o.obs_y; task.obs_ld = o.obs_ld;
    task.xq_next = o.xq_next; task.shift_invariant = o.flags & 1; task.advance_plan = (o.flags >> 1) & 1;
    task.z = a.draw.z; task.xdot_s = a.draw.xdot_s; task.cbc_s = a.draw.cbc_s;
    return launch_unicycle_socp<T>(a.Mk, a.Bk, a.A, a.sign, a.w, a.r, a.relax_mask, a.rho, a.cones, a.cstatus, a.y, a.status,
                                   a.iters, a.Bt, a.max_iters, task, a.stream);
}
}  // namespace bcbf

// the parameters of each argument group, in ABI order (include/bcbf.h), and the records they fill
#define BCBF_US_PARAMS(T)                                                                                              \
    const T* Lop, const T* Vw, const T* X, const T* UHB, const T* ell, const T* s2, const T* Bm, const T* M0,         \
        const T* A, T* x, const T* plan, const T* dot_plan, const T* Kp, T clf_gamma, const T* centers,               \
        const T* radii, const T* tw, const T* gammas, T L_mean, const T* w, const T* r, const T* sign,                \
        const T* relax_mask, const T* rho, T* grad, T* cst, T* fhat, T* ghat, T* Mk, T* Bk, T* cones, int* cstatus,   \
        T* y, int* status, int* iters, T dt, T L_true, int Bt, int N, int Kob, int max_iters, int shared_gp
#define BCBF_US_STREAM void* ev_start, void* ev_stop, void* stream
// (after the stream triple: kernel_kind, then the form and the groups of an observing or sampled entry)
#define BCBF_US_ARGS(T, ...)                                                                                           \
    bcbf::UnicycleStepArgs<T> {                                                                                        \
        Lop, Vw, X, UHB, ell, s2, Bm, M0, A, x, plan, dot_plan, Kp, clf_gamma, centers, radii, tw, gammas, L_mean, w, r, sign,  \
            relax_mask, rho, grad, cst, fhat, ghat, Mk, Bk, cones, cstatus, y, status, iters, dt, L_true, Bt, N, Kob, max_iters, \
            shared_gp, ev_start, ev_stop, stream, __VA_ARGS__                                                          \
    }
#define BCBF_US_OBSERVE_PARAMS(T) const T* xq, T* obs_x, T* obs_uh, T* obs_y, int obs_ld, T* xq_next, int flags
#define BCBF_US_OBSERVE_ARGS(T) bcbf::UnicycleObserveArgs<T> { xq, obs_x, obs_uh, obs_y, obs_ld, xq_next, flags }
#define BCBF_US_SAMPLED_PARAMS(T) int kernel_kind, const T* z, T* xdot_s, T* cbc_s
#define BCBF_US_SAMPLED_ARGS(T) bcbf::UnicycleSampledArgs<T> { z, xdot_s, cbc_s }

// The plain step per data kernel of the learned model (bcbf.h: *_matern52, *_rbfm52 are opt-in; parity unpinned -- the reference
// has no Matern kernel): only the posterior launch differs (one GP per instance, RBF: the streaming kernel; otherwise the query).
// The observing step is built for the RBF kernel; the sampled step takes the kernel as an argument.
#define BCBF_CTRL(T, SUF)                                                                                              \
    extern "C" int bcbf_unicycle_control_step_##SUF(BCBF_US_PARAMS(T), BCBF_US_STREAM) {                               \
        return bcbf::unicycle_control_step<T>(BCBF_US_ARGS(T, 0));                                                     \
    }                                                                                                                  \
    extern "C" int bcbf_unicycle_control_step_matern52_##SUF(BCBF_US_PARAMS(T), BCBF_US_STREAM) {                      \
        return bcbf::unicycle_control_step<T>(BCBF_US_ARGS(T, 1));                                                     \
    }                                                                                                                  \
    extern "C" int bcbf_unicycle_control_step_rbfm52_##SUF(BCBF_US_PARAMS(T), BCBF_US_STREAM) {                        \
        return bcbf::unicycle_control_step<T>(BCBF_US_ARGS(T, 2));                                                     \
    }                                                                                                                  \
    extern "C" int bcbf_unicycle_control_step_observe_##SUF(BCBF_US_PARAMS(T), BCBF_US_OBSERVE_PARAMS(T), BCBF_US_STREAM) { \
        return bcbf::unicycle_control_step<T>(BCBF_US_ARGS(T, 0, bcbf::US_OBSERVE, BCBF_US_OBSERVE_ARGS(T)));          \
    }                                                                                                                  \
    extern "C" int bcbf_unicycle_control_step_sampled_##SUF(BCBF_US_PARAMS(T), BCBF_US_OBSERVE_PARAMS(T),              \
                                                            BCBF_US_SAMPLED_PARAMS(T), BCBF_US_STREAM) {               \
        return bcbf::unicycle_control_step<T>(                                                                         \
            BCBF_US_ARGS(T, kernel_kind, bcbf::US_SAMPLED, BCBF_US_OBSERVE_ARGS(T), BCBF_US_SAMPLED_ARGS(T)));         \
    }
BCBF_CTRL(float, f32)
BCBF_CTRL(double, f64)
