// One event of the self-triggered closed loop for every instance in one launch (bcbf_unicycle_trigger_step): the trigger time
// tau of the control that bcbf_unicycle_control_step (called with dt = 0: solve only) has just left in its workspace, and the
// plant step over that time.  The periodic loops re-solve every dt; this one re-solves when the model says the last control
// stops being safe, each instance on its own clock.
//
// One workgroup per instance, as in trigger.hip, whose pair loop and closed forms it shares (trigger_pairs.h).  What
// trigger_interval_batch forms in torch before that launch -- a dozen launches and a [Bt, Nte, 3] tensor per step -- is done
// here on the test points that are in LDS anyway:
//   uBu  = ubar' Bhyp ubar, ubar = (1, u), u = y[b, 0:2]                                     one thread, fp64
//   xvel = |fhat + ghat u + M_k ubar|      the model's one-step prediction over dt            one thread, fp64, M_k ubar formed as the
//                                                                                             sampled branch of socp_quad_kernel does
//   Lh   = the largest single element of ObstacleCBF.grad_cbf over test points, obstacles and components, with the reference's
//          rho^2 = SUM over all test points of |p_a - c_k|^2 (unicycle_move_to_pose.py:670): per obstacle one block sum, then one
//          block maximum over all of them; wave shuffles, the four waves through LDS, no float atomics.  fp64 in both precisions
//          (Nte Kob / 256 evaluations per thread against Nte^2 / 512 pairs).
// Each of the three is rounded to the working type before the closed forms read it, so the results are those of
// bcbf_trigger_interval fed the same three numbers.  Thread 0 then acts: clamp, Euler step of the true plant (ackermann_euler's
// expressions, unicycle_task.h), the instance's clock, its event count and the planner rows of its new time.  An instance
// whose clock has reached t_end leaves before anything is read or written.
//
// That is one body (trigger_step_body) behind one kernel template and one launcher.  Two optional argument groups add work for
// thread 0; a group the entry does not take is not compiled in, a pointer the caller leaves null switches its piece off.
// Group Q, TriggerAuditArgs (bcbf_unicycle_trigger_step_audit, _observe), in fp64 from the values as the working type stores them,
// every output rounded once, with the draw and the counters of unicycle_task.h that the periodic loop's kernels call:
//   the plant drawn from the posterior (z given): a solved instance moves by xdot_s = fhat + ghat u + M_k ubar +
//     sqrt(max(ubar' B_k ubar, 0)) L_A z held for dt_b (the sampled solve does nothing when called with dt = 0), and the risk
//     counters are kept here because rollout_risk_kernel cannot tell an idle instance from a live one;
//   the audit of the held control (u_held given): the two sides of every obstacle row's cone, mean >= rho std, evaluated with
//     the control of the instance's PREVIOUS event on the rows the solve of this event wrote at the state where that control is
//     released -- what tau promised, measured one launch later.
// Group O, TriggerObserveArgs (bcbf_unicycle_trigger_step_observe), after the plant step: the event as the learner's observation
// row -- unicycle_observe (unicycle_task.h), the function the periodic solve / plant launch calls, on the states as stored and
// with the event's own hold dt_b in place of the batch's dt -- written to the stream row the instance's OWN event count names,
// so one captured graph serves every event, and the shift-invariant query of the next solve.  Plain vector stores from one
// lane, no atomics.
#include "trigger_pairs.h"
#include "unicycle_task.h"
#include <stdio.h>
#include <type_traits>

namespace bcbf {

template <typename T>
struct TriggerStepArgs {
    T* x; const T* y; const int* status; const T* fhat; const T* ghat; const T* Mk;
    const T* centers; const T* tw; const T* off;
    const T* ls; const T* sf; const T* Adiag; const T* Bhyp;
    double r, deltaL, zeta, L_alpha, tau_min, tau_max, t_end;
    T L_true;
    const T* plan_all; const T* dplan_all; double dt_plan;
    double* t; int* events; T* plan; T* dot_plan;
    T* tau; T* dt_used; T* Lfh; T* Lkd; T* Lh; T* xvel; T* uBu;
    int per_instance_hyper, Kob, Nte, P;
};

// group Q: the rows of the solve, the posterior plant (z == nullptr: the true plant) and the audit of the held control
// (u_held == nullptr: none)
template <typename T>
struct TriggerAuditArgs {
    const T* Bk; const T* A; const T* grad; const T* cst; const T* sign; const T* rho;
    const T* z; T* xdot_s; T* cbc_s; int* viol; int* solved; T* min_cbc;
    T* u_held; int* held; T* held_mean; T* held_margin; int* audit_n; int* audit_neg; T* audit_min;
};
struct TriggerNoAudit {};

// group O: the observation stream (obs_x == nullptr: no rows) and the next query (xq_next == nullptr: none); flags bit 0:
// shift-invariant inputs
template <typename T>
struct TriggerObserveArgs {
    T L_mean; T* obs_x; T* obs_uh; T* obs_y; int obs_ld, obs_row0, obs_every; T* xq_next; int flags;
};
struct TriggerNoObserve {};

// sum or maximum of v over the workgroup, through red[slot] (every slot is used once per launch: no barrier after the read)
__device__ inline double block_reduce(double v, double (*red)[TI_WAVES], int slot, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = is_max ? fmax(v, w) : v + w;
    }
    if ((threadIdx.x & 63) == 0) red[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    double out = red[slot][0];
    for (int w = 1; w < TI_WAVES; ++w) out = is_max ? fmax(out, red[slot][w]) : out + red[slot][w];
    return out;
}

// fhat + ghat u + M_k ubar of instance b, u = (ub[1], ub[2]), component d, as the sampled branch of socp_quad_kernel forms it
template <typename T>
__device__ inline double model_velocity(const TriggerStepArgs<T>& a, int b, int d, const double (&ub)[3]) {
    const T* g = a.ghat + ((size_t)b * 3 + d) * 2;
    const T* M = a.Mk + ((size_t)b * 3 + d) * 3;
    const double gu = (double)g[0] * ub[1] + (double)g[1] * ub[2];
    const double mu = (double)M[0] + (double)M[1] * ub[1] + (double)M[2] * ub[2];
    return (double)a.fhat[(size_t)b * 3 + d] + gu + mu;
}

// The audit of the held control (one thread): mean_k, margin_k = mean_k - rho std_k of the obstacle rows for ubar_h = (1, u_held)
template <typename T>
__device__ inline void audit_held_control(const TriggerStepArgs<T>& a, const TriggerAuditArgs<T>& q, int b) {
    const double ub[3] = {1.0, (double)q.u_held[(size_t)b * 2], (double)q.u_held[(size_t)b * 2 + 1]};
    const double s = quad_form3<T>(ub, q.Bk + (size_t)b * 9);
    double m[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) m[d] = model_velocity<T>(a, b, d, ub);
    const double rho = (double)q.rho[b];
    for (int k = 1; k <= a.Kob; ++k) {
        const T* gr = q.grad + ((size_t)b * (1 + a.Kob) + k) * 3;
        const double g[3] = {(double)gr[0], (double)gr[1], (double)gr[2]};
        const double gAg = quad_form3<T>(g, q.A + (size_t)b * 9);
        const double mean = cbc_on((double)q.sign[k], g, m, (double)q.cst[(size_t)b * (1 + a.Kob) + k]);
        const double margin = mean - rho * sqrt(fmax(s * gAg, 0.0));
        const size_t o = (size_t)b * a.Kob + k - 1;
        const T v[2] = {(T)mean, (T)margin};           // the counters see what is stored
        q.held_mean[o] = v[0];
        q.held_margin[o] = v[1];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            q.audit_neg[o * 2 + j] += v[j] >= T(0) ? 0 : 1;
            const T c = nan_is_lowest(v[j]), mn = q.audit_min[o * 2 + j];
            q.audit_min[o * 2 + j] = c < mn ? c : mn;
        }
    }
    q.audit_n[b] += 1;
}

// The plant drawn from the posterior over the hold dt (one thread): x, xdot_s, cbc_s and the risk counters of instance b
template <typename T>
__device__ inline void posterior_plant_step(const TriggerStepArgs<T>& a, const TriggerAuditArgs<T>& q, int b, const T (&xb)[3], T u0,
                                            T u1, bool solved, T dt) {
    const int K = 1 + a.Kob;
    double xd[3] = {0.0, 0.0, 0.0};
    if (solved) {
        const double ub[3] = {1.0, (double)u0, (double)u1};
        const double rs = __builtin_sqrt(fmax(quad_form3<T>(ub, q.Bk + (size_t)b * 9), 0.0));
        double LA[3][3];
        psd_chol3<T>(q.A + (size_t)b * 9, LA);
        const double z[3] = {(double)q.z[(size_t)b * 3], (double)q.z[(size_t)b * 3 + 1], (double)q.z[(size_t)b * 3 + 2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            xd[d] = posterior_draw(model_velocity<T>(a, b, d, ub), rs, LA[d], z);
            a.x[(size_t)b * 3 + d] = (T)((double)xb[d] + xd[d] * (double)dt);
        }
        if (q.solved) q.solved[b] += 1;
    }
    if (q.xdot_s) {
#pragma unroll
        for (int d = 0; d < 3; ++d) q.xdot_s[(size_t)b * 3 + d] = (T)xd[d];
    }
    for (int k = 0; k < K; ++k) {
        T cb = T(0);
        if (solved) {
            const T* gr = q.grad + ((size_t)b * K + k) * 3;
            const double g[3] = {(double)gr[0], (double)gr[1], (double)gr[2]};
            cb = (T)cbc_on((double)q.sign[k], g, xd, (double)q.cst[(size_t)b * K + k]);
        }
        if (q.cbc_s) q.cbc_s[(size_t)b * K + k] = cb;
        if (solved && k > 0 && q.solved) risk_count<T>(cb, q.viol + (size_t)b * a.Kob + k - 1, q.min_cbc + (size_t)b * a.Kob + k - 1);
    }
}

// The observation of the event (one thread, after the plant step): row obs_row0 + e / obs_every of instance b's stream when its
// event count e (before the increment) is a multiple of obs_every and the row exists, and the next query at every event
template <typename T>
__device__ inline void observe_event(const TriggerStepArgs<T>& a, const TriggerObserveArgs<T>& o, int b, const T (&xb)[3], T u0, T u1,
                                     bool solved, T dt) {
    UnicycleTask<T> task = {};
    task.L_mean = o.L_mean;
    task.dt = dt;
    task.shift_invariant = o.flags & 1;
    task.advance_plan = 0;
    task.xq_next = o.xq_next;
    const int e = a.events[b];
    if (o.obs_x != nullptr && e >= 0 && e % o.obs_every == 0) {
        const long long k = (long long)o.obs_row0 + e / o.obs_every;
        if (k < (long long)o.obs_ld) {                 // (a row past the stream is skipped: nothing is written outside the buffer)
            task.obs_x = o.obs_x + (size_t)k * 3;      // unicycle_observe writes row b * obs_ld of what it is handed
            task.obs_uh = o.obs_uh + (size_t)k * 3;
            task.obs_y = o.obs_y + (size_t)k * 3;
            task.obs_ld = o.obs_ld;
        }
    }
    // the state as the plant step stored it (the true drive's or the draw's); an unsolved instance kept its own and applied u = 0
    const T n0 = a.x[(size_t)b * 3], n1 = a.x[(size_t)b * 3 + 1], n2 = a.x[(size_t)b * 3 + 2];
    unicycle_observe<T>(task, b, xb[0], xb[1], xb[2], n0, n1, n2, solved ? u0 : T(0), solved ? u1 : T(0));
}

// The event of one instance by its workgroup.  Q = TriggerNoAudit: bcbf_unicycle_trigger_step; O = TriggerNoObserve: that entry
// and bcbf_unicycle_trigger_step_audit.
template <typename T, typename Q = TriggerNoAudit, typename O = TriggerNoObserve>
__device__ __forceinline__ void trigger_step_body(const TriggerStepArgs<T>& a, const Q& au = Q{}, const O& ob = O{}) {
    constexpr int NS = 3, ST = ti_stride(NS);
    extern __shared__ __attribute__((aligned(16))) unsigned char ts_raw[];
    __shared__ T ts_red[TI_WAVES][NS];
    __shared__ double ts_sum[BCBF_MAX_CONSTRAINTS][TI_WAVES];      // slot k: rho^2 of obstacle k; the last slot: the maximum
    T* pts = reinterpret_cast<T*>(ts_raw);
    const int b = blockIdx.x, hb = a.per_instance_hyper ? b : 0, N = a.Nte;
    const double t0 = a.t[b];
    if (t0 >= a.t_end) return;                          // finished (the whole workgroup: nothing of the instance is touched)
    T xb[NS], q[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        xb[j] = a.x[(size_t)b * NS + j];
        q[j] = T(ti_qscale<T>()) / a.ls[(size_t)hb * NS + j];
    }
    for (int i = threadIdx.x; i < N; i += TI_THREADS) {
#pragma unroll
        for (int j = 0; j < NS; ++j) pts[i * ST + j] = a.off[(size_t)i * NS + j] + xb[j];
    }
    __syncthreads();

    // Lh: grad_cbf on the [Nte, 3] test points of this instance, per obstacle with its batch-wide rho^2
    const double w0 = (double)a.tw[0], w1 = (double)a.tw[1];
    double lh = -INFINITY;
    for (int k = 0; k < a.Kob; ++k) {
        const double cx = (double)a.centers[((size_t)b * a.Kob + k) * 2], cy = (double)a.centers[((size_t)b * a.Kob + k) * 2 + 1];
        double part = 0.0;
        for (int i = threadIdx.x; i < N; i += TI_THREADS) {
            const double gx = (double)pts[i * ST] - cx, gy = (double)pts[i * ST + 1] - cy;
            part += gx * gx + gy * gy;
        }
        const double rho2 = block_reduce(part, ts_sum, k, false);
        for (int i = threadIdx.x; i < N; i += TI_THREADS) {
            const double gx = (double)pts[i * ST] - cx, gy = (double)pts[i * ST + 1] - cy, th = (double)pts[i * ST + 2];
            const double al = atan2(gy, gx), s = sin(al - th);
            lh = fmax(lh, fmax(fmax(w0 * 2.0 * gx + w1 * s * gy / rho2, w0 * 2.0 * gy - w1 * s * gx / rho2), -w1 * sin(th - al)));
        }
    }
    lh = block_reduce(lh, ts_sum, BCBF_MAX_CONSTRAINTS - 1, true);

    ti_pair_max<T, NS>(pts, N, q, ts_red);
    __syncthreads();
    if (threadIdx.x != 0) return;

    // ubar' Bhyp ubar and the model's predicted velocity, then the closed forms on the three numbers as the working type holds them.
    // (This quadratic form and the Euler step below stay written out: called through quad_form3 / ackermann_euler the compiler
    // schedules the plain entry's kernel differently, and that kernel's code is held fixed.)
    const T u0 = a.y[(size_t)b * 3], u1 = a.y[(size_t)b * 3 + 1];
    const double ub[3] = {1.0, (double)u0, (double)u1};
    double uB = 0.0, v2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) uB += ub[i] * (double)a.Bhyp[(size_t)hb * 9 + i * 3 + c] * ub[c];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double v = model_velocity<T>(a, b, d, ub);
        v2 += v * v;
    }
    const T uBT = (T)uB, xvT = (T)sqrt(v2), lhT = (T)lh;
    double lkd[NS], tv;
    const double L = ti_closed_forms<T, NS>(ts_red, a.ls + (size_t)hb * NS, (double)a.sf[hb], a.Adiag + (size_t)hb * NS, (double)uBT,
                                            (double)lhT, (double)xvT, a.r, a.deltaL, a.zeta, a.L_alpha, lkd, tv);
    const T tauT = (T)tv;
    if (a.uBu) a.uBu[b] = uBT;
    if (a.xvel) a.xvel[b] = xvT;
    if (a.Lh) a.Lh[b] = lhT;
    if (a.Lfh) a.Lfh[b] = (T)L;
    if (a.tau) a.tau[b] = tauT;
    if (a.Lkd) {
        for (int j = 0; j < NS; ++j) a.Lkd[(size_t)b * NS + j] = (T)lkd[j];
    }

    // act on it: the time this control is held (tau as the working type holds it; +inf -> tau_max, NaN or <= 0 -> tau_min) ...
    const bool solved = a.status[b] == BCBF_SOCP_OPTIMAL;
    const double tq = (double)tauT, left = a.t_end - t0;
    double hold = a.tau_max;                          // an unsolved instance takes no step: time passes as in the periodic loop
    if (solved) hold = !(tq > 0.0) ? a.tau_min : fmin(fmax(tq, a.tau_min), a.tau_max);
    const bool last = !(hold < left);
    const T dtT = (T)(last ? left : hold);
    bool euler = solved;
    if constexpr (!std::is_same<Q, TriggerNoAudit>::value) {
        // what the last control does at the state where it is released, on this event's rows, before anything of the event
        if (au.u_held != nullptr && au.held[b] != 0) audit_held_control<T>(a, au, b);
        if (au.z != nullptr) {                         // ... the plant drawn from the posterior over it
            euler = false;
            posterior_plant_step<T>(a, au, b, xb, u0, u1, solved, dtT);
        }
        if (au.u_held != nullptr) {
            au.u_held[(size_t)b * 2] = u0;
            au.u_held[(size_t)b * 2 + 1] = u1;
            au.held[b] = solved ? 1 : 0;
        }
    }
    if (euler) {                                      // ... the plant over it
        const T th = xb[2];
        a.x[(size_t)b * 3] = xb[0] + cos(th) * u0 * dtT;
        a.x[(size_t)b * 3 + 1] = xb[1] + sin(th) * u0 * dtT;
        a.x[(size_t)b * 3 + 2] = th + u1 / a.L_true * dtT;
    }
    if (a.dt_used) a.dt_used[b] = dtT;
    if constexpr (!std::is_same<O, TriggerNoObserve>::value) observe_event<T>(a, ob, b, xb, u0, u1, solved, dtT);   // ... what the learner sees of it
    // ... the clock (the step taken, as the plant saw it; the last one lands on t_end itself), the count and the planner's rows
    const double t1 = last ? a.t_end : t0 + (double)dtT;
    a.t[b] = t1;
    a.events[b] += 1;
    const double fi = floor(t1 / a.dt_plan);
    const int row = fi >= (double)(a.P - 1) ? a.P - 1 : (fi > 0.0 ? (int)fi : 0);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a.plan[(size_t)b * 3 + j] = a.plan_all[(size_t)row * 3 + j];
        a.dot_plan[(size_t)b * 3 + j] = a.dplan_all[(size_t)row * 3 + j];
    }
}

// G: nothing, (TriggerAuditArgs<T>) or (TriggerAuditArgs<T>, TriggerObserveArgs<T>)
template <typename T, typename... G>
__global__ void __launch_bounds__(TI_THREADS) unicycle_trigger_step_kernel(const TriggerStepArgs<T> a, const G... g) {
    trigger_step_body<T>(a, g...);
}

// the argument checks, one overload per group present, each after the ones before it
template <typename T>
static int trigger_args_ok(const char* entry, const TriggerStepArgs<T>& a, int Bt, int Bh) {
    static thread_local char msg[280];
    const char* why = nullptr;
    if (!a.x || !a.y || !a.status || !a.fhat || !a.ghat || !a.Mk) why = "null control-step buffer (x, y, status, fhat, ghat, Mk)";
    else if (!a.centers || !a.tw || !a.off) why = "null input pointer (centers, tw, off)";
    else if (!a.ls || !a.sf || !a.Adiag || !a.Bhyp) why = "null hyper-parameter pointer (ls, sf, Adiag, Bhyp)";
    else if (!a.plan_all || !a.dplan_all) why = "null planner table";
    else if (!a.t || !a.events || !a.plan || !a.dot_plan) why = "null in/out pointer (t, events, plan, dot_plan)";
    else if (Bt < 1) why = "Bt < 1";
    else if (Bh != 1 && Bh != Bt) why = "the hyper-parameters' leading extent Bh must be 1 or Bt";
    else if (a.Kob < 1 || a.Kob > BCBF_MAX_CONSTRAINTS - 1) why = "need 1 <= Kob <= BCBF_MAX_CONSTRAINTS - 1";
    else if (a.Nte < 1) why = "Nte < 1";
    else if ((size_t)a.Nte * ti_stride(3) * sizeof(T) > TI_MAX_LDS) why = "Nte too large (the test points of one instance are kept in LDS)";
    else if (a.P < 1) why = "P < 1";
    else if (!(a.dt_plan > 0.0)) why = "dt_plan must be positive";
    else if (!(a.tau_min > 0.0)) why = "tau_min must be positive";
    else if (!(a.tau_min <= a.tau_max)) why = "tau_min > tau_max";
    else if (!(a.tau_max < INFINITY)) why = "tau_max must be finite";
    if (!why) return 1;
    snprintf(msg, sizeof(msg), "%s: %s (Bt=%d Bh=%d Kob=%d Nte=%d P=%d tau_min=%g tau_max=%g)", entry, why, Bt, Bh, a.Kob, a.Nte, a.P,
             a.tau_min, a.tau_max);
    set_error_message(msg);
    return 0;
}

template <typename T>
static int trigger_args_ok(const char* entry, const TriggerStepArgs<T>& a, int Bt, int Bh, const TriggerAuditArgs<T>& q) {
    if (!trigger_args_ok<T>(entry, a, Bt, Bh)) return 0;
    static thread_local char msg[280];
    const int counters = (q.viol != nullptr) + (q.solved != nullptr) + (q.min_cbc != nullptr);
    const int held = (q.u_held != nullptr) + (q.held != nullptr) + (q.held_mean != nullptr) + (q.held_margin != nullptr) +
                     (q.audit_n != nullptr) + (q.audit_neg != nullptr) + (q.audit_min != nullptr);
    const char* why = nullptr;
    if (!q.Bk || !q.A || !q.grad || !q.cst || !q.sign || !q.rho) why = "null row of the solve (Bk, A, grad, cst, sign, rho)";
    else if (a.Kob + 1 > BCBF_MAX_QUAD_CONSTRAINTS) why = "need Kob + 1 <= BCBF_MAX_QUAD_CONSTRAINTS (the rows are the fused solve's)";
    else if (counters != 0 && counters != 3) why = "the risk counters (viol, solved, min_cbc) are given together or not at all";
    else if (!q.z && (q.xdot_s || q.cbc_s || counters)) why = "xdot_s, cbc_s and the risk counters need the draws z";
    else if (held != 0 && held != 7)
        why = "the audit buffers (u_held, held, held_mean, held_margin, audit_n, audit_neg, audit_min) are given together or not at all";
    if (!why) return 1;
    snprintf(msg, sizeof(msg), "%s: %s (Bt=%d Kob=%d counters=%d/3 audit=%d/7)", entry, why, Bt, a.Kob, counters, held);
    set_error_message(msg);
    return 0;
}

template <typename T>
static int trigger_args_ok(const char* entry, const TriggerStepArgs<T>& a, int Bt, int Bh, const TriggerAuditArgs<T>& q,
                           const TriggerObserveArgs<T>& o) {
    if (!trigger_args_ok<T>(entry, a, Bt, Bh, q)) return 0;
    static thread_local char msg[280];
    const int rows = (o.obs_x != nullptr) + (o.obs_uh != nullptr) + (o.obs_y != nullptr);
    const char* why = nullptr;
    if (rows != 0 && rows != 3) why = "the observation rows (obs_x, obs_uh, obs_y) are given together or not at all";
    else if (rows && o.obs_ld < 1) why = "obs_ld < 1";
    else if (rows && o.obs_row0 < 0) why = "obs_row0 < 0";
    else if (rows && o.obs_every < 1) why = "obs_every < 1";
    else if (rows && (o.L_mean != o.L_mean || o.L_mean == T(0))) why = "L_mean must be a number other than 0 (the rows subtract g(theta; L_mean) u)";
    else if (o.flags & ~1) why = "flags: only bit 0 (shift-invariant inputs) is defined";
    if (!why) return 1;
    snprintf(msg, sizeof(msg), "%s: %s (Bt=%d rows=%d/3 obs_ld=%d obs_row0=%d obs_every=%d L_mean=%g flags=%d)", entry, why, Bt, rows,
             o.obs_ld, o.obs_row0, o.obs_every, (double)o.L_mean, o.flags);
    set_error_message(msg);
    return 0;
}

// the one launcher: the checks of the groups present, then unicycle_trigger_step_kernel<T, G...>
template <typename T, typename... G>
static int launch_trigger_step(const char* entry, TriggerStepArgs<T> a, int Bt, int Bh, void* stream, const G&... g) {
    if (!trigger_args_ok<T>(entry, a, Bt, Bh, g...)) return BCBF_EINVAL;
    a.per_instance_hyper = Bh == Bt && Bt > 1 ? 1 : 0;
    const size_t lds = (size_t)a.Nte * ti_stride(3) * sizeof(T);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)unicycle_trigger_step_kernel<T, G...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((unicycle_trigger_step_kernel<T, G...>), dim3(Bt), dim3(TI_THREADS), lds, (hipStream_t)stream, a, g...);
    return check_launch(entry);
}

}  // namespace bcbf

// the parameters the three entries share, in ABI order (include/bcbf.h), and the argument groups they fill
#define BCBF_TS_PARAMS(T)                                                                                                         \
    T* x, const T* y, const int* status, const T* fhat, const T* ghat, const T* Mk, const T* centers, const T* tw, const T* off,  \
        double r, const T* ls, const T* sf, const T* Adiag, const T* Bhyp, double deltaL, double zeta, double L_alpha,            \
        double tau_min, double tau_max, double t_end, T L_true, const T* plan_all, const T* dplan_all, double dt_plan, double* t, \
        int* events, T* plan, T* dot_plan, T* tau, T* dt_used, T* Lfh, T* Lkd, T* Lh, T* xvel, T* uBu
#define BCBF_TS_ARGS(T)                                                                                                           \
    bcbf::TriggerStepArgs<T> {                                                                                                    \
        x, y, status, fhat, ghat, Mk, centers, tw, off, ls, sf, Adiag, Bhyp, r, deltaL, zeta, L_alpha, tau_min, tau_max, t_end,   \
            L_true, plan_all, dplan_all, dt_plan, t, events, plan, dot_plan, tau, dt_used, Lfh, Lkd, Lh, xvel, uBu, 0, Kob, Nte, P \
    }
#define BCBF_TS_AUDIT_PARAMS(T)                                                                                                   \
    const T* Bk, const T* A, const T* grad, const T* cst, const T* sign, const T* rho, const T* z, T* xdot_s, T* cbc_s, int* viol, \
        int* solved, T* min_cbc, T* u_held, int* held, T* held_mean, T* held_margin, int* audit_n, int* audit_neg, T* audit_min
#define BCBF_TS_AUDIT_ARGS(T)                                                                                                     \
    bcbf::TriggerAuditArgs<T> {                                                                                                   \
        Bk, A, grad, cst, sign, rho, z, xdot_s, cbc_s, viol, solved, min_cbc, u_held, held, held_mean, held_margin, audit_n,      \
            audit_neg, audit_min                                                                                                  \
    }
#define BCBF_TS_SIZES int Bt, int Bh, int Kob, int Nte, int P, void* stream
#define BCBF_TRIGGER_STEP(T, SUF)                                                                                                 \
    extern "C" int bcbf_unicycle_trigger_step_##SUF(BCBF_TS_PARAMS(T), BCBF_TS_SIZES) {                                           \
        return bcbf::launch_trigger_step<T>("bcbf_unicycle_trigger_step_" #SUF, BCBF_TS_ARGS(T), Bt, Bh, stream);                 \
    }                                                                                                                             \
    extern "C" int bcbf_unicycle_trigger_step_audit_##SUF(BCBF_TS_PARAMS(T), BCBF_TS_AUDIT_PARAMS(T), BCBF_TS_SIZES) {            \
        return bcbf::launch_trigger_step<T>("bcbf_unicycle_trigger_step_audit_" #SUF, BCBF_TS_ARGS(T), Bt, Bh, stream,            \
                                            BCBF_TS_AUDIT_ARGS(T));                                                               \
    }                                                                                                                             \
    extern "C" int bcbf_unicycle_trigger_step_observe_##SUF(BCBF_TS_PARAMS(T), BCBF_TS_AUDIT_PARAMS(T), float L_mean, T* obs_x,   \
                                                            T* obs_uh, T* obs_y, int obs_ld, int obs_row0, int obs_every,         \
                                                            T* xq_next, int flags, BCBF_TS_SIZES) {                               \
        return bcbf::launch_trigger_step<T>(                                                                                      \
            "bcbf_unicycle_trigger_step_observe_" #SUF, BCBF_TS_ARGS(T), Bt, Bh, stream, BCBF_TS_AUDIT_ARGS(T),                   \
            bcbf::TriggerObserveArgs<T>{(T)L_mean, obs_x, obs_uh, obs_y, obs_ld, obs_row0, obs_every, xq_next, flags});           \
    }
BCBF_TRIGGER_STEP(float, f32)
BCBF_TRIGGER_STEP(double, f64)

