// Batched unicycle / Ackermann task functions: CLFCartesian, ObstacleCBF, prior dynamics and the
// explicit-Euler plant step (reference: bayes_cbf/unicycle_move_to_pose.py:112-139, 235-282,
// 522-615, 618-696; bayes_cbf/misc.py:317-318).  Elementwise, one lane per instance.
#include "unicycle_task.h"

namespace bcbf {

template <typename T>
__global__ void unicycle_constraints_kernel(const T* __restrict__ x, const T* __restrict__ plan,
                                            const T* __restrict__ dot_plan, const T* __restrict__ Kp, T clf_gamma,
                                            const T* __restrict__ centers, const T* __restrict__ radii,
                                            const T* __restrict__ tw, const T* __restrict__ gammas, T L_mean,
                                            T* __restrict__ grad, T* __restrict__ cst, T* __restrict__ fhat,
                                            T* __restrict__ ghat, int Bt, int Kob) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    const T px = x[b * 3], py = x[b * 3 + 1], th = x[b * 3 + 2];
    const int K = 1 + Kob;
    for (int k = 0; k < K; ++k) {
        T g[3], c;
        unicycle_row<T>(k, px, py, th, plan + (size_t)b * 3, dot_plan + (size_t)b * 3, Kp, clf_gamma,
                        centers + (size_t)b * Kob * 2, radii + (size_t)b * Kob, tw, gammas, g, c);
        T* gk = grad + ((size_t)b * K + k) * 3;
        gk[0] = g[0]; gk[1] = g[1]; gk[2] = g[2];
        cst[(size_t)b * K + k] = c;
    }
    fhat[b * 3] = fhat[b * 3 + 1] = fhat[b * 3 + 2] = T(0);
    T G[3][2];
    ackermann_g<T>(th, L_mean, G);
    T* Gp = ghat + (size_t)b * 6;
    for (int d = 0; d < 3; ++d) { Gp[d * 2] = G[d][0]; Gp[d * 2 + 1] = G[d][1]; }
}

template <typename T>
__global__ void unicycle_step_kernel(T* __restrict__ x, const T* __restrict__ u, T dt, T L_true, int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    ackermann_euler<T>(x[b * 3], x[b * 3 + 1], x[b * 3 + 2], u[b * 2], u[b * 2 + 1], dt, L_true, x[b * 3], x[b * 3 + 1], x[b * 3 + 2]);
}

// Safety bookkeeping of one closed-loop step of a Monte-Carlo rollout (rollouts.monte_carlo_safety_rollouts), one launch
// instead of eight elementwise ones: per trajectory  min_h = min(min_h, min_k cst_k / gamma_k)  over the obstacle rows
// (h_k(x_t) before the step; a non-finite h counts as -inf: it can never pass for "collision-free"), and -- only where
// the program was solved, the reference raises ValueError otherwise (unicycle_move_to_pose.py:954-964) --
// cost += sum_i w_i y_i^2;  fails += (status != 0).
template <typename T>
__global__ void rollout_stats_kernel(const T* __restrict__ cst, const T* __restrict__ y, const int* __restrict__ status,
                                     const T* __restrict__ w, const T* __restrict__ gammas, T* __restrict__ min_h,
                                     T* __restrict__ cost, int* __restrict__ fails, int Bt, int Kob, int nv) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    T h = INFINITY;
    for (int k = 0; k < Kob; ++k) {
        T hk = cst[(size_t)b * (1 + Kob) + 1 + k] / gammas[k];
        if (!(hk == hk)) hk = -INFINITY;
        h = hk < h ? hk : h;
    }
    if (Kob > 0) min_h[b] = h < min_h[b] ? h : min_h[b];
    if (status[b] == 0) {
        T c = T(0);
        for (int i = 0; i < nv; ++i) c += w[(size_t)b * nv + i] * y[(size_t)b * nv + i] * y[(size_t)b * nv + i];
        cost[b] += c;
    } else {
        fails[b] += 1;
    }
}

// Risk bookkeeping of one closed-loop step on a plant drawn from the posterior (bcbf_unicycle_control_step_sampled's cbc_s), one
// launch: where the program was solved, solved += 1 and per obstacle row k = 1..Kob  viol += (cbc_s_k < 0)  -- a non-finite value
// counts as a violation -- and min_cbc = min(min_cbc, cbc_s_k).  An unsolved instance took no step: its counters are untouched.
template <typename T>
__global__ void rollout_risk_kernel(const T* __restrict__ cbc_s, const int* __restrict__ status, int* __restrict__ viol,
                                    int* __restrict__ solved, T* __restrict__ min_cbc, int Bt, int Kob) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt || status[b] != 0) return;
    solved[b] += 1;
    for (int k = 0; k < Kob; ++k)
        risk_count<T>(cbc_s[(size_t)b * (1 + Kob) + 1 + k], viol + (size_t)b * Kob + k, min_cbc + (size_t)b * Kob + k);
}

}  // namespace bcbf

extern "C" {
#define BCBF_ROLLOUT_RISK(T, SUF)                                                                                     \
    int bcbf_rollout_risk_##SUF(const T* cbc_s, const int* status, int* viol, int* solved, T* min_cbc, int Bt, int Kob, \
                                void* stream) {                                                                       \
        if (Bt <= 0) return BCBF_OK;                                                                                  \
        if (!cbc_s || !status || !solved || Kob < 0 || (Kob > 0 && (!viol || !min_cbc))) return BCBF_EINVAL;          \
        hipLaunchKernelGGL((bcbf::rollout_risk_kernel<T>), dim3((Bt + 255) / 256), dim3(256), 0, (hipStream_t)stream, \
                           cbc_s, status, viol, solved, min_cbc, Bt, Kob);                                            \
        return bcbf::check_launch("rollout_risk");                                                                    \
    }
BCBF_ROLLOUT_RISK(float, f32)
BCBF_ROLLOUT_RISK(double, f64)
#undef BCBF_ROLLOUT_RISK
#define BCBF_ROLLOUT_STATS(T, SUF)                                                                                    \
    int bcbf_rollout_stats_##SUF(const T* cst, const T* y, const int* status, const T* w, const T* gammas, T* min_h,  \
                                 T* cost, int* fails, int Bt, int Kob, int nv, void* stream) {                        \
        if (Bt <= 0) return BCBF_OK;                                                                                  \
        if (!cst || !y || !status || !w || !min_h || !cost || !fails || Kob < 0 || nv < 1 || (Kob > 0 && !gammas))    \
            return BCBF_EINVAL;                                                                                       \
        hipLaunchKernelGGL((bcbf::rollout_stats_kernel<T>), dim3((Bt + 255) / 256), dim3(256), 0, (hipStream_t)stream, \
                           cst, y, status, w, gammas, min_h, cost, fails, Bt, Kob, nv);                               \
        return bcbf::check_launch("rollout_stats");                                                                   \
    }
BCBF_ROLLOUT_STATS(float, f32)
BCBF_ROLLOUT_STATS(double, f64)
#undef BCBF_ROLLOUT_STATS
#define BCBF_UNI(T, SUF)                                                                                              \
    int bcbf_unicycle_constraints_##SUF(const T* x, const T* plan, const T* dot_plan, const T* Kp, T clf_gamma,       \
                                        const T* centers, const T* radii, const T* tw, const T* gammas, T L_mean,     \
                                        T* grad, T* cst, T* fhat, T* ghat, int Bt, int Kob, void* stream) {           \
        if (Bt <= 0) return BCBF_OK;                                                                                  \
        if (!x || !plan || !dot_plan || !Kp || !grad || !cst || !fhat || !ghat) return BCBF_EINVAL;                   \
        if (Kob < 0 || Kob + 1 > BCBF_MAX_CONSTRAINTS || (Kob > 0 && (!centers || !radii || !tw || !gammas)))         \
            return BCBF_EINVAL;                                                                                       \
        hipLaunchKernelGGL((bcbf::unicycle_constraints_kernel<T>), dim3((Bt + 255) / 256), dim3(256), 0,              \
                           (hipStream_t)stream, x, plan, dot_plan, Kp, clf_gamma, centers, radii, tw, gammas, L_mean, \
                           grad, cst, fhat, ghat, Bt, Kob);                                                           \
        return bcbf::check_launch("unicycle_constraints");                                                            \
    }                                                                                                                 \
    int bcbf_unicycle_step_##SUF(T* x, const T* u, T dt, T L_true, int Bt, void* stream) {                            \
        if (Bt <= 0) return BCBF_OK;                                                                                  \
        if (!x || !u) return BCBF_EINVAL;                                                                             \
        hipLaunchKernelGGL((bcbf::unicycle_step_kernel<T>), dim3((Bt + 255) / 256), dim3(256), 0,                     \
                           (hipStream_t)stream, x, u, dt, L_true, Bt);                                                \
        return bcbf::check_launch("unicycle_step");                                                                   \
    }
BCBF_UNI(float, f32)
BCBF_UNI(double, f64)
}
