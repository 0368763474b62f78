// Obstacle fields for the chance-constrained unicycle step: a working set of at most three obstacle cones in the fused solver,
// chosen from a field of up to BCBF_MAX_FIELD discs, and a certificate that the working-set optimum is the optimum of the
// program with EVERY disc's cone (ObstacleCBF, unicycle_move_to_pose.py:618-696; `_cbcs`, :901-920: one un-relaxed cone per
// obstacle; the program, :926-953).  The program is convex with a strictly convex objective in (u, relax): when no cone outside
// the working set is violated at the working-set optimum, that point is feasible for the full program and therefore its unique
// optimum.  Three kernels; the solver and the posterior kernels are untouched.
//   select  one wave per instance, lanes stride over the discs: h_k(x) of every disc, the S smallest into the working set
//   audit   one wave per instance: every disc's cone at the solved control; certify, or swap the worst violator for a slack slot
//   commit  one lane per instance: the effective status, and the plant step of the certified instances
// Arithmetic is fp64 for both entry precisions (inputs read as stored): the decisions do not depend on the entry's dtype.
// No LDS, no scratch (every register array is indexed by compile-time constants; the build's resource guard checks it).
// (The commit on a plant drawn from the posterior is field_plant.hip; what both files share is obstacle_field.h.)
#include "obstacle_field.h"

namespace bcbf {

template <typename T>
__global__ __launch_bounds__(64 * FIELD_WAVES) void obstacle_field_select_kernel(
    const T* __restrict__ x, const T* __restrict__ centers_f, const T* __restrict__ radii_f, int field_stride,
    const T* __restrict__ tw, int* __restrict__ idx, T* __restrict__ centers_sel, T* __restrict__ radii_sel,
    T* __restrict__ min_h, int* __restrict__ cert, int* __restrict__ rounds, int Bt, int Kf, int S) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * FIELD_WAVES + (threadIdx.x >> 6);
    if (b >= Bt) return;                                          // (wave-uniform)
    const T* cf = centers_f + (size_t)b * field_stride * Kf * 2;
    const T* rf = radii_f + (size_t)b * field_stride * Kf;
    const double px = (double)x[(size_t)b * 3], py = (double)x[(size_t)b * 3 + 1], th = (double)x[(size_t)b * 3 + 2];
    const double tw0 = (double)tw[0], tw1 = (double)tw[1];
    // the keys this lane owns: h_k with NaN below everything (k = lane + 64 lap), +inf past the end of the field
    double key[FIELD_LAPS];
    double hmin = INFINITY;
#pragma unroll
    for (int lap = 0; lap < FIELD_LAPS; ++lap) {
        const int k = lane + 64 * lap;
        key[lap] = INFINITY;
        if (k < Kf) {
            double g[3], h;
            field_row(px, py, th, (double)cf[k * 2], (double)cf[k * 2 + 1], (double)rf[k], tw0, tw1, 1.0, g, h);
            key[lap] = nan_is_lowest(h);
            const double hm = h - h == 0.0 ? h : -INFINITY;       // min_h: anything non-finite counts as -inf
            hmin = hm < hmin ? hm : hmin;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(hmin, off, 64);
        hmin = o < hmin ? o : hmin;
    }
    int chosen[3] = {-1, -1, -1};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (s < S) {                                              // (uniform)
            double v = INFINITY;
            int i = FIELD_NONE;
#pragma unroll
            for (int lap = 0; lap < FIELD_LAPS; ++lap) {
                const int k = lane + 64 * lap;
                const bool free_ = k < Kf && k != chosen[0] && k != chosen[1] && k != chosen[2];
                if (free_ && (key[lap] < v || (key[lap] == v && k < i))) { v = key[lap]; i = k; }
            }
            wave_lexmin(v, i);                                    // S <= Kf: there is always a free disc
            chosen[s] = i;
            if ((i & 63) == lane) {                               // the winning lane writes its disc
                idx[(size_t)b * S + s] = i;
                centers_sel[((size_t)b * S + s) * 2] = cf[i * 2];
                centers_sel[((size_t)b * S + s) * 2 + 1] = cf[i * 2 + 1];
                radii_sel[(size_t)b * S + s] = rf[i];
            }
        }
    }
    if (lane == 0) {
        const T hm = (T)hmin, old = min_h[b];
        min_h[b] = hm < old ? hm : old;
        cert[b] = 0;
        rounds[b] = 0;
    }
}

template <typename T>
__global__ __launch_bounds__(64 * FIELD_WAVES) void obstacle_field_audit_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const int* __restrict__ status, const T* __restrict__ Mk,
    const T* __restrict__ Bk, const T* __restrict__ A, const T* __restrict__ fhat, const T* __restrict__ ghat,
    const T* __restrict__ rho, const T* __restrict__ centers_f, const T* __restrict__ radii_f, int field_stride,
    const T* __restrict__ tw, double gamma, double tol_f, double tol_a, int* __restrict__ idx, T* __restrict__ centers_sel,
    T* __restrict__ radii_sel, int* __restrict__ cert, int* __restrict__ rounds, T* __restrict__ worst_margin,
    int* __restrict__ worst_idx, int* __restrict__ nviol, int Bt, int Kf, int S) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * FIELD_WAVES + (threadIdx.x >> 6);
    if (b >= Bt) return;                                          // (wave-uniform, as every exit below)
    if (cert[b] != 0) return;                                     // decided in an earlier round: nothing is touched
    if (status[b] != BCBF_SOCP_OPTIMAL) {                         // no control to audit
        if (lane == 0) {
            cert[b] = BCBF_FIELD_UNSOLVED;
            worst_margin[b] = std::numeric_limits<T>::quiet_NaN();
            worst_idx[b] = -1;
            nviol[b] = 0;
        }
        return;
    }
    const T* cf = centers_f + (size_t)b * field_stride * Kf * 2;
    const T* rf = radii_f + (size_t)b * field_stride * Kf;
    const double px = (double)x[(size_t)b * 3], py = (double)x[(size_t)b * 3 + 1], th = (double)x[(size_t)b * 3 + 2];
    const double tw0 = (double)tw[0], tw1 = (double)tw[1];
    const double ub[3] = {1.0, (double)y[(size_t)b * 3], (double)y[(size_t)b * 3 + 1]};
    const double rh = (double)rho[b];
    // xdot = fhat + ghat u + M_k ubar, and ubar' B_k ubar: the same for every disc
    double xd[3], Al[9];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        xd[d] = (double)fhat[(size_t)b * 3 + d] + (double)ghat[((size_t)b * 3 + d) * 2] * ub[1]
                + (double)ghat[((size_t)b * 3 + d) * 2 + 1] * ub[2];
        xd[d] += (double)Mk[(size_t)b * 9 + d * 3] + (double)Mk[(size_t)b * 9 + d * 3 + 1] * ub[1]
                 + (double)Mk[(size_t)b * 9 + d * 3 + 2] * ub[2];
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) Al[a] = (double)A[(size_t)b * 9 + a];
    const double bub = quad_form3<T>(ub, Bk + (size_t)b * 9);
    int sel[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) sel[s] = s < S ? idx[(size_t)b * S + s] : -1;

    double wm = INFINITY, vm = INFINITY;             // smallest margin among the unselected discs / among the violators
    int wi = FIELD_NONE, vi = FIELD_NONE, nv = 0;
    double sm[3] = {-INFINITY, -INFINITY, -INFINITY}, sc[3] = {1.0, 1.0, 1.0};    // the slots' margins and scales
#pragma unroll
    for (int lap = 0; lap < FIELD_LAPS; ++lap) {
        const int k = lane + 64 * lap;
        if (k < Kf) {
            double g[3], cst;
            field_row(px, py, th, (double)cf[k * 2], (double)cf[k * 2 + 1], (double)rf[k], tw0, tw1, gamma, g, cst);
            const double E = g[0] * xd[0] + g[1] * xd[1] + g[2] * xd[2] + cst;
            double gAg = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) gAg += g[i] * Al[i * 3 + c] * g[c];
            const double q = bub * gAg;
            const double rs = rh * __builtin_sqrt(q > 0.0 ? q : 0.0);
            const double m = nan_is_lowest(E - rs);
            double scale = 1.0;                                   // max(1, |E|, rho s), a NaN term ignored
            if (__builtin_fabs(E) > scale) scale = __builtin_fabs(E);
            if (rs > scale) scale = rs;
            const bool isslot = k == sel[0] || k == sel[1] || k == sel[2];
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (k == sel[s]) { sm[s] = m; sc[s] = scale; }
            if (!isslot) {
                if (m < wm || (m == wm && k < wi)) { wm = m; wi = k; }
                if (m < -tol_f * scale) {
                    ++nv;
                    if (m < vm || (m == vm && k < vi)) { vm = m; vi = k; }
                }
            }
        }
    }
    wave_lexmin(wm, wi);
    wave_lexmin(vm, vi);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off, 64);
    // the slack-most slot: largest margin, ties to the lower slot
    double bm = -INFINITY, bs = 1.0;
    int bslot = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (s < S) {
            const double m = __shfl(sm[s], sel[s] & 63, 64), scl = __shfl(sc[s], sel[s] & 63, 64);
            if (s == 0 || m > bm) { bm = m; bs = scl; bslot = s; }
        }
    }
    if (lane == 0) {
        worst_margin[b] = (T)wm;
        worst_idx[b] = wi == FIELD_NONE ? -1 : wi;
        nviol[b] = nv;
    }
    if (nv == 0) {
        if (lane == 0) cert[b] = BCBF_FIELD_CERTIFIED;
        return;
    }
    if (bm <= tol_a * bs) {                                       // every slot is active: the working set is full
        if (lane == 0) cert[b] = BCBF_FIELD_FULL;
        return;
    }
    if ((vi & 63) == lane) {                                      // swap the worst violator in for the slack slot
        idx[(size_t)b * S + bslot] = vi;
        centers_sel[((size_t)b * S + bslot) * 2] = cf[vi * 2];
        centers_sel[((size_t)b * S + bslot) * 2 + 1] = cf[vi * 2 + 1];
        radii_sel[(size_t)b * S + bslot] = rf[vi];
        rounds[b] += 1;
    }
}

template <typename T>
__global__ void obstacle_field_commit_kernel(T* __restrict__ x, const T* __restrict__ y, const int* __restrict__ status,
                                             const int* __restrict__ cert, int* __restrict__ status_eff, T dt, T L_true,
                                             int Bt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bt) return;
    const int st = status[b];
    const int eff = cert[b] == BCBF_FIELD_CERTIFIED ? 0 : (st != 0 ? st : BCBF_FIELD_UNCERTIFIED);
    status_eff[b] = eff;
    if (eff == 0 && dt > T(0)) {          // everything else keeps its state: the reference raises ValueError there
        T n0, n1, n2;
        ackermann_euler<T>(x[(size_t)b * 3], x[(size_t)b * 3 + 1], x[(size_t)b * 3 + 2], y[(size_t)b * 3],
                           y[(size_t)b * 3 + 1], dt, L_true, n0, n1, n2);
        x[(size_t)b * 3] = n0; x[(size_t)b * 3 + 1] = n1; x[(size_t)b * 3 + 2] = n2;
    }
}

template <typename T>
static int field_select(const char* entry, const T* x, const T* centers_f, const T* radii_f, int field_stride, const T* tw,
                        int* idx, T* centers_sel, T* radii_sel, T* min_h, int* cert, int* rounds, int Bt, int Kf, int S,
                        void* stream) {
    if (const char* why = field_shape(Bt, Kf, S, field_stride)) return field_einval(entry, why);
    if (!x || !centers_f || !radii_f || !tw) return field_einval(entry, "null x, centers_f, radii_f or tw");
    if (!idx || !centers_sel || !radii_sel) return field_einval(entry, "null idx, centers_sel or radii_sel");
    if (!min_h || !cert || !rounds) return field_einval(entry, "null min_h, cert or rounds");
    hipLaunchKernelGGL((obstacle_field_select_kernel<T>), dim3((Bt + FIELD_WAVES - 1) / FIELD_WAVES), dim3(64 * FIELD_WAVES), 0,
                       (hipStream_t)stream, x, centers_f, radii_f, field_stride, tw, idx, centers_sel, radii_sel, min_h, cert,
                       rounds, Bt, Kf, S);
    return check_launch(entry);
}

template <typename T>
static int field_audit(const char* entry, const T* x, const T* y, const int* status, const T* Mk, const T* Bk, const T* A,
                       const T* fhat, const T* ghat, const T* rho, const T* centers_f, const T* radii_f, int field_stride,
                       const T* tw, T gamma, double tol_f, double tol_a, int* idx, T* centers_sel, T* radii_sel, int* cert,
                       int* rounds, T* worst_margin, int* worst_idx, int* nviol, int Bt, int Kf, int S, void* stream) {
    if (const char* why = field_shape(Bt, Kf, S, field_stride)) return field_einval(entry, why);
    if (!field_finite(tol_f) || tol_f < 0.0) return field_einval(entry, "tol_f must be finite and >= 0");
    if (!field_finite(tol_a) || tol_a < 0.0) return field_einval(entry, "tol_a must be finite and >= 0");
    if (!x || !y || !status) return field_einval(entry, "null x, y or status");
    if (!Mk || !Bk || !A || !fhat || !ghat || !rho) return field_einval(entry, "null Mk, Bk, A, fhat, ghat or rho");
    if (!centers_f || !radii_f || !tw) return field_einval(entry, "null centers_f, radii_f or tw");
    if (!idx || !centers_sel || !radii_sel || !cert || !rounds)
        return field_einval(entry, "null idx, centers_sel, radii_sel, cert or rounds");
    if (!worst_margin || !worst_idx || !nviol) return field_einval(entry, "null worst_margin, worst_idx or nviol");
    hipLaunchKernelGGL((obstacle_field_audit_kernel<T>), dim3((Bt + FIELD_WAVES - 1) / FIELD_WAVES), dim3(64 * FIELD_WAVES), 0,
                       (hipStream_t)stream, x, y, status, Mk, Bk, A, fhat, ghat, rho, centers_f, radii_f, field_stride, tw,
                       (double)gamma, tol_f, tol_a, idx, centers_sel, radii_sel, cert, rounds, worst_margin, worst_idx, nviol,
                       Bt, Kf, S);
    return check_launch(entry);
}

template <typename T>
static int field_commit(const char* entry, T* x, const T* y, const int* status, const int* cert, int* status_eff, T dt,
                        T L_true, int Bt, void* stream) {
    if (Bt <= 0) return field_einval(entry, "Bt <= 0");
    if (!x || !y || !status || !cert || !status_eff) return field_einval(entry, "null x, y, status, cert or status_eff");
    if (!field_finite((double)dt) || dt < T(0)) return field_einval(entry, "dt must be finite and >= 0 (0: no plant step)");
    if (dt > T(0) && (!field_finite((double)L_true) || L_true == T(0)))
        return field_einval(entry, "L_true must be a finite number other than 0");
    hipLaunchKernelGGL((obstacle_field_commit_kernel<T>), dim3((Bt + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y,
                       status, cert, status_eff, dt, L_true, Bt);
    return check_launch(entry);
}

}  // namespace bcbf

extern "C" {
#define BCBF_FIELD(T, SUF)                                                                                                   \
    int bcbf_obstacle_field_select_##SUF(const T* x, const T* centers_f, const T* radii_f, int field_stride, const T* tw,    \
                                         int* idx, T* centers_sel, T* radii_sel, T* min_h, int* cert, int* rounds, int Bt,   \
                                         int Kf, int S, void* stream) {                                                      \
        return bcbf::field_select<T>("bcbf_obstacle_field_select_" #SUF, x, centers_f, radii_f, field_stride, tw, idx,       \
                                     centers_sel, radii_sel, min_h, cert, rounds, Bt, Kf, S, stream);                        \
    }                                                                                                                        \
    int bcbf_obstacle_field_audit_##SUF(const T* x, const T* y, const int* status, const T* Mk, const T* Bk, const T* A,     \
                                        const T* fhat, const T* ghat, const T* rho, const T* centers_f, const T* radii_f,    \
                                        int field_stride, const T* tw, T gamma, double tol_f, double tol_a, int* idx,        \
                                        T* centers_sel, T* radii_sel, int* cert, int* rounds, T* worst_margin,               \
                                        int* worst_idx, int* nviol, int Bt, int Kf, int S, void* stream) {                   \
        return bcbf::field_audit<T>("bcbf_obstacle_field_audit_" #SUF, x, y, status, Mk, Bk, A, fhat, ghat, rho, centers_f,  \
                                    radii_f, field_stride, tw, gamma, tol_f, tol_a, idx, centers_sel, radii_sel, cert,       \
                                    rounds, worst_margin, worst_idx, nviol, Bt, Kf, S, stream);                              \
    }                                                                                                                        \
    int bcbf_obstacle_field_commit_##SUF(T* x, const T* y, const int* status, const int* cert, int* status_eff, T dt,        \
                                         T L_true, int Bt, void* stream) {                                                   \
        return bcbf::field_commit<T>("bcbf_obstacle_field_commit_" #SUF, x, y, status, cert, status_eff, dt, L_true, Bt,     \
                                     stream);                                                                                \
    }
BCBF_FIELD(float, f32)
BCBF_FIELD(double, f64)
#undef BCBF_FIELD
}
