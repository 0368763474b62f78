// The obstacle-field commit on a plant DRAWN FROM THE MODEL'S OWN POSTERIOR (bcbf_obstacle_field_commit_sampled): what
// bcbf_obstacle_field_commit does -- the effective status, and the step of exactly the certified instances -- with the step taken on
// one draw of  xdot | x, u ~ N(fhat + ghat u + M_k ubar, (ubar' B_k ubar) A)  (fu_func_gp(u), unicycle_move_to_pose.py:262-275,
// drawn as GaussianProcessBase.sample draws, gp_algebra.py:33-34), and the condition of EVERY disc of the field evaluated on that
// draw (cbc1.py:10-14; one un-relaxed cone per obstacle, `_cbcs`, unicycle_move_to_pose.py:901-920).  The working-set solve puts at
// most three cones into the program and the audit looks at the others at the posterior mean and spread only; here every disc sees
// the draw, so a rollout can count the risk of the tightest cone -- what max_risk promises, per cone -- and of "any disc violated on
// the draw", which only a union bound covers.
// The audit's mapping: one wave per instance, four waves per workgroup that never talk to each other, lanes stride over the discs
// k = lane + 64 lap.  fp64 for both entry precisions from the inputs as stored, every output rounded to T once.  No LDS, no scratch
// (register arrays indexed by constants only; the build's resource guard checks it).
#include "obstacle_field.h"

namespace bcbf {

template <typename T>
struct FieldPlant {
    T* x;                                            // [Bt,3] advanced in place where status_eff = 0 and dt > 0
    const T* y;
    const int *status, *cert;
    const T *Mk, *Bk, *A, *fhat, *ghat, *rho, *centers_f, *radii_f, *tw;
    const int* idx;                                  // [Bt,S] the working set (what "unselected" means)
    const T* z;                                      // [Bt,3] the caller's standard normals
    int* status_eff;
    T *xdot_s, *cbc_min;                             // this step's outputs
    int *cbc_argmin, *tight_idx;
    T* cbc_tight;
    int* nneg;
    int *solved, *viol_tight, *viol_any, *viol_unselected, *viol_discs;      // the accumulators
    T* min_cbc;
    double gamma, dt;
    int field_stride, Bt, Kf, S;
};

template <typename T>
__global__ __launch_bounds__(64 * FIELD_WAVES) void field_plant_kernel(const FieldPlant<T> a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * FIELD_WAVES + (threadIdx.x >> 6);
    if (b >= a.Bt) return;                                        // (wave-uniform, as the exit below)
    const int st = a.status[b];
    const int eff = a.cert[b] == BCBF_FIELD_CERTIFIED ? 0 : (st != 0 ? st : BCBF_FIELD_UNCERTIFIED);
    if (eff != 0) {                       // keeps its state (the reference raises ValueError there); its accumulators stay
        if (lane == 0) {
            a.status_eff[b] = eff;
            a.xdot_s[(size_t)b * 3] = T(0); a.xdot_s[(size_t)b * 3 + 1] = T(0); a.xdot_s[(size_t)b * 3 + 2] = T(0);
            a.cbc_min[b] = T(0); a.cbc_tight[b] = T(0);
            a.cbc_argmin[b] = -1; a.tight_idx[b] = -1;
            a.nneg[b] = 0;
        }
        return;
    }
    const T* cf = a.centers_f + (size_t)b * a.field_stride * a.Kf * 2;
    const T* rf = a.radii_f + (size_t)b * a.field_stride * a.Kf;
    const double x0[3] = {(double)a.x[(size_t)b * 3], (double)a.x[(size_t)b * 3 + 1], (double)a.x[(size_t)b * 3 + 2]};
    const double tw0 = (double)a.tw[0], tw1 = (double)a.tw[1];
    const double ub[3] = {1.0, (double)a.y[(size_t)b * 3], (double)a.y[(size_t)b * 3 + 1]};
    const double rh = (double)a.rho[b];
    const double zz[3] = {(double)a.z[(size_t)b * 3], (double)a.z[(size_t)b * 3 + 1], (double)a.z[(size_t)b * 3 + 2]};
    // the mean fhat + ghat u + M_k ubar as the audit forms it, ubar' B_k ubar, and the draw on top of the mean
    const double bub = quad_form3<T>(ub, a.Bk + (size_t)b * 9);
    const double rs = __builtin_sqrt(bub > 0.0 ? bub : 0.0);
    double LA[3][3], Al[9], xm[3], xd[3];
    psd_chol3<T>(a.A + (size_t)b * 9, LA);
#pragma unroll
    for (int i = 0; i < 9; ++i) Al[i] = (double)a.A[(size_t)b * 9 + i];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        xm[d] = (double)a.fhat[(size_t)b * 3 + d] + (double)a.ghat[((size_t)b * 3 + d) * 2] * ub[1]
                + (double)a.ghat[((size_t)b * 3 + d) * 2 + 1] * ub[2];
        xm[d] += (double)a.Mk[(size_t)b * 9 + d * 3] + (double)a.Mk[(size_t)b * 9 + d * 3 + 1] * ub[1]
                 + (double)a.Mk[(size_t)b * 9 + d * 3 + 2] * ub[2];
        xd[d] = posterior_draw(xm[d], rs, LA[d], zz);
    }
    int sel[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) sel[s] = s < a.S ? a.idx[(size_t)b * a.S + s] : -1;

    // every disc at the state BEFORE the step: the condition on the draw, and the audit's margin (which cone is the tight one)
    double cm = INFINITY, mm = INFINITY, ct = 0.0;   // smallest condition / smallest margin and the condition of that disc
    int ci = FIELD_NONE, mi = FIELD_NONE, nn = 0, nu = 0;
#pragma unroll
    for (int lap = 0; lap < FIELD_LAPS; ++lap) {
        const int k = lane + 64 * lap;
        if (k < a.Kf) {
            double g[3], cst;
            field_row(x0[0], x0[1], x0[2], (double)cf[k * 2], (double)cf[k * 2 + 1], (double)rf[k], tw0, tw1, a.gamma, g, cst);
            const double cb = cbc_on(1.0, g, xd, cst);
            const double c = cb - cb == 0.0 ? cb : -INFINITY;     // anything non-finite is a violation and takes the minimum
            const double E = g[0] * xm[0] + g[1] * xm[1] + g[2] * xm[2] + cst;
            double gAg = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) gAg += g[i] * Al[i * 3 + j] * g[j];
            const double q = bub * gAg;
            const double m = nan_is_lowest(E - rh * __builtin_sqrt(q > 0.0 ? q : 0.0));
            if (c < cm || (c == cm && k < ci)) { cm = c; ci = k; }
            if (m < mm || (m == mm && k < mi)) { mm = m; mi = k; ct = c; }
            if (c < 0.0) {
                ++nn;
                if (k != sel[0] && k != sel[1] && k != sel[2]) ++nu;
            }
        }
    }
    wave_lexmin(cm, ci);
    wave_lexmin(mm, mi);
    ct = __shfl(ct, mi & 63, 64);                    // the wave's tightest disc is the tightest of the lane that owns it
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nn += __shfl_xor(nn, off, 64);
        nu += __shfl_xor(nu, off, 64);
    }
    if (lane == 0) {
        a.status_eff[b] = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a.xdot_s[(size_t)b * 3 + d] = (T)xd[d];
            if (a.dt > 0.0) a.x[(size_t)b * 3 + d] = (T)(x0[d] + xd[d] * a.dt);
        }
        const T cmT = (T)cm, old = a.min_cbc[b];
        a.cbc_min[b] = cmT;
        a.cbc_argmin[b] = ci;
        a.tight_idx[b] = mi;
        a.cbc_tight[b] = (T)ct;
        a.nneg[b] = nn;
        a.solved[b] += 1;
        a.viol_tight[b] += ct < 0.0 ? 1 : 0;
        a.viol_any[b] += nn > 0 ? 1 : 0;
        a.viol_unselected[b] += nu > 0 ? 1 : 0;
        a.viol_discs[b] += nn;
        a.min_cbc[b] = cmT < old ? cmT : old;
    }
}

template <typename T>
static int field_plant(const char* entry, const FieldPlant<T>& a, void* stream) {
    if (const char* why = field_shape(a.Bt, a.Kf, a.S, a.field_stride)) return field_einval(entry, why);
    if (!field_finite(a.gamma)) return field_einval(entry, "gamma must be finite");
    if (!field_finite(a.dt) || a.dt < 0.0) return field_einval(entry, "dt must be finite and >= 0 (0: the state stays)");
    if (!a.x || !a.y || !a.status || !a.cert) return field_einval(entry, "null x, y, status or cert");
    if (!a.Mk || !a.Bk || !a.A || !a.fhat || !a.ghat || !a.rho) return field_einval(entry, "null Mk, Bk, A, fhat, ghat or rho");
    if (!a.centers_f || !a.radii_f || !a.tw || !a.idx || !a.z) return field_einval(entry, "null centers_f, radii_f, tw, idx or z");
    if (!a.status_eff || !a.xdot_s || !a.cbc_min || !a.cbc_argmin || !a.tight_idx || !a.cbc_tight || !a.nneg)
        return field_einval(entry, "null status_eff, xdot_s, cbc_min, cbc_argmin, tight_idx, cbc_tight or nneg");
    if (!a.solved || !a.viol_tight || !a.viol_any || !a.viol_unselected || !a.viol_discs || !a.min_cbc)
        return field_einval(entry, "null solved, viol_tight, viol_any, viol_unselected, viol_discs or min_cbc");
    hipLaunchKernelGGL((field_plant_kernel<T>), dim3((a.Bt + FIELD_WAVES - 1) / FIELD_WAVES), dim3(64 * FIELD_WAVES), 0,
                       (hipStream_t)stream, a);
    return check_launch(entry);
}

}  // namespace bcbf

extern "C" {
#define BCBF_FIELD_PLANT(T, SUF)                                                                                             \
    int bcbf_obstacle_field_commit_sampled_##SUF(                                                                            \
        T* x, const T* y, const int* status, const int* cert, const T* Mk, const T* Bk, const T* A, const T* fhat,           \
        const T* ghat, const T* rho, const T* centers_f, const T* radii_f, int field_stride, const T* tw, T gamma,           \
        const int* idx, const T* z, int* status_eff, T* xdot_s, T* cbc_min, int* cbc_argmin, int* tight_idx, T* cbc_tight,   \
        int* nneg, int* solved, int* viol_tight, int* viol_any, int* viol_unselected, int* viol_discs, T* min_cbc, T dt,     \
        int Bt, int Kf, int S, void* stream) {                                                                               \
        const bcbf::FieldPlant<T> a = {x, y, status, cert, Mk, Bk, A, fhat, ghat, rho, centers_f, radii_f, tw, idx, z,       \
                                       status_eff, xdot_s, cbc_min, cbc_argmin, tight_idx, cbc_tight, nneg, solved,          \
                                       viol_tight, viol_any, viol_unselected, viol_discs, min_cbc, (double)gamma, (double)dt, \
                                       field_stride, Bt, Kf, S};                                                             \
        return bcbf::field_plant<T>("bcbf_obstacle_field_commit_sampled_" #SUF, a, stream);                                  \
    }
BCBF_FIELD_PLANT(float, f32)
BCBF_FIELD_PLANT(double, f64)
#undef BCBF_FIELD_PLANT
}
