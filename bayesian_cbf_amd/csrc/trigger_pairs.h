// The two halves of the trigger-interval computation that bcbf_trigger_interval (trigger.hip) and the fused event kernel
// bcbf_unicycle_trigger_step (trigger_step.hip) share: the pair maximum over the test points of one instance held in LDS, and the
// closed forms that turn it into Lkd, Lfh and tau.  What the loop computes and why it is laid out so: the head of trigger.hip.
#pragma once
#include "bcbf_common.h"

namespace bcbf {

constexpr int TI_THREADS = 256;
constexpr int TI_WAVES = TI_THREADS / 64;
constexpr int TI_TILE = 64;
constexpr size_t TI_MAX_LDS = 160 * 1024 - 256;      // the points of one instance (the static reduction scratch comes on top)

__host__ __device__ constexpr int ti_stride(int n) { return n == 3 ? 4 : n; }

// e(s) = exp(-s_natural): fp32 takes s in units of ln 2 (the scale is folded into the per-axis factor) and one v_exp_f32
__device__ inline float ti_expneg(float s) { return __builtin_amdgcn_exp2f(-s); }
__device__ inline double ti_expneg(double s) { return exp_neg64(s < 800.0 ? s : 800.0); }     // exp(-800) == 0 in fp64
__device__ inline float ti_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ inline double ti_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T> __host__ __device__ constexpr double ti_qscale() {           // q_j = ti_qscale / ls_j, s = sum (d_j q_j)^2
    return sizeof(T) == 4 ? 0.8493218002880191 /* sqrt(log2(e) / 2) */ : 0.7071067811865476 /* sqrt(1 / 2) */;
}

// max over the unordered pairs (a, b) of the N points pts[N][ti_stride(NS)] (LDS, written and synchronised by the caller) of
// |d_j| e(a, b), d = X_a - X_b, per component j; q[j] = ti_qscale<T>() / ls_j.  Every thread of the workgroup calls it; each wave
// leaves its maxima in red[wave][j].  The caller synchronises before it reads red.
template <typename T, int NS>
__device__ inline void ti_pair_max(const T* pts, int N, const T (&q)[NS], T (*red)[NS]) {
    constexpr int ST = ti_stride(NS);
    const int Tn = (N + TI_TILE - 1) / TI_TILE;
    // S = 0 .. (Tn-1)/2 for every A; for even Tn the half row S = Tn/2, A < Tn/2 (the other half would repeat those tile pairs)
    const int units = Tn * ((Tn - 1) / 2 + 1) + (Tn % 2 == 0 ? Tn / 2 : 0);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    T mx[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) mx[j] = T(0);           // the pairs a == b are part of the maximum: Lkd >= 0
    for (int u = wave; u < units; u += TI_WAVES) {
        const int S = u / Tn, A = u - S * Tn;
        const int Bt = A + S >= Tn ? A + S - Tn : A + S;
        const int ia = min(A * TI_TILE + lane, N - 1);   // (lanes past the last point repeat it: a pair that exists anyway)
        T xa[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) xa[j] = pts[ia * ST + j];
        const T* pb = pts + (size_t)Bt * TI_TILE * ST;
        const int nb = min(TI_TILE, N - Bt * TI_TILE);
#pragma unroll 4
        for (int k = 0; k < nb; ++k) {
            T d[NS], s = T(0);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                d[j] = xa[j] - pb[k * ST + j];
                const T t = d[j] * q[j];
                s = j == 0 ? t * t : ti_fma(t, t, s);
            }
            const T e = ti_expneg(s);
#pragma unroll
            for (int j = 0; j < NS; ++j) mx[j] = fmax(mx[j], fabs(d[j]) * e);
        }
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx[j] = fmax(mx[j], __shfl_xor(mx[j], o, 64));
        if (lane == 0) red[wave][j] = mx[j];
    }
}

// The closed forms of trigger_interval.py:129-165 in fp64, by one thread, from the waves' pair maxima: lkd[NS] (returned as
// doubles; the caller stores them), Lfh (the return value) and tau.  ls, Adiag: the instance's rows; sfv, uB, Lh, xvel: its scalars
// as the working type holds them.  IEEE results pass through: xvel == 0 gives tau = inf, as the reference's numpy does.
template <typename T, int NS>
__device__ inline double ti_closed_forms(const T (*red)[NS], const T* ls, double sfv, const T* Adiag, double uB, double Lh, double xvel,
                                         double r, double deltaL, double zeta, double L_alpha, double (&lkd)[NS], double& tau) {
    const double E = NS, sf2 = sfv * sfv;
    double l2[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double m = 0.0;
        for (int w = 0; w < TI_WAVES; ++w) m = fmax(m, (double)red[w][j]);
        const double l = (double)ls[j];
        l2[j] = l * l;
        lkd[j] = fabs(uB) * (2.0 / (l2[j] * l2[j])) * sf2 * m;
    }
    const double c1 = sqrt(2.0 * log(2.0 * (E * E) / deltaL)), c2 = 12.0 * sqrt(6.0 * E);
    double sum = 0.0;
#pragma unroll
    for (int ei = 0; ei < NS; ++ei) {
        const double a = (double)Adiag[ei];
#pragma unroll
        for (int ej = 0; ej < NS; ++ej) {
            const double maxk = a * uB * (sf2 / l2[ej]);
            const double v = c1 * maxk + c2 * fmax(maxk, sqrt(r * a * lkd[ej]));      // Eq. (11) of the paper (:148-149)
            sum += v * v;
        }
    }
    const double L = sqrt(sum) / E;
    tau = (1.0 / L) * log(1.0 + L * zeta / ((L + L_alpha) * Lh * xvel));
    return L;
}

}  // namespace bcbf
