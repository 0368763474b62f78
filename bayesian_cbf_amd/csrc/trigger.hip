// Self-triggering interval of every instance in one launch (bcbf_trigger_interval): the high-probability Lipschitz constant
// L_fh of the learned dynamics over a cloud of test points around x and the time tau for which the last control stays safe.
//
// The reference's unicycle_trigger_interval_compute (bayes_cbf/trigger_interval.py:128-167) does this per logged step in a
// Python loop over all Nte x Nte ordered pairs of a test grid.  The O(Nte^2) part is
//   Lkd[j] = max over ordered pairs (a, b) of  uBu * 2 ls_j^-4 (X_a - X_b)_j sf^2 exp(-1/2 sum_d ((X_a - X_b)_d / ls_d)^2)
// (rbf_d3_knl_d_x_xp_i as executed, :41-42; sf squared although it is the output scale already, :33).  Ordered pairs carry both
// signs of (X_a - X_b)_j, so the maximum is |uBu| 2 ls_j^-4 sf^2 max over UNORDERED pairs of |d_j| e(a, b): half the work, one
// exponential per pair for all n components.  Everything after it (maxk, Lfs, Lfh, tau, :143-165) is a few dozen flops.
//
// One workgroup per instance.  The test points X = off + x are formed in the working type and kept in LDS (stride 4 for n = 3:
// one 16-byte read per point in fp32).  The points are cut into tiles of 64; a work unit is a tile pair (A, Bt = A + S mod T),
// S = 0 .. T/2 (circulant: every unordered tile pair exactly once, the diagonal tiles as full squares), dealt round-robin to
// the four waves.  Inside a unit lane l owns point 64 A + l in registers and every lane walks the points of tile Bt together:
// the LDS address is wave-uniform (a broadcast read with an immediate offset, no address arithmetic, no bank conflict).  Per
// pair: n subtractions, n multiplies, n fused squares, one exponential, n multiplies and n maxima -- the loop is bound by the
// vector and transcendental issue rate, not by LDS or HBM.  Running maxima stay in registers; wave reduction by shuffles, the
// four waves through LDS, no float atomics.  Lane 0 finishes the instance in fp64 for both precisions (the closed forms cost
// nothing, and log(1 + y) for small y would otherwise lose what the pair maximum kept).
#include "bcbf_common.h"
#include <stdio.h>

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

template <typename T, int NS>
__global__ void __launch_bounds__(TI_THREADS)
trigger_interval_kernel(const T* __restrict__ x, const T* __restrict__ off, const T* __restrict__ ls, const T* __restrict__ sf,
                        const T* __restrict__ Adiag, const T* __restrict__ uBu, const T* __restrict__ xvel, const T* __restrict__ Lh,
                        double r, double deltaL, double zeta, double L_alpha, T* __restrict__ Lkd, T* __restrict__ Lfh,
                        T* __restrict__ tau, int per_instance_hyper, int N) {
    constexpr int ST = ti_stride(NS);
    extern __shared__ __attribute__((aligned(16))) unsigned char ti_raw[];
    __shared__ T ti_red[TI_WAVES][NS];
    T* pts = reinterpret_cast<T*>(ti_raw);
    const int b = blockIdx.x, hb = per_instance_hyper ? b : 0;
    T xb[NS], q[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        xb[j] = x[(size_t)b * NS + j];
        q[j] = T(ti_qscale<T>()) / ls[(size_t)hb * NS + j];
    }
    for (int i = threadIdx.x; i < N; i += TI_THREADS) {
#pragma unroll
        for (int j = 0; j < NS; ++j) pts[i * ST + j] = off[(size_t)i * NS + j] + xb[j];
    }
    __syncthreads();

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
        if (lane == 0) ti_red[wave][j] = mx[j];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;

    // the closed forms of trigger_interval.py:129-165, in fp64
    const double E = NS, uB = (double)uBu[b], sfv = (double)sf[hb], sf2 = sfv * sfv;
    double l2[NS], lkd[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double m = 0.0;
        for (int w = 0; w < TI_WAVES; ++w) m = fmax(m, (double)ti_red[w][j]);
        const double l = (double)ls[(size_t)hb * NS + j];
        l2[j] = l * l;
        lkd[j] = fabs(uB) * (2.0 / (l2[j] * l2[j])) * sf2 * m;
        Lkd[(size_t)b * NS + j] = (T)lkd[j];
    }
    const double c1 = sqrt(2.0 * log(2.0 * (E * E) / deltaL)), c2 = 12.0 * sqrt(6.0 * E);
    double sum = 0.0;
#pragma unroll
    for (int ei = 0; ei < NS; ++ei) {
        const double a = (double)Adiag[(size_t)hb * NS + ei];
#pragma unroll
        for (int ej = 0; ej < NS; ++ej) {
            const double maxk = a * uB * (sf2 / l2[ej]);
            const double v = c1 * maxk + c2 * fmax(maxk, sqrt(r * a * lkd[ej]));      // Eq. (11) of the paper (:148-149)
            sum += v * v;
        }
    }
    const double L = sqrt(sum) / E;
    Lfh[b] = (T)L;
    // IEEE results pass through: xvel == 0 gives tau = inf, as the reference's numpy does
    tau[b] = (T)((1.0 / L) * log(1.0 + L * zeta / ((L + L_alpha) * (double)Lh[b] * (double)xvel[b])));
}

template <typename T>
static int trigger_args_ok(const char* entry, const void* x, const void* off, const void* ls, const void* sf, const void* Adiag,
                           const void* uBu, const void* xvel, const void* Lh, const void* Lkd, const void* Lfh, const void* tau, int B,
                           int Bh, int Nte, int n) {
    static thread_local char msg[240];
    const char* why = nullptr;
    if (!x || !off || !ls || !sf || !Adiag || !uBu || !xvel || !Lh) why = "null input pointer";
    else if (!Lkd || !Lfh || !tau) why = "null output pointer";
    else if (B < 1) why = "B < 1";
    else if (Bh != 1 && Bh != B) why = "the hyper-parameters' leading extent Bh must be 1 or B";
    else if (n < 1 || n > 3) why = "need 1 <= n <= 3";
    else if (Nte < 1) why = "Nte < 1";
    else if ((size_t)Nte * ti_stride(n) * sizeof(T) > TI_MAX_LDS) why = "Nte too large (the test points of one instance are kept in LDS)";
    if (!why) return 1;
    snprintf(msg, sizeof(msg), "%s: %s (B=%d Bh=%d Nte=%d n=%d)", entry, why, B, Bh, Nte, n);
    set_error_message(msg);
    return 0;
}

template <typename T, int NS>
static void trigger_launch_n(const T* x, const T* off, const T* ls, const T* sf, const T* Adiag, const T* uBu, const T* xvel, const T* Lh,
                             double r, double deltaL, double zeta, double L_alpha, T* Lkd, T* Lfh, T* tau, int B, int Bh, int Nte,
                             void* stream) {
    const size_t lds = (size_t)Nte * ti_stride(NS) * sizeof(T);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)trigger_interval_kernel<T, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((trigger_interval_kernel<T, NS>), dim3(B), dim3(TI_THREADS), lds, (hipStream_t)stream, x, off, ls, sf, Adiag, uBu,
                       xvel, Lh, r, deltaL, zeta, L_alpha, Lkd, Lfh, tau, Bh == B && B > 1 ? 1 : 0, Nte);
}

template <typename T>
static int launch_trigger_interval(const char* entry, const T* x, const T* off, const T* ls, const T* sf, const T* Adiag, const T* uBu,
                                   const T* xvel, const T* Lh, double r, double deltaL, double zeta, double L_alpha, T* Lkd, T* Lfh,
                                   T* tau, int B, int Bh, int Nte, int n, void* stream) {
    if (!trigger_args_ok<T>(entry, x, off, ls, sf, Adiag, uBu, xvel, Lh, Lkd, Lfh, tau, B, Bh, Nte, n)) return BCBF_EINVAL;
    if (n == 1) trigger_launch_n<T, 1>(x, off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL, zeta, L_alpha, Lkd, Lfh, tau, B, Bh, Nte, stream);
    else if (n == 2) trigger_launch_n<T, 2>(x, off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL, zeta, L_alpha, Lkd, Lfh, tau, B, Bh, Nte, stream);
    else trigger_launch_n<T, 3>(x, off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL, zeta, L_alpha, Lkd, Lfh, tau, B, Bh, Nte, stream);
    return check_launch(entry);
}

}  // namespace bcbf

extern "C" int bcbf_trigger_interval_f32(const float* x, const float* off, const float* ls, const float* sf, const float* Adiag,
                                         const float* uBu, const float* xvel, const float* Lh, double r, double deltaL, double zeta,
                                         double L_alpha, float* Lkd, float* Lfh, float* tau, int B, int Bh, int Nte, int n, void* stream) {
    return bcbf::launch_trigger_interval("bcbf_trigger_interval_f32", x, off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL, zeta, L_alpha, Lkd,
                                         Lfh, tau, B, Bh, Nte, n, stream);
}
extern "C" int bcbf_trigger_interval_f64(const double* x, const double* off, const double* ls, const double* sf, const double* Adiag,
                                         const double* uBu, const double* xvel, const double* Lh, double r, double deltaL, double zeta,
                                         double L_alpha, double* Lkd, double* Lfh, double* tau, int B, int Bh, int Nte, int n,
                                         void* stream) {
    return bcbf::launch_trigger_interval("bcbf_trigger_interval_f64", x, off, ls, sf, Adiag, uBu, xvel, Lh, r, deltaL, zeta, L_alpha, Lkd,
                                         Lfh, tau, B, Bh, Nte, n, stream);
}
