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
// The pair loop (ti_pair_max) and the closed forms (ti_closed_forms) are in trigger_pairs.h: the fused event kernel of the
// self-triggered loop (trigger_step.hip) runs the same code.
#include "trigger_pairs.h"
#include <stdio.h>

namespace bcbf {

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

    ti_pair_max<T, NS>(pts, N, q, ti_red);
    __syncthreads();
    if (threadIdx.x != 0) return;

    double lkd[NS], tv;
    const double L = ti_closed_forms<T, NS>(ti_red, ls + (size_t)hb * NS, (double)sf[hb], Adiag + (size_t)hb * NS, (double)uBu[b],
                                            (double)Lh[b], (double)xvel[b], r, deltaL, zeta, L_alpha, lkd, tv);
#pragma unroll
    for (int j = 0; j < NS; ++j) Lkd[(size_t)b * NS + j] = (T)lkd[j];
    Lfh[b] = (T)L;
    tau[b] = (T)tv;
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
