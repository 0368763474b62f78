// K1 (dense kernel-matrix build, for callers that want K_b itself) and the C entry points of K1 + K2 (+ packing): every
// refit entry point, the argument checks and the choice of the launch form (refit_forms.h).  The factorization kernels and
// their launchers are refit_mfma.hip (fp32) and refit_mfma64.hip (fp64) -- blocked left-looking Cholesky, one workgroup per
// instance -- and refit_wave64.hip (one, two, four or eight waves per instance), all writing the packed triangular operator
// the per-step kernel streams (bcbf.h "Lop").
#include <atomic>
#include "refit_forms.h"

namespace bcbf {

template <typename T> __device__ inline T texp2(T x);
template <> __device__ inline float texp2<float>(float x) { return expf(x); }
template <> __device__ inline double texp2<double>(double x) { return exp(x); }


// --------------------------------------------------------------------------------------------
// K1 alone: dense K_b (API completeness / parity tests)
template <typename T>
__global__ void kb_build_kernel(const T* __restrict__ X, const T* __restrict__ UH, const T* __restrict__ Bm,
                                const T* __restrict__ ell, const T* __restrict__ s2p, const T* __restrict__ jitter,
                                T* __restrict__ Kb, int N, int n, int C, const T* __restrict__ lin, int kind) {
    const int b = blockIdx.y;
    const int i = blockIdx.x;
    const T* Xb = X + (size_t)b * N * n;
    const T* UHb = UH + (size_t)b * N * C;
    const T* Bmb = Bm + (size_t)b * C * C;
    T ub[BCBF_MAX_TASK_DIM];                           // (1+m) columns, or the (1+m) n of the expanded CoGP system
#pragma unroll
    for (int c = 0; c < BCBF_MAX_TASK_DIM; ++c) {
        T s = T(0);
        if (c < C) for (int a = 0; a < C; ++a) s += UHb[(size_t)i * C + a] * Bmb[a * C + c];
        ub[c] = s;
    }
    const T s2 = s2p[b];
    const T linv = lin != nullptr ? lin[b] : T(0);        // optional linear part: k = s2 (exp(..) + lin x'x')
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        T d2 = T(0), uu = T(0), dot = T(0);
        for (int d = 0; d < n; ++d) {
            const T z = (Xb[(size_t)i * n + d] - Xb[(size_t)j * n + d]) / ell[(size_t)b * n + d];
            d2 += z * z;
            dot += Xb[(size_t)i * n + d] * Xb[(size_t)j * n + d];
        }
#pragma unroll
        for (int a = 0; a < BCBF_MAX_TASK_DIM; ++a)
            if (a < C) uu += ub[a] * UHb[(size_t)j * C + a];
        T shape, dshape_;                                   // (bcbf_common.h: kernel_shape -- RBF | Matern-5/2 | their product)
        kernel_shape(kind, d2, [](T v) { return texp2<T>(v); }, shape, dshape_);
        T val = s2 * (shape + linv * dot) * uu;
        if (i == j && jitter) val += jitter[(size_t)b * N + i];
        Kb[((size_t)b * N + i) * N + j] = val;
    }
}

template <typename T>
static int launch_kb_build(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter,
                           T* Kb, int Bt, int N, int n, int m, void* stream, const T* lin = nullptr, int kind = 0) {
    if (Bt <= 0) return BCBF_OK;
    if (!X || !UH || !Bm || !ell || !s2 || !Kb) return BCBF_EINVAL;
    if (N < 1 || n < 1 || n > BCBF_MAX_STATE_DIM || m < 1 || m + 1 > BCBF_MAX_TASK_DIM) return BCBF_EINVAL;
    hipLaunchKernelGGL((kb_build_kernel<T>), dim3(N, Bt), dim3(256), 0, (hipStream_t)stream, X, UH, Bm, ell, s2,
                       jitter, Kb, N, n, m + 1, lin, kind);
    return check_launch("kb_build");
}

}  // namespace bcbf

extern "C" {
size_t bcbf_lop_elems_f32(int N) { return bcbf::lop_elems<4>(bcbf::round_up(N, bcbf::NB)); }
size_t bcbf_lop_elems_f64(int N) { return bcbf::lop_elems<2>(bcbf::round_up(N, bcbf::NB)); }

int bcbf_kb_build_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                      const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<float>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream);
}
int bcbf_kb_build_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                      const double* jitter, double* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<double>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream);
}
int bcbf_kb_build_rbflin_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                             const float* lin, const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<float>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream, lin);
}
int bcbf_kb_build_rbflin_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                             const double* lin, const double* jitter, double* Kb, int Bt, int N, int n, int m,
                             void* stream) {
    return bcbf::launch_kb_build<double>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream, lin);
}
int bcbf_kb_build_matern52_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                               const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<float>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream, nullptr, 1);
}
int bcbf_kb_build_matern52_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                               const double* jitter, double* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<double>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream, nullptr, 1);
}
int bcbf_kb_build_rbfm52_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                             const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<float>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream, nullptr, 2);
}
int bcbf_kb_build_rbfm52_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                             const double* jitter, double* Kb, int Bt, int N, int n, int m, void* stream) {
    return bcbf::launch_kb_build<double>(X, UH, Bm, ell, s2, jitter, Kb, Bt, N, n, m, stream, nullptr, 2);
}
}

// --------------------------------------------------------------------------------------------
// K1 + K2 (+ packing): which form runs, and the one path every refit entry point takes to it
namespace bcbf {

// Notation: Np = N padded to 32, nb = Np / 32 block columns, dense = a dense input or output, cus = compute units.
// All measurements: MI355X, 256 CUs, ms unless said (tools/bench_refit_forms.py, tools/dev/check_refit_team.py,
// tools/dev/time_refit_one.py).
const char* choose_refit_plan(bool f64, int Bt, int N, int cus, bool has_Kdense, bool has_Ldense, int kind, int form,
                              RefitPlan* plan) {
    const int base = form & 0xf, sup_field = form & 0x30, occ_field = form & 0xc0;
    if (form < 0 || form > 0xff || base > REFIT_TEAM8 || sup_field == 0x30 || occ_field == 0xc0)
        return "refit: form is not a BCBF_FORM_* value";
    if (kind < 0 || kind >= BCBF_KINDS) return "refit: kernel_kind is not 0 (RBF), 1 (Matern-5/2) or 2 (RBF x Matern-5/2)";
    if (N < 1) return "refit: N < 1";
    const int Np = round_up(N, NB), nb = Np / NB;
    const bool dense = has_Kdense || has_Ldense;
    int f = base;
    if (kind != 0) {
        // the opt-in data kernels have one form, the team of eight
        if (f != REFIT_AUTO && f != REFIT_TEAM8) return "refit: the Matern-5/2 data kernels run as BCBF_FORM_TEAM8 only";
        if (has_Kdense) return "refit: Kdense with kernel_kind != 0";
        f = REFIT_TEAM8;
    } else if (f == REFIT_AUTO) {
        // A team of eight waves per instance (one chain wave, seven bulk waves; one workgroup per CU at a time) while ONE
        // round of workgroups holds the batch, two rounds from N = 512 on, four from 1024 with a dense side (without:
        // 1024 x 1024 team / one wave with super-panels, fp32 6.67 / 5.29, fp64 13.2 / 12.8) -- team / best other form,
        // fp32: 1 x 512: 0.27 / 0.71, 256 x 512: 0.30 / 0.86, 512 x 512: 0.61 / 0.93, 1024 x 512: 1.22 / 1.04, 1 x 1024:
        // 1.31 / 2.81, 512 x 1024: 3.32 / 5.89, 256 x 256: 0.108 / 0.140, 512 x 256: 0.21 / 0.16, 256 x 128: 0.047 / 0.045;
        // fp64: 1 x 512: 0.43 / 0.90, 256 x 512: 0.52 / 1.12, 512 x 512: 1.04 / 1.55, 1 x 1024: 2.31 / 3.57, 1 x 2048:
        // 16.8 / 19.3, 256 x 256: 0.173 / 0.219.  (N <= 2048: beyond, no better than the workgroup form -- 1 x 4096 fp64:
        // 128 / 125.)
        const bool team8 = nb <= 64 && ((Np >= 256 && Bt <= cus) || (Np >= 512 && Bt <= 2 * cus) ||
                                        (Np >= 1024 && Bt <= (dense ? 4 : 2) * cus));
        // ... of four waves (two workgroups per CU) for cus < batch <= 2 cus at 256 <= N <= 512: 512 x 256 fp64 0.259 (two
        // waves per instance) / 0.330 (team of eight, two rounds) / 0.210, fp32 0.162 / - / 0.136; 512 x 512 fp32 0.62
        // (team of eight, two rounds) / 0.53
        const bool team4 = nb <= 16 && Np >= 256 && Bt > cus && Bt <= 2 * cus && !has_Kdense;
        // Two waves per instance (the serial chain of diagonal tiles on one wave, every other tile on the other) for small
        // systems while one round of workgroups holds the batch -- workgroup / wave / two waves,
        // fp64: 1024 x 256: 0.822 / 0.357 / 0.328, 64 x 256: 0.303 / 0.311 / 0.204, 1024 x 128: 0.319 / 0.104 / 0.100,
        // 64 x 128: 0.132 / 0.093 / 0.066; a tie at 4096 (x 256: 3.24 / 1.367 / 1.390); loses at N = 512 (256 x 512: 1.12 /
        // 1.50 / 1.40, 1024 x 512: 3.06 / 1.88 / 2.26), where the one-wave form (512 registers) keeps more of the update
        // stream in flight;
        // fp32: 1024 x 128: 0.172 / 0.070 / 0.058, 4096 x 128: 0.67 / 0.20 / 0.22, 1024 x 256: 0.441 / 0.220 / 0.186,
        // 4096 x 256: 1.76 / 0.69 / 0.84, 256 x 512: 1.17 / 0.90 / 0.85, 512 x 512: 1.31 / 0.93 / 0.93, 1024 x 512: 1.69 /
        // 1.04 / 1.18, 4096 x 512: 6.6 / 3.7 / 5.4, 64 x 512: 0.72 / 0.87 / 0.75, 256 x 1024: 5.5 / 5.3 / -.
        // (ONE model, us workgroup / two waves / team, fp32: N = 128: 105 / 41 / 44, 256: 236 / 131 / 96, 512: 705 / 741 /
        // 264, 1024: 2820 / - / 1311; fp64: 128: 133 / 61 / 65, 256: 308 / 199 / 147, 512: 901 / 1193 / 423, 1024: 3565 / - /
        // 2311.)
        const bool pair = !dense && Bt <= 1024 && (Np <= 256 || (!f64 && Np <= 512 && Bt >= 128 && Bt <= 256));   // (fp32 only: the N = 512 window)
        // One wave per instance -- every SIMD advances its own factorisation chain; below these batches the workgroup
        // form, whose four waves share one instance's update stream.  fp64, wave vs workgroup: N = 256: 0.45 vs 0.82 at
        // 1024, 1.75 vs 3.2 at 4096; N = 512: 2.1 vs 3.1 and 8.2 vs 12.0; N = 1024: 15.0 vs 15.7.
        const bool wave = f64 ? Bt >= 1024 || (Bt >= 512 && Np <= 512) || (Bt >= 64 && Np <= 128)
                              : Bt >= 1024 || (Bt >= 256 && Np <= 1024) || (Bt >= 128 && Np <= 512) || (Bt >= 64 && Np <= 128);
        f = team4 ? REFIT_TEAM4 : team8 ? REFIT_TEAM8 : pair ? REFIT_PAIR : wave ? REFIT_WAVE : REFIT_WORKGROUP;
    } else if (f == REFIT_PAIR && (dense || nb > 16)) {
        f = REFIT_WAVE;                          // (the two-wave kernel builds K_b itself, packed output only, N <= 512)
    } else if (f == REFIT_TEAM4 && has_Kdense) {
        f = REFIT_TEAM8;                         // (the team of four is not compiled from a dense K_b)
    }
    if ((f == REFIT_TEAM4 || f == REFIT_TEAM8) && nb > 256) return "refit: the team forms (and kernel_kind != 0) address N <= 8192";
    // the chain + bulk kernels address one instance's operator with 32-bit byte offsets
    if (f >= REFIT_PAIR && (unsigned long long)lop_elems<1>(Np) * (f64 ? 8 : 4) >= (1ull << 31))
        return "refit: a per-instance operator of 2^31 bytes or more";
    *plan = RefitPlan{f, 0, 0, 0};
    switch (f) {
    case REFIT_WORKGROUP:
        // few instances: 8 waves per workgroup (the row tiles of a block column side by side); the thresholds are in N, not
        // Np.  fp32, ONE model, 16 waves (retired) -> 8: 126 -> 107 us at N = 128, 288 -> 235 at 256, 754 -> 702 at 512,
        // 2991 -> 2815 at 1024.  fp64 from N = 256.
        plan->waves = Bt < 128 && N >= (f64 ? 256 : 128) ? 8 : 4;
        break;
    case REFIT_WAVE:
        plan->waves = 1;
        // fp32: more than one instance per SIMD (N >= 1024: one wave with all 512 registers is faster even then, 4096 x
        // 1024: 20.7 against 21.6); fp64: one (two = 256 VGPRs spills)
        plan->waves_per_simd = f64 ? 1 : occ_field == BCBF_FORM_OCC1 ? 1 : occ_field == BCBF_FORM_OCC2 ? 2
                                       : (Bt >= 8 * cus && Np < 1024) ? 2 : 1;
        // 64-column super-panels, never for a given dense K_b or (unless forced) a dense output: those are the few-system
        // paths.  fp32 from N = 512; fp64 from 1024 (1024 x 1024 14.5 -> 12.7; at N = 512 the four fp64 tiles -- 128
        // accumulator registers -- cost more than the halved panel reads save: 4096 x 512 7.35 -> 9.1)
        plan->super_panels = sup_field == BCBF_FORM_SUPER_ON ? !has_Kdense : sup_field == BCBF_FORM_SUPER_OFF ? 0
                                 : Np >= (f64 ? 1024 : 512) && !dense;
        break;
    case REFIT_PAIR: plan->waves = 2; break;
    case REFIT_TEAM4: plan->waves = 4; break;
    default: plan->waves = 8; break;
    }
    return nullptr;
}

// compute units of the current device, asked once per device ordinal
static int device_cus() {
    constexpr int MAXDEV = 64;
    static std::atomic<int> cached[MAXDEV];
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < MAXDEV && (cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (dev >= 0 && dev < MAXDEV) cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

template <typename T>
static int refit_entry(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, const T* Kdense,
                       T* Lop, T* UHB, T* Ldense, const int* prev_info, int* info, int Bt, int N, int n, int m, int kind,
                       int form, void* stream) {
    constexpr bool f64 = sizeof(T) == 8;
    if (!Lop || !info || N < 1 || (prev_info != nullptr && prev_info == info)) return BCBF_EINVAL;
    if (!Kdense) {
        if (!X || !UH || !Bm || !ell || !s2 || !UHB) return BCBF_EINVAL;
        if (n < 1 || n > BCBF_MAX_STATE_DIM || m < 1 || m > BCBF_MAX_CTRL_DIM) return BCBF_EINVAL;
    }
    RefitPlan plan;
    // (no instances: the refusals do not depend on the CU count, and the device is not asked)
    if (const char* why = choose_refit_plan(f64, Bt, N, Bt > 0 ? device_cus() : 1, Kdense != nullptr, Ldense != nullptr, kind, form, &plan)) {
        set_error_message(why);
        return BCBF_EINVAL;
    }
    if (Bt <= 0) return BCBF_OK;
    const RefitArgs<T> a{X, UH, Bm, ell, s2, jitter, Kdense, Lop, UHB, Ldense, prev_info, info,
                         Bt, N, round_up(N, NB), n, m + 1, kind, (hipStream_t)stream};
    int rc;
    const char* what;
    switch (plan.form) {
    case REFIT_TEAM4: case REFIT_TEAM8:
        rc = launch_refit_team(a, plan); what = kind != 0 ? "refit_matern52" : f64 ? "refit_team64" : "refit_team32"; break;
    case REFIT_PAIR: rc = launch_refit_pair(a, plan); what = f64 ? "refit_pair64" : "refit_pair32"; break;
    case REFIT_WAVE: rc = launch_refit_wave(a, plan); what = f64 ? "refit_wave64" : "refit_wave32"; break;
    default: rc = launch_refit_workgroup(a, plan); what = f64 ? "refit_mfma64" : "refit_mfma"; break;
    }
    if (rc != 0) return BCBF_EINVAL;       // a size the form does not address
    return check_launch(what);
}

}  // namespace bcbf

// The C entry points (bcbf.h).  The named ones are bcbf_refit_form with form = AUTO, except that they return BCBF_OK for
// Bt <= 0 before any check: callers hand them the null pointers of empty arrays.
#define BCBF_REFIT_ENTRIES(SUF, T)                                                                                              \
    int bcbf_refit_form_##SUF(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, const T* Kdense,  \
                              T* Lop, T* UHB, T* Ldense, const int* prev_info, int* info, int Bt, int N, int n, int m,          \
                              int kernel_kind, int form, void* stream) {                                                        \
        return bcbf::refit_entry<T>(X, UH, Bm, ell, s2, jitter, Kdense, Lop, UHB, Ldense, prev_info, info, Bt, N, n, m,         \
                                    kernel_kind, form, stream);                                                                 \
    }                                                                                                                           \
    int bcbf_refit_##SUF(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, T* Lop, T* UHB,        \
                         T* Ldense, int* info, int Bt, int N, int n, int m, void* stream) {                                     \
        return Bt <= 0 ? BCBF_OK : bcbf_refit_form_##SUF(X, UH, Bm, ell, s2, jitter, nullptr, Lop, UHB, Ldense, nullptr, info,  \
                                                         Bt, N, n, m, 0, BCBF_FORM_AUTO, stream);                               \
    }                                                                                                                           \
    int bcbf_refit_matern52_##SUF(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, T* Lop,       \
                                  T* UHB, T* Ldense, int* info, int Bt, int N, int n, int m, void* stream) {                    \
        return Bt <= 0 ? BCBF_OK : bcbf_refit_form_##SUF(X, UH, Bm, ell, s2, jitter, nullptr, Lop, UHB, Ldense, nullptr, info,  \
                                                         Bt, N, n, m, 1, BCBF_FORM_AUTO, stream);                               \
    }                                                                                                                           \
    int bcbf_refit_rbfm52_##SUF(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, T* Lop,         \
                                T* UHB, T* Ldense, int* info, int Bt, int N, int n, int m, void* stream) {                      \
        return Bt <= 0 ? BCBF_OK : bcbf_refit_form_##SUF(X, UH, Bm, ell, s2, jitter, nullptr, Lop, UHB, Ldense, nullptr, info,  \
                                                         Bt, N, n, m, 2, BCBF_FORM_AUTO, stream);                               \
    }                                                                                                                           \
    /* make_psd's x10 jitter retry (control_affine_model.py:903-919) WITHOUT a host round trip: factor again, with the          \
       caller's (raised) jitter, only the instances whose previous attempt failed; the others return at once and report 0 */    \
    int bcbf_refit_retry_kind_##SUF(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, T* Lop,     \
                                    T* UHB, const int* prev_info, int* info, int Bt, int N, int n, int m, int kernel_kind,      \
                                    void* stream) {                                                                             \
        return Bt <= 0 ? BCBF_OK : !prev_info ? BCBF_EINVAL                                                                     \
             : bcbf_refit_form_##SUF(X, UH, Bm, ell, s2, jitter, nullptr, Lop, UHB, nullptr, prev_info, info, Bt, N, n, m,      \
                                     kernel_kind, BCBF_FORM_AUTO, stream);                                                      \
    }                                                                                                                           \
    int bcbf_refit_retry_##SUF(const T* X, const T* UH, const T* Bm, const T* ell, const T* s2, const T* jitter, T* Lop,          \
                               T* UHB, const int* prev_info, int* info, int Bt, int N, int n, int m, void* stream) {            \
        return bcbf_refit_retry_kind_##SUF(X, UH, Bm, ell, s2, jitter, Lop, UHB, prev_info, info, Bt, N, n, m, 0, stream);      \
    }                                                                                                                           \
    int bcbf_potrf_##SUF(const T* Kb, T* Lop, T* Ldense, int* info, int Bt, int N, void* stream) {                              \
        return Bt <= 0 ? BCBF_OK : !Kb ? BCBF_EINVAL                                                                            \
             : bcbf_refit_form_##SUF(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Kb, Lop, nullptr, Ldense, nullptr,   \
                                     info, Bt, N, 0, 0, 0, BCBF_FORM_AUTO, stream);                                             \
    }
extern "C" {
BCBF_REFIT_ENTRIES(f32, float)
BCBF_REFIT_ENTRIES(f64, double)
#undef BCBF_REFIT_ENTRIES

int bcbf_refit_plan(int is_f64, int Bt, int N, int cus, int has_Kdense, int has_Ldense, int kernel_kind, int form,
                    int* out_plan) {
    bcbf::RefitPlan plan;
    if (!out_plan) return BCBF_EINVAL;
    if (const char* why = bcbf::choose_refit_plan(is_f64 != 0, Bt, N, cus, has_Kdense != 0, has_Ldense != 0, kernel_kind, form, &plan)) {
        bcbf::set_error_message(why);
        return BCBF_EINVAL;
    }
    out_plan[0] = plan.form, out_plan[1] = plan.waves, out_plan[2] = plan.waves_per_simd, out_plan[3] = plan.super_panels;
    return BCBF_OK;
}
}
