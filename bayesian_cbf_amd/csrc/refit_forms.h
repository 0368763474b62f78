// The launch forms of the fused refit (K_b build + Cholesky + packing) and the one place that chooses among them.
// refit.hip holds the entry points, the argument checks and choose_refit_plan; the kernels and their launchers live in
// refit_mfma.hip (workgroup form, fp32), refit_mfma64.hip (workgroup form, fp64) and refit_wave64.hip (one wave, two waves,
// a team of waves per instance; both precisions).
#pragma once
#include "bcbf_common.h"

namespace bcbf {

// bcbf.h: BCBF_FORM_* -- the low four bits of an entry point's `form` argument; the two sub-form fields sit above them
enum RefitForm : int {
    REFIT_AUTO = BCBF_FORM_AUTO,                // the measured rules of choose_refit_plan
    REFIT_WORKGROUP = BCBF_FORM_WORKGROUP,      // one workgroup of 4 or 8 waves per instance
    REFIT_WAVE = BCBF_FORM_WAVE,                // one wave per instance
    REFIT_PAIR = BCBF_FORM_PAIR,                // a chain wave and a bulk wave per instance
    REFIT_TEAM4 = BCBF_FORM_TEAM4,              // a chain wave and three bulk waves
    REFIT_TEAM8 = BCBF_FORM_TEAM8               // a chain wave and seven bulk waves
};

// What a launch reads and writes.  Kdense != NULL: factor the caller's K_b (X .. jitter, UHB unused); only_bad != NULL: the
// previous attempt's info[Bt] -- an instance whose entry is 0 returns at once and reports 0 again (bcbf_refit_retry).
template <typename T> struct RefitArgs {
    const T *X, *UH, *Bm, *ell, *s2, *jitter, *Kdense;
    T *Lop, *UHB, *Ldense;
    const int* only_bad;
    int* info;
    int Bt, N, Np, n, C, kind;
    hipStream_t stream;
};

struct RefitPlan {
    int form;             // REFIT_WORKGROUP .. REFIT_TEAM8
    int waves;            // per instance: 4 / 8 (workgroup), 1, 2, 4, 8
    int waves_per_simd;   // one-wave form: the register allocation, 1 or 2 (0 for the other forms)
    int super_panels;     // one-wave form: 64-column super-panels
};

// Pure: no device call, no state.  NULL and *plan filled, or the reason the request is refused (BCBF_EINVAL).
const char* choose_refit_plan(bool f64, int Bt, int N, int cus, bool has_Kdense, bool has_Ldense, int kind, int form,
                              RefitPlan* plan);

// 0, or -1 for a size the form does not address (nothing launched).  Defined for float and double.
template <typename T> int launch_refit_workgroup(const RefitArgs<T>& a, const RefitPlan& plan);   // refit_mfma.hip, refit_mfma64.hip
template <typename T> int launch_refit_wave(const RefitArgs<T>& a, const RefitPlan& plan);        // refit_wave64.hip
template <typename T> int launch_refit_pair(const RefitArgs<T>& a, const RefitPlan& plan);        // refit_wave64.hip
template <typename T> int launch_refit_team(const RefitArgs<T>& a, const RefitPlan& plan);        // refit_wave64.hip

}  // namespace bcbf
