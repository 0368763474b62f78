/*
 * libbcbf -- MI355X (gfx950) kernels for the Bayesian-CBF hot path: matrix-variate GP posterior
 * over F(x) = [f(x) g(x)], control-barrier / control-Lyapunov chance-constraint terms and the
 * per-step second-order-cone program, batched over independent control-loop instances.
 *
 * This is the drop-in boundary.  The reference (wecacuee/Bayesian_CBF) has no
 * FFI layer: its "operator API" is the Python call surface of bayes_cbf/control_affine_model.py,
 * cbc2.py, unicycle_move_to_pose.py and optimizers.py, executed with torch CPU/GPU tensors.  Each
 * entry point below cites the reference arithmetic it replaces (file:line, relative to the
 * upstream checkout); INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to a contiguous row-major array; leading axis Bt = number
 *    of independent instances (one GP / one control loop each); the caller owns all memory and
 *    the library allocates nothing;
 *  - N = #training points per instance, n = state dim, m = control dim, C = 1+m;
 *  - `_f32` / `_f64` select the storage + arithmetic type (the conic solver keeps fp64 iterates for both -- the fp32
 *    entry points read and write fp32 and solve the program those numbers define to fp64 accuracy; bcbf_coneqp is
 *    fp64 only);
 *  - `stream` is a hipStream_t (pass 0 for the default stream); calls are asynchronous and
 *    re-entrant; no randomness is drawn inside the library (jitter vectors are inputs);
 *  - return value: 0 on success, <0 on a bad argument / launch failure (BCBF_E*); per-instance
 *    numerical outcomes are reported through `info` / `status` arrays.
 */
#ifndef BCBF_H
#define BCBF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libbcbf.so is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#pragma GCC visibility push(default)

#define BCBF_VERSION_MAJOR 0
#define BCBF_VERSION_MINOR 1

#define BCBF_OK 0
#define BCBF_EINVAL (-1)   /* unsupported size / null pointer */
#define BCBF_ELAUNCH (-2)  /* HIP launch error (see bcbf_last_error) */

/* diagonal-block size of the packed triangular operator ("Lop") */
#define BCBF_NB 32
/* limits of the compiled kernels */
#define BCBF_MAX_STATE_DIM 8
#define BCBF_MAX_CTRL_DIM 3
/* Columns of the control / task factor accepted by the entry points the vector-variate (CoGP) comparator runs on with
 * expanded inputs -- bcbf_kb_build[_rbflin], bcbf_mll_grad_rbflin: (1+m) n task outputs, 9 for the unicycle
 * (control_affine_model.py:1106-1357).  The per-step kernels keep BCBF_MAX_CTRL_DIM. */
#define BCBF_MAX_TASK_DIM 12
#define BCBF_MAX_CONSTRAINTS 8        /* constraint rows per instance: bcbf_cbc_terms, bcbf_unicycle_constraints,
                                         bcbf_controller_cones, bcbf_coneqp (second-order cones) */
#define BCBF_MAX_QUAD_CONSTRAINTS 4   /* the four-lanes-per-instance solver kernels (bcbf_socp, bcbf_cbc_socp,
                                         bcbf_unicycle_control_step): one lane of a quad per cone; programs with more
                                         cones go through bcbf_cbc_terms + bcbf_coneqp (the host wrappers route) */

/* solver status codes (per instance) */
#define BCBF_SOCP_OPTIMAL 0
#define BCBF_SOCP_MAXITER 1
#define BCBF_SOCP_DIVERGED 2   /* infeasible program: the reference raises there (optimizers.py:74-86) */
#define BCBF_SOCP_BADCONE 3    /* [[v,bfv'/2],[bfv/2,V]] not positive definite (unicycle_move_to_pose.py:861) */

int bcbf_version(void);
const char* bcbf_last_error(void);

/* Measurement aid (SURVEY.md 8d asks for the vendor HBM figure AND a ceiling measured on the same box; no reference
 * counterpart): one launch that READS `bytes` of the caller's device buffer `buf` (16-byte aligned) with the access
 * pattern of the roofline kernel's operator stream -- 16-byte non-temporal loads, contiguous per workgroup -- and writes
 * nothing (`sink`: >= 256 floats of device memory, never written for finite data).  `*bytes_read` (host) receives the
 * bytes the launch touches (bytes rounded down to a multiple of 16 * 8192).  Time it with events on `stream`. */
int bcbf_hbm_read_probe(const void* buf, size_t bytes, void* sink, size_t* bytes_read, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Packed triangular operator "Lop" (the HBM layout the per-step kernel streams).
 * Np = N rounded up to BCBF_NB (32), J = floor(j/32).  Two parts:
 *   off-diagonal: column j stores L[i][j] for the rows i = 32 (J+1) .. Np-1 below its 32x32 diagonal block, contiguously,
 *     columns back to back -- every column starts on a 128-byte boundary and is a whole number of 128-byte lines;
 *   then the diagonal blocks, INVERTED (inv(L_JJ)), lower triangles only, column-major packed, 544 elements per block
 *     (528 used).
 *   last, a second copy of the inverted diagonal blocks as full 32x32 tiles (1024 elements per block), read only by the
 *     shared-model matrix-core kernel -- capacity, not traffic: the streaming kernels never touch it.
 * Rows/cols >= N are identity.  Elements per instance = Np*(Np+2)/2 + 32*Np (same for f32 and f64); the streamed part
 * is the exact triangle plus half a row of padding per block.  The layout is private to the library
 * (bcbf_common.h: lop_base, lop_dinv, lop_dfull).
 * ------------------------------------------------------------------------------------------- */
size_t bcbf_lop_elems_f32(int N);
size_t bcbf_lop_elems_f64(int N);

/* K1: K_b[i][j] = s2*exp(-1/2 |(x_i-x_j)/ell|^2) * uh_i' Bm uh_j  (+ jitter[i] on the diagonal).
 * Replaces control_affine_model.py:370-372 (+ the diagonal perturbation of make_psd :907-910).
 * X[Bt,N,n] UH[Bt,N,C] Bm[Bt,C,C] ell[Bt,n] s2[Bt] jitter[Bt,N] (may be NULL) -> Kb[Bt,N,N] (full, symmetric).
 * C = m + 1 up to BCBF_MAX_TASK_DIM here (the expanded CoGP system), also in the _rbflin form. */
int bcbf_kb_build_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                      const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream);
int bcbf_kb_build_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                      const double* jitter, double* Kb, int Bt, int N, int n, int m, void* stream);

/* K1+K2 fused refit: builds K_b (+jitter) on the fly, factors it (blocked left-looking Cholesky),
 * inverts the diagonal blocks and writes the packed operator; also UHB = UH Bm.
 * Replaces _perturbed_cholesky_compute + make_psd (control_affine_model.py:366-377, 899-921).
 * info[b] = 0 ok, k>0: pivot k (1-based) not positive -> caller retries with jitter x10 (:913-919).
 * Ldense (optional, may be NULL): row-major dense L[Bt,N,N] for callers that want the factor itself. */
int bcbf_refit_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                   const float* jitter, float* Lop, float* UHB, float* Ldense, int* info,
                   int Bt, int N, int n, int m, void* stream);
int bcbf_refit_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                   const double* jitter, double* Lop, double* UHB, double* Ldense, int* info,
                   int Bt, int N, int n, int m, void* stream);
/* make_psd's x10 jitter retry (control_affine_model.py:903-919) without a host round trip: arguments of bcbf_refit (no dense
 * output) plus prev_info[Bt] = the info of the previous attempt (a different buffer than info).  Only instances with
 * prev_info[b] != 0 are factored again -- with the jitter the caller has raised for them -- the others return at once and
 * report info[b] = 0; their Lop / UHB are left as the successful attempt wrote them.  Launch it unconditionally after
 * bcbf_refit (and again, ping-ponging the two info buffers, for further levels): a launch in which nothing failed costs
 * microseconds, and no stream waits for the host. */
int bcbf_refit_retry_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                         const float* jitter, float* Lop, float* UHB, const int* prev_info, int* info,
                         int Bt, int N, int n, int m, void* stream);
int bcbf_refit_retry_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                         const double* jitter, double* Lop, double* UHB, const int* prev_info, int* info,
                         int Bt, int N, int n, int m, void* stream);
/* ... for a state of any data kernel (kernel_kind 0 = RBF: bcbf_refit_retry itself; 1 = Matern-5/2, 2 = RBF x Matern-5/2: the
 * retry of bcbf_refit_matern52 / bcbf_refit_rbfm52; opt-in, no reference counterpart) */
int bcbf_refit_retry_kind_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                              const float* jitter, float* Lop, float* UHB, const int* prev_info, int* info,
                              int Bt, int N, int n, int m, int kernel_kind, void* stream);
int bcbf_refit_retry_kind_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                              const double* jitter, double* Lop, double* UHB, const int* prev_info, int* info,
                              int Bt, int N, int n, int m, int kernel_kind, void* stream);

/* The general refit entry: bcbf_refit, bcbf_refit_retry[_kind], bcbf_refit_matern52 / _rbfm52 and bcbf_potrf are this call with
 * form = BCBF_FORM_AUTO.  Kdense != NULL: factor the caller's K_b[Bt,N,N] (bcbf_potrf: X .. jitter, UHB, n, m unused);
 * prev_info != NULL: the retry (factor only the instances with prev_info[b] != 0; prev_info == info is refused);
 * kernel_kind: 0 RBF, 1 Matern-5/2, 2 RBF x Matern-5/2.  BCBF_EINVAL before any launch for a null required pointer, N < 1,
 * n or m out of range (without Kdense), a kernel_kind or form that does not exist, or a form refused below -- these checks
 * run before the Bt <= 0 early return (the older entries return BCBF_OK for Bt <= 0 before they look at anything else).
 *
 * `form` = one of the launch forms below, optionally or-ed with one BCBF_FORM_SUPER_* and one BCBF_FORM_OCC* value.  The
 * library measures and chooses (AUTO); the others exist for parity tests and measurements, and every form computes the same
 * factor (to rounding: the forms accumulate in different orders).  The choice depends on the arguments and the device's
 * compute-unit count only -- never on the process environment.
 *   WORKGROUP  one workgroup of 4 or 8 waves per instance; always honoured.
 *   WAVE       one wave per instance; always honoured.
 *   PAIR       two waves per instance; runs WAVE with a dense input or output (Kdense / Ldense) or N > 512.
 *   TEAM4/8    a chain wave + three / seven bulk waves per instance; TEAM4 from Kdense runs TEAM8; N > 8192: BCBF_EINVAL.
 *   kernel_kind != 0 has one form, TEAM8 (no Kdense, N <= 8192): any form but AUTO / TEAM8 is BCBF_EINVAL.
 * Sub-forms of WAVE (ignored by the other forms): 64-column super-panels on / off (on is honoured unless Kdense), and the
 * register allocation for 1 / 2 waves per SIMD (fp32 only; fp64 always runs 1). */
#define BCBF_FORM_AUTO 0
#define BCBF_FORM_WORKGROUP 1
#define BCBF_FORM_WAVE 2
#define BCBF_FORM_PAIR 3
#define BCBF_FORM_TEAM4 4
#define BCBF_FORM_TEAM8 5
#define BCBF_FORM_SUPER_ON 0x10
#define BCBF_FORM_SUPER_OFF 0x20
#define BCBF_FORM_OCC1 0x40
#define BCBF_FORM_OCC2 0x80
int bcbf_refit_form_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                        const float* jitter, const float* Kdense, float* Lop, float* UHB, float* Ldense,
                        const int* prev_info, int* info, int Bt, int N, int n, int m, int kernel_kind, int form, void* stream);
int bcbf_refit_form_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                        const double* jitter, const double* Kdense, double* Lop, double* UHB, double* Ldense,
                        const int* prev_info, int* info, int Bt, int N, int n, int m, int kernel_kind, int form, void* stream);
/* What bcbf_refit_form would launch on a device of `cus` compute units: out_plan[4] (host) = { form (never AUTO), waves per
 * instance, waves per SIMD (WAVE only, else 0), super-panels 0 / 1 }.  A host function: no device call.  BCBF_EINVAL (reason
 * in bcbf_last_error) where bcbf_refit_form refuses the form. */
int bcbf_refit_plan(int is_f64, int Bt, int N, int cus, int has_Kdense, int has_Ldense, int kernel_kind, int form,
                    int* out_plan);

/* Random max_train subset of a learning loop's observation pool, selected and gathered in one launch: the reference's
 * `np.random.shuffle(indices)` + `shuffled_indices[:max_train]` (LearnedShiftInvariantDynamics.fit,
 * unicycle_move_to_pose.py:377-384) with the randomness supplied by the caller.  keys[B, ldk]: one draw per pool row (uniform
 * in [0,1), fp32 for both precisions); the pool of instance b is stream rows lo .. lo+P-1 of X[B,Ntot,n], UH[B,Ntot,1+m],
 * Y[B,Ntot,n].  Output row j is the pool row with the j-th smallest key, equal keys to the lower pool index first
 * (= torch.sort(keys[:, :P], stable=True).indices[:, :N] + lo): Xo[B,N,n], UHo[B,N,1+m], Yo[B,N,n] (the layout bcbf_refit /
 * bcbf_potrs read) and idx_out[B,N] = the stream row of output row j.  Limits: 1 <= N <= P <= 8192, lo + P <= Ntot,
 * ldk >= P, 1 <= n <= 8, 0 <= m <= 8, B >= 1; otherwise BCBF_EINVAL before any launch, reason in bcbf_last_error. */
int bcbf_subsample_rows_f32(const float* keys, int ldk, int lo, int P, const float* X, const float* UH, const float* Y,
                            int Ntot, int n, int m, int N, float* Xo, float* UHo, float* Yo, int32_t* idx_out, int B,
                            void* stream);
int bcbf_subsample_rows_f64(const float* keys, int ldk, int lo, int P, const double* X, const double* UH, const double* Y,
                            int Ntot, int n, int m, int N, double* Xo, double* UHo, double* Yo, int32_t* idx_out, int B,
                            void* stream);

/* Self-triggering interval of B instances in one launch: the high-probability Lipschitz constant Lfh of the learned dynamics
 * over the test points Xtest = off[Nte,n] + x[b] and the time tau for which the last control stays safe -- the per-step body of
 * unicycle_trigger_interval_compute (bayes_cbf/trigger_interval.py:128-167; rbf_knl / rbf_d*_knl_d_x_xp_i :32-43), RBF data
 * kernel only.  Per instance, E = n:
 *   Lkd[j]     = max over ordered pairs (a, b) of uBu 2 ls_j^-4 (X_a - X_b)_j sf^2 exp(-1/2 sum_d ((X_a - X_b)_d / ls_d)^2)   (:144-147;
 *                sf is squared as the reference executes it, :33; the pairs a == b count, so Lkd >= 0)
 *   maxk[i,j]  = Adiag[i] uBu sf^2 / ls_j^2                                                                                (:143)
 *   Lfs[i,j]   = sqrt(2 log(2 E^2 / deltaL)) maxk + 12 sqrt(6 E) max(maxk, sqrt(r Adiag[i] Lkd[j]))                        (:148-149)
 *   Lfh        = ||Lfs||_F / E                                                                                             (:151)
 *   tau        = (1 / Lfh) log(1 + Lfh zeta / ((Lfh + L_alpha) Lh xvel))        (:165; IEEE results such as inf pass through)
 * x[B,n]; off[Nte,n] shared by the batch, arbitrary points; ls[Bh,n], sf[Bh], Adiag[Bh,n] with Bh = B (per-instance models) or
 * 1 (one model for all); uBu[B] = uh' B uh, xvel[B], Lh[B]; r = the reference's pdist(grid) scalar.  Outputs Lkd[B,n], Lfh[B],
 * tau[B].  The pair maximum runs in the working type, the closed forms in fp64 for both.  One workgroup per instance, the
 * points in LDS: Nte 4 sizeof(T) (n = 3) must fit 160 KB - 256 B.  Limits: B >= 1, Bh in {1, B}, 1 <= n <= 3, Nte >= 1;
 * otherwise BCBF_EINVAL before any launch, reason in bcbf_last_error.  No allocation, no host synchronisation: capturable. */
int bcbf_trigger_interval_f32(const float* x, const float* off, const float* ls, const float* sf, const float* Adiag,
                              const float* uBu, const float* xvel, const float* Lh, double r, double deltaL, double zeta,
                              double L_alpha, float* Lkd, float* Lfh, float* tau, int B, int Bh, int Nte, int n, void* stream);
int bcbf_trigger_interval_f64(const double* x, const double* off, const double* ls, const double* sf, const double* Adiag,
                              const double* uBu, const double* xvel, const double* Lh, double r, double deltaL, double zeta,
                              double L_alpha, double* Lkd, double* Lfh, double* tau, int B, int Bh, int Nte, int n, void* stream);

/* One EVENT of the self-triggered closed loop for Bt unicycle instances in one launch: the trigger time of the control that
 * bcbf_unicycle_control_step[_kind] called with dt = 0 (solve only, no plant) has just left in its workspace, and the plant step
 * over that time -- the loop the paper prescribes, where the periodic loops re-solve every dt whatever the model says.  Every
 * instance runs on its own clock t[b]; an instance with t[b] >= t_end is finished: nothing of it is read or written.  Else:
 *   ubar = (1, u), u = y[b, 0:2];   uBu = ubar' Bhyp ubar;   xvel = |fhat + ghat u + M_k ubar|  (the model's one-step prediction
 *   over dt, the xtp1 the logging loop records; M_k ubar formed as bcbf_unicycle_control_step_sampled forms it);
 *   Lh   = the largest single element of ObstacleCBF.grad_cbf over the test points off[Nte,3] + x[b], the Kob obstacles and the
 *          three components, rho^2 of an obstacle being the SUM over all test points of |p_a - c_k|^2 as the reference's
 *          batch-wide torch.norm takes it (unicycle_move_to_pose.py:670; trigger_interval.py:159);
 *   Lkd, Lfh, tau as bcbf_trigger_interval computes them from these three, each rounded to the working type first (n = 3);
 *   solved (status[b] == BCBF_SOCP_OPTIMAL):  hold = clamp(tau, tau_min, tau_max), tau = +inf giving tau_max and NaN or
 *          tau <= 0 giving tau_min;  dt_b = min(hold, t_end - t[b]);  x[b] += g(x; L_true) u dt_b, the arithmetic of bcbf_unicycle_step;
 *   unsolved: the state is kept and dt_b = min(tau_max, t_end - t[b]), as the periodic loop lets time pass;
 *   t[b] += dt_b (the last, partial step lands on t_end itself), events[b] += 1, and the planner's rows of index
 *   min(floor(t[b] / dt_plan), P - 1) are copied from plan_all[P,3], dplan_all[P,3] into plan[b], dot_plan[b] for the next solve.
 * x, t (fp64 in both precisions), events (int32), plan, dot_plan are in/out; y, status, fhat[Bt,3], ghat[Bt,3,2], Mk[Bt,3,3] are
 * the control step's; centers[Bt,Kob,2], tw[2] the obstacles'; ls[Bh,3], sf[Bh], Adiag[Bh,3], Bhyp[Bh,3,3] the kernel's
 * hyper-parameters with Bh = Bt or 1; r = the reference's pdist(grid) scalar.  Outputs, each may be NULL: tau[Bt] (raw, before
 * the clamp), dt_used[Bt], Lfh[Bt], Lkd[Bt,3], Lh[Bt], xvel[Bt], uBu[Bt].  One workgroup per instance, the points in LDS as in
 * bcbf_trigger_interval; the block sum and maximum of Lh by shuffles and LDS, no atomics.
 * Limits: Bt >= 1, Bh in {1, Bt}, 1 <= Kob < BCBF_MAX_CONSTRAINTS, 1 <= Nte with 16 Nte sizeof(T) / 4 <= 160 KB - 256 B, P >= 1,
 * dt_plan > 0, 0 < tau_min <= tau_max < inf, every pointer but the seven outputs non-NULL; otherwise BCBF_EINVAL before any HIP
 * call, reason in bcbf_last_error.  No allocation, no host synchronisation: capturable. */
int bcbf_unicycle_trigger_step_f32(float* x, const float* y, const int* status, const float* fhat, const float* ghat, const float* Mk,
                                   const float* centers, const float* tw, const float* off, double r, const float* ls, const float* sf,
                                   const float* Adiag, const float* Bhyp, double deltaL, double zeta, double L_alpha, double tau_min,
                                   double tau_max, double t_end, float L_true, const float* plan_all, const float* dplan_all,
                                   double dt_plan, double* t, int* events, float* plan, float* dot_plan, float* tau, float* dt_used,
                                   float* Lfh, float* Lkd, float* Lh, float* xvel, float* uBu, int Bt, int Bh, int Kob, int Nte, int P,
                                   void* stream);
int bcbf_unicycle_trigger_step_f64(double* x, const double* y, const int* status, const double* fhat, const double* ghat,
                                   const double* Mk, const double* centers, const double* tw, const double* off, double r,
                                   const double* ls, const double* sf, const double* Adiag, const double* Bhyp, double deltaL, double zeta,
                                   double L_alpha, double tau_min, double tau_max, double t_end, double L_true, const double* plan_all,
                                   const double* dplan_all, double dt_plan, double* t, int* events, double* plan, double* dot_plan,
                                   double* tau, double* dt_used, double* Lfh, double* Lkd, double* Lh, double* xvel, double* uBu, int Bt,
                                   int Bh, int Kob, int Nte, int P, void* stream);

/* bcbf_unicycle_trigger_step with the plant drawn from the model's own posterior over the variable hold, and an audit of the
 * held control at the moment it is released: the same launch (one workgroup per instance, same pair loop and closed forms), the
 * new work done by one thread in fp64 from the values as the working type stores them, every output rounded once, no atomics.
 * It follows the FUSED solve (bcbf_unicycle_control_step[_kind] with dt = 0), whose rows it reads: Bk[Bt,3,3], A[Bt,3,3],
 * grad[Bt,1+Kob,3], cst[Bt,1+Kob], the task's sign[1+Kob] and rho[Bt] (all required), so Kob + 1 <= BCBF_MAX_QUAD_CONSTRAINTS.
 * Everything bcbf_unicycle_trigger_step writes that does not depend on the plant (tau, Lfh, Lkd, Lh, xvel, uBu, dt_used, t,
 * events, plan, dot_plan) is bit-identical to that entry's; with z == NULL so is x.  A finished instance (t[b] >= t_end) leaves
 * before anything of it is read or written, the new buffers included.
 *  Group P, the posterior plant -- present when z[Bt,3] (the caller's standard normals) is non-NULL; xdot_s[Bt,3] and
 *  cbc_s[Bt,1+Kob] optional; viol[Bt,Kob], solved[Bt] (int32), min_cbc[Bt,Kob] optional, all three or none:
 *   a solved instance steps by the draw instead of the true drive (L_true is ignored):
 *     xdot_s = fhat + ghat u + M_k ubar + sqrt(max(ubar' B_k ubar, 0)) L_A z,  A = L_A L_A' (a pivot <= 0 zeroes its column),
 *     x[b] = (T)(x[b] + xdot_s dt_b)  with dt_b the hold under the clamp rules above, as the working type holds it,
 *     cbc_s[b,k] = sign_k (grad_k . xdot_s + cst_k) for every row, the CLC row included
 *   -- the arithmetic of bcbf_unicycle_control_step_sampled, which takes no plant step when called with dt = 0;
 *   an unsolved instance keeps its state, gets xdot_s = 0, cbc_s = 0 and lets min(tau_max, t_end - t[b]) pass;
 *   the counters of a solved instance: solved[b] += 1, viol[b,k-1] += (cbc_s[b,k] < 0 or non-finite) and min_cbc the running
 *   minimum (a non-finite value entering as -inf), k = 1..Kob, on cbc_s as stored: bcbf_rollout_risk's semantics, done here
 *   because that entry cannot tell an idle instance from a live one.
 *  Group H, the held-control audit -- present when u_held is non-NULL (then all seven buffers are), independent of group P:
 *  u_held[Bt,2] and held[Bt] (int32) in/out; held_mean[Bt,Kob], held_margin[Bt,Kob] out; audit_n[Bt], audit_neg[Bt,Kob,2]
 *  (int32) and audit_min[Bt,Kob,2] in/out counters:
 *   where held[b] != 0, before anything else of the event and whatever its status, on the rows the solve of THIS event wrote at
 *   the current state, with ubar_h = (1, u_held[b]) and for every obstacle row k = 1..Kob:
 *     mean_k   = sign_k (grad_k . (fhat + ghat u_held + M_k ubar_h) + cst_k)
 *     std_k    = sqrt(max((ubar_h' B_k ubar_h) (grad_k' A grad_k), 0))
 *     margin_k = mean_k - rho[b] std_k                         (the two sides of the cone the control was solved under)
 *   held_mean[b,k-1] and held_margin[b,k-1] are written, audit_n[b] += 1, audit_neg[b,k-1,0] += !(mean_k >= 0),
 *   audit_neg[b,k-1,1] += !(margin_k >= 0) (NaN counts as negative) and audit_min[b,k-1,:] takes the running minima (NaN
 *   entering as -inf), all on the values as stored;  where held[b] == 0 -- an instance's first event, and the event after an
 *   unsolved one -- nothing is audited and the output rows are not written;
 *   at the end of the event u_held[b] = u of this event and held[b] = (status[b] == BCBF_SOCP_OPTIMAL).
 * Limits: those of bcbf_unicycle_trigger_step, and Kob <= BCBF_MAX_QUAD_CONSTRAINTS - 1, the six rows non-NULL, no optional
 * buffer of group P without z, each group's counters complete; otherwise BCBF_EINVAL before any HIP call, reason in
 * bcbf_last_error.  No allocation, no host synchronisation: capturable. */
int bcbf_unicycle_trigger_step_audit_f32(float* x, const float* y, const int* status, const float* fhat, const float* ghat,
                                         const float* Mk, const float* centers, const float* tw, const float* off, double r,
                                         const float* ls, const float* sf, const float* Adiag, const float* Bhyp, double deltaL,
                                         double zeta, double L_alpha, double tau_min, double tau_max, double t_end, float L_true,
                                         const float* plan_all, const float* dplan_all, double dt_plan, double* t, int* events,
                                         float* plan, float* dot_plan, float* tau, float* dt_used, float* Lfh, float* Lkd, float* Lh,
                                         float* xvel, float* uBu, const float* Bk, const float* A, const float* grad,
                                         const float* cst, const float* sign, const float* rho, const float* z, float* xdot_s,
                                         float* cbc_s, int* viol, int* solved, float* min_cbc, float* u_held, int* held,
                                         float* held_mean, float* held_margin, int* audit_n, int* audit_neg, float* audit_min, int Bt,
                                         int Bh, int Kob, int Nte, int P, void* stream);
int bcbf_unicycle_trigger_step_audit_f64(double* x, const double* y, const int* status, const double* fhat, const double* ghat,
                                         const double* Mk, const double* centers, const double* tw, const double* off, double r,
                                         const double* ls, const double* sf, const double* Adiag, const double* Bhyp, double deltaL,
                                         double zeta, double L_alpha, double tau_min, double tau_max, double t_end, double L_true,
                                         const double* plan_all, const double* dplan_all, double dt_plan, double* t, int* events,
                                         double* plan, double* dot_plan, double* tau, double* dt_used, double* Lfh, double* Lkd,
                                         double* Lh, double* xvel, double* uBu, const double* Bk, const double* A, const double* grad,
                                         const double* cst, const double* sign, const double* rho, const double* z, double* xdot_s,
                                         double* cbc_s, int* viol, int* solved, double* min_cbc, double* u_held, int* held,
                                         double* held_mean, double* held_margin, int* audit_n, int* audit_neg, double* audit_min,
                                         int Bt, int Bh, int Kob, int Nte, int P, void* stream);

/* bcbf_unicycle_trigger_step_audit that also OBSERVES the event for a learner: the same launch, every argument of that entry
 * with unchanged meaning (groups P and H stay optional), and after the plant step one more piece of work for the same thread,
 * plain stores from one lane, no atomics.  It is what lets the self-triggered loop learn its dynamics online: the periodic
 * observing entry (bcbf_unicycle_control_step_observe) writes its row with the plant step of the SOLVE launch and divides by one
 * dt for the batch; here the solve runs with dt = 0 and every instance holds its control for its own dt_b.
 * Everything the audit entry writes is bit-identical to that entry's on the same inputs.  A finished instance (t[b] >= t_end)
 * leaves before anything of it is read or written, the new buffers included.
 *  Group O, the observation -- rows present when obs_x is non-NULL (then obs_uh and obs_y are), xq_next independent of them:
 *   obs_x, obs_uh, obs_y [Bt, obs_ld, 3]: the observation STREAM of every instance.  With e = events[b] BEFORE the increment:
 *   if e % obs_every == 0 and k = obs_row0 + e / obs_every < obs_ld, row b * obs_ld + k is written; a row with k >= obs_ld is
 *   skipped silently, nothing is written outside the buffers.  The index comes from the device counter, so one captured graph
 *   serves every event and instances whose counts differ write their own rows.  The row is that of
 *   bcbf_unicycle_control_step_observe (LearnedShiftInvariantDynamics.train, unicycle_move_to_pose.py:326-372) with the event's
 *   own hold dt_b, as the working type stores it (dt_used[b]), in place of dt:
 *     obs_x  = the state before the step, (0, 0, theta) with flags bit 0 (shift-invariant inputs)
 *     obs_uh = (1, u)
 *     obs_y  = (x_new - x_old) / dt_b - g(theta; L_mean) u      from the states as stored (rounded to the working type);
 *   an unsolved instance kept its state: obs_uh = (1, 0, 0), obs_y = 0 -- a unicycle at rest.  With group P the row records the
 *   drawn plant (x_new is the state that step stored).  L_mean, the wheelbase of the prior mean AckermannDrive, is a float in
 *   both precisions and is converted to the working type.
 *   xq_next[Bt,3] (optional): the regressor's input at the NEW state -- (0, 0, theta_new) with flags bit 0 -- the query of the
 *   next solve; written at every event of a live instance, observed or not.
 * Limits: those of bcbf_unicycle_trigger_step_audit; the three row buffers together or not at all; with rows obs_ld >= 1,
 * obs_row0 >= 0, obs_every >= 1 and L_mean a number other than 0; no flag but bit 0; otherwise BCBF_EINVAL before any HIP call,
 * reason in bcbf_last_error.  No allocation, no host synchronisation: capturable. */
int bcbf_unicycle_trigger_step_observe_f32(float* x, const float* y, const int* status, const float* fhat, const float* ghat,
        const float* Mk, const float* centers, const float* tw, const float* off, double r, const float* ls, const float* sf, const float* Adiag,
        const float* Bhyp, double deltaL, double zeta, double L_alpha, double tau_min, double tau_max, double t_end, float L_true,
        const float* plan_all, const float* dplan_all, double dt_plan, double* t, int* events, float* plan, float* dot_plan, float* tau,
        float* dt_used, float* Lfh, float* Lkd, float* Lh, float* xvel, float* uBu, const float* Bk, const float* A, const float* grad, const float* cst,
        const float* sign, const float* rho, const float* z, float* xdot_s, float* cbc_s, int* viol, int* solved, float* min_cbc, float* u_held,
        int* held, float* held_mean, float* held_margin, int* audit_n, int* audit_neg, float* audit_min, float L_mean, float* obs_x,
        float* obs_uh, float* obs_y, int obs_ld, int obs_row0, int obs_every, float* xq_next, int flags, int Bt, int Bh, int Kob, int Nte,
        int P, void* stream);
int bcbf_unicycle_trigger_step_observe_f64(double* x, const double* y, const int* status, const double* fhat, const double* ghat,
        const double* Mk, const double* centers, const double* tw, const double* off, double r, const double* ls, const double* sf, const double* Adiag,
        const double* Bhyp, double deltaL, double zeta, double L_alpha, double tau_min, double tau_max, double t_end, double L_true,
        const double* plan_all, const double* dplan_all, double dt_plan, double* t, int* events, double* plan, double* dot_plan, double* tau,
        double* dt_used, double* Lfh, double* Lkd, double* Lh, double* xvel, double* uBu, const double* Bk, const double* A, const double* grad, const double* cst,
        const double* sign, const double* rho, const double* z, double* xdot_s, double* cbc_s, int* viol, int* solved, double* min_cbc, double* u_held,
        int* held, double* held_mean, double* held_margin, int* audit_n, int* audit_neg, double* audit_min, float L_mean, double* obs_x,
        double* obs_uh, double* obs_y, int obs_ld, int obs_row0, int obs_every, double* xq_next, int flags, int Bt, int Bh, int Kob, int Nte,
        int P, void* stream);

/* K2 on a caller-supplied dense SPD matrix (lower triangle of Kb[Bt,N,N] is read): same outputs.
 * Replaces torch.linalg.cholesky (control_affine_model.py:911). */
int bcbf_potrf_f32(const float* Kb, float* Lop, float* Ldense, int* info, int Bt, int N, void* stream);
int bcbf_potrf_f64(const double* Kb, double* Lop, double* Ldense, int* info, int Bt, int N, void* stream);

/* K3: whitened targets Vw = L^-1 Y and alpha = K_b^-1 Y = L^-T Vw from the packed operator.
 * Replaces torch.cholesky_solve (control_affine_model.py:545); Y = Xdot - UH M0 (:525-532) is
 * formed here.  Xdot[Bt,N,n] UH[Bt,N,C] M0[Bt,C,n] -> Vw[Bt,N,n], alpha[Bt,N,n] (alpha may be NULL). */
int bcbf_potrs_f32(const float* Lop, const float* Xdot, const float* UH, const float* M0,
                   float* Vw, float* alpha, int Bt, int N, int n, int m, void* stream);
int bcbf_potrs_f64(const double* Lop, const double* Xdot, const double* UH, const double* M0,
                   double* Vw, double* alpha, int Bt, int N, int n, int m, void* stream);

/* K11: append one training point to the packed operator (bordered Cholesky).  knew[Bt,N] = new
 * row of K_b against the old points, kappa[Bt] its diagonal (incl. jitter).  Lop_in has N points,
 * Lop_out N+1 (may alias Lop_in while N+1 stays inside the same 32-row padding).  info[b] = 0, or N+1 when the new
 * pivot is not positive: then nothing of instance b changes (row N stays an identity padding row, the operator still
 * describes the old N points) and the caller may retry with a larger jitter.  No reference counterpart (the
 * reference refactorises). */
int bcbf_chol_append_f32(const float* Lop_in, const float* knew, const float* kappa, float* Lop_out,
                         int* info, int Bt, int N, void* stream);
int bcbf_chol_append_f64(const double* Lop_in, const double* knew, const double* kappa, double* Lop_out,
                         int* info, int Bt, int N, void* stream);

/* Online update (BASELINE configs[4]): one observation (x_new[Bt,n], uh_new[Bt,1+m] = [1,u],
 * xdot_new[Bt,n]) per instance enters the GP without refactorisation -- the kernel column k(X,x) o (UH B uh) and
 * its diagonal (+ jitter_new[Bt], may be NULL) are formed in the kernel, the packed operator gains the row
 * (bcbf_chol_append), Vw gains (y - l'Vw)/d with y = xdot_new - M0'uh_new, X and UH*B gain their rows.
 * Inputs hold N points ([Bt,N,.]), outputs N+1 ([Bt,N+1,.], distinct buffers: the batch stride changes);
 * Lop_out may alias Lop_in while N+1 stays inside the same 32-row padding.  info[b] = N+1 when the new pivot is not
 * positive: instance b then gains a NEUTRAL point (identity operator row, Vw row 0, UH*B row 0: its posterior is
 * that of the old N points) -- retry by appending again with a larger jitter_new.  Equals bcbf_refit + bcbf_potrs on the
 * N+1 points (the reference refits from scratch: unicycle_move_to_pose.py:340-386, control_affine_model.py:268-335). */
int bcbf_gp_append_f32(const float* Lop_in, const float* Vw_in, const float* X_in, const float* UHB_in,
                       const float* ell, const float* s2, const float* Bm, const float* M0, const float* x_new,
                       const float* uh_new, const float* xdot_new, const float* jitter_new, float* Lop_out,
                       float* Vw_out, float* X_out, float* UHB_out, int* info, int Bt, int N, int n, int m, void* stream);
int bcbf_gp_append_f64(const double* Lop_in, const double* Vw_in, const double* X_in, const double* UHB_in,
                       const double* ell, const double* s2, const double* Bm, const double* M0, const double* x_new,
                       const double* uh_new, const double* xdot_new, const double* jitter_new, double* Lop_out,
                       double* Vw_out, double* X_out, double* UHB_out, int* info, int Bt, int N, int n, int m,
                       void* stream);
/* The same update with the forward solve on the streaming posterior kernel (one query per instance at x_new, at the HBM
 * roofline: W = L^-1 Phi(x_new), l = W uh_new) -- the form for large N (at N = 1500 the simple solve of bcbf_gp_append
 * reads the factor at 40 % of the HBM rate).  Work buffers from the caller: Wwork[Bt, Np, 1+m] (Np = N rounded up to 32),
 * Mk_work[Bt, n, 1+m], Bk_work[Bt, 1+m, 1+m].  Same outputs and info convention. */
int bcbf_gp_append_stream_f32(const float* Lop_in, const float* Vw_in, const float* X_in, const float* UHB_in,
                              const float* ell, const float* s2, const float* Bm, const float* M0, const float* x_new,
                              const float* uh_new, const float* xdot_new, const float* jitter_new, float* Lop_out,
                              float* Vw_out, float* X_out, float* UHB_out, int* info, float* Wwork, float* Mk_work,
                              float* Bk_work, int Bt, int N, int n, int m, void* stream);
int bcbf_gp_append_stream_f64(const double* Lop_in, const double* Vw_in, const double* X_in, const double* UHB_in,
                              const double* ell, const double* s2, const double* Bm, const double* M0, const double* x_new,
                              const double* uh_new, const double* xdot_new, const double* jitter_new, double* Lop_out,
                              double* Vw_out, double* X_out, double* UHB_out, int* info, double* Wwork, double* Mk_work,
                              double* Bk_work, int Bt, int N, int n, int m, void* stream);

/* OPT-IN data kernel: Matern-5/2 with ARD lengthscales under an output scale,
 *   k(x, x') = s2 (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r),   r^2 = sum_d ((x_d - x'_d) / ell_d)^2
 * (gpytorch MaternKernel(nu = 2.5, ard_num_dims = n) inside ScaleKernel).  PARITY UNPINNED: the reference has no Matern
 * kernel anywhere (its data kernels: ScaleKernel(RBFKernel(ard)), control_affine_model.py:164-171, and RBF + Linear,
 * :1121-1122); it is offered because the task statement names an "RBF x Matern kernel-block build", checked at formula level
 * against an independent implementation (scikit-learn's Matern(nu=2.5)), and is never the default.
 * The path: bcbf_refit_matern52 (fused build + jittered Cholesky + packing; or bcbf_kb_build_matern52 -> bcbf_potrf) ->
 * bcbf_potrs -> bcbf_posterior_query_matern52 (streaming kernel; `shared` as in bcbf_posterior_query); rel-degree-2:
 * bcbf_posterior_jets_matern52 + bcbf_cbc2_terms(kernel_kind = 1); fit: bcbf_mll_grad_matern52; online: bcbf_gp_append_matern52.
 * (Round 4: fused refit, jets, likelihood gradient, append.)  Not offered with this kernel: the matrix-core regime-S query
 * and the fused unicycle control step (both read the RBF through their own value code). */
int bcbf_refit_matern52_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                            const float* jitter, float* Lop, float* UHB, float* Ldense, int* info, int Bt, int N, int n, int m,
                            void* stream);
int bcbf_refit_matern52_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                            const double* jitter, double* Lop, double* UHB, double* Ldense, int* info, int Bt, int N, int n, int m,
                            void* stream);
/* arguments of bcbf_posterior_jets / bcbf_mll_grad / bcbf_gp_append */
int bcbf_posterior_jets_matern52_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                     const float* ell, const float* s2, const float* Bm, const float* M0,
                                     const float* xq, float* Mk, float* Bk, float* G, float* Mj, float* Wj, int shared,
                                     int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_jets_matern52_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                     const double* ell, const double* s2, const double* Bm, const double* M0,
                                     const double* xq, double* Mk, double* Bk, double* G, double* Mj, double* Wj, int shared,
                                     int Bt, int N, int n, int m, void* stream);
int bcbf_mll_grad_matern52_f32(const float* Lop, const float* alpha, const float* Kinv, const float* X, const float* UH,
                               const float* R, const float* Ainv, const float* Bm, const float* ell, const float* s2, float* g_ell,
                               float* g_s2, float* g_B, float* logdetK, float* RtA, float* UHtA, int Bt, int N, int n, int m,
                               void* work, void* stream);
int bcbf_mll_grad_matern52_f64(const double* Lop, const double* alpha, const double* Kinv, const double* X, const double* UH,
                               const double* R, const double* Ainv, const double* Bm, const double* ell, const double* s2,
                               double* g_ell, double* g_s2, double* g_B, double* logdetK, double* RtA, double* UHtA, int Bt, int N,
                               int n, int m, void* work, void* stream);
int bcbf_gp_append_matern52_f32(const float* Lop_in, const float* Vw_in, const float* X_in, const float* UHB_in,
                                const float* ell, const float* s2, const float* Bm, const float* M0, const float* x_new,
                                const float* uh_new, const float* xdot_new, const float* jitter_new, float* Lop_out,
                                float* Vw_out, float* X_out, float* UHB_out, int* info, int Bt, int N, int n, int m, void* stream);
int bcbf_gp_append_matern52_f64(const double* Lop_in, const double* Vw_in, const double* X_in, const double* UHB_in,
                                const double* ell, const double* s2, const double* Bm, const double* M0, const double* x_new,
                                const double* uh_new, const double* xdot_new, const double* jitter_new, double* Lop_out,
                                double* Vw_out, double* X_out, double* UHB_out, int* info, int Bt, int N, int n, int m,
                                void* stream);
int bcbf_kb_build_matern52_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                               const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream);
int bcbf_kb_build_matern52_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                               const double* jitter, double* Kb, int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_query_matern52_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                      const float* ell, const float* s2, const float* Bm, const float* M0, const float* xq,
                                      const float* jitter2, float* Mk, float* Bk, float* W, int shared, int Bt, int N,
                                      int n, int m, void* stream);
int bcbf_posterior_query_matern52_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                      const double* ell, const double* s2, const double* Bm, const double* M0,
                                      const double* xq, const double* jitter2, double* Mk, double* Bk, double* W,
                                      int shared, int Bt, int N, int n, int m, void* stream);

/* Safety bookkeeping of one closed-loop step of a Monte-Carlo rollout (BASELINE configs[3]; the statistics are this
 * library's summary of `sample_generator_trajectory` runs, sampling.py:49-75): per trajectory
 * min_h = min(min_h, min_k cst[b,1+k] / gammas[k]) over the Kob obstacle rows of bcbf_unicycle_control_step's `cst` output
 * (h_k(x_t); non-finite -> -inf), and where status[b] == 0: cost += sum_i w[b,i] y[b,i]^2 (nv = m + 1 entries), else
 * fails += 1 (the reference raises ValueError on an unsolved program, unicycle_move_to_pose.py:954-964). */
int bcbf_rollout_stats_f32(const float* cst, const float* y, const int* status, const float* w, const float* gammas,
                           float* min_h, float* cost, int* fails, int Bt, int Kob, int nv, void* stream);
int bcbf_rollout_stats_f64(const double* cst, const double* y, const int* status, const double* w, const double* gammas,
                           double* min_h, double* cost, int* fails, int Bt, int Kob, int nv, void* stream);
/* Risk bookkeeping of one closed-loop step on a posterior-drawn plant (bcbf_unicycle_control_step_sampled's cbc_s[Bt,1+Kob]),
 * the empirical side of the chance constraint P(CBC_k >= 0) >= 1 - max_risk (cbc1.py:10-14): where status[b] == 0,
 * solved[b] += 1, viol[b,k-1] += (cbc_s[b,k] < 0) for the obstacle rows k = 1..Kob (a non-finite value counts as a violation) and
 * min_cbc[b,k-1] = min(min_cbc[b,k-1], cbc_s[b,k]); an unsolved instance took no step and is left alone.  viol[Bt,Kob] and
 * solved[Bt] are int32.  One launch, no host look: capturable in a graph. */
int bcbf_rollout_risk_f32(const float* cbc_s, const int* status, int* viol, int* solved, float* min_cbc, int Bt, int Kob,
                          void* stream);
int bcbf_rollout_risk_f64(const double* cbc_s, const int* status, int* viol, int* solved, double* min_cbc, int Bt, int Kob,
                          void* stream);

/* Capacity-reserving GP storage for the online path (BASELINE configs[4]; the reference refits from scratch,
 * unicycle_move_to_pose.py:340-386).  The packed layout depends on the padded size and X / UH*B / Vw are [Bt,N,.] arrays,
 * so bcbf_gp_append copies every per-instance array on each append and re-packs the operator at every multiple of 32.
 * Reserved storage lays the operator out ONCE for Ncap points (bcbf_lop_elems(Ncap) elements per instance; rows / columns
 * beyond the live N are identity padding) and gives X / UH*B / Vw Ncap rows per instance ([Bt,Ncap,.]):
 *   bcbf_gp_reserve             copies a fitted state of N points into reserved storage of capacity Ncap: Ncap_in = 0 -> the
 *                               inputs are bcbf_refit / bcbf_potrs outputs ([Bt,N,.], packed layout of N points);
 *                               Ncap_in > 0 -> they are reserved storage of that capacity (growing the reservation);
 *   bcbf_posterior_query_reserved   one query per instance on the first N points (the streaming kernel; W optional,
 *                               [Bt, Np, 1+m], Np = N rounded up to 32);
 *   bcbf_gp_append_reserved     one observation per instance enters IN PLACE: the forward solve W = L^-1 Phi(x_new) on the
 *                               streaming kernel, then one operator row, one inverted-diagonal-block row and one row of
 *                               each array are written -- O(N) bytes, no allocation, nothing copied.  N < Ncap; the
 *                               caller's N grows by one.  info as bcbf_gp_append (N+1: neutral point).
 *                               xq[Bt,n] (optional, with Mk[Bt,n,1+m], Bk[Bt,1+m,1+m]): the control step's posterior query on
 *                               the N points BEFORE the append rides along -- both queries share ONE pass over each
 *                               instance's factor (n <= 4, m <= 2; otherwise two passes), halving the traffic of a
 *                               "posterior, then append" step.  Work buffers: Wwork[q Bt, round_up(Ncap,32), 1+m],
 *                               Mk_work[q Bt,n,1+m], Bk_work[q Bt,1+m,1+m] with q = 2 when xq is given, else 1. */
int bcbf_gp_reserve_f32(const float* Lop_in, const float* Vw_in, const float* X_in, const float* UHB_in, float* Lop_r,
                        float* Vw_r, float* X_r, float* UHB_r, int Bt, int N, int Ncap_in, int Ncap, int n, int m,
                        void* stream);
int bcbf_gp_reserve_f64(const double* Lop_in, const double* Vw_in, const double* X_in, const double* UHB_in, double* Lop_r,
                        double* Vw_r, double* X_r, double* UHB_r, int Bt, int N, int Ncap_in, int Ncap, int n, int m,
                        void* stream);
int bcbf_posterior_query_reserved_f32(const float* Lop_r, const float* Vw_r, const float* X_r, const float* UHB_r,
                                      const float* ell, const float* s2, const float* Bm, const float* M0, const float* xq,
                                      const float* jitter2, float* Mk, float* Bk, float* W, int Bt, int N, int Ncap, int n,
                                      int m, void* stream);
int bcbf_posterior_query_reserved_f64(const double* Lop_r, const double* Vw_r, const double* X_r, const double* UHB_r,
                                      const double* ell, const double* s2, const double* Bm, const double* M0,
                                      const double* xq, const double* jitter2, double* Mk, double* Bk, double* W, int Bt,
                                      int N, int Ncap, int n, int m, void* stream);
int bcbf_gp_append_reserved_f32(float* Lop_r, float* Vw_r, float* X_r, float* UHB_r, const float* ell, const float* s2,
                                const float* Bm, const float* M0, const float* x_new, const float* uh_new,
                                const float* xdot_new, const float* jitter_new, int* info, float* Wwork, float* Mk_work,
                                float* Bk_work, const float* xq, float* Mk, float* Bk, int Bt, int N, int Ncap, int n, int m,
                                void* stream);
int bcbf_gp_append_reserved_f64(double* Lop_r, double* Vw_r, double* X_r, double* UHB_r, const double* ell, const double* s2,
                                const double* Bm, const double* M0, const double* x_new, const double* uh_new,
                                const double* xdot_new, const double* jitter_new, int* info, double* Wwork, double* Mk_work,
                                double* Bk_work, const double* xq, double* Mk, double* Bk, int Bt, int N, int Ncap, int n,
                                int m, void* stream);
/* bcbf_gp_append_reserved that also records the RAW rows of the new point in the caller's store -- rawUH[Bt,Ncap,1+m],
 * rawY[Bt,Ncap,n], rawJ[Bt,Ncap]: row N receives (uh_new, xdot_new, jitter_new), or the neutral (0, 0, 1) where the new pivot
 * failed -- the rows a later from-the-data refit of a sliding window is made from (ops.ReservedGP(window=...); the
 * reference keeps its buffer in Python lists, unicycle_move_to_pose.py:340-386).  Same launches, no extra one. */
int bcbf_gp_append_reserved_raw_f32(float* Lop_r, float* Vw_r, float* X_r, float* UHB_r, const float* ell, const float* s2,
                                    const float* Bm, const float* M0, const float* x_new, const float* uh_new,
                                    const float* xdot_new, const float* jitter_new, int* info, float* Wwork, float* Mk_work,
                                    float* Bk_work, const float* xq, float* Mk, float* Bk, float* rawUH, float* rawY,
                                    float* rawJ, int Bt, int N, int Ncap, int n, int m, void* stream);
int bcbf_gp_append_reserved_raw_f64(double* Lop_r, double* Vw_r, double* X_r, double* UHB_r, const double* ell,
                                    const double* s2, const double* Bm, const double* M0, const double* x_new,
                                    const double* uh_new, const double* xdot_new, const double* jitter_new, int* info,
                                    double* Wwork, double* Mk_work, double* Bk_work, const double* xq, double* Mk, double* Bk,
                                    double* rawUH, double* rawY, double* rawJ, int Bt, int N, int Ncap, int n, int m,
                                    void* stream);

/* Window mode with a row-major tail (csrc/tail.hip): the factor of the window's N0 points stays as bcbf_gp_reserve laid it out
 * (Lop_r is only READ; Lcap = the capacity it is laid out for: Ncap for bcbf_gp_reserve's output, N0 for the packed operator of
 * exactly N0 points that bcbf_refit writes -- the window never grows in place, so a window refit needs no re-layout) and the t points observed since the last window refit are rows of a bordered factor kept beside it --
 * Rb[Bt,tcap,round_up(Ncap,32)] (row p: the new point's row over the N0 columns, contiguous), Rinv[Bt,tcap,tcap] (the inverse of the
 * tail's own lower-triangular block), and rows N0+p of X_r / UHB_r / Vw_r (and of the raw store, as in bcbf_gp_append_reserved_raw;
 * rawUH = rawY = rawJ = NULL: none).  One call = one "posterior, then append" step of the online schedule: (Mk[Bt,n,1+m],
 * Bk[Bt,1+m,1+m]) at xq[Bt,n] over all N0 + t points, then (do_append) the observation (x_new, uh_new, xdot_new, jitter_new) enters as
 * tail row t -- one contiguous row written per instance instead of one element in each of the operator's columns, whose ~N dirty
 * 128-byte lines per instance cost the NEXT streaming pass a quarter of its time.  info[Bt] = 0, or N0+t+1 where the new
 * pivot was not positive (a neutral point enters, as in bcbf_gp_append).  do_append = 0: the posterior only (x_new / uh_new still
 * name a valid point; nothing is written but Mk, Bk and the work buffers).  Work buffers: Wwork[Bt,round_up(N0,32),2+m],
 * swork[Bt,1+n].  tcap <= 64, n <= 4, m <= 3; the streaming pass in front keeps its solved columns in LDS and its workgroup covers 2048 rows:
 * N0 <= 2048 (and round_up(N0,32) (2+m) sizeof(T) <= 100 KB, which 2048 points meet for every m <= 3 in both precisions).  The caller counts t and rebuilds the
 * window (refit of the raw rows + bcbf_gp_reserve) before t reaches tcap.  Follows the reference's refit-every-k loop
 * (unicycle_move_to_pose.py:340-386) with k = 1 between refits; posterior: control_affine_model.py:1051-1059. */
int bcbf_gp_tail_step_f32(const float* Lop_r, float* Vw_r, float* X_r, float* UHB_r, const float* ell, const float* s2,
                          const float* Bm, const float* M0, const float* xq, const float* x_new, const float* uh_new,
                          const float* xdot_new, const float* jitter_new, float* Rb, float* Rinv, int* info, float* Wwork,
                          float* swork, float* Mk, float* Bk, float* rawUH, float* rawY, float* rawJ, int Bt, int N0, int t,
                          int tcap, int Ncap, int Lcap, int n, int m, int do_append, void* stream);
int bcbf_gp_tail_step_f64(const double* Lop_r, double* Vw_r, double* X_r, double* UHB_r, const double* ell, const double* s2,
                          const double* Bm, const double* M0, const double* xq, const double* x_new, const double* uh_new,
                          const double* xdot_new, const double* jitter_new, double* Rb, double* Rinv, int* info, double* Wwork,
                          double* swork, double* Mk, double* Bk, double* rawUH, double* rawY, double* rawJ, int Bt, int N0, int t,
                          int tcap, int Ncap, int Lcap, int n, int m, int do_append, void* stream);

/* GROWTH with a row-major tail: a model that keeps growing (no window, BASELINE configs[4]) commits its tail to the reserved column
 * layout one whole 32-row block at a time -- after 32 bcbf_gp_tail_step appends on a window of N0 points (N0 a multiple of 32,
 * Lop_r = bcbf_gp_reserve's output for capacity Ncap >= N0 + 32, Lcap = Ncap) this writes rows N0 .. N0+31 of every column (32
 * consecutive elements per column: full 128-byte lines, where the in-place append of bcbf_gp_append_reserved writes one element
 * per line and step) and the new diagonal block's inverse (Rinv) in both of the layout's forms.  t must be 32; the caller then
 * continues with N0 + 32, t = 0.  X_r / UHB_r / Vw_r already hold the rows (the tail step wrote them). */
int bcbf_gp_tail_commit_f32(float* Lop_r, const float* Rb, const float* Rinv, int Bt, int N0, int t, int tcap, int Ncap, void* stream);
int bcbf_gp_tail_commit_f64(double* Lop_r, const double* Rb, const double* Rinv, int Bt, int N0, int t, int tcap, int Ncap, void* stream);

/* The online entry points above with the OPT-IN data kernels (no reference counterpart: the reference has no Matern kernel;
 * BASELINE.json:north_star names an "RBF x Matern" kernel build): kernel_kind 0 = RBF (identical to the plain entry points),
 * 1 = Matern-5/2, 2 = RBF x Matern-5/2 (bcbf_refit_matern52 / bcbf_refit_rbfm52 build the state).  Same arguments, argument
 * checks, layouts and limits as their namesakes; BCBF_EINVAL for another kind.
 *   bcbf_gp_append_stream_kind      bcbf_gp_append_stream: the forward solve W = L^-1 Phi(x_new) on that kind's streaming kernel;
 *   bcbf_posterior_query_reserved_kind, bcbf_gp_append_reserved_kind (rawUH = rawY = rawJ = NULL: bcbf_gp_append_reserved,
 *                                   else bcbf_gp_append_reserved_raw): the ride-along query, the append's own column and the
 *                                   fallback passes all evaluate the kind;
 *   bcbf_gp_tail_step_kind          bcbf_gp_tail_step: the streaming pass in front, the tail rows k(x_p, xq), k(x_p, x_new).
 * bcbf_gp_reserve, bcbf_gp_tail_commit and bcbf_chol_append do not evaluate the data kernel; a window's host-free refit:
 * bcbf_refit_matern52 / bcbf_refit_rbfm52 + bcbf_refit_retry_kind. */
int bcbf_gp_append_stream_kind_f32(const float* Lop_in, const float* Vw_in, const float* X_in, const float* UHB_in,
                                   const float* ell, const float* s2, const float* Bm, const float* M0, const float* x_new,
                                   const float* uh_new, const float* xdot_new, const float* jitter_new, float* Lop_out,
                                   float* Vw_out, float* X_out, float* UHB_out, int* info, float* Wwork, float* Mk_work,
                                   float* Bk_work, int Bt, int N, int n, int m, int kernel_kind, void* stream);
int bcbf_gp_append_stream_kind_f64(const double* Lop_in, const double* Vw_in, const double* X_in, const double* UHB_in,
                                   const double* ell, const double* s2, const double* Bm, const double* M0,
                                   const double* x_new, const double* uh_new, const double* xdot_new,
                                   const double* jitter_new, double* Lop_out, double* Vw_out, double* X_out, double* UHB_out,
                                   int* info, double* Wwork, double* Mk_work, double* Bk_work, int Bt, int N, int n, int m,
                                   int kernel_kind, void* stream);
int bcbf_posterior_query_reserved_kind_f32(const float* Lop_r, const float* Vw_r, const float* X_r, const float* UHB_r,
                                           const float* ell, const float* s2, const float* Bm, const float* M0,
                                           const float* xq, const float* jitter2, float* Mk, float* Bk, float* W, int Bt,
                                           int N, int Ncap, int n, int m, int kernel_kind, void* stream);
int bcbf_posterior_query_reserved_kind_f64(const double* Lop_r, const double* Vw_r, const double* X_r, const double* UHB_r,
                                           const double* ell, const double* s2, const double* Bm, const double* M0,
                                           const double* xq, const double* jitter2, double* Mk, double* Bk, double* W, int Bt,
                                           int N, int Ncap, int n, int m, int kernel_kind, void* stream);
int bcbf_gp_append_reserved_kind_f32(float* Lop_r, float* Vw_r, float* X_r, float* UHB_r, const float* ell, const float* s2,
                                     const float* Bm, const float* M0, const float* x_new, const float* uh_new,
                                     const float* xdot_new, const float* jitter_new, int* info, float* Wwork, float* Mk_work,
                                     float* Bk_work, const float* xq, float* Mk, float* Bk, float* rawUH, float* rawY,
                                     float* rawJ, int Bt, int N, int Ncap, int n, int m, int kernel_kind, void* stream);
int bcbf_gp_append_reserved_kind_f64(double* Lop_r, double* Vw_r, double* X_r, double* UHB_r, const double* ell,
                                     const double* s2, const double* Bm, const double* M0, const double* x_new,
                                     const double* uh_new, const double* xdot_new, const double* jitter_new, int* info,
                                     double* Wwork, double* Mk_work, double* Bk_work, const double* xq, double* Mk, double* Bk,
                                     double* rawUH, double* rawY, double* rawJ, int Bt, int N, int Ncap, int n, int m,
                                     int kernel_kind, void* stream);
int bcbf_gp_tail_step_kind_f32(const float* Lop_r, float* Vw_r, float* X_r, float* UHB_r, const float* ell, const float* s2,
                               const float* Bm, const float* M0, const float* xq, const float* x_new, const float* uh_new,
                               const float* xdot_new, const float* jitter_new, float* Rb, float* Rinv, int* info,
                               float* Wwork, float* swork, float* Mk, float* Bk, float* rawUH, float* rawY, float* rawJ, int Bt,
                               int N0, int t, int tcap, int Ncap, int Lcap, int n, int m, int do_append, int kernel_kind,
                               void* stream);
int bcbf_gp_tail_step_kind_f64(const double* Lop_r, double* Vw_r, double* X_r, double* UHB_r, const double* ell,
                               const double* s2, const double* Bm, const double* M0, const double* xq, const double* x_new,
                               const double* uh_new, const double* xdot_new, const double* jitter_new, double* Rb,
                               double* Rinv, int* info, double* Wwork, double* swork, double* Mk, double* Bk, double* rawUH,
                               double* rawY, double* rawJ, int Bt, int N0, int t, int tcap, int Ncap, int Lcap, int n, int m,
                               int do_append, int kernel_kind, void* stream);

/* Dense K_b^-1 [Bt,N,N] from the packed factor (fit path): the potrs solve on identity columns, one workgroup per
 * 8 columns. */
int bcbf_potri_f32(const float* Lop, float* Kinv, int Bt, int N, void* stream);
int bcbf_potri_f64(const double* Lop, double* Kinv, int Bt, int N, void* stream);
/* Dense inverse of the Cholesky factor, Linv[Bt,N,N] = L^-1 (lower triangular, zeros above): the forward half of
 * bcbf_potri (whose backward half is latency bound: 2 ms at N = 512 for ONE model). */
/* (batches, Bt >= 4: blocked on the matrix cores, csrc/trtri.hip -- one wave per 32-column block column, X_IJ = -inv(L_II) sum_K
 * L_IK X_KJ as MFMA chains; fewer models: the forward half of bcbf_potri.  Output: the full lower-triangular matrix, zeros above
 * the diagonal.) */
int bcbf_trtri_f32(const float* Lop, float* Linv, int Bt, int N, void* stream);
int bcbf_trtri_f64(const double* Lop, double* Linv, int Bt, int N, void* stream);
/* K_b^-1 = Linv' Linv [Bt,N,N] (full symmetric matrix) from the dense triangular inverse of bcbf_trtri: 32 x 32 output tiles
 * on the matrix cores, one wave per tile, the contraction restricted to the rows below both tiles (Linv is lower
 * triangular); the mirror tile is written from the same accumulators.  The fit path's K_b^-1 (no BLAS library call). */
int bcbf_syrk_lt_f32(const float* Linv, float* Kinv, int Bt, int N, void* stream);
int bcbf_syrk_lt_f64(const double* Linv, double* Kinv, int Bt, int N, void* stream);

/* K12 -- hyper-parameter fit support (ControlAffineRegressor.fit, control_affine_model.py:268-335):
 * the O(N^2) sums of the gradient of  log p(Y) = -1/2 tr(A^-1 R'K_b^-1 R) - n/2 logdet K_b - N/2 logdet A - Nn/2 log 2pi
 * (R = Xdot - UH M0) with respect to the data-kernel parameters and B, for given alpha = K_b^-1 R [Bt,N,n] (bcbf_potrs)
 * and dense K_b^-1 [Bt,N,N] (bcbf_potri):
 *   g_ell[Bt,n] = d/d ell, g_s2[Bt] = d/d s2, g_B[Bt,C,C] = d/dB (B treated as unconstrained, symmetric result),
 *   logdetK[Bt], RtA[Bt,n,n] = R'alpha, UHtA[Bt,C,n] = UH'alpha  (value, d/dA and d/dM0 follow on the host from these).
 * work: bcbf_mll_grad_work_bytes(Bt, N, m) bytes of device memory, or NULL.  With few models (Bt < 64) the N^2 pair terms of
 * each are split over up to 128 workgroups whose partial sums (fp64, in `work`) a second launch adds in a fixed order:
 * the result is bit-identical from run to run.  NULL: one workgroup per model (same numbers up to summation order, slower
 * for a single model: 2 ms instead of 0.1 ms at N = 512). */
size_t bcbf_mll_grad_work_bytes(int Bt, int N, int m);
int bcbf_mll_grad_f32(const float* Lop, const float* alpha, const float* Kinv, const float* X, const float* UH,
                      const float* R, const float* Ainv, const float* Bm, const float* ell, const float* s2, float* g_ell,
                      float* g_s2, float* g_B, float* logdetK, float* RtA, float* UHtA, int Bt, int N, int n, int m,
                      void* work, void* stream);
int bcbf_mll_grad_f64(const double* Lop, const double* alpha, const double* Kinv, const double* X, const double* UH,
                      const double* R, const double* Ainv, const double* Bm, const double* ell, const double* s2,
                      double* g_ell, double* g_s2, double* g_B, double* logdetK, double* RtA, double* UHtA, int Bt, int N,
                      int n, int m, void* work, void* stream);

/* Batched hyper-parameter fit (SURVEY 8f #1 for MANY models; ControlAffineRegressor.fit, control_affine_model.py:268-335 of the
 * reference: ExactMarginalLogLikelihood + autograd through gpytorch's softplus / IndexKernel parameterisation + torch.optim.Adam
 * under MultiStepLR, one model at a time).  theta[Bt,P] holds the reference's RAW parameters of every model,
 *   [ base_kernel.raw_lengthscale (n) | raw_outputscale (1) | task_covar.U.covar_factor (n x rA, row-major) | U.raw_var (n)
 *     | task_covar.V.covar_factor (C x rB) | V.raw_var (C) | mean_module constants (C x n) ],  C = 1 + m,
 *   P = bcbf_fit_param_count(n, m, rA, rB)   (rA, rB = the IndexKernel ranks: n and C by default, 1 "RankOne", 0 "Diag").
 * bcbf_fit_derive: ell[Bt,n] = softplus, s2[Bt] = softplus, A[Bt,n,n] = Wa Wa' + diag softplus(va), Bm[Bt,C,C] likewise,
 *   M0[Bt,C,n], and (optional, NULL to skip) Ainv[Bt,n,n], logdetA[Bt] -- the inputs of bcbf_refit / bcbf_mll_grad.
 * bcbf_fit_adam_step: from bcbf_mll_grad's outputs (g_ell, g_s2, g_B, logdetK, RtA, UHtA) and Ainv / logdetA:
 *   loss[b] = (-log p(Y_b) - log GammaPrior(ell_b)) / (N n)  (gamma_prior = {concentration, rate} or NULL),
 *   grad_out[Bt,P] (optional) = d loss / d theta by the chain rule (:164-171, :268-335), and -- step >= 1 -- ONE update of
 *   torch.optim.Adam(lr, betas = (beta1, beta2), eps) on theta with the moment buffers mom1, mom2 [Bt,P] (zero before step 1);
 *   step = 0: value and gradient only.  skip[b] != 0 (optional): model b is left untouched, loss[b] = NaN.
 * bcbf_kinv_apply: alpha[Bt,N,nt] = Kinv[Bt,N,N] R[Bt,N,nt] for the dense SYMMETRIC K_b^-1 of bcbf_trtri + bcbf_syrk_lt
 *   (nt <= 8) -- replaces the library GEMM `Kinv @ R` of a fit iteration.
 * One iteration = derive, bcbf_refit, bcbf_trtri, bcbf_syrk_lt, bcbf_kinv_apply, bcbf_mll_grad, adam_step: no host round trip
 * except the caller's look at bcbf_refit's info (make_psd's x10 jitter retry, :899-921). */
int bcbf_fit_param_count(int n, int m, int rA, int rB);
int bcbf_fit_derive_f32(const float* theta, float* ell, float* s2, float* A, float* Bm, float* M0, float* Ainv, float* logdetA,
                        int Bt, int n, int m, int rA, int rB, void* stream);
int bcbf_fit_derive_f64(const double* theta, double* ell, double* s2, double* A, double* Bm, double* M0, double* Ainv,
                        double* logdetA, int Bt, int n, int m, int rA, int rB, void* stream);
int bcbf_fit_adam_step_f32(float* theta, float* mom1, float* mom2, const float* g_ell, const float* g_s2, const float* g_B,
                           const float* logdetK, const float* RtA, const float* UHtA, const float* Ainv, const float* logdetA,
                           const int* skip, float* loss, float* grad_out, int Bt, int N, int n, int m, int rA, int rB, int step,
                           double lr, double beta1, double beta2, double eps, const double* gamma_prior, void* stream);
int bcbf_fit_adam_step_f64(double* theta, double* mom1, double* mom2, const double* g_ell, const double* g_s2, const double* g_B,
                           const double* logdetK, const double* RtA, const double* UHtA, const double* Ainv, const double* logdetA,
                           const int* skip, double* loss, double* grad_out, int Bt, int N, int n, int m, int rA, int rB, int step,
                           double lr, double beta1, double beta2, double eps, const double* gamma_prior, void* stream);
int bcbf_kinv_apply_f32(const float* Kinv, const float* R, float* alpha, int Bt, int N, int nt, void* stream);
int bcbf_kinv_apply_f64(const double* Kinv, const double* R, double* alpha, int Bt, int N, int nt, void* stream);

/* K4+K5+K6+K7: one posterior query per instance (the HBM-bound hot kernel).
 *   Phi = diag(k(X, xq)) UHB;  W = L^-1 Phi;  Mk = M0' + Vw' W;  Bk = s2*Bm - W'W (+ diag(jitter2))
 * Replaces ControlAffineRegressorExact._custom_predict_matrix with b = 1
 * (control_affine_model.py:1051-1091; same numbers as custom_predict :536-602).
 * Lop[Bt,lop_elems] Vw[Bt,N,n] X[Bt,N,n] UHB[Bt,N,C] ell[Bt,n] s2[Bt] Bm[Bt,C,C] M0[Bt,C,n]
 * xq[Bt,n] jitter2[Bt,C] (may be NULL) -> Mk[Bt,n,C], Bk[Bt,C,C]. */
int bcbf_posterior_step_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                            const float* ell, const float* s2, const float* Bm, const float* M0,
                            const float* xq, const float* jitter2, float* Mk, float* Bk,
                            int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_step_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                            const double* ell, const double* s2, const double* Bm, const double* M0,
                            const double* xq, const double* jitter2, double* Mk, double* Bk,
                            int Bt, int N, int n, int m, void* stream);

/* Same kernel, query form.  shared != 0: all Bt queries are evaluated against ONE GP (instance 0 of
 * Lop/Vw/X/UHB/ell/s2/Bm/M0) -- the reference's own batched API, custom_predict with b test points
 * (control_affine_model.py:536, 1051).  W (optional, [Bt, Np, C], Np = N rounded up to 32) receives
 * L^-1 Phi(x_b) so the caller can form cross-covariances B_k(x,x') = k(x,x') Bm - W(x)'W(x') (:586, :1079-1088). */
int bcbf_posterior_query_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                             const float* ell, const float* s2, const float* Bm, const float* M0,
                             const float* xq, const float* jitter2, float* Mk, float* Bk, float* W,
                             int shared, int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_query_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                             const double* ell, const double* s2, const double* Bm, const double* M0,
                             const double* xq, const double* jitter2, double* Mk, double* Bk, double* W,
                             int shared, int Bt, int N, int n, int m, void* stream);

/* Regime S on the matrix cores (fp32; N up to ~1600, while Np*(2n+m+17)*4 bytes fit the 160 KB LDS): Bt queries
 * against ONE GP (instance 0 of the GP tensors), 4 queries per wavefront, blocked forward substitution with
 * v_mfma_f32_16x16x4_f32 against the cache-resident factor (N <= 512 and n <= 4: the solution stays in registers,
 * as in the fp64 entry below; larger models keep it in LDS).  Same outputs as bcbf_posterior_query_f32(shared=1), which routes here for Bt >= 16.  Replaces
 * custom_predict with b test points (control_affine_model.py:536-602, 1051-1091). */
int bcbf_posterior_shared_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                              const float* ell, const float* s2, const float* Bm, const float* M0,
                              const float* xq, const float* jitter2, float* Mk, float* Bk, float* W,
                              int Bt, int N, int n, int m, void* stream);
/* The same in fp64 (the reference's unicycle module runs in float64, unicycle_move_to_pose.py:50), N <= 512, n <= 4:
 * v_mfma_f64_16x16x4_f64, 4 queries per wavefront, the solution L^-1 Phi held in registers.
 * bcbf_posterior_query_f64(shared=1) routes here for Bt >= 16, N <= 512 and n <= 4; BCBF_EINVAL outside that range. */
int bcbf_posterior_shared_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                              const double* ell, const double* s2, const double* Bm, const double* M0,
                              const double* xq, const double* jitter2, double* Mk, double* Bk, double* W,
                              int Bt, int N, int n, int m, void* stream);
/* The two matrix-core queries above with the opt-in Matern-5/2 data kernel (see bcbf_posterior_query_matern52; same ranges;
 * bcbf_posterior_query_matern52(shared=1) routes here for Bt >= 16).  No reference counterpart: the reference has no Matern
 * kernel -- BASELINE.json's north_star names one; parity unpinned, formula held to the CPU oracle. */
int bcbf_posterior_shared_matern52_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                       const float* ell, const float* s2, const float* Bm, const float* M0,
                                       const float* xq, const float* jitter2, float* Mk, float* Bk, float* W,
                                       int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_shared_matern52_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                       const double* ell, const double* s2, const double* Bm, const double* M0,
                                       const double* xq, const double* jitter2, double* Mk, double* Bk, double* W,
                                       int Bt, int N, int n, int m, void* stream);

/* Full predictive covariance of a query SET against one GP in one launch, from the Gram G[b, b', 1+m, 1+m] = W_b' Wp_b' of the
 * whitened cross-covariances of its points (W = L^-1 Phi: the W output of bcbf_posterior_query / _shared; the Gram is a plain
 * GEMM on the caller's side):
 *   BkXX[b, b', 1+m, 1+m] = k(x_b, x'_b') Bm - G[b, b']   (+ jitter[b (1+m) + c] on the entries b = b', c = d: the make_psd
 *                           draw of the reference, control_affine_model.py:1089; jitter may be NULL and needs b == b')
 *   Kron[b (1+m) n, b' (1+m) n] = kron(Bk2, A), Bk2 = BkXX with the axes ordered (b, c, b', d)   (torch_kron(Bk2, A), :978)
 * Either output may be NULL.  Xq[b, n], Xqp[bp, n] the test points, ell[n], s2[1], Bm[(1+m)^2], A[n^2] of the one model;
 * kernel_kind 0 = RBF, 1 = the opt-in Matern-5/2.  Replaces the tail of ControlAffineRegressorExact._custom_predict_matrix
 * and custom_predict_fullmat (control_affine_model.py:1051-1091, 963-980: k_b(X*, X*) B - v'v, make_psd, the Kronecker
 * product -- ~20 torch launches on the host path of the published speed test, pendulum.py:1367-1372). */
int bcbf_predict_assemble_f32(const float* G, const float* Xq, const float* Xqp, const float* ell, const float* s2,
                              const float* Bm, const float* A, const float* jitter, float* BkXX, float* Kron, int b, int bp,
                              int n, int m, int kernel_kind, void* stream);
int bcbf_predict_assemble_f64(const double* G, const double* Xq, const double* Xqp, const double* ell, const double* s2,
                              const double* Bm, const double* A, const double* jitter, double* BkXX, double* Kron, int b, int bp,
                              int n, int m, int kernel_kind, void* stream);

/* Gram of whitened cross-covariances on the matrix cores: G[b,bp,C,C] = einsum("bkc,pkd->bpcd", W, Wp) for W[b,Np,C],
 * Wp[bp,Np,C] (the W output of bcbf_posterior_query / bcbf_posterior_shared; Np = N rounded up to 32; C <= 12).  Replaces the
 * library GEMMs `v.t() @ vp` (C = 1, control_affine_model.py:586) and `kb_star' Bdagger` (:1079-1088) of the reference's
 * prediction path.  W == Wp (and b == bp): the symmetric half is computed once and mirrored. */
int bcbf_gram_f32(const float* W, const float* Wp, float* G, int b, int bp, int Np, int C, void* stream);
int bcbf_gram_f64(const double* W, const double* Wp, double* G, int b, int bp, int Np, int C, void* stream);
/* ControlAffineRegressorExact.custom_predict_fullmat (control_affine_model.py:963-980) behind a cached factor, ONE host call:
 * bcbf_posterior_query(shared = 1, W) -> bcbf_gram -> bcbf_predict_assemble on `stream`.  GP tensors of one model (leading axis
 * 1), A[n,n], Xq[b,n], jitter[b(1+m)] (the make_psd draw, may be NULL) -> Mk[b,n,1+m], and BkXX[b,b,1+m,1+m] and / or
 * Kron[b(1+m)n, b(1+m)n]; Bk[b,1+m,1+m], W[b,Np,1+m], G[b,b,1+m,1+m] are caller-provided work arrays (kept as outputs). */
int bcbf_predict_fullmat_f32(const float* Lop, const float* Vw, const float* X, const float* UHB, const float* ell,
                             const float* s2, const float* Bm, const float* M0, const float* A, const float* Xq,
                             const float* jitter, float* Mk, float* Bk, float* W, float* G, float* BkXX, float* Kron, int b,
                             int N, int n, int m, int kernel_kind, void* stream);
int bcbf_predict_fullmat_f64(const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell,
                             const double* s2, const double* Bm, const double* M0, const double* A, const double* Xq,
                             const double* jitter, double* Mk, double* Bk, double* W, double* G, double* BkXX, double* Kron,
                             int b, int N, int n, int m, int kernel_kind, void* stream);

/* Posterior jets: value and first x-derivatives of the posterior factors (one query per instance, or per
 * query of a shared GP).  CT = (1+m)(1+n) right-hand sides [Phi, dPhi/dx_1 .. dPhi/dx_n] of the same stream:
 *   G[Bt,CT,CT] = Wj'Wj,  Mj[Bt,n,CT] = Vw'Wj   (Mk = M0' + Mj[:, :C]; dMk/dx_d = Mj[:, (1+d)C:(2+d)C]),
 * plus Mk, Bk as bcbf_posterior_step.  Wj (optional, may be NULL): [Bt, Np, CT] = L^-1 [Phi, dPhi/dx_d] itself
 * (Np = N rounded up to 32), from which the caller forms derivative kernels between two DIFFERENT states,
 * d/dx_d d/dx'_e B_k(x,x') = d2k/dx_d dx'_e Bm - dW_d(x)'dW_e(x')  (GradientGP.knl(x, x'), gp_algebra.py:355-393).
 * Replaces autograd through custom_predict inside GradientGP (gp_algebra.py:340-402).
 * Every (n <= 4, m <= 3) is compiled (shapes with (1+m)(1+n) + n > 16 use two matrix-core tile columns). */
int bcbf_posterior_jets_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                            const float* ell, const float* s2, const float* Bm, const float* M0,
                            const float* xq, float* Mk, float* Bk, float* G, float* Mj, float* Wj, int shared,
                            int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_jets_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                            const double* ell, const double* s2, const double* Bm, const double* M0,
                            const double* xq, double* Mk, double* Bk, double* G, double* Mj, double* Wj, int shared,
                            int Bt, int N, int n, int m, void* stream);

/* K8, rel-degree 2: CBC2 = grad(L_f h)'(f + g u) + kalpha[0] h + kalpha[1] L_f h as a GP in u, closed form of
 * cbc2_gp + cbc2_quadratic_terms (cbc2.py:7-33; gp_algebra.py:133-168, 319-402) from the jets.
 * h[Bt], gh[Bt,n], Hh[Bt,n,n] = barrier value, gradient, Hessian at x; u0[Bt,m] linearisation point (the
 * cross term cov(grad L_f h, f+gu) is frozen there, as the reference's autograd does); kalpha[2].
 * out[Bt, m+1+m*m+m+1+2] = (mean_A[m], mean_b, Q[m,m], p[m], r, mean(u0), var(u0));
 * The kernel Hessian d2 k_{L_f h} / dx dx' at x' = x goes through the reference's eigenvalue clean-up
 * (gp_algebra.py:384-392): hessian_mode 0 = the reference's formula `eigenvectors.T @ diag(evalz) @ eigenvectors` on the
 * eigenvectors of the GENERAL solver (xGEEV's order and signs, csrc/geev_small.h); 1 = the spectral projection
 * V max(L,0) V' of the symmetric part (what rounds 1-3 did; differs from the reference whenever the branch runs).
 * WHICH branch runs (mode 0) is decided as the reference decides it, from the real parts of the general solver's
 * eigenvalues of H itself (`evalz > -EPS`, `evalz < 0`); only a symmetric part that is positive definite by a wide margin
 * (unpivoted Cholesky, every pivot > 1e-10 of the trace) skips the solver, and only a complex pair / non-convergence falls
 * back to the eigenvalues of the symmetric part (status 6).
 * kernel_kind: the data kernel the jets came from, 0 = RBF (the reference's), 1 = Matern-5/2, 2 = RBF x Matern-5/2 (the prior term
 * d2 k / dx_d dx'_d at x' = x is (5/3) s2 / ell_d^2 instead of s2 / ell_d^2).
 * status[Bt] (optional): 0 = nothing to clean, 1 = an eigenvalue <= -2e-3 (the reference asserts), 4 = eigenvalues in
 * (-2e-3, 0) were zeroed, 6 = zeroed through the projection because xGEEV's path met a complex pair. */
int bcbf_cbc2_terms_f32(const float* Mk, const float* Bk, const float* G, const float* Mj, const float* A,
                        const float* Bm, const float* ell, const float* s2, const float* h, const float* gh,
                        const float* Hh, const float* kalpha, const float* u0, float* out, int* status,
                        int Bt, int n, int m, int hessian_mode, int kernel_kind, void* stream);
int bcbf_cbc2_terms_f64(const double* Mk, const double* Bk, const double* G, const double* Mj, const double* A,
                        const double* Bm, const double* ell, const double* s2, const double* h, const double* gh,
                        const double* Hh, const double* kalpha, const double* u0, double* out, int* status,
                        int Bt, int n, int m, int hessian_mode, int kernel_kind, void* stream);

/* The clean-up of gp_algebra.py:384-392 alone, on a batch of n x n matrices (row-major, n <= 4): every eigenvalue must
 * be > -eps (else status 1 and the matrix is returned unchanged); eigenvalues in (-eps, 0) are zeroed and the matrix
 * rebuilt (mode / status as in bcbf_cbc2_terms).  Hout may alias Hin.  Replaces the torch.eig block of GradientGP.knl. */
int bcbf_clean_hessian_f32(const float* Hin, float* Hout, int* status, int Bt, int n, double eps, int mode, void* stream);
int bcbf_clean_hessian_f64(const double* Hin, double* Hout, int* status, int Bt, int n, double eps, int mode, void* stream);

/* K8 (rel-degree 1) + K9: constraint terms and their cone form, K constraints per instance.
 *   mean(u) = bfe'u + e,  var(u) = u'V u + bfv'u + v   for  sign*(grad' (fhat + ghat u + F(x)[1;u]) + cst)
 * Replaces cbc2_quadratic_terms on a rel-degree-1 expression (cbc2.py:7-23, gp_algebra.py:109-223,
 * unicycle_move_to_pose.py:880-916) and convert_cbc_terms_to_socp_terms (:837-878).
 * Mk[Bt,n,C] Bk[Bt,C,C] A[Bt,n,n] grad[Bt,K,n] cst[Bt,K] sign[K] fhat[Bt,n] ghat[Bt,n,m]
 * -> terms[Bt,K,T] with T = m + 1 + m*m + m + 1 packed (bfe,e,V,bfv,v);
 *    cones[Bt,K,Q] with Q = (m+1)*m + (m+1) + m + 1 packed (A[(m+1),m], b[m+1], c[m], d);
 *    cstatus[Bt,K] = 0 or BCBF_SOCP_BADCONE.  terms / cones may be NULL. */
int bcbf_cbc_terms_f32(const float* Mk, const float* Bk, const float* A, const float* grad, const float* cst,
                       const float* sign, const float* fhat, const float* ghat,
                       float* terms, float* cones, int* cstatus, int Bt, int K, int n, int m, void* stream);
int bcbf_cbc_terms_f64(const double* Mk, const double* Bk, const double* A, const double* grad, const double* cst,
                       const double* sign, const double* fhat, const double* ghat,
                       double* terms, double* cones, int* cstatus, int Bt, int K, int n, int m, void* stream);

/* K10: the per-step program of ControllerCLFBayesian.control (unicycle_move_to_pose.py:926-953):
 *   min sum_i w_i (u_i - r_i)^2 + w_m relax^2   s.t.  c_k'u + d_k + relax_mask_k relax >= rho |A_k u + b_k|
 * Replaces cvxpy+GUROBI (and cvxopt socp, optimizers.py:42-102).  One primal-dual interior-point
 * solve (NT scaling, Mehrotra correction) per instance in registers, four lanes per instance.
 * w[Bt,m+1] r[Bt,m] cones[Bt,K,Q] (layout above) relax_mask[K] rho[Bt]
 * -> y[Bt,m+1] = [u, relax], status[Bt], iters[Bt] (iters may be NULL). */
int bcbf_socp_f32(const float* w, const float* r, const float* cones, const float* relax_mask, const float* rho,
                  float* y, int* status, int* iters, int Bt, int K, int m, int max_iters, void* stream);
int bcbf_socp_f64(const double* w, const double* r, const double* cones, const double* relax_mask, const double* rho,
                  double* y, int* status, int* iters, int Bt, int K, int m, int max_iters, void* stream);

/* K8+K9+K10 fused: bcbf_cbc_terms followed by bcbf_socp in one launch (four lanes per instance, lane k
 * owns constraint k); same inputs and outputs, terms / cones / cstatus optional (may be NULL). */
int bcbf_cbc_socp_f32(const float* Mk, const float* Bk, const float* A, const float* grad, const float* cst,
                      const float* sign, const float* fhat, const float* ghat, const float* w, const float* r,
                      const float* relax_mask, const float* rho, float* terms, float* cones, int* cstatus,
                      float* y, int* status, int* iters, int Bt, int K, int n, int m, int max_iters, void* stream);
int bcbf_cbc_socp_f64(const double* Mk, const double* Bk, const double* A, const double* grad, const double* cst,
                      const double* sign, const double* fhat, const double* ghat, const double* w, const double* r,
                      const double* relax_mask, const double* rho, double* terms, double* cones, int* cstatus,
                      double* y, int* status, int* iters, int Bt, int K, int n, int m, int max_iters, void* stream);

/* Generic small cone QP (the reference's optimizer_socp_* / optimizer_qp_cvxpy, optimizers.py:42-116):
 *   min 1/2 x'P x + q'x  s.t.  G x + s = h,  s in R_+^l x Q^{q_1} x ... x Q^{q_nq}
 * P[Bt,nv,nv] q[Bt,nv] G[Bt,Kt,nv] h[Bt,Kt], Kt = l + sum(qdims), l <= 8, every cone dimension <= 6, nv <= 6,
 * nq <= BCBF_MAX_CONSTRAINTS (up to 4 cones run the register-resident instantiation, more a wider, slower one);
 * qdims is a HOST array.  -> x[Bt,nv], status[Bt], iters[Bt] (may be NULL). */
int bcbf_coneqp_f64(const double* P, const double* q, const double* G, const double* h,
                    int nv, int l, const int* qdims, int nq,
                    double* x, int* status, int* iters, int Bt, int max_iters, void* stream);

/* ---- RBF + Linear data kernel (the CoGP / diag comparators of the published speed test) ----
 * k(x,x') = s2 (exp(-1/2 |(x-x')/ell|^2) + lin x'x'),  lin[Bt]: gpytorch ScaleKernel(RBFKernel() + LinearKernel()) of
 * ControlAffineVectorGP (control_affine_model.py:1106-1126).  The CoGP system of N n scalar observations,
 *   K[(i,a),(j,c)] = k(x_i,x_j) [(uh_i' (x) I_n) Sigma (uh_j (x) I_n)]_ac            (:1203-1230),
 * is the matrix-variate structure K = k(X',X') o (UH' Sigma UH'') with expanded inputs X'[(i,a)] = x_i,
 * UH'[(i,a),(p,a')] = uh_i[p] delta_aa' (C' = (1+m) n <= 4 columns, one target column), so the factorisation,
 * solve and query kernels above serve it unchanged; these entry points only add `lin` to the kernel function.
 * Same arguments as the entry points they extend; lin == NULL means 0. */
int bcbf_kb_build_rbflin_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                             const float* lin, const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream);
int bcbf_kb_build_rbflin_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                             const double* lin, const double* jitter, double* Kb, int Bt, int N, int n, int m,
                             void* stream);
int bcbf_posterior_query_rbflin_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                    const float* ell, const float* s2, const float* lin, const float* Bm,
                                    const float* M0, const float* xq, const float* jitter2, float* Mk,
                                    float* Bk, float* W, int shared, int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_query_rbflin_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                    const double* ell, const double* s2, const double* lin, const double* Bm,
                                    const double* M0, const double* xq, const double* jitter2, double* Mk,
                                    double* Bk, double* W, int shared, int Bt, int N, int n, int m, void* stream);
/* bcbf_mll_grad with nt target columns (R, alpha [Bt,N,nt]; Ainv, RtA [Bt,nt,nt]; UHtA [Bt,C,nt]) and the extra
 * output g_lin[Bt] = d log p / d lin.  C = m + 1 up to BCBF_MAX_TASK_DIM (C nt <= 128). */
int bcbf_mll_grad_rbflin_f32(const float* Lop, const float* alpha, const float* Kinv, const float* X, const float* UH,
                             const float* R, const float* Ainv, const float* Bm, const float* ell, const float* s2,
                             const float* lin, float* g_ell, float* g_s2, float* g_lin, float* g_B, float* logdetK,
                             float* RtA, float* UHtA, int Bt, int N, int n, int m, int nt, void* work, void* stream);
int bcbf_mll_grad_rbflin_f64(const double* Lop, const double* alpha, const double* Kinv, const double* X,
                             const double* UH, const double* R, const double* Ainv, const double* Bm, const double* ell,
                             const double* s2, const double* lin, double* g_ell, double* g_s2, double* g_lin,
                             double* g_B, double* logdetK, double* RtA, double* UHtA, int Bt, int N, int n, int m,
                             int nt, void* work, void* stream);

/* K9 for the generic controllers (controllers.py): rows of the cone program of SOCPController.control (:569-591)
 * / QPController.control (:638-662) over y = [extravars.., u], in the layout bcbf_coneqp_f64 takes
 * (optimizers.py:6-39: |A y + b| <= c'y + d  ->  Gq = [-c'; -A], hq = [d; b]).
 * terms[Bt,K,T] packed (bfe,e,V,bfv,v) as written by bcbf_cbc_terms / bcbf_cbc2_terms; kind[K], factor[K] are
 * HOST arrays.  kind 0 = convert_cbc_terms_to_socp_terms (:423-482, L' form, retry with +1e-3 I, relaxation
 * column extravars-1), kind 1 = _socp_safety (:502-540, lower factor L as the reference has it, times factor;
 * symmetric-eigen fallback sqrt(max(Lambda,0)) V' when a pivot is not positive), kind 2 = the linear row
 * 0 <= c'y + d of QPController._qp_stability (:614-629).  objective != 0 (extravars == 2) adds the epigraph cone of
 * _socp_objective (:396-420) built from u_ref[Bt,m], ctrl_reg, relax_weight.
 * Row order: kind-2 rows, objective cone, then the kind-0/1 cones in input order (m+2 rows each);
 * Kt = bcbf_controller_cones_rows(kind, K, m, objective).  -> G[Bt,Kt,extravars+m], h[Bt,Kt] (fp64),
 * cstatus[Bt,K] (optional; BCBF_SOCP_BADCONE when kind 0 cannot be factored). */
int bcbf_controller_cones_rows(const int* kind, int K, int m, int objective);
int bcbf_controller_cones_f32(const float* terms, const float* u_ref, const int* kind, const double* factor,
                              double ctrl_reg, double relax_weight, int extravars, int objective, double* G, double* h,
                              int* cstatus, int Bt, int K, int m, void* stream);
int bcbf_controller_cones_f64(const double* terms, const double* u_ref, const int* kind, const double* factor,
                              double ctrl_reg, double relax_weight, int extravars, int objective, double* G, double* h,
                              int* cstatus, int Bt, int K, int m, void* stream);

/* Unicycle task functions, batched (unicycle_move_to_pose.py:522-615 CLFCartesian, :618-696
 * ObstacleCBF, :235-257 AckermannDrive.g_func, planner.py:54-64 PiecewiseLinearPlanner).
 * x[Bt,3] plan[Bt,3] dot_plan[Bt,3] Kp[3] clf_gamma; obstacles: centers[Bt,Kob,2] radii[Bt,Kob]
 * tw[2] gammas[Kob]; L_mean -> grad[Bt,1+Kob,3], cst[Bt,1+Kob], fhat[Bt,3], ghat[Bt,3,2].
 * Row 0 is the CLC (sign -1 is applied by bcbf_cbc_terms via `sign`), rows 1.. the obstacles. */
int bcbf_unicycle_constraints_f32(const float* x, const float* plan, const float* dot_plan, const float* Kp,
                                  float clf_gamma, const float* centers, const float* radii, const float* tw,
                                  const float* gammas, float L_mean, float* grad, float* cst, float* fhat,
                                  float* ghat, int Bt, int Kob, void* stream);
int bcbf_unicycle_constraints_f64(const double* x, const double* plan, const double* dot_plan, const double* Kp,
                                  double clf_gamma, const double* centers, const double* radii, const double* tw,
                                  const double* gammas, double L_mean, double* grad, double* cst, double* fhat,
                                  double* ghat, int Bt, int Kob, void* stream);

/* Explicit-Euler plant step x += (g(x; L_true) u) dt  (unicycle_move_to_pose.py:277-282, sampling.py:68-74). */
int bcbf_unicycle_step_f32(float* x, const float* u, float dt, float L_true, int Bt, void* stream);
int bcbf_unicycle_step_f64(double* x, const double* u, double dt, double L_true, int Bt, void* stream);

/* One host call per control step of ControllerCLFBayesian.control on the unicycle
 * (unicycle_move_to_pose.py:926-995), TWO launches on `stream`: the posterior kernel (n=3, m=2), then one kernel
 * that does what bcbf_unicycle_constraints -> bcbf_cbc_terms (K = 1+Kob, sign[K]) -> bcbf_socp ->
 * x += g(x; L_true) u dt (skipped when dt <= 0, and for every instance whose status != BCBF_SOCP_OPTIMAL: the
 * reference raises ValueError(problem.status) there, :954-964, so an unsolved instance keeps its state and is
 * reported through status[]) do separately (each lane forms its own task row from the state).
 * Arguments are those of the individual entry points; grad/cst/fhat/ghat/Mk/Bk/cones/cstatus are caller-provided
 * workspaces that also expose the intermediates; y[Bt,3] = [u, relax].
 * ev_start / ev_stop (optional hipEvent_t) are recorded around the posterior kernel for profiling.
 * Lop == NULL: no posterior launch -- Mk/Bk are inputs (the fixed-kernel model of AckermannDrive.fu_func_gp,
 * unicycle_move_to_pose.py:262-275: Mk = 0, Bk = I, A = diag(kernel_diag_A)).
 * shared_gp != 0: every instance queries ONE learned model (instance 0 of Lop/Vw/X/UHB/ell/s2/Bm/M0; A stays per
 * instance) -- Monte-Carlo rollouts of a fixed model; the posterior then runs as bcbf_posterior_query(shared=1),
 * which for fp32 is the matrix-core kernel. */
int bcbf_unicycle_control_step_f32(
    const float* Lop, const float* Vw, const float* X, const float* UHB, const float* ell, const float* s2,
    const float* Bm, const float* M0, const float* A, float* x, const float* plan, const float* dot_plan,
    const float* Kp, float clf_gamma, const float* centers, const float* radii, const float* tw, const float* gammas,
    float L_mean, const float* w, const float* r, const float* sign, const float* relax_mask, const float* rho,
    float* grad, float* cst, float* fhat, float* ghat, float* Mk, float* Bk, float* cones, int* cstatus,
    float* y, int* status, int* iters, float dt, float L_true, int Bt, int N, int Kob, int max_iters, int shared_gp,
    void* ev_start, void* ev_stop, void* stream);
int bcbf_unicycle_control_step_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, double* x, const double* plan, const double* dot_plan,
    const double* Kp, double clf_gamma, const double* centers, const double* radii, const double* tw,
    const double* gammas, double L_mean, const double* w, const double* r, const double* sign,
    const double* relax_mask, const double* rho, double* grad, double* cst, double* fhat, double* ghat, double* Mk,
    double* Bk, double* cones, int* cstatus, double* y, int* status, int* iters, double dt, double L_true, int Bt,
    int N, int Kob, int max_iters, int shared_gp, void* ev_start, void* ev_stop, void* stream);
/* The control step of a loop that LEARNS FROM ITSELF (LearnedShiftInvariantDynamics.train / fit,
 * unicycle_move_to_pose.py:326-386: every visited (x_t, u_t) is buffered; targets are the finite differences
 * (x_{t+1} - x_t) / dt of the visited states minus the mean model f_mean + g_mean u; inputs go through
 * `_make_trans_invariant`, :326-330).  Arguments of bcbf_unicycle_control_step, plus
 *   xq[Bt,3]      where the posterior is queried (NULL: at x) -- the shift-invariant input (0, 0, theta) of the current state;
 *   obs_x, obs_uh, obs_y  (all three or none; need dt > 0): THIS step's observation, row b * obs_ld of three-column arrays
 *                 (obs_ld = 1: a [Bt,3] array; obs_ld = rows per instance: a column of a [Bt,obs_ld,3] buffer) --
 *                 obs_x = the state BEFORE the step ((0, 0, theta) when shift_invariant != 0), obs_uh = (1, u) (u = 0 where the
 *                 program was not solved: that instance's state is frozen), obs_y = (x_new - x_old) / dt - g_mean(L_mean) u
 *                 computed from the STORED (rounded) states as the reference's buffer does;
 *   xq_next[Bt,3] (optional): the regressor input at the NEW state = the next step's xq (may be the same buffer as xq);
 *   flags         bit 0: shift-invariant regressor inputs (obs_x, xq_next); bit 1: the planner's target moves on with the step,
 *                 plan[b] += dot_plan[b] dt (PiecewiseLinearPlanner, planner.py:54-64: a straight line at constant speed) --
 *                 `plan` is then written, although it is declared const for the entry points that only read it.
 * The rows go to bcbf_gp_append_reserved[_raw] / bcbf_gp_tail_step / the next bcbf_refit as they are. */
int bcbf_unicycle_control_step_observe_f32(
    const float* Lop, const float* Vw, const float* X, const float* UHB, const float* ell, const float* s2,
    const float* Bm, const float* M0, const float* A, float* x, const float* plan, const float* dot_plan,
    const float* Kp, float clf_gamma, const float* centers, const float* radii, const float* tw, const float* gammas,
    float L_mean, const float* w, const float* r, const float* sign, const float* relax_mask, const float* rho,
    float* grad, float* cst, float* fhat, float* ghat, float* Mk, float* Bk, float* cones, int* cstatus,
    float* y, int* status, int* iters, float dt, float L_true, int Bt, int N, int Kob, int max_iters, int shared_gp,
    const float* xq, float* obs_x, float* obs_uh, float* obs_y, int obs_ld, float* xq_next, int flags,
    void* ev_start, void* ev_stop, void* stream);
int bcbf_unicycle_control_step_observe_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, double* x, const double* plan, const double* dot_plan,
    const double* Kp, double clf_gamma, const double* centers, const double* radii, const double* tw,
    const double* gammas, double L_mean, const double* w, const double* r, const double* sign,
    const double* relax_mask, const double* rho, double* grad, double* cst, double* fhat, double* ghat, double* Mk,
    double* Bk, double* cones, int* cstatus, double* y, int* status, int* iters, double dt, double L_true, int Bt,
    int N, int Kob, int max_iters, int shared_gp, const double* xq, double* obs_x, double* obs_uh, double* obs_y,
    int obs_ld, double* xq_next, int flags, void* ev_start, void* ev_stop, void* stream);
/* The control step on a plant DRAWN FROM THE MODEL'S OWN POSTERIOR.  The program of the step asks that every condition hold
 * with probability >= 1 - max_risk under xdot | x, u ~ N(fhat + ghat u + M_k ubar, (ubar' B_k ubar) A), ubar = (1, u): the
 * matrix-variate posterior of fu_func_gp(u) (unicycle_move_to_pose.py:262-275).  This entry draws from that distribution, as
 * GaussianProcessBase.sample(x) does for one state (gp_algebra.py:33-34), inside the solve / plant launch: for an instance whose
 * program was solved (status == BCBF_SOCP_OPTIMAL)
 *     xdot_s = fhat + ghat u + M_k ubar + sqrt(max(ubar' B_k ubar, 0)) L_A z,     x += xdot_s dt       (dt > 0)
 *     cbc_s[b,k] = sign[k] (grad[b,k,:] . xdot_s + cst[b,k])    k = 0 the CLC row, k >= 1 the obstacles (cbc1.py:10-14)
 * with u = y as stored, fhat = 0 and ghat = g(x; L_mean) (the rows of bcbf_unicycle_control_step), A = L_A L_A' factored in the
 * kernel (a pivot <= 0 zeroes its column: a positive-semidefinite A is accepted and draws in its range); fp64 arithmetic on the
 * stored values, each output rounded once.  An unsolved instance keeps its state; its xdot_s and cbc_s rows are 0.  L_true is
 * ignored: the plant is the model's belief.  Draws of different steps are independent: the marginal at every visited (x_t, u_t)
 * is exact, which is all the per-step chance constraint speaks about; a function-consistent draw along a trajectory would have to
 * condition on the earlier draws (bcbf_gp_append) and is not what this entry does.
 * Arguments of bcbf_unicycle_control_step_observe -- the observation rows then record the sampled plant -- plus
 *   kernel_kind   the data kernel of the learned model: 0 = RBF, 1 = Matern-5/2, 2 = RBF x Matern-5/2 (the posterior launch);
 *   z[Bt,3]       standard-normal draws, the caller's: the library draws no random numbers (as bcbf_subsample_rows);
 *   xdot_s[Bt,3], cbc_s[Bt,1+Kob]   outputs, each may be NULL. */
int bcbf_unicycle_control_step_sampled_f32(
    const float* Lop, const float* Vw, const float* X, const float* UHB, const float* ell, const float* s2,
    const float* Bm, const float* M0, const float* A, float* x, const float* plan, const float* dot_plan,
    const float* Kp, float clf_gamma, const float* centers, const float* radii, const float* tw, const float* gammas,
    float L_mean, const float* w, const float* r, const float* sign, const float* relax_mask, const float* rho,
    float* grad, float* cst, float* fhat, float* ghat, float* Mk, float* Bk, float* cones, int* cstatus,
    float* y, int* status, int* iters, float dt, float L_true, int Bt, int N, int Kob, int max_iters, int shared_gp,
    const float* xq, float* obs_x, float* obs_uh, float* obs_y, int obs_ld, float* xq_next, int flags, int kernel_kind,
    const float* z, float* xdot_s, float* cbc_s, void* ev_start, void* ev_stop, void* stream);
int bcbf_unicycle_control_step_sampled_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, double* x, const double* plan, const double* dot_plan,
    const double* Kp, double clf_gamma, const double* centers, const double* radii, const double* tw,
    const double* gammas, double L_mean, const double* w, const double* r, const double* sign,
    const double* relax_mask, const double* rho, double* grad, double* cst, double* fhat, double* ghat, double* Mk,
    double* Bk, double* cones, int* cstatus, double* y, int* status, int* iters, double dt, double L_true, int Bt,
    int N, int Kob, int max_iters, int shared_gp, const double* xq, double* obs_x, double* obs_uh, double* obs_y,
    int obs_ld, double* xq_next, int flags, int kernel_kind, const double* z, double* xdot_s, double* cbc_s,
    void* ev_start, void* ev_stop, void* stream);

/* ---- The pendulum's rel-degree-2 safety loop (SOCPController with cbfs = [RadialCBFRelDegree2], clf = None and the
 * greedy nominal controller: controllers.py:569-591, pendulum.py:643-746), batched: n = 2, m = 1.
 *
 * Explicit-Euler plant step of the true pendulum, x += (f(x) + g(x) u) dt with f = [omega, -(g/l) sin theta],
 * g = [0, 1/(m l)]', then theta <- ((theta + pi) mod 2 pi) - pi (floored modulo): PendulumDynamicsModel.step
 * (sampling_pendulum, pendulum.py:164-233).  x[Bt,2] in place, u[Bt,1]. */
int bcbf_pendulum_plant_step_f32(float* x, const float* u, float mass, float gravity, float length, float dt, int Bt,
                                 void* stream);
int bcbf_pendulum_plant_step_f64(double* x, const double* u, double mass, double gravity, double length, double dt,
                                 int Bt, void* stream);

/* Per-instance status of bcbf_pendulum_control_step (status[Bt]); the instance is driven with u = u_ref unless 0:
 *   0 (BCBF_SOCP_OPTIMAL), 1 (BCBF_SOCP_MAXITER), 2 (BCBF_SOCP_DIVERGED): bcbf_coneqp_f64's status of the program;
 *   3 (BCBF_SOCP_BADCONE): a cone row could not be factored, as SOCPController.control reports it (the kind-1 safety
 *     cone has an eigen fallback, so this step does not produce it today);
 *   BCBF_PENDULUM_BADHESSIAN: the kernel Hessian of L_f h has an eigenvalue <= -2e-3 (bcbf_cbc2_terms status 1), where
 *     the host path raises AssertionError (gp_algebra.py:386); takes precedence over the others. */
#define BCBF_PENDULUM_BADHESSIAN 5

/* One control step of the pendulum safety filter for Bt instances, enqueued on `stream` in one host call with no host
 * synchronisation and no allocation:
 *   1. bcbf_posterior_jets{,_matern52,_rbfm52}_f64 (kernel_kind 0/1/2) at x -- skipped when Lop == NULL;
 *   2. task kernel: Mk += [fhat | ghat], Mj[:, :, (1+i) C] += d fhat / d x_i of the deterministic mean model (a pendulum
 *      (mean_mass, mean_gravity, mean_length) when mean_model != 0; none = ZeroDynamicsModel), exactly as
 *      cbc2.reldeg2_quadratic_terms does; h = cos(delta_c) - cos(theta - theta_c), gh, Hh; u_ref = the caller's
 *      u_ref_in[Bt,1] or, when u_ref_in == NULL, GreedyController (x_goal[2], Q_goal[2,2] row-major and R: HOST
 *      values; lambda = 1/2; this dt) on the shifted posterior mean; P = 0, q = e_0;
 *   3. bcbf_cbc2_terms_f64 (kalpha[2] device, hessian_mode, kernel_kind) linearised at u_ref -> terms2[Bt,7], tstatus;
 *      terms[Bt,5] = its first five entries;
 *   4. bcbf_controller_cones_f64: objective cone (ctrl_reg, relax_weight) and the kind-1 safety cone scaled by
 *      safety_factor (cbc2_safety_factor(max_unsafe_prob)), extravars = 2 -> Gc[Bt,6,3], hc[Bt,6], cstatus[Bt];
 *   5. bcbf_coneqp_f64 (P, q, Gc, hc; cones Q^3 x Q^3; max_iters) -> y[Bt,3] = [y_1, rho, u], sstatus, iters;
 *   6. plant kernel: u[Bt] = y[:, 2] where status == 0, u_ref elsewhere; status (codes above); when min_h / fails are
 *      given (both or neither): min_h = min(min_h, h(x_t)) (a non-finite h counts as -inf), fails += (status != 0);
 *      then x advances as bcbf_pendulum_plant_step (true_mass, true_gravity, true_length, dt).
 * GP (Lop != NULL): Lop, Vw, X, UHB, M0 per instance, or instance 0 only when shared = 1 (regime S: one model, Bt
 * queries); ell[Bt,2], s2[Bt], Bm[Bt,2,2], A[Bt,2,2] are per instance in both regimes (the jets read instance 0 of
 * them when shared) because bcbf_cbc2_terms reads them per instance.
 * No GP (Lop == NULL, ControlCBFCLFGroundTruth: the mean model is the whole model): the task kernel writes Mk, Mj from
 * the mean model alone and zeroes Bk, G; pass s2 = 0 (and finite ell, Bm, A): every variance term of bcbf_cbc2_terms is
 * then exactly 0 and (mean_A, mean_b) = (-A(x), b(x)) of RadialCBFRelDegree2 (pendulum.py:713-746).
 * Workspaces (all required, device, caller-owned): Mk[Bt,2,2], Bk[Bt,2,2], G[Bt,6,6], Mj[Bt,2,6], h[Bt], gh[Bt,2],
 * Hh[Bt,2,2], u_ref[Bt], terms2[Bt,7], terms[Bt,5], tstatus[Bt], Gc, hc, cstatus[Bt], P[Bt,3,3], q[Bt,3], y[Bt,3],
 * sstatus[Bt], iters[Bt] (may be NULL), u[Bt], status[Bt].  ev_start / ev_stop (optional hipEvent_t) bracket the jets.
 * BCBF_EINVAL, before any HIP call, for: n != 2, m != 1, a null required buffer, an incomplete GP, shared not 0/1,
 * kernel_kind not 0..2, hessian_mode not 0/1, max_iters < 1, dt <= 0, R <= 0, ctrl_reg or relax_weight <= 0,
 * safety_factor < 0, a pendulum model with m l == 0.  fp64 only (the reference runs this demo in float64). */
int bcbf_pendulum_control_step_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, int N, int shared, int kernel_kind,
    int mean_model, double mean_mass, double mean_gravity, double mean_length,
    double theta_c, double delta_c, const double* kalpha, const double* x_goal, const double* Q_goal, double R,
    const double* u_ref_in, double safety_factor, double ctrl_reg, double relax_weight, int hessian_mode, int max_iters,
    double true_mass, double true_gravity, double true_length, double dt,
    double* x, double* Mk, double* Bk, double* G, double* Mj, double* h, double* gh, double* Hh, double* u_ref,
    double* terms2, double* terms, int* tstatus, double* Gc, double* hc, int* cstatus, double* P, double* q,
    double* y, int* sstatus, int* iters, double* u, int* status, double* min_h, int* fails,
    int Bt, int n, int m, void* ev_start, void* ev_stop, void* stream);

/* The same step for a loop that LEARNS its dynamics while it runs (ControlPendulumCBFLearned, pendulum.py:909-961, through
 * ControlCBFLearned / MeanAdjustedModel, controllers.py:320-378, 665-736; run_pendulum_control_online_learning,
 * pendulum.py:1041-1048).  Every argument of bcbf_pendulum_control_step_f64 with the same meaning, plus:
 *   prior (0/1): with Lop == NULL and prior = 1 the task kernel writes the GP prior of a regressor that holds no data
 *     (cbc2.posterior_for, control_affine_model.py:495-506): Mk = M0' (M0[Bt,1+m,n] required), Bk = s2 Bm, G = 0, Mj = 0,
 *     then adds the mean model as above; prior = 0 is the no-GP mode of the plain entry.  Ignored when Lop != NULL.
 *   explore[Bt,2] (device; NULL = no exploration), eps, ctrl_range[2] (HOST lo, hi; NULL = no clip): EpsilonGreedyController
 *     (controllers.py:269-285) around the greedy u_ref -- u_ref = lo + explore[b,1] (hi - lo) where explore[b,0] < eps, then
 *     u_ref = max(min(u_ref, hi), lo) (misc.py:287-288).  The program is linearised at, and falls back to, that u_ref.
 *   obs_x, obs_uh, obs_y (all three or none), obs_ld: the plant kernel writes this step's observation row at row b * obs_ld of
 *     each ([.,2] rows; obs_ld = the row stride, as bcbf_unicycle_control_step_observe): x_t, (1, u_t) with the applied
 *     u_t, and (x_{t+1} - x_t) / dt - (f + g u_t)(x_t) of the mean model (zero without one).  The states are the stored,
 *     theta-wrapped ones (the reference's buffer holds them): a step across theta = +-pi gives a target of size ~2 pi / dt.
 * BCBF_EINVAL, before any HIP call, for every refusal of the plain entry and: prior not 0/1, prior = 1 without M0 (no GP),
 * eps NaN or outside [0, 1], explore without ctrl_range, explore with u_ref_in, lo > hi (or NaN), a partial obs set,
 * obs_ld < 1 with obs rows, a mean model with m l == 0. */
int bcbf_pendulum_control_step_observe_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, int N, int shared, int kernel_kind,
    int mean_model, double mean_mass, double mean_gravity, double mean_length,
    double theta_c, double delta_c, const double* kalpha, const double* x_goal, const double* Q_goal, double R,
    const double* u_ref_in, double safety_factor, double ctrl_reg, double relax_weight, int hessian_mode, int max_iters,
    double true_mass, double true_gravity, double true_length, double dt,
    double* x, double* Mk, double* Bk, double* G, double* Mj, double* h, double* gh, double* Hh, double* u_ref,
    double* terms2, double* terms, int* tstatus, double* Gc, double* hc, int* cstatus, double* P, double* q,
    double* y, int* sstatus, int* iters, double* u, int* status, double* min_h, int* fails,
    int prior, const double* explore, double eps, const double* ctrl_range, double* obs_x, double* obs_uh, double* obs_y,
    int obs_ld, int Bt, int n, int m, void* ev_start, void* ev_stop, void* stream);

/* The same step on a plant DRAWN FROM THE MODEL'S OWN POSTERIOR, and the rel-degree-2 condition evaluated on that draw.  The
 * program of the step asks that CBC2(x, u) = grad(L_f h)' (f + g u) + k_alpha[0] h + k_alpha[1] L_f h, L_f h = grad h' f, hold
 * with probability >= 1 - max_unsafe_prob.  CBC2 is a QUADRATIC form in the joint posterior of f, g and the Jacobian of f, and
 * the (mean, var) bcbf_cbc2_terms hands the program are the reference's approximation of that form's moments (both kernel
 * arguments move in the derivative, the cross term is frozen at u_ref, the product variance is 2 tr(C)^2), so Cantelli's bound
 * is no theorem here; this entry is the instrument that measures what the loop holds.  The launches of
 * bcbf_pendulum_control_step_observe_f64 up to the plant kernel, then for EVERY instance
 *     s = (f, g, df/dtheta, df/domega) ~ matrix-variate normal, mean [Mk[:,0], Mk[:,1], Mj[:,(1+0)C], Mj[:,(1+1)C]] (after the
 *         task kernel has added the mean model), covariance A (x) Sigma4 over (state component) x (column);
 *     Sigma4 = rows / columns {0, 1, C, 2C} of Sigma6 = P6 - G,  P6 = blockdiag(s2 Bm, kxx s2/ell_0^2 Bm, kxx s2/ell_1^2 Bm),
 *         kxx = 1, 5/3, 8/3 for kernel_kind 0, 1, 2 (the values bcbf_cbc2_terms uses), the top-left block read from Bk;
 *         Sigma4 = 0 without a GP; in prior mode G = 0 and Sigma4 is the prior.  The marginal of a Gaussian is exact, so the
 *         g-derivative columns are not drawn;
 *     S = mean + L_A Z L_Sigma' with Z = z[b] (2 x 4) and both factors a positive-semidefinite Cholesky (a pivot <= 0 zeroes
 *         its column: a semidefinite A or Sigma4 is accepted and the draw stays in its range);
 *     xdot_s = f_s + g_s u,   cbc_s[b] = (grad h' f_s,  (Hh f_s + J_s' grad h)' xdot_s + k_alpha[0] h + k_alpha[1] grad h' f_s)
 *         with u the APPLIED control (y[2] where status == 0, u_ref elsewhere: an unsolved instance is driven by u_ref on the
 *         draw and its condition is evaluated there);
 *     x += xdot_s dt with the theta wrap of bcbf_pendulum_plant_step; true_mass, true_gravity, true_length are ignored.
 * fp64 arithmetic in registers on the stored values, each output rounded once.  min_h / fails and the observation rows behave
 * as in the observing entry; the rows then record the sampled plant.  Draws of different steps are independent: the marginal at
 * every visited (x_t, u_t) is exact, which is all the per-step chance constraint speaks about; a function-consistent draw along
 * a trajectory would have to condition on the earlier draws and is not what this entry does.
 * Every argument of bcbf_pendulum_control_step_observe_f64, plus
 *   z[Bt,2,4]     standard-normal draws, the caller's: the library draws no random numbers (as bcbf_subsample_rows);
 *   xdot_s[Bt,2], cbc_s[Bt,2]   outputs, each may be NULL; cbc_s is what bcbf_rollout_risk (Kob = 1) counts;
 *   relaxed[Bt], viol_relaxed[Bt] (int32, both or neither), rho_tol (HOST, >= 0): the safety cone is soft, and a step that bought
 *     slack was never promised the risk -- relaxed += (status == 0 && y[1] > rho_tol), viol_relaxed += (that && !(cbc2_s >= 0)).
 * BCBF_EINVAL, before any HIP call, for every refusal of the observing entry and: z == NULL, one counter without the other,
 * rho_tol < 0 or NaN. */
int bcbf_pendulum_control_step_sampled_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, int N, int shared, int kernel_kind,
    int mean_model, double mean_mass, double mean_gravity, double mean_length,
    double theta_c, double delta_c, const double* kalpha, const double* x_goal, const double* Q_goal, double R,
    const double* u_ref_in, double safety_factor, double ctrl_reg, double relax_weight, int hessian_mode, int max_iters,
    double true_mass, double true_gravity, double true_length, double dt,
    double* x, double* Mk, double* Bk, double* G, double* Mj, double* h, double* gh, double* Hh, double* u_ref,
    double* terms2, double* terms, int* tstatus, double* Gc, double* hc, int* cstatus, double* P, double* q,
    double* y, int* sstatus, int* iters, double* u, int* status, double* min_h, int* fails,
    int prior, const double* explore, double eps, const double* ctrl_range, double* obs_x, double* obs_uh, double* obs_y,
    int obs_ld, const double* z, double* xdot_s, double* cbc_s, int* relaxed, int* viol_relaxed, double rho_tol,
    int Bt, int n, int m, void* ev_start, void* ev_stop, void* stream);

/* ---- The reference's LQR nominal controller (LQRController.control, controllers.py:64-115: the default
 * unsafe_controller_class of ControlCBFLearned, controllers.py:681), batched: one lane per instance, the finite-horizon
 * recursion in registers, 64-thread workgroups.  It replaces the reference's two `bdlqr.lqr.LinearSystem(...).solve(x, 1)`
 * calls (controllers.py:87-97, 103-113) and the autograd Jacobians in front of them (controllers.py:77-79, 99-102).  `bdlqr`
 * is an external package; the semantic here is the same author's in-tree statement of its recursion,
 * affine_backpropagation (ilqr.py:43-76), cost u'Ru + 2 z'u + x'Qx + 2 s'x.  Parity with bdlqr's own iterates is not claimed.
 * Inputs in the layout bcbf_posterior_jets* writes (C = 1+m, CT = C (1+n)):  g = Mk[b,:,1:],  Jf[i][d] = Mj[b,i,(1+d)C],
 * Jg_j[i][d] = Mj[b,i,(1+d)C+1+j];  f = Mk[b,:,0] is not read.  Per instance, following the reference's code:
 *     B = g dt,  s = -Q x_goal,  z = 0,  Q_T = Q,  s_T = s
 *     pass(A): P = Q, o = s, then T times  G = R + B'PB,  K = G^-1 B'PA,  k = G^-1 (z + B'o),
 *              P <- Q + A'PA - A'PB K,  o <- s + A'o - K'(z + B'o)  (K, k from the old P, o);  result -K x - k of the last
 *              iteration, x the state itself (not x - x_goal)
 *     u0 = pass(I + dt Jf),   u = pass(I + dt (Jf + sum_j Jg_j u0_j));   ctrl_range is not applied (the reference's LQR does not
 *     clip; its epsilon-greedy wrapper does).
 * Horizon T = max(numSteps - t, 1), t the host value or, when t_dev != NULL, the device int t_dev[0] read by the kernel (held
 * to >= 0) -- a captured graph replays a shrinking horizon by incrementing that counter.  The clamp to 1 is this library's
 * definition: the reference is undefined at t >= numSteps.
 * x_goal[n], Q[n,n], R[m,m] (row-major): HOST values, passed to the kernel by value.  Device: Mk[Bt,n,C], Mj[Bt,n,CT], x[Bt,n]
 * -> u[Bt,m], u0[Bt,m] (the first pass's control; may be NULL), status[Bt]: 0, or 1 where some G had a pivot that is not > 0 in
 * the elimination without exchanges -- then u = u0 = 0 for that instance; other instances are unaffected.
 * Every (1 <= n <= 4, 1 <= m <= 3).  The f32 entry reads and writes fp32 and carries P, o, K, k in fp64, as the f64 entry does.
 * BCBF_EINVAL with a reason, before any HIP call, for: Bt < 0, n or m out of range, a null required pointer, dt <= 0 or NaN,
 * numSteps < 1, t < 0 with t_dev == NULL. */
int bcbf_lqr_nominal_f32(const float* Mk, const float* Mj, const float* x, const float* x_goal, const float* Q, const float* R,
                         float dt, int numSteps, int t, const int* t_dev, float* u, float* u0, int* status, int Bt, int n,
                         int m, void* stream);
int bcbf_lqr_nominal_f64(const double* Mk, const double* Mj, const double* x, const double* x_goal, const double* Q,
                         const double* R, double dt, int numSteps, int t, const int* t_dev, double* u, double* u0, int* status,
                         int Bt, int n, int m, void* stream);

/* The pendulum step with a choice of nominal controller.  Every argument of bcbf_pendulum_control_step_sampled_f64, plus
 *   nominal (0: GreedyController, as the three entries above; 1: LQRController, the reference's default for
 *     ControlPendulumCBFLearned), numSteps, t, t_dev (the horizon, as bcbf_lqr_nominal_f64), lstatus[Bt] (required with
 *     nominal = 1: bcbf_lqr_nominal_f64's status; an instance with lstatus 1 has the nominal control 0 before explore / clip).
 * z == NULL runs the observing entry's true plant, z != NULL the sampled entry's posterior-drawn plant.
 * nominal = 1: after the task kernel has added the mean model to Mk / Mj, u_ref = bcbf_lqr_nominal_f64's u on those factors
 * (x_goal, Q_goal, R, dt of this call; the same kernel), then the epsilon-greedy draw and the clip exactly as in the observing
 * entry -- LQR, explore, clip -- and everything downstream is unchanged.  nominal = 0: bit for bit the observing / sampled entry.
 * BCBF_EINVAL for every refusal of those entries and: nominal not 0 / 1; with nominal = 1: u_ref_in != NULL, lstatus == NULL,
 * numSteps < 1, t < 0 with t_dev == NULL. */
int bcbf_pendulum_control_step_nominal_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, int N, int shared, int kernel_kind,
    int mean_model, double mean_mass, double mean_gravity, double mean_length,
    double theta_c, double delta_c, const double* kalpha, const double* x_goal, const double* Q_goal, double R,
    const double* u_ref_in, double safety_factor, double ctrl_reg, double relax_weight, int hessian_mode, int max_iters,
    double true_mass, double true_gravity, double true_length, double dt,
    double* x, double* Mk, double* Bk, double* G, double* Mj, double* h, double* gh, double* Hh, double* u_ref,
    double* terms2, double* terms, int* tstatus, double* Gc, double* hc, int* cstatus, double* P, double* q,
    double* y, int* sstatus, int* iters, double* u, int* status, double* min_h, int* fails,
    int prior, const double* explore, double eps, const double* ctrl_range, double* obs_x, double* obs_uh, double* obs_y,
    int obs_ld, const double* z, double* xdot_s, double* cbc_s, int* relaxed, int* viol_relaxed, double rho_tol,
    int nominal, int numSteps, int t, const int* t_dev, int* lstatus,
    int Bt, int n, int m, void* ev_start, void* ev_stop, void* stream);

/* ---- The pendulum's CLF-CBF quadratic program on the KNOWN model (PendulumCBFCLFDirect, run_pendulum_control_cbf_clf:
 * pendulum.py:530-640, 770-906, 1019-1024).  Two rows, affine in the control, on the controller's model (m, g, l) at
 * x = (theta, omega), d = theta - theta_c:
 *   row 0, EnergyCLF (relaxed by the slack rho):  V = l omega^2 / 2 + g (1 - cos theta),  A = omega / m,  b = -clf_c V
 *     -- the values the reference RETURNS (grad V . g and -grad V . f - c V); its hand-written `direct = l omega` equals
 *     them only when m l = 1, and its own assert trips for another model;
 *   row 1 (hard), cbf_kind 0, RadialCBFRelDegree2:  h = cos delta_c - cos d,  A = -sin d / (m l),
 *     b = omega^2 cos d - (g/l) sin d sin theta + k_alpha[0] h + k_alpha[1] omega sin d;
 *   row 1 (hard), cbf_kind 1, RadialCBF:  h = (cos delta_c - cos d)(omega^2 + 1),  A = -2 omega (cos delta_c - cos d) / (m l),
 *     b = grad h . f + cbf_gamma h,  grad h = [sin d (omega^2 + 1), 2 omega (cos delta_c - cos d)];
 * and control_QP_cbf_clf with constraint_margin_weights = [slack_weight]:
 *     minimise 1/2 (u^2 + slack_weight rho^2)   subject to   A0 u - rho <= b0,   A1 u <= b1.
 * The objective is strictly convex: the unique optimum is computed in closed form over the four active sets (the
 * reference iterates with cvxopt; parity with its iterates is not claimed).  The program is infeasible exactly when
 * A1 == 0 and b1 < 0: status 1, nothing divided, u and rho not written (a non-finite row or result is reported the same way).
 * ctrl_params: the controller's (m, g, l), device, one shared row (ctrl_stride = 0) or one row per instance
 * (ctrl_stride = 3).  k_alpha[2]: HOST values.
 *
 * One control evaluation for Bt states, no step: x[Bt,2] -> A[Bt,2], b[Bt,2], values[Bt,2] = (V, h), u[Bt], rho[Bt],
 * status[Bt] (int); every output may be NULL.
 * BCBF_EINVAL with a reason in bcbf_last_error, before any HIP call, for: Bt <= 0, null x / ctrl_params / k_alpha,
 * slack_weight <= 0, ctrl_stride not 0 / 3, cbf_kind not 0 / 1. */
int bcbf_pendulum_clf_cbf_control_f32(const float* x, const float* ctrl_params, int ctrl_stride, float clf_c,
                                      const float* k_alpha, float theta_c, float delta_c, float cbf_gamma, int cbf_kind,
                                      float slack_weight, float* A, float* b, float* values, float* u, float* rho,
                                      int* status, int Bt, void* stream);
int bcbf_pendulum_clf_cbf_control_f64(const double* x, const double* ctrl_params, int ctrl_stride, double clf_c,
                                      const double* k_alpha, double theta_c, double delta_c, double cbf_gamma, int cbf_kind,
                                      double slack_weight, double* A, double* b, double* values, double* u, double* rho,
                                      int* status, int Bt, void* stream);

/* The closed loop: numSteps steps for Bt instances in ONE launch, one lane per instance (64-thread workgroups); state,
 * parameters and statistics stay in registers for the whole launch.  Per step, in sampling_pendulum's order
 * (pendulum.py:199-226): rows at x_t on the controller's model; the program; min_h = min(min_h, h(x_t)) (a non-finite h
 * counts as -inf); damage += (0 < theta_t < pi/4); x_{t+1} = x_t + (f + g u) dt on the PLANT's parameters (true_params,
 * true_stride: as ctrl_params; a plant that differs from the controller's model is the mismatch study); theta wrapped as
 * bcbf_pendulum_plant_step does.  An instance whose program cannot be solved at (0-based) step t records
 * status = t_offset + t + 1 and freezes: its state, min_h and damage keep the values they had before that step (the
 * reference raises there).  An instance that arrives with status != 0 stays frozen.
 * In/out, accumulated in place: x[Bt,2], min_h[Bt], damage[Bt] (int), status[Bt] (int) -- two calls of k steps, the
 * second with t_offset = k, equal one call of 2k steps bit for bit.
 * Recording (traj and/or u_rec given, record_every > 0): the steps whose global index t_offset + t is a multiple of
 * record_every write (x_t, u_t) -- before the step; u = 0 for a frozen instance -- to traj[r,Bt,2] and u_rec[r,Bt], r
 * counting from 0 within THIS launch: the caller offsets the pointers between launches and sizes the buffers for
 * the number of such steps.
 * BCBF_EINVAL with a reason, before any HIP call, for: Bt <= 0, numSteps < 0, t_offset < 0, dt <= 0, slack_weight <= 0, a
 * stride not 0 / 3, cbf_kind not 0 / 1, a null required buffer, recording pointers with record_every <= 0. */
int bcbf_pendulum_clf_cbf_rollout_f32(float* x, const float* ctrl_params, int ctrl_stride, const float* true_params,
                                      int true_stride, float clf_c, const float* k_alpha, float theta_c, float delta_c,
                                      float cbf_gamma, int cbf_kind, float slack_weight, float dt, float* min_h, int* damage,
                                      int* status, float* traj, float* u_rec, int record_every, int t_offset, int numSteps,
                                      int Bt, void* stream);
int bcbf_pendulum_clf_cbf_rollout_f64(double* x, const double* ctrl_params, int ctrl_stride, const double* true_params,
                                      int true_stride, double clf_c, const double* k_alpha, double theta_c, double delta_c,
                                      double cbf_gamma, int cbf_kind, double slack_weight, double dt, double* min_h,
                                      int* damage, int* status, double* traj, double* u_rec, int record_every, int t_offset,
                                      int numSteps, int Bt, void* stream);

/* ---- The unicycle's CLF-CBF quadratic program on the MEAN model (ControllerCLF, unicycle_move_to_pose.py:699-791; the
 * controller of move_to_pose_clf_polar / _clf_cartesian / _sample_clf_cartesian / track_trajectory_clf_cartesian, :1579-1656,
 * and of the speed test's trajectories, :2072-2083).  y = (u0, u1, relax):
 *     minimise |u|^2 + relax_weight relax   subject to   lo <= u <= hi,   a_0.u + b_0 - relax <= 0,   a_k.u + b_k >= 0 (k >= 1).
 * relax is free with a positive linear cost, so its row is tight and u* is the Euclidean projection of p = -(relax_weight/2) a_0
 * onto the polygon {box} n {hard rows}; relax* = a_0.u* + b_0 (it may be negative).  The optimum is unique; the program is
 * infeasible exactly when the polygon is empty.  The projection is found by enumerating active sets of size <= 2 over the
 * M = 4 + Kob half-planes in the order lo0, lo1, hi0, hi1, hard rows (Kob <= 3, at most 29 candidates): p; the foot of p on each
 * line in row order (zero normal: no candidate); each pairwise intersection in lexicographic order (determinant exactly 0: no
 * candidate).  A candidate is admissible when every row i NOT in its active set has a_i.u + b_i >= -tol_i,
 * tol_i = 64 eps (|a_i0 u0| + |a_i1 u1| + |b_i|); the answer is the admissible candidate nearest to p, ties to the first in
 * that order.  No admissible candidate, or a non-finite row or result: status 1 and u, relax, active are NOT written.  The
 * reference iterates with GUROBI through cvxpy; parity with its iterates is not claimed.
 *
 * The program alone: a[Bt,K,2], b[Bt,K] (row 0 relaxed, rows 1.. hard, 1 <= K <= 4); lo[2], hi[2], relax_weight: HOST values.
 * -> u[Bt,2], relax[Bt], active[Bt] (int bitmask over the M rows: the winning candidate's active set), status[Bt] (int);
 * every output may be NULL.
 * BCBF_EINVAL with a reason in bcbf_last_error, before any HIP call, for: Bt <= 0, K outside 1..4, null a / b / lo / hi, a
 * non-finite bound, relax_weight not a finite number > 0. */
int bcbf_clf_cbf_qp2_f32(const float* a, const float* b, const float* lo, const float* hi, float relax_weight, float* u,
                         float* relax, int* active, int* status, int Bt, int K, void* stream);
int bcbf_clf_cbf_qp2_f64(const double* a, const double* b, const double* lo, const double* hi, double relax_weight, double* u,
                         double* relax, int* active, int* status, int Bt, int K, void* stream);

/* One control evaluation (ControllerCLF.control, :757-788; _clc :731-742, _cbcs :744-752) for Bt states x[Bt,3] with
 * plan[Bt,3], dot_plan[Bt,3].  Kp[4], lo[2], hi[2], tw[2], gammas[Kob]: HOST values.
 *   clf_kind 0: CLFCartesian (:522-615, Kp[0..2]) and ObstacleCBF (:618-696) on AckermannDrive(L_ctrl) / CartesianDynamics
 *     (L_ctrl = 1), f = 0: a_k = grad_k . g(x; L_ctrl), b_0 = grad_goal V . dot_plan + clf_gamma V, b_k = gammas[k-1] h_k -- the
 *     rows of bcbf_unicycle_constraints;
 *   clf_kind 1: CLFPolar (:442-497) on PolarDynamics (:143-167) through cartesian2polar (:112-139), (rho, alpha, beta) of x
 *     relative to plan:  V = Kp0 rho^2 / 2 + Kp1 (1 - cos alpha) + Kp2 (1 - cos beta) + Kp3 (1 - cos(beta - alpha)),
 *     a_0 = grad V . [[-cos alpha, 0], [-sin alpha / rho, 1], [-sin alpha / rho, 0]],  b_0 = clf_gamma V (grad_clf_wrt_goal = 0);
 *     rho <= 1e-6 is refused as the reference's assert does (status 1).  Kob must be 0: the reference would hand polar
 *     coordinates to ObstacleCBF.
 * L_ctrl: device, one shared value (L_stride 0) or one per instance (1).  centers[.,Kob,2], radii[.,Kob]: device, shared
 * (obs_stride 0) or per instance (1); unused with Kob = 0.
 * -> a[Bt,1+Kob,2], b[Bt,1+Kob], values[Bt,1+Kob] = (V, h_k), u[Bt,2], relax[Bt], active[Bt], status[Bt]; each may be NULL;
 * u, relax and active are not written where status is 1.
 * BCBF_EINVAL with a reason, before any HIP call, for every refusal of the program's entry and: null x / plan / dot_plan / Kp /
 * L_ctrl, Kob outside 0..3, clf_kind not 0 / 1, clf_kind 1 with Kob > 0, a stride not 0 / 1, a non-finite clf_gamma,
 * Kob > 0 with null centers / radii / tw / gammas. */
int bcbf_unicycle_clf_cbf_control_f32(const float* x, const float* plan, const float* dot_plan, const float* Kp, int clf_kind,
                                      float clf_gamma, float relax_weight, const float* lo, const float* hi,
                                      const float* L_ctrl, int L_stride, const float* centers, const float* radii,
                                      int obs_stride, const float* tw, const float* gammas, float* a, float* b, float* values,
                                      float* u, float* relax, int* active, int* status, int Bt, int Kob, void* stream);
int bcbf_unicycle_clf_cbf_control_f64(const double* x, const double* plan, const double* dot_plan, const double* Kp,
                                      int clf_kind, double clf_gamma, double relax_weight, const double* lo, const double* hi,
                                      const double* L_ctrl, int L_stride, const double* centers, const double* radii,
                                      int obs_stride, const double* tw, const double* gammas, double* a, double* b,
                                      double* values, double* u, double* relax, int* active, int* status, int Bt, int Kob,
                                      void* stream);

/* The closed loop (sample_generator_trajectory over ControllerCLF.control, sampling.py:40-80; move_to_pose's while loop,
 * :1456-1488): numSteps steps for Bt instances in ONE launch, one lane per instance (64-thread workgroups); state, parameters,
 * the planner's control points and the statistics stay in registers.  Per (0-based) step t, global step T = t_offset + t:
 *   0. stop_rho > 0: where |goal - x_t| (positions) < stop_rho (isconverged, :495-497, 613-615) the instance records
 *      converged_at = T and stops: state frozen, status stays 0.  converged_at[Bt] (int, in/out): -1 = still running.
 *   1. the plan.  planner_kind 0 (NoPlanner): plan = goal[b], dot_plan = 0.  planner_kind 1 (PiecewiseLinearPlanner,
 *      planner.py:19-64, with the SAME dt): control points from x0_plan[Bt,3] and goal[Bt,3], evaluated at
 *      min(T + lookahead, numStepsPlan); the integers t2 = min(int(numStepsPlan frac), numStepsPlan - 1),
 *      lookahead = max(int(0.1 numStepsPlan), 1) and numStepsPlan are the HOST's (no float-to-int rule on the device);
 *   2. the rows at x_t on the controller's model (L_ctrl), as the control entry forms them;
 *   3. the program;
 *   4. min_h = min(min_h, min_k h_k(x_t)) (non-finite counts as -inf; untouched, and may be NULL, with Kob = 0);
 *      cost += |u_t|^2;
 *   5. x_{t+1} = x_t + g(x_t; L_true) u_t dt on the PLANT's wheelbase (L_true: as L_ctrl; a plant that differs from the
 *      controller's model is the mismatch study).  No angle wrap: the reference applies none.
 * An instance whose program cannot be solved at step t records status = T + 1 and freezes: state and statistics keep the
 * values they had before that step.  An instance that arrives with status != 0 or converged_at >= 0 stays as it is.
 * In/out, accumulated in place: x[Bt,3], min_h[Bt], cost[Bt], status[Bt] (int), converged_at[Bt] (int; may be NULL when
 * stop_rho = 0) -- two calls of k and n - k steps, the second with t_offset = k, equal one call of n steps bit for bit.
 * Recording (traj and/or u_rec given, record_every > 0): the steps whose T is a multiple of record_every write (x_t, u_t) --
 * before the step; u = 0 for a frozen or stopped instance -- to traj[r,Bt,3] and u_rec[r,Bt,2], r counting from 0 within
 * THIS launch.
 * BCBF_EINVAL with a reason, before any HIP call, for every refusal of the control entry's task arguments and: Bt <= 0,
 * numSteps < 0, t_offset < 0 or t_offset + numSteps overflowing, dt not a finite number > 0, stop_rho negative or not finite,
 * stop_rho > 0 without converged_at, null x / goal / cost / status / L_true, null min_h with Kob > 0, planner_kind not 0 / 1,
 * planner_kind 1 without x0_plan or with numStepsPlan < 3, t2 outside [0, numStepsPlan), lookahead outside [1, numStepsPlan],
 * recording pointers with record_every <= 0. */
int bcbf_unicycle_clf_cbf_rollout_f32(float* x, const float* goal, const float* x0_plan, int planner_kind, int t2,
                                      int lookahead, int numStepsPlan, const float* Kp, int clf_kind, float clf_gamma,
                                      float relax_weight, const float* lo, const float* hi, const float* L_ctrl, int Lc_stride,
                                      const float* L_true, int Lt_stride, const float* centers, const float* radii,
                                      int obs_stride, const float* tw, const float* gammas, float dt, float stop_rho,
                                      float* min_h, float* cost, int* status, int* converged_at, float* traj, float* u_rec,
                                      int record_every, int t_offset, int numSteps, int Bt, int Kob, void* stream);
int bcbf_unicycle_clf_cbf_rollout_f64(double* x, const double* goal, const double* x0_plan, int planner_kind, int t2,
                                      int lookahead, int numStepsPlan, const double* Kp, int clf_kind, double clf_gamma,
                                      double relax_weight, const double* lo, const double* hi, const double* L_ctrl,
                                      int Lc_stride, const double* L_true, int Lt_stride, const double* centers,
                                      const double* radii, int obs_stride, const double* tw, const double* gammas, double dt,
                                      double stop_rho, double* min_h, double* cost, int* status, int* converged_at,
                                      double* traj, double* u_rec, int record_every, int t_offset, int numSteps, int Bt,
                                      int Kob, void* stream);
/* The same control step on a model learned with the opt-in Matern-5/2 data kernel (bcbf_refit_matern52 /
 * bcbf_gp_append_matern52 states): identical arguments; the posterior launch evaluates the Matern kernel (one GP per
 * instance: the streaming kernel; shared_gp: the matrix-core query bcbf_posterior_shared_matern52), the fused task rows /
 * terms / SOCP / plant-step launch behind it is the same.  No reference counterpart (the reference has no Matern kernel). */
int bcbf_unicycle_control_step_matern52_f32(
    const float* Lop, const float* Vw, const float* X, const float* UHB, const float* ell, const float* s2,
    const float* Bm, const float* M0, const float* A, float* x, const float* plan, const float* dot_plan,
    const float* Kp, float clf_gamma, const float* centers, const float* radii, const float* tw, const float* gammas,
    float L_mean, const float* w, const float* r, const float* sign, const float* relax_mask, const float* rho,
    float* grad, float* cst, float* fhat, float* ghat, float* Mk, float* Bk, float* cones, int* cstatus,
    float* y, int* status, int* iters, float dt, float L_true, int Bt, int N, int Kob, int max_iters, int shared_gp,
    void* ev_start, void* ev_stop, void* stream);
int bcbf_unicycle_control_step_matern52_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, double* x, const double* plan, const double* dot_plan,
    const double* Kp, double clf_gamma, const double* centers, const double* radii, const double* tw,
    const double* gammas, double L_mean, const double* w, const double* r, const double* sign,
    const double* relax_mask, const double* rho, double* grad, double* cst, double* fhat, double* ghat, double* Mk,
    double* Bk, double* cones, int* cstatus, double* y, int* status, int* iters, double dt, double L_true, int Bt,
    int N, int Kob, int max_iters, int shared_gp, void* ev_start, void* ev_stop, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The PRODUCT data kernel RBF x Matern-5/2 (BASELINE.json north_star: "RBF x Matern kernel-block build"):
 *   k(x, x') = s2 exp(-d2 / 2) (1 + a + a^2 / 3) exp(-a),  d2 = sum_d ((x_d - x'_d) / ell_d)^2,  a = sqrt(5 d2)
 * -- one set of ARD length scales for both factors.  Opt-in, like the Matern-5/2 kernel above, and like it without a
 * reference counterpart (the reference's only data kernel is the RBF): parity unpinned; the formula, its
 * derivative jets and its likelihood gradient are held to the CPU oracle and to finite differences.  Every `*_matern52` entry
 * point has a `*_rbfm52` twin with the same arguments; `kernel_kind` = 2 in bcbf_cbc2_terms / bcbf_predict_assemble. */
int bcbf_refit_rbfm52_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                            const float* jitter, float* Lop, float* UHB, float* Ldense, int* info, int Bt, int N, int n, int m,
                            void* stream);
int bcbf_refit_rbfm52_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                            const double* jitter, double* Lop, double* UHB, double* Ldense, int* info, int Bt, int N, int n, int m,
                            void* stream);
int bcbf_posterior_jets_rbfm52_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                     const float* ell, const float* s2, const float* Bm, const float* M0,
                                     const float* xq, float* Mk, float* Bk, float* G, float* Mj, float* Wj, int shared,
                                     int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_jets_rbfm52_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                     const double* ell, const double* s2, const double* Bm, const double* M0,
                                     const double* xq, double* Mk, double* Bk, double* G, double* Mj, double* Wj, int shared,
                                     int Bt, int N, int n, int m, void* stream);
int bcbf_mll_grad_rbfm52_f32(const float* Lop, const float* alpha, const float* Kinv, const float* X, const float* UH,
                               const float* R, const float* Ainv, const float* Bm, const float* ell, const float* s2, float* g_ell,
                               float* g_s2, float* g_B, float* logdetK, float* RtA, float* UHtA, int Bt, int N, int n, int m,
                               void* work, void* stream);
int bcbf_mll_grad_rbfm52_f64(const double* Lop, const double* alpha, const double* Kinv, const double* X, const double* UH,
                               const double* R, const double* Ainv, const double* Bm, const double* ell, const double* s2,
                               double* g_ell, double* g_s2, double* g_B, double* logdetK, double* RtA, double* UHtA, int Bt, int N,
                               int n, int m, void* work, void* stream);
int bcbf_gp_append_rbfm52_f32(const float* Lop_in, const float* Vw_in, const float* X_in, const float* UHB_in,
                                const float* ell, const float* s2, const float* Bm, const float* M0, const float* x_new,
                                const float* uh_new, const float* xdot_new, const float* jitter_new, float* Lop_out,
                                float* Vw_out, float* X_out, float* UHB_out, int* info, int Bt, int N, int n, int m, void* stream);
int bcbf_gp_append_rbfm52_f64(const double* Lop_in, const double* Vw_in, const double* X_in, const double* UHB_in,
                                const double* ell, const double* s2, const double* Bm, const double* M0, const double* x_new,
                                const double* uh_new, const double* xdot_new, const double* jitter_new, double* Lop_out,
                                double* Vw_out, double* X_out, double* UHB_out, int* info, int Bt, int N, int n, int m,
                                void* stream);
int bcbf_kb_build_rbfm52_f32(const float* X, const float* UH, const float* Bm, const float* ell, const float* s2,
                               const float* jitter, float* Kb, int Bt, int N, int n, int m, void* stream);
int bcbf_kb_build_rbfm52_f64(const double* X, const double* UH, const double* Bm, const double* ell, const double* s2,
                               const double* jitter, double* Kb, int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_query_rbfm52_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                      const float* ell, const float* s2, const float* Bm, const float* M0, const float* xq,
                                      const float* jitter2, float* Mk, float* Bk, float* W, int shared, int Bt, int N,
                                      int n, int m, void* stream);
int bcbf_posterior_query_rbfm52_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                      const double* ell, const double* s2, const double* Bm, const double* M0,
                                      const double* xq, const double* jitter2, double* Mk, double* Bk, double* W,
                                      int shared, int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_shared_rbfm52_f32(const float* Lop, const float* Vw, const float* X, const float* UHB,
                                       const float* ell, const float* s2, const float* Bm, const float* M0,
                                       const float* xq, const float* jitter2, float* Mk, float* Bk, float* W,
                                       int Bt, int N, int n, int m, void* stream);
int bcbf_posterior_shared_rbfm52_f64(const double* Lop, const double* Vw, const double* X, const double* UHB,
                                       const double* ell, const double* s2, const double* Bm, const double* M0,
                                       const double* xq, const double* jitter2, double* Mk, double* Bk, double* W,
                                       int Bt, int N, int n, int m, void* stream);
int bcbf_unicycle_control_step_rbfm52_f32(
    const float* Lop, const float* Vw, const float* X, const float* UHB, const float* ell, const float* s2,
    const float* Bm, const float* M0, const float* A, float* x, const float* plan, const float* dot_plan,
    const float* Kp, float clf_gamma, const float* centers, const float* radii, const float* tw, const float* gammas,
    float L_mean, const float* w, const float* r, const float* sign, const float* relax_mask, const float* rho,
    float* grad, float* cst, float* fhat, float* ghat, float* Mk, float* Bk, float* cones, int* cstatus,
    float* y, int* status, int* iters, float dt, float L_true, int Bt, int N, int Kob, int max_iters, int shared_gp,
    void* ev_start, void* ev_stop, void* stream);
int bcbf_unicycle_control_step_rbfm52_f64(
    const double* Lop, const double* Vw, const double* X, const double* UHB, const double* ell, const double* s2,
    const double* Bm, const double* M0, const double* A, double* x, const double* plan, const double* dot_plan,
    const double* Kp, double clf_gamma, const double* centers, const double* radii, const double* tw,
    const double* gammas, double L_mean, const double* w, const double* r, const double* sign,
    const double* relax_mask, const double* rho, double* grad, double* cst, double* fhat, double* ghat, double* Mk,
    double* Bk, double* cones, int* cstatus, double* y, int* status, int* iters, double dt, double L_true, int Bt,
    int N, int Kob, int max_iters, int shared_gp, void* ev_start, void* ev_stop, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Obstacle fields (obstacle_field.hip): the chance-constrained unicycle step of bcbf_unicycle_control_step among up to
 * BCBF_MAX_FIELD discs, solved on a WORKING SET of S <= 3 of them in the fused kernel and certified against all of them.
 * Reference: ObstacleCBF, unicycle_move_to_pose.py:618-696; one un-relaxed cone per obstacle (`_cbcs`, :901-920); the program
 * (:926-953).  The program is convex and its objective strictly convex in (u, relax): a working-set optimum at which no other
 * disc's cone is violated is feasible for the full program, hence its unique optimum.
 * The field: centers_f[Bf,Kf,2], radii_f[Bf,Kf]; field_stride 0 = one field for every instance (Bf = 1), 1 = one per instance
 * (Bf = Bt).  One gamma for the whole field.  1 <= S <= 3, S <= Kf <= BCBF_MAX_FIELD.  Both precisions carry the arithmetic
 * in fp64 from the inputs as stored, so no decision depends on the entry's precision.  One wave per instance, lanes stride over
 * the discs; no LDS, no scratch.
 *
 * bcbf_obstacle_field_select: h_k(x) = tw0 (|p - c_k|^2 - r_k^2) + tw1 heading_k (ObstacleCBF.cbf, :624-630) of every disc;
 *   idx[Bt,S] = the S smallest (ties to the lower index, NaN below everything), centers_sel[Bt,S,2] / radii_sel[Bt,S] = their
 *   discs -- the `centers` / `radii` the control step reads; min_h[Bt] = min(min_h, min_k h_k) in place (a non-finite h counts
 *   as -inf); cert[Bt] = rounds[Bt] = 0.
 * bcbf_obstacle_field_audit: x[Bt,3] the state the program was formed at (solve with dt = 0), y[Bt,3] = (u, relax) and
 *   status[Bt] of the solve, Mk[Bt,3,3], Bk[Bt,3,3], A[Bt,3,3], fhat[Bt,3], ghat[Bt,3,2] as the control step exposes them,
 *   rho[Bt].  Per instance:
 *     cert != 0 on entry: nothing is touched (the call is idempotent);
 *     status != BCBF_SOCP_OPTIMAL: cert = BCBF_FIELD_UNSOLVED (worst_margin = NaN, worst_idx = -1, nviol = 0);
 *     else for every disc, with ubar = (1, u):  E_k = grad h_k . (fhat + ghat u + M_k ubar) + gamma h_k,
 *       s_k = sqrt(max(ubar' B_k ubar  grad h_k' A grad h_k, 0)),  margin_k = E_k - rho s_k  (NaN counts as -inf) -- the cone of
 *       cbc2_quadratic_terms -> convert_cbc_terms_to_socp_terms (:837-878); an UNSELECTED disc is a violator when
 *       margin_k < -tol_f max(1, |E_k|, rho s_k).  worst_margin / worst_idx = the smallest margin among the unselected discs
 *       (ties to the lower index; +inf / -1 when Kf = S), nviol = the number of violators.
 *       No violator: cert = BCBF_FIELD_CERTIFIED.  Else the slot of largest margin (ties to the lower slot): when that margin is
 *       <= tol_a max(1, |E|, rho s) every slot is active, cert = BCBF_FIELD_FULL; otherwise that slot's idx / centers_sel /
 *       radii_sel are overwritten with the violator of smallest margin (ties to the lower index), rounds += 1, cert stays 0.
 *     Dropping a slack cone keeps the optimum and adding a violated one strictly raises the optimal value: no cycling.
 *   Tolerances: fp64 entries  tol_f = 1e-7 (the solvers' acceptance), tol_a = 1e-6;  fp32 entries, whose solver rows are
 *   formed in fp32:  tol_f = BCBF_FIELD_TOL_F_F32, tol_a = BCBF_FIELD_TOL_A_F32 (measured).
 * bcbf_obstacle_field_commit (one lane per instance): status_eff = 0 where cert == BCBF_FIELD_CERTIFIED, else status when
 *   that is not 0, else BCBF_FIELD_UNCERTIFIED; where status_eff == 0 and dt > 0, x += g(x; L_true) u dt (:277-282).  Every
 *   other instance keeps its state (the reference raises ValueError there, :954-964).
 * BCBF_EINVAL with a reason in bcbf_last_error, before any HIP call, for: Bt <= 0, S outside 1..3, Kf outside S..BCBF_MAX_FIELD,
 * field_stride not 0 / 1, a tolerance negative or not finite, any null pointer; commit: dt negative or not finite, L_true zero
 * or not finite with dt > 0. */
#define BCBF_MAX_FIELD 256
#define BCBF_FIELD_CERTIFIED 1
#define BCBF_FIELD_FULL 2
#define BCBF_FIELD_UNSOLVED 3
#define BCBF_FIELD_UNCERTIFIED 6   /* status_eff: solved on the working set, not certified against the field */
#define BCBF_FIELD_TOL_F_F32 5e-7   /* 10 x 4.81e-8: the audit's fp32-stored margin against the float64 margin of the same inputs */
#define BCBF_FIELD_TOL_A_F32 7e-6   /* 10 x 6.93e-7: the working set's active cones, rows formed in fp32, as the fp64 audit sees them */
int bcbf_obstacle_field_select_f32(const float* x, const float* centers_f, const float* radii_f, int field_stride,
                                   const float* tw, int* idx, float* centers_sel, float* radii_sel, float* min_h, int* cert,
                                   int* rounds, int Bt, int Kf, int S, void* stream);
int bcbf_obstacle_field_select_f64(const double* x, const double* centers_f, const double* radii_f, int field_stride,
                                   const double* tw, int* idx, double* centers_sel, double* radii_sel, double* min_h,
                                   int* cert, int* rounds, int Bt, int Kf, int S, void* stream);
int bcbf_obstacle_field_audit_f32(const float* x, const float* y, const int* status, const float* Mk, const float* Bk,
                                  const float* A, const float* fhat, const float* ghat, const float* rho,
                                  const float* centers_f, const float* radii_f, int field_stride, const float* tw, float gamma,
                                  double tol_f, double tol_a, int* idx, float* centers_sel, float* radii_sel, int* cert,
                                  int* rounds, float* worst_margin, int* worst_idx, int* nviol, int Bt, int Kf, int S,
                                  void* stream);
int bcbf_obstacle_field_audit_f64(const double* x, const double* y, const int* status, const double* Mk, const double* Bk,
                                  const double* A, const double* fhat, const double* ghat, const double* rho,
                                  const double* centers_f, const double* radii_f, int field_stride, const double* tw,
                                  double gamma, double tol_f, double tol_a, int* idx, double* centers_sel, double* radii_sel,
                                  int* cert, int* rounds, double* worst_margin, int* worst_idx, int* nviol, int Bt, int Kf,
                                  int S, void* stream);
int bcbf_obstacle_field_commit_f32(float* x, const float* y, const int* status, const int* cert, int* status_eff, float dt,
                                   float L_true, int Bt, void* stream);
int bcbf_obstacle_field_commit_f64(double* x, const double* y, const int* status, const int* cert, int* status_eff, double dt,
                                   double L_true, int Bt, void* stream);

/* bcbf_obstacle_field_commit_sampled (field_plant.hip; one wave per instance, as the audit): the commit on a plant DRAWN FROM
 * THE MODEL'S OWN POSTERIOR, in place of bcbf_obstacle_field_commit.  Reference: ObstacleCBF, unicycle_move_to_pose.py:618-696;
 * one un-relaxed cone per obstacle (`_cbcs`, :901-920); the program (:926-953); the plant fu_func_gp(u), :262-275, drawn as
 * GaussianProcessBase.sample draws, gp_algebra.py:33-34; the condition on a state derivative, cbc1.py:10-14.
 * status_eff[Bt] is written as the plain commit writes it.  An instance with status_eff = 0, in fp64 from the inputs as stored:
 *     ubar = (1, u),  u = y as stored;   s = max(ubar' B_k ubar, 0);   A = L_A L_A' (a pivot <= 0 zeroes its column)
 *     xdot_s = fhat + ghat u + M_k ubar + sqrt(s) L_A z          z[Bt,3]: the caller's standard normals (the library draws none)
 *     for EVERY disc k of the field, at the state before the step:
 *         cbc_k    = grad h_k . xdot_s + gamma h_k               (anything non-finite counts as -inf)
 *         margin_k = the audit's margin  E_k - rho sqrt(max(s grad h_k' A grad h_k, 0))   (NaN counts as -inf)
 *     x += xdot_s dt                                             (dt = 0: the state stays, everything else is done)
 *   xdot_s[Bt,3];  cbc_min[Bt], cbc_argmin[Bt] (ties to the lower index);  tight_idx[Bt] = the disc of smallest margin_k (ties to
 *   the lower index: the audit's ordering), cbc_tight[Bt] = that disc's cbc_k;  nneg[Bt] = the number of discs with cbc_k < 0.
 *   Accumulators, in place (int32; min_cbc in T):  solved += 1, viol_tight += (cbc_tight < 0), viol_any += (nneg > 0),
 *   viol_unselected += (a disc outside idx[b,:S] has cbc_k < 0), viol_discs += nneg, min_cbc = min(min_cbc, cbc_min).
 *   The counts are taken on the fp64 values; every output is rounded to T once.
 * Every other instance keeps its state bit for bit and its accumulators; it gets xdot_s = 0, cbc_min = cbc_tight = 0,
 * cbc_argmin = tight_idx = -1, nneg = 0.  There is no L_true: the true drive plays no part.
 * BCBF_EINVAL with a reason, before any HIP call, for: Bt <= 0, S outside 1..3, Kf outside S..BCBF_MAX_FIELD, field_stride not
 * 0 / 1, gamma not finite, dt negative or not finite, any null pointer. */
int bcbf_obstacle_field_commit_sampled_f32(
    float* x, const float* y, const int* status, const int* cert, const float* Mk, const float* Bk, const float* A,
    const float* fhat, const float* ghat, const float* rho, const float* centers_f, const float* radii_f, int field_stride,
    const float* tw, float gamma, const int* idx, const float* z, int* status_eff, float* xdot_s, float* cbc_min,
    int* cbc_argmin, int* tight_idx, float* cbc_tight, int* nneg, int* solved, int* viol_tight, int* viol_any,
    int* viol_unselected, int* viol_discs, float* min_cbc, float dt, int Bt, int Kf, int S, void* stream);
int bcbf_obstacle_field_commit_sampled_f64(
    double* x, const double* y, const int* status, const int* cert, const double* Mk, const double* Bk, const double* A,
    const double* fhat, const double* ghat, const double* rho, const double* centers_f, const double* radii_f, int field_stride,
    const double* tw, double gamma, const int* idx, const double* z, int* status_eff, double* xdot_s, double* cbc_min,
    int* cbc_argmin, int* tight_idx, double* cbc_tight, int* nneg, int* solved, int* viol_tight, int* viol_any,
    int* viol_unselected, int* viol_discs, double* min_cbc, double dt, int Bt, int Kf, int S, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BCBF_H */
