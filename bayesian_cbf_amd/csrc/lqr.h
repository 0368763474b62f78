// lqr.hip's entry point for the pendulum step (pendulum.hip, nominal = 1).
#pragma once

namespace bcbf {

// The LQR nominal control of the pendulum step (n = 2, m = 1): bcbf_lqr_nominal_f64's kernel, then the explorer's draw
// (explore[Bt,2], eps) and the clip to [lo, hi] on its result.  x_goal[2], Q[2,2]: HOST values.
int lqr_nominal_step_f64(const double* Mk, const double* Mj, const double* x, const double* x_goal, const double* Q, double R,
                         double dt, int numSteps, int t, const int* t_dev, const double* explore, double eps, int clip,
                         double lo, double hi, double* u_ref, int* lstatus, int Bt, void* stream);

}  // namespace bcbf
