// The true pendulum's explicit-Euler step, shared by the per-step safety loop (pendulum.hip) and the in-kernel CLF-CBF QP
// rollout (pendulum_qp.hip): one definition of the plant arithmetic and of the theta wrap.
#pragma once
#include "bcbf_common.h"

namespace bcbf {

// x <- x + xd dt for a given state derivative xd,  theta wrapped to [-pi, pi) as ((theta + pi) % 2 pi) - pi with Python's
// (floored) modulo
template <typename T>
__device__ inline void pendulum_advance(T& th, T& om, T xd0, T xd1, T dt) {
    const T tn = th + xd0 * dt;
    om = om + xd1 * dt;
    const T two_pi = T(2) * T(M_PI);
    T r = fmod(tn + T(M_PI), two_pi);
    if (r < T(0)) r += two_pi;
    th = r - T(M_PI);
}

// the true pendulum: xd = f(x) + g(x) u,  f = [omega, -(g/l) sin theta],  g = [0, 1/(m l)]'
template <typename T>
__device__ inline void pendulum_euler(T& th, T& om, T u, T mass, T gravity, T length, T dt) {
    const T xd0 = om;
    const T xd1 = -(gravity / length) * sin(th) + T(1) / (mass * length) * u;
    pendulum_advance<T>(th, om, xd0, xd1, dt);
}

}  // namespace bcbf
