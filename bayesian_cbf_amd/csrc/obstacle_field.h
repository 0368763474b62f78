// What the obstacle-field translation units share (obstacle_field.hip: select / audit / commit; field_plant.hip: the commit on a
// plant drawn from the posterior): the wave-per-instance mapping, the disc row in fp64, the wave's lexicographic minimum, and the
// host-side argument checks.
#ifndef BCBF_OBSTACLE_FIELD_H
#define BCBF_OBSTACLE_FIELD_H
#include <limits>
#include <stdio.h>
#include "bcbf_common.h"
#include "unicycle_task.h"

namespace bcbf {

constexpr int FIELD_LAPS = BCBF_MAX_FIELD / 64;      // discs per lane
constexpr int FIELD_WAVES = 4;                       // instances per workgroup (waves never talk to each other)

// (value, index) pairs, ordered by value then by index: the wave's minimum, known to every lane afterwards
__device__ inline void wave_lexmin(double& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// ObstacleCBF of one disc at (px, py, th) in fp64: grad h, and gam * h  (unicycle_row's obstacle branch)
__device__ inline void field_row(double px, double py, double th, double cx, double cy, double rad, double tw0, double tw1,
                                 double gam, double (&g)[3], double& cst) {
    const double z[3] = {0.0, 0.0, 0.0};
    unicycle_row_vals<double>(1, px, py, th, z, z, z, 0.0, cx, cy, rad, tw0, tw1, gam, g, cst);
}

constexpr int FIELD_NONE = 0x7fffffff;               // "no disc": above every index

static int field_einval(const char* entry, const char* why) {
    char msg[240];
    snprintf(msg, sizeof(msg), "%s: %s", entry, why);
    set_error_message(msg);
    return BCBF_EINVAL;
}

static bool field_finite(double v) { return fabs(v) <= std::numeric_limits<double>::max(); }

static const char* field_shape(int Bt, int Kf, int S, int field_stride) {
    if (Bt <= 0) return "Bt <= 0";
    if (S < 1 || S > 3) return "S must be 1..3 (the fused solver's obstacle lanes)";
    if (Kf < S || Kf > BCBF_MAX_FIELD) return "Kf must be S..BCBF_MAX_FIELD";
    if (field_stride != 0 && field_stride != 1) return "field_stride must be 0 (shared) or 1 (per instance)";
    return nullptr;
}

}  // namespace bcbf
#endif
