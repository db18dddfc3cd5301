// xp_per_point.hpp -- the per-point products: ONE kernel, k_per_point, instantiated on the operation.  An operation names its
// inputs and outputs (NIN <= 6, NOUT <= 4) and maps the values of one point, as doubles, through the product's value function,
// which lives with the kernels it belongs to (xp_bundle.hpp, xp_kinematics.hpp, xp_wind_layers.hpp, xp_ecape.hpp, xp_hydrostatic.hpp) and keeps MetPy's / the
// reference's operation order under fp contract(off).  have[i]: input i was given (an input an entry point lets be null).
#pragma once
#include "xp_bundle.hpp"
#include "xp_kinematics.hpp"
#include "xp_wind_layers.hpp"
#include "xp_ecape.hpp"
#include "xp_hydrostatic.hpp"

namespace xp {

struct PointArgs {
    int64_t n;
    const void *in[6];                                   // in the call's dtype; null: not given
    void *out[4];                                        // the same; null: not wanted
};

template <typename T, typename Op> __global__ __launch_bounds__(256)
void k_per_point(PointArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n) return;
    double x[Op::NIN], y[Op::NOUT];
    bool have[Op::NIN];
#pragma unroll
    for (int i = 0; i < Op::NIN; ++i) {
        have[i] = a.in[i] != nullptr;
        x[i] = have[i] ? ld1<T>(a.in[i], c) : qnan();
    }
    Op::apply(x, have, y);
#pragma unroll
    for (int i = 0; i < Op::NOUT; ++i) st(a.out[i], sizeof(T) == 8, c, y[i]);
}

struct ShipOp {                                          // xp_significant_hail_parameter
    static constexpr int NIN = 6, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *, double *y) { y[0] = ship_value(x[0], x[1], x[2], x[3], x[4], x[5]); }
};
struct StpOp {                                           // xp_significant_tornado
    static constexpr int NIN = 4, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *, double *y) { y[0] = stp_value(x[0], x[1], x[2], x[3]); }
};
struct ScpOp {                                           // xp_supercell_composite
    static constexpr int NIN = 3, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *, double *y) { y[0] = scp_value(x[0], x[1], x[2]); }
};
struct CriticalAngleOp {                                 // xp_critical_angle
    static constexpr int NIN = 6, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *, double *y) { y[0] = critical_angle_value(x[0], x[1], x[2], x[3], x[4], x[5]); }
};
struct CorfidiOp {                                       // xp_corfidi_storm_motion; Corfidi (2003): upwind = mean - jet,
    static constexpr int NIN = 4, NOUT = 4;              // downwind = mean + upwind
    static XP_DEV void apply(const double *x, const bool *, double *y) {
#pragma clang fp contract(off)
        const double uu = x[0] - x[2], uv = x[1] - x[3];
        y[0] = uu; y[1] = uv;
        y[2] = x[0] + uu; y[3] = x[1] + uv;
    }
};
struct StpEffectiveOp {                                  // xp_significant_tornado_effective; x[5]: base_height, may be absent
    static constexpr int NIN = 6, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *have, double *y) {
        y[0] = stp_effective_value(x[0], x[1], x[2], x[3], x[4]);
        if (have[5] && x[5] > 0.0) y[0] = 0.0;           // the inflow layer is not surface based
    }
};
struct EcapeOp {                                         // xp_ecape: cape, ncape, el_height, sr_u, sr_v -> ecape, ecape_a, psi
    static constexpr int NIN = 5, NOUT = 3;
    static XP_DEV void apply(const double *x, const bool *, double *y) { ecape_value(x[0], x[1], x[2], x[3], x[4], y); }
};
struct GeopotentialToHeightOp {                          // xp_geopotential_to_height
    static constexpr int NIN = 1, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *, double *y) { y[0] = geopotential_to_height_value(x[0]); }
};
struct HeightToGeopotentialOp {                          // xp_height_to_geopotential
    static constexpr int NIN = 1, NOUT = 1;
    static XP_DEV void apply(const double *x, const bool *, double *y) { y[0] = height_to_geopotential_value(x[0]); }
};

}  // namespace xp
