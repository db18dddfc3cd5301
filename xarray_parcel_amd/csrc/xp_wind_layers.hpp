// xp_wind_layers.hpp -- the wind over caller-chosen layers, and two per-point products built on it (MetPy 1.4):
//   k_wind_layers   metpy.calc.mean_pressure_weighted and bulk_shear over up to four layers given by pressure, by pressure
//                   depth or by height above the lowest level, the wind at each layer's bottom and the layer's strongest
//                   wind, one thread per column;
//   critical_angle_value, stp_effective_value   per point (their kernel is k_per_point, xp_per_point.hpp).
// The rules are stated in include/xparcel.h and restated in NumPy in tests/wind_layers_restatement.py.  The column kernel is
// the walk of k_bunkers_storm_motion (xp_kinematics.hpp) with the layers as arguments: one upward pass with level-major
// loads (coalesced when col_stride == 1) serves every layer of the call whatever its kind; the points of MetPy's get_layer
// (which they are: xp_layer_gate.hpp) are emitted in order as the walk passes them into each layer's running sums, the added
// bound points being the only places a logarithm is taken.  A lane is done at the first level beyond its highest top; the
// loop ends with a wave-uniform ballot, so levels above the deepest top are never read.  The kernel is instantiated on the
// number of layers and on whether a strongest-wind output is wanted: a layer's state is 9 doubles, 13 with the strongest
// wind, and no instantiation may spill (tests/test_wind_layers_cpu.py; the register counts are in DESIGN.md section 7).  It
// lives in a translation unit of its own (xp_wind_layers_tu.hip).
#pragma once
#include "xp_layer_gate.hpp"

namespace xp {

constexpr int WL_MAX_LAYERS = 4;

struct WindLayersArgs {
    View p, u, v, z;                                     // z.data == nullptr: no height
    int64_t nlev, ncol;
    int n;                                               // layers
    int kind[WL_MAX_LAYERS];
    double bottom[WL_MAX_LAYERS], top[WL_MAX_LAYERS];    // as the caller gave them (a NaN bottom pressure: the lowest valid level's)
    void *mean_u[WL_MAX_LAYERS], *mean_v[WL_MAX_LAYERS], *shear_u[WL_MAX_LAYERS], *shear_v[WL_MAX_LAYERS];
    void *bottom_u[WL_MAX_LAYERS], *bottom_v[WL_MAX_LAYERS];
    void *max_u[WL_MAX_LAYERS], *max_v[WL_MAX_LAYERS], *max_p[WL_MAX_LAYERS];
    int32_t *status;
};

// (n layers, strongest wind wanted) of a call in the views' dtype: which instantiation runs it
void launch_wind_layers(const WindLayersArgs &a, bool f64, bool want_max, hipStream_t s);

// The running state of one layer: a LayerGate plus its sums.  The trapezoids of mean_pressure_weighted, trapz(U P, P), are summed
// of the wind relative to the layer's first point (u0, v0), so that mean = u0 + trapz((U - u0) P, P) / (0.5 (P_last^2 -
// P_first^2)) is exact for a constant wind, and the relative wind of the last point is the bulk shear.
template <bool MAXW> struct WindLayer : LayerGate {
    double su, sv, u0, v0, pf, ul, vl;       // sums, first point's wind and pressure, last point's relative wind
    double ms, mu, mv, mp;                   // MAXW: the strongest point so far: speed, wind, pressure
    XP_DEV void init() {
        init_gate(); su = sv = 0.0; u0 = v0 = pf = ul = vl = qnan();
        if constexpr (MAXW) { ms = -1.0; mu = mv = mp = qnan(); }
    }
    XP_DEV void emit(double p, double u, double v, double s) {          // s: hypot(u, v)
#pragma clang fp contract(off)
        if constexpr (MAXW) {
            if (s > ms) { ms = s; mu = u; mv = v; mp = p; }             // (the first of equals stays)
        }
        if (started) {
            u -= u0; v -= v0;
            const double h = (p - pl) * 0.5;
            su += h * (u * p + ul * pl); sv += h * (v * p + vl * pl);
        } else { started = true; pf = p; u0 = u; v0 = v; u = v = 0.0; }
        pl = p; ul = u; vl = v;
    }
    // LayerGate::level's hooks at one valid level (p, u, v; s its speed) with the previous valid level (pp, up, vp) below it
    struct Step {
        WindLayer &r;
        double p, u, v, s, pp, up, vp;
        XP_DEV void below() { r.emit(pp, up, vp, MAXW ? hypot(up, vp) : 0.0); }
        XP_DEV void bound(double pe) {                                  // u, v linear in ln p
#pragma clang fp contract(off)
            const double xe = flog(pe), xp_ = flog(pp), x = flog(p);
            const double f = (xe - x) / (xp_ - x);
            const double ue = u + f * (up - u), ve = v + f * (vp - v);
            r.emit(pe, ue, ve, MAXW ? hypot(ue, ve) : 0.0);
        }
        XP_DEV void here() { r.emit(p, u, v, s); }
    };
};

template <typename T, int NL, bool MAXW> __global__ __launch_bounds__(256)
void k_wind_layers(WindLayersArgs a) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const bool hz = a.z.data != nullptr;
    WindLayer<MAXW> L[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) L[i].init();
    double z0 = qnan(), p0 = qnan();
    double zp = qnan(), pp = qnan(), up = qnan(), vp = qnan();
    bool has_prev = false, done = false;
    int bad = 0;
    for (int64_t k = 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        const double p = ld<T>(a.p, k, c), u = ld<T>(a.u, k, c), v = ld<T>(a.v, k, c);
        const double z = hz ? ld<T>(a.z, k, c) : 0.0;
        if (isnan_(p) || isnan_(u) || isnan_(v) || isnan_(z)) continue;      // missing level: dropped
        if (has_prev) {
            bad = ((!hz || z > zp) ? 0 : ST_BAD_HEIGHT) | (p < pp ? 0 : ST_BAD_PRESSURE);
            if (bad) { done = true; continue; }
        } else {
            z0 = z; p0 = p;
        }
        const double s = MAXW ? hypot(u, v) : 0.0;
        bool all_fin = true;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            WindLayer<MAXW> &r = L[i];
            if (r.fin) continue;
            const LayerBounds b = layer_bounds(r, a.kind[i], a.bottom[i], a.top[i], false, z0, p0, zp, pp, z, p, has_prev);
            r.level(typename WindLayer<MAXW>::Step{r, p, u, v, s, pp, up, vp}, p, pp, has_prev, b);
            all_fin = all_fin && r.fin;
        }
        done = all_fin;
        zp = z; pp = p; up = u; vp = v; has_prev = true;
    }
    int status = bad;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const WindLayer<MAXW> &r = L[i];
        const bool ok = !bad && !isnan_(r.pt);           // the walk reached the top, and with it the bottom below it
        if (!bad && !ok) status |= ST_NO_LAYER;
        const double den = 0.5 * ((r.pl - r.pf) * (r.pl + r.pf));
        st(a.mean_u[i], f64, c, ok ? r.u0 + r.su / den : qnan()); st(a.mean_v[i], f64, c, ok ? r.v0 + r.sv / den : qnan());
        st(a.shear_u[i], f64, c, ok ? r.ul : qnan()); st(a.shear_v[i], f64, c, ok ? r.vl : qnan());
        st(a.bottom_u[i], f64, c, ok ? r.u0 : qnan()); st(a.bottom_v[i], f64, c, ok ? r.v0 : qnan());
        if constexpr (MAXW) {
            st(a.max_u[i], f64, c, ok ? r.mu : qnan()); st(a.max_v[i], f64, c, ok ? r.mv : qnan());
            st(a.max_p[i], f64, c, ok ? r.mp : qnan());
        }
    }
    sti(a.status, c, status);
}

// ---- per point: the value functions ------------------------------------------------------------------------------------
// metpy.calc.critical_angle as atan2(|a x b|, a . b) [degrees]: a the 0-500 m shear, b the storm-relative surface inflow
XP_DEV double critical_angle_value(double au, double av, double su, double sv, double cu, double cv) {
#pragma clang fp contract(off)
    const double bu = cu - su, bv = cv - sv;
    if ((au == 0.0 && av == 0.0) || (bu == 0.0 && bv == 0.0)) return qnan();
    const double cross = au * bv - av * bu, dot = au * bu + av * bv;
    return atan2(fabs(cross), dot) * (180.0 / 3.141592653589793);
}
// SPC's effective-layer significant tornado parameter; comparisons with NaN are false, so NaN propagates through the clips
XP_DEV double stp_effective_value(double mlcape, double mlcin, double lcl_height, double esrh, double ebwd) {
#pragma clang fp contract(off)
    double lcl = lcl_height < 1000.0 ? 1000.0 : (lcl_height > 2000.0 ? 2000.0 : lcl_height);
    lcl = (2000.0 - lcl) / 1000.0;
    double cin = mlcin < -200.0 ? -200.0 : (mlcin > -50.0 ? -50.0 : mlcin);
    cin = (200.0 + cin) / 150.0;
    double shr = ebwd < 12.5 ? 0.0 : (ebwd > 30.0 ? 30.0 : ebwd);
    shr = shr / 20.0;
    return ((((mlcape / 1500.0) * lcl) * (esrh / 150.0)) * shr) * cin;
}

}  // namespace xp
