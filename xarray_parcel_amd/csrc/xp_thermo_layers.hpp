// xp_thermo_layers.hpp -- temperature and humidity over caller-chosen layers (MetPy 1.4): precipitable water, the layer means
// of mixing ratio and relative humidity, thickness and lapse rate between the bounds, and the layer's extremes of equivalent
// potential temperature, for up to four layers of every column, one thread per column.
// The rules are stated in include/xparcel.h and restated in NumPy in tests/thermo_layers_restatement.py.  k_thermo_layers is
// the walk of k_wind_layers (xp_wind_layers.hpp) with other sums: one upward pass with level-major loads serves every layer
// of the call whatever its kind; the points of MetPy's get_layer (which they are: xp_layer_gate.hpp) are emitted in order as
// the walk passes them -- at an added bound point T, Td and z are interpolated in ln p -- into each layer's running state.  A
// lane is done at the first level beyond its highest top; the loop ends with a wave-uniform ballot, so levels above the
// deepest top are never read (an open top reads the whole column).
// What a point carries besides p, T, Td, z -- e_s(Td), w, rh, theta_e -- is evaluated ONCE per level into the column's state
// (Pt) and shared by the layers; at an added bound point it is evaluated from the interpolated T, Td.  A layer keeps only its
// sums, its first and last point and its theta_e extremes: the previous point of a trapezoid is the previous valid level of
// the column, or the bound point emitted in the same step.
// Two definitions: rho_l = 999.97495 kg m^-3 (MetPy 1.4's metpy.constants.rho_l) turns the integral into millimetres, and the
// theta_e extremes are taken over the layer's POINTS, not over the continuous profile between them (the convention of the
// DCAPE source-level search, xp_dcape.hpp).
// Instantiated on the number of layers, on whether a moisture sum (precipitable water, mean mixing ratio, mean RH) is wanted,
// on whether a theta_e output is wanted (a pow-class chain per level and four doubles of state per layer) and on whether a
// bound comes per column (two more doubles per layer); no instantiation may spill (tests/test_thermo_layers_cpu.py; the
// register counts are in DESIGN.md section 7).  It lives in a translation unit of its own (xp_thermo_layers_tu.hip).
#pragma once
#include "xp_wind_layers.hpp"

namespace xp {

constexpr int TL_MAX_LAYERS = WL_MAX_LAYERS;
constexpr double RHO_L = 999.97495;                      // liquid water [kg m^-3] (metpy.constants.rho_l, 1.4)
constexpr double PW_MM = 1e5 / (G * RHO_L);              // trapz(w, p [hPa]) -> mm: hPa -> Pa, m -> mm

struct ThermoLayersArgs {
    View p, t, td, z;                                    // t / td / z .data == nullptr: not supplied
    int64_t nlev, ncol;
    int n;                                               // layers
    int want_rh;                                         // some mean_rh output is wanted: e_s(T) is evaluated
    int kind[TL_MAX_LAYERS], open[TL_MAX_LAYERS];        // open: XP_LAYER_PRESSURE with a NaN scalar top -- to the highest valid level
    double bottom[TL_MAX_LAYERS], top[TL_MAX_LAYERS];    // as the caller gave them (a NaN bottom pressure: the lowest valid level's)
    const void *bottom_col[TL_MAX_LAYERS], *top_col[TL_MAX_LAYERS];   // per column [hPa], in the views' dtype; replace the scalars
    void *pw[TL_MAX_LAYERS], *mean_w[TL_MAX_LAYERS], *mean_rh[TL_MAX_LAYERS], *thickness[TL_MAX_LAYERS], *lapse[TL_MAX_LAYERS];
    void *th_min[TL_MAX_LAYERS], *th_min_p[TL_MAX_LAYERS], *th_max[TL_MAX_LAYERS], *th_max_p[TL_MAX_LAYERS];
    int32_t *status;
};

// (n layers; moisture sums, theta_e, per-column bounds wanted) of a call in the views' dtype: which instantiation runs it
void launch_thermo_layers(const ThermoLayersArgs &a, bool f64, bool moist, bool theta, bool colb, hipStream_t s);

// One point of a column: a valid level, or an added bound point
struct ThermoPt { double p, t, td, z, w, rh, th; };

template <bool MOIST, bool THETA> XP_DEV void thermo_derive(ThermoPt &q, bool want_rh) {
#pragma clang fp contract(off)
    if constexpr (MOIST) {
        const double e = sat_vapor_pressure(q.td);
        q.w = mix_of_e(e, q.p);
        q.rh = want_rh ? fdiv(e, sat_vapor_pressure(q.t)) : 0.0;
    } else { q.w = q.rh = 0.0; }
    q.th = THETA ? theta_e(q.p, q.t, q.td) : 0.0;
}

// the added bound point at pressure pe between the previous level a (higher pressure) and the level b: T, Td, z linear in ln p
template <bool MOIST, bool THETA> XP_DEV ThermoPt thermo_between(double pe, const ThermoPt &a, const ThermoPt &b, bool want_rh) {
#pragma clang fp contract(off)
    const double xe = flog(pe), xa = flog(a.p), xb = flog(b.p);
    const double f = (xe - xb) / (xa - xb);
    ThermoPt q;
    q.p = pe; q.t = b.t + f * (a.t - b.t); q.td = b.td + f * (a.td - b.td); q.z = b.z + f * (a.z - b.z);
    thermo_derive<MOIST, THETA>(q, want_rh);
    return q;
}

// The running state of one layer: a LayerGate plus the trapezoids of w and rh over pressure, the first and the last point, the
// theta_e extremes.
template <bool MOIST, bool THETA, bool COLB> struct ThermoLayer : LayerGate {
    double sw, sr;                           // MOIST: trapz(w, P), trapz(rh, P) so far
    double pf, tf, zf, tl, zl;               // first point, last point
    double tmin, pmin, tmax, pmax;           // THETA: the extremes so far and their pressures
    double pbc, ptc;                         // COLB: this column's bounds (the scalars where no array replaces them)
    XP_DEV void init() {
        init_gate(); sw = sr = 0.0; pf = tf = zf = tl = zl = qnan();
        if constexpr (THETA) tmin = pmin = tmax = pmax = qnan();
    }
    // the point q; b: the point before it, if there is one (started)
    XP_DEV void emit(const ThermoPt &q, const ThermoPt &b) {
#pragma clang fp contract(off)
        if (started) {
            if constexpr (MOIST) {
                const double h = (q.p - b.p) * 0.5;
                sw += h * (q.w + b.w); sr += h * (q.rh + b.rh);
            }
            if constexpr (THETA) {                                           // (the first of equals stays)
                if (q.th < tmin) { tmin = q.th; pmin = q.p; }
                if (q.th > tmax) { tmax = q.th; pmax = q.p; }
            }
        } else {
            started = true; pf = q.p; tf = q.t; zf = q.z;
            if constexpr (THETA) { tmin = tmax = q.th; pmin = pmax = q.p; }
        }
        pl = q.p; tl = q.t; zl = q.z;
    }
    // LayerGate::level's hooks at one valid level `cur` with the previous valid level `prev` below it
    struct Step {
        ThermoLayer &r;
        const ThermoPt &cur, &prev;
        bool want_rh;
        ThermoPt b;                          // the point before the next one emitted, once started: prev, or this step's bound point
        XP_DEV void below() { r.emit(prev, prev); }
        XP_DEV void bound(double pe) {
            const ThermoPt q = thermo_between<MOIST, THETA>(pe, prev, cur, want_rh);
            r.emit(q, b); b = q;
        }
        XP_DEV void here() { r.emit(cur, b); }
    };
};

template <typename T, int NL, bool MOIST, bool THETA, bool COLB> __global__ __launch_bounds__(256)
void k_thermo_layers(ThermoLayersArgs a) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const bool ht = a.t.data != nullptr, htd = a.td.data != nullptr, hz = a.z.data != nullptr;
    const bool want_rh = a.want_rh != 0;
    ThermoLayer<MOIST, THETA, COLB> L[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        L[i].init();
        if constexpr (COLB) {
            L[i].pbc = a.bottom_col[i] ? ld1<T>(a.bottom_col[i], c) : a.bottom[i];
            L[i].ptc = a.top_col[i] ? ld1<T>(a.top_col[i], c) : a.top[i];
        }
    }
    double z0 = qnan(), p0 = qnan();
    ThermoPt prev;
    prev.p = prev.t = prev.td = prev.z = prev.w = prev.rh = prev.th = qnan();
    bool has_prev = false, done = false;
    int bad = 0;
    for (int64_t k = 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        ThermoPt cur;
        cur.p = ld<T>(a.p, k, c);
        cur.t = ht ? ld<T>(a.t, k, c) : 0.0; cur.td = htd ? ld<T>(a.td, k, c) : 0.0; cur.z = hz ? ld<T>(a.z, k, c) : 0.0;
        if (isnan_(cur.p) || isnan_(cur.t) || isnan_(cur.td) || isnan_(cur.z)) continue;   // missing level: dropped
        if (has_prev) {
            bad = ((!hz || cur.z > prev.z) ? 0 : ST_BAD_HEIGHT) | (cur.p < prev.p ? 0 : ST_BAD_PRESSURE);
            if (bad) { done = true; continue; }
        } else {
            z0 = cur.z; p0 = cur.p;
        }
        thermo_derive<MOIST, THETA>(cur, want_rh);
        bool all_fin = true;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            ThermoLayer<MOIST, THETA, COLB> &r = L[i];
            if (r.fin) continue;
            const LayerBounds b = layer_bounds(r, a.kind[i], COLB ? r.pbc : a.bottom[i], COLB ? r.ptc : a.top[i], a.open[i] != 0, z0, p0,
                                               prev.z, prev.p, cur.z, cur.p, has_prev);
            r.level(typename ThermoLayer<MOIST, THETA, COLB>::Step{r, cur, prev, want_rh, prev}, cur.p, prev.p, has_prev, b);
            all_fin = all_fin && r.fin;
        }
        done = all_fin;
        prev = cur; has_prev = true;
    }
    int status = bad;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const ThermoLayer<MOIST, THETA, COLB> &r = L[i];
        // the walk reached the top, and with it the bottom below it; an open top: the column rose above the bottom
        bool ok = !bad && !isnan_(r.pt);
        if (a.open[i]) {
            const double bot = COLB ? r.pbc : a.bottom[i];
            ok = !bad && r.started && r.pl < (isnan_(bot) ? p0 : bot);
        }
        if (!bad && !ok) status |= ST_NO_LAYER;
        const double d = r.pl - r.pf, dz = r.zl - r.zf;
        if constexpr (MOIST) {
            st(a.pw[i], f64, c, ok ? (-r.sw) * PW_MM : qnan());
            st(a.mean_w[i], f64, c, ok ? r.sw / d : qnan());
            st(a.mean_rh[i], f64, c, ok ? r.sr / d : qnan());
        }
        st(a.thickness[i], f64, c, ok ? dz : qnan());
        st(a.lapse[i], f64, c, ok ? -(r.tl - r.tf) / dz * 1000.0 : qnan());
        if constexpr (THETA) {
            st(a.th_min[i], f64, c, ok ? r.tmin : qnan()); st(a.th_min_p[i], f64, c, ok ? r.pmin : qnan());
            st(a.th_max[i], f64, c, ok ? r.tmax : qnan()); st(a.th_max_p[i], f64, c, ok ? r.pmax : qnan());
        }
    }
    sti(a.status, c, status);
}

}  // namespace xp
