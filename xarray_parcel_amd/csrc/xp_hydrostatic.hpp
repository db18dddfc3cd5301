// xp_hydrostatic.hpp -- hydrostatic heights and layer thickness from pressure, temperature and humidity (MetPy's
// thickness_hydrostatic, accumulated level by level): the height of every valid level of every column and the thickness of up
// to four layers by pressure, one thread per column, ONE upward pass with level-major coalesced loads through the look-ahead
// reader (xp_level_reader.hpp) and level-major coalesced stores of the heights.  Also the value functions of the two per-point
// products that go with it, geopotential <-> height (k_per_point, xp_per_point.hpp).
// The rules are stated in include/xparcel.h and restated in NumPy in tests/hydrostatic_restatement.py.
//   - per valid level: x = ln p (flog), Tv = T (w + eps) / (eps (1 + w)) with w from the dewpoint (Bolton's e_s, as
//     xp_thermo_layers.hpp evaluates it), from the specific humidity (q / (1 - q), no dewpoint in between) or 0; the height
//     is the running sum of (RD / G) (0.5 (Tv_a + Tv_b)) (x_a - x_b) over consecutive valid levels from base_height.
//   - the layers are those of k_thermo_layers restricted to the pressure kinds: the points of MetPy's get_layer through
//     LayerGate / layer_bounds (xp_layer_gate.hpp); at an added bound point T and the moisture are interpolated in ln p and Tv
//     is evaluated from them; a layer keeps its gate and ONE sum, which starts at 0 at its first point -- so a thickness never
//     sees base_height.  The previous point of a trapezoid is the previous valid level of the column, or the bound point
//     emitted in the same step.
//   - the whole column is always read: every level gets a height, and a level out of order anywhere sets ST_BAD_PRESSURE.
// e_s and ln come from fexp / flog, not from the library's LDS tables: the tables are interpolants (the values would not be
// those the header states), they would cost a table snapshot and 11.8 KB of LDS per block, and the pass is bound by its four
// (nlev, ncol) arrays, not by its arithmetic.
// Instantiated on dtype x {no moisture, dewpoint, specific humidity} x the number of layers (0 ... 4: a call with one layer -- MetPy's
// thickness_hydrostatic -- does not carry the registers of four); no instantiation may spill or use
// scratch (tests/test_hydrostatic_cpu.py; the register counts are in _lib.py).  It lives in a translation unit of its own
// (xp_hydrostatic_tu.hip).
#pragma once
#include "xp_layer_gate.hpp"
#include "xp_level_reader.hpp"

namespace xp {

constexpr int HY_MAX_LAYERS = 4;
constexpr int HY_DRY = 0, HY_DEWPOINT = 1, HY_SPECIFIC = 2;      // what the moisture view holds
constexpr double RD_OVER_G = RD / G;
constexpr double EARTH_RADIUS = 6371008.7714;                    // metpy.constants.Re [m]

struct HydrostaticArgs {
    View p, t, m;                                        // m.data == nullptr: a dry atmosphere
    int64_t nlev, ncol;
    int n;                                               // layers, 0 ... 4
    int kind[HY_MAX_LAYERS], open[HY_MAX_LAYERS];        // open: XP_LAYER_PRESSURE with a NaN top -- to the highest valid level
    double bottom[HY_MAX_LAYERS], top[HY_MAX_LAYERS];    // as the caller gave them (a NaN bottom: the lowest valid level's pressure)
    const void *base;                                    // the height of the lowest valid level per column [m], views' dtype; null: 0
    void *height;                                        // dense (nlev, ncol), nullable
    void *thickness[HY_MAX_LAYERS];                      // ncol each, nullable
    int32_t *status;
};

// hum: HY_*; a call in the views' dtype: which instantiation runs it
void launch_hydrostatic(const HydrostaticArgs &a, bool f64, int hum, hipStream_t s);

// metpy.calc.geopotential_to_height and height_to_geopotential, in MetPy's operation order
XP_DEV double geopotential_to_height_value(double phi) {
#pragma clang fp contract(off)
    return (phi * EARTH_RADIUS) / (G * EARTH_RADIUS - phi);
}
XP_DEV double height_to_geopotential_value(double z) {
#pragma clang fp contract(off)
    return (G * EARTH_RADIUS * z) / (EARTH_RADIUS + z);
}

// Tv of one point from its pressure, temperature and moisture value
template <int HUM> XP_DEV double hydro_virtual(double p, double t, double m) {
#pragma clang fp contract(off)
    if constexpr (HUM == HY_DRY) return t;
    const double w = HUM == HY_DEWPOINT ? mix_of_e(sat_vapor_pressure(m), p) : fdiv(m, 1.0 - m);
    return t * fdiv(w + EPS, EPS * (1.0 + w));
}

// One point of a column -- a valid level, or an added bound point -- as the trapezoid reads it, and a valid level in full
struct HydroPt { double x, tv; };
struct HydroLevel { double p, t, m, x, tv; };

// The running state of one layer: a LayerGate plus the thickness so far
template <int HUM> struct HydroLayer : LayerGate {
    double sum;
    XP_DEV void init() { init_gate(); sum = 0.0; }
    // the point q at pressure p; b: the point before it, if there is one (started)
    XP_DEV void emit(double p, const HydroPt &q, const HydroPt &b) {
#pragma clang fp contract(off)
        if (started) sum = sum + RD_OVER_G * (0.5 * (b.tv + q.tv)) * (b.x - q.x);
        started = true; pl = p;
    }
    // LayerGate::level's hooks at one valid level `cur` with the previous valid level `prev` below it
    struct Step {
        HydroLayer &r;
        const HydroLevel &cur, &prev;
        HydroPt b;                           // the point before the next one emitted, once started: prev, or this step's bound point
        XP_DEV void below() { r.emit(prev.p, HydroPt{prev.x, prev.tv}, b); }
        XP_DEV void bound(double pe) {
#pragma clang fp contract(off)
            const double xe = flog(pe);
            const double f = (xe - cur.x) / (prev.x - cur.x);
            const double t = cur.t + f * (prev.t - cur.t), m = HUM == HY_DRY ? 0.0 : cur.m + f * (prev.m - cur.m);
            const HydroPt q = {xe, hydro_virtual<HUM>(pe, t, m)};
            r.emit(pe, q, b); b = q;
        }
        XP_DEV void here() { r.emit(cur.p, HydroPt{cur.x, cur.tv}, b); }
    };
};

template <typename T, int HUM, int NL> __global__ __launch_bounds__(256)
void k_hydrostatic(HydrostaticArgs a) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    HydroLayer<HUM> L[NL > 0 ? NL : 1];
#pragma unroll
    for (int i = 0; i < NL; ++i) L[i].init();
    const double base = a.base ? ld1<T>(a.base, c) : 0.0;
    double z = qnan(), p0 = qnan();
    HydroLevel prev;
    prev.p = prev.t = prev.m = prev.x = prev.tv = qnan();
    bool has_prev = false, bad = false;
    auto next = [&] {                                    // (the dry call reads two arrays)
        if constexpr (HUM == HY_DRY) return LookAhead2<T>(a.p, a.t, c, 0);
        else return LookAhead<T>(a.p, a.t, a.m, c, 0);
    }();
    for (int64_t k = 0; k < a.nlev; ++k) {
        HydroLevel cur;
        if constexpr (HUM == HY_DRY) { next.take(k + 1, k + 1 < a.nlev, cur.p, cur.t); cur.m = 0.0; }
        else next.take(k + 1, a.nlev, cur.p, cur.t, cur.m);
        const int64_t o = k * a.ncol + c;
        const bool valid = !(isnan_(cur.p) || isnan_(cur.t) || isnan_(cur.m));
        bad = bad || (valid && has_prev && !(cur.p < prev.p));
        if (!valid || bad) { st(a.height, f64, o, qnan()); continue; }     // a missing level: dropped; from a level out of order upward: NaN
        cur.x = flog(cur.p);
        cur.tv = hydro_virtual<HUM>(cur.p, cur.t, cur.m);
        if (has_prev) z = z + RD_OVER_G * (0.5 * (prev.tv + cur.tv)) * (prev.x - cur.x);
        else { z = base; p0 = cur.p; }
        st(a.height, f64, o, z);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            HydroLayer<HUM> &r = L[i];
            if (r.fin) continue;
            const LayerBounds b = layer_bounds(r, a.kind[i], a.bottom[i], a.top[i], a.open[i] != 0, 0.0, p0, 0.0, prev.p, 0.0, cur.p, has_prev);
            r.level(typename HydroLayer<HUM>::Step{r, cur, prev, HydroPt{prev.x, prev.tv}}, cur.p, prev.p, has_prev, b);
        }
        prev = cur; has_prev = true;
    }
    int status = bad ? ST_BAD_PRESSURE : has_prev ? 0 : ST_NO_LAYER;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const HydroLayer<HUM> &r = L[i];
        // the walk reached the top, and with it the bottom below it; an open top: the column rose above the bottom
        bool ok = !bad && !isnan_(r.pt);
        if (a.open[i]) ok = !bad && r.started && r.pl < (isnan_(a.bottom[i]) ? p0 : a.bottom[i]);
        if (!bad && !ok) status |= ST_NO_LAYER;
        st(a.thickness[i], f64, c, ok ? r.sum : qnan());
    }
    sti(a.status, c, status);
}

}  // namespace xp
