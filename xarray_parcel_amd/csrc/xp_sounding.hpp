// xp_sounding.hpp -- the classic sounding indices (K, total / cross / vertical totals, Showalter, SWEAT) and the convective
// condensation level with the convective temperature (MetPy 1.4's k_index, total_totals_index, cross_totals, vertical_totals,
// showalter_index, sweat_index, ccl) for every column of a grid: one thread per column, level-major coalesced loads through
// the look-ahead level reader (xp_level_reader.hpp), the e_s table in LDS for the Showalter parcel's moist adiabat.
// The rules are stated in include/xparcel.h and restated in NumPy in tests/sounding_indices_restatement.py.
// One upward, wave-uniform walk keeps the last thermodynamically valid level (p, T, Td non-NaN) and the last wind-valid
// level (p, u, v non-NaN) and, as it passes them,
//   - resolves T and Td at 850, 700 and 500 hPa and u, v at 850 and 500 hPa: a valid level on the isobar gives its values
//     as they are, otherwise log_interp_at (xp_dcape.hpp) between the valid levels on either side;
//   - evaluates rt(p), the dewpoint of the CCL's constant mixing ratio, at every valid level and keeps the first or the last
//     sign change of rt - T (the crossing arithmetic of find_intersections: intersect(), xp_primitives.hpp).
// u and v are read only by lanes that are still at or below 500 hPa on the wind levels.  A lane is done once it has
// everything it was asked for -- past 500 hPa where no CCL output is wanted or, for the lowest crossing, once that is found;
// the last crossing needs the whole column -- and the loop ends for a wavefront when all of its lanes are done.
// The mixed-layer CCL's mixing ratio is a pre-pass over the lowest `depth` hPa: the w sum of select_ml (xp_kernels.hpp),
// i.e. k_mixed_layer with v = w_s(p, Td).
// The Showalter parcel is lifted AFTER the walk, not at the level that closes the 500 hPa bracket: the result is the same
// and the lanes of a wavefront then run the LCL iteration and the RK4 march together instead of each at its own level.
// Instantiated on dtype x {winds or not} x {no CCL, surface CCL, mixed-layer CCL}; no instantiation may spill
// (tests/test_sounding_indices_cpu.py).  It lives in a translation unit of its own (xp_sounding_tu.hip).
#pragma once
#include "xp_dcape.hpp"
#include "xp_primitives.hpp"

namespace xp {

constexpr int ST_NO_CCL = 128;
constexpr int CCL_NONE = 0, CCL_SURFACE = 1, CCL_MIXED = 2;      // the kernel's CCL template argument
constexpr int CCL_TOP = 0, CCL_BOTTOM = 1;                       // XP_CCL_*
constexpr double KNOT = 1852.0 / 3600.0;                         // m/s per knot
constexpr double DEG = 57.29577951308232;                        // degrees per radian

struct SoundingArgs {
    View p, t, td, u, v;
    int64_t nlev, ncol;
    int table_mode, which;            // which: CCL_TOP / CCL_BOTTOM
    int want_index;                   // some output of the 850 ... 500 hPa group is wanted
    double ml_depth;                  // CCL_MIXED: the mixing depth [hPa]
    Tables tb;
    const double *es_tab;
    void *k_index, *total_totals, *cross_totals, *vertical_totals, *showalter, *sweat;   // per column, the inputs' dtype
    void *ccl_p, *ccl_t, *conv_t;
    int32_t *status;
};

// (winds read, CCL kind) of a call in the views' dtype: which instantiation runs it
void launch_sounding(const SoundingArgs &a, bool f64, bool wind, int ccl, hipStream_t s);

// The mixed-layer mean of w_s(p, Td) over the lowest `depth` hPa: mixed_layer (pf.py:137-162) of the mixing ratio, the
// statements of k_mixed_layer / select_ml's s_w.
template <typename T> XP_DEV double mixed_layer_w(const View &pv, const View &tdv, int64_t nlev, int64_t c, double depth) {
    double bottom = qnan(), top = qnan(), s = 0.0, pp = qnan(), vp = qnan(), pb = qnan(), vb = qnan();
    bool closed = false;
    T np_ = ldr<T>(pv, 0, c), ntd_ = ldr<T>(tdv, 0, c);                     // one level ahead, as LookAhead (xp_level_reader.hpp)
    for (int64_t k = 0; k < nlev; ++k) {
        const double p = (double)np_, td = (double)ntd_;
        if (k + 1 < nlev) { np_ = ldr<T>(pv, k + 1, c); ntd_ = ldr<T>(tdv, k + 1, c); }
        const double v = sat_mix(p, td);
        if (isnan_(bottom) && !isnan_(p)) { bottom = p; top = bottom - depth; }
        if (!isnan_(p) && p < top) {
            double cb = flog(pb), ca = flog(p), va = v;
            if (pb == top) { ca = cb; va = vb; }
            layer_mean_step(s, pp, vp, top, interp_rule(vb, va, flog(top), cb, ca));
            closed = true;
            break;
        }
        if (k > 0) layer_mean_step(s, pp, vp, p, v);
        pp = p; vp = v;
        if (!isnan_(p)) { pb = p; vb = v; }
    }
    if (!closed) layer_mean_step(s, pp, vp, top, (pb == top) ? vb : qnan());
    return (1.0 / fabs(top - bottom)) * s;
}

// Two variables at the isobar P (ln P = X) as the walk reaches the first valid level (p, x; v1, v2) at or above it; the valid
// level below: (xq; q1, q2), NaN where there is none.
XP_DEV void at_isobar(bool &have, double P, double X, double p, double x, double v1, double v2, double xq, double q1, double q2,
                      double &o1, double &o2) {
    if (have || !(p <= P)) return;
    have = true;
    if (p == P) { o1 = v1; o2 = v2; return; }
    o1 = log_interp_at(X, xq, x, q1, v1); o2 = log_interp_at(X, xq, x, q2, v2);
}

// speed [kt] and meteorological direction [degrees, (0, 360]] of the wind (u, v) [m/s]
XP_DEV void knots_and_direction(double u, double v, double &f, double &dir) {
#pragma clang fp contract(off)
    f = __builtin_sqrt(u * u + v * v) / KNOT;
    dir = 90.0 - atan2(-v, -u) * DEG;
    if (dir <= 0.0) dir += 360.0;
}

template <typename T, bool WIND, int CCL> __global__ __launch_bounds__(256)
void k_sounding(SoundingArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_es[LDS_TAB];
    const double *es = stage_es_table(a.es_tab, s_es);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const bool index = a.want_index != 0;
    const double X850 = flog(850.0), X700 = flog(700.0), X500 = flog(500.0);

    // -- the CCL's mixing ratio, as the factor e / p = r / (eps + r) of vapor_pressure()
    double ef = qnan();
    if constexpr (CCL == CCL_MIXED) {
        const double r = mixed_layer_w<T>(a.p, a.td, a.nlev, c, a.ml_depth);
        ef = fdiv(r, EPS + r);
    }

    double xq = qnan(), tq = qnan(), tdq = qnan();                          // the last thermodynamically valid level
    double xw = qnan(), uw = qnan(), vw = qnan();                           // the last wind-valid level
    double t850 = qnan(), td850 = qnan(), t700 = qnan(), td700 = qnan(), t500 = qnan(), td500 = qnan();
    double u850 = qnan(), v850 = qnan(), u500 = qnan(), v500 = qnan();
    bool h850 = false, h700 = false, h500 = false, w850 = false, w500 = false;
    bool first = true, wfirst = true, span_lo = false, wspan_lo = false;
    double p0 = qnan(), pq = qnan(), dq = qnan(), rtq = qnan();             // CCL: the start level; p, rt - T and rt at the last valid level
    double cp = qnan(), cy = qnan();                                        // the chosen crossing: pressure and rt there
    bool found = false, done = false;

    LookAhead<T> next(a.p, a.t, a.td, c, 0);
    for (int64_t k = 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        double p, t, td;
        next.take(k + 1, a.nlev, p, t, td);
        const bool wneed = WIND && !w500;
        double u = qnan(), v = qnan();
        if (wneed) { u = ld<T>(a.u, k, c); v = ld<T>(a.v, k, c); }
        if (isnan_(p)) continue;                                            // neither kind of level
        const double x = flog(p);
        if (!(isnan_(t) || isnan_(td))) {                                   // a thermodynamically valid level
            if (first) span_lo = p >= 850.0;
            if (index) {
                at_isobar(h850, 850.0, X850, p, x, t, td, xq, tq, tdq, t850, td850);
                at_isobar(h700, 700.0, X700, p, x, t, td, xq, tq, tdq, t700, td700);
                at_isobar(h500, 500.0, X500, p, x, t, td, xq, tq, tdq, t500, td500);
            }
            if constexpr (CCL != CCL_NONE) {
                double rt;
                if (first) {
                    p0 = p;
                    if constexpr (CCL == CCL_SURFACE) {
                        const double r = sat_mix(p, td);
                        ef = fdiv(r, EPS + r);
                    }
                }
                if (CCL == CCL_SURFACE && first) rt = td;                   // the start level: Td0 itself, an exact zero when saturated
                else rt = dewpoint_fast(p * ef);
                const double d = rt - t;
                const bool take = !(found && a.which == CCL_BOTTOM);
                if (!first && take && !isnan_(d) && !isnan_(dq) && sign_(d) != sign_(dq)) {
                    found = true;
                    if (dq == 0.0) { cp = pq; cy = rtq; }                   // a level ON the crossing is the crossing
                    else if (d == 0.0) { cp = p; cy = rt; }
                    else {
                        const Intersection r = intersect(xq, x, rtq, rt, tq, t);
                        cp = fexp(r.x); cy = r.y;
                    }
                }
                pq = p; dq = d; rtq = rt;
            }
            xq = x; tq = t; tdq = td; first = false;
        }
        if (wneed && !(isnan_(u) || isnan_(v))) {                           // a wind-valid level
            if (wfirst) wspan_lo = p >= 850.0;
            at_isobar(w850, 850.0, X850, p, x, u, v, xw, uw, vw, u850, v850);
            at_isobar(w500, 500.0, X500, p, x, u, v, xw, uw, vw, u500, v500);
            xw = x; uw = u; vw = v; wfirst = false;
        }
        done = (!index || h500) && (!WIND || w500) && (CCL == CCL_NONE || (a.which == CCL_BOTTOM && found));
    }

    int status = 0;
    if (index) {
        const bool span = span_lo && h500;
        if (!span) status |= ST_NO_LAYER;
        const double vt = t850 - t500, ct = td850 - t500, tt = vt + ct;
        st(a.vertical_totals, f64, c, span ? vt : qnan());
        st(a.cross_totals, f64, c, span ? ct : qnan());
        st(a.total_totals, f64, c, span ? tt : qnan());
        st(a.k_index, f64, c, span ? (vt + (td850 - 273.15)) - (t700 - td700) : qnan());
        if (a.showalter) {
            // the parcel (850 hPa, T850, Td850): dry to its LCL (dry_lapse, pf.py:291), moist from there to 500 hPa (k_moist_lapse's march)
            const Lcl l = lcl<true>(span ? 850.0 : qnan(), t850, td850);
            if (l.not_converged) status |= ST_LCL_NOT_CONVERGED;
            Moist m; m.start(es, l.p, flog(l.p), l.t, a.table_mode != 0, a.tb);
            double tp = qnan();
            if (!isnan_(l.p)) tp = (l.p <= 500.0) ? t850 * fpow(500.0 / 850.0, KAPPA) : m.at(500.0, X500, a.tb);
            st(a.showalter, f64, c, t500 - tp);
        }
        if constexpr (WIND) {
            double sweat = qnan();
            if (span && wspan_lo && w500) {
                double f850, d850, f500, d500;
                knots_and_direction(u850, v850, f850, d850);
                knots_and_direction(u500, v500, f500, d500);
                const double tdc = td850 - 273.15;
                const bool on = d850 >= 130.0 && d850 <= 250.0 && d500 >= 210.0 && d500 <= 310.0 && d500 - d850 > 0.0 &&
                                f850 >= 15.0 && f500 >= 15.0;
                const double shear = on ? 125.0 * (sin((d500 - d850) / DEG) + 0.2) : 0.0;
                sweat = (((12.0 * (tdc > 0.0 ? tdc : 0.0) + 20.0 * (tt - 49.0 > 0.0 ? tt - 49.0 : 0.0)) + 2.0 * f850) + f500) + shear;
            }
            st(a.sweat, f64, c, sweat);
        }
    }
    if constexpr (CCL != CCL_NONE) {
        if (!found) status |= ST_NO_CCL;
        st(a.ccl_p, f64, c, cp);
        st(a.ccl_t, f64, c, cy);
        st(a.conv_t, f64, c, cy * fpow(p0 / cp, KAPPA));
    }
    sti(a.status, c, status);
}

}  // namespace xp
