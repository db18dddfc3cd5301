// xp_dcape.hpp -- downdraft CAPE (metpy.calc.downdraft_cape, MetPy 1.4) for every column of a grid: one thread per
// column, level-major coalesced loads, the e_s table in LDS.  The semantics, step by step, are in DESIGN.md 1 and in the
// NumPy restatement tests/dcape_restatement.py:
//   - levels where p, T or Td is NaN are dropped;
//   - the layer is every level with b >= p >= u (np.isclose counting as equal; b = bottom, u = bottom - depth), plus b and
//     u themselves where no layer level is close to them, with T and Td linear in ln p between the bracketing levels;
//   - the start point is the first layer point with the smallest Bolton theta_e; its wet-bulb temperature (LCL, then the
//     moist adiabat back down: the xp_wet_bulb_temperature chain) starts a moist descent through every level with p >= p0;
//   - DCAPE = -Rd * trapz(Tv_env - Tv_parcel, ln p) over those levels, Tv in MetPy's form T (w + eps) / (eps (1 + w))
//     with w the saturation mixing ratio at Td (environment) or at the parcel temperature (saturated parcel).
// Two wave-uniform passes: upwards until every lane is above u (bounds, running theta_e minimum, highest down level),
// then downwards from that level to the surface (the descent and the trapezoid sum).
#pragma once
#include "xp_kernels.hpp"

namespace xp {

struct DcapeArgs {
    View p, t, td;
    int64_t nlev, ncol;
    double bottom, top;               // b and u = b - depth [hPa]
    int table_mode;
    Tables tb;
    const double *es_tab;
    void *dcape, *p0, *t0;            // per column, in the inputs' dtype (each may be null)
    int32_t *status;
    void *prof;                       // dense (nlev, ncol) parcel temperature, NaN off the down levels (may be null)
};

// value at ln p = x between the levels lo (higher pressure) and hi: MetPy's interpolate_1d on ln p (log_interpolate_1d).
// Without a level below (lo_x NaN) the result is NaN, as MetPy's fill value outside the data.
XP_DEV double log_interp_at(double x, double lo_x, double hi_x, double lo_v, double hi_v) {
    return hi_v + (lo_v - hi_v) * ((x - hi_x) / (lo_x - hi_x));
}

// metpy.calc.virtual_temperature_from_dewpoint: T (w + eps) / (eps (1 + w)), w the saturation mixing ratio at x
XP_DEV double virt_from_dewpoint(const double *es, double p, double t, double x) {
    double w = mix_of_e(es_tab(es, x), p);
    return t * fdiv(w + EPS, EPS * (1.0 + w));
}

// running np.argmin over the layer points in order of decreasing pressure: the first minimum wins, the first NaN beats
// everything.  k: the highest level at or below the point (its down levels end there).
struct DcStart {
    double th, p, t, td;
    int64_t k;
    XP_DEV void init() { th = qnan(); p = qnan(); t = qnan(); td = qnan(); k = -1; }
    XP_DEV void consider(double th_, double p_, double t_, double td_, int64_t k_) {
        const bool take = isnan_(p) || (!isnan_(th) && (isnan_(th_) || th_ < th));
        if (take) { th = th_; p = p_; t = t_; td = td_; k = k_; }
    }
};

template <typename T> __global__ __launch_bounds__(256)
void k_downdraft_cape(DcapeArgs a) {
    __shared__ double s_es[LDS_TAB];
    const double *es = stage_es_table(a.es_tab, s_es);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    const int f64 = sizeof(T) == 8;
    const double b = a.bottom, u = a.top, xb = flog(b), xu = flog(u);

    // -- upward pass: levels 0, 1, ... until every lane has passed u
    double pp = qnan(), xp_ = qnan(), tp = qnan(), tdp = qnan();           // the last valid level
    int64_t kp = -1;
    double pmax = qnan();
    bool crossed_b = false, hit_b = false, hit_u = false, done = false;
    DcStart s; s.init();
    for (int64_t k = 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        const double p = ld<T>(a.p, k, c), t = ld<T>(a.t, k, c), td = ld<T>(a.td, k, c);
        if (isnan_(p) || isnan_(t) || isnan_(td)) continue;                 // missing level: dropped
        if (isnan_(pmax)) pmax = p;
        const double x = flog(p);
        const bool in_layer = (p < b || isclose_(p, b)) && (p > u || isclose_(p, u));
        if (in_layer) { hit_b = hit_b || isclose_(b, p); hit_u = hit_u || isclose_(u, p); }
        if (!crossed_b && p < b) {               // first level above b: b is a point of its own unless a layer level is on it
            crossed_b = true;
            if (!hit_b) {
                const double tb_ = log_interp_at(xb, xp_, x, tp, t), tdb = log_interp_at(xb, xp_, x, tdp, td);
                s.consider(theta_e(b, tb_, tdb), b, tb_, tdb, kp);
            }
        }
        if (in_layer) s.consider(theta_e(p, t, td), p, t, td, k);
        if (p < u && !isclose_(p, u)) {          // first level beyond the layer: u likewise, then this lane is done
            done = true;
            if (!hit_u) {
                const double tu = log_interp_at(xu, xp_, x, tp, t), tdu = log_interp_at(xu, xp_, x, tdp, td);
                s.consider(theta_e(u, tu, tdu), u, tu, tdu, kp);
            }
        }
        pp = p; xp_ = x; tp = t; tdp = td; kp = k;
    }
    // the layer exists if b is not below the lowest level and u not above the highest (np.isclose counting as inside);
    // pp is the highest valid level seen -- beyond u if the lane is done
    const bool layer = (b <= pmax || isclose_(b, pmax)) && (u >= pp || isclose_(u, pp));
    const double p0 = layer ? s.p : qnan();
    const int64_t kd = layer ? s.k : -1;

    // -- start temperature: wet bulb at (p0, T0, Td0), exactly as k_wet_bulb
    const Lcl l = lcl(p0, s.t, s.td);
    Moist m; m.start(es, l.p, log(l.p), l.t, a.table_mode != 0, a.tb);
    double wb = qnan();
    if (!isnan_(p0)) wb = (p0 == l.p) ? m.at(p0, m.x, a.tb) : m.at(p0, log(p0), a.tb);

    // -- downward pass: from the highest down level to the surface, the moist descent from (p0, wb) as k_moist_lapse
    // marches it (increasing pressure), and the trapezoids between consecutive down levels
    m.start(es, p0, flog(p0), wb, a.table_mode != 0, a.tb);
    double sum = 0.0, dprev = qnan(), xprev = qnan();
    bool first = true;
    for (int64_t k = a.nlev - 1; k >= 0; --k) {
        double tpar = qnan();
        if (__builtin_amdgcn_ballot_w64(k <= kd) != 0ull && k <= kd) {
            const double p = ld<T>(a.p, k, c), t = ld<T>(a.t, k, c), td = ld<T>(a.td, k, c);
            if (!(isnan_(p) || isnan_(t) || isnan_(td)) && p >= p0) {
                const double x = flog(p);
                tpar = m.at(p, x, a.tb, true);
                const double d = virt_from_dewpoint(es, p, t, td) - virt_from_dewpoint(es, p, tpar, tpar);
                if (!first) sum += 0.5 * (d + dprev) * (xprev - x);
                first = false; dprev = d; xprev = x;
            }
        }
        st(a.prof, f64, k * a.ncol + c, tpar);
    }
    st(a.dcape, f64, c, layer ? -RD * sum : qnan());
    st(a.p0, f64, c, p0);
    st(a.t0, f64, c, wb);
    sti(a.status, c, (layer ? 0 : ST_NO_LAYER) | (l.not_converged ? ST_LCL_NOT_CONVERGED : 0));
}

}  // namespace xp
