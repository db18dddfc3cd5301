// xp_kinematics.hpp -- storm motion, helicity and the composites built on them (MetPy 1.4; the reference has none):
//   k_bunkers_storm_motion     metpy.calc.bunkers_storm_motion, one thread per column;
//   k_storm_relative_helicity  metpy.calc.storm_relative_helicity for up to four depths, one thread per column;
//   k_helicity_layers          the same between per-column bounds (up to four tops sharing a bottom), plus the bulk wind
//                              difference over each layer -- both are helicity_walk, one with LAYERS and one without;
//   stp_value, scp_value       metpy.calc.significant_tornado and supercell_composite per point, in MetPy's operation
//                              order (their kernel is k_per_point, xp_per_point.hpp).
// The rules are stated in include/xparcel.h and restated in NumPy in tests/kinematics_restatement.py.  Each column kernel
// makes one upward pass with level-major loads (coalesced when col_stride == 1): the layer points of MetPy's get_layer
// (Bunkers; which they are: xp_layer_gate.hpp) / get_layer_heights (SRH) are emitted in order as the walk passes them -- the
// levels, and the added bound points interpolated between the level below and the level above -- into running sums (trapezoids
// for the Bunkers layer means, the helicity terms for SRH).  A lane is done at the first level beyond its highest top; the loop
// ends with a wave-uniform ballot once every lane is done, so levels above 6 km (Bunkers) or the deepest SRH top are never read.
#pragma once
#include "xp_layer_gate.hpp"

namespace xp {

// ---- Bunkers storm motion ----------------------------------------------------------------------------------------------
struct StormMotionArgs {
    View p, u, v, z;
    int64_t nlev, ncol;
    void *right_u, *right_v, *left_u, *left_v, *mean_u, *mean_v;   // per column, in the inputs' dtype (each may be null)
    int32_t *status;
};

// One layer mean M(zb, d) of MetPy's weighted_continuous_average, streamed.  The kernel finds the bound pressures (np.interp,
// linear in height) when the walk reaches the first level at or above each bound height -- one value per bound height,
// shared by the layers that end or begin there -- and the layer emits its points in order of decreasing pressure into
// trapz(u, p) and trapz(v, p).  The sums are taken of the wind relative to the layer's first point, (u0, v0), and
// M = u0 + trapz(u - u0, p) / (p_last - p_first): the same mean, exact for a constant wind (so that zero shear is exactly
// zero and gives MetPy's NaN movers).
struct LayerMean : LayerGate {               // (xp_layer_gate.hpp: which points are the layer's)
    double su, sv, u0, v0, pf, ul, vl;       // trapz sums, first point's wind and pressure, last point's wind relative to the first
    XP_DEV void init() { init_gate(); su = sv = 0.0; u0 = v0 = pf = ul = vl = qnan(); }
    XP_DEV void emit(double p, double u, double v) {
        if (started) { u -= u0; v -= v0; su += (p - pl) * (u + ul) * 0.5; sv += (p - pl) * (v + vl) * 0.5; }
        else { started = true; pf = p; u0 = u; v0 = v; u = v = 0.0; }
        pl = p; ul = u; vl = v;
    }
    // LayerGate::level's hooks at one valid level (p, u, v) with the previous valid level (pp, up, vp) below it
    struct Step {
        LayerMean &r;
        double p, u, v, pp, up, vp;
        XP_DEV void below() { r.emit(pp, up, vp); }
        XP_DEV void bound(double pe) {                                  // u, v linear in ln p
            const double xe = flog(pe), xp_ = flog(pp), x = flog(p);
            const double f = (xe - x) / (xp_ - x);
            r.emit(pe, u + f * (up - u), v + f * (vp - v));
        }
        XP_DEV void here() { r.emit(p, u, v); }
    };
    XP_DEV double mean_u() const { return u0 + su / (pl - pf); }
    XP_DEV double mean_v() const { return v0 + sv / (pl - pf); }
};

// np.interp(zc, z, p) once the walk reaches the first level (z, p) with z >= zc (now); NaN before that
XP_DEV void bound_p(double &pc, bool &now, double zc, double zp, double pp, double z, double p, bool has_prev) {
    now = isnan_(pc) && z >= zc;
    if (now) pc = interp_p(zc, zp, pp, z, p, has_prev);
}

template <typename T> __global__ __launch_bounds__(256)
void k_bunkers_storm_motion(StormMotionArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    LayerMean mean, low, high;                           // z0 ... z0 + 6000, z0 ... z0 + 500, z0 + 5500 ... z0 + 6000
    mean.init(); low.init(); high.init();
    double z0 = qnan(), p0 = qnan(), p500 = qnan(), p5500 = qnan(), p6000 = qnan();   // the bound pressures
    double zp = qnan(), pp = qnan(), up = qnan(), vp = qnan();
    bool has_prev = false, done = false;
    int bad = 0;
    for (int64_t k = 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        const double p = ld<T>(a.p, k, c), u = ld<T>(a.u, k, c), v = ld<T>(a.v, k, c), z = ld<T>(a.z, k, c);
        if (isnan_(p) || isnan_(u) || isnan_(v) || isnan_(z)) continue;      // missing level: dropped
        if (has_prev) {
            bad = (z > zp ? 0 : ST_BAD_HEIGHT) | (p < pp ? 0 : ST_BAD_PRESSURE);
            if (bad) { done = true; continue; }
        } else {
            z0 = z; p0 = p;
        }
        bool n500, n5500, n6000;
        bound_p(p500, n500, z0 + 500.0, zp, pp, z, p, has_prev);
        bound_p(p5500, n5500, z0 + 5500.0, zp, pp, z, p, has_prev);
        bound_p(p6000, n6000, z0 + 6000.0, zp, pp, z, p, has_prev);
        mean.level(LayerMean::Step{mean, p, u, v, pp, up, vp}, p, pp, has_prev, {p0, !has_prev, p6000, n6000});
        low.level(LayerMean::Step{low, p, u, v, pp, up, vp}, p, pp, has_prev, {p0, !has_prev, p500, n500});
        high.level(LayerMean::Step{high, p, u, v, pp, up, vp}, p, pp, has_prev, {p5500, n5500, p6000, n6000});
        done = mean.fin && low.fin && high.fin;
        zp = z; pp = p; up = u; vp = v; has_prev = true;
    }
    // spanned: some level reached z0 + 6000 (then the 500 m layers are complete too)
    const bool ok = !bad && has_prev && !isnan_(p6000);
    double mu = qnan(), mv = qnan(), ru = qnan(), rv = qnan(), lu = qnan(), lv = qnan();
    if (ok) {
        mu = mean.mean_u(); mv = mean.mean_v();
        const double shu = high.mean_u() - low.mean_u(), shv = high.mean_v() - low.mean_v();
        const double s = 7.5 / hypot(shu, shv);
        const double du = shv * s, dv = -shu * s;
        ru = mu + du; rv = mv + dv; lu = mu - du; lv = mv - dv;
    }
    st(a.right_u, f64, c, ru); st(a.right_v, f64, c, rv);
    st(a.left_u, f64, c, lu); st(a.left_v, f64, c, lv);
    st(a.mean_u, f64, c, mu); st(a.mean_v, f64, c, mv);
    sti(a.status, c, bad ? bad : (ok ? 0 : ST_NO_LAYER));
}

// ---- storm-relative helicity, and the bulk wind difference over per-column layers ------------------------------------------
constexpr int SRH_MAX_DEPTHS = 4;

// One argument struct for both kernels.  k_storm_relative_helicity reads its bounds from bottom / top[] (the same for every
// column) and has no shu / shv; k_helicity_layers reads them per column from bottom_col / top_col[] (in the kernel's own
// height convention).
struct SrhArgs {
    View z, u, v;
    int64_t nlev, ncol;
    const void *sfc_u, *sfc_v, *storm_u, *storm_v;   // per column, in the inputs' dtype (each may be null)
    double bottom;
    double top[SRH_MAX_DEPTHS];                       // bottom + depth
    const void *bottom_col;                           // per column
    const void *top_col[SRH_MAX_DEPTHS];              // per column and layer
    int n;                                            // depths / layers
    void *pos[SRH_MAX_DEPTHS], *neg[SRH_MAX_DEPTHS], *tot[SRH_MAX_DEPTHS], *shu[SRH_MAX_DEPTHS], *shv[SRH_MAX_DEPTHS];
    int32_t *status;
};

// the running helicity of one depth: the storm-relative wind of the last point and the two sums
struct SrhSum {
    double ul, vl, pos, neg;
    bool started, top_hit, spanned, fin;
    XP_DEV void init() { ul = vl = qnan(); pos = neg = 0.0; started = top_hit = spanned = fin = false; }
    XP_DEV void emit(double u, double v) {          // storm-relative wind of the next point
#pragma clang fp contract(off)
        if (started) {
            const double t = u * vl - ul * v;
            if (t > 0.0) pos += t;
            if (t < 0.0) neg += t;
        }
        started = true; ul = u; vl = v;
    }
};

// The walk of both kernels.  LAYERS: the bounds are read per column, and next to the helicity sums goes the ground-relative
// wind at top[i] minus the wind at bottom, both linear in height between the levels on either side (xp_wind_shear's rule,
// not MetPy's ln p bulk_shear).  A layer takes part when i < n, bottom >= 0 and top > bottom (a NaN bound fails both
// comparisons); any other is left out (NaN, XP_ST_NO_LAYER).  The fixed-depth entry point only passes bounds that qualify.
template <typename T, bool LAYERS>
XP_DEV void helicity_walk(const SrhArgs &a) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const double cu = a.storm_u ? ld1<T>(a.storm_u, c) : 0.0, cv = a.storm_v ? ld1<T>(a.storm_v, c) : 0.0;
    const double b = LAYERS ? ld1<T>(a.bottom_col, c) : a.bottom;
    SrhSum s[SRH_MAX_DEPTHS];
    double top[SRH_MAX_DEPTHS];
    // (valid[] apart from s[i].fin, and below the fixed-depth tops read from the arguments again, not from top[]: with either
    // written the shorter way the compiler gives k_storm_relative_helicity a 36-byte scratch frame it never touches)
    bool valid[SRH_MAX_DEPTHS];
#pragma unroll
    for (int i = 0; i < SRH_MAX_DEPTHS; ++i) {
        s[i].init();
        top[i] = LAYERS && i < a.n ? ld1<T>(a.top_col[i], c) : a.top[i];
        valid[i] = i < a.n && b >= 0.0 && top[i] > b;
        s[i].fin = !valid[i];
    }
    bool done = !(valid[0] || valid[1] || valid[2] || valid[3]);
    // the walk: the surface point (k = -1) if given, then the levels; h relative to the first valid point without it
    const bool sfc = a.sfc_u != nullptr;
    double hp = qnan(), h0 = sfc ? 0.0 : qnan();
    // the previous point's wind: storm-relative (the helicity), carried as it was formed; LAYERS carries the ground-relative
    // one (the bulk wind difference) and forms the storm-relative one from it again, the same value in two registers fewer
    double up = qnan(), vp = qnan(), gup = qnan(), gvp = qnan();
    double bu = qnan(), bv = qnan();                                        // LAYERS: the ground-relative wind at the bottom
    bool has_prev = false, bottom_ok = false, bottom_hit = false, bottom_done = false;
    int bad = 0;
    for (int64_t k = sfc ? -1 : 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        double h, u, v;
        if (k < 0) { h = 0.0; u = ld1<T>(a.sfc_u, c); v = ld1<T>(a.sfc_v, c); }
        else { h = ld<T>(a.z, k, c); u = ld<T>(a.u, k, c); v = ld<T>(a.v, k, c); }
        if (isnan_(h) || isnan_(u) || isnan_(v)) continue;                  // missing level: dropped
        if (isnan_(h0)) h0 = h;
        h = h - h0;
        if (has_prev && !(h > hp)) { bad = ST_BAD_HEIGHT; done = true; continue; }
        if (!has_prev) bottom_ok = b >= h;                                  // the bottom lies on or above the lowest point
        const double gu = u, gv = v;
        u = u - cu; v = v - cv;
        if constexpr (LAYERS) { up = gup - cu; vp = gvp - cv; }
        const bool above_b = h >= b || isclose_(h, b);
        // the bottom point, where no level equals it: between the level below and this one, in order
        bool add_b = false;
        double ub = qnan(), vb = qnan();
        if (!bottom_done && h >= b) {
            bottom_done = true;
            bottom_hit = h == b;
            if (bottom_hit) { bu = gu; bv = gv; }
            else if (has_prev) {
                add_b = true;
                const double f = (b - hp) / (h - hp);
                ub = up + f * (u - up); vb = vp + f * (v - vp);
                bu = gup + f * (gu - gup); bv = gvp + f * (gv - gvp);
            }
        }
        bool all_fin = true;
#pragma unroll
        for (int i = 0; i < SRH_MAX_DEPTHS; ++i) {
            SrhSum &r = s[i];
            if (r.fin) continue;
            const double t = LAYERS ? top[i] : a.top[i];
            if (add_b) r.emit(ub, vb);
            const bool below_t = h <= t || isclose_(h, t);
            // the first level at or above the top: the wind there minus the wind at the bottom (known by now: bottom < top)
            // is stored right away, not carried to the end of the walk; a column that turns out bad overwrites it below
            if (LAYERS && h >= t && !r.spanned) {
                double tu = gu, tv = gv;
                if (h != t) {
                    const double f = (t - hp) / (h - hp);
                    tu = gup + f * (gu - gup); tv = gvp + f * (gv - gvp);
                }
                int64_t cc = c;                                             // (keeps the eight store addresses from being formed ahead
                asm volatile("" : "+v"(cc));                                // of the loop and carried -- spilled -- through it)
                st(a.shu[i], f64, cc, tu - bu); st(a.shv[i], f64, cc, tv - bv);
            }
            if (h >= t) r.spanned = true;
            // the top point, where no level equals it: before the first level above it
            if (h > t && !r.top_hit) {
                r.top_hit = true;
                if (has_prev) {
                    const double f = (t - hp) / (h - hp);
                    r.emit(up + f * (u - up), vp + f * (v - vp));
                }
            }
            if (above_b && below_t) {
                r.emit(u, v);
                r.top_hit = r.top_hit || h == t;
            }
            if (!below_t) r.fin = true;
            all_fin = all_fin && r.fin;
        }
        done = all_fin;
        hp = h; has_prev = true;
        if constexpr (LAYERS) { gup = gu; gvp = gv; }
        else { up = u; vp = v; }
    }
    int status = bad;
#pragma unroll
    for (int i = 0; i < SRH_MAX_DEPTHS; ++i) {
        if (i >= a.n) continue;
        const bool span = bottom_ok && s[i].spanned;                        // (a layer left out never gets spanned)
        const bool ok = !bad && span && !isnan_(cu) && !isnan_(cv);
        if (!bad && !span) status |= ST_NO_LAYER;
        const double pos = ok ? s[i].pos : qnan(), neg = ok ? s[i].neg : qnan();
        st(a.pos[i], f64, c, pos); st(a.neg[i], f64, c, neg); st(a.tot[i], f64, c, pos + neg);
        if (LAYERS && (bad || !span)) { st(a.shu[i], f64, c, qnan()); st(a.shv[i], f64, c, qnan()); }
    }
    sti(a.status, c, status);
}

template <typename T> __global__ __launch_bounds__(256)
void k_storm_relative_helicity(SrhArgs a) { helicity_walk<T, false>(a); }
// (256, 4: four workgroups per CU, i.e. the compiler has to stay within 128 VGPRs)
template <typename T> __global__ __launch_bounds__(256, 4)
void k_helicity_layers(SrhArgs a) { helicity_walk<T, true>(a); }

// ---- composites ---------------------------------------------------------------------------------------------------------
// metpy.calc.significant_tornado; comparisons with NaN are false, so NaN propagates through the clips
XP_DEV double stp_value(double sbcape, double lcl_height, double srh, double shear) {
#pragma clang fp contract(off)
    double lcl = lcl_height < 1000.0 ? 1000.0 : (lcl_height > 2000.0 ? 2000.0 : lcl_height);
    lcl = (2000.0 - lcl) / 1000.0;
    double shr = shear < 12.5 ? 0.0 : (shear > 30.0 ? 30.0 : shear);
    shr = shr / 20.0;
    return (sbcape * lcl * srh * shr) / (1500.0 * 150.0);
}
// metpy.calc.supercell_composite
XP_DEV double scp_value(double mucape, double srh, double shear) {
#pragma clang fp contract(off)
    double shr = shear < 10.0 ? 0.0 : (shear > 20.0 ? 20.0 : shear);
    shr = shr / 20.0;
    return (mucape / 1000.0) * (srh / 50.0) * shr;
}

}  // namespace xp
