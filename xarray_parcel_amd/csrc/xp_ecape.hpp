// xp_ecape.hpp -- entraining CAPE (Peters, Chavas, Su, Morrison and Coffer 2023, J. Atmos. Sci.): what the library lacks of
// its ingredients, and the formula itself:
//   k_ncape       the buoyancy-dilution potential NCAPE of every column: between the LFC and the EL, the integral over height
//                 of -(g / (cp T)) (hbar - hs), hbar the mean of the environment's moist static energy from the lowest valid
//                 level up to the height in question and hs its saturated moist static energy there; one thread per column;
//   ecape_value   per point (its kernel is k_per_point, xp_per_point.hpp): CAPE reduced analytically for entrainment.
// The rules are stated in include/xparcel.h and restated in NumPy in tests/ecape_restatement.py.  The column kernel is the
// walk of k_wind_layers (xp_wind_layers.hpp) over the environment alone: one upward pass with level-major loads of p, T, Td
// and z (coalesced when col_stride == 1), the running trapezoid integral of h carried from the lowest valid level, the two
// bound points interpolated between the level below and the level above -- z linear in ln p, b linear in z: the only
// logarithms taken.  A lane is done at the first valid level at or beyond its upper bound; the loop ends with a wave-uniform
// ballot, so levels above the highest EL of a wavefront are never read.  All arithmetic is in double under fp contract(off),
// in the order the restatement follows.  It lives in a translation unit of its own (xp_ecape_tu.hip); it may not spill and
// keeps four waves per SIMD (tests/test_ecape_cpu.py; the register counts are in DESIGN.md section 7).
#pragma once
#include "xp_kernels.hpp"

namespace xp {

struct NcapeArgs {
    View p, t, td, z;
    int64_t nlev, ncol;
    const void *lfc_p, *el_p;                            // per column, in the views' dtype
    void *ncape, *lfc_z, *el_z;                          // the same (each may be null)
    int32_t *status;
};

void launch_ncape(const NcapeArgs &a, bool f64, hipStream_t s);

// the bound pressure pb between the valid level below (pp, zp, bp) and the valid level above (p, z, b), pp > pb > p
XP_DEV void ncape_bound(double pb, double pp, double zp, double bp, double p, double z, double b, double &zb, double &bb) {
#pragma clang fp contract(off)
    const double x = flog(p);
    const double f = (flog(pb) - x) / (flog(pp) - x);
    zb = z + f * (zp - z);
    bb = b + f * (bp - b);
}

template <typename T> __global__ __launch_bounds__(256)
void k_ncape(NcapeArgs a) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    double pl = ld1<T>(a.lfc_p, c), pe = ld1<T>(a.el_p, c);    // L and E; clamped to p0 at the lowest valid level
    const bool no_lfc = isnan_(pl), inverted = !no_lfc && pe >= pl;          // (a NaN E compares false)
    double z0 = qnan(), zp = qnan(), pp = qnan(), bp = qnan(), hp = qnan();  // the lowest valid level; the previous one
    double I = 0.0;                                      // trapz(h, z) from z0 to the previous valid level
    double sum = 0.0, zq = qnan(), bq = qnan();          // trapz(b, z) from z_L to the last point (zq, bq)
    double zl = qnan(), ze = qnan();                     // z_L, z_E once the walk has reached them
    int nvalid = 0, bad = 0;
    bool started = false, fin = false, done = no_lfc || inverted;
    for (int64_t k = 0; k < a.nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        const double p = ld<T>(a.p, k, c), t = ld<T>(a.t, k, c), td = ld<T>(a.td, k, c), z = ld<T>(a.z, k, c);
        if (isnan_(p) || isnan_(t) || isnan_(td) || isnan_(z)) continue;     // missing level: dropped
        const double w = sat_mix(p, td), ws = sat_mix(p, t);
        const double q = w / (1.0 + w), qs = ws / (1.0 + ws);
        const double dry = CP_D * t, gz = G * z;
        const double h = (dry + LV * q) + gz, hs = (dry + LV * qs) + gz;
        double hbar = h;
        if (nvalid) {
            bad = (z > zp ? 0 : ST_BAD_HEIGHT) | (p < pp ? 0 : ST_BAD_PRESSURE);
            if (bad) { done = true; continue; }
            I += (0.5 * (h + hp)) * (z - zp);
            hbar = I / (z - z0);
        } else {
            z0 = z;
            pl = pl > p ? p : pl; pe = pe > p ? p : pe;  // clamped into the column from below (a NaN E stays NaN)
        }
        const double b = -(G / dry) * (hbar - hs);
        ++nvalid;
        if (!fin) {
            bool on_l = false;                           // the level itself is the point z_L
            if (!started && p <= pl) {
                started = true;
                on_l = p == pl;
                if (on_l) { zq = z; bq = b; } else ncape_bound(pl, pp, zp, bp, p, z, b, zq, bq);
                zl = zq;
            }
            if (started) {
                const bool top = p <= pe;                // at or beyond E: the point z_E closes the integral
                double zn = z, bn = b;
                if (top && p != pe) ncape_bound(pe, pp, zp, bp, p, z, b, zn, bn);
                if (!(on_l && !top)) sum += (0.5 * (bn + bq)) * (zn - zq);
                zq = zn; bq = bn;
                if (top) { ze = zn; fin = true; }
            }
        }
        done = fin && nvalid >= 2;
        zp = z; pp = p; bp = b; hp = h;
    }
    // the walk ran out of levels below E (a NaN E, or one above the highest valid level): the integral ends at that level;
    // below L as well: the layer, clamped onto the highest valid level, is empty
    if (!fin) {
        if (!started) zl = zp;
        ze = zp;
    }
    int status = bad;
    double r_n = qnan(), r_l = qnan(), r_e = qnan();
    if (no_lfc) r_n = 0.0;
    else if (inverted || (!bad && nvalid < 2)) status = ST_NO_LAYER;
    else if (!bad) { r_n = sum; r_l = zl - z0; r_e = ze - z0; }
    st(a.ncape, f64, c, r_n); st(a.lfc_z, f64, c, r_l); st(a.el_z, f64, c, r_e);
    sti(a.status, c, status);
}

// ---- per point: ECAPE from CAPE, NCAPE, the EL height and the storm-relative inflow --------------------------------------
// k^2 a^2 pi^2 Lmix / (4 Pr s^2) with k = 0.42, a = 0.8, Lmix = 120 m, Pr = 1/3, s = 1.1 [m]
constexpr double ECAPE_C_PSI = 82.87727046436741;
// y: ecape, ecape_a (with the inflow's kinetic energy), psi
XP_DEV void ecape_value(double cape, double ncape, double el_height, double sr_u, double sr_v, double *y) {
#pragma clang fp contract(off)
    y[0] = y[1] = y[2] = qnan();
    if (isnan_(cape) || isnan_(ncape) || isnan_(sr_u) || isnan_(sr_v) || !(el_height > 0.0)) return;
    const double psi = ECAPE_C_PSI / el_height;
    y[0] = y[1] = 0.0; y[2] = psi;
    if (cape <= 0.0) return;
    const double sp = hypot(sr_u, sr_v);
    const double V = sp > 1e-3 ? sp : 1e-3;
    const double V2 = V * V, K = 0.5 * V2, e = psi / V2;
    const double B = (1.0 + psi) + (2.0 * e) * ncape;
    const double x = (8.0 * e) * (cape - psi * ncape);
    const double r = B * B + x;
    if (r < 0.0) return;                                 // entrainment leaves no updraft
    const double s = sqrt(r);
    const double num = B >= 0.0 ? (B + s == 0.0 ? 0.0 : x / (B + s)) : s - B;          // (no cancellation)
    const double ea = K + num / (4.0 * e);
    y[1] = ea > 0.0 ? ea : 0.0;
    const double en = y[1] - K;
    y[0] = en > 0.0 ? en : 0.0;
}

}  // namespace xp
