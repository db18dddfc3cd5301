// xp_cape_layers.hpp -- CAPE / CIN over per-column pressure layers (0-3 km CAPE, hail-growth-zone CAPE, ...): one ascent of
// the chosen parcel, the nodes of xp_cape_cin in the same arithmetic, and 1 ... 4 layers per column clipped out of it.  The
// rules are in include/xparcel.h and restated in NumPy in tests/layer_cape_restatement.py.
// xp::Scan keeps CAPE and CIN as running sums of positive and negative area (Scan::cape, Scan::cin) that it snapshots at
// the LCL node, the LFC and the EL; Scan::finish forms its results from differences of those snapshots.  A layer bound is
// one more place to snapshot the same two sums: F+(ln p) and F-(ln p), the sums as they stand at a bound -- after the node
// below it plus the part of the interval up to the bound (area_up_to) -- and then
//     cape = RD * max(0, min(cE, F+(top)) - max(cL, F+(bottom))),   cin = RD * min(0, max(nL, F-(top)) - F-(bottom))
// with cL, cE, nL what finish() used (Scan::terms): exact because F+ never decreases and F- never increases with height.
// No second ascent and no profile arrays.
// One thread per column, the e_s / ln table, the Scan slots and the bound slots in LDS.  Per bound two LDS doubles: the
// bound's ln p until the ascent passes it, F+ there afterwards, and F-; which of the two the first holds is a bit of the
// lane's `pending` mask.  The ascent only compares each node's ln p with the highest pending bound (xnext); everything
// else sits behind that one branch, taken at most eight times per column.
// The level index is WAVE-UNIFORM, as in the effective-inflow kernel (xp_effective.hpp): the wavefront walks up from the
// lowest first level of its lanes -- a most-unstable or mixed-layer parcel starts where its search left it -- and a lane
// sits out until the walk reaches its own; the level loads stay level-major and coalesced.  Every lane feeds exactly one
// node per iteration through xp::below_lcl_node (xp_lcl_node.hpp).
#pragma once
#include "xp_kernels.hpp"

namespace xp {

constexpr int CL_MAX_LAYERS = 4;
struct CapeLayersArgs {
    CapeArgs base;                    // views, shape, parcel, options, tables (base.s / base.prof / base.flags unused)
    int pmode, nlayer;
    const void *bottom[CL_MAX_LAYERS], *top[CL_MAX_LAYERS];    // hPa per column, in the views' dtype (bottom[i] may be null)
    void *cape[CL_MAX_LAYERS], *cin[CL_MAX_LAYERS];            // per column, in the views' dtype (each may be null)
    void *total_cape, *total_cin, *lfc_p, *el_p, *lcl_p;
    int32_t *status;
};

// The area of y between ln p = Xo and xb, Xn <= xb <= Xo, split by sign (ap >= 0, an <= 0): y is linear in ln p from
// (Xo, yo) to (Xn, yn) with its zero where Scan::special puts it.  An interval with a NaN end has no area (Scan::add).
XP_DEV void area_up_to(double Xo, double yo, double Xn, double yn, double xb, double &ap, double &an) {
    const bool same = (yn * yo > 0.0) | ((yn == 0.0) & (yo == 0.0));
    double a1, a2 = 0.0;
    if (same) {
        const double yb = yo + (yn - yo) * fdiv(Xo - xb, Xo - Xn);
        a1 = (Xo - xb) * ((yo + yb) * 0.5);
    } else {
        const double xs = fdiv(yn * Xo - yo * Xn, yn - yo);
        if (xb >= xs) {                                                     // the bound lies below the zero
            const double yb = yo * fdiv(xb - xs, Xo - xs);
            a1 = (Xo - xb) * ((yo + yb) * 0.5);
        } else {                                                            // the lower triangle and part of the upper one
            const double yb = yn * fdiv(xs - xb, xs - Xn);
            a1 = (yo * 0.5) * fabs(Xo - xs);
            a2 = (xs - xb) * (yb * 0.5);
        }
    }
    ap = fmax(a1, 0.0) + fmax(a2, 0.0);                                     // maxNum / minNum drop a NaN operand
    an = fmin(a1, 0.0) + fmin(a2, 0.0);
}

// TABLE: the reference's lookup tables instead of the RK4 stepper.  Compiled in a translation unit of its own
// (xp_cape_layers_tu.hip) with -disable-machine-licm, for the reason k_effective_inflow gives.
template <typename T, bool TABLE> __global__ __launch_bounds__(256)
void k_cape_layers(CapeLayersArgs a) {
    struct Lds { double es[LDS_TAB]; double slot[SLOT_FIELDS * SLOT_STRIDE]; double snap[4 * CL_MAX_LAYERS * SLOT_STRIDE]; };   // the table first (see k_cape_cin)
    __shared__ Lds lds;
    static_assert(SLOT_STRIDE == 256, "one Scan slot column per thread of the workgroup");
    const double *es = stage_es_table(a.base.es_tab, lds.es);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.base.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const CapeArgs &b = a.base;
    const bool vtc = b.vtc != 0, log_interp = b.log_interp != 0;
    const bool need_w = vtc;
    const int nlev = (int)b.nlev, nlayer = a.nlayer;
    double *const slot = lds.slot + threadIdx.x;
    double *const snap = lds.snap + threadIdx.x;             // bound q (2 i: bottom of layer i, 2 i + 1: its top) at snap[2 q], snap[2 q + 1]

    // ---- the bounds: ln p of each into its slot; a layer without a bottom starts at the first node (F = 0) ---------------
    unsigned pending = 0, nolayer = 0;
    double xnext = -__builtin_inf();                         // the highest ln p among the pending bounds
    for (int i = 0; i < nlayer; ++i) {
        const double pb = a.bottom[i] ? ld1<T>(a.bottom[i], c) : qnan(), pt = ld1<T>(a.top[i], c);
        const bool bad = isnan_(pt) || pt >= pb;                            // (a NaN bottom compares false)
        snap[(4 * i) * SLOT_STRIDE] = 0.0; snap[(4 * i + 1) * SLOT_STRIDE] = 0.0;
        snap[(4 * i + 2) * SLOT_STRIDE] = 0.0; snap[(4 * i + 3) * SLOT_STRIDE] = 0.0;
        if (bad) nolayer |= 1u << i;
        if (!bad && !isnan_(pb)) { const double x = log(pb); snap[(4 * i) * SLOT_STRIDE] = x; pending |= 1u << (2 * i); xnext = fmax(xnext, x); }
        if (!bad) { const double x = log(pt); snap[(4 * i + 2) * SLOT_STRIDE] = x; pending |= 2u << (2 * i); xnext = fmax(xnext, x); }
    }

    const Parcel pc = choose_parcel<T, false>(b, a.pmode, c, es, b.depth);
    Lcl l; BelowLcl n; Scan sc;
    int status;
    const bool live = start_column<true>(es, pc, need_w, vtc, true, slot, l, n, sc, status);   // false: a NaN parcel / LCL blanks the profile
    Moist m;
    if (live) m.start(es, l.p, n.x_lcl, l.t, TABLE, b.tb);
    // the moist adiabat: see lift_candidate (xp_effective.hpp)
    auto adiabat = [&](bool above, double P, double X, double &tp, double &tvp) __attribute__((always_inline)) {
        if (!TABLE && !above) { tp = l.t; return; }
        tp = m.at(P, X, b.tb);
        tvp = need_w ? virt(tp, mix_of_e(TABLE ? es_tab(es, tp) : m.e, P)) : tp;
    };
    bool lcl_done = false;
    // One node, and the bounds it passes: every pending bound at or below the node just fed (ln p >= the node's) takes
    // the sums as they stood before the node plus the part of the interval up to the bound -- after the first node of the
    // column that is F = 0, the "from the first node" of a bottom below it.  A bound ON the node takes the sums after it.
    auto feed = [&](double P, double T_, double Td_, bool skew, bool last) __attribute__((always_inline)) {
        const double Xo = sc.Xp, yo = sc.yp, co = sc.cape, no = sc.cin;
        lcl_done = below_lcl_node(es, sc, n, vtc, log_interp, P, T_, Td_, skew, last, status, adiabat);
        const double Xn = sc.Xp;
        if (Xn <= xnext) {
            const double yn = sc.yp;
            double xn = -__builtin_inf();
            for (int q = 0; q < 2 * nlayer; ++q) {
                if (!((pending >> q) & 1u)) continue;
                const double xb = snap[(2 * q) * SLOT_STRIDE];
                if (xb >= Xn) {
                    double ap, an;
                    area_up_to(Xo, yo, Xn, yn, xb, ap, an);
                    snap[(2 * q) * SLOT_STRIDE] = (xb == Xn) ? sc.cape : co + ap;
                    snap[(2 * q + 1) * SLOT_STRIDE] = (xb == Xn) ? sc.cin : no + an;
                    pending &= ~(1u << q);
                } else xn = fmax(xn, xb);
            }
            xnext = xn;
        }
    };

    const int first = live ? (int)pc.first : nlev + 1;                      // (a blank column sits the whole walk out)
    // mixed layer: the parcel is the new level 0 of its profile (pf.py:1641-1644); a supersaturated mixed parcel lies above
    // its own LCL: the LCL node went first and the parcel node follows it
    const bool pre = pc.prepend && live;
    if (__builtin_amdgcn_ballot_w64(pre) != 0ull && pre) {
        feed(pc.p, pc.t, pc.td, false, false);
        const bool again = lcl_done;
        if (__builtin_amdgcn_ballot_w64(again) != 0ull && again) feed(pc.p, pc.t, pc.td, true, false);
    }
    int k0 = nlev + 1;
    for (int probe = 0; probe <= nlev; ++probe) if (__builtin_amdgcn_ballot_w64(first <= probe) != 0ull) { k0 = probe; break; }
    if (k0 <= nlev) {
        double sP = qnan(), sT = qnan(), sM = qnan();                       // the level that waits while the LCL node is fed
        LookAhead<T> next(b.p, b.t, b.td, c, k0 < nlev ? k0 : nlev - 1);
        for (int k = k0; k <= nlev; ++k) {
            const bool last = k >= nlev;
            double Pc, Tc, Mc;
            next.take(k + 1, nlev, Pc, Tc, Mc);
            if (last) Pc = Tc = Mc = qnan();
            if (k >= first) {
                const bool skew = lcl_done;
                if (!skew || k > first) feed(skew ? sP : Pc, skew ? sT : Tc, skew ? sM : Mc, skew, last);   // (k == first past the LCL: nothing waits yet)
                sP = Pc; sT = Tc; sM = Mc;
            }
        }
    }

    // ---- results (output pointers fetched from the kernel arguments only now: late_kernargs, xp_lcl_node.hpp) --------------
    const auto late = late_kernargs<CapeLayersArgs>();
    if (nolayer) status |= ST_NO_LAYER;
    if (!live) {
        for (int i = 0; i < nlayer; ++i) {
            const double v = ((nolayer >> i) & 1u) ? qnan() : 0.0;
            st(late->cape[i], f64, c, v); st(late->cin[i], f64, c, v);
        }
        st(late->total_cape, f64, c, 0.0); st(late->total_cin, f64, c, 0.0);
        st(late->lfc_p, f64, c, qnan()); st(late->el_p, f64, c, qnan()); st(late->lcl_p, f64, c, l.p);
        sti(late->status, c, status);
        return;
    }
    const Scan::Result r = sc.finish(late->base.post_zero != 0);
    const Scan::Terms t = sc.terms(r);
    for (int i = 0; i < nlayer; ++i) {
        // a bound the ascent never passed lies above the last valid node: "to the top", the final sums
        const bool pb_ = (pending >> (2 * i)) & 1u, pt_ = (pending >> (2 * i + 1)) & 1u;
        const double fpb = pb_ ? sc.cape : snap[(4 * i) * SLOT_STRIDE], fnb = pb_ ? sc.cin : snap[(4 * i + 1) * SLOT_STRIDE];
        const double fpt = pt_ ? sc.cape : snap[(4 * i + 2) * SLOT_STRIDE], fnt = pt_ ? sc.cin : snap[(4 * i + 3) * SLOT_STRIDE];
        double cape = (t.E < t.L) ? RD * fmax(0.0, fmin(t.cE, fpt) - fmax(t.cL, fpb)) : 0.0;
        double cin = isnan_(t.L) ? 0.0 : RD * fmin(0.0, fmax(t.nL, fnt) - fnb);
        if ((nolayer >> i) & 1u) cape = cin = qnan();
        st(late->cape[i], f64, c, cape); st(late->cin[i], f64, c, cin);
    }
    st(late->total_cape, f64, c, r.cape); st(late->total_cin, f64, c, r.cin);
    st(late->lfc_p, f64, c, r.lfc_p); st(late->el_p, f64, c, r.el_p); st(late->lcl_p, f64, c, l.p);
    sti(late->status, c, status | r.status);
}

// defined in xp_cape_layers_tu.hip
void launch_cape_layers(const CapeLayersArgs &a, bool f64, bool table, hipStream_t s);

}  // namespace xp
