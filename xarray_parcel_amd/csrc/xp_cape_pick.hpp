// xp_cape_pick.hpp -- CAPE / CIN of ONE positive layer of the ascent (xp_opts.flags, XP_OPT_LAYER_*): the lowest, the
// highest, the deepest or the one with the most CAPE instead of the reference's envelope (bottom LFC, top EL).  The rule is
// in include/xparcel.h and restated in NumPy in tests/positive_layer_restatement.py.
// One ascent of the chosen parcel, the nodes of xp_cape_cin in the same arithmetic -- k_cape_layers' walk (xp_cape_layers.hpp:
// one thread per column, the wave-uniform level index, xp::below_lcl_node for every node) -- and an observer of the scan's
// crossings (Scan::special's OBS): xp::Scan keeps F+ and F- as running sums and shows every crossing that qualifies as an
// LFC or an EL candidate to Pick::up / Pick::down, which keep two records per column in LDS slots beside the scan's: the
// bottom of the layer that is open, and the best closed layer so far.  Nothing is added to the per-level path: the records
// are touched inside the crossing path only.  Scan::finish still forms the envelope's result; a column with fewer than two
// layers stores it unchanged, so there the call IS the default call.
// LDS: the e_s / ln table, the scan's 13 slots and 14 more per thread: 67120 B per 256-thread workgroup, two workgroups per
// CU -- the layer kernel's operating point (xp_cape_layers.hpp), half the exact-mode xp_cape_cin kernels' occupancy.
#pragma once
#include "xp_kernels.hpp"

namespace xp {

enum { PICK_LOWEST = 1, PICK_HIGHEST = 2, PICK_DEEPEST = 3, PICK_MOST_CAPE = 4 };      // XP_OPT_LAYER_* >> XP_OPT_LAYER_SHIFT

// the slots of a column's two records (field f of thread t at rec[f * SLOT_STRIDE + t]); PK_IDX holds three int32 in two
// doubles: the open bottom's interval index, the best layer's bottom and top index
enum { PK_O_X = 0, PK_O_T, PK_O_C, PK_O_N, PK_B_XL, PK_B_TL, PK_B_CL, PK_B_NL, PK_B_XE, PK_B_TE, PK_B_CE, PK_B_M, PK_IDX, PK_IDX2, PK_FIELDS };

struct Pick {
    double *rec;           // this thread's record slots
    int which;             // PICK_*
    int nclosed;           // layers closed so far
    int open;              // a layer is open (an int for the reason Scan::any_inc gives)
    XP_DEV int *idx() const { return (int *)(rec + PK_IDX * SLOT_STRIDE); }              // [0] open bottom, [1] best bottom; the best top: idx2()
    XP_DEV int *idx2() const { return (int *)(rec + PK_IDX2 * SLOT_STRIDE); }
    XP_DEV void init(double *rec_, int which_) { rec = rec_; which = which_; nclosed = 0; open = 0; }
    // layer number k (1 ...) with bottom (xl, cl) and top (xe, ce): the metric the selection compares
    XP_DEV double metric(int k, double xl, double cl, double xe, double ce) const {
        return which == PICK_LOWEST ? -(double)k : which == PICK_HIGHEST ? (double)k : which == PICK_DEEPEST ? xl - xe : ce - cl;
    }
    // the first layer is taken, a later one on a strictly greater metric: the lower of equals stays, a NaN never wins
    XP_DEV bool wins(int k, double m) const { return k == 1 || m > rec[PK_B_M * SLOT_STRIDE]; }
    XP_DEV void up(const Scan &sc, double xs, double ys, int i) {
        if (open) return;                                                   // an increasing crossing inside an open layer
        open = 1;
        rec[PK_O_X * SLOT_STRIDE] = xs; rec[PK_O_T * SLOT_STRIDE] = ys; idx()[0] = i;
        rec[PK_O_C * SLOT_STRIDE] = sc.cape; rec[PK_O_N * SLOT_STRIDE] = sc.cin;
    }
    XP_DEV void down(const Scan &sc, double xs, double ys, int i) {
        if (!open && nclosed > 0) return;                                   // a decreasing crossing between two layers
        // ON the LCL (within the scan's own tie window there, Scan::special): the layer from the LCL that it would close has
        // no depth, and whether the crossing counts as "above the LCL" at all hangs on the last bit of exp / log
        if (!open && fabs(xs - sc.x_lcl) <= 2e-9) return;
        // no layer yet and none open: the layer began at the LCL (the existing replacement: L = the LCL, lfc_index -2)
        const double xl = open ? rec[PK_O_X * SLOT_STRIDE] : sc.x_lcl, tl = open ? rec[PK_O_T * SLOT_STRIDE] : sc.slot[SL_LCL_T * SLOT_STRIDE];
        const double cl = open ? rec[PK_O_C * SLOT_STRIDE] : sc.slot[SL_CAPE_LCL * SLOT_STRIDE], nl = open ? rec[PK_O_N * SLOT_STRIDE] : sc.slot[SL_CIN_LCL * SLOT_STRIDE];
        const int il = open ? idx()[0] : -2;
        open = 0;
        const int k = ++nclosed;
        const double m = metric(k, xl, cl, xs, sc.cape);
        if (!wins(k, m)) return;
        rec[PK_B_XL * SLOT_STRIDE] = xl; rec[PK_B_TL * SLOT_STRIDE] = tl; rec[PK_B_CL * SLOT_STRIDE] = cl; rec[PK_B_NL * SLOT_STRIDE] = nl;
        rec[PK_B_XE * SLOT_STRIDE] = xs; rec[PK_B_TE * SLOT_STRIDE] = ys; rec[PK_B_CE * SLOT_STRIDE] = sc.cape; rec[PK_B_M * SLOT_STRIDE] = m;
        idx()[1] = il; idx2()[0] = i;
    }
};

// TABLE: the reference's lookup tables instead of the RK4 stepper; HUM: the moisture view holds specific humidity, converted
// on load.  Compiled in a translation unit of its own (xp_cape_pick_tu.hip) with -disable-machine-licm, as k_cape_layers.
template <typename T, bool TABLE, bool HUM> __global__ __launch_bounds__(256)
void k_cape_pick(CapeArgs a, int pmode, int which) {
    struct Lds { double es[LDS_TAB]; double slot[SLOT_FIELDS * SLOT_STRIDE]; double rec[PK_FIELDS * SLOT_STRIDE]; };   // the table first (see k_cape_cin)
    __shared__ Lds lds;
    static_assert(SLOT_STRIDE == 256, "one Scan slot column per thread of the workgroup");
    const double *es = stage_es_table(a.es_tab, lds.es);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    const bool vtc = a.vtc != 0, log_interp = a.log_interp != 0;
    const bool need_w = vtc;
    const int nlev = (int)a.nlev;
    double *const slot = lds.slot + threadIdx.x;

    const Parcel pc = choose_parcel<T, HUM>(a, pmode, c, es, a.depth);
    Lcl l; BelowLcl n; Scan sc;
    int status;
    const bool live = start_column<true>(es, pc, need_w, vtc, true, slot, l, n, sc, status);   // false: a NaN parcel / LCL blanks the profile
    Pick pick; pick.init(lds.rec + threadIdx.x, which);
    Moist m;
    if (live) m.start(es, l.p, n.x_lcl, l.t, TABLE, a.tb);
    // the moist adiabat: see lift_candidate (xp_effective.hpp)
    auto adiabat = [&](bool above, double P, double X, double &tp, double &tvp) __attribute__((always_inline)) {
        if (!TABLE && !above) { tp = l.t; return; }
        tp = m.at(P, X, a.tb);
        tvp = need_w ? virt(tp, mix_of_e(TABLE ? es_tab(es, tp) : m.e, P)) : tp;
    };
    bool lcl_done = false;
    auto feed = [&](double P, double T_, double Td_, bool skew, bool last) __attribute__((always_inline)) {
        lcl_done = below_lcl_node(es, sc, n, vtc, log_interp, P, T_, Td_, skew, last, status, adiabat, &pick);
    };

    // the walk of k_cape_layers (xp_cape_layers.hpp says what each step is for)
    const int first = live ? (int)pc.first : nlev + 1;
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
        LookAhead<T> next(a.p, a.t, a.td, c, k0 < nlev ? k0 : nlev - 1);
        for (int k = k0; k <= nlev; ++k) {
            const bool last = k >= nlev;
            double Pc, Tc, Mc;
            next.take(k + 1, nlev, Pc, Tc, Mc);
            Mc = as_dewpoint<HUM>(es, Pc, Tc, Mc);
            if (last) Pc = Tc = Mc = qnan();
            if (k >= first) {
                const bool skew = lcl_done;
                if (!skew || k > first) feed(skew ? sP : Pc, skew ? sT : Tc, skew ? sM : Mc, skew, last);   // (k == first past the LCL: nothing waits yet)
                sP = Pc; sT = Tc; sM = Mc;
            }
        }
    }

    // ---- results (output pointers fetched from the kernel arguments only now: late_kernargs, xp_lcl_node.hpp) --------------
    const auto late = late_kernargs<CapeArgs>();
    if (!live) { store_blank_column(late->s, c, pc, l, status); return; }
    store_parcel_and_lcl(late->s, c, pc, l);
    Scan::Result r = sc.finish(late->post_zero != 0);                       // the envelope: what a column with K <= 1 stores
    // a layer still open after the last node closes at the lowest valid pressure, with the final F+ and no EL
    const double *rec = pick.rec;
    const double min_p = slot[SL_MIN_P * SLOT_STRIDE];
    const int K = pick.nclosed + pick.open;
    bool top = false;                                                       // the open layer is the chosen one
    if (pick.open) top = pick.wins(K, pick.metric(K, rec[PK_O_X * SLOT_STRIDE], rec[PK_O_C * SLOT_STRIDE], log(min_p), sc.cape));
    const int il = top ? pick.idx()[0] : pick.idx()[1];
    const double xl = rec[(top ? PK_O_X : PK_B_XL) * SLOT_STRIDE], tl = rec[(top ? PK_O_T : PK_B_TL) * SLOT_STRIDE];
    const double cl = rec[(top ? PK_O_C : PK_B_CL) * SLOT_STRIDE], nl = rec[(top ? PK_O_N : PK_B_NL) * SLOT_STRIDE];
    const bool many = K >= 2;
    // (every lane calls crossing_pressure: it ballots)
    const double lp = sc.crossing_pressure(many && il != -2 ? xl : qnan()), ep = sc.crossing_pressure(many && !top ? rec[PK_B_XE * SLOT_STRIDE] : qnan());
    if (many) {
        const double L = il == -2 ? sc.p_lcl : lp, E = top ? min_p : ep;
        const double cE = top ? sc.cape : rec[PK_B_CE * SLOT_STRIDE];
        r.cape = (E < L) ? RD * (cE - cl) : 0.0;
        r.cin = RD * nl;
        if (late->post_zero != 0 && !(r.cin <= 0.0)) r.cin = 0.0;
        r.lfc_p = L; r.lfc_t = tl; r.lfc_idx = il;
        r.el_p = top ? qnan() : ep; r.el_t = top ? qnan() : rec[PK_B_TE * SLOT_STRIDE]; r.el_idx = top ? -1 : pick.idx2()[0];
    }
    store_scan_result(late->s, c, r, status | r.status);
}

// defined in xp_cape_pick_tu.hip: which = PICK_*, pmode = PM_*
void launch_cape_pick(const CapeArgs &a, int pmode, int which, bool f64, bool table, hipStream_t s);

}  // namespace xp
