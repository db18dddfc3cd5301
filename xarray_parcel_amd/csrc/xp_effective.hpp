// xp_effective.hpp -- the effective inflow layer (Thompson et al. 2007) of every column of a grid: the lowest contiguous
// run of levels whose lifted parcels have CAPE >= cape_min and CIN >= cin_min.  The rules are in include/xparcel.h and
// restated in NumPy in tests/effective_layer_restatement.py:
//   - a level is valid when p, T and Td are all non-NaN; the candidates are the valid levels with p >= p0 - search_depth
//     (p0 the lowest valid level's pressure), in level order;
//   - candidate k is lifted as xp_cape_cin lifts the surface parcel of the column cut off below k, the same nodes in the
//     same arithmetic: what is written to candidate_cape / candidate_cin is what xp_cape_cin writes for that view;
//   - base = the first passing candidate, top = the last passing candidate before the first failure above the base;
//     candidates above that failure are not lifted.
// One thread per column, the e_s / ln table and the Scan slots in LDS.  The candidate index is WAVE-UNIFORM: the outer loop
// runs k = 0, 1, ... for the whole wavefront, a lane whose level k is invalid, outside its window, or whose layer is closed
// sits the candidate out, and a ballot ends the loop when no lane has work left.  Every lane that takes part in a candidate
// starts at level k, so the level loads stay level-major and coalesced and the inner loop bound is scalar.  The LCL differs
// per lane; each lane feeds exactly one node per inner iteration -- below its LCL the level just loaded, at the crossing the
// LCL node instead (the level waits), above it the level that has been waiting -- which is k_cape_cin's phase A, node for
// node, including its tie rules (LCL_SNAP, the saturated parcel, a level on the LCL).
#pragma once
#include "xp_kernels.hpp"

namespace xp {

struct EffectiveArgs {
    View p, t, td, z;                 // z.data may be null (no heights)
    int64_t nlev, ncol;
    double cape_min, cin_min, depth;
    int vtc, log_interp, pos_neg, post_zero;
    Tables tb;
    const double *es_tab;
    void *base_p, *top_p, *base_z, *top_z;   // per column, in the inputs' dtype (each may be null)
    int32_t *base_idx, *top_idx, *status;
    void *cand_cape, *cand_cin;              // dense (nlev, ncol), NaN where the level was not lifted (each may be null)
};

// CAPE / CIN of the parcel of level k0 lifted through the levels k0 ... nlev - 1 of column c: k_cape_cin's surface parcel
// on the views cut off below k0.  k0 and nlev are wave-uniform; every active lane runs the same nlev - k0 + 1 iterations.
template <typename T, bool TABLE>
XP_DEV void lift_candidate(const EffectiveArgs &a, const double *es, double *slot, int64_t c, int k0, int nlev,
                           double pc_p, double pc_t, double pc_td, double &cape, double &cin, int &status) {
    const bool vtc = a.vtc != 0, pos_neg = a.pos_neg != 0, log_interp = a.log_interp != 0;
    const bool need_w = vtc;
    const Lcl l = lcl<true>(pc_p, pc_t, pc_td);
    status = l.not_converged ? ST_LCL_NOT_CONVERGED : 0;
    cape = 0.0; cin = 0.0;
    if (isnan_(l.p)) return;                                               // a NaN LCL blanks the profile: CAPE = CIN = 0.0
    const double vf_parcel = need_w ? virt_factor_tab(es, pc_t, pc_td, pc_p, false) : 1.0;
    const double x_lcl = log(l.p);
    const double x0 = (pc_p == l.p) ? x_lcl : log_tab<true>(es, pc_p);

    Scan sc; sc.init(l.p, x_lcl, pos_neg, slot);
    sc.slot[SL_LCL_T * SLOT_STRIDE] = vtc ? l.tv : l.t;
    Moist m;
    m.start(es, l.p, x_lcl, l.t, TABLE, a.tb);
    double *const br = sc.slot;
    br[SL_BR_P * SLOT_STRIDE] = qnan(); br[SL_BR_X * SLOT_STRIDE] = qnan(); br[SL_BR_T * SLOT_STRIDE] = qnan(); br[SL_BR_TD * SLOT_STRIDE] = qnan();

    bool lcl_done = false;
    double sP = qnan(), sT = qnan(), sM = qnan();                          // the level that waits while the LCL node is fed
    // one-level look-ahead, kept in the input type until it is used (see select_mu_exact)
    T np_ = ldr<T>(a.p, k0, c), nt_ = ldr<T>(a.t, k0, c), ntd_ = ldr<T>(a.td, k0, c);
    for (int k = k0; k <= nlev; ++k) {
        const bool last = k >= nlev;
        const double Pc = last ? qnan() : (double)np_, Tc = last ? qnan() : (double)nt_, Mc = last ? qnan() : (double)ntd_;
        if (k + 1 < nlev) { np_ = ldr<T>(a.p, k + 1, c); nt_ = ldr<T>(a.t, k + 1, c); ntd_ = ldr<T>(a.td, k + 1, c); }
        // ---- k_cape_cin's `source`, for a dewpoint view without profile output
        const bool skew = lcl_done;
        double P = skew ? sP : Pc, T_ = skew ? sT : Tc;
        double Td_ = skew ? sM : Mc;
        if (fabs(P - l.p) <= LCL_SNAP * l.p) P = l.p;                       // on the LCL (see xp::lcl)
        double X = log_tab<true>(es, P);
        X = (P == l.p) ? x_lcl : X;
        const bool cross = !skew && (last || P < l.p);
        // the moist adiabat: above the LCL, and at a level exactly on it (there the state does not move: X == x_lcl)
        const bool on_lcl = need_w && !skew && !cross && (P == l.p);
        double tm = qnan();
        if (skew || on_lcl) tm = m.at(P, X, a.tb);
        double tp, tvp;
        if (!skew) {                                                       // dry adiabat
            tp = pc_t * dry_factor(es, KAPPA * (X - x0));
            tvp = need_w ? tp * vf_parcel : tp;
        } else {
            tp = tm;
            tvp = need_w ? virt(tp, mix_of_e(TABLE ? es_tab(es, tp) : m.e, P)) : tp;
        }
        if (cross) {                                                       // this lane's node is its LCL
            const double at = log_interp ? x_lcl : l.p;
            const double pb = br[SL_BR_P * SLOT_STRIDE], xb = br[SL_BR_X * SLOT_STRIDE], tb_ = br[SL_BR_T * SLOT_STRIDE], tdb = br[SL_BR_TD * SLOT_STRIDE];
            lds_wait_all();
            double cb = log_interp ? xb : pb, ca = log_interp ? X : P;
            double ta2 = T_, tda2 = Td_;
            if (pb == l.p) { ca = cb; ta2 = tb_; tda2 = tdb; }             // a level sits exactly on the LCL
            const double te = interp_rule(tb_, ta2, at, cb, ca), tde = interp_rule(tdb, tda2, at, cb, ca);
            const double lsel = br[SL_LCL_T * SLOT_STRIDE];
            P = l.p; X = x_lcl; T_ = te; Td_ = tde;
            tp = lsel; tvp = lsel;
        }
        double tve = T_;
        if (need_w) {                                                      // one wave-uniform range test for the two e_s
            if (__builtin_amdgcn_ballot_w64(!all_in_table(umax_(table_dist(T_), table_dist(Td_)))) == 0ull) tve = virt_env_tab(es, T_, Td_, P, true);
            else { double tq = T_; asm volatile("" : "+v"(tq)); tve = virt_env_tab(es, tq, Td_, P, false); }
        }
        // saturated parcel (LCL == parcel level): the reference's own operation order decides the sign at the LCL node
        const bool tie = need_w && cross && (l.p == pc_p);
        if (tie) { double q = T_; asm volatile("" : "+v"(q)); tve = virt_ref(q, Td_, l.p); }
        // a level exactly ON the LCL pairs the dry temperature with the saturation mixing ratio at the moist-adiabat temperature
        if (on_lcl) {
            double ta = tm;
            asm volatile("" : "+v"(ta));
            const double ea = es_ref(ta);
            tvp = tp * (1.0 + VT_EPS * (EPS * ea / (P - ea)));
            tve = virt_ref(T_, Td_, P);
        }
        sc.template node<false, false>(P, X, vtc ? tvp : tp, vtc ? tve : T_, cross);
        if (!isnan_(P) && !skew && !cross) { br[SL_BR_P * SLOT_STRIDE] = P; br[SL_BR_X * SLOT_STRIDE] = X; br[SL_BR_T * SLOT_STRIDE] = T_; br[SL_BR_TD * SLOT_STRIDE] = Td_; }
        lcl_done = skew || cross;
        sP = Pc; sT = Tc; sM = Mc;
    }
    const Scan::Result r = sc.finish(a.post_zero != 0);
    status |= r.status & ST_BAD_PRESSURE;
    cape = r.cape; cin = r.cin;
}

// TABLE: the reference's lookup tables instead of the RK4 stepper, a compile-time switch as k_cape_cin's MODE.
// The kernel is compiled in a translation unit of its own (xp_effective_tu.hip) with -disable-machine-licm: the LCL iteration
// sits INSIDE the candidate loop here, and left alone the compiler hoists the materialisation of the ~50 fp64 constants of
// its exp / ln polynomials (and of the level loop's) out of both loops and keeps them in registers through every ascent --
// 160-169 VGPRs, or 128 with 22-64 of them spilled when the bound is forced; 106-112 VGPRs without a spill with the flag.
template <typename T, bool TABLE> __global__ __launch_bounds__(256)
void k_effective_inflow(EffectiveArgs a) {
    struct Lds { double es[LDS_TAB]; double slot[SLOT_FIELDS * SLOT_STRIDE]; };   // the table first (see k_cape_cin)
    __shared__ Lds l;
    static_assert(SLOT_STRIDE == 256, "one Scan slot column per thread of the workgroup");
    const double *es = stage_es_table(a.es_tab, l.es);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const int nlev = (int)a.nlev;
    double *const slot = l.slot + threadIdx.x;

    double bound = qnan();                       // p0 - search_depth, once the lowest valid level is known
    int k_first = -1, base = -1, top = -1, status = 0;
    bool done = false, failed = false;           // done: nothing left to lift; failed: a candidate above the base failed
    int k = 0;
    for (; k < nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        bool lift = false;
        double p = qnan(), t = qnan(), td = qnan();
        if (!done) {
            p = ld<T>(a.p, k, c); t = ld<T>(a.t, k, c); td = ld<T>(a.td, k, c);
            if (!(isnan_(p) || isnan_(t) || isnan_(td))) {                 // an invalid level is skipped
                if (k_first < 0) { k_first = k; bound = p - a.depth; }
                lift = p >= bound;
                done = !lift;                                              // the first valid level beyond the window ends the search
            }
        }
        double cape = qnan(), cin = qnan();
        if (lift) {
            int cst;
            lift_candidate<T, TABLE>(a, es, slot, c, k, nlev, p, t, td, cape, cin, cst);
            status |= cst;
            const bool pass = cape >= a.cape_min && cin >= a.cin_min;
            if (pass) { if (base < 0) base = k; top = k; }
            else if (base >= 0) { failed = true; done = true; }
        }
        st(a.cand_cape, f64, (int64_t)k * a.ncol + c, cape);
        st(a.cand_cin, f64, (int64_t)k * a.ncol + c, cin);
    }
    if (a.cand_cape || a.cand_cin)
        for (; k < nlev; ++k) { st(a.cand_cape, f64, (int64_t)k * a.ncol + c, qnan()); st(a.cand_cin, f64, (int64_t)k * a.ncol + c, qnan()); }

    if (base < 0) status |= ST_NO_LAYER;
    else if (!failed) status |= ST_LAYER_OPEN;                             // the last candidate of the window passes
    double bp = qnan(), tpv = qnan(), bz = qnan(), tz = qnan();
    if (base >= 0) {
        bp = ld<T>(a.p, base, c); tpv = ld<T>(a.p, top, c);
        if (a.z.data) {
            const double z0 = ld<T>(a.z, k_first, c);
            bz = ld<T>(a.z, base, c) - z0; tz = ld<T>(a.z, top, c) - z0;
        }
    }
    st(a.base_p, f64, c, bp); st(a.top_p, f64, c, tpv);
    st(a.base_z, f64, c, bz); st(a.top_z, f64, c, tz);
    sti(a.base_idx, c, base); sti(a.top_idx, c, top);
    sti(a.status, c, status);
}

// defined in xp_effective_tu.hip
void launch_effective_inflow(const EffectiveArgs &a, bool f64, bool table, hipStream_t s);

}  // namespace xp
