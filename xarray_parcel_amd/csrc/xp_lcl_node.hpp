// xp_lcl_node.hpp -- what the kernels that lift a parcel share up to its LCL, once.
// The start of a column (start_column): a parcel's LCL, what it carries up to it (BelowLcl) and the initialised scan --
// for the fused several-parcels kernel and the effective inflow layer; k_cape_cin spells the same statements out (it says why).
// The node a lifted parcel feeds while it is at or below its LCL ("phase A" of the level loops):
// the pieces -- the snap onto the LCL, the bracket slots, the environment at the LCL, the environment's virtual temperature
// behind one range test, the two tie rules -- and below_lcl_node, their composition for the kernels without profile
// output (the fused several-parcels kernel, xp_multi.hpp, and the effective inflow layer, xp_effective.hpp).  k_cape_cin
// (xp_kernels.hpp) composes the same pieces itself, around its profile output.  The public contract is that the three
// agree bit for bit (tests/test_gpu_multi.py, tests/test_gpu_effective_layer.py): a rule changes here or nowhere.
// Also here: the views and stores of the kernels, the store groups of a column's scalars, the late kernel-argument
// pointer they are stored through, and the tile loop of the persistent kernels.
// How the levels are read: xp_level_reader.hpp; the profile output: xp_profile_out.hpp.
#pragma once
#include "xp_device.hpp"

namespace xp {

struct View { const void *data; int64_t ls, cs; };           // element strides
struct OutView { void *data; int64_t ls, cs; };

template <typename T> XP_DEV double ld(const View &v, int64_t k, int64_t c) {
    return (double)((const T *)v.data)[k * v.ls + c * v.cs];
}
template <typename T> XP_DEV T ldr(const View &v, int64_t k, int64_t c) { return ((const T *)v.data)[k * v.ls + c * v.cs]; }   // raw: no conversion at the load
template <typename T> XP_DEV double ld1(const void *p, int64_t c) { return (double)((const T *)p)[c]; }
XP_DEV void st(void *p, int f64, int64_t i, double v) {
    if (p == nullptr) return;
    if (f64) ((double *)p)[i] = v; else ((float *)p)[i] = (float)v;
}
XP_DEV void sti(int32_t *p, int64_t i, int v) { if (p) p[i] = v; }

struct ScalarsOut {
    void *cape, *cin, *lcl_p, *lcl_t, *lcl_tv, *lfc_p, *lfc_t, *el_p, *el_t;
    int32_t *lfc_idx, *el_idx, *status, *parcel_idx;
    void *par_p, *par_t, *par_td;
    int f64;
};

struct Parcel { double p, t, td; int64_t first; int idx; bool prepend; };

// ---- the store groups of a column's scalars --------------------------------------------------------------------------
// (S: ScalarsOut, or the same behind the kernarg pointer of a kernel that fetches its output pointers late)
template <typename S> XP_DEV void store_parcel_and_lcl(const S &s, int64_t c, const Parcel &pc, const Lcl &l) {
    st(s.lcl_p, s.f64, c, l.p); st(s.lcl_t, s.f64, c, l.t); st(s.lcl_tv, s.f64, c, l.tv);
    sti(s.parcel_idx, c, pc.idx);
    st(s.par_p, s.f64, c, pc.p); st(s.par_t, s.f64, c, pc.t); st(s.par_td, s.f64, c, pc.td);
}
// NaN parcel / LCL blanks the whole profile (pf.py:965-985): CAPE = CIN = 0.0, everything else NaN
template <typename S> XP_DEV void store_blank_column(const S &s, int64_t c, const Parcel &pc, const Lcl &l, int status) {
    st(s.cape, s.f64, c, 0.0); st(s.cin, s.f64, c, 0.0);
    st(s.lfc_p, s.f64, c, qnan()); st(s.lfc_t, s.f64, c, qnan()); st(s.el_p, s.f64, c, qnan()); st(s.el_t, s.f64, c, qnan());
    sti(s.lfc_idx, c, -1); sti(s.el_idx, c, -1); sti(s.status, c, status);
    store_parcel_and_lcl(s, c, pc, l);
}
template <typename S> XP_DEV void store_scan_result(const S &s, int64_t c, const Scan::Result &r, int status) {
    const int f64 = s.f64;
    st(s.cape, f64, c, r.cape); st(s.cin, f64, c, r.cin);
    st(s.lfc_p, f64, c, r.lfc_p); st(s.lfc_t, f64, c, r.lfc_t);
    st(s.el_p, f64, c, r.el_p); st(s.el_t, f64, c, r.el_t);
    sti(s.lfc_idx, c, r.lfc_idx); sti(s.el_idx, c, r.el_idx); sti(s.status, c, status);
}

// The output pointers are fetched from the kernel arguments only after the level loop, through a pointer the compiler
// cannot see through, so that it does not load all of them up front and carry ~26 scalar registers across the level loop
// (where they were being spilled into VGPR lanes and read back lane by lane: 840 v_readlane in the family kernel).
// Args is the kernel's only parameter, so it sits at offset 0 of the kernarg segment; taking its address instead would
// make the compiler copy the whole struct to scratch.
template <typename Args> XP_DEV const Args __attribute__((address_space(4))) *late_kernargs() {
    typedef const Args __attribute__((address_space(4))) *KernargPtr;
    KernargPtr late = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(late) : : "memory");
    return late;
}

// ---- the tile loop of the persistent kernels -------------------------------------------------------------------------
// Every workgroup owns a contiguous share of the grid's 64-column tiles and its wavefronts take them one by one from a
// counter in LDS (s_next: set to the workgroup's number of wavefronts before the staging barrier).  (One device-wide
// counter in memory was measured first: same-address atomics execute at the memory side one after the other, ~50 ns
// each -- 12 000 of them are most of c2's 0.7 ms.)
template <typename F> XP_DEV void persistent_tiles(int64_t ncol, int &s_next, const F &column) {
    const int64_t ntiles = (ncol + 63) >> 6;
    const int t0 = (int)(ntiles * blockIdx.x / gridDim.x), t1 = (int)(ntiles * (blockIdx.x + 1) / gridDim.x);
    int tile = t0 + (int)(threadIdx.x >> 6);
    while (tile < t1) {
        const int64_t c = ((int64_t)tile << 6) + (threadIdx.x & 63);
        if (c < ncol) column(c);
        if ((threadIdx.x & 63) == 0) tile = t0 + atomicAdd(&s_next, 1);
        tile = __builtin_amdgcn_readfirstlane(tile);
    }
}

// ---- the pieces of the node at or below the LCL ----------------------------------------------------------------------
XP_DEV double interp_rule(double xb, double xa, double at, double cb, double ca) {   // pf.py:1798-1806
    double res = xb + (xa - xb) * fdiv(at - cb, ca - cb);
    return (xb == xa) ? xb : res;
}

// A level within LCL_SNAP (relative) of the LCL lies ON it (see xp::lcl).  ln p bookkeeping: levels use the table logarithm,
// and a level that sits exactly on the LCL pressure takes the LCL's value (the library log), so that the interval between
// the two stays zero-width.
XP_DEV void snap_to_lcl(const double *es, double lp, double x_lcl, double &P, double &X) {
    if (fabs(P - lp) <= LCL_SNAP * lp) P = lp;
    X = log_tab<true>(es, P);
    X = (P == lp) ? x_lcl : X;
}

// The last valid-pressure level at or below the LCL, the lower bracket of the LCL interpolation: LDS slots of the scan
// (br = Scan::slot), written below the LCL only.
XP_DEV void clear_bracket(double *br) {
    br[SL_BR_P * SLOT_STRIDE] = qnan(); br[SL_BR_X * SLOT_STRIDE] = qnan(); br[SL_BR_T * SLOT_STRIDE] = qnan(); br[SL_BR_TD * SLOT_STRIDE] = qnan();
}
XP_DEV void store_bracket(double *br, double P, double X, double T_, double Td_) {
    br[SL_BR_P * SLOT_STRIDE] = P; br[SL_BR_X * SLOT_STRIDE] = X; br[SL_BR_T * SLOT_STRIDE] = T_; br[SL_BR_TD * SLOT_STRIDE] = Td_;
}
// environment at the LCL: bracketing-level interpolation in ln p or p (pf.py:897-906, 1758-1811) between the bracket slots
// and the first level above the LCL (pa, xa, ta, tda)
XP_DEV void lcl_environment(const double *br, bool log_interp, double lp, double x_lcl, double pa, double xa, double ta, double tda,
                            double &te, double &tde) {
    const double at = log_interp ? x_lcl : lp;
    const double pb = br[SL_BR_P * SLOT_STRIDE], xb = br[SL_BR_X * SLOT_STRIDE], tb_ = br[SL_BR_T * SLOT_STRIDE], tdb = br[SL_BR_TD * SLOT_STRIDE];
    lds_wait_all();
    double cb = log_interp ? xb : pb, ca = log_interp ? xa : pa;
    if (pb == lp) { ca = cb; ta = tb_; tda = tdb; }                        // a level sits exactly on the LCL
    te = interp_rule(tb_, ta, at, cb, ca); tde = interp_rule(tdb, tda, at, cb, ca);
}

// The environment's virtual temperature of a level (pf.py:839-843, 911-920): one wave-uniform range test for the two e_s
// instead of one per evaluation; the two sides are separate code (the asm barrier keeps the compiler from merging them
// into one path full of selects).  PAIR: see virt_factor_tab.
template <bool PAIR = false> XP_DEV double virt_env_ranged(const double *es, double T_, double Td_, double P) {
    if (__builtin_amdgcn_ballot_w64(!all_in_table(umax_(table_dist(T_), table_dist(Td_)))) == 0ull) return virt_env_tab<PAIR>(es, T_, Td_, P, true);
    double tq = T_;
    asm volatile("" : "+v"(tq));
    return virt_env_tab(es, tq, Td_, P, false);
}

// The two tie rules of a node (need_w: virtual temperatures are wanted; cross: the node is the LCL node; P, T_, Td_: the
// node's environment; tp: the parcel's temperature there; moist_t(): the moist-adiabat temperature at this node, asked
// for in the second case only).
//  - A saturated parcel (`sat`: LCL == parcel level): the sign of parcel-minus-environment at the LCL node is rounding
//    noise of exactly the reference's expressions, so those columns evaluate them in its operation order.
//  - A level exactly ON the LCL pairs the dry temperature with the saturation mixing ratio at the moist-adiabat
//    temperature (pf.py:773 uses <=).  For a saturated parcel this is the parcel's own level and the same holds.
// The rare branches here and in below_lcl_node are plain divergent branches (saveexec + execz), behind ONE early return
// on !need_w, on which the compiler unswitches the callers' node.  Measured, same box, medians of alternated runs, against
// the kernels before the node was shared: this form -- the effective-inflow kernel 18.66 against 19.19-19.23 ms (64 x 1 Mi
// f64), the fused step of the c5 share 28.36-28.45 against 28.18-28.31 ms, the fused kernels' VGPRs as before (169 / 178);
// need_w tested in each rule instead -- fused 27.96 ms but 170 / 179 VGPRs, inflow 19.16 against 18.94-18.98; the rules
// behind ballots (the fused kernel's earlier form) -- fused 28.61-28.74 ms.
template <typename F> XP_DEV void lcl_ties(bool need_w, bool cross, bool sat, double P, double lp, double tp, double T_, double Td_,
                                           F moist_t, double &tvp, double &tve) {
    if (!need_w) return;
    if (cross && sat) { double q = T_; asm volatile("" : "+v"(q)); tve = virt_ref(q, Td_, lp); }
    if (!cross && (P == lp)) {
        double ta = moist_t();
        asm volatile("" : "+v"(ta));
        const double ea = es_ref(ta);
        tvp = tp * (1.0 + VT_EPS * (EPS * ea / (P - ea)));
        tve = virt_ref(T_, Td_, P);
    }
}

// ---- the node, for the kernels without profile output ----------------------------------------------------------------
// What a parcel carries up to its LCL: the LCL (pressure, its library logarithm), the dry adiabat (parcel temperature,
// ln of its pressure, 1 + 0.608 x its mixing ratio: pf.py:748), and whether the LCL lies on the parcel's own level.
struct BelowLcl { double lp, x_lcl, t0, x0, vfac; bool sat; };

// The start of a column: the parcel's LCL, what it carries up to it, and the scan -- initialised, with the LCL temperature
// the correction switch picks in its SL_LCL_T slot (pf.py:1442 / 1461) and the bracket slots cleared.  status takes
// ST_LCL_NOT_CONVERGED.  Returns false for a NaN parcel / LCL, which blanks the whole profile (pf.py:965-985): the scan
// is not touched then, `n` carries no adiabat, and the caller stores its blank column.
// need_w: somebody wants virtual temperatures (the correction switch, or profile output).  FLAT: see xp::lcl.
// ln p bookkeeping.  Levels use the table logarithm; the LCL node uses the library log (its crossing tests
// "p* < p_lcl" then break ties as on the CPU); a level that sits exactly on the LCL pressure takes the LCL's
// value so that the interval between the two stays zero-width; and the parcel's own ln p (x0) is whatever its
// level gets, so that the surface parcel reproduces its level bit for bit (T0 * exp(0)) -- the reference's lfc_el
// branches on that exact equality (pf.py:1117-1120).
template <bool FLAT = false>
XP_DEV bool start_column(const double *es, const Parcel &pc, bool need_w, bool vtc, bool pos_neg, double *slot,
                         Lcl &l, BelowLcl &n, Scan &sc, int &status) {
    l = lcl<FLAT>(pc.p, pc.t, pc.td);
    status = l.not_converged ? ST_LCL_NOT_CONVERGED : 0;
    n.lp = l.p; n.x_lcl = qnan(); n.t0 = pc.t; n.x0 = qnan(); n.vfac = 1.0; n.sat = false;
    if (isnan_(l.p)) return false;
    n.vfac = need_w ? virt_factor_tab(es, pc.t, pc.td, pc.p, false) : 1.0;     // 1 + 0.608 w of the parcel (pf.py:748, 767)
    n.x_lcl = log(l.p);
    n.sat = (l.p == pc.p);
    n.x0 = n.sat ? n.x_lcl : log_tab<true>(es, pc.p);
    sc.init(l.p, n.x_lcl, pos_neg, slot);
    slot[SL_LCL_T * SLOT_STRIDE] = vtc ? l.tv : l.t;
    clear_bracket(slot);
    return true;
}

// One node of a lane at / below / just above its LCL.  Every lane feeds exactly ONE node per call (k_cape_cin's `source`
// says why): with `skew` unset (P, T_, Td_) is the level just loaded -- fed on the dry adiabat, or, when it lies above the
// LCL (or nothing is left: `last`), the LCL node is fed in its place and the level has to wait; with `skew` set the lane
// is past its LCL and (P, T_, Td_) is the level that has been waiting.  Returns whether the LCL node has been fed.
// adiabat(above, P, X, tp, tvp): the moist adiabat, the one thing the callers differ in -- above the LCL (above = true)
// the parcel's temperature and virtual temperature at the node; for a node ON the LCL (above = false) tp = the
// moist-adiabat temperature there, nothing else.
// status: takes ST_NAN_PRESSURE for a NaN pressure below the LCL (see xparcel.h).
// obs: an observer of the scan's crossings (Scan::special), for the positive-layer kernel; nobody by default.
template <typename A, typename OBS = void>
XP_DEV bool below_lcl_node(const double *es, Scan &sc, const BelowLcl &n, bool vtc, bool log_interp,
                           double P, double T_, double Td_, bool skew, bool last, int &status, A adiabat, OBS *obs = nullptr) {
    const bool need_w = vtc;
    double X;
    snap_to_lcl(es, n.lp, n.x_lcl, P, X);
    const bool cross = !skew && (last || P < n.lp);
    if (isnan_(P) && !skew && !last) status |= ST_NAN_PRESSURE;
    // only the parcel temperature / mixing ratio is branched, the environment and the scan node are shared
    double tp, tvp;
    if (!skew) {                                                           // dry adiabat (pf.py:313, 767)
        tp = n.t0 * dry_factor(es, KAPPA * (X - n.x0));
        tvp = need_w ? tp * n.vfac : tp;
    } else adiabat(true, P, X, tp, tvp);
    if (cross) {                                                           // this lane's node is its LCL
        double te, tde;
        lcl_environment(sc.slot, log_interp, n.lp, n.x_lcl, P, X, T_, Td_, te, tde);
        // the scan only sees the temperature picked by the correction switch, which sits in the SL_LCL_T slot: neither LCL
        // temperature has to stay in registers through the loop
        const double lsel = sc.slot[SL_LCL_T * SLOT_STRIDE];
        P = n.lp; X = n.x_lcl; T_ = te; Td_ = tde;
        tp = lsel; tvp = lsel;
    }
    double tve = need_w ? virt_env_ranged(es, T_, Td_, P) : T_;
    lcl_ties(need_w, cross, n.sat, P, n.lp, tp, T_, Td_, [&]() __attribute__((always_inline)) { double t, tv; adiabat(false, P, X, t, tv); return t; }, tvp, tve);
    sc.template node<false, false, OBS>(P, X, vtc ? tvp : tp, vtc ? tve : T_, cross, obs);
    if (!isnan_(P) && !skew && !cross) store_bracket(sc.slot, P, X, T_, Td_);
    return skew || cross;
}

}  // namespace xp
