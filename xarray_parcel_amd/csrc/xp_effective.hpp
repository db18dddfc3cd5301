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
// LCL node instead (the level waits), above it the level that has been waiting: xp::below_lcl_node (xp_lcl_node.hpp), the
// node k_cape_cin and the fused kernel feed there, tie rules included, with the RK4 / table moist adiabat.
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
    cape = 0.0; cin = 0.0;
    Parcel pc; pc.p = pc_p; pc.t = pc_t; pc.td = pc_td;
    Lcl l; BelowLcl n; Scan sc;
    if (!start_column<true>(es, pc, need_w, vtc, pos_neg, slot, l, n, sc, status)) return;   // a NaN LCL blanks the profile: CAPE = CIN = 0.0
    Moist m;
    m.start(es, l.p, n.x_lcl, l.t, TABLE, a.tb);
    // The moist adiabat by the RK4 stepper or the reference's tables.  A level exactly on the LCL comes before the stepper
    // has moved, and Moist::at at its own start point returns the start temperature, l.t, as it stands: taken directly (the
    // stepper inlined a second time cost the RK4 kernels 2-4 VGPRs and 450 instructions); the tables are interpolated there.
    auto adiabat = [&](bool above, double P, double X, double &tp, double &tvp) __attribute__((always_inline)) {
        if (!TABLE && !above) { tp = l.t; return; }
        tp = m.at(P, X, a.tb);
        tvp = need_w ? virt(tp, mix_of_e(TABLE ? es_tab(es, tp) : m.e, P)) : tp;
    };

    bool lcl_done = false;
    int unreported = 0;                                                    // (a NaN pressure below the LCL is not reported here)
    double sP = qnan(), sT = qnan(), sM = qnan();                          // the level that waits while the LCL node is fed
    LookAhead<T> next(a.p, a.t, a.td, c, k0);
    for (int k = k0; k <= nlev; ++k) {
        const bool last = k >= nlev;
        double Pc, Tc, Mc;
        next.take(k + 1, nlev, Pc, Tc, Mc);
        if (last) Pc = Tc = Mc = qnan();
        const bool skew = lcl_done;
        lcl_done = below_lcl_node(es, sc, n, vtc, log_interp, skew ? sP : Pc, skew ? sT : Tc, skew ? sM : Mc, skew, last, unreported, adiabat);
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
