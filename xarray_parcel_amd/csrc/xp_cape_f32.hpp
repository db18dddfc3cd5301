// xp_cape_f32.hpp -- xp_opts.compute == XP_F32: surface-parcel CAPE / CIN of float32 grids with the level walk above the
// LCL in fp32 arithmetic (the contract: include/xparcel.h at xp_opts.compute; the dispatch: xp_cape_cin in xparcel.hip).
//
// What stays fp64, and is the fp64 family kernel's own code (k_cape_cin<float, PM_SURFACE, false, 2, false, true, true>):
//   - the column prologue: the parcel, xp::lcl, the label of the adiabat (Family::start), the stores of the LCL and parcel
//     outputs -- once per column; the LCL / parcel outputs are bit-identical to the fp64 path's;
//   - every node at or below the LCL ("phase A" of k_cape_cin: the dry adiabat, the LCL node, the snap and the two tie
//     rules of xp_lcl_node.hpp), through the same functions in the same order.  Node 0 of a surface parcel therefore has
//     parcel == environment bit for bit, as there (pf.py:1117-1120);
//   - the scan (xp::Scan): the sign tests, the crossings, the LFC / EL choice and the two running sums (two fp64 adds per
//     level) see one number per node, y = parcel minus environment virtual temperature, and its ln p.
// What is fp32: above the LCL a node's ln p (v_log_f32), the environment's Tv - T (Bolton's e_s twice through v_exp_f32 and
// v_rcp_f32), the parcel's virtual temperature (Horner on nine fp32 coefficients, collapsed in fp32 from an fp32 copy of the
// family table in LDS: 23 KB instead of 46.7 KB) and y itself.  The e_s / ln tables stay in LDS for the fp64 parts.
//
// XP_F32_GUARD: a bound on |y_fp32 - y_fp64| at a node above the LCL, with y_fp64 what the fp64 kernel feeds its scan
// (itself within 1e-12 K of exact arithmetic on the same formulas, so it stands for the exact value).  Operations and
// their errors (u = 2^-24 = 6e-8; v_log_f32, v_exp_f32 and v_rcp_f32 are accurate to 1 ulp; inputs are float32, so the
// conversions are exact).  THE DOMAIN of the bound: 1 hPa <= p <= 1100 hPa, 150 K <= Td <= T <= 330 K, e_s(T) <= 0.1 p,
// T c w <= 8 K with c w = 0.608 w, i.e. a mixing ratio up to 0.04 -- any sounding of the troposphere and the stratosphere up
// to 1 hPa.  Outside it (a level warmer than 253 K at 12 hPa, say) the environment's quotient loses its digits in both
// arithmetics and nothing is promised.  Inside the family table (p >= 20.1 hPa):
//   X = ln2f * log2(p)             log2 p < 16: 1 ulp = 9.5e-7, x ln 2 = 6.6e-7; the product's rounding (X < 8) 2.4e-7; the
//                                   constant's own error 2.4e-8 * 7 = 1.7e-7                            |dX| <= 1.07e-6
//   z = fma(4, X, m4)              4 |dX| + the rounding of m4 (|m4| < 32: 9.5e-7) + its own (|z| <= 1: 6e-8)   |dz| <= 5.3e-6
//   parcel, through z              |dTv/dz| = |dTv/dln p| / 4 <= 25 K: a moist adiabat is never steeper in ln p than the dry
//                                   one, kappa T (1 + c w) < 95 K, plus c T dw_s/dln p < 6 K                       1.33e-4 K
//   Horner in z                    nine steps; the last rounds a value < 512 (1.53e-5), the one before a value < 32
//                                   (|c1| = |dTv/dz|: 9.5e-7), the seven before values < 8 (2.4e-7 each)            1.8e-5 K
//   the coefficients c_n(s)        each a Horner sum in s over nine rounded table entries: c_0 (< 512) 2 * 1.53e-5 from its
//                                   leading entry and last step + 3.4e-5 from the eight others (< 64 each); c_1 (< 32)
//                                   4e-6; c_2 ... c_8 (< 8) 1e-6 each; the label s itself, 6e-8 * |dTv/ds| (< 40 K)  7.8e-5 K
//   environment Tv - T = T c e_s(Td) / (p - e_s(T)), c = 0.608 * 0.62196:
//     a = 17.67 - 4302.645 rcp(t - 29.65)   the difference, the reciprocal and the product 4 u relative on a term <= 36,
//                                   the sum's rounding 2.4e-7                                               |da| <= 9e-6
//     e_s = 6.112 exp2(a log2e)    |a log2e| < 32: the product rounds by 9.5e-7, x ln 2; exp2 and the factor 2 u
//                                   relative                                                        |de/e| <= 9.8e-6
//     the quotient                 e_s(Td): 9.8e-6; p - e_s(T) with e_s(T) <= 0.1 p: 1e-6; the reciprocal and the three
//                                   products 5 u                                                              1.12e-5
//     times T c w <= 8 K                                                                                           9e-5 K
//   y = (Tv_parcel - T) - (Tv_env - T)   the first difference is exact (two floats within a factor two), the second rounds
//                                   by |y| u: nothing where |y| < GUARD
//   sum                                                                                                          3.2e-4 K
// Above the table's top (1 hPa <= p < 20.1 hPa) the parcel continues dry, Tv = v(-1) exp2(kappa log2e (X - X_lo)), X_lo = ln 20.1:
//   v(-1)                          Horner at z = -1 exactly (no ln p in it): its rounding and the coefficients', as above   9.6e-5 K
//   X                              log2 p < 4.4: 4.8e-7 x ln 2 = 3.3e-7, the product (X < 4) 1.2e-7, the constant 7e-8      |dX| <= 5.3e-7
//   the exponent                   X - X_lo with X_lo rounded (1.2e-7) and the difference's rounding (1.2e-7), times kappa log2e
//                                   = 0.412 with the constant's 6e-8 on an exponent <= 1.25: 4.7e-7 in the exponent, x ln 2 = 3.3e-7
//                                   relative; exp2 and the product 2 u                                            5.1e-7 relative
//   times v(-1) < 260 K                                                                                            1.33e-4 K
//   environment                    as above with T c w < 0.1 K there                                                  1e-6 K
//   sum                                                                                                          2.3e-4 K
// XP_F32_GUARD = 4e-4 K.  A node with |y_fp32| >= GUARD has the sign of y_fp64; any other node whose inputs are all there --
// and, whatever its y, the first node above an LCL node whose own y is next to nothing (XP_F32_TIE: the fp64 kernel's tie
// window) and any node within 8e-6 (relative) of the LCL pressure, where ln p itself has to be on the right side of
// ln p_lcl -- is evaluated again by the fp64 kernel's own functions (log_tab,
// virt_env_tab, the fp64 family polynomial read from the table in global memory), behind a ballot.  Every decision of the
// scan is then taken on the fp64 kernel's number, so the two classify every column (of the domain) alike; values differ by what the
// undoubted nodes carry: at most GUARD in y at a node (CAPE / CIN: Rd * GUARD * ln(p_lcl / p_top) < 0.35 J/kg if every
// node erred one way by the whole bound; measured: tests/test_gpu_compute32.py) and 1.07e-6 in a node's ln p.
// Nodes at or below the LCL that lie above some other lane's LCL in phase A take the fp32 parcel against the fp64
// environment and ln p, under the same rule (their error is the parcel's share of the sum).
// NOT INVARIANT under a permutation of the columns, unlike the fp64 path: which of a column's nodes are fed in phase A (fp64
// ln p and environment) and at which level its coefficients are collapsed again (Family32::at reloads the whole wavefront,
// which replaces the first set -- the label solve's fp64 collapse, rounded -- by the fp32 collapse) depend on the other 63
// columns of its wavefront.  The classification does not; CAPE, CIN and the crossing pressures move within the bounds above.
#pragma once
#include "xp_kernels.hpp"

namespace xp {

constexpr float XP_F32_GUARD = 4e-4f;
constexpr double XP_F32_NEAR_LCL = 8e-6;     // relative distance in pressure inside which a node's ln p is the fp64 one
// The first node above the LCL is taken in fp64 whatever its y when the LCL node's own y is this small against it: the
// crossing between the two then lies within 1e-5 of the interval (3e-7 in ln p for an interval of 0.03) from the LCL, two
// orders outside the fp64 kernel's 2e-9 tie window, inside which "p* < p_lcl" is decided on the last bits of both y.
constexpr double XP_F32_TIE = 1e-5;

constexpr float F32_LN2 = 0.6931471805599453f, F32_LOG2E = 1.4426950408889634f;

// Bolton's e_s on the hardware's exp2 and reciprocal (see the derivation above)
XP_DEV float es_f32(float t) {
    const float a = __builtin_fmaf(-4302.645f, __builtin_amdgcn_rcpf(t - 29.65f), 17.67f);
    return 6.112f * __builtin_amdgcn_exp2f(a * F32_LOG2E);
}

// The parcel's virtual temperature along its moist adiabat in fp32: Family's scheme (xp_device.hpp) with nine fp32
// coefficients per column, collapsed in fp32 from the fp32 copy of the table in LDS.  A wavefront whose lanes cross a
// piece boundary reloads together (Family::at's rule).  The label (q, s) comes from Family::start, in fp64.
struct Family32 {
    const float *tab;      // LDS: the coefficient table in the device layout, rounded to fp32
    float c[FAM_ND + 1];
    float m4, s;
    int q;
    bool bad;

    XP_DEV void load_piece(int j) {
        const float *a = tab + (j * FAM_SJ + q);
#pragma unroll
        for (int n = 0; n <= FAM_ND; ++n) {
            const float *r = a + n * FAM_SN;
            float k[FAM_MD + 1];
#pragma unroll
            for (int m = 0; m <= FAM_MD; ++m) k[m] = r[m * FAM_SM];
            float v = k[FAM_MD];
#pragma unroll
            for (int m = FAM_MD - 1; m >= 0; --m) v = __builtin_fmaf(v, s, k[m]);
            c[n] = v;
        }
        m4 = (float)(-(2.0 / FAM_WX) * Family::x_mid(j));
    }
    XP_DEV void poison() {
#pragma unroll
        for (int n = 0; n <= FAM_ND; ++n) c[n] = __builtin_nanf("");
        m4 = __builtin_nanf("");
    }
    XP_DEV float horner(float z) const {
        float v = c[FAM_ND];
#pragma unroll
        for (int n = FAM_ND - 1; n >= 0; --n) v = __builtin_fmaf(v, z, c[n]);
        return v;
    }
    XP_DEV float at(float X) {
        float z = __builtin_fmaf((float)(2.0 / FAM_WX), X, m4);
        const bool move = (z <= -1.0f) || (z > 1.0f);                       // a NaN z (NaN pressure, poisoned lane) stays put
        if (__builtin_amdgcn_ballot_w64(move) != 0ull) {                    // rare: another x-piece, or off the table
            const float u = __builtin_fmaf(-(float)(1.0 / FAM_WX), X, (float)(FAM_XHI * (1.0 / FAM_WX)));
            bool go = move;
            if (go && u < 0.0f) { bad = true; go = false; }                  // p > 1100 hPa
            const int jn = (int)u;
            const bool top = go && jn > FAM_NPX - 1;                        // above the table top: dry continuation
            const int jcur = (int)__builtin_rintf(__builtin_fmaf(m4, 0.5f, (float)(FAM_XHI * (1.0 / FAM_WX) - 0.5)));
            const int j = go ? (jn > FAM_NPX - 1 ? FAM_NPX - 1 : jn) : jcur;
            load_piece(bad ? 0 : j);
            if (bad) poison();
            z = __builtin_fmaf((float)(2.0 / FAM_WX), X, m4);
            if (__builtin_amdgcn_ballot_w64(top) != 0ull) {
                const float v = horner(top ? -1.0f : z);
                return top ? v * __builtin_amdgcn_exp2f(((float)KAPPA * F32_LOG2E) * (X - (float)FAM_XLO)) : v;
            }
        }
        return horner(z);
    }
};

// The fp64 kernel's parcel virtual temperature at ln p = X for the label (q, s): Family::at's value bit for bit -- the piece
// that holds X (the oracle's floor rule), its nine coefficients collapsed as Family::load_piece_into collapses them, Horner
// in z = 4 X + m4, the dry continuation above the table top -- with the coefficients read from the fp64 table in global
// memory and consumed row by row, so that the rare branch that calls this holds nine doubles at a time.
XP_DEV double family_tv64(const double *tab, int q, double s, double X) {
    const double u = __builtin_fma(-(1.0 / FAM_WX), X, FAM_XHI * (1.0 / FAM_WX));
    if (!(u >= 0.0)) return qnan();                                         // NaN pressure (p > 1100 hPa cannot occur above an LCL inside the table)
    const int jn = (int)u;
    const bool top = jn > FAM_NPX - 1;
    const int j = top ? FAM_NPX - 1 : jn;
    const double m4 = -(2.0 / FAM_WX) * Family::x_mid(j);
    const double z = top ? -1.0 : __builtin_fma(2.0 / FAM_WX, X, m4);
    const double *a = tab + (j * FAM_SJ + q);
    double v = 0.0;
#pragma unroll
    for (int n = FAM_ND; n >= 0; --n) {
        const double *r = a + n * FAM_SN;
        double k[FAM_MD + 1];
#pragma unroll
        for (int m = 0; m <= FAM_MD; ++m) k[m] = r[m * FAM_SM];
        double cn = k[FAM_MD];
#pragma unroll
        for (int m = FAM_MD - 1; m >= 0; --m) cn = __builtin_fma(cn, s, k[m]);
        asm volatile("" : "+v"(cn) : : "memory");
        v = (n == FAM_ND) ? cn : __builtin_fma(v, z, cn);
    }
    return top ? v * fexp(KAPPA * (X - FAM_XLO)) : v;
}

// One column per lane, level-major coalesced row reads (k_cape_cin's layout); T is float (the kernel is a template so that
// it is compiled in its own translation unit, xp_cape_f32_tu.hip).  PERSIST: k_cape_cin's persistent wavefronts -- one
// workgroup per CU stages the tables once and its wavefronts take 64-column tiles until the grid is done -- on the grids
// the fp64 family kernel runs that way (persist(), xparcel.hip).
template <typename T, bool PERSIST>
__global__ __launch_bounds__(XP_CAPE_THREADS) void k_cape_f32(CapeArgs a) {
    struct Lds { double es[LDS_TAB]; double slot[SLOT_FIELDS * SLOT_STRIDE]; float fam[FAM_COEFS]; int next; };
    __shared__ Lds lds;
    for (int i = threadIdx.x; i < FAM_COEFS; i += blockDim.x) lds.fam[i] = (float)a.fam_tab[i];
    if (PERSIST && threadIdx.x == 0) lds.next = (int)(blockDim.x >> 6);
    const double *es = stage_es_table(a.es_tab, lds.es);
    const int64_t c0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!PERSIST && c0 >= a.ncol) return;

    auto column = [&](const int64_t c) __attribute__((always_inline)) {
    const Parcel pc = choose_parcel<T, false>(a, PM_SURFACE, c, es, a.depth);
    const Lcl l = lcl<true>(pc.p, pc.t, pc.td);
    if (isnan_(l.p)) {
        store_blank_column(a.s, c, pc, l, 0);
        a.flags[c] = 0;
        return;
    }
    store_parcel_and_lcl(a.s, c, pc, l);
    const double vf_parcel = virt_factor_tab(es, pc.t, pc.td, pc.p, false);
    const double x_lcl = log(l.p);
    const double x0 = (pc.p == l.p) ? x_lcl : log_tab<true>(es, pc.p);

    Scan sc; sc.init(l.p, x_lcl, true, lds.slot + threadIdx.x);
    sc.slot[SL_LCL_T * SLOT_STRIDE] = l.tv;
    double *const br = sc.slot;
    clear_bracket(br);

    // the label in fp64; its collapse of the LCL's x-piece, rounded, is the first set of fp32 coefficients
    Family32 f;
    double s64;
    {
        Family f64;
        f64.start(a.fam_tab, es, l.p, x_lcl, l.t, l.tv);
        f.tab = lds.fam; f.q = f64.q; f.bad = f64.bad; s64 = f64.s; f.s = (float)f64.s; f.m4 = (float)f64.m4;
#pragma unroll
        for (int n = 0; n <= FAM_ND; ++n) f.c[n] = (float)f64.c[n];
    }
    const int q = f.q;
    float p_near = (float)(l.p * (1.0 - XP_F32_NEAR_LCL));
    asm volatile("" : "+v"(p_near));                                        // (formed once: not again at every level)
    bool first_moist = true;                                                // the next node above the LCL is this lane's first

    // ---- phase A: some lane of the wavefront is at or below its LCL (k_cape_cin's `source`, LEAN, default options) ----
    bool lcl_done = false;
    double sP = qnan(), sT = qnan(), sM = qnan();
    auto source = [&](double Pc, double Tc, double Mc, bool last) __attribute__((always_inline)) {
        const bool skew = lcl_done;
        double P = skew ? sP : Pc, T_ = skew ? sT : Tc, Td_ = skew ? sM : Mc;
        double X;
        snap_to_lcl(es, l.p, x_lcl, P, X);
        const bool cross = !skew && (last || P < l.p);
        double tp, tvp;
        if (!skew) {                                                        // dry adiabat (pf.py:313, 767)
            tp = pc.t * dry_factor(es, KAPPA * (X - x0));
            tvp = tp * vf_parcel;
        } else {
            tvp = (double)f.at((float)X);
            tp = tvp;
        }
        if (cross) {                                                        // this lane's node is its LCL
            double te, tde;
            lcl_environment(br, true, l.p, x_lcl, P, X, T_, Td_, te, tde);
            const double lsel = br[SL_LCL_T * SLOT_STRIDE];
            P = l.p; X = x_lcl; T_ = te; Td_ = tde;
            tp = lsel; tvp = lsel;
        }
        double tve = virt_env_ranged<true>(es, T_, Td_, P);
        lcl_ties(true, cross, l.p == pc.p, P, l.p, tp, T_, Td_, [&]() __attribute__((always_inline)) { return l.t; }, tvp, tve);
        if (skew) {
            const bool there = !isnan_(P + T_ + Td_) && !f.bad;
            const double ye = tvp - tve;
            const bool doubt = there && ((first_moist && !(fabs(sc.yp) > XP_F32_TIE * fabs(ye))) || !(fabs(ye) >= (double)XP_F32_GUARD));
            if (__builtin_amdgcn_ballot_w64(doubt) != 0ull && doubt) tvp = family_tv64(a.fam_tab, q, s64, X);
            first_moist = false;
        }
        sc.template node<true, false>(P, X, tvp, tve, cross);
        if (!isnan_(P) && !skew && !cross) store_bracket(br, P, X, T_, Td_);
        lcl_done = skew || cross;
        sP = Pc; sT = Tc; sM = Mc;
    };

    LevelReader<T> rd(a.p, a.t, a.td, c);
    const int nlev = (int)a.nlev;
    int k = 0;
    rd.start(k, nlev);
    for (; k <= nlev; ++k) {
        if (__ballot(!lcl_done) == 0ull) break;                             // wave-uniform: everybody is above its LCL
        double P, T_, M_;
        rd.take(k + 1 < nlev, P, T_, M_);
        source(P, T_, M_, k >= nlev);
    }

    // ---- phase B: every lane is above its LCL and one level behind the loads: the waiting level is fed in fp32 ----
    float wP = (float)sP, wT = (float)sT, wM = (float)sM;                   // (levels: exact in float)
    for (; k <= nlev; ++k) {
        rd.wait();
        const float nP = rd.np_, nT = rd.nt_, nM = rd.ntd_;
        if (k + 1 < nlev) rd.request();
        else rd.refill_nan();
        const float P = wP, T_ = wT, Td_ = wM;
        const float X = F32_LN2 * __builtin_amdgcn_logf(P);
        const float e_td = es_f32(Td_), e_t = es_f32(T_);
        const float dtv_env = T_ * (((float)(VT_EPS * EPS) * e_td) * __builtin_amdgcn_rcpf(P - e_t));
        const float tvp = f.at(X);
        const float y = (tvp - T_) - dtv_env;
        const bool there = !(P + T_ + Td_ != P + T_ + Td_) && !f.bad;
        const bool doubt = there && ((first_moist && !(fabs(sc.yp) > XP_F32_TIE * (double)__builtin_fabsf(y))) || P > p_near ||
                                     !(__builtin_fabsf(y) >= XP_F32_GUARD));
        first_moist = false;
        double X2 = (double)X, par = (double)y, env = 0.0;
        if (__builtin_amdgcn_ballot_w64(doubt) != 0ull && doubt) {          // the fp64 kernel's own node
            const double Pd = (double)P, Td = (double)T_, Tdd = (double)Td_;
            X2 = log_tab<true>(es, Pd);
            par = family_tv64(a.fam_tab, q, s64, X2);
            env = virt_env_tab(es, Td, Tdd, Pd, false);
        }
        sc.template node<true, true>((double)P, X2, par, env, false);
        wP = nP; wT = nT; wM = nM;
    }

    // the lowest valid pressure of the profile (stands in for a missing EL, pf.py:1329): the smaller of the LCL pressure
    // and the last level with a valid pressure, found by looking down from the top (k_cape_cin's rule for LEAN)
    double pm = l.p;
    bool found = false;
    for (int kk = nlev - 1; kk >= 0; --kk) {
        if (__ballot(!found) == 0ull) break;
        const double qv = ld<T>(a.p, kk, c);
        if (!found && !isnan_(qv)) { pm = (qv < pm) ? qv : pm; found = true; }
    }
    sc.slot[SL_MIN_P * SLOT_STRIDE] = pm;

    const auto late = late_kernargs<CapeArgs>();
    Scan::Result r = sc.finish(false);
    late->flags[c] = f.bad ? 1 : 0;
    store_scan_result(late->s, c, r, r.status);
    };   // column

    if (PERSIST) persistent_tiles(a.ncol, lds.next, column);
    else column(c0);
}

// host-side launcher, defined in xp_cape_f32_tu.hip
void launch_cape_f32(const CapeArgs &a, hipStream_t s);

}  // namespace xp
