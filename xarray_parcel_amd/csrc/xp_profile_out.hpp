// xp_profile_out.hpp -- the profile output of k_cape_cin (xp_kernels.hpp): the six arrays of a lifted profile, row by row,
// and the lifted index taken from the same nodes.  ProfileSink is what the kernel's `emit` hands every node to when the
// caller wants any of it; the scan (xp::Scan) does not know about it.
#pragma once
#include "xp_lcl_node.hpp"

namespace xp {

struct ProfileOut {
    void *v[6];            // p, t_parcel, tv_parcel, t_env, tv_env, td_env (each may be null)
    int64_t nlev_out, ls, cs;
    int f64;
    int native6;           // all six arrays wanted, in the dtype of the input views: the row is stored without per-array tests
    void *li;              // lifted index (pf.py:1722): environment minus parcel temperature of this profile at exp(li_x) hPa
    double li_x;           // ln of that pressure
};

// T: the dtype of the input views (the native6 rows).  LAZY: the lifted index and none of the rows (k_cape_cin says when).
template <typename T, bool LAZY> struct ProfileSink {
    int jout = 0;                                                           // profile row
    double li_d = qnan();                                                   // environment minus parcel temperature of the node before this one (lifted index)
    // LAZY: the node before this one as it came -- its parcel temperature where the node had one (dry adiabat, LCL), else
    // its virtual temperature, to be inverted if the next node turns out to close the bracket
    double lz_te = qnan(), lz_tq = qnan(), lz_p = qnan();
    int lz_known = 1;
    bool li_done = false;

    // NaN parcel / LCL blanks the whole profile (pf.py:965-985)
    static XP_DEV void blank(const ProfileOut &o, int64_t c) {
        for (int64_t j = 0; j < o.nlev_out; ++j)
            for (int v = 0; v < 6; ++v) st(o.v[v], o.f64, j * o.ls + c * o.cs, qnan());
        st(o.li, o.f64, c, qnan());
    }

    // one row of the six arrays
    XP_DEV void row(const ProfileOut &o, int64_t c, double P, double tp, double tvp, double te, double tve, double tde) const {
        if (!LAZY && jout < o.nlev_out) {
            int64_t i = jout * o.ls + c * o.cs;
            bool dead = isnan_(P);                                         // NaN-coordinate rows come out all-NaN (pf.py:963, 988)
#ifndef XP_NO_NATIVE6
            if (o.native6) {
                // the common request (the drivers, BASELINE config 3): six stores of the input dtype, no null / dtype
                // test per array (each was two scalar branches plus, at this register pressure, two v_readlane), the
                // NaN-row select done on the converted value
                const T vP = (T)P;
                ((T *)o.v[0])[i] = vP;
                ((T *)o.v[1])[i] = dead ? vP : (T)tp;
                ((T *)o.v[2])[i] = dead ? vP : (T)tvp;
                ((T *)o.v[3])[i] = dead ? vP : (T)te;
                ((T *)o.v[4])[i] = dead ? vP : (T)tve;
                ((T *)o.v[5])[i] = dead ? vP : (T)tde;
            } else
#endif
            {
            st(o.v[0], o.f64, i, P);
            st(o.v[1], o.f64, i, dead ? P : tp);
            st(o.v[2], o.f64, i, dead ? P : tvp);
            st(o.v[3], o.f64, i, dead ? P : te);
            st(o.v[4], o.f64, i, dead ? P : tve);
            st(o.v[5], o.f64, i, dead ? P : tde);
            }
        }
    }

    // lifted_index (pf.py:1722 = log_interp of the profile's two temperatures at one pressure, pf.py:1813): the
    // nodes come with decreasing pressure, so the first one at or above the level closes the bracket that the
    // node before it opened (coords_before / coords_after of pf.py:1774-1775; a NaN-pressure row is no
    // coordinate; value rule of pf.py:1802-1806)
    // -- both temperatures take the same weight, so their difference is interpolated: one value of state.
    // The state lives in an LDS slot where the workgroup has one to spare (not the 1024-thread family build).
    // sc: the scan BEFORE it has seen this node (sc.Xp is the node before).
    XP_DEV void lifted_index(const ProfileOut &o, int64_t c, const double *es, const Scan &sc, double P, double X, double tp, double tvp, double te) {
        if constexpr (LAZY) {
            // (a node without a parcel temperature of its own hands in NaN for it; a NaN parcel inverts to NaN)
            const bool known = !isnan_(tp);
            if (!li_done && X <= o.li_x + 1e-12) {
                const bool on = X >= o.li_x - 1e-12;
                double off0 = 0.0, off1 = 0.0;
                const double tc = known ? tp : Family::temperature_from(es, P, tvp, off0);
                const double tb4 = lz_known ? lz_tq : Family::temperature_from(es, lz_p, lz_tq, off1);
                const double d_ = te - tc, dp = lz_te - tb4;
                const double wgt = (o.li_x - sc.Xp) / (X - sc.Xp);
                st(o.li, o.f64, c, (on || dp == d_) ? d_ : dp + (d_ - dp) * wgt);
                li_done = true;
            }
            if (!isnan_(P)) { lz_te = te; lz_tq = known ? tp : tvp; lz_p = P; lz_known = known ? 1 : 0; }
        } else if (o.li) {
            constexpr bool LI_SLOT = SLOT_FIELDS > SL_LI;
            const double d_ = te - tp;
            if (!li_done && X <= o.li_x + 1e-12) {
                // a node ON the level (the table logarithm and the host's differ in the last bits) is its own bracket
                const bool on = X >= o.li_x - 1e-12;
                const double dp = LI_SLOT ? sc.slot[(LI_SLOT ? SL_LI : 0) * SLOT_STRIDE] : li_d;
                const double wgt = (o.li_x - sc.Xp) / (X - sc.Xp);
                st(o.li, o.f64, c, (on || dp == d_) ? d_ : dp + (d_ - dp) * wgt);
                li_done = true;
            }
            if (!isnan_(P)) { if (LI_SLOT) sc.slot[(LI_SLOT ? SL_LI : 0) * SLOT_STRIDE] = d_; else li_d = d_; }
        }
    }

    // one node of the profile: its row, then the lifted index
    XP_DEV void node(const ProfileOut &o, int64_t c, const double *es, const Scan &sc, double P, double X, double tp, double tvp, double te, double tve, double tde) {
        row(o, c, P, tp, tvp, te, tve, tde);
        ++jout;
        lifted_index(o, c, es, sc, P, X, tp, tvp, te);
    }

    // the rows the profile did not reach come out NaN, and so does a lifted index whose level it never reached
    XP_DEV void finish(const ProfileOut &o, int64_t c) {
        for (; jout < o.nlev_out; ++jout) {
            int64_t i = jout * o.ls + c * o.cs;
            for (int v = 0; v < 6; ++v) st(o.v[v], o.f64, i, qnan());
        }
        if (!li_done) st(o.li, o.f64, c, qnan());
    }
};

}  // namespace xp
