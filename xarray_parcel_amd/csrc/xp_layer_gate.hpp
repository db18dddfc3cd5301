// xp_layer_gate.hpp -- which points of a column are the points of MetPy's get_layer, stated once for the kernels that walk a
// column upward and feed those points into running sums (k_bunkers_storm_motion, k_wind_layers, k_thermo_layers): the levels
// between the bounds; a level that is isclose to a bound stands in for it; otherwise the bound is an added point, interpolated
// in ln p between the level below and the level above.  Shared: that decision (LayerGate::level) and how a layer's kind and
// bounds become a column's bound pressures (layer_bounds).  Not shared: the walks -- each kernel keeps its loop, loads, sums
// and stores and plugs them in as three inlined hooks (Bunkers as a case of a general walk was 1.5x slower).
#pragma once
#include "xp_kernels.hpp"

namespace xp {

constexpr int WL_PRESSURE = 0, WL_PRESSURE_DEPTH = 1, WL_HEIGHT = 2;   // include/xparcel.h's XP_LAYER_*

// A layer's bounds at one valid level of a column.  pb, b_now: the bottom pressure, which became known at this level -- the first
// one at or beyond it (pb is read at that level only); pt: the top pressure once the walk has reached it (NaN before), t_now: now.
struct LayerBounds { double pb; bool b_now; double pt; bool t_now; };

// The state of one layer that the rule reads.  A layer derives from it, adds its sums and an emit() that sets `started` and
// `pl`, and gives level() -- one valid level at pressure p, the previous valid level (pp) below it if has_prev -- a step object
// with three hooks: below() emits the previous level, bound(pe) the added point at pressure pe between the two, here() this level.
struct LayerGate {
    double pl;                               // the last point emitted (pressure)
    double pt;                               // layer_bounds' copy of the top pressure once reached (NaN before); unused by Bunkers
    bool begun, started, top_close, fin;     // the bottom pressure is known; a point has been emitted; ...; finished
    XP_DEV void init_gate() { pl = pt = qnan(); begun = started = top_close = fin = false; }
    template <typename Step> XP_DEV void level(Step s, double p, double pp, bool has_prev, const LayerBounds &b) {
        if (fin) return;
        if (b.b_now) {
            begun = true;
            if (has_prev && isclose_(pp, b.pb)) s.below();                 // the level below, close to pb, is the first point
            else if (!isclose_(p, b.pb)) s.bound(b.pb);                    // pb itself (strictly between the levels)
        }
        if (!begun) return;
        if (b.t_now) top_close = started && isclose_(pl, b.pt);         // the top appears: was the last point close to it?
        if (isnan_(b.pt) || p >= b.pt || isclose_(p, b.pt)) {
            s.here();
            top_close = top_close || (!isnan_(b.pt) && isclose_(p, b.pt));
        } else {                                         // the first level beyond the top: pt closes the layer
            // (pt appeared at this level: had it appeared earlier, that level was in the layer and close to it)
            if (!top_close && b.t_now) s.bound(b.pt);
            fin = true;
        }
    }
};

// np.interp(zc, z, p) at the first level (z, p) with z >= zc, the previous valid level (zp, pp) below it
XP_DEV double interp_p(double zc, double zp, double pp, double z, double p, bool has_prev) {
#pragma clang fp contract(off)
    return (z == zc || !has_prev) ? p : (p - pp) / (z - zp) * (zc - zp) + pp;
}

// The bounds of the layer r (kind, bottom, top as the caller gave them; a NaN bottom pressure: the lowest valid level's) at the
// valid level (z, p) of a column whose lowest valid level is (z0, p0) and whose previous one, if has_prev, is (zp, pp); by
// height they appear as the walk reaches them.  open: a NaN top means "to the highest valid level", not an empty layer.  A
// layer that is left out (no point emitted, no top reached) is finished here: level() then does nothing.
XP_DEV LayerBounds layer_bounds(LayerGate &r, int kind, double bottom, double top, bool open, double z0, double p0, double zp,
                                double pp, double z, double p, bool has_prev) {
#pragma clang fp contract(off)
    LayerBounds b = {qnan(), false, qnan(), false};
    if (kind == WL_HEIGHT) {
        const double zb = z0 + bottom, zt = z0 + top;
        b.b_now = !r.begun && z >= zb;
        b.t_now = isnan_(r.pt) && z >= zt;
        if (b.b_now) b.pb = interp_p(zb, zp, pp, z, p, has_prev);
        if (b.t_now) r.pt = interp_p(zt, zp, pp, z, p, has_prev);
    } else {
        b.pb = isnan_(bottom) ? p0 : bottom;
        const double ptn = kind == WL_PRESSURE ? top : b.pb - top;
        // a layer that is empty (a NaN top that is not the open one included) or begins below the lowest level: left out
        if (!has_prev && ((!open && !(ptn < b.pb)) || b.pb > p0)) { r.fin = true; return b; }
        b.b_now = !r.begun && p <= b.pb;
        b.t_now = isnan_(r.pt) && p <= ptn;              // (never, for an open top: every level above the bottom is a point)
        if (b.t_now) r.pt = ptn;
    }
    b.pt = r.pt;
    return b;
}

}  // namespace xp
