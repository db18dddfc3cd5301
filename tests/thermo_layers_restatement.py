"""NumPy restatement of xp_thermo_layers as include/xparcel.h specifies it, one column at a time, in MetPy's own terms (get_layer,
precipitable_water, np.trapz over the layer's points) rather than the device's single streaming pass:
  1. levels where any SUPPLIED input is NaN are dropped (_valid);
  2. the levels read, and the ordering rule on them, are those of tests/wind_layers_restatement.py (levels_read below is its
     loop with the two extensions: an open top reads every level, a per-column bound stands in for the scalar);
  3. a layer's bounds pb, pt: as there; an open top (XP_LAYER_PRESSURE with a NaN scalar top) is the smallest valid pressure;
     a per-column bottom that is NaN is p0, a per-column top that is NaN is no layer;
  4. its points: wind_layers_restatement.points_between -- MetPy's get_layer -- on (T, Td) and on z, each linear in ln p at an
     added bound point (_log_point);
  5. at every point, from the point's own (interpolated) T and Td, with oracle.thermo: e = e_s(Td), es = e_s(T),
     w = eps e / (P - e), rh = e / es, th = equivalent_potential_temperature(P, T, Td);
  6. S = trapz(w, P), R = trapz(rh, P), D = P_last - P_first: precipitable_water = -S 1e5 / (g rho_l) [mm], mean_mixing_ratio =
     S / D, mean_relative_humidity = R / D, thickness = z_last - z_first, lapse_rate = -(T_last - T_first) / thickness * 1000,
     theta_e_min / theta_e_max and their pressures by argmin / argmax (the first of equals);
  7. a layer with pt >= pb, pb > p0, pt < min p or (height kind) a bound above max z: NaN, ST_NO_LAYER.
Also returned per layer: gap_min, gap_max, the relative gap between the two smallest and between the two largest th (inf with
fewer than two points): how clearly the extreme point stands out, as wind_layers_restatement.speed_gap."""
import numpy as np

from oracle import thermo as O
from tests.kinematics_restatement import ST_BAD_HEIGHT, ST_BAD_PRESSURE, ST_NO_LAYER, _log_point, _trapz, _valid, close
from tests.wind_layers_restatement import HEIGHT, PRESSURE, PRESSURE_DEPTH, layer_points, points_between

G = 9.80665                     # metpy.constants.g
RHO_L = 999.97495               # metpy.constants.rho_l (MetPy 1.4) [kg m^-3]
PW_MM = 1e5 / (G * RHO_L)       # trapz(w, p [hPa]) -> mm
THERMO_KEYS = ('precipitable_water', 'mean_mixing_ratio', 'mean_relative_humidity', 'thickness', 'lapse_rate', 'theta_e_min',
               'theta_e_min_pressure', 'theta_e_max', 'theta_e_max_pressure')
GAPS = ('gap_min', 'gap_max')
__all__ = ['layer_points', 'close', '_valid', '_log_point', 'HEIGHT', 'PRESSURE', 'PRESSURE_DEPTH', 'ST_BAD_HEIGHT',
           'ST_BAD_PRESSURE', 'ST_NO_LAYER']


def _bounds(kind, bottom, top, bcol, tcol, p0):
    """(pb, pt, open) of a layer by pressure; pt is NaN for an open top and for a NaN per-column top."""
    bottom = bottom if bcol is None else bcol
    pb = p0 if np.isnan(bottom) else float(bottom)
    if tcol is not None:
        return pb, float(tcol), False
    if kind == PRESSURE:
        return pb, float(top), bool(np.isnan(top))
    return pb, pb - float(top), False


def levels_read(p, z, layers, bcols, tcols):
    """How many of the valid levels (p, z; z may be None) the call reads: layer j is finished at the first level below its
    top and not close to it -- a layer known to be empty or to begin below the lowest level at the first level; an open top
    never -- and reading ends at the first level at which every layer is."""
    p0 = p[0]
    last = []
    for (kind, bottom, top), bcol, tcol in zip(layers, bcols, tcols):
        if kind == HEIGHT:
            reach = np.nonzero(z >= z[0] + top)[0]
            if reach.size == 0:
                last.append(p.size - 1)
                continue
            i = reach[0]
            pt = float(np.interp(z[0] + top, z[:i + 1], p[:i + 1]))
        else:
            pb, pt, open_top = _bounds(kind, bottom, top, bcol, tcol, p0)
            if pb > p0 or (not open_top and not (pt < pb)):
                last.append(0)
                continue
            if open_top:
                last.append(p.size - 1)
                continue
            i = 0
        beyond = np.nonzero((p[i:] < pt) & ~close(p[i:], pt))[0]
        last.append(i + beyond[0] if beyond.size else p.size - 1)
    return max(last) + 1


def extreme_gaps(th):
    """((second smallest - smallest) / |smallest|, (largest - second largest) / |largest|) of th; inf with fewer than two."""
    s = np.sort(th)
    if s.size < 2:
        return np.inf, np.inf
    with np.errstate(divide='ignore', invalid='ignore'):
        return (s[1] - s[0]) / abs(s[0]), (s[-1] - s[-2]) / abs(s[-1])


def thermo_layers_column(p, t, td, z, layers, bottom_columns=None, top_columns=None):
    """One column (nlev,); t, td, z may each be None; layers: (kind, bottom, top) tuples, a NaN top by pressure being the open
    one; bottom_columns / top_columns: per layer None or this column's bound [hPa].  Returns a dict of THERMO_KEYS and GAPS
    (one value per layer; what needs a view that is None is computed from zeros and means nothing) and 'status'."""
    nl = len(layers)
    bcols = [None] * nl if bottom_columns is None else list(bottom_columns)
    tcols = [None] * nl if top_columns is None else list(top_columns)
    out = {k: np.full(nl, np.nan) for k in THERMO_KEYS + GAPS}
    out['status'] = 0
    given = [a for a in (t, td, z) if a is not None]
    cols = _valid(p, *given)
    p = cols[0]
    it = iter(cols[1:])
    t, td, z = (None if a is None else next(it) for a in (t, td, z))
    if p.size == 0:
        out['status'] = ST_NO_LAYER
        return out
    p0 = p[0]
    n = levels_read(p, z, layers, bcols, tcols)
    bad_p = np.nonzero(~(p[1:n] < p[:n - 1]))[0]
    bad_z = np.nonzero(~(z[1:n] > z[:n - 1]))[0] if z is not None else bad_p[:0]
    if bad_p.size or bad_z.size:                         # the first level out of order is where reading stops
        first = min(np.r_[bad_p, bad_z])
        out['status'] = (ST_BAD_PRESSURE if first in bad_p else 0) | (ST_BAD_HEIGHT if first in bad_z else 0)
        return out
    p = p[:n]
    t, td, z = (None if a is None else a[:n] for a in (t, td, z))
    zero = np.zeros_like(p)
    for j, (kind, bottom, top) in enumerate(layers):
        if kind == HEIGHT:
            bottom = 0.0 if np.isnan(bottom) else bottom
            if z[0] + bottom > z.max() or z[0] + top > z.max():
                out['status'] |= ST_NO_LAYER
                continue
            pb, pt = float(np.interp(z[0] + bottom, z, p)), float(np.interp(z[0] + top, z, p))
        else:
            pb, pt, open_top = _bounds(kind, bottom, top, bcols[j], tcols[j], p0)
            if open_top:
                pt = float(p.min())
        if not (pt < pb) or pb > p0 or pt < p.min():
            out['status'] |= ST_NO_LAYER
            continue
        P, T, Td = points_between(p, zero if t is None else t, zero if td is None else td, pb, pt)   # (sorted: pb first, pt last)
        Z = points_between(p, zero if z is None else z, zero, pb, pt)[1]
        with np.errstate(divide='ignore', invalid='ignore'):
            e, es = O.saturation_vapor_pressure(Td), O.saturation_vapor_pressure(T)
            w, rh = O.mixing_ratio(e, P), e / es
            th = O.equivalent_potential_temperature(P, T, Td) if t is not None and td is not None else np.zeros_like(P)
            S, R, D = _trapz(w, P), _trapz(rh, P), P[-1] - P[0]
            out['precipitable_water'][j] = -S * PW_MM
            out['mean_mixing_ratio'][j], out['mean_relative_humidity'][j] = np.float64(S) / D, np.float64(R) / D
            out['thickness'][j] = Z[-1] - Z[0]
            out['lapse_rate'][j] = -(T[-1] - T[0]) / np.float64(Z[-1] - Z[0]) * 1000.0
        lo, hi = int(np.argmin(th)), int(np.argmax(th))                  # (the first of equals)
        out['theta_e_min'][j], out['theta_e_min_pressure'][j] = th[lo], P[lo]
        out['theta_e_max'][j], out['theta_e_max_pressure'][j] = th[hi], P[hi]
        out['gap_min'][j], out['gap_max'][j] = extreme_gaps(th)
    return out


def thermo_layers_grid(p, t, td, z, layers, bottom_columns=None, top_columns=None, cols=None):
    """thermo_layers_column() for the columns `cols` (default: all) of (nlev, ncol) arrays; bottom_columns / top_columns: per
    layer None or an (ncol,) array.  Returns a dict of (nlayer, len(cols)) arrays and the (len(cols),) status."""
    cols = range(p.shape[1]) if cols is None else cols
    nl = len(layers)
    bc = [None] * nl if bottom_columns is None else bottom_columns
    tc = [None] * nl if top_columns is None else top_columns
    res = [thermo_layers_column(p[:, c], *(None if a is None else a[:, c] for a in (t, td, z)), layers,
                                [None if b is None else float(b[c]) for b in bc], [None if b is None else float(b[c]) for b in tc])
           for c in cols]
    out = {k: np.stack([r[k] for r in res], axis=1) for k in THERMO_KEYS + GAPS}
    out['status'] = np.array([r['status'] for r in res])
    return out
