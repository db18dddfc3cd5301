"""NumPy restatement of xp_wind_layers, xp_critical_angle, xp_corfidi_storm_motion and xp_significant_tornado_effective as
include/xparcel.h specifies them, one column at a time, in MetPy's own terms (get_layer, mean_pressure_weighted, bulk_shear,
critical_angle, corfidi_storm_motion) rather than the device's single streaming pass:
  1. levels where any supplied input is NaN are dropped;
  2. the levels read are those up to and including the first one beyond every layer's top (every level, while some layer's
     top has not been reached); on them pressures must decrease and, if given, heights increase strictly (else
     ST_BAD_PRESSURE / ST_BAD_HEIGHT, everything NaN);
  3. a layer's bounds: pb, pt in hPa (pressure kinds; a NaN bottom is the lowest valid level's pressure p0, a depth counts
     down from pb), or np.interp(z0 + bottom, z, p), np.interp(z0 + top, z, p) (height kind);
  4. its points: the levels with pt <= p <= pb (np.isclose counting as inside) plus pb and pt where no selected level is close
     to them (u, v linear in ln p there), in order of decreasing pressure -- layer_points of tests/kinematics_restatement.py
     with the bounds given as pressures;
  5. mean = trapz(U P, P) / (0.5 (P_last^2 - P_first^2)), shear = last point - first point, bottom = first point, max = the
     first point of largest hypot(U, V);
  6. a layer with pt >= pb, pb > p0, pt < min p or (height kind) a bound above max z: NaN, ST_NO_LAYER."""
import numpy as np

from tests.kinematics_restatement import (ST_BAD_HEIGHT, ST_BAD_PRESSURE, ST_NO_LAYER, _log_point, _trapz, _valid, close,
                                          layer_points)

PRESSURE, PRESSURE_DEPTH, HEIGHT = 0, 1, 2
WIND_KEYS = ('mean_u', 'mean_v', 'shear_u', 'shear_v', 'bottom_u', 'bottom_v', 'max_u', 'max_v', 'max_pressure')
__all__ = ['layer_points', 'close', '_valid']           # (what this restatement takes from the Bunkers one, besides the bits)


def points_between(p, u, v, pb, pt):
    """MetPy's get_layer(p, u, v, bottom=pb, depth=pb - pt) on ordered levels: kinematics_restatement.layer_points with the
    bound pressures given, not interpolated from heights."""
    near_b, near_t = close(p, pb), close(p, pt)          # (close() on arrays: element by element)
    sel = ((p < pb) | near_b) & ((p > pt) | near_t)
    P, U, V = p[sel], u[sel], v[sel]
    if not near_t[sel].any():                            # the bounds go where the order of decreasing pressure puts them
        ue, ve = _log_point(pt, p, u, v)
        P, U, V = np.r_[P, pt], np.r_[U, ue], np.r_[V, ve]
    if not near_b[sel].any():
        ue, ve = _log_point(pb, p, u, v)
        P, U, V = np.r_[pb, P], np.r_[ue, U], np.r_[ve, V]
    return P, U, V


def _pressure_bounds(kind, bottom, top, p0):
    pb = p0 if np.isnan(bottom) else float(bottom)
    return pb, (float(top) if kind == PRESSURE else pb - float(top))


def speed_gap(U, V):
    """(largest - second largest) / largest of hypot(U, V): how clearly the layer's strongest point stands out."""
    s = np.sort(np.hypot(U, V))
    return np.inf if s.size < 2 or s[-1] == 0.0 else (s[-1] - s[-2]) / s[-1]


def wind_layers_column(p, u, v, z, layers):
    """One column (nlev,); z may be None; layers: (kind, bottom, top) tuples.  Returns a dict of WIND_KEYS (one value per
    layer), 'status', and 'gap' (speed_gap of each layer's points; NaN where there is no layer)."""
    nl = len(layers)
    out = {k: np.full(nl, np.nan) for k in WIND_KEYS + ('gap',)}
    out['status'] = 0
    if z is None:
        p, u, v = _valid(p, u, v)
    else:
        p, u, v, z = _valid(p, u, v, z)
    if p.size == 0:
        out['status'] = ST_NO_LAYER
        return out
    p0 = p[0]
    z0 = None if z is None else z[0]
    # the levels read: layer j is finished at the first level below its top and not close to it -- a layer known to be empty
    # or to begin below the lowest level from the start -- and reading ends at the first level at which every layer is; on
    # the levels read the order must hold
    last = []
    for kind, bottom, top in layers:
        if kind == HEIGHT:
            reach = np.nonzero(z >= z0 + top)[0]
            if reach.size == 0:
                last.append(p.size - 1)
                continue
            i = reach[0]
            pt = float(np.interp(z0 + top, z[:i + 1], p[:i + 1]))
        else:
            pb, pt = _pressure_bounds(kind, bottom, top, p0)
            if not (pt < pb) or pb > p0:
                last.append(0)
                continue
            i = 0
        beyond = np.nonzero((p[i:] < pt) & ~close(p[i:], pt))[0]
        last.append(i + beyond[0] if beyond.size else p.size - 1)
    n = max(last) + 1
    bad_p = np.nonzero(~(p[1:n] < p[:n - 1]))[0]
    bad_z = np.nonzero(~(z[1:n] > z[:n - 1]))[0] if z is not None else bad_p[:0]
    if bad_p.size or bad_z.size:                         # the first level out of order is where reading stops
        first = min(np.r_[bad_p, bad_z])
        out['status'] = (ST_BAD_PRESSURE if first in bad_p else 0) | (ST_BAD_HEIGHT if first in bad_z else 0)
        return out
    p, u, v = p[:n], u[:n], v[:n]
    z = None if z is None else z[:n]
    for j, (kind, bottom, top) in enumerate(layers):
        if kind == HEIGHT:
            bottom = 0.0 if np.isnan(bottom) else bottom
            if z0 + bottom > z.max() or z0 + top > z.max():
                out['status'] |= ST_NO_LAYER
                continue
            pb, pt = float(np.interp(z0 + bottom, z, p)), float(np.interp(z0 + top, z, p))
        else:
            pb, pt = _pressure_bounds(kind, bottom, top, p0)
        if pt >= pb or pb > p0 or pt < p.min():
            out['status'] |= ST_NO_LAYER
            continue
        P, U, V = points_between(p, u, v, pb, pt)        # (sorted: pb first, pt last)
        den = 0.5 * (P[-1] ** 2 - P[0] ** 2)
        with np.errstate(divide='ignore', invalid='ignore'):
            out['mean_u'][j], out['mean_v'][j] = _trapz(U * P, P) / den, _trapz(V * P, P) / den
        out['shear_u'][j], out['shear_v'][j] = U[-1] - U[0], V[-1] - V[0]
        out['bottom_u'][j], out['bottom_v'][j] = U[0], V[0]
        k = int(np.argmax(np.hypot(U, V)))               # (argmax: the first of equals)
        out['max_u'][j], out['max_v'][j], out['max_pressure'][j] = U[k], V[k], P[k]
        out['gap'][j] = speed_gap(U, V)
    return out


def wind_layers_grid(p, u, v, z, layers, cols=None):
    """wind_layers_column() for the columns `cols` (default: all) of (nlev, ncol) arrays: dict of (nlayer, len(cols)) arrays
    and the (len(cols),) status."""
    cols = range(p.shape[1]) if cols is None else cols
    res = [wind_layers_column(p[:, c], u[:, c], v[:, c], None if z is None else z[:, c], layers) for c in cols]
    out = {k: np.stack([r[k] for r in res], axis=1) for k in WIND_KEYS + ('gap',)}
    out['status'] = np.array([r['status'] for r in res])
    return out


# ---- per point ---------------------------------------------------------------------------------------------------------
def _clip(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def critical_angle(shear_u, shear_v, surface_u, surface_v, storm_u, storm_v):
    """atan2(|a x b|, a . b) in degrees, a the shear, b the storm motion minus the surface wind; NaN for a zero vector."""
    au, av, su, sv, cu, cv = (np.asarray(x, dtype=np.float64) for x in (shear_u, shear_v, surface_u, surface_v, storm_u, storm_v))
    bu, bv = cu - su, cv - sv
    ang = np.arctan2(np.abs(au * bv - av * bu), au * bu + av * bv) * (180.0 / np.pi)
    return np.where(((au == 0) & (av == 0)) | ((bu == 0) & (bv == 0)), np.nan, ang)


def critical_angle_arccos(shear_u, shear_v, surface_u, surface_v, storm_u, storm_v):
    """MetPy's own form: arccos(a . b / (|a| |b|)) in degrees."""
    au, av, su, sv, cu, cv = (np.asarray(x, dtype=np.float64) for x in (shear_u, shear_v, surface_u, surface_v, storm_u, storm_v))
    bu, bv = cu - su, cv - sv
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.degrees(np.arccos((au * bu + av * bv) / (np.hypot(au, av) * np.hypot(bu, bv))))


def corfidi_storm_motion(mean_u, mean_v, llj_u, llj_v):
    """(upwind_u, upwind_v, downwind_u, downwind_v): upwind = mean - llj, downwind = mean + upwind."""
    mu, mv, ju, jv = (np.asarray(x, dtype=np.float64) for x in (mean_u, mean_v, llj_u, llj_v))
    uu, uv = mu - ju, mv - jv
    return uu, uv, mu + uu, mv + uv


def significant_tornado_effective(mlcape, mlcin, lcl_height, esrh, ebwd, base_height=None):
    mlcape, mlcin, lcl_height, esrh, ebwd = (np.asarray(x, dtype=np.float64) for x in (mlcape, mlcin, lcl_height, esrh, ebwd))
    lcl = (2000.0 - _clip(lcl_height, 1000.0, 2000.0)) / 1000.0
    cin = (200.0 + _clip(mlcin, -200.0, -50.0)) / 150.0
    shr = np.where(ebwd < 12.5, 0.0, np.where(ebwd > 30.0, 30.0, ebwd)) / 20.0
    stp = ((((mlcape / 1500.0) * lcl) * (esrh / 150.0)) * shr) * cin
    if base_height is not None:
        stp = np.where(np.asarray(base_height, dtype=np.float64) > 0.0, 0.0, stp)
    return stp
