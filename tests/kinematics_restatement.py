"""NumPy restatement of the kinematics entry points -- xp_bunkers_storm_motion, xp_storm_relative_helicity,
xp_significant_tornado, xp_supercell_composite (MetPy 1.4's bunkers_storm_motion, storm_relative_helicity,
significant_tornado, supercell_composite) -- as include/xparcel.h specifies them, one column at a time, in MetPy's own
terms (get_layer / get_layer_heights, np.interp, trapz) rather than the device's single streaming pass:
  1. levels where any input is NaN are dropped;
  2. the levels read are those up to and including the first one beyond the highest top; on them heights must increase
     and pressures decrease strictly (else ST_BAD_HEIGHT / ST_BAD_PRESSURE, everything NaN);
  3. Bunkers: M(zb, d) = trapz(u, p) / (p_last - p_first) over the levels with pt <= p <= pb (np.isclose counting as
     inside) plus pb = np.interp(zb, z, p) and pt = np.interp(zb + d, z, p) where no point is close to them (u, v linear
     in ln p there); mean = M(z0, 6000), low = M(z0, 500), high = M(z0 + 5500, 500), rdev = (shear_v, -shear_u) * 7.5 / |shear|;
  4. SRH: h = z - z_first (or heights as given after the surface point at 0 m); the levels with bottom <= h <= top (np.isclose
     counting) plus bottom and top where no level equals them (u, v linear in height); the helicity terms of the
     storm-relative wind, summed by sign;
  5. the composites in MetPy's operation order."""
import numpy as np

ST_BAD_PRESSURE, ST_NO_LAYER, ST_BAD_HEIGHT = 8, 16, 32
BUNKERS_KEYS = ('right_u', 'right_v', 'left_u', 'left_v', 'mean_u', 'mean_v')
SRH_KEYS = ('positive', 'negative', 'total')


def close(x, y):
    """np.isclose(x, y): |x - y| <= 1e-8 + 1e-5 |y|."""
    return abs(x - y) <= 1e-8 + 1e-5 * abs(y)


def _trapz(y, x):
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def _valid(*arrays):
    arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
    ok = ~np.any([np.isnan(a) for a in arrays], axis=0)
    return [a[ok] for a in arrays]


# ---- Bunkers storm motion -----------------------------------------------------------------------------------------------
def _log_point(pe, p, u, v):
    """u, v at pressure pe, linear in ln p between the levels on either side of it."""
    lo, hi = np.nonzero(p > pe)[0][-1], np.nonzero(p < pe)[0][0]
    f = (np.log(pe) - np.log(p[hi])) / (np.log(p[lo]) - np.log(p[hi]))
    return u[hi] + f * (u[lo] - u[hi]), v[hi] + f * (v[lo] - v[hi])


def layer_points(p, u, v, z, zb, depth):
    """MetPy's get_layer(p, u, v, height=z, bottom=zb, depth=depth) on ordered levels: (P, U, V) in order of decreasing
    pressure."""
    pb, pt = float(np.interp(zb, z, p)), float(np.interp(zb + depth, z, p))
    sel = np.array([(pk < pb or close(pk, pb)) and (pk > pt or close(pk, pt)) for pk in p], dtype=bool)
    pts = [(pk, uk, vk) for pk, uk, vk in zip(p[sel], u[sel], v[sel])]
    if not any(close(pk, pt) for pk, _, _ in pts):
        pts.append((pt,) + _log_point(pt, p, u, v))
    if not any(close(pk, pb) for pk, _, _ in pts):
        pts.append((pb,) + _log_point(pb, p, u, v))
    pts.sort(key=lambda t: -t[0])
    return tuple(np.array(c) for c in zip(*pts))


def layer_mean(p, u, v, z, zb, depth):
    """weighted_continuous_average: (mean u, mean v) over the layer."""
    P, U, V = layer_points(p, u, v, z, zb, depth)
    return np.array([_trapz(U, P) / (P[-1] - P[0]), _trapz(V, P) / (P[-1] - P[0])])


def bunkers_column(p, u, v, z):
    """One column (nlev,): dict of right_u, right_v, left_u, left_v, mean_u, mean_v and status."""
    out = {k: np.nan for k in BUNKERS_KEYS}
    out['status'] = 0
    p, u, v, z = _valid(p, u, v, z)
    if p.size == 0:
        out['status'] = ST_NO_LAYER
        return out
    zt = z[0] + 6000.0
    n = p.size
    for i in range(1, p.size):                   # the levels read, and their order
        bad = (0 if z[i] > z[i - 1] else ST_BAD_HEIGHT) | (0 if p[i] < p[i - 1] else ST_BAD_PRESSURE)
        if bad:
            out['status'] = bad
            return out
        if z[i] >= zt:
            pt = float(np.interp(zt, z[:i + 1], p[:i + 1]))
            if p[i] < pt and not close(p[i], pt):
                n = i + 1
                break
    p, u, v, z = p[:n], u[:n], v[:n], z[:n]
    if zt > z.max():
        out['status'] = ST_NO_LAYER
        return out
    mean = layer_mean(p, u, v, z, z[0], 6000.0)
    shear = layer_mean(p, u, v, z, z[0] + 5500.0, 500.0) - layer_mean(p, u, v, z, z[0], 500.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        rdev = np.array([shear[1], -shear[0]]) * (7.5 / np.hypot(*shear))
    right, left = mean + rdev, mean - rdev
    out.update(right_u=right[0], right_v=right[1], left_u=left[0], left_v=left[1], mean_u=mean[0], mean_v=mean[1])
    return out


def bunkers_grid(p, u, v, z, cols=None):
    """bunkers_column() for the columns `cols` (default: all) of (nlev, ncol) arrays: dict of (len(cols),) arrays."""
    cols = range(p.shape[1]) if cols is None else cols
    res = [bunkers_column(p[:, c], u[:, c], v[:, c], z[:, c]) for c in cols]
    return {k: np.array([r[k] for r in res]) for k in BUNKERS_KEYS + ('status',)}


# ---- storm-relative helicity ----------------------------------------------------------------------------------------------
def _lin_point(he, h, u, v):
    """u, v at height he, linear in height between the levels on either side of it."""
    lo, hi = np.nonzero(h < he)[0][-1], np.nonzero(h > he)[0][0]
    f = (he - h[lo]) / (h[hi] - h[lo])
    return u[lo] + f * (u[hi] - u[lo]), v[lo] + f * (v[hi] - v[lo])


def srh_points(h, u, v, bottom, depth):
    """MetPy's get_layer_heights(h, depth, u, v, bottom=bottom) on ordered heights: (H, U, V) in increasing height."""
    top = bottom + depth
    sel = np.array([(hk > bottom or close(hk, bottom)) and (hk < top or close(hk, top)) for hk in h], dtype=bool)
    pts = [(hk, uk, vk) for hk, uk, vk in zip(h[sel], u[sel], v[sel])]
    if top not in [t[0] for t in pts]:
        pts.append((top,) + _lin_point(top, h, u, v))
    if bottom not in [t[0] for t in pts]:
        pts.append((bottom,) + _lin_point(bottom, h, u, v))
    pts.sort(key=lambda t: t[0])
    return tuple(np.array(c) for c in zip(*pts))


def srh_column(z, u, v, depths, bottom=0.0, storm_u=0.0, storm_v=0.0, surface_u=None, surface_v=None):
    """One column (nlev,): dict of positive, negative, total (one value per depth) and status."""
    depths = [float(d) for d in np.atleast_1d(depths)]
    nd = len(depths)
    out = {k: np.full(nd, np.nan) for k in SRH_KEYS}
    out['status'] = 0
    h, u, v = _valid(z, u, v)
    if surface_u is None:
        h = h - h[0] if h.size else h
    elif not (np.isnan(surface_u) or np.isnan(surface_v)):
        h, u, v = (np.concatenate([[s], a]) for s, a in ((0.0, h), (surface_u, u), (surface_v, v)))
    tmax = bottom + max(depths)
    n = h.size
    for i in range(h.size):                      # the points read, and their order
        if i and not h[i] > h[i - 1]:
            out['status'] = ST_BAD_HEIGHT
            return out
        if h[i] > tmax and not close(h[i], tmax):
            n = i + 1
            break
    h, u, v = h[:n], u[:n], v[:n]
    for j, d in enumerate(depths):
        if h.size == 0 or bottom + d > h.max() or bottom < h.min():
            out['status'] |= ST_NO_LAYER
            continue
        H, U, V = srh_points(h, u, v, bottom, d)
        su, sv = U - storm_u, V - storm_v
        terms = su[1:] * sv[:-1] - su[:-1] * sv[1:]
        pos, neg = float(terms[terms > 0].sum()), float(terms[terms < 0].sum())
        if np.isnan(storm_u) or np.isnan(storm_v):
            pos = neg = np.nan
        out['positive'][j], out['negative'][j], out['total'][j] = pos, neg, pos + neg
    return out


def srh_grid(z, u, v, depths, bottom=0.0, storm_u=0.0, storm_v=0.0, surface_u=None, surface_v=None, cols=None):
    """srh_column() for the columns `cols` of (nlev, ncol) arrays; storm_u, ... scalars or (ncol,) arrays.  Returns dict
    of (ndepth, len(cols)) arrays and the (len(cols),) status."""
    cols = range(z.shape[1]) if cols is None else cols
    ncol = z.shape[1]
    per = [None if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (ncol,))
           for a in (storm_u, storm_v, surface_u, surface_v)]
    res = [srh_column(z[:, c], u[:, c], v[:, c], depths, bottom, per[0][c], per[1][c],
                      None if per[2] is None else per[2][c], None if per[3] is None else per[3][c]) for c in cols]
    out = {k: np.stack([r[k] for r in res], axis=1) for k in SRH_KEYS}
    out['status'] = np.array([r['status'] for r in res])
    return out


# ---- composites ------------------------------------------------------------------------------------------------------------
def significant_tornado(sbcape, lcl_height, srh, shear):
    sbcape, lcl_height, srh, shear = (np.asarray(a, dtype=np.float64) for a in (sbcape, lcl_height, srh, shear))
    lcl = (2000.0 - np.clip(lcl_height, 1000.0, 2000.0)) / 1000.0
    shr = np.where(shear < 12.5, 0.0, np.minimum(shear, 30.0)) / 20.0
    return (sbcape * lcl * srh * shr) / (1500.0 * 150.0)


def supercell_composite(mucape, srh, shear):
    mucape, srh, shear = (np.asarray(a, dtype=np.float64) for a in (mucape, srh, shear))
    shr = np.where(shear < 10.0, 0.0, np.minimum(shear, 20.0)) / 20.0
    return (mucape / 1000.0) * (srh / 50.0) * shr
