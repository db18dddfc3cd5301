"""NumPy restatement of xp_effective_inflow_layer and xp_storm_relative_helicity_layers as include/xparcel.h specifies
them, built from the oracle: candidate k of a column is lifted with oracle.c_oracle.cape_cin_grid(p[k:], t[k:], td[k:],
parcel='surface'), nothing else.

Effective inflow layer (Thompson et al. 2007), per column:
  1. a level is valid when p, T and Td are all non-NaN; p0 = the pressure of the lowest valid level; the candidates are
     the valid levels with p >= p0 - search_depth (plain comparison), in level order;
  2. candidate k passes when CAPE_k >= cape_min and CIN_k >= cin_min, (CAPE_k, CIN_k) the surface parcel of the column
     cut off below k;
  3. base = the first passing candidate; top = the last passing candidate before the first failing candidate above
     base, or the last candidate if none fails; candidates above that failure are not lifted;
  4. heights are relative to the lowest valid level; status: NO_LAYER (no candidate passes), LAYER_OPEN (the last
     candidate of the window passes), LCL_NOT_CONVERGED and BAD_PRESSURE ORed over the candidates lifted.
The grid function walks k = 0, 1, ... and hands the oracle, at every k, the columns that lift candidate k.

Helicity over per-column layers: tests/kinematics_restatement.py's storm-relative helicity with the bounds bottom, top
given per column and layer, plus the wind at top minus the wind at bottom (linear in height)."""
import numpy as np

from oracle import c_oracle

from tests import kinematics_restatement as kr

ST_LCL_NOT_CONVERGED, ST_BAD_PRESSURE, ST_NO_LAYER, ST_BAD_HEIGHT, ST_LAYER_OPEN = 2, 8, 16, 32, 64
OUT_F = ('base_pressure', 'top_pressure', 'base_height', 'top_height')
OUT_I = ('base_index', 'top_index', 'status')


def inflow_grid(p, t, td, z=None, cape_min=100.0, cin_min=-250.0, search_depth=300.0, moist='rk4', **opts):
    """(nlev, ncol) arrays -> dict of the per-column outputs, candidate_cape / candidate_cin (nlev, ncol; NaN where the
    level was not lifted).  Arithmetic in float64 on the inputs as they are."""
    p, t, td = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    nlev, ncol = p.shape
    valid = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    has = valid.any(axis=0)
    k0 = np.where(has, np.argmax(valid, axis=0), 0)                      # the lowest valid level
    cols = np.arange(ncol)
    p0 = np.where(has, p[k0, cols], np.nan)
    with np.errstate(invalid='ignore'):
        cand = valid & (p >= (p0 - search_depth)[None, :])
    base = np.full(ncol, -1, dtype=np.int32)
    top = np.full(ncol, -1, dtype=np.int32)
    status = np.zeros(ncol, dtype=np.int32)
    closed = np.zeros(ncol, dtype=bool)                                  # a candidate above the base has failed
    ccape = np.full((nlev, ncol), np.nan)
    ccin = np.full((nlev, ncol), np.nan)
    for k in range(nlev):
        act = np.nonzero(cand[k] & ~closed)[0]
        if act.size == 0:
            continue
        r = c_oracle.cape_cin_grid(p[k:, act], t[k:, act], td[k:, act], parcel='surface', moist=moist, **opts)
        ccape[k, act], ccin[k, act] = r['cape'], r['cin']
        status[act] |= r['status'] & (ST_LCL_NOT_CONVERGED | ST_BAD_PRESSURE)
        ok = (r['cape'] >= cape_min) & (r['cin'] >= cin_min)
        first = ok & (base[act] < 0)
        base[act[first]] = k
        top[act[ok]] = k
        closed[act[~ok & (base[act] >= 0)]] = True
    status[base < 0] |= ST_NO_LAYER
    status[(base >= 0) & ~closed] |= ST_LAYER_OPEN
    out = {'base_index': base, 'top_index': top, 'status': status, 'candidate_cape': ccape, 'candidate_cin': ccin}
    lay = base >= 0
    b, tt = np.where(lay, base, 0), np.where(lay, top, 0)
    out['base_pressure'] = np.where(lay, p[b, cols], np.nan)
    out['top_pressure'] = np.where(lay, p[tt, cols], np.nan)
    if z is None:
        out['base_height'] = out['top_height'] = np.full(ncol, np.nan)
    else:
        z = np.asarray(z, dtype=np.float64)
        out['base_height'] = np.where(lay, z[b, cols] - z[k0, cols], np.nan)
        out['top_height'] = np.where(lay, z[tt, cols] - z[k0, cols], np.nan)
    return out


def near_threshold(res, cape_min=100.0, cin_min=-250.0, tol=1e-5):
    """True for the columns where some lifted candidate sits within `tol` of a threshold: whether it passes hangs on the
    last digits of CAPE / CIN."""
    with np.errstate(invalid='ignore'):
        near = (np.abs(res['candidate_cape'] - cape_min) <= tol) | (np.abs(res['candidate_cin'] - cin_min) <= tol)
    return near.any(axis=0)


# ---- helicity and bulk wind difference over per-column layers -------------------------------------------------------------
LAYER_KEYS = kr.SRH_KEYS + ('shear_u', 'shear_v')


def _wind_at(he, h, u, v):
    """The wind at height he: a level exactly on it gives its own, otherwise linear in height between its neighbours."""
    on = np.nonzero(h == he)[0]
    if on.size:
        return u[on[0]], v[on[0]]
    return kr._lin_point(he, h, u, v)


def _points(h, u, v, bottom, top):
    """kr.srh_points with the top given, not bottom + depth."""
    sel = np.array([(hk > bottom or kr.close(hk, bottom)) and (hk < top or kr.close(hk, top)) for hk in h], dtype=bool)
    pts = [(hk, uk, vk) for hk, uk, vk in zip(h[sel], u[sel], v[sel])]
    if top not in [q[0] for q in pts]:
        pts.append((top,) + kr._lin_point(top, h, u, v))
    if bottom not in [q[0] for q in pts]:
        pts.append((bottom,) + kr._lin_point(bottom, h, u, v))
    pts.sort(key=lambda q: q[0])
    return tuple(np.array(c) for c in zip(*pts))


def layers_column(z, u, v, bottom, tops, storm_u=0.0, storm_v=0.0, surface_u=None, surface_v=None):
    """One column (nlev,), one bottom, len(tops) tops: dict of positive, negative, total, shear_u, shear_v (one value per
    layer) and status."""
    tops = [float(x) for x in tops]
    out = {k: np.full(len(tops), np.nan) for k in LAYER_KEYS}
    out['status'] = 0
    bottom = float(bottom)
    good = [bottom >= 0.0 and x > bottom for x in tops]                  # NaN bounds compare false
    if not any(good):
        out['status'] = ST_NO_LAYER
        return out
    h, u, v = kr._valid(z, u, v)
    if surface_u is None:
        h = h - h[0] if h.size else h
    elif not (np.isnan(surface_u) or np.isnan(surface_v)):
        h, u, v = (np.concatenate([[s], a]) for s, a in ((0.0, h), (surface_u, u), (surface_v, v)))
    tmax = max(x for x, g in zip(tops, good) if g)
    n = h.size
    for i in range(h.size):                      # the points read, and their order
        if i and not h[i] > h[i - 1]:
            out['status'] = ST_BAD_HEIGHT
            return out
        if h[i] > tmax and not kr.close(h[i], tmax):
            n = i + 1
            break
    h, u, v = h[:n], u[:n], v[:n]
    for j, x in enumerate(tops):
        if not good[j] or h.size == 0 or x > h.max() or bottom < h.min():
            out['status'] |= ST_NO_LAYER
            continue
        H, U, V = _points(h, u, v, bottom, x)
        su, sv = U - storm_u, V - storm_v
        terms = su[1:] * sv[:-1] - su[:-1] * sv[1:]
        pos, neg = float(terms[terms > 0].sum()), float(terms[terms < 0].sum())
        if np.isnan(storm_u) or np.isnan(storm_v):
            pos = neg = np.nan
        out['positive'][j], out['negative'][j], out['total'][j] = pos, neg, pos + neg
        (ut, vt), (ub, vb) = _wind_at(x, h, u, v), _wind_at(bottom, h, u, v)
        out['shear_u'][j], out['shear_v'][j] = ut - ub, vt - vb
    return out


def layers_grid(z, u, v, bottom, tops, storm_u=0.0, storm_v=0.0, surface_u=None, surface_v=None, cols=None):
    """layers_column() for the columns `cols` of (nlev, ncol) arrays; bottom (ncol,), tops a sequence of (ncol,) arrays.
    Returns dict of (nlayer, len(cols)) arrays and the (len(cols),) status."""
    ncol = z.shape[1]
    cols = range(ncol) if cols is None else cols
    bc = lambda a: None if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (ncol,))
    b, ts = bc(bottom), [bc(x) for x in tops]
    per = [bc(a) for a in (storm_u, storm_v, surface_u, surface_v)]
    res = [layers_column(z[:, c], u[:, c], v[:, c], b[c], [x[c] for x in ts], per[0][c], per[1][c],
                         None if per[2] is None else per[2][c], None if per[3] is None else per[3][c]) for c in cols]
    out = {k: np.stack([r[k] for r in res], axis=1) for k in LAYER_KEYS}
    out['status'] = np.array([r['status'] for r in res])
    return out
