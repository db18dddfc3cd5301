"""NumPy restatement of xp_cape_cin_layers as include/xparcel.h specifies it, built from the oracle only:
oracle.c_oracle.cape_cin_grid(..., want_profile=True) gives every column's lifted profile (the nodes, LCL included) and
its LFC / EL; every layer bound is inserted into that profile as one more node, parcel and environment interpolated in
ln p between the nodes on either side, and the layer's CAPE / CIN are the oracle's own cape_cin_base on that profile:

  CAPE  cape_cin_base with lfc' = min(lfc_p, pb) and el' = max(el_p, pt): the positive area inside the layer and between
        LFC and EL (el_p: the lowest valid pressure where there is no EL, as cape_cin_base itself substitutes);
  CIN   the cape_cin_base CIN up to max(lfc_p, pt) minus the one up to pb, clamped at 0: the negative area inside the layer
        and below the LFC.

Edge rules: no bottom, a NaN bottom or one above the first node's pressure = from the first node; a top below the last
valid node's pressure = to the top; a NaN top, or top >= bottom with both given, = NaN and ST_NO_LAYER; a NaN parcel / LCL
= 0.0 for every valid layer; no LFC = CAPE and CIN 0.0.  An inserted node next to a node without a pressure or a temperature
has NaN temperatures itself, so the two intervals it makes contribute as little as the one it splits."""
import numpy as np

from oracle import c_oracle

ST_NO_LAYER = 16
TOTALS = ('total_cape', 'total_cin', 'lfc_pressure', 'el_pressure', 'lcl_pressure')


def insert_bound(p, par, env, bound):
    """The profile (nodes in order, NaN rows allowed) with a node at pressure `bound`, unless a node sits exactly on it or it
    lies outside the valid pressures: parcel and environment linear in ln p between the nodes before and after it."""
    valid = np.nonzero(~np.isnan(p))[0]
    if valid.size == 0 or np.any(p[valid] == bound) or not (p[valid].min() < bound < p[valid].max()):
        return p, par, env
    i = valid[p[valid] > bound][-1]                      # pressures decrease along the profile: the last node below the bound
    w = (np.log(bound) - np.log(p[i])) / (np.log(p[i + 1]) - np.log(p[i]))
    row = lambda a: np.insert(a, i + 1, a[i] + w * (a[i + 1] - a[i]))
    return np.insert(p, i + 1, bound), row(par), row(env)


def layer_column(p, par, env, lfc_p, el_p, pb, pt):
    """(cape, cin) of one layer of one lifted profile; pb None / NaN = from the first node."""
    if np.isnan(pt) or (pb is not None and pt >= pb):
        return np.nan, np.nan
    valid = p[~np.isnan(p)]
    if np.isnan(lfc_p) or valid.size == 0:
        return 0.0, 0.0
    if pb is None or np.isnan(pb) or pb > valid.max():
        pb = None
    for b in (pb, pt):
        if b is not None:
            p, par, env = insert_bound(p, par, env, b)
    base = lambda lfc, el: c_oracle.cape_cin_base(p, env, lfc, el, par, pos_cape_neg_cin=True)
    el_eff = el_p if not np.isnan(el_p) else valid.min()
    to_top = pt < valid.min()
    cape = base(lfc_p if pb is None else min(lfc_p, pb), el_eff if to_top else max(el_eff, pt))['cape']
    cin_top = base(lfc_p if to_top else max(lfc_p, pt), el_eff)['cin']
    cin_bottom = 0.0 if pb is None else base(pb, el_eff)['cin']
    return cape, min(0.0, cin_top - cin_bottom)


def layers_grid(p, t, td, bottoms, tops, cols=None, vtc=True, **opts):
    """(nlev, ncol) arrays, per layer a bottom (None, or (ncol,)) and a top (ncol,) -> dict of 'cape', 'cin' (nlayer, ncol'),
    the totals and 'status' of the columns `cols` (default: all), and 'oracle': cape_cin_grid's own result for them.
    opts: cape_cin_grid's (parcel, depth, moist, parcel_values, lcl_interp, ...)."""
    p, t, td = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    cols = np.arange(p.shape[1]) if cols is None else np.asarray(cols)
    pv = opts.pop('parcel_values', None)
    if pv is not None:
        pv = np.asarray(pv, dtype=np.float64)[:, cols]
    r = c_oracle.cape_cin_grid(p[:, cols], t[:, cols], td[:, cols], parcel_values=pv, want_profile=True,
                               virtual_temperature_correction=vtc, **opts)
    prof = r['profile']
    P = prof['pressure']
    PAR = prof['virtual_temperature' if vtc else 'temperature']
    ENV = prof['environment_virtual_temperature' if vtc else 'environment_temperature']
    n = len(tops)
    cape, cin = np.zeros((n, cols.size)), np.zeros((n, cols.size))
    status = r['status'].copy()
    blank = np.isnan(r['lcl_pressure'])
    for i in range(n):
        pt = np.asarray(tops[i], dtype=np.float64)[cols]
        pb = None if bottoms[i] is None else np.asarray(bottoms[i], dtype=np.float64)[cols]
        for j in range(cols.size):
            b = None if pb is None else pb[j]
            if blank[j]:
                bad = np.isnan(pt[j]) or (b is not None and pt[j] >= b)
                cape[i, j] = cin[i, j] = np.nan if bad else 0.0
            else:
                cape[i, j], cin[i, j] = layer_column(P[:, j], PAR[:, j], ENV[:, j], r['lfc_pressure'][j], r['el_pressure'][j], b, pt[j])
        status[np.isnan(cape[i])] |= ST_NO_LAYER
    return {'cape': cape, 'cin': cin, 'status': status, 'total_cape': r['cape'], 'total_cin': r['cin'],
            'lfc_pressure': r['lfc_pressure'], 'el_pressure': r['el_pressure'], 'lcl_pressure': r['lcl_pressure'], 'oracle': r}


def crossing_height(z, a, value):
    """The lowest crossing of a(z) with `value` per column (crossing_level's rule: every interval whose sign changes or is
    NaN at an end, linear in z, the smallest finite one), NaN when there is none."""
    z, d = np.asarray(z, dtype=np.float64), np.asarray(a, dtype=np.float64) - value
    with np.errstate(invalid='ignore', divide='ignore'):
        xi = (d[1:] * z[:-1] - d[:-1] * z[1:]) / (d[1:] - d[:-1])
        hit = np.isnan(d[:-1]) | np.isnan(d[1:]) | (np.sign(d[:-1]) != np.sign(d[1:]))
    xi = np.where(hit, xi, np.nan)
    out = np.full(z.shape[1:], np.nan)
    any_ = ~np.all(np.isnan(xi), axis=0)
    out[any_] = np.nanmin(xi[:, any_], axis=0)
    return out


def pressure_at_height(z, p, at):
    """np.interp(at, z, p) per column over the levels where both exist; NaN outside them."""
    z, p = np.asarray(z, dtype=np.float64), np.asarray(p, dtype=np.float64)
    out = np.full(z.shape[1], np.nan)
    for c in range(z.shape[1]):
        ok = ~(np.isnan(z[:, c]) | np.isnan(p[:, c]))
        if ok.any() and not np.isnan(at[c]):
            out[c] = np.interp(at[c], z[ok, c], p[ok, c], left=np.nan, right=np.nan)
    return out
