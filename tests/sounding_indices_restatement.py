"""NumPy restatement of xp_sounding_indices (include/xparcel.h has the rules), one column at a time, built from the oracle's
pieces: e_s, dewpoint, mixing ratio and vapour pressure (oracle.thermo), the per-column LCL, the moist adiabat in 'rk4', 'ode'
or 'table' mode and the mixed-layer parcel (oracle.parcel_oracle).  The steps:
  1. thermodynamically valid levels: p, T, Td non-NaN; wind-valid levels: p, u, v non-NaN; the others are dropped;
  2. a variable at 850 / 700 / 500 hPa: the first valid level at or above the isobar gives its value if it lies ON it,
     otherwise the value is linear in ln p between that level and the valid level below it (NaN without one);
  3. span: the first valid level has p >= 850 and some valid level p <= 500 -- else the six indices are NaN (XP_ST_NO_LAYER);
     SWEAT needs the same of the wind-valid levels;
  4. VT, CT, TT, K from the isobar values; Showalter: the parcel (850, T850, Td850) to its LCL, dry to 500 hPa if the LCL lies
     at or above it, moist from the LCL otherwise; SWEAT from the interpolated winds;
  5. CCL: rt = dewpoint(p r / (eps + r)) at every valid level (r: w_s(p0, Td0), rt at the start level Td0 itself; or the
     mixed-layer mean mixing ratio), crossings where np.sign(rt - T) of two consecutive valid levels differ (a NaN is no
     sign), located by find_intersections' expressions in ln p, or at the level itself where rt - T is exactly 0 there."""
import numpy as np

from oracle import parcel_oracle as po
from oracle import thermo as th

ST_LCL_NOT_CONVERGED, ST_NO_LAYER, ST_NO_CCL = 2, 16, 128
KNOT = 1852.0 / 3600.0
DEG = 57.29577951308232
INDEX_KEYS = ('k_index', 'total_totals', 'cross_totals', 'vertical_totals', 'showalter_index', 'sweat_index')
CCL_KEYS = ('ccl_pressure', 'ccl_temperature', 'convective_temperature')
KEYS = INDEX_KEYS + CCL_KEYS
NAN = float('nan')


def at_isobar(P, p, *vals):
    """Step 2 on the valid levels p (in level order) of one column: the values of `vals` at P."""
    at = np.nonzero(p <= P)[0]
    if at.size == 0:
        return [NAN] * len(vals)
    i = int(at[0])
    if p[i] == P:
        return [float(v[i]) for v in vals]
    if i == 0:
        return [NAN] * len(vals)
    f = (np.log(P) - np.log(p[i])) / (np.log(p[i - 1]) - np.log(p[i]))
    return [float(v[i] + (v[i - 1] - v[i]) * f) for v in vals]


def spans(p):
    return bool(p.size and p[0] >= 850.0 and np.any(p <= 500.0))


def knots_and_direction(u, v):
    f = np.sqrt(u * u + v * v) / KNOT
    d = 90.0 - np.arctan2(-v, -u) * DEG
    return f, (d + 360.0 if d <= 0.0 else d)


def sweat_terms(td850, tt, u850, v850, u500, v500):
    """The quantities SWEAT compares with thresholds, and the index."""
    f850, d850 = knots_and_direction(u850, v850)
    f500, d500 = knots_and_direction(u500, v500)
    on = bool(130.0 <= d850 <= 250.0 and 210.0 <= d500 <= 310.0 and d500 - d850 > 0.0 and f850 >= 15.0 and f500 >= 15.0)
    shear = 125.0 * (np.sin((d500 - d850) / DEG) + 0.2) if on else 0.0
    tdc = td850 - 273.15
    sweat = (((12.0 * max(tdc, 0.0) + 20.0 * max(tt - 49.0, 0.0)) + 2.0 * f850) + f500) + shear
    return {'f850': f850, 'd850': d850, 'f500': f500, 'd500': d500, 'shear_on': on, 'shear': shear, 'sweat_index': sweat}


def showalter_parcel(t850, td850, moist='rk4'):
    """(Tp500, LCL pressure, status) of the parcel (850 hPa, T850, Td850)."""
    if np.isnan(t850) or np.isnan(td850):
        return NAN, NAN, 0
    with np.errstate(all='ignore'):
        l = po.lcl(850.0, t850, td850, per_column=True)
    pl, tl = l['lcl_pressure'], l['lcl_temperature']
    if np.isnan(pl):
        return NAN, NAN, ST_LCL_NOT_CONVERGED
    if pl <= 500.0:
        return t850 * (500.0 / 850.0) ** th.KAPPA, pl, 0
    return float(po.moist_lapse(np.array([500.0]), tl, pl, moist=moist)[0]), pl, 0


def ccl_line(p, t, td, depth=0.0):
    """Step 5 up to the crossings: (pv, tv, rt, crossings) with crossings a list of (pressure, rt) from the bottom up."""
    p, t, td = (np.asarray(x, dtype=np.float64) for x in (p, t, td))
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    pv, tv, tdv = p[ok], t[ok], td[ok]
    if pv.size == 0:
        return pv, tv, pv.copy(), []
    with np.errstate(all='ignore'):
        r = th.saturation_mixing_ratio(pv[0], tdv[0]) if depth == 0 else po.mixed_parcel(p, t, td, depth=depth)['mixing_ratio']
        rt = np.atleast_1d(th.dewpoint(th.vapor_pressure(pv, r))).astype(np.float64)
    if depth == 0:
        rt[0] = tdv[0]
    d, x = rt - tv, np.log(pv)
    out = []
    for i in range(pv.size - 1):
        d0, d1 = d[i], d[i + 1]
        if np.isnan(d0) or np.isnan(d1) or np.sign(d0) == np.sign(d1):
            continue
        if d0 == 0.0:
            out.append((float(pv[i]), float(rt[i])))
        elif d1 == 0.0:
            out.append((float(pv[i + 1]), float(rt[i + 1])))
        else:
            ix = (d1 * x[i] - d0 * x[i + 1]) / (d1 - d0)                                        # pf.py:1046
            iy = ((ix - x[i]) / (x[i + 1] - x[i])) * (rt[i + 1] - rt[i]) + rt[i]                # pf.py:1050
            out.append((float(np.exp(ix)), float(iy)))
    return pv, tv, rt, out


def column(p, t, td, u=None, v=None, moist='rk4', which='top', mixed_layer_depth=0.0):
    """One column (nlev,): dict of the nine outputs, 'status', and what the tests look at besides: the isobar values
    ('t850', 'td850', 't700', 'td700', 't500', 'u850', 'v850', 'u500', 'v500'), 'lcl_pressure' of the Showalter parcel,
    'parcel_500' (Tp500), 'sweat' (sweat_terms or None) and 'crossings'."""
    p, t, td = (np.asarray(x, dtype=np.float64) for x in (p, t, td))
    out = {k: NAN for k in KEYS}
    out.update(status=0, sweat=None, lcl_pressure=NAN, parcel_500=NAN)
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    pv, tv, tdv = p[ok], t[ok], td[ok]
    for P in (850, 700, 500):
        out['t%d' % P], out['td%d' % P] = at_isobar(float(P), pv, tv, tdv)
    span = spans(pv)
    wspan = False
    if u is not None:
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        wok = ~(np.isnan(p) | np.isnan(u) | np.isnan(v))
        for P in (850, 500):
            out['u%d' % P], out['v%d' % P] = at_isobar(float(P), p[wok], u[wok], v[wok])
        wspan = spans(p[wok])
    if span:
        vt, ct = out['t850'] - out['t500'], out['td850'] - out['t500']
        tt = vt + ct
        out.update(vertical_totals=vt, cross_totals=ct, total_totals=tt,
                   k_index=(vt + (out['td850'] - 273.15)) - (out['t700'] - out['td700']))
        tp, pl, st = showalter_parcel(out['t850'], out['td850'], moist)
        out.update(showalter_index=out['t500'] - tp, parcel_500=tp, lcl_pressure=pl)
        out['status'] |= st
        if wspan:
            out['sweat'] = sweat_terms(out['td850'], tt, out['u850'], out['v850'], out['u500'], out['v500'])
            out['sweat_index'] = out['sweat']['sweat_index']
    else:
        out['status'] |= ST_NO_LAYER
    pv, tv, rt, crossings = ccl_line(p, t, td, float(mixed_layer_depth or 0.0))
    out['crossings'] = crossings
    if crossings:
        cp, cy = crossings[-1] if which == 'top' else crossings[0]
        out.update(ccl_pressure=cp, ccl_temperature=cy, convective_temperature=cy * (pv[0] / cp) ** th.KAPPA)
    else:
        out['status'] |= ST_NO_CCL
    return out


def grid(p, t, td, u=None, v=None, cols=None, **kwargs):
    """column() for the columns `cols` (default: all) of (nlev, ncol) arrays: dict of (len(cols),) arrays of the nine outputs,
    'status', 'parcel_500', 'lcl_pressure' and the number of crossings 'n_crossings', plus the list of columns 'columns'."""
    cols = range(p.shape[1]) if cols is None else cols
    res = [column(p[:, c], t[:, c], td[:, c], None if u is None else u[:, c], None if v is None else v[:, c], **kwargs) for c in cols]
    out = {k: np.array([r[k] for r in res], dtype=np.float64) for k in KEYS + ('parcel_500', 'lcl_pressure')}
    out['status'] = np.array([r['status'] for r in res], dtype=np.int32)
    out['n_crossings'] = np.array([len(r['crossings']) for r in res])
    out['columns'] = res
    return out


def _rel_near(x, thr, tol):
    return abs(x - thr) <= tol * abs(thr)


def near_tie(p, t, td, u=None, v=None, mixed_layer_depth=0.0, col=None):
    """True where the column's outcome hangs on the last bits of a comparison: |rt - T| < 1e-6 K at a valid level other than a
    surface-mode start level; a SWEAT threshold quantity within 1e-9 (relative) of its threshold (dir500 - dir850 against 0:
    relative to the larger direction); the Showalter parcel's LCL pressure within 1e-9 (relative) of 500 hPa.
    col: the column's column() result, if the caller has it."""
    depth = float(mixed_layer_depth or 0.0)
    pv, tv, rt, _ = ccl_line(p, t, td, depth)
    d = np.abs(rt - tv)[(1 if depth == 0 else 0):]
    if np.any(d < 1e-6):
        return True
    r = column(p, t, td, u, v, mixed_layer_depth=depth) if col is None else col
    if not np.isnan(r['lcl_pressure']) and _rel_near(r['lcl_pressure'], 500.0, 1e-9):
        return True
    s = r['sweat']
    if s is not None:
        tol = 1e-9
        if (_rel_near(s['d850'], 130.0, tol) or _rel_near(s['d850'], 250.0, tol) or _rel_near(s['d500'], 210.0, tol) or
                _rel_near(s['d500'], 310.0, tol) or abs(s['d500'] - s['d850']) <= tol * max(s['d500'], s['d850']) or
                _rel_near(s['f850'], 15.0, tol) or _rel_near(s['f500'], 15.0, tol)):
            return True
    return False
