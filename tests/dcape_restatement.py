"""NumPy restatement of downdraft CAPE (metpy.calc.downdraft_cape, MetPy 1.4) as xp_downdraft_cape specifies it, one
column at a time, built from the oracle's pieces: Bolton theta_e and e_s (oracle.thermo), the per-column LCL and the
moist adiabat in 'rk4', 'ode' or 'table' mode (oracle.parcel_oracle).  The steps:
  1. levels where p, T or Td is NaN are dropped;
  2. the column has a layer if b <= max p and u >= min p (np.isclose counting), b = bottom, u = bottom - depth;
  3. the layer: levels with u <= p <= b (np.isclose counting), plus b and u where no layer level is close to them, T and
     Td there linear in ln p between the bracketing levels (MetPy's get_layer(..., interpolate=True));
  4. the start point: the first layer point (decreasing pressure) with the smallest theta_e (np.argmin);
  5. its wet bulb: the LCL, then the moist adiabat from the LCL back down to p0 (as test_wet_bulb_and_interp_vs_oracle);
  6. the parcel: the moist adiabat through (p0, wb0) on every level with p >= p0;
  7. Tv = T (w + eps) / (eps (1 + w)), w the saturation mixing ratio at Td (environment) or at the parcel temperature;
  8. DCAPE = -Rd * trapz(Tv_env - Tv_parcel, ln p)."""
import numpy as np

from oracle import parcel_oracle as po
from oracle import thermo as th

ST_LCL_NOT_CONVERGED, ST_NO_LAYER = 2, 16


def close(x, y):
    """np.isclose(x, y): |x - y| <= 1e-8 + 1e-5 |y|."""
    return abs(x - y) <= 1e-8 + 1e-5 * abs(y)


def _bound_point(x, p, t, td):
    """T and Td at pressure x, linear in ln p between the levels that bracket it (NaN without both)."""
    lo = np.nonzero(p > x)[0]
    hi = np.nonzero(p < x)[0]
    if lo.size == 0 or hi.size == 0:
        return np.nan, np.nan
    lo, hi = lo[-1], hi[0]
    f = (np.log(x) - np.log(p[hi])) / (np.log(p[lo]) - np.log(p[hi]))
    return t[hi] + (t[lo] - t[hi]) * f, td[hi] + (td[lo] - td[hi]) * f


def layer_points(p, t, td, bottom=700.0, depth=200.0):
    """Steps 1-3 on one column: (P, T, Td) of the layer points in order of decreasing pressure, or None (no layer)."""
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    p, t, td = (np.asarray(v, dtype=np.float64)[ok] for v in (p, t, td))
    b, u = float(bottom), float(bottom) - float(depth)
    if p.size == 0 or not ((b <= p.max() or close(b, p.max())) and (u >= p.min() or close(u, p.min()))):
        return None
    lay = np.array([(pk < b or close(pk, b)) and (pk > u or close(pk, u)) for pk in p], dtype=bool)
    P, T, TD = list(p[lay]), list(t[lay]), list(td[lay])
    if not any(close(b, pk) for pk in p[lay]):
        tb, tdb = _bound_point(b, p, t, td)
        P, T, TD = [b] + P, [tb] + T, [tdb] + TD
    if not any(close(u, pk) for pk in p[lay]):
        tu, tdu = _bound_point(u, p, t, td)
        P, T, TD = P + [u], T + [tu], TD + [tdu]
    return np.array(P), np.array(T), np.array(TD)


def theta_e_of_points(pts):
    return th.equivalent_potential_temperature(pts[0], pts[1], pts[2])


def _virt(p, t, x):
    es = th.saturation_vapor_pressure(x)
    w = th.EPSILON * es / (p - es)
    return t * (w + th.EPSILON) / (th.EPSILON * (1.0 + w))


def column(p, t, td, bottom=700.0, depth=200.0, moist='rk4'):
    """One column (nlev,): dict of dcape, start_pressure, start_temperature, status and parcel_temperature (nlev,)."""
    p, t, td = (np.asarray(v, dtype=np.float64) for v in (p, t, td))
    out = {'dcape': np.nan, 'start_pressure': np.nan, 'start_temperature': np.nan, 'status': 0,
           'parcel_temperature': np.full(p.shape, np.nan)}
    pts = layer_points(p, t, td, bottom, depth)
    if pts is None:
        out['status'] = ST_NO_LAYER
        return out
    i0 = int(np.argmin(theta_e_of_points(pts)))
    p0, t0, td0 = (float(v[i0]) for v in pts)
    lcl = po.lcl(p0, t0, td0, per_column=True)
    if np.isnan(lcl['lcl_pressure']) and not np.isnan(t0 + td0):
        out['status'] |= ST_LCL_NOT_CONVERGED
    wb0 = float(po.moist_lapse(np.array([p0]), lcl['lcl_temperature'], lcl['lcl_pressure'], moist=moist)[0])
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    down = np.nonzero(ok & (p >= p0))[0]
    tp = po.moist_lapse(p[down], wb0, p0, moist=moist) if down.size else np.zeros(0)
    d = _virt(p[down], t[down], td[down]) - _virt(p[down], tp, tp)
    lnp = np.log(p[down])
    out['dcape'] = -th.RD * float(np.sum(0.5 * (d[1:] + d[:-1]) * (lnp[1:] - lnp[:-1])))
    out['start_pressure'], out['start_temperature'] = p0, wb0
    out['parcel_temperature'][down] = tp
    return out


def grid(p, t, td, cols=None, bottom=700.0, depth=200.0, moist='rk4'):
    """column() for the columns `cols` (default: all) of (nlev, ncol) arrays: dict of (len(cols),) arrays and the
    (nlev, len(cols)) parcel_temperature."""
    cols = range(p.shape[1]) if cols is None else cols
    res = [column(p[:, c], t[:, c], td[:, c], bottom, depth, moist) for c in cols]
    out = {k: np.array([r[k] for r in res]) for k in ('dcape', 'start_pressure', 'start_temperature', 'status')}
    out['parcel_temperature'] = np.stack([r['parcel_temperature'] for r in res], axis=1)
    return out


def near_tie(p, t, td, bottom=700.0, depth=200.0, tol=1e-9):
    """True where a layer point other than the argmin has a theta_e within `tol` K of the minimum: which of the two the
    device picks hangs on the last bits of theta_e."""
    pts = layer_points(p, t, td, bottom, depth)
    if pts is None:
        return False
    th_e = theta_e_of_points(pts)
    i0 = int(np.argmin(th_e))
    if np.isnan(th_e[i0]):
        return False
    gap = np.abs(np.delete(th_e, i0) - th_e[i0])
    return bool(np.any(gap <= tol))
