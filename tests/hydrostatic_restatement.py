"""NumPy restatement of xp_hydrostatic_height, xp_geopotential_to_height and xp_height_to_geopotential as include/xparcel.h
specifies them, one column at a time, in MetPy's own terms (thickness_hydrostatic: the trapezoid of Tv over ln p; get_layer)
rather than the device's single streaming pass:
  1. levels where p, T or the supplied moisture is NaN are dropped (_valid); their height is NaN;
  2. Tv per valid level: T (w + eps) / (eps (1 + w)) with w = eps e_s(Td) / (p - e_s(Td)) from a dewpoint (oracle.thermo's
     Bolton formula), w = q / (1 - q) from a specific humidity, Tv = T without moisture;
  3. the first valid level whose pressure is not below the previous one's: ST_BAD_PRESSURE, heights from there upward NaN,
     every thickness NaN, no layer judged;
  4. heights: base at the lowest valid level, then z_b = z_a + (Rd / g) * (0.5 * (Tv_a + Tv_b)) * (x_a - x_b), x = ln p, level
     by level in that operation order;
  5. a layer's bounds pb, pt as in tests/thermo_layers_restatement.py (pressure kinds; an open top is the smallest valid
     pressure); its points: wind_layers_restatement.points_between -- MetPy's get_layer -- on (T, moisture), each linear in
     ln p at an added bound point (_log_point), Tv from the interpolated values; thickness: the same terms summed over
     consecutive points from 0;
  6. a layer with pt >= pb, pb > p0 or pt < min p: NaN, ST_NO_LAYER; a column without a valid level: all NaN, ST_NO_LAYER."""
import numpy as np

from oracle import thermo as O
from tests.kinematics_restatement import ST_BAD_PRESSURE, ST_NO_LAYER, _valid
from tests.wind_layers_restatement import PRESSURE, PRESSURE_DEPTH, points_between

RD = 287.04749097718457
G = 9.80665
EPS = 0.6219569100577033
RE = 6371008.7714               # metpy.constants.Re [m]
RD_G = RD / G
DRY, DEWPOINT, SPECIFIC = 'dry', 'dewpoint', 'specific'
__all__ = ['ST_BAD_PRESSURE', 'ST_NO_LAYER', 'PRESSURE', 'PRESSURE_DEPTH']


def virtual_temperature(p, t, m, kind):
    """Tv of points (p, T, moisture); kind: DRY, DEWPOINT or SPECIFIC."""
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if kind == DRY:
        return t.copy()
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        w = O.mixing_ratio(O.saturation_vapor_pressure(m), p) if kind == DEWPOINT else m / (1.0 - m)
        return t * (w + EPS) / (EPS * (1.0 + w))


def _running(x, tv, start):
    """start, then the trapezoid terms added one by one, in the header's operation order."""
    z = np.empty(len(x))
    acc = start
    for k in range(len(x)):
        if k:
            acc = acc + RD_G * (0.5 * (tv[k - 1] + tv[k])) * (x[k - 1] - x[k])
        z[k] = acc
    return z


def _bounds(kind, bottom, top, p):
    pb = p[0] if np.isnan(bottom) else float(bottom)
    if kind == PRESSURE:
        return pb, (float(p.min()) if np.isnan(top) else float(top))
    return pb, pb - float(top)


def column(p, t, m=None, kind=DRY, base=0.0, layers=()):
    """One column (nlev,); m: the moisture or None; layers: (kind, bottom, top) tuples by pressure, a NaN top with PRESSURE
    being the open one.  Returns a dict: 'height' (nlev,), 'thickness' (nlayer,), 'status', 'resolved' (nlayer,) bool and
    'nvalid', the number of valid levels."""
    nlev = len(p)
    out = {'height': np.full(nlev, np.nan), 'thickness': np.full(len(layers), np.nan), 'status': 0,
           'resolved': np.zeros(len(layers), bool), 'nvalid': 0}
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    m = np.zeros(nlev) if m is None or kind == DRY else np.asarray(m, dtype=np.float64)
    idx = np.nonzero(~(np.isnan(p) | np.isnan(t) | np.isnan(m)))[0]
    p, t, m = _valid(p, t, m)
    out['nvalid'] = int(p.size)
    if p.size == 0:
        out['status'] = ST_NO_LAYER
        return out
    bad = np.nonzero(~(p[1:] < p[:-1]))[0]
    n = bad[0] + 1 if bad.size else p.size                # the levels below the first one out of order
    tv = virtual_temperature(p[:n], t[:n], m[:n], kind)
    out['height'][idx[:n]] = _running(np.log(p[:n]), tv, float(base))
    if bad.size:
        out['status'] = ST_BAD_PRESSURE
        return out
    for j, (lk, bottom, top) in enumerate(layers):
        pb, pt = _bounds(lk, bottom, top, p)
        if not (pt < pb) or pb > p[0] or pt < p.min():
            out['status'] |= ST_NO_LAYER
            continue
        P, T, M = points_between(p, t, m, pb, pt)        # (sorted: pb first, pt last)
        out['thickness'][j] = _running(np.log(P), virtual_temperature(P, T, M, kind), 0.0)[-1]
        out['resolved'][j] = True
    return out


def grid(p, t, m=None, kind=DRY, base=None, layers=()):
    """column() for every column of (nlev, ncol) arrays; base: None or (ncol,).  Returns 'height' (nlev, ncol), 'thickness'
    (nlayer, ncol), 'status' (ncol,), 'resolved' (nlayer, ncol) and 'nvalid' (ncol,)."""
    ncol = p.shape[1]
    res = [column(p[:, c], t[:, c], None if m is None else m[:, c], kind, 0.0 if base is None else float(base[c]), layers)
           for c in range(ncol)]
    return {'height': np.stack([r['height'] for r in res], 1), 'thickness': np.stack([r['thickness'] for r in res], 1).reshape(len(layers), ncol),
            'status': np.array([r['status'] for r in res], dtype=np.int32), 'nvalid': np.array([r['nvalid'] for r in res]), 'resolved': np.stack([r['resolved'] for r in res], 1).reshape(len(layers), ncol)}


def geopotential_to_height(phi):
    phi = np.asarray(phi, dtype=np.float64)
    return (phi * RE) / (G * RE - phi)


def height_to_geopotential(z):
    z = np.asarray(z, dtype=np.float64)
    return (G * RE * z) / (RE + z)
