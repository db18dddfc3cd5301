"""NumPy restatement, in float64 and in the stated operation order, of xp_ncape and xp_ecape as include/xparcel.h specifies
them -- one column (or point) at a time, on arrays of the whole column rather than the device's single streaming pass:
  1. levels where p, T, Td or z is NaN are dropped; z0, p0 the lowest valid level, p_top the pressure of the highest;
  2. per valid level: q = w / (1 + w) with w = w_s(p, Td), qs likewise at T (Bolton's e_s), h = (cp T + Lv q) + g z,
     hs = (cp T + Lv qs) + g z, I = the running trapezoid integral of h over z from z0, hbar = I / (z - z0) (h at z0),
     b = -(g / (cp T)) (hbar - hs);
  3. the bounds: L NaN -> ncape 0.0, heights NaN; L, E non-NaN with E >= L -> NaN, ST_NO_LAYER; E NaN -> to the highest valid
     level; otherwise both clamped into [p_top, p0]; fewer than two valid levels -> NaN, ST_NO_LAYER;
  4. the levels read: up to and including the first valid level with p <= E, and at least two; on them pressures must decrease
     and heights increase strictly (else ST_BAD_PRESSURE / ST_BAD_HEIGHT, everything NaN);
  5. a bound between two levels: f = (ln pb - ln p) / (ln pp - ln p), z_b = z + f (zp - z), b_b = b + f (bp - b); a bound
     equal to a level's pressure is that level;
  6. ncape = trapz(b, z) over z_L, the levels strictly between, z_E; heights relative to z0.
ecape_value() is the per-point formula, element-wise on arrays."""
import numpy as np

RD = 287.04749097718457
EPS = 0.6219569100577033
CP_D = RD / (2.0 / 7.0)
LV = 2.50084e6
G = 9.80665
C_PSI = 82.87727046436741          # k^2 a^2 pi^2 Lmix / (4 Pr s^2): k = 0.42, a = 0.8, Lmix = 120 m, Pr = 1/3, s = 1.1
ST_BAD_PRESSURE, ST_NO_LAYER, ST_BAD_HEIGHT = 8, 16, 32
KEYS = ('ncape', 'lfc_height', 'el_height', 'status')


def sat_mix(p, t):
    """Saturation mixing ratio, Bolton (1980) e_s."""
    e = 6.112 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
    return EPS * e / (p - e)


def levels(p, t, td, z):
    """Steps 1 and 2 on one column: the valid levels' (p, z, h, hs, hbar, b)."""
    p, t, td, z = (np.asarray(a, dtype=np.float64) for a in (p, t, td, z))
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td) | np.isnan(z))
    p, t, td, z = p[ok], t[ok], td[ok], z[ok]
    w, ws = sat_mix(p, td), sat_mix(p, t)
    q, qs = w / (1.0 + w), ws / (1.0 + ws)
    h, hs = (CP_D * t + LV * q) + G * z, (CP_D * t + LV * qs) + G * z
    hbar = h.copy()
    acc = 0.0
    for k in range(1, p.size):
        acc += (0.5 * (h[k] + h[k - 1])) * (z[k] - z[k - 1])
        with np.errstate(divide='ignore', invalid='ignore'):
            hbar[k] = acc / (z[k] - z[0])
    b = -(G / (CP_D * t)) * (hbar - hs)
    return p, z, h, hs, hbar, b


def _bound(pb, p, z, b):
    """Step 5: (z_b, b_b) at pressure pb, p_top <= pb <= p0, on ordered levels."""
    on = np.nonzero(p == pb)[0]
    if on.size:
        return z[on[0]], b[on[0]]
    k = int(np.nonzero(p < pb)[0][0])                    # the level above; k - 1 the level below
    f = (np.log(pb) - np.log(p[k])) / (np.log(p[k - 1]) - np.log(p[k]))
    return z[k] + f * (z[k - 1] - z[k]), b[k] + f * (b[k - 1] - b[k])


def column(p, t, td, z, lfc_pressure, el_pressure):
    """One column (nlev,) and its two bounds: dict of KEYS."""
    out = {'ncape': np.nan, 'lfc_height': np.nan, 'el_height': np.nan, 'status': 0}
    L, E = float(lfc_pressure), float(el_pressure)
    if np.isnan(L):
        out['ncape'] = 0.0
        return out
    if not np.isnan(E) and E >= L:
        out['status'] = ST_NO_LAYER
        return out
    p, z, _, _, _, b = levels(p, t, td, z)
    if p.size:
        L, E = min(L, p[0]), (E if np.isnan(E) else min(E, p[0]))
        beyond = np.nonzero(p <= E)[0]                   # (a NaN E: none)
        n = min(max(int(beyond[0]) + 1, 2), p.size) if beyond.size else p.size
        bad_p, bad_z = np.nonzero(~(p[1:n] < p[:n - 1]))[0], np.nonzero(~(z[1:n] > z[:n - 1]))[0]
        if bad_p.size or bad_z.size:                     # the first level out of order is where reading stops
            first = min(np.r_[bad_p, bad_z])
            out['status'] = (ST_BAD_PRESSURE if first in bad_p else 0) | (ST_BAD_HEIGHT if first in bad_z else 0)
            return out
        p, z, b = p[:n], z[:n], b[:n]
    if p.size < 2:
        out['status'] = ST_NO_LAYER
        return out
    L = max(L, p[-1])                                    # clamped from above as well: p[-1] is p_top unless E ended the reading
    E = p[-1] if np.isnan(E) else max(E, p[-1])
    (zl, bl), (ze, be) = _bound(L, p, z, b), _bound(E, p, z, b)
    inside = (p < L) & (p > E)
    Z, B = np.r_[zl, z[inside], ze], np.r_[bl, b[inside], be]
    acc = 0.0
    for k in range(1, Z.size):
        acc += (0.5 * (B[k] + B[k - 1])) * (Z[k] - Z[k - 1])
    out.update(ncape=acc, lfc_height=zl - z[0], el_height=ze - z[0])
    return out


def grid(p, t, td, z, lfc_pressure, el_pressure, cols=None):
    """column() for the columns `cols` (default: all) of (nlev, ncol) arrays and (ncol,) bounds: dict of (len(cols),) arrays."""
    cols = range(p.shape[1]) if cols is None else cols
    res = [column(p[:, c], t[:, c], td[:, c], z[:, c], lfc_pressure[c], el_pressure[c]) for c in cols]
    return {k: np.array([r[k] for r in res], dtype=np.int32 if k == 'status' else np.float64) for k in KEYS}


def ecape_value(cape, ncape, el_height, sr_u, sr_v):
    """(ecape, ecape_a, psi) per point, element-wise on float64 arrays."""
    cape, ncape, H, su, sv = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (cape, ncape, el_height, sr_u, sr_v)))
    with np.errstate(all='ignore'):
        nan = np.isnan(cape) | np.isnan(ncape) | np.isnan(su) | np.isnan(sv) | ~(H > 0.0)
        psi = C_PSI / H
        sp = np.hypot(su, sv)
        V = np.where(sp > 1e-3, sp, 1e-3)
        V2 = V * V
        K, e = 0.5 * V2, psi / V2
        B = (1.0 + psi) + (2.0 * e) * ncape
        x = (8.0 * e) * (cape - psi * ncape)
        r = B * B + x
        s = np.sqrt(r)
        num = np.where(B >= 0.0, np.where(B + s == 0.0, 0.0, x / (B + s)), s - B)
        ea = K + num / (4.0 * e)
        ea = np.where(ea > 0.0, ea, 0.0)
        en = ea - K
        en = np.where(en > 0.0, en, 0.0)
        zero = (cape <= 0.0) | (r < 0.0)
        ea, en = np.where(zero, 0.0, ea), np.where(zero, 0.0, en)
    return tuple(np.where(nan, np.nan, a) for a in (en, ea, psi))
