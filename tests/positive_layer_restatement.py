"""NumPy restatement of the positive-layer choice of xp_cape_cin (xp_opts.flags, XP_OPT_LAYER_*) as include/xparcel.h
specifies it, built from the oracle only: oracle.c_oracle.cape_cin_grid(..., want_profile=True) gives every column's lifted
profile (the nodes, LCL included) and the default (envelope) result.  Per column the nodes are walked once:

  F+ / F-   the running sums of the positive / negative area of y = parcel - environment over ln p: an interval whose ends
            share a sign is a trapezoid, one with a valid zero two triangles around it (find_intersections' two
            expressions, pf.py:1046 / 1050, in ln p), anything with a NaN contributes nothing;
  events    an UP is an increasing crossing above the LCL (exp(x*) < p_lcl) in the selected set (every interval when
            env[0] != par[0], else every interval but the first: pf.py:1117-1120), a DOWN a decreasing one above the LCL that
            is not in the first interval; each carries its ln p, the parcel temperature there, its interval index and F+, F-
            after the triangle below it;
  layers    opened and closed by the events as the header says; a first DOWN closes a layer that began at the LCL -- unless
            it lies ON the LCL (within 2e-9 in ln p), where that layer would have no depth; a layer open after the last node
            ends at the lowest valid pressure with the final F+;
  choice    lowest / highest / deepest (ln L - ln E) / most_cape (cE - cL), the lower of equals, among K >= 2 layers;
            with K <= 1 every choice IS the oracle's default result.

column() returns K, every layer and the result of every choice; grid() does that for a grid and stacks the results."""
import numpy as np

from oracle import c_oracle
from oracle.thermo import RD

CHOICES = ('lowest', 'highest', 'deepest', 'most_cape')
FIELDS = ('cape', 'cin', 'lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature')
INDICES = ('lfc_index', 'el_index')
LCL_WINDOW = 2e-9       # in ln p: a DOWN this close to the LCL with no layer open closes nothing (a layer of no depth)


def walk(p, par, env, lcl_p):
    """The nodes of one column -> (events, sums at the LCL node, final F+, lowest valid pressure).  events: a list of
    dicts kind ('up' | 'down'), x (ln p), t, index, fp, fn."""
    n = len(p)
    with np.errstate(invalid='ignore', divide='ignore'):
        x = np.log(p)
    y = par - env
    use_all = bool(env[0] != par[0])
    fp = fn = 0.0
    at_lcl = (0.0, 0.0)
    events = []

    def add(a):
        nonlocal fp, fn
        if a > 0:
            fp += a
        elif a < 0:
            fn += a

    for i in range(n - 1):
        y0, y1 = y[i], y[i + 1]
        same = (y0 * y1 > 0) or (y0 == 0 and y1 == 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            trapezoid = abs(x[i + 1] - x[i]) * ((y0 + y1) * 0.5)
            if same:
                add(trapezoid)
            else:
                xs = (y1 * x[i] - y0 * x[i + 1]) / (y1 - y0)                      # pf.py:1046
                frac = (xs - x[i]) / (x[i + 1] - x[i])
                if np.isnan(frac * (y1 - y0) + y0):                               # no valid zero: the plain trapezoid (NaN: nothing)
                    add(trapezoid)
                else:
                    add((y0 * 0.5) * abs(x[i] - xs))
                    ts = frac * (par[i + 1] - par[i]) + par[i]                    # pf.py:1050
                    above = np.exp(xs) < lcl_p
                    if y1 > 0 and (use_all or i >= 1) and above:
                        events.append(dict(kind='up', x=xs, t=ts, index=i, fp=fp, fn=fn))
                    if y1 < 0 and i >= 1 and above:
                        events.append(dict(kind='down', x=xs, t=ts, index=i, fp=fp, fn=fn))
                    add((y1 * 0.5) * abs(x[i + 1] - xs))
        if p[i + 1] == lcl_p:
            at_lcl = (fp, fn)
    if n and p[0] == lcl_p:
        at_lcl = (0.0, 0.0)
    valid = p[~np.isnan(p)]
    return events, at_lcl, fp, (valid.min() if valid.size else np.nan)


def layers_of(events, at_lcl, fp_final, min_p, lcl_p, lcl_t):
    """The positive layers, bottom up: dicts L, xL, tL, iL, cL, nL, E, xE, tE, iE, cE, open."""
    layers, bottom = [], None
    for e in events:
        if e['kind'] == 'up':
            if bottom is None:
                bottom = dict(L=float(np.exp(e['x'])), xL=e['x'], tL=e['t'], iL=e['index'], cL=e['fp'], nL=e['fn'])
        else:
            if bottom is None and (layers or abs(e['x'] - np.log(lcl_p)) <= LCL_WINDOW):
                continue
            if bottom is None:
                bottom = dict(L=lcl_p, xL=float(np.log(lcl_p)), tL=lcl_t, iL=-2, cL=at_lcl[0], nL=at_lcl[1])
            layers.append(dict(bottom, E=float(np.exp(e['x'])), xE=e['x'], tE=e['t'], iE=e['index'], cE=e['fp'], open=False))
            bottom = None
    if bottom is not None:
        layers.append(dict(bottom, E=min_p, xE=float(np.log(min_p)), tE=np.nan, iE=-1, cE=fp_final, open=True))
    return layers


def metric(choice, k, lay):
    return {'lowest': -float(k), 'highest': float(k), 'deepest': lay['xL'] - lay['xE'], 'most_cape': lay['cE'] - lay['cL']}[choice]


def choose(layers, choice):
    """The index of the chosen layer: the first, replaced on a strictly greater metric only."""
    best, best_m = 0, metric(choice, 1, layers[0])
    for k, lay in enumerate(layers[1:], start=2):
        m = metric(choice, k, lay)
        if m > best_m:
            best, best_m = k - 1, m
    return best


def result(lay, post_zero_cin=False):
    cin = RD * lay['nL']
    if post_zero_cin and not cin <= 0.0:
        cin = 0.0
    return {'cape': RD * (lay['cE'] - lay['cL']) if lay['E'] < lay['L'] else 0.0, 'cin': cin,
            'lfc_pressure': lay['L'], 'lfc_temperature': lay['tL'], 'lfc_index': lay['iL'],
            'el_pressure': np.nan if lay['open'] else lay['E'], 'el_temperature': lay['tE'], 'el_index': lay['iE']}


def column(p, par, env, lcl_p, lcl_t, default, post_zero_cin=False):
    """One lifted profile and the oracle's default result for it (a dict of FIELDS + INDICES) -> dict: 'K', 'layers',
    'events', 'picked' (choice -> layer number from 0, -1 where K <= 1) and per choice the result."""
    out = {'K': 0, 'layers': [], 'events': [], 'picked': {c: -1 for c in CHOICES}}
    if not np.isnan(lcl_p):
        events, at_lcl, fp_final, min_p = walk(p, par, env, lcl_p)
        out['events'] = events
        out['layers'] = layers_of(events, at_lcl, fp_final, min_p, lcl_p, lcl_t)
        out['K'] = len(out['layers'])
    for c in CHOICES:
        if out['K'] >= 2:
            out['picked'][c] = choose(out['layers'], c)
            out[c] = result(out['layers'][out['picked'][c]], post_zero_cin)
        else:
            out[c] = {k: default[k] for k in FIELDS + INDICES}
    return out


def grid(p, t, td, vtc=True, **opts):
    """(nlev, ncol) arrays -> dict: 'oracle' (cape_cin_grid's own result, profile included), 'K' (ncol,), 'columns' (the
    column() dicts) and per choice a dict of (ncol,) arrays FIELDS + INDICES + 'picked'.
    opts: cape_cin_grid's (parcel, depth, moist, parcel_values, lcl_interp, post_zero_cin, ...)."""
    p, t, td = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    r = c_oracle.cape_cin_grid(p, t, td, want_profile=True, virtual_temperature_correction=vtc, **opts)
    prof = r['profile']
    P = prof['pressure']
    PAR = prof['virtual_temperature' if vtc else 'temperature']
    ENV = prof['environment_virtual_temperature' if vtc else 'environment_temperature']
    lcl_t = r['lcl_virtual_temperature' if vtc else 'lcl_temperature']
    ncol = p.shape[1]
    cols = []
    for j in range(ncol):
        default = {k: r[k][j] for k in FIELDS + INDICES}
        cols.append(column(P[:, j], PAR[:, j], ENV[:, j], r['lcl_pressure'][j], lcl_t[j], default, bool(opts.get('post_zero_cin', False))))
    out = {'oracle': r, 'K': np.array([c['K'] for c in cols]), 'columns': cols}
    for ch in CHOICES:
        out[ch] = {k: np.array([c[ch][k] for c in cols], dtype=np.int32 if k in INDICES else np.float64) for k in FIELDS + INDICES}
        out[ch]['picked'] = np.array([c['picked'][ch] for c in cols])
    return out
