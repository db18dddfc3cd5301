"""Deterministic inputs and the reference for the grid-scale tests of the product bundle (xp_conv_properties: k_conv_columns
and k_conv_finish in csrc/xp_bundle.hpp): tests/test_gpu_bundle_grid.py runs the bundle on the GPU in both dtypes against
level_reference() below, tests/test_bundle_cases_cpu.py checks here, without a GPU, that every class of column named below
is present -- also after the inputs are rounded to float32 -- and that the reference shows every outcome.

bundle_grid() is a pure function of its arguments (seeded generators, drawn from in a fixed order) and returns the nine
inputs of numpy_api.conv_properties as float64 arrays, (nlev, ncol), (nwind, ncol) and (ncol,).  Pressure, temperature,
height, the wind heights and the winds are multiples of 1/64, specific humidity is a multiple of 2 ** -22: every value is a
float32 number, so that "on a level", "duplicate" and "equal" survive the cast.  One exception: the level of the freezing
class 'on_value' holds 273.15 K, which is no float32 number -- that class is exact in float64 only, as in
primitive_cases.crossing_cases (after the cast the level sits 6e-6 K below the value and is an ordinary crossing).

Column c belongs to class AXIS[c % len(AXIS)] on each of five axes.  The axes' lengths (10, 7, 11, 13, 9: classes repeat
where an axis has fewer) are pairwise coprime, so every pair of classes of two axes occurs, at least every 143rd column.
    ISOBAR    primitive_cases.LEVEL_CLASSES around one of the isobars the bundle looks up, TARGETS[(c // 10) % 3]
    FREEZING  the temperature's sign against 273.15 K: the first five of primitive_cases.CROSSING_CLASSES; three of four
              'once' columns hold a warm, moist, unstable sounding (warm_columns), every other column stays within 6 K of
              273.15 K
    HUMIDITY  moist / q == 0, q < 0, q NaN at one level / q above saturation at one level
    HEIGHT    clean / NaN height at a level that brackets 700 or 500 hPa / NaN height at a level next to a 273.15 K crossing
    WIND      where 6000 m falls among the wind levels, NaN winds and the tie of the strict `>` of positive_shear
"""
import numpy as np

from oracle import parcel_oracle as po
from oracle import thermo as th
from tests import component_cases as cc
from tests import primitive_cases as pc

TARGETS = (850.0, 700.0, 500.0)
ISOBAR = pc.LEVEL_CLASSES                                               # 10
FREEZING = pc.CROSSING_CLASSES[:5] + ('once', 'three_times')            # 7
HUMIDITY = ('moist', 'q_zero', 'q_negative', 'q_nan', 'supersaturated', 'moist', 'moist', 'q_zero', 'moist', 'q_nan', 'moist')   # 11
HEIGHT = ('clean', 'nan_z_bracket', 'nan_z_crossing', 'clean', 'clean', 'nan_z_bracket', 'clean', 'clean', 'nan_z_crossing',
          'clean', 'clean', 'clean', 'clean')                           # 13
WIND = ('between', 'on_level', 'two_levels', 'above_top', 'below_bottom', 'nan_wind_bracket', 'nan_wind_height', 'nan_surface_wind',
        'equal_speed')                                                  # 9
AXES = {'isobar': ISOBAR, 'freezing': FREEZING, 'humidity': HUMIDITY, 'height': HEIGHT, 'wind': WIND}
NWIND = 9
SHEAR_HEIGHT = 6000.0
GRID_INPUTS = ('pressure', 'temperature', 'specific_humidity', 'height_asl')
WIND_INPUTS = ('wind_u', 'wind_v', 'wind_height_above_surface')
POINT_INPUTS = ('surface_wind_u', 'surface_wind_v')
INPUTS = GRID_INPUTS + WIND_INPUTS + POINT_INPUTS
SEED = 4711
Q_STEP = 2.0 ** -22


def qq(x):
    return np.round(np.asarray(x, dtype=np.float64) / Q_STEP) * Q_STEP


def cls_of(d, axis, name):
    """The columns of class `name` on `axis` (a class that an axis repeats: all of its places)."""
    return np.array([n == name for n in AXES[axis]])[d['cls_' + axis]]


def target_of(ncol):
    """The isobar the ISOBAR class of column c is built around."""
    return np.array(TARGETS)[(np.arange(ncol) // len(ISOBAR)) % len(TARGETS)]


def warm_columns(ncol):
    """The columns that hold the warm sounding: three of four of the freezing class 'once'."""
    col = np.arange(ncol)
    return (np.array(FREEZING)[col % len(FREEZING)] == 'once') & ((col // len(FREEZING)) % 4 != 3)


ORACLE_MAX = 200


def oracle_columns(d, ignore_nans=False):
    """Up to ORACLE_MAX of the columns whose pressure decreases strictly and holds no NaN -- what the full oracle is asked
    about: every warm column among them that reaches all three isobars (ISOBAR 'between' or 'on_level': the ones that can
    have a lapse rate, hence a SHIP), and a seeded random draw of the others (a plain stride over them meets only part of
    an axis whose length it shares a factor with: three of them, six of the nine wind classes).  With ignore_nans the
    columns with a NaN temperature or humidity (or q <= 0) in their lowest 250 hPa are left out: the parcels come from
    there, and the oracle's LCL iteration (scipy.optimize.fixed_point) raises on a NaN parcel instead of returning NaN;
    without ignore_nans such a column is blanked and not lifted at all."""
    p, ncol = d['pressure'], d['pressure'].shape[1]
    with np.errstate(invalid='ignore'):
        ok = ~np.isnan(p).any(axis=0) & np.all(np.diff(p, axis=0) < 0, axis=0)
        if ignore_nans:
            low = p > p[0] - 250.0
            ok &= ~((np.isnan(d['temperature']) | ~(d['specific_humidity'] > 0)) & low).any(axis=0)
    ok = np.nonzero(ok)[0]
    first = warm_columns(ncol) & (cls_of(d, 'isobar', 'between') | cls_of(d, 'isobar', 'on_level'))
    a, b = ok[first[ok]], ok[~first[ok]]
    rest = np.random.default_rng(SEED).permutation(b)[:max(ORACLE_MAX - a.size, 0)]
    return np.sort(np.concatenate([a, rest]))


def oracle_bundle(d, cols, ignore_nans):
    """po.conv_properties (RK4) on the float64 inputs, column by column: name -> array over `cols`."""
    o = inputs(d, np.float64)[1]
    po.set_moist_lapse('rk4')
    try:
        with np.errstate(all='ignore'):
            ref = [po.conv_properties(*(o[k][:, c] for k in GRID_INPUTS), o['surface_wind_u'][c], o['surface_wind_v'][c],
                                      *(o[k][:, c] for k in WIND_INPUTS), ignore_nans=ignore_nans) for c in cols]
    finally:
        po.set_moist_lapse('ode')
    return {k: np.array([x[k] for x in ref]).astype(bool if k == 'positive_shear' else np.float64) for k in ref[0]}


def _first_sign_change(d):
    """The first interval (k, k + 1) over which d changes sign, or None."""
    with np.errstate(invalid='ignore'):
        s = np.sign(d)
        k = np.nonzero(s[1:] * s[:-1] < 0)[0]
    return int(k[0]) if k.size else None


def bundle_grid(nlev=cc.NLEV, ncol=cc.NCOL, seed=SEED, nwind=None):
    nwind = (1 if nlev == 1 else NWIND) if nwind is None else nwind
    rng = np.random.default_rng(seed)
    col = np.arange(ncol)
    cls = {k: col % len(v) for k, v in AXES.items()}
    # ISOBAR: level_cases' own columns, built in turn around each isobar (one seed: the three share their draws, and differ
    # only in what a class does to a column); column c takes the one of its target.  Its temperature and dewpoint are only
    # read for their NaNs: where one of the two values at a duplicated pressure is missing
    tgt = target_of(ncol)
    lc = {t: pc.level_cases(nlev, ncol, seed, target=t) for t in TARGETS}
    pick = lambda f: np.select([tgt[None, :] == t for t in TARGETS], [f(lc[t]) for t in TARGETS])
    p = pick(lambda x: x['coords'])
    t_nan, td_nan = (np.isnan(pick(lambda x, i=i: x['variables'][i])) for i in (0, 1))
    z = pick(lambda x: x['variables'][2])
    z0 = pc.q64(44330.0 * (1.0 - (cc.pressures(nlev, ncol, seed) / 1013.25) ** 0.19))      # level_cases' height, before its NaNs
    assert nlev < 2 or np.all(np.diff(z0, axis=0) > 0)
    # duplicate_one_nan: level_cases takes temperature and height out together, or the humidity; here the NaN alternates
    # among temperature alone, height alone and the humidity
    one_nan = (cls['isobar'] == ISOBAR.index('duplicate_one_nan')) & ((col // len(ISOBAR)) % 2 == 1)
    t_only = one_nan & ((col // len(ISOBAR)) % 4 == 1)
    z = np.where(t_only[None, :], z0, z)
    t_nan &= ~(one_nan & ~t_only)[None, :]
    # FREEZING: temperature = 273.15 + d, d with the class's sign changes (primitive_cases._signed: |d| a multiple of 0.25 K
    # in 0.25 ... 6), rounded to 1/64 K -- which leaves every sign as it is
    d = np.empty((nlev, ncol))
    on_value = np.zeros((nlev, ncol), dtype=bool)
    for c in range(ncol):
        name = FREEZING[cls['freezing'][c]]
        n = min({'never': 0, 'once': 1, 'three_times': 3, 'nan_between': 1, 'on_value': 2}[name], nlev - 1)
        cuts = sorted(rng.choice(nlev - 1, size=n, replace=False).tolist()) if n else []
        if name == 'nan_between' and nlev > 2:
            cuts = [int(rng.integers(nlev - 2))]
        d[:, c] = pc._signed(rng, nlev, set(cuts), 1.0 if rng.integers(2) else -1.0)
        if name == 'on_value':
            on_value[pc._interior(rng, nlev), c] = True
        elif name == 'nan_between' and nlev > 2:
            t_nan[cuts[0] + 1, c] = True                                # its neighbours have opposite signs
    # WARM: three of four 'once' columns are a warm, moist, conditionally unstable sounding instead -- 293 ... 304 K at the
    # lowest level, 6.3 ... 7.8 K/km in the height above, so that the one crossing of 273.15 K is near 600 hPa; a mixing
    # ratio of 10.6 ... 14.0 g/kg in the lowest 120 hPa (SHIP's window is 11 ... 13.6), drying with the cube of the pressure
    # above.  The other columns stay within 6 K of 273.15 K at every level and are convectively dead: without these, no
    # parcel has CAPE worth the name, no storm proxy is ever True and SHIP is NaN everywhere
    warm = warm_columns(ncol)
    p0 = cc.pressures(nlev, ncol, seed)
    tw = pc.q64((293.0 + 11.0 * rng.random(ncol)) * (p0 / p0[0]) ** (0.19 * (6.3 + 1.5 * rng.random(ncol)) / 6.5))
    tw = np.maximum(tw, 216.0 - 0.25 * np.arange(nlev)[:, None])       # a tropopause of a kind: still decreasing, and q stays > 0
    d = np.where(warm[None, :], tw - 273.15, d)
    assert nlev < 2 or np.all((np.diff(np.sign(d[:, warm]), axis=0) != 0).sum(axis=0) == 1)
    t = np.where(on_value, 273.15, np.where(warm[None, :], tw, pc.q64(273.15 + d)))
    assert np.all(np.sign(t - 273.15) == np.where(on_value, 0.0, np.sign(d)))
    # HUMIDITY: q of a dewpoint 0.5 ... 20.5 K below the temperature (WARM: of the moist layer), then the class's level
    td = t - pc.q64(0.5 + 20.0 * rng.random((nlev, ncol)))
    ww = 1e-3 * (10.6 + 3.4 * rng.random(ncol)) * np.minimum(1.0, p0 / (p0[0] - 120.0)) ** 3
    ww = np.maximum(ww, 1e-5)
    td = np.where(warm[None, :], pc.q64(np.minimum(th.dewpoint(p0 * ww / (th.EPSILON + ww)), t - 0.5)), td)
    with np.errstate(invalid='ignore'):
        w = th.saturation_mixing_ratio(p, td)
        ws = th.saturation_mixing_ratio(p, t)
    q = qq(w / (1.0 + w))
    for c in range(ncol):
        name = HUMIDITY[cls['humidity'][c]]
        k = int(rng.integers(nlev))
        if name == 'q_zero':
            q[k, c] = 0.0
        elif name == 'q_negative':
            q[k, c] = -1.0 / 8192.0
        elif name == 'q_nan':
            q[k, c] = np.nan
        elif name == 'supersaturated' and not np.isnan(ws[k, c]):
            q[k, c] = qq(1.25 * ws[k, c] / (1.0 + ws[k, c])) + Q_STEP
    t = np.where(t_nan, np.nan, t)
    q = np.where(td_nan | np.isnan(p), np.nan, q)
    # HEIGHT
    for c in range(ncol):
        name = HEIGHT[cls['height'][c]]
        if name == 'nan_z_bracket':
            at = (700.0, 500.0)[(c // len(HEIGHT)) % 2]
            with np.errstate(invalid='ignore'):
                below = np.nonzero(p[:, c] >= at)[0]
            k = int(below[-1]) if below.size else 0                     # the last level at or below the isobar ...
            z[min(k + (c // (2 * len(HEIGHT))) % 2, nlev - 1), c] = np.nan   # ... or the one above it
        elif name == 'nan_z_crossing':
            k = _first_sign_change(d[:, c])
            k = int(rng.integers(nlev)) if k is None else k
            z[min(k + (c // len(HEIGHT)) % 2, nlev - 1), c] = np.nan
    # WIND: nwind levels at about 50 ... 9000 m above the surface
    wh = pc.q64(np.linspace(50.0, 9000.0, nwind)[:, None] + rng.uniform(0.0, 40.0, (1, ncol)))     # (no level within 300 m of 6000)
    wu = pc.q64(5.0 + wh * 2.5e-3 + rng.normal(0.0, 3.0, (nwind, ncol)))
    wv = pc.q64(-2.0 + wh * 1.0e-3 + rng.normal(0.0, 3.0, (nwind, ncol)))
    su, sv = pc.q64(rng.normal(2.0, 2.0, ncol)), pc.q64(rng.normal(0.0, 2.0, ncol))
    for c in range(ncol):
        name = WIND[cls['wind'][c]]
        j = int(np.argmin(np.abs(wh[:, c] - SHEAR_HEIGHT)))
        jn = min(j + 1, nwind - 1)
        lo = int(np.nonzero(wh[:, c] < SHEAR_HEIGHT)[0][-1])            # the bracket of 6000 m: levels lo, lo + 1
        m = min(lo + (c // len(WIND)) % 2, nwind - 1)
        if name in ('on_level', 'two_levels', 'equal_speed'):
            wh[j, c] = SHEAR_HEIGHT
            if name == 'two_levels':
                wh[jn, c] = SHEAR_HEIGHT
            elif name == 'equal_speed':                                 # |(3, 4) s| == |(5, 0) s| exactly: not `>`
                s = 1.0 + (c % 64) / 64.0
                wu[j, c], wv[j, c], su[c], sv[c] = 3.0 * s, 4.0 * s, (5.0 * s, 0.0)[(c // len(WIND)) % 2], (0.0, -5.0 * s)[(c // len(WIND)) % 2]
        elif name == 'above_top':
            wh[:, c] = pc.q64(wh[:, c] * 0.5)
        elif name == 'below_bottom':
            wh[:, c] += SHEAR_HEIGHT
        elif name == 'nan_wind_bracket':
            (wu, wv)[(c // (2 * len(WIND))) % 2][m, c] = np.nan
        elif name == 'nan_wind_height':
            wh[m, c] = np.nan
        elif name == 'nan_surface_wind':
            (su, sv)[(c // len(WIND)) % 2][c] = np.nan
    out = {'pressure': p, 'temperature': t, 'specific_humidity': q, 'height_asl': z, 'wind_u': wu, 'wind_v': wv,
           'wind_height_above_surface': wh, 'surface_wind_u': su, 'surface_wind_v': sv}
    for k, v in out.items():                                            # every value is a float32 number, but for 273.15 itself
        exact = (v.astype(np.float32).astype(np.float64) == v) | np.isnan(v)
        assert np.all(exact | (on_value & ~t_nan if k == 'temperature' else False)), k
    out.update({'cls_' + k: v for k, v in cls.items()})
    out['on_value'] = on_value & ~t_nan
    return out


def inputs(d, dtype):
    """(what the kernel is given, the same values in float64) of the nine inputs."""
    g, o = {}, {}
    for k in INPUTS:
        g[k], o[k] = cc.cast(d[k], dtype)
    return g, o


# ---- the reference: everything in the bundle that is not parcel lifting ------------------------------------------------------
LEVEL_OUT = ('temp_500', 'lapse_rate_700_500', 'freezing_level', 'melting_level', 'dci_plus_lifted_index', 'shear_u', 'shear_v',
             'shear_magnitude')


def wet_bulb_third(t, td):
    """pf.py:364-387 as the array expression evaluates on arrays of the data's own type: float32 data stay float32, one
    rounding per operation.  (po.wet_bulb_temperature_fast is this expression behind a cast to float64: the same for
    float64 data -- tests/test_bundle_cases_cpu.py holds the two together --, not for float32.)"""
    return t - (1 / 3) * (t - td)


def crossings(x, a, value=273.15):
    """How many crossings find_intersections reports between a and the constant, per column."""
    n = np.zeros(x.shape[1], dtype=np.int64)
    with np.errstate(all='ignore'):
        for c in range(x.shape[1]):
            ix = po.find_intersections(x[:, c], a[:, c], np.full(x.shape[0], value))['all_intersect_x']
            n[c] = int((~np.isnan(ix)).sum())
    return n


def level_reference(d, dtype, ignore_nans, dewpoint=None):
    """pf.py:1951-2100 without the parcels, column by column with the oracle's own functions, on the inputs rounded to
    `dtype`.  `dewpoint`: the (nlev, ncol) dewpoint the bundle works with -- float32: the library's own
    dewpoint_from_specific_humidity of the same inputs (that entry point is held to the oracle on its own grid, and the
    bundle's scratch dewpoint is by contract the same bits); None: the oracle's.  The per-point values that the kernels
    store in the data's type between k_conv_columns / interp_levels and k_conv_finish are rounded to it here.  Returns
    the LEVEL_OUT arrays (float64, not yet rounded to `dtype`), 'positive_shear', the mask 'valid' (pf.py:1976-1981) and,
    for the census, 'n_freezing' / 'n_melting': the crossings of either level."""
    o = inputs(d, dtype)[1]
    p, t, q, z = (o[k] for k in GRID_INPUTS)
    wu, wv, wh = (o[k] for k in WIND_INPUTS)
    ncol = p.shape[1]
    rd = lambda x: np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)
    with np.errstate(all='ignore'):
        td = th.dewpoint_from_specific_humidity(p, t, q) if dewpoint is None else np.asarray(dewpoint, dtype=np.float64)
        valid = ~(np.isnan(td).any(0) | np.isnan(p).any(0) | np.isnan(t).any(0) | np.isnan(q).any(0))
        wb = wet_bulb_third(t.astype(dtype), td.astype(dtype)).astype(np.float64)
        assert wb.shape == t.shape
        out = {k: np.full(ncol, np.nan) for k in LEVEL_OUT}
        pos = np.zeros(ncol, dtype=bool)
        for c in range(ncol):
            pc_, tc, tdc, zc = p[:, c], t[:, c], td[:, c], z[:, c]
            a850 = po.log_interp({'t': tc, 'td': tdc}, pc_, 850.0)
            a700 = po.log_interp({'t': tc, 'z': zc}, pc_, 700.0)
            a500 = po.log_interp({'t': tc, 'z': zc}, pc_, 500.0)
            t850, td850, t700, z700, t500, z500 = (rd(x) for x in (a850['t'], a850['td'], a700['t'], a700['z'], a500['t'], a500['z']))
            out['temp_500'][c] = t500
            out['lapse_rate_700_500'][c] = (t500 - t700) / (z500 / 1000 - z700 / 1000)                 # pf.py:2102
            out['dci_plus_lifted_index'][c] = (t850 - 273.15) + (td850 - 273.15)                       # pf.py:1830 + li
            out['freezing_level'][c] = po.freezing_level_height(tc, zc)
            out['melting_level'][c] = po.freezing_level_height(wb[:, c], zc)
            # wind_shear: the 6000 m wind is stored in the data's type; po.wind_shear then meets it as a one-level column
            hu, hv = rd(po.linear_interp(wu[:, c], wh[:, c], SHEAR_HEIGHT)), rd(po.linear_interp(wv[:, c], wh[:, c], SHEAR_HEIGHT))
            at = np.array([SHEAR_HEIGHT])
            s = po.wind_shear(o['surface_wind_u'][c], o['surface_wind_v'][c], np.array([hu]), np.array([hv]), at)
            for k in ('shear_u', 'shear_v', 'shear_magnitude'):
                out[k][c] = s[k]
            pos[c] = s['positive_shear']
    out['n_freezing'], out['n_melting'] = crossings(z, t), crossings(z, wb)
    if not ignore_nans:                                                 # out.where(valid_points), pf.py:2097-2098
        for k in LEVEL_OUT:
            out[k] = np.where(valid, out[k], np.nan)
        pos = pos & valid
    out['positive_shear'], out['valid'] = pos, valid
    return out
