"""The inputs of the XP_PARCEL_OVER_GROUND tests, shared by the census on the CPU (tests/test_ground_cpu.py) and the device
tests (tests/test_gpu_ground.py): one grid of 16 isobars x 1337 columns whose columns are, by construction, of every class
the re-basing rule distinguishes, a one-column grid and a two-level grid.  Every value is exact in float32, so the float32
and the float64 tests run on the same numbers."""
import functools

import numpy as np

from oracle import thermo as O
from tests import ground_restatement as R
from xarray_parcel_amd import synth

NLEV, NCOL, SEED = 16, 1337, 1337
ISOBARS = 1000.0 - 60.0 * np.arange(NLEV)                 # 1000 ... 100 hPa
# where the ground lies (k = a level index; k0 = the levels dropped):
CLASSES = ('below_all',      # ps above every level's pressure: nothing dropped, k0 = 0
           'between',        # p[k] > ps > p[k + 1] for every k = 0 ... 14: k0 = k + 1
           'on_level',       # ps == p[k] exactly, every k = 0 ... 15: that level is replaced by the surface, k0 = k + 1
           'above_top',      # ps below the top level's pressure: the surface alone, k0 = 16
           'nan_ps', 'nan_ts', 'nan_tds',      # one surface value NaN: the whole column NaN
           'nan_dropped',    # a NaN level (p, or T and Td, or all three) inside the dropped prefix: without effect
           'nan_above_t',    # T and Td NaN at the first level above the ground: kept, a missing level in row 1
           'nan_above_p',    # p NaN at the first level above the ground: compares false, so it is dropped too
           'saturated')      # Tds == Ts
NCLASS = len(CLASSES)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _environment(u, p):
    """synth's sounding formula on isobars: T and Td at the pressures p (nlev, ncol) of columns with the uniforms u."""
    t = (283.0 + 26.0 * u[1]) * (p / 1000.0) ** (synth.RD_OVER_G * (5.5 + 3.0 * u[2]) * 1e-3)
    t = np.maximum(t, 205.0) + (1.0 + 5.0 * u[4]) * (u[3] < 0.25) * np.exp(-((p - (800.0 + 100.0 * u[5])) / 25.0) ** 2)
    dd = 0.3 + 13.7 * u[6]
    return t, t - (dd + (30.0 - dd) * np.log(1000.0 / p) / np.log(1000.0 / synth.P_TOP))


def column_classes(ncol=NCOL):
    """(class index, index within the class) per column: the classes take turns, so every wavefront holds all of them."""
    c = np.arange(ncol)
    return c % NCLASS, c // NCLASS


def _build(isobars, ncol, seed):
    nlev = len(isobars)
    u = synth.column_uniforms(ncol, seed)
    cls, j = column_classes(ncol)
    is_ = lambda name: cls == CLASSES.index(name)
    p = np.ascontiguousarray(isobars[:, None] * np.ones((1, ncol)))
    t, td = _environment(u, p)
    step = isobars[0] - isobars[1]
    # the ground between levels k and k + 1 unless the class says otherwise
    k = (7 * j + cls) % (nlev - 1)
    k = np.where(is_('between'), j % (nlev - 1), k)
    if nlev > 2:
        k = np.where(is_('nan_dropped'), 1 + j % (nlev - 2), k)
    ps = isobars[k] - (0.1 + 0.8 * u[0]) * step
    ps = np.where(is_('below_all'), isobars[0] + 1.0 + 30.0 * u[0], ps)
    ps = np.where(is_('on_level'), isobars[j % nlev], ps)
    ps = np.where(is_('above_top'), isobars[-1] - 1.0 - 38.0 * u[0], ps)
    ps = _f32(ps)
    ts_env, tds_env = _environment(u, ps[None, :])
    ts = ts_env[0] + 0.5 + 3.0 * u[8]                         # a surface a little warmer than the free air at its pressure
    # (a plateau under the top level alone lifts into the isothermal stratosphere: only a hot one has an LFC)
    ts = ts + 25.0 * (is_('between') & (k == nlev - 2) & (nlev > 2))
    tds = ts - np.minimum(ts_env[0] - tds_env[0], 40.0 - 38.0 * (is_('between') & (k == nlev - 2)))
    tds = np.where(is_('saturated'), ts, tds)
    k0 = R.levels_below_ground(p, ps)
    cols = np.arange(ncol)
    for c in cols[is_('nan_dropped')]:
        kn, what = (j[c] // 3) % k0[c], j[c] % 3
        if what != 1:
            p[kn, c] = np.nan
        if what != 0:
            t[kn, c] = td[kn, c] = np.nan
    for c in cols[is_('nan_above_t')]:
        t[k0[c], c] = td[k0[c], c] = np.nan
    for c in cols[is_('nan_above_p')]:
        p[k0[c], c] = np.nan
    ps, ts, tds = (np.where(is_(name), np.nan, x) for name, x in (('nan_ps', ps), ('nan_ts', ts), ('nan_tds', tds)))
    out = tuple(np.ascontiguousarray(_f32(x)) for x in (p, t, td, ps, ts, tds))
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def grid():
    """p, T, Td (16, 1337) and ps, Ts, Tds (1337,), float64 holding float32-exact values; read-only, shared."""
    return _build(ISOBARS, NCOL, SEED)


@functools.lru_cache(maxsize=None)
def two_level_grid():
    """Two isobars (1000, 700 hPa) x 143 columns of the same classes (the NaN-in-the-prefix class has one level to drop)."""
    return _build(np.array([1000.0, 700.0]), 143, SEED + 2)


def one_column_grid(c=12):
    """Column c of grid() as a (16, 1) grid: by default a 'between' column with a level dropped."""
    return tuple(np.ascontiguousarray(a[..., c:c + 1]) for a in grid())


def as_dtype(arrays, dtype):
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in arrays)


def specific_humidity(p, td):
    """q = w / (1 + w) of the dewpoint's mixing ratio (NaN wherever p or Td is)."""
    w = O.mixing_ratio(O.saturation_vapor_pressure(td), p)
    return w / (1.0 + w)
