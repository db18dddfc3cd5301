"""The inputs of the XP_PARCEL_MAX_CAPE tests, shared by the census on the CPU (tests/test_max_cape_cpu.py) and the device
tests (tests/test_gpu_max_cape.py): synthetic grids whose best departure level often lies above the ground, and a set of
hand-built columns.  Every value is exact in float32, so the float32 and the float64 tests run on the same numbers.

The grids: synth.columns(nan_fraction=0.05) with
  - a nocturnal-style surface layer in ~60 % of the columns (hashed): the lowest 1 ... 5 levels are cooled, by 3 ... 12 K at
    level 0 tapering linearly to 0 at the layer's top, and the dewpoint is lowered by the same amount plus 0 or 2 K;
  - in ~40 % (hashed) the dewpoint of one candidate level aloft is raised, by bisection, until that level's theta-e leads the
    column's other candidates by 0.05 ... 0.65 K (where saturation allows it): the level of the most-unstable parcel, and
    not always the level with the largest CAPE."""
import functools

import numpy as np

from oracle import thermo as O
from tests import max_cape_restatement as R
from xarray_parcel_amd import synth

SEED = 20250718
DEPTH = 300.0
GRIDS = {'24x1337': (24, 1337), '40x640': (40, 640), '7x65': (7, 65), '2x130': (2, 130), '1x70': (1, 70)}
MAIN = '24x1337'
NAN = float('nan')


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _build(nlev, ncol):
    p, t, td = synth.columns(nlev, ncol, seed=SEED, nan_fraction=0.05)
    u = synth.column_uniforms(ncol, SEED + 4)
    k = np.arange(nlev)[:, None]
    # the cooled surface layer
    n = 1 + np.minimum((u[1] * 5).astype(np.int64), 4)                          # 1 ... 5 levels
    dt = (3.0 + 9.0 * u[2]) * np.clip(1.0 - k / n[None, :], 0.0, None) * (u[0] < 0.6)[None, :]
    t = t - dt
    td = td - dt - np.where(dt > 0, 2.0 * (u[3] < 0.5)[None, :], 0.0)
    # one candidate aloft with the column's highest theta-e
    cand = R.candidates(p, t, td, DEPTH)
    first = np.argmax(cand, axis=0)
    ncand = cand.sum(axis=0)
    pick = (u[4] < 0.4) & (ncand >= 2)
    rank = 1 + np.minimum((u[5] * (ncand - 1)).astype(np.int64), np.maximum(ncand - 2, 0))   # the rank-th candidate above the lowest
    order = np.cumsum(cand, axis=0) - 1
    level = np.argmax(cand & (order == rank[None, :]), axis=0)
    cols = np.nonzero(pick & (level > first))[0]
    if cols.size:
        lv = level[cols]
        with np.errstate(invalid='ignore'):
            th = np.where(cand[:, cols], O.equivalent_potential_temperature(p[:, cols], t[:, cols], td[:, cols]), -np.inf)
        th[lv, np.arange(cols.size)] = -np.inf
        target = th.max(axis=0) + 0.05 + 0.6 * u[6][cols]
        pk, tk = p[lv, cols], t[lv, cols]
        lo, hi = td[lv, cols].copy(), tk.copy()
        reach = O.equivalent_potential_temperature(pk, tk, hi) >= target       # saturation allows it
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            above = O.equivalent_potential_temperature(pk, tk, mid) >= target
            hi = np.where(above, mid, hi)
            lo = np.where(above, lo, mid)
        td[lv[reach], cols[reach]] = hi[reach]
    out = tuple(np.ascontiguousarray(_f32(x)) for x in (p, t, td))
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def grid(name=MAIN):
    """p, T, Td of the grid `name` (a key of GRIDS), float64 holding float32-exact values; read-only, shared."""
    return _build(*GRIDS[name])


@functools.lru_cache(maxsize=None)
def restated(name=MAIN, moist='rk4'):
    """tests.max_cape_restatement.max_cape_grid of grid(name) at DEPTH, computed once."""
    return R.max_cape_grid(*grid(name), depth=DEPTH, moist=moist)


def as_dtype(arrays, dtype):
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in arrays)


# -- hand-built columns ------------------------------------------------------------------------------------------------------
def sounding(t_sfc=303.0, td_sfc=296.0, moist_top=850.0, nlev=20, sfc_cool=0.0, sfc_levels=0):
    """20 levels from 1000 to 145 hPa: 6.8 K/km down to 210 K, a moist layer below `moist_top` hPa and dry air above;
    `sfc_cool` cools the lowest `sfc_levels` levels and dries them by as much."""
    p = 1000.0 - 45.0 * np.arange(nlev)
    z = 44330.8 * (1 - (p / 1013.25) ** 0.190263)
    t = np.maximum(t_sfc - 6.8e-3 * (z - z[0]), 210.0)
    td = np.where(p >= moist_top, td_sfc - 2.0e-3 * (z - z[0]), t - 15.0 - 10.0 * (moist_top - p) / moist_top)
    td = np.minimum(td, t - 0.5)
    t[:sfc_levels] -= sfc_cool
    td[:sfc_levels] -= sfc_cool
    return p, t, td


HAND = ('best_0', 'best_aloft', 'all_zero', 'nan_inside', 'all_nan', 'level0_invalid', 'one_level_window', 'whole_column')
# depth [hPa] of each, and what the rule gives (checked against the restatement in tests/test_max_cape_cpu.py)
HAND_DEPTH = {'one_level_window': 10.0, 'whole_column': 2000.0}
HAND_KSTAR = {'best_0': 0, 'best_aloft': 3, 'all_zero': 0, 'nan_inside': 3, 'all_nan': 0, 'level0_invalid': 1,
              'one_level_window': 0, 'whole_column': 3}


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> (p, T, Td) columns of 20 levels, float32-exact and read-only."""
    out = {}
    out['best_0'] = sounding(moist_top=990.0)                                     # the moist layer is level 0 alone
    out['best_aloft'] = sounding(sfc_cool=9.0, sfc_levels=3)                      # a cold pool under the moist layer
    out['all_zero'] = sounding(t_sfc=285.0, td_sfc=255.0)
    p, t, td = sounding(sfc_cool=9.0, sfc_levels=3)
    t[2] = NAN                                                                    # a NaN level inside the window
    out['nan_inside'] = (p, t, td)
    out['all_nan'] = tuple(np.full(20, NAN) for _ in range(3))
    p, t, td = sounding(moist_top=940.0)
    td[0] = NAN                                                                   # the column starts at level 1
    out['level0_invalid'] = (p, t, td)
    out['one_level_window'] = sounding(sfc_cool=9.0, sfc_levels=3)                # depth 10 hPa: level 0 alone
    out['whole_column'] = sounding(sfc_cool=9.0, sfc_levels=3)                    # depth 2000 hPa: every level
    out = {k: tuple(np.ascontiguousarray(_f32(a)) for a in v) for k, v in out.items()}
    for v in out.values():
        for a in v:
            a.flags.writeable = False
    return out


def hand_grid(names=HAND):
    """The hand-built columns `names` side by side as (20, len(names)) arrays (those that share the default depth unless named)."""
    cols = hand_built()
    return tuple(np.ascontiguousarray(np.stack([cols[n][i] for n in names], axis=1)) for i in range(3))
