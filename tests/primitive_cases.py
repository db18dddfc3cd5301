"""Deterministic inputs for the grid-scale tests of the array primitives (csrc/xp_primitives.hpp: insert_level,
find_intersections, trapz, trap_around_zeros, bound_pressure, get_layer, shift_out_nans, the two re-basings, interp1d) and
of the small per-element and per-column kernels (csrc/xp_kernels.hpp: k_wet_bulb, k_interp_level, k_interp_levels,
k_crossing_level, k_mixing_ratio, k_dewpoint_from_q): tests/test_gpu_primitive_grid.py runs them on the GPU in both
dtypes against oracle/parcel_oracle.py, tests/test_primitive_cases_cpu.py checks here, without a GPU, that every class
of column named below is present -- also after the inputs are rounded to float32 -- and that the oracles evaluate every
case.

Every builder is a pure function of its arguments (one seeded generator, drawn from in a fixed order) and returns
float64 arrays laid out (nlev, ncol).  Coordinates are multiples of 1/64 hPa (1/64 m, 1/64 of the unit of interp1d's
abscissa) and the quantised values multiples of 1/64 K, so that "exactly on a level", "exactly equal" and "exactly zero"
survive the rounding of the inputs to float32.  Column c of a builder belongs to the class CLASSES[c % len(CLASSES)]
of that builder ('cls' in its result); the last three classes of every column-wise builder are COMMON.

Wet bulb: every kind of element asked for passed the agreement check of the two CPU oracles
(test_primitive_cases_cpu.py::test_wet_bulb_oracles_agree), none was taken out of wet_bulb_elements().
"""
import numpy as np

from oracle import parcel_oracle as po
from tests import component_cases as cc
from xarray_parcel_amd import synth

GRID = (cc.NLEV, cc.NCOL)
SHAPES = (GRID,) + cc.SMALL_SHAPES
COMMON = ('nan_column', 'one_valid_level', 'nan_coords_inside')


def q64(x):
    return np.round(np.asarray(x, dtype=np.float64) * 64.0) / 64.0


def cls_of(case, classes, name):
    """The columns of class `name`."""
    return case['cls'] == classes.index(name)


def _classes(ncol, classes):
    return np.arange(ncol) % len(classes)


def _interior(rng, nlev):
    """A level with a neighbour on either side where the column has one: 1 ... nlev - 2."""
    return min(1 + int(rng.integers(max(nlev - 2, 1))), nlev - 1)


def _apply_common(name, rng, coord, others):
    """The COMMON classes on one column (views of it): NaN throughout; one valid level; NaN coordinates inside."""
    nlev = coord.shape[0]
    if name == 'nan_column':
        coord[:] = np.nan
        for a in others:
            a[:] = np.nan
    elif name == 'one_valid_level':
        keep = int(rng.integers(nlev))
        coord[np.arange(nlev) != keep] = np.nan
    elif name == 'nan_coords_inside' and nlev > 2:
        coord[_interior(rng, nlev)] = np.nan
        coord[_interior(rng, nlev)] = np.nan


def _sounding(nlev, ncol, seed):
    """Pressure (cc.pressures), temperature and dewpoint, all multiples of 1/64."""
    rng = np.random.default_rng(seed)
    p = cc.pressures(nlev, ncol, seed)
    t = q64(200.0 + 95.0 * (p / 1050.0) + 3.0 * rng.random((nlev, ncol)))
    td = q64(t - 0.5 - 20.0 * rng.random((nlev, ncol)))
    return rng, p, t, td


# ---- insert_level ------------------------------------------------------------------------------------------------------
INSERT_CLASSES = ('between', 'on_level', 'nan_level', 'below_bottom', 'above_top', 'fill_value') + COMMON
FILL = -999.0


def insert_level_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=711):
    """A dataset (pressure, temperature, dewpoint) and one new level per column."""
    rng, p, t, td = _sounding(nlev, ncol, seed)
    cls = _classes(ncol, INSERT_CLASSES)
    lev_p = np.empty(ncol)
    lev_t, lev_td = q64(rng.uniform(200.0, 300.0, ncol)), q64(rng.uniform(190.0, 290.0, ncol))
    for c in range(ncol):
        name = INSERT_CLASSES[cls[c]]
        k = int(rng.integers(max(nlev - 1, 1)))
        kn = min(k + 1, nlev - 1)
        lev_p[c] = 0.5 * (p[k, c] + p[kn, c]) if nlev > 1 else p[0, c] - 3.0           # a multiple of 1/128
        if name == 'on_level':
            lev_p[c] = p[k, c]
        elif name == 'nan_level':
            lev_p[c] = np.nan
        elif name == 'below_bottom':
            lev_p[c] = p[0, c] + 20.0
        elif name == 'above_top':
            lev_p[c] = p[-1, c] - 20.0
        elif name == 'fill_value':
            t[k, c] = FILL
            td[kn, c] = FILL
        _apply_common(name, rng, p[:, c], (t[:, c], td[:, c]))
    return {'pressure': p, 'temperature': t, 'dewpoint': td, 'level_pressure': lev_p, 'level_temperature': lev_t,
            'level_dewpoint': lev_td, 'cls': cls}


# ---- find_intersections / trapz / trap_around_zeros --------------------------------------------------------------------
CROSS_CLASSES = ('no_crossing', 'crossings_1', 'crossings_2', 'crossings_3', 'crossings_4', 'crossings_5', 'equal_one_level',
                 'equal_two_levels', 'adjacent_crossings', 'nan_a', 'nan_b', 'nan_x') + COMMON


def _signed(rng, nlev, cuts, first):
    """Differences with a sign change after every level in `cuts`, |value| a multiple of 0.25 in 0.25 ... 6."""
    mag = np.maximum(np.round(rng.uniform(0.25, 6.0, nlev) * 4.0) / 4.0, 0.25)
    d, s = np.empty(nlev), first
    for k in range(nlev):
        d[k] = s * mag[k]
        if k in cuts:
            s = -s
    return d


def crossing_profiles(nlev=cc.NLEV, ncol=cc.NCOL, seed=722):
    """x (pressure: decreasing, positive, so that log_x applies), a and b with a prescribed a - b (exact in float32 too:
    b is a multiple of 1/64 K below 512 K, a - b a multiple of 0.25 K).  'cuts': the intervals holding a sign change."""
    rng = np.random.default_rng(seed)
    x = cc.pressures(nlev, ncol, seed)
    b = q64(200.0 + 95.0 * (x / 1050.0))
    d = np.empty((nlev, ncol))
    a_nan, b_nan = np.zeros((nlev, ncol), dtype=bool), np.zeros((nlev, ncol), dtype=bool)
    cls = _classes(ncol, CROSS_CLASSES)
    ncuts = np.zeros(ncol, dtype=np.int64)
    for c in range(ncol):
        name = CROSS_CLASSES[cls[c]]
        first = 1.0 if rng.integers(2) else -1.0
        n = {'no_crossing': 0, 'adjacent_crossings': 2}.get(name, int(name[-1]) if name.startswith('crossings_') else 3)
        n = min(n, nlev - 1)
        cuts = sorted(rng.choice(nlev - 1, size=n, replace=False).tolist()) if n else []
        if name == 'adjacent_crossings' and nlev > 2:
            j = int(rng.integers(nlev - 2))
            cuts = [j, j + 1]
        col = _signed(rng, nlev, set(cuts), first)
        k = _interior(rng, nlev)
        if name == 'equal_one_level':
            col[k] = 0.0
        elif name == 'equal_two_levels':
            col[k] = col[min(k + 1, nlev - 1)] = 0.0
        elif name in ('nan_a', 'nan_b', 'nan_x') and cuts:
            j = cuts[0]                                    # the sign changes between levels j and j + 1
            m = j + 2 if j + 2 < nlev else max(j - 1, 0)   # the level next to that interval
            if name == 'nan_a':
                a_nan[m, c] = True
            elif name == 'nan_b':
                b_nan[m, c] = True
            else:
                x[m, c] = np.nan
        d[:, c] = col
        ncuts[c] = len(cuts)
        _apply_common(name, rng, x[:, c], ())
        if name == 'nan_column':
            a_nan[:, c] = b_nan[:, c] = True
    a = np.where(a_nan, np.nan, b + d)
    return {'x': x, 'a': a, 'b': np.where(b_nan, np.nan, b), 'diff': np.where(a_nan | b_nan, np.nan, d), 'cls': cls,
            'cuts': ncuts}


TRAPZ_CLASSES = ('both_signs', 'one_sign', 'nan_dat', 'nan_x', 'zero_area') + COMMON


def trapz_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=733):
    """dat (multiples of 0.25), x (pressure) and an interval mask that keeps about 70 %."""
    rng = np.random.default_rng(seed)
    x = cc.pressures(nlev, ncol, seed)
    dat = np.empty((nlev, ncol))
    cls = _classes(ncol, TRAPZ_CLASSES)
    for c in range(ncol):
        name = TRAPZ_CLASSES[cls[c]]
        n = 0 if name == 'one_sign' else min(1 + int(rng.integers(4)), nlev - 1)
        cuts = set(rng.choice(nlev - 1, size=n, replace=False).tolist()) if n else set()
        col = _signed(rng, nlev, cuts, 1.0 if rng.integers(2) else -1.0)
        k = _interior(rng, nlev)
        if name == 'nan_dat':
            col[k] = np.nan
        elif name == 'nan_x':
            x[k, c] = np.nan
        elif name == 'zero_area' and nlev > 1:
            col[k] = -col[k - 1]                           # the mean of the interval (k - 1, k) is exactly zero
        dat[:, c] = col
        _apply_common(name, rng, x[:, c], (dat[:, c],))
    mask = rng.random((max(nlev - 1, 0), ncol)) < 0.7
    return {'dat': dat, 'x': x, 'mask': mask, 'cls': cls}


# ---- bound_pressure / get_layer ----------------------------------------------------------------------------------------
LAYER_DEPTHS = (100.0, 300.0, 2000.0)
LAYER_CLASSES = ('bound_between', 'bound_on_level', 'bound_outside', 'top_on_level_100', 'top_on_level_300',
                 'max_not_at_0', 'plain') + COMMON


def layer_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=744):
    """A dataset and one bound per column.  'top_on_level_D': bottom pressure - D is exactly a level's pressure."""
    rng, p, t, td = _sounding(nlev, ncol, seed)
    cls = _classes(ncol, LAYER_CLASSES)
    bound = q64(rng.uniform(300.0, 1000.0, ncol)) + 1.0 / 256.0                        # on no level, in no middle
    for c in range(ncol):
        name = LAYER_CLASSES[cls[c]]
        k = int(rng.integers(max(nlev - 1, 1)))
        kn = min(k + 1, nlev - 1)
        if name == 'bound_between':
            bound[c] = 0.5 * (p[k, c] + p[kn, c])          # equally far from both: the larger pressure wins
        elif name == 'bound_on_level':
            bound[c] = p[kn, c]
        elif name == 'bound_outside':
            bound[c] = p[0, c] + 40.0 if c % 2 else p[-1, c] - 40.0
        elif name.startswith('top_on_level') and nlev > 2:
            depth = float(name.rsplit('_', 1)[1])
            p[0, c] = np.round(p[0, c] * 4.0) / 4.0
            top = p[0, c] - depth
            j = 1 + int(np.argmin(np.abs(p[1:, c] - top)))
            p[j, c] = top
            assert p[j - 1, c] > top and (j + 1 >= nlev or p[j + 1, c] < top)
        elif name == 'max_not_at_0' and nlev > 1:
            p[0, c] = p[1, c] - 5.0                        # level 1 carries the column's highest pressure
        _apply_common(name, rng, p[:, c], (t[:, c], td[:, c]))
    return {'pressure': p, 'temperature': t, 'dewpoint': td, 'bound': bound, 'cls': cls}


# ---- shift_out_nans ----------------------------------------------------------------------------------------------------
def shift_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=755):
    """Column c has c % (nlev + 1) leading NaN pressures (nlev of them: a NaN-only column); every third column has NaN
    pressures after its first valid level as well, which stay where they are."""
    rng, p, t, _ = _sounding(nlev, ncol, seed)
    lead = np.arange(ncol) % (nlev + 1)
    later = np.zeros(ncol, dtype=bool)
    for c in range(ncol):
        p[:lead[c], c] = np.nan
        if c % 3 == 0 and lead[c] + 2 < nlev:
            p[lead[c] + 1 + int(rng.integers(nlev - lead[c] - 1)), c] = np.nan
            later[c] = True
    return {'pressure': p, 'temperature': t, 'lead': lead, 'nan_later': later}


def shift_reference(x, name):
    """The reference's loop (pf.py:1714-1718) on a dict of (nlev, ncol) arrays."""
    x = {k: np.array(v, dtype=np.float64) for k, v in x.items()}
    nlev, ncol = x[name].shape
    for _ in range(nlev):
        first = np.isnan(x[name][0])
        if not first.any():
            break
        x = {k: np.where(first[None, :], np.concatenate([v[1:], np.full((1, ncol), np.nan)]), v) for k, v in x.items()}
    return x


# ---- from_most_unstable_parcel / mix_layer -----------------------------------------------------------------------------
REBASE = {'most_unstable': 300, 'mixed_layer': 100}


def rebase_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=766):
    """synth.columns without NaN, the lowest three dewpoints 25 K down: no column's most-unstable parcel sits there, so
    the grid-wide dropna removes those levels (and the mixed layer removes the levels every column mixes)."""
    p, t, td = synth.columns(nlev=nlev, ncol=ncol, seed=seed, nan_fraction=0.0, dtype=np.float64)
    p, t, td = q64(p), q64(t), q64(td)
    td[:3] -= 25.0
    assert np.all(np.diff(p, axis=0) < 0)
    return {'pressure': p, 'temperature': t, 'dewpoint': td}


def rebase_reference(p, t, td, mode):
    """from_most_unstable_parcel (pf.py:1517) / mix_layer (pf.py:1604) restated on the grid with the oracle's parcels:
    where + dropna(how='all') + shift_out_nans (+ the parcel underneath).  Returns the three profiles, the parcel
    (dict of per-column arrays) and the mask of surviving levels."""
    ncol = p.shape[1]
    with np.errstate(all='ignore'):
        if mode == 'most_unstable':
            par = [po.most_unstable_parcel(p[:, c], t[:, c], td[:, c], depth=REBASE[mode]) for c in range(ncol)]
            keep = p <= np.array([m['pressure'] for m in par])[None, :]
        else:
            par = [po.mixed_parcel(p[:, c], t[:, c], td[:, c], depth=REBASE[mode]) for c in range(ncol)]
            keep = p < (np.nanmax(p, axis=0) - REBASE[mode])[None, :]
    parcel = {k: np.array([float(m[k]) for m in par]) for k in ('pressure', 'temperature', 'dewpoint')}
    if mode == 'most_unstable':
        parcel['index'] = np.array([m['index'] for m in par])
    cols = {'pressure': np.where(keep, p, np.nan), 'temperature': np.where(keep, t, np.nan), 'dewpoint': np.where(keep, td, np.nan)}
    kept = ~np.all(np.stack([np.isnan(v) for v in cols.values()]), axis=(0, 2))
    cols = shift_reference({k: v[kept] for k, v in cols.items()}, 'pressure')
    if mode == 'mixed_layer':
        cols = {k: np.concatenate([parcel[k][None, :], v]) for k, v in cols.items()}
    return cols, parcel, kept


# ---- interp1d ----------------------------------------------------------------------------------------------------------
INTERP1D_CLASSES = ('inside', 'on_knot', 'nan_at', 'on_first', 'on_last', 'below_first', 'above_last')


def interp1d_cases(n=40, m=17, ncol=cc.NCOL, seed=777):
    """xp (n, ncol) strictly increasing, fp, and at (m, ncol) whose row 3 takes the column's class.  'xp_shared': one set
    of points for all columns (the col_stride 0 form)."""
    rng = np.random.default_rng(seed)
    xp = np.cumsum(1.0 / 64.0 + q64(rng.uniform(0.0, 4.0, (n, ncol))), axis=0)
    fp = q64(rng.normal(size=(n, ncol)) * 8.0)
    at = q64(rng.uniform(xp[0] + 1.0, xp[-1] - 1.0, (m, ncol))) + 1.0 / 256.0
    cls = _classes(ncol, INTERP1D_CLASSES)
    c = np.arange(ncol)
    name = np.array(INTERP1D_CLASSES)[cls]
    at[3, name == 'on_knot'] = xp[(c % (n - 2)) + 1, c][name == 'on_knot']
    at[3, name == 'nan_at'] = np.nan
    at[3, name == 'on_first'] = xp[0, name == 'on_first']
    at[3, name == 'on_last'] = xp[-1, name == 'on_last']
    at[3, name == 'below_first'] = xp[0, name == 'below_first'] - 2.5
    at[3, name == 'above_last'] = xp[-1, name == 'above_last'] + 2.5
    shared = np.ascontiguousarray(xp[:, 0])
    at_shared = at.copy()
    at_shared[3] = np.where(name == 'on_knot', shared[(c % (n - 2)) + 1], np.where(name == 'nan_at', np.nan, np.where(
        name == 'on_first', shared[0], np.where(name == 'on_last', shared[-1], np.where(
            name == 'below_first', shared[0] - 2.5, np.where(name == 'above_last', shared[-1] + 2.5, at[3]))))))
    at_shared = np.clip(at_shared, shared[0] - 3.0, shared[-1] + 3.0)
    return {'xp': xp, 'fp': fp, 'at': at, 'xp_shared': shared, 'at_shared': at_shared, 'cls': cls}


# ---- interp_level / interp_levels --------------------------------------------------------------------------------------
LEVEL_TARGET = 500.0
LEVEL_TARGETS = (850.0, LEVEL_TARGET, LEVEL_TARGET, 300.0)          # interp_levels: 1 ... 4 of these, one repeated
LEVEL_CLASSES = ('between', 'on_level', 'duplicate_mean', 'duplicate_one_nan', 'outside_below', 'outside_above',
                 'nan_coord_next') + COMMON


def level_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=788, target=LEVEL_TARGET):
    """Coordinates (pressure) and four variables, built around `target` (tests/bundle_cases.py asks for 850, 700 and 500
    hPa in turn): the class of a column says where that coordinate falls in it ('duplicate_one_nan': one of the two
    values is NaN, in variables 0 and 2 or in variables 1 and 3, alternating along the columns of the class).  'at' is the
    per-column form of the target: `target` itself, except in the classes 'between' (the exact middle of two levels) and
    the COMMON ones (a random coordinate)."""
    rng, p, t, td = _sounding(nlev, ncol, seed)
    z = q64(44330.0 * (1.0 - (p / 1013.25) ** 0.19))
    w = q64(rng.normal(size=(nlev, ncol)) * 10.0)
    cls = _classes(ncol, LEVEL_CLASSES)
    at = np.full(ncol, float(target))
    for c in range(ncol):
        name = LEVEL_CLASSES[cls[c]]
        j = int(np.argmin(np.abs(p[:, c] - target)))                       # the level nearest the target
        jn = min(j + 1, nlev - 1)
        if name == 'between':
            k = int(rng.integers(max(nlev - 1, 1)))
            at[c] = 0.5 * (p[k, c] + p[min(k + 1, nlev - 1), c])
        elif name in ('on_level', 'duplicate_mean', 'duplicate_one_nan'):
            p[j, c] = target
            if name != 'on_level':
                p[jn, c] = target                                            # two levels carry the coordinate
            if name == 'duplicate_one_nan':                                   # in two of the four variables, so that the
                n = c // len(LEVEL_CLASSES)                                   # variables of one call average different counts
                for v in ((t, z) if n % 2 else (td, w)):
                    v[j if n % 4 < 2 else jn, c] = np.nan
        elif name == 'outside_below':
            p[:, c] = q64(p[:, c] * 0.25 + 100.0)                            # every coordinate below the target
        elif name == 'outside_above':
            p[:, c] = q64(p[:, c] * 0.25 + (target + 100.0))                   # every coordinate above it
        elif name == 'nan_coord_next':
            below = np.nonzero(p[:, c] > target)[0]
            k = int(below[-1]) if below.size else 0                          # the last level below the target: its bracket
            p[max(k - 1, 0) if c % 2 else min(k + 2, nlev - 1), c] = np.nan
        else:
            at[c] = q64(rng.uniform(150.0, 1000.0))
        _apply_common(name, rng, p[:, c], ())
        if name == 'nan_column':
            for v in (t, td, z, w):
                v[:, c] = np.nan
    return {'coords': p, 'variables': (t, td, z, w), 'at': at, 'cls': cls}


# ---- crossing_level ----------------------------------------------------------------------------------------------------
CROSSING_VALUES = (273.15, 263.15, 0.0)
CROSSING_CLASSES = ('never', 'once', 'three_times', 'on_value', 'nan_between') + COMMON


def crossing_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=799, value=273.15, increasing=True):
    """x (a height, increasing, or a pressure, decreasing) and a = value + d with d a multiple of 0.25.  In 'on_value'
    one level holds `value` itself (exactly so in float32 only where `value` is a float32 number: 0.0 of the three)."""
    rng = np.random.default_rng(seed)
    p = cc.pressures(nlev, ncol, seed)
    x = q64(44330.0 * (1.0 - (p / 1013.25) ** 0.19)) if increasing else p
    assert nlev < 2 or np.all(np.diff(x, axis=0) != 0)
    a = np.empty((nlev, ncol))
    cls = _classes(ncol, CROSSING_CLASSES)
    for c in range(ncol):
        name = CROSSING_CLASSES[cls[c]]
        n = min({'never': 0, 'once': 1, 'three_times': 3, 'nan_between': 1}.get(name, 2), nlev - 1)
        cuts = sorted(rng.choice(nlev - 1, size=n, replace=False).tolist()) if n else []
        if name == 'nan_between' and nlev > 2:
            cuts = [int(rng.integers(nlev - 2))]
        col = value + _signed(rng, nlev, set(cuts), 1.0 if rng.integers(2) else -1.0)
        if name == 'on_value':
            col[_interior(rng, nlev)] = value
        elif name == 'nan_between' and nlev > 2:
            col[cuts[0] + 1] = np.nan                      # its neighbours have opposite signs
        a[:, c] = col
        _apply_common(name, rng, x[:, c], (a[:, c],))
    return {'x': x, 'a': a, 'cls': cls}


def crossing_reference(x, a, value):
    """crossing_level restated once: the smallest of find_intersections' all_intersect_x with the constant `value`."""
    x, a = np.asarray(x, dtype=np.float64), np.asarray(a, dtype=np.float64)
    out = np.full(x.shape[1], np.nan)
    with np.errstate(all='ignore'):
        for c in range(x.shape[1]):
            ix = po.find_intersections(x[:, c], a[:, c], np.full(x.shape[0], value))['all_intersect_x']
            ix = ix[~np.isnan(ix)]
            if ix.size:
                out[c] = ix.min()
    return out


# ---- wet_bulb_temperature ----------------------------------------------------------------------------------------------
WET_BULB_EXTRA = ('supersaturated', 'low_pressure', 'td_below_150')
WET_BULB_KINDS = tuple(dict.fromkeys(cc.LCL_KINDS_OF_PARCEL)) + WET_BULB_EXTRA
N_EXTRA = 168                                              # of each extra kind: 1337 + 3 * 168 = 1841 = 7 * 263


def wet_bulb_elements(seed=811):
    """The elements of cc.lcl_parcels() and N_EXTRA of each kind of WET_BULB_EXTRA -- outside the box in which lcl()
    takes its fast path -- in one fixed random order, so that a wavefront holds several kinds whichever way the
    elements are laid out.  1-D arrays of 1841 = 7 * 263 elements; 'kind' indexes WET_BULB_KINDS."""
    base = cc.lcl_parcels()
    rng = np.random.default_rng(seed)
    names = np.array(cc.LCL_KINDS_OF_PARCEL)[base['kind']]
    kind = [np.array([WET_BULB_KINDS.index(n) for n in names])]
    p, t, td = [base['pressure']], [base['temperature']], [base['dewpoint']]
    for name in WET_BULB_EXTRA:
        pe = 600.0 + 450.0 * rng.random(N_EXTRA)
        te = 235.0 + 70.0 * rng.random(N_EXTRA)
        tde = te - (0.5 + 20.0 * rng.random(N_EXTRA))
        if name == 'supersaturated':
            tde = te + 0.25 + 2.75 * rng.random(N_EXTRA)
        elif name == 'low_pressure':
            pe = 10.0 + 40.0 * rng.random(N_EXTRA)
            te = 200.0 + 40.0 * rng.random(N_EXTRA)
            tde = te - (2.0 + 20.0 * rng.random(N_EXTRA))
        else:
            tde = 110.0 + 39.0 * rng.random(N_EXTRA)
        p.append(pe), t.append(te), td.append(tde)
        kind.append(np.full(N_EXTRA, WET_BULB_KINDS.index(name)))
    order = rng.permutation(cc.NCOL + 3 * N_EXTRA)
    p, t, td, kind = (np.concatenate(v)[order] for v in (p, t, td, kind))
    return {'pressure': q64(p), 'temperature': q64(t), 'dewpoint': q64(td), 'kind': kind}


WET_BULB_LAYOUTS = ((1, 1841), (7, 263))


def wet_bulb_reference(o, p, t, td):
    """Normand's rule element by element with the oracle `o` (oracle.c_oracle, or cc.numpy_oracle()): lcl, then the
    moist adiabat from the LCL back to the element's pressure.  p, t, td: arrays of one shape."""
    import warnings
    out = np.full(p.shape, np.nan)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in np.ndindex(p.shape):
            l = o.lcl(float(p[i]), float(t[i]), float(td[i]))
            out[i] = np.asarray(o.moist_lapse(np.array([p[i]]), float(l['lcl_temperature']), float(l['lcl_pressure'])))[0]
    return out


# ---- mixing_ratio / dewpoint_from_specific_humidity --------------------------------------------------------------------
def humidity_cases(nlev=cc.NLEV, ncol=cc.NCOL, seed=822):
    """p, t, td and a specific humidity with NaNs (2 % each), q == 0 and q < 0."""
    rng, p, t, td = _sounding(nlev, ncol, seed)
    q = np.round((1e-4 + 0.02 * rng.random((nlev, ncol)) * (p / 1050.0) ** 3) * 2.0 ** 20) / 2.0 ** 20
    k, c = np.arange(nlev)[:, None], np.arange(ncol)[None, :]
    q[(k + 3 * c) % 17 == 3] = 0.0
    q[(k + 5 * c) % 19 == 4] = -1.0 / 8192.0
    for a in (p, t, td, q):
        a[rng.random((nlev, ncol)) < 0.02] = np.nan
    return {'pressure': p, 'temperature': t, 'dewpoint': td, 'specific_humidity': q}


# ---- the per-column oracle loops (shared by the CPU guard and the GPU tests) ---------------------------------------------
def per_column(fn, ncol):
    """fn(c) -> dict of arrays / array, for every column: stacked with the column axis last."""
    with np.errstate(all='ignore'):
        rows = [fn(c) for c in range(ncol)]
    if isinstance(rows[0], dict):
        return {k: np.stack([np.asarray(r[k], dtype=np.float64) for r in rows], axis=-1) for k in rows[0]}
    return np.stack([np.asarray(r, dtype=np.float64) for r in rows], axis=-1)


DATASET = ('pressure', 'temperature', 'dewpoint')


def ref_insert_level(d):
    return per_column(lambda c: po.insert_level({k: d[k][:, c] for k in DATASET}, {k: d['level_' + k][c] for k in DATASET}),
                      d['pressure'].shape[1])


def ref_find_intersections(x, a, b, log_x):
    zero = np.zeros(x.shape[0])
    return per_column(lambda c: po.find_intersections(x[:, c], a[:, c], zero if b is None else b[:, c], log_x=log_x), x.shape[1])


def ref_trapz(dat, x, mask, **kw):
    return per_column(lambda c: po.trapz(dat[:, c], x[:, c], mask=None if mask is None else mask[:, c], **kw), x.shape[1])


def ref_trap_around_zeros(x, y, log_x):
    """areas (2 nlev - 1, ncol) with x_from / x_to from pf.py:1276-1277, and the (nlev, ncol) mask with its last row True."""
    with np.errstate(all='ignore'):
        rows = [po.trap_around_zeros(x[:, c], y[:, c], log_x=log_x) for c in range(x.shape[1])]
    areas = {k: np.stack([a[k] for a, _ in rows], axis=-1) for k in ('area', 'x', 'dx')}
    areas['x_from'], areas['x_to'] = areas['x'] - areas['dx'] / 2, areas['x'] + areas['dx'] / 2
    mask = np.concatenate([np.stack([m for _, m in rows], axis=-1).reshape(x.shape[0] - 1, x.shape[1]),
                           np.ones((1, x.shape[1]), dtype=bool)])
    return areas, mask


def ref_bound_pressure(p, bound):
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), (p.shape[1],))
    return per_column(lambda c: po.bound_pressure(p[:, c], b[c]), p.shape[1])


def ref_get_layer(d, depth, interpolate):
    return per_column(lambda c: po.get_layer({k: d[k][:, c] for k in DATASET}, depth=depth, interpolate=interpolate),
                      d['pressure'].shape[1])


def ref_interp_level(coords, variable, at, log):
    a = np.broadcast_to(np.asarray(at, dtype=np.float64), (coords.shape[1],))
    fn = po.log_interp if log else po.linear_interp
    return per_column(lambda c: fn(variable[:, c], coords[:, c], a[c]), coords.shape[1])


def ref_interp1d(at, xp, fp):
    return np.stack([np.interp(at[:, c], xp if xp.ndim == 1 else xp[:, c], fp[:, c]) for c in range(at.shape[1])], axis=-1)
