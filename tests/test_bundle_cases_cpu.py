"""CPU guard of tests/bundle_cases.py (no GPU): bundle_grid() is deterministic; every class of every axis is present in
numbers and is what its name says, every pair of classes of two axes occurs, in float64 and after the inputs are rounded
to float32; and the reference of tests/test_gpu_bundle_grid.py shows every outcome the GPU test is meant to see -- finite
and NaN values per class, zero, one and several crossings, both values of positive_shear, blanked and kept columns -- on
the full grid, and evaluates the small shapes."""
import functools
import itertools

import numpy as np
import pytest

from oracle import parcel_oracle as po
from tests import bundle_cases as bc
from tests import component_cases as cc
from tests import primitive_cases as pc
from tests.test_component_cases_cpu import _same

DTYPES = (np.float64, np.float32)
both = pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: d.__name__)
MIN_CLASS, MIN_PAIR = 30, 3


@functools.lru_cache(maxsize=None)
def _grid(shape=pc.GRID):
    return bc.bundle_grid(*shape)


@functools.lru_cache(maxsize=None)
def _cast(dtype, shape=pc.GRID):
    """The grid as the oracle sees it when the kernel is given `dtype`, with the class arrays."""
    d = _grid(shape)
    return {**d, **bc.inputs(d, dtype)[1]}


@functools.lru_cache(maxsize=None)
def _ref(dtype, ignore_nans, shape=pc.GRID):
    return bc.level_reference(_grid(shape), dtype, ignore_nans)


def test_grid_is_deterministic_and_has_the_shapes_asked_for():
    assert _same(bc.bundle_grid(), bc.bundle_grid())
    for shape in pc.SHAPES:
        d = _grid(shape)
        nwind = 1 if shape[0] == 1 else bc.NWIND
        assert all(d[k].shape == shape for k in bc.GRID_INPUTS) and all(d[k].shape == (nwind, shape[1]) for k in bc.WIND_INPUTS)
        assert all(d[k].shape == (shape[1],) for k in bc.POINT_INPUTS)
        assert all(d[k].dtype == np.float64 for k in bc.INPUTS)
    lens = [len(v) for v in bc.AXES.values()]
    assert all(np.gcd(a, b) == 1 for a, b in itertools.combinations(lens, 2)), 'axis lengths must be pairwise coprime'


@both
def test_every_value_is_a_float32_number_but_the_on_value_level(dtype):
    d = _grid()
    for k in bc.INPUTS:
        same = (d[k].astype(np.float32).astype(np.float64) == d[k]) | np.isnan(d[k])
        assert np.all(same | (d['on_value'] if k == 'temperature' else False)), k
    assert d['on_value'].sum() >= MIN_CLASS and np.all(d['temperature'][d['on_value']] == 273.15)
    q = d['specific_humidity']
    assert np.array_equal(np.round(q / bc.Q_STEP) * bc.Q_STEP, q, equal_nan=True)
    for k in ('pressure', 'height_asl') + bc.WIND_INPUTS + bc.POINT_INPUTS:
        assert np.array_equal(pc.q64(d[k]), d[k], equal_nan=True), k
    c = _cast(dtype)
    if dtype == np.float32:                                             # 273.15 rounds to 273.149994: below the value, as the docstring says
        assert np.all(c['temperature'][d['on_value']] < 273.15)


@both
def test_census_of_classes_and_pairs(dtype):
    d = _cast(dtype)
    for ax, names in bc.AXES.items():
        for n in set(names):
            assert bc.cls_of(d, ax, n).sum() >= MIN_CLASS, (ax, n)
    for a, b in itertools.combinations(bc.AXES, 2):
        for na, nb in itertools.product(set(bc.AXES[a]), set(bc.AXES[b])):
            assert (bc.cls_of(d, a, na) & bc.cls_of(d, b, nb)).sum() >= MIN_PAIR, (a, na, b, nb)
    # each isobar class around each of the three isobars
    tgt = bc.target_of(cc.NCOL)
    for n in bc.ISOBAR:
        for t in bc.TARGETS:
            assert (bc.cls_of(d, 'isobar', n) & (tgt == t)).sum() >= MIN_CLASS, (n, t)


@both
def test_isobar_classes_are_what_they_say(dtype):
    d = _cast(dtype)
    p, t, q, z = (d[k] for k in bc.GRID_INPUTS)
    tgt = bc.target_of(cc.NCOL)
    cls = lambda n: bc.cls_of(d, 'isobar', n)
    with np.errstate(invalid='ignore'):
        on = (p == tgt[None, :]).sum(axis=0)
        below, above = (p > tgt[None, :]).sum(axis=0), (p < tgt[None, :]).sum(axis=0)
    valid = (~np.isnan(p)).sum(axis=0)
    assert np.all(on[cls('between')] == 0) and np.all(below[cls('between')] > 0) and np.all(above[cls('between')] > 0)
    assert np.all(on[cls('on_level')] == 1) and np.all(on[cls('duplicate_mean')] == 2) and np.all(on[cls('duplicate_one_nan')] == 2)
    assert np.all(below[cls('outside_below')] == 0) and np.all(above[cls('outside_above')] == 0)
    assert np.all(valid[cls('nan_column')] == 0) and np.all(valid[cls('one_valid_level')] == 1)
    assert np.all(valid[cls('nan_coord_next')] == cc.NLEV - 1)
    n_nan = cc.NLEV - valid[cls('nan_coords_inside')]
    assert np.all((n_nan >= 1) & (n_nan <= 2))
    # a column that does not reach an isobar, for each of the three (terrain above 850 hPa among them)
    with np.errstate(invalid='ignore'):
        for at in bc.TARGETS:
            assert ((p >= at).sum(axis=0)[valid > 1] == 0).sum() >= MIN_CLASS and ((p <= at).sum(axis=0)[valid > 1] == 0).sum() >= MIN_CLASS, at
    # duplicate_one_nan: at one of the two levels on the isobar exactly one of T, q, z is NaN, each of them in turn
    sel = np.nonzero(cls('duplicate_one_nan'))[0]
    who = []
    for c in sel:
        k = np.nonzero(p[:, c] == tgt[c])[0]
        nans = np.array([np.isnan(v[k, c]) for v in (t, q, z)])        # (variable, the two levels)
        # (the other axes put NaNs of their own on some of these levels: count the columns where the class's is alone)
        if nans.sum() == 1:
            who.append(int(np.nonzero(nans.any(axis=1))[0][0]))
    assert all(who.count(v) >= 10 for v in range(3)), [who.count(v) for v in range(3)]
    # duplicate_mean: two different values to average, in T and in z
    sel = cls('duplicate_mean')
    k = np.argmax(p == tgt[None, :], axis=0)
    c = np.arange(cc.NCOL)
    assert (t[k, c] != t[k + 1, c])[sel].sum() >= MIN_CLASS and np.all((z[k, c] != z[k + 1, c])[sel])


@both
def test_freezing_humidity_height_and_wind_classes_are_what_they_say(dtype):
    d = _cast(dtype)
    p, t, q, z = (d[k] for k in bc.GRID_INPUTS)
    wu, wv, wh = (d[k] for k in bc.WIND_INPUTS)
    f64 = dtype == np.float64
    with np.errstate(invalid='ignore'):
        s = np.sign(t - 273.15)
        change = (s[1:] * s[:-1] < 0).sum(axis=0)
    nan_t = np.isnan(t).any(axis=0)
    for name, n in (('never', 0), ('once', 1), ('three_times', 3)):
        sel = bc.cls_of(d, 'freezing', name) & ~nan_t
        assert sel.sum() >= MIN_CLASS and np.all(change[sel] == n), name
    sel = bc.cls_of(d, 'freezing', 'on_value')
    assert np.all((s == 0).sum(axis=0)[sel & ~nan_t] == (1 if f64 else 0)) and (s == 0).sum() == (d['on_value'].sum() if f64 else 0)
    alone = bc.cls_of(d, 'freezing', 'nan_between') & (np.isnan(t).sum(axis=0) == 1)      # (the isobar axis has NaNs of its own)
    assert alone.sum() >= MIN_CLASS
    for c in np.nonzero(alone)[0]:
        j = int(np.nonzero(np.isnan(t[:, c]))[0][0])
        assert 0 < j < cc.NLEV - 1 and s[j - 1, c] * s[j + 1, c] < 0, c
    # the height increases strictly wherever it is there
    for c in range(cc.NCOL):
        zc = z[:, c][~np.isnan(z[:, c])]
        assert np.all(np.diff(zc) > 0)
    # humidity
    with np.errstate(invalid='ignore'):
        ws = bc.th.saturation_mixing_ratio(p, t)
        over = q > ws / (1.0 + ws)
    for name, hit in (('q_zero', q == 0.0), ('q_negative', q < 0.0), ('supersaturated', over)):
        sel = bc.cls_of(d, 'humidity', name)
        assert (hit.sum(axis=0)[sel] == 1).sum() >= MIN_CLASS and hit[:, ~sel].sum() == 0, name
    clean = ~np.isnan(p).any(axis=0) & (bc.cls_of(d, 'isobar', 'duplicate_one_nan') == 0)
    assert np.all(np.isnan(q).sum(axis=0)[bc.cls_of(d, 'humidity', 'q_nan') & clean] == 1)
    assert np.all(np.isnan(q).sum(axis=0)[~bc.cls_of(d, 'humidity', 'q_nan') & clean] == 0)
    # height: NaNs only where the two classes (and the isobar axis) put them
    nz = np.isnan(z).sum(axis=0)
    iso = bc.cls_of(d, 'isobar', 'duplicate_one_nan') | bc.cls_of(d, 'isobar', 'nan_column')
    assert np.all(nz[bc.cls_of(d, 'height', 'clean') & ~iso] == 0)
    for name in ('nan_z_bracket', 'nan_z_crossing'):
        assert np.all(nz[bc.cls_of(d, 'height', name) & ~iso] == 1), name
    # wind
    w = lambda n: bc.cls_of(d, 'wind', n)
    with np.errstate(invalid='ignore'):
        on = (wh == bc.SHEAR_HEIGHT).sum(axis=0)
        lo, hi = (wh < bc.SHEAR_HEIGHT).sum(axis=0), (wh > bc.SHEAR_HEIGHT).sum(axis=0)
    assert np.all(on[w('between')] == 0) and np.all(lo[w('between')] > 0) and np.all(hi[w('between')] > 0)
    assert np.all(on[w('on_level')] == 1) and np.all(on[w('two_levels')] == 2) and np.all(on[w('equal_speed')] == 1)
    assert np.all(hi[w('above_top')] + on[w('above_top')] == 0) and np.all(lo[w('below_bottom')] + on[w('below_bottom')] == 0)
    assert np.all((np.isnan(wu) | np.isnan(wv)).sum(axis=0)[w('nan_wind_bracket')] == 1)
    assert np.isnan(wu[:, w('nan_wind_bracket')]).any() and np.isnan(wv[:, w('nan_wind_bracket')]).any()
    assert np.all(np.isnan(wh).sum(axis=0)[w('nan_wind_height')] == 1) and np.isnan(wh).sum() == w('nan_wind_height').sum()
    sfc_nan = np.isnan(d['surface_wind_u']) | np.isnan(d['surface_wind_v'])
    assert np.array_equal(sfc_nan, w('nan_surface_wind')) and np.isnan(d['surface_wind_u']).any() and np.isnan(d['surface_wind_v']).any()
    # the tie of positive_shear's strict `>`: both speeds are the same number, so the reference says False
    ref = _ref(dtype, True)
    sel = w('equal_speed')
    k = np.argmax(wh == bc.SHEAR_HEIGHT, axis=0)
    c = np.arange(cc.NCOL)
    assert np.all(np.hypot(wu[k, c], wv[k, c])[sel] == np.hypot(d['surface_wind_u'], d['surface_wind_v'])[sel])
    assert not ref['positive_shear'][sel].any() and np.all(ref['shear_magnitude'][sel] > 0)


# (axis, class) -> the outputs that are NaN in every column of the class, and why
NAN_ONLY = {
    ('isobar', 'outside_below'): ('temp_500', 'lapse_rate_700_500', 'dci_plus_lifted_index'),   # every pressure below 500 hPa
    ('isobar', 'outside_above'): ('temp_500', 'lapse_rate_700_500'),                             # every pressure above 600 hPa
    ('isobar', 'nan_column'): ('temp_500', 'lapse_rate_700_500', 'freezing_level', 'melting_level', 'dci_plus_lifted_index'),
    # one level: no bracket (but on the isobar itself, which a random level is not), and a NaN dewpoint beside every level
    ('isobar', 'one_valid_level'): ('temp_500', 'lapse_rate_700_500', 'melting_level', 'dci_plus_lifted_index'),
    ('freezing', 'never'): ('freezing_level',),
    ('freezing', 'nan_between'): ('freezing_level',),                   # the NaN takes both intervals of the one sign change
    ('wind', 'above_top'): ('shear_u', 'shear_v', 'shear_magnitude'),
    ('wind', 'below_bottom'): ('shear_u', 'shear_v', 'shear_magnitude'),
    ('wind', 'nan_wind_bracket'): ('shear_magnitude',),
    ('wind', 'nan_surface_wind'): ('shear_magnitude',),
}
# the shear depends on the wind axis alone: in these classes it cannot be NaN (a NaN wind height is skipped, pf.py:1786)
WIND_FINITE_ONLY = ('between', 'on_level', 'two_levels', 'nan_wind_height', 'equal_speed')


@both
def test_reference_is_finite_and_nan_in_every_class_where_both_can_happen(dtype):
    d, ref = _grid(), _ref(dtype, True)
    for ax, names in bc.AXES.items():
        for n in set(names):
            sel = bc.cls_of(d, ax, n)
            for k in bc.LEVEL_OUT:
                finite, nan = np.isfinite(ref[k][sel]).any(), np.isnan(ref[k][sel]).any()
                assert finite != (k in NAN_ONLY.get((ax, n), ())), (ax, n, k, 'finite' if finite else 'NaN only')
                shear_only = k.startswith('shear') and (ax != 'wind' or n in WIND_FINITE_ONLY)
                if ax == 'wind' and n in WIND_FINITE_ONLY and k.startswith('shear'):
                    assert not nan, (ax, n, k)
                elif not shear_only and not (ax, n, k) == ('isobar', 'nan_coord_next', 'temp_500'):
                    assert nan, (ax, n, k)
    # the humidity classes reach the outputs through the dewpoint: 850 hPa dewpoint and the melting level
    for n in ('q_zero', 'q_negative', 'q_nan'):
        sel = bc.cls_of(d, 'humidity', n) & bc.cls_of(d, 'isobar', 'between')
        assert not ref['valid'][sel].any(), n
    assert ref['valid'][bc.cls_of(d, 'humidity', 'supersaturated')].any()
    # a NaN height does not invalidate a column (pf.py:1976-1981 does not look at it)
    for n in ('nan_z_bracket', 'nan_z_crossing'):
        assert ref['valid'][bc.cls_of(d, 'height', n)].any(), n


@both
def test_reference_shows_every_outcome(dtype):
    ref, blanked = _ref(dtype, True), _ref(dtype, False)
    for k in ('n_freezing', 'n_melting'):
        n = ref[k]
        assert (n == 0).sum() >= MIN_CLASS and (n == 1).sum() >= MIN_CLASS and (n >= 3).sum() >= MIN_CLASS, (k, np.bincount(n))
        lvl = ref[k[2:] + '_level']
        assert np.array_equal(np.isnan(lvl), n == 0)
    assert ref['positive_shear'].sum() >= MIN_CLASS and (~ref['positive_shear']).sum() >= MIN_CLASS
    valid = ref['valid']
    assert valid.sum() >= MIN_CLASS and (~valid).sum() >= MIN_CLASS and np.array_equal(valid, blanked['valid'])
    for k in bc.LEVEL_OUT:
        assert np.all(np.isnan(blanked[k][~valid])) and np.array_equal(blanked[k][valid], ref[k][valid], equal_nan=True), k
        assert np.isfinite(ref[k][~valid]).any(), k                    # blanking takes something away
        assert np.isfinite(blanked[k][valid]).any() and np.isnan(blanked[k][valid]).any(), k
    assert not blanked['positive_shear'][~valid].any() and ref['positive_shear'][~valid].any() and blanked['positive_shear'][valid].any()


def test_wet_bulb_expression_is_the_oracles_in_float64():
    d = _grid()
    t, q, p = d['temperature'], d['specific_humidity'], d['pressure']
    with np.errstate(all='ignore'):
        td = bc.th.dewpoint_from_specific_humidity(p, t, q)
    assert np.array_equal(bc.wet_bulb_third(t, td), po.wet_bulb_temperature_fast(t, td), equal_nan=True)
    t32, td32 = t.astype(np.float32), td.astype(np.float32)
    wb32 = bc.wet_bulb_third(t32, td32)
    assert wb32.dtype == np.float32
    with np.errstate(invalid='ignore'):
        ref = t32 - np.float32(1 / 3) * (t32 - td32)
    assert np.array_equal(wb32, ref, equal_nan=True)
    assert (wb32.astype(np.float64) != po.wet_bulb_temperature_fast(t32, td32))[~np.isnan(wb32)].any()      # the type matters


@both
@pytest.mark.parametrize('shape', cc.SMALL_SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('ignore_nans', [False, True])
def test_small_shapes_evaluate(shape, dtype, ignore_nans):
    ref = _ref(dtype, ignore_nans, shape)
    assert all(ref[k].shape == (shape[1],) for k in bc.LEVEL_OUT + ('positive_shear', 'valid'))
    assert np.isfinite(ref['shear_u']).any()
    if shape[0] > 1 and shape[1] > 1:
        assert np.isfinite(ref['freezing_level']).any() or not ignore_nans


# ---- the columns the full oracle is asked about: convectively alive, so that CAPE, CIN, the proxies and SHIP are values --------
@functools.lru_cache(maxsize=None)
def _oracle(ignore_nans):
    d = _grid()
    cols = bc.oracle_columns(d, ignore_nans)
    return cols, bc.oracle_bundle(d, cols, ignore_nans)


@pytest.mark.parametrize('ignore_nans', [False, True])
def test_oracle_columns_cover_the_classes_and_are_convectively_alive(ignore_nans):
    d = _grid()
    cols, ref = _oracle(ignore_nans)
    assert 150 <= cols.size <= bc.ORACLE_MAX and np.all(np.diff(cols) > 0)
    assert np.array_equal(cols, bc.oracle_columns(d, ignore_nans))                      # the draw is seeded
    p = d['pressure'][:, cols]
    assert not np.isnan(p).any() and np.all(np.diff(p, axis=0) < 0)
    for ax in ('freezing', 'humidity', 'wind'):
        assert set(np.array(bc.AXES[ax])[d['cls_' + ax][cols]]) == set(bc.AXES[ax]), ax
    assert bc.warm_columns(cc.NCOL)[cols].sum() >= 50
    # parcels: CAPE and CIN are values, not zeros, for each of the three parcels
    with np.errstate(invalid='ignore'):
        for pre in ('mu', 'mixed_100', 'mixed_50'):
            assert (ref[pre + '_cape'] > 100.0).sum() >= 30 and (ref[pre + '_cin'] < -1.0).sum() >= 20, pre
            assert (ref[pre + '_lifted_index'] < 0.0).sum() >= 20 and (ref[pre + '_lifted_index'] > 0.0).sum() >= 20, pre
            assert (ref[pre + '_dci'] > 25.7).sum() >= 10 and (ref[pre + '_dci'] < 25.7).sum() >= 10, pre
    # the proxies: every flag takes both values, the CAPE x shear ones in numbers; SHIP is a number in several columns
    prox = po.storm_proxies(ref)
    for k, v in prox.items():
        if k != 'ship':
            assert v.any() and not v.all(), k
    for k in ('proxy_Craven2004', 'proxy_Trapp2007', 'proxy_Marsh2009', 'proxy_Allen2011', 'proxy_Eccel2012', 'proxy_SHIP_0.1'):
        assert prox[k].sum() >= 5, (k, int(prox[k].sum()))
    ship = prox['ship']
    assert np.isfinite(ship).sum() >= 5 and np.isnan(ship).sum() >= 50 and np.nanmax(ship) > 1.0


def test_the_cold_columns_alone_would_leave_the_proxies_dead():
    """What the warm columns are there for: without them no flag is ever True and SHIP is NaN everywhere."""
    cols, ref = _oracle(True)
    cold = ~bc.warm_columns(cc.NCOL)[cols]
    prox = po.storm_proxies({k: v[cold] for k, v in ref.items()})
    assert not any(v.any() for k, v in prox.items() if k != 'ship') and np.isnan(prox['ship']).all()
