"""CPU guard of tests/primitive_cases.py (no GPU): the builders are deterministic; every class of column they name is
present in numbers and is what its name says, in float64 and after the inputs are rounded to float32 (coordinates that
were equal stay equal, zeros stay zeros, ties stay ties); oracle/parcel_oracle.py evaluates every case on every shape,
the one-level grid and the NaN-only column included, and returns the shapes the GPU tests rely on; the restatement of
crossing_level agrees with the one of tests/layer_cape_restatement.py; and the two CPU oracles agree on every kind of
wet-bulb element before the GPU is asked."""
import warnings

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import parcel_oracle as po
from tests import component_cases as cc
from tests import layer_cape_restatement as lr
from tests import primitive_cases as pc
from tests.test_component_cases_cpu import _same

DTYPES = (np.float64, np.float32)
MIN = 80                      # columns per class on the 1337-column grid: 1337 // 15 = 89 for the longest class list


def _cast(case, dtype):
    """The float arrays of a case as the oracle sees them when the kernel is given `dtype`."""
    out = {}
    for k, v in case.items():
        if isinstance(v, tuple):
            out[k] = tuple(cc.cast(x, dtype)[1] for x in v)
        else:
            out[k] = cc.cast(v, dtype)[1] if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else v
    return out


def _sign_changes(d):
    with np.errstate(invalid='ignore'):
        s = np.sign(d)
        return s[1:] * s[:-1] < 0


BUILDERS = (pc.insert_level_cases, pc.crossing_profiles, pc.trapz_cases, pc.layer_cases, pc.shift_cases, pc.rebase_cases,
            pc.level_cases, pc.crossing_cases, pc.humidity_cases)


@pytest.mark.parametrize('builder', BUILDERS + (pc.interp1d_cases, pc.wet_bulb_elements))
def test_builders_are_deterministic(builder):
    assert _same(builder(), builder())
    if builder in BUILDERS:
        for shape in cc.SMALL_SHAPES:
            a = builder(*shape)
            assert _same(a, builder(*shape))
            assert all(v.shape[-2:] == shape for v in a.values() if isinstance(v, np.ndarray) and v.ndim == 2 and v.dtype.kind == 'f'
                       and v.shape[0] == shape[0])


# ---- the census: one function per builder, so that the last test can show it failing on a doctored case ----------------
def _common(case, classes, coord, others=()):
    c = case[coord]
    valid = (~np.isnan(c)).sum(axis=0)
    sel = pc.cls_of(case, classes, 'nan_column')
    assert sel.sum() >= MIN and np.all(valid[sel] == 0) and all(np.all(np.isnan(case[k][:, sel])) for k in others)
    sel = pc.cls_of(case, classes, 'one_valid_level')
    assert sel.sum() >= MIN and np.all(valid[sel] == 1)
    sel = pc.cls_of(case, classes, 'nan_coords_inside')
    n_nan = c.shape[0] - valid[sel]
    assert sel.sum() >= MIN and np.all((n_nan >= 1) & (n_nan <= 2)) and not np.isnan(c[[0, -1]][:, sel]).any()


def census_insert_level(case):
    p, lev = case['pressure'], case['level_pressure']
    cls = lambda name: pc.cls_of(case, pc.INSERT_CLASSES, name)
    for name in pc.INSERT_CLASSES:
        assert cls(name).sum() >= MIN, name
    with np.errstate(invalid='ignore'):
        between = ((p[:-1] > lev[None, :]) & (p[1:] < lev[None, :])).sum(axis=0)
        on = (p == lev[None, :]).sum(axis=0)
    assert np.all(between[cls('between')] == 1) and np.all(on[cls('between')] == 0)
    assert np.all(on[cls('on_level')] == 1)
    assert np.all(np.isnan(lev[cls('nan_level')]))
    assert np.all(lev[cls('below_bottom')] > p[0, cls('below_bottom')])
    assert np.all(lev[cls('above_top')] < p[-1, cls('above_top')])
    for k in ('temperature', 'dewpoint'):
        assert np.all((case[k][:, cls('fill_value')] == pc.FILL).sum(axis=0) == 1) and (case[k] == pc.FILL).sum() == cls('fill_value').sum()
    assert not np.any(p == pc.FILL)
    _common(case, pc.INSERT_CLASSES, 'pressure', ('temperature', 'dewpoint'))


def census_crossing_profiles(case):
    x, a, b = case['x'], case['a'], case['b']
    cls = lambda name: pc.cls_of(case, pc.CROSS_CLASSES, name)
    for name in pc.CROSS_CLASSES:
        assert cls(name).sum() >= MIN, name
    d = a - b
    change = _sign_changes(d)
    n = change.sum(axis=0)
    assert np.all(n[cls('no_crossing')] == 0) and not np.isnan(d[:, cls('no_crossing')]).any()
    for k in range(1, 6):
        sel = cls('crossings_%d' % k)
        assert np.all(n[sel] == k) and not np.any(d[:, sel] == 0)
        up = (change & (d[1:] > 0))[:, sel].sum()
        assert 0 < up < change[:, sel].sum()                                 # both directions
    zero = d == 0.0
    assert np.all(zero[:, cls('equal_one_level')].sum(axis=0) == 1)
    sel = cls('equal_two_levels')
    assert np.all(zero[:, sel].sum(axis=0) == 2) and np.all((zero[1:] & zero[:-1])[:, sel].sum(axis=0) == 1)
    assert zero.sum() == cls('equal_one_level').sum() + 2 * sel.sum()
    sel = cls('adjacent_crossings')
    assert np.all((change[1:] & change[:-1])[:, sel].sum(axis=0) == 1) and np.all(n[sel] == 2)
    for name, arr in (('nan_a', a), ('nan_b', b), ('nan_x', x)):
        for c in np.nonzero(cls(name))[0]:
            m = np.nonzero(np.isnan(arr[:, c]))[0]
            assert m.size == 1, (name, c)
            near = [j for j in (m[0] - 2, m[0] + 1) if 0 <= j < change.shape[0] and change[j, c]]
            assert near, (name, c)                                           # next to an interval whose sign changes
    _common(case, pc.CROSS_CLASSES, 'x', ('a', 'b'))


def census_trapz(case):
    dat, x = case['dat'], case['x']
    cls = lambda name: pc.cls_of(case, pc.TRAPZ_CLASSES, name)
    for name in pc.TRAPZ_CLASSES:
        assert cls(name).sum() >= MIN, name
    with np.errstate(invalid='ignore'):
        pos, neg = (dat > 0).any(axis=0), (dat < 0).any(axis=0)
    assert np.all(pos[cls('both_signs')] & neg[cls('both_signs')]) and np.all(pos[cls('one_sign')] != neg[cls('one_sign')])
    assert np.all(np.isnan(dat[1:-1, cls('nan_dat')]).sum(axis=0) == 1) and np.all(np.isnan(x[1:-1, cls('nan_x')]).sum(axis=0) == 1)
    assert np.all(((dat[1:] + dat[:-1]) == 0.0)[:, cls('zero_area')].sum(axis=0) >= 1)
    assert 0.6 < case['mask'].mean() < 0.8
    _common(case, pc.TRAPZ_CLASSES, 'x', ('dat',))


def census_layer(case):
    p, bound = case['pressure'], case['bound']
    cls = lambda name: pc.cls_of(case, pc.LAYER_CLASSES, name)
    for name in pc.LAYER_CLASSES:
        assert cls(name).sum() >= MIN, name
    dist = np.abs(p - bound[None, :])
    ok = ~np.all(np.isnan(p), axis=0)
    closest = np.zeros(p.shape[1], dtype=np.int64)
    closest[ok] = (dist[:, ok] == np.nanmin(dist[:, ok], axis=0)[None, :]).sum(axis=0)
    assert np.all(closest[cls('bound_between')] == 2)                        # a tie: the larger pressure wins
    assert np.all(closest[ok & ~cls('bound_between')] == 1)
    assert np.all((p == bound[None, :]).sum(axis=0)[cls('bound_on_level')] == 1)
    sel = cls('bound_outside')
    assert np.all((bound[sel] > p[0, sel]) | (bound[sel] < p[-1, sel]))
    for depth in (100.0, 300.0):
        sel = cls('top_on_level_%d' % depth)
        assert np.all((p[:, sel] == (p[0, sel] - depth)[None, :]).sum(axis=0) == 1), depth
    sel = cls('max_not_at_0')
    assert np.all(np.argmax(p[:, sel], axis=0) == 1)
    assert np.all((p[0] - p[-1])[cls('plain')] < max(pc.LAYER_DEPTHS)) and np.all((p[0] - p[-1])[cls('plain')] > 300.0)
    _common(case, pc.LAYER_CLASSES, 'pressure', ('temperature', 'dewpoint'))


def census_shift(case):
    p, lead = case['pressure'], case['lead']
    nlev = p.shape[0]
    for n in range(nlev + 1):
        assert (lead == n).sum() >= 20, n
    first_valid = np.where(np.isnan(p).all(axis=0), nlev, np.argmin(np.isnan(p), axis=0))
    assert np.array_equal(first_valid, lead) and np.all(np.isnan(p[:, lead == nlev]))
    later = np.isnan(p).sum(axis=0) - lead
    assert np.array_equal(later > 0, case['nan_later']) and case['nan_later'].sum() >= 200


def census_interp1d(case):
    xp, at = case['xp'], case['at']
    cls = lambda name: pc.cls_of(case, pc.INTERP1D_CLASSES, name)
    assert np.all(np.diff(xp, axis=0) > 0) and np.all(np.diff(case['xp_shared']) > 0)
    for name in pc.INTERP1D_CLASSES:
        assert cls(name).sum() >= MIN, name
    for points, a in ((xp, at), (case['xp_shared'][:, None], case['at_shared'])):
        r = a[3]
        assert np.all((points[1:-1] == r[None, :]).sum(axis=0)[cls('on_knot')] == 1)
        assert np.all(np.isnan(r[cls('nan_at')])) and np.isnan(a).sum() == cls('nan_at').sum()
        lo, hi = np.broadcast_to(points[0], r.shape), np.broadcast_to(points[-1], r.shape)
        assert np.all(r[cls('on_first')] == lo[cls('on_first')]) and np.all(r[cls('on_last')] == hi[cls('on_last')])
        assert np.all(r[cls('below_first')] < lo[cls('below_first')]) and np.all(r[cls('above_last')] > hi[cls('above_last')])
        inside = np.delete(a, 3, axis=0)
        assert not np.any(inside[:, :, None] == points.T[None, :, :] if points.shape[1] > 1 else inside[:, :, None] == points[:, 0])


def census_level(case):
    p, at = case['coords'], case['at']
    t = case['variables'][0]
    cls = lambda name: pc.cls_of(case, pc.LEVEL_CLASSES, name)
    for name in pc.LEVEL_CLASSES:
        assert cls(name).sum() >= MIN, name
    on = p == at[None, :]
    with np.errstate(invalid='ignore'):
        mid = (0.5 * (p[:-1] + p[1:]) == at[None, :]).sum(axis=0)
    assert np.all(mid[cls('between')] == 1) and np.all(on.sum(axis=0)[cls('between')] == 0)
    assert np.all(on.sum(axis=0)[cls('on_level')] == 1)
    target = np.all(at[cls('on_level') | cls('duplicate_mean') | cls('duplicate_one_nan') | cls('outside_below') |
                       cls('outside_above') | cls('nan_coord_next')] == pc.LEVEL_TARGET)
    assert target
    for c in np.nonzero(cls('duplicate_mean') | cls('duplicate_one_nan'))[0]:
        k = np.nonzero(on[:, c])[0]
        assert k.size == 2 and k[1] == k[0] + 1, c
        for i, v in enumerate(case['variables']):
            if pc.LEVEL_CLASSES[case['cls'][c]] == 'duplicate_mean' or i % 2 == (c // len(pc.LEVEL_CLASSES)) % 2:
                assert v[k[0], c] != v[k[1], c] and not np.isnan(v[k, c]).any(), c     # the mean is neither of the two
            else:
                assert np.isnan(v[k, c]).sum() == 1, c                                 # the other value alone
    for parity in (0, 1):                                                   # either way round within one interp_levels call
        assert (cls('duplicate_one_nan') & ((np.arange(p.shape[1]) // len(pc.LEVEL_CLASSES)) % 2 == parity)).sum() >= MIN // 2
    assert np.all(p[:, cls('outside_below')] < pc.LEVEL_TARGET) and np.all(p[:, cls('outside_above')] > pc.LEVEL_TARGET)
    for c in np.nonzero(cls('nan_coord_next'))[0]:
        m = np.nonzero(np.isnan(p[:, c]))[0]
        with np.errstate(invalid='ignore'):
            k = np.nonzero(p[:, c] > pc.LEVEL_TARGET)[0][-1]                 # the bracket is (k, first valid level above k)
        assert m.size == 1 and m[0] in (k - 1, k + 1, k + 2), c
    for tgt in pc.LEVEL_TARGETS:                                            # the other targets fall between levels of most columns
        with np.errstate(invalid='ignore'):
            assert (((p > tgt).any(axis=0)) & ((p < tgt).any(axis=0))).sum() >= 500, tgt
    assert not np.isnan(t[:, cls('on_level')]).any()
    _common(case, pc.LEVEL_CLASSES, 'coords')


def census_crossing(case, value, exact_zero=True):
    x, a = case['x'], case['a']
    cls = lambda name: pc.cls_of(case, pc.CROSSING_CLASSES, name)
    for name in pc.CROSSING_CLASSES:
        assert cls(name).sum() >= MIN, name
    d = a - value
    n = _sign_changes(d).sum(axis=0)
    assert np.all(n[cls('never')] == 0) and np.all(n[cls('once')] == 1) and np.all(n[cls('three_times')] == 3)
    for name in ('never', 'once', 'three_times'):
        assert not np.isnan(d[:, cls(name)]).any() and not np.isnan(x[:, cls(name)]).any()
    if exact_zero:
        assert np.all((d == 0.0)[:, cls('on_value')].sum(axis=0) == 1)
    for c in np.nonzero(cls('nan_between'))[0]:
        m = np.nonzero(np.isnan(a[:, c]))[0]
        assert m.size == 1 and d[m[0] - 1, c] * d[m[0] + 1, c] < 0, c
    _common(case, pc.CROSSING_CLASSES, 'x', ('a',))


def census_wet_bulb(e):
    p, t, td, kind = e['pressure'], e['temperature'], e['dewpoint'], e['kind']
    k = lambda name: kind == pc.WET_BULB_KINDS.index(name)
    assert p.shape == (1841,) and pc.WET_BULB_LAYOUTS[1][0] * pc.WET_BULB_LAYOUTS[1][1] == p.size
    for name in pc.WET_BULB_KINDS:
        assert k(name).sum() >= 160, name
    dd = t - td
    assert np.all(dd[k('saturated')] == 0.0) and np.all(dd[k('depression_40')] == 40.0)
    assert np.all((dd[k('supersaturated')] <= -0.25) & (dd[k('supersaturated')] >= -3.0))
    assert np.all((p[k('low_pressure')] >= 10.0) & (p[k('low_pressure')] <= 50.0)) and np.all(td[k('td_below_150')] < 150.0)
    assert np.all(np.isnan(p + t + td)[k('nan_input')]) and not np.isnan(p + t + td)[~k('nan_input')].any()
    assert np.all((dd[k('humid')] > 0) & (dd[k('humid')] <= 2.5)) and np.all(t[k('cold')] < 235.0)
    # one wavefront holds several kinds, those off lcl()'s fast path among them, whichever way the elements are laid out
    sane = (td <= t) & (td > 150.0) & (t < 350.0) & (p > 50.0) & (p < 1200.0) & (td != t)
    for w in range(0, p.size, 64):
        assert len(set(kind[w:w + 64].tolist())) >= 4 and (0 < sane[w:w + 64].sum() < kind[w:w + 64].size), w


def census_humidity(case):
    q = case['specific_humidity']
    assert (q == 0.0).sum() >= 1000 and (q < 0.0).sum() >= 1000 and (q > 0.0).sum() >= 20000
    for k in ('pressure', 'temperature', 'dewpoint', 'specific_humidity'):
        assert 300 <= np.isnan(case[k]).sum() <= 1000, k


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_class_is_there_and_survives_float32(dtype):
    """Each class at least MIN times on the grid, and each column what its class says, in the values the kernel is given."""
    census_insert_level(_cast(pc.insert_level_cases(), dtype))
    census_crossing_profiles(_cast(pc.crossing_profiles(), dtype))
    census_trapz(_cast(pc.trapz_cases(), dtype))
    census_layer(_cast(pc.layer_cases(), dtype))
    census_shift(_cast(pc.shift_cases(), dtype))
    census_interp1d(_cast(pc.interp1d_cases(), dtype))
    census_level(_cast(pc.level_cases(), dtype))
    for value in pc.CROSSING_VALUES:
        for increasing in (True, False):
            # a level exactly on 273.15 or 263.15 is not a float32 number: that class is exact in float32 for 0.0 only
            census_crossing(_cast(pc.crossing_cases(value=value, increasing=increasing), dtype), value,
                            exact_zero=dtype == np.float64 or value == 0.0)
    census_wet_bulb(_cast(pc.wet_bulb_elements(), dtype))
    census_humidity(_cast(pc.humidity_cases(), dtype))


def test_float32_rounding_changes_no_crafted_value():
    """Coordinates and quantised values are float32 numbers already (multiples of 1/64 or 1/128 below 2048)."""
    for case, keys in ((pc.insert_level_cases(), ('pressure', 'temperature', 'dewpoint', 'level_pressure')),
                       (pc.crossing_profiles(), ('x', 'a', 'b')), (pc.trapz_cases(), ('dat', 'x')),
                       (pc.layer_cases(), ('pressure', 'temperature', 'dewpoint', 'bound')), (pc.shift_cases(), ('pressure',)),
                       (pc.level_cases(), ('coords', 'at')), (pc.crossing_cases(value=0.0), ('a',)),
                       (pc.crossing_cases(increasing=False), ('x',)), (pc.wet_bulb_elements(), ('pressure', 'temperature', 'dewpoint')),
                       (pc.interp1d_cases(), ('xp', 'fp', 'at', 'xp_shared', 'at_shared'))):
        for k in keys:
            assert np.array_equal(cc.cast(case[k], np.float32)[1], case[k], equal_nan=True), k


def test_the_census_fails_when_a_class_goes_missing():
    """Doctored copies of the cases, each with one class emptied of what makes it that class: the census objects."""
    case = pc.insert_level_cases()
    sel = pc.cls_of(case, pc.INSERT_CLASSES, 'on_level')
    case['level_pressure'] = np.where(sel, case['level_pressure'] - 1.0 / 128.0, case['level_pressure'])
    with pytest.raises(AssertionError):
        census_insert_level(case)
    case = pc.crossing_profiles()
    sel = pc.cls_of(case, pc.CROSS_CLASSES, 'equal_two_levels')
    case['a'] = np.where(sel[None, :] & (case['a'] == case['b']), case['a'] + 0.25, case['a'])
    with pytest.raises(AssertionError):
        census_crossing_profiles(case)
    case = pc.level_cases()
    sel = pc.cls_of(case, pc.LEVEL_CLASSES, 'duplicate_mean')
    case['coords'] = np.where(sel[None, :] & (np.cumsum(case['coords'] == pc.LEVEL_TARGET, axis=0) == 2), pc.LEVEL_TARGET - 1.0,
                              case['coords'])
    with pytest.raises(AssertionError):
        census_level(case)
    case = pc.crossing_cases()
    case['cls'] = np.where(pc.cls_of(case, pc.CROSSING_CLASSES, 'three_times'), pc.CROSSING_CLASSES.index('once'), case['cls'])
    with pytest.raises(AssertionError):
        census_crossing(case, 273.15)
    e = pc.wet_bulb_elements()
    e['dewpoint'] = np.minimum(e['dewpoint'], e['temperature'])              # no supersaturated element left
    with pytest.raises(AssertionError):
        census_wet_bulb(e)
    case = pc.shift_cases()
    case['pressure'][:, case['lead'] == case['pressure'].shape[0]] = 500.0   # no NaN-only column left
    with pytest.raises(AssertionError):
        census_shift(case)


# ---- the oracle evaluates every case ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', pc.SHAPES)
def test_the_oracle_evaluates_every_case(shape):
    """No call raises, on any shape; the results have the shapes the GPU tests compare against -- with one level:
    find_intersections zero rows, trap_around_zeros one all-NaN row and a mask of ones, trapz 0."""
    nlev, ncol = shape
    r = pc.ref_insert_level(pc.insert_level_cases(*shape))
    assert all(r[k].shape == (nlev + 1, ncol) for k in pc.DATASET)
    s = pc.crossing_profiles(*shape)
    for log_x in (False, True):
        for b in (s['b'], None):
            r = pc.ref_find_intersections(s['x'], s['a'] if b is not None else s['diff'], b, log_x)
            assert len(r) == 6 and all(v.shape == (nlev - 1, ncol) for v in r.values())
            if shape == pc.GRID:
                assert np.isfinite(r['increasing_x']).sum() >= 500 and np.isfinite(r['decreasing_x']).sum() >= 500
        areas, mask = pc.ref_trap_around_zeros(s['x'], s['diff'], log_x)
        assert all(v.shape == (2 * nlev - 1, ncol) for v in areas.values()) and mask.shape == shape and mask[-1].all()
        if nlev == 1:
            assert all(np.isnan(v).all() for v in areas.values())
        if shape == pc.GRID:
            assert (~mask).sum() >= 1000
    z = pc.trapz_cases(*shape)
    for kw in (dict(), dict(only_positive=True), dict(only_negative=True)):
        for m in (None, z['mask']):
            r = pc.ref_trapz(z['dat'], z['x'], m, **kw)
            assert r.shape == (ncol,) and not np.isnan(r).any() and (nlev > 1 or np.all(r == 0.0))
    lay = pc.layer_cases(*shape)
    assert pc.ref_bound_pressure(lay['pressure'], lay['bound']).shape == (ncol,)
    assert pc.ref_bound_pressure(lay['pressure'], 700.0).shape == (ncol,)
    for interpolate in (True, False):
        for depth in pc.LAYER_DEPTHS:
            r = pc.ref_get_layer(lay, depth, interpolate)
            assert all(r[k].shape == (nlev + (1 if interpolate else 0), ncol) for k in pc.DATASET)
            if shape == pc.GRID:
                sel = pc.cls_of(lay, pc.LAYER_CLASSES, 'nan_column')
                assert np.isnan(r['pressure'][:, sel]).all() and np.isfinite(r['temperature']).sum() >= 2000
    sh = pc.shift_cases(*shape)
    r = pc.shift_reference({k: sh[k] for k in ('pressure', 'temperature')}, 'pressure')
    assert r['pressure'].shape == shape and not np.isnan(r['pressure'][0, sh['lead'] < nlev]).any()
    lv = pc.level_cases(*shape)
    for log in (False, True):
        assert pc.ref_interp_level(lv['coords'], lv['variables'][0], lv['at'], log).shape == (ncol,)
        for tgt in set(pc.LEVEL_TARGETS):
            assert pc.ref_interp_level(lv['coords'], lv['variables'][2], tgt, log).shape == (ncol,)
    for value in pc.CROSSING_VALUES:
        for increasing in (True, False):
            k = pc.crossing_cases(*shape, value=value, increasing=increasing)
            r = pc.crossing_reference(k['x'], k['a'], value)
            assert r.shape == (ncol,)
            if shape == pc.GRID:
                cls = lambda name: pc.cls_of(k, pc.CROSSING_CLASSES, name)
                assert np.isnan(r[cls('never') | cls('nan_column') | cls('one_valid_level')]).all()
                assert not np.isnan(r[cls('once') | cls('three_times') | cls('on_value')]).any()
    h = pc.humidity_cases(*shape)
    with np.errstate(all='ignore'):
        from oracle import thermo as th
        assert po.mixing_ratio(h['temperature'], h['dewpoint'], h['pressure']).shape == shape
        td = th.dewpoint_from_specific_humidity(h['pressure'], h['temperature'], h['specific_humidity'])
    assert td.shape == shape and np.isnan(td[h['specific_humidity'] <= 0.0]).all()


@pytest.mark.parametrize('shape', (pc.GRID, cc.SMALL_SHAPES[0]))
@pytest.mark.parametrize('mode', sorted(pc.REBASE))
def test_the_rebased_profiles_drop_levels(shape, mode):
    r = pc.rebase_cases(*shape)
    cols, parcel, kept = pc.rebase_reference(r['pressure'], r['temperature'], r['dewpoint'], mode)
    assert (~kept).sum() >= 2 and kept.sum() >= 10                           # levels that every column loses do get dropped
    assert cols['pressure'].shape == (int(kept.sum()) + (mode == 'mixed_layer'), shape[1])
    assert not np.isnan(cols['pressure'][0]).any() and not np.isnan(parcel['temperature']).any()
    if mode == 'most_unstable' and shape == pc.GRID:
        assert len(set(parcel['index'].tolist())) >= 3 and parcel['index'].min() >= 3


def test_interp1d_reference_on_the_cases():
    case = pc.interp1d_cases()
    assert pc.ref_interp1d(case['at'], case['xp'], case['fp']).shape == case['at'].shape
    r = pc.ref_interp1d(case['at_shared'], case['xp_shared'], case['fp'])
    assert np.isnan(r).sum() == pc.cls_of(case, pc.INTERP1D_CLASSES, 'nan_at').sum()


# ---- crossing_level: two restatements --------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', pc.CROSSING_VALUES)
@pytest.mark.parametrize('increasing', [True, False])
def test_crossing_restatements_agree(value, increasing):
    """min over find_intersections' all_intersect_x against tests/layer_cape_restatement.py's crossing rule: the same
    number wherever both are defined (the lowest crossing of an increasing x); with a decreasing x the smallest x is the
    LAST crossing met, which is what sets 'smallest' apart from 'first'."""
    for shape in pc.SHAPES:
        k = pc.crossing_cases(*shape, value=value, increasing=increasing)
        a = pc.crossing_reference(k['x'], k['a'], value)
        b = lr.crossing_height(k['x'], k['a'], value) if shape[0] > 1 else np.full(shape[1], np.nan)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(a)
        assert np.all(np.abs(a[ok] - b[ok]) <= 1e-12 * np.abs(b[ok]))
    k = pc.crossing_cases(value=value, increasing=increasing)
    a = pc.crossing_reference(k['x'], k['a'], value)
    sel = pc.cls_of(k, pc.CROSSING_CLASSES, 'three_times')
    d = k['a'][:, sel] - value
    first = np.argmax(np.sign(d[1:]) != np.sign(d[:-1]), axis=0)             # the first interval whose sign changes
    x0, x1 = k['x'][first, np.nonzero(sel)[0]], k['x'][first + 1, np.nonzero(sel)[0]]
    inside_first = (a[sel] >= np.minimum(x0, x1)) & (a[sel] <= np.maximum(x0, x1))
    assert np.all(inside_first) if increasing else not np.any(inside_first)


# ---- wet bulb: two CPU oracles ---------------------------------------------------------------------------------------------
def test_wet_bulb_oracles_agree():
    """po.wet_bulb_temperature with the RK4 adiabat against the C oracle's lcl followed by its moist_lapse, element by
    element: the same NaN pattern and values within the GPU test's 1e-8 K, for every kind -- those outside the box in
    which the device lcl() takes its fast path included (none of them had to be taken out of the builder)."""
    e = pc.wet_bulb_elements()
    for dtype in DTYPES:
        p, t, td = (cc.cast(e[k], dtype)[1] for k in ('pressure', 'temperature', 'dewpoint'))
        a = pc.wet_bulb_reference(co, p, t, td)
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            b = po.wet_bulb_temperature(p, t, td, moist='rk4')
        for i, name in enumerate(pc.WET_BULB_KINDS):
            sel = e['kind'] == i
            assert np.array_equal(np.isnan(a[sel]), np.isnan(b[sel])), name
            ok = sel & ~np.isnan(a)
            err = float(np.max(np.abs(a[ok] - b[ok]), initial=0.0))
            print('%-16s %4d elements, %4d NaN, oracles differ by at most %.3e K' % (name, sel.sum(), np.isnan(a[sel]).sum(), err))
            assert err <= 1e-8, (name, err)
            assert np.isnan(a[sel]).all() if name == 'nan_input' else not np.isnan(a[sel]).any(), name
    for layout in pc.WET_BULB_LAYOUTS:
        assert pc.wet_bulb_reference(co, *(e[k].reshape(layout) for k in ('pressure', 'temperature', 'dewpoint'))).shape == layout
