"""CPU guard of tests/component_cases.py (no GPU): the builders are deterministic, the C and the NumPy oracle agree on
every generated case -- indices exactly, floats to 1e-9 -- so that the inputs themselves carry no ambiguity that a GPU
comparison could trip over, and every class of input the GPU tests rely on is present in numbers."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import component_cases as cc

SHAPES = ((cc.NLEV, cc.NCOL),) + cc.SMALL_SHAPES


@pytest.fixture(scope='module')
def po():
    return cc.numpy_oracle()


@pytest.fixture(scope='module')
def scan():
    s = cc.scan_profiles()
    s['lfc_el'] = cc.run_lfc_el(co, s['pressure'], s['parcel'], s['env'], s['lcl_pressure'], s['lcl_temperature'])
    return s


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None or np.isscalar(a):
        return a is b or a == b
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def _agree(a, b, what):
    """Two oracle results (dicts of stacked arrays, or arrays): integers and NaN patterns identical, floats within 1e-9."""
    if not isinstance(a, dict):
        a, b = {'': a}, {'': b}
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (what, k)
        if x.dtype.kind != 'f':
            assert np.array_equal(x, y), (what, k, np.nonzero(x != y)[0][:10])
            continue
        assert np.array_equal(np.isnan(x), np.isnan(y)), (what, k)
        ok = ~np.isnan(x)
        assert np.all(np.abs(x[ok] - y[ok]) <= 1e-9), (what, k, float(np.max(np.abs(x[ok] - y[ok]))))


@pytest.mark.parametrize('builder', [cc.scan_profiles, cc.lcl_parcels, cc.lapse_cases, cc.parcel_profile_cases,
                                     cc.select_cases, cc.pipeline_columns])
def test_builders_are_deterministic(builder):
    assert _same(builder(), builder())
    if builder not in (cc.lcl_parcels, cc.pipeline_columns):
        for shape in cc.SMALL_SHAPES:
            a = builder(*shape)
            assert _same(a, builder(*shape)) and a['pressure'].shape == shape


@pytest.mark.parametrize('shape', SHAPES)
def test_oracles_agree_on_the_scan_profiles(shape, po):
    s = cc.scan_profiles(*shape)
    args = (s['pressure'], s['parcel'], s['env'], s['lcl_pressure'], s['lcl_temperature'])
    ref = cc.run_lfc_el(co, *args)
    _agree(ref, cc.run_lfc_el(po, *args), 'lfc_el')
    for source in cc.BASE_SOURCES:
        lfc, el = cc.base_bounds(s['pressure'], source, ref)
        for opts in cc.BASE_OPTIONS:
            _agree(cc.run_cape_cin_base(co, s['pressure'], s['env'], s['parcel'], lfc, el, **opts),
                   cc.run_cape_cin_base(po, s['pressure'], s['env'], s['parcel'], lfc, el, **opts), (source, opts))


def test_oracles_agree_on_the_point_and_lapse_cases(po):
    parcels = cc.lcl_parcels()
    args = (parcels['pressure'], parcels['temperature'], parcels['dewpoint'])
    _agree(cc.run_lcl(co, *args), cc.run_lcl(po, *args), 'lcl')
    for shape in SHAPES:
        case = cc.lapse_cases(*shape)
        for variant in ('none', 'scalar', 'array'):
            t0, pp = case[variant]
            for name in ('dry_lapse', 'moist_lapse'):
                _agree(cc.run_lapse(getattr(co, name), case['pressure'], t0, pp),
                       cc.run_lapse(getattr(po, name), case['pressure'], t0, pp), (name, variant, shape))
        case = cc.parcel_profile_cases(*shape)
        args = (case['pressure'], case['parcel_pressure'], case['parcel_temperature'], case['parcel_dewpoint'])
        _agree(cc.run_parcel_profile(co, *args), cc.run_parcel_profile(po, *args), ('parcel_profile', shape))


@pytest.mark.parametrize('shape', SHAPES)
def test_oracles_agree_on_the_selection_cases(shape, po):
    case = cc.select_cases(*shape)
    args = (case['pressure'], case['temperature'], case['dewpoint'])
    for depth in cc.MU_DEPTHS:
        _agree(cc.run_most_unstable(co, *args, depth), cc.run_most_unstable(po, *args, depth), ('most_unstable', depth))
    for depth in cc.ML_DEPTHS:
        _agree(cc.run_mixed(co, *args, depth), cc.run_mixed(po, *args, depth), ('mixed', depth))


def test_scan_profile_classes_are_all_there(scan):
    """At least 20 columns in every class: the builder cannot degrade silently."""
    y = scan['parcel'] - scan['env']
    nlev = y.shape[0]
    for i, name in enumerate(cc.SCAN_SHAPES):
        assert (scan['shape'] == i).sum() >= 20, name
    for i, name in enumerate(cc.LCL_KINDS):
        assert (scan['lcl_kind'] == i).sum() >= 20, name
    # ... and the columns are what their class says
    with np.errstate(invalid='ignore'):
        sign = np.sign(y)
    changes = (sign[1:] * sign[:-1] < 0).sum(axis=0)
    cls = lambda name: scan['shape'] == cc.SCAN_SHAPES.index(name)
    for n in range(1, 7):
        assert np.all(changes[cls('crossings_%d' % n)] == n)
    assert (changes >= 3).sum() >= 20
    assert np.all(y[:, cls('all_positive')] > 0) and np.all(y[:, cls('all_negative')] < 0)
    zeros = y == 0.0
    assert np.all(zeros[1:-1][:, cls('zero_interior')].sum(axis=0) == 1) and np.all(zeros[0, cls('zero_first')])
    assert np.all(zeros[-1, cls('zero_last')]) and np.all((zeros[1:] & zeros[:-1])[:, cls('zero_pair')].sum(axis=0) == 1)
    q = cls('zero_interior') | cls('zero_first') | cls('zero_last') | cls('zero_pair')
    assert np.all(y[:, q] * 4.0 == np.round(y[:, q] * 4.0))                 # quantised to 0.25 K
    for who, arrays in (('parcel', ('parcel',)), ('env', ('env',)), ('both', ('parcel', 'env'))):
        for where, rows in (('interior', slice(1, nlev - 1)), ('first', slice(0, 1)), ('last', slice(nlev - 1, nlev))):
            sel = cls('nan_%s_%s' % (who, where))
            for a in ('parcel', 'env'):
                n_nan = np.isnan(scan[a][:, sel]).sum(axis=0)
                assert np.all(n_nan == (1 if a in arrays else 0)), (who, where, a)
                assert np.all(np.isnan(scan[a][rows][:, sel]).sum(axis=0) == (1 if a in arrays else 0)), (who, where, a)
    assert np.all(np.isnan(scan['parcel'][:, cls('nan_parcel_all')]))
    p, lp = scan['pressure'], scan['lcl_pressure']
    kind = lambda name: scan['lcl_kind'] == cc.LCL_KINDS.index(name)
    assert np.all((p == lp[None, :]).sum(axis=0)[kind('on_level')] == 1)
    between = ((p[:-1] > lp[None, :]) & (p[1:] < lp[None, :])).sum(axis=0)
    assert np.all(between[kind('between')] == 1) and not np.any((p == lp[None, :])[:, kind('between')])
    assert np.all(lp[kind('below_bottom')] > p[0, kind('below_bottom')])
    assert np.all(lp[kind('above_top')] < p[-1, kind('above_top')]) and np.all(lp[kind('above_top')] > 0)
    assert np.all(np.isnan(lp[kind('nan')]))
    # what the oracle makes of them
    r = scan['lfc_el']
    assert (r['lfc_index'] == -2).sum() >= 20 and (r['lfc_index'] == -1).sum() >= 20 and (r['lfc_index'] >= 0).sum() >= 20
    assert (r['el_index'] >= 0).sum() >= 20 and r['status_top_nan'].sum() >= 20


def test_knife_edge_columns_stay_below_the_cap(scan):
    """A crossing within 1e-9 of the LCL pressure: only the crafted columns, at most 2 % of all, and in them both outcomes
    of the tie give the same LFC pressure and temperature (the crossing is followed by an EL, so an LFC that does not
    count as above the LCL is replaced by the LCL)."""
    knife = cc.knife_edge_columns(scan['pressure'], scan['parcel'], scan['env'], scan['lcl_pressure'])
    assert np.array_equal(knife, scan['crafted_knife_edge'])
    assert 5 <= knife.sum() <= 0.02 * knife.size
    r = scan['lfc_el']
    lp, lt = scan['lcl_pressure'][knife], scan['lcl_temperature'][knife]
    assert np.all(np.abs(r['lfc_pressure'][knife] - lp) <= 1e-9 * lp) and np.all(np.abs(r['lfc_temperature'][knife] - lt) <= 1e-9)
    assert np.all(r['el_pressure'][knife] < lp)
    for dtype in (np.float32,):                                           # the same columns after rounding the inputs
        a = [cc.cast(scan[k], dtype)[1] for k in ('pressure', 'parcel', 'env', 'lcl_pressure')]
        assert np.array_equal(cc.knife_edge_columns(*a), knife)
    for shape in cc.SMALL_SHAPES:
        s = cc.scan_profiles(*shape)
        assert cc.knife_edge_columns(s['pressure'], s['parcel'], s['env'], s['lcl_pressure']).sum() <= 0.02 * shape[1]


def test_lapse_and_profile_cases_cover_their_edges():
    case = cc.lapse_cases()
    p, (t0, ref) = case['pressure'], case['array']
    with np.errstate(invalid='ignore'):
        below, above, on = (p > ref[None, :]).sum(axis=0), (p < ref[None, :]).sum(axis=0), (p == ref[None, :]).sum(axis=0)
    name = np.array(cc.REF_KINDS)[case['ref_kind']]
    ok = ~np.isnan(ref)
    assert ((below >= 1) & (above >= 1) & (on == 0) & (name == 'inside')).sum() >= 200      # levels on both sides
    assert (on == 1).sum() >= 100
    assert np.all(below[(name == 'above_top') & ok] == (~np.isnan(p)).sum(axis=0)[(name == 'above_top') & ok])
    assert np.all(above[(name == 'below_bottom') & ok] == (~np.isnan(p)).sum(axis=0)[(name == 'below_bottom') & ok])
    k = np.arange(p.shape[0])[:, None]
    nan_below = (np.isnan(p) & (k <= case['bracket'][None, :])).any(axis=0) & (name == 'inside')
    nan_above = (np.isnan(p) & (k > case['bracket'][None, :])).any(axis=0) & (name == 'inside')
    assert nan_below.sum() >= 50 and nan_above.sum() >= 50 and (nan_below & nan_above).sum() >= 50
    assert np.isnan(p[0]).sum() >= 50 and np.isnan(t0).sum() >= 50 and np.isnan(ref).sum() >= 50
    case = cc.parcel_profile_cases()
    ref = cc.run_parcel_profile(co, case['pressure'], case['parcel_pressure'], case['parcel_temperature'], case['parcel_dewpoint'])
    sel = case['saturated_on_level']
    assert sel.sum() >= 100 and np.all(ref['lcl_pressure'][sel] == case['parcel_pressure'][sel])
    assert ((case['pressure'] == ref['lcl_pressure'][None, :]).any(axis=0) & sel).sum() >= 100   # the P == LCL branch
    assert np.isnan(case['pressure']).any(axis=0).sum() >= 200


def test_selection_cases_cover_their_edges():
    case = cc.select_cases()
    p, t, group = case['pressure'], case['temperature'], case['group']
    grp = lambda name: np.array(cc.SELECT_GROUPS)[group] == name
    assert grp('shallow').sum() >= 20 and np.all(p[0, grp('shallow')] - p[-1, grp('shallow')] < min(cc.MU_DEPTHS + cc.ML_DEPTHS))
    for depth in sorted(set(cc.MU_DEPTHS + cc.ML_DEPTHS)):
        sel = grp('top_on_level_%d' % depth)
        assert sel.sum() >= 20 and np.all((p[:, sel] == (p[0, sel] - depth)[None, :]).sum(axis=0) == 1), depth
        p32 = p[:, sel].astype(np.float32).astype(np.float64)
        assert np.all((p32 == (p32[0] - depth)[None, :]).sum(axis=0) == 1), depth       # also after rounding to float32
    for depth in cc.ML_DEPTHS:
        sel = grp('nan_below_top_%d' % depth)
        last_below = (p[:, sel] > (p[0, sel] - depth)[None, :]).sum(axis=0) - 1
        assert sel.sum() >= 20 and np.all(np.isnan(t[last_below, np.nonzero(sel)[0]]))
    # theta_e near ties: both sides of the 2e-5 threshold of the fp64 repeat, either level leading
    d = case['tie_delta'][grp('theta_e_tie')]
    assert not np.any(np.isnan(d))
    for delta in cc.TIE_DELTAS:
        for s in (1.0, -1.0):
            assert (np.abs(d - s * delta) <= 1e-3 * delta).sum() >= 5, (delta, s)
    assert (np.abs(d) < 2e-5).sum() >= 20 and (np.abs(d) > 2e-5).sum() >= 20
    args = (p, t, case['dewpoint'])
    for depth in cc.MU_DEPTHS:
        idx = cc.run_most_unstable(co, *args, depth)['index'][grp('theta_e_tie')]
        assert np.array_equal(idx, np.where(d > 0, cc.TIE_LEVELS[1], cc.TIE_LEVELS[0]))
