"""XP_HUM_RELATIVE and XP_HUM_MIXING_RATIO without a GPU: the enumerators in the header and the binding, the census of the
grids the device tests run on (tests/humidity_cases.py), the round trip through the NumPy restatement
(tests/humidity_restatement.py), the array API and the DataArray modules around a stubbed launch, the percent guard, and
the conversion kernel's resources."""
import os
import re

import numpy as np
import pytest

from tests import humidity_cases as K
from tests import humidity_restatement as R
from tests.resource_report import needs_hipcc, resources
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import ground, kinematics, layer_cape, max_cape
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import parcel_functions as pf
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_enumerators():
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert L.HUMIDITY == {'dewpoint': 0, 'specific': 1, 'relative': 2, 'mixing_ratio': 3} == R.ENUM
    assert re.search(r'enum \{ XP_HUM_DEWPOINT = 0, XP_HUM_SPECIFIC = 1, XP_HUM_RELATIVE = 2, XP_HUM_MIXING_RATIO = 3 \};', hdr)
    section = hdr[hdr.index('XP_HUM_RELATIVE and XP_HUM_MIXING_RATIO:'):hdr.index('enum { XP_HUM_DEWPOINT')]
    for rule in ('FRACTION', 'not percent', 'e = m * e_s(T)', 'e = p * m / (eps + m)', 'D = 273.15 + 243.5 v / (17.67 - v)',
                 'v = ln(e / 6.112)', 'NaN unless m > 0 by plain comparison', 'no upper', 'needs T and not p', 'p and not T',
                 "views' dtype, rounded once", 'bit for', 'environment_dewpoint', 'Explicit parcels stay', 'XP_PARCEL_OVER_GROUND',
                 'converted once per call', 'XP_OPT_FUSE_PARCELS', 'xp_cape_cin_layers', 'xp_effective_inflow_layer',
                 'XP_PARCEL_MAX_CAPE accepts both', 'XP_F32 rejects', 'xp_conv_properties', 'xp_hydrostatic_height', 'COST',
                 'one streaming pass', 'one dense (nlev, ncol) scratch', 'never written'):
        assert rule in section, rule


def test_no_new_entry_point_and_a_unit_of_its_own():
    assert len(L.SYMBOLS) == 56 and len(set(L.SYMBOLS)) == 56 and set(L.SYMBOLS) == set(L.ARGTYPES)
    assert [u for u in L.UNITS if u[1] == 'xp_humidity_tu.hip'] == [('humidity', 'xp_humidity_tu.hip', [])]
    src = lambda f: open(os.path.join(L.SRC_DIR, f)).read()
    assert 'k_dewpoint_from<' in src('xp_humidity_tu.hip') and 'launch_dewpoint_from' in src('xparcel.hip')
    # the conversion sits in front of the CAPE / CIN kernels, whose sources do not know about it
    for f in ('xp_kernels.hpp', 'xp_multi.hpp', 'xp_cape_f32.hpp', 'xp_ground.hpp', 'xp_cape_tu.hip', 'xp_multi_tu.hip', 'xp_cape_f32_tu.hip'):
        assert 'HUM_RELATIVE' not in src(f) and 'xp_humidity' not in src(f), f


# -- the grids of the device tests ----------------------------------------------------------------------------------------------
def test_census_of_the_class_columns():
    """What the device tests convert: in the base grid the share of elements with a dewpoint is 0.97 ... 0.99 per kind
    (counted: 0.9867 for both); every class column is what its name says; the shapes are leading blocks."""
    b = K.base()
    p, t, rh, w = b['pressure'], b['temperature'], b[R.RELATIVE], b[R.MIXING_RATIO]
    assert p.shape == t.shape == rh.shape == w.shape == (K.NLEV, K.NCOL) and K.NCOL % 64 != 0
    assert sorted(K.CLASSES.values()) == list(range(2, 47, 5)) and max(K.CLASSES.values()) < 63
    col = lambda a, name: a[:, K.CLASSES[name]]
    for m in (rh, w):
        assert (col(m, 'zero') == 0).all() and (col(m, 'negative') < 0).all() and np.isnan(col(m, 'nan')).all() and np.isposinf(col(m, 'inf')).all()
    assert (col(rh, 'rh_1.05') == 1.05).all() and (col(rh, 'rh_1e-6') == 1e-6).all() and (col(w, 'w_0.04') == 0.04).all()
    nan_t, nan_p = np.isnan(col(t, 't_nan')), np.isnan(col(p, 'p_nan'))
    assert np.nonzero(nan_t)[0].tolist() == list(K.T_NAN_LEVELS) and np.nonzero(nan_p)[0].tolist() == list(K.P_NAN_LEVELS)
    others = [c for n, c in K.CLASSES.items() if n != 'p_nan']
    assert not np.isnan(p[:, others]).any() and not np.isnan(t[:, [c for n, c in K.CLASSES.items() if n != 't_nan']]).any()
    d = {k: R.dewpoint64(k, p, t, b[k]) for k in R.KINDS}
    for k in R.KINDS:
        share = np.isfinite(d[k]).mean()
        print(k, 'finite share %.4f' % share)
        assert 0.97 <= share <= 0.99
        for name in ('zero', 'negative', 'nan', 'inf'):
            assert np.isnan(col(d[k], name)).all(), (k, name)
    # no upper bound: D above T; a very dry value is a (cold) dewpoint; T and p matter to one kind each
    assert (col(d[R.RELATIVE], 'rh_1.05') > col(t, 'rh_1.05')).all() and np.isfinite(col(d[R.RELATIVE], 'rh_1e-6')).all()
    assert (col(d[R.RELATIVE], 'rh_1e-6') < 200.0).all() and np.isfinite(col(d[R.MIXING_RATIO], 'w_0.04')).all()
    assert np.array_equal(np.isnan(col(d[R.RELATIVE], 't_nan')), nan_t) and np.isfinite(col(d[R.MIXING_RATIO], 't_nan')).all()
    assert np.array_equal(np.isnan(col(d[R.MIXING_RATIO], 'p_nan')), nan_p) and np.isfinite(col(d[R.RELATIVE], 'p_nan')).all()
    # the shapes
    assert K.SHAPES[K.MAIN] == (K.NLEV, K.NCOL) and {s[1] for s in K.SHAPES.values()} >= {1, 63, 64, 65, 257, 1337} and (1, 1337) in K.SHAPES.values()
    for name, (nlev, ncol) in K.SHAPES.items():
        for dtype in (np.float32, np.float64):
            g = K.grid(name, R.RELATIVE, dtype)
            assert all(a.shape == (nlev, ncol) and a.dtype == dtype and a.flags.c_contiguous for a in g)
            assert np.array_equal(g[2], rh[:nlev, :ncol].astype(dtype), equal_nan=True)


def test_round_trip_gives_the_dewpoint_back():
    """Td -> rh -> Td and Td -> w -> Td through the oracle's functions on the grid before the class columns are written:
    within 1e-10 K (counted: 2.9e-14 K both ways); rh spans 0.006 ... 1, w 4e-7 ... 0.039."""
    p, t, td = K.source()
    rh, w = R.relative_humidity(t, td), R.mixing_ratio(p, td)
    ok = ~np.isnan(td)
    for kind, m in ((R.RELATIVE, rh), (R.MIXING_RATIO, w)):
        back = R.dewpoint64(kind, p, t, m)
        assert np.array_equal(np.isnan(back), ~ok)
        err = np.abs(back[ok] - td[ok]).max()
        print(kind, 'round trip %.2e K, moisture %.3g ... %.3g' % (err, np.nanmin(m), np.nanmax(m)))
        assert err <= 1e-10
    assert 0.004 < np.nanmin(rh) < 0.008 and np.nanmax(rh) == 1.0 and 2e-7 < np.nanmin(w) < 6e-7 and 0.035 < np.nanmax(w) < 0.04
    # stored in the views' dtype, rounded once
    d32 = R.dewpoint(R.RELATIVE, p.astype(np.float32), t.astype(np.float32), rh.astype(np.float32))
    assert d32.dtype == np.float32 and np.array_equal(d32, R.dewpoint64(R.RELATIVE, None, t.astype(np.float32), rh.astype(np.float32)).astype(np.float32), equal_nan=True)
    assert np.array_equal(R.dewpoint64(R.MIXING_RATIO, K.isobars(), t, w), R.dewpoint64(R.MIXING_RATIO, np.broadcast_to(K.isobars()[:, None], w.shape), t, w), equal_nan=True)


# -- the array API and the DataArray modules around a stubbed launch ---------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def run(self, name, *args):
        opts = [a for a in args if isinstance(a, L.Opts)]
        seen.append((name, opts[0].humidity if opts else None, opts[0].compute if opts else None, opts[0].flags if opts else None))
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _small(dtype=np.float32, ncol=6):
    return K.grid('24x63', R.RELATIVE, dtype)[0][:, :ncol].copy(), K.grid('24x63', R.RELATIVE, dtype)[1][:, :ncol].copy(), \
        K.grid('24x63', R.RELATIVE, dtype)[2][:, :ncol].copy()


@pytest.mark.parametrize('kind', R.KINDS)
def test_array_api_passes_the_kind(calls, kind):
    p, t, m = _small()
    want = L.HUMIDITY[kind]
    sfc = tuple(a[0] for a in (p, t, t))
    z = np.ascontiguousarray(np.cumsum(np.ones_like(p), axis=0) * 500.0)
    for parcel in ('surface', 'most_unstable', 'mixed_layer', 'max_cape'):
        api.cape_cin_columns(p, t, m, parcel=parcel, humidity=kind)
        assert calls[-1][:2] == ('xp_cape_cin', want), parcel
    api.cape_cin_columns(p, t, m, parcel='explicit', parcel_values=sfc, humidity=kind, moist='family', want_profile=True)
    assert calls[-1][:2] == ('xp_cape_cin', want)
    api.cape_cin_columns(p, t, m, parcel='most_unstable', ground=sfc, humidity=kind)
    assert calls[-1][:2] == ('xp_cape_cin', want)
    for fn in (api.surface_based_cape_cin, api.most_unstable_cape_cin, api.mixed_layer_cape_cin, api.max_cape_cape_cin):
        fn(p, t, m, humidity=kind)
        assert calls[-1][:2] == ('xp_cape_cin', want), fn.__name__
    for fused in (False, True):
        api.cape_cin_multi(p, t, m, ['surface', 'mixed_layer'], moist='family', fused=fused, humidity=kind)
        assert calls[-1] == ('xp_cape_cin_multi', want, L.XP_F64, L.OPT_FUSE_PARCELS if fused else 0)
    api.cape_cin_multi(p, t, m, ['surface', 'max_cape'], ground=None, humidity=kind)
    assert calls[-1][:2] == ('xp_cape_cin_multi', want)
    api.cape_cin_layers(p, t, m, [{'top': 500.0}], humidity=kind)
    assert calls[-1][:2] == ('xp_cape_cin_layers', want)
    api.cape_3km(p, t, m, z, humidity=kind)
    assert calls[-1][:2] == ('xp_cape_cin_layers', want)
    api.hail_growth_zone_cape(p, t, m, z, parcel='mixed_layer', humidity=kind)
    assert calls[-1][:2] == ('xp_cape_cin_layers', want)
    api.effective_inflow_layer(p, t, m, z, humidity=kind)
    assert calls[-1][:2] == ('xp_effective_inflow_layer', want)
    # the defaults are what they were
    api.cape_cin_columns(p, t, m)
    api.effective_inflow_layer(p, t, m)
    api.cape_cin_layers(p, t, m, [{'top': 500.0}])
    assert [c[1] for c in calls[-3:]] == [0, 0, 0]
    # compute='float32' keeps its own rule: the preference falls back to fp64, the keyword reaches the library, which rejects it
    api.set_compute('float32')
    try:
        api.cape_cin_columns(p, t, m, moist='family', humidity=kind)
        assert calls[-1][1:3] == (want, L.XP_F64)
        api.cape_cin_columns(p, t, m, moist='family')
        assert calls[-1][1:3] == (0, L.XP_F32)
    finally:
        api.set_compute('float64')
    api.cape_cin_columns(p, t, m, moist='family', humidity=kind, compute='float32')
    assert calls[-1][1:3] == (want, L.XP_F32)


def test_array_api_assertions(calls):
    p, t, m = _small()
    with pytest.raises(AssertionError, match='relative'):
        api.cape_cin_columns(p, t, m, humidity='percent')
    with pytest.raises(AssertionError, match='does not take specific humidity'):
        api.cape_cin_layers(p, t, m, [{'top': 500.0}], humidity='specific')
    with pytest.raises(AssertionError, match='does not take specific humidity'):
        api.effective_inflow_layer(p, t, m, humidity='specific')
    assert not calls
    for fn in (api.cape_cin_columns, api.cape_cin_layers, api.effective_inflow_layer):
        assert "'relative'" in fn.__doc__ and "'mixing_ratio'" in fn.__doc__, fn.__name__


def _da(a, units=None, name=None):
    nlev, ncol = a.shape
    return DataArray(a.reshape(nlev, 2, ncol // 2), dims=(VD, 'y', 'x'), attrs={} if units is None else {'units': units}, name=name)


def _mirror_calls(p, t, m, kind):
    """Every DataArray entry that takes the keyword, as (name, thunk)."""
    sfc = [DataArray(np.asarray(a.values[0]), dims=('y', 'x')) for a in (p, t, t)]
    z = _da(np.ascontiguousarray(np.cumsum(np.ones(p.values.reshape(p.shape[0], -1).shape), axis=0) * 500.0))
    kw = dict(humidity=kind)
    return [('pf.surface', lambda: pf.surface_based_cape_cin(p, t, m, **kw)),
            ('pf.most_unstable', lambda: pf.most_unstable_cape_cin(p, t, m, **kw)),
            ('pf.mixed_layer', lambda: pf.mixed_layer_cape_cin(p, t, m, **kw)),
            ('ground.surface', lambda: ground.surface_based_cape_cin(p, t, m, *sfc, **kw)),
            ('ground.most_unstable', lambda: ground.most_unstable_cape_cin(p, t, m, *sfc, **kw)),
            ('ground.mixed_layer', lambda: ground.mixed_layer_cape_cin(p, t, m, *sfc, **kw)),
            ('ground.multi', lambda: ground.cape_cin_multi(p, t, m, *sfc, ['surface', 'mixed_layer'], **kw)),
            ('max_cape', lambda: max_cape.max_cape_cape_cin(p, t, m, **kw)),
            ('layers', lambda: layer_cape.cape_cin_layers(p, t, m, [{'top': 500.0}], **kw)),
            ('cape_3km', lambda: layer_cape.cape_3km(p, t, m, z, **kw)),
            ('hail_growth_zone', lambda: layer_cape.hail_growth_zone_cape(p, t, m, z, **kw)),
            ('inflow', lambda: kinematics.effective_inflow_layer(p, t, m, z, **kw))]


@pytest.mark.parametrize('kind', R.KINDS)
def test_dataarray_modules_pass_the_keyword_through(calls, kind):
    p, t, m = (_da(a, name=n) for a, n in zip(_small(np.float64), ('pressure', 'temperature', 'dewpoint')))
    for name, thunk in _mirror_calls(p, t, m, kind):
        n = len(calls)
        thunk()
        hum = [c[1] for c in calls[n:] if c[1] is not None]
        assert hum and set(hum) == {L.HUMIDITY[kind]}, (name, calls[n:])
    # the defaults are unchanged
    n = len(calls)
    max_cape.max_cape_cape_cin(p, t, m)
    kinematics.effective_inflow_layer(p, t, m)
    layer_cape.cape_cin_layers(p, t, m, [{'top': 500.0}])
    assert [c[1] for c in calls[n:] if c[1] is not None] == [0, 0, 0]


@pytest.mark.parametrize('units', ('%', 'percent', 'Percentage', ' % '))
def test_percent_guard(calls, units):
    p, t, m = _small(np.float64)
    P, T = _da(p, name='pressure'), _da(t, name='temperature')
    for name, thunk in _mirror_calls(P, T, _da(m * 100.0, units, 'dewpoint'), R.RELATIVE):
        with pytest.raises(ValueError, match='fraction'):
            thunk()
    assert not calls
    # a fraction, a moisture without units, and the other kinds pass
    for ok_units, kind in (('1', R.RELATIVE), (None, R.RELATIVE), ('kg kg-1', R.MIXING_RATIO), (units, 'dewpoint')):
        for name, thunk in _mirror_calls(P, T, _da(m, ok_units, 'dewpoint'), kind)[:1] + _mirror_calls(P, T, _da(m, ok_units, 'dewpoint'), kind)[7:9]:
            thunk()
    assert calls


# -- the kernel's resources ----------------------------------------------------------------------------------------------------
# (dtype, kind, 16-byte runs) -> VGPRs, waves per SIMD as recorded in _lib.py
RECORDED = L.HUMIDITY_RESOURCES


def test_every_instantiation_has_a_record():
    assert sorted(RECORDED) == sorted((d, k, v) for d in 'df' for k in (L.HUMIDITY['relative'], L.HUMIDITY['mixing_ratio']) for v in (0, 1))
    assert all(occ == 8 and vgprs <= 64 for vgprs, occ in RECORDED.values())       # 8 waves per SIMD: at most 64 VGPRs


@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_dewpoint_from is instantiated on dtype x kind x {16-byte runs, one column per lane}: eight kernels, none of which may
    use LDS or scratch or spill a vector register, each no worse than recorded in VGPRs and occupancy."""
    unit = [x for x in L.UNITS if x[1] == 'xp_humidity_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    found = {}
    for n, r in rec.items():
        m = re.search(r'k_dewpoint_fromI([df])Li([23])ELb([01])E', n)
        if m:
            found[(m.group(1), int(m.group(2)), int(m.group(3)))] = r
    assert sorted(found) == sorted(RECORDED), sorted(rec)
    for key, r in sorted(found.items()):
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['lds'] == 0 and r['vgprs'] <= RECORDED[key][0] and r['occupancy'] >= RECORDED[key][1], (key, r)
