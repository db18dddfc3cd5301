"""The classic sounding indices and the CCL without a GPU: the C ABI declarations, the array API and the DataArray module
around a stubbed launch, the NumPy restatement (tests/sounding_indices_restatement.py) against closed forms, a census of the
inputs the device tests run on (tests/sounding_indices_cases.py), and the kernel's resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import parcel_oracle as po
from oracle import thermo as O
from tests import sounding_indices_cases as K
from tests import sounding_indices_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import sounding_indices as mirror
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'
NAN = float('nan')


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_sounding_out') == [f[0] for f in L.SoundingOut._fields_]
    assert _struct_fields('xp_sounding_opts') == [f[0] for f in L.SoundingOpts._fields_]
    assert [f[0] for f in L.SoundingOut._fields_][:9] == list(L.SOUNDING_OUT) == list(R.KEYS)
    assert C.sizeof(L.SoundingOut) == 10 * 8 + 8 and C.sizeof(L.SoundingOpts) == 16
    got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES['xp_sounding_indices']]
    assert got == _prototypes()['xp_sounding_indices'] == ['pointer'] * 8 and 'xp_sounding_indices' in L.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'XP_ST_NO_CCL = %d\b' % L.ST_NO_CCL, hdr) and L.ST_NO_CCL == R.ST_NO_CCL == 128
    assert re.search(r'enum \{ XP_CCL_TOP = 0, XP_CCL_BOTTOM = 1 \};', hdr) and L.CCL_WHICH == {'top': 0, 'bottom': 1}
    assert 'UNPINNED' in hdr[hdr.index('The classic sounding indices'):hdr.index('xp_sounding_opts;')]
    assert [u for u in L.UNITS if u[1] == 'xp_sounding_tu.hip'] == [('sounding', 'xp_sounding_tu.hip', [])]


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def run(self, name, *args):
        seen.append((name, args))
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _cols(nlev=9, ncol=5, dtype=np.float32):
    return np.linspace(1000., 200., nlev, dtype=dtype)[:, None] * np.ones((1, ncol), dtype)


def test_sounding_indices_array_api_arguments(calls):
    p = _cols()
    res = api.sounding_indices(p, p, p, p, p, moist='table', which='bottom', mixed_layer_depth=100)
    name, (pv, tv, dv, uv, vv, opts, out) = calls[-1]
    assert name == 'xp_sounding_indices' and (pv.nlev, pv.ncol, pv.dtype, vv.ncol) == (9, 5, L.XP_F32, 5)
    assert all(x.data == p.ctypes.data for x in (pv, tv, dv, uv, vv))
    assert (opts.moist_mode, opts.ccl_which, opts.ccl_mixed_layer_depth) == (L.MOIST['table'], 1, 100.0)
    assert set(res) == set(R.KEYS) | {'status'}
    for k in R.KEYS:
        assert res[k].shape == (5,) and res[k].dtype == np.float32 and getattr(out, k) == res[k].ctypes.data
    assert out.status == res['status'].ctypes.data and res['status'].dtype == np.int32
    assert out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    # no winds: no SWEAT by default, null views; the defaults; want=
    p3 = p.reshape(9, 1, 5).astype(np.float64)
    res = api.sounding_indices(p3, p3, p3)
    pv, tv, dv, uv, vv, opts, out = calls[-1][1]
    assert uv is None and vv is None and dv.dtype == L.XP_F64 and out.sweat_index is None
    assert (opts.moist_mode, opts.ccl_which, opts.ccl_mixed_layer_depth) == (L.MOIST['exact'], 0, 0.0)
    assert set(res) == set(R.KEYS) - {'sweat_index'} | {'status'} and res['k_index'].shape == (1, 5)
    res = api.sounding_indices(p, p, p, want=('ccl_pressure',))
    out = calls[-1][1][6]
    assert set(res) == {'ccl_pressure', 'status'} and out.k_index is None and out.convective_temperature is None and out.ccl_pressure
    for kw in ({'u': p}, {'v': p}, {'which': 'middle'}, {'mixed_layer_depth': -1.0}, {'mixed_layer_depth': NAN}, {'want': ('k',)},
               {'want': ('sweat_index',)}, {'u': p[:4], 'v': p[:4]}):
        with pytest.raises(AssertionError):
            api.sounding_indices(p, p, p, **kw)
    with pytest.raises(KeyError):
        api.sounding_indices(p, p, p, moist='fast')


def test_thin_functions_reach_the_abi_with_their_outputs(calls):
    p = _cols()
    for fn, key in ((api.k_index, 'k_index'), (api.total_totals_index, 'total_totals'), (api.cross_totals, 'cross_totals'),
                    (api.vertical_totals, 'vertical_totals'), (api.showalter_index, 'showalter_index')):
        x = fn(p, p, p)
        out = calls[-1][1][6]
        assert x.shape == (5,) and getattr(out, key) == x.ctypes.data
        assert [k for k in R.KEYS if getattr(out, k)] == [key] and calls[-1][1][3] is None
    api.vertical_totals(p, p + 1)
    assert calls[-1][1][2].data == calls[-1][1][1].data                      # no dewpoint: the temperature stands in
    api.showalter_index(p, p, p, moist='table')
    assert calls[-1][1][5].moist_mode == L.MOIST['table']
    x = api.sweat_index(p, p, p, p, p)
    assert calls[-1][1][3] is not None and calls[-1][1][6].sweat_index == x.ctypes.data and calls[-1][1][6].k_index is None
    cp, ct, tc = api.ccl(p, p, p, mixed_layer_depth=50.0, which='bottom')
    opts, out = calls[-1][1][5:]
    assert (opts.ccl_which, opts.ccl_mixed_layer_depth) == (1, 50.0)
    assert (out.ccl_pressure, out.ccl_temperature, out.convective_temperature) == (cp.ctypes.data, ct.ctypes.data, tc.ctypes.data)
    assert out.k_index is None and out.showalter_index is None


def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def _names(ds):
    return list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys())


def test_mirror_wraps_the_array_api(calls):
    lev = np.arange(1., 10.)
    p, t, td, u = _grid(1050. - 100 * lev, 'p'), _grid(300. - 5 * lev, 't'), _grid(290. - 5 * lev, 'td'), _grid(2 * lev, 'u')
    ds = mirror.sounding_indices(p, t, td, u, u, which='bottom')
    name, args = calls[-1]
    assert name == 'xp_sounding_indices' and (args[0].nlev, args[0].ncol) == (9, 6) and args[3] is not None and args[5].ccl_which == 1
    assert _names(ds) == list(R.KEYS) + ['status']
    for k in R.KEYS:
        assert ds[k].dims == ('lat', 'lon') and ds[k].shape == (2, 3) and ds[k].name == k
        assert 'long_name' in ds[k].attrs and 'units' in ds[k].attrs
    assert ds['ccl_pressure'].attrs['units'] == 'hPa' and ds['k_index'].attrs['units'] == 'K' and ds['status'].dims == ('lat', 'lon')
    ds = mirror.sounding_indices(p, t, td, want=('total_totals',))
    assert _names(ds) == ['total_totals', 'status'] and calls[-1][1][3] is None
    for fn, key in ((mirror.k_index, 'k_index'), (mirror.total_totals_index, 'total_totals'), (mirror.cross_totals, 'cross_totals'),
                    (mirror.vertical_totals, 'vertical_totals'), (mirror.showalter_index, 'showalter_index')):
        x = fn(p, t, td)
        assert x.name == key and x.dims == ('lat', 'lon') and [k for k in R.KEYS if getattr(calls[-1][1][6], k)] == [key]
    assert mirror.sweat_index(p, t, td, u, u).name == 'sweat_index' and calls[-1][1][4] is not None
    ds = mirror.ccl(p, t, td, mixed_layer_depth=100.0)
    assert _names(ds) == list(R.CCL_KEYS) and calls[-1][1][5].ccl_mixed_layer_depth == 100.0
    assert ds['convective_temperature'].attrs['units'] == 'K'


# -- the restatement against closed forms ---------------------------------------------------------------------------------
def test_levels_on_the_isobars_give_the_textbook_indices():
    p, t, td, u, v = K.mandatory_columns()
    for c in range(p.shape[1]):
        r = R.column(p[:, c], t[:, c], td[:, c], u[:, c], v[:, c])
        t850, t700, t500, td850, td700 = t[2, c], t[3, c], t[4, c], td[2, c], td[3, c]
        assert (r['t850'], r['td850'], r['t700'], r['td700'], r['t500']) == (t850, td850, t700, td700, t500)
        assert r['vertical_totals'] == t850 - t500 and r['cross_totals'] == td850 - t500
        assert r['total_totals'] == (t850 - t500) + (td850 - t500)
        assert r['k_index'] == ((t850 - t500) + (td850 - 273.15)) - (t700 - td700)
        assert (r['u850'], r['v850'], r['u500'], r['v500']) == (u[2, c], v[2, c], u[4, c], v[4, c]) and r['status'] == 0
    # the first column by hand: T 289.9 / 280.1 / 262.4, Td 287.9 / 273.6
    r = R.column(p[:, 0], t[:, 0], td[:, 0])
    assert abs(r['vertical_totals'] - 27.5) < 1e-12 and abs(r['cross_totals'] - 25.5) < 1e-12 and abs(r['total_totals'] - 53.0) < 1e-12
    assert abs(r['k_index'] - (27.5 + 14.75 - 6.5)) < 1e-12


def test_interpolation_is_linear_in_ln_p():
    """T = a + b ln p and Td = c + d ln p on levels that miss every isobar: the isobar values are the profile's."""
    p = np.array([1013.0, 930.0, 871.0, 790.0, 655.0, 540.0, 433.0, 310.0])
    t, td = 20.0 + 40.0 * np.log(p), -30.0 + 46.0 * np.log(p)
    r = R.column(p, t, td)
    for P in (850, 700, 500):
        assert abs(r['t%d' % P] - (20.0 + 40.0 * np.log(P))) < 1e-11 and abs(r['td%d' % P] - (-30.0 + 46.0 * np.log(P))) < 1e-11
    assert abs(r['vertical_totals'] - 40.0 * np.log(850.0 / 500.0)) < 1e-11 and r['status'] & R.ST_NO_LAYER == 0


def _sweat(d850, f850, d500, f500, td850=285.15, tt=55.0):
    return R.sweat_terms(td850, tt, *K.wind_from(f850, d850), *K.wind_from(f500, d500))


def test_sweat_shear_term_and_its_conditions():
    s = _sweat(180.0, 30.0, 250.0, 50.0)                                      # by hand: 12 * 12 + 20 * 6 + 2 * 30 + 50 + 125 (sin 70 + 0.2)
    want = 144.0 + 120.0 + 60.0 + 50.0 + 125.0 * (np.sin(np.deg2rad(70.0)) + 0.2)
    assert s['shear_on'] and abs(s['sweat_index'] - want) < 1e-9 and abs(s['d850'] - 180.0) < 1e-12 and abs(s['f500'] - 50.0) < 1e-12
    # each condition failing in turn, and calm winds
    for kw in (dict(d850=120.0), dict(d850=255.0, d500=300.0), dict(d500=200.0, d850=150.0), dict(d500=320.0), dict(d850=240.0, d500=220.0),
               dict(f850=14.0), dict(f500=14.0), dict(f850=0.0, f500=0.0)):
        a = dict(d850=180.0, f850=30.0, d500=250.0, f500=50.0)
        a.update(kw)
        s = _sweat(**a)
        assert not s['shear_on'] and s['shear'] == 0.0, kw
        assert abs(s['sweat_index'] - (144.0 + 120.0 + 2.0 * a['f850'] + a['f500'])) < 1e-9, kw
    # the thermodynamic terms floor at zero; a northerly wind is 360, not 0
    s = _sweat(180.0, 20.0, 250.0, 20.0, td850=268.15, tt=40.0)
    assert abs(s['sweat_index'] - (60.0 + 125.0 * (np.sin(np.deg2rad(70.0)) + 0.2))) < 1e-9
    assert R.knots_and_direction(0.0, -5.0)[1] == 360.0 and R.knots_and_direction(-5.0, 0.0)[1] == 90.0


def test_sweat_in_a_column_uses_the_interpolated_winds():
    p, t, td, u, v = (a[:, 0] for a in K.mandatory_columns())
    r = R.column(p, t, td, u, v)
    s = R.sweat_terms(td[2], r['total_totals'], u[2], v[2], u[4], v[4])
    assert r['sweat_index'] == s['sweat_index'] and s['shear_on'] and abs(s['d850'] - 180.0) < 1e-9 and abs(s['d500'] - 250.0) < 1e-9
    # winds on other levels than the thermodynamics: u, v at 850 hPa come from the wind-valid neighbours 925 and 700
    u2, v2 = u.copy(), v.copy()
    u2[2] = v2[2] = NAN
    r2 = R.column(p, t, td, u2, v2)
    f = (np.log(850.0) - np.log(700.0)) / (np.log(925.0) - np.log(700.0))
    assert abs(r2['u850'] - (u[3] + (u[1] - u[3]) * f)) < 1e-12 and r2['t850'] == t[2] and not np.isnan(r2['sweat_index'])


def test_very_dry_parcel_takes_the_dry_branch():
    p = np.array([1000.0, 850.0, 700.0, 500.0, 300.0])
    t = np.array([305.0, 295.0, 283.0, 262.0, 230.0])
    td = t - np.array([40.0, 62.0, 50.0, 40.0, 30.0])
    r = R.column(p, t, td)
    assert r['lcl_pressure'] <= 500.0 and r['status'] == 0
    assert r['parcel_500'] == 295.0 * (500.0 / 850.0) ** O.KAPPA and r['showalter_index'] == 262.0 - r['parcel_500']
    # a moist one goes through the moist adiabat and ends warmer than the dry adiabat would leave it
    r = R.column(p, t, t - 2.0)
    lcl = po.lcl(850.0, 295.0, 293.0, per_column=True)
    assert r['lcl_pressure'] == lcl['lcl_pressure'] > 500.0
    assert r['parcel_500'] == po.moist_lapse(np.array([500.0]), lcl['lcl_temperature'], lcl['lcl_pressure'], moist='rk4')[0]
    assert r['parcel_500'] > 295.0 * (500.0 / 850.0) ** O.KAPPA + 10.0


def test_saturated_surface_is_its_own_ccl():
    p = np.array([1003.7, 950.0, 900.0, 800.0, 650.0, 500.0])
    t = np.array([297.3, 294.0, 291.0, 285.0, 275.0, 262.0])
    td = t - np.array([0.0, 4.0, 5.0, 8.0, 12.0, 20.0])
    r = R.column(p, t, td, which='bottom')
    assert r['ccl_pressure'] == p[0] and r['ccl_temperature'] == td[0] and r['convective_temperature'] == t[0] and r['status'] == 0
    # by the round trip through r the start level's rt would be off by rounding: the rule keeps the zero exact
    assert R.ccl_line(p, t, td)[2][0] == td[0]


def test_ccl_crossings_top_and_bottom():
    """rt against a temperature with an inversion: three crossings, 'bottom' the first and 'top' the last."""
    p = np.array([1000.0, 950.0, 900.0, 850.0, 800.0, 700.0, 500.0])
    td0 = 290.0
    pv, tv, rt, _ = R.ccl_line(p, np.full(7, 400.0), np.r_[td0, np.full(6, 200.0)])
    t = rt + np.array([4.0, 1.0, -1.0, 2.0, 3.0, -2.0, -9.0])               # rt - T: - - + - - + +
    r = {w: R.column(p, t, np.r_[td0, t[1:] - 5.0], which=w) for w in ('top', 'bottom')}
    assert len(r['top']['crossings']) == 3 and r['top']['status'] == 0
    assert 900.0 < r['bottom']['ccl_pressure'] < 950.0 and 700.0 < r['top']['ccl_pressure'] < 800.0
    # rt - T is linear in ln p between the levels: 1 -> -1 crosses half way in ln p
    assert abs(r['bottom']['ccl_pressure'] - np.sqrt(950.0 * 900.0)) < 1e-9
    assert abs(r['bottom']['ccl_temperature'] - 0.5 * (rt[1] + rt[2])) < 1e-9
    tc = r['top']['ccl_temperature'] * (1000.0 / r['top']['ccl_pressure']) ** O.KAPPA
    assert r['top']['convective_temperature'] == tc > r['bottom']['convective_temperature']
    # a level exactly on the line is the crossing itself
    t2 = t.copy()
    t2[2] = rt[2]
    r2 = R.column(p, t2, np.r_[td0, t2[1:] - 5.0], which='bottom')
    assert r2['ccl_pressure'] == 900.0 and r2['ccl_temperature'] == rt[2]


def test_no_ccl_and_mixed_layer_ccl():
    p = np.array([1000.0, 900.0, 800.0, 650.0, 500.0, 300.0])
    r = R.column(p, np.full(6, 300.0), np.full(6, 290.0))                     # isothermal: rt falls away from T
    assert r['status'] == R.ST_NO_CCL and all(np.isnan(r[k]) for k in R.CCL_KEYS) and not np.isnan(r['k_index'])
    # a mixed layer drier than the surface: its CCL lies higher
    t = np.array([300.0, 292.0, 284.0, 273.0, 259.0, 228.0])
    td = t - np.array([4.0, 8.0, 9.0, 12.0, 18.0, 30.0])
    sfc, ml = R.column(p, t, td), R.column(p, t, td, mixed_layer_depth=100.0)
    w = po.mixed_parcel(p, t, td, depth=100.0)['mixing_ratio']
    assert ml['ccl_pressure'] < sfc['ccl_pressure'] and w < O.saturation_mixing_ratio(p[0], td[0])
    assert abs(ml['ccl_temperature'] - O.dewpoint(O.vapor_pressure(ml['ccl_pressure'], w))) < 0.05


def test_dropped_levels_and_span_failures():
    p, t, td, u, v = (a[:, 1].copy() for a in K.mandatory_columns())
    full = R.column(p, t, td, u, v)
    # a NaN level is dropped, not interpolated through: 850 hPa then comes from 925 and 700
    t2 = t.copy()
    t2[2] = NAN
    r = R.column(p, t2, td, u, v)
    f = (np.log(850.0) - np.log(700.0)) / (np.log(925.0) - np.log(700.0))
    assert abs(r['t850'] - (t[3] + (t[1] - t[3]) * f)) < 1e-12 and abs(r['td850'] - (td[3] + (td[1] - td[3]) * f)) < 1e-12
    assert r['u850'] == u[2] and r['status'] == 0
    # inserting all-NaN levels changes nothing
    ins = lambda a: np.insert(a, [1, 3, 5], NAN)
    r = R.column(ins(p), ins(t), ins(td), ins(u), ins(v))
    assert all(r[k] == full[k] for k in R.KEYS) and r['status'] == full['status']
    # span: the lowest valid level above 850 hPa; the highest below 500 hPa; the same of the wind levels alone
    for cut in (slice(3, None), slice(0, 4)):
        r = R.column(p[cut], t[cut], td[cut], u[cut], v[cut])
        assert r['status'] & R.ST_NO_LAYER and all(np.isnan(r[k]) for k in R.INDEX_KEYS) and not np.isnan(r['ccl_pressure'])
    for gone in (slice(0, 3), slice(4, None)):
        u2, v2 = u.copy(), v.copy()
        u2[gone] = v2[gone] = NAN
        r = R.column(p, t, td, u2, v2)
        assert r['status'] == 0 and np.isnan(r['sweat_index']) and r['k_index'] == full['k_index'] and r['showalter_index'] == full['showalter_index']
    r = R.column(np.full(4, NAN), t[:4], td[:4])
    assert r['status'] == R.ST_NO_LAYER | R.ST_NO_CCL and all(np.isnan(r[k]) for k in R.KEYS)


def test_near_tie_names_what_it_should():
    p, t, td, u, v = (a[:, 0].copy() for a in K.mandatory_columns())
    assert not R.near_tie(p, t, td, u, v)
    pv, tv, rt, _ = R.ccl_line(p, t, td)
    t2 = t.copy()
    t2[3] = rt[3] + 5e-7
    assert R.near_tie(p, t2, td, u, v) and not R.near_tie(p, np.r_[td[0], t[1:]], td, u, v)     # a saturated start level is no tie
    u2, v2 = u.copy(), v.copy()
    u2[2], v2[2] = K.wind_from(15.0 * (1 + 1e-12), 180.0)
    assert R.near_tie(p, t, td, u2, v2)
    u2[2], v2[2] = K.wind_from(25.0, 130.0 * (1 + 1e-11))
    assert R.near_tie(p, t, td, u2, v2)


# -- a census of the device tests' inputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(K.GRIDS))
def test_input_census(name):
    """What the device tests compare is not hollowed out by their exclusions: per grid, near-tie columns are at most 1 %; at
    least 5 columns have two or more distinct crossings ('top' differs from 'bottom'); the SWEAT shear term is on in at least
    10 % of the columns and off in at least 10 %; at least 5 % do not span 850 ... 500 hPa; at least one has no CCL."""
    nlev, ncol, seed = K.GRIDS[name]
    p, t, td, u, v = K.inputs(nlev, ncol, seed)
    ref = R.grid(p, t, td, u, v)
    tie = sum(R.near_tie(p[:, c], t[:, c], td[:, c], u[:, c], v[:, c], col=ref['columns'][c]) for c in range(ncol))
    multi = sum(len(set(r['crossings'])) >= 2 for r in ref['columns'])
    on = sum(bool(r['sweat'] and r['sweat']['shear_on']) for r in ref['columns'])
    off = sum(bool(r['sweat'] and not r['sweat']['shear_on']) for r in ref['columns'])
    no_layer, no_ccl = int(np.sum(ref['status'] & R.ST_NO_LAYER != 0)), int(np.sum(ref['status'] & R.ST_NO_CCL != 0))
    print(name, dict(tie=tie, multi=multi, on=on, off=off, no_layer=no_layer, no_ccl=no_ccl))
    assert tie <= 0.01 * ncol and multi >= 5 and on >= 0.1 * ncol and off >= 0.1 * ncol and no_layer >= 0.05 * ncol and no_ccl >= 1
    ml = R.grid(p, t, td, cols=range(0, ncol, 3), mixed_layer_depth=100.0)
    assert np.isfinite(ml['ccl_pressure']).sum() >= 0.5 * len(ml['ccl_pressure'])
    top = np.array([r['crossings'][-1][0] if r['crossings'] else NAN for r in ref['columns']])
    bot = np.array([r['crossings'][0][0] if r['crossings'] else NAN for r in ref['columns']])
    assert np.sum(top < bot) == multi


# -- the kernel's resources -------------------------------------------------------------------------------------------------
@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_sounding is instantiated on dtype x {winds or not} x {no CCL, surface CCL, mixed-layer CCL}: twelve kernels, none of
    which may use scratch or spill a vector register, and none below four waves per SIMD."""
    unit = [x for x in L.UNITS if x[1] == 'xp_sounding_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    walk = {}
    for n, r in rec.items():
        m = re.search(r'k_soundingI([df])Lb([01])ELi(\d)E', n)
        if m:
            walk[(m.group(1), int(m.group(2)), int(m.group(3)))] = r
    assert sorted(walk) == sorted((t, w, c) for t in 'df' for w in (0, 1) for c in (0, 1, 2)), sorted(rec)
    for key, r in walk.items():
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['occupancy'] >= 4 and r['lds'] == 8 * (5 * 257 + 193), (key, r)
