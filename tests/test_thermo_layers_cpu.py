"""Temperature and humidity over caller-chosen layers without a GPU: the C ABI declarations, the array API and the DataArray
module around a stubbed launch, the NumPy restatement (tests/thermo_layers_restatement.py) against closed forms, and the
kernel's resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import thermo as O
from tests import thermo_layers_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import thermo_layers as mirror
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'
NAN = float('nan')
TK = R.THERMO_KEYS


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_thermo_layers_out') == [f[0] for f in L.ThermoLayersOut._fields_]
    assert [f[0] for f in L.ThermoLayersOut._fields_][:9] == list(L.THERMO_LAYERS_OUT) == list(TK)
    assert set(L.THERMO_LAYERS_NEEDS) == set(TK)
    got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES['xp_thermo_layers']]
    assert got == _prototypes()['xp_thermo_layers'] and 'xp_thermo_layers' in L.SYMBOLS and len(got) == 10
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'void \*theta_e_min\[4\], \*theta_e_min_pressure\[4\], \*theta_e_max\[4\], \*theta_e_max_pressure\[4\];', hdr)
    assert L.THERMO_MAX_LAYERS == 4 and C.sizeof(L.ThermoLayersOut) == 9 * 4 * 8 + 16
    assert 'rho_l = %r' % R.RHO_L in hdr and 'constexpr double RHO_L = %r;' % R.RHO_L in open(os.path.join(L.SRC_DIR, 'xp_thermo_layers.hpp')).read()
    assert [u for u in L.UNITS if u[1] == 'xp_thermo_layers_tu.hip'] == [('thermo_layers', 'xp_thermo_layers_tu.hip', L.THERMO_LAYERS_FLAGS)]


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


def _layers(args):
    n, arr = args[4], args[5]
    return [(arr[i].kind, arr[i].bottom, arr[i].top) for i in range(n)]


def test_thermo_layers_array_api_arguments(calls):
    p = _cols()
    pb, pt = np.linspace(900., 800., 5), np.linspace(500., 400., 5)
    res = api.thermo_layers(p, p, p, p, layers=[{'bottom': 700, 'top': 500}, {'depth': 150}, {'top_height': 3000}, {'bottom': pb, 'top': pt}])
    name, args = calls[-1]
    pv, tv, dv, zv, n, arr, bc, tc, out = args
    assert name == 'xp_thermo_layers' and (pv.nlev, pv.ncol, pv.dtype, zv.ncol) == (9, 5, L.XP_F32, 5) and n == 4
    assert all(v.data == p.ctypes.data for v in (pv, tv, dv, zv))
    got = _layers(args)
    assert got[0] == (L.LAYER_PRESSURE, 700.0, 500.0) and got[1][0] == L.LAYER_PRESSURE_DEPTH and np.isnan(got[1][1]) and got[1][2] == 150.0
    assert got[2] == (L.LAYER_HEIGHT, 0.0, 3000.0) and got[3][0] == L.LAYER_PRESSURE and np.isnan(got[3][1]) and np.isnan(got[3][2])
    assert [bc[i] for i in range(3)] == [None] * 3 and [tc[i] for i in range(3)] == [None] * 3 and bc[3] and tc[3] and bc[3] != tc[3]
    assert set(res) == set(TK) | {'status'}
    assert res['thickness'].shape == (4, 5) and res['thickness'].dtype == np.float32 and res['status'].dtype == np.int32
    assert out.theta_e_max_pressure[3] == res['theta_e_max_pressure'][3].ctypes.data and out.lapse_rate[0] == res['lapse_rate'][0].ctypes.data
    assert out.status == res['status'].ctypes.data and out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    # the open top, a view left out, want=, and the default want of a call without temperature and height
    p3 = p.reshape(9, 1, 5).astype(np.float64)
    res = api.thermo_layers(p3, dewpoint=p3, layers=[{'bottom': None, 'top': None}, ('pressure', 850.0, None)])
    pv, tv, dv, zv, n, arr, bc, tc, out = calls[-1][1]
    assert tv is None and zv is None and dv.dtype == L.XP_F64 and n == 2 and bc is None and tc is None
    assert set(res) == {'precipitable_water', 'mean_mixing_ratio', 'status'} and res['precipitable_water'].shape == (2, 1, 5)
    assert np.isnan(arr[0].bottom) and np.isnan(arr[0].top) and arr[1].bottom == 850.0 and np.isnan(arr[1].top)
    assert out.precipitable_water[2] is None and out.thickness[0] is None and out.theta_e_min[0] is None
    res = api.thermo_layers(p, p, None, p, layers=[{'top_height': 500}], want=('lapse_rate',))
    assert set(res) == {'lapse_rate', 'status'} and calls[-1][1][2] is None and calls[-1][1][8].thickness[0] is None
    for bad in ([], [{'depth': 100}] * 5, [{'bottom': 900}], [{'top': 300, 'depth': 100}], [{'top_height': 500, 'bottom': 900}],
                [('sigma', 1, 2)], [{'bottom': pb[:3], 'top': 500}]):
        with pytest.raises(AssertionError):
            api.thermo_layers(p, p, p, p, layers=bad)
    with pytest.raises(AssertionError):
        api.thermo_layers(p, p, p, layers=[{'top_height': 500}])                       # a layer by height without height
    with pytest.raises(AssertionError):
        api.thermo_layers(p, p, p[:4], layers=[{'depth': 100}])
    with pytest.raises(AssertionError):
        api.thermo_layers(p, p, p, layers=[{'depth': 100}], want=('mean',))
    for want, views in ((('mean_relative_humidity',), (None, p, None)), (('precipitable_water',), (p, None, None)),
                        (('thickness',), (p, p, None)), (('theta_e_min',), (None, p, p))):
        with pytest.raises(AssertionError):
            api.thermo_layers(p, *views, layers=[{'depth': 100}], want=want)


def test_convenience_functions_reach_the_abi_with_their_layers(calls):
    p = _cols()
    pw = api.precipitable_water(p, p)
    args = calls[-1][1]
    assert np.isnan(_layers(args)[0][1]) and np.isnan(_layers(args)[0][2]) and _layers(args)[0][0] == L.LAYER_PRESSURE
    assert args[1] is None and args[3] is None and args[2] is not None and pw.shape == (5,)
    assert args[8].precipitable_water[0] == pw.ctypes.data and args[8].mean_mixing_ratio[0] is None
    api.precipitable_water(p, p, bottom=900.0, top=np.linspace(500., 400., 5))
    args = calls[-1][1]
    assert _layers(args)[0][1] == 900.0 and args[6] is None and args[7][0]
    rh = api.mean_relative_humidity(p, p, p)
    args = calls[-1][1]
    assert _layers(args) == [(L.LAYER_PRESSURE, 700.0, 500.0)] and args[8].mean_relative_humidity[0] == rh.ctypes.data and args[3] is None
    api.mean_relative_humidity(p, p, p, height=p, layer={'bottom_height': 3000, 'top_height': 6000})
    assert _layers(calls[-1][1]) == [(L.LAYER_HEIGHT, 3000.0, 6000.0)] and calls[-1][1][3] is not None
    lr, th = api.layer_lapse_rate(p, p, p, layer=('pressure', 850.0, 500.0))
    args = calls[-1][1]
    assert _layers(args) == [(L.LAYER_PRESSURE, 850.0, 500.0)] and args[2] is None
    assert (args[8].lapse_rate[0], args[8].thickness[0]) == (lr.ctypes.data, th.ctypes.data) and args[8].precipitable_water[0] is None

    del calls[:]
    thick, lapse = api.hail_growth_zone_thickness(p, p, p)
    names = [n for n, _ in calls]
    assert names == ['xp_crossing_level', 'xp_interp_level', 'xp_crossing_level', 'xp_interp_level', 'xp_thermo_layers']
    assert calls[0][1][2] == 263.15 and calls[2][1][2] == 243.15
    args = calls[-1][1]
    assert args[6][0] and args[7][0] and args[2] is None and _layers(args)[0][0] == L.LAYER_PRESSURE
    assert (args[8].thickness[0], args[8].lapse_rate[0]) == (thick.ctypes.data, lapse.ctypes.data)

    del calls[:]
    ted = api.theta_e_difference(p, p, p, p)
    (name, args), = calls
    assert _layers(args) == [(L.LAYER_HEIGHT, 0.0, 3000.0)] and args[8].theta_e_min[0] and args[8].theta_e_max_pressure[0]
    assert args[8].precipitable_water[0] is None and ted.shape == (5,) and ted.dtype == np.float32


def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def _horiz(val, name):
    return DataArray(np.full((2, 3), val), dims=('lat', 'lon'), coords={'lat': [10., 20.], 'lon': [1., 2., 3.]}, name=name)


def _names(ds):
    return list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys())


def test_mirror_wraps_the_array_api(calls):
    lev = np.arange(1., 10.)
    p, t, td, z = _grid(1000. - 50 * lev, 'p'), _grid(300. - 5 * lev, 't'), _grid(290. - 5 * lev, 'td'), _grid(500. * lev, 'z')
    ds = mirror.thermo_layers(p, t, td, z, layers=[{'top_height': 3000}, {'bottom': _horiz(800., 'pb'), 'top': None}])
    name, args = calls[-1]
    assert name == 'xp_thermo_layers' and (args[0].nlev, args[0].ncol, args[4]) == (9, 6, 2)
    assert args[6][0] is None and args[6][1] and args[7] is None and np.isnan(args[5][1].top)
    assert _names(ds) == list(TK) + ['status']
    for k in TK:
        assert ds[k].dims == ('thermo_layer', 'lat', 'lon') and ds[k].shape == (2, 2, 3) and ds[k].name == k
        assert 'long_name' in ds[k].attrs and 'units' in ds[k].attrs
    assert ds['precipitable_water'].attrs['units'] == 'mm' and ds['theta_e_max_pressure'].attrs['units'] == 'hPa'
    assert list(ds['thickness'].coords['thermo_layer']) == [0, 1] and ds['status'].dims == ('lat', 'lon')
    ds = mirror.thermo_layers(p, dewpoint=td, layers=[{'depth': 100.0}], want=('mean_mixing_ratio',))
    assert _names(ds) == ['mean_mixing_ratio', 'status'] and calls[-1][1][1] is None
    pw = mirror.precipitable_water(p, td, top=_horiz(400., 'pt'))
    assert calls[-1][1][7][0] and pw.dims == ('lat', 'lon') and pw.name == 'precipitable_water' and pw.attrs['units'] == 'mm'
    rh = mirror.mean_relative_humidity(p, t, td, layer={'bottom': 850, 'top': 500})
    assert _layers(calls[-1][1]) == [(L.LAYER_PRESSURE, 850.0, 500.0)] and rh.name == 'mean_relative_humidity'
    ds = mirror.layer_lapse_rate(p, t, z)
    assert _names(ds) == ['lapse_rate', 'thickness'] and ds['lapse_rate'].attrs['units'] == 'K km$^{-1}$' and ds['thickness'].dims == ('lat', 'lon')
    ds = mirror.hail_growth_zone_thickness(p, t, z)
    assert calls[-1][0] == 'xp_thermo_layers' and _names(ds) == ['hail_growth_zone_thickness', 'hail_growth_zone_lapse_rate']
    ted = mirror.theta_e_difference(p, t, td, z)
    assert _layers(calls[-1][1]) == [(L.LAYER_HEIGHT, 0.0, 3000.0)] and ted.name == 'theta_e_difference' and ted.attrs['units'] == 'K'


# -- the restatement against closed forms ---------------------------------------------------------------------------------
def _column(nlev=24, top=13000.0, z0=150.0, p0=1005.0):
    z = z0 + np.linspace(0.0, top, nlev) + np.r_[0.0, np.sin(np.arange(1, nlev)) * 60.0]
    return p0 * np.exp(-(z - z0) / 8000.0), z


def _td_of_w(w, p):
    """the dewpoint at which the mixing ratio at pressure p is w"""
    return O.dewpoint(O.vapor_pressure(p, w))


def test_constant_mixing_ratio_gives_precipitable_water_in_closed_form():
    p, z = _column()
    w = 0.008
    td = _td_of_w(w, p)
    t = td + 5.0
    # bounds on levels: w at an added bound point, from the interpolated dewpoint, would differ from w in the 6th digit
    layers = [(R.PRESSURE, p[2], p[11]), (R.PRESSURE, NAN, p[7]), (R.PRESSURE, p[4], NAN)]
    r = R.thermo_layers_column(p, t, td, z, layers)
    assert r['status'] == 0
    for j, (pb, pt) in enumerate([(p[2], p[11]), (p[0], p[7]), (p[4], p[-1])]):
        want = w * (pb - pt) * 1e5 / (R.G * R.RHO_L)
        assert abs(r['precipitable_water'][j] - want) < 1e-10 * want and abs(r['mean_mixing_ratio'][j] - w) < 1e-13
        assert r['thickness'][j] == z[list(p).index(pt)] - z[list(p).index(pb)]
    assert 20.0 < r['precipitable_water'][1] / (p[0] - p[7]) * 250.0 < 21.0          # 8 g/kg over 250 hPa: about 20.4 mm
    between = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, 0.5 * (p[2] + p[3]), 0.5 * (p[10] + p[11]))])
    assert abs(between['mean_mixing_ratio'][0] - w) < 1e-5 and between['mean_mixing_ratio'][0] != w


def test_saturation_gives_unit_relative_humidity_and_isothermal_no_lapse():
    # pressures and bounds with two binary places: every trapezoid of rh = 1 and their sum are exact, so the mean is 1.0 itself
    p = 1000.0 - 37.5 * np.arange(24)
    z = 150.0 + 8000.0 * np.log(1000.0 / p)
    t = 288.0 - 6.5e-3 * (z - z[0])
    exact = [(R.PRESSURE, 843.25, 311.75), (R.PRESSURE_DEPTH, NAN, 123.5), (R.PRESSURE, 925.0, 700.0), (R.PRESSURE, NAN, NAN)]
    r = R.thermo_layers_column(p, t, t.copy(), z, exact)
    assert r['status'] == 0 and np.all(r['mean_relative_humidity'] == 1.0)
    layers = exact[:2] + [(R.HEIGHT, 250.0, 3333.0)] + exact[3:]
    r = R.thermo_layers_column(p, t, t.copy(), z, layers)
    assert r['status'] == 0 and np.all(np.abs(r['mean_relative_humidity'] - 1.0) < 1e-14)
    half = R.thermo_layers_column(p, t, O.dewpoint(0.5 * O.saturation_vapor_pressure(t)), z, [(R.PRESSURE, p[2], p[10]), (R.PRESSURE, NAN, NAN)])
    assert np.all(np.abs(half['mean_relative_humidity'] - 0.5) < 1e-12)            # (bounds on levels: rh is not linear in ln p)
    iso = R.thermo_layers_column(p, np.full_like(p, 250.0), np.full_like(p, 240.0), z, layers)
    assert iso['status'] == 0 and np.all(iso['lapse_rate'] == 0.0) and np.all(iso['thickness'] > 0.0)
    assert np.array_equal(r['thickness'], iso['thickness'])


def test_linear_temperature_gives_its_slope_and_bounds_interpolate_in_ln_p():
    p, z = _column()
    t = 290.0 - 7.25e-3 * (z - z[0])
    td = t - 3.0
    # a thin layer inside one interval: T and z are both linear in ln p there, so the slope is that of the two levels
    pb, pt = p[5] - 0.3 * (p[5] - p[6]), p[5] - 0.6 * (p[5] - p[6])
    r = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, pb, pt), (R.PRESSURE, p[3], p[9]), (R.HEIGHT, z[2] - z[0], z[8] - z[0])])
    assert r['status'] == 0 and np.all(np.abs(r['lapse_rate'] - 7.25) < 1e-9)
    f = (np.log(pb) - np.log(p[6])) / (np.log(p[5]) - np.log(p[6]))
    g = (np.log(pt) - np.log(p[6])) / (np.log(p[5]) - np.log(p[6]))
    assert abs(r['thickness'][0] - (g - f) * (z[5] - z[6])) < 1e-9 and r['thickness'][1] == z[9] - z[3]
    assert abs(r['thickness'][2] - (z[8] - z[2])) < 1e-9
    # e_s, w, rh, theta_e at the bound point come from the interpolated T and Td
    tb, tdb = t[6] + f * (t[5] - t[6]), td[6] + f * (td[5] - td[6])
    assert r['theta_e_max_pressure'][0] in (pb, pt) and r['theta_e_min_pressure'][0] in (pb, pt)
    th = O.equivalent_potential_temperature(pb, tb, tdb)
    assert th in (r['theta_e_min'][0], r['theta_e_max'][0])


def test_open_top_equals_an_explicit_top_at_the_highest_valid_pressure():
    p, z = _column()
    t = 288.0 - 6.5e-3 * (z - z[0]) + np.cos(z / 700.0)
    td = t - 2.0 - np.sin(z / 900.0) ** 2 * 8.0
    t[-1] = NAN                                          # the highest VALID level is the one below
    for bottom in (NAN, 900.0, p[3]):
        a = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, bottom, NAN)])
        b = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, bottom, p[-2])])
        assert a['status'] == b['status'] == 0 and all(np.array_equal(a[k], b[k]) for k in TK + R.GAPS)
    # per-column bounds: the same numbers as scalars; a NaN bottom is p0, a NaN top no layer (not the open one)
    a = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, NAN, NAN)] * 3, [850.0, NAN, 850.0], [400.0, 400.0, NAN])
    b = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, 850.0, 400.0), (R.PRESSURE, NAN, 400.0)])
    assert a['status'] == R.ST_NO_LAYER and b['status'] == 0 and np.isnan(a['precipitable_water'][2])
    assert all(np.array_equal(a[k][:2], b[k]) for k in TK)


def test_theta_e_tie_goes_to_the_first_point(monkeypatch):
    p, z = _column()
    t, td = np.full_like(p, 280.0), np.full_like(p, 270.0)
    th = O.equivalent_potential_temperature(p, t, td)
    assert np.all(np.diff(th) > 0)                       # isothermal: theta_e rises with height
    r = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, p[2], p[9])])
    assert (r['theta_e_min_pressure'][0], r['theta_e_max_pressure'][0]) == (p[2], p[9]) and r['theta_e_min'][0] == th[2]
    assert r['gap_min'][0] == (th[3] - th[2]) / th[2] and r['gap_max'][0] == (th[9] - th[8]) / th[9]
    # exact ties need equal bits, which distinct pressures do not give: a theta_e of two plateaus stands in for the formula
    monkeypatch.setattr(O, 'equivalent_potential_temperature', lambda pp, tt, dd: np.where(np.asarray(pp) > p[6], 300.0, 310.0))
    pb = 0.5 * (p[2] + p[3])
    r = R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, pb, p[9]), (R.PRESSURE, p[7], p[9]), (R.PRESSURE, NAN, p[5])])
    assert (r['theta_e_min_pressure'][0], r['theta_e_max_pressure'][0]) == (pb, p[6])         # the first of each plateau
    assert (r['theta_e_min'][0], r['theta_e_max'][0]) == (300.0, 310.0) and r['gap_min'][0] == 0.0 and r['gap_max'][0] == 0.0
    assert (r['theta_e_min_pressure'][1], r['theta_e_max_pressure'][1]) == (p[7], p[7])       # one plateau: both the first point
    assert (r['theta_e_min_pressure'][2], r['theta_e_max_pressure'][2]) == (p[0], p[0])
    assert R.extreme_gaps(np.array([1.0, 1.0, 2.0])) == (0.0, 0.5) and R.extreme_gaps(np.array([5.0])) == (np.inf, np.inf)


def test_missing_levels_are_dropped():
    p, z = _column()
    t = 288.0 - 6.5e-3 * (z - z[0]) + np.cos(z / 700.0)
    td = t - 2.0 - np.sin(z / 900.0) ** 2 * 8.0
    layers = [(R.PRESSURE, 850.0, 300.0), (R.PRESSURE_DEPTH, NAN, 100.0), (R.HEIGHT, 0.0, 6000.0), (R.PRESSURE, NAN, NAN)]
    t2, td2, z2, p2 = t.copy(), td.copy(), z.copy(), p.copy()
    t2[3], z2[9], p2[5], td2[12] = NAN, NAN, NAN, NAN
    keep = np.ones(p.size, bool)
    keep[[3, 5, 9, 12]] = False
    got = R.thermo_layers_column(p2, t2, td2, z2, layers)
    want = R.thermo_layers_column(p[keep], t[keep], td[keep], z[keep], layers)
    assert got['status'] == want['status'] == 0 and all(np.array_equal(got[k], want[k]) for k in TK)
    # a view that is not supplied cannot drop a level: without temperature its NaN does not count
    a = R.thermo_layers_column(p, None, td, z, layers)
    b = R.thermo_layers_column(p, t2, td, z, layers)
    c = R.thermo_layers_column(p, None, td2, None, layers[:2])
    for k in ('precipitable_water', 'mean_mixing_ratio', 'thickness'):
        assert np.array_equal(a[k], R.thermo_layers_column(p, t, td, z, layers)[k])
    assert not np.array_equal(a['precipitable_water'], b['precipitable_water'])       # (supplied, it does)
    assert np.array_equal(c['precipitable_water'], R.thermo_layers_column(p[td2 == td2], None, td[td2 == td2], None, layers[:2])['precipitable_water'])


def test_layers_not_spanned_and_ordering():
    p, z = _column(top=9000.0)                           # ends near 326 hPa
    t = 288.0 - 6.5e-3 * (z - z[0])
    td = t - 4.0
    layers = [(R.PRESSURE, 850.0, 300.0), (R.PRESSURE, NAN, 850.0), (R.HEIGHT, 0.0, 9500.0), (R.HEIGHT, 0.0, 500.0)]
    r = R.thermo_layers_column(p, t, td, z, layers)
    assert r['status'] == R.ST_NO_LAYER and np.isnan(r['thickness'][[0, 2]]).all() and np.isfinite(r['thickness'][[1, 3]]).all()
    hi = R.thermo_layers_column(p * 0.8, t, td, z, layers)                # the lowest level above 850 hPa
    assert hi['status'] == R.ST_NO_LAYER and np.isnan(hi['theta_e_max'][[0, 1, 2]]).all() and np.isfinite(hi['theta_e_max'][3])
    for lay in ((R.PRESSURE, 700.0, 700.0), (R.PRESSURE, 600.0, 700.0), (R.PRESSURE, p[0] * (1 + 1e-7), 700.0),
                (R.PRESSURE, p[0] + 1.0, NAN), (R.PRESSURE, p[-1], NAN), (R.PRESSURE, p[-1] - 1.0, NAN)):
        assert R.thermo_layers_column(p, t, td, z, [lay])['status'] == R.ST_NO_LAYER, lay
    for bc, tc in ((NAN, NAN), (600.0, 700.0), (p[0] + 1.0, 500.0), (800.0, 300.0)):
        assert R.thermo_layers_column(p, t, td, z, [(R.PRESSURE, NAN, NAN)], [bc], [tc])['status'] == R.ST_NO_LAYER, (bc, tc)
    empty = R.thermo_layers_column(p * NAN, t, td, z, layers)
    assert empty['status'] == R.ST_NO_LAYER and np.isnan(empty['precipitable_water']).all()
    p2, z2 = p.copy(), z.copy()
    p2[-1], z2[-1] = p2[-2] + 5.0, z2[-2] - 5.0                          # above the levels read: not seen ...
    assert R.thermo_layers_column(p2, t, td, z2, layers[3:])['status'] == 0
    assert R.thermo_layers_column(p2, t, td, z2, layers[1:2])['status'] == 0
    assert R.thermo_layers_column(p2, t, td, z2, [(R.PRESSURE, NAN, NAN)], [900.0], [500.0])['status'] == 0
    r = R.thermo_layers_column(p2, t, td, z2, layers)                    # ... unless a layer has not found its top ...
    assert r['status'] == (R.ST_BAD_PRESSURE | R.ST_BAD_HEIGHT) and np.isnan(r['thickness']).all()
    r = R.thermo_layers_column(p2, t, td, z2, [layers[3], (R.PRESSURE, NAN, NAN)])   # ... or is open: the whole column is read
    assert r['status'] == (R.ST_BAD_PRESSURE | R.ST_BAD_HEIGHT) and np.isnan(r['thickness']).all()
    assert R.thermo_layers_column(p2, t, td, None, layers[:2])['status'] == R.ST_BAD_PRESSURE
    z3 = z.copy()
    z3[4] = z3[3]
    assert R.thermo_layers_column(p, t, td, z3, layers[1:2])['status'] == R.ST_BAD_HEIGHT
    assert R.thermo_layers_column(p, t, td, None, layers[1:2])['status'] == 0


def test_the_gpu_test_seed_leaves_few_ambiguous_theta_e_extremes():
    """tests/test_gpu_thermo_layers.py compares the theta_e pressures only where the extreme stands out by more than 1e-9
    (relative) and asserts that this leaves out at most 1 % of the layers: checked here, on a slice of its inputs."""
    from tests.test_gpu_thermo_layers import NCOL, NLEV, SEED, inputs, restate
    arrs, pb, pt, cls = inputs(NLEV, NCOL, SEED)
    ref = restate(arrs, pb, pt, cols=range(0, NCOL, 12))
    for k, gap in (('theta_e_min_pressure', 'gap_min'), ('theta_e_max_pressure', 'gap_max')):
        has = ~np.isnan(ref[k])
        assert has.sum() > 1000 and np.mean(ref[gap][has] <= 1e-9) <= 0.01, k


# -- kernel resources -----------------------------------------------------------------------------------------------------
@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_thermo_layers is instantiated on dtype x number of layers x moisture sums x theta_e x per-column bounds: sixty-four
    kernels, none of which may use scratch or spill a vector register, and none below two waves per SIMD (DESIGN.md section 7
    has the table).  One layer of precipitable water -- the commonest call -- runs at five waves or more."""
    unit = [x for x in L.UNITS if x[1] == 'xp_thermo_layers_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    walk = {}
    for n, r in rec.items():
        m = re.search(r'k_thermo_layersI([df])Li(\d)ELb([01])ELb([01])ELb([01])E', n)
        if m:
            walk[(m.group(1),) + tuple(int(x) for x in m.groups()[1:])] = r
    assert sorted(walk) == sorted((t, n, m, th, cb) for t in 'df' for n in (1, 2, 3, 4) for m in (0, 1) for th in (0, 1) for cb in (0, 1)), sorted(rec)
    for key, r in walk.items():
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['occupancy'] >= 2, (key, r)
    for t in 'df':
        assert walk[(t, 1, 1, 0, 0)]['occupancy'] >= 5 and walk[(t, 1, 1, 0, 1)]['occupancy'] >= 5
