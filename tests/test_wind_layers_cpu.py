"""The wind over caller-chosen layers and the per-point products on it without a GPU: the C ABI declarations, the array API
and the DataArray module around a stubbed launch, the NumPy restatement (tests/wind_layers_restatement.py) against closed
forms, and the kernels' resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import kinematics_restatement as K
from tests import wind_layers_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import kinematics
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'
ENTRIES = ('xp_wind_layers', 'xp_critical_angle', 'xp_corfidi_storm_motion', 'xp_significant_tornado_effective')


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_wind_layer') == [f[0] for f in L.WindLayer._fields_]
    assert _struct_fields('xp_wind_layers_out') == [f[0] for f in L.WindLayersOut._fields_]
    assert [f[0] for f in L.WindLayersOut._fields_][:9] == list(L.WIND_LAYERS_OUT) == list(R.WIND_KEYS)
    protos = _prototypes()
    for name in ENTRIES:
        got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[name]]
        assert got == protos[name] and name in L.SYMBOLS, name
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    m = re.search(r'XP_LAYER_PRESSURE = (\d), XP_LAYER_PRESSURE_DEPTH = (\d), XP_LAYER_HEIGHT = (\d)', hdr)
    assert tuple(map(int, m.groups())) == (L.LAYER_PRESSURE, L.LAYER_PRESSURE_DEPTH, L.LAYER_HEIGHT) == (R.PRESSURE, R.PRESSURE_DEPTH, R.HEIGHT)
    assert re.search(r'void \*max_u\[4\], \*max_v\[4\], \*max_pressure\[4\];', hdr) and L.WIND_MAX_LAYERS == 4
    assert C.sizeof(L.WindLayer) == 24 and L.WindLayer.bottom.offset == 8


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


def test_wind_layers_array_api_arguments(calls):
    p = _cols()
    res = api.wind_layers(p, p, p, p, layers=[{'bottom': 850, 'top': 300}, {'depth': 150}, {'top_height': 500},
                                              ('height', 5500.0, 6000.0)])
    name, args = calls[-1]
    pv, uv, vv, zv, n, arr, out = args
    assert name == 'xp_wind_layers' and (pv.nlev, pv.ncol, pv.dtype, zv.ncol) == (9, 5, L.XP_F32, 5) and n == 4
    got = _layers(args)
    assert got[0] == (L.LAYER_PRESSURE, 850.0, 300.0) and got[1][0] == L.LAYER_PRESSURE_DEPTH and np.isnan(got[1][1])
    assert got[1][2] == 150.0 and got[2] == (L.LAYER_HEIGHT, 0.0, 500.0) and got[3] == (L.LAYER_HEIGHT, 5500.0, 6000.0)
    assert set(res) == set(L.WIND_LAYERS_OUT) | {'status'}
    assert res['mean_u'].shape == (4, 5) and res['mean_u'].dtype == np.float32 and res['status'].dtype == np.int32
    assert out.max_pressure[3] == res['max_pressure'][3].ctypes.data and out.shear_u[0] == res['shear_u'][0].ctypes.data
    assert out.status == res['status'].ctypes.data and out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    p3 = p.reshape(9, 1, 5)
    res = api.wind_layers(p3.astype(np.float64), p3, p3, layers=[{'bottom': None, 'top': 850}], want=('max_u',))
    pv, uv, vv, zv, n, arr, out = calls[-1][1]
    assert zv is None and n == 1 and pv.dtype == L.XP_F64 and set(res) == {'max_u', 'status'} and res['max_u'].shape == (1, 1, 5)
    assert out.max_u[1] is None and out.mean_u[0] is None and np.isnan(arr[0].bottom) and arr[0].top == 850.0
    for bad in ([], [{'depth': 100}] * 5, [{'top_height': 500}], [{'bottom': 900}], [{'top': 300, 'depth': 100}],
                [{'top_height': 500, 'bottom': 900}], [('sigma', 1, 2)]):
        with pytest.raises(AssertionError):
            api.wind_layers(p, p, p, layers=bad)
    with pytest.raises(AssertionError):
        api.wind_layers(p, p, p[:4], layers=[{'depth': 100}])
    with pytest.raises(AssertionError):
        api.wind_layers(p, p, p, layers=[{'depth': 100}], want=('mean',))


def test_convenience_functions_reach_the_abi_with_their_layers(calls):
    p = _cols()
    mu, mv = api.mean_pressure_weighted(p, p, p)
    args = calls[-1][1]
    assert _layers(args)[0][0] == L.LAYER_PRESSURE_DEPTH and np.isnan(_layers(args)[0][1]) and _layers(args)[0][2] == 100.0
    assert args[3] is None and mu.shape == (5,) and args[6].mean_u[0] == mu.ctypes.data and args[6].shear_u[0] is None
    api.mean_pressure_weighted(p, p, p, height=p, depth=200.0)         # no bottom: still hPa, and the heights are not read
    assert _layers(calls[-1][1]) == [(L.LAYER_PRESSURE_DEPTH, pytest.approx(np.nan, nan_ok=True), 200.0)] and calls[-1][1][3] is None
    api.mean_pressure_weighted(p, p, p, bottom=900.0, depth=300.0)
    assert _layers(calls[-1][1]) == [(L.LAYER_PRESSURE_DEPTH, 900.0, 300.0)]
    su, sv = api.bulk_shear(p, p, p, height=p, bottom=0.0, depth=6000.0)
    args = calls[-1][1]
    assert _layers(args) == [(L.LAYER_HEIGHT, 0.0, 6000.0)] and args[3] is not None
    assert args[6].shear_v[0] == sv.ctypes.data and args[6].mean_u[0] is None and args[6].max_u[0] is None
    api.bulk_shear(p, p, p, height=p, bottom=1000.0, depth=2000.0)
    assert _layers(calls[-1][1]) == [(L.LAYER_HEIGHT, 1000.0, 3000.0)]

    del calls[:]
    ang = api.critical_angle(p, p, p, p, 3.0, np.arange(5.0))
    (n1, a1), (n2, a2) = calls
    assert n1 == 'xp_wind_layers' and _layers(a1) == [(L.LAYER_HEIGHT, 0.0, 500.0)] and a1[6].max_u[0] is None
    assert a1[6].shear_u[0] and a1[6].bottom_v[0] and a1[6].mean_u[0] is None
    assert n2 == 'xp_critical_angle' and a2[:3] == (5, L.XP_F32, L.XP_MEM_HOST) and len(a2) == 10
    assert [x.ctypes.data for x in a2[3:7]] == [a1[6].shear_u[0], a1[6].shear_v[0], a1[6].bottom_u[0], a1[6].bottom_v[0]]
    assert np.all(a2[7] == 3.0) and a2[7].dtype == np.float32 and a2[7].shape == (5,) and np.array_equal(a2[8], np.arange(5.0))
    assert a2[9] is ang and ang.shape == (5,) and ang.dtype == np.float32

    del calls[:]
    res = api.corfidi_storm_motion(p, p, p)
    (n1, a1), (n2, a2) = calls
    assert _layers(a1)[0] == (L.LAYER_PRESSURE, 850.0, 300.0) and _layers(a1)[1][0] == L.LAYER_PRESSURE
    assert np.isnan(_layers(a1)[1][1]) and _layers(a1)[1][2] == 850.0 and a1[3] is None and a1[4] == 2
    assert n2 == 'xp_corfidi_storm_motion' and len(a2) == 11
    assert [x.ctypes.data for x in a2[3:7]] == [a1[6].mean_u[0], a1[6].mean_v[0], a1[6].max_u[1], a1[6].max_v[1]]
    assert a1[6].max_u[0] is not None and a1[6].shear_u[0] is None       # (one output array per key wanted, a row per layer)
    assert set(res) == {'upwind_u', 'upwind_v', 'downwind_u', 'downwind_v', 'status'} and a2[7] is res['upwind_u'] and a2[10] is res['downwind_v']
    del calls[:]
    api.corfidi_storm_motion(p, p, p, llj_u=2.0, llj_v=np.ones(5))
    (n1, a1), (n2, a2) = calls
    assert a1[4] == 1 and a1[6].max_u[0] is None and np.all(a2[5] == 2.0) and np.all(a2[6] == 1.0) and a2[5].dtype == np.float32
    with pytest.raises(AssertionError):
        api.corfidi_storm_motion(p, p, p, llj_u=2.0)
    with pytest.raises(AssertionError):
        api.corfidi_storm_motion(p, p, p, llj_v=np.ones(5))

    x = np.ones((2, 3))
    out = api.significant_tornado_effective(x, x, x, x, x)
    name, a = calls[-1]
    assert name == 'xp_significant_tornado_effective' and a[:3] == (6, L.XP_F64, L.XP_MEM_HOST) and a[8] is None and a[9] is out
    out = api.significant_tornado_effective(x, x, x, x, x, base_height=2 * x)
    assert np.all(calls[-1][1][8] == 2.0) and calls[-1][1][9] is out and out.shape == (2, 3)
    with pytest.raises(AssertionError):
        api.significant_tornado_effective(x, x, x, x, x[:1])


def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def _horiz(val, name):
    return DataArray(np.full((2, 3), val), dims=('lat', 'lon'), coords={'lat': [10., 20.], 'lon': [1., 2., 3.]}, name=name)


def test_mirror_wraps_the_array_api(calls):
    lev = np.arange(1., 10.)
    p, u, v, z = _grid(1000. - 50 * lev, 'p'), _grid(lev, 'u'), _grid(lev, 'v'), _grid(500. * lev, 'z')
    ds = kinematics.wind_layers(p, u, v, z, layers=[{'top_height': 500}, {'bottom': 850, 'top': 300}])
    name, args = calls[-1]
    assert name == 'xp_wind_layers' and (args[0].nlev, args[0].ncol, args[4]) == (9, 6, 2)
    names = list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys())
    assert names == list(kinematics._WIND_LAYERS.values()) + ['status']
    for k in kinematics._WIND_LAYERS.values():
        assert ds[k].dims == ('wind_layer', 'lat', 'lon') and ds[k].shape == (2, 2, 3) and ds[k].name == k
        assert ds[k].attrs['units'] == ('hPa' if k == 'max_wind_pressure' else 'm s$^{-1}$')
    assert list(ds['bulk_shear_u'].coords['wind_layer']) == [0, 1] and ds['status'].dims == ('lat', 'lon')
    ds = kinematics.mean_pressure_weighted(p, u, v, depth=150.0)
    assert _layers(calls[-1][1])[0][2] == 150.0 and ds['layer_mean_wind_u'].dims == ('lat', 'lon')
    ds = kinematics.bulk_shear(p, u, v, z, bottom=0.0, depth=6000.0)
    assert _layers(calls[-1][1]) == [(L.LAYER_HEIGHT, 0.0, 6000.0)] and ds['bulk_shear_v'].attrs['units'] == 'm s$^{-1}$'
    ang = kinematics.critical_angle(p, u, v, z, _horiz(3.0, 'cu'), 1.0)
    name, args = calls[-1]
    assert name == 'xp_critical_angle' and np.all(args[7] == 3.0) and np.all(args[8] == 1.0)
    assert ang.dims == ('lat', 'lon') and ang.name == 'critical_angle' and ang.attrs['units'] == 'degrees'
    ds = kinematics.corfidi_storm_motion(p, u, v)
    assert calls[-1][0] == 'xp_corfidi_storm_motion' and calls[-2][1][4] == 2
    assert list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys()) == list(kinematics._CORFIDI.values())
    ds = kinematics.corfidi_storm_motion(p, u, v, llj_u=_horiz(4.0, 'ju'), llj_v=_horiz(-1.0, 'jv'))
    assert calls[-2][1][4] == 1 and np.all(calls[-1][1][5] == 4.0) and ds['corfidi_downwind_u'].dims == ('lat', 'lon')
    h = [_horiz(x, 'x') for x in (2000., -20., 900., 200., 25.)]
    stp = kinematics.significant_tornado_effective(*h, base_height=_horiz(0.0, 'b'))
    assert calls[-1][0] == 'xp_significant_tornado_effective' and calls[-1][1][0] == 6 and np.all(calls[-1][1][8] == 0.0)
    assert stp.dims == ('lat', 'lon') and stp.name == 'significant_tornado_effective'
    for key in list(kinematics._WIND_LAYERS.values()) + list(kinematics._CORFIDI.values()) + ['critical_angle', 'significant_tornado_effective']:
        assert 'long_name' in kinematics._ATTRS[key]


# -- the restatement against closed forms ---------------------------------------------------------------------------------
def _column(nlev=24, top=13000.0, z0=150.0, p0=1005.0):
    z = z0 + np.linspace(0.0, top, nlev) + np.r_[0.0, np.sin(np.arange(1, nlev)) * 60.0]
    return p0 * np.exp(-(z - z0) / 8000.0), z


def test_log_pressure_profile_gives_the_shear_in_closed_form():
    p, z = _column()
    a, b = 3.0, -7.5
    u, v = a + b * np.log(p), 2.0 - 1.5 * np.log(p)
    layers = [(R.PRESSURE, 843.21, 311.7), (R.PRESSURE_DEPTH, np.nan, 123.4), (R.PRESSURE_DEPTH, 901.5, 300.0), (R.HEIGHT, 250.0, 3333.0)]
    r = R.wind_layers_column(p, u, v, z, layers)
    assert r['status'] == 0
    pbt = [(843.21, 311.7), (p[0], p[0] - 123.4), (901.5, 601.5),
           (float(np.interp(z[0] + 250.0, z, p)), float(np.interp(z[0] + 3333.0, z, p)))]
    for j, (pb, pt) in enumerate(pbt):
        assert abs(r['shear_u'][j] - b * np.log(pt / pb)) < 1e-12 and abs(r['shear_v'][j] + 1.5 * np.log(pt / pb)) < 1e-12
        assert abs(r['bottom_u'][j] - (a + b * np.log(pb))) < 1e-12
        # |u| and |v| shrink with height here: the strongest point is the bottom
        assert r['max_pressure'][j] == pb and abs(r['max_u'][j] - (a + b * np.log(pb))) < 1e-12


def test_constant_wind_is_its_own_mean_and_its_first_point_the_strongest():
    p, z = _column()
    u, v = np.full_like(p, 7.25), np.full_like(p, -3.5)
    layers = [(R.PRESSURE, 850.0, 300.0), (R.PRESSURE, np.nan, 850.0), (R.HEIGHT, 0.0, 6000.0), (R.HEIGHT, 5500.0, 6000.0)]
    r = R.wind_layers_column(p, u, v, z, layers)
    assert r['status'] == 0
    for j in range(4):
        assert abs(r['mean_u'][j] - 7.25) < 1e-12 and abs(r['mean_v'][j] + 3.5) < 1e-12
        assert r['shear_u'][j] == 0.0 and r['shear_v'][j] == 0.0 and r['gap'][j] == 0.0
        assert (r['max_u'][j], r['max_v'][j]) == (7.25, -3.5)
    assert r['max_pressure'][0] == 850.0 and r['max_pressure'][1] == p[0] and r['max_pressure'][2] == p[0]
    assert r['max_pressure'][3] == float(np.interp(z[0] + 5500.0, z, p))


def test_linear_in_pressure_wind_has_the_closed_form_mean():
    p = np.linspace(1000.0, 200.0, 401)                  # (trapz of a quadratic: exact only in the limit, so compare loosely)
    u = 2.0 + 0.01 * p
    r = R.wind_layers_column(p, u, np.zeros_like(p), None, [(R.PRESSURE, 900.0, 400.0)])
    pb, pt = 900.0, 400.0
    want = (2.0 * 0.5 * (pt ** 2 - pb ** 2) + 0.01 * (pt ** 3 - pb ** 3) / 3.0) / (0.5 * (pt ** 2 - pb ** 2))
    assert abs(r['mean_u'][0] - want) < 1e-3 and r['status'] == 0


def test_bounds_on_levels_add_no_points_and_height_layers_are_bunkers_layers():
    p, z = _column()
    u, v = 5.0 + 2e-3 * z, np.sin(z / 2000.0)
    P = R.points_between(p, u, v, p[3], p[9])[0]
    assert list(P) == list(p[3:10])
    P = R.points_between(p, u, v, p[3] * (1 + 1e-6), p[9] * (1 - 1e-6))[0]         # close to the levels: still no new points
    assert list(P) == list(p[3:10])
    P = R.points_between(p, u, v, p[3] * (1 + 2e-5), p[9] * (1 - 2e-5))[0]         # not close: the bounds are points, the
    assert len(P) == 9 and P[0] == p[3] * (1 + 2e-5) and P[-1] == p[9] * (1 - 2e-5)   # levels stay inside
    P = R.points_between(p, u, v, p[3] * (1 - 2e-5), p[9] * (1 + 2e-5))[0]         # not close, the levels outside
    assert len(P) == 7 and P[1] == p[4] and P[-2] == p[8]
    r = R.wind_layers_column(p, u, v, z, [(R.PRESSURE, p[3], p[9])])
    assert (r['bottom_u'][0], r['shear_u'][0]) == (u[3], u[9] - u[3])
    for zb, d in ((0.0, 500.0), (5500.0, 500.0), (0.0, 6000.0), (z[2] - z[0], z[7] - z[2])):
        want = K.layer_points(p, u, v, z, z[0] + zb, d)
        pb, pt = float(np.interp(z[0] + zb, z, p)), float(np.interp(z[0] + zb + d, z, p))
        got = R.points_between(p, u, v, pb, pt)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        r = R.wind_layers_column(p, u, v, z, [(R.HEIGHT, zb, zb + d)])
        m = K.layer_mean(p, u, v, z, z[0] + zb, d)       # Bunkers' plain mean and the pressure-weighted one: both inside
        assert min(want[1]) <= r['mean_u'][0] <= max(want[1]) and min(want[1]) <= m[0] <= max(want[1])
        assert r['bottom_u'][0] == want[1][0] and r['shear_v'][0] == want[2][-1] - want[2][0]


def test_missing_levels_are_dropped():
    p, z = _column()
    u, v = 5.0 + 2e-3 * z + np.cos(z / 900.0), np.sin(z / 2000.0)
    layers = [(R.PRESSURE, 850.0, 300.0), (R.PRESSURE_DEPTH, np.nan, 100.0), (R.HEIGHT, 0.0, 6000.0)]
    u2, z2, p2 = u.copy(), z.copy(), p.copy()
    u2[3], z2[9], p2[5] = np.nan, np.nan, np.nan
    keep = np.ones(p.size, bool)
    keep[[3, 5, 9]] = False
    got, want = R.wind_layers_column(p2, u2, v, z2, layers), R.wind_layers_column(p[keep], u[keep], v[keep], z[keep], layers)
    assert got['status'] == want['status'] == 0 and all(np.array_equal(got[k], want[k]) for k in R.WIND_KEYS)
    got = R.wind_layers_column(p, u, v, None, layers[:2])                # without height, a NaN height cannot drop a level
    assert all(np.array_equal(got[k], R.wind_layers_column(p, u, v, z, layers[:2])[k]) for k in R.WIND_KEYS)


def test_layers_not_spanned_and_ordering():
    p, z = _column(top=9000.0)                           # ends near 326 hPa
    u, v = 5.0 + 2e-3 * z, np.sin(z / 2000.0)
    layers = [(R.PRESSURE, 850.0, 300.0), (R.PRESSURE, np.nan, 850.0), (R.HEIGHT, 0.0, 9500.0), (R.HEIGHT, 0.0, 500.0)]
    r = R.wind_layers_column(p, u, v, z, layers)
    assert r['status'] == R.ST_NO_LAYER and np.isnan(r['mean_u'][[0, 2]]).all() and np.isfinite(r['mean_u'][[1, 3]]).all()
    hi = R.wind_layers_column(p * 0.8, u, v, z, layers)                  # the lowest level above 850 hPa
    assert hi['status'] == R.ST_NO_LAYER and np.isnan(hi['max_u'][[0, 1, 2]]).all() and np.isfinite(hi['max_u'][3])
    for lay in ((R.PRESSURE, 700.0, 700.0), (R.PRESSURE, 600.0, 700.0), (R.PRESSURE, p[0] * (1 + 1e-7), 700.0)):
        assert R.wind_layers_column(p, u, v, z, [lay])['status'] == R.ST_NO_LAYER
    empty = R.wind_layers_column(p * np.nan, u, v, z, layers)
    assert empty['status'] == R.ST_NO_LAYER and np.isnan(empty['shear_u']).all()
    p2, z2 = p.copy(), z.copy()
    p2[-1], z2[-1] = p2[-2] + 5.0, z2[-2] - 5.0                          # above the levels read: not seen ...
    assert R.wind_layers_column(p2, u, v, z2, layers[3:])['status'] == 0
    assert R.wind_layers_column(p2, u, v, z2, layers[1:2])['status'] == 0
    r = R.wind_layers_column(p2, u, v, z2, layers)                       # ... unless a layer has not found its top
    assert r['status'] == (R.ST_BAD_PRESSURE | R.ST_BAD_HEIGHT) and np.isnan(r['mean_u']).all()
    assert R.wind_layers_column(p2, u, v, None, layers[:2])['status'] == R.ST_BAD_PRESSURE


def test_critical_angle_closed_forms():
    def ang(a, b, sfc=(1.0, -2.0)):
        return float(R.critical_angle(a[0], a[1], sfc[0], sfc[1], b[0] + sfc[0], b[1] + sfc[1]))
    assert ang((3.0, 0.0), (0.0, 5.0)) == 90.0 and ang((0.0, -2.0), (4.0, 0.0)) == 90.0
    assert ang((3.0, 4.0), (6.0, 8.0)) == 0.0 and ang((3.0, 4.0), (-1.5, -2.0)) == 180.0
    assert abs(ang((1.0, 0.0), (1.0, 1.0)) - 45.0) < 1e-12 and abs(ang((1.0, 0.0), (-1.0, -1.0)) - 135.0) < 1e-12
    assert np.isnan(ang((0.0, 0.0), (1.0, 1.0))) and np.isnan(ang((1.0, 1.0), (0.0, 0.0)))
    assert np.isnan(ang((np.nan, 0.0), (1.0, 1.0)))
    rng = np.random.default_rng(0)
    x = rng.normal(0, 10, (6, 2000))
    a, b = R.critical_angle(*x), R.critical_angle_arccos(*x)
    mid = (a > 1.0) & (a < 179.0)
    assert mid.sum() > 1900 and np.max(np.abs(a[mid] - b[mid])) < 1e-9
    # where MetPy's form fails: parallel vectors whose cosine rounds above 1
    au, av = np.full(2000, 0.1) * rng.uniform(1, 9, 2000), np.full(2000, 0.3) * 1.0
    s = rng.uniform(1, 9, 2000)
    with np.errstate(invalid='ignore'):
        cos_form = R.critical_angle_arccos(au, av, 0.0, 0.0, au * s, av * s)
    assert np.all(R.critical_angle(au, av, 0.0, 0.0, au * s, av * s) < 1e-6) and (np.isnan(cos_form).any() or np.nanmax(cos_form) < 1e-5)


def test_corfidi_and_effective_stp_closed_forms():
    uu, uv, du, dv = R.corfidi_storm_motion(10.0, 4.0, 3.0, -6.0)
    assert (uu, uv, du, dv) == (7.0, 10.0, 17.0, 14.0)
    stp = R.significant_tornado_effective
    full = stp(1500.0, -50.0, 1000.0, 150.0, 20.0)
    assert full == 1.0 and stp(1500.0, 0.0, 500.0, 150.0, 20.0) == 1.0                    # clipped: LCL below 1000, CIN above -50
    assert stp(1500.0, -200.0, 1000.0, 150.0, 20.0) == 0.0 and stp(1500.0, -300.0, 1000.0, 150.0, 20.0) == 0.0
    assert stp(1500.0, -125.0, 1000.0, 150.0, 20.0) == 0.5 and stp(1500.0, -50.0, 1500.0, 150.0, 20.0) == 0.5
    assert stp(1500.0, -50.0, 2000.0, 150.0, 20.0) == 0.0 and stp(1500.0, -50.0, 2500.0, 150.0, 20.0) == 0.0
    assert stp(1500.0, -50.0, 1000.0, 150.0, 12.5) == 0.625 and stp(1500.0, -50.0, 1000.0, 150.0, 12.499) == 0.0
    assert stp(1500.0, -50.0, 1000.0, 150.0, 30.0) == 1.5 and stp(1500.0, -50.0, 1000.0, 150.0, 45.0) == 1.5
    assert stp(3000.0, -50.0, 1000.0, -300.0, 20.0) == -4.0
    for i in range(5):
        x = [1500.0, -50.0, 1000.0, 150.0, 20.0]
        x[i] = np.nan
        assert np.isnan(stp(*x)) and stp(*x, base_height=10.0) == 0.0
    assert stp(1500.0, -50.0, 1000.0, 150.0, 20.0, base_height=0.0) == 1.0 and stp(1500.0, -50.0, 1000.0, 150.0, 20.0, base_height=250.0) == 0.0
    assert stp(1500.0, -50.0, 1000.0, 150.0, 20.0, base_height=np.nan) == 1.0


def test_the_gpu_test_seed_leaves_few_ambiguous_strongest_winds():
    """tests/test_gpu_wind_layers.py compares max_pressure only where the strongest point stands out by more than 1e-9
    (relative) and asserts that this leaves out at most 1 % of the layers: checked here, on a slice of its inputs."""
    from tests.test_gpu_wind_layers import LAYERS, SEED, inputs
    p, u, v, z = inputs(48, 6000, SEED)
    ref = R.wind_layers_grid(p, u, v, z, LAYERS, cols=range(0, 6000, 12))
    has = ~np.isnan(ref['max_pressure'])
    assert has.sum() > 1000 and np.mean(ref['gap'][has] <= 1e-9) <= 0.01


# -- kernel resources -----------------------------------------------------------------------------------------------------
@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_wind_layers is instantiated on dtype x number of layers x strongest wind wanted: sixteen kernels, none of which may
    use scratch or spill a vector register.  Four layers do not fit four waves per SIMD (DESIGN.md section 7 has the table):
    the operating point is four waves up to three layers without the strongest wind -- mean_pressure_weighted, bulk_shear,
    critical_angle, the three Bunkers layers -- and up to two with it (corfidi_storm_motion), and never fewer than two."""
    unit = [x for x in L.UNITS if x[1] == 'xp_wind_layers_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    walk = {}
    for n, r in rec.items():
        m = re.search(r'k_wind_layersI([df])Li(\d)ELb([01])E', n)
        if m:
            walk[(m.group(1), int(m.group(2)), int(m.group(3)))] = r
    assert sorted(walk) == sorted((t, n, m) for t in 'df' for n in (1, 2, 3, 4) for m in (0, 1)), sorted(rec)
    # the three per-point products are instantiations of k_per_point, which lives in the main unit
    main = resources(tmp_path, 'xparcel.hip')
    point = [n for n in main if re.search(r'k_per_pointI[df]NS_\d+(CriticalAngleOp|CorfidiOp|StpEffectiveOp)E', n)]
    assert len(point) == 6, sorted(main)
    for key, r in list(walk.items()) + [(n, main[n]) for n in point]:
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['occupancy'] >= 2, (key, r)
    for t in 'df':
        for n, m in ((1, 0), (2, 0), (3, 0), (1, 1), (2, 1)):
            assert walk[(t, n, m)]['vgprs'] <= 128 and walk[(t, n, m)]['occupancy'] >= 4, (t, n, m, walk[(t, n, m)])
