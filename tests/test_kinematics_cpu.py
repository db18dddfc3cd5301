"""Storm motion, helicity and the composites without a GPU: the NumPy restatement (tests/kinematics_restatement.py) on
analytic and hand-built columns, the C ABI declarations, the xarray mirror (xarray_parcel_amd/kinematics.py) around a
stubbed launch, and the kernels' resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import kinematics_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import kinematics
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'


# -- analytic columns ---------------------------------------------------------------------------------------------------
def circular_hodograph(n=12, radius=10.0, turn=np.pi / 2, centre=(3.0, -2.0), dh=250.0, clockwise=True):
    """Heights 0, dh, ... n dh; the wind turns through `turn` in n equal steps on a circle of `radius` about `centre`."""
    h = dh * np.arange(n + 1)
    th = 0.3 + (-1.0 if clockwise else 1.0) * turn * np.arange(n + 1) / n
    return h, centre[0] + radius * np.cos(th), centre[1] + radius * np.sin(th)


@pytest.mark.parametrize('clockwise', [True, False])
def test_circular_hodograph(clockwise):
    n, rad, turn = 12, 10.0, np.pi / 2
    h, u, v = circular_hodograph(n, rad, turn, clockwise=clockwise)
    r = R.srh_column(h, u, v, [n * 250.0], storm_u=3.0, storm_v=-2.0)
    want = n * rad ** 2 * np.sin(turn / n)
    assert r['status'] == 0
    if clockwise:
        assert abs(r['positive'][0] - want) < 1e-9 * want and r['negative'][0] == 0.0
        assert abs(r['total'][0] - want) < 1e-9 * want
    else:
        assert abs(r['negative'][0] + want) < 1e-9 * want and r['positive'][0] == 0.0
        assert abs(r['total'][0] + want) < 1e-9 * want


@pytest.mark.parametrize('cu,cv', [(0.0, 0.0), (4.0, 3.0), (-2.0, -6.5)])
def test_straight_hodograph(cu, cv):
    a = 4e-3
    h = np.array([0., 150., 400., 800., 1300., 2100., 3000., 4200.])
    r = R.srh_column(h, a * h, np.zeros_like(h), [3000.0], storm_u=cu, storm_v=cv)
    want = -cv * (a * 3000.0)
    assert abs(r['total'][0] - want) <= 1e-12 * (1 + abs(want))
    assert r['positive'][0] >= 0 and r['negative'][0] <= 0


def bunkers_column(nlev=30, top=12000.0, u=lambda z: 2.0 + 3e-3 * z, v=lambda z: np.full_like(z, 1.5), z0=120.0):
    z = z0 + np.linspace(0.0, top, nlev) + np.r_[0.0, np.sin(np.arange(1, nlev)) * 40.0]
    p = 1010.0 * np.exp(-(z - z0) / 8200.0)
    return p, u(z), v(z), z


def test_unidirectional_westerly_shear():
    r = R.bunkers_column(*bunkers_column())
    assert r['status'] == 0
    assert abs(r['right_v'] - (r['mean_v'] - 7.5)) < 1e-12 and abs(r['left_v'] - (r['mean_v'] + 7.5)) < 1e-12
    assert abs(r['right_u'] - r['mean_u']) < 1e-12 and abs(r['left_u'] - r['mean_u']) < 1e-12
    assert abs(r['mean_v'] - 1.5) < 1e-12 and 2.0 + 3e-3 * 120 < r['mean_u'] < 2.0 + 3e-3 * 6120


def test_constant_wind_is_its_own_mean_and_has_no_movers():
    r = R.bunkers_column(*bunkers_column(u=lambda z: np.full_like(z, 7.25), v=lambda z: np.full_like(z, -3.5)))
    assert r['status'] == 0
    assert abs(r['mean_u'] - 7.25) < 1e-12 and abs(r['mean_v'] + 3.5) < 1e-12
    assert all(np.isnan(r[k]) for k in ('right_u', 'right_v', 'left_u', 'left_v'))


# -- bounds: isclose (pressure, Bunkers) and exact equality (height, SRH) --------------------------------------------------
def _column_with_level(zlev):
    """A Bunkers column from z0 = 0 with an extra level at height zlev."""
    z = np.sort(np.r_[np.arange(0.0, 9000.0, 700.0), zlev])
    p = 1000.0 * np.exp(-z / 8000.0)
    return p, 5.0 + 2e-3 * z, np.sin(z / 2000.0), z


@pytest.mark.parametrize('zb,d', [(0.0, 500.0), (5500.0, 500.0), (0.0, 6000.0)])
def test_bunkers_bounds_on_levels_are_not_added(zb, d):
    for bound in (zb, zb + d):
        if bound == 0.0:
            continue
        p, u, v, z = _column_with_level(bound)
        P = R.layer_points(p, u, v, z, zb, d)[0]
        k = list(z).index(bound)
        assert p[k] in P and len(P) == len(set(P))
        # a level 0.02 m off the bound: its pressure is within np.isclose of the bound's, so the bound is not added
        for off in (0.02, -0.02):
            p, u, v, z = _column_with_level(bound + off)
            pb = float(np.interp(bound, z, p))
            k = list(z).index(bound + off)
            P = R.layer_points(p, u, v, z, zb, d)[0]
            assert R.close(p[k], pb) and p[k] in P and pb not in P
        # 5 m off: not close; the bound is a point of its own, the level is inside the layer only if between the bounds
        for off in (5.0, -5.0):
            p, u, v, z = _column_with_level(bound + off)
            pb = float(np.interp(bound, z, p))
            P = R.layer_points(p, u, v, z, zb, d)[0]
            k = list(z).index(bound + off)
            assert pb in P and (p[k] in P) == (zb < z[k] < zb + d)


def test_srh_top_uses_exact_equality_not_isclose():
    h = np.array([0., 300., 700., 1000.000001, 1500., 2500.])
    u, v = 3.0 + 0.01 * h, np.cos(h / 400.0)
    H = R.srh_points(h, u, v, 0.0, 1000.0)[0]
    assert list(H) == [0., 300., 700., 1000., 1000.000001]         # the close level and the added top both count
    H = R.srh_points(np.array([0., 300., 700., 1000., 1500.]), u[:5], v[:5], 0.0, 1000.0)[0]
    assert list(H) == [0., 300., 700., 1000.]
    H = R.srh_points(np.array([0., 300., 700., 999.9, 1000.1, 1500.]), u, v, 0.0, 1000.0)[0]
    assert list(H) == [0., 300., 700., 999.9, 1000.]                # 1000.1 is not close to 1000


def test_srh_bottom_above_the_surface():
    h = np.array([0., 200., 600., 1100., 1800., 3000.])
    u, v = 2.0 + 0.01 * h, 0.004 * h
    H = R.srh_points(h, u, v, 500.0, 1000.0)[0]
    assert list(H) == [500., 600., 1100., 1500.]
    H = R.srh_points(h, u, v, 600.0 - 1e-6, 500.0)[0]
    assert list(H) == [600. - 1e-6, 600., (600. - 1e-6) + 500., 1100.]   # close to the bounds: inside, and the bounds added


def test_srh_surface_point_and_relative_heights():
    h = np.array([110., 300., 700., 1200., 2000.])
    u, v = np.array([2., 4., 7., 9., 12.]), np.array([0., 2., 3., 3., 2.])
    rel = R.srh_column(h, u, v, [1000.0])
    assert rel['total'][0] == R.srh_column(h - 110.0, u, v, [1000.0])['total'][0]
    sfc = R.srh_column(h, u, v, [1000.0], surface_u=1.0, surface_v=-1.0)
    want = R.srh_column(np.r_[0.0, h], np.r_[1.0, u], np.r_[-1.0, v], [1000.0])
    assert sfc['total'][0] == want['total'][0] and sfc['status'] == 0
    miss = R.srh_column(h, u, v, [1000.0], surface_u=np.nan, surface_v=-1.0)   # dropped: the bottom is below the data
    assert miss['status'] == R.ST_NO_LAYER and np.isnan(miss['total'][0])


# -- missing levels, spans, ordering --------------------------------------------------------------------------------------
def test_missing_levels_are_dropped():
    p, u, v, z = bunkers_column(u=lambda z: 2.0 + 3e-3 * z, v=lambda z: 1e-3 * z - 2.0)
    u2, z2 = u.copy(), z.copy()
    u2[3], z2[9] = np.nan, np.nan
    keep = np.ones(p.size, bool)
    keep[[3, 9]] = False
    got, want = R.bunkers_column(p, u2, v, z2), R.bunkers_column(p[keep], u[keep], v[keep], z[keep])
    assert all(got[k] == want[k] for k in R.BUNKERS_KEYS + ('status',))
    got = R.srh_column(z2, u2, v, [1000.0, 3000.0])
    want = R.srh_column(z[keep], u[keep], v[keep], [1000.0, 3000.0])
    assert np.array_equal(got['total'], want['total'])


def test_columns_not_spanned():
    p, u, v, z = bunkers_column(top=5999.0, nlev=12)
    r = R.bunkers_column(p, u, v, z)
    assert r['status'] == R.ST_NO_LAYER and all(np.isnan(r[k]) for k in R.BUNKERS_KEYS)
    r = R.bunkers_column(*(a[:1] for a in (p, u, v, z)))
    assert r['status'] == R.ST_NO_LAYER
    p, u, v, z = bunkers_column(top=6000.0, nlev=12)
    z[-1] = z[0] + 6000.0
    assert R.bunkers_column(p, u, v, z)['status'] == 0               # the top on the last level: spanned
    h = np.array([0., 400., 900., 2500.])
    r = R.srh_column(h, h * 0.01, h * 0.002, [1000.0, 3000.0, 2500.0])
    assert r['status'] == R.ST_NO_LAYER
    assert np.isfinite(r['total'][0]) and np.isnan(r['total'][1]) and np.isfinite(r['total'][2])


def test_ordering_violations():
    p, u, v, z = bunkers_column()
    z2 = z.copy()
    z2[4] = z2[3]
    assert R.bunkers_column(p, u, v, z2)['status'] == R.ST_BAD_HEIGHT
    p2 = p.copy()
    p2[5] = p2[4] + 1.0
    r = R.bunkers_column(p2, u, v, z)
    assert r['status'] == R.ST_BAD_PRESSURE and np.isnan(r['mean_u'])
    p2, z2 = p.copy(), z.copy()
    p2[-1], z2[-1] = p2[-2] + 5.0, z2[-2] - 5.0                      # above the levels read: not seen
    assert R.bunkers_column(p2, u, v, z2)['status'] == 0
    r = R.srh_column(z2, u, v, [1000.0])
    assert r['status'] == 0
    r = R.srh_column(z2, u, v, [12500.0])                           # every level read
    assert r['status'] == R.ST_BAD_HEIGHT and np.isnan(r['total'][0])


def test_nan_storm_motion_gives_nan():
    h, u, v = circular_hodograph()
    r = R.srh_column(h, u, v, [1000.0], storm_u=np.nan)
    assert r['status'] == 0 and np.isnan(r['total'][0]) and np.isnan(r['positive'][0])


def test_composites():
    stp = R.significant_tornado([3000., 3000., 3000., np.nan], [500., 1500., 2500., 800.], [150., 150., 150., 150.],
                                [40., 20., 12.4, 20.])
    assert stp[0] == (3000. * 1.0 * 150. * 1.5) / 225000. and stp[1] == (3000. * 0.5 * 150. * 1.0) / 225000.
    assert stp[2] == 0.0 and np.isnan(stp[3])
    scp = R.supercell_composite([2000., 2000., 2000.], [100., 100., np.nan], [9.99, 25., 15.])
    assert scp[0] == 0.0 and scp[1] == 2.0 * 2.0 * 1.0 and np.isnan(scp[2])


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_storm_motion_out') == [f[0] for f in L.StormMotionOut._fields_]
    assert _struct_fields('xp_srh_out') == [f[0] for f in L.SrhOut._fields_]
    protos = _prototypes()
    for name in ('xp_bunkers_storm_motion', 'xp_storm_relative_helicity', 'xp_significant_tornado', 'xp_supercell_composite'):
        got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[name]]
        assert got == protos[name] and name in L.SYMBOLS, name
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'XP_ST_BAD_HEIGHT\s*=\s*32\b', hdr) and L.ST_BAD_HEIGHT == 32 == R.ST_BAD_HEIGHT
    assert re.search(r'void \*positive\[4\], \*negative\[4\], \*total\[4\];', hdr) and L.SRH_MAX_DEPTHS == 4


# -- the array API and the mirror around a stubbed launch -----------------------------------------------------------------
def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def _horiz(val, name):
    return DataArray(np.full((2, 3), val), dims=('lat', 'lon'), coords={'lat': [10., 20.], 'lon': [1., 2., 3.]}, name=name)


def test_srh_array_api_arguments(monkeypatch):
    seen = {}

    def run(self, name, *args):
        seen['name'], seen['args'] = name, args
    monkeypatch.setattr(api._Call, 'run', run)
    z = np.linspace(0., 4000., 9, dtype=np.float32)[:, None] * np.ones((1, 5), np.float32)
    res = api.storm_relative_helicity(z, z, z, [1000, 3000], bottom=10, storm_u=2.5)
    zv, uv, vv, su, sv, cu, cv, bottom, nd, depths, out = seen['args']
    assert seen['name'] == 'xp_storm_relative_helicity' and (zv.nlev, zv.ncol, zv.dtype) == (9, 5, L.XP_F32)
    assert su is None and sv is None and np.all(cu == 2.5) and np.all(cv == 0.0) and cu.dtype == np.float32
    assert bottom == 10.0 and nd == 2 and list(depths) == [1000.0, 3000.0]
    assert res['total'].shape == (2, 5) and res['status'].shape == (5,) and res['status'].dtype == np.int32
    assert out.total[0] == res['total'][0].ctypes.data and out.total[1] == res['total'][1].ctypes.data
    assert out.total[2] is None and out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    res = api.storm_relative_helicity(z, z, z, 1000.0, surface_u=np.ones(5), surface_v=0.0)
    assert res['positive'].shape == (5,) and seen['args'][8] == 1 and np.all(seen['args'][3] == 1.0)
    with pytest.raises(AssertionError):
        api.storm_relative_helicity(z, z, z, [1, 2, 3, 4, 5])
    with pytest.raises(AssertionError):
        api.storm_relative_helicity(z, z, z, 1000.0, surface_u=1.0)


def test_mirror_wraps_the_array_api(monkeypatch):
    calls = []

    def run(self, name, *args):
        calls.append((name, args))
    monkeypatch.setattr(api._Call, 'run', run)
    lev = np.arange(1., 10.)
    ds = kinematics.bunkers_storm_motion(_grid(1000. - 50 * lev, 'pressure'), _grid(lev, 'u'), _grid(lev, 'v'),
                                         _grid(500. * lev, 'height'))
    name, args = calls[-1]
    assert name == 'xp_bunkers_storm_motion' and (args[0].nlev, args[0].ncol) == (9, 6)
    assert list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys()) == list(kinematics._BUNKERS.values())
    for k in kinematics._BUNKERS.values():
        assert ds[k].dims == ('lat', 'lon') and ds[k].attrs['units'] == 'm s$^{-1}$' and ds[k].name == k
    ds = kinematics.storm_relative_helicity(_grid(500. * lev, 'height'), _grid(lev, 'u'), _grid(lev, 'v'), 1000,
                                            storm_u=_horiz(3.0, 'su'), storm_v=1.0)
    name, args = calls[-1]
    assert name == 'xp_storm_relative_helicity' and np.all(args[5] == 3.0) and np.all(args[6] == 1.0)
    assert ds['total_srh'].dims == ('lat', 'lon') and ds['total_srh'].attrs['units'] == 'm$^{2}$ s$^{-2}$'
    ds = kinematics.storm_relative_helicity(_grid(500. * lev, 'height'), _grid(lev, 'u'), _grid(lev, 'v'), [1000, 3000])
    assert ds['positive_srh'].dims == ('srh_depth', 'lat', 'lon') and list(ds['positive_srh'].coords['srh_depth']) == [1000., 3000.]
    stp = kinematics.significant_tornado(_horiz(2000., 'c'), _horiz(900., 'l'), _horiz(200., 's'), _horiz(25., 'sh'))
    assert calls[-1][0] == 'xp_significant_tornado' and calls[-1][1][0] == 6
    assert stp.dims == ('lat', 'lon') and stp.name == 'significant_tornado'
    scp = kinematics.supercell_composite(_horiz(2000., 'c'), _horiz(200., 's'), _horiz(25., 'sh'))
    assert calls[-1][0] == 'xp_supercell_composite' and scp.name == 'supercell_composite'


def test_parcel_functions_gains_nothing():
    from xarray_parcel_amd import parcel_functions as pf
    for name in ('bunkers_storm_motion', 'storm_relative_helicity', 'significant_tornado', 'supercell_composite'):
        assert not hasattr(pf, name)


# -- kernel resources -----------------------------------------------------------------------------------------------------
@needs_hipcc
def test_kernels_keep_four_waves_per_simd_without_spills(tmp_path):
    rec = resources(tmp_path, 'xparcel.hip')
    # the two composites are instantiations of the one per-point kernel (csrc/xp_per_point.hpp) on their operations
    kernels = [n for n in rec if re.search(r'k_(bunkers_storm_motion|storm_relative_helicity)I[df]E|'
                                           r'k_per_pointI[df]NS_\d+(StpOp|ScpOp)E', n)]
    assert len(kernels) == 8, sorted(rec)
    for k in ('k_bunkers_storm_motion', 'k_storm_relative_helicity', 'StpOp', 'ScpOp'):
        assert sum(k in n for n in kernels) == 2, (k, kernels)
    for n in kernels:
        assert rec[n]['in_asm'] and not rec[n]['scratch_insts'], n
        assert rec[n]['vgprs'] <= 128 and rec[n]['occupancy'] >= 4 and rec[n]['scratch'] == 0, (n, rec[n])
    # the fixed-depth helicity kernel shares its walk with k_helicity_layers (which is held to four waves): it has run at
    # five waves per SIMD since it was written, and the shared walk must not cost it that
    for n in kernels:
        if 'k_storm_relative_helicity' in n:
            assert rec[n]['occupancy'] >= 5, (n, rec[n])
