"""Entraining CAPE without a GPU: the C ABI declarations, the array API and the DataArray module around a stubbed launch, the
NumPy restatement (tests/ecape_restatement.py) against closed forms, and the NCAPE kernel's resources."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from tests import ecape_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import entrainment
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

VD = 'model_level_number'
CHAIN_KEYS = ('ecape', 'ecape_a', 'psi', 'ncape', 'cape', 'cin', 'lfc_height', 'el_height', 'sr_u', 'sr_v', 'status')


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_ncape_out') == [f[0] for f in L.NcapeOut._fields_]
    assert [f[0] for f in L.NcapeOut._fields_][:4] == list(L.NCAPE_OUT) == list(R.KEYS)
    protos = _prototypes()
    for name in ('xp_ncape', 'xp_ecape'):
        got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[name]]
        assert got == protos[name] and name in L.SYMBOLS, name
    assert len(L.ARGTYPES['xp_ncape']) == 8 and len(L.ARGTYPES['xp_ecape']) == 3 + len(L.ECAPE_IN) + len(L.ECAPE_OUT) + 1
    assert (R.ST_BAD_PRESSURE, R.ST_NO_LAYER, R.ST_BAD_HEIGHT) == (L.ST_BAD_PRESSURE, L.XP_ST_NO_LAYER, L.ST_BAD_HEIGHT)
    assert any(u[1] == 'xp_ecape_tu.hip' for u in L.UNITS)


def test_the_constants_are_the_stated_ones():
    k, a, lmix, pr, s = 0.42, 0.8, 120.0, 1.0 / 3.0, 1.1
    assert abs(R.C_PSI - k * k * a * a * math.pi ** 2 * lmix / (4.0 * pr * s * s)) < 1e-13 * R.C_PSI
    src = open(L.SRC_DIR + '/xp_ecape.hpp').read() + open(L.SRC_DIR + '/xp_device.hpp').read()
    assert re.search(r'ECAPE_C_PSI = %r;' % R.C_PSI, src) and re.search(r'constexpr double G = %r;' % R.G, src)
    for name in ('RD', 'EPS', 'LV'):
        assert float(re.search(r'constexpr double %s = ([0-9.e+-]+);' % name, src).group(1)) == getattr(R, name)


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
def _fill(ptr, like, value):
    """Write `value` into the output array at address `ptr`, which has the shape and dtype of `like`."""
    np.frombuffer((C.c_char * like.nbytes).from_address(ptr), dtype=like.dtype)[:] = value


@pytest.fixture
def calls(monkeypatch):
    """The launches of the array API, recorded instead of run; the storm motions and the layer mean get known values."""
    seen = []

    def run(self, name, *args):
        seen.append((name, args))
        one = np.empty(self.ncol, self.dtype)
        if name == 'xp_bunkers_storm_motion':
            for i, k in enumerate(L.STORM_MOTION_OUT[:6]):
                _fill(getattr(args[4], k), one, float(i + 1))
        if name == 'xp_wind_layers':
            _fill(args[6].mean_u[0], one, 10.0)
            _fill(args[6].mean_v[0], one, 20.0)
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _cols(nlev=9, ncol=5, dtype=np.float32):
    return np.linspace(1000., 200., nlev, dtype=dtype)[:, None] * np.ones((1, ncol), dtype)


def test_ncape_array_api_arguments(calls):
    p = _cols()
    lfc, el = np.linspace(900., 800., 5), 300.0
    res = api.ncape(p, p, p, p, lfc, el)
    name, (pv, tv, tdv, zv, l, e, out) = calls[-1]
    assert name == 'xp_ncape' and all((v.nlev, v.ncol, v.dtype, v.mem) == (9, 5, L.XP_F32, L.XP_MEM_HOST) for v in (pv, tv, tdv, zv))
    assert l.dtype == np.float32 and np.array_equal(l, lfc.astype(np.float32)) and e.shape == (5,) and np.all(e == 300.0)
    assert set(res) == set(L.NCAPE_OUT) and res['ncape'].dtype == np.float32 and res['status'].dtype == np.int32
    assert [getattr(out, k) for k in L.NCAPE_OUT] == [res[k].ctypes.data for k in L.NCAPE_OUT]
    assert (out.dtype, out.mem) == (L.XP_F32, L.XP_MEM_HOST)
    p3 = p.reshape(9, 1, 5).astype(np.float64)
    res = api.ncape(p3, p3, p3, p3, lfc.reshape(1, 5), np.full((1, 5), np.nan))
    assert calls[-1][1][0].dtype == L.XP_F64 and res['el_height'].shape == (1, 5) and np.isnan(calls[-1][1][5]).all()
    with pytest.raises(AssertionError):
        api.ncape(p, p, p, p[:4], lfc, el)
    with pytest.raises(AssertionError):
        api.ncape(p, p, p, p, lfc[:3], el)


def test_ecape_from_ncape_goes_through_the_per_point_path(calls):
    x = np.ones((2, 3))
    res = api.ecape_from_ncape(x, 2 * x, 3 * x, 4 * x, 5 * x)
    name, a = calls[-1]
    assert name == 'xp_ecape' and a[:3] == (6, L.XP_F64, L.XP_MEM_HOST) and len(a) == 11
    assert [float(v.flat[0]) for v in a[3:8]] == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert list(res) == list(L.ECAPE_OUT) and all(a[8 + i] is res[k] and res[k].shape == (2, 3) for i, k in enumerate(L.ECAPE_OUT))
    with pytest.raises(AssertionError):
        api.ecape_from_ncape(x, x, x, x, x[:1])


@pytest.mark.parametrize('storm,motion', [('right', (1.0, 2.0)), ('left', (3.0, 4.0)), ('mean', (5.0, 6.0))])
def test_the_chain_reaches_the_abi_call_by_call(calls, storm, motion):
    p = _cols(dtype=np.float64)
    with np.errstate(all='ignore'):
        res = api.ecape(p, p, p, p, p, p, storm=storm, parcel='mixed_layer', depth=75.0, moist='exact',
                        virtual_temperature_correction=False)
    assert [n for n, _ in calls] == ['xp_cape_cin', 'xp_ncape', 'xp_bunkers_storm_motion', 'xp_wind_layers', 'xp_ecape']
    cc, nc, bm, wl, ec = (a for _, a in calls)
    assert cc[3].mode == L.PARCEL['mixed_layer'] and cc[3].depth == 75.0 and cc[4].moist_mode == L.MOIST['exact']
    assert cc[4].virtual_temperature_correction == 0 and cc[6] is None
    wanted = {k for k in L.SCALAR_F + L.SCALAR_I + L.SCALAR_P if getattr(cc[5], k)}
    assert wanted == {'cape', 'cin', 'lfc_pressure', 'el_pressure', 'status'}
    # NCAPE between the lift's own LFC and EL
    assert (nc[4].ctypes.data, nc[5].ctypes.data) == (cc[5].lfc_pressure, cc[5].el_pressure)
    # one layer, 0 ... 1000 m above the lowest valid level, its mean only
    assert wl[4] == 1 and (wl[5][0].kind, wl[5][0].bottom, wl[5][0].top) == (L.LAYER_HEIGHT, 0.0, 1000.0) and wl[3] is not None
    assert wl[6].mean_u[0] and wl[6].mean_v[0] and all(getattr(wl[6], k)[0] is None for k in L.WIND_LAYERS_OUT[2:])
    # the per-point call: cape of the lift, ncape and el_height of xp_ncape, the mean minus the chosen motion
    assert ec[3].ctypes.data == cc[5].cape and (ec[4].ctypes.data, ec[5].ctypes.data) == (nc[6].ncape, nc[6].el_height)
    assert np.all(ec[6] == 10.0 - motion[0]) and np.all(ec[7] == 20.0 - motion[1])
    assert set(res) == set(CHAIN_KEYS) and all(res[k].shape == (5,) for k in CHAIN_KEYS) and res['status'].dtype == np.int32
    assert res['sr_u'] is ec[6] and res['ecape'] is ec[8] and res['ecape_a'] is ec[9] and res['psi'] is ec[10]
    assert res['ncape'].ctypes.data == nc[6].ncape and res['lfc_height'].ctypes.data == nc[6].lfc_height


def test_a_given_storm_motion_replaces_bunkers(calls):
    p = _cols(dtype=np.float64)
    with np.errstate(all='ignore'):
        api.ecape(p, p, p, p, p, p, storm_u=4.0, storm_v=np.arange(5.0))
    assert [n for n, _ in calls] == ['xp_cape_cin', 'xp_ncape', 'xp_wind_layers', 'xp_ecape']
    cc, ec = calls[0][1], calls[-1][1]
    assert cc[3].mode == L.PARCEL['most_unstable'] and cc[3].depth == 300.0          # the defaults
    assert np.all(ec[6] == 6.0) and np.array_equal(ec[7], 20.0 - np.arange(5.0))
    for bad in ({'storm': 'up'}, {'storm_u': 1.0}, {'storm_v': 1.0}):
        with pytest.raises(AssertionError):
            api.ecape(p, p, p, p, p, p, **bad)
    assert 'pressure-weighted' in ' '.join(api.ecape.__doc__.lower().split())


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
    p, t, td, z, u, v = (_grid(f(lev), n) for f, n in ((lambda x: 1000. - 50 * x, 'p'), (lambda x: 300. - 5 * x, 't'),
                                                        (lambda x: 290. - 6 * x, 'td'), (lambda x: 500. * x, 'z'),
                                                        (lambda x: x, 'u'), (lambda x: -x, 'v')))
    ds = entrainment.ncape(p, t, td, z, _horiz(900.0, 'lfc'), 250.0)
    name, args = calls[-1]
    assert name == 'xp_ncape' and (args[0].nlev, args[0].ncol) == (9, 6) and np.all(args[4] == 900.0) and np.all(args[5] == 250.0)
    assert _names(ds) == list(L.NCAPE_OUT)
    assert ds['ncape'].dims == ('lat', 'lon') and ds['ncape'].attrs['units'] == 'J kg$^{-1}$' and ds['el_height'].attrs['units'] == 'm'
    h = [_horiz(x, 'x') for x in (2000., 300., 11000., 8., -3.)]
    ds = entrainment.ecape_from_ncape(*h)
    assert calls[-1][0] == 'xp_ecape' and calls[-1][1][0] == 6 and np.all(calls[-1][1][5] == 11000.0)
    assert _names(ds) == list(L.ECAPE_OUT) and ds['psi'].dims == ('lat', 'lon') and ds['psi'].attrs['units'] == '1'
    del calls[:]
    with np.errstate(all='ignore'):
        ds = entrainment.ecape(p, t, td, z, u, v, storm='left', moist='exact')
    assert [n for n, _ in calls] == ['xp_cape_cin', 'xp_ncape', 'xp_bunkers_storm_motion', 'xp_wind_layers', 'xp_ecape']
    assert np.all(calls[-1][1][6] == 10.0 - 3.0) and _names(ds) == list(CHAIN_KEYS)
    del calls[:]
    with np.errstate(all='ignore'):
        ds = entrainment.ecape(p, t, td, z, u, v, storm_u=_horiz(2.0, 'su'), storm_v=1.0, parcel='surface', moist='exact')
    assert [n for n, _ in calls] == ['xp_cape_cin', 'xp_ncape', 'xp_wind_layers', 'xp_ecape'] and np.all(calls[-1][1][6] == 8.0)
    assert calls[0][1][3].mode == L.PARCEL['surface']
    for k in CHAIN_KEYS:
        assert ds[k].dims == ('lat', 'lon') and ds[k].name == k and 'long_name' in ds[k].attrs
        assert k == 'status' or 'units' in ds[k].attrs


# -- the restatement against closed forms ---------------------------------------------------------------------------------
def _column(nlev=24, top=13000.0, z0=150.0, p0=1005.0):
    z = z0 + np.linspace(0.0, top, nlev) + np.r_[0.0, np.sin(np.arange(1, nlev)) * 60.0]
    p = p0 * np.exp(-(z - z0) / 8000.0)
    t = 300.0 - 6.5e-3 * (z - z0) + np.cos(z / 1500.0)
    td = t - 3.0 - 2.0e-3 * (z - z0)
    return p, t, td, z


def _hand(p, z, b, L, E):
    """trapz(b, z) between the pressures L > E with the two bounds interpolated by hand."""
    def at(pb):
        k = int(np.nonzero(p <= pb)[0][0])
        if p[k] == pb:
            return z[k], b[k]
        f = math.log(pb / p[k]) / math.log(p[k - 1] / p[k])
        return z[k] + f * (z[k - 1] - z[k]), b[k] + f * (b[k - 1] - b[k])
    (zl, bl), (ze, be) = at(L), at(E)
    mid = (p < L) & (p > E)
    Z, B = np.r_[zl, z[mid], ze], np.r_[bl, b[mid], be]
    return float(np.sum(0.5 * (B[1:] + B[:-1]) * np.diff(Z))), zl - z[0], ze - z[0]


def test_constant_moist_static_energy_is_its_own_mean():
    p, _, td, z = _column()
    h0 = 3.4e5
    w = R.sat_mix(p, td)
    t = (h0 - R.LV * (w / (1.0 + w)) - R.G * z) / R.CP_D            # h = cp T + Lv q + g z = h0 at every level
    _, _, h, hs, hbar, b = R.levels(p, t, td, z)
    assert np.allclose(h, h0, rtol=1e-14, atol=0.0) and np.allclose(hbar, h0, rtol=1e-13, atol=0.0)
    assert np.allclose(b, -(R.G / (R.CP_D * t)) * (h0 - hs), rtol=0.0, atol=1e-12)
    assert np.array_equal(b > 0.0, t > td)                         # positive where the level is unsaturated (hs > h)


def test_bounds_on_and_between_levels_agree_with_a_hand_trapezoid():
    p, t, td, z = _column()
    pv, zv, _, _, hbar, b = R.levels(p, t, td, z)
    assert hbar[0] == R.levels(p, t, td, z)[2][0]
    for L, E in ((p[3], p[9]), (0.5 * (p[3] + p[4]), 0.5 * (p[9] + p[10])), (p[3], 0.3 * p[9] + 0.7 * p[10]),
                 (0.9 * p[5] + 0.1 * p[6], 0.2 * p[5] + 0.8 * p[6])):
        r = R.column(p, t, td, z, L, E)
        want = _hand(pv, zv, b, L, E)
        assert r['status'] == 0 and abs(r['ncape'] - want[0]) < 1e-9 * max(1.0, abs(want[0]))
        assert abs(r['lfc_height'] - want[1]) < 1e-9 and abs(r['el_height'] - want[2]) < 1e-9
    r = R.column(p, t, td, z, p[3], p[9])
    assert r['ncape'] == sum((0.5 * (b[k] + b[k - 1])) * (z[k] - z[k - 1]) for k in range(4, 10))
    assert (r['lfc_height'], r['el_height']) == (z[3] - z[0], z[9] - z[0])


def test_ncape_is_additive_over_abutting_layers():
    p, t, td, z = _column()
    L, E = 0.4 * p[2] + 0.6 * p[3], 0.5 * (p[17] + p[18])
    whole = R.column(p, t, td, z, L, E)
    for M in (p[8], 0.3 * p[8] + 0.7 * p[9], 0.5 * (L + p[3])):
        lo, hi = R.column(p, t, td, z, L, M), R.column(p, t, td, z, M, E)
        assert abs(lo['ncape'] + hi['ncape'] - whole['ncape']) < 1e-9 * abs(whole['ncape'])
        assert abs(lo['el_height'] - hi['lfc_height']) < 1e-9 and lo['lfc_height'] == whole['lfc_height']


def test_clamped_bounds_and_a_missing_el_give_the_integral_to_the_top():
    p, t, td, z = _column()
    full = R.column(p, t, td, z, p[0], p[-1])
    assert full['status'] == 0 and (full['lfc_height'], full['el_height']) == (0.0, z[-1] - z[0])
    for L, E in ((2000.0, np.nan), (p[0], np.nan), (1100.0, 1.0), (p[0] * (1 + 1e-12), p[-1] * (1 - 1e-12))):
        r = R.column(p, t, td, z, L, E)
        assert r == full, (L, E, r)
    part = R.column(p, t, td, z, p[6], np.nan)
    assert part['ncape'] == R.column(p, t, td, z, p[6], 5.0)['ncape'] == R.column(p, t, td, z, p[6], p[-1])['ncape']
    # empty after clamping: both bounds below the lowest level, or both above the highest
    lo, hi = R.column(p, t, td, z, 1500.0, 1200.0), R.column(p, t, td, z, 50.0, 20.0)
    assert (lo['ncape'], lo['lfc_height'], lo['el_height'], lo['status']) == (0.0, 0.0, 0.0, 0)
    assert (hi['ncape'], hi['lfc_height'], hi['el_height'], hi['status']) == (0.0, z[-1] - z[0], z[-1] - z[0], 0)


def test_bounds_rules_missing_levels_and_ordering():
    p, t, td, z = _column()
    r = R.column(p, t, td, z, np.nan, 300.0)
    assert (r['ncape'], r['status']) == (0.0, 0) and np.isnan(r['lfc_height']) and np.isnan(r['el_height'])
    assert R.column(p * np.nan, t, td, z, np.nan, np.nan)['ncape'] == 0.0                # whatever the column holds
    for L, E in ((500.0, 500.0), (500.0, 700.0)):
        r = R.column(p, t, td, z, L, E)
        assert r['status'] == R.ST_NO_LAYER and np.isnan([r['ncape'], r['lfc_height'], r['el_height']]).all()
    one = np.where(np.arange(p.size) == 4, p, np.nan)
    for pp in (one, p * np.nan):
        r = R.column(pp, t, td, z, 900.0, 300.0)
        assert r['status'] == R.ST_NO_LAYER and np.isnan(r['ncape'])
    # missing levels are dropped
    t2, z2, p2 = t.copy(), z.copy(), p.copy()
    t2[3], z2[9], p2[5] = np.nan, np.nan, np.nan
    keep = np.ones(p.size, bool)
    keep[[3, 5, 9]] = False
    assert R.column(p2, t2, td, z2, 880.0, 260.0) == R.column(p[keep], t[keep], td[keep], z[keep], 880.0, 260.0)
    # the order is checked on the levels read only
    p3, z3 = p.copy(), z.copy()
    p3[-1], z3[-1] = p3[-2] + 5.0, z3[-2] - 5.0
    assert R.column(p3, t, td, z3, 900.0, p[10])['status'] == 0
    r = R.column(p3, t, td, z3, 900.0, np.nan)
    assert r['status'] == (R.ST_BAD_PRESSURE | R.ST_BAD_HEIGHT) and np.isnan(r['ncape'])
    z4 = z.copy()
    z4[5] = z4[4]
    assert R.column(p, t, td, z4, 900.0, 300.0)['status'] == R.ST_BAD_HEIGHT
    assert R.column(p, t, td, z4, 2000.0, 1500.0)['status'] == 0                         # two levels read


def test_the_formula_at_its_limits():
    e = lambda *a: tuple(float(x) for x in R.ecape_value(*a))
    assert abs(e(3000.0, 500.0, 1e15, 15.0, 0.0)[0] - 3000.0) < 1e-6                      # psi -> 0: no entrainment
    assert abs(e(3000.0, 500.0, 12000.0, 9.0, 12.0)[0] - 2514.0) < 0.5                   # |(9, 12)| = 15
    assert abs(e(3000.0, 500.0, 12000.0, 1e-3, 0.0)[0]) < 1e-2 and e(3000.0, 500.0, 12000.0, 0.0, 0.0) == e(3000.0, 500.0, 12000.0, 1e-3, 0.0)
    assert abs(e(1000.0, -200.0, 12000.0, 0.0, 0.0)[0] - 200.0) < 1e-2                   # V -> 0: max(0, -ncape)
    assert abs(e(1000.0, 0.0, 12000.0, 15.0, 0.0)[2] - R.C_PSI / 12000.0) == 0.0
    for cape in (0.0, -5.0):
        assert e(cape, 500.0, 12000.0, 15.0, 0.0)[:2] == (0.0, 0.0) and e(cape, 500.0, 12000.0, 15.0, 0.0)[2] > 0.0
    for i in range(5):
        x = [3000.0, 500.0, 12000.0, 15.0, 3.0]
        x[i] = np.nan
        assert np.isnan(e(*x)).all()
    for h in (0.0, -100.0):
        assert np.isnan(e(3000.0, 500.0, h, 15.0, 3.0)).all()
    # monotone: more dilution potential, less ECAPE; and never more than ... the undiluted CAPE plus nothing
    n = np.linspace(-500.0, 3000.0, 50)
    en = R.ecape_value(3000.0, n, 12000.0, 15.0, 0.0)[0]
    assert np.all(np.diff(en) < 0.0)


def test_ecape_a_exceeds_ecape_by_the_inflow_kinetic_energy():
    rng = np.random.default_rng(3)
    cape, ncape = rng.uniform(500.0, 5000.0, 2000), rng.uniform(-300.0, 1500.0, 2000)
    h, su, sv = rng.uniform(5000.0, 16000.0, 2000), rng.normal(0, 12, 2000), rng.normal(0, 12, 2000)
    en, ea, _ = R.ecape_value(cape, ncape, h, su, sv)
    k = 0.5 * np.hypot(su, sv) ** 2
    free = (en > 0.0) & (ea > 0.0)
    assert free.sum() > 1500 and np.max(np.abs((ea - en - k)[free])) <= 1e-12 * np.max(ea)
    assert np.all(ea[~free] >= 0.0) and np.all(en[~free] == 0.0)


# -- kernel resources -----------------------------------------------------------------------------------------------------
@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_ncape is instantiated on the dtype only: two kernels, neither of which may use scratch or spill a vector register,
    and both of which keep at least four waves per SIMD (DESIGN.md section 7 records the counts printed here)."""
    unit = [x for x in L.UNITS if x[1] == 'xp_ecape_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    walk = {}
    for n, r in rec.items():
        m = re.search(r'k_ncapeI([df])E', n)
        if m:
            walk[m.group(1)] = r
    assert sorted(walk) == ['d', 'f'], sorted(rec)
    for key, r in walk.items():
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['occupancy'] >= 4 and r['vgprs'] <= 128, (key, r)
