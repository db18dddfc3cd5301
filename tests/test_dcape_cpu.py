"""Downdraft CAPE without a GPU: the NumPy restatement (tests/dcape_restatement.py) on hand-built columns, the C ABI
declarations, the xarray mirror (xarray_parcel_amd/downdraft.py) around a stubbed launch, and the kernel's resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import thermo as th
from tests import dcape_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import downdraft
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import parcel_functions as pf
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'

P = np.array([1000., 925., 850., 775., 700., 600., 500., 400., 300.])
T = np.array([303., 298., 293., 289., 283., 275., 266., 255., 241.])
TD = np.array([295., 291., 284., 276., 268., 256., 246., 236., 225.])


def _run(p, t=None, td=None, **kw):
    if t is None:
        t, td = np.interp(np.log(p), np.log(P[::-1]), T[::-1]), np.interp(np.log(p), np.log(P[::-1]), TD[::-1])
    return R.column(np.asarray(p, float), np.asarray(t, float), np.asarray(td, float), **kw)


# -- the restatement on hand-built columns ---------------------------------------------------------------------------
def test_bounds_on_levels_are_not_added():
    pts = R.layer_points(P, T, TD)
    assert list(pts[0]) == [700., 600., 500.] and list(pts[1]) == [283., 275., 266.]
    r = _run(P, T, TD)
    assert r['start_pressure'] in (700., 600., 500.) and r['status'] == 0
    assert r['dcape'] > 0 and np.isfinite(r['start_temperature'])
    k0 = list(P).index(r['start_pressure'])
    assert np.all(np.isfinite(r['parcel_temperature'][:k0 + 1])) and np.all(np.isnan(r['parcel_temperature'][k0 + 1:]))
    assert r['parcel_temperature'][k0] == r['start_temperature']                 # exact mode: the adiabat's own point


def test_bounds_between_levels_are_added_log_linear():
    p = np.array([1000., 900., 750., 650., 550., 450., 300.])
    t = np.array([300., 294., 285., 279., 271., 262., 245.])
    td = t - np.array([5., 7., 10., 14., 20., 24., 25.])
    P_, T_, TD_ = R.layer_points(p, t, td)
    assert list(P_) == [700., 650., 550., 500.]
    f = (np.log(700.) - np.log(650.)) / (np.log(750.) - np.log(650.))
    assert abs(T_[0] - (279. + (285. - 279.) * f)) < 1e-12 and abs(TD_[0] - (td[3] + (td[2] - td[3]) * f)) < 1e-12
    r = R.column(p, t, td)
    assert np.isfinite(r['dcape']) and r['start_pressure'] in P_


def test_level_close_to_the_bottom_replaces_it():
    p = P.copy()
    p[4] = 700.004                                     # within 1e-8 + 1e-5 * 700 = 0.007 hPa of 700: 700 is not added
    P_ = R.layer_points(p, T, TD)[0]
    assert P_[0] == 700.004 and 700. not in P_
    p[4] = 700.01                                      # not close: the level is below the layer and 700 is added
    P_ = R.layer_points(p, T, TD)[0]
    assert list(P_[:2]) == [700., 600.] and 700.01 not in P_


def test_theta_e_tie_goes_to_the_first_point(monkeypatch):
    monkeypatch.setattr(R, 'theta_e_of_points', lambda pts: np.full(len(pts[0]), 330.0))
    assert _run(P, T, TD)['start_pressure'] == 700.
    p = np.array([1000., 900., 750., 650., 550., 450., 300.])
    assert _run(p)['start_pressure'] == 700.          # the added bottom bound is the first point


def test_missing_levels_are_dropped():
    t, td = T.copy(), TD.copy()
    t[2] = np.nan
    td[5] = np.nan
    got = R.column(P, t, td)
    keep = np.array([0, 1, 3, 4, 6, 7, 8])
    want = R.column(P[keep], T[keep], TD[keep])
    for k in ('dcape', 'start_pressure', 'start_temperature', 'status'):
        assert got[k] == want[k], k
    assert np.array_equal(got['parcel_temperature'][keep], want['parcel_temperature'], equal_nan=True)
    assert np.isnan(got['parcel_temperature'][[2, 5]]).all()


@pytest.mark.parametrize('p', [np.array([690., 650., 600., 500., 400.]),            # surface above 700 hPa
                               np.array([1000., 850., 700., 600., 520.])])           # top below 500 hPa
def test_columns_that_miss_the_layer_are_nan(p):
    r = _run(p)
    assert r['status'] == R.ST_NO_LAYER
    assert all(np.isnan(r[k]) for k in ('dcape', 'start_pressure', 'start_temperature'))
    assert np.isnan(r['parcel_temperature']).all()


def test_surface_at_the_bottom_bound_gives_zero():
    p = np.array([700., 600., 500., 400.])
    t = np.array([283., 276., 268., 257.])
    td = np.array([243., 262., 255., 245.])           # dry at 700 hPa: the theta_e minimum sits on the surface
    r = R.column(p, t, td)
    assert r['start_pressure'] == 700. and r['dcape'] == 0.0 and r['status'] == 0


def saturated_column():
    """Td = T on the 'rk4' moist adiabat through 280 K at 700 hPa from the surface up to 500 hPa (both are levels)."""
    p = np.array([1000., 950., 900., 850., 800., 750., 700., 650., 600., 550., 500., 400., 300.])
    t = th.moist_lapse_rk4(p, 280.0, 700.0)
    t[-2:] = t[-3] - np.array([8., 20.])
    return p, t, t.copy()


def test_saturated_column_on_its_moist_adiabat_has_no_dcape():
    r = R.column(*saturated_column())
    assert r['status'] == 0 and abs(r['dcape']) < 0.01, r


# -- C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_dcape_out') == [f[0] for f in L.DcapeOut._fields_]
    got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES['xp_downdraft_cape']]
    assert got == _prototypes()['xp_downdraft_cape'] and 'xp_downdraft_cape' in L.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'XP_ST_NO_LAYER\s*=\s*16\b', hdr) and L.XP_ST_NO_LAYER == 16 == R.ST_NO_LAYER


# -- the mirror around a stubbed launch ------------------------------------------------------------------------------
def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def test_mirror_wraps_the_array_api(monkeypatch):
    seen = {}

    def run(self, name, *args):
        seen['name'], seen['args'] = name, args
    monkeypatch.setattr(api._Call, 'run', run)
    ds, prof = downdraft.downdraft_cape(_grid(P, 'pressure'), _grid(T, 'temperature'), _grid(TD, 'dewpoint'),
                                        bottom=650, depth=150)
    assert seen['name'] == 'xp_downdraft_cape'
    pv, tv, tdv, bottom, depth, mode, out = seen['args']
    assert (pv.nlev, pv.ncol, bottom, depth, mode) == (9, 6, 650.0, 150.0, L.MOIST['exact'])
    assert isinstance(bottom, float) and isinstance(depth, float)
    assert out.dtype == L.XP_F64 and out.mem == L.XP_MEM_HOST and all(getattr(out, k) for k in L.DCAPE_OUT)
    names = list(ds.data_vars) if hasattr(ds, 'data_vars') else list(ds.keys())
    assert names == ['dcape', 'dcape_start_pressure', 'dcape_start_temperature']
    for k in names:
        assert ds[k].dims == ('lat', 'lon') and ds[k].name == k and ds[k].shape == (2, 3)
        assert list(np.asarray(ds[k].coords['lat'])) == [10., 20.] and list(np.asarray(ds[k].coords['lon'])) == [1., 2., 3.]
    assert ds['dcape'].attrs == {'long_name': 'Downdraft convective available potential energy', 'units': 'J kg$^{-1}$'}
    assert ds['dcape_start_pressure'].attrs['units'] == 'hPa' and ds['dcape_start_temperature'].attrs['units'] == 'K'
    assert prof.name == 'dcape_parcel_temperature' and prof.dims == (VD, 'lat', 'lon') and prof.shape == (9, 2, 3)
    assert list(np.asarray(prof.coords[VD])) == list(range(1, 10)) and prof.attrs['units'] == 'K'


def test_mirror_passes_bottom_depth_and_moist(monkeypatch):
    calls = []

    def fake(p, t, td, **kw):
        calls.append(kw)
        h = p.shape[1:]
        return {'dcape': np.zeros(h), 'start_pressure': np.zeros(h), 'start_temperature': np.zeros(h),
                'status': np.zeros(h, np.int32), 'parcel_temperature': np.zeros(p.shape)}
    monkeypatch.setattr(api, 'downdraft_cape', fake)
    args = _grid(P, 'pressure'), _grid(T, 'temperature'), _grid(TD, 'dewpoint')
    downdraft.downdraft_cape(*args)
    downdraft.downdraft_cape(*args, bottom=800, depth=300, moist='family')
    pf.set_moist_lapse('table')
    downdraft.downdraft_cape(*args)
    assert calls == [{'bottom': 700, 'depth': 200, 'moist': 'exact', 'want_profile': True},
                     {'bottom': 800, 'depth': 300, 'moist': 'family', 'want_profile': True},
                     {'bottom': 700, 'depth': 200, 'moist': 'table', 'want_profile': True}]


def test_mirror_without_tables_asserts(monkeypatch):
    class _NoTables:
        def xp_tables_loaded(self):
            return 0
    monkeypatch.setattr(L, 'load', lambda: _NoTables())
    args = _grid(P, 'pressure'), _grid(T, 'temperature'), _grid(TD, 'dewpoint')
    pf.set_moist_lapse(None)
    with pytest.raises(AssertionError, match='Call load_moist_adiabat_lookups first.'):
        downdraft.downdraft_cape(*args)
    pf.set_moist_lapse('exact')

    def fail(self, name, *a):
        raise L.XParcelError(L.XP_E_NO_TABLES, 'stand-in')
    monkeypatch.setattr(api._Call, 'run', fail)
    with pytest.raises(AssertionError, match='Call load_moist_adiabat_lookups first.'):
        downdraft.downdraft_cape(*args, moist='table')


# -- kernel resources ------------------------------------------------------------------------------------------------
@needs_hipcc
def test_kernel_keeps_four_waves_per_simd_without_spills(tmp_path):
    rec = resources(tmp_path, 'xparcel.hip')
    kernels = [n for n in rec if 'k_downdraft_cape' in n]
    assert sorted(kernels) == ['_ZN2xp16k_downdraft_capeIdEEvNS_9DcapeArgsE', '_ZN2xp16k_downdraft_capeIfEEvNS_9DcapeArgsE']
    for n in kernels:
        assert rec[n]['in_asm'] and not rec[n]['scratch_insts'], n
        assert rec[n]['vgprs'] <= 128 and rec[n]['occupancy'] >= 4, (n, rec[n])
