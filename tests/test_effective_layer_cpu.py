"""Effective inflow layer and helicity / bulk wind difference over per-column layers without a GPU: the NumPy restatement
on hand-built columns, the C ABI declarations against ctypes, the array API and the DataArray module around a stubbed
launch, and the operating point of the two kernels (cross-compiled for gfx950)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import effective_layer_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from tests.test_kinematics_cpu import circular_hodograph
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import kinematics
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'


# -- hand-built columns -----------------------------------------------------------------------------------------------------
def sounding(t_sfc=303.0, td_sfc=296.0, moist_top=850.0, nlev=40, cap=0.0, sfc_cool=0.0, sfc_levels=0):
    """40 levels from 1000 to 100 hPa: 6.8 K/km down to 210 K, a moist layer below `moist_top` hPa and dry air above;
    `cap` warms everything above 880 hPa, `sfc_cool` cools the lowest `sfc_levels` levels (kept 1 K from saturation)."""
    p = np.linspace(1000.0, 100.0, nlev)
    z = 44330.8 * (1 - (p / 1013.25) ** 0.190263)
    t = np.maximum(t_sfc - 6.8e-3 * (z - z[0]), 210.0)
    t[p < 880.0] += cap
    td = np.where(p >= moist_top, td_sfc - 2.0e-3 * (z - z[0]), t - 15.0 - 10.0 * (moist_top - p) / moist_top)
    td = np.minimum(td, t - 0.5)
    t[:sfc_levels] -= sfc_cool
    td[:sfc_levels] = np.minimum(td[:sfc_levels], t[:sfc_levels] - 1.0)
    return p, t, td, z


def restate(col, **kw):
    p, t, td, z = col
    r = R.inflow_grid(p[:, None], t[:, None], td[:, None], z=z[:, None], **kw)
    return {k: (v[0] if v.ndim == 1 else v[:, 0]) for k, v in r.items()}


def test_stable_column_has_no_layer():
    r = restate(sounding(t_sfc=285.0, td_sfc=265.0))
    assert r['status'] == R.ST_NO_LAYER and r['base_index'] == -1 and r['top_index'] == -1
    assert all(np.isnan(r[k]) for k in R.OUT_F)
    p = sounding()[0]
    lifted = ~np.isnan(r['candidate_cape'])
    assert np.array_equal(lifted, p >= 700.0) and np.all(r['candidate_cape'][lifted] < 100.0)   # the whole window was tried


def test_surface_based_layer():
    col = sounding()
    r = restate(col)
    assert r['status'] == 0 and r['base_index'] == 0 and r['top_index'] == 6
    assert r['base_pressure'] == col[0][0] and r['top_pressure'] == col[0][6]
    assert r['base_height'] == 0.0 and r['top_height'] == col[3][6] - col[3][0]
    cc, ci = r['candidate_cape'], r['candidate_cin']
    assert np.all(cc[:7] >= 100.0) and np.all(ci[:7] >= -250.0) and cc[7] < 100.0     # level 7 closes the layer ...
    assert np.all(np.isnan(cc[8:])) and np.all(np.isnan(ci[8:]))                      # ... and nothing above it is lifted
    # candidate k IS the surface parcel of the column cut off below k
    from oracle import c_oracle
    one = c_oracle.cape_cin_grid(col[0][3:, None], col[1][3:, None], col[2][3:, None], parcel='surface', moist='rk4')
    assert cc[3] == one['cape'][0] and ci[3] == one['cin'][0]
    # without heights the indices and pressures stand, the heights are NaN
    p, t, td, _ = col
    r2 = R.inflow_grid(p[:, None], t[:, None], td[:, None])
    assert r2['base_index'][0] == 0 and np.isnan(r2['base_height'][0]) and np.isnan(r2['top_height'][0])


def test_capped_column_has_an_elevated_base():
    col = sounding(t_sfc=305.0, td_sfc=297.0, cap=3.0, sfc_cool=4.0, sfc_levels=2)
    r = restate(col)
    cc, ci = r['candidate_cape'], r['candidate_cin']
    assert np.all(cc[:2] >= 100.0) and np.all(ci[:2] < -250.0)                        # the CAPE is there, the cap is too strong
    assert r['status'] == 0 and r['base_index'] == 2 and r['top_index'] == 6
    assert r['base_height'] == col[3][2] - col[3][0] and r['base_height'] > 0.0
    # with a laxer CIN threshold the same column is surface based
    assert restate(col, cin_min=-400.0)['base_index'] == 0
    # and with a CAPE threshold nobody meets it has no layer
    assert restate(col, cape_min=1e5)['status'] == R.ST_NO_LAYER


def test_missing_level_neither_closes_nor_extends_the_layer():
    col = sounding()
    col[1][3] = np.nan                                                                # inside the layer
    r = restate(col)
    assert r['status'] == 0 and r['base_index'] == 0 and r['top_index'] == 6
    assert np.isnan(r['candidate_cape'][3]) and np.isfinite(r['candidate_cape'][4])
    col = sounding()
    col[2][6] = np.nan                                                                # the top level itself: the layer ends below
    r = restate(col)
    assert r['base_index'] == 0 and r['top_index'] == 5 and np.isnan(r['candidate_cape'][6])
    col = sounding()
    col[0][0] = np.nan                                                                # the lowest level: the column starts at 1
    r = restate(col)
    assert r['base_index'] == 1 and r['base_height'] == 0.0 and r['base_pressure'] == col[0][1]


def test_window_cuts_the_layer():
    col = sounding()
    r = restate(col, search_depth=60.0)
    assert r['status'] == R.ST_LAYER_OPEN == 64 and r['base_index'] == 0 and r['top_index'] == 2
    assert np.all(np.isnan(r['candidate_cape'][3:]))
    r = restate(col, search_depth=1.0)                                                # smaller than the level spacing
    assert r['status'] == R.ST_LAYER_OPEN and r['base_index'] == 0 and r['top_index'] == 0
    assert r['base_height'] == 0.0 and r['top_height'] == 0.0


def test_layers_restatement_against_the_scalar_one():
    from tests import kinematics_restatement as K
    h, u, v = circular_hodograph()
    want = K.srh_column(h, u, v, [1000.0, 2400.0], bottom=500.0, storm_u=1.0, storm_v=-4.0)
    got = R.layers_column(h, u, v, 500.0, [1500.0, 2900.0], storm_u=1.0, storm_v=-4.0)
    for k in K.SRH_KEYS:
        assert np.array_equal(got[k], want[k]) and np.all(np.isfinite(got[k])), k
    assert got['status'] == 0 and abs(got['total'][1]) > 10.0
    # the bulk wind difference: wind at top minus wind at bottom, linear in height
    hh = np.array([0., 400., 900., 2500.])
    r = R.layers_column(hh, hh * 0.01, 5.0 - hh * 0.002, 200.0, [900.0, 1700.0])
    assert np.allclose(r['shear_u'], [7.0, 15.0]) and np.allclose(r['shear_v'], [-1.4, -3.0])
    # NaN, inverted, negative and unspanned bounds
    r = R.layers_column(hh, hh * 0.01, hh * 0.002, 200.0, [np.nan, 100.0, 2600.0, 900.0])
    assert r['status'] == R.ST_NO_LAYER and np.isnan(r['total'][:3]).all() and np.isfinite(r['total'][3])
    assert np.isnan(r['shear_u'][:3]).all() and np.isfinite(r['shear_u'][3])
    for b in (np.nan, -1.0):
        r = R.layers_column(hh, hh * 0.01, hh * 0.002, b, [900.0])
        assert r['status'] == R.ST_NO_LAYER and np.isnan(r['total'][0]) and np.isnan(r['shear_v'][0])
    r = R.layers_column(hh, hh * 0.01, hh * 0.002, 0.0, [900.0], storm_u=np.nan)
    assert r['status'] == 0 and np.isnan(r['total'][0]) and np.isfinite(r['shear_u'][0])


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_effective_layer_out') == [f[0] for f in L.EffectiveLayerOut._fields_]
    assert _struct_fields('xp_srh_layers_out') == [f[0] for f in L.SrhLayersOut._fields_]
    protos = _prototypes()
    for name in ('xp_effective_inflow_layer', 'xp_storm_relative_helicity_layers'):
        got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[name]]
        assert got == protos[name] and name in L.SYMBOLS, name
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'XP_ST_LAYER_OPEN\s*=\s*64\b', hdr) and L.ST_LAYER_OPEN == 64 == R.ST_LAYER_OPEN
    assert re.search(r'void \*shear_u\[4\], \*shear_v\[4\];', hdr) and L.SRH_MAX_DEPTHS == 4
    assert not [k for k in dir(L) if k.startswith('XP_E_') and k not in
                ('XP_E_ARG', 'XP_E_NOT_INIT', 'XP_E_NO_TABLES', 'XP_E_INTERP', 'XP_E_HIP', 'XP_E_NO_DEVICE')]
    L.build()
    lib = L.load()
    assert hasattr(lib, 'xp_effective_inflow_layer') and hasattr(lib, 'xp_storm_relative_helicity_layers')


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def _horiz(val, name):
    return DataArray(np.full((2, 3), val), dims=('lat', 'lon'), coords={'lat': [10., 20.], 'lon': [1., 2., 3.]}, name=name)


def test_effective_layer_array_api_arguments(monkeypatch):
    seen = {}

    def run(self, name, *args):
        seen['name'], seen['args'] = name, args
    monkeypatch.setattr(api._Call, 'run', run)
    p = np.linspace(1000., 300., 9, dtype=np.float32)[:, None] * np.ones((1, 5), np.float32)
    res = api.effective_inflow_layer(p, p, p)
    pv, tv, tdv, zv, cape_min, cin_min, depth, o, out = seen['args']
    assert seen['name'] == 'xp_effective_inflow_layer' and (pv.nlev, pv.ncol, pv.dtype) == (9, 5, L.XP_F32)
    assert zv is None and (cape_min, cin_min, depth) == (100.0, -250.0, 300.0)
    assert (o.virtual_temperature_correction, o.lcl_interp, o.pos_cape_neg_cin, o.post_zero_cin) == (1, 1, 1, 0)
    assert o.moist_mode == L.MOIST['exact'] and o.humidity == L.HUMIDITY['dewpoint']
    assert set(res) == set(L.EFFECTIVE_F + L.EFFECTIVE_I)
    assert res['base_pressure'].shape == (5,) and res['base_pressure'].dtype == np.float32
    assert res['base_index'].dtype == np.int32 and res['status'].dtype == np.int32
    assert out.base_pressure == res['base_pressure'].ctypes.data and out.top_index == res['top_index'].ctypes.data
    assert out.candidate_cape is None and out.candidate_cin is None and out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    p64 = p.astype(np.float64).reshape(9, 1, 5)
    res = api.effective_inflow_layer(p64, p64, p64, height=p64, cape_min=50, cin_min=-100, search_depth=200, moist='table',
                                     want_candidates=True, virtual_temperature_correction=False, lcl_interp='linear',
                                     pos_cape_neg_cin=False, post_zero_cin=True)
    pv, tv, tdv, zv, cape_min, cin_min, depth, o, out = seen['args']
    assert (zv.nlev, zv.ncol, zv.dtype) == (9, 5, L.XP_F64) and (cape_min, cin_min, depth) == (50.0, -100.0, 200.0)
    assert (o.virtual_temperature_correction, o.lcl_interp, o.pos_cape_neg_cin, o.post_zero_cin, o.moist_mode) == (0, 0, 0, 1, 1)
    assert res['candidate_cape'].shape == (9, 1, 5) and res['top_height'].shape == (1, 5)
    assert out.candidate_cin == res['candidate_cin'].ctypes.data
    with pytest.raises(AssertionError):
        api.effective_inflow_layer(p, p, p, humidity='specific')
    with pytest.raises(AssertionError):
        api.effective_inflow_layer(p, p, p[:4])


def test_layers_array_api_arguments(monkeypatch):
    seen = {}

    def run(self, name, *args):
        seen['name'], seen['args'] = name, args
    monkeypatch.setattr(api._Call, 'run', run)
    z = np.linspace(0., 4000., 9, dtype=np.float32)[:, None] * np.ones((1, 5), np.float32)
    b, t1, t2 = np.arange(5.) * 10, np.full(5, 1000.0), np.full(5, 3000.0)
    res = api.storm_relative_helicity_layers(z, z, z, b, [t1, t2], storm_u=2.5)
    zv, uv, vv, su, sv, cu, cv, bottom, nl, tops, out = seen['args']
    assert seen['name'] == 'xp_storm_relative_helicity_layers' and (zv.nlev, zv.ncol, zv.dtype) == (9, 5, L.XP_F32)
    assert su is None and sv is None and np.all(cu == 2.5) and np.all(cv == 0.0)
    assert bottom.dtype == np.float32 and np.array_equal(bottom, b.astype(np.float32)) and nl == 2 and len(tops) == 2
    assert set(res) == {'positive', 'negative', 'total', 'shear_u', 'shear_v', 'shear_magnitude', 'status'}
    assert res['total'].shape == (2, 5) and res['shear_magnitude'].shape == (2, 5) and res['status'].shape == (5,)
    assert out.shear_u[1] == res['shear_u'][1].ctypes.data and out.total[0] == res['total'][0].ctypes.data
    assert out.shear_v[2] is None and out.dtype == L.XP_F32 and out.mem == L.XP_MEM_HOST
    res = api.storm_relative_helicity_layers(z, z, z, 0.0, t1, surface_u=np.ones(5), surface_v=0.0)
    assert res['shear_u'].shape == (5,) and seen['args'][8] == 1 and np.all(seen['args'][7] == 0.0) and np.all(seen['args'][3] == 1.0)
    with pytest.raises(AssertionError):
        api.storm_relative_helicity_layers(z, z, z, b, [t1] * 5)
    with pytest.raises(AssertionError):
        api.storm_relative_helicity_layers(z, z, z, b, t1, surface_u=1.0)
    with pytest.raises(AssertionError):
        api.storm_relative_helicity_layers(z, z, z, b[:3], t1)


def test_mirror_wraps_the_array_api(monkeypatch):
    calls = []

    def run(self, name, *args):
        calls.append((name, args))
    monkeypatch.setattr(api._Call, 'run', run)
    lev = np.arange(1., 10.)
    ds = kinematics.effective_inflow_layer(_grid(1000. - 50 * lev, 'p'), _grid(300. - lev, 't'), _grid(290. - lev, 'td'),
                                           _grid(500. * lev, 'z'), cape_min=50.0, want_candidates=True)
    name, args = calls[-1]
    assert name == 'xp_effective_inflow_layer' and (args[0].nlev, args[0].ncol) == (9, 6) and args[4] == 50.0
    names = list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys())
    assert names == list(kinematics._EFFECTIVE) + ['candidate_cape', 'candidate_cin']
    assert ds['base_height'].dims == ('lat', 'lon') and ds['base_height'].attrs['units'] == 'm'
    assert ds['top_pressure'].attrs['units'] == 'hPa' and ds['base_index'].values.dtype == np.int32
    assert ds['candidate_cape'].dims == (VD, 'lat', 'lon') and ds['candidate_cape'].shape == (9, 2, 3)
    ds = kinematics.effective_inflow_layer(_grid(1000. - 50 * lev, 'p'), _grid(300. - lev, 't'), _grid(290. - lev, 'td'))
    assert calls[-1][1][3] is None and 'candidate_cape' not in ds
    ds = kinematics.storm_relative_helicity_layers(_grid(500. * lev, 'z'), _grid(lev, 'u'), _grid(lev, 'v'),
                                                   _horiz(100.0, 'b'), _horiz(2000.0, 't'), storm_u=_horiz(3.0, 'su'))
    name, args = calls[-1]
    assert name == 'xp_storm_relative_helicity_layers' and np.all(args[7] == 100.0) and np.all(args[5] == 3.0) and args[8] == 1
    assert ds['total_srh'].dims == ('lat', 'lon') and ds['shear_magnitude'].attrs['units'] == 'm s$^{-1}$'
    ds = kinematics.storm_relative_helicity_layers(_grid(500. * lev, 'z'), _grid(lev, 'u'), _grid(lev, 'v'), 0.0,
                                                   [_horiz(2000.0, 't'), 3000.0])
    assert calls[-1][1][8] == 2 and ds['shear_u'].dims == ('srh_layer', 'lat', 'lon')
    assert list(ds['shear_u'].coords['srh_layer']) == [0, 1]


def test_parcel_functions_gains_nothing():
    from xarray_parcel_amd import parcel_functions as pf
    for name in ('effective_inflow_layer', 'storm_relative_helicity_layers'):
        assert not hasattr(pf, name)


# -- kernel resources -----------------------------------------------------------------------------------------------------
def _check(rec, kernels, lds_cap=None):
    for n in kernels:
        print(n, rec[n])
        assert rec[n]['in_asm'] and not rec[n]['scratch_insts'], n
        assert rec[n]['vgprs'] <= 128 and rec[n]['occupancy'] >= 4 and rec[n]['scratch'] == 0, (n, rec[n])
        if lds_cap is not None:
            assert rec[n]['lds'] <= lds_cap, (n, rec[n])


@needs_hipcc
def test_kernels_keep_four_waves_per_simd_without_spills(tmp_path):
    """Both kernels, f32 and f64: at most 128 VGPRs, four waves per SIMD, no scratch at all (ScratchSize 0, no scratch
    instruction in the body), and the inflow kernel's LDS -- the e_s / ln table plus 13 Scan slots per thread -- within 40 KB,
    i.e. four workgroups per CU.  The layers kernel lives in xparcel.hip; the inflow kernel is compiled as the library
    compiles it, in its own unit with that unit's flags (_lib.UNITS)."""
    rec = resources(tmp_path, 'xparcel.hip')
    layers = [n for n in rec if re.search(r'k_helicity_layersI', n)]
    assert len(layers) == 2, sorted(rec)
    assert not [n for n in rec if 'k_effective_inflow' in n]
    _check(rec, layers)
    unit = [u for u in L.UNITS if u[1] == 'xp_effective_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    inflow = [n for n in rec if re.search(r'k_effective_inflowI', n)]
    assert len(inflow) == 4, sorted(rec)                                  # f64 / f32 x RK4 / lookup tables
    _check(rec, inflow, lds_cap=40 * 1024)
