"""Hydrostatic heights and thickness without a GPU: the C ABI declarations, the array API and the DataArray module around a
stubbed launch, the NumPy restatement (tests/hydrostatic_restatement.py) against closed forms, a census of the inputs the
device tests run on (tests/hydrostatic_cases.py), and the kernel's resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import hydrostatic_cases as K
from tests import hydrostatic_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import hydrostatic as mirror
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'
NAN = float('nan')
ENTRY = 'xp_hydrostatic_height'
POINT = ('xp_geopotential_to_height', 'xp_height_to_geopotential')


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_hydrostatic_out') == [f[0] for f in L.HydrostaticOut._fields_]
    assert _struct_fields('xp_hydrostatic_opts') == [f[0] for f in L.HydrostaticOpts._fields_]
    assert C.sizeof(L.HydrostaticOut) == 6 * 8 + 8 and C.sizeof(L.HydrostaticOpts) == 8
    assert L.HydrostaticOut.thickness.size == 4 * 8 == L.HYDRO_MAX_LAYERS * 8
    protos = _prototypes()
    kinds = lambda name: ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[name]]
    assert kinds(ENTRY) == protos[ENTRY] == ['pointer'] * 4 + ['int32'] + ['pointer'] * 4 and ENTRY in L.SYMBOLS
    for name in POINT:
        assert kinds(name) == protos[name] == ['int64', 'int32', 'int32', 'pointer', 'pointer', 'pointer'] and name in L.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'XP_HUM_DEWPOINT = %d, XP_HUM_SPECIFIC = %d\b' % (L.HUM_DEWPOINT, L.HUM_SPECIFIC), hdr)
    assert L.XP_ST_NO_LAYER == R.ST_NO_LAYER and L.ST_BAD_PRESSURE == R.ST_BAD_PRESSURE
    assert (L.LAYER_PRESSURE, L.LAYER_PRESSURE_DEPTH) == (R.PRESSURE, R.PRESSURE_DEPTH)
    section = hdr[hdr.index('Hydrostatic heights and layer thickness'):hdr.index('xp_hydrostatic_opts;')]
    assert 'UNPINNED' in section and 'not as mixing ratio' in section and '(Rd / g) * (0.5 * (Tv_a + Tv_b)) * (x_a - x_b)' in section
    assert '%r' % R.RD in section and '%r' % R.G in section and '%r' % R.RE in hdr
    unit = [u for u in L.UNITS if u[1] == 'xp_hydrostatic_tu.hip']
    assert unit == [('hydrostatic', 'xp_hydrostatic_tu.hip', L.HYDROSTATIC_FLAGS)]


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def run(self, name, *args):
        if name in POINT:
            n, dtype, mem, src, dst = args
            seen.append(dict(name=name, n=n, dtype=dtype, mem=mem, src=src, dst=dst))
            return
        p, t, m, base, nlayer, layers, opts, out = args
        seen.append(dict(name=name, p=p, t=t, m=m, base=base, nlayer=nlayer,
                         layers=[(layers[i].kind, layers[i].bottom, layers[i].top) for i in range(nlayer)], layers_arg=layers,
                         opts=(opts.humidity, opts.reserved), height=out.height, thickness=list(out.thickness), status=out.status,
                         dtype=out.dtype, mem=out.mem))
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _cols(nlev=9, ncol=5, dtype=np.float32):
    return np.ascontiguousarray(np.linspace(1000., 200., nlev, dtype=dtype)[:, None] * np.ones((1, ncol), dtype))


def _same(a, b):
    return all((np.isnan(x) and np.isnan(y)) or x == y for la, lb in zip(a, b) for x, y in zip(la, lb)) and len(a) == len(b)


def test_array_api_arguments_and_defaults(calls):
    p, t, td = _cols(), _cols() * 0.3, _cols() * 0.29
    res = api.hydrostatic(p, t, td, layers=K.API_LAYERS)
    c = calls[-1]
    assert len(calls) == 1 and c['name'] == ENTRY
    assert (c['p'].nlev, c['p'].ncol, c['p'].dtype, c['p'].mem) == (9, 5, L.XP_F32, L.XP_MEM_HOST)
    assert (c['p'].data, c['t'].data, c['m'].data) == (p.ctypes.data, t.ctypes.data, td.ctypes.data)
    assert c['base'] is None and c['opts'] == (L.HUM_DEWPOINT, 0) and (c['dtype'], c['mem']) == (L.XP_F32, L.XP_MEM_HOST)
    assert c['nlayer'] == 4 and _same(c['layers'], K.LAYERS)
    assert sorted(res) == ['height', 'status', 'thickness'] and res['height'].shape == (9, 5) and res['height'].dtype == np.float32
    assert len(res['thickness']) == 4 and all(x.shape == (5,) and x.dtype == np.float32 for x in res['thickness'])
    assert res['status'].shape == (5,) and res['status'].dtype == np.int32
    assert c['height'] == res['height'].ctypes.data and c['status'] == res['status'].ctypes.data
    assert c['thickness'] == [x.ctypes.data for x in res['thickness']]
    # specific humidity, a base height per column, the horizontal shape kept; no layers: a NULL layer list
    p3, base = p.reshape(9, 1, 5).astype(np.float64), np.arange(5.0).reshape(1, 5)
    res = api.hydrostatic(p3, p3, specific_humidity=p3 * 1e-5, base_height=base)
    c = calls[-1]
    assert c['opts'] == (L.HUM_SPECIFIC, 0) and c['dtype'] == L.XP_F64 and c['nlayer'] == 0 and c['layers_arg'] is None
    assert np.array_equal(c['base'], np.arange(5.0)) and c['base'].dtype == np.float64
    assert res['height'].shape == (9, 1, 5) and res['thickness'] == [] and c['thickness'] == [None] * 4 and res['status'].shape == (1, 5)
    # dry, a scalar base height, want=
    res = api.hydrostatic(p, t, base_height=120.0, layers=[{'depth': 100.0}], want=('thickness',))
    c = calls[-1]
    assert c['m'] is None and np.array_equal(c['base'], np.full(5, 120.0, np.float32)) and c['height'] is None and c['status'] is None
    assert sorted(res) == ['thickness'] and c['thickness'] == [res['thickness'][0].ctypes.data, None, None, None]
    assert _same(c['layers'], [(R.PRESSURE_DEPTH, NAN, 100.0)])


def test_wrappers(calls):
    p, t, td = _cols(dtype=np.float64), _cols(dtype=np.float64) * 0.3, _cols(dtype=np.float64) * 0.29
    z = api.hydrostatic_height(p, t, td)
    c = calls[-1]
    assert z.shape == (9, 5) and c['height'] == z.ctypes.data and c['status'] is None and c['nlayer'] == 0 and c['opts'][0] == L.HUM_DEWPOINT
    z, st = api.hydrostatic_height(p, t, specific_humidity=td, base_height=3.0, status=True)
    c = calls[-1]
    assert c['status'] == st.ctypes.data and c['opts'][0] == L.HUM_SPECIFIC and np.array_equal(c['base'], np.full(5, 3.0))
    # MetPy's layer rule: bottom=None is the lowest valid level, depth=None goes to the highest valid level
    th = api.thickness_hydrostatic(p, t, td)
    c = calls[-1]
    assert th.shape == (5,) and c['thickness'][0] == th.ctypes.data and c['height'] is None and _same(c['layers'], [(R.PRESSURE, NAN, NAN)])
    api.thickness_hydrostatic(p, t, bottom=900.0, depth=400.0)
    assert _same(calls[-1]['layers'], [(R.PRESSURE_DEPTH, 900.0, 400.0)]) and calls[-1]['m'] is None
    api.thickness_hydrostatic(p, t, specific_humidity=td, bottom=900.0)
    assert _same(calls[-1]['layers'], [(R.PRESSURE, 900.0, NAN)]) and calls[-1]['opts'][0] == L.HUM_SPECIFIC
    assert 'not as mixing_ratio' in api.thickness_hydrostatic.__doc__
    # the per-point products
    phi = np.linspace(0.0, 2e5, 12).reshape(3, 4)
    for fn, name in zip((api.geopotential_to_height, api.height_to_geopotential), POINT):
        out = fn(phi)
        c = calls[-1]
        assert (c['name'], c['n'], c['dtype'], c['mem']) == (name, 12, L.XP_F64, L.XP_MEM_HOST)
        assert out.shape == (3, 4) and c['dst'].ctypes.data == out.ctypes.data and np.array_equal(c['src'], phi)
    assert fn(phi.astype(np.float32)).dtype == np.float32 and calls[-1]['dtype'] == L.XP_F32


def test_array_api_assertions(calls):
    p = _cols()
    with pytest.raises(AssertionError, match='not both'):
        api.hydrostatic(p, p, dewpoint=p, specific_humidity=p)
    for layers in ([('height', 0.0, 3000.0)], [{'bottom_height': 0.0, 'top_height': 3000.0}], [{'depth': 100.0}] * 5,
                   [{'bottom': 900.0}], [('nonsense', 1.0, 2.0)]):
        with pytest.raises(AssertionError):
            api.hydrostatic(p, p, layers=layers)
    with pytest.raises(AssertionError):
        api.hydrostatic(p, p, want=('heights',))
    with pytest.raises(AssertionError):
        api.hydrostatic(p, p[:4])
    with pytest.raises(AssertionError):
        api.hydrostatic(p, p, p[:, :3])
    with pytest.raises(AssertionError):
        api.hydrostatic(p[:4, 0], p)
    with pytest.raises(AssertionError):
        api.hydrostatic(p, p, base_height=np.ones(3))
    assert not calls


def test_one_dimensional_pressure_is_expanded(calls):
    import torch
    p1 = np.linspace(1000., 200., 9)
    t = _cols(dtype=np.float64).reshape(9, 1, 5) * 0.3
    api.hydrostatic_height(p1, t)
    c = calls[-1]
    assert (c['p'].nlev, c['p'].ncol, c['p'].lev_stride, c['p'].col_stride) == (9, 5, 5, 1)          # dense: no zero stride asked of the ABI
    got = np.ctypeslib.as_array(C.cast(c['p'].data, C.POINTER(C.c_double)), (9, 5))
    assert np.array_equal(got, p1[:, None] * np.ones((1, 5)))
    api.thickness_hydrostatic(torch.from_numpy(p1), torch.from_numpy(t))
    got = np.ctypeslib.as_array(C.cast(calls[-1]['p'].data, C.POINTER(C.c_double)), (9, 5))
    assert np.array_equal(got, p1[:, None] * np.ones((1, 5))) and calls[-1]['mem'] == L.XP_MEM_HOST


def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name)


def _names(ds):
    return list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys())


def test_mirror_wraps_the_array_api(calls):
    lev = np.arange(1., 10.)
    p, t, td = _grid(1050. - 100 * lev, 'p'), _grid(300. - 5 * lev, 't'), _grid(290. - 6 * lev, 'td')
    base = DataArray(np.arange(6.).reshape(2, 3), dims=('lat', 'lon'))
    ds = mirror.hydrostatic(p, t, td, base_height=base, layers=K.API_LAYERS[:2])
    c = calls[-1]
    assert c['name'] == ENTRY and (c['p'].nlev, c['p'].ncol, c['nlayer']) == (9, 6, 2) and np.array_equal(c['base'], np.arange(6.))
    assert _names(ds) == ['height', 'thickness', 'status']
    assert ds['height'].dims == (VD, 'lat', 'lon') and ds['height'].shape == (9, 2, 3) and ds['height'].name == 'height'
    assert ds['height'].attrs == {'long_name': 'Hydrostatic height', 'units': 'm'}
    assert np.array_equal(np.asarray(ds['height'].coords[VD]), np.arange(1, 10)) and np.array_equal(np.asarray(ds['height'].coords['lat']), [10., 20.])
    assert ds['thickness'].dims == ('hydrostatic_layer', 'lat', 'lon') and ds['thickness'].shape == (2, 2, 3) and ds['thickness'].attrs['units'] == 'm'
    assert ds['status'].dims == ('lat', 'lon')
    z = mirror.hydrostatic_height(p, t, specific_humidity=td, base_height=50.0)
    assert z.dims == (VD, 'lat', 'lon') and z.attrs['units'] == 'm' and 'long_name' in z.attrs and calls[-1]['opts'][0] == L.HUM_SPECIFIC
    assert np.array_equal(calls[-1]['base'], np.full(6, 50.0)) and calls[-1]['status'] is None
    # a pressure with the vertical dim alone is isobaric data
    p1 = DataArray(1050. - 100 * lev, dims=(VD,), name='p')
    th = mirror.thickness_hydrostatic(p1, t, bottom=900.0, depth=300.0)
    assert th.dims == ('lat', 'lon') and th.shape == (2, 3) and th.attrs['units'] == 'm' and calls[-1]['p'].ncol == 6
    assert _same(calls[-1]['layers'], [(R.PRESSURE_DEPTH, 900.0, 300.0)]) and calls[-1]['m'] is None
    phi = DataArray(np.arange(6.).reshape(2, 3) * 1e4, dims=('lat', 'lon'), coords={'lat': [10., 20.]})
    for fn, units, name in ((mirror.geopotential_to_height, 'm', POINT[0]), (mirror.height_to_geopotential, 'm$^{2}$ s$^{-2}$', POINT[1])):
        out = fn(phi)
        assert out.dims == ('lat', 'lon') and out.attrs['units'] == units and calls[-1]['name'] == name and calls[-1]['n'] == 6


# -- the restatement against closed forms ---------------------------------------------------------------------------------
P16 = np.geomspace(1000.0, 1000.0 / 9.0, 64)               # an isothermal 250 K column reaches 16 km at its top


def test_isothermal_dry_column():
    r = R.column(P16, np.full(64, 250.0))
    want = R.RD * 250.0 / R.G * np.log(P16[0] / P16)
    print('isothermal: top %.1f m, max |difference| %.3e m' % (want[-1], np.abs(r['height'] - want).max()))
    assert 16000.0 < want[-1] < 16200.0 and np.abs(r['height'] - want).max() <= 1e-9 and r['status'] == 0
    assert np.abs(R.column(P16, np.full(64, 250.0), base=812.5)['height'] - (812.5 + r['height'])).max() <= 1e-9


def test_temperature_linear_in_ln_p_makes_the_trapezoid_exact():
    x = np.log(P16)
    a, b = 288.0 - 35.0 * x[0], 35.0                         # T = a + b x: 288 K at the bottom, 211 K at the top
    r = R.column(P16, a + b * x)
    want = R.RD / R.G * (a * (x[0] - x) + 0.5 * b * (x[0] ** 2 - x ** 2))
    print('linear in ln p: top %.1f m, max |difference| %.3e m' % (want[-1], np.abs(r['height'] - want).max()))
    assert want[-1] > 16000.0 and np.abs(r['height'] - want).max() <= 1e-9


def test_thickness_between_levels_is_the_difference_of_the_heights():
    p, t, td, q, base = K.inputs(24, 300, 4)
    done = 0
    for c in range(0, 300, 7):
        ok = np.nonzero(~np.isnan(t[:, c]))[0]
        if ok.size < 4:
            continue
        lo, hi = ok[1], ok[-2]
        layers = ((R.PRESSURE, p[lo, c], p[hi, c]), (R.PRESSURE_DEPTH, p[lo, c], p[lo, c] - p[hi, c]), (R.PRESSURE, NAN, NAN))
        r = R.column(p[:, c], t[:, c], td[:, c], R.DEWPOINT, base[c], layers)
        z = R.column(p[:, c], t[:, c], td[:, c], R.DEWPOINT, 0.0)['height']
        assert r['status'] == 0 and np.all(np.abs(r['thickness'] - [z[hi] - z[lo], z[hi] - z[lo], z[ok[-1]]]) <= 1e-9), c
        done += 1
    assert done >= 35


def test_dewpoint_and_the_specific_humidity_derived_from_it_agree():
    worst = 0.0
    for name in ('12x640', '24x300'):
        p, t, td, q, base = K.inputs(*K.GRIDS[name])
        a, b = R.grid(p, t, td, R.DEWPOINT, base), R.grid(p, t, q, R.SPECIFIC, base)
        assert np.array_equal(np.isnan(a['height']), np.isnan(b['height'])) and np.array_equal(a['status'], b['status'])
        worst = max(worst, np.nanmax(np.abs(a['height'] - b['height'])))
        dry = R.grid(p, t, None, R.DRY, base)
        moister = np.nanmax(a['height'] - dry['height'])
    print('dewpoint against derived specific humidity: %.3e m; moist above dry by up to %.1f m' % (worst, moister))
    assert worst <= 1e-9 and moister > 20.0


def test_geopotential_round_trip():
    z = np.r_[0.0, np.geomspace(1.0, 8e4, 50), -300.0]
    phi = R.height_to_geopotential(z)
    back = R.geopotential_to_height(phi)
    assert np.all(np.abs(back - z) <= 1e-12 * np.maximum(np.abs(z), 1.0) * 8)
    assert np.all(phi[1:-1] < R.G * z[1:-1]) and abs(phi[1] / (R.G * z[1]) - 1.0) < 1e-6        # below g z, and g z near the ground
    assert np.isnan(R.geopotential_to_height(NAN)) and np.isnan(R.height_to_geopotential(NAN))


def test_hand_built_columns_on_the_restatement():
    p, t, td = K.hand_columns()
    r = R.grid(p, t, td, R.DRY, None, K.HAND_LAYERS)
    z, th, st = r['height'], r['thickness'], r['status']
    assert list(st) == [0, 0, R.ST_NO_LAYER, R.ST_NO_LAYER, 0, R.ST_BAD_PRESSURE, 0, 0]
    assert np.all(np.abs(z[:, 0] - R.RD * 250.0 / R.G * np.log(1000.0 / p[:, 0])) <= 1e-9)
    assert np.isnan(z[:, 2]).all() and np.isnan(th[:, 2]).all()
    assert z[4, 3] == 0.0 and np.isnan(np.delete(z[:, 3], 4)).all() and np.isnan(th[:, 3]).all()
    assert np.isnan(z[3, 4]) and np.isfinite(np.delete(z[:, 4], 3)).all() and np.array_equal(z[:3, 4], z[:3, 1])
    assert np.isfinite(z[:4, 5]).all() and np.isnan(z[4:, 5]).all() and np.isnan(th[:, 5]).all()
    # bounds on levels: thickness = the difference of the heights; close levels stand in for the bounds
    assert abs(th[0, 6] - (z[5, 6] - z[2, 6])) <= 1e-9 and abs(th[0, 7] - (z[5, 7] - z[2, 7])) <= 1e-9 and th[0, 7] != th[0, 6]
    assert abs(th[2, 1] - z[7, 1]) <= 1e-9 and np.all(th[3, [0, 1, 4, 6, 7]] > 2900.0)


# -- a census of the device tests' inputs -----------------------------------------------------------------------------------
# how many columns resolve each of K.LAYERS, from the restatement (dewpoint)
RESOLVED = {'12x640': (290, 635, 635, 635), '40x640': (292, 630, 630, 630), '7x65': (37, 64, 65, 65), '24x300': (137, 294, 294, 294),
            '1x70': (0, 0, 0, 0), '2x130': (67, 126, 126, 126)}
ALL_NAN = {'12x640': 5, '40x640': 10, '7x65': 0, '24x300': 6, '1x70': 1, '2x130': 1}


@pytest.mark.parametrize('name', sorted(K.GRIDS))
def test_input_census(name):
    """What the device tests compare, per grid: the finite share of the heights is at least 0.95 (counted: 0.965 ... 0.987);
    every column's finite heights increase strictly; no status bit is set by the heights alone except XP_ST_NO_LAYER on the
    5 / 10 / 0 / 6 / 1 / 1 all-NaN columns; the highest top of a grid with a top level lies at 20.5 ... 21.6 km (asserted: 20 ... 22
    km, where 29.3 m/K x a mean Tv of 240 ... 255 K x ln(1035 / 60) puts the 60 hPa top of synth.columns' deepest columns).  How many columns resolve each of the
    four layers is printed and pinned; on the 40x640 grid every layer is resolved in at least a quarter of the columns and
    the 1000-500 hPa layer is XP_ST_NO_LAYER in some."""
    nlev, ncol, seed = K.GRIDS[name]
    p, t, td, q, base = K.inputs(nlev, ncol, seed)
    alone, r = R.grid(p, t, td, R.DEWPOINT), R.grid(p, t, td, R.DEWPOINT, base, K.LAYERS)
    z = alone['height']
    fin = np.isfinite(z)
    empty = ~fin.any(axis=0)
    tops = z[-1, fin[-1]]
    resolved = tuple(int(x) for x in r['resolved'].sum(axis=1))
    print(name, dict(finite=round(float(fin.mean()), 4), empty=int(empty.sum()), resolved=dict(zip(K.LAYER_NAMES, resolved)),
                     tops=(float(tops.min()), float(tops.max())) if tops.size else None, base_nan=int(np.isnan(base).sum())))
    assert fin.mean() >= 0.95 and all(np.all(np.diff(z[fin[:, c], c]) > 0) for c in range(ncol))
    assert empty.sum() == ALL_NAN[name] and np.all(alone['status'][empty] == R.ST_NO_LAYER) and not alone['status'][~empty].any()
    assert nlev == 1 or 20000.0 <= tops.max() <= 22000.0
    assert np.array_equal(np.isnan(r['thickness']), ~r['resolved']) and not np.any(r['status'] & ~R.ST_NO_LAYER)
    assert np.array_equal(np.isnan(r['height']), np.isnan(z) | np.isnan(base)[None, :])             # a NaN base: that column's heights
    assert resolved == RESOLVED[name]
    if name == '40x640':
        assert min(resolved) >= ncol // 4 and resolved[0] < ncol - empty.sum() and np.isnan(base).sum() >= 5


# -- the kernel's resources -------------------------------------------------------------------------------------------------
# (VGPRs, waves / SIMD) of every instantiation (dtype, moisture kind, number of layers) as recorded in _lib.py: a change may not make
# them worse
RECORDED = {('d', 0): ((39, 8), (58, 8), (77, 6), (85, 5), (94, 5)), ('d', 1): ((45, 8), (67, 7), (84, 5), (92, 5), (101, 4)),
            ('d', 2): ((45, 8), (68, 7), (87, 5), (95, 5), (104, 4)), ('f', 0): ((38, 8), (56, 8), (75, 6), (83, 5), (92, 5)),
            ('f', 1): ((42, 8), (64, 8), (81, 5), (89, 5), (98, 4)), ('f', 2): ((44, 8), (66, 7), (85, 5), (93, 5), (102, 4))}
RECORDED = {k + (n,): v for k, row in RECORDED.items() for n, v in enumerate(row)}


@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_hydrostatic is instantiated on dtype x {dry, dewpoint, specific humidity} x the number of layers (0 ... 4): thirty
    kernels, none of which may use scratch, spill a vector register or use LDS, each no worse than recorded in VGPRs and
    occupancy."""
    unit = [x for x in L.UNITS if x[1] == 'xp_hydrostatic_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    walk = {}
    for n, r in rec.items():
        m = re.search(r'k_hydrostaticI([df])Li([012])ELi([0-4])E', n)
        if m:
            walk[(m.group(1), int(m.group(2)), int(m.group(3)))] = r
    assert sorted(walk) == sorted(RECORDED), sorted(rec)
    for key, r in sorted(walk.items()):
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['lds'] == 0 and r['vgprs'] <= RECORDED[key][0] and r['occupancy'] >= RECORDED[key][1], (key, r)
