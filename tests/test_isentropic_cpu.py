"""Isentropic interpolation without a GPU: the C ABI declarations, the array API and the DataArray module around a stubbed
launch, the NumPy restatement (tests/isentropic_restatement.py) against closed forms, a census of the inputs the device tests
run on (tests/isentropic_cases.py), and the kernel's resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import isentropic_cases as K
from tests import isentropic_restatement as R
from tests.resource_report import needs_hipcc, resources
from tests.test_abi_cpu import _KINDS, _prototypes, _struct_fields
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import isentropic as mirror
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'
NAN = float('nan')
ENTRY = 'xp_isentropic_interpolation'


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declarations_agree():
    assert _struct_fields('xp_isentropic_out') == [f[0] for f in L.IsentropicOut._fields_]
    assert _struct_fields('xp_isentropic_opts') == [f[0] for f in L.IsentropicOpts._fields_]
    assert C.sizeof(L.IsentropicOut) == 7 * 8 + 8 and C.sizeof(L.IsentropicOpts) == 16
    assert L.IsentropicOut.vars.size == 4 * 8 == L.ISEN_MAX_VARS * 8
    got = ['pointer' if t is C.c_void_p or issubclass(t, C._Pointer) else _KINDS[t] for t in L.ARGTYPES[ENTRY]]
    assert got == _prototypes()[ENTRY] == ['pointer', 'pointer', 'int32', 'pointer', 'int32'] + ['pointer'] * 4 and ENTRY in L.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'XP_ST_NOT_CONVERGED = %d\b' % L.ST_NOT_CONVERGED, hdr) and L.ST_NOT_CONVERGED == R.ST_NOT_CONVERGED == 256
    assert re.search(r'enum \{ XP_ISEN_MAX_LEVELS = %d \};' % L.ISEN_MAX_LEVELS, hdr) and L.ISEN_MAX_LEVELS == R.MAX_LEVELS == 64
    assert L.XP_ST_NO_LAYER == R.ST_NO_LAYER
    section = hdr[hdr.index('Isentropic interpolation (metpy.calc.isentropic_interpolation'):hdr.index('xp_isentropic_opts;')]
    assert 'UNPINNED' in section and 'fixed_point' in section and 'interpolate_1d' in section and 'instead of raising' in section
    assert [u for u in L.UNITS if u[1] == 'xp_isentropic_tu.hip'] == [('isentropic', 'xp_isentropic_tu.hip', [])]


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def run(self, name, *args):
        p, t, nvar, vptrs, nlevel, lev, opts, out = args
        seen.append(dict(name=name, p=p, t=t, nvar=nvar, views=[vptrs[i].contents for i in range(nvar)], nlevel=nlevel,
                         levels=[lev[i] for i in range(nlevel)], opts=(opts.from_below, opts.max_iters, opts.eps),
                         pressure=out.pressure, temperature=out.temperature, vars=list(out.vars), status=out.status,
                         dtype=out.dtype, mem=out.mem, vptrs=vptrs))
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _cols(nlev=9, ncol=5, dtype=np.float32):
    return np.ascontiguousarray(np.linspace(1000., 200., nlev, dtype=dtype)[:, None] * np.ones((1, ncol), dtype))


def test_array_api_arguments_and_defaults(calls):
    p, t, a, b = _cols(), _cols() * 0.3, _cols() + 1, _cols() + 2
    res = api.isentropic_interpolation([320.0, 300.0, 310.0], p, t, a, b, temperature_out=True, status=True)
    assert len(calls) == 1
    c = calls[0]
    assert c['name'] == ENTRY and (c['p'].nlev, c['p'].ncol, c['p'].dtype, c['p'].mem) == (9, 5, L.XP_F32, L.XP_MEM_HOST)
    assert (c['p'].data, c['t'].data) == (p.ctypes.data, t.ctypes.data) and [v.data for v in c['views']] == [a.ctypes.data, b.ctypes.data]
    assert c['levels'] == [300.0, 310.0, 320.0] and c['nlevel'] == 3 and c['nvar'] == 2             # sorted ascending
    assert c['opts'] == (1, 50, 1e-6) and (c['dtype'], c['mem']) == (L.XP_F32, L.XP_MEM_HOST)       # MetPy's defaults
    assert len(res) == 5 and all(x.shape == (3, 5) and x.dtype == np.float32 for x in res[:4])
    assert res[4].shape == (5,) and res[4].dtype == np.int32 and c['status'] == res[4].ctypes.data
    assert [c['pressure'], c['temperature']] + c['vars'] == [x.ctypes.data for x in res[:4]] + [None, None]
    # MetPy's list: the pressure alone by default; no temperature, no status, no variables
    p3 = p.reshape(9, 1, 5).astype(np.float64)
    res = api.isentropic_interpolation(np.array([300.0]), p3, p3, max_iters=7, eps=1e-9, bottom_up_search=False)
    c = calls[-1]
    assert len(res) == 1 and res[0].shape == (1, 1, 5) and res[0].dtype == np.float64 and c['pressure'] == res[0].ctypes.data
    assert c['temperature'] is None and c['vars'] == [None] * 4 and c['nvar'] == 0 and c['vptrs'] is None and c['status'] is not None
    assert c['opts'] == (0, 7, 1e-9) and c['dtype'] == L.XP_F64
    res = api.isentropic_interpolation(300.0, p, t, a)
    assert len(res) == 2 and calls[-1]['vars'][0] == res[1].ctypes.data and calls[-1]['levels'] == [300.0]


def test_array_api_assertions(calls):
    p = _cols()
    for lev, kw in (([300.0, 300.0], {}), ([], {}), ([300.0, NAN], {}), ([300.0, float('inf')], {}), ([300.0], {'max_iters': 0}),
                    ([300.0], {'eps': 0.0}), ([300.0], {'eps': -1.0}), ([300.0], {'eps': NAN})):
        with pytest.raises(AssertionError):
            api.isentropic_interpolation(lev, p, p, **kw)
    with pytest.raises(AssertionError):
        api.isentropic_interpolation([300.0], p, p[:4])
    with pytest.raises(AssertionError):
        api.isentropic_interpolation([300.0], p, p, p[:, :3])
    with pytest.raises(AssertionError):
        api.isentropic_interpolation([300.0], p[:4, 0], p)
    assert not calls


def test_more_than_64_levels_and_4_args_are_further_calls(calls):
    p = _cols(dtype=np.float64)
    lev = 300.0 + np.arange(65.0)
    extras = [p + i for i in range(5)]
    res = api.isentropic_interpolation(lev[::-1], p, p, *extras, temperature_out=True, status=True)
    assert [(c['nlevel'], c['nvar']) for c in calls] == [(64, 4), (1, 4), (64, 1), (1, 1)]
    assert calls[0]['levels'] == list(lev[:64]) and calls[1]['levels'] == [364.0] and calls[3]['levels'] == [364.0]
    P, T, V, S = res[0], res[1], res[2:7], res[7]
    assert len(res) == 8 and all(x.shape == (65, 5) for x in res[:7]) and S.shape == (5,)
    row = 64 * 5 * 8
    # the pressure, the temperature and the status come from the first calls; every call writes its slab of the level-major outputs
    assert [c['pressure'] for c in calls] == [P.ctypes.data, P.ctypes.data + row, None, None]
    assert [c['temperature'] for c in calls] == [T.ctypes.data, T.ctypes.data + row, None, None]
    assert calls[0]['status'] and calls[1]['status'] and calls[2]['status'] is None and calls[3]['status'] is None
    assert calls[0]['vars'] == [v.ctypes.data for v in V[:4]] and calls[1]['vars'] == [v.ctypes.data + row for v in V[:4]]
    assert calls[2]['vars'] == [V[4].ctypes.data, None, None, None] and calls[3]['vars'] == [V[4].ctypes.data + row, None, None, None]
    assert [v.data for v in calls[2]['views']] == [calls[3]['views'][0].data] and calls[2]['views'][0].nlev == 9
    # 64 levels and 4 args: one call
    del calls[:]
    api.isentropic_interpolation(lev[:64], p, p, *extras[:4])
    assert [(c['nlevel'], c['nvar']) for c in calls] == [(64, 4)]


def test_one_dimensional_pressure_is_expanded(calls):
    import torch
    p1 = np.linspace(1000., 200., 9)
    t = _cols(dtype=np.float64).reshape(9, 1, 5) * 0.3
    api.isentropic_interpolation([300.0], p1, t)
    c = calls[-1]
    assert (c['p'].nlev, c['p'].ncol, c['p'].lev_stride, c['p'].col_stride) == (9, 5, 5, 1)          # dense: no zero stride asked of the ABI
    got = np.ctypeslib.as_array(C.cast(c['p'].data, C.POINTER(C.c_double)), (9, 5))
    assert np.array_equal(got, p1[:, None] * np.ones((1, 5)))
    api.isentropic_interpolation([300.0], torch.from_numpy(p1), torch.from_numpy(t))
    got = np.ctypeslib.as_array(C.cast(calls[-1]['p'].data, C.POINTER(C.c_double)), (9, 5))
    assert np.array_equal(got, p1[:, None] * np.ones((1, 5))) and calls[-1]['mem'] == L.XP_MEM_HOST


def _grid(v, name):
    off = np.arange(6.).reshape(2, 3)[:, None, :] / 4
    return DataArray(v[None, :, None] + off, dims=('lat', VD, 'lon'),
                     coords={'lat': [10., 20.], 'lon': [1., 2., 3.], VD: np.arange(1, len(v) + 1)}, name=name,
                     attrs={'units': 'unit of ' + str(name)})


def _names(ds):
    return list(ds.data_vars if hasattr(ds, 'data_vars') else ds.keys())


def test_mirror_wraps_the_array_api(calls):
    lev = np.arange(1., 10.)
    p, t, q, u = _grid(1050. - 100 * lev, 'p'), _grid(300. - 5 * lev, 't'), _grid(0.01 / lev, 'q'), _grid(2 * lev, None)
    ds = mirror.isentropic_interpolation([310.0, 300.0], p, t, q, u, temperature_out=True, bottom_up_search=False, max_iters=9)
    c = calls[-1]
    assert c['name'] == ENTRY and (c['p'].nlev, c['p'].ncol, c['nvar']) == (9, 6, 2) and c['opts'] == (0, 9, 1e-6)
    assert c['levels'] == [300.0, 310.0] and c['temperature'] and c['status']
    assert _names(ds) == ['pressure', 'temperature', 'q', 'var1', 'status']
    for k in ('pressure', 'temperature', 'q', 'var1'):
        assert ds[k].dims == ('isentropic_level', 'lat', 'lon') and ds[k].shape == (2, 2, 3) and ds[k].name == k
        assert np.array_equal(np.asarray(ds[k].coords['isentropic_level']), [300.0, 310.0])
        assert np.array_equal(np.asarray(ds[k].coords['lat']), [10., 20.])
    assert ds['pressure'].attrs['units'] == 'hPa' and ds['temperature'].attrs['units'] == 'K' and ds['q'].attrs['units'] == 'unit of q'
    assert ds['status'].dims == ('lat', 'lon') and ds['status'].shape == (2, 3) and ds.attrs['isentropic_level_units'] == 'K'
    # the defaults: the pressure and the status alone; a pressure with the vertical dim alone is isobaric data
    p1 = DataArray(1050. - 100 * lev, dims=(VD,), name='p')
    ds = mirror.isentropic_interpolation([300.0], p1, t)
    assert _names(ds) == ['pressure', 'status'] and calls[-1]['opts'] == (1, 50, 1e-6) and calls[-1]['p'].ncol == 6
    assert calls[-1]['temperature'] is None and ds['pressure'].dims == ('isentropic_level', 'lat', 'lon')
    with pytest.raises(AssertionError):
        mirror.isentropic_interpolation([300.0], p, t, q, q)


# -- the restatement against closed forms ---------------------------------------------------------------------------------
def test_isothermal_column():
    p = np.array([1000.0, 850.0, 700.0, 500.0, 300.0, 200.0])
    lev = np.array([255.0, 280.0, 310.0, 350.0, 390.0, 420.0])
    for up in (True, False):
        r = R.column(p, np.full(6, 250.0), lev, from_below=up, eps=1e-12)
        want = 1000.0 * (250.0 / lev) ** (1.0 / R.KAPPA)
        assert np.all(np.abs(r['pressure'][:5] / want[:5] - 1.0) < 1e-12) and np.isnan(r['pressure'][5]) and r['status'] == R.ST_NO_LAYER
        assert np.all(np.abs(r['temperature'][:5] - 250.0) < 1e-10)


def test_dry_adiabatic_column_has_no_crossing_but_its_own_theta():
    p = np.array([1000.0, 850.0, 700.0, 500.0, 300.0])
    t = 300.0 * (p / 1000.0) ** R.KAPPA
    r = R.column(p, t, [290.0, 299.0, 301.0, 310.0])
    assert np.isnan(r['pressure']).all() and r['status'] == R.ST_NO_LAYER and all(len(x) == 0 for x in r['pairs'])
    # a target equal to its theta: the rounding of each level's theta decides which pairs flip, so only count that some may
    th = R.theta_of(np.log(p), t)
    assert np.all(np.abs(th - 300.0) < 1e-12)
    r = R.column(p, np.r_[t[:2], t[2:] * (1 + 1e-3)], [300.0 * (1 + 5e-4)])
    assert r['pair'][0] == 1 and 700.0 < r['pressure'][0] < 850.0


def _bisect(f, lo, hi):
    flo = f(lo)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if (f(mid) > 0) == (flo > 0):
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def test_newton_against_bisection_and_extras_linear_in_theta():
    p = np.array([1000.0, 800.0, 600.0, 400.0])
    x = np.log(p)
    t = np.array([290.0, 281.0, 262.0, 240.0])
    th = R.theta_of(x, t)
    lev = np.array([th[0] + 1.0, 0.5 * (th[1] + th[2]), th[3] - 0.25])
    v = 3.0 - 0.5 * th                                                         # linear in theta: comes back exactly linear
    r = R.column(p, t, lev, [v], eps=1e-13)
    for j, k in enumerate((0, 1, 2)):
        a = (t[k + 1] - t[k]) / (x[k + 1] - x[k])
        b = t[k + 1] - a * x[k + 1]
        root = _bisect(lambda y: lev[j] - (a * y + b) * np.exp(R.KAPPA * (R.LN1000 - y)), x[k], x[k + 1])
        assert r['pair'][j] == k and abs(np.log(r['pressure'][j]) - root) < 1e-13
        assert abs(r['temperature'][j] - (a * root + b)) < 1e-10
        assert abs(r['vars'][0][j] - (3.0 - 0.5 * lev[j])) < 1e-12
    assert r['status'] == 0 and r['steps'].max() <= 6
    # the default eps stops earlier and moves the pressure by less than 1e-11 relative; one step does not converge
    r6 = R.column(p, t, lev, [v])
    assert np.all(np.abs(r6['pressure'] / r['pressure'] - 1.0) < 1e-11) and np.all(r6['steps'] <= r['steps'])
    r1 = R.column(p, t, lev, [v], max_iters=1)
    assert r1['status'] == R.ST_NOT_CONVERGED and np.isnan(r1['pressure']).all() and np.isnan(r1['vars'][0]).all()


def test_hand_built_columns_on_the_restatement():
    p, t, v, lev = K.hand_columns()
    up, down = (R.grid(p, t, lev, [v], from_below=b, eps=1e-10) for b in (True, False))
    assert abs(up['pressure'][1, 0] - 800.0) < 1e-9 and up['columns'][0]['pair'][1] == 2             # theta_k <= theta* on the level
    assert [list(x) for x in up['columns'][1]['pairs']][2] == [1, 2, 3]                            # either direction counts
    assert 800.0 < up['pressure'][2, 1] < 900.0 and 500.0 < down['pressure'][2, 1] < 650.0
    assert np.array_equal(up['pressure'][:, [0, 2, 3, 4, 5, 6]], down['pressure'][:, [0, 2, 3, 4, 5, 6]], equal_nan=True)
    assert np.isnan(up['pressure'][:, [2, 3, 5]]).all() and np.all(up['status'] == R.ST_NO_LAYER)
    assert up['columns'][4]['pair'][1] == 1 and 650.0 < up['pressure'][1, 4] < 900.0                 # the NaN level is dropped
    assert np.isnan(up['vars'][0][3, 0]) and np.isfinite(up['pressure'][3, 0])                       # a NaN end of the extra alone
    assert not R.tie_column(up['columns'][6], lev) and R.tie_column(up['columns'][0], lev)


# -- a census of the device tests' inputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(K.GRIDS))
def test_input_census(name):
    """What the device tests compare is not hollowed out by their exclusions.  Per grid: at least 75 % of the targets resolve;
    on the three larger grids at least 15 columns have a first crossing that differs from the last; tie columns are at most
    1 %; the smallest |d theta| over all bracketing pairs is at least 0.05 K; Newton takes at most 10 steps at eps = 1e-6 and
    always converges.  (Counted: 8404, 8321, 859, 3906 targets resolved; 59, 169, 0, 64 columns whose theta is not monotone;
    21, 71, 0, 20 where the two crossings differ; no tie; 0.052 K; 6 steps; eps 1e-6 against 1e-13 moves a pressure by at
    most 7.8e-13 relative.)"""
    nlev, ncol, seed = K.GRIDS[name]
    p, t, td, w = K.inputs(nlev, ncol, seed)
    up, down = (R.grid(p, t, K.LEVELS, [td, w], from_below=b) for b in (True, False))
    resolved = int(np.isfinite(up['pressure']).sum())
    differ = sum(bool(np.any(a['pair'] != b['pair'])) for a, b in zip(up['columns'], down['columns']))
    nonmono = sum(bool(np.any(np.diff(c['theta']) <= 0)) for c in up['columns'])
    tie = sum(R.tie_column(c, K.LEVELS) for c in up['columns'])
    dth = min([abs(c['theta'][k + 1] - c['theta'][k]) for c in up['columns'] for pr in c['pairs'] for k in pr])
    steps = max(int(c['steps'].max()) for c in up['columns'])
    print(name, dict(resolved=resolved, differ=differ, nonmono=nonmono, tie=tie, dth=dth, steps=steps))
    assert resolved >= 0.75 * up['pressure'].size and (differ >= 15 or name == '7x65') and nonmono >= differ
    assert tie <= 0.01 * ncol and dth >= 0.05 and steps <= 10
    assert not np.any((up['status'] | down['status']) & R.ST_NOT_CONVERGED)
    # the extras: the NaNs of the second one reach its outputs, those of a dropped level do not
    assert np.array_equal(np.isfinite(up['vars'][0]), np.isfinite(up['pressure']))
    assert 0.6 * resolved <= np.isfinite(up['vars'][1]).sum() < 0.95 * resolved


# -- the kernel's resources -------------------------------------------------------------------------------------------------
# (VGPRs, waves / SIMD) of every instantiation as recorded in DESIGN.md 7: a change may not make them worse
RECORDED = {('d', 0): (52, 7), ('d', 1): (87, 5), ('f', 0): (50, 7), ('f', 1): (86, 5)}


@needs_hipcc
def test_no_instantiation_spills(tmp_path):
    """k_isentropic is instantiated on dtype x {extras or not}: four kernels, none of which may use scratch or spill a vector
    register, each with 512 B of LDS (the target list) and no worse than recorded in VGPRs and occupancy."""
    unit = [x for x in L.UNITS if x[1] == 'xp_isentropic_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    walk = {}
    for n, r in rec.items():
        m = re.search(r'k_isentropicI([df])Lb([01])E', n)
        if m:
            walk[(m.group(1), int(m.group(2)))] = r
    assert sorted(walk) == sorted(RECORDED), sorted(rec)
    for key, r in walk.items():
        print(key, r)
        assert r['in_asm'] and r['vgpr_spill'] == 0 and r['scratch'] == 0 and not r['scratch_insts'] and not r['spills'], (key, r)
        assert r['lds'] == 512 <= 1024 and r['vgprs'] <= RECORDED[key][0] and r['occupancy'] >= RECORDED[key][1], (key, r)
