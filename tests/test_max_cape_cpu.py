"""XP_PARCEL_MAX_CAPE without a GPU: the enumerator in the header and the binding, the array API and the DataArray module
around a stubbed launch, the NumPy restatement (tests/max_cape_restatement.py) on the hand-built columns, a census of the
grids the device tests run on (tests/max_cape_cases.py), and the kernels' resources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import max_cape_cases as K
from tests import max_cape_restatement as R
from tests.resource_report import needs_hipcc, resources
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import max_cape as mirror
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd._xr import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VD = 'model_level_number'
MODE = 4


# -- C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_enumerator():
    hdr = open(os.path.join(ROOT, 'include', 'xparcel.h')).read()
    assert re.search(r'enum \{ XP_PARCEL_MAX_CAPE = %d \};' % L.PARCEL['max_cape'], hdr) and L.PARCEL['max_cape'] == MODE
    assert L.PARCEL == {'surface': 0, 'most_unstable': 1, 'mixed_layer': 2, 'explicit': 3, 'max_cape': 4}
    assert L.PARCEL['max_cape'] & L.PARCEL_OVER_GROUND == 0
    section = hdr[hdr.index('XP_PARCEL_MAX_CAPE, a fifth parcel kind'):hdr.index('enum { XP_PARCEL_MAX_CAPE')]
    for rule in ('p >= p0 - depth', 'p[k:], T[k:], Td[k:]', 'FOR THE SELECTION ONLY', 'no early stop', 'CAPE_k > best',
                 'a NaN CAPE_k never wins', 'k* = 0', 'row j = level k* + j', 'bit for bit', 'parcel_index = k*',
                 'nlev_out >= nlev + 1', 'XP_HUM_SPECIFIC', 'XP_PARCEL_OVER_GROUND', 'one ascent per candidate and column',
                 'three (nlev, ncol) scratch arrays'):
        assert rule in section, rule
    assert C.sizeof(L.Parcel) == 40 and C.sizeof(L.ScalarsOut) == 16 * 8 + 8        # no struct changes layout


def test_no_new_entry_point_and_a_unit_of_its_own():
    assert len(L.SYMBOLS) == 56 and len(set(L.SYMBOLS)) == 56 and not [s for s in L.SYMBOLS if 'max_cape' in s]
    assert set(L.SYMBOLS) == set(L.ARGTYPES)
    assert [u for u in L.UNITS if u[1] == 'xp_max_cape_tu.hip'] == [('max_cape', 'xp_max_cape_tu.hip', L.EFFECTIVE_FLAGS)]
    assert L.EFFECTIVE_FLAGS == ['-mllvm', '-disable-machine-licm']
    src = lambda f: open(os.path.join(L.SRC_DIR, f)).read()
    assert 'k_max_cape_select' not in src('xp_effective_tu.hip') and 'k_max_cape_select' not in src('xp_effective.hpp')
    assert 'lift_candidate<T, TABLE>(a.e,' in src('xp_max_cape.hpp')                # the inflow kernel's lifter, unchanged
    L.build()
    lib = L.load()
    assert all(hasattr(lib, s) for s in L.SYMBOLS)


# -- the array API and the DataArray module around a stubbed launch ---------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def run(self, name, *args):
        views, rest = args[:3], args[3:]
        rec = dict(name=name, call=self, views=[(v.data, v.dtype, v.mem, v.nlev, v.ncol, v.lev_stride, v.col_stride) for v in views])
        if name == 'xp_cape_cin_multi':
            n, pcs, opts, sos, pos = rest
            rec.update(parcels=[bytes(pcs[i]) for i in range(n)], opts=bytes(opts))
        else:
            po = rest[3] if name == 'xp_cape_cin' else None
            rec.update(parcels=[bytes(rest[0])], opts=bytes(rest[1]) if name == 'xp_cape_cin' else None,
                       nlev_out=None if po is None else po.nlev_out)
        seen.append(rec)
    monkeypatch.setattr(api._Call, 'run', run)
    return seen


def _parcel(mode, depth):
    return bytes(L.Parcel(mode, 0, depth, None, None, None))


def _small(dtype=np.float32, ncol=6):
    return tuple(np.ascontiguousarray(a[:, :ncol], dtype=dtype) for a in K.grid())


def test_array_api_passes_the_mode_and_the_depth(calls):
    p, t, td = _small()
    res = api.cape_cin_columns(p, t, td, parcel='max_cape', want_profile=True)
    c = calls[-1]
    assert c['name'] == 'xp_cape_cin' and c['parcels'] == [_parcel(MODE, 300.0)] and c['nlev_out'] == 24 + 1
    assert c['views'] == [(a.ctypes.data, L.XP_F32, L.XP_MEM_HOST, 24, 6, 6, 1) for a in (p, t, td)]
    assert c['opts'] == bytes(api._opts()) and res['profile']['pressure'].shape == (25, 6) and res['parcel_index'].dtype == np.int32
    api.cape_cin_columns(p, t, td, parcel='max_cape', depth=150, moist='family', post_zero_cin=True)
    c = calls[-1]
    assert c['parcels'] == [_parcel(MODE, 150.0)] and c['opts'] == bytes(api._opts(moist='family', post_zero_cin=True))
    # the other kinds are what they were
    api.cape_cin_columns(p, t, td, parcel='most_unstable')
    assert calls[-1]['parcels'] == [_parcel(1, 300.0)]
    api.cape_cin_columns(p, t, td, parcel='mixed_layer')
    assert calls[-1]['parcels'] == [_parcel(2, 100.0)]
    # the several-parcels call, in any mix
    outs = api.cape_cin_multi(p, t, td, ['surface', ('max_cape', 200), 'max_cape', ('most_unstable', 300)], fused=True)
    c = calls[-1]
    assert c['name'] == 'xp_cape_cin_multi' and len(outs) == 4
    assert c['parcels'] == [_parcel(0, 100.0), _parcel(MODE, 200.0), _parcel(MODE, 300.0), _parcel(1, 300.0)]
    assert C.cast(c['opts'], C.POINTER(L.Opts)).contents.flags == L.OPT_FUSE_PARCELS
    with pytest.raises(AssertionError, match='parcels: surface, most_unstable or mixed_layer'):
        api.cape_cin_multi(p, t, td, ['explicit'])
    # the selector and the reference-style pair
    r = api.max_cape_parcel(p, t, td)
    assert calls[-1]['name'] == 'xp_select_parcel' and calls[-1]['parcels'] == [_parcel(MODE, 300.0)]
    assert sorted(r) == ['dewpoint', 'index', 'pressure', 'temperature'] and r['index'].dtype == np.int32 and r['pressure'].shape == (6,)
    api.max_cape_parcel(p, t, td, depth=120)
    assert calls[-1]['parcels'] == [_parcel(MODE, 120.0)]
    cc, prof, pc = api.max_cape_cape_cin(p, t, td, depth=250, moist='table')
    c = calls[-1]
    assert c['name'] == 'xp_cape_cin' and c['parcels'] == [_parcel(MODE, 250.0)] and c['nlev_out'] == 25
    assert sorted(cc) == ['cape', 'cin'] and sorted(pc) == ['dewpoint', 'index', 'pressure', 'temperature'] and 'lfc_pressure' in prof
    mu = api.most_unstable_cape_cin(p, t, td)
    assert [sorted(x) for x in mu] == [sorted(x) for x in (cc, prof, pc)]
    # what it does not combine with
    sfc = tuple(a[0] for a in (p, t, td))
    with pytest.raises(AssertionError, match='max_cape'):
        api.cape_cin_columns(p, t, td, parcel='max_cape', ground=sfc)
    with pytest.raises(AssertionError, match='max_cape'):
        api.cape_cin_multi(p, t, td, ['surface', 'max_cape'], ground=sfc)
    # a set_compute('float32') preference leaves the call in fp64
    api.set_compute('float32')
    try:
        api.cape_cin_columns(p, t, td, parcel='max_cape', moist='family')
        assert C.cast(calls[-1]['opts'], C.POINTER(L.Opts)).contents.compute == L.XP_F64
    finally:
        api.set_compute('float64')


def test_dataarray_module(calls):
    p, t, td = _small(np.float64)
    hc = {'lat': [10.0, 20.0], 'lon': [1.0, 2.0, 3.0]}
    on_grid = lambda a: DataArray(a.reshape(24, 2, 3).transpose(1, 0, 2), dims=('lat', VD, 'lon'), coords={**hc, VD: np.arange(24)})
    ds = mirror.max_cape_cape_cin(on_grid(p), on_grid(t), on_grid(td), moist='family')
    c = calls[-1]
    assert c['name'] == 'xp_cape_cin' and c['parcels'] == [_parcel(MODE, 300.0)] and c['nlev_out'] is None          # no profile
    assert c['views'][0][1:] == (L.XP_F64, L.XP_MEM_HOST, 24, 6, 6, 1)
    assert set(ds.keys()) == set(L.SCALAR_F + L.SCALAR_I + L.SCALAR_P)
    assert ds['cape'].dims == ('lat', 'lon') and ds['cape'].shape == (2, 3) and ds['cape'].attrs['units'] == 'J kg$^{-1}$'
    assert ds['parcel_index'].values.dtype == np.int32 and 'largest CAPE' in ds['parcel_index'].attrs['long_name']
    ds = mirror.max_cape_cape_cin(on_grid(p), on_grid(t), on_grid(td), depth=200, want=('cape', 'cin'))
    assert calls[-1]['parcels'] == [_parcel(MODE, 200.0)] and set(ds.keys()) == {'cape', 'cin'}
    ds = mirror.max_cape_parcel(on_grid(p), on_grid(t), on_grid(td), depth=180)
    c = calls[-1]
    assert c['name'] == 'xp_select_parcel' and c['parcels'] == [_parcel(MODE, 180.0)]
    assert set(ds.keys()) == {'parcel_pressure', 'parcel_temperature', 'parcel_dewpoint', 'parcel_index'}
    assert ds['parcel_pressure'].dims == ('lat', 'lon') and ds['parcel_pressure'].attrs['units'] == 'hPa'


def test_parcel_functions_gains_nothing():
    from xarray_parcel_amd import parcel_functions as pf
    for name in ('max_cape_cape_cin', 'max_cape_parcel'):
        assert not hasattr(pf, name)


# -- the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_on_the_hand_built_columns():
    cols = K.hand_built()
    assert set(cols) == set(K.HAND) == set(K.HAND_KSTAR)
    got = {}
    for name in K.HAND:
        p, t, td = (a[:, None] for a in cols[name])
        r = got[name] = R.max_cape_grid(p, t, td, depth=K.HAND_DEPTH.get(name, K.DEPTH))
        print(name, r['kstar'][0], np.round(r['candidate_cape'][:8, 0], 1))
        assert r['kstar'][0] == K.HAND_KSTAR[name], name
        k = int(r['kstar'][0])
        for a, b in zip((p, t, td), (r['pressure'], r['temperature'], r['dewpoint'])):
            assert b.shape == a.shape and np.array_equal(b[:20 - k, 0], a[k:, 0], equal_nan=True) and np.all(np.isnan(b[20 - k:, 0]))
    cape = lambda name: got[name]['candidate_cape'][:, 0]
    lifted = lambda name: np.nonzero(got[name]['candidates'][:, 0])[0].tolist()
    assert lifted('best_0') == list(range(7)) and cape('best_0')[0] > 1000.0 and np.all(cape('best_0')[1:7] == 0.0)
    assert cape('best_aloft')[3] > 1000.0 and np.all(cape('best_aloft')[:3] == 0.0)          # the cold pool has none
    assert lifted('all_zero') == list(range(7)) and np.all(cape('all_zero')[:7] == 0.0)       # every CAPE 0: the surface parcel
    assert lifted('nan_inside') == [0, 1, 3, 4, 5, 6] and np.isnan(cape('nan_inside')[2])
    assert lifted('all_nan') == [] and not got['all_nan']['tie'][0]
    assert lifted('level0_invalid') == list(range(1, 8))                                      # p0 = level 1's pressure: 955 - 300 hPa
    assert lifted('one_level_window') == [0]
    assert lifted('whole_column') == list(range(20))
    # candidate k IS the surface parcel of the column cut off below k
    p, t, td = cols['best_aloft']
    one = co.cape_cin_grid(p[3:, None], t[3:, None], td[3:, None], parcel='surface', moist='rk4')
    assert cape('best_aloft')[3] == one['cape'][0]
    # the selection rule by itself: the lowest of equal maxima, a NaN never replaces the holder, no candidate: 0
    cand = np.array([[0, 1, 1, 1, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 0], [1, 0, 1, 1, 0]], dtype=bool)
    c = np.array([[9., 5., 0., 1., 9.], [2., 7., 0., np.nan, 9.], [3., 7., 0., 1., 9.], [3., 9., 0., 2., 9.]])
    assert R.choose(cand, c).tolist() == [2, 1, 0, 3, 0]
    assert R.tie_class(cand, c).tolist() == [True, True, False, False, False]


# -- census of the device tests' inputs ------------------------------------------------------------------------------------
def _census(name):
    p, t, td = K.grid(name)
    r = K.restated(name)
    ks, cand, cc = r['kstar'], r['candidates'], r['candidate_cape']
    has = cand.any(axis=0)
    best = np.where(has, np.where(cand, cc, -np.inf).max(axis=0), 0.0)
    mu = co.cape_cin_grid(p, t, td, parcel='most_unstable', depth=K.DEPTH, moist='rk4')
    values, counts = np.unique(ks, return_counts=True)
    out = dict(ncol=p.shape[1], aloft=int(((ks > 0) & (best > 0)).sum()), distinct=int((counts >= 5).sum()),
               mu_differs=int(((mu['parcel_index'] != ks) & (np.abs(best - mu['cape']) > 1.0)).sum()),
               no_candidate=int((~has).sum()), tie=int(r['tie'].sum()))
    print(name, out)
    return out


def test_census_of_the_main_grid():
    """Counted with the C oracle (RK4) at depth 300 hPa on '24x1337': the best departure level lies above the lowest valid
    level, with CAPE > 0, in 689 columns (52 %); ten k* values are held by at least 5 columns each (k* = 0 ... 9: 644, 129,
    122, 79, 136, 125, 51, 22, 15, 14); the oracle's most-unstable parcel_index differs from k* with a CAPE gap above 1 J/kg
    in 15 columns (up to 114 J/kg); 7 columns have no candidate; no column is in the tie class."""
    p, t, td = K.grid()
    assert p.shape == K.GRIDS[K.MAIN] == (24, 1337)
    for a in K.grid():
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64), equal_nan=True)          # exact in float32
    c = _census(K.MAIN)
    assert 4 * c['aloft'] >= c['ncol']
    assert c['distinct'] >= 6
    assert c['mu_differs'] >= 10
    assert c['no_candidate'] >= 1
    assert 100 * c['tie'] <= c['ncol']


def test_census_of_the_other_grids():
    """'40x640': 375 columns aloft with CAPE > 0, 15 where the most-unstable parcel differs by more than 1 J/kg (up to 124).
    The small grids are there for their shapes: fewer levels than the unrolled copy takes at once, a window that ends at the
    column's top, one level."""
    c = _census('40x640')
    assert 4 * c['aloft'] >= c['ncol'] and c['mu_differs'] >= 10 and 100 * c['tie'] <= c['ncol']
    for name in ('7x65', '2x130', '1x70'):
        c = _census(name)
        assert K.grid(name)[0].shape == K.GRIDS[name] and 100 * c['tie'] <= c['ncol']
    assert _census('7x65')['aloft'] >= 5 and _census('1x70')['no_candidate'] >= 1


# -- kernel resources --------------------------------------------------------------------------------------------------------
# VGPRs, waves per SIMD as recorded in _lib.py at EFFECTIVE_FLAGS, by mangled-name fragment
RECORDED = {'k_max_cape_selectIdLb0E': (108, 4), 'k_max_cape_selectIdLb1E': (112, 4), 'k_max_cape_selectIfLb0E': (105, 4),
            'k_max_cape_selectIfLb1E': (110, 4), 'k_rebase_fromIdE': (43, 8), 'k_rebase_fromIfE': (40, 8)}


@needs_hipcc
def test_kernels_keep_four_waves_per_simd_without_spills(tmp_path):
    """Every instantiation -- the selection for f64 / f32 x RK4 / lookup tables and the two copies -- compiled as the library
    compiles it (its own unit, that unit's flags): no scratch (ScratchSize 0, no scratch instruction in the body, no VGPR
    spilled), at most 128 VGPRs, at most 40 KB of LDS -- the bounds k_effective_inflow is held to -- and the pairs recorded in
    _lib.py.  Neither kernel lives in xparcel.hip or in the inflow kernel's unit."""
    unit = [u for u in L.UNITS if u[1] == 'xp_max_cape_tu.hip']
    assert len(unit) == 1
    rec = resources(tmp_path, unit[0][1], unit[0][2])
    kernels = {f: [n for n in rec if f in n] for f in RECORDED}
    assert all(len(v) == 1 for v in kernels.values()), sorted(rec)
    assert len([n for n in rec if 'k_max_cape_select' in n or 'k_rebase_from' in n]) == len(RECORDED)
    for frag, (name,) in kernels.items():
        r = rec[name]
        print(name, r)
        assert r['in_asm'] and not r['scratch_insts'] and r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r)
        assert r['vgprs'] <= 128 and r['occupancy'] >= 4 and r['lds'] <= 40 * 1024, (name, r)
        assert (r['vgprs'], r['occupancy']) == RECORDED[frag], (name, r)
    copies = [kernels[f][0] for f in RECORDED if 'rebase' in f]
    assert all(rec[n]['lds'] == 0 and rec[n]['occupancy'] == 8 for n in copies)
    src = open(os.path.join(L.SRC_DIR, 'xparcel.hip')).read()
    assert 'k_max_cape_select' not in src and 'k_rebase_from' not in src
