"""XP_PARCEL_OVER_GROUND on the device (include/xparcel.h): with the flag a call IS the same call without it on the re-based
columns, bit for bit.  The re-based columns come from the NumPy restatement (tests/ground_restatement.py), the grids from
tests/ground_cases.py (every class of column, census in tests/test_ground_cpu.py); every output of every column is compared
with np.array_equal(..., equal_nan=True) -- no tolerance, no column left out."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ground_cases as K
from tests import ground_restatement as R
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import synth
from xarray_parcel_amd._lib import XP_E_ARG

pytestmark = pytest.mark.gpu

PARCELS = ('surface', 'most_unstable', 'mixed_layer')
MOISTS = ('exact', 'table', 'family')
DTYPES = (np.float32, np.float64)
GROUND = L.PARCEL_OVER_GROUND


@pytest.fixture(scope='module', autouse=True)
def _api():
    global xa, torch
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    xa = numpy_api
    yield


@pytest.fixture(scope='module')
def tables():
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    adiabat_tables.set_tables(tab.index, tab.adiabats)
    return tab


@functools.lru_cache(maxsize=None)
def grid(dtype, which='grid'):
    """(p, T, Td, ps, Ts, Tds) of one of the grids in `dtype`, and its re-based (p, T, Td): computed once, shared, read-only."""
    g = K.as_dtype({'grid': K.grid, 'two': K.two_level_grid, 'one': K.one_column_grid}[which](), dtype)
    rebased = R.rebase(*g)
    for a in g + rebased:
        a.flags.writeable = False
    assert all(a.dtype == dtype for a in rebased) and rebased[0].shape == (g[0].shape[0] + 1, g[0].shape[1])
    return g, rebased


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def assert_same(got, want, where=''):
    """Two results of the array API -- dicts of arrays, 'profile' a dict of its own -- equal bit for bit, NaN where NaN."""
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    for k in want:
        if isinstance(want[k], dict):
            assert_same(got[k], want[k], where + k + '.')
            continue
        a, b = _np(got[k]), _np(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (where + k, a.shape, b.shape, a.dtype, b.dtype)
        same = (a == b) | ((a != a) & (b != b))
        assert same.all(), (where + k, int((~same).sum()), np.argwhere(~same)[:5].tolist(), a[~same][:5], b[~same][:5])


def _cuda(*arrays):
    return tuple(torch.as_tensor(np.array(a)).cuda() for a in arrays)


# -- xp_cape_cin: every parcel, moist mode and dtype; all scalars, status and the six profile arrays -------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
@pytest.mark.parametrize('moist', MOISTS)
@pytest.mark.parametrize('parcel', PARCELS)
def test_cape_cin_equals_the_call_on_the_rebased_grid(parcel, moist, dtype, tables):
    (p, t, td, ps, ts, tds), rebased = grid(dtype)
    got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, want_profile=True, ground=(ps, ts, tds))
    want = xa.cape_cin_columns(*rebased, parcel=parcel, moist=moist, want_profile=True)
    assert got['profile']['pressure'].shape == (K.NLEV + 2, K.NCOL) and got['status'].dtype == np.int32
    assert_same(got, want)
    assert int((got['cape'] > 0).sum()) > K.NCOL // 8                # (the comparison is not one of NaN with NaN)


@pytest.mark.parametrize('kwargs', [dict(virtual_temperature_correction=False, lcl_interp='linear'),
                                    dict(pos_cape_neg_cin=False, post_zero_cin=True), dict(lifted_index_at=500.0, depth=60.0)],
                         ids=('no_vtc_linear', 'signs', 'lifted_index'))
def test_cape_cin_options_pass_through(kwargs):
    (p, t, td, ps, ts, tds), rebased = grid(np.float64)
    for parcel in ('surface', 'mixed_layer'):
        got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='family', ground=(ps, ts, tds), **kwargs)
        assert_same(got, xa.cape_cin_columns(*rebased, parcel=parcel, moist='family', **kwargs), parcel + ' ')


# -- xp_select_parcel and xp_cape_cin_multi ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
def test_select_parcel(dtype):
    (p, t, td, ps, ts, tds), rebased = grid(dtype)
    assert_same(xa.most_unstable_parcel(p, t, td, depth=250, ground=(ps, ts, tds)), xa.most_unstable_parcel(*rebased, depth=250))
    assert_same(xa.mixed_parcel(p, t, td, ground=(ps, ts, tds)), xa.mixed_parcel(*rebased))
    got = xa.most_unstable_parcel(p, t, td, ground=(ps, ts, tds))
    assert (got['index'] > 0).any() and (got['index'] == 0).any()      # row 0 is the surface: both it and a level above win somewhere


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
@pytest.mark.parametrize('fused', (False, True), ids=('unfused', 'fused'))
def test_multi(fused, dtype):
    (p, t, td, ps, ts, tds), rebased = grid(dtype)
    parcels = [('most_unstable', 300), ('mixed_layer', 100)]
    got = xa.cape_cin_multi(p, t, td, parcels, moist='family', fused=fused, ground=(ps, ts, tds))
    want = xa.cape_cin_multi(*rebased, parcels, moist='family', fused=fused)
    single = [xa.cape_cin_columns(*rebased, parcel=n, depth=d, moist='family') for n, d in parcels]
    for i in range(2):
        assert_same(got[i], want[i], 'parcel %d ' % i)
        assert_same(got[i], single[i], 'parcel %d (single) ' % i)


def test_multi_three_parcels_with_lifted_index(tables):
    (p, t, td, ps, ts, tds), rebased = grid(np.float32)
    parcels = ['surface', ('most_unstable', 250), ('mixed_layer', 50)]
    for moist in ('exact', 'table'):
        got = xa.cape_cin_multi(p, t, td, parcels, moist=moist, lifted_index_at=500.0, ground=(ps, ts, tds))
        want = xa.cape_cin_multi(*rebased, parcels, moist=moist, lifted_index_at=500.0)
        for i in range(3):
            assert_same(got[i], want[i], '%s parcel %d ' % (moist, i))


# -- where the arrays live and how they are laid out -------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
def test_device_tensors_and_a_stride_0_pressure(dtype):
    (p, t, td, ps, ts, tds), rebased = grid(dtype)
    dev = _cuda(p, t, td, ps, ts, tds)
    want = xa.cape_cin_columns(*rebased, parcel='most_unstable', moist='family', want_profile=True)
    got = xa.cape_cin_columns(*dev[:3], parcel='most_unstable', moist='family', want_profile=True, ground=dev[3:])
    assert all(v.is_cuda for k, v in got.items() if k != 'profile') and got['profile']['temperature'].is_cuda
    assert_same(got, want)
    # host grids with device surface fields: everything goes to the device
    host = [np.array(a) for a in (p, t, td)]
    assert_same(xa.cape_cin_columns(*host, parcel='most_unstable', moist='family', want_profile=True, ground=dev[3:]), want)
    # the nlev isobars: a device tensor is read in place through a view with col_stride 0, a host array is expanded
    iso = np.ascontiguousarray(K.ISOBARS, dtype=dtype)
    shared = R.rebase(iso, t, td, ps, ts, tds)
    for parcel in PARCELS:
        want = xa.cape_cin_columns(*shared, parcel=parcel, moist='family', want_profile=True)
        assert_same(xa.cape_cin_columns(_cuda(iso)[0], *dev[1:3], parcel=parcel, moist='family', want_profile=True, ground=dev[3:]), want)
        assert_same(xa.cape_cin_columns(iso, t, td, parcel=parcel, moist='family', want_profile=True, ground=(ps, ts, tds)), want)
    assert_same(xa.most_unstable_parcel(_cuda(iso)[0], *dev[1:3], ground=dev[3:]), xa.most_unstable_parcel(*shared))


def _raw_call(lib, views, mode, surface, scalars, dtype, ncol, moist='family', depth=100.0):
    so = L.ScalarsOut(dtype=dtype, mem=L.XP_MEM_DEVICE)
    for k, a in scalars.items():
        setattr(so, k, a.data_ptr())
    pc = L.Parcel(mode, 0, depth, *[None if x is None else x.data_ptr() for x in surface])
    o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST[moist], L.XP_F64, L.HUMIDITY['dewpoint'], 0)
    stream = torch.cuda.current_stream().cuda_stream
    return lib.xp_cape_cin(*[C.byref(v) for v in views], C.byref(pc), C.byref(o), C.byref(so), None, stream)


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
def test_every_second_column_through_the_raw_abi(dtype):
    """Strided device views: the data in the even columns of arrays twice as wide (the odd ones hold a value that would show),
    each view with strides of its own -- the pressure also as the isobars with col_stride 0."""
    (p, t, td, ps, ts, tds), _ = grid(dtype)
    lib = L.init(0)
    nlev, ncol = p.shape
    xdt = L.XP_F64 if dtype == np.float64 else L.XP_F32
    wide = []
    for a in (p, t, td):
        w = np.full((nlev, 2 * ncol), 777.0, dtype=dtype)
        w[:, ::2] = a
        wide.append(_cuda(w)[0])
    sfc = _cuda(ps, ts, tds)
    tall = _cuda(np.ascontiguousarray(np.repeat(t, 2, axis=0)))[0]           # every second ROW: a view with lev_stride 2 * ncol
    iso = _cuda(np.ascontiguousarray(K.ISOBARS, dtype=dtype))[0]
    every2 = lambda w: L.View(w.data_ptr(), xdt, L.XP_MEM_DEVICE, nlev, ncol, 2 * ncol, 2)
    layouts = {'every second column': ([every2(w) for w in wide], (p, t, td)),
               'strides of their own': ([every2(wide[0]), L.View(tall.data_ptr(), xdt, L.XP_MEM_DEVICE, nlev, ncol, 2 * ncol, 1), every2(wide[2])], (p, t, td)),
               'shared isobars': ([L.View(iso.data_ptr(), xdt, L.XP_MEM_DEVICE, nlev, ncol, 1, 0)] + [every2(w) for w in wide[1:]],
                                  (np.ascontiguousarray(K.ISOBARS, dtype=dtype), t, td))}
    names = ('cape', 'cin', 'lfc_pressure', 'el_pressure', 'lcl_pressure', 'parcel_pressure')
    for what, (views, arrays) in layouts.items():
        for parcel in ('surface', 'mixed_layer'):
            out = {k: torch.full((ncol,), -5.0, dtype=sfc[0].dtype, device='cuda') for k in names}
            out['status'] = torch.full((ncol,), -5, dtype=torch.int32, device='cuda')
            rc = _raw_call(lib, views, L.PARCEL[parcel] | GROUND, sfc, out, xdt, ncol)
            assert rc == 0, lib.xp_last_error()
            torch.cuda.synchronize()
            want = xa.cape_cin_columns(*R.rebase(*arrays, ps, ts, tds), parcel=parcel, moist='family', want=names + ('status',))
            assert_same(out, want, '%s, %s: ' % (what, parcel))


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
def test_specific_humidity_is_the_two_step_definition(dtype):
    """humidity='specific': xp_dewpoint_from_specific_humidity followed by the dewpoint-input ground call."""
    (p, t, td, ps, ts, tds), _ = grid(dtype)
    q = np.ascontiguousarray(K.specific_humidity(p.astype(np.float64), td.astype(np.float64)), dtype=dtype)
    q[3, ::50] = 0.0                                                   # no dewpoint: NaN by the conversion's own rule
    td2 = xa.dewpoint_from_specific_humidity(p, t, q)
    assert td2.dtype == dtype and np.isnan(td2[3, ::50]).all() and np.isfinite(td2).sum() > 0.8 * td2.size
    for parcel, moist in (('surface', 'family'), ('most_unstable', 'exact'), ('mixed_layer', 'family')):
        got = xa.cape_cin_columns(p, t, q, parcel=parcel, moist=moist, want_profile=True, humidity='specific', ground=(ps, ts, tds))
        assert_same(got, xa.cape_cin_columns(p, t, td2, parcel=parcel, moist=moist, want_profile=True, ground=(ps, ts, tds)), parcel + ' ')
        assert_same(got, xa.cape_cin_columns(*R.rebase(p, t, td2, ps, ts, tds), parcel=parcel, moist=moist, want_profile=True), parcel + ' ')
    got = xa.cape_cin_multi(p, t, q, ['surface', 'mixed_layer'], moist='family', fused=True, humidity='specific', ground=(ps, ts, tds))
    want = xa.cape_cin_multi(*R.rebase(p, t, td2, ps, ts, tds), ['surface', 'mixed_layer'], moist='family', fused=True)
    for i in range(2):
        assert_same(got[i], want[i])


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
def test_a_surface_equal_to_level_0_changes_nothing(dtype):
    """Invariance: with (ps, Ts, Tds) = level 0 of a full column the re-based column is the column itself (level 0 replaced by
    its equal, one NaN row on top): CAPE and CIN equal the ordinary call on the original grid bit for bit."""
    p, t, td = synth.columns(nlev=20, ncol=700, seed=5, saturate_some=True, dtype=dtype)
    names = ('cape', 'cin', 'lcl_pressure', 'parcel_index', 'parcel_pressure', 'parcel_temperature', 'parcel_dewpoint')
    for parcel in PARCELS:
        for moist in ('exact', 'family'):
            got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, want=names, ground=(p[0], t[0], td[0]))
            assert_same(got, xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, want=names), '%s %s ' % (parcel, moist))
    assert int((got['cape'] > 0).sum()) > 100


@pytest.mark.parametrize('which', ('one', 'two'))
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
def test_one_column_and_two_levels(dtype, which, tables):
    (p, t, td, ps, ts, tds), rebased = grid(dtype, which)
    for parcel in PARCELS:
        for moist in MOISTS:
            got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, want_profile=True, ground=(ps, ts, tds))
            assert got['profile']['pressure'].shape == (p.shape[0] + 2, p.shape[1])
            assert_same(got, xa.cape_cin_columns(*rebased, parcel=parcel, moist=moist, want_profile=True), '%s %s ' % (parcel, moist))


# -- what is rejected, with the outputs untouched -----------------------------------------------------------------------------
def _host_view(a, dtype=L.XP_F64):
    return L.View(a.ctypes.data, dtype, L.XP_MEM_HOST, a.shape[0], a.shape[1], a.shape[1], 1)


def test_rejections_leave_the_outputs_untouched():
    lib = L.init(0)
    (p, t, td, ps, ts, tds), _ = grid(np.float64)
    p, t, td, ps, ts, tds = (np.array(a[..., :40]) for a in (p, t, td, ps, ts, tds))
    nlev, ncol = p.shape
    views = [_host_view(a) for a in (p, t, td)]
    vref = [C.byref(v) for v in views]
    outs = {k: np.full(ncol, -5.0) for k in ('cape', 'cin', 'parcel_pressure')}
    outs['parcel_index'] = np.full(ncol, -5, dtype=np.int32)
    so = L.ScalarsOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    for k, a in outs.items():
        setattr(so, k, a.ctypes.data)
    prof = np.full((nlev + 2, ncol), -5.0)
    po = L.ProfileOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, nlev_out=nlev + 2, lev_stride=ncol, col_stride=1, temperature=prof.ctypes.data)
    sfc = (ps.ctypes.data, ts.ctypes.data, tds.ctypes.data)
    parcel = lambda mode, ptrs=sfc: L.Parcel(mode, 0, 100.0, *ptrs)
    opts = lambda **kw: L.Opts(**{**dict(virtual_temperature_correction=1, lcl_interp=1, pos_cape_neg_cin=1, post_zero_cin=0,
                                         moist_mode=L.MOIST['family'], compute=L.XP_F64, humidity=0, flags=0), **kw})

    def rejected(rc, *words):
        msg = lib.xp_last_error().decode()
        assert rc == XP_E_ARG, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert all((a == -5).all() for a in outs.values()) and (prof == -5).all()

    cape = lambda pc, o=None, profile=None: lib.xp_cape_cin(*vref, C.byref(pc), C.byref(o or opts()), C.byref(so), profile, None)
    rejected(cape(parcel(L.PARCEL['explicit'] | GROUND)), 'XP_PARCEL_OVER_GROUND', 'XP_PARCEL_EXPLICIT')
    for mode in (7, 9, 20, 32, 16 | 64, -16, GROUND << 1 | 1):
        rejected(cape(parcel(mode)), 'parcel: bad mode')
    for i in range(3):
        rejected(cape(parcel(GROUND, tuple(None if j == i else x for j, x in enumerate(sfc)))), 'XP_PARCEL_OVER_GROUND', 'surface')
    po.nlev_out = nlev + 1                                             # the re-based column has a row more
    rejected(cape(parcel(GROUND), profile=C.byref(po)), 'nlev_out')
    po.nlev_out = nlev + 2
    rejected(cape(parcel(GROUND), opts(compute=L.XP_F32)), 'XP_F32')                           # (float64 views: its first rule)
    # xp_opts.compute = XP_F32 on float32 views: mode must be exactly XP_PARCEL_SURFACE
    f32 = [np.ascontiguousarray(a, dtype=np.float32) for a in (p, t, td, ps, ts, tds)]
    v32 = [C.byref(_host_view(a, L.XP_F32)) for a in f32[:3]]
    so32 = L.ScalarsOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, cape=outs['cape'].ctypes.data)
    pc32 = L.Parcel(GROUND, 0, 100.0, *[a.ctypes.data for a in f32[3:]])
    rejected(lib.xp_cape_cin(*v32, C.byref(pc32), C.byref(opts(compute=L.XP_F32)), C.byref(so32), None, None), 'XP_F32', 'parcel->mode')
    # xp_cape_cin_multi: every parcel flagged and over the same surface arrays, or none
    sos = (L.ScalarsOut * 2)(so, so)
    multi = lambda a, b: lib.xp_cape_cin_multi(*vref, 2, (L.Parcel * 2)(a, b), C.byref(opts()), sos, None, None)
    rejected(multi(parcel(GROUND), parcel(L.PARCEL['mixed_layer'], (None, None, None))), 'XP_PARCEL_OVER_GROUND', 'every parcel')
    rejected(multi(parcel(L.PARCEL['most_unstable'], (None, None, None)), parcel(2 | GROUND)), 'XP_PARCEL_OVER_GROUND', 'every parcel')
    rejected(multi(parcel(GROUND), parcel(2 | GROUND, (sfc[0], sfc[2], sfc[1]))), 'same surface arrays')
    rejected(multi(parcel(GROUND), parcel(3 | GROUND)), 'XP_PARCEL_EXPLICIT')
    # xp_select_parcel takes the two searching parcels
    rejected(lib.xp_select_parcel(*vref, C.byref(parcel(GROUND)), C.byref(so), None), 'most-unstable or mixed-layer')
    rejected(lib.xp_select_parcel(*vref, C.byref(parcel(1 | GROUND, (sfc[0], None, sfc[2]))), C.byref(so), None), 'XP_PARCEL_OVER_GROUND')
    # the entry points whose outputs would change shape name the flag
    big = [np.full((nlev + 2, ncol), -5.0) for _ in range(3)]
    kept, n_out = np.full(nlev + 2, -5, dtype=np.int32), C.c_int64(-5)
    rejected(lib.xp_rebase_profile(*vref, C.byref(parcel(1 | GROUND)), *[a.ctypes.data for a in big], C.byref(so), kept.ctypes.data,
                                   C.byref(n_out), None), 'XP_PARCEL_OVER_GROUND', 'xp_cape_cin')
    assert all((a == -5).all() for a in big) and (kept == -5).all() and n_out.value == -5
    lo = L.CapeLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    layer = np.full(ncol, -5.0)
    lo.cape[0] = lo.total_cape = layer.ctypes.data
    top = np.full(ncol, 500.0)
    tops = (C.c_void_p * 1)(top.ctypes.data)
    rejected(lib.xp_cape_cin_layers(*vref, C.byref(parcel(GROUND)), C.byref(opts(moist_mode=L.MOIST['exact'])), 1, None, tops, C.byref(lo), None),
             'XP_PARCEL_OVER_GROUND', 'xp_cape_cin')
    assert (layer == -5).all()
    # and the same arguments with a valid mode run
    assert cape(parcel(2 | GROUND), profile=C.byref(po)) == 0, lib.xp_last_error()
    assert not (outs['cape'] == -5).any() and not (prof == -5).any() and (outs['parcel_index'] == -1).all()
    # an empty grid: nothing to re-base, nothing written
    before = {k: v.copy() for k, v in outs.items()}
    empty = [C.byref(L.View(x.ctypes.data, L.XP_F64, L.XP_MEM_HOST, nlev, 0, 0, 1)) for x in (p, t, td)]
    assert lib.xp_cape_cin(*empty, C.byref(parcel(GROUND)), C.byref(opts()), C.byref(so), None, None) == 0, lib.xp_last_error()
    assert all(np.array_equal(outs[k], before[k], equal_nan=True) for k in outs)


def test_dataarray_module_on_the_device(tables):
    """xarray_parcel_amd/ground.py end to end: Datasets on the horizontal dims, the isobars as a 1-D DataArray."""
    from xarray_parcel_amd import ground
    from xarray_parcel_amd._xr import DataArray
    (p, t, td, ps, ts, tds), _ = grid(np.float32)
    ny, nx = 7, 191                                                    # 1337 = 7 x 191
    hc = {'y': np.arange(ny), 'x': np.arange(nx)}
    lev = lambda a: DataArray(a.reshape(K.NLEV, ny, nx).transpose(1, 0, 2), dims=('y', 'lev', 'x'), coords={**hc, 'lev': np.arange(K.NLEV)})
    sfc = [DataArray(a.reshape(ny, nx), dims=('y', 'x'), coords=hc) for a in (ps, ts, tds)]
    iso = DataArray(K.ISOBARS.astype(np.float32), dims=('lev',))
    shared = R.rebase(K.ISOBARS.astype(np.float32), t, td, ps, ts, tds)
    k0 = R.levels_below_ground(K.ISOBARS, ps).reshape(ny, nx)
    for fn, parcel, moist in ((ground.surface_based_cape_cin, 'surface', 'family'), (ground.most_unstable_cape_cin, 'most_unstable', 'table'),
                              (ground.mixed_layer_cape_cin, 'mixed_layer', 'exact')):
        ds = fn(iso, lev(t), lev(td), *sfc, vert_dim='lev', moist=moist)
        want = xa.cape_cin_columns(*shared, parcel=parcel, moist=moist)
        assert set(ds.keys()) == set(want) | {'levels_below_ground'}
        for k, v in want.items():
            assert ds[k].dims == ('y', 'x') and np.array_equal(np.asarray(ds[k].values), v.reshape(ny, nx), equal_nan=True), (parcel, k)
        assert np.array_equal(np.asarray(ds['levels_below_ground'].values), k0)
    ds = ground.cape_cin_multi(lev(p), lev(t), lev(td), *sfc, parcels=['surface', ('mixed_layer', 50)], vert_dim='lev', moist='family', want=('cape', 'cin'))
    _, rebased = grid(np.float32)
    for i, (parcel, depth) in enumerate((('surface', None), ('mixed_layer', 50))):
        want = xa.cape_cin_columns(*rebased, parcel=parcel, depth=depth, moist='family', want=('cape', 'cin'))
        for k in ('cape', 'cin'):
            assert np.array_equal(np.asarray(ds['%s_%d' % (k, i)].values), want[k].reshape(ny, nx), equal_nan=True), (parcel, k)
    assert np.array_equal(np.asarray(ds['levels_below_ground'].values), R.levels_below_ground(p, ps).reshape(ny, nx))
