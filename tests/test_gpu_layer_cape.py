"""CAPE / CIN over per-column layers on the device (xp_cape_cin_layers) against the NumPy restatement
tests/layer_cape_restatement.py, against xp_cape_cin itself, and its own interface and argument checks.

Tolerance against the restatement: 1e-6 J/kg (plus one float32 spacing for float32 outputs) -- what tests/test_gpu_parity.py
holds xp_cape_cin to against the same oracle; the layer arithmetic adds about ten fp64 operations on sums below 1e3.
Columns that test_gpu_parity._saturated_tie_columns classifies as saturated-parcel sign ties are left out, under that
function's own bounds; nothing else is."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import layer_cape_restatement as R
from tests.test_gpu_dcape import inputs
from tests.test_gpu_parity import _saturated_tie_columns
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu
NLEV, NCOL = 40, 3000
ORACLE_MOIST = {'exact': 'rk4', 'table': 'table'}
PARCELS = ('surface', 'explicit', 'most_unstable', 'mixed_layer')
WHOLE = ('cape', 'cin', 'lfc_pressure', 'el_pressure', 'lcl_pressure', 'status')       # cape_cin_columns' names of the totals
TOTAL_OF = {'cape': 'total_cape', 'cin': 'total_cin'}


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def heights(p):
    return 44330.8 * (1.0 - (p / 1013.25) ** 0.190263)


@pytest.fixture(scope='module')
def oracle_tables():
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    co.set_tables(tab)
    adiabat_tables.set_tables(tab.index, tab.adiabats)       # both sides look up the SAME arrays
    return tab


@functools.lru_cache(maxsize=None)
def grid(dtype):
    return inputs(NLEV, NCOL, seed=11, dtype=dtype)


def parcel_kw(parcel, p, t, td):
    """The explicit parcel: the surface level, a kelvin warmer and half a kelvin drier."""
    if parcel != 'explicit':
        return {}
    return {'parcel_values': (p[0].copy(), t[0] + p.dtype.type(1.0), td[0] - p.dtype.type(0.5))}


@functools.lru_cache(maxsize=None)
def whole(parcel, moist, dtype):
    """xp_cape_cin's own all-outputs result for the grid."""
    p, t, td = grid(dtype)
    return xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, **parcel_kw(parcel, p, t, td))


def mixed_layers(parcel, moist, dtype):
    """Four layers per column that mix: plain pressure bounds; bounds exactly on level pressures (every column); no bottom and
    the top on the LCL pressure, or the layer wholly below the LFC, or wholly above the EL; and NaN, inverted and
    out-of-column bounds (every sixth column each: 500 of 3000), an ordinary layer elsewhere."""
    p, t, td = grid(dtype)
    w = whole(parcel, moist, dtype)
    rng = np.random.default_rng(5)
    cols = np.arange(NCOL)
    nan = np.nan
    b0 = rng.uniform(600.0, 1000.0, NCOL)
    t0 = b0 - rng.uniform(50.0, 400.0, NCOL)
    k1 = rng.integers(0, NLEV // 2, NCOL)
    k2 = k1 + rng.integers(1, NLEV // 2, NCOL)
    b1, t1 = p[k1, cols].astype(np.float64), p[k2, cols].astype(np.float64)                # NaN levels: no bottom / no layer
    lcl, lfc, el = (np.asarray(w[k], dtype=np.float64) for k in ('lcl_pressure', 'lfc_pressure', 'el_pressure'))
    kind = cols % 3
    b2 = np.where(kind == 0, nan, np.where(kind == 1, lfc + 60.0, el - 5.0))
    t2 = np.where(kind == 0, lcl, np.where(kind == 1, lfc + 5.0, el - 80.0))                # a NaN LFC / EL: no layer there
    edge = cols % 6
    b3 = np.select([edge == 0, edge == 1, edge == 2, edge == 3], [800.0, 500.0, 1150.0, 8.0], rng.uniform(700.0, 950.0, NCOL))
    t3 = np.select([edge == 0, edge == 1, edge == 2, edge == 3, edge == 4], [nan, 650.0, 1e-3, 5.0, 1100.0], rng.uniform(150.0, 600.0, NCOL))
    b3 = np.where(edge == 4, 1200.0, b3)
    cast = lambda a: a.astype(dtype)
    return [cast(b0), cast(b1), cast(b2), cast(b3)], [cast(t0), cast(t1), cast(t2), cast(t3)]


@functools.lru_cache(maxsize=None)
def restated(parcel, moist, dtype):
    p, t, td = grid(dtype)
    bottoms, tops = mixed_layers(parcel, moist, dtype)
    kw = parcel_kw(parcel, p, t, td)
    if kw:
        kw = {'parcel_values': np.stack(kw['parcel_values'])}
    return R.layers_grid(p, t, td, bottoms, tops, parcel=parcel, moist=ORACLE_MOIST[moist], **kw)


def compare(got, ref, whole_got, dtype, tag, n_layer_min=None):
    """got against the restatement `ref`; whole_got: cape_cin_columns' result for the same columns (the tie classification)."""
    _, excluded = _saturated_tie_columns(whole_got, ref['oracle'])
    keep = ~excluded
    f32 = dtype == np.float32
    # the status bits the oracle has (TOP_NAN, LCL_NOT_CONVERGED) and NO_LAYER; NAN_PRESSURE / BAD_PRESSURE are the library's own
    # (the oracle never sets them): test_totals_are_xp_cape_cin_bit_for_bit holds the whole word to xp_cape_cin's
    st = _np(got['status']) & (L.ST_TOP_NAN | L.ST_LCL_NOT_CONVERGED | L.XP_ST_NO_LAYER)
    bad = np.nonzero((st != ref['status']) & keep)[0]
    assert bad.size == 0, (tag, 'status', bad[:8], _np(got['status'])[bad[:8]], ref['status'][bad[:8]])
    worst = {}
    for k in ('cape', 'cin') + R.TOTALS:
        g, r = _np(got[k]).astype(np.float64)[..., keep], ref[k][..., keep]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k, np.argwhere(np.isnan(g) != np.isnan(r))[:5])
        ok = ~np.isnan(r)
        tol = np.full(ok.sum(), 1e-6)
        if f32:
            tol = tol + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        err = np.abs(g[ok] - r[ok])
        worst[k] = float(err.max()) if err.size else 0.0
        print('%s %s: max |error| %.3e over %d values' % (tag, k, worst[k], err.size))
        assert np.all(err <= tol), (tag, k, worst[k], np.argwhere(ok)[np.argmax(err - tol)])
    return keep


# -- 1. against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('parcel,moist', [(pc, 'exact') for pc in PARCELS] + [('surface', 'table'), ('most_unstable', 'table')])
def test_mixed_layers_vs_restatement(parcel, moist, dtype, oracle_tables):
    p, t, td = grid(dtype)
    bottoms, tops = mixed_layers(parcel, moist, dtype)
    layers = [{'bottom': b, 'top': tp} for b, tp in zip(bottoms, tops)]
    got = xa.cape_cin_layers(p, t, td, layers, parcel=parcel, moist=moist, **parcel_kw(parcel, p, t, td))
    ref = restated(parcel, moist, dtype)
    assert got['cape'].dtype == dtype and got['cape'].shape == (4, NCOL)
    keep = compare(got, ref, whole(parcel, moist, dtype), dtype, '%s %s %s' % (parcel, moist, np.dtype(dtype).name))
    # what the layers were built to hit
    cape, cin = ref['cape'], ref['cin']
    lev_p = np.asarray(p, dtype=np.float64)
    on_level = [(np.asarray(b, dtype=np.float64)[None] == lev_p).any(axis=0) for b in (bottoms[1], tops[1])]
    assert (on_level[0] & on_level[1] & np.isfinite(cape[1])).sum() >= 300
    edge = np.arange(NCOL) % 6
    assert np.isnan(cape[3][edge == 0]).all() and np.isnan(cape[3][edge == 1]).all() and np.isnan(cin[3][edge == 1]).all()
    assert ((ref['status'] & R.ST_NO_LAYER) != 0)[edge <= 1].all()
    live = ~np.isnan(ref['lcl_pressure'])
    assert np.array_equal(cape[3][(edge == 2) & live], ref['total_cape'][(edge == 2) & live])         # beyond both ends: the whole ascent
    assert (cape[3][edge == 3] == 0.0).all() and (cape[3][edge == 4] == 0.0).all() and (cin[3][edge == 4] == 0.0).all()
    kind = np.arange(NCOL) % 3
    below = (kind == 1) & np.isfinite(cape[2]) & keep                  # (a tie column's LFC / EL is not the one the bounds were built on)
    above = (kind == 2) & np.isfinite(cape[2]) & keep
    assert below.sum() >= 50 and (cape[2][below] == 0.0).all() and (cin[2][below] < 0.0).sum() >= 25
    assert above.sum() >= 50 and (cape[2][above] == 0.0).all() and (cin[2][above] == 0.0).all()
    assert (np.isfinite(cape[2]) & (kind == 0)).sum() >= 800                                          # the top on the LCL
    some = (np.nan_to_num(_np(got['cape']).astype(np.float64)) != 0.0).any(axis=0)
    assert some.sum() >= NCOL // 2, some.sum()


# -- 2. against the library itself ----------------------------------------------------------------------------------------------
def abutting(p, dtype):
    """first node -> p1 -> p2 -> top, per column, and the whole ascent as layer 0."""
    rng = np.random.default_rng(9)
    p1 = rng.uniform(650.0, 950.0, p.shape[1]).astype(dtype)
    p2 = (p1 - rng.uniform(40.0, 400.0, p.shape[1])).astype(dtype)
    return [{'top': 1e-3}, {'top': p1}, {'bottom': p1, 'top': p2}, {'bottom': p2, 'top': 1e-3}]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('moist', ['exact', 'table'])
@pytest.mark.parametrize('parcel', PARCELS)
def test_totals_are_xp_cape_cin_bit_for_bit(parcel, moist, dtype, oracle_tables):
    """total_cape, total_cin, the LFC / EL / LCL pressures and the status ARE xp_cape_cin's; a layer without a bottom and a
    top above the column reproduces the totals bit for bit; three abutting layers sum to them."""
    p, t, td = grid(dtype)
    want = whole(parcel, moist, dtype)
    got = xa.cape_cin_layers(p, t, td, abutting(p, dtype), parcel=parcel, moist=moist, **parcel_kw(parcel, p, t, td))
    for k in WHOLE:
        g, w = got[TOTAL_OF.get(k, k)], want[k]
        diff = ~((g == w) | (np.isnan(g) & np.isnan(w))) if k != 'status' else g != w
        print('%s %s %s %s: %d of %d differ' % (parcel, moist, np.dtype(dtype).name, k, diff.sum(), diff.size))
        assert not diff.any(), (k, np.nonzero(diff)[0][:5], g[diff][:5], w[diff][:5])
    assert np.array_equal(got['cape'][0], got['total_cape']) and np.array_equal(got['cin'][0], got['total_cin'])
    if dtype == np.float64:                  # (float32 outputs are each rounded to 6e-8 relative: 1e-9 of the total says nothing there)
        for k in ('cape', 'cin'):
            tot = got['total_' + k]
            err = np.abs(got[k][1:].sum(axis=0) - tot)
            print('%s %s %s: abutting layers off by at most %.3e' % (parcel, moist, k, err.max()))
            assert np.all(err <= 1e-9 * np.maximum(1.0, np.abs(tot))), (k, err.max())
    assert (got['total_cape'] > 0).sum() >= NCOL // 4 and not np.isnan(got['cape']).any()


# -- 3. the interface -----------------------------------------------------------------------------------------------------------
def test_family_mode_runs_as_exact():
    p, t, td = grid(np.float64)
    layers = abutting(p, np.float64)
    a = xa.cape_cin_layers(p, t, td, layers, parcel='most_unstable', moist='exact')
    b = xa.cape_cin_layers(p, t, td, layers, parcel='most_unstable', moist='family')
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _abi_out(ncol, device, nlayer=4, skip=()):
    """xp_cape_layers_out with every output (but `skip`: names, or (name, layer)) allocated, in device or host memory."""
    import torch
    res = {}
    for k in L.CAPE_LAYERS_OUT + L.CAPE_LAYERS_TOTAL + ('status',):
        shape = (nlayer, ncol) if k in L.CAPE_LAYERS_OUT else (ncol,)
        if device:
            res[k] = torch.zeros(shape, dtype=torch.int32 if k == 'status' else torch.float64, device='cuda')
        else:
            res[k] = np.zeros(shape, dtype=np.int32 if k == 'status' else np.float64)
    ptr = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
    out = L.CapeLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE if device else L.XP_MEM_HOST)
    for k, a in res.items():
        if k in L.CAPE_LAYERS_OUT:
            for i in range(nlayer):
                if (k, i) not in skip:
                    getattr(out, k)[i] = ptr(a[i])
        elif k not in skip:
            setattr(out, k, ptr(a))
    return res, out


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else (a.data_ptr() if hasattr(a, 'data_ptr') else a.ctypes.data) for a in arrays])


def test_input_kinds_agree_bit_for_bit():
    import torch
    p, t, td = (a[:, :777] for a in grid(np.float64))
    bottoms, tops = ([a[:777] for a in x] for x in mixed_layers('mixed_layer', 'exact', np.float64))
    layers = [{'bottom': b, 'top': tp} for b, tp in zip(bottoms, tops)]
    layers[2] = {'top': tops[2]}
    want = xa.cape_cin_layers(p, t, td, layers, parcel='mixed_layer')
    dev = [torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in (p, t, td)]
    dl = [{k: torch.as_tensor(v).cuda() for k, v in l.items()} for l in layers]
    got = xa.cape_cin_layers(*dev, dl, parcel='mixed_layer')
    assert got['cape'].is_cuda and got['status'].dtype == torch.int32 and got['top_pressure'].is_cuda
    for k in want:
        assert np.array_equal(_np(got[k]), want[k], equal_nan=True), k
    # strided device views through the C ABI: every other column of a (nlev, 2 ncol) buffer, read in place
    wide = [torch.full((NLEV, 2 * 777), float('nan'), dtype=torch.float64, device='cuda') for _ in range(3)]
    for w, a in zip(wide, dev):
        w[:, ::2] = a
    res, out = _abi_out(777, True)
    views = [L.View(w.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, NLEV, 777, 2 * 777, 2) for w in wide]
    pc = L.Parcel(L.PARCEL['mixed_layer'], 0, 100.0, None, None, None)
    bs = [l.get('bottom') for l in dl]
    ts = [l['top'] for l in dl]
    L.check(L.init(0).xp_cape_cin_layers(*views, pc, None, 4, _ptrs(bs), _ptrs(ts), out, None))
    torch.cuda.synchronize()
    for k in res:
        assert np.array_equal(_np(res[k]), want[k], equal_nan=True), k


def _host_view(a, dtype=L.XP_F64):
    return L.View(a.ctypes.data, dtype, L.XP_MEM_HOST, a.shape[0], a.shape[1], a.shape[1], 1)


def test_null_outputs_and_null_bottoms():
    p, t, td = (np.ascontiguousarray(a[:, :300]) for a in grid(np.float64))
    bottoms, tops = ([np.ascontiguousarray(a[:300]) for a in x] for x in mixed_layers('surface', 'exact', np.float64))
    want = xa.cape_cin_layers(p, t, td, [{'bottom': b, 'top': tp} for b, tp in zip(bottoms, tops)])
    lib = L.init(0)
    views = [_host_view(a) for a in (p, t, td)]
    pc = L.Parcel(L.PARCEL['surface'], 0, 100.0, None, None, None)
    names = [(k, i) for k in L.CAPE_LAYERS_OUT for i in range(4)] + list(L.CAPE_LAYERS_TOTAL) + ['status']
    for skip in names:                                                  # every output pointer NULL in turn
        res, out = _abi_out(300, False, skip=(skip,))
        L.check(lib.xp_cape_cin_layers(*views, pc, None, 4, _ptrs(bottoms), _ptrs(tops), out, None))
        for k in res:
            for i in ([None] if res[k].ndim == 1 else range(4)):
                if skip in (k, (k, i)):
                    continue
                assert np.array_equal(res[k][i] if i is not None else res[k], want[k][i] if i is not None else want[k], equal_nan=True), (skip, k, i)
    res, out = _abi_out(300, False, skip=names)                         # all of them
    L.check(lib.xp_cape_cin_layers(*views, pc, None, 4, _ptrs(bottoms), _ptrs(tops), out, None))
    # a NULL bottom array is four NULL bottoms is four NaN bottoms
    none = xa.cape_cin_layers(p, t, td, [{'top': tp} for tp in tops])
    nans = xa.cape_cin_layers(p, t, td, [{'bottom': np.nan, 'top': tp} for tp in tops])
    res, out = _abi_out(300, False)
    L.check(lib.xp_cape_cin_layers(*views, pc, None, 4, None, _ptrs(tops), out, None))
    for k in res:
        assert np.array_equal(res[k], none[k], equal_nan=True) and np.array_equal(res[k], nans[k], equal_nan=True), k
    # fewer layers: the entries past nlayer are not touched
    res, out = _abi_out(300, False)
    L.check(lib.xp_cape_cin_layers(*views, pc, None, 2, _ptrs(bottoms), _ptrs(tops), out, None))
    assert np.array_equal(res['cape'][:2], want['cape'][:2], equal_nan=True) and (res['cape'][2:] == 0.0).all()


def test_argument_errors():
    p, t, td = (np.ascontiguousarray(a[:12, :40]) for a in grid(np.float64))
    lib = L.init(0)
    vp, vt, vtd = (_host_view(a) for a in (p, t, td))
    res, out = _abi_out(40, False)
    top = np.full(40, 500.0)
    pc = L.Parcel(L.PARCEL['surface'], 0, 100.0, None, None, None)

    def call(views=(vp, vt, vtd), parcel=pc, o=None, n=1, bottom=None, tops=(top,), out_=out):
        return lib.xp_cape_cin_layers(*views, parcel, o, n, bottom, None if tops is None else _ptrs(tops), out_, None)

    def opts(**kw):
        o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST['exact'], L.XP_F64, L.HUMIDITY['dewpoint'], 0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    assert call() == 0 and call(o=opts()) == 0 and call(o=opts(post_zero_cin=1)) == 0 and call(n=4, tops=(top,) * 4) == 0
    narrow = np.ascontiguousarray(t[:, :-1])
    for bad in (dict(n=0), dict(n=5, tops=(top,) * 5), dict(tops=None), dict(tops=(None,)), dict(n=2, tops=(top, None)),
                dict(views=(vp, _host_view(narrow), vtd)), dict(views=(vp, vt, _host_view(td.astype(np.float32), L.XP_F32))),
                dict(views=(None, vt, vtd)), dict(o=opts(humidity=L.HUMIDITY['specific'])), dict(o=opts(pos_cape_neg_cin=0)),
                dict(o=opts(moist_mode=9)), dict(parcel=None), dict(parcel=L.Parcel(7, 0, 100.0, None, None, None)),
                dict(parcel=L.Parcel(L.PARCEL['explicit'], 0, 100.0, None, None, None)), dict(out_=None),
                dict(out_=L.CapeLayersOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST))):
        assert call(**bad) == L.XP_E_ARG, (bad, lib.xp_last_error())
    assert call(o=opts(lcl_interp=5)) == L.XP_E_INTERP
    with pytest.raises(L.XParcelError):
        xa.cape_cin_layers(p, t, td, [{'top': 500.0}], pos_cape_neg_cin=False)


@pytest.mark.parametrize('kw', [dict(virtual_temperature_correction=False), dict(lcl_interp='linear'), dict(post_zero_cin=True)])
def test_options(kw):
    """The CAPE / CIN options reach the kernel: the totals stay xp_cape_cin's bit for bit, and without the virtual-temperature
    correction the layers follow the restatement on plain temperatures."""
    p, t, td = (np.ascontiguousarray(a[:, :1000]) for a in grid(np.float64))
    bottoms, tops = ([a[:1000] for a in x] for x in mixed_layers('surface', 'exact', np.float64))
    want = xa.cape_cin_columns(p, t, td, **kw)
    got = xa.cape_cin_layers(p, t, td, [{'bottom': b, 'top': tp} for b, tp in zip(bottoms[:2], tops[:2])], **kw)
    valid = (got['status'] & L.XP_ST_NO_LAYER) == 0
    for k in WHOLE:
        g = got[TOTAL_OF.get(k, k)]
        assert np.array_equal(g[valid], want[k][valid], equal_nan=True), k
    opts = dict(kw)
    vtc = opts.pop('virtual_temperature_correction', True)
    opts.pop('post_zero_cin', None)                                      # changes nothing: CIN <= 0 by construction
    ref = R.layers_grid(p, t, td, bottoms[:2], tops[:2], vtc=vtc, parcel='surface', moist='rk4', **opts)
    compare(got, ref, want, np.float64, str(kw))


# -- 4. the wrappers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_cape_3km_and_hail_growth_zone_cape(dtype):
    """The two wrappers equal cape_cin_layers called with bounds resolved on the host: np.interp in height from the lowest
    valid level, and the restatement's lowest-crossing rule for the -10 / -30 degC levels."""
    p, t, td = grid(dtype)
    z = heights(p)
    z64, p64, t64 = (np.asarray(a, dtype=np.float64) for a in (z, p, t))
    ok = ~(np.isnan(z64) | np.isnan(p64))
    z0 = np.where(ok.any(axis=0), z64[np.argmax(ok, axis=0), np.arange(NCOL)], np.nan)

    def close(a, b, tag):
        a, b = (np.asarray(x, dtype=np.float64) for x in (a, b))
        assert np.array_equal(np.isnan(a), np.isnan(b)), (tag, np.nonzero(np.isnan(a) != np.isnan(b))[0][:5])
        ok_ = ~np.isnan(b)
        tol = 1e-6 + (np.spacing(np.abs(b[ok_]).astype(np.float32)).astype(np.float64) if dtype == np.float32 else 0.0)
        err = np.abs(a[ok_] - b[ok_])
        print('%s %s: max |difference| %.3e over %d columns' % (tag, np.dtype(dtype).name, err.max(), err.size))
        assert np.all(err <= tol), (tag, err.max())
        return ok_

    for parcel in ('surface', 'most_unstable'):
        at = (z0.astype(dtype) + dtype(3000.0)).astype(np.float64)                       # z0 + h in the inputs' dtype, as the wrapper forms it
        top = R.pressure_at_height(z64, p64, at).astype(dtype)
        c3 = xa.cape_3km(p, t, td, z, parcel=parcel)
        by_hand = xa.cape_cin_layers(p, t, td, [{'top': top}], parcel=parcel)
        ok3 = close(c3, by_hand['cape'][0], 'cape_3km ' + parcel)
        assert ok3.sum() >= NCOL // 2 and np.all(c3[ok3] <= by_hand['total_cape'][ok3]) and (c3[ok3] > 0).sum() >= 100
        same = xa.cape_cin_layers(p, t, td, [{'top_height': 3000.0}], height=z, parcel=parcel)
        assert np.array_equal(same['cape'][0], c3, equal_nan=True)
        close(same['top_pressure'][0], top, 'top pressure ' + parcel)
        bot, top = (R.pressure_at_height(z64, p64, R.crossing_height(z64, t64, v).astype(dtype).astype(np.float64)).astype(dtype)
                    for v in (263.15, 243.15))
        hgz = xa.hail_growth_zone_cape(p, t, td, z, parcel=parcel)
        by_hand = xa.cape_cin_layers(p, t, td, [{'bottom': bot, 'top': top}], parcel=parcel)
        okh = close(hgz, by_hand['cape'][0], 'hail growth zone ' + parcel)
        assert okh.sum() >= NCOL // 2 and (hgz[okh] > 0).sum() >= 50 and np.all(hgz[okh] <= by_hand['total_cape'][okh])


# -- 5. at scale ------------------------------------------------------------------------------------------------------------------
def test_full_size_grid_sample():
    import torch
    nlev, ncol = 64, 1 << 20
    p, t, td = synth.columns_torch(nlev, ncol, 'cuda', seed=5)
    z = heights(p)
    b = torch.as_tensor(np.random.default_rng(3).uniform(600.0, 1000.0, ncol), device='cuda')
    res = xa.cape_cin_layers(p, t, td, [{'top_height': 3000.0}, {'bottom': b, 'top': b - 350.0}], height=z, parcel='most_unstable')
    whole_ = xa.cape_cin_columns(p, t, td, parcel='most_unstable')
    torch.cuda.synchronize()
    idx = np.linspace(0, ncol - 1, 4096).astype(np.int64)
    idx[-64:] = np.arange(ncol - 64, ncol)                              # the last wavefront too
    ti = torch.as_tensor(idx, device='cuda')
    hp, ht, htd = (a[:, ti].cpu().numpy() for a in (p, t, td))
    got = {k: _np(a[..., ti]) for k, a in res.items()}
    ref = R.layers_grid(hp, ht, htd, [None, got['bottom_pressure'][1]], list(got['top_pressure']), parcel='most_unstable', moist='rk4')
    compare(got, ref, {k: _np(a[ti]) for k, a in whole_.items()}, np.float64, 'full size')
    assert (ref['cape'][0] > 0).sum() >= 400 and (ref['cape'][1] > 0).sum() >= 400 and np.isfinite(ref['cape']).all()
