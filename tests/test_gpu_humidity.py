"""XP_HUM_RELATIVE and XP_HUM_MIXING_RATIO on the device (include/xparcel.h): the moisture view holds relative humidity (a
fraction) or the mixing ratio, one streaming kernel (csrc/xp_humidity.hpp) turns it into the dewpoint D, and the call IS the
dewpoint call on D, bit for bit.

1. D itself.  The conversion is element-wise, so D is read out of the library without an entry point of its own: the grid
   as (1, nlev * ncol) views, a surface-parcel call, parcel_dewpoint in the views' dtype.  Against the NumPy restatement
   (tests/humidity_restatement.py): fp64 within 1e-10 K (the suite's tolerance for element-wise fp64 formulas,
   tests/test_gpu_indices.py), fp32 within half a float32 ulp of the restatement's float64 value plus 1e-10 K; the same NaNs.
2. The call is the dewpoint call on D: every scalar, the status and the six profile arrays compared with ==, NaN where NaN;
   the moisture buffer's bytes are what they were after every call.
3. Against the C oracle on the restated D at the tolerances tests/test_gpu_parity.py states.
4. A call on a side stream behind a delay equals the default-stream call.
5. What is rejected, with the outputs untouched.
Grids, class columns and strided layouts: tests/humidity_cases.py (census in tests/test_humidity_cpu.py)."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import humidity_cases as K
from tests import humidity_restatement as R
from tests.test_gpu_parity import FKEYS, IKEYS, _saturated_tie_columns
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd._lib import XP_E_ARG

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
DTYPE_IDS = ('f32', 'f64')
SPACES = ('host', 'device')
# parcel, moist adiabat, further arguments: the single-parcel combinations of part 2
COMBOS = (('surface', 'family', {}), ('most_unstable', 'exact', {}), ('mixed_layer', 'family', {}), ('surface', 'table', {}),
          ('max_cape', 'exact', {}))


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


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def _cuda(a):
    return torch.as_tensor(np.array(a)).cuda()


def _in(space, *arrays):
    return tuple(_cuda(a) for a in arrays) if space == 'device' else arrays


def _bits(a):
    """The bytes of an array or tensor as integers (NaN payloads compare)."""
    a = _np(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32).copy()


def assert_same(got, want, where=''):
    """Two results of the array API -- dicts of arrays, 'profile' a dict of its own, or lists of them -- equal bit for bit, NaN where NaN."""
    if isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, '%s[%d] ' % (where, i))
        return
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    for k in want:
        if isinstance(want[k], dict):
            assert_same(got[k], want[k], where + k + '.')
            continue
        a, b = _np(got[k]), _np(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (where + k, a.shape, b.shape, a.dtype, b.dtype)
        same = (a == b) | ((a != a) & (b != b))
        assert same.all(), (where + k, int((~same).sum()), np.argwhere(~same)[:5].tolist(), a[~same][:5], b[~same][:5])


def library_dewpoint(kind, p, t, m, space='host'):
    """D of the dense arrays p, T, m as the library computes it, read out element by element (part 1 of the module docstring)."""
    flat = _in(space, *(np.ascontiguousarray(a).reshape(1, -1) for a in (p, t, m)))
    d = xa.cape_cin_columns(*flat, parcel='surface', moist='family', humidity=kind, want=('parcel_dewpoint',))['parcel_dewpoint']
    d = _np(d)
    assert d.dtype == m.dtype and d.shape == (m.size,)
    return np.ascontiguousarray(d.reshape(m.shape))


@functools.lru_cache(maxsize=None)
def grid_with_dewpoint(name, kind, dtype):
    """(p, T, m, D) of a grid of tests/humidity_cases.py, D by the library (host arrays); shared, read-only."""
    p, t, m = K.grid(name, kind, dtype)
    d = library_dewpoint(kind, p, t, m)
    d.flags.writeable = False
    return p, t, m, d


def heights(p):
    with np.errstate(invalid='ignore'):
        return np.ascontiguousarray((8000.0 * np.log(p[0:1].astype(np.float64) / p.astype(np.float64))).astype(p.dtype))


# -- 1. D itself ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', SPACES)
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', tuple(K.SHAPES))
def test_dewpoint_is_the_restatement_s(name, kind, dtype, space):
    p, t, m = K.grid(name, kind, dtype)
    before = _bits(m)
    got = library_dewpoint(kind, p, t, m, space).astype(np.float64)
    want = R.dewpoint64(kind, p, t, m)
    assert np.array_equal(np.isnan(got), np.isnan(want)), np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()
    ok = ~np.isnan(want)
    assert np.isfinite(want[ok]).all() and np.isfinite(got[ok]).all()
    err = np.abs(got[ok] - want[ok])
    tol = 1e-10 if dtype == np.float64 else 0.5 * np.spacing(np.abs(want[ok]).astype(np.float32)).astype(np.float64) + 1e-10
    print('%s %s %s %s: %d of %d finite, max |D - restatement| %.3e K (bound %.3e)'
          % (name, kind, np.dtype(dtype).name, space, ok.sum(), ok.size, err.max() if ok.any() else 0.0, np.max(tol)))
    assert (err <= tol).all(), (err.max(), np.argwhere(err > tol)[:5].tolist())
    assert np.array_equal(_bits(m), before)
    if name == K.MAIN:                                       # the class columns say what they are named for
        col = lambda c: got[:, K.CLASSES[c]]
        assert all(np.isnan(col(c)).all() for c in K.MOISTURE_VALUE)
        assert np.isnan(col('t_nan')[list(K.T_NAN_LEVELS)]).all() == (kind == R.RELATIVE)
        assert np.isnan(col('p_nan')[list(K.P_NAN_LEVELS)]).all() == (kind == R.MIXING_RATIO)
        if kind == R.RELATIVE:
            assert (col('rh_1.05') > t[:, K.CLASSES['rh_1.05']]).all() and np.isfinite(col('rh_1e-6')).all()
        else:
            assert np.isfinite(col('w_0.04')).all()


# -- 2. the call is the dewpoint call on D ------------------------------------------------------------------------------------------
def _ground(p, t, d):
    """Surface fields that cut one to three levels off every column: pressure, temperature, DEWPOINT (from D)."""
    cols = np.arange(p.shape[1])
    ks = np.minimum(1 + cols % 3, p.shape[0] - 1)
    return tuple(np.ascontiguousarray(a) for a in ((p[ks, cols] + 3.0).astype(p.dtype), (t[ks, cols] + 0.5).astype(p.dtype), d[ks, cols]))


@pytest.mark.parametrize('space', SPACES)
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('ground', (False, True), ids=('levels', 'ground'))
def test_single_parcel_calls(ground, kind, dtype, space, tables):
    p, t, m, d = grid_with_dewpoint(K.MAIN, kind, dtype)
    P, T, M, D = _in(space, p, t, m, d)
    before = _bits(M)
    sfc = _in(space, *_ground(p, t, d)) if ground else None
    for parcel, moist, kw in COMBOS:
        if ground and parcel == 'max_cape':                  # (the two do not combine)
            continue
        kw = dict(kw, parcel=parcel, moist=moist, want_profile=True, ground=sfc)
        got = xa.cape_cin_columns(P, T, M, humidity=kind, **kw)
        want = xa.cape_cin_columns(P, T, D, **kw)
        assert got['profile']['environment_dewpoint'].shape[0] == p.shape[0] + (2 if ground else 1)
        assert_same(got, want, '%s %s: ' % (parcel, moist))
        assert np.array_equal(_bits(M), before), (parcel, moist)
        if parcel == 'surface' and not ground:               # (the comparison is not one of NaN with NaN)
            assert np.isfinite(_np(got['cape'])).all() and (_np(got['cape']) > 0).sum() * 4 >= p.shape[1]
            assert np.isfinite(_np(got['profile']['environment_dewpoint'])).mean() > 0.8


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', tuple(n for n in K.SHAPES if n != K.MAIN))
def test_every_shape(name, kind, dtype):
    """The shapes around the 16-byte run and the wavefront edge, rows addressed as rows: the surface call with its profile."""
    p, t, m, d = grid_with_dewpoint(name, kind, dtype)
    for space in SPACES:
        P, T, M, D = _in(space, p, t, m, d)
        got = xa.cape_cin_columns(P, T, M, humidity=kind, moist='family', want_profile=True)
        assert_same(got, xa.cape_cin_columns(P, T, D, moist='family', want_profile=True), '%s %s: ' % (name, space))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('fused', (False, True), ids=('unfused', 'fused'))
def test_multi(fused, kind, dtype):
    p, t, m, d = grid_with_dewpoint(K.MAIN, kind, dtype)
    before = _bits(m)
    for space in SPACES:
        P, T, M, D = _in(space, p, t, m, d)
        for parcels in (['surface', 'mixed_layer'], [('most_unstable', 300), ('mixed_layer', 100)], ['surface', ('max_cape', 250), 'most_unstable']):
            got = xa.cape_cin_multi(P, T, M, parcels, moist='family', fused=fused, humidity=kind)
            assert_same(got, xa.cape_cin_multi(P, T, D, parcels, moist='family', fused=fused), '%s %s: ' % (space, parcels))
        sfc = _in(space, *_ground(p, t, d))
        got = xa.cape_cin_multi(P, T, M, ['surface', 'mixed_layer'], moist='family', fused=fused, humidity=kind, ground=sfc, lifted_index_at=500.0)
        assert_same(got, xa.cape_cin_multi(P, T, D, ['surface', 'mixed_layer'], moist='family', fused=fused, ground=sfc, lifted_index_at=500.0), space + ' ground: ')
        assert np.array_equal(_bits(M), before)
    # the converted grid is what the single calls see
    single = xa.cape_cin_columns(p, t, m, parcel='mixed_layer', moist='family', humidity=kind)
    assert_same(xa.cape_cin_multi(p, t, m, ['surface', 'mixed_layer'], moist='family', fused=fused, humidity=kind)[1], single)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', R.KINDS)
def test_layers_and_inflow(kind, dtype, tables):
    p, t, m, d = grid_with_dewpoint(K.MAIN, kind, dtype)
    z = heights(p)
    before = _bits(m)
    layers = [{'top': 500.0}, {'bottom': 900.0, 'top': 600.0}, {'top_height': 3000.0}]
    for space in SPACES:
        P, T, M, D, Z = _in(space, p, t, m, d, z)
        for parcel, moist in (('surface', 'exact'), ('mixed_layer', 'table'), ('most_unstable', 'exact')):
            got = xa.cape_cin_layers(P, T, M, layers, height=Z, parcel=parcel, moist=moist, humidity=kind)
            assert_same(got, xa.cape_cin_layers(P, T, D, layers, height=Z, parcel=parcel, moist=moist), '%s layers %s: ' % (space, parcel))
        assert_same({'x': xa.cape_3km(P, T, M, Z, humidity=kind)}, {'x': xa.cape_3km(P, T, D, Z)}, space + ' cape_3km ')
        assert_same({'x': xa.hail_growth_zone_cape(P, T, M, Z, humidity=kind)}, {'x': xa.hail_growth_zone_cape(P, T, D, Z)}, space + ' hail ')
        for moist in ('exact', 'table'):
            got = xa.effective_inflow_layer(P, T, M, Z, moist=moist, want_candidates=True, humidity=kind)
            want = xa.effective_inflow_layer(P, T, D, Z, moist=moist, want_candidates=True)
            assert_same(got, want, '%s inflow %s: ' % (space, moist))
        assert (_np(want['base_index']) >= 0).any()
        assert np.array_equal(_bits(M), before)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', ('24x64', '24x257'))
def test_strided_views_through_the_raw_abi(name, kind, dtype):
    p, t, m = K.grid(name, kind, dtype)
    lib = L.init(0)
    nlev, ncol = p.shape
    xdt = L.XP_F64 if dtype == np.float64 else L.XP_F32
    names = ('cape', 'cin', 'lcl_pressure', 'lfc_pressure', 'el_pressure', 'parcel_dewpoint')
    stream = torch.cuda.current_stream().cuda_stream
    for what, (views, dense, mt, keep) in K.device_layouts(p, t, m, _cuda).items():
        d = library_dewpoint(kind, *dense)
        before = _bits(mt)
        for parcel, moist in (('surface', 'family'), ('mixed_layer', 'exact')):
            want = xa.cape_cin_columns(dense[0], dense[1], d, parcel=parcel, moist=moist, want=names + ('status', 'lfc_index'), want_profile=True)
            out = {k: torch.full((ncol,), -5.0, dtype=mt.dtype, device='cuda') for k in names}
            out['status'] = torch.full((ncol,), -5, dtype=torch.int32, device='cuda')
            out['lfc_index'] = torch.full((ncol,), -5, dtype=torch.int32, device='cuda')
            prof = {k: torch.full((nlev + 1, ncol), -5.0, dtype=mt.dtype, device='cuda') for k in L.PROFILE_VARS}
            so = L.ScalarsOut(dtype=xdt, mem=L.XP_MEM_DEVICE)
            for k, a in out.items():
                setattr(so, k, a.data_ptr())
            po = L.ProfileOut(dtype=xdt, mem=L.XP_MEM_DEVICE, nlev_out=nlev + 1, lev_stride=ncol, col_stride=1)
            for k, a in prof.items():
                setattr(po, k, a.data_ptr())
            pc = L.Parcel(L.PARCEL[parcel], 0, 100.0, None, None, None)
            o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST[moist], L.XP_F64, L.HUMIDITY[kind], 0)
            rc = lib.xp_cape_cin(*[C.byref(v) for v in views], C.byref(pc), C.byref(o), C.byref(so), C.byref(po), stream)
            assert rc == 0, lib.xp_last_error()
            torch.cuda.synchronize()
            assert_same({**out, 'profile': prof}, want, '%s, %s %s: ' % (what, parcel, moist))
            assert np.array_equal(_bits(mt), before), what
        # the inflow call stages its own views
        eo = L.EffectiveLayerOut(dtype=xdt, mem=L.XP_MEM_DEVICE)
        res = {k: torch.full((ncol,), -5.0, dtype=mt.dtype, device='cuda') for k in ('base_pressure', 'top_pressure')}
        for k, a in res.items():
            setattr(eo, k, a.data_ptr())
        o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST['exact'], L.XP_F64, L.HUMIDITY[kind], 0)
        rc = lib.xp_effective_inflow_layer(*[C.byref(v) for v in views], None, 100.0, -250.0, 300.0, C.byref(o), C.byref(eo), stream)
        assert rc == 0, lib.xp_last_error()
        torch.cuda.synchronize()
        want = xa.effective_inflow_layer(dense[0], dense[1], d, moist='exact')
        assert_same(res, {k: want[k] for k in res}, what + ', inflow: ')
        assert np.array_equal(_bits(mt), before), what


# -- 3. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('parcel', ('surface', 'most_unstable', 'mixed_layer'))
@pytest.mark.parametrize('kind', R.KINDS)
def test_against_the_oracle_on_the_restated_dewpoint(kind, parcel):
    """fp64: CAPE / CIN within 1e-6 J/kg, pressures and temperatures within 1e-7 hPa / K, indices and status exact, outside the
    saturated-parcel ties tests/test_gpu_parity.py describes and bounds.  One column leaves the comparison for the two searching
    parcels: the class column with a NaN PRESSURE (level 5).  That is outside the oracle's input contract; the kernels treat such
    a level as missing where the reference's literal insert_level and its layer search do something else
    (test_nan_pressure_levels of tests/test_gpu_parity.py is the contract), and in this column the two differ by 40 J/kg of CAPE
    for the most-unstable parcel and by 83 J/kg for the mixed-layer parcel -- with a dewpoint view just as with the new kinds:
    part 2 compares the column bit for bit.  For the surface parcel, where they agree, the column is compared like any other."""
    p, t, m = K.grid(K.MAIN, kind, np.float64)
    got = {k: _np(v) for k, v in xa.cape_cin_columns(p, t, m, parcel=parcel, moist='exact', humidity=kind).items()}
    ref = co.cape_cin_grid(p, t, R.dewpoint(kind, p, t, m), parcel=parcel, moist='rk4')
    label_only, excluded = _saturated_tie_columns(got, ref)
    keep = ~excluded
    if parcel != 'surface':
        keep[K.CLASSES['p_nan']] = False
    print('%s %s: %d columns, %d sign ties left out, %d label ties' % (kind, parcel, keep.size, excluded.sum(), label_only.sum()))
    worst = {}
    for k in FKEYS:
        a, b = got[k][keep], ref[k][keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (k, np.nonzero(np.isnan(a) != np.isnan(b))[0][:10])
        ok = ~np.isnan(b)
        worst[k] = np.abs(a[ok] - b[ok]).max()
    print(' '.join('%s %.2e' % kv for kv in worst.items()))
    for k in IKEYS:
        ok = keep & ~label_only if k == 'lfc_index' else keep
        assert np.array_equal(got[k][ok], ref[k][ok]), (k, np.nonzero((got[k] != ref[k]) & ok)[0][:10])
    for k in FKEYS:
        assert worst[k] <= (1e-6 if k in ('cape', 'cin') else 1e-7), (k, worst[k])
    assert (ref['cape'] > 0).sum() * 4 >= keep.size


# -- 4. side stream --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_side_stream_behind_a_delay(kind):
    """The inputs are NaN-filled buffers; on a side stream a delay is enqueued, then the copies of the real inputs, then the
    call.  Whatever the call put on another stream would read NaN.  The call must return with the delay still running."""
    p, t, m, d = grid_with_dewpoint(K.MAIN, kind, np.float64)
    real = _in('device', p, t, m)
    kw = dict(parcel='mixed_layer', moist='family', humidity=kind, want_profile=True)
    want = xa.cape_cin_columns(*real, **kw)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for cycles in (150_000_000, 600_000_000, 2_400_000_000):         # ~60 ms, then x 4 (tests/test_gpu_streams.py)
        bufs = [torch.full_like(x, float('nan')) for x in real]
        torch.cuda.synchronize()
        e = torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            e.record()
            for b, x in zip(bufs, real):
                b.copy_(x, non_blocking=True)
            t0 = time.perf_counter()
            got = xa.cape_cin_columns(*bufs, **kw)
            dt = time.perf_counter() - t0
            pending = not e.query()
        s.synchronize()
        print('%s: enqueue %.3f ms behind %d cycles, event pending: %s' % (kind, 1e3 * dt, cycles, pending))
        if pending:
            break
    assert pending, 'the call blocks, or its enqueue outlasts every delay'
    assert_same(got, want, 'side stream: ')
    assert np.isfinite(_np(got['cape'])).all()


# -- 5. what is rejected, with the outputs untouched ---------------------------------------------------------------------------
def _host_view(a, dtype=L.XP_F64):
    return L.View(a.ctypes.data, dtype, L.XP_MEM_HOST, a.shape[0], a.shape[1], a.shape[1], 1)


def test_rejections_leave_the_outputs_untouched():
    lib = L.init(0)
    p, t, m = (np.array(a[:, :40]) for a in K.grid(K.MAIN, R.RELATIVE, np.float64))
    nlev, ncol = p.shape
    vref = [C.byref(v) for v in [_host_view(a) for a in (p, t, m)]]
    outs = {k: np.full(ncol, -5.0) for k in ('cape', 'cin', 'parcel_dewpoint')}
    so = L.ScalarsOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    for k, a in outs.items():
        setattr(so, k, a.ctypes.data)
    opts = lambda **kw: L.Opts(**{**dict(virtual_temperature_correction=1, lcl_interp=1, pos_cape_neg_cin=1, post_zero_cin=0,
                                         moist_mode=L.MOIST['exact'], compute=L.XP_F64, humidity=0, flags=0), **kw})
    parcel = lambda mode=0, depth=300.0: L.Parcel(mode, 0, depth, None, None, None)
    layer = np.full(ncol, -5.0)
    lo = L.CapeLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    lo.cape[0] = lo.total_cape = layer.ctypes.data
    top = np.full(ncol, 500.0)
    tops = (C.c_void_p * 1)(top.ctypes.data)
    base = np.full(ncol, -5.0)
    eo = L.EffectiveLayerOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, base_pressure=base.ctypes.data)

    def rejected(rc, *words):
        msg = lib.xp_last_error().decode()
        assert rc == XP_E_ARG, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert all((a == -5).all() for a in outs.values()) and (layer == -5).all() and (base == -5).all()

    cape = lambda pc, o: lib.xp_cape_cin(*vref, C.byref(pc), C.byref(o), C.byref(so), None, None)
    sos = (L.ScalarsOut * 2)(so, so)
    multi = lambda a, b, o: lib.xp_cape_cin_multi(*vref, 2, (L.Parcel * 2)(a, b), C.byref(o), sos, None, None)
    layers = lambda o: lib.xp_cape_cin_layers(*vref, C.byref(parcel()), C.byref(o), 1, None, tops, C.byref(lo), None)
    inflow = lambda o: lib.xp_effective_inflow_layer(*vref, None, 100.0, -250.0, 300.0, C.byref(o), C.byref(eo), None)
    for bad in (-1, 4, 5, 1 << 20):
        rejected(cape(parcel(), opts(humidity=bad)), 'bad xp_opts.humidity')
        rejected(multi(parcel(), parcel(2, 100.0), opts(humidity=bad)), 'bad xp_opts.humidity')
        rejected(layers(opts(humidity=bad)), 'bad xp_opts.humidity')
        rejected(inflow(opts(humidity=bad)), 'bad xp_opts.humidity')
    # specific humidity is still refused where it was, in the same words
    spec = L.HUMIDITY['specific']
    rejected(layers(opts(humidity=spec)), 'xp_cape_cin_layers: humidity must be XP_HUM_DEWPOINT')
    rejected(inflow(opts(humidity=spec)), 'xp_effective_inflow_layer: humidity must be XP_HUM_DEWPOINT')
    rejected(cape(parcel(L.PARCEL['max_cape']), opts(humidity=spec)), 'parcel: XP_PARCEL_MAX_CAPE: humidity must be XP_HUM_DEWPOINT')
    rejected(multi(parcel(), parcel(L.PARCEL['max_cape']), opts(humidity=spec)), 'parcel: XP_PARCEL_MAX_CAPE: humidity must be XP_HUM_DEWPOINT')
    # fp32 arithmetic takes dewpoints only
    f32 = [np.ascontiguousarray(a, dtype=np.float32) for a in (p, t, m)]
    v32 = [C.byref(_host_view(a, L.XP_F32)) for a in f32]
    so32 = L.ScalarsOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, cape=outs['cape'].ctypes.data)
    for kind in R.KINDS + ('specific',):
        o = opts(moist_mode=L.MOIST['family'], compute=L.XP_F32, humidity=L.HUMIDITY[kind])
        rejected(lib.xp_cape_cin(*v32, C.byref(parcel()), C.byref(o), C.byref(so32), None, None),
                 'xp_opts.compute = XP_F32: humidity must be XP_HUM_DEWPOINT')
    # and the same arguments with the new kinds run
    for kind in R.KINDS:
        o = opts(humidity=L.HUMIDITY[kind])
        assert cape(parcel(), o) == 0, lib.xp_last_error()
        assert cape(parcel(L.PARCEL['max_cape']), o) == 0, lib.xp_last_error()
        assert layers(o) == 0 and inflow(o) == 0, lib.xp_last_error()
    want = xa.cape_cin_columns(p, t, m, parcel='max_cape', moist='exact', humidity=R.MIXING_RATIO, want=tuple(outs))
    assert_same(outs, want)
    assert (layer != -5).all() and (base != -5).all()
    # an empty grid: nothing to convert, nothing written
    before = {k: v.copy() for k, v in outs.items()}
    empty = [C.byref(L.View(x.ctypes.data, L.XP_F64, L.XP_MEM_HOST, nlev, 0, 0, 1)) for x in (p, t, m)]
    assert lib.xp_cape_cin(*empty, C.byref(parcel()), C.byref(opts(humidity=2)), C.byref(so), None, None) == 0, lib.xp_last_error()
    assert all(np.array_equal(outs[k], before[k], equal_nan=True) for k in outs)


# -- the DataArray modules end to end ------------------------------------------------------------------------------------------------
def test_dataarray_modules_on_the_device():
    from xarray_parcel_amd import ground, kinematics, layer_cape, max_cape
    from xarray_parcel_amd._xr import DataArray
    p, t, m, d = grid_with_dewpoint(K.MAIN, R.RELATIVE, np.float32)
    nlev, ny, nx = p.shape[0], 7, 191                                   # 1337 = 7 x 191
    lev = lambda a, units=None: DataArray(a.reshape(nlev, ny, nx).transpose(1, 0, 2), dims=('y', 'lev', 'x'),
                                          attrs={} if units is None else {'units': units})
    flat = lambda a: DataArray(a.reshape(ny, nx), dims=('y', 'x'))
    P, T, M, Z = lev(p), lev(t), lev(m, '1'), lev(heights(p))
    same = lambda da, a: np.array_equal(np.asarray(da.values).reshape(-1), _np(a).reshape(-1), equal_nan=True)
    ds = max_cape.max_cape_cape_cin(P, T, M, vert_dim='lev', moist='family', humidity='relative')
    want = xa.cape_cin_columns(p, t, d, parcel='max_cape', moist='family')
    assert all(same(ds[k], v) for k, v in want.items())
    sfc = _ground(p, t, d)
    ds = ground.mixed_layer_cape_cin(P, T, M, *map(flat, sfc), vert_dim='lev', moist='family', humidity='relative')
    want = xa.cape_cin_columns(p, t, d, parcel='mixed_layer', depth=100, moist='family', ground=sfc)
    assert all(same(ds[k], v) for k, v in want.items())
    ds = layer_cape.cape_cin_layers(P, T, M, [{'top': 500.0}], vert_dim='lev', humidity='relative')
    assert same(ds['cape'], xa.cape_cin_layers(p, t, d, [{'top': 500.0}])['cape'])
    ds = kinematics.effective_inflow_layer(P, T, M, Z, vert_dim='lev', humidity='relative')
    assert same(ds['base_pressure'], xa.effective_inflow_layer(p, t, d, heights(p))['base_pressure'])
    with pytest.raises(ValueError, match='fraction'):
        max_cape.max_cape_cape_cin(P, T, lev(m * 100, 'percent'), vert_dim='lev', humidity='relative')
