"""The positive-layer choice of xp_cape_cin / xp_cape_cin_multi (xp_opts.flags, XP_OPT_LAYER_*) on the device: against the
NumPy restatement tests/positive_layer_restatement.py on the layered grid of tests/positive_layer_cases.py, bit for bit
against the library itself where the header promises that, and its argument checks.

Tolerance against the restatement: 1e-6 (J/kg, hPa, K; plus one float32 spacing for float32 outputs) -- what
tests/test_gpu_layer_cape.py holds total_cape and lfc_pressure to against the same oracle.  Columns that
test_gpu_parity._saturated_tie_columns classifies as saturated-parcel sign ties are left out, under that function's own
bounds, and its label ties are exempt from the lfc_index comparison as they are there; nothing else is.
K itself is no output of the call: it is held through the indices, the NaN classes and the K <= 1 identity."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import ground_restatement as GR
from tests import humidity_restatement as HR
from tests import max_cape_restatement as MR
from tests import positive_layer_cases as K
from tests import positive_layer_restatement as R
from tests.test_gpu_parity import _saturated_tie_columns
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd._lib import XP_E_ARG

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
DTYPE_IDS = ('f64', 'f32')
REST = ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'status', 'parcel_index', 'parcel_pressure', 'parcel_temperature',
        'parcel_dewpoint')                                               # what no choice changes


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
    co.set_tables(tab)
    adiabat_tables.set_tables(tab.index, tab.adiabats)                   # both sides look up the SAME arrays
    return tab


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def _cuda(*arrays):
    return tuple(torch.as_tensor(np.array(a)).cuda() for a in arrays)


def assert_same(got, want, where='', cols=None):
    """Two results of the array API (dicts of arrays, or lists of them) equal bit for bit, NaN where NaN; cols: on these columns."""
    if isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, '%s[%d] ' % (where, i), cols)
        return
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    for k in want:
        a, b = _np(got[k]), _np(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (where + k, a.shape, b.shape, a.dtype, b.dtype)
        if cols is not None:
            a, b = a[cols], b[cols]
        same = (a == b) | ((a != a) & (b != b))
        assert same.all(), (where + k, int((~same).sum()), np.argwhere(~same)[:5].tolist(), a[~same][:5], b[~same][:5])


@functools.lru_cache(maxsize=None)
def default_call(parcel, moist, dtype, spec=K.MAIN):
    """The library's own default (envelope) result for a grid: computed once, shared."""
    return xa.cape_cin_columns(*K.grid(spec, dtype), parcel=parcel, moist=moist)


def compare(got, ref, whole, oracle, dtype, tag):
    """got against the restated choice `ref`; whole: the default call's result for the same columns (the tie classification and
    the scalars no choice changes)."""
    label_only, excluded = _saturated_tie_columns(whole, oracle)
    keep = ~excluded
    f32 = dtype == np.float32
    for k in R.FIELDS:
        g, r = _np(got[k]).astype(np.float64)[keep], ref[k][keep]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k, np.nonzero(np.isnan(g) != np.isnan(r))[0][:5])
        ok = ~np.isnan(r)
        tol = np.full(ok.sum(), 1e-6)
        if f32:
            tol = tol + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        err = np.abs(g[ok] - r[ok])
        print('%s %s: max |error| %.3e over %d values' % (tag, k, err.max() if err.size else 0.0, err.size))
        assert np.all(err <= tol), (tag, k, float(err.max()), np.nonzero(keep)[0][np.nonzero(ok)[0][np.argmax(err - tol)]])
    assert np.array_equal(_np(got['el_index'])[keep], ref['el_index'][keep]), (tag, 'el_index')
    idx = keep & ~label_only
    bad = np.nonzero(idx & (_np(got['lfc_index']) != ref['lfc_index']))[0]
    assert bad.size == 0, (tag, 'lfc_index', bad[:5], _np(got['lfc_index'])[bad[:5]], ref['lfc_index'][bad[:5]])
    assert_same({k: got[k] for k in REST}, {k: whole[k] for k in REST}, tag + ' ')
    return keep


# -- 1. against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('parcel', K.PARCELS)
def test_choices_vs_restatement(parcel, dtype):
    p, t, td = K.grid(K.MAIN, dtype)
    g = K.restated(parcel)
    whole = default_call(parcel, 'exact', dtype)
    dev = _cuda(p, t, td)
    moved = {}
    for ch in K.CHOICES:
        got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='exact', positive_layer=ch)
        assert got['cape'].dtype == dtype and got['lfc_index'].dtype == np.int32
        keep = compare(got, g[ch], whole, g['oracle'], dtype, '%s %s %s' % (parcel, ch, np.dtype(dtype).name))
        on_device = xa.cape_cin_columns(*dev, parcel=parcel, moist='exact', positive_layer=ch)
        assert on_device['cape'].is_cuda and on_device['status'].dtype == torch.int32
        assert_same(on_device, got, 'device tensors ')
        moved[ch] = int((keep & (_np(got['cape']) != _np(whole['cape']))).sum())
    print(parcel, 'columns whose cape left the default:', moved)
    assert all(n >= 100 for n in moved.values()), moved                    # (the comparison is not one of the default with itself)
    assert int(np.isnan(p).sum() + np.isnan(t).sum()) > 1000               # the NaN levels the grid carries


def test_table_mode_vs_restatement(tables):
    p, t, td = K.grid()
    g = K.restated('surface', 'table')
    whole = default_call('surface', 'table', np.float64)
    for ch in K.CHOICES:
        got = xa.cape_cin_columns(p, t, td, parcel='surface', moist='table', positive_layer=ch)
        compare(got, g[ch], whole, g['oracle'], np.float64, 'table ' + ch)
    assert (g['K'] >= 2).sum() >= 150


# -- 2. against the library itself, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('parcel,moist', [(pc, 'exact') for pc in K.PARCELS] + [('surface', 'table')])
def test_columns_with_at_most_one_layer_are_the_default_call(parcel, moist, dtype, tables):
    p, t, td = K.grid(K.MAIN, dtype)
    g = K.restated(parcel, moist)
    whole = default_call(parcel, moist, dtype)
    label_only, excluded = _saturated_tie_columns(whole, g['oracle'])
    few = (g['K'] <= 1) & ~excluded & ~label_only
    assert few.sum() >= 2000
    for ch in K.CHOICES:
        got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, positive_layer=ch)
        assert_same(got, whole, '%s %s %s: ' % (parcel, moist, ch), cols=few)
    # and the envelope by name is the default call
    assert_same(xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, positive_layer='envelope'), whole)


def test_family_request_runs_as_exact():
    p, t, td = K.grid()
    for parcel, ch in (('surface', 'most_cape'), ('most_unstable', 'highest')):
        a = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='exact', positive_layer=ch)
        b = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='family', positive_layer=ch)
        assert_same(b, a, parcel + ' ')


@pytest.mark.parametrize('fused', (False, True))
def test_multi_equals_the_single_calls(fused):
    p, t, td = K.grid(K.MAIN, np.float32)
    parcels = ['surface', ('most_unstable', 300), ('mixed_layer', 100)] if not fused else [('most_unstable', 300), ('mixed_layer', 100)]
    for ch, moist in (('deepest', 'exact'), ('lowest', 'family')):
        outs = xa.cape_cin_multi(p, t, td, parcels, moist=moist, fused=fused, positive_layer=ch)
        want = [xa.cape_cin_columns(p, t, td, parcel=pc if isinstance(pc, str) else pc[0], depth=None if isinstance(pc, str) else pc[1],
                                    moist=moist, positive_layer=ch) for pc in parcels]
        assert_same(outs, want, '%s %s ' % (ch, moist))


def test_a_permutation_of_the_columns_permutes_the_results():
    p, t, td = K.grid()
    perm = np.random.default_rng(2).permutation(p.shape[1])
    for parcel, ch in (('surface', 'deepest'), ('mixed_layer', 'most_cape'), ('most_unstable', 'lowest')):
        a = xa.cape_cin_columns(p, t, td, parcel=parcel, positive_layer=ch)
        b = xa.cape_cin_columns(*(np.ascontiguousarray(x[:, perm]) for x in (p, t, td)), parcel=parcel, positive_layer=ch)
        assert_same(b, {k: v[perm] for k, v in a.items()}, parcel + ' ')


# -- 3. composition with the passes in front, bit for bit ----------------------------------------------------------------------
def _compose_grid(dtype):
    return K.grid(K.COMPOSE, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_relative_humidity_composes(dtype):
    """humidity='relative': the call is the dewpoint call on D, D read out of the library as tests/test_gpu_humidity.py does."""
    p, t, td = _compose_grid(dtype)
    rh = np.ascontiguousarray(HR.relative_humidity(t, td).astype(dtype))
    flat = tuple(np.ascontiguousarray(a).reshape(1, -1) for a in (p, t, rh))
    d = _np(xa.cape_cin_columns(*flat, parcel='surface', moist='family', humidity='relative', want=('parcel_dewpoint',))['parcel_dewpoint'])
    d = np.ascontiguousarray(d.reshape(rh.shape))
    assert d.dtype == dtype and np.isfinite(d).mean() > 0.8
    for parcel, ch in (('surface', 'most_cape'), ('most_unstable', 'deepest'), ('mixed_layer', 'highest')):
        got = xa.cape_cin_columns(p, t, rh, parcel=parcel, humidity='relative', positive_layer=ch)
        want = xa.cape_cin_columns(p, t, d, parcel=parcel, positive_layer=ch)
        assert_same(got, want, parcel + ' ')
        assert (_np(got['cape']) != _np(xa.cape_cin_columns(p, t, d, parcel=parcel)['cape'])).sum() >= 5


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_ground_composes(dtype):
    """ground=: the call is the call on the re-based columns of tests/ground_restatement.py, as tests/test_gpu_ground.py has it."""
    p, t, td = _compose_grid(dtype)
    cols = np.arange(p.shape[1])
    ks = 1 + cols % 3                                                    # one to three levels below the ground
    sfc = tuple(np.ascontiguousarray(a) for a in ((p[ks, cols] + 3.0).astype(dtype), (t[ks, cols] + 0.5).astype(dtype), td[ks, cols]))
    rebased = GR.rebase(p, t, td, *sfc)
    assert rebased[0].shape == (p.shape[0] + 1, p.shape[1]) and rebased[0].dtype == dtype
    for parcel, ch in (('surface', 'highest'), ('most_unstable', 'most_cape'), ('mixed_layer', 'deepest')):
        got = xa.cape_cin_columns(p, t, td, parcel=parcel, ground=sfc, positive_layer=ch)
        want = xa.cape_cin_columns(*rebased, parcel=parcel, positive_layer=ch)
        assert_same(got, want, parcel + ' ')
        assert (_np(got['cape']) != _np(xa.cape_cin_columns(*rebased, parcel=parcel)['cape'])).sum() >= 5


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_max_cape_parcel_composes(dtype):
    """parcel='max_cape': the surface call on the columns from k* on, k* composed from the library's own surface calls as
    tests/test_gpu_max_cape.py composes it; parcel_index = k*."""
    p, t, td = _compose_grid(dtype)
    cand = MR.candidates(p, t, td, 300.0)
    cape = np.full(cand.shape, np.nan)
    for k in np.nonzero(cand.any(axis=1))[0]:
        cape[k] = _np(xa.cape_cin_columns(p[k:], t[k:], td[k:], parcel='surface', moist='exact', want=('cape',))['cape'])
    kstar = MR.choose(cand, np.where(cand, cape, np.nan))
    rebased = MR.rebase(p, t, td, kstar)
    for ch in ('lowest', 'most_cape'):
        got = xa.cape_cin_columns(p, t, td, parcel='max_cape', depth=300.0, positive_layer=ch)
        want = xa.cape_cin_columns(*rebased, parcel='surface', positive_layer=ch)
        assert (_np(want['parcel_index']) == 0).all()
        want['parcel_index'] = kstar.astype(np.int32)
        assert_same(got, want, ch + ' ')
    assert (kstar > 0).sum() >= 30


# -- 4. edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tuple(K.SMALL))
def test_small_grids(name):
    """One and two levels: three or four nodes, and no column of these grids has two layers (the restatement says so), so every
    choice IS the default call; the one column of 40 levels has two layers and follows the restatement."""
    spec = K.SMALL[name]
    p, t, td = K.grid(spec)
    assert p.shape == spec[:2]
    for parcel in ('surface', 'mixed_layer'):
        g = K.restated(parcel, 'exact', spec)
        whole = xa.cape_cin_columns(p, t, td, parcel=parcel)
        for ch in K.CHOICES:
            got = xa.cape_cin_columns(p, t, td, parcel=parcel, positive_layer=ch)
            if p.shape[0] <= 2:
                # (a saturated parcel -- LCL on its own level -- can have a crossing ON the LCL, and whether xp_cape_cin counts
                # it hangs on the last bit and on whether the wavefront's other columns have passed their LCLs: Scan::special's
                # ABOVE form takes it, the general form breaks the tie.  The oracle's bounds on that class do not hold on 64
                # two-level columns, so here the class is left out by what defines it)
                unsaturated = np.nonzero(~(_np(whole['lcl_pressure']) == _np(whole['parcel_pressure'])))[0]
                assert g['K'].max() <= 1 and unsaturated.size >= 56
                assert_same(got, whole, '%s %s %s ' % (name, parcel, ch), cols=unsaturated)
            else:
                assert g['K'].min() >= 2
                compare(got, g[ch], whole, g['oracle'], np.float64, '%s %s %s' % (name, parcel, ch))


def test_all_nan_column_and_one_column():
    p, t, td = (np.array(a[:, :130]) for a in K.grid())
    t[:, 7] = np.nan
    td[:, 64] = np.nan
    p[:, 129] = np.nan
    whole = xa.cape_cin_columns(p, t, td, parcel='most_unstable')
    for ch in K.CHOICES:
        got = xa.cape_cin_columns(p, t, td, parcel='most_unstable', positive_layer=ch)
        assert_same(got, whole, ch + ' ', cols=np.array([7, 64, 129]))
        assert got['cape'][7] == 0.0 and got['cin'][129] == 0.0 and np.isnan(got['lfc_pressure'][64]) and got['lfc_index'][7] == -1
        one = xa.cape_cin_columns(*(np.ascontiguousarray(a[:, 3:4]) for a in (p, t, td)), parcel='most_unstable', positive_layer=ch)
        assert_same(one, {k: v[3:4] for k, v in got.items()}, ch + ' one column ')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_every_second_column_through_the_raw_abi(dtype):
    """Strided device views: the data in the even columns of arrays twice as wide (the odd ones hold a value that would show)."""
    p, t, td = (np.ascontiguousarray(a[:, :777]) for a in K.grid(K.MAIN, dtype))
    lib = L.init(0)
    nlev, ncol = p.shape
    xdt = L.XP_F64 if dtype == np.float64 else L.XP_F32
    wide = []
    for a in (p, t, td):
        w = np.full((nlev, 2 * ncol), 777.0, dtype=dtype)
        w[:, ::2] = a
        wide.append(_cuda(w)[0])
    views = [L.View(w.data_ptr(), xdt, L.XP_MEM_DEVICE, nlev, ncol, 2 * ncol, 2) for w in wide]
    names = ('cape', 'cin', 'lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature', 'lcl_pressure')
    ints = ('lfc_index', 'el_index', 'status')
    stream = torch.cuda.current_stream().cuda_stream
    for ch, mode in (('deepest', 'mixed_layer'), ('highest', 'surface')):
        want = xa.cape_cin_columns(p, t, td, parcel=mode, positive_layer=ch, want=names + ints)
        out = {k: torch.full((ncol,), -5.0, dtype=wide[0].dtype, device='cuda') for k in names}
        out.update({k: torch.full((ncol,), -5, dtype=torch.int32, device='cuda') for k in ints})
        so = L.ScalarsOut(dtype=xdt, mem=L.XP_MEM_DEVICE)
        for k, a in out.items():
            setattr(so, k, a.data_ptr())
        pc = L.Parcel(L.PARCEL[mode], 0, 100.0, None, None, None)
        o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST['exact'], L.XP_F64, L.HUMIDITY['dewpoint'], K.FLAGS[ch])
        rc = lib.xp_cape_cin(*[C.byref(v) for v in views], C.byref(pc), C.byref(o), C.byref(so), None, stream)
        assert rc == 0, lib.xp_last_error()
        torch.cuda.synchronize()
        assert_same(out, want, ch + ': ')


def test_specific_humidity_and_options():
    """XP_HUM_SPECIFIC is converted on load: the call is, within the restatement's tolerance, the dewpoint call on the library's
    own dewpoint_from_specific_humidity; post_zero_cin and the uncorrected temperatures reach the kernel."""
    p, t, td = K.grid(K.COMPOSE)
    with np.errstate(invalid='ignore'):
        e = 6.112 * np.exp(17.67 * (td - 273.15) / (td - 29.65))
        w = 0.6219569100577033 * e / (p - e)
    q = np.ascontiguousarray(w / (1.0 + w))
    d = xa.dewpoint_from_specific_humidity(p, t, q)
    for parcel, ch in (('surface', 'most_cape'), ('mixed_layer', 'highest')):
        got = xa.cape_cin_columns(p, t, q, parcel=parcel, humidity='specific', positive_layer=ch)
        want = xa.cape_cin_columns(p, t, d, parcel=parcel, positive_layer=ch)
        for k in R.FIELDS:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (parcel, k)
            ok = ~np.isnan(want[k])
            assert np.all(np.abs(got[k][ok] - want[k][ok]) <= 1e-6), (parcel, k, np.abs(got[k][ok] - want[k][ok]).max())
        assert np.array_equal(got['lfc_index'], want['lfc_index']) and np.array_equal(got['el_index'], want['el_index'])
    g = R.grid(p, t, td, vtc=False, parcel='surface', moist='rk4', lcl_interp='linear', post_zero_cin=True)
    kw = dict(virtual_temperature_correction=False, lcl_interp='linear', post_zero_cin=True)
    whole = xa.cape_cin_columns(p, t, td, **kw)
    for ch in K.CHOICES:
        compare(xa.cape_cin_columns(p, t, td, positive_layer=ch, **kw), g[ch], whole, g['oracle'], np.float64, 'options ' + ch)
    assert (g['K'] >= 2).sum() >= 10


# -- 5. what is rejected, with the outputs untouched --------------------------------------------------------------------------------
def _host_view(a, dtype=L.XP_F64):
    return L.View(a.ctypes.data, dtype, L.XP_MEM_HOST, a.shape[0], a.shape[1], a.shape[1], 1)


def test_rejections_leave_the_outputs_untouched():
    lib = L.init(0)
    p, t, td = (np.array(a[:, :40]) for a in K.grid())
    nlev, ncol = p.shape
    views = [_host_view(a) for a in (p, t, td)]
    vref = [C.byref(v) for v in views]
    outs = {k: np.full(ncol, -5.0) for k in ('cape', 'cin', 'lfc_pressure', 'el_pressure')}
    so = L.ScalarsOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    for k, a in outs.items():
        setattr(so, k, a.ctypes.data)
    prof = np.full((nlev + 1, ncol), -5.0)
    po = L.ProfileOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, nlev_out=nlev + 1, lev_stride=ncol, col_stride=1, temperature=prof.ctypes.data)
    other = np.full((nlev, ncol), -5.0)
    parcel = L.Parcel(L.PARCEL['surface'], 0, 100.0, None, None, None)
    opts = lambda **kw: L.Opts(**{**dict(virtual_temperature_correction=1, lcl_interp=1, pos_cape_neg_cin=1, post_zero_cin=0,
                                         moist_mode=L.MOIST['exact'], compute=L.XP_F64, humidity=0, flags=K.FLAGS['deepest']), **kw})

    def rejected(rc, *words):
        msg = lib.xp_last_error().decode()
        assert rc == XP_E_ARG, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert all((a == -5).all() for a in outs.values()) and (prof == -5).all() and (other == -5).all()

    cape = lambda o, profile=None: lib.xp_cape_cin(*vref, C.byref(parcel), C.byref(o), C.byref(so), profile, None)
    sos = (L.ScalarsOut * 2)(so, so)
    multi = lambda o, profiles=None: lib.xp_cape_cin_multi(*vref, 2, (L.Parcel * 2)(parcel, parcel), C.byref(o), sos, profiles, None)
    for value in (5, 6, 7):
        rejected(cape(opts(flags=value << 4)), 'XP_OPT_LAYER')
        rejected(multi(opts(flags=(value << 4) | L.OPT_FUSE_PARCELS)), 'XP_OPT_LAYER')
    rejected(cape(opts(pos_cape_neg_cin=0)), 'XP_OPT_LAYER', 'pos_cape_neg_cin')
    rejected(multi(opts(pos_cape_neg_cin=0)), 'XP_OPT_LAYER', 'pos_cape_neg_cin')
    rejected(cape(opts(), C.byref(po)), 'XP_OPT_LAYER', 'profile')
    rejected(multi(opts(), (L.ProfileOut * 2)(po, po)), 'XP_OPT_LAYER', 'profile')
    rejected(cape(opts(compute=L.XP_F32)), 'XP_OPT_LAYER', 'XP_F32')
    f32 = [np.ascontiguousarray(a, dtype=np.float32) for a in (p, t, td)]
    v32 = [C.byref(_host_view(a, L.XP_F32)) for a in f32]
    so32 = L.ScalarsOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST)
    cape32 = np.full(ncol, -5.0, dtype=np.float32)
    so32.cape = cape32.ctypes.data
    rejected(lib.xp_cape_cin(*v32, C.byref(parcel), C.byref(opts(compute=L.XP_F32, moist_mode=L.MOIST['family'])), C.byref(so32), None, None),
             'XP_OPT_LAYER', 'XP_F32')
    assert (cape32 == -5).all()
    # every other entry point that takes an xp_opts
    lo = L.CapeLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    lo.cape[0] = lo.total_cape = outs['cape'].ctypes.data
    top = np.full(ncol, 500.0)
    tops = (C.c_void_p * 1)(top.ctypes.data)
    rejected(lib.xp_cape_cin_layers(*vref, C.byref(parcel), C.byref(opts()), 1, None, tops, C.byref(lo), None), 'XP_OPT_LAYER')
    eo = L.EffectiveLayerOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, base_pressure=outs['cape'].ctypes.data, candidate_cape=other.ctypes.data)
    rejected(lib.xp_effective_inflow_layer(*vref, None, 100.0, -250.0, 300.0, C.byref(opts()), C.byref(eo), None), 'XP_OPT_LAYER')
    rejected(lib.xp_cape_cin_base(vref[0], vref[1], vref[2], outs['lfc_pressure'].ctypes.data, outs['el_pressure'].ctypes.data, C.byref(opts()),
                                  outs['cape'].ctypes.data, outs['cin'].ctypes.data, None), 'xp_cape_cin_base', 'XP_OPT_LAYER')
    ci = L.ConvIn(*[C.pointer(views[i]) for i in (0, 1, 2, 0, 1, 1, 0)], outs['lfc_pressure'].ctypes.data, outs['el_pressure'].ctypes.data)
    cout = L.ConvOut(mu_cape=outs['cape'].ctypes.data, mixed_100_cin=outs['cin'].ctypes.data)
    rejected(lib.xp_conv_properties(C.byref(ci), C.byref(opts()), 0, C.byref(cout), None), 'XP_OPT_LAYER')
    # and the same arguments with a valid field run
    assert cape(opts()) == 0, lib.xp_last_error()
    want = xa.cape_cin_columns(p, t, td, positive_layer='deepest', want=tuple(outs))
    assert_same(outs, want)
    for a in outs.values():
        a[:] = -5.0
    assert multi(opts(flags=K.FLAGS['deepest'] | L.OPT_FUSE_PARCELS, moist_mode=L.MOIST['family'])) == 0, lib.xp_last_error()
    assert_same(outs, want)
    with pytest.raises(L.XParcelError, match='profile'):
        xa.cape_cin_columns(p, t, td, positive_layer='lowest', want_profile=True)
    with pytest.raises(L.XParcelError, match='pos_cape_neg_cin'):
        xa.cape_cin_columns(p, t, td, positive_layer='lowest', pos_cape_neg_cin=False)
    # an empty grid: nothing written
    for a in outs.values():
        a[:] = -5.0
    empty = [C.byref(L.View(x.ctypes.data, L.XP_F64, L.XP_MEM_HOST, nlev, 0, 0, 1)) for x in (p, t, td)]
    assert lib.xp_cape_cin(*empty, C.byref(parcel), C.byref(opts()), C.byref(so), None, None) == 0, lib.xp_last_error()
    assert all((a == -5).all() for a in outs.values())


# -- 6. the Python spellings ------------------------------------------------------------------------------------------------------
def test_keyword_and_metpy_pairs_agree():
    p, t, td = (np.ascontiguousarray(a[:, :640]) for a in K.grid(K.MAIN, np.float32))
    default = xa.cape_cin_columns(p, t, td, parcel='mixed_layer')
    for (lfc, el), name in K.PAIRS.items():
        a = xa.cape_cin_columns(p, t, td, parcel='mixed_layer', positive_layer=name)
        b = xa.cape_cin_columns(p, t, td, parcel='mixed_layer', which_lfc=lfc, which_el=el)
        assert_same(b, a, name + ' ')
        if name == 'envelope':
            assert_same(a, default)
        else:
            assert (a['cape'] != default['cape']).sum() >= 20, name
        m = xa.cape_cin_multi(p, t, td, [('mixed_layer', 100)], which_lfc=lfc, which_el=el)
        assert_same(m, [a], name + ' multi ')
    for lfc, el in K.BAD_PAIRS:
        with pytest.raises(ValueError, match='which_lfc'):
            xa.cape_cin_columns(p, t, td, which_lfc=lfc, which_el=el)
    with pytest.raises(ValueError, match='not both'):
        xa.cape_cin_multi(p, t, td, ['surface'], positive_layer='deepest', which_lfc='wide', which_el='wide')


def test_dataarray_module_on_the_device():
    """xarray_parcel_amd/positive_layer.py end to end: a Dataset on the horizontal dims."""
    from xarray_parcel_amd import positive_layer
    from xarray_parcel_amd._xr import DataArray
    p, t, td = K.grid(K.MAIN, np.float32)
    nlev, ny, nx = p.shape[0], 30, 100
    hc = {'y': np.arange(ny), 'x': np.arange(nx)}
    lev = lambda a: DataArray(a.reshape(nlev, ny, nx).transpose(1, 0, 2), dims=('y', 'lev', 'x'), coords={**hc, 'lev': np.arange(nlev)})
    ds = positive_layer.cape_cin(lev(p), lev(t), lev(td), parcel='most_unstable', which_lfc='most_cape', which_el='most_cape', vert_dim='lev')
    want = xa.cape_cin_columns(p, t, td, parcel='most_unstable', positive_layer='most_cape', want=positive_layer.WANT)
    assert set(ds.keys()) == set(want)
    for k, v in want.items():
        assert ds[k].dims == ('y', 'x') and np.array_equal(np.asarray(ds[k].values), v.reshape(ny, nx), equal_nan=True), k
