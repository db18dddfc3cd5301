"""Grid-scale parity tests of the staged component kernels (run with -m gpu on an MI355X): k_lcl, k_dry_lapse,
k_moist_lapse, k_parcel_profile, k_lfc_el, k_cape_cin_base, k_select_parcel and k_mixed_layer of csrc/xp_kernels.hpp,
called through numpy_api, against the C oracle column by column on the inputs of tests/component_cases.py (whose CPU
guard, tests/test_component_cases_cpu.py, shows that the two CPU oracles agree on every one of them).

Shapes: 24 levels x 1337 columns (five full 256-thread blocks and a ragged one, a last wavefront with 7 idle lanes),
and every kernel once more on one column, on one level and on two levels.  Both dtypes throughout.

Tolerances (the project's, tests/test_gpu_parity.py): pressures 1e-7 hPa, temperatures 1e-7 K (dry_lapse, a closed
form: 1e-10 K), CAPE / CIN 1e-6 J/kg, indices, status words and NaN patterns identical.  float32 data: the oracle is fed
the float32-rounded inputs, its float64 result is rounded to float32, and the slack is 2e-7 * max(|b|, 1) + tolerance.
The staged pipeline against the fused kernel: 2e-6 J/kg and 2e-7 hPa / K -- each side is within 1e-6 / 1e-7 of the same
oracle.  Every comparison prints its largest error before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import component_cases as cc
from tests.test_gpu_parity import MODES, _saturated_tie_columns, oracle_tables  # noqa: F401  (oracle_tables: a fixture)

pytestmark = pytest.mark.gpu

xa = None
DTYPES = [np.float64, np.float32]
GRID = (cc.NLEV, cc.NCOL)
SHAPES = (GRID,) + cc.SMALL_SHAPES
MOIST = {'exact': 'rk4', 'table': 'table'}           # numpy_api's name of a moist mode -> the C oracle's


@pytest.fixture(scope='module', autouse=True)
def _api():
    global xa
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    xa = numpy_api
    yield


def _close(got, ref, dtype, ftol, what, keep=None):
    """NaN pattern identical, values within ftol (float32: after rounding the oracle's result, 2e-7 relative slack)."""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if keep is not None:
        a, b = a[..., keep], b[..., keep]
    if dtype == np.float32:
        b = b.astype(np.float32).astype(np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, 'NaN pattern', np.argwhere(np.isnan(a) != np.isnan(b))[:10])
    ok = ~np.isnan(b) & (a != b)
    tol = ftol if dtype == np.float64 else 2e-7 * np.maximum(np.abs(b[ok]), 1.0) + ftol
    err = np.abs(a[ok] - b[ok])
    print('%-60s max |diff| %.3e over %d values' % (what, err.max() if err.size else 0.0, int((~np.isnan(b)).sum())))
    assert np.all(err <= tol), (what, float(err.max()), np.argwhere(ok)[err > tol][:10])


def _table_mode(mode, request):
    if mode == 'table':
        request.getfixturevalue('oracle_tables')        # both sides look up the same arrays


def _with_oracle_mode(mode, fn):
    co.set_moist_lapse(MOIST[mode])
    try:
        return fn()
    finally:
        co.set_moist_lapse('rk4')


# ---- 1. lfc_el and cape_cin_base on crafted difference profiles --------------------------------------------------------
SCAN_KEYS = ('pressure', 'parcel', 'env', 'lcl_pressure', 'lcl_temperature')


@functools.lru_cache(maxsize=None)
def _scan(shape, dtype):
    """The profiles in `dtype`, the same values in float64, the oracle's lfc_el of those and the knife-edge columns."""
    s = cc.scan_profiles(*shape)
    g, o = {}, {}
    for k in SCAN_KEYS:
        g[k], o[k] = cc.cast(s[k], dtype)
    ref = cc.run_lfc_el(co, *(o[k] for k in SCAN_KEYS))
    knife = cc.knife_edge_columns(o['pressure'], o['parcel'], o['env'], o['lcl_pressure'])
    assert knife.sum() <= 0.02 * max(knife.size, 50)
    return g, o, ref, knife


def _check_lfc_el(got, ref, knife, dtype, what):
    """Indices identical outside the knife-edge columns (a crossing within 1e-9 of the LCL pressure, where the label --
    interval index or -2, 'replaced by the LCL' -- hangs on the last bit of exp / log); everything else everywhere."""
    for k in ('lfc_index', 'el_index'):
        bad = np.nonzero((np.asarray(got[k]) != ref[k]) & ~knife)[0]
        assert bad.size == 0, (what, k, bad[:10], np.asarray(got[k])[bad[:10]], ref[k][bad[:10]])
    print('%-60s %d knife-edge columns, %d labelled differently' % (what, int(knife.sum()), int(
        ((np.asarray(got['lfc_index']) != ref['lfc_index']) | (np.asarray(got['el_index']) != ref['el_index'])).sum())))
    assert np.array_equal(np.asarray(got['status']), ref['status_top_nan'].astype(np.int32)), (what, 'status')
    for k in cc.LFC_EL_FLOATS:
        _close(got[k], ref[k], dtype, 1e-7, '%s %s' % (what, k))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_lfc_el_vs_oracle(shape, dtype):
    g, o, ref, knife = _scan(shape, dtype)
    got = xa.lfc_el(*(g[k] for k in SCAN_KEYS))
    if shape == GRID:
        assert (ref['lfc_index'] == -2).sum() >= 20 and (ref['lfc_index'] >= 0).sum() >= 20 and (ref['el_index'] >= 0).sum() >= 20
        assert ref['status_top_nan'].sum() >= 20 and knife.sum() >= 5
    _check_lfc_el(got, ref, knife, dtype, 'lfc_el %s %s' % (shape, dtype.__name__))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('source', cc.BASE_SOURCES)
@pytest.mark.parametrize('shape', SHAPES)
def test_cape_cin_base_vs_oracle(shape, source, dtype):
    g, o, lfc_el, _ = _scan(shape, dtype)
    bounds = [cc.cast(x, dtype) for x in cc.base_bounds(o['pressure'], source, lfc_el)]
    for opts in cc.BASE_OPTIONS:
        got = xa.cape_cin_base(g['pressure'], g['env'], bounds[0][0], bounds[1][0], g['parcel'], **opts)
        ref = cc.run_cape_cin_base(co, o['pressure'], o['env'], o['parcel'], bounds[0][1], bounds[1][1], **opts)
        if shape == GRID:
            assert (ref['cape'] > 0).sum() >= 200 and (ref['cin'] != 0).sum() >= 200
        for k in ('cape', 'cin'):
            _close(got[k], ref[k], dtype, 1e-6, 'cape_cin_base %s %s %s %s %s' % (shape, source, dtype.__name__, opts, k))


# ---- 2. the point and lapse kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_lcl_vs_oracle(dtype):
    """1337 parcels as a 1-D and as a 2-D array, and some of them one at a time as scalars.  (numpy_api.lcl computes NumPy
    input in float64 whatever its dtype; float32 goes in as torch CPU tensors.)"""
    import torch
    parcels = cc.lcl_parcels()
    g, o = zip(*(cc.cast(parcels[k], dtype) for k in cc.PARCEL_KEYS))
    ref = cc.run_lcl(co, *o)
    assert (ref['lcl_pressure'] == o[0]).sum() >= 100 and np.isnan(ref['lcl_pressure']).sum() >= 100
    wrap = (lambda x: x) if dtype == np.float64 else torch.from_numpy
    got = xa.lcl(*(wrap(x) for x in g))
    got2 = xa.lcl(*(wrap(x.reshape(7, 191)) for x in g))
    for k in cc.LCL_KEYS:
        assert np.asarray(got[k]).dtype == dtype and np.asarray(got2[k]).shape == (7, 191)
        _close(got[k], ref[k], dtype, 1e-7, 'lcl 1-D %s %s' % (dtype.__name__, k))
        _close(np.asarray(got2[k]).reshape(-1), ref[k], dtype, 1e-7, 'lcl 2-D %s %s' % (dtype.__name__, k))
    if dtype == np.float64:
        for i in range(24):                                  # every kind of parcel, a NaN in each of the three inputs
            one = xa.lcl(float(g[0][i]), float(g[1][i]), float(g[2][i]))
            for k in cc.LCL_KEYS:
                assert np.shape(one[k]) == ()
                _close(np.reshape(one[k], (1,)), ref[k][i:i + 1], dtype, 1e-7, 'lcl scalar %d %s' % (i, k))


@functools.lru_cache(maxsize=None)
def _lapse(shape, dtype):
    case = cc.lapse_cases(*shape)
    g, o = {}, {}
    g['pressure'], o['pressure'] = cc.cast(case['pressure'], dtype)
    for v in ('none', 'scalar', 'array'):
        t0, pp = case[v]
        (gt, ot), (gp, op) = cc.cast(t0, dtype), cc.cast(pp, dtype)
        g[v], o[v] = (gt, gp if np.ndim(pp) else pp), (ot, op if np.ndim(pp) else pp)
    return g, o


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_dry_lapse_vs_oracle(shape, dtype):
    g, o = _lapse(shape, dtype)
    for v in ('none', 'scalar', 'array'):
        got = xa.dry_lapse(g['pressure'], *g[v])
        ref = cc.run_lapse(co.dry_lapse, o['pressure'], *o[v])
        _close(got, ref, dtype, 1e-10, 'dry_lapse %s %s parcel pressure: %s' % (shape, dtype.__name__, v))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', sorted(MOIST))
@pytest.mark.parametrize('shape', SHAPES)
def test_moist_lapse_vs_oracle(shape, mode, dtype, request):
    """Both marches: upwards from the reference pressure and, in reverse level order, downwards for the levels below it."""
    _table_mode(mode, request)
    g, o = _lapse(shape, dtype)
    for v in ('none', 'scalar', 'array'):
        got = xa.moist_lapse(g['pressure'], *g[v], moist=mode)
        ref = _with_oracle_mode(mode, lambda: cc.run_lapse(co.moist_lapse, o['pressure'], *o[v]))
        if shape == GRID:
            assert (~np.isnan(ref)).sum() >= (8000 if mode == 'exact' else 4000)
        _close(got, ref, dtype, 1e-7, 'moist_lapse %s %s %s parcel pressure: %s' % (shape, mode, dtype.__name__, v))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', sorted(MOIST))
@pytest.mark.parametrize('shape', SHAPES)
def test_parcel_profile_vs_oracle(shape, mode, dtype, request):
    _table_mode(mode, request)
    case = cc.parcel_profile_cases(*shape)
    keys = ('pressure', 'parcel_pressure', 'parcel_temperature', 'parcel_dewpoint')
    g, o = zip(*(cc.cast(case[k], dtype) for k in keys))
    got = xa.parcel_profile(*g, moist=mode)
    ref = _with_oracle_mode(mode, lambda: cc.run_parcel_profile(co, *o))
    if shape == GRID:
        on_level = (o[0] == ref['lcl_pressure'][None, :]).any(axis=0)
        assert on_level.sum() >= 100                                      # the P == LCL branch
    for k in ('temperature', 'virtual_temperature') + cc.LCL_KEYS:
        _close(got[k], ref[k], dtype, 1e-7, 'parcel_profile %s %s %s %s' % (shape, mode, dtype.__name__, k))


# ---- 3. parcel selection ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _select(shape, dtype):
    case = cc.select_cases(*shape)
    g, o = zip(*(cc.cast(case[k], dtype) for k in cc.PARCEL_KEYS))
    return g, o, ~np.isnan(case['tie_delta'])


def _check_most_unstable(shape, dtype, depth):
    g, o, tie = _select(shape, dtype)
    got = xa.most_unstable_parcel(*g, depth=depth)
    ref = cc.run_most_unstable(co, *o, depth)
    what = 'most_unstable_parcel %s %s depth %d' % (shape, dtype.__name__, depth)
    bad = np.nonzero(np.asarray(got['index']) != ref['index'])[0]
    assert bad.size == 0, (what, bad[:10], np.asarray(got['index'])[bad[:10]], ref['index'][bad[:10]])
    for k in cc.PARCEL_KEYS:
        _close(got[k], ref[k], dtype, 1e-7, '%s %s' % (what, k))
    return ref['index'][tie]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('depth', cc.MU_DEPTHS)
def test_most_unstable_parcel_vs_oracle(depth, dtype):
    """... including columns whose two best levels are 1e-7 ... 1e-4 apart in ln theta_e, either one leading: both sides of
    the window (2e-5) below which the float32 ranking is repeated in float64."""
    idx = _check_most_unstable(GRID, dtype, depth)
    assert min((idx == k).sum() for k in cc.TIE_LEVELS) >= 60 and set(idx) == set(cc.TIE_LEVELS)


def _check_mixed(shape, dtype, depth):
    g, o, _ = _select(shape, dtype)
    got = dict(xa.mixed_parcel(*g, depth=depth))
    got.update({'mean_' + k: v for k, v in xa.mixed_layer(dict(zip(cc.PARCEL_KEYS, g)), depth=depth).items()})
    ref = cc.run_mixed(co, *o, depth)
    assert set(got) == set(ref)
    for k in ref:
        _close(got[k], ref[k], dtype, 1e-7, 'mixed_parcel / mixed_layer %s %s depth %d %s' % (shape, dtype.__name__, depth, k))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('depth', cc.ML_DEPTHS)
def test_mixed_parcel_and_mixed_layer_vs_oracle(depth, dtype):
    _check_mixed(GRID, dtype, depth)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', cc.SMALL_SHAPES)
def test_parcel_selection_on_small_shapes(shape, dtype):
    for depth in cc.MU_DEPTHS:
        _check_most_unstable(shape, dtype, depth)
    for depth in cc.ML_DEPTHS:
        _check_mixed(shape, dtype, depth)


# ---- 4. the staged pipeline equals the fused kernel ------------------------------------------------------------------------
@pytest.mark.parametrize('mode', range(len(MODES)))
@pytest.mark.parametrize('parcel', ['surface', 'explicit'])
def test_staged_pipeline_equals_the_fused_kernel(parcel, mode):
    """parcel_profile_with_lcl -> lfc_el on the (virtual) temperatures cape_cin selects -> cape_cin_base, against
    cape_cin_columns of the same parcel.  The inserted LCL row has the LCL's own pressure: a crossing on it is the tie
    that _saturated_tie_columns classifies and bounds."""
    kw = MODES[mode]
    case = cc.pipeline_columns()
    p, t, td = (case[k] for k in cc.PARCEL_KEYS)
    pp, pt, ptd = case[parcel]
    fused = xa.cape_cin_columns(p, t, td, **(dict(parcel='surface') if parcel == 'surface' else
                                              dict(parcel='explicit', parcel_values=(pp, pt, ptd))), **kw)
    vtc = kw.get('virtual_temperature_correction', True)
    prof = xa.parcel_profile_with_lcl(p, t, td, pp, pt, ptd, lcl_interp=kw.get('lcl_interp', 'log'))
    par = prof['virtual_temperature' if vtc else 'temperature']
    env = prof['environment_virtual_temperature' if vtc else 'environment_temperature']
    staged = xa.lfc_el(prof['pressure'], par, env, prof['lcl_pressure'], prof['lcl_virtual_temperature' if vtc else 'lcl_temperature'])
    staged.update(xa.cape_cin_base(prof['pressure'], env, staged['lfc_pressure'], staged['el_pressure'], par,
                                   pos_cape_neg_cin=kw.get('pos_cape_neg_cin', True), post_zero_cin=kw.get('post_zero_cin', False)))
    staged['parcel_pressure'] = pp
    ref = {k: np.asarray(v) for k, v in fused.items()}
    for k in cc.LCL_KEYS:
        _close(prof[k], ref[k], np.float64, 2e-7, 'staged pipeline %s mode %d %s' % (parcel, mode, k))
    label_only, excluded = _saturated_tie_columns(staged, ref)
    keep = ~excluded
    what = 'staged pipeline %s mode %d' % (parcel, mode)
    print('%-60s %d label ties, %d sign ties, %d columns with CAPE' % (what, int(label_only.sum()), int(excluded.sum()), int((ref['cape'] > 0).sum())))
    assert (ref['cape'] > 0).sum() >= 300
    for k in ('lfc_index', 'el_index'):
        ok = keep & ~label_only if k == 'lfc_index' else keep
        bad = np.nonzero((staged[k] != ref[k]) & ok)[0]
        assert bad.size == 0, (what, k, bad[:10], staged[k][bad[:10]], ref[k][bad[:10]])
    assert np.array_equal(staged['status'][keep] & 9, ref['status'][keep] & 9), (what, 'status')
    for k in ('cape', 'cin'):
        _close(staged[k], ref[k], np.float64, 2e-6, '%s %s' % (what, k), keep)
    for k in cc.LFC_EL_FLOATS:
        _close(staged[k], ref[k], np.float64, 2e-7, '%s %s' % (what, k), keep)


# ---- 5. input kinds ------------------------------------------------------------------------------------------------------
def _xp_dtype(dtype):
    from xarray_parcel_amd import _lib as L
    return L.XP_F64 if dtype == np.float64 else L.XP_F32


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


@pytest.mark.parametrize('dtype', DTYPES)
def test_lfc_el_input_kinds(dtype):
    """Device tensors, and (ncol, nlev)-major device arrays through the raw ABI: bit-identical to the dense host call."""
    import torch
    from xarray_parcel_amd import _lib as L
    g, _, _, _ = _scan(GRID, dtype)
    dense = xa.lfc_el(*(g[k] for k in SCAN_KEYS))
    dev = xa.lfc_el(*(torch.from_numpy(g[k]).cuda() for k in SCAN_KEYS))
    torch.cuda.synchronize()
    for k in dense:
        assert dev[k].is_cuda and _same_bits(dev[k].cpu().numpy(), dense[k]), k
    nlev, ncol = GRID
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(g[k].T)).cuda() for k in SCAN_KEYS[:3]]          # (ncol, nlev)
    views = [L.View(x.data_ptr(), _xp_dtype(dtype), L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    lcl = [torch.from_numpy(g[k]).cuda() for k in SCAN_KEYS[3:]]
    so = L.ScalarsOut()
    so.dtype, so.mem = _xp_dtype(dtype), L.XP_MEM_DEVICE
    out = {k: torch.empty(ncol, dtype=torch.int32 if k in L.SCALAR_I else lcl[0].dtype, device='cuda') for k in dense}
    for k, v in out.items():
        setattr(so, k, v.data_ptr())
    L.check(lib.xp_lfc_el(C.byref(views[0]), C.byref(views[1]), C.byref(views[2]), lcl[0].data_ptr(), lcl[1].data_ptr(),
                          C.byref(so), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for k in dense:
        assert _same_bits(out[k].cpu().numpy(), dense[k]), k


@pytest.mark.parametrize('dtype', DTYPES)
def test_moist_lapse_input_kinds(dtype):
    import torch
    from xarray_parcel_amd import _lib as L
    g, _ = _lapse(GRID, dtype)
    p, (t0, ref) = g['pressure'], g['array']
    dense = xa.moist_lapse(p, t0, ref, moist='exact')
    assert (~np.isnan(dense)).sum() >= 8000
    dev = xa.moist_lapse(*(torch.from_numpy(x).cuda() for x in (p, t0, ref)), moist='exact')
    torch.cuda.synchronize()
    assert dev.is_cuda and _same_bits(dev.cpu().numpy(), dense)
    nlev, ncol = GRID
    lib = L.init(0)
    cols = torch.from_numpy(np.ascontiguousarray(p.T)).cuda()                                      # (ncol, nlev)
    view = L.View(cols.data_ptr(), _xp_dtype(dtype), L.XP_MEM_DEVICE, nlev, ncol, 1, nlev)
    dt0, dref = torch.from_numpy(t0).cuda(), torch.from_numpy(ref).cuda()
    out = torch.empty_like(cols)                                          # written with the strides of the pressure view
    L.check(lib.xp_moist_lapse(C.byref(view), dt0.data_ptr(), dref.data_ptr(), L.MOIST['exact'], out.data_ptr(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert _same_bits(out.cpu().numpy().T, dense)
