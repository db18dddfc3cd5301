"""Grid-scale parity tests of the array primitives (csrc/xp_primitives.hpp) and of the per-element and per-column kernels
k_wet_bulb, k_interp_level, k_interp_levels, k_crossing_level, k_mixing_ratio and k_dewpoint_from_q (csrc/xp_kernels.hpp)
on the inputs of tests/primitive_cases.py, whose CPU guard (tests/test_primitive_cases_cpu.py) shows that every class of
column is present, survives the rounding to float32 and is evaluated by the oracle.  Run with -m gpu on an MI355X.

(a), (b)  Every call through numpy_api against oracle/parcel_oracle.py column by column (wet bulb: the C oracle's lcl and
moist_lapse element by element), on 24 levels x 1337 columns (five full 256-thread blocks and a ragged one, a last
wavefront with idle lanes) and on one column, one level and two levels; float64 and float32; host arrays and device
tensors.  No column is left out of any comparison.
(c)  Strided device views through the raw C ABI -- column-major, padded rows, and views of one call that do not share
their strides -- bit-identical to the dense call, for every entry point of this tier and xp_dry_lapse / xp_moist_lapse;
host views with such strides are refused.

Comparison: tests/test_gpu_components.py::_close -- NaN pattern identical, float64 within the call's tolerance; float32:
the oracle is fed the float32-rounded inputs, its result is rounded to float32 and the slack is 2e-7 * max(|b|, 1) plus the
float64 tolerance.  The float64 tolerances are the ones these calls have in tests/test_gpu_primitives.py,
test_gpu_indices.py and test_gpu_parity.py: primitives 1e-12 relative (trapz: + 1e-13, get_layer 1e-13 relative); data
movement, masks, integer outputs, the kept-level mask and the increasing / decreasing split exact; the re-based parcel
1e-10 relative; interp1d 1e-14 relative + 1e-15; interp_level(s) 1e-10; crossing_level 1e-9 relative; mixing_ratio 1e-14
relative; dewpoint from q 1e-10 K; wet bulb 1e-8 K in exact mode and 1e-7 K in table mode (moist_lapse's in
test_gpu_components.py, both sides looking up the oracle's tables).  Every comparison prints its largest difference
before it asserts.

find_intersections with b = None: the y of a crossing with zero is zero, and what comes out is rounding residue; a
relative bound has nothing to hold on to there, so those three outputs are held to 1e-12 of the larger of the two
values the interval connects (see the test).

Largest differences measured on the MI355X (float64 / float32 after the oracle's result is rounded to float32; over all
shapes and both memory spaces; absolute, in the unit of the output):
    insert_level, shift_out_nans, bound_pressure, trapz, interp1d (both forms), crossing_level,
    the re-based profiles, every mask and index      0 / 0
    find_intersections                               1.1e-12 (of about 1e3 hPa) / 0;  y with b = None: 7.1e-14 / 7.1e-14
    trap_around_zeros                                2.6e-15 / 0
    get_layer                                        5.1e-13 / 0
    the re-based parcel                              1.1e-13 / 0
    interp_level                                     1.1e-13 / 0
    interp_levels                                    4.6e-11 (heights of about 1e4 m, in ln p) / 0
    mixing_ratio                                     8.7e-18 / 0
    dewpoint_from_specific_humidity                  5.7e-14 K / 0
    wet_bulb_temperature, exact mode                 8.2e-13 K / 0   (every kind of element, the new ones included)
    wet_bulb_temperature, table mode                 0 / 0           (1458 of 1841 elements inside the tables)
    strided views: all 294 outputs bit-identical to the dense call
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import parcel_oracle as po
from oracle import thermo as th
from tests import component_cases as cc
from tests import primitive_cases as pc
from tests.test_gpu_components import _close, oracle_tables  # noqa: F401  (oracle_tables: a fixture)

pytestmark = pytest.mark.gpu

xa = None
DTYPES = [np.float64, np.float32]
SPACES = ['host', 'device']
grid = pytest.mark.parametrize('shape', pc.SHAPES, ids=lambda s: '%dx%d' % s)
both = pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: d.__name__)
spaces = pytest.mark.parametrize('space', SPACES)


@pytest.fixture(scope='module', autouse=True)
def _api():
    global xa
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    xa = numpy_api
    yield


def _rclose(got, ref, dtype, what, rtol=0.0, atol=0.0):
    """_close with a tolerance of atol + rtol * |reference| per value (the reference after its rounding to `dtype`)."""
    a, b = np.asarray(_np(got), dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ftol = atol
    if (rtol or np.ndim(atol)) and a.shape == b.shape:
        if dtype == np.float32:
            b = b.astype(np.float32).astype(np.float64)
        ftol = (atol + rtol * np.abs(b))[~np.isnan(b) & (a != b)]      # for the values _close compares, in its order
    _close(a, ref, dtype, ftol, what)


def _same(got, ref, what):
    """Masks and integers: identical in every column."""
    g, r = _np(got), np.asarray(ref)
    assert g.shape == r.shape and np.array_equal(g, r), (what, g.shape, r.shape, np.argwhere(g != r)[:10] if g.shape == r.shape else None)


def _to(space, x):
    """The arguments of a call as host arrays or as device tensors."""
    import torch
    if isinstance(x, dict):
        return {k: _to(space, v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to(space, v) for v in x)
    return torch.as_tensor(x).cuda() if space == 'device' and isinstance(x, np.ndarray) else x


def _np(x):
    import torch
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_np(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _is(space, x):
    """Results live where the inputs live."""
    import torch
    assert (torch.is_tensor(x) and x.is_cuda) if space == 'device' else isinstance(x, np.ndarray), (space, type(x))


@functools.lru_cache(maxsize=None)
def _case(builder, shape, dtype, **kw):
    """(what the kernel is given, the same values in float64) of one builder of tests/primitive_cases.py."""
    case = getattr(pc, builder)(*shape, **kw)
    g, o = {}, {}
    for k, v in case.items():
        if isinstance(v, tuple):
            g[k], o[k] = (tuple(x) for x in zip(*(cc.cast(a, dtype) for a in v)))
        elif isinstance(v, np.ndarray) and v.dtype.kind == 'f':
            g[k], o[k] = cc.cast(v, dtype)
        else:
            g[k] = o[k] = v
    return g, o


def _tag(*parts):
    return ' '.join(p.__name__ if isinstance(p, type) else str(p) for p in parts)


# ---- insert_level ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_insert_level(shape, dtype):
    return pc.ref_insert_level(_case('insert_level_cases', shape, dtype)[1])


@grid
@both
@spaces
def test_insert_level(shape, dtype, space):
    g = _to(space, _case('insert_level_cases', shape, dtype)[0])
    got = xa.insert_level({k: g[k] for k in pc.DATASET}, {k: g['level_' + k] for k in pc.DATASET}, coords='pressure')
    ref = _ref_insert_level(shape, dtype)
    for k in pc.DATASET:
        _is(space, got[k])
        assert tuple(got[k].shape) == (shape[0] + 1, shape[1])
        _rclose(got[k], ref[k], dtype, _tag('insert_level', shape, dtype, space, k))          # pure data movement: exact


# ---- find_intersections ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_find_intersections(shape, dtype, log_x, with_b):
    o = _case('crossing_profiles', shape, dtype)[1]
    return pc.ref_find_intersections(o['x'], o['a'] if with_b else o['diff'], o['b'] if with_b else None, log_x)


@grid
@both
@spaces
@pytest.mark.parametrize('log_x', [False, True])
@pytest.mark.parametrize('with_b', [True, False])
def test_find_intersections(shape, dtype, space, log_x, with_b):
    """With one level: six arrays of zero rows, nothing read or written."""
    g = _to(space, _case('crossing_profiles', shape, dtype)[0])
    got = xa.find_intersections(g['x'], g['a'], g['b'], log_x=log_x) if with_b else xa.find_intersections(g['x'], g['diff'], None, log_x=log_x)
    ref = _ref_find_intersections(shape, dtype, log_x, with_b)
    assert set(got) == set(ref) and len(got) == 6
    # b = None: the y of a crossing is mathematically zero, what is computed is the rounding residue of
    # ((ix - x0) / (x1 - x0)) * (a1 - a0) + a0, of the size of one ulp of ix (the last bit of the library's log) times
    # |x| / |x1 - x0| times |a1 - a0|: there is no value for a relative bound to hold on to, so the bound is 1e-12 of
    # the operands a0, a1 instead (measured: 7.1e-14 K with log_x, 0 without)
    a = _case('crossing_profiles', shape, dtype)[1]['diff']
    with np.errstate(invalid='ignore'):
        scale = np.fmax(np.abs(a[:-1]), np.abs(a[1:]))
    scale = np.where(np.isnan(scale), 0.0, scale)
    for k in ref:
        _is(space, got[k])
        assert tuple(got[k].shape) == (shape[0] - 1, shape[1])
        _rclose(got[k], ref[k], dtype, _tag('find_intersections', shape, dtype, space, 'log_x' if log_x else 'lin_x', 'b' if with_b else 'b=None', k),
                rtol=1e-12, atol=1e-12 * scale if k.endswith('_y') and not with_b else 0.0)
    # the increasing / decreasing split: exact in every column, whatever the values
    a = _np(got)
    for side in ('increasing', 'decreasing'):
        assert np.array_equal(np.isnan(a[side + '_x']), np.isnan(ref[side + '_x'])) and np.array_equal(np.isnan(a[side + '_y']), np.isnan(ref[side + '_y']))


# ---- trapz -------------------------------------------------------------------------------------------------------------------
TRAPZ_OPTS = (dict(), dict(only_positive=True), dict(only_negative=True))


@functools.lru_cache(maxsize=None)
def _ref_trapz(shape, dtype, i, masked):
    o = _case('trapz_cases', shape, dtype)[1]
    return pc.ref_trapz(o['dat'], o['x'], o['mask'] if masked else None, **TRAPZ_OPTS[i])


@grid
@both
@spaces
def test_trapz(shape, dtype, space):
    g = _to(space, _case('trapz_cases', shape, dtype)[0])
    for i, kw in enumerate(TRAPZ_OPTS):
        for masked in (False, True):
            got = xa.trapz(g['dat'], g['x'], mask=g['mask'] if masked else None, **kw)
            _is(space, got)
            ref = _ref_trapz(shape, dtype, i, masked)
            if shape[0] == 1:
                assert np.all(_np(got) == 0.0)
            _rclose(got, ref, dtype, _tag('trapz', shape, dtype, space, kw, 'mask' if masked else 'no mask'), rtol=1e-12, atol=1e-13)


# ---- trap_around_zeros -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_trap_around_zeros(shape, dtype, log_x):
    o = _case('crossing_profiles', shape, dtype)[1]
    return pc.ref_trap_around_zeros(o['x'], o['diff'], log_x)


@grid
@both
@spaces
@pytest.mark.parametrize('log_x', [True, False])
def test_trap_around_zeros(shape, dtype, space, log_x):
    """With one level: one all-NaN row and a mask of ones."""
    g = _to(space, _case('crossing_profiles', shape, dtype)[0])
    areas, mask = xa.trap_around_zeros(g['x'], g['diff'], log_x=log_x)
    ref, rmask = _ref_trap_around_zeros(shape, dtype, log_x)
    assert set(areas) == set(ref)
    for k in ('area', 'dx', 'x', 'x_from', 'x_to'):
        _is(space, areas[k])
        assert tuple(areas[k].shape) == (2 * shape[0] - 1, shape[1])
        _rclose(areas[k], ref[k], dtype, _tag('trap_around_zeros', shape, dtype, space, 'log_x' if log_x else 'lin_x', k), rtol=1e-12)
    m = _np(mask)
    assert m.dtype == bool
    _same(m, rmask, 'trap_around_zeros mask')
    if shape[0] == 1:
        assert m.all() and all(np.isnan(_np(v)).all() for v in areas.values())


# ---- bound_pressure / get_layer ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_layer(shape, dtype, what, *args):
    o = _case('layer_cases', shape, dtype)[1]
    if what == 'bound':
        return pc.ref_bound_pressure(o['pressure'], o['bound'] if args[0] is None else args[0])
    return pc.ref_get_layer(o, *args)


@grid
@both
@spaces
def test_bound_pressure(shape, dtype, space):
    g = _to(space, _case('layer_cases', shape, dtype)[0])
    for bound, name in ((g['bound'], None), (700.0, 700.0)):
        got = xa.bound_pressure(g['pressure'], bound)
        _is(space, got)
        _rclose(got, _ref_layer(shape, dtype, 'bound', name), dtype, _tag('bound_pressure', shape, dtype, space, name))      # a level's pressure: exact


@grid
@both
@spaces
@pytest.mark.parametrize('interpolate', [True, False])
def test_get_layer(shape, dtype, space, interpolate):
    g = _to(space, _case('layer_cases', shape, dtype)[0])
    for depth in pc.LAYER_DEPTHS:
        got = xa.get_layer({k: g[k] for k in pc.DATASET}, depth=depth, interpolate=interpolate)
        ref = _ref_layer(shape, dtype, 'layer', depth, interpolate)
        for k in pc.DATASET:
            _is(space, got[k])
            assert tuple(got[k].shape) == (shape[0] + (1 if interpolate else 0), shape[1])
            _rclose(got[k], ref[k], dtype, _tag('get_layer', shape, dtype, space, depth, 'interpolate' if interpolate else 'nearest', k), rtol=1e-13)


# ---- shift_out_nans ----------------------------------------------------------------------------------------------------------
@grid
@both
@spaces
def test_shift_out_nans(shape, dtype, space):
    g, o = _case('shift_cases', shape, dtype)
    got = xa.shift_out_nans(_to(space, {k: g[k] for k in ('pressure', 'temperature')}), 'pressure')
    ref = pc.shift_reference({k: o[k] for k in ('pressure', 'temperature')}, 'pressure')
    for k in ref:
        _is(space, got[k])
        _rclose(got[k], ref[k], dtype, _tag('shift_out_nans', shape, dtype, space, k))       # pure data movement: exact


# ---- from_most_unstable_parcel / mix_layer -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_rebase(shape, dtype, mode):
    o = _case('rebase_cases', shape, dtype)[1]
    return pc.rebase_reference(o['pressure'], o['temperature'], o['dewpoint'], mode)


@pytest.mark.parametrize('shape', (pc.GRID, cc.SMALL_SHAPES[0]), ids=lambda s: '%dx%d' % s)
@both
@spaces
@pytest.mark.parametrize('mode', sorted(pc.REBASE))
def test_rebased_profiles(shape, dtype, space, mode):
    g = _to(space, _case('rebase_cases', shape, dtype)[0])
    fn = xa.from_most_unstable_parcel if mode == 'most_unstable' else xa.mix_layer
    rp, rt, rtd, parcel, kept = fn(g['pressure'], g['temperature'], g['dewpoint'], depth=pc.REBASE[mode])
    cols, rparcel, rkept = _ref_rebase(shape, dtype, mode)
    what = _tag(mode, shape, dtype, space)
    assert isinstance(kept, np.ndarray) and kept.dtype == bool
    _same(kept, rkept, what + ' kept levels')
    assert (~rkept).any()
    if mode == 'most_unstable':
        _same(parcel['index'], rparcel['index'], what + ' parcel index')
    for k in pc.DATASET:
        _rclose(parcel[k], rparcel[k], dtype, what + ' parcel ' + k, rtol=1e-10)
    first = 1 if mode == 'mixed_layer' else 0                                   # row 0 of mix_layer is the parcel again
    for k, got in zip(pc.DATASET, (rp, rt, rtd)):
        _is(space, got)
        assert tuple(got.shape) == cols[k].shape
        _rclose(_np(got)[first:], cols[k][first:], dtype, what + ' ' + k)     # pure data movement: exact
        if first:
            _rclose(_np(got)[0], rparcel[k], dtype, what + ' row 0 ' + k, rtol=1e-10)
            assert np.array_equal(_np(got)[0], _np(parcel[k]))


# ---- interp1d ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _interp1d(dtype):
    case = pc.interp1d_cases()
    g, o = zip(*(cc.cast(case[k], dtype) for k in ('at', 'xp', 'fp', 'at_shared', 'xp_shared')))
    return g, pc.ref_interp1d(o[0], o[1], o[2]), pc.ref_interp1d(o[3], o[4], o[2])


@both
@spaces
def test_interp1d(dtype, space):
    """One set of points per column, and one for all columns (the col_stride 0 form)."""
    (at, xp, fp, at_s, xp_s), ref, ref_shared = _interp1d(dtype)
    got = xa.interp1d(*_to(space, (at, xp, fp)))
    _is(space, got)
    _rclose(got, ref, dtype, _tag('interp1d', dtype, space), rtol=1e-14, atol=1e-15)
    got = xa.interp1d(*_to(space, (at_s, xp_s, fp)))
    _rclose(got, ref_shared, dtype, _tag('interp1d shared xp', dtype, space), rtol=1e-14, atol=1e-15)


# ---- interp_level / interp_levels ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_level(shape, dtype, log, var, at):
    """Variable `var` at the per-column coordinate (at None) or at the scalar `at`."""
    o = _case('level_cases', shape, dtype)[1]
    return pc.ref_interp_level(o['coords'], o['variables'][var], o['at'] if at is None else at, log)


@grid
@both
@spaces
@pytest.mark.parametrize('log', [False, True])
def test_interp_level(shape, dtype, space, log):
    g = _to(space, _case('level_cases', shape, dtype)[0])
    for at, name in ((g['at'], None), (pc.LEVEL_TARGET, pc.LEVEL_TARGET)):
        got = xa.interp_level(g['coords'], g['variables'][0], at, log=log)
        _is(space, got)
        _rclose(got, _ref_level(shape, dtype, log, 0, name), dtype,
                _tag('interp_level', shape, dtype, space, 'log' if log else 'linear', 'per column' if name is None else name), atol=1e-10)


@grid
@both
@spaces
@pytest.mark.parametrize('log', [False, True])
def test_interp_levels(shape, dtype, space, log):
    """1 ... 4 variables at 1 ... 4 coordinates (one of them twice): each of the sixteen instantiations against the
    oracle's interpolation of that variable at that coordinate -- not against k_interp_level."""
    g = _to(space, _case('level_cases', shape, dtype)[0])
    for nv in range(1, 5):
        for nt in range(1, 5):
            ats = pc.LEVEL_TARGETS[4 - nt:] if nv % 2 else pc.LEVEL_TARGETS[:nt]
            got = xa.interp_levels(g['coords'], list(g['variables'][:nv]), list(ats), log=log)
            assert len(got) == nv and all(len(row) == nt for row in got)
            for v in range(nv):
                for j, at in enumerate(ats):
                    _is(space, got[v][j])
                    ref = _ref_level(shape, dtype, log, v, at)
                    _rclose(got[v][j], ref, dtype, _tag('interp_levels', shape, dtype, space, 'log' if log else 'linear', nv, 'x', nt, 'var', v, 'at', at), atol=1e-10)


# ---- crossing_level ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_crossing(shape, dtype, value, increasing):
    o = _case('crossing_cases', shape, dtype, value=value, increasing=increasing)[1]
    return pc.crossing_reference(o['x'], o['a'], value)


@grid
@both
@spaces
@pytest.mark.parametrize('value', pc.CROSSING_VALUES)
@pytest.mark.parametrize('increasing', [True, False], ids=['height', 'pressure'])
def test_crossing_level(shape, dtype, space, value, increasing):
    g = _to(space, _case('crossing_cases', shape, dtype, value=value, increasing=increasing)[0])
    got = xa.crossing_level(g['x'], g['a'], value)
    _is(space, got)
    _rclose(got, _ref_crossing(shape, dtype, value, increasing), dtype,
            _tag('crossing_level', shape, dtype, space, value, 'height' if increasing else 'pressure'), rtol=1e-9)


# ---- wet_bulb_temperature ------------------------------------------------------------------------------------------------------
WET_BULB_TOL = {'exact': 1e-8, 'table': 1e-7}


@functools.lru_cache(maxsize=None)
def _ref_wet_bulb(dtype, mode):
    e = pc.wet_bulb_elements()
    g, o = zip(*(cc.cast(e[k], dtype) for k in pc.DATASET))
    co.set_moist_lapse({'exact': 'rk4', 'table': 'table'}[mode])
    try:
        return g, pc.wet_bulb_reference(co, *o), e['kind']
    finally:
        co.set_moist_lapse('rk4')


@pytest.mark.parametrize('layout', pc.WET_BULB_LAYOUTS, ids=lambda s: '%dx%d' % s)
@both
@spaces
@pytest.mark.parametrize('mode', ['exact', 'table'])
def test_wet_bulb_temperature(layout, dtype, space, mode, request):
    """Every kind of element of the builder, those that take lcl_reference behind the wave ballot in the same wavefront
    as those that do not, and the saturated ones (the p == l.p branch)."""
    if mode == 'table':
        request.getfixturevalue('oracle_tables')        # both sides look up the same arrays
    g, ref, kind = _ref_wet_bulb(dtype, mode)
    got = xa.wet_bulb_temperature(*_to(space, tuple(x.reshape(layout) for x in g)), moist=mode)
    _is(space, got)
    assert tuple(got.shape) == layout
    a = _np(got).reshape(-1).astype(np.float64)
    for i, name in enumerate(pc.WET_BULB_KINDS):
        sel = (kind == i) & ~np.isnan(ref) & ~np.isnan(a)
        print('%-44s %-16s max |diff| %.3e' % (_tag('wet_bulb', layout, dtype, space, mode), name,
                                              np.max(np.abs(a[sel] - ref[sel]), initial=0.0)))
    _rclose(a, ref, dtype, _tag('wet_bulb_temperature', layout, dtype, space, mode), atol=WET_BULB_TOL[mode])


# ---- mixing_ratio / dewpoint_from_specific_humidity ------------------------------------------------------------------------------
@grid
@both
@spaces
def test_mixing_ratio_and_dewpoint_from_specific_humidity(shape, dtype, space):
    g, o = _case('humidity_cases', shape, dtype)
    g = _to(space, g)
    with np.errstate(all='ignore'):
        ref_w = po.mixing_ratio(o['temperature'], o['dewpoint'], o['pressure'])
        ref_td = th.dewpoint_from_specific_humidity(o['pressure'], o['temperature'], o['specific_humidity'])
    got = xa.mixing_ratio(g['temperature'], g['dewpoint'], g['pressure'])
    _is(space, got)
    _rclose(got, ref_w, dtype, _tag('mixing_ratio', shape, dtype, space), rtol=1e-14)
    got = xa.dewpoint_from_specific_humidity(g['pressure'], g['temperature'], g['specific_humidity'])
    _is(space, got)
    _rclose(got, ref_td, dtype, _tag('dewpoint_from_specific_humidity', shape, dtype, space), atol=1e-10)


# ---- (c) strided device views through the raw C ABI ------------------------------------------------------------------------------
RAW_SHAPE = (24, 1000)
SENTINEL = -12345.0
LAYOUTS = ('column_major', 'padded', 'mixed')


class _Raw:
    """One raw-ABI call: device views in a layout, dense outputs, and outputs that take the layout of a view.
    column_major: (ncol, nlev) tensors, lev_stride 1, col_stride nlev; padded: the first ncol columns of a
    (nlev, ncol + 3) tensor, lev_stride ncol + 3, col_stride 1; mixed: the first view of the call dense, the others
    column-major.  Every buffer is sized from its rows and columns here, and filled with SENTINEL beforehand."""

    def __init__(self, layout, dtype):
        import torch
        from xarray_parcel_amd import _lib as L
        self.torch, self.L, self.layout, self.dtype = torch, L, layout, dtype
        self.tdt = torch.float64 if dtype == np.float64 else torch.float32
        self.xp = L.XP_F64 if dtype == np.float64 else L.XP_F32
        self.lib = L.init(0)
        self.nviews, self.keep, self.layout_of = 0, [], {}

    def _layout(self):
        lay = self.layout
        if lay == 'mixed':
            lay = 'dense' if self.nviews == 0 else 'column_major'
        self.nviews += 1
        return lay

    def _buffer(self, lay, rows, ncol, values=None):
        """(tensor, lev_stride, col_stride, the (rows, ncol) window of it)."""
        t = self.torch
        if lay == 'dense':
            buf = t.full((rows, ncol), SENTINEL, dtype=self.tdt, device='cuda')
            win, ls, cs = buf, ncol, 1
        elif lay == 'column_major':
            buf = t.full((ncol, rows), SENTINEL, dtype=self.tdt, device='cuda')
            win, ls, cs = buf.T, 1, rows
        else:
            buf = t.full((rows, ncol + 3), SENTINEL, dtype=self.tdt, device='cuda')
            win, ls, cs = buf[:, :ncol], ncol + 3, 1
        if values is not None:
            win.copy_(t.from_numpy(values).cuda())
        return buf, ls, cs, win

    def view(self, x, lay=None):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(self.dtype))
        rows, ncol = a.shape
        lay = lay or self._layout()
        buf, ls, cs, _ = self._buffer(lay, rows, ncol, a)
        self.keep.append(buf)
        v = self.L.View(buf.data_ptr(), self.xp, self.L.XP_MEM_DEVICE, rows, ncol, ls, cs)
        self.layout_of[buf.data_ptr()] = (lay, rows, ncol)
        return v

    def col(self, x):
        a = self.torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(self.dtype))).cuda()
        self.keep.append(a)
        return a

    def dense(self, rows, ncol, dtype=None):
        return self.torch.full((rows, ncol), 57 if dtype else SENTINEL, dtype=dtype or self.tdt, device='cuda')

    def like(self, view):
        """An output with the layout of `view`, of that view's full extent: read back through the same strides, the padding
        must still hold the sentinel."""
        lay, rows, ncol = self.layout_of[view.data]
        buf, _, _, win = self._buffer(lay, rows, ncol)

        def read():
            if lay == 'padded':
                assert bool((buf[:, ncol:] == SENTINEL).all()), 'the padding of an out_like output was written'
            return win.cpu().numpy().copy()
        buf.read = read
        return buf

    def call(self, name, *args):
        t = self.torch
        args = [a.data_ptr() if t.is_tensor(a) else a for a in args]
        self.L.check(getattr(self.lib, name)(*args, C.c_void_p(t.cuda.current_stream().cuda_stream)))
        t.cuda.synchronize()

    def ptrs(self, tensors):
        return (C.c_void_p * len(tensors))(*[x.data_ptr() for x in tensors])


@functools.lru_cache(maxsize=None)
def _raw_data():
    nlev, ncol = RAW_SHAPE
    d = {'layer': pc.layer_cases(nlev, ncol), 'cross': pc.crossing_profiles(nlev, ncol), 'trapz': pc.trapz_cases(nlev, ncol),
         'shift': pc.shift_cases(nlev, ncol), 'rebase': pc.rebase_cases(nlev, ncol), 'interp1d': pc.interp1d_cases(ncol=ncol),
         'level': pc.level_cases(nlev, ncol), 'crossing': pc.crossing_cases(nlev, ncol), 'humidity': pc.humidity_cases(nlev, ncol),
         'insert': pc.insert_level_cases(nlev, ncol)}
    return d


def _np_out(xs):
    return [x.read() if hasattr(x, 'read') else x.cpu().numpy() for x in xs]


def _e_insert_level(h, d):
    i = d['insert']
    out = h.dense(RAW_SHAPE[0] + 1, RAW_SHAPE[1])
    h.call('xp_insert_level', h.view(i['pressure']), h.view(i['temperature']), h.col(i['level_pressure']), h.col(i['level_temperature']),
           pc.FILL, out)
    return [out]


def _e_find_intersections(h, d):
    c = d['cross']
    outs = [h.dense(RAW_SHAPE[0] - 1, RAW_SHAPE[1]) for _ in range(6)]
    h.call('xp_find_intersections', h.view(c['x']), h.view(c['a']), h.view(c['b']), 1, h.ptrs(outs))
    return outs


def _e_trapz(h, d):
    z = d['trapz']
    mask = h.torch.from_numpy(np.ascontiguousarray(z['mask'].astype(np.uint8))).cuda()       # dense (nlev - 1, ncol) bytes
    out = h.dense(1, RAW_SHAPE[1])
    h.call('xp_trapz', h.view(z['dat']), h.view(z['x']), mask, 0, 0, out)
    return [out]


def _e_trap_around_zeros(h, d):
    c = d['cross']
    outs = [h.dense(2 * RAW_SHAPE[0] - 1, RAW_SHAPE[1]) for _ in range(5)]
    mask = h.dense(RAW_SHAPE[0], RAW_SHAPE[1], h.torch.uint8)
    h.call('xp_trap_around_zeros', h.view(c['x']), h.view(c['diff']), 1, h.ptrs(outs), mask)
    return outs + [mask]


def _e_bound_pressure(h, d):
    out = h.dense(1, RAW_SHAPE[1])
    h.call('xp_bound_pressure', h.view(d['layer']['pressure']), h.col(d['layer']['bound']), out)
    return [out]


def _e_get_layer(h, d):
    outs = []
    for interpolate in (1, 0):
        out = h.dense(RAW_SHAPE[0] + interpolate, RAW_SHAPE[1])
        h.nviews = 0
        h.call('xp_get_layer', h.view(d['layer']['pressure']), h.view(d['layer']['temperature']), 100.0, interpolate, 0, out)
        outs.append(out)
    return outs


def _e_shift_out_nans(h, d):
    out = h.dense(*RAW_SHAPE)
    h.call('xp_shift_out_nans', h.view(d['shift']['pressure']), h.view(d['shift']['temperature']), out)
    return [out]


def _e_rebase_profile(h, d):
    L, r = h.L, d['rebase']
    res = []
    for mode, extra in (('most_unstable', 0), ('mixed_layer', 1)):
        h.nviews = 0
        outs = [h.dense(RAW_SHAPE[0] + extra, RAW_SHAPE[1]) for _ in range(3)]
        par = [h.dense(1, RAW_SHAPE[1]) for _ in range(3)]
        idx = h.dense(1, RAW_SHAPE[1], h.torch.int32)
        so = L.ScalarsOut(dtype=h.xp, mem=L.XP_MEM_DEVICE)
        for k, a in zip(L.SCALAR_P + ('parcel_index',), par + [idx]):
            setattr(so, k, a.data_ptr())
        kept = np.zeros(RAW_SHAPE[0], dtype=np.int32)
        nout = C.c_int64(0)
        h.call('xp_rebase_profile', h.view(r['pressure']), h.view(r['temperature']), h.view(r['dewpoint']),
               L.Parcel(L.PARCEL[mode], 0, float(pc.REBASE[mode]), None, None, None), *outs, so, kept.ctypes.data, C.byref(nout))
        assert nout.value == int((kept != 0).sum()) + extra
        res += [o[:nout.value] for o in outs] + par + [idx, h.torch.from_numpy(kept)]
    return res


def _e_interp1d(h, d):
    i = d['interp1d']
    res = []
    for xp in (i['xp'], i['xp_shared'][:, None]):
        h.nviews = 0
        out = h.dense(i['at'].shape[0], RAW_SHAPE[1])
        h.call('xp_interp1d', h.view(i['at'] if xp.shape[1] > 1 else i['at_shared']), h.view(xp, 'dense' if xp.shape[1] == 1 else None),
               h.view(i['fp']), out)
        res.append(out)
    return res


def _e_interp_level(h, d):
    lv = d['level']
    out = h.dense(1, RAW_SHAPE[1])
    h.call('xp_interp_level', h.view(lv['coords']), h.view(lv['variables'][0]), h.col(lv['at']), 0, 1, out)
    return [out]


def _e_interp_levels(h, d):
    lv = d['level']
    cv = h.view(lv['coords'])
    views = [h.view(v) for v in lv['variables'][:3]]
    outs = [h.dense(1, RAW_SHAPE[1]) for _ in range(3 * 2)]
    vptrs = (C.POINTER(h.L.View) * 3)(*[C.pointer(v) for v in views])
    h.call('xp_interp_levels', cv, 3, vptrs, 2, (C.c_double * 2)(850.0, pc.LEVEL_TARGET), 0, h.ptrs(outs))
    return outs


def _e_crossing_level(h, d):
    out = h.dense(1, RAW_SHAPE[1])
    h.call('xp_crossing_level', h.view(d['crossing']['x']), h.view(d['crossing']['a']), 273.15, out)
    return [out]


def _e_wet_bulb_temperature(h, d):
    s = d['humidity']
    p = h.view(s['pressure'])
    out = h.like(p)
    h.call('xp_wet_bulb_temperature', p, h.view(s['temperature']), h.view(s['dewpoint']), h.L.MOIST['exact'], out)
    return [out]


def _e_mixing_ratio(h, d):
    s = d['humidity']
    t = h.view(s['temperature'])
    out = h.like(t)
    h.call('xp_mixing_ratio', t, h.view(s['dewpoint']), h.view(s['pressure']), out)
    return [out]


def _e_dewpoint_from_specific_humidity(h, d):
    s = d['humidity']
    p = h.view(s['pressure'])
    out = h.like(p)
    h.call('xp_dewpoint_from_specific_humidity', p, h.view(s['temperature']), h.view(s['specific_humidity']), out)
    return [out]


def _lapse(name, *mode):
    def entry(h, d):
        lay = d['layer']
        p = h.view(lay['pressure'])
        out = h.like(p)
        t0 = np.where(np.isnan(lay['temperature'][0]), 285.0, lay['temperature'][0])
        h.call(name, p, h.col(t0), h.col(np.full(RAW_SHAPE[1], 900.0)), *[h.L.MOIST[m] for m in mode], out)
        return [out]
    return entry


RAW_ENTRIES = {'xp_insert_level': _e_insert_level, 'xp_find_intersections': _e_find_intersections, 'xp_trapz': _e_trapz,
               'xp_trap_around_zeros': _e_trap_around_zeros, 'xp_bound_pressure': _e_bound_pressure, 'xp_get_layer': _e_get_layer,
               'xp_shift_out_nans': _e_shift_out_nans, 'xp_rebase_profile': _e_rebase_profile, 'xp_interp1d': _e_interp1d,
               'xp_interp_level': _e_interp_level, 'xp_interp_levels': _e_interp_levels, 'xp_crossing_level': _e_crossing_level,
               'xp_wet_bulb_temperature': _e_wet_bulb_temperature, 'xp_mixing_ratio': _e_mixing_ratio,
               'xp_dewpoint_from_specific_humidity': _e_dewpoint_from_specific_humidity,
               'xp_dry_lapse': _lapse('xp_dry_lapse'), 'xp_moist_lapse': _lapse('xp_moist_lapse', 'exact')}


@functools.lru_cache(maxsize=None)
def _raw_dense(entry, dtype):
    return _np_out(RAW_ENTRIES[entry](_Raw('dense', dtype), _raw_data()))


@pytest.mark.parametrize('entry', sorted(RAW_ENTRIES))
@both
def test_strided_device_views_through_the_raw_abi(entry, dtype):
    """include/xparcel.h promises general element strides for every view: each layout gives the dense call's bits.  The
    primitives write dense outputs whatever the strides of their inputs; the element-wise kernels and the two lapse
    kernels write through the strides of their first view, and nowhere else."""
    dense = _raw_dense(entry, dtype)
    assert any(np.isfinite(x.astype(np.float64)).any() and not np.all(x == SENTINEL) for x in dense), 'the dense call wrote nothing'
    for layout in LAYOUTS:
        got = _np_out(RAW_ENTRIES[entry](_Raw(layout, dtype), _raw_data()))
        assert len(got) == len(dense)
        for i, (g, r) in enumerate(zip(got, dense)):
            assert g.shape == r.shape and g.dtype == r.dtype, (entry, layout, i, g.shape, r.shape)
            same = np.array_equal(g, r, equal_nan=g.dtype.kind == 'f')
            print('%-40s %-12s %-8s output %d: %s' % (entry, layout, dtype.__name__, i, 'bit-identical' if same else 'DIFFERENT'))
            assert same, (entry, layout, i, np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))[:10] if g.dtype.kind == 'f' else None)


@both
def test_strided_host_views_are_refused(dtype):
    """check_view: host views must be dense (nlev, ncol) C-order -- XP_E_ARG before anything is staged or launched, for one
    entry point of csrc/xp_primitives_abi.hpp and one of csrc/xparcel.hip; the outputs stay untouched."""
    from xarray_parcel_amd import _lib as L
    lib = L.init(0)
    nlev, ncol = RAW_SHAPE
    xp = L.XP_F64 if dtype == np.float64 else L.XP_F32
    s = pc.humidity_cases(nlev, ncol)
    host = [np.ascontiguousarray(s[k].astype(dtype).T) for k in pc.DATASET]                      # (ncol, nlev)
    views = [L.View(a.ctypes.data, xp, L.XP_MEM_HOST, nlev, ncol, 1, nlev) for a in host]
    outs = [np.full((nlev - 1, ncol), SENTINEL, dtype=dtype) for _ in range(6)]
    rc = lib.xp_find_intersections(views[0], views[1], views[2], 0, (C.c_void_p * 6)(*[o.ctypes.data for o in outs]), None)
    assert rc == -1 and b'host views must be dense' in lib.xp_last_error()                      # XP_E_ARG
    out = np.full((nlev, ncol), SENTINEL, dtype=dtype)
    rc = lib.xp_wet_bulb_temperature(views[0], views[1], views[2], L.MOIST['exact'], out.ctypes.data, None)
    assert rc == -1 and b'host views must be dense' in lib.xp_last_error()
    assert all(np.all(o == SENTINEL) for o in outs + [out])
    # the padded layout likewise
    pad = np.full((nlev, ncol + 3), 1.0, dtype=dtype)
    v = L.View(pad.ctypes.data, xp, L.XP_MEM_HOST, nlev, ncol, ncol + 3, 1)
    assert lib.xp_crossing_level(v, v, 273.15, out.ctypes.data, None) == -1
