"""Grid-scale parity tests of the product bundle xp_conv_properties -- k_conv_columns and k_conv_finish (csrc/xp_bundle.hpp),
the three parcel passes and the 6000 m wind between them -- on the inputs of tests/bundle_cases.py, whose CPU guard
(tests/test_bundle_cases_cpu.py) shows that every class of column is present, survives the rounding to float32 and that the
reference shows every outcome.  Run with -m gpu on an MI355X.

(a)  The level-derived outputs against bundle_cases.level_reference (the oracle's own log_interp, freezing_level_height,
     wind_shear ... column by column): NaN pattern identical; float64 within 1e-8 * max(1, |ref|); float32: temp_500,
     freezing_level and melting_level equal to the float32-rounded reference, the rest within 3e-4 + 2e-6 * max(1, |ref|).
(b)  Blanking: exactly the columns of the reference's mask, every floating output and positive_shear.
(c)  The nine CAPE / CIN / lifted-index outputs bit-identical to the stand-alone cape_cin_columns fed the library's own
     dewpoint; mu_mixing_ratio within 4 ulp of the NumPy formula.
(d)  The whole bundle against oracle/parcel_oracle.py (RK4) on up to 200 columns with strictly decreasing, NaN-free
     pressure; storm_proxies / significant_hail_parameter on the bundle's own outputs of the whole grid.
(e)  Each of the 21 nullable outputs asked for alone, and none, through the raw ABI into guarded buffers.
(f)  Host arrays against device tensors; column-major and mixed strided device views through the raw ABI.
(g)  Rejections, each with device allocations of the full size behind every pointer.
(h)  The xarray mirror on (time, model_level_number, y, x) grids.

Largest differences measured on the MI355X (the tests print them before they assert).
(a), over the four shapes and both values of ignore_nans, |difference| in the unit of the output, float64 / float32 (after
the reference is rounded to float32); none within a factor of ten of its bound (the nearest: float32 dci + lifted index,
0.015 of it):
    temp_500 0 / 0;  lapse_rate_700_500 4.2e-14 / 0;  freezing_level 1.8e-12 / 0;  melting_level 6.8e-12 / 0;
    dci + lifted_index 8.0e-13 / 4.8e-06;  shear_u, shear_v 3.6e-15 / 0;  shear_magnitude 7.1e-15 / 0;  positive_shear identical
(c)  CAPE, CIN and lifted index bit-identical to the same request in all 36 comparisons (of 1337 columns CAPE is non-zero in
    314 / 298 / 250 for the three parcels, CIN in 190 / 150 / 155); mu_mixing_ratio 4.0 ulp in float64 -- AT its bound of
    4 ulp: the device's exp against NumPy's, then three quotients -- and 0.5 ulp in float32.
(d), relative to max(1, |ref|), 200 columns (80 of them warm): CAPE 4.6e-13 and CIN 1.4e-12 (bound 1e-6; non-zero in 67 and
    50 columns for the mixed parcels); lifted index 2.5e-13, DCI 2.4e-14, mu_mixing_ratio 1.7e-16, lapse rate 1.1e-15,
    temp_500 0, freezing level 3.0e-16, melting level 7.6e-15, shear 3.6e-16 (bound 1e-8).  Proxies on the bundle's own
    outputs of all 1337 columns: every flag identical and taking both values (True in 1 ... 79 columns blanked, 9 ... 202
    with ignore_nans); SHIP finite in 12 / 48 columns, 0.06 ... 3.2, equal to the oracle's to the last bit (bound 4e-16).
(e), (f), (g), (h): every bit identity and every guard held.

Teeth (scratch builds, one edit in csrc/xp_bundle.hpp each, none committed; the tests of this file that fail):
    bracket sums without the !isnan_(x[v]) test          (a) 24x1337, all four dtype x ignore_nans cases
    `s0 != s1` -> `s0 * s1 < 0` in both crossing rules   (a) float64 24x1337 and 2x300 (the 'on_value' columns: float64
                                                         only, as bundle_cases says), (d) both
    Td left out of `valid`                               (a) ignore_nans=False on 24x1337, 1x300, 2x300, (b) the same, (d) blank
    wet_bulb_third in double for float data              (a) float32 24x1337 and 2x300 (melting_level no longer equal)
    t500 where t700 belongs in the lapse rate            (a) 12 of 16 cases (1x300 has no lapse rate), (d) both, proxies both
    positive_shear ignoring `keep`                       (a) ignore_nans=False on 24x1337, 1x300, 2x300, (b) the same, (d) blank
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import parcel_oracle as po
from tests import bundle_cases as bc
from tests import component_cases as cc
from tests import primitive_cases as pc
from tests.output_struct_cases import Guarded

pytestmark = pytest.mark.gpu

xa = None
DTYPES = [np.float64, np.float32]
grid = pytest.mark.parametrize('shape', pc.SHAPES, ids=lambda s: '%dx%d' % s)
both = pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: d.__name__)
ignore = pytest.mark.parametrize('ignore_nans', [False, True], ids=['blank', 'ignore_nans'])
PARCELS = (('mu', 'most_unstable', 250), ('mixed_100', 'mixed_layer', 100), ('mixed_50', 'mixed_layer', 50))
RAW_SHAPE = (cc.NLEV, 300)
FLOAT_OUT = None                                                       # _lib.CONV_OUT without positive_shear, set by _api


@pytest.fixture(scope='module', autouse=True)
def _api():
    global xa, FLOAT_OUT
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    xa = numpy_api
    FLOAT_OUT = tuple(k for k in xa.L.CONV_OUT if k != 'positive_shear')
    yield


def _np(x):
    import torch
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


@functools.lru_cache(maxsize=None)
def _data(shape):
    return bc.bundle_grid(*shape)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """The nine inputs as the kernel is given them (host arrays, read-only)."""
    g = bc.inputs(_data(shape), dtype)[0]
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _dewpoint(shape, dtype):
    """The library's own q -> dewpoint of the inputs, in the data's type: what the bundle's parcels and levels read."""
    g = _inputs(shape, dtype)
    td = np.asarray(xa.dewpoint_from_specific_humidity(g['pressure'], g['temperature'], g['specific_humidity']))
    assert td.dtype == dtype and td.shape == shape
    return td


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, ignore_nans):
    return bc.level_reference(_data(shape), dtype, ignore_nans, dewpoint=None if dtype == np.float64 else _dewpoint(shape, dtype))


@functools.lru_cache(maxsize=None)
def _bundle(shape, dtype, ignore_nans, moist='exact'):
    got = _np(xa.conv_properties(_inputs(shape, dtype), ignore_nans=ignore_nans, moist=moist))
    assert set(got) == set(xa.L.CONV_OUT)
    for k, v in got.items():
        assert v.shape == (shape[1],) and v.dtype == (bool if k == 'positive_shear' else dtype), k
    return got


def _level_outputs(got):
    """The outputs of (a) by the reference's names: 'dci_plus_lifted_index' of the three parcels side by side."""
    g = {k: np.asarray(got[k], dtype=np.float64) for k in bc.LEVEL_OUT if k != 'dci_plus_lifted_index'}
    g['dci_plus_lifted_index'] = np.stack([np.asarray(got[pre + '_dci'], dtype=np.float64) + np.asarray(got[pre + '_lifted_index'], dtype=np.float64)
                                           for pre, _, _ in PARCELS])
    return g


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
EXACT32 = ('temp_500', 'freezing_level', 'melting_level')


@grid
@both
@ignore
def test_level_outputs_against_the_restatement(shape, dtype, ignore_nans):
    """NaN pattern identical; the bounds of the module docstring, where the measured maxima are."""
    got, ref = _bundle(shape, dtype, ignore_nans), _reference(shape, dtype, ignore_nans)
    g = _level_outputs(got)
    failed = []
    for k in bc.LEVEL_OUT:
        a, b = g[k], ref[k]
        nan_b = np.isnan(b)
        if k == 'dci_plus_lifted_index':                               # a NaN lifted index (no parcel, no 500 hPa) hides the level part
            li = np.stack([np.isnan(np.asarray(got[pre + '_lifted_index'], dtype=np.float64)) for pre, _, _ in PARCELS])
            b = np.broadcast_to(b, a.shape)
            nan_b = np.isnan(b) | li
        if not np.array_equal(np.isnan(a), nan_b):
            failed.append((k, 'NaN pattern', np.argwhere(np.isnan(a) != nan_b)[:8].tolist()))
            continue
        ok = ~nan_b
        if dtype == np.float32:
            b = b.astype(np.float32).astype(np.float64)
        err = np.abs(a[ok] - b[ok])
        if dtype == np.float64:
            lim = 1e-8 * np.maximum(1.0, np.abs(b[ok]))
        elif k in EXACT32:
            lim = np.zeros(err.shape)
        else:
            lim = 3e-4 + 2e-6 * np.maximum(1.0, np.abs(b[ok]))
        worst = float(err.max()) if err.size else 0.0
        ratio = float((err / np.where(lim > 0, lim, 1.0)).max()) if err.size and np.all(lim > 0) else float('nan')
        print('(a) %-9s %-8s %-12s %-22s n=%4d max|diff| %.3e  of its bound %.3g' % ('%dx%d' % shape, dtype.__name__,
              'ignore_nans' if ignore_nans else 'blank', k, int(ok.sum()), worst, ratio))
        if np.any(err > lim):
            failed.append((k, worst, np.argwhere(np.abs(a - b) > (lim.max() if lim.size else 0))[:8].tolist()))
    assert np.array_equal(got['positive_shear'], ref['positive_shear']), np.nonzero(got['positive_shear'] != ref['positive_shear'])[0][:8]
    assert not failed, failed


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
@grid
@both
def test_blanking_follows_the_references_mask(shape, dtype):
    valid = _reference(shape, dtype, False)['valid']
    blank, kept = _bundle(shape, dtype, False), _bundle(shape, dtype, True)
    for k in FLOAT_OUT:
        assert np.all(np.isnan(blank[k][~valid])), k
        assert np.array_equal(blank[k][valid], kept[k][valid], equal_nan=True), k      # nothing else changes
    assert not blank['positive_shear'][~valid].any()
    assert np.array_equal(blank['positive_shear'][valid], kept['positive_shear'][valid])
    if shape == pc.GRID:                                                # ignore_nans=True blanks nothing: invalid columns keep values
        for k in FLOAT_OUT:
            assert np.isfinite(kept[k][~valid]).any(), k
        assert kept['positive_shear'][~valid].any()


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('moist', ['exact', 'family'])
def test_parcel_outputs_equal_the_stand_alone_calls(dtype, moist):
    """The stand-alone call asks for what the bundle's pass asks for (CAPE, CIN, the lifted index; the parcel of the
    most-unstable pass) and so runs the same kernel: bit-identical in every mode.  Against the call that asks for every
    scalar, CAPE and CIN are bit-identical too, and so is the lifted index in exact mode; in family mode that request
    selects the profile-output kernel (the parcel's virtual temperature inverted at every node) where the bundle's selects
    the lifted-index-only instantiation (inverted at the two nodes around 500 hPa): two evaluations that
    tests/test_gpu_parity.py::test_lifted_index_only_kernels_of_family_mode holds together to 1e-9 K (float32: 2e-4 K), the
    bound here.  Measured: float64 family 5.7e-14 K in the most-unstable pass, 1.7e-13 K in the mixed-layer ones; float32 0."""
    shape = pc.GRID
    g, td = _inputs(shape, dtype), _dewpoint(shape, dtype)
    got = _bundle(shape, dtype, True, moist)
    for pre, parcel, depth in PARCELS:
        call = functools.partial(xa.cape_cin_columns, g['pressure'], g['temperature'], td, parcel=parcel, depth=depth, lifted_index_at=500.0,
                                 moist=moist)
        one = _np(call(want=('cape', 'cin') + (('parcel_pressure', 'parcel_dewpoint') if pre == 'mu' else ())))
        every = _np(call())
        for k in ('cape', 'cin', 'lifted_index'):
            a, b, e = got['%s_%s' % (pre, k)], one[k], every[k]
            assert a.dtype == b.dtype == e.dtype == dtype
            same = (a == b) | (np.isnan(a) & np.isnan(b))
            assert np.array_equal(np.isnan(a), np.isnan(e)), (pre, k)
            diff = float(np.nanmax(np.abs(a.astype(np.float64) - e.astype(np.float64)), initial=0.0))
            print('(c) %-8s %-7s %-9s %-12s finite %4d non-zero %4d  %s; against the all-scalars call: max|diff| %.3e' % (
                dtype.__name__, moist, pre, k, int(np.isfinite(b).sum()), int((np.nan_to_num(b) != 0).sum()), 'bit-identical' if same.all() else 'DIFFERENT', diff))
            assert same.all(), (pre, k, np.nonzero(~same)[0][:8], a[~same][:4], b[~same][:4])
            # values, not zeros (the warm columns of the grid; the others are convectively dead)
            assert np.isfinite(b).sum() >= 100 and (k == 'lifted_index' or (np.nan_to_num(b) != 0).sum() >= (60 if k == 'cape' else 30)), (pre, k)
            assert diff <= ((1e-9 if dtype == np.float64 else 2e-4) if moist == 'family' and k == 'lifted_index' else 0.0), (pre, k, diff)
        if pre == 'mu':
            p, tdp = one['parcel_pressure'].astype(np.float64), one['parcel_dewpoint'].astype(np.float64)
            with np.errstate(all='ignore'):
                e = 6.112 * np.exp(17.67 * (tdp - 273.15) / (tdp - 29.65))
                w = bc.th.EPSILON * e / (p - e)
                qs = w / (1.0 + w)
                ref = qs / (1.0 - qs)
            a = got['mu_mixing_ratio'].astype(np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(ref))
            ok = ~np.isnan(ref)
            ulp = np.spacing(np.abs(ref[ok]).astype(dtype)).astype(np.float64)
            err = np.abs(a[ok] - ref[ok]) / ulp
            print('(c) %-8s %-7s mu_mixing_ratio finite %4d  max %.2f ulp' % (dtype.__name__, moist, int(ok.sum()), float(err.max())))
            assert ok.sum() >= 100 and np.all(err <= 4.0), float(err.max())


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
@ignore
def test_the_whole_bundle_against_the_oracle(ignore_nans):
    """The columns are bundle_cases.oracle_columns: tests/test_bundle_cases_cpu.py shows that they cover the classes and that
    CAPE, CIN, the lifted index and the DCI are values on them (the warm columns), not zeros."""
    d = _data(pc.GRID)
    cols = bc.oracle_columns(d, ignore_nans)
    assert 150 <= cols.size <= bc.ORACLE_MAX
    got = _bundle(pc.GRID, np.float64, ignore_nans)
    ref = bc.oracle_bundle(d, cols, ignore_nans)
    tol = {'cape': 1e-6, 'cin': 1e-6}
    failed = []
    for k in xa.L.CONV_OUT:
        g, r = got[k][cols], ref[k]
        if k == 'positive_shear':
            assert np.array_equal(g, r.astype(bool)), k
            continue
        if not np.array_equal(np.isnan(g), np.isnan(r)):
            failed.append((k, 'NaN pattern', cols[np.isnan(g) != np.isnan(r)][:8].tolist()))
            continue
        ok = ~np.isnan(r)
        rel = np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))
        worst = float(rel.max()) if rel.size else 0.0
        lim = tol.get(k.split('_')[-1], 1e-8)
        print('(d) %-12s %-24s n=%3d non-zero %3d max rel diff %.3e  (bound %.0e)' % ('ignore_nans' if ignore_nans else 'blank', k, int(ok.sum()),
              int((r[ok] != 0).sum()), worst, lim))
        if worst > lim:
            failed.append((k, worst, cols[ok][rel > lim][:8].tolist()))
    assert not failed, failed


@ignore
def test_storm_proxies_on_the_bundles_own_outputs(ignore_nans):
    got = _bundle(pc.GRID, np.float64, ignore_nans)
    gp, rp = xa.storm_proxies(got), po.storm_proxies(got)
    assert list(gp) == list(rp)
    if not ignore_nans:
        for k in xa.L.PROXIES_IN:
            assert np.isnan(got[k]).any(), k                           # NaN in every input
    for k in rp:
        if k == 'ship':
            a, b = np.asarray(gp[k]), rp[k]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            ok = ~np.isnan(b)
            rel = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)
            print('(d) %-12s SHIP finite in %d columns, %.3g ... %.3g, max rel diff %.2e' % (
                'ignore_nans' if ignore_nans else 'blank', int(ok.sum()), b[ok].min(initial=np.inf), b[ok].max(initial=-np.inf), rel.max(initial=0.0)))
            assert ok.sum() >= 5 and (b[ok] > 0.1).any(), 'SHIP must be a number somewhere'     # (the warm columns of the grid)
            assert np.all(rel <= 4e-16)
        else:
            print('(d) %-12s %-18s True in %d columns' % ('ignore_nans' if ignore_nans else 'blank', k, int(rp[k].sum())))
            assert np.asarray(gp[k]).dtype == bool and np.array_equal(np.asarray(gp[k]), rp[k]), k
            assert rp[k].any() and not rp[k].all(), k                   # both values
    ship = xa.significant_hail_parameter(got['mu_cape'], got['mu_mixing_ratio'], got['lapse_rate_700_500'], got['temp_500'],
                                         got['shear_magnitude'], got['freezing_level'])
    with np.errstate(invalid='ignore'):
        r = po.significant_hail_parameter(got['mu_cape'], got['mu_mixing_ratio'], got['lapse_rate_700_500'], got['temp_500'],
                                          got['shear_magnitude'], got['freezing_level'])
    ok = ~np.isnan(r)
    assert np.array_equal(np.isnan(ship), np.isnan(r)) and np.all(np.abs(ship[ok] - r[ok]) <= 4e-16 * np.maximum(np.abs(r[ok]), 1e-300))


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------------
LAYOUTS = ('dense', 'column_major', 'padded')
PAD = 5


class _Raw:
    """One xp_conv_properties call through ctypes on device tensors."""

    def __init__(self, dtype, shape=RAW_SHAPE):
        import torch
        from xarray_parcel_amd import _lib as L
        self.torch, self.L, self.lib = torch, L, L.init(0)
        self.dtype, self.xp = dtype, (L.XP_F64 if dtype == np.float64 else L.XP_F32)
        self.shape, self.g = shape, _inputs(shape, dtype)
        self.keep = []

    def tensor(self, a, layout='dense'):
        """A device tensor holding `a` (rows, ncol) in `layout`; (tensor, lev_stride, col_stride)."""
        t = self.torch
        rows, ncol = a.shape
        a = np.array(a)                                                 # (a writable copy: the cached inputs are read-only)
        if layout == 'dense':
            buf, ls, cs = t.from_numpy(a).cuda(), ncol, 1
        elif layout == 'column_major':
            buf, ls, cs = t.from_numpy(np.ascontiguousarray(a.T)).cuda(), 1, rows
        else:
            buf = t.full((rows, ncol + PAD), float('nan'), dtype=t.from_numpy(a).dtype, device='cuda')
            buf[:, :ncol] = t.from_numpy(a).cuda()
            ls, cs = ncol + PAD, 1
        self.keep.append(buf)
        return buf, ls, cs

    def view(self, name, layout='dense', mem=None, dtype=None, ncol=None):
        a = self.g[name]
        if dtype is not None:                                           # a claimed dtype: the allocation covers the larger of the two
            a = a.astype(np.float64)
        buf, ls, cs = self.tensor(a, layout)
        n = a.shape[1] if ncol is None else ncol
        if ncol is not None and layout == 'dense':
            ls = n
        return self.L.View(buf.data_ptr(), self.xp if dtype is None else dtype, self.L.XP_MEM_DEVICE if mem is None else mem,
                           a.shape[0], n, ls, cs)

    def views(self, layouts=None, **over):
        layouts = layouts or {}
        return [over.get(k) or self.view(k, layouts.get(k, 'dense')) for k in self.L.CONV_IN_VIEWS]

    def outputs(self, want=None):
        """Guarded device buffers for the outputs in `want` (default: all 21); the others stay NULL."""
        want = self.L.CONV_OUT if want is None else want
        ncol = self.shape[1]
        return {k: Guarded.row(ncol, np.int32 if k == 'positive_shear' else self.dtype, 'device') for k in want}

    def call(self, views, outs, opts=None, ignore_nans=1, sfc=True, null_in=False, null_out=False):
        L = self.L
        sfu = self.tensor(self.g['surface_wind_u'][None, :])[0].data_ptr() if sfc in (True, 'u') else None
        sfv = self.tensor(self.g['surface_wind_v'][None, :])[0].data_ptr() if sfc in (True, 'v') else None
        ci = L.ConvIn(*[C.pointer(v) for v in views], sfu, sfv)
        co = L.ConvOut()
        for k, b in outs.items():
            setattr(co, k, b.ptr)
        rc = self.lib.xp_conv_properties(None if null_in else C.byref(ci), None if opts is None else C.byref(opts), C.c_int32(ignore_nans),
                                         None if null_out else C.byref(co), None)
        self.torch.cuda.synchronize()
        return rc

    def opts(self, **kw):
        L = self.L
        o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST['exact'], L.XP_F64, L.HUMIDITY['dewpoint'], 0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o


@functools.lru_cache(maxsize=None)
def _raw_all(dtype, ignore_nans=1):
    """The all-outputs call on dense device views: name -> (ncol,) array."""
    h = _Raw(dtype)
    outs = h.outputs()
    rc = h.call(h.views(), outs, h.opts(), ignore_nans)
    assert rc == 0, h.lib.xp_last_error()
    for k, b in outs.items():
        assert b.untouched() and b.written(), k
    res = {k: b.read()[0] for k, b in outs.items()}
    assert all(np.isfinite(res[k]).sum() >= 20 for k in res if k != 'positive_shear'), {k: int(np.isfinite(v).sum()) for k, v in res.items()}
    return res


def _identical(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
@both
@ignore
def test_null_outputs_through_the_raw_abi(dtype, ignore_nans):
    """21 nullable outputs select between the caller's buffer and scratch, and nine of them (CAPE, CIN, lifted index) plus
    the freezing and melting level are also inputs of the per-point kernel: each asked for alone gives the all-outputs
    call's bits and touches nothing but its ncol elements; a call that asks for nothing succeeds."""
    ref = _raw_all(dtype, int(ignore_nans))
    h = _Raw(dtype)
    views = h.views()
    assert h.call(views, {}, h.opts(), int(ignore_nans)) == 0, h.lib.xp_last_error()
    assert len(h.L.CONV_OUT) == 21
    for k in h.L.CONV_OUT:
        outs = h.outputs((k,))
        assert h.call(views, outs, h.opts(), int(ignore_nans)) == 0, (k, h.lib.xp_last_error())
        assert outs[k].untouched(), k
        assert _identical(outs[k].read()[0], ref[k]), k
    # and the complement of each parcel's triple: the per-point kernel reads CAPE / CIN / lifted index from scratch
    for pre, _, _ in PARCELS:
        want = tuple(k for k in h.L.CONV_OUT if not (k.startswith(pre + '_') and k.split('_')[-1] in ('cape', 'cin', 'index')))
        outs = h.outputs(want)
        assert h.call(views, outs, h.opts(), int(ignore_nans)) == 0, (pre, h.lib.xp_last_error())
        for k in want:
            assert outs[k].untouched() and _identical(outs[k].read()[0], ref[k]), (pre, k)


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('moist', ['exact', 'family'])
def test_host_arrays_equal_device_tensors(dtype, moist):
    import torch
    g = _inputs(pc.GRID, dtype)
    dev = xa.conv_properties({k: torch.from_numpy(np.array(v)).cuda() for k, v in g.items()}, ignore_nans=True, moist=moist)
    host = _bundle(pc.GRID, dtype, True, moist)
    for k in host:
        assert torch.is_tensor(dev[k]) and dev[k].is_cuda and isinstance(host[k], np.ndarray)
        assert _identical(dev[k].cpu().numpy(), host[k]), k


MIXED = {'pressure': 'column_major', 'temperature': 'column_major', 'specific_humidity': 'dense', 'height_asl': 'dense',
         'wind_u': 'padded', 'wind_v': 'padded', 'wind_height_above_surface': 'padded'}


@both
@pytest.mark.parametrize('layouts', ['column_major', 'mixed'])
def test_strided_device_views_through_the_raw_abi(dtype, layouts):
    """include/xparcel.h promises general element strides for every view.  k_conv_columns reads the strided grids in place;
    the parcel passes densify them (stage_cape), because the scratch dewpoint beside them is dense: every output has the
    dense call's bits either way."""
    ref = _raw_all(dtype)
    h = _Raw(dtype)
    lay = MIXED if layouts == 'mixed' else {k: 'column_major' for k in h.L.CONV_IN_VIEWS}
    outs = h.outputs()
    assert h.call(h.views(lay), outs, h.opts()) == 0, h.lib.xp_last_error()
    for k, b in outs.items():
        same = _identical(b.read()[0], ref[k])
        print('(f) %-12s %-8s %-24s %s' % (layouts, dtype.__name__, k, 'bit-identical' if same else 'DIFFERENT'))
        assert b.untouched() and same, k


# ---- (g) ---------------------------------------------------------------------------------------------------------------------
def _rejected(h, rc, outs, code, *words):
    msg = h.lib.xp_last_error().decode()
    assert rc == code, (rc, code, msg)
    for w in words:
        assert w in msg, (w, msg)
    for k, b in outs.items():
        assert b.pristine(), k


@both
def test_rejections(dtype):
    """Every pointer of every call is a device allocation of the full size, whatever its `mem` field says: a library that
    wrongly accepts a call reads and writes valid memory, and the test fails by the return code."""
    from xarray_parcel_amd._lib import XP_E_ARG, XP_E_INTERP
    h = _Raw(dtype)
    L = h.L
    HOST, DEV = L.XP_MEM_HOST, L.XP_MEM_DEVICE
    outs = h.outputs()
    other = L.XP_F32 if dtype == np.float64 else L.XP_F64
    # a view that lives elsewhere than pressure: each of the six, both ways round
    for k in L.CONV_IN_VIEWS[1:]:
        _rejected(h, h.call(h.views(**{k: h.view(k, mem=HOST)}), outs, h.opts()), outs, XP_E_ARG, 'pressure/' + k, 'mem')
        host_but = [h.view(n, mem=DEV if n == k else HOST) for n in L.CONV_IN_VIEWS]
        _rejected(h, h.call(host_but, outs, h.opts()), outs, XP_E_ARG, 'pressure/' + k, 'mem')
    # the wind views against the grid: dtype, columns
    wind = L.CONV_IN_VIEWS[4:]
    _rejected(h, h.call(h.views(**{k: h.view(k, dtype=other) for k in wind}), outs, h.opts()), outs, XP_E_ARG, 'pressure/wind_u')
    _rejected(h, h.call(h.views(**{k: h.view(k, ncol=h.shape[1] - 1) for k in wind}), outs, h.opts()), outs, XP_E_ARG, 'pressure/wind_u')
    # ... and among themselves, and the grids among themselves
    _rejected(h, h.call(h.views(wind_v=h.view('wind_v', ncol=h.shape[1] - 1)), outs, h.opts()), outs, XP_E_ARG, 'wind_u/wind_v')
    _rejected(h, h.call(h.views(height_asl=h.view('height_asl', dtype=other)), outs, h.opts()), outs, XP_E_ARG, 'pressure/height_asl')
    # a strided host view
    for k, lay in (('pressure', 'column_major'), ('wind_height_above_surface', 'padded')):
        vs = [h.view(n, lay if n == k else 'dense', mem=HOST) for n in L.CONV_IN_VIEWS]
        _rejected(h, h.call(vs, outs, h.opts()), outs, XP_E_ARG, k, 'host views must be dense')
    # NULL in, out, surface winds, a NULL view
    _rejected(h, h.call(h.views(), outs, h.opts(), null_in=True), outs, XP_E_ARG, 'null')
    _rejected(h, h.call(h.views(), outs, h.opts(), null_out=True), outs, XP_E_ARG, 'null')
    _rejected(h, h.call(h.views(), outs, h.opts(), sfc='u'), outs, XP_E_ARG, 'null surface wind')
    _rejected(h, h.call(h.views(), outs, h.opts(), sfc='v'), outs, XP_E_ARG, 'null surface wind')
    # the options -- on an empty grid as well
    empty = [L.View(v.data, v.dtype, v.mem, v.nlev, 0, 0, 1) for v in h.views()]
    for views in (h.views(), empty):
        _rejected(h, h.call(views, outs, h.opts(compute=L.XP_F32)), outs, XP_E_ARG, 'compute')
        _rejected(h, h.call(views, outs, h.opts(moist_mode=9)), outs, XP_E_ARG, 'moist_mode')
        _rejected(h, h.call(views, outs, h.opts(lcl_interp=5)), outs, XP_E_INTERP, 'linear or log')
    assert h.call(empty, outs, h.opts()) == 0 and all(b.pristine() for b in outs.values())
    # the same buffers, a valid call: accepted and written
    assert h.call(h.views(), outs, h.opts()) == 0, h.lib.xp_last_error()
    ref = _raw_all(dtype)
    assert all(_identical(b.read()[0], ref[k]) for k, b in outs.items())


# ---- (h) ---------------------------------------------------------------------------------------------------------------------
@both
def test_the_xarray_mirror_on_a_four_dimensional_grid(dtype):
    from xarray_parcel_amd import parcel_functions as pf
    from xarray_parcel_amd._xr import DataArray, Dataset
    nt, ny, nx = 2, 7, 9
    ncol = nt * ny * nx
    g = {k: np.ascontiguousarray(v[..., :ncol]) for k, v in _inputs(pc.GRID, dtype).items()}
    nlev, nwind = g['pressure'].shape[0], g['wind_u'].shape[0]
    coords = {'time': np.arange(nt) * 6, 'y': np.linspace(-30.0, -20.0, ny), 'x': np.linspace(140.0, 150.0, nx)}
    ds = Dataset({})
    for k in bc.GRID_INPUTS:                                            # the vertical is not the leading dim
        a = np.moveaxis(g[k].reshape(nlev, nt, ny, nx), 0, 1)
        ds[k] = DataArray(a, dims=('time', 'model_level_number', 'y', 'x'), coords={**coords, 'model_level_number': np.arange(nlev)})
    for k in bc.WIND_INPUTS:                                            # the winds' vertical is a dim of its own, last
        a = np.moveaxis(g[k].reshape(nwind, nt, ny, nx), 0, 3)
        ds[k] = DataArray(a, dims=('time', 'y', 'x', 'wind_level'), coords=coords)
    for k in bc.POINT_INPUTS:
        ds[k] = DataArray(g[k].reshape(nt, ny, nx), dims=('time', 'y', 'x'), coords=coords)
    for ignore_nans in (False, True):
        flat = _np(xa.conv_properties(g, ignore_nans=ignore_nans, moist='exact'))
        props = pf.conv_properties(ds, ignore_nans=ignore_nans, moist='exact')
        assert set(props.keys()) == set(flat)
        for k in flat:
            v = props[k]
            assert v.dims == ('time', 'y', 'x') and v.shape == (nt, ny, nx), k
            assert _identical(np.asarray(v.values).reshape(-1), flat[k]), k
            assert all(np.array_equal(np.asarray(v.coords[c]), coords[c]) for c in coords), k
    # the reference's attrs (pf.py:1951-2100: each product keeps the attrs of the function that made it)
    for pre, _, _ in PARCELS:
        assert props[pre + '_dci'].attrs['units'] == 'C' and props[pre + '_cape'].attrs['units'] == 'J kg$^{-1}$'
        assert props[pre + '_cin'].attrs['long_name'] == 'Convective inhibition'
    assert props['lapse_rate_700_500'].attrs == {'long_name': 'Lapse rate', 'description': '700-500 hPa lapse rate', 'units': 'K km$^{-1}$'}
    assert props['temp_500'].attrs == {'description': 'Temperature at 500 hPa.', 'long_name': 'Isobar temperature', 'units': 'K'}
    assert props['freezing_level'].attrs['description'] == 'Height of zero degree dry-bulb temperature isotherm.'
    assert props['melting_level'].attrs['description'] == 'Height of zero degree wet-bulb temperature isotherm.'
    assert props['mu_mixing_ratio'].attrs['description'] == 'Mixing ratio of most unstable parcel'
