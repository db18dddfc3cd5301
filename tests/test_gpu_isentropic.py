"""Isentropic interpolation on the device (xp_isentropic_interpolation) against the NumPy restatement
tests/isentropic_restatement.py, and its own argument checks.  The inputs and what they hold are counted on the CPU
(tests/test_isentropic_cpu.py::test_input_census).
Comparison rule: status words and NaN patterns equal the restatement's; columns where some target lies within 1e-9 theta* of
a level's theta (the bracket may differ by the last bit of exp) are excluded and must be at most 1 % (the census: 0); the
parity tests run at eps = 1e-10, where both sides sit on the fixed point to rounding.
Bounds (TOL): the pair's |d theta| >= 0.05 K bounds the conditioning -- a 1e-13 K rounding of theta moves ln p by about
2e-13 -- so anything near 1e-9 is a bug, not rounding.  Measured on an MI355X over the four grids, both directions, 1, 16 and
64 targets (f64): pressure 2.4e-14 relative, temperature 1.9e-12 K, the extras 5.0e-13 of max(|v_k|, |v_k+1|); TOL is at
least 100 x that and tighter than the 1e-9 / 1e-8 K / 1e-8 it may never exceed.  Default eps against the restatement at the
same eps: 1.4e-14 relative (bound 1e-10)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import isentropic_cases as K
from tests import isentropic_restatement as R
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
EPS = 1e-10
# |device - restatement|: pressure relative, temperature [K], the extras relative to max(|v_k|, |v_k+1|) of the pair
TOL = {'pressure': 1e-11, 'temperature': 1e-9, 'vars': 1e-10}


@functools.lru_cache(maxsize=None)
def inputs(name, dtype=np.float64):
    return K.inputs(*K.GRIDS[name], dtype=dtype)


@functools.lru_cache(maxsize=None)
def restated(name, from_below=True, eps=EPS, max_iters=50, levels='16', dtype=np.float64):
    """The restatement of one grid (computed once, shared, left unchanged) and its tie columns."""
    p, t, td, w = (a.astype(np.float64) for a in inputs(name, dtype))
    lev = {'16': K.LEVELS, '64': K.LEVELS_64, '1': K.LEVELS[5:6]}[levels]
    ref = R.grid(p, t, lev, [td, w], from_below=from_below, eps=eps, max_iters=max_iters)
    tie = np.array([R.tie_column(c, lev) for c in ref['columns']])
    assert tie.sum() <= 0.01 * len(tie), tie.sum()
    return ref, tie, lev


def run(levels, p, t, *extras, **kw):
    res = xa.isentropic_interpolation(levels, p, t, *extras, temperature_out=True, status=True, **kw)
    return {'pressure': res[0], 'temperature': res[1], 'vars': res[2:-1], 'status': res[-1]}


def compare(got, ref, keep, f32=False, label=''):
    """Status and NaN patterns equal, every output within its bound; prints the largest difference of each."""
    assert np.array_equal(np.asarray(got['status'])[keep], ref['status'][keep]), label
    rows = [('pressure', got['pressure'], ref['pressure'], None), ('temperature', got['temperature'], ref['temperature'], None)]
    rows += [('vars', g, r, s) for g, r, s in zip(got['vars'], ref['vars'], ref['vscale'])]
    for k, g, r, scale in rows:
        g, r = np.asarray(g).astype(np.float64)[:, keep], r[:, keep]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, k, np.argwhere(np.isnan(g) != np.isnan(r))[:5])
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        unit = np.abs(r[ok]) if k == 'pressure' else scale[:, keep][ok] if k == 'vars' else np.ones(ok.sum())
        bound = TOL[k] * unit
        if f32:
            bound = bound + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        print('%s %-12s n = %5d  max = %.3e' % (label, k, ok.sum(), (err / unit).max() if ok.any() else 0.0))
        assert np.all(err <= bound), (label, k, float((err / unit).max()), np.argwhere(ok)[np.argmax(err - bound)])


@pytest.mark.parametrize('name', sorted(K.GRIDS))
def test_grid_parity_both_directions(name):
    p, t, td, w = inputs(name)
    got = {}
    for up in (True, False):
        ref, tie, lev = restated(name, up)
        got[up] = run(lev, p, t, td, w, eps=EPS, bottom_up_search=up)
        compare(got[up], ref, ~tie, label='%s %s' % (name, 'up' if up else 'down'))
        assert np.isfinite(got[up]['pressure']).sum() >= 0.75 * got[up]['pressure'].size
    differs = ~np.all((got[True]['pressure'] == got[False]['pressure']) | np.isnan(got[True]['pressure']), axis=0)
    print(name, 'columns where from_below changes the pressure:', differs.sum())
    assert differs.sum() >= (15 if name != '7x65' else 0)


def test_default_eps_agrees_with_the_restatement_at_the_same_eps():
    p, t, td, w = inputs('40x640')
    ref, tie, lev = restated('40x640', True, 1e-6)
    got = xa.isentropic_interpolation(lev, p, t)[0]
    keep = ~tie
    assert np.array_equal(np.isnan(got[:, keep]), np.isnan(ref['pressure'][:, keep]))
    rel = np.abs(got / ref['pressure'] - 1.0)[:, keep]
    print('default eps: max relative difference %.3e' % np.nanmax(rel))
    assert np.nanmax(rel) <= 1e-10


@pytest.mark.parametrize('levels', ['1', '64'])
def test_one_and_sixty_four_targets(levels):
    p, t, td, w = inputs('24x300')
    ref, tie, lev = restated('24x300', True, EPS, 50, levels)
    compare(run(lev, p, t, td, w, eps=EPS), ref, ~tie, label='24x300 n=' + levels)


def test_seventy_targets_are_two_calls_put_together():
    p, t, td, w = inputs('24x300')
    lev = np.arange(280.0, 420.0, 2.0)
    assert lev.size == 70
    whole, a, b = run(lev, p, t, td, w), run(lev[:64], p, t, td, w), run(lev[64:], p, t, td, w)
    for k in ('pressure', 'temperature'):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]]), equal_nan=True), k
    for q in range(2):
        assert np.array_equal(whole['vars'][q], np.concatenate([a['vars'][q], b['vars'][q]]), equal_nan=True), q
    assert np.array_equal(whole['status'], a['status'] | b['status']) and whole['pressure'].shape == (70, 300)
    # levels are sorted, and more than four further variables are further calls
    rev = xa.isentropic_interpolation(lev[::-1], p, t, td, w, td, w, td, temperature_out=True)
    assert len(rev) == 7 and np.array_equal(rev[0], whole['pressure'], equal_nan=True)
    for q in range(5):
        assert np.array_equal(rev[2 + q], whole['vars'][q % 2], equal_nan=True), q


def test_fp32_inputs_round_like_the_restatement():
    p, t, td, w = inputs('12x640', np.float32)
    ref, tie, lev = restated('12x640', True, EPS, 50, '16', np.float32)
    got = run(lev, p, t, td, w, eps=EPS)
    assert got['pressure'].dtype == np.float32 and got['vars'][1].dtype == np.float32 and got['status'].dtype == np.int32
    compare(got, ref, ~tie, f32=True, label='f32')


def test_outputs_do_not_depend_on_each_other():
    p, t, td, w = inputs('24x300')
    for up in (True, False):
        full = run(K.LEVELS, p, t, td, w, bottom_up_search=up)
        alone = xa.isentropic_interpolation(K.LEVELS, p, t, bottom_up_search=up, status=True)
        assert len(alone) == 2 and np.array_equal(alone[0], full['pressure'], equal_nan=True)
        assert np.array_equal(alone[1], full['status'])
        one = xa.isentropic_interpolation(K.LEVELS, p, t, w, bottom_up_search=up)
        assert len(one) == 2 and np.array_equal(one[1], full['vars'][1], equal_nan=True)
    # one extra alone through the raw ABI: no pressure, no temperature, no status
    lib = L.init(0)
    nlev, ncol = p.shape
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, nlev, ncol, ncol, 1) for a in (p, t, w)]
    v = np.empty((len(K.LEVELS), ncol))
    out = L.IsentropicOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    out.vars[0] = v.ctypes.data
    L.check(lib.xp_isentropic_interpolation(views[0], views[1], 1, (C.POINTER(L.View) * 1)(C.pointer(views[2])), len(K.LEVELS),
                                            (C.c_double * len(K.LEVELS))(*K.LEVELS), None, out, None))
    assert np.array_equal(v, run(K.LEVELS, p, t, td, w)['vars'][1], equal_nan=True)


def test_convergence_limit():
    p, t, td, w = inputs('7x65')
    ref1, tie, lev = restated('7x65', True, 1e-6, 1)
    full, _, _ = restated('7x65', True, 1e-6, 50)
    got = run(lev, p, t, td, w, max_iters=1)
    compare(got, ref1, ~tie, label='max_iters=1')
    steps = np.stack([c['steps'] for c in full['columns']], 1)
    assert (steps >= 2).sum() >= 500
    assert np.all(np.isnan(got['pressure'][steps >= 2])) and np.all(np.isnan(got['vars'][0][steps >= 2]))
    late = (steps >= 2).any(axis=0)
    assert np.all(np.asarray(got['status'])[late] & L.ST_NOT_CONVERGED) and not np.any(np.asarray(got['status'])[~late] & L.ST_NOT_CONVERGED)


def test_hand_built_columns():
    p, t, v, lev = K.hand_columns()
    for up in (True, False):
        ref = R.grid(p, t, lev, [v], from_below=up, eps=EPS)
        got = run(lev, p, t, v, eps=EPS, bottom_up_search=up)
        compare(got, ref, np.ones(7, bool), label='hand %s' % up)
        P, ST = got['pressure'], got['status']
        assert abs(P[1, 0] / 800.0 - 1.0) <= 1e-9 and abs(got['vars'][0][1, 0] - v[2, 0]) <= 1e-8 * abs(v[2, 0])   # a target ON a level
        assert np.isnan(got['vars'][0][3, 0]) and np.isfinite(P[3, 0])                  # a NaN end of the extra alone
        assert (900.0 > P[2, 1] > 800.0) if up else (650.0 > P[2, 1] > 500.0)           # an unstable layer: first and last crossing
        assert np.isnan(P[:, 2]).all() and np.isnan(P[:, 3]).all() and ST[2] == ST[3] == L.XP_ST_NO_LAYER
        assert 900.0 > P[1, 4] > 650.0 and np.isnan(P[:, 5]).all()                      # dropped level; dry adiabat: no crossing
        assert np.isnan(P[0, :6]).all() and np.isnan(P[4]).all() and np.all(ST == L.XP_ST_NO_LAYER)
        # isothermal: p* = 1000 (T / theta*)^(1 / kappa)
        want = 1000.0 * (250.0 / lev[:4]) ** 3.5
        assert np.all(np.abs(P[:4, 6] / want - 1.0) <= 1e-9)


def test_input_kinds_and_strided_views():
    import torch
    p, t, td, w = inputs('24x300')
    ref = run(K.LEVELS, p, t, td, w)
    cpu = run(K.LEVELS, *(torch.from_numpy(a) for a in (p, t, td, w)))
    dev = run(K.LEVELS, *(torch.from_numpy(a).cuda() for a in (p, t, td, w)))
    flat = lambda r: [r['pressure'], r['temperature'], *r['vars'], r['status']]
    for a, b, c in zip(flat(ref), flat(cpu), flat(dev)):
        assert isinstance(b, np.ndarray) and c.is_cuda
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c.cpu().numpy(), equal_nan=True)
    # a 1-D pressure (isobaric data) is expanded to the grid
    p1 = p[:, 0].copy()
    pg = np.ascontiguousarray(np.broadcast_to(p1[:, None], p.shape))
    want = run(K.LEVELS, pg, t, td)
    for one in (run(K.LEVELS, p1, t, td), run(K.LEVELS, torch.from_numpy(p1), torch.from_numpy(t).cuda(), td)):
        assert np.array_equal(np.asarray(one['pressure'].cpu() if hasattr(one['pressure'], 'cpu') else one['pressure']),
                              want['pressure'], equal_nan=True)
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev, ncol = p.shape
    n = len(K.LEVELS)
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, t, td, w)]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    outs = [torch.empty((n, ncol), dtype=torch.float64, device='cuda') for _ in range(4)]
    status = torch.empty(ncol, dtype=torch.int32, device='cuda')
    o = L.IsentropicOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, pressure=outs[0].data_ptr(), temperature=outs[1].data_ptr(),
                        status=status.data_ptr())
    o.vars[0], o.vars[1] = outs[2].data_ptr(), outs[3].data_ptr()
    vp = (C.POINTER(L.View) * 2)(C.pointer(views[2]), C.pointer(views[3]))
    L.check(lib.xp_isentropic_interpolation(views[0], views[1], 2, vp, n, (C.c_double * n)(*K.LEVELS), L.IsentropicOpts(1, 50, 1e-6), o, None))
    torch.cuda.synchronize()
    for a, b in zip(flat(ref), outs + [status]):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)


def test_raw_abi_errors():
    lib = L.init(0)
    arrs = [np.ascontiguousarray(a) for a in K.inputs(12, 8, seed=2)]
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 12, 8, 8, 1) for a in arrs]
    short = L.View(arrs[1].ctypes.data, L.XP_F64, L.XP_MEM_HOST, 6, 8, 8, 1)
    null = C.POINTER(L.View)()
    lev = [300.0, 310.0, 320.0]
    pr, v0, v2 = np.empty((3, 8)), np.empty((3, 8)), np.empty((3, 8))

    def call(p=views[0], t=views[1], nvar=2, variables=(views[2], views[3]), levels=lev, nlevel=None, opts=(1, 50, 1e-6), out=True,
             dtype=L.XP_F64, mem=L.XP_MEM_HOST, first=True, extra=None):
        vp = None if variables is None else (C.POINTER(L.View) * len(variables))(*[null if v is None else C.pointer(v) for v in variables])
        o = L.IsentropicOut(dtype=dtype, mem=mem, pressure=pr.ctypes.data)
        if first:
            o.vars[0] = v0.ctypes.data
        if extra is not None:
            o.vars[extra] = v2.ctypes.data
        lv = None if levels is None else (C.c_double * len(levels))(*levels)
        n = (0 if levels is None else len(levels)) if nlevel is None else nlevel
        return lib.xp_isentropic_interpolation(p, t, nvar, vp, n, lv, None if opts is None else L.IsentropicOpts(*opts), o if out else None, None)
    pr[:] = 0.0
    assert call() == L.XP_OK and np.isfinite(pr).any() and call(opts=None) == L.XP_OK
    assert call(nvar=0, variables=None, first=False) == L.XP_OK
    inf, nan = float('inf'), float('nan')
    for kw, word in (({'p': None}, 'pressure'), ({'t': None}, 'temperature'), ({'t': short}, 'temperature'),
                     ({'nvar': -1}, 'nvar'), ({'nvar': 5}, 'nvar'), ({'variables': None}, 'variables'),
                     ({'variables': (views[2], None)}, 'variables[1]'), ({'variables': (views[2], short)}, 'variables[1]'),
                     ({'nvar': 1, 'extra': 2}, 'vars[2]'), ({'nvar': 0, 'variables': None}, 'vars[0]'),
                     ({'nlevel': 0}, 'nlevel'), ({'levels': [300.0 + i for i in range(65)]}, 'nlevel'), ({'levels': None, 'nlevel': 3}, 'levels'),
                     ({'levels': [300.0, inf]}, 'levels'), ({'levels': [nan, 310.0]}, 'levels'), ({'levels': [300.0, 300.0]}, 'levels'),
                     ({'levels': [310.0, 300.0]}, 'levels'), ({'opts': (1, 0, 1e-6)}, 'max_iters'), ({'opts': (1, -3, 1e-6)}, 'max_iters'),
                     ({'opts': (1, 50, 0.0)}, 'eps'), ({'opts': (1, 50, -1e-6)}, 'eps'), ({'opts': (1, 50, nan)}, 'eps'),
                     ({'opts': (1, 50, inf)}, 'eps'), ({'out': False}, 'out'), ({'dtype': L.XP_F32}, 'out'),
                     ({'mem': L.XP_MEM_DEVICE}, 'out')):
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())


def test_dataarray_module_end_to_end():
    from xarray_parcel_amd import isentropic as mirror
    from xarray_parcel_amd._xr import DataArray
    p, t, td, w = inputs('12x640')
    full = run(K.LEVELS, p, t, td, w)
    da = [DataArray(a.reshape(12, 20, 32), dims=('model_level_number', 'y', 'x'), name=n)
          for a, n in zip((p, t, td, w), ('p', 't', 'dewpoint', None))]
    ds = mirror.isentropic_interpolation(K.LEVELS[::-1], *da, temperature_out=True)
    for k, want in (('pressure', full['pressure']), ('temperature', full['temperature']), ('dewpoint', full['vars'][0]),
                    ('var1', full['vars'][1])):
        assert ds[k].dims == ('isentropic_level', 'y', 'x') and np.array_equal(np.asarray(ds[k].coords['isentropic_level']), K.LEVELS)
        assert np.array_equal(np.asarray(ds[k].values).reshape(16, -1), want, equal_nan=True), k
    assert np.array_equal(np.asarray(ds['status'].values).reshape(-1), full['status']) and ds['status'].dims == ('y', 'x')
