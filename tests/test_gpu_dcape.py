"""Downdraft CAPE on the device (xp_downdraft_cape) against the NumPy restatement tests/dcape_restatement.py, the
existing entry points it shares its code with, and its own argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dcape_restatement as R
from tests.test_dcape_cpu import saturated_column
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ('dcape', 'start_pressure', 'start_temperature', 'status', 'parcel_temperature')


def inputs(nlev, ncol, seed, dtype=np.float64):
    """synth.columns with missing levels, plus hand-built elevated columns (the lowest levels dropped: surfaces at
    640 ... 730 hPa, below 700 hPa for half of them) and truncated ones (levels above 470 ... 530 hPa dropped)."""
    p, t, td = (np.array(a) for a in synth.columns(nlev=nlev, ncol=ncol, seed=seed, nan_fraction=0.1, dtype=np.float64))
    rng = np.random.default_rng(seed)
    n = ncol // 8
    for c, cut in zip(range(n), rng.uniform(640.0, 730.0, n)):
        gone = p[:, c] > cut
        p[gone, c] = t[gone, c] = td[gone, c] = np.nan
    for c, cut in zip(range(n, 2 * n), rng.uniform(470.0, 530.0, n)):
        gone = p[:, c] < cut
        p[gone, c] = t[gone, c] = td[gone, c] = np.nan
    return p.astype(dtype), t.astype(dtype), td.astype(dtype)


def restate(p, t, td, moist='rk4', cols=None, **kw):
    p, t, td = (np.asarray(a, dtype=np.float64) for a in (p, t, td))
    cols = list(range(p.shape[1])) if cols is None else list(cols)
    ref = R.grid(p, t, td, cols=cols, moist=moist, **kw)
    tie = np.array([R.near_tie(p[:, c], t[:, c], td[:, c], **kw) for c in cols])
    assert tie.sum() <= 0.01 * len(cols), tie.sum()
    return ref, tie


def compare(got, ref, keep, f32=False, dcape_tol=(1e-6, 1e-9), t_tol=1e-8):
    g = {k: np.asarray(got[k])[..., keep] if k != 'parcel_temperature' else np.asarray(got[k])[:, keep] for k in KEYS}
    r = {k: np.asarray(ref[k])[..., keep] if k != 'parcel_temperature' else np.asarray(ref[k])[:, keep] for k in KEYS}
    assert np.array_equal(g['status'], r['status'])
    for k in KEYS[:3] + KEYS[4:]:
        gk, rk = g[k].astype(np.float64), r[k]
        assert np.array_equal(np.isnan(gk), np.isnan(rk)), (k, np.argwhere(np.isnan(gk) != np.isnan(rk))[:5])
        ok = ~np.isnan(rk)
        if k == 'start_pressure':
            want = rk[ok].astype(np.float32).astype(np.float64) if f32 else rk[ok]
            assert np.array_equal(gk[ok], want), k
            continue
        tol = (dcape_tol[0] + dcape_tol[1] * np.abs(rk[ok])) if k == 'dcape' else np.full(ok.sum(), t_tol)
        if f32:
            tol = tol + np.spacing(np.abs(rk[ok]).astype(np.float32)).astype(np.float64)
        err = np.abs(gk[ok] - rk[ok])
        assert np.all(err <= tol), (k, float(err.max()), np.argwhere(ok)[np.argmax(err - tol)])


@pytest.mark.parametrize('nlev', [12, 40])
def test_exact_mode_vs_rk4_restatement(nlev):
    p, t, td = inputs(nlev, 640, seed=nlev)
    got = xa.downdraft_cape(p, t, td, moist='exact', want_profile=True)
    ref, tie = restate(p, t, td)
    compare(got, ref, ~tie)
    st = np.asarray(got['status'])
    assert (st == R.ST_NO_LAYER).sum() >= 40 and np.isfinite(np.asarray(got['dcape'])).sum() >= 400


def test_fp32_inputs_round_like_the_restatement():
    p, t, td = inputs(40, 480, seed=5, dtype=np.float32)
    got = xa.downdraft_cape(p, t, td, moist='exact', want_profile=True)
    assert np.asarray(got['dcape']).dtype == np.float32
    ref, tie = restate(p, t, td)
    compare(got, ref, ~tie, f32=True)


def test_exact_mode_vs_ode_restatement():
    p, t, td = inputs(40, 96, seed=8)
    got = xa.downdraft_cape(p, t, td, moist='exact', want_profile=True)
    ref, tie = restate(p, t, td, moist='ode')
    compare(got, ref, ~tie, dcape_tol=(0.2, 0.0), t_tol=1e-3)


@pytest.fixture(scope='module')
def oracle_tables():
    from oracle import parcel_oracle as po
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    adiabat_tables.set_tables(tab.index, tab.adiabats)       # both sides look up the SAME arrays
    po.set_moist_lapse('ode', tab)
    yield tab
    po.set_moist_lapse('ode')


def test_table_mode_vs_table_restatement(oracle_tables):
    p, t, td = inputs(40, 320, seed=11)
    got = xa.downdraft_cape(p, t, td, moist='table', want_profile=True)
    ref, tie = restate(p, t, td, moist='table')
    compare(got, ref, ~tie)
    assert np.isfinite(np.asarray(got['dcape'])).sum() >= 200


def test_saturated_column_has_no_dcape():
    p, t, td = saturated_column()
    got = xa.downdraft_cape(p, t, td, moist='exact')
    assert int(got['status']) == 0 and abs(float(got['dcape'])) < 0.01, got


def _dense_inputs(seed, ncol=512):
    p, t, td = synth.columns(nlev=40, ncol=ncol, seed=seed, dtype=np.float64)
    return np.array(p), np.array(t), np.array(td)


@pytest.mark.parametrize('moist', ['exact', 'table'])
def test_bit_identical_with_wet_bulb_and_moist_lapse(moist, oracle_tables):
    p, t, td = _dense_inputs(21)
    got = xa.downdraft_cape(p, t, td, moist=moist, want_profile=True)
    p0, wb0, prof = got['start_pressure'], got['start_temperature'], got['parcel_temperature']
    assert np.isfinite(p0).all() and np.isfinite(wb0).all()
    wb = xa.wet_bulb_temperature(p, t, td, moist=moist)
    on_level = p == p0[None, :]
    cols = np.nonzero(on_level.any(axis=0))[0]
    assert len(cols) >= 0.5 * p.shape[1]
    k0 = np.argmax(on_level, axis=0)[cols]
    assert np.array_equal(wb0[cols], wb[k0, cols])
    ml = xa.moist_lapse(p, wb0, p0, moist=moist)
    down = p >= p0[None, :]
    assert np.array_equal(prof[down], ml[down]) and np.isnan(prof[~down]).all()


def test_input_kinds_and_strided_views():
    import torch
    p, t, td = inputs(24, 300, seed=4)
    ref = xa.downdraft_cape(p, t, td, want_profile=True)
    cpu = xa.downdraft_cape(*(torch.from_numpy(a) for a in (p, t, td)), want_profile=True)
    dev = xa.downdraft_cape(*(torch.from_numpy(a).cuda() for a in (p, t, td)), want_profile=True)
    for k in KEYS:
        assert np.array_equal(np.asarray(cpu[k]), ref[k], equal_nan=True), k
        assert np.array_equal(dev[k].cpu().numpy(), ref[k], equal_nan=True), k
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev, ncol = p.shape
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, t, td)]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    outs = {k: torch.empty(ncol, dtype=torch.int32 if k == 'status' else torch.float64, device='cuda') for k in KEYS[:4]}
    outs['parcel_temperature'] = torch.empty(nlev, ncol, dtype=torch.float64, device='cuda')
    o = L.DcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, **{k: v.data_ptr() for k, v in outs.items()})
    L.check(lib.xp_downdraft_cape(*views, 700.0, 200.0, L.MOIST['exact'], o, None))
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(outs[k].cpu().numpy(), ref[k], equal_nan=True), k


def test_raw_abi_errors():
    lib = L.init(0)
    p, t, td = (np.ascontiguousarray(a) for a in inputs(12, 8, seed=2))
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 12, 8, 8, 1) for a in (p, t, td)]
    dc = np.empty(8)
    good = dict(dtype=L.XP_F64, mem=L.XP_MEM_HOST, dcape=dc.ctypes.data)

    def call(bottom=700.0, depth=200.0, mode=L.MOIST['exact'], out=True, **o):
        return lib.xp_downdraft_cape(*views, bottom, depth, mode, L.DcapeOut(**{**good, **o}) if out else None, None)
    assert call() == L.XP_OK and np.isfinite(dc).any()
    for kw, word in (({'out': False}, 'out'), ({'dtype': L.XP_F32}, 'out'), ({'mem': L.XP_MEM_DEVICE}, 'out'),
                     ({'bottom': float('nan')}, 'layer_bottom'), ({'bottom': float('inf')}, 'layer_bottom'),
                     ({'bottom': 0.0}, 'layer_bottom'), ({'bottom': -700.0}, 'layer_bottom'),
                     ({'depth': 0.0}, 'layer_depth'), ({'depth': -10.0}, 'layer_depth'), ({'depth': 700.0}, 'layer_depth'),
                     ({'depth': float('nan')}, 'layer_depth'), ({'mode': 7}, 'moist_mode')):
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    if not lib.xp_tables_loaded():
        assert call(mode=L.MOIST['table']) == L.XP_E_NO_TABLES


def test_raw_abi_without_tables():
    """XP_E_NO_TABLES in table mode while no tables are loaded (run in a fresh process: other tests load them)."""
    code = ('import numpy as np; from xarray_parcel_amd import _lib as L; lib = L.init(0); a = np.full((2, 1), 800.0); '
            'v = L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 2, 1, 1, 1); d = np.empty(1); '
            'o = L.DcapeOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, dcape=d.ctypes.data); '
            'print(lib.xp_tables_loaded(), lib.xp_downdraft_cape(v, v, v, 700.0, 200.0, L.MOIST["table"], o, None))')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ['0', str(L.XP_E_NO_TABLES)], out.stdout


def test_full_grid_64_levels_by_1mi_columns():
    import torch
    ncol = 1 << 20
    p, t, td = synth.columns_torch(64, ncol, 'cuda', dtype=torch.float64)
    got = xa.downdraft_cape(p, t, td, moist='exact')
    torch.cuda.synchronize()
    for k in KEYS[:3]:
        assert bool(torch.isfinite(got[k]).all()), k
    assert bool((got['status'] == 0).all())
    cols = np.random.default_rng(0).choice(ncol, 4000, replace=False)
    idx = torch.from_numpy(cols).cuda()
    ps, ts, tds = (x[:, idx].cpu().numpy() for x in (p, t, td))
    del p, t, td
    ref, tie = restate(ps, ts, tds)
    sub = {k: got[k][idx].cpu().numpy() for k in KEYS[:4]}
    sub['parcel_temperature'] = ref['parcel_temperature']          # not asked for on the full grid
    compare(sub, ref, ~tie)
