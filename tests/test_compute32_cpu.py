"""xp_opts.compute = XP_F32 without a GPU: the census of doubt columns at the committed XP_F32_GUARD, the resources of the
new translation unit as the compiler reports them, and the ctypes surface."""
import numpy as np
import pytest

from tests import compute32_cases as cc
from tests.resource_report import needs_hipcc, resources
from xarray_parcel_amd import _lib


@pytest.mark.parametrize('name', cc.CENSUS_GRIDS)
def test_census_bounds(name):
    """At the committed guard the refinement branch runs (at least 5 doubt columns that are not saturated parcels, whose
    node on the LCL is a doubt node of its own kind) and stays rare (at most 10 % doubt columns).  The reference alone, on
    these two grids: 0.3 % / 0.5 % at 1e-4 K, 3.9 % / 1.7 % at 5e-4 K, 5.8 % / 5.9 % at 2e-3 K, 9.0 % / 13.4 % at 5e-3 K: a
    guard above 2e-3 K would mean an error analysis that is too loose."""
    g = cc.guard()
    assert 0.0 < g <= 2e-3, g
    c = cc.census(name)
    n = c['doubt'].size
    assert n == 6007
    unsaturated = int((c['doubt'] & ~c['saturated']).sum())
    share = c['doubt'].mean()
    print('%s: guard %.1e K, doubt columns %d of %d (%.2f %%), %d of them not saturated' % (name, g, int(c['doubt'].sum()), n, 100 * share, unsaturated))
    assert unsaturated >= 5, unsaturated
    assert share <= 0.10, share


def test_grids_are_float32_and_ragged():
    for name in cc.GRIDS:
        p, t, td = cc.grid(name)
        assert p.dtype == t.dtype == td.dtype == np.float32 and p.shape == t.shape == td.shape, name
    assert cc.grid('hashed64')[0].shape == (64, 6007) and cc.grid('hashed128')[0].shape == (128, 6007)
    assert cc.grid('layered48')[0].shape == (48, 6007)
    assert cc.grid('one_level')[0].shape == (1, 257) and cc.grid('two_levels')[0].shape == (2, 257)
    assert cc.grid('one_column')[0].shape[1] == 1 and cc.grid('no_columns')[0].shape[1] == 0
    assert np.isnan(cc.grid('hashed64')[1]).any() and cc.census('hashed64')['saturated'].any()
    # the edge grid leaves the family table on every side: above its top (~20.1 hPa), above 1100 hPa, and through NaN pressures
    p = cc.grid('edges')[0]
    ref = cc.oracle('edges')
    with np.errstate(invalid='ignore'):
        assert (np.nanmin(p, axis=0) < 20.0).sum() >= 300 and (p[0, list(cc.EDGE_HIGH_SURFACE)] > 1100.0).all()
        assert (ref['lcl_pressure'][list(cc.EDGE_HIGH_SURFACE)] > 1100.0).all() and (ref['cape'][list(cc.EDGE_HIGH_SURFACE)] > 500.0).sum() >= 3
        holes = np.isnan(p)
        assert holes.any(axis=0).sum() >= 100
        above = np.where(holes, np.roll(p, 1, axis=0), np.nan)            # the pressure of the level below each hole
        assert np.nanmax(above - ref['lcl_pressure'][None, :]) < 0.0       # every hole lies above its column's LCL


def test_sharded_cape_cin_forwards_a_string_compute(monkeypatch):
    """distributed.sharded_cape_cin's `compute` is the stand-in callable of the CPU rehearsal; a string is numpy_api's compute=
    keyword and reaches cape_cin_columns with the other keywords."""
    import torch
    from xarray_parcel_amd import distributed, numpy_api
    seen = {}

    def fake(p, t, td, want=None, **kw):
        seen.update(kw, want=want)
        return {k: np.zeros(3, np.float32) for k in want}

    monkeypatch.setattr(numpy_api, 'cape_cin_columns', fake)
    monkeypatch.setattr(distributed, 'gather_columns', lambda local, names, dst=0, group=None: local)
    out = distributed.sharded_cape_cin(None, None, None, compute='float32', moist='family')
    assert seen == {'compute': 'float32', 'moist': 'family', 'want': ('cape', 'cin')} and set(out) == {'cape', 'cin'}
    seen.clear()
    distributed.sharded_cape_cin(None, None, None, moist='family')
    assert 'compute' not in seen
    seen.clear()
    distributed.sharded_cape_cin(None, None, None, compute=lambda *a, **kw: fake(*a, **dict(kw, marker=1)))
    assert seen.get('marker') == 1 and 'compute' not in seen


@needs_hipcc
def test_kernel_resources(tmp_path):
    """The new translation unit cross-compiles for gfx950; its kernel has no scratch and no spill, and its workgroup's LDS
    fits a CU (the numbers themselves: DESIGN.md 3)."""
    assert ('cape_f32', 'xp_cape_f32_tu.hip', _lib.CAPE_F32_FLAGS) in _lib.UNITS
    rec = resources(tmp_path, 'xp_cape_f32_tu.hip', _lib.CAPE_F32_FLAGS)
    kernels = {n: r for n, r in rec.items() if 'k_cape_f32' in n}
    assert len(kernels) == 2, list(rec)                      # the ordinary launch and the persistent wavefronts
    for n, r in kernels.items():
        print(n, r)
        assert r['in_asm'], n
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['spills'] == 0 and r['scratch_insts'] == 0, (n, r)
        assert r['lds'] <= 160 * 1024, (n, r)


def test_ctypes_exposes_compute():
    assert _lib.XP_F32 == 0 and _lib.XP_F64 == 1
    assert _lib.COMPUTE == {'float32': _lib.XP_F32, 'float64': _lib.XP_F64}
    o = _lib.Opts(1, 1, 1, 0, _lib.MOIST['family'], _lib.XP_F32, 0, 0)
    assert o.compute == _lib.XP_F32 and [f for f, _ in _lib.Opts._fields_][5] == 'compute'
    from xarray_parcel_amd import numpy_api
    assert numpy_api._opts(compute='float32').compute == _lib.XP_F32 and numpy_api._opts().compute == _lib.XP_F64
    with pytest.raises(AssertionError):
        numpy_api._opts(compute='float16')
    assert set(numpy_api.COMPUTE32_WANT) == set(_lib.SCALAR_F + _lib.SCALAR_I + _lib.SCALAR_P) - {
        'lfc_temperature', 'el_temperature', 'lfc_index', 'el_index', 'status'}
