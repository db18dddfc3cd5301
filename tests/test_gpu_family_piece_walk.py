"""The CAPE / CIN-only family kernels of the surface and explicit parcels keep TWO coefficient sets in the walk above the
LCLs (Family::locate / Family::value, csrc/xp_device.hpp): the lanes of a wavefront cross an x-piece boundary over several
levels, and the ones that have crossed take the next piece's coefficients while the others keep theirs.  What a column
gets must not depend on its wave-mates, so for every case below

  (a) the CAPE / CIN-only call equals the all-outputs call (the generic kernel, which reloads every lane: Family::at)
      bit for bit, and the all-outputs call agrees with the C oracle's family mode at 1e-6;
  (b) permuting the columns permutes the outputs bit for bit.

Shapes (64-column tiles of synth.columns(seed=77); reload levels counted on the CPU with the kernel's piece rule,
floor((ln 1100 - ln p) / 0.5)): 33 levels -- 8 levels with a reload per tile, 5 of them with only some lanes moving; 24
levels -- 7 and 4; 8 and 6 levels -- every tile has a lane that skips a piece, i.e. the reload-everybody path.  Then a tile
of 64 copies of one column (every lane moves together), a tile with one odd column (one lane moves alone), columns that
reach above the table top (~20 hPa), a surface above 1100 hPa (served by the RK4 fix-up), NaN temperatures, NaN
pressures, ragged column counts, both dtypes, both parcels -- and all of it once more with persistent wavefronts
(XP_PERSIST_MIN_COLS = 0 is read once per process: a child process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import test_gpu_parity as tp
from xarray_parcel_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN = ('cape', 'cin')


def _base(nlev, ncol, dtype, **kw):
    return synth.columns(nlev=nlev, ncol=ncol, seed=77, dtype=dtype, **kw)


def _copies(nlev, dtype):
    p, t, td = _base(nlev, 64, dtype)
    return tuple(np.ascontiguousarray(np.repeat(a[:, 5:6], 64, axis=1)) for a in (p, t, td))


def _one_odd(nlev, dtype):
    p, t, td = _base(nlev, 64, dtype)
    out = [np.repeat(a[:, 5:6], 64, axis=1) for a in (p, t, td)]
    for o, a in zip(out, (p, t, td)):
        o[:, 17] = a[:, 40]
    return tuple(np.ascontiguousarray(o) for o in out)


def _low_top(nlev, dtype):
    # every third column stretched so that its top level lies at 12 hPa: the upper levels leave the table (dry continuation)
    p, t, td = _base(nlev, 1000, np.float64)
    k = np.arange(nlev, dtype=np.float64)[:, None] / (nlev - 1)
    r = (12.0 / p[-1, ::3])[None, :] ** k
    p[:, ::3] = p[:, ::3] * r
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (p, t, td))


def _high_surface(nlev, dtype):
    p, t, td = _base(nlev, 200, np.float64)
    p[0, 70] = 1105.0
    td[0, 70] = t[0, 70] - 0.2                      # LCL above 1100 hPa: outside the table, flagged, redone by the RK4 kernel
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (p, t, td))


# name -> (builder(dtype) -> (p, t, td), dtypes, parcels)
BOTH, F64 = (np.float64, np.float32), (np.float64,)
CASES = {
    'lev33': (lambda d: _base(33, 4097, d), BOTH, ('surface', 'explicit')),
    'lev24': (lambda d: _base(24, 4097, d), BOTH, ('surface', 'explicit')),
    'lev8': (lambda d: _base(8, 4097, d), BOTH, ('surface', 'explicit')),
    'lev6': (lambda d: _base(6, 4097, d), BOTH, ('surface', 'explicit')),
    'one_column': (lambda d: _base(33, 1, d), BOTH, ('surface',)),
    'ncol63': (lambda d: _base(33, 63, d), BOTH, ('surface', 'explicit')),
    'copies': (lambda d: _copies(33, d), BOTH, ('surface', 'explicit')),
    'one_odd': (lambda d: _one_odd(33, d), BOTH, ('surface', 'explicit')),
    'low_top': (lambda d: _low_top(33, d), BOTH, ('surface', 'explicit')),
    'high_surface': (lambda d: _high_surface(33, d), F64, ('surface',)),
    'nan_levels': (lambda d: _base(33, 4097, d, nan_fraction=0.08), BOTH, ('surface', 'explicit')),
    'nan_pressure': (lambda d: _base(33, 4097, d, nan_fraction=0.08, nan_pressure_fraction=0.05), BOTH, ('surface', 'explicit')),
}
PARAMS = [(n, d, pc) for n, (_, ds, pcs) in CASES.items() for d in ds for pc in pcs]


def _call(xa, p, t, td, parcel, ex, want=None):
    kw = dict(parcel=parcel, moist='family')
    if parcel == 'explicit':
        kw['parcel_values'] = ex
    if want is not None:
        kw['want'] = want
    return xa.cape_cin_columns(p, t, td, **kw)


def _against_oracle(name, p, t, td, parcel, ex, full, dtype):
    okw = dict(parcel=parcel, moist='family')
    if parcel == 'explicit':
        okw['parcel_values'] = np.stack(ex)
    got = {k: np.asarray(v) for k, v in full.items() if k != 'profile'}
    ref = co.cape_cin_grid(p, t, td, **okw)
    if name != 'nan_pressure':
        tp._compare(got, ref, dtype, 1e-6)
        return
    # A NaN PRESSURE is outside the reference's input contract, and tests/test_gpu_parity.py::test_nan_pressure_levels states
    # what the kernels do with one: above the LCL the reference's own reading (an all-NaN node); below it a MISSING level
    # (status bit 4), not the reference's insert_level artefact -- stated there for holes at least two levels below the
    # LCL's lower bracket.  The same split here: columns without a hole or with it above the first level over the LCL
    # against the oracle as they stand, columns with it that far below against the oracle on the missing-level reading;
    # the few with the hole next to the LCL are left to (a)'s bitwise comparison with the generic kernel and to (b).
    p0 = _base(p.shape[0], p.shape[1], dtype, nan_fraction=0.08)[0]
    hole = np.isnan(p)
    kh = np.where(hole.any(axis=0), hole.argmax(axis=0), -1)
    base = co.cape_cin_grid(p0, t, td, **okw)
    with np.errstate(invalid='ignore'):
        first_above = np.argmax(p0.astype(np.float64) < base['lcl_pressure'][None, :], axis=0)
    as_is = (kh < 0) | (kh > first_above)
    below = (kh >= 1) & (kh <= first_above - 3)
    assert as_is.sum() > 0.9 * as_is.size and below.sum() >= 20, (int(as_is.sum()), int(below.sum()))
    tp._compare({k: v[as_is] for k, v in got.items()}, {k: v[as_is] for k, v in ref.items()}, dtype, 1e-6)
    assert np.all(got['status'][below] & 4)
    t2, td2 = t[:, below].copy(), td[:, below].copy()
    t2[hole[:, below]] = np.nan; td2[hole[:, below]] = np.nan
    okw2 = dict(okw)
    if parcel == 'explicit':
        okw2['parcel_values'] = np.ascontiguousarray(np.stack(ex)[:, below])
    miss = co.cape_cin_grid(np.ascontiguousarray(p0[:, below]), t2, td2, **okw2)
    g = {k: v[below] for k, v in got.items()}
    g['status'] = g['status'] & ~4
    tp._compare(g, miss, dtype, 1e-6)


def check_case(xa, name, dtype, parcel):
    p, t, td = CASES[name][0](dtype)
    ncol = p.shape[1]
    ex = (p[0] + 5.0, t[0] + 1.0, td[0] - 1.0) if parcel == 'explicit' else None
    full = _call(xa, p, t, td, parcel, ex)
    lean = _call(xa, p, t, td, parcel, ex, LEAN)
    # (a) the two-set walk against the generic kernel, bit for bit; the generic kernel against the oracle
    for k in LEAN:
        assert np.array_equal(np.asarray(lean[k]), np.asarray(full[k]), equal_nan=True), (name, dtype.__name__, parcel, k)
    _against_oracle(name, p, t, td, parcel, ex, full, dtype)
    # (b) a column does not see its wave-mates
    perm = np.random.default_rng(5).permutation(ncol)
    pp, tt, dd = (np.ascontiguousarray(a[:, perm]) for a in (p, t, td))
    exp_ = tuple(np.ascontiguousarray(a[perm]) for a in ex) if ex is not None else None
    lean_p = _call(xa, pp, tt, dd, parcel, exp_, LEAN)
    for k in LEAN:
        assert np.array_equal(np.asarray(lean_p[k]), np.asarray(lean[k])[perm], equal_nan=True), (name, dtype.__name__, parcel, k, 'permuted')


@pytest.fixture(scope='module')
def xa():
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    own = numpy_api.family_table()
    numpy_api.set_family_table(co.family_table())          # both sides interpolate the same numbers (test_gpu_parity.family_tables)
    yield numpy_api
    numpy_api.set_family_table(own)


@pytest.mark.gpu
@pytest.mark.parametrize('name,dtype,parcel', PARAMS, ids=['%s-%s-%s' % (n, d.__name__, pc) for n, d, pc in PARAMS])
def test_two_set_walk_matches_the_generic_kernel_and_ignores_wave_mates(xa, name, dtype, parcel):
    check_case(xa, name, dtype, parcel)


def run_all():
    """Every case in this process (the child of the persistent-launch test)."""
    from xarray_parcel_amd import numpy_api
    numpy_api.set_family_table(co.family_table())
    for name, dtype, parcel in PARAMS:
        check_case(numpy_api, name, dtype, parcel)
    print('PIECE_WALK_OK')


@pytest.mark.gpu
def test_two_set_walk_with_persistent_wavefronts():
    env = dict(os.environ, XP_PERSIST_MIN_COLS='0')
    code = 'import sys; sys.path.insert(0, %r); from tests import test_gpu_family_piece_walk as m; m.run_all()' % ROOT
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and 'PIECE_WALK_OK' in out.stdout, out.stderr[-3000:]
