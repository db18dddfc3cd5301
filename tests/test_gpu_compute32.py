"""xp_opts.compute = XP_F32 on the GPU (csrc/xp_cape_f32.hpp; the contract: include/xparcel.h at xp_opts.compute): the
fp32-arithmetic surface CAPE / CIN against the untouched fp64 family path (classification, every column, no exemptions)
and against the C oracle (values), what it rejects, and that nothing else moved.  Grids: tests/compute32_cases.py.

Measured on an MI355X (the maxima test_values_against_the_oracle prints, all grids): |dCAPE| 0.021 J/kg, |dCIN| 0.008
J/kg against the bound of 0.5 J/kg; LFC / EL |d ln p| at most 0.18 / 0.08 of the propagated bound."""
import numpy as np
import pytest

from tests import compute32_cases as cc
from xarray_parcel_amd import _lib as L

pytestmark = pytest.mark.gpu

xa = None
NONEMPTY = tuple(g for g in cc.GRIDS if g != 'no_columns')
LCL_PARCEL = ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'parcel_index', 'parcel_pressure',
              'parcel_temperature', 'parcel_dewpoint')
_cache = {}


@pytest.fixture(scope='module', autouse=True)
def _api():
    global xa
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from xarray_parcel_amd import numpy_api
    xa = numpy_api
    yield
    _cache.clear()


def f32(name):
    """The fp32-arithmetic result on host arrays, computed once per grid."""
    if ('f32', name) not in _cache:
        _cache['f32', name] = xa.cape_cin_columns(*cc.grid(name), moist='family', compute='float32')
    return _cache['f32', name]


def f64(name):
    """The fp64 family path on the same inputs: the all-outputs kernel (indices for the tie classification below)."""
    if ('f64', name) not in _cache:
        _cache['f64', name] = xa.cape_cin_columns(*cc.grid(name), moist='family', compute='float64')
    return _cache['f64', name]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def rejected(fn):
    with pytest.raises(L.XParcelError) as e:
        fn()
    assert e.value.code == L.XP_E_ARG, e.value
    assert 'compute' in str(e.value), e.value              # the message names the offending argument
    return str(e.value)


@pytest.mark.parametrize('name', cc.GRIDS)
def test_feature_works_on_every_grid_and_input_kind(name):
    """Host arrays, device tensors and a strided device view give the same bits; XP_E_ARG before this feature."""
    import torch
    p, t, td = cc.grid(name)
    host = f32(name)
    assert set(host) == set(xa.COMPUTE32_WANT)
    ncol = p.shape[1]
    for k in xa.COMPUTE32_WANT:
        assert np.asarray(host[k]).shape == (ncol,) and np.asarray(host[k]).dtype == (np.int32 if k == 'parcel_index' else np.float32), k
    if ncol == 0:
        return
    assert np.isfinite(host['cape']).all() and np.isfinite(host['cin']).all() and (host['cin'] <= 0).all()
    dev = xa.cape_cin_columns(*(torch.from_numpy(np.array(a)).cuda() for a in (p, t, td)), moist='family', compute='float32')
    for k in xa.COMPUTE32_WANT:
        assert same(dev[k].cpu().numpy(), host[k]), k
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev = p.shape[0]
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (p, t, td)]
    views = [L.View(x.data_ptr(), L.XP_F32, L.XP_MEM_DEVICE, nlev, ncol, 1, nlev) for x in cols]
    outs = {k: torch.empty(ncol, dtype=torch.int32 if k == 'parcel_index' else torch.float32, device='cuda') for k in xa.COMPUTE32_WANT}
    so = L.ScalarsOut(dtype=L.XP_F32, mem=L.XP_MEM_DEVICE, **{k: v.data_ptr() for k, v in outs.items()})
    L.check(lib.xp_cape_cin(*views, L.Parcel(L.PARCEL['surface'], 0, 100.0, None, None, None),
                            xa._opts(moist='family', compute='float32'), so, None, None))
    torch.cuda.synchronize()
    for k in xa.COMPUTE32_WANT:
        assert same(outs[k].cpu().numpy(), host[k]), k


@pytest.mark.parametrize('name', NONEMPTY)
def test_classification_is_the_fp64_paths(name):
    """Every column, no exemptions: the NaN patterns of CAPE, CIN and the LFC / EL pressures are the fp64 family path's,
    and the LCL and parcel outputs are bit-identical to it."""
    a, b = f32(name), f64(name)
    for k in ('cape', 'cin', 'lfc_pressure', 'el_pressure'):
        na, nb = np.isnan(np.asarray(a[k])), np.isnan(np.asarray(b[k]))
        assert np.array_equal(na, nb), (name, k, np.nonzero(na != nb)[0][:10])
    for k in LCL_PARCEL:
        assert same(a[k], b[k]), (name, k)
    # which of the two replaces the LFC by the LCL is a classification too: where the fp64 path does, so does the walk
    lfc_is_lcl = np.asarray(b['lfc_index']) == -2
    assert same(np.asarray(a['lfc_pressure'])[lfc_is_lcl], np.asarray(b['lfc_pressure'])[lfc_is_lcl]), name


def test_unserved_columns_take_the_rk4_launch():
    """A column whose LCL lies outside the family table (above 1100 hPa) is flagged by the fp32 pass and redone by the
    only_flagged RK4 launch: its outputs are the RK4 kernel's, bit for bit -- moist='exact' with the same request -- and not
    what a family pass leaves behind for a poisoned lane.  The grid also holds columns above the table's top (the fp32 dry
    continuation and its fp64 twin) and NaN pressures above the LCL; the classification and value tests run on it."""
    p, t, td = cc.grid('edges')
    got, full = f32('edges'), f64('edges')
    unserved = np.asarray(full['lcl_pressure'], dtype=np.float64) > 1100.0
    hs = list(cc.EDGE_HIGH_SURFACE)
    assert unserved[hs].all()
    exact = xa.cape_cin_columns(p, t, td, moist='exact', want=xa.COMPUTE32_WANT)
    for k in xa.COMPUTE32_WANT:
        assert same(np.asarray(got[k])[unserved], np.asarray(exact[k])[unserved]), k
    # (what a family pass alone leaves for such a lane is a NaN parcel above the LCL: no CAPE, no LFC, no EL)
    assert (np.asarray(got['cape'])[hs] > 500.0).sum() >= 3 and (~np.isnan(np.asarray(got['el_pressure'])[hs])).sum() >= 3
    served = ~unserved & ~np.isnan(np.asarray(full['lcl_pressure']))
    assert not same(np.asarray(got['cape'])[served], np.asarray(exact['cape'])[served])     # the others did not come from there
    with np.errstate(invalid='ignore'):
        # walks that pass the table's top, and whose EL hangs on the sign of the last node up there
        assert ((np.nanmin(p, axis=0) < 20.0) & (np.asarray(got['cape']) > 0) & ~np.isnan(np.asarray(got['el_pressure']))).sum() >= 50


# The reference of the value test, per grid.  The C oracle's RK4 ascent on the float32-rounded inputs (an ascent that
# owes nothing to the family table) -- except on the layered grid, which takes the oracle's family ascent, as tests/test_gpu_layered.py does for
# family-mode kernels on that grid: its values are multiples of 1/64 K chosen to put nodes ON the knife edges, and on 46 of its
# 195 saturated columns the oracle's own two ascents disagree about the LFC interval (tests/test_gpu_parity.py's sign and label
# ties: the RK4 and the family adiabat differ by 2e-5 K where the tie is decided by 1e-14 K).  Against the RK4 ascent the fp64
# family path -- untouched code -- has 16 sign ties there, one more than that file's cap of 15 admits, so the comparison
# cannot be made under its caps with either arithmetic; the sixteenth column differs by 2810 J/kg in both.
VALUE_REFERENCE = {name: 'family' if name == 'layered48' else 'rk4' for name in NONEMPTY}


@pytest.mark.parametrize('name', NONEMPTY)
def test_values_against_the_oracle(name):
    """CAPE / CIN within 0.5 J/kg (+ float32 rounding) of the C oracle on the float32-rounded inputs; an LFC / EL in the
    oracle's interval (a, b) within the propagated bound 2 GUARD |x_b - x_a| / |y_b - y_a| + 2e-7 in ln p (index -2, the
    LCL: to rounding).  Left out: tests/test_gpu_parity.py's saturated-parcel sign ties of the fp64 family path (which the
    walk classifies like: test_classification_is_the_fp64_paths) against the same reference, under its own caps."""
    from tests.test_gpu_parity import _saturated_tie_columns
    g = cc.guard()
    got, ref = f32(name), cc.oracle(name, VALUE_REFERENCE[name])
    _, excluded = _saturated_tie_columns(f64(name), ref)
    keep = ~excluded
    worst, failures = {}, []
    for k in ('cape', 'cin'):
        a, b = np.asarray(got[k], dtype=np.float64), ref[k]
        err = np.abs(a - b)[keep]
        tol = 0.5 + 2e-7 * np.maximum(np.abs(b[keep]), 1.0)
        worst[k] = float(err.max(initial=0.0))
        if not np.all(err <= tol):
            failures.append((k, worst[k]))
    prof = ref['profile']
    with np.errstate(invalid='ignore', divide='ignore'):
        x = np.log(prof['pressure'])
        y = prof['virtual_temperature'] - prof['environment_virtual_temperature']
    cols = np.arange(x.shape[1])
    for key, kp, ki in (('lfc', 'lfc_pressure', 'lfc_index'), ('el', 'el_pressure', 'el_index')):
        a, b, i = np.asarray(got[kp], dtype=np.float64), ref[kp], ref[ki]
        assert np.array_equal(np.isnan(a[keep]), np.isnan(b[keep])), (name, kp)
        both = keep & ~np.isnan(b)
        at_lcl = both & (i == -2)
        r = b[at_lcl].astype(np.float32).astype(np.float64)
        if not np.all(np.abs(a[at_lcl] - r) <= 2e-7 * np.maximum(np.abs(r), 1.0)):
            failures.append((key, 'at the LCL'))
        inside = both & (i >= 0)
        ii = np.where(inside, i, 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            bound = 2.0 * g * np.abs(x[ii + 1, cols] - x[ii, cols]) / np.abs(y[ii + 1, cols] - y[ii, cols]) + 2e-7
            dlnp = np.abs(np.log(a) - np.log(b))
        ratio = (dlnp / bound)[inside]
        worst[key] = float(ratio.max(initial=0.0))
        if not np.all(dlnp[inside] <= bound[inside]):
            failures.append((key, worst[key]))
    print('compute32 %s (%s oracle, %d columns left out): |dCAPE| %.5f J/kg, |dCIN| %.5f J/kg (bound 0.5); LFC |d ln p| / bound %.4f, EL %.4f (bound 1)' %
          (name, VALUE_REFERENCE[name], int(excluded.sum()), worst['cape'], worst['cin'], worst['lfc'], worst['el']))
    assert not failures, (name, failures)


def test_rejections():
    """Everything outside the contract is XP_E_ARG with a message that names xp_opts.compute."""
    p, t, td = (np.array(a[:, :64]) for a in cc.grid('hashed64'))
    ok = dict(moist='family', compute='float32')
    call = lambda *a, **kw: (lambda: xa.cape_cin_columns(*a, **{**ok, **kw}))
    assert 'XP_F32' in rejected(call(*(a.astype(np.float64) for a in (p, t, td))))
    for moist in ('exact', 'table'):
        assert 'moist_mode' in rejected(call(p, t, td, moist=moist))
    for parcel in ('most_unstable', 'mixed_layer'):
        assert 'parcel' in rejected(call(p, t, td, parcel=parcel))
    assert 'parcel' in rejected(call(p, t, td, parcel='explicit', parcel_values=(p[0], t[0], td[0])))
    for opt in (dict(virtual_temperature_correction=False), dict(lcl_interp='linear'), dict(pos_cape_neg_cin=False), dict(post_zero_cin=True)):
        assert 'defaults' in rejected(call(p, t, td, **opt))
    assert 'lfc_index' in rejected(call(p, t, td, want=('lfc_index',)))
    for k in ('lfc_temperature', 'el_temperature', 'el_index', 'status'):
        rejected(call(p, t, td, want=('cape', k)))
    assert 'profile' in rejected(call(p, t, td, want_profile=True))
    assert 'profile' in rejected(call(p, t, td, lifted_index_at=500.0))
    assert 'humidity' in rejected(call(p, t, td, humidity='specific'))
    rejected(lambda: xa.cape_cin_multi(p, t, td, ['surface'], **ok))
    rejected(lambda: xa.surface_based_cape_cin(p, t, td, **ok))          # it returns the profile
    # the other entry points that take an xp_opts keep rejecting it
    rejected(lambda: xa.cape_cin_layers(p, t, td, [{'top': 500.0}], compute='float32'))
    # an unknown value is rejected as before
    lib = L.init(0)
    o = xa._opts(moist='family')
    o.compute = 7
    v = [L.View(a.ctypes.data, L.XP_F32, L.XP_MEM_HOST, p.shape[0], 64, 64, 1) for a in (p, t, td)]
    cape = np.empty(64, np.float32)
    rc = lib.xp_cape_cin(*v, L.Parcel(0, 0, 100.0, None, None, None), o, L.ScalarsOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST, cape=cape.ctypes.data), None, None)
    assert rc == L.XP_E_ARG and b'compute' in lib.xp_last_error()


@pytest.fixture(scope='module')
def lookup_tables():
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    adiabat_tables.set_tables(tab.index, tab.adiabats)


@pytest.mark.parametrize('moist', ['exact', 'table', 'family'])
def test_default_is_unchanged(moist, lookup_tables):
    """compute=None is compute='float64', bit for bit, for the all-outputs and for the CAPE/CIN-only request."""
    p, t, td = cc.grid('hashed64')
    for want in (None, xa.COMPUTE32_WANT):
        a = xa.cape_cin_columns(p, t, td, moist=moist, want=want)
        b = xa.cape_cin_columns(p, t, td, moist=moist, want=want, compute='float64')
        assert set(a) == set(b)
        for k in a:
            assert same(a[k], b[k]), (moist, k)
    if moist == 'family':
        for k in xa.COMPUTE32_WANT:                  # ... and the all-outputs result is the f64() the other tests compare with
            assert same(a[k], f64('hashed64')[k]), k


def test_set_compute_is_a_preference():
    """set_compute('float32') switches the calls the contract covers and leaves the others in fp64, where the keyword raises."""
    p, t, td = cc.grid('two_levels')
    ref32, ref64 = f32('two_levels'), f64('two_levels')
    xa.set_compute('float32')
    try:
        got = xa.cape_cin_columns(p, t, td, moist='family')
        assert set(got) == set(xa.COMPUTE32_WANT) and all(same(got[k], ref32[k]) for k in got)
        full = xa.cape_cin_columns(p, t, td, moist='family', want=L.SCALAR_F + L.SCALAR_I + L.SCALAR_P)      # not covered: fp64
        assert all(same(full[k], ref64[k]) for k in full)
        mu = xa.cape_cin_columns(p, t, td, moist='family', parcel='most_unstable', want=('cape',))
        assert same(mu['cape'], xa.cape_cin_columns(p, t, td, moist='family', parcel='most_unstable', want=('cape',), compute='float64')['cape'])
        assert same(xa.cape_cin_columns(p, t, td, moist='exact', want=('cape',))['cape'],
                    xa.cape_cin_columns(p, t, td, moist='exact', want=('cape',), compute='float64')['cape'])
    finally:
        xa.set_compute('float64')


def test_the_fp32_table_follows_the_fp64_table():
    """The fp32 coefficients are derived from the fp64 table the library holds: replacing that table by itself leaves the fp32
    result unchanged, and replacing it by the oracle's independently built copy moves the fp32 result with the fp64 one."""
    from oracle import c_oracle as co
    p, t, td = cc.grid('hashed128')
    own = xa.family_table()
    before = f32('hashed128')
    try:
        xa.set_family_table(own)
        again = xa.cape_cin_columns(p, t, td, moist='family', compute='float32')
        assert all(same(again[k], before[k]) for k in before)
        xa.set_family_table(co.family_table())
        a32 = xa.cape_cin_columns(p, t, td, moist='family', compute='float32')
        a64 = xa.cape_cin_columns(p, t, td, moist='family', want=xa.COMPUTE32_WANT)
        for k in ('lfc_pressure', 'el_pressure'):
            assert np.array_equal(np.isnan(a32[k]), np.isnan(a64[k])), k
        assert np.max(np.abs(np.asarray(a32['cape'], dtype=np.float64) - np.asarray(a64['cape'], dtype=np.float64))) <= 0.5
    finally:
        xa.set_family_table(own)
    assert all(same(xa.cape_cin_columns(p, t, td, moist='family', compute='float32')[k], before[k]) for k in before)


PERSISTENT = '''
import sys
sys.path.insert(0, %r)
import numpy as np
from tests import compute32_cases as cc
from xarray_parcel_amd import numpy_api as xa
out = {}
for name in %r:
    res = xa.cape_cin_columns(*cc.grid(name), moist='family', compute='float32')
    out.update({name + '/' + k: np.asarray(v) for k, v in res.items()})
np.savez(sys.argv[1], **out)
print('COMPUTE32_PERSISTENT_OK')
'''


def test_persistent_wavefronts(tmp_path):
    """The grids the fp64 family kernel walks with persistent wavefronts (persist(), xparcel.hip) take k_cape_f32's
    persistent instantiation: forced onto the small grids (XP_PERSIST_MIN_COLS = 0 is read once per process: a fresh child,
    as tests/test_gpu_persistent.py starts one), it gives the ordinary launch's bits -- a wavefront holds the same 64 columns."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ('hashed64', 'hashed128', 'layered48', 'edges', 'two_levels', 'one_column')
    path = str(tmp_path / 'persistent.npz')
    out = subprocess.run([sys.executable, '-c', PERSISTENT % (root, names), path], env=dict(os.environ, XP_PERSIST_MIN_COLS='0'),
                         capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0 and 'COMPUTE32_PERSISTENT_OK' in out.stdout, out.stderr[-3000:]
    with np.load(path) as z:
        for name in names:
            for k, v in f32(name).items():
                assert same(z[name + '/' + k], v), (name, k)
