"""The streaming CAPE / CIN kernels on LAYERED soundings (tests/layered_soundings.py), through the C ABI, against the C oracle.

xarray_parcel_amd.synth gives ascents with at most two positive areas; here a column has up to nine sign changes of parcel
minus environment, the most-unstable parcel starts on any of the lowest twenty levels, the LFC is replaced by the LCL in a
third of the columns, and the net-sum CIN (pos_cape_neg_cin=False) is positive -- so that post_zero_cin acts -- in a third
to a half.  tests/test_layered_soundings_cpu.py holds those numbers.  What is exercised: the bottom-LFC / top-EL selection,
the running-sum snapshots, the net-sum mode over several areas, the gated phase-B walk with lanes that start on widely
different levels, and every finish(post_zero) call site.

Every comparison is tests/test_gpu_parity.py's own (_compare, _saturated_tie_columns: 1e-6 J/kg, 1e-7 hPa / K, indices and
status bit-exact, its float32 rule and its tie caps), or the comparison function of the module that owns the kernel.  The
grids are exact in float32, so both dtypes are held to one oracle run.  Family mode runs on the oracle's table, table
mode on the oracle's tables.  Option sets: O0 ... O3 = test_gpu_parity.MODES[:4], O4 = net sum + post_zero_cin."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import thermo as th
from tests import ecape_restatement as ER
from tests import effective_layer_restatement as FR
from tests import layer_cape_restatement as LR
from tests import layered_soundings as ls
from tests import test_gpu_ecape as TE
from tests import test_gpu_effective_layer as TF
from tests import test_gpu_layer_cape as TL
from tests.test_gpu_multi import _same
from tests.test_gpu_parity import MODES, _compare
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {'A': ls.GRID_A, 'B': ls.GRID_B, 'R': ls.GRID_REPLAY}
OPTS = ls.OPTION_SETS
ORACLE_MOIST = {'exact': 'rk4', 'family': 'family', 'table': 'table'}
DTYPES = [np.float64, np.float32]
PARCELS = list(ls.PARCELS)
LEAN_WANTS = [('cape', 'cin'), ('cape', 'cin', 'lfc_pressure', 'el_pressure', 'parcel_index')]
ORDER_KEYS = ('cape', 'cin', 'lfc_index', 'el_index', 'parcel_index')
FUSED_SETS = [[('most_unstable', 300.0), ('mixed_layer', 100.0)], [('surface', None), ('most_unstable', 250.0)]]


def test_option_sets_are_the_suites():
    assert OPTS == MODES[:5] and OPTS[4] == dict(pos_cape_neg_cin=False, post_zero_cin=True)


@pytest.fixture(scope='module', autouse=True)
def _oracle_family_table():
    """Both sides interpolate the oracle's adiabat-family table for the whole module; the library's own is put back after."""
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU'
    own = xa.family_table()
    ref = co.family_table()
    assert own.size == ref.size and float(np.max(np.abs(own - ref.reshape(own.shape)))) < 1e-8
    xa.set_family_table(ref)
    yield
    xa.set_family_table(own)


@pytest.fixture(scope='module')
def oracle_tables():
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    co.set_tables(tab)
    adiabat_tables.set_tables(tab.index, tab.adiabats)       # both sides look up the SAME arrays
    return tab


def grid(name, dtype=np.float64):
    return ls.grid(*GRIDS[name], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(name, parcel, opt, moist, profile=False):
    """The C oracle on a grid, computed once and shared (the float32 grid holds the same numbers)."""
    p, t, td = grid(name)
    return co.cape_cin_grid(p, t, td, parcel=parcel, moist=ORACLE_MOIST[moist], want_profile=profile, **OPTS[opt])


@functools.lru_cache(maxsize=None)
def full(name, parcel, moist, dtype, opt):
    """The all-outputs kernel's result, computed once and shared."""
    p, t, td = grid(name, dtype)
    return xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, **OPTS[opt])


def report(tag, got, ref):
    """The worst CAPE / CIN difference over the columns whose LFC / EL indices agree (a saturated-parcel tie does not)."""
    same = (np.asarray(got['lfc_index']) == ref['lfc_index']) & (np.asarray(got['el_index']) == ref['el_index'])
    with np.errstate(invalid='ignore'):
        worst = [np.nanmax(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])[same], initial=0.0) for k in ('cape', 'cin')]
    print('%s: worst |CAPE difference| %.3g, |CIN difference| %.3g J/kg over %d columns' % (tag, worst[0], worst[1], same.sum()))


def identical(a, b, keys, tag):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), (tag, k, np.nonzero(~((x == y) | ((x != x) & (y != y))))[0][:10])


# -- 1. the all-outputs kernels against the oracle --------------------------------------------------------------------------
CASES = ([('A', 'exact', o, d) for o in range(5) for d in DTYPES] + [('B', 'exact', o, d) for o in (0, 4) for d in DTYPES] +
         [('A', 'family', o, d) for o in (0, 2, 4) for d in DTYPES])


def _against_oracle(name, moist, opt, dtype, parcel):
    got = full(name, parcel, moist, dtype, opt)
    ref = reference(name, parcel, opt, moist)
    report('%s %s O%d %s %s' % (name, moist, opt, np.dtype(dtype).name, parcel), got, ref)
    _compare(got, ref, dtype, 1e-6)
    if opt == 4:                                                        # the option is seen to act
        net = full(name, parcel, moist, dtype, 2)
        acts = (np.asarray(got['cin']) == 0.0) & (np.asarray(net['cin']) > 0.0)
        print('post_zero_cin clamps %d of %d columns' % (acts.sum(), acts.size))
        assert acts.sum() >= 0.15 * acts.size, int(acts.sum())
        identical(got, net, ('cape', 'lfc_index', 'el_index', 'lfc_pressure', 'el_pressure'), 'O4 against O2')


@pytest.mark.parametrize('parcel', PARCELS)
@pytest.mark.parametrize('name,moist,opt,dtype', CASES)
def test_columns_vs_oracle(name, moist, opt, dtype, parcel):
    _against_oracle(name, moist, opt, dtype, parcel)


@pytest.mark.parametrize('parcel', PARCELS)
@pytest.mark.parametrize('opt', [0, 4])
def test_table_mode_columns_vs_oracle(opt, parcel, oracle_tables):
    _against_oracle('A', 'table', opt, np.float64, parcel)


@pytest.mark.parametrize('moist', ['exact', 'family'])
def test_explicit_parcel_vs_oracle(moist):
    p, t, td = grid('A')
    pv = np.stack([p[0] + 5.0, t[0] + 1.0, td[0] - 1.0])
    for opt in (0, 4):
        got = xa.cape_cin_columns(p, t, td, parcel='explicit', parcel_values=(pv[0], pv[1], pv[2]), moist=moist, **OPTS[opt])
        ref = co.cape_cin_grid(p, t, td, parcel='explicit', parcel_values=pv, moist=ORACLE_MOIST[moist], **OPTS[opt])
        report('A %s O%d explicit' % (moist, opt), got, ref)
        _compare(got, ref, np.float64, 1e-6)


# -- 2. the CAPE / CIN-only (LEAN) instantiations --------------------------------------------------------------------------------
@pytest.mark.parametrize('parcel', PARCELS)
@pytest.mark.parametrize('moist', ['exact', 'family'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('opt', [0, 4])
def test_cape_cin_only_kernels_equal_the_all_outputs_kernel(parcel, moist, dtype, opt):
    p, t, td = grid('A', dtype)
    want_all = full('A', parcel, moist, dtype, opt)
    for want in LEAN_WANTS:
        got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, want=want, **OPTS[opt])
        assert set(got) == set(want)
        identical(got, want_all, want, (parcel, moist, opt, want))


# -- 3. profile output and the lifted index -----------------------------------------------------------------------------------
@pytest.mark.parametrize('parcel', PARCELS)
@pytest.mark.parametrize('moist', ['exact', 'family'])
def test_profile_and_lifted_index(parcel, moist):
    p, t, td = grid('A')
    got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, want_profile=True)
    ref = reference('A', parcel, 0, moist, profile=True)
    for k in ref['profile']:
        a, b = got['profile'][k], ref['profile'][k]
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (parcel, k)
        ok = ~np.isnan(b)
        worst = np.max(np.abs(a[ok] - b[ok]))
        print('%s %s profile %s: worst difference %.3g over %d nodes' % (parcel, moist, k, worst, ok.sum()))
        assert worst <= 1e-8, (parcel, k, worst)
    identical(got, full('A', parcel, moist, np.float64, 0), ORDER_KEYS, 'profile call')
    li = xa.lifted_index(got['profile'])
    eager = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, lifted_index_at=500.0)           # all scalars wanted
    lazy = xa.cape_cin_columns(p, t, td, parcel=parcel, moist=moist, lifted_index_at=500.0, want=('cape', 'cin'))
    assert set(lazy) == {'cape', 'cin', 'lifted_index'} and 'profile' not in eager
    ok = ~np.isnan(li)
    assert ok.sum() >= 4500
    for tag, r in (('eager', eager), ('lazy', lazy)):
        assert np.array_equal(np.isnan(r['lifted_index']), np.isnan(li)), (parcel, tag)
        worst = np.max(np.abs(r['lifted_index'][ok] - li[ok]))
        print('%s %s lifted index (%s): worst difference %.3g' % (parcel, moist, tag, worst))
        assert worst <= 1e-9, (parcel, tag, worst)
        identical(r, got, ('cape', 'cin'), tag)


# -- 4. specific-humidity input ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('moist,parcel', [('exact', pc) for pc in PARCELS] + [('family', 'surface'), ('family', 'mixed_layer')])
def test_specific_humidity_input(moist, parcel, dtype):
    p, t, td = grid('A')
    with np.errstate(all='ignore'):
        e = th.saturation_vapor_pressure(td)
        w = th.EPSILON * e / (p - e)
        q = (w / (1.0 + w)).astype(dtype)
        td_ref = th.dewpoint_from_specific_humidity(p, t, q.astype(np.float64))       # the dewpoint of the ROUNDED q
    got = xa.cape_cin_columns(p.astype(dtype), t.astype(dtype), q, parcel=parcel, moist=moist, humidity='specific')
    ref = co.cape_cin_grid(p, t, td_ref, parcel=parcel, moist=ORACLE_MOIST[moist])
    report('A %s specific humidity %s %s' % (moist, np.dtype(dtype).name, parcel), got, ref)
    _compare(got, ref, dtype, 1e-6)


# -- 5. the fused two-parcel kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'B'])
@pytest.mark.parametrize('pset', [0, 1])
@pytest.mark.parametrize('opt', [0, 2, 4])
@pytest.mark.parametrize('dtype', DTYPES)
def test_fused_equals_separate_calls_and_the_oracle(name, pset, opt, dtype):
    p, t, td = grid(name, dtype)
    parcels = FUSED_SETS[pset]
    got = xa.cape_cin_multi(p, t, td, parcels, moist='family', fused=True, **OPTS[opt])
    for (parcel, depth), g in zip(parcels, got):
        if depth in (None, 300.0 if parcel == 'most_unstable' else 100.0):
            sep = full(name, parcel, 'family', dtype, opt)
        else:
            sep = xa.cape_cin_columns(p, t, td, parcel=parcel, depth=depth, moist='family', **OPTS[opt])
        _same(g, sep, (name, parcel, depth, opt))
        if pset == 0 and opt in (0, 4):
            _compare(g, reference(name, parcel, opt, 'family'), dtype, 1e-6)


# -- 6. persistent wavefronts ------------------------------------------------------------------------------------------------------
PERSISTENT = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from oracle import c_oracle as co
from tests import layered_soundings as ls
from tests import test_gpu_parity as tp
from xarray_parcel_amd import numpy_api as xa
xa.set_family_table(co.family_table())
for parcel in ls.PARCELS:
    for opt in (0, 4):
        ref = co.cape_cin_grid(*ls.grid(*ls.GRID_A), parcel=parcel, moist='family', **ls.OPTION_SETS[opt])
        for dtype in (np.float64, np.float32):
            p, t, td = ls.grid(*ls.GRID_A, dtype=dtype)
            got = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='family', **ls.OPTION_SETS[opt])
            tp._compare(got, ref, dtype, 1e-6)
            lean = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='family', want=('cape', 'cin'), **ls.OPTION_SETS[opt])
            for k in ('cape', 'cin'):
                assert np.array_equal(lean[k], got[k], equal_nan=True), (parcel, opt, k)
            if opt == 4:
                assert (np.asarray(got['cin']) == 0.0).sum() >= 0.15 * p.shape[1]
print('LAYERED_PERSISTENT_OK')
''' % ROOT


def test_persistent_wavefronts():
    """XP_PERSIST_MIN_COLS is read once per process: a fresh child, as tests/test_gpu_persistent.py starts one."""
    env = dict(os.environ, XP_PERSIST_MIN_COLS='0')
    out = subprocess.run([sys.executable, '-c', PERSISTENT], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and 'LAYERED_PERSISTENT_OK' in out.stdout, out.stderr[-3000:]


# -- 7. independence from the neighbouring lanes -----------------------------------------------------------------------------
@pytest.mark.parametrize('parcel', PARCELS)
@pytest.mark.parametrize('moist', ['exact', 'family'])
def test_results_do_not_depend_on_the_column_order(parcel, moist):
    """Whether a node is fed in phase A or in phase B depends on the other columns of the wavefront: a random permutation,
    and the columns sorted by the start level of the most-unstable parcel (wavefronts homogeneous in it, where the grid as
    it comes is as heterogeneous as it gets), give every column the same bits."""
    p, t, td = grid('A')
    want_all = full('A', parcel, moist, np.float64, 0)
    start = reference('A', 'most_unstable', 0, 'exact')['parcel_index']
    orders = {'permuted': np.random.default_rng(7).permutation(p.shape[1]), 'sorted by start level': np.argsort(start, kind='stable')}
    uniform = lambda s: np.mean([len(np.unique(s[i:i + 64])) == 1 for i in range(0, s.size - 63, 64)])     # share of wavefronts
    assert uniform(start[orders['sorted by start level']]) > 0.7 and uniform(start) < 0.05
    for tag, order in orders.items():
        q, u, ud = (np.ascontiguousarray(a[:, order]) for a in (p, t, td))
        got = xa.cape_cin_columns(q, u, ud, parcel=parcel, moist=moist)
        identical(got, {k: np.asarray(want_all[k])[order] for k in ORDER_KEYS}, ORDER_KEYS, (tag, 'all outputs'))
        lean = xa.cape_cin_columns(q, u, ud, parcel=parcel, moist=moist, want=LEAN_WANTS[1])
        identical(lean, {k: np.asarray(want_all[k])[order] for k in LEAN_WANTS[1]}, LEAN_WANTS[1], (tag, 'lean'))


# -- 8. the kernels that replay the ascent -------------------------------------------------------------------------------------
def replay_heights(dtype):
    return TL.heights(grid('R')[0]).astype(dtype)


@pytest.mark.parametrize('parcel', PARCELS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_cape_vs_restatement(parcel, dtype):
    """Surface -> 700 hPa, 700 -> 400 hPa, LFC + 60 -> EL - 5 per column, and the -10 / -30 degC levels of the environment
    (hail_growth_zone_cape's path)."""
    p, t, td = grid('R', dtype)
    ncol = p.shape[1]
    z = replay_heights(dtype)
    whole = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='exact')
    layers = [{'top': 700.0}, {'bottom': 700.0, 'top': 400.0},
              {'bottom': whole['lfc_pressure'] + dtype(60.0), 'top': whole['el_pressure'] - dtype(5.0)},
              {'bottom_temperature': 263.15, 'top_temperature': 243.15}]
    got = xa.cape_cin_layers(p, t, td, layers, height=z, parcel=parcel, moist='exact')
    assert got['cape'].dtype == dtype and got['cape'].shape == (4, ncol)
    # the temperature bounds, resolved on the host by the restatement's lowest-crossing rule
    z64, p64, t64 = (np.asarray(a, dtype=np.float64) for a in (z, p, t))
    with np.errstate(invalid='ignore'):
        s = np.sign(t64 - 263.15)
        crossings = (s[1:] * s[:-1] < 0).sum(axis=0)
    # (the recipe clips the perturbation at +-6 K and its most stable layer adds 5 K/km to a background of 5.5 ... 8.5 K/km: the
    # environment hardly ever warms with height, and NO column of this grid crosses 263.15 K twice -- 0 of 3000, measured on the
    # CPU.  The count is printed; half of nothing is no floor.  The bounds are still resolved through the crossing search.)
    print('%d of %d columns cross 263.15 K more than once' % ((crossings > 1).sum(), ncol))
    assert (crossings >= 1).sum() >= 0.9 * ncol
    for k, v in (('bottom_pressure', 263.15), ('top_pressure', 243.15)):
        host = LR.pressure_at_height(z64, p64, LR.crossing_height(z64, t64, v).astype(dtype).astype(np.float64))
        g = np.asarray(got[k][3], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(host)), (k, np.nonzero(np.isnan(g) != np.isnan(host))[0][:5])
        ok = ~np.isnan(host)
        tol = 1e-6 + (np.spacing(np.abs(host[ok]).astype(np.float32)).astype(np.float64) if dtype == np.float32 else 0.0)
        assert np.all(np.abs(g[ok] - host[ok]) <= tol), (k, float(np.max(np.abs(g[ok] - host[ok]))))
    bottoms = [None] + [np.asarray(got['bottom_pressure'][i], dtype=np.float64) for i in (1, 2, 3)]
    tops = [np.asarray(got['top_pressure'][i], dtype=np.float64) for i in range(4)]
    ref = LR.layers_grid(p, t, td, bottoms, tops, parcel=parcel, moist='rk4')
    TL.compare(got, ref, whole, dtype, 'layered %s %s' % (parcel, np.dtype(dtype).name))
    for k in TL.WHOLE:                                                  # the totals ARE xp_cape_cin's (a column without an LFC or an
        g, w = got[TL.TOTAL_OF.get(k, k)], whole[k]                     # EL has a NaN bound in layer 2: XP_ST_NO_LAYER on top of them)
        if k == 'status':
            assert np.array_equal(g & ~TL.L.XP_ST_NO_LAYER, w) and np.array_equal((g & TL.L.XP_ST_NO_LAYER) != 0, np.isnan(got['cape']).any(axis=0))
        else:
            assert np.array_equal(g, w, equal_nan=True), k
    live = np.isfinite(ref['cape'])
    assert all(live[i].sum() >= ncol // 4 for i in range(4)) and all((ref['cape'][i][live[i]] > 0).sum() >= 100 for i in range(4))
    assert (ref['cin'][0][live[0]] < 0).sum() >= 100


@pytest.mark.parametrize('dtype', DTYPES)
def test_effective_inflow_layer_vs_restatement(dtype):
    p, t, td = grid('R', dtype)
    z = replay_heights(dtype)
    got = xa.effective_inflow_layer(p, t, td, height=z, moist='exact', want_candidates=True)
    ref = FR.inflow_grid(p, t, td, z=z, moist='rk4')
    TF.compare_inflow(got, ref, dtype, 'layered %s' % np.dtype(dtype).name, ties=TF.saturated_ties(p, t, td, got))
    b = ref['base_index']
    print('layers %d, elevated bases %d' % ((b >= 0).sum(), (b > 0).sum()))
    assert (b >= 0).sum() >= 1500 and (b > 0).sum() >= 400


@pytest.mark.parametrize('opt', [0, 4])
@pytest.mark.parametrize('dtype', DTYPES)
def test_inflow_candidates_are_bit_identical_to_cape_cin(dtype, opt):
    p, t, td = grid('R', dtype)
    got = xa.effective_inflow_layer(p, t, td, moist='exact', want_candidates=True, **OPTS[opt])
    cc, ci = got['candidate_cape'], got['candidate_cin']
    n = 0
    for k in range(p.shape[0]):
        lifted = ~np.isnan(cc[k])
        if not lifted.any():
            continue
        ref = xa.cape_cin_columns(p[k:], t[k:], td[k:], parcel='surface', moist='exact', want=('cape', 'cin'), **OPTS[opt])
        assert np.array_equal(cc[k][lifted], ref['cape'][lifted]), (k, np.nonzero(cc[k][lifted] != ref['cape'][lifted])[0][:5])
        assert np.array_equal(ci[k][lifted], ref['cin'][lifted]), (k, np.nonzero(ci[k][lifted] != ref['cin'][lifted])[0][:5])
        n += int(lifted.sum())
    print('%d lifted candidates bit-identical to xp_cape_cin (%s, O%d)' % (n, np.dtype(dtype).name, opt))
    assert n >= 20000
    if opt == 4:
        assert (ci[~np.isnan(ci)] == 0.0).mean() >= 0.15 and not (ci > 0.0).any()


@pytest.mark.parametrize('parcel', ['most_unstable', 'surface'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_ncape_vs_restatement(parcel, dtype):
    """NCAPE between the LFC and the EL that cape_cin_columns returns for the same grid."""
    p, t, td = grid('R', dtype)
    z = replay_heights(dtype)
    cc = xa.cape_cin_columns(p, t, td, parcel=parcel, moist='exact', want=('lfc_pressure', 'el_pressure'))
    got = xa.ncape(p, t, td, z, cc['lfc_pressure'], cc['el_pressure'])
    ref = ER.grid(*(np.asarray(a, dtype=np.float64) for a in (p, t, td, z, cc['lfc_pressure'], cc['el_pressure'])))
    TE.compare(got, ref, dtype == np.float32, 'layered ncape %s %s' % (parcel, np.dtype(dtype).name))
    assert np.count_nonzero(np.isfinite(ref['ncape']) & (ref['ncape'] != 0.0)) >= 1000
