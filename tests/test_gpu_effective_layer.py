"""xp_effective_inflow_layer and xp_storm_relative_helicity_layers on the GPU: against the NumPy restatements
(tests/effective_layer_restatement.py), against the library's own xp_cape_cin / xp_storm_relative_helicity / xp_wind_shear
bit for bit where the header promises it, argument handling through the raw C ABI, the recipe up to the supercell
composite, and one grid at scale.

Tolerances.  candidate_cape / candidate_cin against the oracle: 1e-6 J/kg, what tests/test_gpu_parity.py holds xp_cape_cin
to against the same oracle, plus one f32 spacing for f32 outputs (tests/test_gpu_dcape.py::compare).  A column is left out
of the index comparison only when some lifted candidate lies within 1e-5 J/kg (ten times that tolerance) of a threshold in
the restatement, and such columns may be at most 1 % of the grid.  Helicity: 1e-9 x max(1, |positive| + |negative|), shear
components 1e-9 x max(1, |value|), plus one f32 spacing for f32 outputs (tests/test_gpu_kinematics.py::compare).

Saturated candidates.  tests/test_gpu_parity.py holds xp_cape_cin to the oracle everywhere but on the sign ties of SATURATED
parcels (its _saturated_tie_columns: the LCL sits on the parcel level and whether a crossing is seen there hangs on the last
bit of exp / log in whichever libm evaluates it; both outcomes are the reference's, and their number is bounded there).  A
candidate is xp_cape_cin's surface parcel bit for bit (test_candidates_are_bit_identical_to_cape_cin), so the same
candidates differ from the oracle here -- found on the first GPU run: 47 and 880 J/kg on one saturated level-0 candidate
each.  saturated_ties() classifies them with that very function, from xp_cape_cin's and the oracle's own outputs on the cut
column, under its bounds; such a candidate is left out of the value comparison, and its column out of the index
comparison only if the two values fall on different sides of a threshold."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import effective_layer_restatement as R
from tests import kinematics_restatement as K
from tests import test_gpu_kinematics as TK
from tests.test_effective_layer_cpu import sounding
from tests.test_gpu_dcape import inputs as dcape_inputs
from tests.test_gpu_parity import _saturated_tie_columns
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

pytestmark = pytest.mark.gpu
OUT = L.EFFECTIVE_F + L.EFFECTIVE_I


def heights(p):
    """A height for every level (standard atmosphere on the pressure, NaN where the pressure is), in p's dtype."""
    return (44330.8 * (1.0 - (np.asarray(p, dtype=np.float64) / 1013.25) ** 0.190263)).astype(p.dtype)


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def saturated_ties(p, t, td, got, moist='exact', **opts):
    """(nlev, ncol) mask of the lifted candidates that are saturated-parcel sign ties between xp_cape_cin and the oracle, by
    tests/test_gpu_parity.py's own classification (and under its bounds) of the two on the column cut off below the level."""
    p, t, td = (_np(a) for a in (p, t, td))
    lifted = ~np.isnan(_np(got['candidate_cape']))
    ties = np.zeros(lifted.shape, dtype=bool)
    for k in range(p.shape[0]):
        if not (lifted[k] & (t[k] == td[k])).any():
            continue
        cols = np.nonzero(lifted[k])[0]
        view = [np.ascontiguousarray(a[k:, cols]) for a in (p, t, td)]
        full = xa.cape_cin_columns(*view, parcel='surface', moist=moist, **opts)
        ref = co.cape_cin_grid(*view, parcel='surface', moist='rk4' if moist == 'exact' else moist, **opts)
        _, excluded = _saturated_tie_columns(full, ref)
        ties[k, cols[excluded]] = True
    return ties


def compare_inflow(got, ref, dtype, tag, cape_min=100.0, cin_min=-250.0, ties=None):
    f32 = dtype == np.float32
    near = R.near_threshold(ref, cape_min, cin_min, 1e-5)
    print('%s: %d of %d columns within 1e-5 J/kg of a threshold' % (tag, near.sum(), near.size))
    assert near.sum() <= 0.01 * near.size
    keep = ~near
    gc, gi = (_np(got[k]).astype(np.float64) for k in L.EFFECTIVE_CANDIDATES)
    if ties is None:
        ties = np.zeros(gc.shape, dtype=bool)
    with np.errstate(invalid='ignore'):
        flip = ties & (((gc >= cape_min) & (gi >= cin_min)) != ((ref['candidate_cape'] >= cape_min) & (ref['candidate_cin'] >= cin_min)))
    print('%s: %d saturated-parcel sign ties among the candidates, %d across a threshold' % (tag, ties.sum(), flip.sum()))
    keep &= ~flip.any(axis=0)
    for k in L.EFFECTIVE_CANDIDATES:
        g, r = _np(got[k]).astype(np.float64)[:, keep], ref[k][:, keep]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k, np.argwhere(np.isnan(g) != np.isnan(r))[:5])
        ok = ~np.isnan(r) & ~ties[:, keep]
        tol = np.full(ok.sum(), 1e-6)
        if f32:
            tol = tol + np.spacing(np.abs(r[ok]).astype(np.float32)).astype(np.float64)
        err = np.abs(g[ok] - r[ok])
        print('%s: %s worst difference %.3g J/kg over %d lifted candidates' % (tag, k, err.max() if err.size else 0.0, err.size))
        assert np.all(err <= tol), (tag, k, float(err.max()), np.argwhere(ok)[np.argmax(err - tol)])
    for k in L.EFFECTIVE_I:
        assert np.array_equal(_np(got[k])[keep], ref[k][keep]), (tag, k, np.nonzero(_np(got[k])[keep] != ref[k][keep])[0][:5])
    for k in L.EFFECTIVE_F:                                               # bit-equal to the levels they name
        g, r = _np(got[k])[keep], ref[k][keep].astype(dtype)
        assert g.dtype == dtype and np.array_equal(g, r, equal_nan=True), (tag, k)


def inflow_inputs(nlev, ncol, seed, dtype):
    p, t, td = dcape_inputs(nlev, ncol, seed, dtype)
    return p, t, td, heights(p)


# -- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('nlev', [40, 64])
def test_exact_mode_vs_restatement(nlev, dtype):
    p, t, td, z = inflow_inputs(nlev, 3000, seed=nlev + 1, dtype=dtype)
    got = xa.effective_inflow_layer(p, t, td, height=z, moist='exact', want_candidates=True)
    ref = R.inflow_grid(p, t, td, z=z, moist='rk4')
    compare_inflow(got, ref, dtype, 'exact nlev %d %s' % (nlev, np.dtype(dtype).name), ties=saturated_ties(p, t, td, got))
    st, b = ref['status'], ref['base_index']
    cc, ci = ref['candidate_cape'], ref['candidate_cin']
    with np.errstate(invalid='ignore'):
        cin_fail = ((cc >= 100.0) & (ci < -250.0)).any(axis=0)
    print('layers %d, elevated %d, CAPE-but-CIN failures %d, open %d, none %d' %
          ((b >= 0).sum(), (b > 0).sum(), cin_fail.sum(), ((st & R.ST_LAYER_OPEN) != 0).sum(), ((st & R.ST_NO_LAYER) != 0).sum()))
    assert (b >= 0).sum() >= 1500 and (b > 0).sum() >= 60 and cin_fail.sum() >= 20
    assert ((st & R.ST_LAYER_OPEN) != 0).sum() >= 5 and ((st & R.ST_NO_LAYER) != 0).sum() >= 300


@pytest.fixture(scope='module')
def oracle_tables():
    from oracle import tables as tb
    from xarray_parcel_amd import adiabat_tables
    tab = tb.get_tables()
    co.set_tables(tab)
    adiabat_tables.set_tables(tab.index, tab.adiabats)       # both sides look up the SAME arrays
    return tab


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_table_mode_vs_restatement(dtype, oracle_tables):
    p, t, td, z = inflow_inputs(40, 2000, seed=13, dtype=dtype)
    got = xa.effective_inflow_layer(p, t, td, height=z, moist='table', want_candidates=True)
    ref = R.inflow_grid(p, t, td, z=z, moist='table')
    compare_inflow(got, ref, dtype, 'table %s' % np.dtype(dtype).name, ties=saturated_ties(p, t, td, got, moist='table'))
    assert (ref['base_index'] >= 0).sum() >= 800


def test_family_mode_runs_as_exact():
    p, t, td, z = inflow_inputs(40, 512, seed=3, dtype=np.float64)
    a = xa.effective_inflow_layer(p, t, td, height=z, moist='exact', want_candidates=True)
    b = xa.effective_inflow_layer(p, t, td, height=z, moist='family', want_candidates=True)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_hand_built_columns():
    cols = [sounding(t_sfc=285.0, td_sfc=265.0), sounding(), sounding(t_sfc=305.0, td_sfc=297.0, cap=3.0, sfc_cool=4.0, sfc_levels=2)]
    nan_in = sounding()
    nan_in[1][3] = np.nan
    cols.append(nan_in)
    p, t, td, z = (np.stack([c[i] for c in cols], axis=1) for i in range(4))
    got = xa.effective_inflow_layer(p, t, td, height=z, want_candidates=True)
    assert list(got['base_index']) == [-1, 0, 2, 0] and list(got['top_index']) == [-1, 6, 6, 6]
    assert list(got['status']) == [L.XP_ST_NO_LAYER, 0, 0, 0]
    assert np.isnan(got['base_pressure'][0]) and got['base_height'][1] == 0.0 and got['base_height'][2] == z[2, 2] - z[0, 2]
    assert np.isnan(got['candidate_cape'][3, 3]) and np.isfinite(got['candidate_cape'][4, 3])
    compare_inflow(got, R.inflow_grid(p, t, td, z=z), np.float64, 'hand-built')
    got = xa.effective_inflow_layer(p, t, td, height=z, search_depth=60.0)
    assert list(got['status']) == [L.XP_ST_NO_LAYER, L.ST_LAYER_OPEN, L.ST_LAYER_OPEN, L.ST_LAYER_OPEN]
    assert list(got['top_index']) == [-1, 2, 2, 2]


# -- 2. against the library itself -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_candidates_are_bit_identical_to_cape_cin(dtype):
    """candidate_cape[k] / candidate_cin[k] ARE xp_cape_cin's surface parcel on p[k:], T[k:], Td[k:], bit for bit,
    wherever the kernel lifted k."""
    p, t, td, _ = inflow_inputs(40, 3000, seed=21, dtype=dtype)
    got = xa.effective_inflow_layer(p, t, td, moist='exact', want_candidates=True)
    cc, ci = got['candidate_cape'], got['candidate_cin']
    n = 0
    for k in range(p.shape[0]):
        lifted = ~np.isnan(cc[k])
        if not lifted.any():
            continue
        ref = xa.cape_cin_columns(p[k:], t[k:], td[k:], parcel='surface', moist='exact')
        assert np.array_equal(cc[k][lifted], ref['cape'][lifted]), (k, np.nonzero(cc[k][lifted] != ref['cape'][lifted])[0][:5])
        assert np.array_equal(ci[k][lifted], ref['cin'][lifted]), (k, np.nonzero(ci[k][lifted] != ref['cin'][lifted])[0][:5])
        n += int(lifted.sum())
    print('%d lifted candidates bit-identical to xp_cape_cin (%s)' % (n, np.dtype(dtype).name))
    assert n >= 20000


# -- 3. thresholds, options, input kinds, NULL outputs, argument errors ---------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(cape_min=500.0, cin_min=-50.0), dict(cape_min=0.5, cin_min=-1000.0, search_depth=150.0),
                                dict(search_depth=1.0), dict(search_depth=1e4), dict(virtual_temperature_correction=False),
                                dict(lcl_interp='linear'), dict(pos_cape_neg_cin=False), dict(post_zero_cin=True),
                                dict(pos_cape_neg_cin=False, post_zero_cin=True)])
def test_thresholds_and_options(kw):
    p, t, td, z = inflow_inputs(40, 1000, seed=17, dtype=np.float64)
    got = xa.effective_inflow_layer(p, t, td, height=z, want_candidates=True, **kw)
    ref = R.inflow_grid(p, t, td, z=z, **kw)
    opts = {k: v for k, v in kw.items() if k not in ('cape_min', 'cin_min', 'search_depth')}
    compare_inflow(got, ref, np.float64, str(kw), kw.get('cape_min', 100.0), kw.get('cin_min', -250.0),
                   ties=saturated_ties(p, t, td, got, **opts))
    if kw.get('search_depth') == 1.0:                                   # the window is the lowest valid level alone
        lay = ref['base_index'] >= 0
        assert lay.sum() >= 300 and np.array_equal(ref['base_index'][lay], ref['top_index'][lay])
        assert np.all(ref['status'][lay] & R.ST_LAYER_OPEN) and np.all((~np.isnan(ref['candidate_cape'])).sum(axis=0) <= 1)
    assert (ref['base_index'] >= 0).sum() >= 100


def test_input_kinds_agree_bit_for_bit():
    import torch
    p, t, td, z = inflow_inputs(40, 777, seed=23, dtype=np.float64)
    want = xa.effective_inflow_layer(p, t, td, height=z, want_candidates=True)
    dev = [torch.as_tensor(a).cuda() for a in (p, t, td, z)]
    got = xa.effective_inflow_layer(*dev[:3], height=dev[3], want_candidates=True)
    assert got['base_height'].is_cuda and got['base_index'].dtype == torch.int32
    for k in want:
        assert np.array_equal(_np(got[k]), want[k], equal_nan=True), k
    # strided device views through the C ABI: every other column of a (nlev, 2 ncol) buffer, read in place
    wide = [torch.full((40, 2 * 777), float('nan'), dtype=torch.float64, device='cuda') for _ in range(4)]
    for w, a in zip(wide, dev):
        w[:, ::2] = a
    res, out = _abi_out(40, 777, True)
    views = [L.View(w.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, 40, 777, 2 * 777, 2) for w in wide]
    lib = L.init(0)
    L.check(lib.xp_effective_inflow_layer(*views, 100.0, -250.0, 300.0, None, out, None))
    torch.cuda.synchronize()
    for k in want:
        assert np.array_equal(_np(res[k]).reshape(want[k].shape), want[k], equal_nan=True), k


def _abi_out(nlev, ncol, device, skip=()):
    """xp_effective_layer_out with every output (but `skip`) allocated, in device or host memory."""
    import torch
    res = {}
    for k in OUT + L.EFFECTIVE_CANDIDATES:
        if k in skip:
            continue
        shape = (nlev, ncol) if k in L.EFFECTIVE_CANDIDATES else (ncol,)
        if device:
            res[k] = torch.zeros(shape, dtype=torch.int32 if k in L.EFFECTIVE_I else torch.float64, device='cuda')
        else:
            res[k] = np.zeros(shape, dtype=np.int32 if k in L.EFFECTIVE_I else np.float64)
    out = L.EffectiveLayerOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE if device else L.XP_MEM_HOST)
    for k, a in res.items():
        setattr(out, k, a.data_ptr() if device else a.ctypes.data)
    return res, out


def _host_view(a, dtype=L.XP_F64):
    return L.View(a.ctypes.data, dtype, L.XP_MEM_HOST, a.shape[0], a.shape[1], a.shape[1], 1)


def test_height_absent_and_null_outputs():
    p, t, td, z = inflow_inputs(40, 300, seed=29, dtype=np.float64)
    want = xa.effective_inflow_layer(p, t, td, height=z, want_candidates=True)
    got = xa.effective_inflow_layer(p, t, td, want_candidates=True)
    for k in want:
        if k in ('base_height', 'top_height'):
            assert np.all(np.isnan(got[k]))
        else:
            assert np.array_equal(got[k], want[k], equal_nan=True), k
    lib = L.init(0)
    views = [_host_view(a) for a in (p, t, td, z)]
    for skip in OUT + L.EFFECTIVE_CANDIDATES:                           # every output pointer NULL in turn
        res, out = _abi_out(40, 300, False, skip=(skip,))
        L.check(lib.xp_effective_inflow_layer(*views, 100.0, -250.0, 300.0, None, out, None))
        for k in res:
            assert np.array_equal(res[k], want[k], equal_nan=True), (skip, k)
    res, out = _abi_out(40, 300, False, skip=OUT + L.EFFECTIVE_CANDIDATES)   # all of them
    L.check(lib.xp_effective_inflow_layer(*views, 100.0, -250.0, 300.0, None, out, None))


def test_argument_errors():
    p, t, td, z = inflow_inputs(12, 40, seed=5, dtype=np.float64)
    lib = L.init(0)
    vp, vt, vtd, vz = (_host_view(a) for a in (p, t, td, z))
    res, out = _abi_out(12, 40, False)

    def call(views=(vp, vt, vtd, vz), cape=100.0, cin=-250.0, depth=300.0, o=None, out_=out):
        return lib.xp_effective_inflow_layer(*views, cape, cin, depth, o, out_, None)

    def opts(**kw):
        o = L.Opts(1, L.LCL_INTERP['log'], 1, 0, L.MOIST['exact'], L.XP_F64, L.HUMIDITY['dewpoint'], 0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    assert call() == 0 and call(o=opts()) == 0
    narrow = np.ascontiguousarray(z[:, :-1])
    f32 = z.astype(np.float32)
    for bad in (dict(cape=float('nan')), dict(cin=float('inf')), dict(cin=float('nan')), dict(depth=0.0), dict(depth=-5.0),
                dict(depth=float('nan')), dict(depth=float('inf')), dict(o=opts(humidity=L.HUMIDITY['specific'])),
                dict(o=opts(moist_mode=9)), dict(views=(vp, vt, vtd, _host_view(narrow))),
                dict(views=(vp, _host_view(narrow), vtd, vz)), dict(views=(vp, vt, vtd, _host_view(f32, L.XP_F32))),
                dict(views=(None, vt, vtd, vz)), dict(out_=None),
                dict(out_=L.EffectiveLayerOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST))):
        assert call(**bad) == L.XP_E_ARG, (bad, lib.xp_last_error())
    assert call(o=opts(lcl_interp=5)) == L.XP_E_INTERP
    # the layers kernel
    _, u, v, zz = TK.inputs(12, 40, seed=2)
    b, tp = np.zeros(40), np.full(40, 1000.0)
    lo = L.SrhLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST)
    tot = np.zeros(40)
    lo.total[0] = tot.ctypes.data
    vs = [_host_view(a) for a in (zz, u, v)]

    def layers(views=vs, su=None, sv=None, bottom=b.ctypes.data, n=1, tops=(tp.ctypes.data,), out_=lo):
        arr = (C.c_void_p * max(len(tops), 1))(*tops) if tops is not None else None
        return lib.xp_storm_relative_helicity_layers(*views, su, sv, None, None, bottom, n, arr, out_, None)
    assert layers() == 0
    for bad in (dict(n=0), dict(n=5), dict(bottom=None), dict(tops=None), dict(tops=(None,)), dict(su=b.ctypes.data),
                dict(out_=None), dict(views=[vs[0], vs[1], _host_view(np.ascontiguousarray(v[:, :-1]))]),
                dict(out_=L.SrhLayersOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST))):
        assert layers(**bad) == L.XP_E_ARG, (bad, lib.xp_last_error())


# -- 4. the layers kernel ---------------------------------------------------------------------------------------------------
def _layer_scale(ref):
    s = np.maximum(1.0, np.abs(ref['positive']) + np.abs(ref['negative']))
    return lambda k: s if k in K.SRH_KEYS else np.maximum(1.0, np.abs(ref[k]))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_layers_vs_restatement(dtype):
    n = 3000
    p, u, v, z = TK.inputs(40, n, seed=6, dtype=dtype)
    rng = np.random.default_rng(7)
    cu, cv = rng.normal(8, 4, n).astype(dtype), rng.normal(2, 4, n).astype(dtype)
    b = rng.uniform(0.0, 1500.0, n)
    b[rng.random(n) < 0.3] = 0.0
    tops = [b + rng.uniform(50.0, 4000.0, n) for _ in range(4)]
    # bounds on levels, NaN / inverted / negative / unspanned ones
    h = z.astype(np.float64) - np.array([col[~np.isnan(col)][0] if (~np.isnan(col)).any() else np.nan for col in z.T.astype(np.float64)])
    on = rng.permutation(n)[:600]
    for c in on[:300]:
        lev = h[:, c][~np.isnan(h[:, c])]
        if lev.size > 6:
            b[c], tops[0][c] = lev[1], lev[5]
    tops[1][on[300:350]] = np.nan
    b[on[350:400]] = np.nan
    tops[2][on[400:450]] = b[on[400:450]] - 10.0
    tops[3][on[450:500]] = b[on[450:500]]
    b[on[500:550]] = -5.0
    tops[0][on[550:600]] = 5.0e4
    b = b.astype(dtype)
    tops = [x.astype(dtype) for x in tops]
    for kw in ({}, {'surface_u': rng.normal(2, 2, n).astype(dtype), 'surface_v': rng.normal(0, 2, n).astype(dtype)}):
        if kw:
            z = (z - np.nanmin(z, axis=0) + 10.0).astype(dtype)
        got = xa.storm_relative_helicity_layers(z, u, v, b, tops, storm_u=cu, storm_v=cv, **kw)
        assert _np(got['shear_u']).dtype == dtype and _np(got['total']).shape == (4, n)
        f = lambda a: np.asarray(a, dtype=np.float64)
        ref = R.layers_grid(f(z), f(u), f(v), f(b), [f(x) for x in tops], f(cu), f(cv), **{k: f(x) for k, x in kw.items()})
        TK.compare(got, ref, R.LAYER_KEYS, _layer_scale(ref), dtype == np.float32, 'layers %s' % np.dtype(dtype).name)
        mag = np.hypot(_np(got['shear_u']), _np(got['shear_v']))
        assert np.array_equal(_np(got['shear_magnitude']), mag, equal_nan=True)
        ok = np.isfinite(ref['total'])
        # (300 columns were given a NaN, inverted, empty, negative or unreachable bound above)
        assert ok.sum() >= 4000 and (ref['status'] & R.ST_NO_LAYER).astype(bool).sum() >= 300
        assert np.isfinite(ref['shear_u']).sum() >= 4000


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_constant_bounds_are_bit_identical_to_the_scalar_kernel(dtype):
    n = 2000
    p, u, v, z = TK.inputs(40, n, seed=8, dtype=dtype)
    rng = np.random.default_rng(9)
    cu, cv = rng.normal(8, 4, n).astype(dtype), rng.normal(2, 4, n).astype(dtype)
    for b, depths in ((0.0, [500.0]), (500.0, [500.0, 2500.0, 5500.0, 1000.0]), (0.0, [1000.0, 3000.0, 6000.0, 500.0])):
        want = xa.storm_relative_helicity(z, u, v, depths, bottom=b, storm_u=cu, storm_v=cv)
        got = xa.storm_relative_helicity_layers(z, u, v, np.full(n, b, dtype), [np.full(n, b + d, dtype) for d in depths],
                                                storm_u=cu, storm_v=cv)
        for k in K.SRH_KEYS:
            assert np.array_equal(_np(got[k]), _np(want[k]), equal_nan=True), (b, k)
        assert np.array_equal(got['status'], want['status'])
        assert np.isfinite(_np(want['total'])).sum() >= 1000
    one = xa.storm_relative_helicity_layers(z, u, v, 0.0, np.full(n, 500.0, dtype), storm_u=cu, storm_v=cv)
    want = xa.storm_relative_helicity(z, u, v, 500.0, storm_u=cu, storm_v=cv)
    assert one['total'].shape == (n,) and np.array_equal(one['total'], want['total'], equal_nan=True)


def test_layer_shear_agrees_with_wind_shear():
    n = 1500
    rng = np.random.default_rng(11)
    z = 10.0 + np.vstack([np.zeros(n), np.cumsum(rng.uniform(80.0, 600.0, (29, n)), axis=0)])     # heights above the surface
    u = 5.0 + z * 2.5e-3 + rng.normal(0, 3, z.shape)
    v = -2.0 + z * 1.0e-3 + rng.normal(0, 3, z.shape)
    su, sv = rng.normal(2, 2, n), rng.normal(0, 2, n)
    for hgt in (500.0, 3000.0, 6000.0):
        got = xa.storm_relative_helicity_layers(z, u, v, 0.0, np.full(n, hgt), surface_u=su, surface_v=sv)
        want = xa.wind_shear(su, sv, u, v, z, shear_height=hgt)
        assert np.all(got['status'] == 0)
        for k in ('shear_u', 'shear_v', 'shear_magnitude'):
            err = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
            print('layer 0 ... %g m: %s worst relative difference from wind_shear %.3g' % (hgt, k, err.max()))
            assert np.all(err <= 1e-9), (hgt, k, float(err.max()))


def test_layers_ordering_violations():
    p, u, v, z = TK.inputs(30, 256, seed=9)
    z[4, :64] = z[3, :64]                               # equal heights
    for a in (u, v, z):
        a[:, 200:] = a[:, 200:][::-1]                   # upside down
    b, tops = np.zeros(256), [np.full(256, 1000.0), np.full(256, 3000.0)]
    got = xa.storm_relative_helicity_layers(z, u, v, b, tops)
    ref = R.layers_grid(z, u, v, b, tops)
    TK.compare(got, ref, R.LAYER_KEYS, _layer_scale(ref), False, 'layers ordering')
    assert np.count_nonzero(ref['status'] & R.ST_BAD_HEIGHT) >= 90
    bad = (ref['status'] & R.ST_BAD_HEIGHT) != 0
    assert np.all(np.isnan(_np(got['shear_u'])[:, bad])) and np.all(np.isnan(_np(got['total'])[:, bad]))


# -- 5. the chain -------------------------------------------------------------------------------------------------------------
def test_recipe_up_to_the_supercell_composite():
    """most_unstable_cape_cin -> el_pressure -> interp_level(height) -> effective_inflow_layer ->
    storm_relative_helicity_layers(top = [top_height, base_height + 0.5 (z_EL - base_height)]) -> supercell_composite, on the
    device, against the restatements composed on the host."""
    n, nlev = 2000, 40
    p, t, td = synth.columns(nlev=nlev, ncol=n, seed=41, dtype=np.float64)
    z = heights(p)
    rng = np.random.default_rng(42)
    h = z - z[0]
    u = 5.0 + h * 2.5e-3 + rng.normal(0, 3, (nlev, n))
    v = -2.0 + h * 1.0e-3 + rng.normal(0, 3, (nlev, n))
    mu = xa.cape_cin_columns(p, t, td, parcel='most_unstable', moist='exact')
    z_el = xa.interp_level(p, z, mu['el_pressure'], log=True) - z[0]
    eff = xa.effective_inflow_layer(p, t, td, height=z)
    bm = xa.bunkers_storm_motion(p, u, v, z)
    half = eff['base_height'] + 0.5 * (z_el - eff['base_height'])
    lay = xa.storm_relative_helicity_layers(z, u, v, eff['base_height'], [eff['top_height'], half],
                                            storm_u=bm['right_u'], storm_v=bm['right_v'])
    scp = xa.supercell_composite(mu['cape'], lay['total'][0], lay['shear_magnitude'][1])
    # the host side, from the oracle and the restatements
    r_mu = co.cape_cin_grid(p, t, td, parcel='most_unstable', moist='rk4')
    r_eff = R.inflow_grid(p, t, td, z=z)
    keep = ~R.near_threshold(r_eff)
    assert np.array_equal(eff['base_index'][keep], r_eff['base_index'][keep])
    r_bm = K.bunkers_grid(p, u, v, z)
    x, xe = np.log(p), np.log(r_mu['el_pressure'])
    r_zel = np.full(n, np.nan)
    for c in range(n):                                                  # log-p interpolation of the height at the EL
        if not np.isnan(xe[c]):
            r_zel[c] = np.interp(-xe[c], -x[:, c], z[:, c]) - z[0, c]
    assert np.allclose(z_el, r_zel, rtol=0, atol=1e-6, equal_nan=True)
    r_half = r_eff['base_height'] + 0.5 * (r_zel - r_eff['base_height'])
    r_lay = R.layers_grid(z, u, v, r_eff['base_height'], [r_eff['top_height'], r_half], r_bm['right_u'], r_bm['right_v'])
    r_scp = K.supercell_composite(r_mu['cape'], r_lay['total'][0], np.hypot(r_lay['shear_u'][1], r_lay['shear_v'][1]))
    assert np.array_equal(np.isnan(scp[keep]), np.isnan(r_scp[keep]))
    ok = keep & ~np.isnan(r_scp)
    # SCP = (cape / 1000) (srh / 50) (shear / 20): the CAPE within 1e-6 J/kg, i.e. 1e-9 of cape / 1000; the helicity within
    # 1e-9 (|positive| + |negative|); the shear within 1e-9; and the z_EL -> half-depth chain in front of the shear another
    # 1e-9: four factors' worth of 1e-9 on the product formed with |positive| + |negative| in place of the helicity
    s = np.maximum(1.0, (r_mu['cape'] / 1000.0) * ((np.abs(r_lay['positive'][0]) + np.abs(r_lay['negative'][0])) / 50.0))[ok]
    err = np.abs(scp[ok] - r_scp[ok]) / s
    print('SCP on %d columns (%d non-zero): worst difference %.3g of the scale' % (ok.sum(), (r_scp[ok] != 0).sum(), err.max()))
    assert ok.sum() >= 1000 and (r_scp[ok] != 0).sum() >= 300 and np.all(err <= 4e-9)


# -- 6. at scale ----------------------------------------------------------------------------------------------------------------
def test_full_size_grid_sample():
    import torch
    nlev, ncol = 64, 1 << 20
    p, t, td = synth.columns_torch(nlev, ncol, 'cuda', seed=5)
    z = 44330.8 * (1.0 - (p / 1013.25) ** 0.190263)
    eff = xa.effective_inflow_layer(p, t, td, height=z, want_candidates=True)
    torch.cuda.synchronize()
    idx = np.linspace(0, ncol - 1, 4096).astype(np.int64)
    idx[-64:] = np.arange(ncol - 64, ncol)                              # the last wavefront too
    ti = torch.as_tensor(idx, device='cuda')
    hp, ht, htd, hz = (a[:, ti].cpu().numpy() for a in (p, t, td, z))
    ref = R.inflow_grid(hp, ht, htd, z=hz)
    got = {k: _np(a[..., ti]) for k, a in eff.items()}
    compare_inflow(got, ref, np.float64, 'full size', ties=saturated_ties(hp, ht, htd, got))
    assert (ref['base_index'] >= 0).sum() >= 2000
    del eff
    h = z - z[0]
    u = 5.0 + h * 2.5e-3 + torch.sin(h * 7e-3 + p[0])
    v = -2.0 + h * 1.0e-3 + torch.cos(h * 5e-3 + t[0])
    b = torch.as_tensor(np.random.default_rng(3).uniform(0.0, 800.0, ncol), device='cuda')
    tops = [b + d for d in (300.0, 1200.0, 2500.0, 5000.0)]
    lay = xa.storm_relative_helicity_layers(z, u, v, b, tops, storm_u=7.0, storm_v=3.0)
    torch.cuda.synchronize()
    ref = R.layers_grid(hz, _np(u[:, ti]), _np(v[:, ti]), _np(b[ti]), [_np(x[ti]) for x in tops], 7.0, 3.0)
    got = {k: _np(a[..., ti]) for k, a in lay.items()}
    TK.compare(got, ref, R.LAYER_KEYS, _layer_scale(ref), False, 'layers full size')
    assert np.isfinite(ref['total']).sum() >= 4 * 4000
