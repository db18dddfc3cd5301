"""xp_thermo_layers on the GPU: against the NumPy restatement (tests/thermo_layers_restatement.py), bit for bit across the forms
of one request, across input kinds and through the convenience functions, and the argument checks of the raw C ABI.

Tolerances.  tests/test_gpu_kinematics.py::compare's rule, 1e-9 x scale plus one f32 spacing of the reference for f32
outputs; scale = max(1, the largest magnitude of the quantity's per-level values in the column): theta_e for the theta_e
outputs, p for their pressures, 1 for precipitable water [mm] and the two means (w and rh stay below 1), max(1, |ref|) for
thickness and lapse rate.  The device's fexp / flog are within a few ulp of libm and every sum has one sign; 1e-9 is the
project's existing allowance.  The theta_e pressures are compared only where the restatement's extreme stands out by more
than 1e-9 (relative) from the runner-up: below that the choice between two points hangs on the last bits of the pow chain,
and both are the layer's extreme; at most 1 % of the layers may be left out (tests/test_thermo_layers_cpu.py checks the
seed)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import thermo_layers_restatement as R
from tests.test_gpu_kinematics import _f64, compare
from tests.test_gpu_wind_layers import OFFSETS
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa

pytestmark = pytest.mark.gpu
NAN = float('nan')
SEED = 5
NLEV, NCOL = 48, 6000
TK = R.THERMO_KEYS
VALUE_KEYS = tuple(k for k in TK if not k.endswith('_pressure'))
NO_T = ('precipitable_water', 'mean_mixing_ratio', 'thickness')             # the outputs that do not read temperature
NO_TD = ('thickness', 'lapse_rate')                                          # ... that do not read dewpoint
# 0-3 km by height; 700-500 hPa; the whole column (open top); the per-column layer of inputs()
LAYERS = [(R.HEIGHT, 0.0, 3000.0), (R.PRESSURE, 700.0, 500.0), (R.PRESSURE, NAN, NAN), (R.PRESSURE, NAN, NAN)]
CLASSES = ('between', 'one_interval', 'on_levels', 'nan_top', 'below_p0', 'inverted', 'nan_bottom')


def api_layers(pb, pt):
    return [{'bottom_height': 0.0, 'top_height': 3000.0}, {'bottom': 700.0, 'top': 500.0}, {'bottom': None, 'top': None},
            {'bottom': pb, 'top': pt}]


def inputs(nlev, ncol, seed, dtype=np.float64, p0=None):
    """Pressure, temperature, dewpoint, height (nlev, ncol), the per-column bounds (pb, pt) of the fourth layer and the class
    of each.  Pressure and height as tests/test_gpu_wind_layers.py::inputs builds them: pressure hydrostatic-like on the
    heights, p0 in 985 ... 1030 hPa (or `p0` everywhere); a sixteenth of the columns with p0 in 800 ... 845 hPa; in half of
    the columns one level moved onto a bound of LAYERS or next to it by OFFSETS (the height for z0 + 3000 m, the pressure for
    700 and 500 hPa); ~5 % missing values; an eighth of the columns truncated at 2 ... 7 km.  T follows a lapse rate of
    5 ... 8 K/km plus noise, Td = T minus a non-negative depression; an eighth of the columns are saturated (Td == T) over a
    run of levels.  The fourth layer's bounds are drawn from the column's own valid levels (in `dtype`), a seventh of the
    columns per class of CLASSES; the non-degenerate ones are at least 5 hPa deep."""
    rng = np.random.default_rng(seed)
    z0 = rng.integers(0, 1500, ncol).astype(np.float64)        # (z0 + 3000 is exact)
    z = z0 + np.vstack([np.zeros(ncol), np.cumsum(rng.uniform(80.0, 600.0, (nlev - 1, ncol)), axis=0)])
    cols = rng.permutation(ncol)
    targets = [('z', 3000.0), ('p', 700.0), ('p', 500.0)]
    combos = [(t, o) for t in targets for o in OFFSETS]
    groups = np.array_split(cols[:ncol // 2], len(combos))
    for g, ((kind, t), off) in zip(groups, combos):
        if kind != 'z':
            continue
        for c in g:
            want = z0[c] + t + off * 8200.0
            k = int(np.argmin(np.abs(z[:, c] - want)))
            if k and k + 1 < nlev and z[k - 1, c] < want < z[k + 1, c]:
                z[k, c] = want
    h = z - z0
    psfc = rng.uniform(985.0, 1030.0, ncol) if p0 is None else np.full(ncol, float(p0))
    high = cols[ncol // 2 + ncol // 8: ncol // 2 + ncol // 8 + ncol // 16]
    if p0 is None:
        psfc[high] = rng.uniform(800.0, 845.0, high.size)
    p = psfc * np.exp(-h / rng.uniform(7600.0, 8800.0, ncol))
    for g, ((kind, t), off) in zip(groups, combos):
        if kind != 'p':
            continue
        for c in g:
            want = t * (1.0 + off)
            k = int(np.argmin(np.abs(p[:, c] - want)))
            if k and k + 1 < nlev and p[k - 1, c] > want > p[k + 1, c]:
                p[k, c] = want
    t = rng.uniform(285.0, 305.0, ncol) - h * rng.uniform(5e-3, 8e-3, ncol) + rng.normal(0, 0.5, (nlev, ncol))
    dep = np.abs(rng.normal(0, 6.0, (nlev, ncol)))
    sat = cols[ncol // 4: ncol // 4 + ncol // 8]
    k0 = rng.integers(0, nlev - 8, sat.size)
    for c, k in zip(sat, k0):
        dep[k:k + rng.integers(2, 8), c] = 0.0
    td = t - dep
    arrs = [p, t, td, z]
    miss = rng.random((nlev, ncol)) < 0.05
    which = rng.integers(0, 4, (nlev, ncol))
    for i, a in enumerate(arrs):
        a[miss & (which == i)] = np.nan
    for c in cols[ncol // 2: ncol // 2 + ncol // 8]:
        cut = z0[c] + rng.uniform(2000.0, 7000.0)
        for a in arrs:
            a[z[:, c] > cut, c] = np.nan
    arrs = [a.astype(dtype) for a in arrs]
    # the per-column layer, from the levels as the call will see them
    pd = arrs[0].astype(np.float64)
    ok = ~np.any([np.isnan(a) for a in arrs], axis=0)
    pb, pt = np.full(ncol, NAN), np.full(ncol, NAN)
    cls = rng.integers(0, len(CLASSES), ncol)
    for c in range(ncol):
        lv = pd[ok[:, c], c]
        if lv.size < 8:
            cls[c] = CLASSES.index('nan_top')
            continue
        name = CLASSES[cls[c]]
        i = int(rng.integers(0, min(20, lv.size - 6)))           # (below ~7 km: two intervals are more than 5 hPa)
        j = i + int(rng.integers(2, 6))
        if name == 'between':
            pb[c], pt[c] = 0.5 * (lv[i] + lv[i + 1]), 0.5 * (lv[j] + lv[j + 1])
        elif name == 'one_interval':
            i = int(np.argmax(lv[:-1] - lv[1:]))                 # the column's deepest interval: more than 10 hPa
            pb[c], pt[c] = lv[i] - 0.2 * (lv[i] - lv[i + 1]), lv[i] - 0.8 * (lv[i] - lv[i + 1])
        elif name == 'on_levels':
            pb[c], pt[c] = lv[i], lv[j]
        elif name == 'nan_top':
            pb[c] = lv[i]
        elif name == 'below_p0':
            pb[c], pt[c] = lv[0] + 5.0, lv[j]
        elif name == 'inverted':
            pb[c], pt[c] = lv[j], lv[i]
        else:                                                    # 'nan_bottom': from the lowest valid level
            pt[c] = 0.5 * (lv[j] + lv[j + 1])
    deep = ~np.isnan(pb) & ~np.isnan(pt) & (pt < pb)
    assert np.all((pb - pt)[deep] >= 5.0)
    return arrs, pb.astype(dtype), pt.astype(dtype), cls


@functools.lru_cache(maxsize=None)
def case(dtype):
    """The inputs of the comparison at 48 x 6000 and the restatement on them, computed once per dtype and left unchanged."""
    arrs, pb, pt, cls = inputs(NLEV, NCOL, SEED, dtype)
    ref = restate(arrs, pb, pt)
    for a in list(arrs) + [pb, pt, cls] + list(ref.values()):
        a.setflags(write=False)
    return arrs, pb, pt, cls, ref


def restate(arrs, pb, pt, cols=None, layers=LAYERS):
    return R.thermo_layers_grid(*(a.astype(np.float64) for a in arrs), layers, [None, None, None, pb.astype(np.float64)][:len(layers)],
                                [None, None, None, pt.astype(np.float64)][:len(layers)], cols=cols)


def scales(arrs, ref):
    """scale(k) of compare(): (nlayer, ncol)."""
    p, t, td, z = (a.astype(np.float64) for a in arrs)
    ok = ~(np.isnan(p) | np.isnan(t) | np.isnan(td) | np.isnan(z))
    with np.errstate(invalid='ignore', divide='ignore'):
        th = np.where(ok, R.O.equivalent_potential_temperature(p, t, td), 0.0)
    big_th = np.maximum(1.0, np.nanmax(np.abs(th), axis=0))
    big_p = np.maximum(1.0, np.max(np.where(ok, p, 0.0), axis=0))
    ones = np.ones_like(ref['thickness'])

    def scale(k):
        if k in ('theta_e_min', 'theta_e_max'):
            return big_th[None, :] * ones
        if k.endswith('_pressure'):
            return big_p[None, :] * ones
        if k in ('thickness', 'lapse_rate'):
            return np.maximum(1.0, np.abs(ref[k]))
        return ones
    return scale


def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def same_bits(a, b, keys, tag, sel=slice(None)):
    for k in keys:
        assert np.array_equal(_np(a[k])[..., sel], _np(b[k])[..., sel], equal_nan=True), (tag, k)


def compare_pressures(got, ref, scale, f32, tag):
    """theta_e_min_pressure / theta_e_max_pressure where the extreme stands out; returns the fraction of layers left out."""
    worst_left = 0.0
    for k, gap in (('theta_e_min_pressure', 'gap_min'), ('theta_e_max_pressure', 'gap_max')):
        has = ~np.isnan(ref[k])
        clear = has & (ref[gap] > 1e-9)
        left_out = 1.0 - clear.sum() / has.sum()
        print('%s: %s compared on %d of %d layers (%.3f %% left out)' % (tag, k, clear.sum(), has.sum(), 100 * left_out))
        worst_left = max(worst_left, left_out)
        g = _f64(got[k])
        assert np.array_equal(np.isnan(g), ~has), (tag, k)
        tol = 1e-9 * scale(k)[clear]
        if f32:
            tol = tol + np.spacing(np.abs(ref[k][clear]).astype(np.float32)).astype(np.float64)
        err = np.abs(g[clear] - ref[k][clear])
        assert np.all(err <= tol), (tag, k, float(err.max()), np.argwhere(clear)[np.argmax(err - tol)])
    return worst_left


# -- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_thermo_layers_vs_restatement(dtype):
    arrs, pb, pt, cls, ref = case(dtype)
    got = xa.thermo_layers(*arrs, layers=api_layers(pb, pt))
    assert set(got) == set(TK) | {'status'}
    assert got['thickness'].dtype == dtype and got['thickness'].shape == (4, NCOL) and got['status'].shape == (NCOL,)
    f32 = dtype == np.float32
    tag = 'thermo_layers %s' % np.dtype(dtype).name
    scale = scales(arrs, ref)
    compare(got, ref, VALUE_KEYS, scale, f32, tag)
    assert compare_pressures(got, ref, scale, f32, tag) <= 0.01
    # the inputs exercise what they are meant to
    st = ref['status']
    nan_l = np.isnan(ref['thickness'])
    assert (st == 0).sum() >= 1500 and (st == R.ST_NO_LAYER).sum() >= 2000 and not np.any(st & (R.ST_BAD_HEIGHT | R.ST_BAD_PRESSURE))
    for i, least in enumerate((100, 300, 0, 2000)):      # (the whole column is a layer wherever there are two valid levels)
        assert nan_l[i].sum() >= least and (~nan_l[i]).sum() >= 2500, i
    assert (nan_l[1] & ~nan_l[0]).sum() >= 100 and (nan_l[0] & ~nan_l[2]).sum() >= 100
    for target in (700.0, 500.0):                        # levels on the bound, inside np.isclose of it, just outside
        r = np.abs(arrs[0].astype(np.float64) / target - 1.0)
        assert (r == 0.0).sum() >= 100 and ((r > 0.0) & (r <= 1e-5)).sum() >= 200 and ((r > 1e-5) & (r < 1e-4)).sum() >= 200, target
    for name in ('between', 'one_interval', 'on_levels', 'nan_bottom'):
        sel = cls == CLASSES.index(name)
        assert (~nan_l[3][sel]).sum() >= 500, name
    for name in ('nan_top', 'below_p0', 'inverted'):
        sel = cls == CLASSES.index(name)
        assert sel.sum() >= 500 and nan_l[3][sel].all() and np.all(st[sel] & R.ST_NO_LAYER), name
    assert np.nanmax(ref['mean_relative_humidity']) <= 1.0 + 1e-12 and (arrs[2] == arrs[1]).sum() >= 2000   # saturated levels
    assert np.nanmin(ref['precipitable_water'][2]) > 0.5 and np.nanmax(ref['precipitable_water'][2]) < 120.0
    on = cls == CLASSES.index('on_levels')
    assert (ref['theta_e_max_pressure'][3][on] == pb[on].astype(np.float64)).sum() >= 50       # an extreme on a bound that is a level
    between = (cls == CLASSES.index('between')) & ~nan_l[3]
    ends = (ref['theta_e_max_pressure'][3] == pb.astype(np.float64)) | (ref['theta_e_min_pressure'][3] == pb.astype(np.float64))
    assert (ends & between).sum() >= 50                                                        # ... and on an added bound point


# -- 2. one request, several forms: bit for bit ---------------------------------------------------------------------------
def test_four_layers_equal_each_alone_and_any_subset_of_outputs():
    arrs, pb, pt, cls, _ = case(np.float64)
    lay = api_layers(pb, pt)
    many = xa.thermo_layers(*arrs, layers=lay)
    for i, one_layer in enumerate(lay):
        one = xa.thermo_layers(*arrs, layers=[one_layer])
        for k in TK:
            assert np.array_equal(many[k][i], one[k][0], equal_nan=True), (i, k)
        assert np.array_equal(one['status'] != 0, np.isnan(one['thickness'][0]))
        assert np.all((many['status'] & R.ST_NO_LAYER) >= (one['status'] & R.ST_NO_LAYER))
    # subsets of the outputs cross the instantiations: no theta_e; no moisture sums; neither; one of each
    for want in (TK[:5], TK[3:], TK[3:5], ('precipitable_water',), ('mean_relative_humidity', 'theta_e_max_pressure'), ('theta_e_min',)):
        part = xa.thermo_layers(*arrs, layers=lay[:3], want=want)
        assert set(part) == set(want) | {'status'}
        for k in want:
            assert np.array_equal(part[k], many[k][:3], equal_nan=True), (want, k)


def test_absent_views_do_not_change_what_does_not_read_them():
    (p, t, td, z), pb, pt, cls, _ = case(np.float64)
    lay = api_layers(pb, pt)
    full = xa.thermo_layers(p, t, td, z, layers=lay)
    valid = ~(np.isnan(p) | np.isnan(td) | np.isnan(z))
    clean_t = ~np.any(np.isnan(t) & valid, axis=0)            # no level that only temperature would have dropped
    valid = ~(np.isnan(p) | np.isnan(t) | np.isnan(z))
    clean_td = ~np.any(np.isnan(td) & valid, axis=0)
    assert clean_t.sum() >= 2500 and clean_td.sum() >= 2500
    same_bits(xa.thermo_layers(p, None, td, z, layers=lay, want=NO_T), full, NO_T + ('status',), 'no temperature', clean_t)
    same_bits(xa.thermo_layers(p, t, None, z, layers=lay, want=NO_TD), full, NO_TD + ('status',), 'no dewpoint', clean_td)
    # without height: the pressure layers, on columns where no level hangs on the height alone
    valid = ~(np.isnan(p) | np.isnan(t) | np.isnan(td))
    clean_z = ~np.any(np.isnan(z) & valid, axis=0)
    noz = xa.thermo_layers(p, t, td, layers=lay[1:])
    assert set(noz) == set(TK) - {'thickness', 'lapse_rate'} | {'status'}
    sub = xa.thermo_layers(p, t, td, z, layers=lay[1:])
    same_bits(noz, sub, tuple(set(TK) - {'thickness', 'lapse_rate'}) + ('status',), 'no height', clean_z)


def test_scalar_bounds_equal_constant_arrays_and_depth_equals_pressure():
    arrs, pb, pt, _ = inputs(NLEV, 1500, seed=11, p0=1000.0)
    p, t, td, z = arrs
    full = lambda v: np.full(p.shape[1], v)
    a = xa.thermo_layers(*arrs, layers=[{'bottom': 850.0, 'top': 400.0}, {'bottom': None, 'top': 600.0}, {'bottom': 900.0, 'top': None}])
    b = xa.thermo_layers(*arrs, layers=[{'bottom': full(850.0), 'top': full(400.0)}, {'bottom': full(NAN), 'top': full(600.0)},
                                        {'bottom': full(900.0), 'top': None}])
    same_bits(a, b, TK + ('status',), 'constant arrays')
    assert np.isfinite(a['precipitable_water']).sum() >= 3000
    base = ~np.any([np.isnan(x[0]) for x in arrs], axis=0)                # the lowest valid level is level 0: p0 = 1000
    assert base.sum() >= 1200
    for d in (100.0, 150.0, 700.0):
        a = xa.thermo_layers(*arrs, layers=[('pressure_depth', None, d), ('pressure_depth', 900.0, d)])
        b = xa.thermo_layers(*arrs, layers=[('pressure', 1000.0, 1000.0 - d), ('pressure', 900.0, 900.0 - d)])
        same_bits(a, b, TK + ('status',), ('depth', d), base)
        assert np.isfinite(a['mean_mixing_ratio'][0, base]).sum() >= 900


# -- 3. ordering violations ---------------------------------------------------------------------------------------------
def test_ordering_violations():
    arrs, pb, pt, _ = inputs(30, 256, seed=9)
    p, t, td, z = arrs
    z[4, :64] = z[3, :64]                               # equal heights
    p[6, 64:128] = p[5, 64:128] + 1.0                   # pressure rising
    for a in arrs:
        a[:, 200:] = a[:, 200:][::-1]                   # upside down
    ref = restate(arrs, pb, pt)
    got = xa.thermo_layers(*arrs, layers=api_layers(pb, pt))
    compare(got, ref, VALUE_KEYS, scales(arrs, ref), False, 'thermo_layers ordering')
    assert np.count_nonzero(ref['status'] & R.ST_BAD_HEIGHT) >= 90 and np.count_nonzero(ref['status'] & R.ST_BAD_PRESSURE) >= 90
    assert np.isnan(_np(got['thickness'])[:, (ref['status'] & (R.ST_BAD_HEIGHT | R.ST_BAD_PRESSURE)) != 0]).all()
    ref = R.thermo_layers_grid(p, t, td, None, LAYERS[1:], [None, None, pb], [None, None, pt])
    got = xa.thermo_layers(p, t, td, layers=api_layers(pb, pt)[1:])             # without height its order is not looked at
    assert np.array_equal(got['status'], ref['status']) and not np.any(ref['status'] & R.ST_BAD_HEIGHT)
    assert np.array_equal(np.isnan(got['precipitable_water']), np.isnan(ref['precipitable_water']))


# -- 4. small grids -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncol', [1, 257])
def test_small_grids(ncol):
    arrs, pb, pt, cls, _ = case(np.float64)
    cols = np.arange(40, 40 + ncol)
    got = xa.thermo_layers(*(np.ascontiguousarray(a[:, cols]) for a in arrs), layers=api_layers(pb[cols], pt[cols]))
    full = xa.thermo_layers(*arrs, layers=api_layers(pb, pt))
    for k in TK + ('status',):
        assert np.array_equal(got[k], full[k][..., cols], equal_nan=True), k
    if ncol == 1:
        one = xa.thermo_layers(*(a[:, 40] for a in arrs), layers=api_layers(pb[40:41], pt[40:41]))   # a single column, (nlev,)
        assert one['thickness'].shape == (4,) and one['status'].shape == ()
        for k in TK:
            assert np.array_equal(one[k], got[k][:, 0], equal_nan=True), k


# -- 5. input kinds -------------------------------------------------------------------------------------------------------
def _abi_out(n, ncol, device, keys=TK):
    import torch
    res = {k: (torch.empty(n, ncol, dtype=torch.float64, device='cuda') if device else np.empty((n, ncol))) for k in keys}
    res['status'] = torch.empty(ncol, dtype=torch.int32, device='cuda') if device else np.empty(ncol, np.int32)
    ptr = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
    out = L.ThermoLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE if device else L.XP_MEM_HOST, status=ptr(res['status']))
    for k in keys:
        for i in range(n):
            getattr(out, k)[i] = ptr(res[k][i])
    return out, res


def _abi_layers(layers=LAYERS):
    return (L.WindLayer * len(layers))(*[L.WindLayer(k, 0, b, t) for k, b, t in layers])


def _abi_cols(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else (a.data_ptr() if hasattr(a, 'data_ptr') else a.ctypes.data) for a in arrays])


def test_input_kinds_and_strided_views():
    import torch
    arrs, pb, pt, cls, _ = case(np.float64)
    n = 1500
    arrs = [np.ascontiguousarray(a[:, :n]) for a in arrs]
    pb, pt = pb[:n].copy(), pt[:n].copy()
    ref = xa.thermo_layers(*arrs, layers=api_layers(pb, pt))
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        got = xa.thermo_layers(*(conv(a) for a in arrs), layers=api_layers(conv(pb), conv(pt)))
        same_bits(got, ref, TK + ('status',), 'torch')
    assert got['thickness'].is_cuda and got['status'].dtype == torch.int32
    # (ncol, nlev)-major device arrays through the raw ABI: lev_stride 1, col_stride nlev
    nlev = arrs[0].shape[0]
    lib = L.init(0)
    cols = [torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in arrs]
    views = [L.View(x.data_ptr(), L.XP_F64, L.XP_MEM_DEVICE, nlev, n, 1, nlev) for x in cols]
    dpb, dpt = torch.from_numpy(pb).cuda(), torch.from_numpy(pt).cuda()
    out, res = _abi_out(4, n, True)
    L.check(lib.xp_thermo_layers(*views, 4, _abi_layers(), _abi_cols([None, None, None, dpb]), _abi_cols([None, None, None, dpt]), out, None))
    torch.cuda.synchronize()
    same_bits(res, ref, TK + ('status',), 'strided')


# -- 6. the conveniences ------------------------------------------------------------------------------------------------------
def test_conveniences():
    import torch
    (p, t, td, z), pb, pt, cls, ref = case(np.float64)
    n = 3000
    hp, ht, htd, hz = (np.ascontiguousarray(a[:, :n]) for a in (p, t, td, z))
    # precipitable_water: the open layer of thermo_layers (called with pressure and dewpoint alone)
    pw = xa.precipitable_water(hp, htd)
    whole = xa.thermo_layers(hp, dewpoint=htd, layers=[{'bottom': None, 'top': None}, {'bottom': 900.0, 'top': 400.0}], want=('precipitable_water',))
    assert pw.shape == (n,) and np.array_equal(pw, whole['precipitable_water'][0], equal_nan=True) and np.isfinite(pw).sum() >= 2500
    assert np.array_equal(xa.precipitable_water(hp, htd, bottom=900.0, top=400.0), whole['precipitable_water'][1], equal_nan=True)
    rh = xa.mean_relative_humidity(hp, ht, htd)
    lr, th = xa.layer_lapse_rate(hp, ht, hz)
    both = xa.thermo_layers(hp, ht, htd, layers=[('pressure', 700.0, 500.0)], want=('mean_relative_humidity',))   # (no height, as above)
    assert np.array_equal(rh, both['mean_relative_humidity'][0], equal_nan=True) and np.isfinite(rh).sum() >= 1500
    assert np.all(lr[np.isfinite(lr)] > 3.0) and np.all(th[np.isfinite(th)] > 2000.0) and np.isfinite(lr).sum() >= 1500
    # the hail growth zone on the device: the bounds of crossing_level / interp_level, passed on as per-column pressures
    dp, dt, dtd, dz = (torch.from_numpy(a).cuda() for a in (hp, ht, htd, hz))
    thick, lapse = xa.hail_growth_zone_thickness(dp, dt, dz)
    assert thick.is_cuda and lapse.is_cuda and thick.shape == (n,)
    zb, zt = xa.crossing_level(dz, dt, 263.15), xa.crossing_level(dz, dt, 243.15)
    bounds = {'bottom': xa.interp_level(dz, dp, zb), 'top': xa.interp_level(dz, dp, zt)}
    want = xa.thermo_layers(dp, dt, None, dz, layers=[bounds], want=('thickness', 'lapse_rate'))
    assert torch.equal(torch.nan_to_num(thick, nan=-1.0), torch.nan_to_num(want['thickness'][0], nan=-1.0))
    assert torch.equal(torch.nan_to_num(lapse, nan=-1.0), torch.nan_to_num(want['lapse_rate'][0], nan=-1.0))
    host = _np(thick)
    print('hail growth zone: %d of %d columns, %.0f ... %.0f m' % (np.isfinite(host).sum(), n, np.nanmin(host), np.nanmax(host)))
    # (a column without a -10 degC crossing among its valid levels has no bottom: its zone starts at the lowest valid level)
    no_bottom = np.isnan(_np(bounds['bottom']))
    assert np.isfinite(host).sum() >= 1000 and np.all(host[np.isfinite(host)] > 0.0) and np.isfinite(host[~no_bottom]).sum() >= 1000
    # the restatement on the host copies agrees with the device where the layer exists
    r = R.thermo_layers_grid(hp, ht, None, hz, [(R.PRESSURE, NAN, NAN)], [_np(bounds['bottom'])], [_np(bounds['top'])])
    assert np.array_equal(np.isnan(host), np.isnan(r['thickness'][0]))
    has = np.isfinite(host)
    assert np.all(np.abs(host[has] - r['thickness'][0][has]) <= 1e-9 * np.maximum(1.0, r['thickness'][0][has]))
    # theta_e_difference: the restated rule on the arrays the device handed over
    ted = xa.theta_e_difference(dp, dt, dtd, dz)
    assert ted.is_cuda and ted.shape == (n,)
    lay = xa.thermo_layers(dp, dt, dtd, dz, layers=[('height', 0.0, 3000.0)], want=TK[5:])
    tmin, pmin, tmax, pmax = (_np(lay[k][0]) for k in TK[5:])
    rule = np.where(pmax < pmin, 0.0, tmax - tmin)
    got = _np(ted)
    assert np.array_equal(got, rule, equal_nan=True)
    assert np.isnan(got).sum() >= 30 and (got == 0.0).sum() >= 100 and (got > 0.0).sum() >= 1000
    host_ted = xa.theta_e_difference(hp.astype(np.float32), ht.astype(np.float32), htd.astype(np.float32), hz.astype(np.float32))
    assert host_ted.dtype == np.float32 and host_ted.shape == (n,)


# -- 7. the raw ABI's argument checks --------------------------------------------------------------------------------------------
def test_raw_abi_errors():
    lib = L.init(0)
    arrs, pb, pt, _ = inputs(30, 8, seed=2)
    arrs = [np.ascontiguousarray(a) for a in arrs]
    views = [L.View(a.ctypes.data, L.XP_F64, L.XP_MEM_HOST, 30, 8, 8, 1) for a in arrs]
    short = L.View(arrs[3].ctypes.data, L.XP_F64, L.XP_MEM_HOST, 30, 4, 4, 1)
    f32 = L.View(arrs[3].ctypes.data, L.XP_F32, L.XP_MEM_HOST, 30, 8, 8, 1)
    null = L.View(None, L.XP_F64, L.XP_MEM_HOST, 30, 8, 8, 1)
    out, res = _abi_out(4, 8, False)
    bcols, tcols = _abi_cols([None, None, None, pb]), _abi_cols([None, None, None, pt])

    def only(*keys):
        """an output struct that wants just `keys` (of layer 0 ... 3), into the same buffers"""
        o = L.ThermoLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, status=res['status'].ctypes.data)
        for k in keys:
            for i in range(4):
                getattr(o, k)[i] = res[k][i].ctypes.data
        return o

    def call(layers=LAYERS, n=None, vs=views, o=out, arr=True, bc=bcols, tc=tcols):
        for a in res.values():
            a[...] = -77
        rc = lib.xp_thermo_layers(*vs, len(layers) if n is None else n, _abi_layers(layers) if arr else None, bc, tc, o, None)
        if rc != L.XP_OK:
            assert all(np.all(a == -77) for a in res.values()), 'outputs touched'
        return rc
    P, T, TD, Z = views
    assert call() == L.XP_OK and np.isfinite(res['thickness']).any() and not np.any(res['status'] == -77)
    # what may be absent: each view with the outputs that do not read it; the column arrays altogether
    assert call(vs=[P, None, TD, Z], o=only(*NO_T)) == L.XP_OK and np.all(res['lapse_rate'] == -77) and np.isfinite(res['thickness']).any()
    assert call(vs=[P, T, None, Z], o=only(*NO_TD)) == L.XP_OK and np.all(res['theta_e_min'] == -77)
    assert call(LAYERS[1:3], vs=[P, T, TD, None], o=only(*(set(TK) - {'thickness', 'lapse_rate'})), bc=None, tc=None) == L.XP_OK
    assert np.all(res['precipitable_water'][2:] == -77) and np.isfinite(res['precipitable_water'][:2]).any()
    assert call(LAYERS[1:3], vs=[P, None, None, None], o=only(), bc=None, tc=None) == L.XP_OK and not np.any(res['status'] == -77)
    assert call([(R.PRESSURE, 850.0, NAN)], bc=None, tc=None) == L.XP_OK                  # the open top: not an error here
    assert call([(R.PRESSURE, float('inf'), float('inf'))], bc=_abi_cols([pb]), tc=_abi_cols([pt])) == L.XP_OK   # replaced scalars: not looked at
    inf = float('inf')
    no_cols = dict(bc=None, tc=None)
    bad = [(dict(layers=LAYERS[:1], vs=[P, T, TD, None], o=only('precipitable_water'), **no_cols), 'needs height'),
           (dict(n=0), 'nlayer'), (dict(layers=LAYERS + LAYERS[:1], n=5), 'nlayer'), (dict(arr=False), 'null'),
           (dict(layers=[(R.PRESSURE_DEPTH, NAN, 0.0)], **no_cols), 'depth'), (dict(layers=[(R.PRESSURE_DEPTH, 900.0, -10.0)], **no_cols), 'depth'),
           (dict(layers=[(R.PRESSURE_DEPTH, 900.0, NAN)], **no_cols), 'top'),
           (dict(layers=[(R.HEIGHT, 500.0, 500.0)], **no_cols), 'depth'), (dict(layers=[(R.HEIGHT, 600.0, 500.0)], **no_cols), 'depth'),
           (dict(layers=[(R.HEIGHT, -1.0, 500.0)], **no_cols), 'bottom'), (dict(layers=[(R.HEIGHT, 0.0, NAN)], **no_cols), 'top'),
           (dict(layers=[(R.PRESSURE, 850.0, inf)], **no_cols), 'top'), (dict(layers=[(R.HEIGHT, 0.0, inf)], **no_cols), 'top'),
           (dict(layers=[(R.PRESSURE, inf, 300.0)], **no_cols), 'bottom'), (dict(layers=[(R.PRESSURE, -inf, 300.0)], **no_cols), 'bottom'),
           (dict(layers=LAYERS[:3] + [(3, 0.0, 1.0)]), 'kind'), (dict(layers=[(-1, 0.0, 1.0)], **no_cols), 'kind'),
           # a per-column array on a layer that is not by pressure
           (dict(layers=[(R.HEIGHT, 0.0, 3000.0)], bc=_abi_cols([pb]), tc=None), 'per-column'),
           (dict(layers=[(R.PRESSURE_DEPTH, NAN, 100.0)], bc=None, tc=_abi_cols([pt])), 'per-column'),
           (dict(layers=LAYERS, bc=_abi_cols([None, None, None, pb]), tc=_abi_cols([pt, None, None, pt])), 'per-column'),
           # a wanted output whose view is absent
           (dict(vs=[P, None, TD, Z], o=only('mean_relative_humidity')), 'temperature'),
           (dict(vs=[P, None, TD, Z], o=only('lapse_rate')), 'temperature'),
           (dict(vs=[P, None, TD, Z], o=only('theta_e_max_pressure')), 'temperature'),
           (dict(vs=[P, T, None, Z], o=only('precipitable_water')), 'dewpoint'), (dict(vs=[P, T, None, Z], o=only('mean_mixing_ratio')), 'dewpoint'),
           (dict(vs=[P, T, None, Z], o=only('mean_relative_humidity')), 'dewpoint'), (dict(vs=[P, T, None, Z], o=only('theta_e_min')), 'dewpoint'),
           (dict(layers=LAYERS[1:], vs=[P, T, TD, None], o=only('thickness'), bc=_abi_cols([None, None, pb]), tc=_abi_cols([None, None, pt])), 'height'),
           (dict(layers=LAYERS[1:], vs=[P, T, TD, None], o=only('lapse_rate'), bc=_abi_cols([None, None, pb]), tc=_abi_cols([None, None, pt])), 'height'),
           # the views and the output struct
           (dict(vs=[None, T, TD, Z]), 'pressure'), (dict(vs=[null, T, TD, Z]), 'pressure'),
           (dict(vs=[P, T, TD, short]), 'differ'), (dict(vs=[P, short, TD, Z]), 'differ'), (dict(vs=[P, T, f32, Z]), 'differ'),
           (dict(o=None), 'out'),
           (dict(o=L.ThermoLayersOut(dtype=L.XP_F32, mem=L.XP_MEM_HOST, status=res['status'].ctypes.data)), 'out'),
           (dict(o=L.ThermoLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_DEVICE, status=res['status'].ctypes.data)), 'out')]
    for kw, word in bad:
        assert call(**kw) == L.XP_E_ARG, kw
        assert word in lib.xp_last_error().decode(), (kw, lib.xp_last_error())
    # and the wind entry still rejects the NaN top that is the open one here
    wout = L.WindLayersOut(dtype=L.XP_F64, mem=L.XP_MEM_HOST, status=res['status'].ctypes.data)
    assert lib.xp_wind_layers(P, T, TD, Z, 1, _abi_layers([(R.PRESSURE, 850.0, NAN)]), wout, None) == L.XP_E_ARG


# -- 8. the wind walk and this one choose the same layers -------------------------------------------------------------------
# one by pressure, one by pressure depth from the lowest valid level, two by height
SHARED_LAYERS = [('pressure', 850.0, 500.0), ('pressure_depth', None, 150.0), ('height', 0.0, 1000.0), ('height', 500.0, 3000.0)]


def shared_inputs(ncol, dtype):
    """Pressure and height (24, 257) for both entries, and u, v / T, Td with their missing values at the same (level, column):
    ~6 % of them, the lowest level among them, so that the lowest valid level differs between columns.  In every column one
    valid level is moved onto a bound of SHARED_LAYERS -- 850 and 500 hPa, p0 - 150 hPa, z0 + 500, 1000 and 3000 m -- or next
    to it by OFFSETS (relative in pressure; a height offset of 8200 m x the relative one), bound and offset cycling with the
    column; one column in 13 ends 2.5 km up, one in 17 600 m up, and one in 11 begins above 850 hPa.  ncol == 1: column 5."""
    rng = np.random.default_rng(23)
    nlev, n = 24, 257
    miss = rng.random((nlev, n)) < 0.06
    miss[:, ::16] = False
    ok0 = np.argmin(miss, axis=0)                                # the lowest valid level
    z = rng.integers(0, 1500, n) + np.vstack([np.zeros(n), np.cumsum(rng.uniform(100.0, 700.0, (nlev - 1, n)), axis=0)])
    psfc = rng.uniform(985.0, 1030.0, n)
    psfc[3::11] = rng.uniform(780.0, 840.0, psfc[3::11].size)    # (11, 13, 17: every bound and offset meets every kind of column)
    cols = np.arange(n)
    z0 = z[ok0, cols]
    scale = rng.uniform(7600.0, 8800.0, n)
    targets = [('p', 850.0), ('p', 500.0), ('dp', 150.0), ('z', 500.0), ('z', 1000.0), ('z', 3000.0)]
    combos = [(t, o) for t in targets for o in OFFSETS]
    for c in cols:
        (kind, t), off = combos[c % len(combos)]
        if kind == 'z':
            want = z0[c] + t + off * 8200.0
            k = int(np.argmin(np.where(miss[:, c], np.inf, np.abs(z[:, c] - want))))
            if ok0[c] < k < nlev - 1 and z[k - 1, c] < want < z[k + 1, c]:
                z[k, c] = want
    p = psfc * np.exp(-(z - z[0]) / scale)
    p0 = p[ok0, cols]
    for c in cols:
        (kind, t), off = combos[c % len(combos)]
        if kind != 'z':
            want = (t if kind == 'p' else p0[c] - t) * (1.0 + off)
            k = int(np.argmin(np.where(miss[:, c], np.inf, np.abs(p[:, c] - want))))
            if ok0[c] < k < nlev - 1 and p[k - 1, c] > want > p[k + 1, c]:
                p[k, c] = want
    u = rng.normal(5.0, 8.0, (nlev, n))
    v = rng.normal(0.0, 8.0, (nlev, n))
    t = 295.0 - 6.5e-3 * (z - z[0]) + rng.normal(0.0, 0.5, (nlev, n))
    td = t - np.abs(rng.normal(0.0, 6.0, (nlev, n)))
    u[miss] = np.nan
    t[miss] = np.nan
    p[(z - z0 > 2500.0) & (cols % 13 == 7)] = np.nan
    p[(z - z0 > 600.0) & (cols % 17 == 9)] = np.nan
    sel = slice(None) if ncol == n else slice(5, 5 + ncol)
    return [np.ascontiguousarray(a[:, sel].astype(dtype)) for a in (p, z, u, v, t, td)]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('ncol', [257, 1])
def test_wind_and_thermo_walks_choose_the_same_layers(ncol, dtype):
    """k_wind_layers and k_thermo_layers take which points a layer has from one rule (csrc/xp_layer_gate.hpp): on the same
    pressure, height and layers, with the missing levels in the same places, they find the same layers -- the same status in
    every column, and a layer's mean wind is NaN exactly where its thickness is.  24 x 257: one full workgroup and a one-lane
    tail.  Nothing is left out of the comparison."""
    p, z, u, v, t, td = shared_inputs(ncol, dtype)
    wind = xa.wind_layers(p, u, v, z, layers=SHARED_LAYERS, want=('mean_u',))
    thermo = xa.thermo_layers(p, t, td, z, layers=SHARED_LAYERS, want=('thickness',))
    assert wind['status'].shape == thermo['status'].shape == (ncol,)
    assert np.array_equal(wind['status'], thermo['status'])
    for i in range(len(SHARED_LAYERS)):
        assert np.array_equal(np.isnan(wind['mean_u'][i]), np.isnan(thermo['thickness'][i])), i
    if ncol > 1:                                                 # every layer is found in some columns and missing in others
        nan_l = np.isnan(thermo['thickness'])
        assert np.all(nan_l.sum(axis=1) >= 10) and np.all((~nan_l).sum(axis=1) >= 100), nan_l.sum(axis=1)
