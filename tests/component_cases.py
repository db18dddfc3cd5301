"""Deterministic inputs for the grid-scale tests of the staged component kernels (lcl, dry_lapse, moist_lapse,
parcel_profile, lfc_el, cape_cin_base, most_unstable_parcel, mixed_parcel, mixed_layer): tests/test_gpu_components.py
runs them on the GPU against the C oracle, tests/test_component_cases_cpu.py checks here, without a GPU, that the two
CPU oracles agree on every one of them and that no class of input has silently gone missing.

Every builder is a pure function of its arguments (one seeded generator, drawn from in a fixed order) and returns
float64 arrays laid out (nlev, ncol).  Pressures are multiples of 1/64 hPa below 1100 hPa and the quantised temperatures
multiples of 1/64 K, so that "exactly on a level" and "exactly zero" survive the rounding of the inputs to float32.
"""
import numpy as np

from oracle import thermo as th
from xarray_parcel_amd import synth

NCOL, NLEV = 1337, 24           # five full 256-thread blocks + a ragged one, a last wavefront with 7 idle lanes
SMALL_SHAPES = ((NLEV, 1), (1, 300), (2, 300))      # (nlev, ncol): one column; one and two levels over two blocks


def cast(x, dtype):
    """x rounded to `dtype` (what the kernel is given) and the same values as float64 (what the oracle is given)."""
    if x is None:
        return None, None
    g = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(dtype))
    return g, g.astype(np.float64)


def pressures(nlev, ncol, seed):
    """Strictly decreasing columns from 950 ... 1030 hPa down to 100 hPa, multiples of 1/64 hPa."""
    u = synth.column_uniforms(ncol, seed)
    k = np.arange(nlev, dtype=np.float64)[:, None]
    sigma = 1.0 - (k / float(max(nlev - 1, 1))) ** 1.3
    p = 100.0 + (950.0 + 80.0 * u[0] - 100.0) * sigma
    p = np.round(p * 64.0) / 64.0
    assert nlev < 2 or np.all(np.diff(p, axis=0) < 0)
    return p


def per_column(fn, ncol):
    """fn(c) -> dict of scalars / arrays, for every column: dict of stacked arrays with the column axis last."""
    rows = [fn(c) for c in range(ncol)]
    return {k: np.stack([np.asarray(r[k]) for r in rows], axis=-1) for k in rows[0]}


# ---- 1. crafted difference profiles for lfc_el / cape_cin_base ------------------------------------------------------
SCAN_SHAPES = ('all_positive', 'all_negative', 'crossings_1', 'crossings_2', 'crossings_3', 'crossings_4', 'crossings_5',
               'crossings_6', 'zero_interior', 'zero_first', 'zero_last', 'zero_pair',
               'nan_parcel_interior', 'nan_parcel_first', 'nan_parcel_last', 'nan_env_interior', 'nan_env_first',
               'nan_env_last', 'nan_both_interior', 'nan_both_first', 'nan_both_last', 'nan_parcel_all')
LCL_KINDS = ('on_level', 'between', 'below_bottom', 'above_top', 'nan')


def _signed_profile(rng, nlev, crossings, first_sign, quantised):
    """parcel - environment with `crossings` sign changes (between nodes, none on a node), |value| in 0.25 ... 6 K."""
    crossings = min(crossings, nlev - 1)
    cuts = set(rng.choice(nlev - 1, size=crossings, replace=False).tolist()) if crossings else set()
    mag = rng.uniform(0.25, 6.0, nlev)
    if quantised:
        mag = np.maximum(np.round(mag * 4.0) / 4.0, 0.25)
    d, s = np.empty(nlev), first_sign
    for k in range(nlev):
        d[k] = s * mag[k]
        if k in cuts:
            s = -s
    return d


def scan_profiles(nlev=NLEV, ncol=NCOL, seed=101):
    """Columns of (p, parcel, env) with a prescribed parcel - env, an LCL pressure and an LCL temperature each.
    Column c has shape class SCAN_SHAPES[c % 22] and LCL placement LCL_KINDS[c % 5] (22 and 5 are coprime: every
    combination occurs).  The columns of class 'zero_interior' whose LCL is 'on_level' are the knife-edge ones: negative
    below a node that is exactly zero and carries the LCL, positive above it, negative again further up -- the crossing
    sits ON the LCL, and whether it counts as an LFC above the LCL or the LFC is replaced by the LCL hangs on the last
    bit of exp(log(p)); pressure and temperature of the LFC are the same either way."""
    rng = np.random.default_rng(seed)
    p = pressures(nlev, ncol, seed)
    env = np.round((200.0 + 95.0 * (p / 1050.0)) * 64.0) / 64.0
    diff = np.empty((nlev, ncol))
    par_nan = np.zeros((nlev, ncol), dtype=bool)
    env_nan = np.zeros((nlev, ncol), dtype=bool)
    lcl_p, lcl_t = np.empty(ncol), np.empty(ncol)
    shape = np.arange(ncol) % len(SCAN_SHAPES)
    kind = np.arange(ncol) % len(LCL_KINDS)
    crafted = np.zeros(ncol, dtype=bool)
    interior = lambda: min(1 + int(rng.integers(max(nlev - 2, 1))), nlev - 1)
    for c in range(ncol):
        name = SCAN_SHAPES[shape[c]]
        first = 1.0 if rng.integers(2) else -1.0
        on_level = None
        if name == 'all_positive':
            d = _signed_profile(rng, nlev, 0, 1.0, False)
        elif name == 'all_negative':
            d = _signed_profile(rng, nlev, 0, -1.0, False)
        elif name.startswith('crossings_'):
            d = _signed_profile(rng, nlev, int(name[-1]), first, False)
        elif name.startswith('zero_'):
            d = _signed_profile(rng, nlev, 1 + int(rng.integers(3)), first, True)
            k = interior()
            if name == 'zero_interior' and LCL_KINDS[kind[c]] == 'on_level' and nlev >= 4:
                k = 1 + int(rng.integers(nlev - 3))                       # 1 ... nlev - 3
                m = k + 1 + int(rng.integers(nlev - 2 - k))               # k + 1 ... nlev - 2: last positive node
                d = np.abs(d)
                d[:k] *= -1.0
                d[m + 1:] *= -1.0
                on_level, crafted[c] = k, True
            pair = min(k, max(nlev - 3, 0))
            d[{'zero_interior': k, 'zero_first': 0, 'zero_last': nlev - 1, 'zero_pair': pair}[name]] = 0.0
            if name == 'zero_pair':
                d[min(pair + 1, nlev - 1)] = 0.0                           # two consecutive nodes
        else:
            d = _signed_profile(rng, nlev, int(rng.integers(4)), first, False)
            where = {'interior': interior(), 'first': 0, 'last': nlev - 1, 'all': slice(None)}[name.rsplit('_', 1)[1]]
            if '_parcel_' in name or '_both_' in name:
                par_nan[where, c] = True
            if '_env_' in name or '_both_' in name:
                env_nan[where, c] = True
        diff[:, c] = d
        # the LCL
        lk = LCL_KINDS[kind[c]]
        lcl_t[c] = 250.0 + 40.0 * rng.random()
        f = 0.2 + 0.6 * rng.random()
        if lk == 'on_level':
            k = int(rng.integers(nlev)) if on_level is None else on_level
            for _ in range(nlev):                                          # not on a zero node unless crafted so
                if on_level is not None or d[k] != 0.0:
                    break
                k = (k + 1) % nlev
            lcl_p[c] = p[k, c]
            if on_level is not None:
                lcl_t[c] = env[k, c] + d[k]
        elif lk == 'between':
            k = int(rng.integers(max(nlev - 1, 1)))
            lcl_p[c] = p[k, c] * (1.0 - f) + p[min(k + 1, nlev - 1), c] * f if nlev > 1 else p[0, c] - 3.0
        elif lk == 'below_bottom':
            lcl_p[c] = p[0, c] + 5.0 + 25.0 * f
        elif lk == 'above_top':
            lcl_p[c] = p[-1, c] - 1.0 - 19.0 * f
        else:
            lcl_p[c] = np.nan
    parcel = np.where(par_nan, np.nan, env + diff)
    return {'pressure': p, 'parcel': parcel, 'env': np.where(env_nan, np.nan, env), 'lcl_pressure': lcl_p,
            'lcl_temperature': lcl_t, 'shape': shape, 'lcl_kind': kind, 'crafted_knife_edge': crafted}


def knife_edge_columns(pressure, parcel, env, lcl_pressure):
    """Columns that hold a zero or a sign change of parcel - env whose pressure is within 1e-9 (relative) of the LCL
    pressure -- from the inputs alone (float64 copies of what the kernel is given)."""
    p, y = np.asarray(pressure, dtype=np.float64), np.asarray(parcel, dtype=np.float64) - np.asarray(env, dtype=np.float64)
    if p.shape[0] < 2:
        return np.zeros(p.shape[1], dtype=bool)
    with np.errstate(all='ignore'):
        x, y0, y1 = np.log(p), y[:-1], y[1:]
        change = (np.sign(y0) != np.sign(y1)) & ~np.isnan(y0) & ~np.isnan(y1)
        xs = (y1 * x[:-1] - y0 * x[1:]) / (y1 - y0)
        near = np.abs(np.exp(xs) - lcl_pressure[None, :]) <= 1e-9 * lcl_pressure[None, :]
    return np.any(change & near, axis=0)


BASE_SOURCES = ('oracle_lfc_el', 'level_and_nan', 'between_levels')
# (the fourth set is the one in which post_zero_cin has something to do: unfiltered sums can leave CIN positive)
BASE_OPTIONS = (dict(), dict(pos_cape_neg_cin=False), dict(post_zero_cin=True), dict(pos_cape_neg_cin=False, post_zero_cin=True))


def base_bounds(pressure, source, lfc_el=None):
    """(LFC pressure, EL pressure) per column for cape_cin_base: what lfc_el found; a level pressure with a NaN EL (the
    pf.py:1329 fallback onto the lowest pressure of the column); values strictly between levels."""
    p = np.asarray(pressure, dtype=np.float64)
    nlev, ncol = p.shape
    c = np.arange(ncol)
    if source == 'oracle_lfc_el':
        return np.asarray(lfc_el['lfc_pressure'], dtype=np.float64), np.asarray(lfc_el['el_pressure'], dtype=np.float64)
    if source == 'level_and_nan':
        return p[c % nlev, c].copy(), np.full(ncol, np.nan)
    if nlev == 1:
        return p[0] * 0.9, p[0] * 0.5
    j = c % (nlev - 1)
    m = np.minimum(j + 1 + (c // 7) % np.maximum(nlev - 2 - j, 1), nlev - 2)
    return p[j, c] * 0.63 + p[j + 1, c] * 0.37, p[m, c] * 0.39 + p[m + 1, c] * 0.61


# ---- 2. the point and lapse kernels -----------------------------------------------------------------------------------
LCL_KINDS_OF_PARCEL = ('ordinary', 'ordinary', 'saturated', 'depression_40', 'cold', 'nan_input', 'ordinary', 'humid')


def lcl_parcels(n=NCOL, seed=202):
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % len(LCL_KINDS_OF_PARCEL)
    p = 600.0 + 450.0 * rng.random(n)
    t = 235.0 + 80.0 * rng.random(n)
    dd = 0.5 + 24.5 * rng.random(n)
    name = np.array(LCL_KINDS_OF_PARCEL)[kind]
    dd[name == 'saturated'] = 0.0
    dd[name == 'depression_40'] = 40.0
    cold = name == 'cold'
    t[cold] = 220.0 + 15.0 * rng.random(int(cold.sum()))
    dd[cold] = 1.0 + 14.0 * rng.random(int(cold.sum()))
    dd[name == 'humid'] = 0.5 + 2.0 * rng.random(int((name == 'humid').sum()))
    td = t - dd
    which = (np.arange(n) // len(LCL_KINDS_OF_PARCEL)) % 3                  # NaN in each input, one at a time
    nan = name == 'nan_input'
    p[nan & (which == 0)] = np.nan
    t[nan & (which == 1)] = np.nan
    td[nan & (which == 2)] = np.nan
    return {'pressure': p, 'temperature': t, 'dewpoint': td, 'kind': kind}


REF_KINDS = ('inside', 'inside', 'on_level', 'above_top', 'below_bottom', 'inside')


def lapse_cases(nlev=NLEV, ncol=NCOL, seed=303):
    """Pressure columns with NaN levels and three ways of giving the reference pressure: 'none' (the kernel's default),
    'scalar' (700 hPa: inside every column) and 'array' (per column: strictly inside the column, exactly on a level,
    above the top, below the bottom).  A third of the columns has a NaN level on either side of the per-column reference
    pressure, every 11th a NaN bottom level; some parcel temperatures, and some per-column reference pressures, are NaN."""
    rng = np.random.default_rng(seed)
    p = pressures(nlev, ncol, seed)
    c = np.arange(ncol)
    kind = c % len(REF_KINDS)
    name = np.array(REF_KINDS)[kind]
    f = 0.15 + 0.7 * rng.random(ncol)
    j = rng.integers(max(nlev - 1, 1), size=ncol)                          # lower bracket of the reference pressure
    jn = np.minimum(j + 1, nlev - 1)
    ref = p[j, c] * (1.0 - f) + p[jn, c] * f
    ref[name == 'on_level'] = p[j, c][name == 'on_level']
    ref[name == 'above_top'] = p[-1, c][name == 'above_top'] - 20.0
    ref[name == 'below_bottom'] = p[0, c][name == 'below_bottom'] + 15.0 + 25.0 * f[name == 'below_bottom']
    if nlev == 1:
        ref[name == 'inside'] = p[0, c][name == 'inside'] - 30.0
    holes = np.nonzero(c % 3 == 0)[0]
    for col in holes:                                                      # a NaN level on either side of the reference
        for k in (j[col] - 1, j[col] + 2):
            if 0 <= k < nlev and nlev > 2:
                p[k, col] = np.nan
    bottom = p[0].copy()
    p[0, c % 11 == 0] = np.nan
    theta = 280.0 + 30.0 * rng.random(ncol)

    def t_at(pref):
        with np.errstate(invalid='ignore'):
            t0 = np.maximum(theta * (pref / 1000.0) ** th.KAPPA, 185.0)
        t0 = np.where(c % 13 == 5, np.nan, t0)
        return t0
    ref_nan = ref.copy()
    ref_nan[c % 17 == 7] = np.nan
    return {'pressure': p, 'ref_kind': kind, 'bracket': j,
            'none': (t_at(bottom), None), 'scalar': (t_at(np.full(ncol, 700.0)), 700.0), 'array': (t_at(ref), ref_nan)}


def parcel_profile_cases(nlev=NLEV, ncol=NCOL, seed=404):
    """Pressure columns (a quarter with NaN levels) and one parcel per column: on the bottom level, on an interior
    level, or below the column; every fifth saturated -- on a level its LCL is that level (the P == LCL branch)."""
    rng = np.random.default_rng(seed)
    p = pressures(nlev, ncol, seed)
    c = np.arange(ncol)
    j = np.minimum(1 + c % 5, nlev - 1)
    pp = np.where(c % 3 == 0, p[0], np.where(c % 3 == 1, p[j, c], p[0] + 7.0))
    pt = 200.0 + 95.0 * (pp / 1050.0) + 4.0 * rng.random(ncol)
    dd = np.where(c % 5 == 0, 0.0, 0.5 + 19.5 * rng.random(ncol))
    ptd = pt - dd
    bad = c % 29 == 3
    pp, pt, ptd = np.where(bad & (c % 2 == 0), np.nan, pp), np.where(bad & (c % 2 == 1), np.nan, pt), ptd.copy()
    holes = np.nonzero(c % 4 == 1)[0]
    if nlev > 8:
        p[7 + holes % (nlev - 8), holes] = np.nan
        p[nlev - 1, holes[::3]] = np.nan
    elif nlev == 2:
        p[1, holes] = np.nan
    return {'pressure': p, 'parcel_pressure': pp, 'parcel_temperature': pt, 'parcel_dewpoint': ptd,
            'saturated_on_level': (c % 5 == 0) & (c % 3 != 2) & ~bad}


# ---- 3. parcel selection -------------------------------------------------------------------------------------------
MU_DEPTHS, ML_DEPTHS = (100, 300), (50, 100, 250)
TIE_DELTAS = (1e-7, 1e-6, 1e-5, 1.9e-5, 2.1e-5, 1e-4)        # in ln theta_e; the fp64 repeat of the search starts below 2e-5
SELECT_GROUPS = ('shallow', 'top_on_level_50', 'top_on_level_100', 'top_on_level_250', 'top_on_level_300',
                 'nan_below_top_50', 'nan_below_top_100', 'nan_below_top_250', 'top_on_level_100_nan_below',
                 'theta_e_tie', 'theta_e_tie', 'plain', 'plain', 'plain', 'plain', 'plain')
TIE_LEVELS = (1, 3)


def ln_theta_e(p, t, td):
    with np.errstate(all='ignore'):
        return np.log(th.equivalent_potential_temperature(p, t, td))


def select_cases(nlev=NLEV, ncol=NCOL, seed=505):
    """synth.columns(nan_fraction=0.08) with, per SELECT_GROUPS[c % 16]: columns shallower than every depth; the layer
    top (bottom pressure - depth) exactly on a level; NaN temperature and dewpoint at the last level below the layer
    top; and columns in which levels 1 and 3 carry the two highest theta_e of the layer, TIE_DELTAS apart in
    ln theta_e with the leader alternating (dewpoint of level 3 found by bisection), everything else far behind."""
    p, t, td = synth.columns(nlev=nlev, ncol=ncol, seed=seed, nan_fraction=0.08)
    clean = synth.columns(nlev=nlev, ncol=ncol, seed=seed)
    group = np.arange(ncol) % len(SELECT_GROUPS)
    tie_delta = np.full(ncol, np.nan)
    if nlev < 8:
        return {'pressure': p, 'temperature': t, 'dewpoint': td, 'group': group, 'tie_delta': tie_delta}
    n_tie = 0
    for c in range(ncol):
        name = SELECT_GROUPS[group[c]]
        if name == 'shallow':
            p[:, c] = np.round(p[0, c] * 4.0) / 4.0 - 1.5 * np.arange(nlev)
        depth = float(name.split('_')[3]) if name.startswith(('top_on_level', 'nan_below_top')) else None
        if name.startswith('top_on_level'):
            p[0, c] = np.round(p[0, c] * 4.0) / 4.0                        # bottom - depth is then exact in float32 too
            top = p[0, c] - depth
            k = 1 + int(np.argmin(np.abs(p[1:, c] - top)))
            p[k, c] = top
            assert p[k - 1, c] > top and (k + 1 >= nlev or p[k + 1, c] < top)
        if name.startswith('nan_below_top') or name.endswith('nan_below'):
            k = int(np.nonzero(p[:, c] > p[0, c] - depth)[0][-1])          # last level strictly below the layer top
            t[k, c] = td[k, c] = np.nan
        if name == 'theta_e_tie':
            a, b = TIE_LEVELS
            delta = TIE_DELTAS[n_tie % len(TIE_DELTAS)] * (1.0 if (n_tie // len(TIE_DELTAS)) % 2 == 0 else -1.0)
            n_tie += 1
            pc, tc = clean[0][:, c], clean[1][:, c].copy()
            layer = np.nonzero(pc >= pc[0] - 320.0)[0]
            tc[layer] -= 12.0                                              # every other level of the layer: cold and dry
            tdc = tc - 20.0
            tc[a] = tc[b] = clean[1][a, c]
            tdc[a] = tc[a] - 3.0
            target = ln_theta_e(pc[a], tc[a], tdc[a]) + delta              # delta > 0: level b leads
            lo, hi = tc[b] - 30.0, tc[b]
            assert ln_theta_e(pc[b], tc[b], lo) < target < ln_theta_e(pc[b], tc[b], hi)
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if mid == lo or mid == hi:
                    break
                if ln_theta_e(pc[b], tc[b], mid) < target:
                    lo = mid
                else:
                    hi = mid
            tdc[b] = hi if delta > 0 else lo
            t[:, c], td[:, c] = tc, tdc
            e = ln_theta_e(pc, tc, tdc)
            tie_delta[c] = e[b] - e[a]
            assert np.max(np.delete(e[layer], [a, b])) < min(e[a], e[b]) - 1e-3
    return {'pressure': p, 'temperature': t, 'dewpoint': td, 'group': group, 'tie_delta': tie_delta}


# ---- 4. the staged pipeline --------------------------------------------------------------------------------------------
def pipeline_columns(ncol=NCOL, seed=606):
    p, t, td = synth.columns(nlev=33, ncol=ncol, seed=seed, nan_fraction=0.08)
    return {'pressure': p, 'temperature': t, 'dewpoint': td,
            'surface': (p[0].copy(), t[0].copy(), td[0].copy()), 'explicit': (p[0] + 5.0, t[0] + 1.0, td[0] - 1.0)}


# ---- the per-column oracle loops (shared by the CPU guard and the GPU tests) -------------------------------------------
def numpy_oracle():
    """oracle/parcel_oracle.py behind the call signatures of oracle/c_oracle.py (RK4 moist adiabat, per-column LCL)."""
    from types import SimpleNamespace
    from oracle import parcel_oracle as po

    def mixed_parcel(p, t, td, depth=100):
        r = po.mixed_parcel(p, t, td, depth=depth)
        return {k: float(r[k]) for k in ('pressure', 'temperature', 'dewpoint')}
    return SimpleNamespace(
        lfc_el=po.lfc_el, cape_cin_base=po.cape_cin_base, dry_lapse=po.dry_lapse, mixed_layer=po.mixed_layer,
        lcl=lambda p, t, td: po.lcl(p, t, td, per_column=True),
        moist_lapse=lambda p, t0, pp=None: po.moist_lapse(p, t0, pp, moist='rk4'),
        parcel_profile=lambda p, pp, pt, ptd: po.parcel_profile(p, pp, pt, ptd, moist='rk4', per_column_lcl=True),
        most_unstable_parcel=po.most_unstable_parcel, mixed_parcel=mixed_parcel)


LFC_EL_FLOATS = ('lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature')
LFC_EL_KEYS = LFC_EL_FLOATS + ('lfc_index', 'el_index', 'status_top_nan')
LCL_KEYS = ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature')
PARCEL_KEYS = ('pressure', 'temperature', 'dewpoint')


def run_lfc_el(o, p, parcel, env, lcl_p, lcl_t):
    with np.errstate(all='ignore'):
        return per_column(lambda c: o.lfc_el(p[:, c], parcel[:, c], env[:, c], lcl_p[c], lcl_t[c]), p.shape[1])


def run_cape_cin_base(o, p, env, parcel, lfc_p, el_p, **opts):
    with np.errstate(all='ignore'):
        return per_column(lambda c: o.cape_cin_base(p[:, c], env[:, c], lfc_p[c], el_p[c], parcel[:, c], **opts), p.shape[1])


def run_lcl(o, p, t, td):
    with np.errstate(all='ignore'):
        return per_column(lambda c: {k: float(v) for k, v in o.lcl(p[c], t[c], td[c]).items()}, p.shape[0])


def run_lapse(fn, p, t0, pp):
    """dry_lapse / moist_lapse column by column; pp: None, a scalar or one reference pressure per column."""
    ncol = p.shape[1]
    ppc = None if pp is None else np.broadcast_to(np.asarray(pp, dtype=np.float64), (ncol,))
    import warnings
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.stack([np.asarray(fn(p[:, c], float(t0[c]), None if ppc is None else float(ppc[c])), dtype=np.float64)
                         for c in range(ncol)], axis=-1)


def run_parcel_profile(o, p, pp, pt, ptd):
    def one(c):
        r = o.parcel_profile(p[:, c], float(pp[c]), float(pt[c]), float(ptd[c]))
        return {k: r[k] for k in ('temperature', 'virtual_temperature') + LCL_KEYS}
    with np.errstate(all='ignore'):
        return per_column(one, p.shape[1])


def run_most_unstable(o, p, t, td, depth):
    with np.errstate(all='ignore'):
        return per_column(lambda c: o.most_unstable_parcel(p[:, c], t[:, c], td[:, c], depth=depth), p.shape[1])


def run_mixed(o, p, t, td, depth):
    """mixed_parcel (pressure, temperature, dewpoint) and mixed_layer of temperature and dewpoint ('mean_...')."""
    def one(c):
        r = {k: float(v) for k, v in o.mixed_parcel(p[:, c], t[:, c], td[:, c], depth=depth).items() if k in PARCEL_KEYS}
        m = o.mixed_layer({'pressure': p[:, c], 'temperature': t[:, c], 'dewpoint': td[:, c]}, depth=depth)
        r.update({'mean_' + k: float(v) for k, v in m.items()})
        return r
    import warnings
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return per_column(one, p.shape[1])
