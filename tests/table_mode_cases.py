"""Deterministic inputs for the lookup-table moist mode (XP_MOIST_TABLE, pf.py:525-607), placed relative to the TABLE's grid
rather than to the column: tests/test_gpu_table_mode.py runs them on the GPU, tests/test_table_mode_cases_cpu.py checks here,
without a GPU, that the oracles agree on every one of them and that no class of input has silently gone missing.

What Moist::start / Moist::at (csrc/xp_device.hpp) do that no other moist mode does, and the class that reaches it:
  nearest cell, pandas' tie rules (pressure index DEcreasing: the higher pressure wins; temperature index increasing: the
  higher temperature wins)                                 p_tie, t_tie and their one-ulp neighbours, node
  a start point outside the index grid is clamped          p_above_max, p_below_min, t_below_min, t_above_max
  index value 0: no adiabat, NaN above the LCL             empty_first (next to filled_edge, the last filled cell of its row)
  NaN start point                                          nan_p, nan_t, nan_both
  levels outside p_min ... p_max are NaN, the lo >= n_p - 1 end case, np.interp with IEEE division       eval_pressures()
  geometry other than 2196 x 7150                          small_table()

Every builder is a pure function of its arguments.  Arrays come in the dtype asked for (what the kernel is given); the
oracles are fed the same values as float64, as everywhere in this suite.
"""
import numpy as np

from xarray_parcel_amd import synth

NLEV, NCOL = 33, 1337           # five full 256-thread blocks and a ragged one


def full_tables():
    from oracle import tables as tb
    return tb.get_tables()


def node_pressure(tab, ip):
    return tab.p_max - np.asarray(ip, dtype=np.float64) * tab.p_step


def node_temperature(tab, jt):
    return tab.t_min + np.asarray(jt, dtype=np.float64) * tab.t_step


def raw_cell(tab, pressure, temperature):
    """Nearest cell of (pressure, temperature) BEFORE clamping, with pandas' tie rules (oracle/tables.py nearest_index_*),
    as float arrays (NaN for a NaN input)."""
    p, t = np.asarray(pressure, dtype=np.float64), np.asarray(temperature, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        fi, fj = (tab.p_max - p) / tab.p_step, (t - tab.t_min) / tab.t_step
        i0, j0 = np.floor(fi), np.floor(fj)
        ip = np.where((i0 + 1.0) - fi < fi - i0, i0 + 1.0, i0)
        jt = np.where((j0 + 1.0) - fj <= fj - j0, j0 + 1.0, j0)
    return ip, jt


def cell_class(tab, pressure, temperature):
    """'nan', 'clamped' (the nearest cell lies outside the index grid), 'empty' (inside, index value 0) or 'ordinary', per
    point -- from the point and the index array alone."""
    ip, jt = raw_cell(tab, pressure, temperature)
    out = np.full(ip.shape, 'ordinary', dtype=object)
    nan = np.isnan(ip) | np.isnan(jt)
    with np.errstate(invalid='ignore'):
        clamped = ~nan & ((ip < 0) | (ip > tab.n_p - 1) | (jt < 0) | (jt > tab.n_t - 1))
    inside = ~nan & ~clamped
    cell = np.zeros(ip.shape, dtype=np.int64)
    cell[inside] = tab.index[ip[inside].astype(np.int64), jt[inside].astype(np.int64)]
    out[inside & (cell == 0)] = 'empty'
    out[clamped] = 'clamped'
    out[nan] = 'nan'
    return out


def near_cell_boundary(tab, pressure, temperature, tol=1e-6):
    """Points within `tol` (hPa, K) of the boundary between two cells: there, and only there, a last-bit difference in the LCL
    may select another adiabat.  From the oracle's LCL alone; NaN points are not near anything."""
    p, t = np.asarray(pressure, dtype=np.float64), np.asarray(temperature, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        fi, fj = (tab.p_max - p) / tab.p_step, (t - tab.t_min) / tab.t_step
        dp = np.abs(fi - np.floor(fi) - 0.5) * tab.p_step
        dt = np.abs(fj - np.floor(fj) - 0.5) * tab.t_step
        # (outside the index grid every point is clamped onto the edge row / column: no boundary there)
        in_p = (fi >= 0.25) & (fi <= tab.n_p - 1.25)
        in_t = (fj >= 0.25) & (fj <= tab.n_t - 1.25)
        return ((dp <= tol) & in_p) | ((dt <= tol) & in_t)


def _step(x, dtype, up):
    x = np.asarray(x, dtype=dtype)
    return np.nextafter(x, np.asarray(np.inf if up else -np.inf, dtype=dtype))


START_CLASSES = ('p_tie', 'p_tie_minus', 'p_tie_plus', 't_tie', 't_tie_minus', 't_tie_plus', 'node', 'p_above_max',
                 'p_below_min', 't_below_min', 't_above_max', 'filled_edge', 'empty_first', 'nan_p', 'nan_t', 'nan_both')
SINGLE_POINT_CLASSES = ('nan_p', 'nan_t', 'nan_both')
N_PER_CLASS = 24


def start_cells(dtype=np.float64, tab=None):
    """Reference points (p_ref, T_ref) of moist_lapse.  Returns {'pressure', 'temperature'} in `dtype`, 'kind' (index into
    START_CLASSES) and, for the tie classes, 'cells': the two cells (ip, jt) a tie lies between, (-1, -1) elsewhere.

    p_tie: k * 0.5 + 0.25 hPa, exactly halfway between two index pressures in either dtype; both neighbours filled, with
    different adiabats.  t_tie (float64): 173 + (j + 0.5) * 0.02 as float64 arithmetic yields it, for those j at which
    (T - 173) / 0.02 then has the fraction 0.5 exactly -- the computed tie, which is what the rule decides; float32 holds
    no such value, there the class is the float32 nearest to the tie.  The _minus / _plus classes are one ulp (of `dtype`)
    to either side."""
    tab = tab or full_tables()
    dtype = np.dtype(dtype).type
    n = N_PER_CLASS
    ps, ts, kinds, cells = [], [], [], []

    def add(name, p, t, cell=None):
        p, t = np.broadcast_arrays(np.asarray(p, dtype=dtype), np.asarray(t, dtype=dtype))
        ps.append(p.ravel()); ts.append(t.ravel())
        kinds.append(np.full(p.size, START_CLASSES.index(name)))
        cells.append(np.full((p.size, 2), -1, dtype=np.int64) if cell is None else np.asarray(cell, dtype=np.int64).reshape(p.size, 2))

    # pressure ties: between rows ip and ip + 1, at a temperature node both of whose cells are filled
    # (rows at 590 hPa and more: there p_max - p is exact, so that one ulp of p is one ulp of the quotient the rule looks
    # at; below 550 hPa the subtraction rounds, and a pressure one ulp off a tie IS the tie to kernel and oracle alike)
    ip = 100 + 40 * np.arange(n)                                            # 1050 ... 590 hPa
    jt = 1500 + 97 * np.arange(n)                                           # 203 ... 247.6 K
    p_tie = tab.p_max - (ip + 0.5) * tab.p_step
    a, b = tab.index[ip, jt], tab.index[ip + 1, jt]
    assert np.all(a > 0) and np.all(b > 0) and np.all(a != b), 'pressure ties need two different adiabats around them'
    assert np.array_equal(p_tie.astype(np.float32).astype(np.float64), p_tie)
    tn = node_temperature(tab, jt)
    add('p_tie', p_tie, tn, np.stack([ip, jt], axis=1))
    add('p_tie_minus', _step(p_tie, dtype, False), tn, np.stack([ip, jt], axis=1))
    add('p_tie_plus', _step(p_tie, dtype, True), tn, np.stack([ip, jt], axis=1))
    # temperature ties: between columns j and j + 1, on a pressure node
    j_all = np.arange(1000, 6000)
    t_all = tab.t_min + (j_all + 0.5) * tab.t_step
    if dtype == np.float64:
        f = (t_all - tab.t_min) / tab.t_step
        j_all, t_all = j_all[f - np.floor(f) == 0.5], t_all[f - np.floor(f) == 0.5]
    pick = np.linspace(0, j_all.size - 1, n).astype(np.int64)
    jt, t_tie = j_all[pick], t_all[pick]
    ip = np.array([int(np.nonzero((tab.index[:, j] > 0) & (tab.index[:, j + 1] > 0) & (tab.index[:, j] != tab.index[:, j + 1]))[0][k * 7 % 40])
                   for k, j in enumerate(jt)])
    pn = node_pressure(tab, ip)
    add('t_tie', pn, t_tie, np.stack([ip, jt], axis=1))
    add('t_tie_minus', pn, _step(np.asarray(t_tie, dtype=dtype), dtype, False), np.stack([ip, jt], axis=1))
    add('t_tie_plus', pn, _step(np.asarray(t_tie, dtype=dtype), dtype, True), np.stack([ip, jt], axis=1))
    # both on a node
    ip, jt = 40 + 61 * np.arange(n), 900 + 131 * np.arange(n)
    ok = tab.index[ip, jt] > 0
    assert ok.sum() >= 20
    add('node', node_pressure(tab, ip), node_temperature(tab, jt))
    # outside the index grid: clamped onto its edge
    k = np.arange(n)
    add('p_above_max', np.where(k % 3 == 0, 1100.25, np.where(k % 3 == 1, 1104.0, 1150.0)), 250.0 + 2.5 * k)
    add('p_below_min', np.where(k % 3 == 0, 2.25, np.where(k % 3 == 1, 2.0, 1.0)), 173.0 + 0.5 * k)
    add('t_below_min', 1100.0 - 40.0 * k, np.where(k % 3 == 0, 172.98, np.where(k % 3 == 1, 172.0, 150.0)))
    add('t_above_max', np.where(k < 12, 1100.0 - 0.5 * k, 1090.0 - 20.0 * (k - 12)),
        np.array([315.99, 316.0, 317.5, 330.0])[k % 4])
    # the edge of the filled region, read from the index array: the last filled cell of a row and the empty one after it
    ip = 200 + 75 * np.arange(n)                                            # 1000 ... 137.5 hPa
    jl = np.array([int(np.nonzero(tab.index[i])[0][-1]) for i in ip])
    assert np.all(jl + 1 < tab.n_t) and np.all(tab.index[ip, jl + 1] == 0)
    add('filled_edge', node_pressure(tab, ip), node_temperature(tab, jl))
    add('empty_first', node_pressure(tab, ip), node_temperature(tab, jl + 1))
    add('nan_p', np.nan, 280.0)
    add('nan_t', 900.0, np.nan)
    add('nan_both', np.nan, np.nan)
    return {'pressure': np.concatenate(ps), 'temperature': np.concatenate(ts), 'kind': np.concatenate(kinds),
            'cells': np.concatenate(cells)}


def tie_winner(tab, cells_of, kind):
    """The cell pandas' rules give the start cells of the six tie classes, from the class alone: a pressure tie, and a
    pressure one ulp above it, go to the higher pressure (row ip), one ulp below it to row ip + 1; a temperature tie, and one
    ulp above it, go to the higher temperature (column jt + 1), one ulp below it to column jt."""
    name = START_CLASSES[kind]
    ip, jt = cells_of
    return {'p_tie': (ip, jt), 'p_tie_plus': (ip, jt), 'p_tie_minus': (ip + 1, jt),
            't_tie': (ip, jt + 1), 't_tie_plus': (ip, jt + 1), 't_tie_minus': (ip, jt)}[name]


EVAL_LENGTHS = (1, 2, 24)


def eval_pressures(dtype=np.float64):
    """{nlev: (nlev, n_variants) level columns in `dtype`}: a level exactly on a table pressure, exactly 2.5 and 1100.0,
    nextafter just outside each, 2.0, 1.0 and 1104 hPa and a NaN level among ordinary ones.  Pressure decreases upwards."""
    dtype = np.dtype(dtype).type
    lo, hi = dtype(2.5), dtype(1100.0)
    below, above = np.nextafter(hi, dtype(np.inf)), np.nextafter(lo, dtype(-np.inf))
    col = [1104.0, below, hi, np.nextafter(hi, dtype(0)), 1099.75, 1000.0, 987.3, 850.17, 700.25, 612.5, 500.0, np.nan, 300.1,
           100.0, 50.3, 10.0, 5.1, 3.0, 2.75, np.nextafter(lo, dtype(np.inf)), lo, above, 2.0, 1.0]
    assert len(col) == 24
    pairs = [(1104.0, hi), (below, 1000.0), (lo, above), (np.nan, 500.0), (700.5, 2.0), (900.0, 1.0), (hi, lo), (850.0, np.nan),
             (1099.9, 2.6)]
    singles = [1104.0, below, hi, 1000.0, 700.25, np.nan, lo, above, 2.0, 1.0, 431.7]
    return {24: np.asarray(col, dtype=dtype).reshape(24, 1), 2: np.asarray(pairs, dtype=dtype).T.copy(),
            1: np.asarray(singles, dtype=dtype).reshape(1, -1)}


def cross(cells, levels):
    """start_cells x the variants of one eval_pressures entry: (pressure (nlev, n), T_ref (n,), p_ref (n,), cell number (n,))
    with n = cells x variants."""
    nc, nv = cells['pressure'].size, levels.shape[1]
    p = np.ascontiguousarray(np.tile(levels, (1, nc)))                       # variant fastest
    which = np.repeat(np.arange(nc), nv)
    return p, np.ascontiguousarray(cells['temperature'][which]), np.ascontiguousarray(cells['pressure'][which]), which


def table_lapse(tab, pressure, t_ref, p_ref):
    """oracle.tables.moist_lapse_table column by column on float64 copies of the inputs."""
    from oracle import tables as tb
    p = np.asarray(pressure, dtype=np.float64)
    t0, p0 = np.asarray(t_ref, dtype=np.float64), np.asarray(p_ref, dtype=np.float64)
    return np.stack([tb.moist_lapse_table(tab, p[:, c], float(t0[c]), float(p0[c])) for c in range(p.shape[1])], axis=1)


# ---- soundings from below the table's bottom to above its top ---------------------------------------------------------
TALL_PARCELS = ('unsaturated', 'empty', 'clamped', 'below_surface')
TALL_CLASSES = ('ordinary', 'empty', 'clamped')
TALL_SEED = 7


def tall_columns(nlev=NLEV, ncol=NCOL, seed=TALL_SEED, tab=None):
    """Soundings from 1100.5 ... 1104 hPa at the surface to 1 hPa at the top: smooth temperature (isothermal at 205 K aloft),
    dewpoint depression >= 0.5 K everywhere, the three highest levels at 5, 2 and 1 hPa (the last two above the table's
    2.5 hPa).  'parcel': one explicit parcel per column, by TALL_PARCELS[c % 4]:
      unsaturated    700 ... 1000 hPa, 0.5 ... 5.5 K depression: an LCL wherever it falls
      empty          saturated, on a node, 0.5 ... 2.5 K beyond the last filled cell of its row
      clamped        saturated: at the surface (> 1100 hPa); at 1090 hPa and 317.5 K; at 30 hPa and 172 K; at 2 hPa
      below_surface  5 hPa below the surface, 2 ... 10 K depression
    The class a test counts is read from the oracle's LCL (cell_class), not from this label."""
    assert nlev >= 8
    tab = tab or full_tables()
    u = synth.column_uniforms(ncol, seed)
    c = np.arange(ncol)
    p_sfc = np.round((1100.5 + 3.5 * u[0]) * 64.0) / 64.0
    p_sfc[::5] = 1104.0
    m = nlev - 3
    sigma = 1.0 - (np.arange(m, dtype=np.float64)[:, None] / float(m - 1)) ** 1.3
    p = np.concatenate([20.0 + (p_sfc - 20.0) * sigma, np.repeat(np.array([[5.0], [2.0], [1.0]]), ncol, axis=1)], axis=0)
    t_sfc = 280.0 + 20.0 * u[1]
    gamma = (5.5 + 3.0 * u[2]) * 1e-3
    t = np.maximum(t_sfc * (p / p_sfc) ** (synth.RD_OVER_G * gamma), 205.0)
    dd_sfc = 0.5 + 12.0 * u[6]
    td = t - (dd_sfc + (30.0 - dd_sfc) * np.log(p_sfc / p) / np.log(p_sfc / 1.0))
    kind = c % len(TALL_PARCELS)
    pp = 1000.0 - 300.0 * u[3]
    pt = 265.0 + 25.0 * u[4]
    ptd = pt - (0.5 + 5.0 * u[5])
    e = kind == 1
    ip = (400 + (u[3] * 1000).astype(np.int64))                              # 900 ... 400 hPa
    jl = np.array([int(np.nonzero(tab.index[i])[0][-1]) for i in ip])
    je = np.minimum(jl + 25 + (100 * u[4]).astype(np.int64), tab.n_t - 3)
    assert np.all(tab.index[ip[e], je[e]] == 0)
    pp[e], pt[e] = node_pressure(tab, ip)[e], node_temperature(tab, je)[e]
    ptd[e] = pt[e]
    sub = (c // len(TALL_PARCELS)) % 4
    for s, (a, b) in enumerate(((None, None), (1090.0, 317.5), (30.0, 172.0), (2.0, 200.0))):
        sel = (kind == 2) & (sub == s)
        pp[sel] = p_sfc[sel] if a is None else a
        pt[sel] = t[0, sel] + 1.0 if b is None else b
        ptd[sel] = pt[sel]
    b = kind == 3
    pp[b], pt[b] = p_sfc[b] + 5.0, t[0, b] + 1.0
    ptd[b] = pt[b] - (2.0 + 8.0 * u[5][b])
    return {'pressure': p, 'temperature': t, 'dewpoint': td, 'parcel': (pp, pt, ptd), 'parcel_kind': kind}


def cast3(x, dtype):
    """The arrays of `x` rounded to `dtype`, and the same values as float64."""
    g = tuple(np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(dtype)) for v in x)
    return g, tuple(v.astype(np.float64) for v in g)


# ---- a table of another geometry --------------------------------------------------------------------------------------
SMALL_N_P, SMALL_N_T, SMALL_N_ADIABAT = 23, 31, 12
SMALL_GEOMETRY = dict(p_max=1000.0, p_step=40.0, t_min=200.0, t_step=3.5)        # 1000 ... 120 hPa, 200 ... 305 K


def small_coefficients():
    """T_a(p) = A_a + B_a p: B multiples of 1/256 K/hPa and A of 1/32 K, so every table entry (p a multiple of 40 hPa) is a
    multiple of 1/32 K below 512 K: exact in float32."""
    a = np.arange(SMALL_N_ADIABAT, dtype=np.float64)
    b = 0.03125 + a / 256.0
    t1000 = 240.0 + 6.0 * a
    return t1000 - 1000.0 * b, b


def small_table():
    """An oracle.tables.Tables of 23 pressures x 31 temperatures and a dozen straight 'adiabats'; a cell holds the adiabat
    that passes nearest to it, 0 where none comes within 6 K and in a sprinkled tenth of the others."""
    from oracle import tables as tb
    g = SMALL_GEOMETRY
    A, B = small_coefficients()
    p_desc = g['p_max'] - g['p_step'] * np.arange(SMALL_N_P)
    t_node = g['t_min'] + g['t_step'] * np.arange(SMALL_N_T)
    curves = A[:, None] + B[:, None] * p_desc[None, :]                        # [adiabat][p descending]
    d = np.abs(curves.T[:, None, :] - t_node[None, :, None])                # [p][t][adiabat]
    index = (1 + np.argmin(d, axis=2)).astype(np.uint16)
    ipg, jtg = np.meshgrid(np.arange(SMALL_N_P), np.arange(SMALL_N_T), indexing='ij')
    index[(d.min(axis=2) > 6.0) | ((ipg * 5 + jtg * 3) % 11 == 0)] = 0
    adiabats = np.ascontiguousarray(curves[:, ::-1].astype(np.float32))     # ascending pressure
    assert np.array_equal(adiabats.astype(np.float64), curves[:, ::-1])
    return tb.Tables(index=np.ascontiguousarray(index), adiabats=adiabats, **g)


def small_closed_form(tab, pressure, t_ref, p_ref):
    """What table mode must return on small_table(), written down without either oracle: the nearest cell (ties: higher
    pressure, higher temperature; clamped), its adiabat's A + B p inside 120 ... 1000 hPa, NaN outside, for an empty cell and
    for NaN input.  pressure (nlev, n); t_ref, p_ref (n,)."""
    g = SMALL_GEOMETRY
    A, B = small_coefficients()
    p = np.asarray(pressure, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    p_min = g['p_max'] - (SMALL_N_P - 1) * g['p_step']
    for c in range(p.shape[1]):
        p0, t0 = float(p_ref[c]), float(t_ref[c])
        if np.isnan(p0) or np.isnan(t0):
            continue
        fi, fj = (g['p_max'] - p0) / g['p_step'], (t0 - g['t_min']) / g['t_step']
        ip = int(np.ceil(fi - 0.5))                                          # a tie goes DOWN in row number: higher pressure
        jt = int(np.floor(fj + 0.5))                                         # a tie goes UP in column number: higher temperature
        ip, jt = min(max(ip, 0), SMALL_N_P - 1), min(max(jt, 0), SMALL_N_T - 1)
        a = int(tab.index[ip, jt])
        if a == 0:
            continue
        with np.errstate(invalid='ignore'):
            ok = (p[:, c] >= p_min) & (p[:, c] <= g['p_max'])
        out[ok, c] = A[a - 1] + B[a - 1] * p[ok, c]
    return out


def small_cases(dtype=np.float64):
    """Start points and level columns for small_table(): nodes, both kinds of tie, points outside every edge, NaN; levels on
    nodes, between them, on and just outside 120 and 1000 hPa."""
    dtype = np.dtype(dtype).type
    g = SMALL_GEOMETRY
    # (100 hPa is the tie between the last row and the first one past it; 60 and 20 hPa lie one and two rows past the last,
    # whose cells at 207 ... 245.5 K are filled: a start that is not clamped there reads behind the index array)
    p0 = [1000.0, 980.0, 979.0, 981.0, 960.0, 500.0, 140.0, 120.0, 100.0, 60.0, 20.0, 1020.0, 1021.0, 1100.0, 700.0, 620.0, np.nan, 400.0]
    t0 = [200.0, 201.75, 205.25, 206.0, 249.0, 250.75, 254.25, 265.0, 280.0, 290.0, 303.25, 305.0, 306.75, 307.0, 320.0, 199.0, 190.0,
          np.nan, 271.3, 214.0, 221.0, 228.0, 242.0]
    pg, tg = np.meshgrid(np.asarray(p0, dtype=dtype), np.asarray(t0, dtype=dtype), indexing='ij')
    lo, hi = dtype(120.0), dtype(g['p_max'])
    lev = np.asarray([1104.0, np.nextafter(hi, dtype(np.inf)), hi, np.nextafter(hi, dtype(0)), 990.0, 960.0, 731.7, 500.0, np.nan, 160.0,
                      150.5, np.nextafter(lo, dtype(np.inf)), lo, np.nextafter(lo, dtype(0)), 100.0, 1.0], dtype=dtype)
    n = pg.size
    return np.ascontiguousarray(np.repeat(lev[:, None], n, axis=1)), np.ascontiguousarray(tg.ravel()), np.ascontiguousarray(pg.ravel())
