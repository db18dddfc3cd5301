"""The inputs of the XP_HUM_RELATIVE / XP_HUM_MIXING_RATIO tests, shared by the census on the CPU (tests/test_humidity_cpu.py)
and the device tests (tests/test_gpu_humidity.py).

The base grid is synth.columns(24, 1337, nan_fraction=0.05) -- 1337 columns: the suite's ragged width, no multiple of 64 --
with relative humidity rh = e_s(Td) / e_s(T) and mixing ratio w = eps e_s(Td) / (p - e_s(Td)) derived from its dewpoints in
float64 (tests/humidity_restatement.py), so that the conversion gives the dewpoints back.  Over it the CLASS COLUMNS are
written, each a copy of the grid's first NaN-free column with one thing changed (CLASSES: name -> column; all of them among
the first 63 columns, so every shape of SHAPES but 24x1 holds them):
    zero, negative, nan, inf       the moisture (rh and w alike) of every level is 0, -0.001, NaN, +inf: D is NaN
    rh_1.05, rh_1e-6               rh of every level: D above T; a very dry but valid value
    w_0.04                         w of every level: moister than anything in the grid
    t_nan                          T of levels 0 and 5 is NaN, the moisture valid: D NaN for rh, finite for w
    p_nan                          p of level 5 is NaN, the moisture valid: D finite for rh, NaN for w
The shapes are leading blocks base[:nlev, :ncol] of it: one row, one column, and widths around the wavefront (63, 64, 65) and
beyond a block (257), each crossing the 16-byte run and the wavefront edge one way or another; 64 is the width whose rows
keep a 16-byte pitch in both dtypes."""
import functools

import numpy as np

from tests import humidity_restatement as R
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import synth

SEED = 20250718
NLEV, NCOL = 24, 1337
MAIN = '24x1337'
SHAPES = {MAIN: (24, 1337), '1x1337': (1, 1337), '24x1': (24, 1), '24x63': (24, 63), '24x64': (24, 64), '24x65': (24, 65),
          '24x257': (24, 257)}
CLASSES = {name: 2 + 5 * i for i, name in enumerate(('zero', 'negative', 'nan', 'inf', 'rh_1.05', 'rh_1e-6', 'w_0.04', 't_nan', 'p_nan'))}
MOISTURE_VALUE = {'zero': 0.0, 'negative': -0.001, 'nan': np.nan, 'inf': np.inf}
T_NAN_LEVELS, P_NAN_LEVELS = (0, 5), (5,)


@functools.lru_cache(maxsize=None)
def source():
    """(p, T, Td) of synth.columns before anything is written over it, float64."""
    return synth.columns(NLEV, NCOL, seed=SEED, nan_fraction=0.05)


@functools.lru_cache(maxsize=None)
def base():
    """{'pressure', 'temperature', 'relative', 'mixing_ratio'}: the base grid with its class columns, float64, read-only."""
    p, t, td = (a.copy() for a in source())
    clean = int(np.argmax(~(np.isnan(p) | np.isnan(t) | np.isnan(td)).any(axis=0)))
    assert clean not in CLASSES.values()
    for c in CLASSES.values():
        p[:, c], t[:, c], td[:, c] = p[:, clean], t[:, clean], td[:, clean]
    rh, w = R.relative_humidity(t, td), R.mixing_ratio(p, td)
    for name, v in MOISTURE_VALUE.items():
        rh[:, CLASSES[name]] = w[:, CLASSES[name]] = v
    rh[:, CLASSES['rh_1.05']] = 1.05
    rh[:, CLASSES['rh_1e-6']] = 1e-6
    w[:, CLASSES['w_0.04']] = 0.04
    t[list(T_NAN_LEVELS), CLASSES['t_nan']] = np.nan
    p[list(P_NAN_LEVELS), CLASSES['p_nan']] = np.nan
    out = {'pressure': p, 'temperature': t, R.RELATIVE: rh, R.MIXING_RATIO: w}
    for a in out.values():
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def grid(name, kind, dtype):
    """(p, T, m) of shape SHAPES[name] with the moisture of `kind`, contiguous in `dtype`, read-only."""
    nlev, ncol = SHAPES[name]
    b = base()
    out = tuple(np.ascontiguousarray(b[k][:nlev, :ncol], dtype=dtype) for k in ('pressure', 'temperature', kind))
    for a in out:
        a.flags.writeable = False
    return out


def isobars(nlev=NLEV):
    """nlev pressures shared by all columns (exact in float32)."""
    return np.round(np.linspace(1000.0, 100.0, nlev)).astype(np.float64)


def device_layouts(p, t, m, cuda):
    """The strided device views of the raw-ABI tests for the dense (nlev, ncol) arrays p, T, m: name -> (views of p, T, m; the
    dense arrays the call is equivalent to; the tensor that holds the moisture, whose bytes a call must leave alone).
    `cuda`: array -> device tensor.
      column_major         (ncol, nlev)-major storage: lev_stride 1, col_stride nlev
      every_second_column  the data in the even columns of arrays twice as wide (777 in the odd ones)
      shared_isobars       the pressure is nlev isobars behind col_stride == 0 (T and m dense)
      offset_base          dense, the base pointer one element into its allocation: the layout the 16-byte path must refuse"""
    nlev, ncol = p.shape
    dt = p.dtype
    xdt = L.XP_F64 if dt == np.float64 else L.XP_F32
    view = lambda ptr, ls, cs: L.View(ptr, xdt, L.XP_MEM_DEVICE, nlev, ncol, ls, cs)
    out = {}
    tr = [cuda(np.ascontiguousarray(a.T)) for a in (p, t, m)]
    out['column_major'] = ([view(x.data_ptr(), 1, nlev) for x in tr], (p, t, m), tr[2], tr)
    wide = []
    for a in (p, t, m):
        w = np.full((nlev, 2 * ncol), 777.0, dtype=dt)
        w[:, ::2] = a
        wide.append(cuda(w))
    out['every_second_column'] = ([view(x.data_ptr(), 2 * ncol, 2) for x in wide], (p, t, m), wide[2], wide)
    p1 = isobars(nlev).astype(dt)
    dense = [cuda(np.array(a)) for a in (p1, t, m)]
    pfull = np.ascontiguousarray(np.broadcast_to(p1[:, None], (nlev, ncol)))
    out['shared_isobars'] = ([view(dense[0].data_ptr(), 1, 0), view(dense[1].data_ptr(), ncol, 1), view(dense[2].data_ptr(), ncol, 1)],
                             (pfull, t, m), dense[2], dense)
    off = [cuda(np.concatenate([np.full(1, 777.0, dtype=dt), a.reshape(-1)])) for a in (p, t, m)]
    out['offset_base'] = ([view(x.data_ptr() + dt.itemsize, ncol, 1) for x in off], (p, t, m), off[2], off)
    return out
