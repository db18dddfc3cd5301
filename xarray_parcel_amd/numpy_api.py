"""
Array-level host API over libxparcel: the reference's function names
(modules/parcel_functions.py, "pf.py") on plain arrays.

Inputs are NumPy arrays or torch CPU tensors (host memory, staged through the library)
or torch CUDA tensors (used in place, on torch's current stream), laid out (nlev, ...) with the
vertical first: (nlev,), (nlev, ncol) or (nlev, ny, nx).  Per-column results come
back with the horizontal shape of the input; profiles as (nlev+1, ...).  Returned
containers are plain dicts -- the xarray-facing mirrors in parcel_functions.py
wrap them into Datasets.

With CUDA tensors for every array argument a function only enqueues work on torch's current stream and returns
without waiting for it (tests/test_gpu_streams.py); from_most_unstable_parcel and mix_layer, whose output shape
comes back from the device, are the exception; a Python scalar given for a per-column argument is uploaded
with a blocking copy; and a call that takes internal scratch (moist='family') straight after another one can wait
in the HIP runtime's hipFreeAsync while the stream is still busy, as conv_properties_composed's second parcel does.

There is no CPU path here: every function ends in a kernel launch.
"""
import ctypes as C
import functools
import math

import numpy as np

from . import _lib as L

L_EPS = 0.6219569100577033        # Mw / Md (metpy.constants, 1.4.1)

try:  # torch is plumbing (device memory, streams); the API also works without it on host arrays
    import torch
    _TORCH_DTYPE = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}
except Exception:  # pragma: no cover
    torch = None


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _ptr(a):
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


class _Call:
    """One library call being assembled from its array inputs, which decide, once:
    - dtype: float64 if any torch input is float64 or any other input is not float32, float32 otherwise;
    - memory space: the device if and only if some input is a CUDA tensor -- NumPy arrays, scalars and CPU tensors are then
      uploaded to that tensor's device; otherwise every input, CPU tensors included, is staged as host memory.  Outputs
      live in the same space;
    - device and stream: the library runs on that device, on torch's current stream of that device (not of torch's
      current device); host calls use the NULL stream.
    `ins` holds the inputs in that dtype and space; an absent input (None) is left out (views() puts it back).  Every array
    the call stages is kept alive as long as the call."""

    def __init__(self, *xs):
        xs = [x for x in xs if x is not None]
        devs = [x.device for x in xs if _is_torch(x) and x.is_cuda]
        assert all(d == devs[0] for d in devs), 'all device tensors of one call must live on the same GPU'
        self.device = devs[0] if devs else None
        f64 = any(x.dtype == torch.float64 if _is_torch(x) else np.asarray(x).dtype != np.float32 for x in xs)
        self.dtype = np.float64 if f64 else np.float32
        self.xp_dtype = L.XP_F64 if f64 else L.XP_F32
        self.mem = L.XP_MEM_HOST if self.device is None else L.XP_MEM_DEVICE
        self._keep = []
        self.ins = [self.array(x) for x in xs]
        # the grid: the first input, (nlev, ...) with `hshape` the horizontal shape of its ncol columns
        shape = tuple(self.ins[0].shape)
        self.nlev, self.hshape = (shape[0], shape[1:]) if shape else (1, ())
        self.ncol = math.prod(self.hshape)

    def array(self, x, dtype=None):
        """x as a contiguous array of `dtype` (default: the call's) in the call's memory space."""
        dtype = dtype or self.dtype
        if self.device is None:
            a = x.detach().to('cpu', _TORCH_DTYPE[dtype]).numpy() if _is_torch(x) else x
            a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        else:
            a = x if _is_torch(x) else torch.as_tensor(np.asarray(x, dtype=dtype))
            a = a.to(self.device, _TORCH_DTYPE[dtype]).contiguous()
        self._keep.append(a)
        return a

    def per_col(self, x, n=None, msg='per-column argument does not match the grid'):
        """Per-column argument (a scalar, broadcast, or one value per column of the grid) -> n elements (default: ncol)."""
        n = self.ncol if n is None else n
        if not _is_torch(x):
            x = np.asarray(x, dtype=self.dtype).reshape(-1)
            if x.size == 1 and n != 1:
                x = np.full(n, x[0], dtype=self.dtype)
        a = self.array(x).reshape(-1)
        assert int(np.prod(a.shape)) == n, msg
        return a

    def mask(self, m, shape):
        """bool / integer mask -> dense uint8 of `shape`."""
        return self.array(((m != 0) if _is_torch(m) else (np.asarray(m) != 0)).reshape(shape), np.uint8)

    def view(self, a, nlev=None, ncol=None):
        """xp_view of a staged array, (nlev, ...) as (nlev, ncol) unless given."""
        nlev = a.shape[0] if nlev is None else nlev
        ncol = math.prod(a.shape[1:]) if ncol is None else ncol
        return L.View(_ptr(a), self.xp_dtype, self.mem, nlev, ncol, ncol, 1)

    def views(self, given):
        """The xp_views of the call's leading inputs, laid out as the arguments `given` they were: None where one is absent."""
        ins = iter(self.ins)
        return [None if x is None else self.view(next(ins)) for x in given]

    def out(self, shape, dtype=None):
        dtype = dtype or self.dtype
        if self.device is None:
            return np.empty(shape, dtype=dtype)
        return torch.empty(shape, dtype=_TORCH_DTYPE[dtype], device=self.device)

    def struct(self, out_type, per_col=(), layered=(), n=0, per_level=(), nlev=None):
        """An output struct of `out_type` and the outputs it points at, as (struct, dict name -> array), allocated in this
        order: for each name in `layered` an (n, ...) array, its field holding one pointer per layer; in `per_col` one value
        per column (int32 for the names in L.INT32_OUT, the call's dtype otherwise); in `per_level` an (nlev, ...) array
        (nlev: the grid's unless given).  dtype and mem are set where the struct has them."""
        out = out_type(dtype=self.xp_dtype, mem=self.mem) if hasattr(out_type, 'dtype') else out_type()
        res = {}
        for k in layered:
            a = res[k] = self.out((n,) + self.hshape)
            rows = getattr(out, k)
            for i in range(n):
                rows[i] = _ptr(a[i:i + 1])               # (a[i] of a grid without horizontal dims is no array)
        for k in per_col:
            a = res[k] = self.out(self.hshape, np.int32 if k in L.INT32_OUT else None)
            setattr(out, k, _ptr(a))
        if per_level:
            shape = (self.nlev if nlev is None else nlev,) + self.hshape
            for k in per_level:
                a = res[k] = self.out(shape)
                setattr(out, k, _ptr(a))
        return out, res

    def scalars(self, names, shape):
        """xp_scalars_out with an output of `shape`, the grid's horizontal shape, for each of `names`."""
        assert shape == self.hshape
        return self.struct(L.ScalarsOut, names)

    def profile(self, names, nlev_out, shape, lifted_index_at=None):
        """xp_profile_out with an (nlev_out,) + shape output for each of `names` and, with lifted_index_at, the lifted index
        (one per column, under 'lifted_index')."""
        assert shape == self.hshape
        po, out = self.struct(L.ProfileOut, per_level=names, nlev=nlev_out)
        po.nlev_out, po.lev_stride, po.col_stride = nlev_out, self.ncol, 1
        if lifted_index_at is not None:
            out['lifted_index'] = self.out(shape)
            po.lifted_index, po.lifted_index_pressure = _ptr(out['lifted_index']), float(lifted_index_at)
        return po, out

    def run(self, name, *args):
        """Launch entry point `name` on the call's device and stream; arrays are passed as their addresses."""
        lib = L.init(None if self.device is None else self.device.index)
        stream = None if self.device is None else torch.cuda.current_stream(self.device).cuda_stream
        args = [_ptr(a) if isinstance(a, np.ndarray) or _is_torch(a) else a for a in args]
        L.check(getattr(lib, name)(*args, stream))


def _opts(virtual_temperature_correction=True, lcl_interp='log', pos_cape_neg_cin=True, post_zero_cin=False,
          moist='exact', humidity='dewpoint', compute='float64'):
    if lcl_interp not in L.LCL_INTERP:
        raise AssertionError('interpolator must be linear or log')          # pf.py:878
    assert humidity in L.HUMIDITY, "humidity must be 'dewpoint', 'specific', 'relative' or 'mixing_ratio'"
    assert compute in L.COMPUTE, "compute must be 'float64' or 'float32'"
    return L.Opts(int(bool(virtual_temperature_correction)), L.LCL_INTERP[lcl_interp], int(bool(pos_cape_neg_cin)),
                  int(bool(post_zero_cin)), L.MOIST[moist], L.COMPUTE[compute], L.HUMIDITY[humidity], 0)


def _layer_flags(positive_layer=None, which_lfc=None, which_el=None):
    """The XP_OPT_LAYER_* bits of xp_opts.flags (include/xparcel.h) for positive_layer= 'envelope' (the default: the
    reference's bottom LFC and top EL), 'lowest', 'highest', 'deepest' or 'most_cape', or for MetPy's pair which_lfc= /
    which_el= that names the same layer; any other pair, or both spellings at once, is a ValueError."""
    if which_lfc is None and which_el is None:
        name = 'envelope' if positive_layer is None else positive_layer
        if name not in L.POSITIVE_LAYER:
            raise ValueError('positive_layer must be one of %s, got %r' % (', '.join(map(repr, L.POSITIVE_LAYER)), positive_layer))
    else:
        pairs = ', '.join('(%r, %r) = %r' % (a, b, n) for (a, b), n in L.WHICH_LFC_EL.items())
        if positive_layer is not None:
            raise ValueError('give positive_layer= or the pair which_lfc= / which_el=, not both; the pairs are ' + pairs)
        if (which_lfc, which_el) not in L.WHICH_LFC_EL:
            raise ValueError('(which_lfc, which_el) = (%r, %r) names no positive layer; the pairs are %s' % (which_lfc, which_el, pairs))
        name = L.WHICH_LFC_EL[(which_lfc, which_el)]
    return L.POSITIVE_LAYER[name]


_DEFAULT = {'moist': 'exact', 'compute': 'float64'}

# what a compute='float32' call can return (include/xparcel.h at xp_opts.compute): everything but the LFC / EL temperatures,
# the interval indices and the status word
COMPUTE32_WANT = ('cape', 'cin', 'lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'lfc_pressure', 'el_pressure',
                  'parcel_index', 'parcel_pressure', 'parcel_temperature', 'parcel_dewpoint')


def set_compute(mode):
    """The arithmetic of the CAPE / CIN level walk: 'float64' (the default) or 'float32' (fp32 arithmetic above the LCL,
    same classification of every column, CAPE / CIN within 0.5 J/kg: include/xparcel.h at xp_opts.compute).  A preference:
    it applies to the calls the fp32 kernel covers -- cape_cin_columns on float32 arrays, surface parcel, moist='family',
    dewpoint input, default options, no profile, no lifted index, `want` within COMPUTE32_WANT (or None) -- and every
    other call runs in fp64 as before.  The keyword compute='float32' of a call is strict instead: it raises XParcelError
    where the kernel does not apply."""
    assert mode in L.COMPUTE
    _DEFAULT['compute'] = mode


def _compute32_applies(c, parcel, moist, want, want_profile, lifted_index_at, kwargs):
    return (c.xp_dtype == L.XP_F32 and parcel == 'surface' and moist == 'family' and not want_profile and
            lifted_index_at is None and (want is None or all(k in COMPUTE32_WANT for k in want)) and
            kwargs.get('humidity', 'dewpoint') == 'dewpoint' and bool(kwargs.get('virtual_temperature_correction', True)) and
            kwargs.get('lcl_interp', 'log') == 'log' and bool(kwargs.get('pos_cape_neg_cin', True)) and
            not kwargs.get('post_zero_cin', False))


def set_moist_lapse(mode):
    """'exact' (RK4 integration of MetPy's ODE), 'family' (the same ODE from the adiabat-family table, faster) or
    'table' (the reference's lookup tables; needs adiabat_tables.load_moist_adiabat_lookups())."""
    assert mode in L.MOIST
    _DEFAULT['moist'] = mode


def _same_shape(arrays, msg):
    """Assert, with the caller's message, that the arrays share the first one's shape."""
    shape = arrays[0].shape
    for a in arrays:
        assert a.shape == shape, msg


def _is_isobars(pressure, like):
    """Whether `pressure` holds just the nlev isobars of the (nlev, ...) grid of `like` (isobaric data)."""
    if len(np.shape(pressure)) != 1 or len(np.shape(like)) <= 1:
        return False
    assert np.shape(pressure)[0] == np.shape(like)[0], 'a 1-D pressure must have one value per level'
    return True


def _on_grid(pressure, like):
    """A 1-D pressure of nlev values (isobaric data) on the (nlev, ...) grid of `like`, in pressure's own space."""
    shape = tuple(like.shape)
    col = (-1,) + (1,) * (len(shape) - 1)
    if _is_torch(pressure):
        return pressure.reshape(col).expand(shape)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(pressure).reshape(col), shape))


def _full_pressure(pressure, like):
    """The pressure of isobaric data (_is_isobars) expanded onto the grid of `like`; any other pressure as it is."""
    return _on_grid(pressure, like) if _is_isobars(pressure, like) else pressure


def _sounding(pressure, temperature, dewpoint, ground=None):
    """The sounding of a CAPE-family call: its _Call, the xp_views of pressure, temperature and moisture, and the surface:
    None, or, for a ground= call (XP_PARCEL_OVER_GROUND, include/xparcel.h), the three per-column surface arrays.  The grid
    of a ground= call is temperature's; its pressure may be the nlev isobars, which are expanded on the host (_full_pressure), or,
    as a device tensor, passed as they are: a view whose col_stride is 0."""
    if ground is None:
        c = _Call(pressure, temperature, dewpoint)
        _same_shape(c.ins, 'pressure, temperature, dewpoint must share a shape')
        return c, tuple(map(c.view, c.ins)), None
    assert len(ground) == 3, 'ground: (surface_pressure, surface_temperature, surface_dewpoint)'
    isobars = _is_isobars(pressure, temperature) and _is_torch(pressure) and pressure.is_cuda
    if not isobars:
        pressure = _full_pressure(pressure, temperature)
    c = _Call(temperature, dewpoint, pressure, *[x for x in ground if _is_torch(x)])
    t, td, p = c.ins[:3]
    assert t.shape == td.shape and (isobars or p.shape == t.shape), 'pressure, temperature, dewpoint must share a shape'
    pv = c.view(t)
    pv.data = _ptr(p)
    if isobars:
        pv.lev_stride, pv.col_stride = 1, 0
    return c, (pv, c.view(t), c.view(td)), [c.per_col(x) for x in ground]


def _parcel(c, name, depth=None, parcel_values=None, surface=None):
    """The xp_parcel `name` of a call: `depth` [hPa] defaults to the reference's; an explicit parcel points at its
    (pressure, temperature, dewpoint) `parcel_values`, one per column, staged on `c`; with the `surface` arrays of a ground=
    call (_sounding) it carries XP_PARCEL_OVER_GROUND and points at those ('max_cape' does not combine with it)."""
    if depth is None:
        depth = 300.0 if name in ('most_unstable', 'max_cape') else 100.0  # pf.py:1558, 1652
    pc = L.Parcel(L.PARCEL[name], 0, float(depth), None, None, None)
    if name == 'explicit':
        pc.pressure, pc.temperature, pc.dewpoint = (_ptr(c.per_col(x)) for x in parcel_values)
    if surface is not None:
        assert name != 'explicit', 'ground: not with an explicit parcel'
        assert name != 'max_cape', 'ground: not with the max_cape parcel'
        pc.mode |= L.PARCEL_OVER_GROUND
        pc.pressure, pc.temperature, pc.dewpoint = (_ptr(x) for x in surface)
    return pc


def cape_cin_columns(pressure, temperature, dewpoint, parcel='surface', depth=None, parcel_values=None,
                     want_profile=False, want=None, moist=None, lifted_index_at=None, compute=None, ground=None,
                     positive_layer=None, which_lfc=None, which_el=None, **kwargs):
    """pf.py:1394-1475 with the three drivers.  Returns a dict of per-column arrays (and 'profile').
    want_profile: True for the six profile arrays of pf.py:806-931, or an iterable of their names for a subset (the ones
    not named are neither allocated nor written: lifted_index needs three of the six).
    lifted_index_at: a pressure [hPa] (the reference: 500): 'lifted_index' (pf.py:1722) of the lifted profile comes back
    with the scalars, computed in the same pass -- no profile array has to exist for it.
    humidity='specific' (keyword): `dewpoint` holds specific humidity [kg/kg] and is converted on load
    (parcel_test.py:262-266 fused into the pass).
    humidity='relative' / 'mixing_ratio' (XP_HUM_RELATIVE / XP_HUM_MIXING_RATIO, include/xparcel.h): `dewpoint` holds relative
    humidity over liquid water as a FRACTION (1 = saturated, not percent) or the water-vapour mixing ratio [kg/kg].  One
    streaming pass in front of the call turns it into a dewpoint (NaN unless the value is > 0), and every result is that of
    the dewpoint call on it.  They combine with every parcel (an explicit parcel's and ground='s surface dewpoint stay
    dewpoints), with ground= and with parcel='max_cape'; not with compute='float32'.
    compute='float32': the level walk above the LCL in fp32 arithmetic (float32 arrays, surface parcel, moist='family',
    default options, no profile; `want` then defaults to COMPUTE32_WANT); raises where that kernel does not apply.  None:
    the module default (set_compute), which falls back to fp64 where it does not.
    ground=(surface_pressure, surface_temperature, surface_dewpoint): pressure-level data (XP_PARCEL_OVER_GROUND,
    include/xparcel.h).  The arrays hold isobaric levels, `pressure` possibly just the nlev isobars, and each column is cut
    at its surface pressure: the surface values become level 0, the levels above the ground follow, NaN fills the rest.
    Every result is that of the call on those re-based columns: the indices count their rows, and the profile has
    nlev + 2 rows.  Not with an explicit parcel, nor with compute='float32'.
    parcel='max_cape' (XP_PARCEL_MAX_CAPE, include/xparcel.h): the departure level of the lowest `depth` hPa (default 300)
    whose parcel has the largest CAPE -- every level of the window is lifted.  The results are those of the surface call on
    the column from that level on, 'parcel_index' the level.  Not with ground=, humidity='specific' or compute='float32'
    (humidity='relative' and 'mixing_ratio' are fine).
    positive_layer='envelope' | 'lowest' | 'highest' | 'deepest' | 'most_cape' (XP_OPT_LAYER_*, include/xparcel.h): which
    positive layer of a sounding with several of them CAPE, CIN, the LFC and the EL describe.  'envelope', the default, is
    the reference's rule -- the bottom LFC and the top EL, every positive area between them added up; the others pick one
    LFC / EL pair: the lowest layer, the highest, the deepest in ln p, or the one with the most CAPE.  A column with at most
    one positive layer returns the default's numbers whatever the choice.  which_lfc= / which_el= take MetPy's spelling of
    the same five: ('bottom', 'top'), ('bottom', 'bottom'), ('top', 'top'), ('wide', 'wide'), ('most_cape', 'most_cape').
    Not with want_profile, lifted_index_at or compute='float32'; moist='family' runs as 'exact'."""
    layer = _layer_flags(positive_layer, which_lfc, which_el)
    c, views, surface = _sounding(pressure, temperature, dewpoint, ground)
    moist = moist or _DEFAULT['moist']
    if compute is None:
        compute = _DEFAULT['compute']
        if compute == 'float32' and not (ground is None and layer == 0 and
                                         _compute32_applies(c, parcel, moist, want, want_profile, lifted_index_at, kwargs)):
            compute = 'float64'
    if compute == 'float32' and want is None:
        want = COMPUTE32_WANT
    o = _opts(moist=moist, compute=compute, **kwargs)
    o.flags |= layer
    pc = _parcel(c, parcel, depth, parcel_values, surface)
    so, res = c.scalars(L.SCALAR_F + L.SCALAR_I + L.SCALAR_P if want is None else tuple(want), c.hshape)
    po = None
    if want_profile or lifted_index_at is not None:
        pvars = L.PROFILE_VARS if want_profile is True else tuple(want_profile or ())
        assert all(k in L.PROFILE_VARS for k in pvars), f'profile variables are {L.PROFILE_VARS}'
        po, prof = c.profile(pvars, c.nlev + (1 if ground is None else 2), c.hshape, lifted_index_at)
        if lifted_index_at is not None:
            res['lifted_index'] = prof.pop('lifted_index')
    c.run('xp_cape_cin', *views, pc, o, so, po)
    if want_profile:
        res['profile'] = prof
    return res


def cape_cin_multi(pressure, temperature, dewpoint, parcels, want=None, moist=None, lifted_index_at=None, fused=False,
                   ground=None, positive_layer=None, which_lfc=None, which_el=None, **kwargs):
    """Several parcels of one grid in ONE call (xp_cape_cin_multi): `parcels` is a sequence of names or (name, depth)
    pairs out of 'surface', 'most_unstable', 'mixed_layer', 'max_cape' -- e.g. [('most_unstable', 300), ('mixed_layer', 100)] for
    BASELINE config 5, [('most_unstable', 250), ('mixed_layer', 100), ('mixed_layer', 50)] for conv_properties
    (pf.py:1984-2006).  Returns one dict per parcel, bit-identical to what cape_cin_columns() returns for it.
    fused=True (XP_OPT_FUSE_PARCELS; moist='family', two parcels): one pass over the grid for both -- same numbers,
    measured slower than a pass per parcel on MI355X, hence opt-in.
    humidity (keyword): as in cape_cin_columns; 'relative' and 'mixing_ratio' are converted once for all the parcels.
    ground: as in cape_cin_columns; the grid is cut at the ground once for all the parcels.
    positive_layer / which_lfc, which_el: as in cape_cin_columns, one choice for all the parcels (then a pass per parcel,
    whatever `fused` says; not with lifted_index_at)."""
    layer = _layer_flags(positive_layer, which_lfc, which_el)
    c, views, surface = _sounding(pressure, temperature, dewpoint, ground)
    o = _opts(moist=moist or _DEFAULT['moist'], **kwargs)
    o.flags = (L.OPT_FUSE_PARCELS if fused else 0) | layer
    pcs = []
    for pc in parcels:
        name, depth = (pc, None) if isinstance(pc, str) else (pc[0], pc[1])
        assert name in ('surface', 'most_unstable', 'mixed_layer', 'max_cape'), 'parcels: surface, most_unstable or mixed_layer, or max_cape'
        pcs.append(_parcel(c, name, depth, surface=surface))
    n = len(pcs)
    pcs = (L.Parcel * n)(*pcs)
    names = L.SCALAR_F + L.SCALAR_I + L.SCALAR_P if want is None else tuple(want)
    sos = (L.ScalarsOut * n)()
    pos = (L.ProfileOut * n)() if lifted_index_at is not None else None
    outs = []
    for i in range(n):
        sos[i], out = c.scalars(names, c.hshape)
        if pos is not None:
            pos[i], li = c.profile((), c.nlev + (1 if ground is None else 2), c.hshape, lifted_index_at)
            out.update(li)
        outs.append(out)
    c.run('xp_cape_cin_multi', *views, n, pcs, o, sos, pos)
    return outs


# ---- reference-named functions (one column or a grid) -----------------------------------------
def _split(res):
    cc = {'cape': res['cape'], 'cin': res['cin']}
    prof = dict(res.get('profile', {}))
    for k in ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'lfc_pressure', 'lfc_temperature',
              'el_pressure', 'el_temperature', 'lfc_index', 'el_index', 'status'):
        prof[k] = res[k]
    return cc, prof


def cape_cin(pressure, temperature, dewpoint, parcel_temperature, parcel_pressure, parcel_dewpoint, **kwargs):
    """pf.py:1394."""
    return _split(cape_cin_columns(pressure, temperature, dewpoint, parcel='explicit',
                                   parcel_values=(parcel_pressure, parcel_temperature, parcel_dewpoint),
                                   want_profile=True, **kwargs))


def surface_based_cape_cin(pressure, temperature, dewpoint, **kwargs):
    """pf.py:1477.  It returns the profile, which the fp32 walk does not produce: compute='float32' always raises here, and
    a set_compute('float32') preference leaves it in fp64 (cape_cin_columns(parcel='surface') is the call that takes it)."""
    return _split(cape_cin_columns(pressure, temperature, dewpoint, parcel='surface', want_profile=True, **kwargs))


def most_unstable_cape_cin(pressure, temperature, dewpoint, depth=300, **kwargs):
    """pf.py:1557."""
    res = cape_cin_columns(pressure, temperature, dewpoint, parcel='most_unstable', depth=depth, want_profile=True,
                           **kwargs)
    cc, prof = _split(res)
    return cc, prof, {'pressure': res['parcel_pressure'], 'temperature': res['parcel_temperature'],
                      'dewpoint': res['parcel_dewpoint'], 'index': res['parcel_index']}


def max_cape_cape_cin(pressure, temperature, dewpoint, depth=300, **kwargs):
    """As most_unstable_cape_cin for the parcel with the largest CAPE of the lowest `depth` hPa (parcel='max_cape')."""
    res = cape_cin_columns(pressure, temperature, dewpoint, parcel='max_cape', depth=depth, want_profile=True, **kwargs)
    cc, prof = _split(res)
    return cc, prof, {'pressure': res['parcel_pressure'], 'temperature': res['parcel_temperature'],
                      'dewpoint': res['parcel_dewpoint'], 'index': res['parcel_index']}


def mixed_layer_cape_cin(pressure, temperature, dewpoint, depth=100, **kwargs):
    """pf.py:1651."""
    res = cape_cin_columns(pressure, temperature, dewpoint, parcel='mixed_layer', depth=depth, want_profile=True,
                           **kwargs)
    cc, prof = _split(res)
    return cc, prof, {'pressure': res['parcel_pressure'], 'temperature': res['parcel_temperature'],
                      'dewpoint': res['parcel_dewpoint']}


def parcel_profile_with_lcl(pressure, temperature, dewpoint, parcel_pressure, parcel_temperature, parcel_dewpoint,
                            lcl_interp='log', moist=None):
    """pf.py:806."""
    res = cape_cin_columns(pressure, temperature, dewpoint, parcel='explicit',
                           parcel_values=(parcel_pressure, parcel_temperature, parcel_dewpoint), want_profile=True,
                           lcl_interp=lcl_interp, moist=moist,
                           want=('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature'))
    out = dict(res['profile'])
    for k in ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature'):
        out[k] = res[k]
    return out


def _select(pressure, temperature, dewpoint, mode, depth, ground=None):
    c, views, surface = _sounding(pressure, temperature, dewpoint, ground)
    so, out = c.scalars(L.SCALAR_P + ('parcel_index',), c.hshape)
    c.run('xp_select_parcel', *views, _parcel(c, mode, depth, surface=surface), so)
    return {'pressure': out['parcel_pressure'], 'temperature': out['parcel_temperature'],
            'dewpoint': out['parcel_dewpoint'], 'index': out['parcel_index']}


def most_unstable_parcel(pressure, temperature, dewpoint, depth=300, ground=None):
    """pf.py:102.  ground: as in cape_cin_columns ('index' counts the rows of the column cut at the ground)."""
    return _select(pressure, temperature, dewpoint, 'most_unstable', depth, ground)


def max_cape_parcel(pressure, temperature, dewpoint, depth=300):
    """The departure level of the lowest `depth` hPa whose parcel has the largest CAPE (XP_PARCEL_MAX_CAPE, include/xparcel.h;
    default options, exact moist adiabat): what most_unstable_parcel returns."""
    return _select(pressure, temperature, dewpoint, 'max_cape', depth)


def mixed_parcel(pressure, temperature, dewpoint, depth=100, ground=None):
    """pf.py:229.  ground: as in cape_cin_columns."""
    r = _select(pressure, temperature, dewpoint, 'mixed_layer', depth, ground)
    r.pop('index')
    return r


def mixed_layer(dat, depth=100):
    """pf.py:137: dat = dict with 'pressure' and variables to mix."""
    out = {}
    for k, v in dat.items():
        if k == 'pressure':
            continue
        c = _Call(dat['pressure'], v)
        out[k] = c.out(c.hshape)
        c.run('xp_mixed_layer', *map(c.view, c.ins), float(depth), out[k])
    return out


def lcl(parcel_pressure, parcel_temperature, parcel_dewpoint):
    """pf.py:609."""
    c = _Call(*(x if _is_torch(x) else np.atleast_1d(np.asarray(x, dtype=np.float64))
                for x in (parcel_pressure, parcel_temperature, parcel_dewpoint)))
    p, t, td = c.ins
    shape = tuple(p.shape) if np.ndim(parcel_pressure) else ()
    outs = [c.out(shape) for _ in range(3)]
    c.run('xp_lcl', int(np.prod(p.shape)), c.xp_dtype, c.mem, p, t, td, *outs, c.out(shape, np.int32))
    return {'lcl_pressure': outs[0], 'lcl_temperature': outs[1], 'lcl_virtual_temperature': outs[2]}


def _lapse(fn_name, pressure, parcel_temperature, parcel_pressure, moist_mode=None):
    c = _Call(pressure)
    pp = c.per_col(parcel_pressure) if parcel_pressure is not None else None
    out = c.out(c.ins[0].shape)
    c.run(fn_name, c.view(c.ins[0]), c.per_col(parcel_temperature), pp, *(() if moist_mode is None else (moist_mode,)), out)
    return out


def dry_lapse(pressure, parcel_temperature, parcel_pressure=None):
    """pf.py:291."""
    return _lapse('xp_dry_lapse', pressure, parcel_temperature, parcel_pressure)


def moist_lapse(pressure, parcel_temperature, parcel_pressure=None, moist=None):
    """pf.py:525."""
    return _lapse('xp_moist_lapse', pressure, parcel_temperature, parcel_pressure,
                  moist_mode=L.MOIST[moist or _DEFAULT['moist']])


def parcel_profile(pressure, parcel_pressure, parcel_temperature, parcel_dewpoint, moist=None):
    """pf.py:712."""
    c = _Call(pressure)
    p = c.ins[0]
    pp, pt, ptd = (c.per_col(x) for x in (parcel_pressure, parcel_temperature, parcel_dewpoint))
    res = {'pressure': p, 'temperature': c.out(p.shape), 'virtual_temperature': c.out(p.shape),
           'lcl_pressure': c.out(c.hshape), 'lcl_temperature': c.out(c.hshape), 'lcl_virtual_temperature': c.out(c.hshape)}
    c.run('xp_parcel_profile', c.view(p), pp, pt, ptd, L.MOIST[moist or _DEFAULT['moist']], *list(res.values())[1:])
    return res


def lfc_el(pressure, parcel_temperature, temperature, lcl_pressure, lcl_temperature):
    """pf.py:1066."""
    c = _Call(pressure, parcel_temperature, temperature)
    so, out = c.scalars(('lfc_pressure', 'lfc_temperature', 'el_pressure', 'el_temperature', 'lfc_index', 'el_index',
                         'status'), c.hshape)
    c.run('xp_lfc_el', *map(c.view, c.ins), c.per_col(lcl_pressure), c.per_col(lcl_temperature), so)
    return out


def cape_cin_base(pressure, temperature, lfc_pressure, el_pressure, parcel_temperature, pos_cape_neg_cin=True,
                  post_zero_cin=False, **_ignored):
    """pf.py:1291."""
    c = _Call(pressure, temperature, parcel_temperature)
    o = _opts(pos_cape_neg_cin=pos_cape_neg_cin, post_zero_cin=post_zero_cin)
    res = {'cape': c.out(c.hshape), 'cin': c.out(c.hshape)}
    c.run('xp_cape_cin_base', *map(c.view, c.ins), c.per_col(lfc_pressure), c.per_col(el_pressure), o, res['cape'], res['cin'])
    return res


# ---- SURVEY 8(f) items that reuse the hot-path device code -------------------------------------------------
def wet_bulb_temperature(pressure, temperature, dewpoint, moist=None):
    """pf.py:389: Normand's rule, every element independently."""
    c = _Call(pressure, temperature, dewpoint)
    out = c.out(c.ins[0].shape)
    c.run('xp_wet_bulb_temperature', *map(c.view, c.ins), L.MOIST[moist or _DEFAULT['moist']], out)
    return out


def downdraft_cape(pressure, temperature, dewpoint, bottom=700.0, depth=200.0, moist=None, want_profile=False):
    """metpy.calc.downdraft_cape for every column (xp_downdraft_cape; the layer from `bottom` up `depth` hPa, MetPy's
    700 and 200).  Returns a dict of per-column 'dcape' [J/kg], 'start_pressure' (p0), 'start_temperature' (its wet bulb)
    and 'status' (ST_LCL_NOT_CONVERGED, XP_ST_NO_LAYER: the column does not span the layer, everything NaN); with
    want_profile also 'parcel_temperature', the descending parcel on the levels with p >= p0 (NaN elsewhere), shaped like
    the input."""
    c, views, _ = _sounding(pressure, temperature, dewpoint)
    out, res = c.struct(L.DcapeOut, L.DCAPE_OUT[:4], per_level=L.DCAPE_OUT[4:] if want_profile else ())
    c.run('xp_downdraft_cape', *views, float(bottom), float(depth), L.MOIST[moist or _DEFAULT['moist']], out)
    return res


def effective_inflow_layer(pressure, temperature, dewpoint, height=None, cape_min=100.0, cin_min=-250.0, search_depth=300.0,
                           moist=None, want_candidates=False, **cape_cin_options):
    """The effective inflow layer of Thompson et al. (2007) for every column (xp_effective_inflow_layer): the lowest
    contiguous run of levels whose parcels, each lifted as the surface parcel of the column cut off below it, have
    CAPE >= cape_min [J/kg] and CIN >= cin_min (CIN is <= 0 here).  Levels with a NaN in p, T or Td are skipped; the search
    covers the levels with p >= p_lowest - search_depth [hPa].  cape_cin_options: the CAPE / CIN options of
    cape_cin_columns (virtual_temperature_correction, lcl_interp, pos_cape_neg_cin, post_zero_cin, and humidity='relative' /
    'mixing_ratio' for what `dewpoint` holds -- not 'specific'); moist: 'exact' or 'table' ('family' runs as 'exact').
    Returns a dict of per-column 'base_pressure', 'top_pressure' [hPa],
    'base_height', 'top_height' [m above the lowest valid level: the bounds storm_relative_helicity_layers takes; NaN
    without `height`], 'base_index', 'top_index' (level indices, -1 = none) and 'status' (XP_ST_NO_LAYER: no level
    passes; ST_LAYER_OPEN: the window cut the layer; ST_LCL_NOT_CONVERGED, ST_BAD_PRESSURE); with want_candidates also
    'candidate_cape', 'candidate_cin', shaped like the input: what was computed for every level that was lifted, NaN
    elsewhere."""
    assert cape_cin_options.get('humidity') != 'specific', 'effective_inflow_layer does not take specific humidity'
    c = _Call(pressure, temperature, dewpoint, height)
    _same_shape(c.ins, 'pressure, temperature, dewpoint, height must share a shape')
    o = _opts(moist=moist or _DEFAULT['moist'], **cape_cin_options)
    out, res = c.struct(L.EffectiveLayerOut, L.EFFECTIVE_F + L.EFFECTIVE_I,
                        per_level=L.EFFECTIVE_CANDIDATES if want_candidates else ())
    c.run('xp_effective_inflow_layer', *c.views((pressure, temperature, dewpoint, height)), float(cape_min), float(cin_min),
          float(search_depth), o, out)
    return res


_LAYER_BOUND_KEYS = ('', '_height', '_temperature')


def _lowest_valid_height(pressure, height):
    """The height of the lowest level of every column at which pressure and height are both non-NaN (NaN: no such level),
    in the arrays' own memory space."""
    if _is_torch(height):
        valid = ~(torch.isnan(pressure) | torch.isnan(height))
        z0 = torch.gather(height, 0, valid.to(torch.uint8).argmax(0, keepdim=True))[0]
        return torch.where(valid.any(0), z0, torch.full_like(z0, float('nan')))
    valid = ~(np.isnan(pressure) | np.isnan(height))
    z0 = np.take_along_axis(height, valid.argmax(0)[None], 0)[0]
    return np.where(valid.any(0), z0, np.nan).astype(height.dtype)


def _layer_bound(c, spec, side, p, t, z, z0):
    """One bound of a cape_cin_layers layer as a per-column pressure [hPa] in the call's space, or None (no bottom)."""
    given = [k for k in _LAYER_BOUND_KEYS if spec.get(side + k) is not None]
    assert len(given) <= 1, f'layers: give {side} at most once (pressure, height or temperature)'
    if not given:
        assert side == 'bottom', 'layers: every layer needs a top'
        return None
    value = spec[side + given[0]]
    if given[0] == '':
        return c.per_col(value)
    assert z is not None, 'layers: a bound by height or temperature needs height'
    if given[0] == '_height':
        at = z0 + c.per_col(value).reshape(z0.shape)
    else:
        assert np.ndim(value) == 0 and not _is_torch(value), 'layers: a temperature bound is one value [K]'
        at = crossing_level(z, t, float(value))
    return c.per_col(interp_level(z, p, at))


def cape_cin_layers(pressure, temperature, dewpoint, layers, height=None, parcel='surface', depth=None, parcel_values=None,
                    moist=None, **cape_cin_options):
    """CAPE and CIN over 1 ... 4 layers of ONE ascent per column (xp_cape_cin_layers): the positive area inside the layer
    between LFC and EL, and the negative area inside the layer below the LFC, of the profile cape_cin_columns lifts for
    the same parcel -- clipped out of its running sums, no profile arrays.  `layers`: a sequence of dicts that give each
    bound at most once, as
      'bottom' / 'top'                          a pressure [hPa], a scalar or one value per column;
      'bottom_height' / 'top_height'            metres above the lowest level with a valid pressure and height; the pressure
                                                is interp_level(height, pressure, z0 + h), linear in height (the rule of
                                                wind_layers' layers by height);
      'bottom_temperature' / 'top_temperature'  [K]: the height is crossing_level(height, temperature, value), the lowest
                                                crossing (freezing_level_height's rule), turned into a pressure likewise.
    No bottom: from the first node of the ascent.  Bounds by height or temperature need `height`; they are resolved with
    the library's own entry points in the inputs' memory space.  parcel, depth, parcel_values, moist and the options as in
    cape_cin_columns (pos_cape_neg_cin must stay True; 'family' runs as 'exact'; humidity 'dewpoint', 'relative' or
    'mixing_ratio', not 'specific').
    Returns a dict: 'cape', 'cin' [J/kg] of shape (nlayer,) + columns, 'bottom_pressure', 'top_pressure' (the resolved
    bounds; NaN bottom = from the first node), and per column 'total_cape', 'total_cin', 'lfc_pressure', 'el_pressure',
    'lcl_pressure', 'status' (cape_cin_columns' bits, and XP_ST_NO_LAYER where a layer has a NaN top or top >= bottom: that
    layer is NaN)."""
    assert cape_cin_options.get('humidity') != 'specific', 'cape_cin_layers does not take specific humidity'
    layers = list(layers)
    n = len(layers)
    assert 1 <= n <= L.CAPE_MAX_LAYERS, 'layers: one to four layers'
    assert all(set(l) <= {s + k for s in ('bottom', 'top') for k in _LAYER_BOUND_KEYS} for l in layers), 'layers: unknown key'
    bound_arrays = [v for l in layers for v in l.values() if _is_torch(v)]
    pv = list(parcel_values) if parcel == 'explicit' else []
    c = _Call(pressure, temperature, dewpoint, height, *[x for x in pv + bound_arrays if _is_torch(x)])
    p, t, td = c.ins[:3]
    z = None if height is None else c.ins[3]
    _same_shape(c.ins[:3 if z is None else 4], 'pressure, temperature, dewpoint, height must share a shape')
    o = _opts(moist=moist or _DEFAULT['moist'], **cape_cin_options)
    pc = _parcel(c, parcel, depth, pv)
    by_height = any(l.get(s + '_height') is not None for l in layers for s in ('bottom', 'top'))
    z0 = _lowest_valid_height(p, z) if by_height and z is not None else None
    bottoms = [_layer_bound(c, l, 'bottom', p, t, z, z0) for l in layers]
    tops = [_layer_bound(c, l, 'top', p, t, z, z0) for l in layers]
    out, res = c.struct(L.CapeLayersOut, L.CAPE_LAYERS_TOTAL + ('status',), L.CAPE_LAYERS_OUT, n)
    c.run('xp_cape_cin_layers', c.view(p), c.view(t), c.view(td), pc, o, n,
          (C.c_void_p * n)(*[None if b is None else _ptr(b) for b in bottoms]), (C.c_void_p * n)(*map(_ptr, tops)), out)
    nan = c.out(c.hshape)
    nan[...] = float('nan')
    stack = torch.stack if c.device is not None else np.stack
    res['bottom_pressure'] = stack([nan if b is None else b.reshape(c.hshape) for b in bottoms])
    res['top_pressure'] = stack([b.reshape(c.hshape) for b in tops])
    return res


def cape_3km(pressure, temperature, dewpoint, height, **kwargs):
    """0-3 km CAPE [J/kg] per column: cape_cin_layers between the first node of the ascent and 3000 m above the lowest
    valid level.  kwargs: parcel, depth, parcel_values, moist and the CAPE / CIN options."""
    return cape_cin_layers(pressure, temperature, dewpoint, [{'top_height': 3000.0}], height=height, **kwargs)['cape'][0]


def hail_growth_zone_cape(pressure, temperature, dewpoint, height, **kwargs):
    """Hail-growth-zone CAPE [J/kg] per column: cape_cin_layers between the environment's lowest -10 degC and -30 degC
    levels.  NaN (XP_ST_NO_LAYER) where the column has no -30 degC crossing or the two come in the wrong order; a column
    without a -10 degC crossing (a surface already colder) has no bottom, i.e. the layer starts at the first node of the
    ascent.  kwargs as cape_3km."""
    return cape_cin_layers(pressure, temperature, dewpoint, [{'bottom_temperature': 263.15, 'top_temperature': 243.15}],
                           height=height, **kwargs)['cape'][0]


def interp_level(coords, variable, at, log=False):
    """pf.py:1758 linear_interp (log=False) / pf.py:1813 log_interp (log=True) of one variable."""
    c = _Call(coords, variable)
    scalar = np.ndim(at) == 0 and not _is_torch(at)
    out = c.out(c.hshape)
    c.run('xp_interp_level', *map(c.view, c.ins), c.array([at]) if scalar else c.per_col(at), int(scalar), int(log), out)
    return out


def interp_levels(coords, variables, ats, log=False):
    """interp_level() for up to four variables at up to four scalar coordinates in one pass over the column
    (xp_interp_levels): returns [[variable v at ats[j] for j] for v]."""
    c = _Call(coords, *variables)
    cds, xs = c.ins[0], c.ins[1:]
    assert 1 <= len(xs) <= 4 and 1 <= len(ats) <= 4, 'one to four variables, one to four coordinates'
    _same_shape(c.ins, 'coords and variables must share a shape')
    vptrs = (C.POINTER(L.View) * len(xs))(*[C.pointer(c.view(x)) for x in xs])
    outs = [[c.out(c.hshape) for _ in ats] for _ in xs]
    optrs = (C.c_void_p * (len(xs) * len(ats)))(*[_ptr(o) for row in outs for o in row])
    at = (C.c_double * len(ats))(*[float(a) for a in ats])
    c.run('xp_interp_levels', c.view(cds), len(xs), vptrs, len(ats), at, int(log), optrs)
    return outs


def dewpoint_from_specific_humidity(pressure, temperature, specific_humidity):
    """metpy.calc.dewpoint_from_specific_humidity, MetPy 1.4.1 chain (parcel_test.py:262-266, pf.py:1889), K."""
    c = _Call(pressure, temperature, specific_humidity)
    _same_shape(c.ins, 'pressure, temperature, specific_humidity must share a shape')
    out = c.out(c.ins[0].shape)
    c.run('xp_dewpoint_from_specific_humidity', *map(c.view, c.ins), out)
    return out


def mixing_ratio(temperature, dewpoint, pressure):
    """pf.py:684: RH(T, Td) x saturation mixing ratio at (p, T) [kg/kg]."""
    c = _Call(temperature, dewpoint, pressure)
    _same_shape(c.ins, 'temperature, dewpoint, pressure must share a shape')
    shape = c.ins[0].shape
    n = int(np.prod(shape))
    out = c.out(shape)
    c.run('xp_mixing_ratio', *[c.view(a, 1, n) for a in c.ins], out)
    return out


def virtual_temperature(temperature, mixing_ratio, epsilon=0.608):
    """pf.py:782 (Doswell & Rasmussen 1994): one multiply-add, plain array arithmetic."""
    return temperature * (1 + epsilon * mixing_ratio)


def crossing_level(x, a, value):
    """Smallest x over all intersections of the profile a(x) with the constant `value` (find_intersections
    pf.py:992 + the min of pf.py:2153): freezing_level_height is crossing_level(height, temperature, 273.15)."""
    c = _Call(x, a)
    assert c.ins[0].shape == c.ins[1].shape
    out = c.out(c.hshape)
    c.run('xp_crossing_level', *map(c.view, c.ins), float(value), out)
    return out


# -- the reference's array primitives (pf.py:63-100, 164-227, 858-1064, 1200-1289, 1517-1555, 1604-1649, 1699-1720) --------
# The CAPE / CIN kernels never build these arrays; the functions exist because the reference offers them to its callers.
# Arrays are (nlev, ...) with the vertical first, datasets are dicts name -> array.  One level is a valid column: outputs of
# nlev - 1 rows then have zero rows (a zero-size buffer has no address: the library gets NULL for it and neither reads nor
# writes it) -- find_intersections returns six empty arrays, trap_around_zeros one all-NaN row and a mask of ones, trapz 0.
def insert_level(d, level, coords='pressure', fill_value=-999):
    """pf.py:933: insert `level` (dict name -> one value per column) into the dataset `d` sorted by decreasing `coords`;
    the keys of `level` define the output (pf.py:983)."""
    out = {}
    for k in level.keys():
        c = _Call(d[coords], d[k])
        _same_shape(c.ins, 'variables of a dataset must share a shape')
        out[k] = c.out((c.nlev + 1,) + c.hshape)
        c.run('xp_insert_level', *map(c.view, c.ins), c.per_col(level[coords]), c.per_col(level[k]), float(fill_value),
              out[k])
    return out


INTERSECTION_KEYS = ('all_intersect_x', 'all_intersect_y', 'increasing_x', 'increasing_y', 'decreasing_x', 'decreasing_y')


def find_intersections(x, a, b=None, log_x=False):
    """pf.py:992: dict of six (nlev - 1, ...) arrays; entry i belongs to the interval between levels i and i + 1."""
    c = _Call(x, a, b)
    _same_shape(c.ins, 'x, a, b must share a shape')
    out = {k: c.out((c.nlev - 1,) + c.hshape) for k in INTERSECTION_KEYS}
    c.run('xp_find_intersections', *c.views((x, a, b)), int(bool(log_x)), (C.c_void_p * 6)(*map(_ptr, out.values())))
    return out


def trapz(dat, x, mask=None, only_positive=False, only_negative=False):
    """pf.py:164 for one variable (array) or several (dict name -> array): sum of |dx| * mean over the intervals."""
    assert not (only_positive and only_negative), 'Only negative OR positive regions can be included in trapz.'   # pf.py:200
    if isinstance(dat, dict):
        return {k: trapz(v, x, mask=mask, only_positive=only_positive, only_negative=only_negative) for k, v in dat.items()}
    c = _Call(dat, x)
    _same_shape(c.ins, 'dat and x must share a shape')
    out = c.out(c.hshape)
    c.run('xp_trapz', *map(c.view, c.ins), None if mask is None else c.mask(mask, (max(c.nlev - 1, 0), c.ncol)),
          int(bool(only_positive)), int(bool(only_negative)), out)
    return out


AREA_KEYS = ('area', 'dx', 'x', 'x_from', 'x_to')


def trap_around_zeros(x, y, log_x=True, start=0):
    """pf.py:1200 (start = 0, the only value the reference uses): (areas, mask).  areas: dict of five (2 nlev - 1, ...)
    arrays, the areas before the zeros of y (rows 0 .. nlev-1) followed by the areas after them; mask: (nlev, ...) bool,
    True where no area was taken out of an interval."""
    assert start == 0, 'only start=0 is implemented (the reference never passes anything else)'
    c = _Call(x, y)
    _same_shape(c.ins, 'x and y must share a shape')
    areas = {k: c.out((2 * c.nlev - 1,) + c.hshape) for k in AREA_KEYS}
    mask = c.out(c.ins[0].shape, np.uint8)
    c.run('xp_trap_around_zeros', *map(c.view, c.ins), int(bool(log_x)), (C.c_void_p * 5)(*map(_ptr, areas.values())),
          mask)
    return areas, mask != 0


def bound_pressure(pressure, bound):
    """pf.py:208: the pressure of each column closest to `bound` (scalar or one per column)."""
    c = _Call(pressure)
    out = c.out(c.hshape)
    c.run('xp_bound_pressure', c.view(c.ins[0]), c.per_col(bound), out)
    return out


def get_layer(dat, depth=100, interpolate=True):
    """pf.py:63: dat = dict with 'pressure' and variables; the lowest `depth` hPa, NaN outside; with interpolate the layer top
    is inserted as a level (nlev + 1 rows)."""
    out = {}
    for k, v in dat.items():
        c = _Call(dat['pressure'], v)
        _same_shape(c.ins, 'variables of a dataset must share a shape')
        out[k] = c.out((c.nlev + (1 if interpolate else 0),) + c.hshape)
        c.run('xp_get_layer', *map(c.view, c.ins), float(depth), int(bool(interpolate)), int(k == 'pressure'), out[k])
    return out


def shift_out_nans(x, name):
    """pf.py:1699: x = dict name -> array; every column of every variable is moved down by the number of leading NaNs of
    x[name] in that column."""
    out = {}
    for k, v in x.items():
        c = _Call(x[name], v)
        _same_shape(c.ins, 'variables of a dataset must share a shape')
        out[k] = c.out(c.ins[0].shape)
        c.run('xp_shift_out_nans', *map(c.view, c.ins), out[k])
    return out


def _rebase(pressure, temperature, dewpoint, mode, depth):
    c, views, _ = _sounding(pressure, temperature, dewpoint)
    so, par = c.scalars(L.SCALAR_P + ('parcel_index',), c.hshape)
    outs = [c.out((c.nlev + (1 if mode == 'mixed_layer' else 0),) + c.hshape) for _ in range(3)]
    kept = np.zeros(c.nlev, dtype=np.int32)
    nout = C.c_int64(0)
    c.run('xp_rebase_profile', *views, _parcel(c, mode, depth), *outs, so, kept, C.byref(nout))
    n = nout.value
    parcel = {'pressure': par['parcel_pressure'], 'temperature': par['parcel_temperature'],
              'dewpoint': par['parcel_dewpoint'], 'index': par['parcel_index']}
    return outs[0][:n], outs[1][:n], outs[2][:n], parcel, kept.astype(bool)


def from_most_unstable_parcel(pressure, temperature, dewpoint, depth=300):
    """pf.py:1517: (pressure, temperature, dewpoint) at and above each column's most-unstable parcel -- levels that no column
    keeps dropped, columns shifted onto their first kept level -- the parcel, and the mask of input levels that survived."""
    return _rebase(pressure, temperature, dewpoint, 'most_unstable', depth)


def mix_layer(pressure, temperature, dewpoint, depth=100):
    """pf.py:1604: the profiles with the lowest `depth` hPa replaced by the mixed parcel (row 0), the parcel, and the mask of
    input levels that survived."""
    p, t, td, parcel, kept = _rebase(pressure, temperature, dewpoint, 'mixed_layer', depth)
    parcel.pop('index')
    return p, t, td, parcel, kept


def interp1d(at, xp, fp):
    """pf.py:23 interp1d_numba = numpy.interp along the vertical: at (m, ...), xp / fp (n, ...) or (n,) shared by all
    columns; xp increasing along the vertical."""
    c = _Call(at)
    ah = c.ins[0]

    def pts(v):
        a = c.array(v)
        cols = int(np.prod(a.shape[1:]))
        assert cols in (1, c.ncol), 'xp / fp must have one column or one per column of `at`'
        return a, a.shape[0], cols
    (xh, n, xc), (fh, n2, fc) = pts(xp), pts(fp)
    assert n == n2, 'xp and fp must have the same number of points'
    out = c.out(ah.shape)
    c.run('xp_interp1d', c.view(ah), c.view(xh, n, xc), c.view(fh, n, fc), out)
    return out


def add_lcl_to_profile(profile, environment=None, interpolator='log'):
    """pf.py:858: profile = dict with pressure, temperature, virtual_temperature (nlev, ...) and lcl_pressure,
    lcl_temperature, lcl_virtual_temperature (...); environment = dict with pressure and variables.  Returns the profile
    with the LCL inserted as a level (nlev + 1 rows) and, per environment variable k, environment_k with the environment
    interpolated at the LCL inserted likewise (its virtual temperature recomputed from the interpolated temperature and
    dewpoint, pf.py:911-920)."""
    if interpolator not in ('linear', 'log'):
        raise AssertionError('interpolator must be linear or log')                      # pf.py:878
    level = {'pressure': profile['lcl_pressure'], 'temperature': profile['lcl_temperature'],
             'virtual_temperature': profile['lcl_virtual_temperature']}
    out = insert_level({k: profile[k] for k in level}, level, coords='pressure')
    for k in ('lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature'):
        out[k] = profile[k]
    if environment is not None:
        il = {k: interp_level(environment['pressure'], v, level['pressure'], log=(interpolator == 'log'))
              for k, v in environment.items()}
        il['pressure'] = level['pressure']
        if 'virtual_temperature' in il:
            il['virtual_temperature'] = virtual_temperature(il['temperature'],
                                                            mixing_ratio(il['temperature'], il['dewpoint'], il['pressure']))
        env = insert_level(environment, il, coords='pressure')
        for k in environment.keys():
            if k != 'pressure':
                out['environment_' + k] = env[k]
    return out


def freezing_level_height(temperature, height):
    """pf.py:2137."""
    return crossing_level(height, temperature, 273.15)


def wet_bulb_temperature_fast(temperature, dewpoint):
    """pf.py:364: the "1/3 rule" estimate -- plain array arithmetic, no kernel of its own."""
    return temperature - (1 / 3) * (temperature - dewpoint)


def melting_level_height(pressure, temperature, dewpoint, height, fast=True, moist=None):
    """pf.py:2160: freezing level of the wet-bulb temperature field; returns (height, wet bulb)."""
    wb = wet_bulb_temperature_fast(temperature, dewpoint) if fast else \
        wet_bulb_temperature(pressure, temperature, dewpoint, moist=moist)
    return crossing_level(height, wb, 273.15), wb


def isobar_temperature(pressure, temperature, isobar):
    """pf.py:2193."""
    return interp_level(pressure, temperature, isobar, log=True)


def lapse_rate(pressure, temperature, height, from_pressure=700, to_pressure=500):
    """pf.py:2102: (T_to - T_from) / (z_to - z_from) with z in km, all four by log-p interpolation."""
    t0 = interp_level(pressure, temperature, from_pressure, log=True)
    t1 = interp_level(pressure, temperature, to_pressure, log=True)
    z0 = interp_level(pressure, height, from_pressure, log=True) / 1000
    z1 = interp_level(pressure, height, to_pressure, log=True) / 1000
    return (t1 - t0) / (z1 - z0)


def deep_convective_index(pressure, temperature, dewpoint, lifted_index):
    """pf.py:1830 (Kunz 2009): T850 + Td850 [deg C] - LI."""
    t850 = interp_level(pressure, temperature, 850.0, log=True) - 273.15
    td850 = interp_level(pressure, dewpoint, 850.0, log=True) - 273.15
    return t850 + td850 - lifted_index


LIFTED_INDEX_VARS = ('pressure', 'temperature', 'environment_temperature')      # the profile rows lifted_index() reads


def lifted_index(profile):
    """pf.py:1722: environment minus parcel temperature at 500 hPa (log-p interpolation of the profile)."""
    env = interp_level(profile['pressure'], profile['environment_temperature'], 500.0, log=True)
    par = interp_level(profile['pressure'], profile['temperature'], 500.0, log=True)
    return env - par


# ---- product bundle (pf.py:1951-2100, 2216-2407): compositions of the calls above + array arithmetic ---------------
def _ns(x):
    """numpy-or-torch namespace shim for the few element-wise helpers the bundle needs."""
    if _is_torch(x):
        return torch
    return np


def _where(c, a, b):
    if _is_torch(c) or _is_torch(a) or _is_torch(b):
        dev = next(v.device for v in (c, a, b) if _is_torch(v))
        a = a if _is_torch(a) else torch.as_tensor(a, device=dev, dtype=torch.float64)
        if np.ndim(b) == 0 and not _is_torch(b):
            return torch.where(c, a, float(b))          # (a scalar goes in by value: uploading it would wait for the stream)
        b = b if _is_torch(b) else torch.as_tensor(b, device=dev, dtype=a.dtype)
        return torch.where(c, a, b.to(a.dtype))
    return np.where(c, a, b)


def _flat(hs):
    n = int(np.prod(hs[0].shape)) if hs[0].shape else 1
    assert all((int(np.prod(h.shape)) if h.shape else 1) == n for h in hs), 'per-point arguments must share a shape'
    return n


def wind_shear(surface_wind_u, surface_wind_v, wind_u, wind_v, height, shear_height=6000):
    """pf.py:2216: wind at `shear_height` (linear interpolation in height) minus the surface wind (xp_wind_shear)."""
    c = _Call(wind_u, wind_v, height)
    _same_shape(c.ins, 'wind_u, wind_v, height must share a shape')
    res = {k: c.out(c.hshape) for k in ('shear_u', 'shear_v', 'shear_magnitude')}
    pos = c.out(c.hshape, np.int32)
    c.run('xp_wind_shear', *map(c.view, c.ins), c.per_col(surface_wind_u), c.per_col(surface_wind_v), float(shear_height),
          *res.values(), pos)
    res['positive_shear'] = pos != 0
    return res


def significant_hail_parameter(mucape, mixing_ratio, lapse, temp_500, shear, flh):
    """pf.py:2261 (SPC SHIP) with the reference's validity windows (xp_significant_hail_parameter)."""
    return _per_point('xp_significant_hail_parameter', [mucape, mixing_ratio, lapse, temp_500, shear, flh], (), 1)[0]


def bunkers_storm_motion(pressure, u, v, height):
    """metpy.calc.bunkers_storm_motion for every column (xp_bunkers_storm_motion): pressure [hPa], u, v [m/s] and height
    [m] on one vertical, (nlev, ...).  Returns a dict of per-column 'right_u', 'right_v', 'left_u', 'left_v', 'mean_u',
    'mean_v' [m/s] and 'status' (XP_ST_NO_LAYER: the column does not reach 6 km above its lowest level; ST_BAD_HEIGHT /
    ST_BAD_PRESSURE: the levels are out of order; everything NaN)."""
    c = _Call(pressure, u, v, height)
    _same_shape(c.ins, 'pressure, u, v, height must share a shape')
    out, res = c.struct(L.StormMotionOut, L.STORM_MOTION_OUT)
    c.run('xp_bunkers_storm_motion', *map(c.view, c.ins), out)
    return res


def _helicity(entry, height, u, v, per_col, storm, surface, n, many, keys, out_type, bounds):
    """What the two helicity calls share: the _Call (CUDA tensors among the per-column arguments decide the device), the
    storm and surface wind per column, one output per key with a leading axis of the n layers (if `many`) and the status.
    bounds(cols), cols being per_col as per-column arrays: the entry point's own arguments between the storm motion and the
    output struct."""
    assert (surface[0] is None) == (surface[1] is None), 'surface_u, surface_v: give both or neither'
    c = _Call(height, u, v, *[x for x in (*per_col, *storm, *surface) if _is_torch(x)])
    _same_shape(c.ins[:3], 'height, u, v must share a shape')
    sfc = [None, None] if surface[0] is None else [c.per_col(x) for x in surface]
    out, res = c.struct(out_type, ('status',), keys, n)
    cols = [c.per_col(x) for x in per_col]
    c.run(entry, *map(c.view, c.ins[:3]), *sfc, *[c.per_col(x) for x in storm], *bounds(cols), out)
    return res if many else {k: a.reshape(c.hshape) for k, a in res.items()}


def storm_relative_helicity(height, u, v, depth, bottom=0.0, storm_u=0.0, storm_v=0.0, surface_u=None, surface_v=None):
    """metpy.calc.storm_relative_helicity for every column (xp_storm_relative_helicity): height [m], u, v [m/s] (nlev, ...);
    heights are taken relative to the lowest valid level, or, with surface_u / surface_v, as heights above the surface
    with the surface wind as the point at 0 m.  `depth` [m]: a scalar, or a sequence of up to four depths computed in one
    pass (the outputs then gain a leading axis, one entry per depth); the layer runs from `bottom` to bottom + depth.
    storm_u, storm_v, surface_u, surface_v: scalars or one value per column.  With CUDA-tensor inputs the outputs of
    bunkers_storm_motion can be passed straight back as the storm motion (e.g. storm_u=bm['right_u']).  Returns a dict of
    'positive', 'negative', 'total' [m^2/s^2] and 'status' (XP_ST_NO_LAYER: some depth is not spanned, its values NaN;
    ST_BAD_HEIGHT: heights out of order, everything NaN)."""
    depths = [float(d) for d in np.atleast_1d(depth)]
    assert 1 <= len(depths) <= L.SRH_MAX_DEPTHS, 'depth: one to four depths'
    return _helicity('xp_storm_relative_helicity', height, u, v, (), (storm_u, storm_v), (surface_u, surface_v), len(depths),
                     np.ndim(depth) > 0, L.SRH_OUT, L.SrhOut,
                     lambda cols: (float(bottom), len(depths), (C.c_double * len(depths))(*depths)))


def storm_relative_helicity_layers(height, u, v, bottom, top, storm_u=0.0, storm_v=0.0, surface_u=None, surface_v=None):
    """Storm-relative helicity and the bulk wind difference between PER-COLUMN bounds (xp_storm_relative_helicity_layers):
    `bottom` and `top` [m] one value per column (scalars are broadcast) in storm_relative_helicity's height convention --
    above the lowest valid level, or above the surface with surface_u / surface_v: what effective_inflow_layer returns
    as base_height / top_height.  `top`: one array, or a sequence of up to four that share the bottom, computed in one
    pass (the outputs then gain a leading axis).  Returns a dict of 'positive', 'negative', 'total' [m^2/s^2], 'shear_u',
    'shear_v' (the wind at top minus the wind at bottom, each linear in height: wind_shear's rule, not MetPy's ln p
    bulk_shear), 'shear_magnitude' [m/s] and 'status' (XP_ST_NO_LAYER: a NaN or inverted bound, bottom < 0 or a layer the
    column does not span -- that layer NaN; ST_BAD_HEIGHT)."""
    many = isinstance(top, (list, tuple))
    tops = list(top) if many else [top]
    assert 1 <= len(tops) <= L.SRH_MAX_DEPTHS, 'top: one to four arrays'
    res = _helicity('xp_storm_relative_helicity_layers', height, u, v, (bottom, *tops), (storm_u, storm_v),
                    (surface_u, surface_v), len(tops), many, L.SRH_LAYERS_OUT, L.SrhLayersOut,
                    lambda cols: (cols[0], len(tops), (C.c_void_p * len(tops))(*map(_ptr, cols[1:]))))
    hyp = torch.hypot if _is_torch(res['shear_u']) else np.hypot
    return {**{k: res[k] for k in L.SRH_LAYERS_OUT}, 'shear_magnitude': hyp(res['shear_u'], res['shear_v']), 'status': res['status']}


def significant_tornado(sbcape, lcl_height, storm_helicity_1km, shear_6km):
    """metpy.calc.significant_tornado per point (xp_significant_tornado): sbcape [J/kg], LCL height [m], 0-1 km SRH
    [m^2/s^2], 0-6 km bulk shear [m/s]."""
    return _per_point('xp_significant_tornado', [sbcape, lcl_height, storm_helicity_1km, shear_6km], (), 1)[0]


def supercell_composite(mucape, effective_storm_helicity, effective_shear):
    """metpy.calc.supercell_composite per point (xp_supercell_composite): mucape [J/kg], SRH [m^2/s^2], shear [m/s]."""
    return _per_point('xp_supercell_composite', [mucape, effective_storm_helicity, effective_shear], (), 1)[0]


def _wind_layer(spec):
    """One layer of wind_layers() as (kind, bottom, top) of xp_wind_layer.  A dict: bottom= [hPa; None or absent: the lowest
    valid level] with top= [hPa] or depth= [hPa], or bottom_height= [m above the lowest valid level; default 0] with
    top_height= [m].  A tuple: ('pressure', bottom, top), ('pressure_depth', bottom, depth) or ('height', bottom, top)."""
    kinds = {'pressure': L.LAYER_PRESSURE, 'pressure_depth': L.LAYER_PRESSURE_DEPTH, 'height': L.LAYER_HEIGHT}
    if isinstance(spec, dict):
        assert set(spec) <= {'bottom', 'top', 'depth', 'bottom_height', 'top_height'}, 'layer: unknown key in %r' % (spec,)
        if 'top_height' in spec:
            assert set(spec) <= {'bottom_height', 'top_height'}, 'layer: heights and pressures cannot be mixed'
            kind, bottom, top = 'height', spec.get('bottom_height', 0.0), spec['top_height']
        else:
            assert ('top' in spec) != ('depth' in spec) and 'bottom_height' not in spec, 'layer: give top= or depth= (hPa), or top_height='
            kind, bottom, top = ('pressure', spec.get('bottom'), spec['top']) if 'top' in spec else ('pressure_depth', spec.get('bottom'), spec['depth'])
    else:
        kind, bottom, top = spec
    assert kind in kinds, "layer: kind must be 'pressure', 'pressure_depth' or 'height'"
    return kinds[kind], float('nan') if bottom is None else float(bottom), float(top)


def wind_layers(pressure, u, v, height=None, layers=(), want=None):
    """The wind over up to four layers of every column in one pass (xp_wind_layers): pressure [hPa], u, v [m/s] and, for
    layers given by height, height [m] on one vertical, (nlev, ...).  `layers`: a sequence of layers, each a dict or a tuple
    (see _wind_layer): {'bottom': 850, 'top': 300}, {'depth': 100} (the lowest 100 hPa), {'bottom_height': 0, 'top_height':
    6000}.  Returns a dict with a leading layer axis: 'mean_u', 'mean_v' (metpy.calc.mean_pressure_weighted), 'shear_u',
    'shear_v' (metpy.calc.bulk_shear: top minus bottom, the bounds interpolated in ln p), 'bottom_u', 'bottom_v' (the wind
    at the layer's bottom), 'max_u', 'max_v', 'max_pressure' (the layer's strongest wind and where it blows) -- or those of
    them that `want` names -- and the per-column 'status' (XP_ST_NO_LAYER: some layer is empty or not spanned by the column,
    its values NaN; ST_BAD_HEIGHT / ST_BAD_PRESSURE: levels out of order, everything NaN)."""
    specs = [_wind_layer(s) for s in layers]
    assert 1 <= len(specs) <= L.WIND_MAX_LAYERS, 'layers: one to four layers'
    assert height is not None or all(k != L.LAYER_HEIGHT for k, _, _ in specs), 'a layer given by height needs height'
    keys = L.WIND_LAYERS_OUT if want is None else tuple(want)
    assert set(keys) <= set(L.WIND_LAYERS_OUT), 'want: unknown output'
    c = _Call(pressure, u, v, height)
    _same_shape(c.ins, 'pressure, u, v, height must share a shape')
    n = len(specs)
    out, res = c.struct(L.WindLayersOut, ('status',), keys, n)
    c.run('xp_wind_layers', *c.views((pressure, u, v, height)), n, (L.WindLayer * n)(*[L.WindLayer(k, 0, b, t) for k, b, t in specs]), out)
    return res


def _one_layer(pressure, u, v, height, bottom, depth, want):
    """The layer of mean_pressure_weighted / bulk_shear, which take MetPy's bottom= and depth= without its units: with
    `height` AND `bottom` given, bottom and depth are metres, bottom counted from the lowest valid level; otherwise they are
    hPa, bottom=None being the lowest valid level."""
    if height is not None and bottom is not None:
        layer = ('height', bottom, float(bottom) + float(depth))
    else:
        height, layer = None, ('pressure_depth', bottom, depth)
    res = wind_layers(pressure, u, v, height, [layer], want=want)
    return tuple(res[k][0] for k in want), res['status']


def mean_pressure_weighted(pressure, u, v, height=None, bottom=None, depth=100.0):
    """metpy.calc.mean_pressure_weighted of the wind for every column: (mean_u, mean_v) [m/s] over the layer from `bottom` up
    `depth`.  The exact rule for the two, MetPy's taking them with units: if `height` [m] is given and `bottom` is not
    None, bottom and depth are metres and bottom is counted from the lowest valid level (0: that level); in every other
    case they are hPa and bottom=None is the lowest valid level -- so the defaults are MetPy's, the lowest 100 hPa.  Columns
    that do not span the layer are NaN."""
    return _one_layer(pressure, u, v, height, bottom, depth, ('mean_u', 'mean_v'))[0]


def bulk_shear(pressure, u, v, height=None, bottom=None, depth=100.0):
    """metpy.calc.bulk_shear for every column: (shear_u, shear_v) [m/s], the wind at the top of the layer minus the wind at
    its bottom, each interpolated in ln p where it lies between levels.  bottom, depth: as in mean_pressure_weighted."""
    return _one_layer(pressure, u, v, height, bottom, depth, ('shear_u', 'shear_v'))[0]


def _per_point(entry, ins, per_col, nout, extra=()):
    """A per-point entry point on the arrays `ins` (one shape) and the per-column arguments `per_col` (scalars broadcast;
    CUDA tensors among them take part in deciding the device): `nout` outputs of that shape."""
    c = _Call(*ins, *[x for x in per_col if _is_torch(x)])
    _same_shape(c.ins[:len(ins)], 'per-point arguments must share a shape')
    shape = tuple(c.ins[0].shape)
    n = int(np.prod(shape))
    cols = [None if x is None else c.per_col(x, n, 'per-point arguments must share a shape') for x in per_col]
    outs = [c.out(shape) for _ in range(nout)]
    c.run(entry, n, c.xp_dtype, c.mem, *c.ins[:len(ins)], *cols, *extra, *outs)
    return outs


def critical_angle(pressure, u, v, height, storm_u, storm_v):
    """metpy.calc.critical_angle for every column [degrees]: the angle between the 0-500 m bulk shear and the storm-relative
    inflow at the lowest valid level, storm_u / storm_v being scalars or one value per column (e.g. bunkers_storm_motion's
    right_u, right_v; CUDA tensors stay on the device).  One wind_layers call (0-500 m above the lowest valid level by
    height: shear_* and bottom_*), then xp_critical_angle.  NaN where the column does not reach 500 m or a vector is zero."""
    wl = wind_layers(pressure, u, v, height, [('height', 0.0, 500.0)], want=('shear_u', 'shear_v', 'bottom_u', 'bottom_v'))
    return _per_point('xp_critical_angle', [wl[k][0] for k in ('shear_u', 'shear_v', 'bottom_u', 'bottom_v')],
                      (storm_u, storm_v), 1)[0]


def corfidi_storm_motion(pressure, u, v, llj_u=None, llj_v=None):
    """Corfidi (2003) upwind- and downwind-propagating MCS motion for every column (metpy.calc.corfidi_storm_motion): the
    mean wind is the 850-300 hPa pressure-weighted mean; the low-level jet llj_u / llj_v (both or neither; scalars or one
    value per column) defaults to the strongest wind at or below 850 hPa -- both from ONE wind_layers call.  Returns a dict of
    'upwind_u', 'upwind_v', 'downwind_u', 'downwind_v' [m/s] and the 'status' of the wind_layers call; columns whose lowest
    level lies above 850 hPa or that end below 300 hPa are NaN."""
    assert (llj_u is None) == (llj_v is None), 'llj_u, llj_v: give both or neither'
    layers, want = [('pressure', 850.0, 300.0)], ('mean_u', 'mean_v')
    if llj_u is None:
        layers, want = layers + [('pressure', None, 850.0)], want + ('max_u', 'max_v')
    wl = wind_layers(pressure, u, v, None, layers, want=want)
    ins = [wl['mean_u'][0], wl['mean_v'][0]] + ([wl['max_u'][1], wl['max_v'][1]] if llj_u is None else [])
    outs = _per_point('xp_corfidi_storm_motion', ins, () if llj_u is None else (llj_u, llj_v), 4)
    return dict(zip(('upwind_u', 'upwind_v', 'downwind_u', 'downwind_v'), outs), status=wl['status'])


def significant_tornado_effective(mlcape, mlcin, lcl_height, esrh, ebwd, base_height=None):
    """SPC's effective-layer significant tornado parameter per point (xp_significant_tornado_effective): mixed-layer CAPE
    and CIN [J/kg; CIN <= 0], mixed-layer LCL height [m], effective SRH [m^2/s^2] and effective bulk wind difference [m/s].
    base_height [m]: the effective inflow base (effective_inflow_layer's base_height); where it is > 0 the result is 0."""
    ins = [mlcape, mlcin, lcl_height, esrh, ebwd] + ([] if base_height is None else [base_height])
    return _per_point('xp_significant_tornado_effective', ins, (), 1, extra=(None,) if base_height is None else ())[0]


def _is_per_column(x):
    return _is_torch(x) or (x is not None and np.ndim(x) > 0)


def _thermo_layer(spec):
    """One layer of thermo_layers() as (kind, bottom, top, bottom_column, top_column): _wind_layer's layers, and for a layer
    by pressure -- {'bottom': ..., 'top': ...} or ('pressure', bottom, top) -- top=None (to the highest valid level) and
    bottom / top given per column (an array or a tensor, which replaces the scalar)."""
    if isinstance(spec, dict) and 'top' in spec:
        assert set(spec) <= {'bottom', 'top'}, 'layer: top= [hPa] goes with bottom= only, in %r' % (spec,)
        bottom, top = spec.get('bottom'), spec['top']
    elif not isinstance(spec, dict) and len(spec) == 3 and spec[0] == 'pressure':
        bottom, top = spec[1:]
    else:
        return _wind_layer(spec) + (None, None)
    bcol, tcol = (x if _is_per_column(x) else None for x in (bottom, top))
    kind, b, t = _wind_layer(('pressure', None if bcol is not None else bottom, float('nan') if tcol is not None or top is None else top))
    return kind, b, t, bcol, tcol


def thermo_layers(pressure, temperature=None, dewpoint=None, height=None, layers=(), want=None):
    """Temperature and humidity over up to four layers of every column in one pass (xp_thermo_layers): pressure [hPa] and,
    as far as the wanted outputs read them, temperature, dewpoint [K] and height [m] on one vertical, (nlev, ...).  `layers`:
    as in wind_layers -- {'bottom': 700, 'top': 500}, {'depth': 100}, {'bottom_height': 0, 'top_height': 3000} -- and, for a
    layer by pressure, 'top': None (to the highest valid level) and 'bottom' / 'top' given per column (arrays or device
    tensors of the horizontal shape; a NaN bottom: the lowest valid level; a NaN top: no layer).  Returns a dict with a
    leading layer axis: 'precipitable_water' [mm] (metpy.calc.precipitable_water), 'mean_mixing_ratio' [kg/kg],
    'mean_relative_humidity' [0 ... 1] (pressure-weighted layer means), 'thickness' [m], 'lapse_rate' [K/km, positive where
    it cools upward], 'theta_e_min', 'theta_e_max' [K] with 'theta_e_min_pressure', 'theta_e_max_pressure' [hPa] (over the
    layer's points) -- those that `want` names; by default every one the supplied inputs allow -- and the per-column 'status'
    (XP_ST_NO_LAYER: some layer is empty or not spanned by the column, its values NaN; ST_BAD_HEIGHT / ST_BAD_PRESSURE: levels
    out of order, everything NaN)."""
    specs = [_thermo_layer(s) for s in layers]
    n = len(specs)
    assert 1 <= n <= L.THERMO_MAX_LAYERS, 'layers: one to four layers'
    assert height is not None or all(s[0] != L.LAYER_HEIGHT for s in specs), 'a layer given by height needs height'
    given = {'temperature': temperature, 'dewpoint': dewpoint, 'height': height}
    if want is None:
        keys = tuple(k for k in L.THERMO_LAYERS_OUT if all(given[v] is not None for v in L.THERMO_LAYERS_NEEDS[k]))
    else:
        keys = tuple(want)
        assert set(keys) <= set(L.THERMO_LAYERS_OUT), 'want: unknown output'
        for k in keys:
            assert all(given[v] is not None for v in L.THERMO_LAYERS_NEEDS[k]), '%s needs %s' % (k, ' and '.join(L.THERMO_LAYERS_NEEDS[k]))
    soundings = (pressure, temperature, dewpoint, height)
    bounds = [x for s in specs for x in s[3:] if _is_torch(x)]
    c = _Call(*soundings, *bounds)
    _same_shape(c.ins[:len(c.ins) - len(bounds)], 'pressure, temperature, dewpoint, height must share a shape')
    out, res = c.struct(L.ThermoLayersOut, ('status',), keys, n)
    cols = [[None if s[j] is None else c.per_col(s[j]) for s in specs] for j in (3, 4)]
    bcols, tcols = (None if all(x is None for x in col) else (C.c_void_p * n)(*[None if x is None else _ptr(x) for x in col])
                    for col in cols)
    c.run('xp_thermo_layers', *c.views(soundings), n, (L.WindLayer * n)(*[L.WindLayer(s[0], 0, s[1], s[2]) for s in specs]), bcols, tcols, out)
    return res


def precipitable_water(pressure, dewpoint, bottom=None, top=None):
    """metpy.calc.precipitable_water for every column [mm]: -1 / (g rho_l) times the integral of the mixing ratio w(p, Td) over
    pressure from `bottom` [hPa; None: the lowest valid level] to `top` [hPa; None: the highest valid level], the bounds
    interpolated in ln p where they lie between levels; bottom / top may be per-column arrays.  NaN where the column does not
    span the layer."""
    return thermo_layers(pressure, dewpoint=dewpoint, layers=[{'bottom': bottom, 'top': top}], want=('precipitable_water',))['precipitable_water'][0]


def mean_relative_humidity(pressure, temperature, dewpoint, height=None, layer=('pressure', 700.0, 500.0)):
    """The pressure-weighted mean relative humidity [0 ... 1] of one layer of every column: trapz(e_s(Td) / e_s(T), p) over
    the layer's depth.  `layer`: one layer of thermo_layers (by height: give `height`); default 700-500 hPa."""
    return thermo_layers(pressure, temperature, dewpoint, height, layers=[layer], want=('mean_relative_humidity',))['mean_relative_humidity'][0]


def layer_lapse_rate(pressure, temperature, height, layer=('pressure', 700.0, 500.0)):
    """(lapse_rate [K/km, positive where it cools upward], thickness [m]) between the bounds of one layer of every column,
    temperature and height interpolated in ln p where a bound lies between levels.  `layer`: one layer of thermo_layers;
    default 700-500 hPa."""
    res = thermo_layers(pressure, temperature, None, height, layers=[layer], want=('lapse_rate', 'thickness'))
    return res['lapse_rate'][0], res['thickness'][0]


def hail_growth_zone_thickness(pressure, temperature, height):
    """(thickness [m], lapse_rate [K/km]) of the hail growth zone of every column: the layer between the environment's lowest
    -10 degC and -30 degC levels, resolved as hail_growth_zone_cape resolves them (crossing_level in height, turned into a
    pressure by interp_level) in the inputs' memory space and passed on as per-column pressures.  NaN where the column has no
    -30 degC crossing or the two come in the wrong order; from the lowest valid level where it has no -10 degC crossing."""
    c = _Call(pressure, temperature, height)
    p, t, z = c.ins
    _same_shape(c.ins, 'pressure, temperature, height must share a shape')
    spec = {'bottom_temperature': 263.15, 'top_temperature': 243.15}
    bottom, top = (_layer_bound(c, spec, side, p, t, z, None).reshape(c.hshape or (1,)) for side in ('bottom', 'top'))
    res = thermo_layers(p, t, None, z, layers=[{'bottom': bottom, 'top': top}], want=('thickness', 'lapse_rate'))
    return res['thickness'][0], res['lapse_rate'][0]


def theta_e_difference(pressure, temperature, dewpoint, height):
    """The theta_e-difference index of every column [K] (Atkins and Wakimoto 1991, wet microbursts): the largest minus the
    smallest equivalent potential temperature among the points of the lowest 3 km above the lowest valid level, and 0 where
    the largest lies ABOVE the smallest (theta_e_max_pressure < theta_e_min_pressure).  NaN where the column does not reach
    3 km."""
    res = thermo_layers(pressure, temperature, dewpoint, height, layers=[('height', 0.0, 3000.0)],
                        want=('theta_e_min', 'theta_e_min_pressure', 'theta_e_max', 'theta_e_max_pressure'))
    diff = res['theta_e_max'][0] - res['theta_e_min'][0]
    return _where(~(res['theta_e_max_pressure'][0] < res['theta_e_min_pressure'][0]), diff, 0.0)


def sounding_indices(pressure, temperature, dewpoint, u=None, v=None, *, moist=None, which='top', mixed_layer_depth=None,
                     want=None):
    """The classic sounding indices and the convective condensation level of every column in one pass (xp_sounding_indices;
    include/xparcel.h has the rules): pressure [hPa], temperature, dewpoint [K] and, for the SWEAT index, u, v [m/s] on one
    vertical, (nlev, ...).  Values at 850, 700 and 500 hPa are the level's own where a valid level lies on the isobar and
    linear in ln p between the neighbouring valid levels otherwise.  Returns a dict of per-column 'k_index', 'total_totals',
    'cross_totals', 'vertical_totals', 'showalter_index' [K], 'sweat_index', 'ccl_pressure' [hPa], 'ccl_temperature' and
    'convective_temperature' [K] -- those that `want` names; by default all of them, 'sweat_index' only with winds -- and
    'status' (XP_ST_NO_LAYER: the column does not span 850 ... 500 hPa, the indices NaN; ST_NO_CCL: no CCL, its three outputs
    NaN; ST_LCL_NOT_CONVERGED: the Showalter parcel's LCL; each bit only where an output it belongs to is wanted).
    moist: the Showalter parcel's moist adiabat ('exact', 'family': RK4; 'table': the lookup tables).  which: 'top' (MetPy's
    default) or 'bottom', the CCL crossing taken.  mixed_layer_depth [hPa]: the CCL of the mixed-layer mean mixing ratio over
    that depth instead of the lowest valid level's (None or 0)."""
    assert (u is None) == (v is None), 'u and v must be given together'
    assert which in L.CCL_WHICH, "which must be 'top' or 'bottom'"
    depth = 0.0 if mixed_layer_depth is None else float(mixed_layer_depth)
    assert np.isfinite(depth) and depth >= 0.0, 'mixed_layer_depth must be None, 0 or finite and positive'
    if want is None:
        keys = tuple(k for k in L.SOUNDING_OUT if k != 'sweat_index' or u is not None)
    else:
        keys = tuple(want)
        assert set(keys) <= set(L.SOUNDING_OUT), 'want: unknown output'
        assert 'sweat_index' not in keys or u is not None, 'sweat_index needs u and v'
    c = _Call(pressure, temperature, dewpoint, u, v)
    _same_shape(c.ins, 'pressure, temperature, dewpoint, u, v must share a shape')
    out, res = c.struct(L.SoundingOut, keys + ('status',))
    c.run('xp_sounding_indices', *c.views((pressure, temperature, dewpoint, u, v)), L.SoundingOpts(L.MOIST[moist or _DEFAULT['moist']], L.CCL_WHICH[which], depth), out)
    return res


def k_index(pressure, temperature, dewpoint):
    """metpy.calc.k_index [K] of every column: (T850 - T500) + Td850[degC] - (T700 - Td700)."""
    return sounding_indices(pressure, temperature, dewpoint, want=('k_index',))['k_index']


def total_totals_index(pressure, temperature, dewpoint):
    """metpy.calc.total_totals_index [K] of every column: (T850 - T500) + (Td850 - T500)."""
    return sounding_indices(pressure, temperature, dewpoint, want=('total_totals',))['total_totals']


def cross_totals(pressure, temperature, dewpoint):
    """metpy.calc.cross_totals [K] of every column: Td850 - T500."""
    return sounding_indices(pressure, temperature, dewpoint, want=('cross_totals',))['cross_totals']


def vertical_totals(pressure, temperature, dewpoint=None):
    """metpy.calc.vertical_totals [K] of every column: T850 - T500.  MetPy's takes no dewpoint; here a level counts only
    where its dewpoint is valid too, so without one the temperature stands in for it."""
    return sounding_indices(pressure, temperature, temperature if dewpoint is None else dewpoint,
                            want=('vertical_totals',))['vertical_totals']


def showalter_index(pressure, temperature, dewpoint, moist=None):
    """metpy.calc.showalter_index [K] of every column: T500 minus the 500 hPa temperature of the parcel lifted from 850 hPa."""
    return sounding_indices(pressure, temperature, dewpoint, moist=moist, want=('showalter_index',))['showalter_index']


def sweat_index(pressure, temperature, dewpoint, u, v):
    """metpy.calc.sweat_index of every column, from u, v [m/s] instead of MetPy's speed and direction."""
    return sounding_indices(pressure, temperature, dewpoint, u, v, want=('sweat_index',))['sweat_index']


def ccl(pressure, temperature, dewpoint, mixed_layer_depth=None, which='top'):
    """metpy.calc.ccl of every column: (ccl_pressure [hPa], ccl_temperature [K], convective_temperature [K]); NaN where
    the dewpoint line of the parcel's mixing ratio never crosses the temperature."""
    res = sounding_indices(pressure, temperature, dewpoint, which=which, mixed_layer_depth=mixed_layer_depth, want=L.SOUNDING_CCL_OUT)
    return tuple(res[k] for k in L.SOUNDING_CCL_OUT)


def isentropic_interpolation(levels, pressure, temperature, *args, temperature_out=False, max_iters=50, eps=1e-6,
                             bottom_up_search=True, status=False):
    """metpy.calc.isentropic_interpolation of every column (xp_isentropic_interpolation; include/xparcel.h has the rules and
    the three deliberate differences from MetPy): pressure [hPa] -- (nlev, ...) or, for isobaric data, the nlev values --
    temperature [K] and any further variables `args` on the same vertical are put onto the surfaces of potential temperature
    `levels` [K].  Returns MetPy's list: the pressure, the temperature if `temperature_out`, one array per arg and, with
    status=True, the int32 per-column status (XP_ST_NO_LAYER: some target has no bracketing pair in the column;
    ST_NOT_CONVERGED: some target's Newton iteration took max_iters steps without meeting eps; such targets are NaN).  Each
    array is (nlevel,) + the horizontal shape, in the inputs' space.  levels are sorted ascending, as MetPy does, and the
    outputs come in that order; duplicates are rejected.  bottom_up_search: the lowest bracketing pair (True) or the highest.
    More than 64 levels or 4 args are served by consecutive calls of at most that many."""
    lev = np.sort(np.asarray(levels, dtype=np.float64).reshape(-1))
    assert lev.size >= 1 and np.all(np.isfinite(lev)), 'levels must be finite, at least one'
    assert np.all(np.diff(lev) > 0), 'levels must not hold duplicates'
    assert int(max_iters) >= 1, 'max_iters must be at least 1'
    assert np.isfinite(eps) and eps > 0, 'eps must be finite and positive'
    c = _Call(_full_pressure(pressure, temperature), temperature, *args)
    _same_shape(c.ins, 'pressure, temperature and the further variables must share a shape')
    views, n = [c.view(a) for a in c.ins], len(lev)
    shape = (n,) + c.hshape
    p_out, t_out = c.out(shape), c.out(shape) if temperature_out else None
    v_out = [c.out(shape) for _ in args]
    st_out = None
    opts = L.IsentropicOpts(int(bool(bottom_up_search)), int(max_iters), float(eps))
    for i0 in range(0, max(len(args), 1), L.ISEN_MAX_VARS):
        vs = views[2 + i0:2 + i0 + L.ISEN_MAX_VARS]
        vptrs = (C.POINTER(L.View) * len(vs))(*[C.pointer(v) for v in vs]) if vs else None
        for j0 in range(0, n, L.ISEN_MAX_LEVELS):
            j1 = min(n, j0 + L.ISEN_MAX_LEVELS)
            out = L.IsentropicOut(dtype=c.xp_dtype, mem=c.mem)
            for q in range(len(vs)):
                out.vars[q] = _ptr(v_out[i0 + q][j0:j1])
            if i0 == 0:                                       # the pressure, the temperature and the status come from the first call
                out.pressure = _ptr(p_out[j0:j1])
                if temperature_out:
                    out.temperature = _ptr(t_out[j0:j1])
                part = c.out(c.hshape, np.int32)
                out.status = _ptr(part)
            c.run('xp_isentropic_interpolation', views[0], views[1], len(vs), vptrs, j1 - j0, (C.c_double * (j1 - j0))(*lev[j0:j1]),
                  opts, out)
            if i0 == 0:
                st_out = part if st_out is None else st_out | part
    return [p_out] + ([t_out] if temperature_out else []) + v_out + ([st_out] if status else [])


def _hydro_layer(spec):
    """One layer of hydrostatic() as (kind, bottom, top) of xp_wind_layer: _wind_layer's layers by pressure, and for
    {'bottom': ..., 'top': ...} / ('pressure', bottom, top) top=None, to the highest valid level."""
    if isinstance(spec, dict) and 'top' in spec and spec['top'] is None:
        spec = dict(spec, top=float('nan'))
    elif not isinstance(spec, dict) and len(spec) == 3 and spec[0] == 'pressure' and spec[2] is None:
        spec = (spec[0], spec[1], float('nan'))
    kind, bottom, top = _wind_layer(spec)
    assert kind != L.LAYER_HEIGHT, 'hydrostatic: layers are given by pressure (the heights are what the call computes)'
    return kind, bottom, top


def hydrostatic(pressure, temperature, dewpoint=None, specific_humidity=None, base_height=None, layers=(), want=None):
    """Hydrostatic heights and layer thickness of every column in one pass (xp_hydrostatic_height; include/xparcel.h has the
    rules): pressure [hPa] -- (nlev, ...) or, for isobaric data, the nlev values -- temperature [K] and, for the virtual
    temperature, EITHER dewpoint [K] OR specific_humidity [kg/kg] on the same vertical (neither: a dry atmosphere).
    base_height [m]: the height of each column's lowest valid level, a scalar or one value per column; None: 0, heights above
    the lowest valid level.  `layers`: up to four layers by pressure as in thermo_layers -- {'bottom': 1000, 'top': 500},
    {'depth': 150} (the lowest 150 hPa), {'bottom': None, 'top': None} (the whole column).  Returns a dict: 'height' (nlev, ...)
    [m], NaN at invalid levels; 'thickness', a list of one per-column array per layer [m], NaN where the column does not span
    the layer; the per-column 'status' (XP_ST_NO_LAYER: some layer is not spanned, or the column has no valid level;
    XP_ST_BAD_PRESSURE: a level out of order, the heights from it upward and every thickness NaN) -- or those of them that
    `want` names.  Values do not depend on what else is asked for."""
    assert dewpoint is None or specific_humidity is None, 'give dewpoint or specific_humidity, not both'
    specs = [_hydro_layer(s) for s in layers]
    n = len(specs)
    assert n <= L.HYDRO_MAX_LAYERS, 'layers: at most four layers'
    keys = ('height', 'thickness', 'status') if want is None else tuple(want)
    assert set(keys) <= {'height', 'thickness', 'status'}, 'want: unknown output'
    moisture = dewpoint if dewpoint is not None else specific_humidity
    c = _Call(_full_pressure(pressure, temperature), temperature, moisture, base_height if _is_torch(base_height) else None)
    _same_shape(c.ins[:2 if moisture is None else 3], 'pressure, temperature and the moisture must share a shape')
    res = {}
    out = L.HydrostaticOut(dtype=c.xp_dtype, mem=c.mem)
    if 'height' in keys:
        res['height'] = c.out((c.nlev,) + c.hshape)
        out.height = _ptr(res['height'])
    if 'thickness' in keys:
        res['thickness'] = [c.out(c.hshape) for _ in range(n)]
        for i, a in enumerate(res['thickness']):
            out.thickness[i] = _ptr(a)
    if 'status' in keys:
        res['status'] = c.out(c.hshape, np.int32)
        out.status = _ptr(res['status'])
    base = None if base_height is None else c.per_col(base_height)
    opts = L.HydrostaticOpts(L.HUM_SPECIFIC if specific_humidity is not None else L.HUM_DEWPOINT, 0)
    c.run('xp_hydrostatic_height', *c.views((pressure, temperature, moisture)), base, n, (L.WindLayer * n)(*[L.WindLayer(k, 0, b, t) for k, b, t in specs]) if n else None,
          opts, out)
    return res


def hydrostatic_height(pressure, temperature, dewpoint=None, specific_humidity=None, base_height=None, status=False):
    """The hydrostatic height [m] of every level of every column, (nlev, ...): base_height (None: 0) at the lowest valid level,
    then the trapezoid of the virtual temperature over ln p, level by level (MetPy's thickness_hydrostatic accumulated);
    NaN at invalid levels.  Arguments as hydrostatic(); with status=True the int32 per-column status follows."""
    res = hydrostatic(pressure, temperature, dewpoint, specific_humidity, base_height, want=('height', 'status') if status else ('height',))
    return (res['height'], res['status']) if status else res['height']


def thickness_hydrostatic(pressure, temperature, dewpoint=None, specific_humidity=None, bottom=None, depth=None):
    """metpy.calc.thickness_hydrostatic for every column [m]: the hydrostatic thickness of the layer from `bottom` [hPa; None:
    the lowest valid level] up `depth` [hPa; None: to the highest valid level], the bounds interpolated in ln p where they lie
    between levels (MetPy's get_layer).  One deviation from MetPy: the moisture is given as dewpoint [K] or as
    specific_humidity [kg/kg], not as mixing_ratio; neither: a dry atmosphere.  NaN where the column does not span the layer."""
    layer = ('pressure', bottom, None) if depth is None else ('pressure_depth', bottom, depth)
    return hydrostatic(pressure, temperature, dewpoint, specific_humidity, layers=[layer], want=('thickness',))['thickness'][0]


def geopotential_to_height(geopotential):
    """metpy.calc.geopotential_to_height per point: geopotential [m^2/s^2] -> height [m] = (Phi Re) / (g Re - Phi)."""
    return _per_point('xp_geopotential_to_height', [geopotential], (), 1)[0]


def height_to_geopotential(height):
    """metpy.calc.height_to_geopotential per point: height [m] -> geopotential [m^2/s^2] = (g Re z) / (Re + z)."""
    return _per_point('xp_height_to_geopotential', [height], (), 1)[0]


def ncape(pressure, temperature, dewpoint, height, lfc_pressure, el_pressure):
    """The buoyancy-dilution potential NCAPE of entraining CAPE (Peters et al. 2023) for every column (xp_ncape): the integral
    over height, between the LFC and the EL, of -(g / (cp T)) (hbar - hs) of the ENVIRONMENT -- hbar the mean moist static
    energy from the lowest valid level up to the height in question, hs the saturated moist static energy there.  pressure
    [hPa], temperature, dewpoint [K], height [m] on one vertical, (nlev, ...); lfc_pressure, el_pressure [hPa]: one value per
    column, what cape_cin_columns returns for the parcel of interest (NaN LFC: ncape 0; NaN EL: up to the highest valid
    level).  Returns a dict of per-column 'ncape' [J/kg], 'lfc_height', 'el_height' [m above the lowest valid level] and
    'status' (XP_ST_NO_LAYER: EL not above the LFC or fewer than two valid levels; ST_BAD_HEIGHT / ST_BAD_PRESSURE: levels out
    of order; everything NaN)."""
    c = _Call(pressure, temperature, dewpoint, height, *[x for x in (lfc_pressure, el_pressure) if _is_torch(x)])
    _same_shape(c.ins[:4], 'pressure, temperature, dewpoint, height must share a shape')
    out, res = c.struct(L.NcapeOut, L.NCAPE_OUT)
    c.run('xp_ncape', *map(c.view, c.ins[:4]), c.per_col(lfc_pressure), c.per_col(el_pressure), out)
    return res


def ecape_from_ncape(cape, ncape, el_height, sr_u, sr_v):
    """Entraining CAPE per point (xp_ecape; include/xparcel.h has the formula): cape, ncape [J/kg], el_height [m above the
    lowest valid level: ncape()'s] and the storm-relative 0-1 km mean wind sr_u, sr_v [m/s], all of one shape.  Returns a dict
    of 'ecape' [J/kg], 'ecape_a' (ecape plus the inflow's kinetic energy) and 'psi' (the entrainment parameter, 1);
    NaN where an input is NaN or el_height <= 0."""
    return dict(zip(L.ECAPE_OUT, _per_point('xp_ecape', [cape, ncape, el_height, sr_u, sr_v], (), 3)))


def _in_space_of(x, ref):
    """A per-column argument (scalar, array or tensor) in the memory space and dtype of the per-column result `ref`."""
    if _is_torch(ref):
        x = x if _is_torch(x) else torch.as_tensor(np.asarray(x))
        return x.to(ref.device, ref.dtype)
    return np.asarray(x.detach().cpu().numpy() if _is_torch(x) else x, dtype=ref.dtype)


def ecape(pressure, temperature, dewpoint, height, u, v, parcel='most_unstable', depth=None, storm='right', storm_u=None,
          storm_v=None, moist=None, **cape_cin_options):
    """Entraining CAPE of every column from the sounding grid, end to end on the device (NumPy arrays are staged per call;
    CUDA tensors stay where they are): pressure [hPa], temperature, dewpoint [K], height [m], u, v [m/s] on one vertical,
    (nlev, ...).  The chain:
      1. cape_cin_columns for `parcel` ('surface', 'most_unstable', 'mixed_layer'; depth, moist and cape_cin_options as
         there): cape, cin, lfc_pressure, el_pressure;
      2. ncape between that LFC and EL;
      3. the storm motion: bunkers_storm_motion's `storm` = 'right', 'left' or 'mean' -- unless storm_u and storm_v (scalars
         or one value per column) are given;
      4. the 0-1 km inflow: wind_layers over 0 ... 1000 m above the lowest valid level -- its PRESSURE-WEIGHTED mean
         (metpy.calc.mean_pressure_weighted), not a plain average of the levels;
      5. sr_u, sr_v = that mean minus the storm motion;
      6. ecape_from_ncape.
    Returns a dict of per-column 'ecape', 'ecape_a', 'psi', 'ncape', 'cape', 'cin', 'lfc_height', 'el_height', 'sr_u', 'sr_v'
    and 'status': the OR of the status words of the calls above.  A column without an LFC has cape 0, ncape 0 and no EL
    height, hence NaN ecape, ecape_a and psi."""
    assert storm in ('right', 'left', 'mean'), "storm must be 'right', 'left' or 'mean'"
    assert (storm_u is None) == (storm_v is None), 'storm_u, storm_v: give both or neither'
    cc = cape_cin_columns(pressure, temperature, dewpoint, parcel=parcel, depth=depth, moist=moist,
                          want=('cape', 'cin', 'lfc_pressure', 'el_pressure', 'status'), **cape_cin_options)
    nc = ncape(pressure, temperature, dewpoint, height, cc['lfc_pressure'], cc['el_pressure'])
    status = cc['status'] | nc['status']
    if storm_u is None:
        bm = bunkers_storm_motion(pressure, u, v, height)
        storm_u, storm_v, status = bm[storm + '_u'], bm[storm + '_v'], status | bm['status']
    wl = wind_layers(pressure, u, v, height, [{'bottom_height': 0.0, 'top_height': 1000.0}], want=('mean_u', 'mean_v'))
    mean_u, mean_v = wl['mean_u'][0], wl['mean_v'][0]
    sr_u, sr_v = mean_u - _in_space_of(storm_u, mean_u), mean_v - _in_space_of(storm_v, mean_v)
    res = ecape_from_ncape(cc['cape'], nc['ncape'], nc['el_height'], sr_u, sr_v)
    res.update(ncape=nc['ncape'], cape=cc['cape'], cin=cc['cin'], lfc_height=nc['lfc_height'], el_height=nc['el_height'],
               sr_u=sr_u, sr_v=sr_v, status=status | wl['status'])
    return res


def conv_properties(dat, ignore_nans=False, moist=None):
    """pf.py:1951: the reference's convective-property bundle for a grid, ONE library call (xp_conv_properties): the
    q -> dewpoint step, the NaN mask, the fixed-level interpolations and the freezing / melting levels are one pass over
    the four grids, the three parcels' CAPE / CIN / lifted index three more, the rest one per-point kernel -- no array
    arithmetic on this side.  `dat`: mapping with pressure [hPa], temperature [K], specific_humidity [kg/kg],
    height_asl [m] (nlev, ...), wind_u, wind_v, wind_height_above_surface (nwind, ...), surface_wind_u, surface_wind_v
    (...): NumPy arrays (staged through the library) or torch CUDA tensors (in place).  Returns a dict of per-column
    arrays with the reference's variable names (positive_shear: bool)."""
    order = L.CONV_IN_VIEWS + ('surface_wind_u', 'surface_wind_v')
    c = _Call(*[dat[k] for k in order])
    h = dict(zip(order, c.ins))
    _same_shape(c.ins[:4], 'pressure, temperature, specific_humidity, height_asl must share a shape')
    wu = h['wind_u']
    assert wu.shape == h['wind_v'].shape == h['wind_height_above_surface'].shape and tuple(wu.shape[1:]) == c.hshape, 'wind arrays must be (nwind, ...) over the same points'
    views = [C.pointer(c.view(h[k])) for k in L.CONV_IN_VIEWS]
    assert int(np.prod(h['surface_wind_u'].shape)) == c.ncol and int(np.prod(h['surface_wind_v'].shape)) == c.ncol
    ci = L.ConvIn(*views, _ptr(h['surface_wind_u']), _ptr(h['surface_wind_v']))
    co, res = c.struct(L.ConvOut, L.CONV_OUT)
    c.run('xp_conv_properties', ci, _opts(moist=moist or _DEFAULT['moist']), int(bool(ignore_nans)), co)
    res['positive_shear'] = res['positive_shear'] != 0
    return res


def _on_device_once(bundle):
    """A bundle of ~25 launches given host arrays uploads them once, works on device-resident data and brings its results
    back as NumPy arrays."""
    @functools.wraps(bundle)
    def call(dat, *args, **kwargs):
        host_in = not any(_is_torch(v) and v.is_cuda for v in dat.values())
        if host_in and torch is not None and torch.cuda.is_available():
            dat = {k: torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).cuda() for k, v in dat.items()}
        out = bundle(dat, *args, **kwargs)
        return {k: (v.cpu().numpy() if _is_torch(v) else v) for k, v in out.items()} if host_in else out
    return call


@_on_device_once
def conv_properties_composed(dat, ignore_nans=False, moist=None):
    """The same bundle as a composition of the stand-alone calls plus array arithmetic (what conv_properties() was before
    xp_conv_properties existed): kept as the cross-check of the fused call (tests/test_gpu_indices.py)."""
    p, t, q = dat['pressure'], dat['temperature'], dat['specific_humidity']
    td = dewpoint_from_specific_humidity(p, t, q)
    xp = _ns(td)
    to = (lambda a: torch.as_tensor(np.asarray(a), device=td.device) if not _is_torch(a) else a) if _is_torch(td) else np.asarray
    p, t, q, z = to(p), to(t), to(q), to(dat['height_asl'])
    valid = ~(xp.isnan(td).any(0) | xp.isnan(p).any(0) | xp.isnan(t).any(0) | xp.isnan(q).any(0))
    out = {}
    # (lifted_index_at: pf.py:1722 on the lifted profile, in the same pass, instead of writing the profile and interpolating it)
    mu = cape_cin_columns(p, t, td, parcel='most_unstable', depth=250, lifted_index_at=500.0, moist=moist)
    out['mu_cape'], out['mu_cin'] = mu['cape'], mu['cin']
    e = 6.112 * xp.exp(17.67 * (mu['parcel_dewpoint'] - 273.15) / (mu['parcel_dewpoint'] - 29.65))
    w = L_EPS * e / (mu['parcel_pressure'] - e)                       # specific_humidity_from_dewpoint -> mixing ratio
    qs = w / (1.0 + w)
    out['mu_mixing_ratio'] = qs / (1.0 - qs)
    out['mu_lifted_index'] = mu['lifted_index']
    for depth in (100, 50):
        ml = cape_cin_columns(p, t, td, parcel='mixed_layer', depth=depth, lifted_index_at=500.0, moist=moist)
        out[f'mixed_{depth}_cape'], out[f'mixed_{depth}_cin'] = ml['cape'], ml['cin']
        out[f'mixed_{depth}_lifted_index'] = ml['lifted_index']
    # temperature, dewpoint and height at 850 / 700 / 500 hPa in ONE pass over the column: what deep_convective_index
    # (pf.py:1830), lapse_rate (pf.py:2102) and isobar_temperature (pf.py:2193) interpolate one launch at a time
    (t850, t700, t500), (td850, _, _), (_, z700, z500) = interp_levels(p, [t, td, z], [850.0, 700.0, 500.0], log=True)
    for pre in ('mu', 'mixed_100', 'mixed_50'):
        out[pre + '_dci'] = (t850 - 273.15) + (td850 - 273.15) - out[pre + '_lifted_index']
    out['lapse_rate_700_500'] = (t500 - t700) / (z500 / 1000 - z700 / 1000)
    out['temp_500'] = t500
    out['freezing_level'] = freezing_level_height(t, z)
    out['melting_level'], _ = melting_level_height(p, t, td, z)
    out.update(wind_shear(to(dat['surface_wind_u']), to(dat['surface_wind_v']), to(dat['wind_u']), to(dat['wind_v']),
                          to(dat['wind_height_above_surface'])))
    if not ignore_nans:
        for k in out:
            if k != 'positive_shear':
                out[k] = _where(valid, out[k], float('nan'))
            else:
                out[k] = out[k] & valid          # xarray's where() turns a masked boolean into NaN; here: False
    return out


@_on_device_once
def min_conv_properties(dat, moist=None):
    """pf.py:1873: the minimal bundle -- 100 hPa mixed-layer CAPE / CIN and lifted index, 700-500 hPa lapse rate, 500 hPa
    temperature, freezing and melting level, 0-6 km shear.  Same input mapping as conv_properties(); no NaN blanking
    (the reference has none here)."""
    p, t, z = dat['pressure'], dat['temperature'], dat['height_asl']
    td = dewpoint_from_specific_humidity(p, t, dat['specific_humidity'])
    ml = cape_cin_columns(p, t, td, parcel='mixed_layer', depth=100, lifted_index_at=500.0, moist=moist)
    (t700, t500), (z700, z500) = interp_levels(p, [t, z], [700.0, 500.0], log=True)      # pf.py:2102, 2193 in one pass
    out = {'mixed_100_cape': ml['cape'], 'mixed_100_cin': ml['cin'], 'mixed_100_lifted_index': ml['lifted_index'],
           'lapse_rate_700_500': (t500 - t700) / (z500 / 1000 - z700 / 1000), 'temp_500': t500,
           'freezing_level': freezing_level_height(t, z), 'melting_level': melting_level_height(p, t, td, z)[0]}
    out.update(wind_shear(dat['surface_wind_u'], dat['surface_wind_v'], dat['wind_u'], dat['wind_v'],
                          dat['wind_height_above_surface']))
    return out


def storm_proxies(dat):
    """pf.py:2323: hail / storm proxies (booleans) and SHIP from the output of conv_properties(), one per-point kernel
    (xp_storm_proxies)."""
    c = _Call(*[dat[k] for k in L.PROXIES_IN])
    n, shape = _flat(c.ins), c.ins[0].shape
    ps = c.array(dat['positive_shear'], np.int32).reshape(-1)
    assert int(np.prod(ps.shape)) == n, 'positive_shear does not match the other arrays'
    flags = {k: c.out(shape, np.int32) for k in L.PROXIES_OUT}
    ship = c.out(shape)
    c.run('xp_storm_proxies', n, c.xp_dtype, c.mem, L.ProxiesIn(*map(_ptr, c.ins), _ptr(ps)),
          L.ProxiesOut(*map(_ptr, flags.values()), _ptr(ship)))
    out = {k: f != 0 for k, f in flags.items()}
    # the reference's order of variables (pf.py:2395-2405): proxies, SHIP, the SHIP proxy
    return {**{k: out[k] for k in L.PROXIES_OUT[:8]}, 'ship': ship, 'proxy_SHIP_0.1': out['proxy_SHIP_0.1']}


def family_table():
    """The adiabat-family coefficient table of moist='family' as a (n_coef_rows, n_label_pieces) float64 array: rows are
    (x-piece, power of z, power of s), C-order (xp_family_table)."""
    lib = L.init()
    n1, n2 = C.c_int64(), C.c_int64()
    L.check(lib.xp_family_table(None, C.byref(n1), C.byref(n2)))
    out = np.empty((n1.value, n2.value), dtype=np.float64)
    L.check(lib.xp_family_table(out.ctypes.data, None, None))
    return out


def set_family_table(table):
    """Replace the adiabat-family table (xp_set_family_table)."""
    t = np.ascontiguousarray(table, dtype=np.float64)
    t = t.reshape(-1, t.shape[-1])
    L.check(L.init().xp_set_family_table(t.ctypes.data, *t.shape))
