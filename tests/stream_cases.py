"""One recipe per way into the library, for the stream, thread and device contract at the head of include/xparcel.h: shared by
the census on the CPU (tests/test_stream_cases_cpu.py) and the device tests (tests/test_gpu_streams.py).

A recipe is a name, the set of xp_* entry points it reaches and a function (grid, dtype, to_device) -> flat list of output
arrays.  The function takes its inputs out of `grid` (float64 NumPy arrays, see grid()), casts the floating ones to `dtype`,
hands EVERY array -- per-column arguments and masks included -- to `to_device` and calls numpy_api on what comes back, so the
caller decides where the inputs live: the identity gives a host call, an upload a device call, and the side-stream test returns
buffers it allocated beforehand.  Nothing but arrays from `to_device` and Python scalars that the library takes by value
reaches numpy_api: a Python scalar that numpy_api would have to upload (a scalar per-column argument) is a blocking copy and
has no place in a recipe.  Recipes are deterministic: the same arrays go through `to_device` in the same order on every run.

The shared grid is synth.columns(24, 1337, nan_fraction=0.1) -- six workgroups of 256, not a multiple of 64 -- with the
specific humidity and base heights of tests/hydrostatic_cases.py, hydrostatic heights and hashed winds.  The two persistent-
wavefront recipes bring their own grids, the smallest over the thresholds of persist() in csrc/xparcel.hip, and run in
float32 only (Recipe.dtypes)."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from oracle import thermo as O
from tests import hydrostatic_cases as HK
from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as xa
from xarray_parcel_amd import synth

NLEV, NCOL, SEED = 24, 1337, 20250718
NWIND = 12
BOTH = (np.float64, np.float32)
PERSIST_SURFACE = (8, 3 * 2 ** 18 + 77)          # family mode, surface parcel: persist() from 3 * 2^18 columns on
PERSIST_FUSED = (8, 2 ** 19 + 77)                # searching parcels and the fused kernel: from 2^19 columns on

Recipe = namedtuple('Recipe', 'name entries fn dtypes host grid')
RECIPES = {}


def recipe(name, entries, dtypes=BOTH, host=True, grid=(NLEV, NCOL)):
    """Register fn as recipe `name`.  host=False: the recipe only exists with device memory (the library rejects strided
    host views).  grid: the (nlev, ncol) of the grid it wants."""
    def deco(fn):
        assert name not in RECIPES
        RECIPES[name] = Recipe(name, frozenset(entries), fn, tuple(dtypes), host, grid)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def grid(seed=SEED, nlev=NLEV, ncol=NCOL):
    """The inputs of every recipe as float64 arrays (masks uint8): p, t, td (synth.columns with missing levels), q, base
    (tests/hydrostatic_cases.py), z (hydrostatic height above sea level of the same columns without their missing levels, so
    it is complete and strictly increasing), u, v (a hashed hodograph per column, NaN at some levels where t is), the
    (NWIND, ncol) wind grid of conv_properties with its surface winds, and the per-column / per-level odds and ends the
    primitives want.  Shared and left unchanged."""
    p, t, td = synth.columns(nlev, ncol, seed=seed, nan_fraction=0.1)
    _, tc, tdc = synth.columns(nlev, ncol, seed=seed, nan_fraction=0.0, saturate_some=True)
    w = synth.column_uniforms(ncol, seed + 4000)
    tv = tc * (1.0 + 0.608 * O.mixing_ratio(O.saturation_vapor_pressure(tdc), p))
    dz = synth.RD_OVER_G * 0.5 * (tv[1:] + tv[:-1]) * np.log(p[:-1] / p[1:])
    z = np.concatenate([np.zeros((1, ncol)), np.cumsum(dz, axis=0)]) + 1500.0 * w[9]
    zk = (z - z[0]) / 1000.0
    u = -10.0 + 20.0 * w[0] + (2.0 + 4.0 * w[1]) * zk + 4.0 * np.sin(zk * (0.5 + w[2]) + 6.28 * w[3])
    v = -10.0 + 20.0 * w[4] + (1.0 + 2.0 * w[5]) * np.sqrt(zk) + 4.0 * np.cos(zk * (0.5 + w[6]) + 6.28 * w[7])
    gap = np.isnan(t) & (w[8] < 0.5)
    u, v = np.where(gap, np.nan, u), np.where(gap, np.nan, v)
    k = np.arange(nlev, dtype=np.float64)[:, None]
    g = {'p': p, 't': t, 'td': td, 'q': HK.specific_humidity(p, td), 'base': HK.base_heights(ncol, seed), 'z': z, 'u': u, 'v': v,
         'wind_u': u[:NWIND], 'wind_v': v[:NWIND], 'wind_z': (z - z[0])[:NWIND] + 10.0,
         'sfc_u': -5.0 + 10.0 * w[0], 'sfc_v': -5.0 + 10.0 * w[4],
         'storm_u': -8.0 + 16.0 * w[2], 'storm_v': -8.0 + 16.0 * w[6],
         # a second profile that crosses t a few times, their difference, a level to insert, a pressure to look for
         'tb': tc + 3.0 * np.sin(1.3 * k + 6.28 * w[3]), 'level_p': p[3] - 0.4 * (p[3] - p[4]), 'level_t': t[3] - 1.0,
         'bound': 300.0 + 600.0 * w[1], 'at_p': p[6] * (0.9 + 0.2 * w[5]),
         'layer_bottom': p[2], 'layer_top': p[11],
         'mask': (np.arange((nlev - 1) * ncol).reshape(nlev - 1, ncol) % 5 != 0).astype(np.uint8),
         'zq': z[0] + np.array([-50.0, 10.0, 900.0, 5000.0, 40000.0])[:, None] * (0.5 + w[8]),
         # per-point composites: CAPE-like, mixing-ratio-like, ... values with a NaN here and there
         'cape': np.where(w[7] < 0.05, np.nan, 4000.0 * w[0]), 'cin': -300.0 * w[1], 'mixr': 4.0 + 16.0 * w[2],
         'lapse': 5.0 + 4.0 * w[3], 't500': 250.0 + 15.0 * w[4], 'shear': 40.0 * w[5], 'flh': 1500.0 + 3500.0 * w[6],
         'lcl_z': 2500.0 * w[7], 'srh': -100.0 + 500.0 * w[8], 'base_z': np.where(w[9] < 0.5, 0.0, 400.0 * w[9])}
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def big_grid(nlev, ncol, seed=SEED):
    p, t, td = synth.columns(nlev, ncol, seed=seed, nan_fraction=0.1)
    g = {'p': p, 't': t, 'td': td}
    for a in g.values():
        a.setflags(write=False)
    return g


def grid_of(r, seed=SEED):
    """The grid recipe r runs on."""
    return grid(seed) if r.grid == (NLEV, NCOL) else big_grid(*r.grid, seed=seed)


def cast(a, dtype):
    """A floating array in `dtype`; masks and integers as they are."""
    return np.array(a, dtype=dtype if a.dtype.kind == 'f' else a.dtype, order='C')          # always a fresh, writable copy


def take(g, dtype, dev, *names):
    return [dev(cast(g[n], dtype)) for n in names]


def flat(x):
    """Every array of a nested result, in a fixed order."""
    if x is None:
        return []
    if isinstance(x, dict):
        return [a for k in x for a in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in flat(y)]
    return [x]


# ---- xp_cape_cin and xp_cape_cin_multi: every multi-kernel path ------------------------------------------------------------
@recipe('cape_surface_exact', ['xp_cape_cin'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), moist='exact'))


@recipe('cape_surface_family', ['xp_cape_cin'])          # the flags scratch, the fast pass, the flagged RK4 pass
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), moist='family'))


@recipe('cape_surface_family_lean', ['xp_cape_cin'])     # the CAPE/CIN-only kernels
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), moist='family', want=('cape', 'cin')))


@recipe('cape_surface_table', ['xp_cape_cin'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), moist='table'))


@recipe('cape_most_unstable_family', ['xp_cape_cin'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), parcel='most_unstable', moist='family'))


@recipe('cape_mixed_layer_family', ['xp_cape_cin'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), parcel='mixed_layer', moist='family',
                                    lifted_index_at=500.0))


@recipe('cape_profile_most_unstable_exact', ['xp_cape_cin'])          # profile output, re-based
def _(g, dtype, dev):
    return flat(xa.most_unstable_cape_cin(*take(g, dtype, dev, 'p', 't', 'td'), moist='exact'))


@recipe('cape_profile_explicit_family', ['xp_cape_cin'])              # profile output, explicit parcel, family mode
def _(g, dtype, dev):
    p, t, td = take(g, dtype, dev, 'p', 't', 'td')
    pp, pt, ptd = (dev(cast(g[n][1], dtype)) for n in ('p', 't', 'td'))
    return flat(xa.cape_cin(p, t, td, pt, pp, ptd, moist='family'))


@recipe('cape_profile_table', ['xp_cape_cin'])
def _(g, dtype, dev):
    return flat(xa.mixed_layer_cape_cin(*take(g, dtype, dev, 'p', 't', 'td'), moist='table'))


@recipe('cape_specific_humidity', ['xp_cape_cin'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'q'), parcel='mixed_layer', moist='family',
                                    humidity='specific'))


@recipe('cape_densify', ['xp_cape_cin'], host=False)
def _(g, dtype, dev):
    """The raw ABI with a temperature view of other strides than the pressure's ((ncol, nlev)-major): k_densify and its three
    scratch arrays run before the family passes."""
    p, t, td = take(g, dtype, dev, 'p', 't', 'td')
    c = xa._Call(p, t, td)
    p, t, td = c.ins
    t_cols = t.t().contiguous()
    tv = L.View(t_cols.data_ptr(), c.xp_dtype, c.mem, c.nlev, c.ncol, 1, c.nlev)
    so, res = c.scalars(L.SCALAR_F + L.SCALAR_I, c.hshape)
    o = xa._opts(moist='family')
    c.run('xp_cape_cin', c.view(p), tv, c.view(td), L.Parcel(L.PARCEL['surface'], 0, 100.0, None, None, None), o, so, None)
    return flat(res) + [t_cols]


@recipe('multi_family', ['xp_cape_cin_multi'])           # one pass per parcel, back to back, shared flags
def _(g, dtype, dev):
    return flat(xa.cape_cin_multi(*take(g, dtype, dev, 'p', 't', 'td'), [('most_unstable', 300), ('mixed_layer', 100)],
                                  moist='family', lifted_index_at=500.0))


@recipe('multi_fused', ['xp_cape_cin_multi'])            # XP_OPT_FUSE_PARCELS: k_cape_cin_multi and the flagged passes
def _(g, dtype, dev):
    return flat(xa.cape_cin_multi(*take(g, dtype, dev, 'p', 't', 'td'), [('most_unstable', 300), ('mixed_layer', 100)],
                                  moist='family', fused=True))


@recipe('multi_three_exact', ['xp_cape_cin_multi'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_multi(*take(g, dtype, dev, 'p', 't', 'td'),
                                  [('most_unstable', 250), ('mixed_layer', 100), ('mixed_layer', 50)], moist='exact'))


@recipe('multi_table', ['xp_cape_cin_multi'])
def _(g, dtype, dev):
    return flat(xa.cape_cin_multi(*take(g, dtype, dev, 'p', 't', 'td'), ['surface', 'most_unstable'], moist='table',
                                  want=('cape', 'cin', 'status')))


@recipe('persistent_surface', ['xp_cape_cin'], dtypes=(np.float32,), grid=PERSIST_SURFACE)
def _(g, dtype, dev):
    return flat(xa.cape_cin_columns(*take(g, dtype, dev, 'p', 't', 'td'), moist='family', want=('cape', 'cin')))


@recipe('persistent_fused', ['xp_cape_cin_multi'], dtypes=(np.float32,), grid=PERSIST_FUSED)
def _(g, dtype, dev):
    return flat(xa.cape_cin_multi(*take(g, dtype, dev, 'p', 't', 'td'), [('most_unstable', 300), ('mixed_layer', 100)],
                                  moist='family', fused=True, want=('cape', 'cin')))


# ---- the component entry points ------------------------------------------------------------------------------------------
@recipe('lcl', ['xp_lcl'])
def _(g, dtype, dev):
    return flat(xa.lcl(*(dev(cast(g[n][0], dtype)) for n in ('p', 't', 'td'))))


@recipe('lapse', ['xp_dry_lapse', 'xp_moist_lapse'])
def _(g, dtype, dev):
    p, t0, p0 = dev(cast(g['p'], dtype)), dev(cast(g['t'][1], dtype)), dev(cast(g['p'][1], dtype))
    return [xa.dry_lapse(p, t0, p0), xa.dry_lapse(p, t0), xa.moist_lapse(p, t0, p0, moist='exact'),
            xa.moist_lapse(p, t0, p0, moist='table')]


@recipe('component_chain', ['xp_parcel_profile', 'xp_lfc_el', 'xp_cape_cin_base'])
def _(g, dtype, dev):
    """parcel_profile -> lfc_el -> cape_cin_base, each fed with the outputs of the one before."""
    p, t = take(g, dtype, dev, 'p', 't')
    pp, pt, ptd = (dev(cast(g[n][0], dtype)) for n in ('p', 't', 'td'))
    prof = xa.parcel_profile(p, pp, pt, ptd, moist='exact')
    le = xa.lfc_el(p, prof['temperature'], t, prof['lcl_pressure'], prof['lcl_temperature'])
    cc = xa.cape_cin_base(p, t, le['lfc_pressure'], le['el_pressure'], prof['temperature'])
    return flat([{k: a for k, a in prof.items() if k != 'pressure'}, le, cc])


@recipe('select_parcel', ['xp_select_parcel'])
def _(g, dtype, dev):
    ins = take(g, dtype, dev, 'p', 't', 'td')
    return flat([xa.most_unstable_parcel(*ins), xa.mixed_parcel(*ins, depth=50)])


@recipe('mixed_layer', ['xp_mixed_layer'])
def _(g, dtype, dev):
    p, t, td = take(g, dtype, dev, 'p', 't', 'td')
    return flat(xa.mixed_layer({'pressure': p, 'temperature': t, 'dewpoint': td}, depth=100))


@recipe('wet_bulb', ['xp_wet_bulb_temperature'])
def _(g, dtype, dev):
    ins = take(g, dtype, dev, 'p', 't', 'td')
    return [xa.wet_bulb_temperature(*ins, moist='exact'), xa.wet_bulb_temperature(*ins, moist='table')]


@recipe('downdraft_cape', ['xp_downdraft_cape'])
def _(g, dtype, dev):
    return flat(xa.downdraft_cape(*take(g, dtype, dev, 'p', 't', 'td'), moist='exact', want_profile=True))


@recipe('effective_layer_chain', ['xp_effective_inflow_layer', 'xp_storm_relative_helicity_layers'])
def _(g, dtype, dev):
    """The effective inflow layer and the helicity between its bounds, which stay on the device."""
    p, t, td, z, u, v, su, sv = take(g, dtype, dev, 'p', 't', 'td', 'z', 'u', 'v', 'storm_u', 'storm_v')
    eff = xa.effective_inflow_layer(p, t, td, z, moist='exact', want_candidates=True)
    srh = xa.storm_relative_helicity_layers(z, u, v, eff['base_height'], eff['top_height'], storm_u=su, storm_v=sv)
    # (shear_magnitude is numpy_api's own hypot of two outputs, NumPy's on the host and torch's on the device: not the library's)
    return flat([eff, {k: a for k, a in srh.items() if k != 'shear_magnitude'}])


@recipe('cape_layers', ['xp_cape_cin_layers'])
def _(g, dtype, dev):
    p, t, td, lb, lt = take(g, dtype, dev, 'p', 't', 'td', 'layer_bottom', 'layer_top')
    return flat(xa.cape_cin_layers(p, t, td, [{'bottom': lb, 'top': lt}, {'top': lt}], parcel='mixed_layer', moist='exact'))


@recipe('hail_growth_zone_cape', ['xp_cape_cin_layers', 'xp_crossing_level', 'xp_interp_level'])
def _(g, dtype, dev):
    return [xa.hail_growth_zone_cape(*take(g, dtype, dev, 'p', 't', 'td', 'z'), moist='table')]


@recipe('hail_growth_zone_thickness', ['xp_thermo_layers', 'xp_crossing_level', 'xp_interp_level'])
def _(g, dtype, dev):
    return flat(xa.hail_growth_zone_thickness(*take(g, dtype, dev, 'p', 't', 'z')))


@recipe('interp_level', ['xp_interp_level'])
def _(g, dtype, dev):
    p, t, at = take(g, dtype, dev, 'p', 't', 'at_p')
    return [xa.interp_level(p, t, at, log=True), xa.interp_level(p, t, at, log=False)]


@recipe('interp_levels', ['xp_interp_levels'])
def _(g, dtype, dev):
    p, t, td, z = take(g, dtype, dev, 'p', 't', 'td', 'z')
    return flat(xa.interp_levels(p, [t, td, z], [850.0, 700.0, 500.0], log=True))


@recipe('dewpoint_from_specific_humidity', ['xp_dewpoint_from_specific_humidity'])
def _(g, dtype, dev):
    return [xa.dewpoint_from_specific_humidity(*take(g, dtype, dev, 'p', 't', 'q'))]


@recipe('crossing_level', ['xp_crossing_level'])
def _(g, dtype, dev):
    return [xa.freezing_level_height(*take(g, dtype, dev, 't', 'z'))]


@recipe('mixing_ratio', ['xp_mixing_ratio'])
def _(g, dtype, dev):
    return [xa.mixing_ratio(*take(g, dtype, dev, 't', 'td', 'p'))]


def _conv_dat(g, dtype, dev):
    names = ('p', 't', 'q', 'z', 'wind_u', 'wind_v', 'wind_z', 'sfc_u', 'sfc_v')
    return dict(zip(L.CONV_IN_VIEWS + ('surface_wind_u', 'surface_wind_v'), take(g, dtype, dev, *names)))


@recipe('conv_properties_and_proxies', ['xp_conv_properties', 'xp_storm_proxies'])
def _(g, dtype, dev):
    """The bundle (about 25 launches and its stream-ordered scratch) and the proxies on its outputs."""
    cp = xa.conv_properties(_conv_dat(g, dtype, dev), moist='family')
    return flat([cp, xa.storm_proxies(cp)])


@recipe('conv_properties_composed', ['xp_dewpoint_from_specific_humidity', 'xp_cape_cin', 'xp_interp_levels', 'xp_crossing_level',
                                     'xp_wind_shear'])
def _(g, dtype, dev):
    return flat(xa.conv_properties_composed(_conv_dat(g, dtype, dev), moist='family'))


@recipe('wind_shear', ['xp_wind_shear'])
def _(g, dtype, dev):
    return flat(xa.wind_shear(*take(g, dtype, dev, 'sfc_u', 'sfc_v', 'wind_u', 'wind_v', 'wind_z'), shear_height=3000))


@recipe('per_point_composites', ['xp_significant_hail_parameter', 'xp_significant_tornado', 'xp_supercell_composite',
                                 'xp_significant_tornado_effective'])
def _(g, dtype, dev):
    x = dict(zip(('cape', 'cin', 'mixr', 'lapse', 't500', 'shear', 'flh', 'lcl_z', 'srh', 'base_z'),
                 take(g, dtype, dev, 'cape', 'cin', 'mixr', 'lapse', 't500', 'shear', 'flh', 'lcl_z', 'srh', 'base_z')))
    return [xa.significant_hail_parameter(x['cape'], x['mixr'], x['lapse'], x['t500'], x['shear'], x['flh']),
            xa.significant_tornado(x['cape'], x['lcl_z'], x['srh'], x['shear']),
            xa.supercell_composite(x['cape'], x['srh'], x['shear']),
            xa.significant_tornado_effective(x['cape'], x['cin'], x['lcl_z'], x['srh'], x['shear']),
            xa.significant_tornado_effective(x['cape'], x['cin'], x['lcl_z'], x['srh'], x['shear'], x['base_z'])]


@recipe('storm_motion_chain', ['xp_bunkers_storm_motion', 'xp_storm_relative_helicity'])
def _(g, dtype, dev):
    """Bunkers' right mover straight back in as the storm motion of the helicity."""
    p, u, v, z, su, sv = take(g, dtype, dev, 'p', 'u', 'v', 'z', 'sfc_u', 'sfc_v')
    bm = xa.bunkers_storm_motion(p, u, v, z)
    srh = xa.storm_relative_helicity(z, u, v, [1000.0, 3000.0], storm_u=bm['right_u'], storm_v=bm['right_v'])
    sfc = xa.storm_relative_helicity(z - z[0], u, v, 1000.0, storm_u=bm['left_u'], storm_v=bm['left_v'], surface_u=su, surface_v=sv)
    return flat([bm, srh, sfc])


@recipe('wind_layers', ['xp_wind_layers'])
def _(g, dtype, dev):
    return flat(xa.wind_layers(*take(g, dtype, dev, 'p', 'u', 'v', 'z'),
                               layers=[{'bottom': 850.0, 'top': 300.0}, {'depth': 100.0}, {'bottom_height': 0.0, 'top_height': 6000.0}]))


@recipe('thermo_layers', ['xp_thermo_layers'])
def _(g, dtype, dev):
    p, t, td, z, lb, lt = take(g, dtype, dev, 'p', 't', 'td', 'z', 'layer_bottom', 'layer_top')
    return flat(xa.thermo_layers(p, t, td, z, layers=[{'bottom': 700.0, 'top': 500.0}, {'bottom': None, 'top': None},
                                                      {'bottom_height': 0.0, 'top_height': 3000.0}, {'bottom': lb, 'top': lt}]))


@recipe('theta_e_difference', ['xp_thermo_layers'])
def _(g, dtype, dev):
    return [xa.theta_e_difference(*take(g, dtype, dev, 'p', 't', 'td', 'z'))]


@recipe('sounding_indices', ['xp_sounding_indices'])
def _(g, dtype, dev):
    ins = take(g, dtype, dev, 'p', 't', 'td', 'u', 'v')
    return flat([xa.sounding_indices(*ins, moist='exact'), xa.ccl(*ins[:3], mixed_layer_depth=50.0, which='bottom')])


@recipe('isentropic_interpolation', ['xp_isentropic_interpolation'])
def _(g, dtype, dev):
    p, t, u = take(g, dtype, dev, 'p', 't', 'u')
    return flat(xa.isentropic_interpolation([300.0, 310.0, 330.0, 360.0], p, t, u, temperature_out=True, status=True))


@recipe('hydrostatic', ['xp_hydrostatic_height'])
def _(g, dtype, dev):
    p, t, td, q, base = take(g, dtype, dev, 'p', 't', 'td', 'q', 'base')
    return flat([xa.hydrostatic(p, t, dewpoint=td, base_height=base, layers=HK.API_LAYERS),
                 xa.hydrostatic(p, t, specific_humidity=q, layers=HK.API_LAYERS[:2]), xa.hydrostatic_height(p, t)])


@recipe('geopotential', ['xp_height_to_geopotential', 'xp_geopotential_to_height'])
def _(g, dtype, dev):
    phi = xa.height_to_geopotential(dev(cast(g['z'], dtype)))
    return [phi, xa.geopotential_to_height(phi)]


@recipe('critical_angle', ['xp_wind_layers', 'xp_critical_angle'])
def _(g, dtype, dev):
    return [xa.critical_angle(*take(g, dtype, dev, 'p', 'u', 'v', 'z', 'storm_u', 'storm_v'))]


@recipe('corfidi_storm_motion', ['xp_wind_layers', 'xp_corfidi_storm_motion'])
def _(g, dtype, dev):
    p, u, v, ju, jv = take(g, dtype, dev, 'p', 'u', 'v', 'sfc_u', 'sfc_v')
    return flat([xa.corfidi_storm_motion(p, u, v), xa.corfidi_storm_motion(p, u, v, llj_u=ju, llj_v=jv)])


@recipe('ecape', ['xp_cape_cin', 'xp_ncape', 'xp_bunkers_storm_motion', 'xp_wind_layers', 'xp_ecape'])
def _(g, dtype, dev):
    """The longest chain: five calls, each on the outputs of the ones before."""
    return flat(xa.ecape(*take(g, dtype, dev, 'p', 't', 'td', 'z', 'u', 'v'), moist='family'))


# ---- the reference's array primitives --------------------------------------------------------------------------------------
@recipe('insert_level', ['xp_insert_level'])
def _(g, dtype, dev):
    p, t, lp, lt = take(g, dtype, dev, 'p', 't', 'level_p', 'level_t')
    return flat(xa.insert_level({'pressure': p, 'temperature': t}, {'pressure': lp, 'temperature': lt}))


@recipe('find_intersections', ['xp_find_intersections'])
def _(g, dtype, dev):
    p, t, tb = take(g, dtype, dev, 'p', 't', 'tb')
    return flat([xa.find_intersections(p, t, tb, log_x=True), xa.find_intersections(p, t - tb)])


@recipe('trapz', ['xp_trapz'])
def _(g, dtype, dev):
    p, t, tb, mask = take(g, dtype, dev, 'p', 't', 'tb', 'mask')
    return [xa.trapz(t - tb, p), xa.trapz(t - tb, p, mask=mask, only_positive=True)]


@recipe('trap_around_zeros', ['xp_trap_around_zeros'])
def _(g, dtype, dev):
    p, t, tb = take(g, dtype, dev, 'p', 't', 'tb')
    return flat(xa.trap_around_zeros(p, t - tb))


@recipe('bound_pressure', ['xp_bound_pressure'])
def _(g, dtype, dev):
    return [xa.bound_pressure(*take(g, dtype, dev, 'p', 'bound'))]


@recipe('get_layer', ['xp_get_layer'])
def _(g, dtype, dev):
    p, t = take(g, dtype, dev, 'p', 't')
    return flat([xa.get_layer({'pressure': p, 'temperature': t}, depth=100), xa.get_layer({'pressure': p}, depth=300, interpolate=False)])


@recipe('shift_out_nans', ['xp_shift_out_nans'])
def _(g, dtype, dev):
    p, t = take(g, dtype, dev, 'p', 't')
    return flat(xa.shift_out_nans({'temperature': t, 'pressure': p}, 'temperature'))


@recipe('rebase_most_unstable', ['xp_rebase_profile'])
def _(g, dtype, dev):
    return flat(xa.from_most_unstable_parcel(*take(g, dtype, dev, 'p', 't', 'td')))


@recipe('rebase_mixed_layer', ['xp_rebase_profile'])
def _(g, dtype, dev):
    return flat(xa.mix_layer(*take(g, dtype, dev, 'p', 't', 'td')))


@recipe('interp1d', ['xp_interp1d'])
def _(g, dtype, dev):
    return [xa.interp1d(*take(g, dtype, dev, 'zq', 'z', 't'))]


# Recipes whose library call synchronises the stream although its buffers live on the device, with the header's own words.
_REBASE = 'xp_rebase_profile: "*nlev_out (HOST) = rows in use.  Synchronises the stream." (include/xparcel.h)'
SYNCHRONISES = {
    'rebase_most_unstable': _REBASE,
    'rebase_mixed_layer': _REBASE,
    # Not the library's own wait: a call that takes stream-ordered scratch (family mode's flags) straight after another one,
    # while the stream is still busy, gets the block the first call released back from hipMallocAsync, and the HIP runtime's
    # hipFreeAsync of a block recycled before its earlier release has executed waits for the stream.  Measured with the
    # runtime alone on an MI355X: malloc 5348 B, free, malloc 5348 B (the same block), free behind a 100 ms delay -- the last
    # free took 99.96 ms, with 1 MiB for the second allocation (another block) 0.002 ms.  Of the recipes only this chain makes
    # two such calls in a row (most-unstable, then two mixed-layer parcels in family mode).
    'conv_properties_composed': 'the second family-mode xp_cape_cin in a row: hipFreeAsync of a scratch block that hipMallocAsync '
                                'recycled from a release still pending on the stream waits for the stream (HIP runtime)',
}
# Entry points that take a stream and have no recipe, each with its reason.  Meant to stay empty.
EXEMPT = {}

# (b) host buffers on a side stream: one recipe per translation unit of the library, the per-point and the primitive paths
HOST_SUBSET = ('cape_surface_family', 'cape_profile_table', 'cape_surface_exact',       # xp_cape_tu.hip, modes 2, 1, 0
               'multi_fused',                                                           # xp_multi_tu.hip
               'effective_layer_chain', 'wind_layers', 'thermo_layers', 'cape_layers',  # their own units; xparcel.hip's helicity
               'ecape', 'sounding_indices', 'isentropic_interpolation', 'hydrostatic',  # xp_ecape_tu.hip ... xp_hydrostatic_tu.hip
               'conv_properties_and_proxies', 'per_point_composites', 'geopotential',   # xparcel.hip: the bundle, per-point kernels
               'trapz', 'insert_level', 'rebase_mixed_layer', 'interp1d')               # xp_primitives_abi.hpp
# (c) four threads on four streams: the multi-kernel recipes and a handful of single-kernel ones
THREAD_RECIPES = ('cape_surface_family', 'cape_surface_table', 'multi_family', 'multi_fused', 'cape_densify',
                  'conv_properties_and_proxies', 'ecape', 'effective_layer_chain', 'component_chain',
                  'lcl', 'wind_layers', 'trapz', 'hydrostatic', 'per_point_composites')
PERSISTENT = ('persistent_surface', 'persistent_fused')
# (e) another current device: a column kernel, a per-point product, a chain
OTHER_DEVICE_RECIPES = ('cape_surface_family', 'per_point_composites', 'ecape')


def header_stream_entries(path=L.INCLUDE):
    """The functions include/xparcel.h declares with `void *stream` as their last parameter."""
    import re
    with open(path) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    found = re.findall(r'\bint\s+(xp_\w+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S)
    return {name for name, params in found if re.search(r'\bvoid\s*\*\s*stream\s*$', params.strip())}
