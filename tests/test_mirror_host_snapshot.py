"""CPU snapshot of the xarray mirror (xarray_parcel_amd/parcel_functions.py and the feature modules next to it) around the
array API, and of what the array API hands the library.

The launch (`numpy_api._Call.run`) only records and every output the API allocates (`_Call.out`) is filled with a
pattern keyed on the number of outputs that call has allocated so far.  The mirror then runs to the end on a machine
without a GPU, and what it does around the API is recorded: every numpy_api call it makes (name, array arguments with
dtype, shape and values, scalar and keyword arguments), every launch under it (the entry point and its arguments as they
reach the ABI: scalars by value, arrays as dtype, shape and a digest, ctypes structures field by field, every pointer as
"array k of this call, byte offset") and what the mirror returns (types, names, dims, coords, attrs, dtypes, shapes,
values).  The recordings are tests/golden/mirror_host_snapshot.json (parcel_functions.py: its numpy_api calls and results)
and mirror_host_snapshot_features.json (the launches of those cases, and everything of the feature modules' cases, kept
short: an array of more than six elements, and the attrs and coords of a DataArray, as digests); `python -m tests.test_mirror_host_snapshot` rewrites
them.  Not covered here: the table generators (moist_adiabat_lookup, moist_adiabat_tables, load_moist_adiabat_lookups), which compute
on the device and use none of the DataArray plumbing."""
import ctypes as C
import functools
import hashlib
import inspect
import json
import os

import numpy as np
import pytest

from xarray_parcel_amd import _lib as L
from xarray_parcel_amd import numpy_api as api
from xarray_parcel_amd import parcel_functions as pf
from xarray_parcel_amd import (downdraft, entrainment, ground, hydrostatic, isentropic, kinematics, layer_cape,
                               sounding_indices, thermo_layers)
from xarray_parcel_amd._xr import DataArray, Dataset

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = os.path.join(_GOLDEN_DIR, 'mirror_host_snapshot.json')
GOLDEN_FEATURES = os.path.join(_GOLDEN_DIR, 'mirror_host_snapshot_features.json')
FEATURE_MODULES = (kinematics, thermo_layers, layer_cape, hydrostatic, entrainment, sounding_indices, isentropic, downdraft,
                   ground)
VD = 'model_level_number'
NOT_RECORDED = {'moist_adiabat_lookup', 'moist_adiabat_tables', 'load_moist_adiabat_lookups',   # device table generators
                'set_moist_lapse', 'lookup_tables_loaded'}                                     # test_table_asserts

# -- inputs: 5 levels, one column or a 2 x 3 grid ------------------------------------------------------------------------
P = np.array([1000., 925., 850., 700., 500.])
T = np.array([300., 295., 290., 282., 265.])
TD = np.array([295., 290., 283., 270., 250.])
Z = np.array([100., 800., 1500., 3000., 5500.])
Q = np.array([16., 13., 10., 6., 2.]) / 1000
OFF = np.arange(6.).reshape(2, 3) / 2
HC = {'lat': [10., 20.], 'lon': [1., 2., 3.]}


def col(v, name=None, coord=True, dtype=np.float64):
    """One column on VD (coordinate 1..5 unless coord=False)."""
    return DataArray(np.asarray(v, dtype=dtype), dims=(VD,), coords={VD: np.arange(1, 6)} if coord else None,
                     attrs={'units': 'x'}, name=name)


def grid(v, name=None, vdim=VD):
    """(lat, vdim, lon): the vertical between the horizontal dims, as in test_grid_dims_are_preserved."""
    return DataArray(v[None, :, None] + OFF[:, None, :], dims=('lat', vdim, 'lon'),
                     coords={**HC, vdim: np.arange(1, 6)}, attrs={'units': 'g'}, name=name)


def horiz(v, name=None):
    """A per-point field on (lat, lon)."""
    return DataArray(v + OFF, dims=('lat', 'lon'), coords=HC, attrs={'units': 'h'}, name=name)


def named(mk):
    return mk(P, 'pressure'), mk(T, 'temperature'), mk(TD, 'dewpoint')


def bundle():
    return Dataset({'pressure': grid(P), 'temperature': grid(T), 'specific_humidity': grid(Q), 'height_asl': grid(Z),
                    'wind_u': grid(np.arange(5.), vdim='wind_level'), 'wind_v': grid(-np.arange(5.), vdim='wind_level'),
                    'wind_height_above_surface': grid(Z - 100, vdim='wind_level'),
                    'surface_wind_u': horiz(1.0), 'surface_wind_v': horiz(-1.0)})


def profile():
    return Dataset({'pressure': grid(P, 'pressure'), 'temperature': grid(T - 1, 'temperature'),
                    'virtual_temperature': grid(T + 1, 'virtual_temperature'),
                    'environment_temperature': grid(T, 'environment_temperature'),
                    'lcl_pressure': horiz(900., 'lcl_pressure'), 'lcl_temperature': horiz(288., 'lcl_temperature'),
                    'lcl_virtual_temperature': horiz(289., 'lcl_virtual_temperature')})


def env():
    return Dataset({'pressure': grid(P, 'pressure'), 'temperature': grid(T, 'temperature'),
                    'dewpoint': grid(TD, 'dewpoint'), 'virtual_temperature': grid(T + 2, 'virtual_temperature')})


def ptd(surface=True):
    """pressure, temperature, dewpoint and (surface=True) a variable without the vertical."""
    ds = Dataset({'pressure': grid(P, 'pressure'), 'temperature': grid(T, 'temperature'), 'dewpoint': grid(TD, 'dewpoint')})
    if surface:
        ds['surface'] = horiz(5.0, 'surface')
    return ds


PV = (np.full((2, 3), 990.), np.full((2, 3), 299.), np.full((2, 3), 293.))
AT = np.linspace(520., 980., 4)

# name 'function' or 'function:variant' -> the call
CASES = {
    # drivers
    'surface_based_cape_cin:grid': lambda: pf.surface_based_cape_cin(grid(P), grid(T), grid(TD)),
    'surface_based_cape_cin:column_prefix': lambda: pf.surface_based_cape_cin(
        col(P), col(T), col(TD), prefix='sb', virtual_temperature_correction=False, lcl_interp='linear'),
    'surface_based_cape_cin:no_vert_coord': lambda: pf.surface_based_cape_cin(
        col(P, coord=False), col(T, coord=False), col(TD, coord=False)),
    'surface_based_cape_cin:f32_dataarray': lambda: pf.surface_based_cape_cin(
        col(P, dtype=np.float32), col(T, dtype=np.float32), col(TD, dtype=np.float32)),
    'surface_based_cape_cin:f32_ndarray': lambda: pf.surface_based_cape_cin(
        P.astype(np.float32), T.astype(np.float32), TD.astype(np.float32)),
    'cape_cin:grid': lambda: pf.cape_cin(grid(P), grid(T), grid(TD), PV[1], PV[0], PV[2], moist='family'),
    'most_unstable_cape_cin:column': lambda: pf.most_unstable_cape_cin(*named(col), depth=200, prefix='mu'),
    'most_unstable_cape_cin:grid': lambda: pf.most_unstable_cape_cin(*named(grid)),
    'mixed_layer_cape_cin:column': lambda: pf.mixed_layer_cape_cin(*named(col), prefix='ml'),
    'mixed_layer_cape_cin:grid': lambda: pf.mixed_layer_cape_cin(*named(grid), depth=50, lcl_interp='linear'),
    # column algorithms
    'lcl:grid': lambda: pf.lcl(horiz(990.), horiz(299.), PV[2]),
    'lcl:scalars': lambda: pf.lcl(1000., 300., 290.),
    'dry_lapse:grid': lambda: pf.dry_lapse(grid(P), PV[1], parcel_pressure=horiz(990.)),
    'dry_lapse:column': lambda: pf.dry_lapse(col(P), np.array([300.])),
    'moist_lapse:grid': lambda: pf.moist_lapse(grid(P), horiz(299.), parcel_pressure=PV[0]),
    'moist_lapse:column_table': lambda: pf.moist_lapse(col(P), np.array([300.]), moist='table'),
    'parcel_profile:column': lambda: pf.parcel_profile(col(P), 1000., 300., 295.),
    'parcel_profile:grid': lambda: pf.parcel_profile(grid(P), *PV, moist='family'),
    'parcel_profile_with_lcl:grid': lambda: pf.parcel_profile_with_lcl(grid(P), grid(T), grid(TD), *PV, lcl_interp='linear'),
    'lfc_el:grid': lambda: pf.lfc_el(grid(P), grid(T + 3), grid(T), horiz(900.), PV[1]),
    'cape_cin_base:grid': lambda: pf.cape_cin_base(grid(P), grid(T), horiz(850.), PV[0] - 500, grid(T + 3),
                                                   pos_cape_neg_cin=False, post_zero_cin=True),
    'most_unstable_parcel:grid': lambda: pf.most_unstable_parcel(ptd(False), depth=250),
    'mixed_parcel:grid': lambda: pf.mixed_parcel(*named(grid), depth=50),
    'mixed_layer:grid': lambda: pf.mixed_layer(ptd(False)),
    'wet_bulb_temperature:grid': lambda: pf.wet_bulb_temperature(grid(P), grid(T), grid(TD)),
    'wet_bulb_temperature:no_vertical': lambda: pf.wet_bulb_temperature(horiz(900.), horiz(290.), horiz(285.)),
    'log_interp:dataarray': lambda: pf.log_interp(grid(T, 'temperature'), grid(P), 500.),
    'log_interp:dataset': lambda: pf.log_interp(env(), grid(P), horiz(600.)),
    'linear_interp:no_attrs': lambda: pf.linear_interp(grid(T, 'temperature'), grid(P), 600., keep_attrs=False),
    'lifted_index:grid': lambda: pf.lifted_index(profile()),
    'lifted_index:prefix': lambda: pf.lifted_index(profile(), description='500 hPa', prefix='mu'),
    'mixing_ratio:dataarray': lambda: pf.mixing_ratio(grid(T), grid(TD), grid(P)),
    'mixing_ratio:ndarray': lambda: pf.mixing_ratio(T, TD, P),
    'virtual_temperature:dataarray': lambda: pf.virtual_temperature(grid(T), 0.01),
    'virtual_temperature:ndarray': lambda: pf.virtual_temperature(T, 0.01),
    'wet_bulb_temperature_fast:grid': lambda: pf.wet_bulb_temperature_fast(grid(T, 'temperature'), grid(TD)),
    'deep_convective_index:grid': lambda: pf.deep_convective_index(grid(P), grid(T), grid(TD), horiz(-2.)),
    'deep_convective_index:prefix': lambda: pf.deep_convective_index(grid(P), grid(T), grid(TD), PV[0] / 100,
                                                                     description='d', prefix='mu'),
    'lapse_rate:grid': lambda: pf.lapse_rate(grid(P), grid(T), grid(Z), from_pressure=850, to_pressure=500),
    'lapse_rate:f32_dataarray': lambda: pf.lapse_rate(col(P, dtype=np.float32), col(T, dtype=np.float32),
                                                      col(Z, dtype=np.float32)),
    'lapse_rate:f32_ndarray': lambda: pf.lapse_rate(P.astype(np.float32), T.astype(np.float32), Z.astype(np.float32)),
    'freezing_level_height:grid': lambda: pf.freezing_level_height(grid(T), grid(Z)),
    'melting_level_height:fast': lambda: pf.melting_level_height(grid(P), grid(T), grid(TD), grid(Z)),
    'melting_level_height:slow': lambda: pf.melting_level_height(grid(P), grid(T), grid(TD), grid(Z), fast=False),
    'isobar_temperature:grid': lambda: pf.isobar_temperature(grid(P), grid(T), 700),
    'dewpoint_from_specific_humidity:grid': lambda: pf.dewpoint_from_specific_humidity(grid(P), grid(T), grid(Q)),
    'dewpoint_from_specific_humidity:no_vertical': lambda: pf.dewpoint_from_specific_humidity(
        horiz(900.), horiz(290.), horiz(0.01)),
    # product bundle
    'wind_shear:grid': lambda: pf.wind_shear(horiz(1.), PV[0] / 1000, grid(np.arange(5.), vdim='wind_level'),
                                             grid(-np.arange(5.), vdim='wind_level'), grid(Z, vdim='wind_level'),
                                             shear_height=3000, vert_dim='wind_level'),
    'significant_hail_parameter:dataarray': lambda: pf.significant_hail_parameter(
        horiz(2000.), horiz(12.), horiz(7.), horiz(-15.), horiz(25.), horiz(3500.)),
    'significant_hail_parameter:ndarray': lambda: pf.significant_hail_parameter(*(np.full(3, v) for v in (
        2000., 12., 7., -15., 25., 3500.))),
    'valid_data:dataset': lambda: pf.valid_data(Dataset({'pressure': grid(P), VD: DataArray(np.arange(1, 6), dims=(VD,))}),
                                                VD),
    'conv_properties:grid': lambda: pf.conv_properties(bundle()),
    'conv_properties:ignore_nans': lambda: pf.conv_properties(bundle(), ignore_nans=True, moist='family'),
    'min_conv_properties:grid': lambda: pf.min_conv_properties(bundle()),
    'storm_proxies:grid': lambda: pf.storm_proxies(pf.conv_properties(bundle())),
    # array primitives
    'round_to:array': lambda: pf.round_to(np.array([1.2345, 273.149]), 0.02),
    'interp1d_numba:grid': lambda: pf.interp1d_numba(np.broadcast_to(AT, (2, 3, 4)), P[::-1] + OFF[..., None],
                                                     T[::-1] + OFF[..., None]),
    'interp1d_numba:shared_xp': lambda: pf.interp1d_numba(AT, P[::-1], np.stack([T[::-1], TD[::-1]])),
    'interp1d_numba:out': lambda: pf.interp1d_numba(np.broadcast_to(AT, (3, 4)), P[::-1], T[::-1], out=np.zeros((3, 4))),
    'bound_pressure:grid': lambda: pf.bound_pressure(grid(P, 'pressure'), horiz(700.)),
    'bound_pressure:scalar': lambda: pf.bound_pressure(col(P), 650.),
    'get_layer:grid': lambda: pf.get_layer(ptd(), depth=100),
    'get_layer:no_interpolate': lambda: pf.get_layer(ptd(), depth=300, interpolate=False),
    'insert_level:grid': lambda: pf.insert_level(
        ptd(), Dataset({'pressure': horiz(800.), 'temperature': horiz(285.), 'dewpoint': horiz(280.)}), 'pressure'),
    'find_intersections:grid': lambda: pf.find_intersections(grid(P), grid(T), grid(TD), VD, log_x=True),
    'trapz:grid': lambda: pf.trapz(ptd(), 'pressure', VD),
    'trapz:mask': lambda: pf.trapz(ptd(), 'pressure', VD, mask=grid(np.array([1., 0, 1, 0, 1])), only_positive=True),
    'trapz:ndarray_mask': lambda: pf.trapz(ptd(), 'pressure', VD, mask=np.array([1, 0, 1, 0, 1]).reshape(5, 1, 1),
                                           only_negative=True),
    'trap_around_zeros:grid': lambda: pf.trap_around_zeros(grid(P), grid(T - TD - 5), VD, log_x=False),
    'shift_out_nans:grid': lambda: pf.shift_out_nans(ptd(), 'pressure', VD),
    'from_most_unstable_parcel:grid': lambda: pf.from_most_unstable_parcel(*named(grid), depth=200),
    'mix_layer:grid': lambda: pf.mix_layer(*named(grid)),
    'add_lcl_to_profile:environment': lambda: pf.add_lcl_to_profile(profile(), environment=env(), interpolator='linear'),
    'add_lcl_to_profile:plain': lambda: pf.add_lcl_to_profile(profile()),
}

# -- the feature modules: 'module.function:variant' ----------------------------------------------------------------------
U = np.arange(5.)
K, TL, LC, HY, EN, SI, IS, DD, GR = FEATURE_MODULES


def sfc():
    """Surface pressure, 2 m temperature and 2 m dewpoint on (lat, lon)."""
    return horiz(990.), horiz(299.), horiz(293.)


def ptz(mk=grid):
    return mk(P), mk(T), mk(TD), mk(Z)


def puv(mk=grid):
    return mk(P), mk(U), mk(-U)


def zuv(mk=grid):
    return mk(Z), mk(U), mk(-U)


FEATURE_CASES = {
    # kinematics: per-column arguments as DataArrays, scalars and None; one layer and several; a grid without horizontal dims
    'kinematics.bunkers_storm_motion:grid': lambda: K.bunkers_storm_motion(*puv(), grid(Z)),
    'kinematics.storm_relative_helicity:depths': lambda: K.storm_relative_helicity(
        *zuv(), [1000., 3000.], storm_u=horiz(1.), storm_v=2.0),
    'kinematics.storm_relative_helicity:column_surface': lambda: K.storm_relative_helicity(
        *zuv(col), 3000., bottom=100., surface_u=1.0, surface_v=-1.0),
    'kinematics.storm_relative_helicity:grid_surface': lambda: K.storm_relative_helicity(
        *zuv(), 1000., surface_u=horiz(1.), surface_v=horiz(-1.)),
    'kinematics.effective_inflow_layer:candidates': lambda: K.effective_inflow_layer(*ptz(), want_candidates=True),
    'kinematics.effective_inflow_layer:column_no_height': lambda: K.effective_inflow_layer(
        col(P), col(T), col(TD), cape_min=50., moist='family', lcl_interp='linear'),
    'kinematics.storm_relative_helicity_layers:tops': lambda: K.storm_relative_helicity_layers(
        *zuv(), horiz(0.), [horiz(1000.), 3000.], storm_u=horiz(1.), surface_u=horiz(1.), surface_v=1.0),
    'kinematics.storm_relative_helicity_layers:one_top': lambda: K.storm_relative_helicity_layers(*zuv(), 0., horiz(3000.)),
    'kinematics.significant_tornado:dataarray': lambda: K.significant_tornado(horiz(2000.), horiz(800.), horiz(150.), horiz(20.)),
    'kinematics.supercell_composite:dataarray': lambda: K.supercell_composite(horiz(2000.), horiz(150.), horiz(20.)),
    'kinematics.wind_layers:layers': lambda: K.wind_layers(*puv(), grid(Z), layers=[{'bottom': 850, 'top': 300},
                                                                                    {'top_height': 3000}]),
    'kinematics.wind_layers:column_no_height': lambda: K.wind_layers(*puv(col), layers=[{'depth': 100}]),
    'kinematics.mean_pressure_weighted:pressure': lambda: K.mean_pressure_weighted(*puv()),
    'kinematics.mean_pressure_weighted:height': lambda: K.mean_pressure_weighted(*puv(), grid(Z), bottom=0., depth=1000.),
    'kinematics.bulk_shear:pressure': lambda: K.bulk_shear(*puv(), bottom=900., depth=300.),
    'kinematics.bulk_shear:height': lambda: K.bulk_shear(*puv(), grid(Z), bottom=500., depth=2500.),
    'kinematics.critical_angle:grid': lambda: K.critical_angle(*puv(), grid(Z), horiz(1.), 2.0),
    'kinematics.corfidi_storm_motion:default': lambda: K.corfidi_storm_motion(*puv()),
    'kinematics.corfidi_storm_motion:llj': lambda: K.corfidi_storm_motion(*puv(), llj_u=horiz(5.), llj_v=1.0),
    'kinematics.significant_tornado_effective:base_height': lambda: K.significant_tornado_effective(
        horiz(2000.), horiz(-20.), horiz(800.), horiz(150.), horiz(20.), base_height=horiz(0.)),
    'kinematics.significant_tornado_effective:no_base': lambda: K.significant_tornado_effective(
        horiz(2000.), horiz(-20.), horiz(800.), horiz(150.), horiz(20.)),
    # thermo_layers: absent views, bounds per column, by scalar and None, dict and tuple layers
    'thermo_layers.thermo_layers:layers': lambda: TL.thermo_layers(*ptz(), layers=[
        {'bottom': horiz(900.), 'top': 500}, {'depth': 100}, ('pressure', None, horiz(600.)), {'top_height': 3000}]),
    'thermo_layers.thermo_layers:want_no_views': lambda: TL.thermo_layers(
        grid(P), dewpoint=grid(TD), layers=[{'bottom': None, 'top': None}], want=('precipitable_water',)),
    'thermo_layers.thermo_layers:column': lambda: TL.thermo_layers(col(P), col(T), col(TD), layers=[{'bottom': 900, 'top': 600}]),
    'thermo_layers.precipitable_water:default': lambda: TL.precipitable_water(grid(P), grid(TD)),
    'thermo_layers.precipitable_water:bounds': lambda: TL.precipitable_water(grid(P), grid(TD), bottom=horiz(950.), top=600.),
    'thermo_layers.mean_relative_humidity:default': lambda: TL.mean_relative_humidity(grid(P), grid(T), grid(TD)),
    'thermo_layers.mean_relative_humidity:height_layer': lambda: TL.mean_relative_humidity(
        *ptz(), layer={'bottom_height': 0, 'top_height': 3000}),
    'thermo_layers.layer_lapse_rate:default': lambda: TL.layer_lapse_rate(grid(P), grid(T), grid(Z)),
    'thermo_layers.layer_lapse_rate:per_column': lambda: TL.layer_lapse_rate(grid(P), grid(T), grid(Z),
                                                                           layer=('pressure', horiz(900.), 500.)),
    'thermo_layers.hail_growth_zone_thickness:grid': lambda: TL.hail_growth_zone_thickness(grid(P), grid(T), grid(Z)),
    'thermo_layers.hail_growth_zone_thickness:column': lambda: TL.hail_growth_zone_thickness(col(P), col(T), col(Z)),
    'thermo_layers.theta_e_difference:grid': lambda: TL.theta_e_difference(*ptz()),
    # layer_cape: bounds by pressure, height and temperature; the parcels
    'layer_cape.cape_cin_layers:bounds': lambda: LC.cape_cin_layers(grid(P), grid(T), grid(TD), [
        {'top_height': 3000.}, {'bottom': horiz(900.), 'top': 500.}, {'bottom_temperature': 280., 'top_temperature': 270.}],
        height=grid(Z)),
    'layer_cape.cape_cin_layers:explicit': lambda: LC.cape_cin_layers(
        grid(P), grid(T), grid(TD), [{'top': 500.}], parcel='explicit', parcel_values=[horiz(990.), 299., horiz(293.)]),
    'layer_cape.cape_cin_layers:most_unstable': lambda: LC.cape_cin_layers(
        grid(P), grid(T), grid(TD), [{'bottom': 900., 'top': 600.}, {'top': 500.}], parcel='most_unstable', moist='family'),
    'layer_cape.cape_cin_layers:mixed_layer_depth': lambda: LC.cape_cin_layers(
        grid(P), grid(T), grid(TD), [{'top': horiz(500.)}], parcel='mixed_layer', depth=50, lcl_interp='linear'),
    'layer_cape.cape_3km:grid': lambda: LC.cape_3km(*ptz()),
    'layer_cape.cape_3km:explicit': lambda: LC.cape_3km(*ptz(), parcel='explicit', parcel_values=sfc()),
    'layer_cape.hail_growth_zone_cape:grid': lambda: LC.hail_growth_zone_cape(*ptz(), parcel='mixed_layer'),
    # hydrostatic: isobaric pressure, the moisture choices, base height as a field, a scalar and None
    'hydrostatic.hydrostatic:isobaric_layers': lambda: HY.hydrostatic(
        col(P), grid(T), grid(TD), base_height=horiz(10.), layers=[{'depth': 150}, {'bottom': 1000, 'top': 500}]),
    'hydrostatic.hydrostatic:specific_want': lambda: HY.hydrostatic(
        grid(P), grid(T), specific_humidity=grid(Q), base_height=5.0, want=('height', 'status')),
    'hydrostatic.hydrostatic:dry_column': lambda: HY.hydrostatic(col(P), col(T), layers=[{'bottom': None, 'top': None}],
                                                                want=('thickness',)),
    'hydrostatic.hydrostatic_height:grid': lambda: HY.hydrostatic_height(grid(P), grid(T), grid(TD), base_height=horiz(10.)),
    'hydrostatic.hydrostatic_height:dry_isobaric': lambda: HY.hydrostatic_height(col(P), grid(T)),
    'hydrostatic.thickness_hydrostatic:default': lambda: HY.thickness_hydrostatic(grid(P), grid(T), grid(TD)),
    'hydrostatic.thickness_hydrostatic:depth': lambda: HY.thickness_hydrostatic(
        grid(P), grid(T), specific_humidity=grid(Q), bottom=950, depth=200),
    'hydrostatic.geopotential_to_height:dataarray': lambda: HY.geopotential_to_height(horiz(1000., 'phi')),
    'hydrostatic.geopotential_to_height:ndarray': lambda: HY.geopotential_to_height(np.array([0., 1000., 50000.])),
    'hydrostatic.height_to_geopotential:dataarray': lambda: HY.height_to_geopotential(grid(Z)),
    'hydrostatic.height_to_geopotential:ndarray': lambda: HY.height_to_geopotential(Z),
    # entrainment
    'entrainment.ncape:grid': lambda: EN.ncape(*ptz(), horiz(900.), horiz(300.)),
    'entrainment.ncape:scalar_el': lambda: EN.ncape(*ptz(), horiz(900.), 300.),
    'entrainment.ecape_from_ncape:grid': lambda: EN.ecape_from_ncape(horiz(2000.), horiz(1500.), horiz(11000.), horiz(5.),
                                                                     horiz(-3.)),
    'entrainment.ecape:bunkers': lambda: EN.ecape(*ptz(), grid(U), grid(-U)),
    'entrainment.ecape:storm': lambda: EN.ecape(*ptz(), grid(U), grid(-U), parcel='mixed_layer', storm_u=horiz(1.), storm_v=2.0,
                                                moist='family'),
    'entrainment.ecape:surface_left': lambda: EN.ecape(*ptz(), grid(U), grid(-U), parcel='surface', storm='left'),
    # sounding_indices
    'sounding_indices.sounding_indices:winds': lambda: SI.sounding_indices(grid(P), grid(T), grid(TD), grid(U), grid(-U)),
    'sounding_indices.sounding_indices:no_winds': lambda: SI.sounding_indices(grid(P), grid(T), grid(TD)),
    'sounding_indices.sounding_indices:want': lambda: SI.sounding_indices(
        col(P), col(T), col(TD), want=('k_index', 'ccl_pressure'), which='bottom', mixed_layer_depth=50, moist='family'),
    'sounding_indices.k_index:grid': lambda: SI.k_index(grid(P), grid(T), grid(TD)),
    'sounding_indices.total_totals_index:grid': lambda: SI.total_totals_index(grid(P), grid(T), grid(TD)),
    'sounding_indices.cross_totals:grid': lambda: SI.cross_totals(grid(P), grid(T), grid(TD)),
    'sounding_indices.vertical_totals:no_dewpoint': lambda: SI.vertical_totals(grid(P), grid(T)),
    'sounding_indices.showalter_index:grid': lambda: SI.showalter_index(grid(P), grid(T), grid(TD), moist='family'),
    'sounding_indices.sweat_index:grid': lambda: SI.sweat_index(grid(P), grid(T), grid(TD), grid(U), grid(-U)),
    'sounding_indices.ccl:grid': lambda: SI.ccl(grid(P), grid(T), grid(TD), mixed_layer_depth=100),
    # isentropic
    'isentropic.isentropic_interpolation:temperature_out_args': lambda: IS.isentropic_interpolation(
        [310., 300.], grid(P), grid(T), grid(Z, 'z'), grid(U), temperature_out=True),
    'isentropic.isentropic_interpolation:isobaric': lambda: IS.isentropic_interpolation([300.], col(P), grid(T),
                                                                                       bottom_up_search=False),
    'isentropic.isentropic_interpolation:column': lambda: IS.isentropic_interpolation(305., col(P), col(T), col(Z, 'z')),
    # downdraft
    'downdraft.downdraft_cape:grid': lambda: DD.downdraft_cape(grid(P), grid(T), grid(TD)),
    'downdraft.downdraft_cape:column': lambda: DD.downdraft_cape(col(P), col(T), col(TD), bottom=850, depth=300, moist='family'),
    # ground: the pressure on the grid and as the isobars
    'ground.levels_below_ground:isobars': lambda: GR.levels_below_ground(P, 940. + 20 * OFF),
    'ground.surface_based_cape_cin:grid': lambda: GR.surface_based_cape_cin(grid(P), grid(T), grid(TD), *sfc()),
    'ground.surface_based_cape_cin:isobaric': lambda: GR.surface_based_cape_cin(col(P), grid(T), grid(TD), *sfc(),
                                                                               moist='family', want=('cape', 'cin')),
    'ground.most_unstable_cape_cin:isobaric': lambda: GR.most_unstable_cape_cin(col(P), grid(T), grid(TD), *sfc()),
    'ground.mixed_layer_cape_cin:grid': lambda: GR.mixed_layer_cape_cin(grid(P), grid(T), grid(TD), *sfc(), depth=50,
                                                                       lifted_index_at=500.),
    'ground.cape_cin_multi:isobaric': lambda: GR.cape_cin_multi(
        col(P), grid(T), grid(TD), *sfc(), ['surface', ('most_unstable', 300), ('mixed_layer', 50), 'most_unstable'],
        lifted_index_at=500.),
    'ground.cape_cin_multi:grid': lambda: GR.cape_cin_multi(grid(P), grid(T), grid(TD), *sfc(), [('mixed_layer', None)],
                                                            want=('cape', 'cin'), moist='family'),
}
ALL_CASES = {**CASES, **FEATURE_CASES}


# -- the stand-ins for the launch and the outputs ------------------------------------------------------------------------
def _fake_out(self, shape, dtype=None):
    """Output number k of this call: 10 k + i/2 for element i (ints: (k + i) mod 3), its last row NaN when it has at least
    three rows -- the NaN padding the drivers trim."""
    dtype = np.dtype(dtype or self.dtype)
    outs = self.__dict__.setdefault('_outs', [])
    i = np.arange(int(np.prod(shape)))
    if dtype.kind in 'iu':
        a = ((len(outs) + 1 + i) % 3).astype(dtype).reshape(shape)
    else:
        a = (10 * (len(outs) + 1) + 0.5 * i).astype(dtype).reshape(shape)
        if len(shape) and shape[0] >= 3:
            a[-1] = np.nan
    outs.append(a)
    return a


def _located(address, call, foreign_ok=False):
    """A pointer as 'in<k>+<byte offset>' or 'out<k>+<byte offset>': into the k-th array the call staged (_Call._keep) or allocated (_fake_out),
    the first that holds the address; None for a null pointer (and, for an array argument, for one that is not the call's)."""
    if not address:
        return None
    for space, arrays in (('in', call._keep), ('out', call.__dict__.get('_outs', []))):
        for k, a in enumerate(arrays):
            if a.ctypes.data <= address < a.ctypes.data + max(a.nbytes, 1):
                return '%s%d+%d' % (space, k, address - a.ctypes.data)
    assert foreign_ok, 'a pointer into no array of its call'


def _abi(v, t, call):
    """The value `v` of ctypes type `t`, as an argument or a field of one, in JSON form."""
    if issubclass(t, C.Structure):
        return [_abi(getattr(v, name), ft, call) for name, ft in t._fields_]           # (in the order of the fields)
    if issubclass(t, C.Array):
        return [_abi(x, t._type_, call) for x in v]
    if issubclass(t, C._Pointer):
        return _abi(v.contents, t._type_, call) if v else None
    v = getattr(v, 'value', v)
    return _located(v, call) if t is C.c_void_p else v


def _digest(a):
    return hashlib.sha1(a.tobytes()).hexdigest()[:12]


def _launch(call, name, args):
    """What _Call.run hands entry point `name`."""
    out = []
    for a in args:
        if isinstance(a, np.ndarray):
            out.append([str(a.dtype), list(a.shape), _digest(a), _located(a.ctypes.data, call, foreign_ok=True)])
        elif isinstance(a, (C.Structure, C.Array, C._Pointer, C._SimpleCData)):
            out.append(_abi(a, type(a), call))
        elif hasattr(a, '_obj'):                                           # byref(x)
            out.append(_abi(a._obj, type(a._obj), call))
        else:
            assert a is None or isinstance(a, (int, float)), type(a)
            out.append(a)
    return {'launch': name, 'args': out}


_BRIEF = [False]            # the feature modules' cases: _enc records arrays of more than six elements, and the attrs and coords
                            # of a DataArray, as digests


def _enc(x):
    """JSON form of an argument or result."""
    if isinstance(x, Dataset):
        names = list(x.data_vars) if hasattr(x, 'data_vars') else list(x.keys())
        return {'type': 'Dataset', 'vars': [[k, _enc(x[k])] for k in names],
                'attrs': x.attrs if isinstance(x.attrs, list) else _enc(dict(x.attrs))}
    if isinstance(x, DataArray):
        labels = {'attrs': _enc(dict(x.attrs)), 'coords': {k: _enc(np.asarray(v)) for k, v in x.coords.items()}}
        if _BRIEF[0]:                                                   # (attrs and coords: a digest of their JSON form)
            labels = {'labels': hashlib.sha1(_canon(labels).encode()).hexdigest()[:12]}
        return {'type': 'DataArray', 'name': x.name, 'dims': list(x.dims), 'data': _enc(np.asarray(x.values)), **labels}
    if isinstance(x, (np.ndarray, np.generic)):
        x = np.asarray(x)
        return [str(x.dtype), list(x.shape), _digest(x) if _BRIEF[0] and x.size > 6 else x.tolist()]   # dtype, shape, values
    if isinstance(x, dict):
        return {str(k): _enc(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_enc(v) for v in x]
    assert x is None or isinstance(x, (bool, int, float, str)), type(x)
    return x


def _result(x):
    return {'type': type(x).__name__, 'value': _enc(x)}


def _offline(monkeypatch):
    """The API without its launches; returns the list the mirror's numpy_api calls and their launches are recorded into."""
    calls, depth = [], [0]
    monkeypatch.setattr(api._Call, 'run', lambda self, name, *args: calls.append(_launch(self, name, args)))
    monkeypatch.setattr(api._Call, 'out', _fake_out)
    monkeypatch.setattr(api.torch.cuda, 'is_available', lambda: False)      # the bundles stay on the host

    def recorded(name, fn):
        def call(*args, **kwargs):
            if depth[0] == 0:
                calls.append({'fn': name, 'args': _enc(list(args)), 'kwargs': _enc(kwargs)})
            depth[0] += 1
            try:
                return fn(*args, **kwargs)
            finally:
                depth[0] -= 1
        return call
    for name, fn in inspect.getmembers(api, inspect.isfunction):
        if not name.startswith('_') and fn.__module__ == api.__name__:
            monkeypatch.setattr(api, name, recorded(name, fn))
    return calls


@pytest.fixture
def offline(monkeypatch):
    return _offline(monkeypatch)


def _record(case, calls):
    """The numpy_api calls of a case, its launches as [index of the call they ran under, entry point, arguments] and its
    result."""
    del calls[:]
    _BRIEF[0] = case in FEATURE_CASES
    out = _result(ALL_CASES[case]())
    fns = [c for c in calls if 'fn' in c]
    launches = [[sum('fn' in d for d in calls[:i]) - 1, c['launch'], c['args']] for i, c in enumerate(calls) if 'launch' in c]
    return {'calls': fns, 'launches': launches, 'result': out}


def _canon(x):
    return json.dumps(x, sort_keys=True)


def _public(module):
    return {n for n, f in inspect.getmembers(module, inspect.isfunction)
            if not n.startswith('_') and f.__module__ == module.__name__}


def test_every_public_function_is_recorded():
    covered = {c.split(':')[0] for c in CASES}
    assert covered <= _public(pf) and _public(pf) - covered == NOT_RECORDED, (covered - _public(pf),
                                                                             _public(pf) - covered - NOT_RECORDED)
    public = {'%s.%s' % (m.__name__.split('.')[-1], n) for m in FEATURE_MODULES for n in _public(m)}
    covered = {c.split(':')[0] for c in FEATURE_CASES}
    assert covered == public, (covered - public, public - covered)              # (no exceptions in the feature modules)


@functools.lru_cache(maxsize=None)
def _golden(path):
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize('case', list(ALL_CASES))
def test_mirror_matches_snapshot(case, offline):
    gold = dict(_golden(GOLDEN)[case] if case in CASES else {}, **_golden(GOLDEN_FEATURES)[case])
    got = json.loads(_canon(_record(case, offline)))
    assert [c['fn'] for c in got['calls']] == [c['fn'] for c in gold['calls']]
    for i, (g, w) in enumerate(zip(got['calls'], gold['calls'])):
        assert _canon(g) == _canon(w), f'numpy_api call {i} ({w["fn"]})'
    assert [l[:2] for l in got['launches']] == [l[:2] for l in gold['launches']]
    for g, w in zip(got['launches'], gold['launches']):
        assert _canon(g) == _canon(w), f'launch of {w[1]} under numpy_api call {w[0]}'
    assert _canon(got['result']) == _canon(gold['result'])


def test_layered_outputs_of_one_column(offline):
    """Several layers of a grid without horizontal dims: row i of every layered output is handed over as a pointer i
    elements into it (these two calls failed before the output structs were built in one place, so no recording has them)."""
    for call, entry, keys in (
            (lambda: K.storm_relative_helicity_layers(*zuv(col), 0., [1000., 3000.]), 'xp_storm_relative_helicity_layers',
             L.SRH_LAYERS_OUT),
            (lambda: LC.cape_cin_layers(col(P), col(T), col(TD), [{'bottom': 900., 'top': 600.}, {'top': 500.}]),
             'xp_cape_cin_layers', L.CAPE_LAYERS_OUT)):
        del offline[:]
        ds = call()
        out = next(c for c in offline if c.get('launch') == entry)['args'][-1]
        for j in range(len(keys)):                                # (the layered fields lead their struct)
            assert out[j] == ['out%d+0' % j, 'out%d+8' % j, None, None], keys[j]
        assert ds['total_srh' if 'total' in keys else 'cape'].shape == (2,)


def test_scalar_for_a_view_is_refused(offline):
    """An optional view given as a scalar reaches numpy_api as it is and fails its shape assertion."""
    for call in (lambda: SI.sounding_indices(grid(P), grid(T), grid(TD), u=1.0, v=2.0),
                 lambda: TL.thermo_layers(grid(P), temperature=300., layers=[{'depth': 100}]),
                 lambda: K.wind_layers(*puv(), height=1000., layers=[{'depth': 100}]),
                 lambda: LC.cape_cin_layers(grid(P), grid(T), grid(TD), [{'top': 500.}], height=1000.)):
        with pytest.raises(AssertionError, match='must share a shape'):
            call()


# -- assert paths: the reference's messages ------------------------------------------------------------------------------
def test_reference_asserts(offline):
    p, t, td = named(grid)
    for args, msg in (((col(P), t, td), 'Pressure requires name pressure.'),
                      ((p, col(T), td), 'Temperature requires name temperature.'),
                      ((p, t, col(TD)), 'Dewpoint requires name dewpoint.')):
        for fn in (pf.most_unstable_cape_cin, pf.mixed_layer_cape_cin, pf.from_most_unstable_parcel, pf.mix_layer):
            with pytest.raises(AssertionError, match=msg):
                fn(*args)
    with pytest.raises(AssertionError, match='pressure requires name pressure.'):
        pf.mixed_parcel(grid(P, None), t, td)
    step2 = lambda v: DataArray(v, dims=(VD,), coords={VD: np.arange(5) * 2}, name='pressure')
    with pytest.raises(AssertionError, match='Vert_dim index increments must all be 1.'):
        pf.surface_based_cape_cin(step2(P), step2(T), step2(TD))
    with pytest.raises(AssertionError, match='Vert_dim index increments must all be 1.'):
        pf.insert_level(Dataset({'pressure': step2(P)}), Dataset({'pressure': DataArray(800.)}), 'pressure')
    with pytest.raises(AssertionError, match='Vert_dim index increments must all be 1.'):
        pf.add_lcl_to_profile(Dataset({'pressure': step2(P), 'temperature': step2(T), 'virtual_temperature': step2(T),
                                       'lcl_pressure': DataArray(900.), 'lcl_temperature': DataArray(288.),
                                       'lcl_virtual_temperature': DataArray(289.)}))
    for call in (lambda: pf.lfc_el(step2(P), step2(T), step2(T), 900., 288.),
                 lambda: pf.cape_cin_base(step2(P), step2(T), 850., 300., step2(T)),
                 lambda: pf.freezing_level_height(step2(T), step2(Z)),
                 lambda: pf.find_intersections(step2(P), step2(T), step2(TD), VD),
                 lambda: pf.trapz(Dataset({'pressure': step2(P)}), 'pressure', VD),
                 lambda: pf.trap_around_zeros(step2(P), step2(T), VD),
                 lambda: pf.shift_out_nans(Dataset({'pressure': step2(P)}), 'pressure', VD)):
        with pytest.raises(AssertionError, match='Index increments must all be 1.'):
            call()
    with pytest.raises(AssertionError, match='Index increments must all be 1.'):
        pf.valid_data(Dataset({'pressure': grid(P), VD: DataArray(np.arange(5) * 2, dims=(VD,))}), VD)
    with pytest.raises(AssertionError, match='Pressures must decrease with increasing level number.'):
        pf.valid_data(Dataset({'pressure': grid(P[::-1]), VD: DataArray(np.arange(1, 6), dims=(VD,))}), VD)
    with pytest.raises(AssertionError, match='dataset d contains fill_value.'):
        pf.insert_level(Dataset({'pressure': col(np.where(P == 700, -999, P))}), Dataset({'pressure': DataArray(800.)}),
                        'pressure')
    with pytest.raises(AssertionError, match='extrapolation is not part of the MI355X path'):
        pf.linear_interp(grid(T), grid(P), 500., extrapolate=True)
    with pytest.raises(AssertionError, match='interpolator must be linear or log'):
        pf.add_lcl_to_profile(profile(), interpolator='cubic')
    with pytest.raises(AssertionError, match='Only negative OR positive regions can be included in trapz.'):
        pf.trapz(ptd(), 'pressure', VD, only_positive=True, only_negative=True)
    with pytest.raises(AssertionError, match='only the default table grid is implemented'):
        pf.moist_adiabat_lookup(pressure_levels=np.array([1000., 999.5]))


# every mirror function that lifts a parcel moist-adiabatically
MOIST_CALLS = {
    'surface_based_cape_cin': lambda **kw: pf.surface_based_cape_cin(grid(P), grid(T), grid(TD), **kw),
    'most_unstable_cape_cin': lambda **kw: pf.most_unstable_cape_cin(*named(grid), **kw),
    'mixed_layer_cape_cin': lambda **kw: pf.mixed_layer_cape_cin(*named(grid), **kw),
    'cape_cin': lambda **kw: pf.cape_cin(grid(P), grid(T), grid(TD), PV[1], PV[0], PV[2], **kw),
    'moist_lapse': lambda **kw: pf.moist_lapse(col(P), np.array([300.]), **kw),
    'parcel_profile': lambda **kw: pf.parcel_profile(col(P), 1000., 300., 295., **kw),
    'parcel_profile_with_lcl': lambda **kw: pf.parcel_profile_with_lcl(grid(P), grid(T), grid(TD), *PV, **kw),
    'wet_bulb_temperature': lambda **kw: pf.wet_bulb_temperature(grid(P), grid(T), grid(TD), **kw),
    'melting_level_height': lambda **kw: pf.melting_level_height(grid(P), grid(T), grid(TD), grid(Z), fast=False, **kw),
    'conv_properties': lambda **kw: pf.conv_properties(bundle(), **kw),
    'min_conv_properties': lambda **kw: pf.min_conv_properties(bundle(), **kw),
}


@pytest.mark.parametrize('fn', list(MOIST_CALLS))
def test_table_asserts(fn, offline, monkeypatch):
    """Without tables the reference's 'Call load_moist_adiabat_lookups first.': from lookup_tables_loaded() under the
    default mode, and from the library's XP_E_NO_TABLES under an explicit moist='table'.  Other library errors pass
    through as they are."""
    class _NoTables:
        def xp_tables_loaded(self):
            return 0
    monkeypatch.setattr(L, 'load', lambda: _NoTables())
    pf.set_moist_lapse(None)
    with pytest.raises(AssertionError, match='Call load_moist_adiabat_lookups first.'):
        MOIST_CALLS[fn]()
    pf.set_moist_lapse('exact')
    for code, err in ((L.XP_E_NO_TABLES, AssertionError), (L.XP_E_ARG, L.XParcelError)):
        def fail(self, name, *args, code=code):
            raise L.XParcelError(code, 'stand-in')
        monkeypatch.setattr(api._Call, 'run', fail)
        with pytest.raises(err) as e:
            MOIST_CALLS[fn](moist='table')
        assert err is L.XParcelError or str(e.value) == 'Call load_moist_adiabat_lookups first.'


if __name__ == '__main__':
    mp = pytest.MonkeyPatch()
    pf.set_moist_lapse('exact')                     # the suite's mode (tests/conftest.py)
    calls = _offline(mp)
    snap = {case: _record(case, calls) for case in ALL_CASES}
    launches = {case: {'launches': snap[case].pop('launches')} for case in CASES}
    for path, cases in ((GOLDEN, {case: snap[case] for case in CASES}),
                        (GOLDEN_FEATURES, {**launches, **{case: snap[case] for case in FEATURE_CASES}})):
        with open(path, 'w') as f:
            f.write(json.dumps(cases, sort_keys=True, separators=(',', ':')) + '\n')
        print(f'{path}: {len(cases)} cases, {os.path.getsize(path)} bytes')
    mp.undo()
