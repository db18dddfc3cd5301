"""ctypes binding of libxparcel.so (include/xparcel.h).  No CPU fallback: if the library is missing
or no MI355X is visible, calls raise."""
import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('XPARCEL_LIB') or os.path.join(_HERE, 'lib', 'libxparcel.so')   # env override: A/B builds
SRC_DIR = os.path.join(_HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(_HERE), 'include', 'xparcel.h')

XP_F32, XP_F64 = 0, 1
XP_MEM_HOST, XP_MEM_DEVICE = 0, 1
PARCEL = {'surface': 0, 'most_unstable': 1, 'mixed_layer': 2, 'explicit': 3, 'max_cape': 4}
PARCEL_OVER_GROUND = 16       # XP_PARCEL_OVER_GROUND: a flag on xp_parcel.mode (isobaric levels cut at the ground)
MOIST = {'exact': 0, 'table': 1, 'family': 2}
LCL_INTERP = {'linear': 0, 'log': 1}
HUMIDITY = {'dewpoint': 0, 'specific': 1, 'relative': 2, 'mixing_ratio': 3}     # xp_opts.humidity: what the moisture view holds
COMPUTE = {'float32': XP_F32, 'float64': XP_F64}      # xp_opts.compute: the arithmetic type
OPT_FUSE_PARCELS = 1
# xp_opts.flags, bits 4-6 (XP_OPT_LAYER_*): which positive layer a CAPE / CIN call describes; 'envelope' is the reference's rule
OPT_LAYER_SHIFT, OPT_LAYER_MASK = 4, 7 << 4
POSITIVE_LAYER = {'envelope': 0 << 4, 'lowest': 1 << 4, 'highest': 2 << 4, 'deepest': 3 << 4, 'most_cape': 4 << 4}
# ... and MetPy's (which_lfc, which_el) pairs that name one
WHICH_LFC_EL = {('bottom', 'top'): 'envelope', ('bottom', 'bottom'): 'lowest', ('top', 'top'): 'highest', ('wide', 'wide'): 'deepest',
                ('most_cape', 'most_cape'): 'most_cape'}
ST_TOP_NAN, ST_LCL_NOT_CONVERGED, ST_NAN_PRESSURE, ST_BAD_PRESSURE = 1, 2, 4, 8

# every symbol include/xparcel.h declares
SYMBOLS = ('xp_version', 'xp_init', 'xp_set_tables', 'xp_tables_loaded', 'xp_family_table', 'xp_set_family_table', 'xp_cape_cin', 'xp_cape_cin_multi', 'xp_lcl', 'xp_dry_lapse',
           'xp_moist_lapse', 'xp_parcel_profile', 'xp_lfc_el', 'xp_cape_cin_base', 'xp_select_parcel',
           'xp_mixed_layer', 'xp_wet_bulb_temperature', 'xp_downdraft_cape', 'xp_effective_inflow_layer', 'xp_cape_cin_layers', 'xp_interp_level', 'xp_interp_levels',
           'xp_dewpoint_from_specific_humidity',
           'xp_crossing_level', 'xp_mixing_ratio', 'xp_conv_properties', 'xp_insert_level', 'xp_find_intersections', 'xp_trapz',
           'xp_trap_around_zeros', 'xp_bound_pressure', 'xp_get_layer', 'xp_shift_out_nans', 'xp_rebase_profile', 'xp_interp1d',
           'xp_wind_shear', 'xp_significant_hail_parameter', 'xp_storm_proxies', 'xp_bunkers_storm_motion',
           'xp_storm_relative_helicity', 'xp_storm_relative_helicity_layers', 'xp_significant_tornado', 'xp_supercell_composite',
           'xp_wind_layers', 'xp_thermo_layers', 'xp_sounding_indices', 'xp_isentropic_interpolation', 'xp_hydrostatic_height',
           'xp_geopotential_to_height', 'xp_height_to_geopotential', 'xp_critical_angle', 'xp_corfidi_storm_motion', 'xp_significant_tornado_effective',
           'xp_ncape', 'xp_ecape', 'xp_last_error')


class View(C.Structure):
    _fields_ = [('data', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32), ('nlev', C.c_int64),
                ('ncol', C.c_int64), ('lev_stride', C.c_int64), ('col_stride', C.c_int64)]


class Parcel(C.Structure):
    _fields_ = [('mode', C.c_int32), ('reserved', C.c_int32), ('depth', C.c_double), ('pressure', C.c_void_p),
                ('temperature', C.c_void_p), ('dewpoint', C.c_void_p)]


class Opts(C.Structure):
    _fields_ = [('virtual_temperature_correction', C.c_int32), ('lcl_interp', C.c_int32),
                ('pos_cape_neg_cin', C.c_int32), ('post_zero_cin', C.c_int32), ('moist_mode', C.c_int32),
                ('compute', C.c_int32), ('humidity', C.c_int32), ('flags', C.c_int32)]


SCALAR_F = ('cape', 'cin', 'lcl_pressure', 'lcl_temperature', 'lcl_virtual_temperature', 'lfc_pressure',
            'lfc_temperature', 'el_pressure', 'el_temperature')
SCALAR_I = ('lfc_index', 'el_index', 'status', 'parcel_index')
SCALAR_P = ('parcel_pressure', 'parcel_temperature', 'parcel_dewpoint')


class ScalarsOut(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in SCALAR_F] + [(k, C.c_void_p) for k in SCALAR_I] +
                [(k, C.c_void_p) for k in SCALAR_P] + [('dtype', C.c_int32), ('mem', C.c_int32)])


PROFILE_VARS = ('pressure', 'temperature', 'virtual_temperature', 'environment_temperature',
                'environment_virtual_temperature', 'environment_dewpoint')


class ProfileOut(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in PROFILE_VARS] +
                [('dtype', C.c_int32), ('mem', C.c_int32), ('nlev_out', C.c_int64), ('lev_stride', C.c_int64),
                 ('col_stride', C.c_int64), ('lifted_index', C.c_void_p), ('lifted_index_pressure', C.c_double)])


CONV_IN_VIEWS = ('pressure', 'temperature', 'specific_humidity', 'height_asl', 'wind_u', 'wind_v', 'wind_height_above_surface')
CONV_OUT = ('mu_cape', 'mu_cin', 'mu_mixing_ratio', 'mu_lifted_index', 'mu_dci', 'mixed_100_cape', 'mixed_100_cin',
            'mixed_100_lifted_index', 'mixed_100_dci', 'mixed_50_cape', 'mixed_50_cin', 'mixed_50_lifted_index', 'mixed_50_dci',
            'lapse_rate_700_500', 'temp_500', 'freezing_level', 'melting_level', 'shear_u', 'shear_v', 'shear_magnitude',
            'positive_shear')


class ConvIn(C.Structure):
    _fields_ = [(k, C.POINTER(View)) for k in CONV_IN_VIEWS] + [('surface_wind_u', C.c_void_p), ('surface_wind_v', C.c_void_p)]


class ConvOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in CONV_OUT]


PROXIES_IN = ('mu_cape', 'mu_mixing_ratio', 'mixed_100_cape', 'mixed_100_cin', 'mixed_100_lifted_index', 'mixed_100_dci',
              'mixed_50_cape', 'mixed_50_cin', 'lapse_rate_700_500', 'temp_500', 'freezing_level', 'shear_magnitude')
PROXIES_OUT = ('proxy_Craven2004', 'proxy_Kunz2007', 'proxy_Trapp2007', 'proxy_Marsh2009', 'proxy_Allen2011', 'proxy_Allen2014',
               'proxy_Eccel2012', 'proxy_Mohr2013', 'proxy_SHIP_0.1')


class ProxiesIn(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in PROXIES_IN] + [('positive_shear', C.c_void_p)]


class ProxiesOut(C.Structure):
    _fields_ = [('f%d' % i, C.c_void_p) for i in range(9)] + [('ship', C.c_void_p)]


# xp_downdraft_cape: its outputs, and the status bit of a column that does not span the layer
XP_ST_NO_LAYER = 16
DCAPE_OUT = ('dcape', 'start_pressure', 'start_temperature', 'status', 'parcel_temperature')


class DcapeOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in DCAPE_OUT] + [('dtype', C.c_int32), ('mem', C.c_int32)]


# xp_bunkers_storm_motion / xp_storm_relative_helicity: their outputs (SRH: per depth, up to SRH_MAX_DEPTHS), and the
# status bit of a column whose heights do not increase
ST_BAD_HEIGHT = 32
SRH_MAX_DEPTHS = 4
STORM_MOTION_OUT = ('right_u', 'right_v', 'left_u', 'left_v', 'mean_u', 'mean_v', 'status')
SRH_OUT = ('positive', 'negative', 'total')


class StormMotionOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in STORM_MOTION_OUT] + [('dtype', C.c_int32), ('mem', C.c_int32)]


class SrhOut(C.Structure):
    _fields_ = ([(k, C.c_void_p * SRH_MAX_DEPTHS) for k in SRH_OUT] +
                [('status', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32)])


# xp_effective_inflow_layer: its outputs (per column; the last two dense (nlev, ncol)), and the status bit of a layer that
# the search window cut
ST_LAYER_OPEN = 64
EFFECTIVE_F = ('base_pressure', 'top_pressure', 'base_height', 'top_height')
EFFECTIVE_I = ('base_index', 'top_index', 'status')
EFFECTIVE_CANDIDATES = ('candidate_cape', 'candidate_cin')
# the named outputs of every struct that are int32_t * (indices, the status word, the shear flag); all others have the call's dtype
INT32_OUT = frozenset(SCALAR_I + EFFECTIVE_I + ('positive_shear',))


class EffectiveLayerOut(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in EFFECTIVE_F + EFFECTIVE_I + EFFECTIVE_CANDIDATES] +
                [('dtype', C.c_int32), ('mem', C.c_int32)])


# xp_cape_cin_layers: per layer (up to CAPE_MAX_LAYERS) CAPE and CIN, and the whole ascent's scalars
CAPE_MAX_LAYERS = 4
CAPE_LAYERS_OUT = ('cape', 'cin')
CAPE_LAYERS_TOTAL = ('total_cape', 'total_cin', 'lfc_pressure', 'el_pressure', 'lcl_pressure')


class CapeLayersOut(C.Structure):
    _fields_ = ([(k, C.c_void_p * CAPE_MAX_LAYERS) for k in CAPE_LAYERS_OUT] + [(k, C.c_void_p) for k in CAPE_LAYERS_TOTAL] +
                [('status', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32)])


# xp_storm_relative_helicity_layers: per layer (up to SRH_MAX_DEPTHS) the helicity sums and the bulk wind difference
SRH_LAYERS_OUT = SRH_OUT + ('shear_u', 'shear_v')


class SrhLayersOut(C.Structure):
    _fields_ = ([(k, C.c_void_p * SRH_MAX_DEPTHS) for k in SRH_LAYERS_OUT] +
                [('status', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32)])


# xp_wind_layers: the layer kinds, one layer of the request, and per layer (up to WIND_MAX_LAYERS) the outputs
LAYER_PRESSURE, LAYER_PRESSURE_DEPTH, LAYER_HEIGHT = 0, 1, 2
WIND_MAX_LAYERS = 4
WIND_LAYERS_OUT = ('mean_u', 'mean_v', 'shear_u', 'shear_v', 'bottom_u', 'bottom_v', 'max_u', 'max_v', 'max_pressure')


class WindLayer(C.Structure):
    _fields_ = [('kind', C.c_int32), ('reserved', C.c_int32), ('bottom', C.c_double), ('top', C.c_double)]


class WindLayersOut(C.Structure):
    _fields_ = ([(k, C.c_void_p * WIND_MAX_LAYERS) for k in WIND_LAYERS_OUT] +
                [('status', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32)])


# xp_thermo_layers: xp_wind_layers' layers (a NaN top by pressure: to the highest valid level) and, per layer, the outputs
THERMO_MAX_LAYERS = 4
THERMO_LAYERS_OUT = ('precipitable_water', 'mean_mixing_ratio', 'mean_relative_humidity', 'thickness', 'lapse_rate',
                     'theta_e_min', 'theta_e_min_pressure', 'theta_e_max', 'theta_e_max_pressure')
# the input views (temperature, dewpoint, height) each output reads besides pressure
THERMO_LAYERS_NEEDS = {'precipitable_water': ('dewpoint',), 'mean_mixing_ratio': ('dewpoint',),
                       'mean_relative_humidity': ('temperature', 'dewpoint'), 'thickness': ('height',),
                       'lapse_rate': ('temperature', 'height'), 'theta_e_min': ('temperature', 'dewpoint'),
                       'theta_e_min_pressure': ('temperature', 'dewpoint'), 'theta_e_max': ('temperature', 'dewpoint'),
                       'theta_e_max_pressure': ('temperature', 'dewpoint')}


class ThermoLayersOut(C.Structure):
    _fields_ = ([(k, C.c_void_p * THERMO_MAX_LAYERS) for k in THERMO_LAYERS_OUT] +
                [('status', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32)])


# xp_sounding_indices: its options and per-column outputs, the CCL choices, and the status bit of a column without a CCL
ST_NO_CCL = 128
CCL_WHICH = {'top': 0, 'bottom': 1}
SOUNDING_INDEX_OUT = ('k_index', 'total_totals', 'cross_totals', 'vertical_totals', 'showalter_index', 'sweat_index')
SOUNDING_CCL_OUT = ('ccl_pressure', 'ccl_temperature', 'convective_temperature')
SOUNDING_OUT = SOUNDING_INDEX_OUT + SOUNDING_CCL_OUT


class SoundingOpts(C.Structure):
    _fields_ = [('moist_mode', C.c_int32), ('ccl_which', C.c_int32), ('ccl_mixed_layer_depth', C.c_double)]


class SoundingOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in SOUNDING_OUT + ('status',)] + [('dtype', C.c_int32), ('mem', C.c_int32)]


# xp_isentropic_interpolation: its options and (nlevel, ncol) outputs, its limits, and the status bit of a target whose
# Newton iteration did not converge
ST_NOT_CONVERGED = 256
ISEN_MAX_LEVELS = 64
ISEN_MAX_VARS = 4


class IsentropicOpts(C.Structure):
    _fields_ = [('from_below', C.c_int32), ('max_iters', C.c_int32), ('eps', C.c_double)]


class IsentropicOut(C.Structure):
    _fields_ = [('pressure', C.c_void_p), ('temperature', C.c_void_p), ('vars', C.c_void_p * ISEN_MAX_VARS),
                ('status', C.c_void_p), ('dtype', C.c_int32), ('mem', C.c_int32)]


# xp_hydrostatic_height: what its moisture view holds (the header's XP_HUM_*), its options and outputs; the layers are
# xp_wind_layers' by pressure (a NaN top: to the highest valid level)
HUM_DEWPOINT, HUM_SPECIFIC = 0, 1
HYDRO_MAX_LAYERS = 4


class HydrostaticOpts(C.Structure):
    _fields_ = [('humidity', C.c_int32), ('reserved', C.c_int32)]


class HydrostaticOut(C.Structure):
    _fields_ = [('height', C.c_void_p), ('thickness', C.c_void_p * HYDRO_MAX_LAYERS), ('status', C.c_void_p),
                ('dtype', C.c_int32), ('mem', C.c_int32)]


# xp_ncape: its per-column outputs; xp_ecape: its per-point inputs and outputs
NCAPE_OUT = ('ncape', 'lfc_height', 'el_height', 'status')
ECAPE_IN = ('cape', 'ncape', 'el_height', 'sr_u', 'sr_v')
ECAPE_OUT = ('ecape', 'ecape_a', 'psi')


class NcapeOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in NCAPE_OUT] + [('dtype', C.c_int32), ('mem', C.c_int32)]


class Tables(C.Structure):
    _fields_ = [('n_pressure', C.c_int64), ('n_temperature', C.c_int64), ('n_adiabat', C.c_int64),
                ('p_max', C.c_double), ('p_step', C.c_double), ('t_min', C.c_double), ('t_step', C.c_double),
                ('index', C.c_void_p), ('adiabats', C.c_void_p)]


_i32, _i64, _f64, _ptr = C.c_int32, C.c_int64, C.c_double, C.c_void_p
_V, _P, _O, _S, _PO = (C.POINTER(s) for s in (View, Parcel, Opts, ScalarsOut, ProfileOut))

# argtypes of every entry point, in the order of include/xparcel.h.  Data pointers (void *, double *, int32_t * outputs,
# uint8_t * masks) are _ptr: it takes an address, None, or any ctypes pointer, array or byref(); a struct pointer takes the
# struct itself (passed by reference), byref() or an array of structs.  Every entry point returns int except xp_last_error.
# The trailing _ptr of the compute entry points is the hipStream_t.
ARGTYPES = {
    'xp_version': (),
    'xp_init': (_i32,),
    'xp_set_tables': (C.POINTER(Tables),),
    'xp_tables_loaded': (),
    'xp_family_table': (_ptr, C.POINTER(_i64), C.POINTER(_i64)),
    'xp_set_family_table': (_ptr, _i64, _i64),
    'xp_cape_cin': (_V, _V, _V, _P, _O, _S, _PO, _ptr),
    'xp_cape_cin_multi': (_V, _V, _V, _i32, _P, _O, _S, _PO, _ptr),
    'xp_lcl': (_i64, _i32, _i32) + (_ptr,) * 8,
    'xp_dry_lapse': (_V, _ptr, _ptr, _ptr, _ptr),
    'xp_moist_lapse': (_V, _ptr, _ptr, _i32, _ptr, _ptr),
    'xp_parcel_profile': (_V, _ptr, _ptr, _ptr, _i32) + (_ptr,) * 6,
    'xp_lfc_el': (_V, _V, _V, _ptr, _ptr, _S, _ptr),
    'xp_cape_cin_base': (_V, _V, _V, _ptr, _ptr, _O, _ptr, _ptr, _ptr),
    'xp_select_parcel': (_V, _V, _V, _P, _S, _ptr),
    'xp_mixed_layer': (_V, _V, _f64, _ptr, _ptr),
    'xp_wet_bulb_temperature': (_V, _V, _V, _i32, _ptr, _ptr),
    'xp_downdraft_cape': (_V, _V, _V, _f64, _f64, _i32, C.POINTER(DcapeOut), _ptr),
    'xp_effective_inflow_layer': (_V, _V, _V, _V, _f64, _f64, _f64, _O, C.POINTER(EffectiveLayerOut), _ptr),
    'xp_cape_cin_layers': (_V, _V, _V, _P, _O, _i32, C.POINTER(_ptr), C.POINTER(_ptr), C.POINTER(CapeLayersOut), _ptr),
    'xp_interp_level': (_V, _V, _ptr, _i32, _i32, _ptr, _ptr),
    'xp_interp_levels': (_V, _i32, C.POINTER(_V), _i32, _ptr, _i32, C.POINTER(_ptr), _ptr),
    'xp_dewpoint_from_specific_humidity': (_V, _V, _V, _ptr, _ptr),
    'xp_crossing_level': (_V, _V, _f64, _ptr, _ptr),
    'xp_mixing_ratio': (_V, _V, _V, _ptr, _ptr),
    'xp_conv_properties': (C.POINTER(ConvIn), _O, _i32, C.POINTER(ConvOut), _ptr),
    'xp_insert_level': (_V, _V, _ptr, _ptr, _f64, _ptr, _ptr),
    'xp_find_intersections': (_V, _V, _V, _i32, C.POINTER(_ptr), _ptr),
    'xp_trapz': (_V, _V, _ptr, _i32, _i32, _ptr, _ptr),
    'xp_trap_around_zeros': (_V, _V, _i32, C.POINTER(_ptr), _ptr, _ptr),
    'xp_bound_pressure': (_V, _ptr, _ptr, _ptr),
    'xp_get_layer': (_V, _V, _f64, _i32, _i32, _ptr, _ptr),
    'xp_shift_out_nans': (_V, _V, _ptr, _ptr),
    'xp_rebase_profile': (_V, _V, _V, _P, _ptr, _ptr, _ptr, _S, _ptr, C.POINTER(_i64), _ptr),
    'xp_interp1d': (_V, _V, _V, _ptr, _ptr),
    'xp_wind_shear': (_V, _V, _V, _ptr, _ptr, _f64) + (_ptr,) * 5,
    'xp_significant_hail_parameter': (_i64, _i32, _i32) + (_ptr,) * 8,
    'xp_storm_proxies': (_i64, _i32, _i32, C.POINTER(ProxiesIn), C.POINTER(ProxiesOut), _ptr),
    'xp_bunkers_storm_motion': (_V, _V, _V, _V, C.POINTER(StormMotionOut), _ptr),
    'xp_storm_relative_helicity': (_V, _V, _V, _ptr, _ptr, _ptr, _ptr, _f64, _i32, _ptr, C.POINTER(SrhOut), _ptr),
    'xp_storm_relative_helicity_layers': (_V, _V, _V, _ptr, _ptr, _ptr, _ptr, _ptr, _i32, C.POINTER(_ptr),
                                          C.POINTER(SrhLayersOut), _ptr),
    'xp_significant_tornado': (_i64, _i32, _i32) + (_ptr,) * 6,
    'xp_supercell_composite': (_i64, _i32, _i32) + (_ptr,) * 5,
    'xp_wind_layers': (_V, _V, _V, _V, _i32, C.POINTER(WindLayer), C.POINTER(WindLayersOut), _ptr),
    'xp_thermo_layers': (_V, _V, _V, _V, _i32, C.POINTER(WindLayer), C.POINTER(_ptr), C.POINTER(_ptr),
                         C.POINTER(ThermoLayersOut), _ptr),
    'xp_sounding_indices': (_V, _V, _V, _V, _V, C.POINTER(SoundingOpts), C.POINTER(SoundingOut), _ptr),
    'xp_isentropic_interpolation': (_V, _V, _i32, C.POINTER(_V), _i32, C.POINTER(_f64), C.POINTER(IsentropicOpts),
                                    C.POINTER(IsentropicOut), _ptr),
    'xp_hydrostatic_height': (_V, _V, _V, _ptr, _i32, C.POINTER(WindLayer), C.POINTER(HydrostaticOpts),
                              C.POINTER(HydrostaticOut), _ptr),
    'xp_geopotential_to_height': (_i64, _i32, _i32) + (_ptr,) * 3,
    'xp_height_to_geopotential': (_i64, _i32, _i32) + (_ptr,) * 3,
    'xp_critical_angle': (_i64, _i32, _i32) + (_ptr,) * 8,
    'xp_corfidi_storm_motion': (_i64, _i32, _i32) + (_ptr,) * 9,
    'xp_significant_tornado_effective': (_i64, _i32, _i32) + (_ptr,) * 8,
    'xp_ncape': (_V, _V, _V, _V, _ptr, _ptr, C.POINTER(NcapeOut), _ptr),
    'xp_ecape': (_i64, _i32, _i32) + (_ptr,) * 9,
    'xp_last_error': (),
}


# return codes of the entry points (the error-code enum of include/xparcel.h)
XP_OK, XP_E_ARG, XP_E_NOT_INIT, XP_E_NO_TABLES, XP_E_INTERP, XP_E_HIP, XP_E_NO_DEVICE = 0, -1, -2, -3, -4, -5, -6


class XParcelError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libxparcel error {code}: {msg}')
        self.code = code


HIPCC_FLAGS = ['-O3', '--offload-arch=gfx950', '-std=c++17', '-fPIC'] + os.environ.get('XP_EXTRA_DEFS', '').split()   # (A/B builds)
# translation units: the ABI + small kernels, and k_cape_cin once per (dtype, moist mode) -- see csrc/xp_cape_tu.hip
# Per-moist-mode compile flags of the k_cape_cin translation units (XP_TU_FLAGS_<mode> overrides them for A/B builds).
# Mode 2 (adiabat family): ONE 1024-thread workgroup per CU -- the family coefficient table (46.7 KB) is staged into LDS
# next to the e_s / ln tables and the per-thread scan slots (157.5 of the CU's 160 KB) -- which caps the kernel at 128
# VGPRs; -disable-machine-licm keeps the compiler from hoisting the materialisation of ~40 fp64 constants out of the
# level loop into registers it then has to spill (128 VGPRs + 200 B of scratch with it, no spills in the loop without;
# the RK4 kernels lose ~2 % to the flag and do not get it).
TU_FLAGS = {0: [], 1: [], 2: ['-DXP_CAPE_THREADS=1024', '-mllvm', '-disable-machine-licm']}
for _m in list(TU_FLAGS):
    if os.environ.get(f'XP_TU_FLAGS_{_m}') is not None:
        TU_FLAGS[_m] = os.environ[f'XP_TU_FLAGS_{_m}'].split()
# The fused several-parcels kernel (csrc/xp_multi.hpp), one unit per (dtype, number of parcels): workgroup size and LDS
# slot fields per chain such that 58.6 KB of tables + NP x fields x threads x 8 B fit the CU's 160 KB.
MULTI_FLAGS = {2: ['-DXP_CAPE_THREADS=512', '-DXP_SLOT_FIELDS=12', '-mllvm', '-disable-machine-licm']}
for _m in list(MULTI_FLAGS):
    if os.environ.get(f'XP_MULTI_FLAGS_{_m}') is not None:
        MULTI_FLAGS[_m] = os.environ[f'XP_MULTI_FLAGS_{_m}'].split()
# The effective-inflow-layer kernel (csrc/xp_effective.hpp): its LCL iteration sits inside the candidate loop, and with
# machine LICM the fp64 constants of both loops are kept in registers through every ascent (160+ VGPRs instead of 106-112).
EFFECTIVE_FLAGS = ['-mllvm', '-disable-machine-licm']
# The maximum-CAPE parcel's kernels (csrc/xp_max_cape.hpp) are that sweep with another bookkeeping, in a unit of their own
# with the same flag.  VGPRs, waves per SIMD: k_max_cape_select f64 RK4 108, 4 / f64 tables 112, 4 / f32 RK4 105, 4 /
# f32 tables 110, 4 (38448 B of LDS: four workgroups per CU); k_rebase_from f64 43, 8 / f32 40, 8 (no LDS); no scratch.
# The wind-layers kernel (csrc/xp_wind_layers.hpp): each layer can add two bound points, each with three logarithms, and
# with machine LICM their fp64 constants are carried through the level loop (14 VGPRs more in every instantiation: three
# layers without the strongest wind 131 instead of 119, two with it 143 instead of 128 -- a wave per SIMD each).
WIND_LAYERS_FLAGS = ['-mllvm', '-disable-machine-licm']
# The thermodynamic-layers kernel (csrc/xp_thermo_layers.hpp): the same walk, the same bound points, the same flag.
THERMO_LAYERS_FLAGS = ['-mllvm', '-disable-machine-licm']
# The layer CAPE / CIN kernel (csrc/xp_cape_layers.hpp): the ascent of the effective-inflow kernel, and its flag for its reason
# (104-111 VGPRs without a spill).
CAPE_LAYERS_FLAGS = ['-mllvm', '-disable-machine-licm']
# The positive-layer kernel (csrc/xp_cape_pick.hpp): the same ascent with two more records per column, the same flag.
CAPE_PICK_FLAGS = ['-mllvm', '-disable-machine-licm']
# The sounding-indices kernel (csrc/xp_sounding.hpp) takes no flag: 59-84 VGPRs without winds, 81-105 with them, no scratch.
# The isentropic-interpolation kernel (csrc/xp_isentropic.hpp) takes none either: 50-52 VGPRs without extras, 86-87 with them, no scratch.
# The hydrostatic kernel (csrc/xp_hydrostatic.hpp), instantiated on dtype x {dry, dewpoint, specific humidity} x the number of
# layers (0 ... 4): no instantiation spills with or without machine LICM, but as in the other LayerGate kernels the flag keeps the
# fp64 constants of flog / fexp out of the level loop's registers (12 to 21 VGPRs fewer in every instantiation, a wave per SIMD
# more in most layered ones; on 64 x 1 Mi f64 the four-layer call 0.845 ms instead of 0.968, heights alone unchanged).
# VGPRs, waves per SIMD with the flag, by the number of layers 0 / 1 / 2 / 3 / 4:
#   f64 dry       39, 8 / 58, 8 / 77, 6 / 85, 5 /  94, 5      f32 dry       38, 8 / 56, 8 / 75, 6 / 83, 5 /  92, 5
#   f64 dewpoint  45, 8 / 67, 7 / 84, 5 / 92, 5 / 101, 4      f32 dewpoint  42, 8 / 64, 8 / 81, 5 / 89, 5 /  98, 4
#   f64 specific  45, 8 / 68, 7 / 87, 5 / 95, 5 / 104, 4      f32 specific  44, 8 / 66, 7 / 85, 5 / 93, 5 / 102, 4
# (without it 50-61 / 72-88 / 91-104 / 99-112 / 108-122); no LDS, no scratch.
HYDROSTATIC_FLAGS = ['-mllvm', '-disable-machine-licm']
# The humidity conversion in front of the CAPE / CIN calls (csrc/xp_humidity.hpp, XP_HUM_RELATIVE / XP_HUM_MIXING_RATIO) takes no
# flag either: a streaming kernel without a level loop to keep constants out of.  No LDS, no scratch; as cross-compiled,
# k_dewpoint_from<T, KIND, VEC> by (T: 'd' / 'f', KIND: XP_HUM_*, VEC: 16-byte runs or one column per lane) -> (VGPRs, waves
# per SIMD), which tests/test_humidity_cpu.py holds the unit to:
HUMIDITY_RESOURCES = {('d', 2, 1): (52, 8), ('d', 2, 0): (41, 8), ('d', 3, 1): (44, 8), ('d', 3, 0): (38, 8),
                      ('f', 2, 1): (52, 8), ('f', 2, 0): (43, 8), ('f', 3, 1): (46, 8), ('f', 3, 0): (40, 8)}
# The fp32-arithmetic surface CAPE / CIN kernel (csrc/xp_cape_f32.hpp, xp_opts.compute = XP_F32): the family units' workgroup
# and flag (e_s / ln tables + the fp32 copy of the family table + the scan slots: 130.3 KB of LDS, one workgroup per CU).
CAPE_F32_FLAGS = ['-DXP_CAPE_THREADS=1024', '-mllvm', '-disable-machine-licm']
UNITS = [('xparcel', 'xparcel.hip', []), ('cape_f32', 'xp_cape_f32_tu.hip', CAPE_F32_FLAGS),
         ('effective', 'xp_effective_tu.hip', EFFECTIVE_FLAGS), ('max_cape', 'xp_max_cape_tu.hip', EFFECTIVE_FLAGS),
         ('wind_layers', 'xp_wind_layers_tu.hip', WIND_LAYERS_FLAGS),
         ('thermo_layers', 'xp_thermo_layers_tu.hip', THERMO_LAYERS_FLAGS),
         ('cape_layers', 'xp_cape_layers_tu.hip', CAPE_LAYERS_FLAGS), ('cape_pick', 'xp_cape_pick_tu.hip', CAPE_PICK_FLAGS), ('ecape', 'xp_ecape_tu.hip', []),
         ('sounding', 'xp_sounding_tu.hip', []), ('isentropic', 'xp_isentropic_tu.hip', []),
         ('hydrostatic', 'xp_hydrostatic_tu.hip', HYDROSTATIC_FLAGS), ('humidity', 'xp_humidity_tu.hip', [])] + [
    (f'cape_{t[0]}{m}', 'xp_cape_tu.hip', [f'-DXP_TU_T={t}', f'-DXP_TU_MODE={m}'] + TU_FLAGS[m])
    for t in ('double', 'float') for m in (0, 1, 2)] + [
    (f'multi_{t[0]}{n}', 'xp_multi_tu.hip', [f'-DXP_TU_T={t}', f'-DXP_MULTI_NP={n}'] + MULTI_FLAGS[n])
    for t in ('double', 'float') for n in sorted(MULTI_FLAGS)]


def build(force=False, verbose=False, jobs=None):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU): the translation units in
    parallel (hipcc -c), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(SRC_DIR, f) for f in sorted(os.listdir(SRC_DIR))] + [INCLUDE]
    if (not force and os.path.exists(LIB_PATH)
            and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in srcs)):
        return LIB_PATH
    libdir = os.path.dirname(LIB_PATH)
    objdir = os.path.join(libdir, 'obj%d' % os.getpid())
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

    def compile_unit(u):
        name, src, defs = u
        obj = os.path.join(objdir, name + '.o')
        cmd = [hipcc] + HIPCC_FLAGS + defs + ['-c', os.path.join(SRC_DIR, src), '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    try:
        with ThreadPoolExecutor(max_workers=jobs or min(len(UNITS), os.cpu_count() or 1)) as ex:
            objs = list(ex.map(compile_unit, UNITS))
        tmp = LIB_PATH + '.tmp%d' % os.getpid()
        cmd = [hipcc, '--offload-arch=gfx950', '-fPIC', '-shared', '-o', tmp] + objs
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(tmp, LIB_PATH)       # atomic: a concurrent loader never sees a half-written library
    finally:
        import shutil
        shutil.rmtree(objdir, ignore_errors=True)
    return LIB_PATH


def csrc_sha():
    """Fingerprint of the kernel sources (csrc/ + the ABI header): profiles taken on the GPU box record it, and bench.py
    only quotes a profile's counters next to a timing when the fingerprints match."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.listdir(SRC_DIR)) + [INCLUDE]:
        path = f if os.path.isabs(f) else os.path.join(SRC_DIR, f)
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


_lib = None
_lock = threading.Lock()
_inited_device = None


def load():
    """dlopen the library (no GPU needed for this)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(f'{LIB_PATH} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                                  '(there is no CPU fallback)')
            # torch ships its own HIP runtime: when torch is going to be used in this process it has to be the first to
            # load one, or the library's hipGetDeviceCount() later reports "no ROCm-capable device" (two runtimes in one
            # process).  torch is plumbing here (device memory, streams), so importing it is not a product dependency.
            try:
                import torch  # noqa: F401
            except Exception:
                pass
            lib = C.CDLL(LIB_PATH)
            for s in SYMBOLS:
                f = getattr(lib, s)
                f.argtypes, f.restype = ARGTYPES[s], C.c_char_p if s == 'xp_last_error' else C.c_int
            _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise XParcelError(rc, load().xp_last_error().decode())


def init(device=None):
    """xp_init on the given (or torch-current, or 0) device."""
    global _inited_device
    lib = load()
    if device is None:
        device = _inited_device if _inited_device is not None else int(os.environ.get('LOCAL_RANK', '0'))
    if _inited_device != device:
        check(lib.xp_init(int(device)))
        _inited_device = device
    return lib
