/*
 * xparcel.h -- C ABI of libxparcel (MI355X / gfx950), the drop-in boundary for the
 * parcel-lifting hot path of traupach/xarray_parcel.
 *
 * The reference has no FFI layer of its own: its boundary is the set of Python
 * functions in modules/parcel_functions.py ("pf.py").  Each entry point below names
 * the reference function it replaces (file:line); the host-side mirror in
 * xarray_parcel_amd/parcel_functions.py keeps the reference's signatures and calls
 * these through ctypes (INTEGRATION.md shows the binding a maintainer of the
 * reference would add).
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer; the library never
 *     allocates caller-visible memory and never frees caller memory;
 *   - arrays are (nlev, ncol): level 0 = surface, pressure strictly decreasing
 *     upwards (README.md:9, pf.py:2319-2320), hPa / K / K, NaN = missing; element
 *     (k, c) of a view lives at data[k*lev_stride + c*col_stride] (strides in
 *     elements).  col_stride == 1 (the (lev, y, x) C-order layout) is the coalesced
 *     fast path; anything else is correct but slower;
 *   - dtype is XP_F32 or XP_F64 for data in memory; arithmetic is fp64 (one exception, on request: xp_opts.compute);
 *   - mem says where a buffer lives: XP_MEM_DEVICE pointers are used in place,
 *     XP_MEM_HOST buffers are staged through internal device scratch (PCIe time
 *     is then part of the call);
 *   - every function returns 0 on success or a negative XP_E* code; the message is
 *     available from xp_last_error() (thread-local).  The reference's data-dependent
 *     asserts (pf.py:131, 1149, 1158) become per-column status bits, not aborts;
 *   - one device per process (the deployment model is one process per GPU): xp_init(device)
 *     binds the library's state -- lookup tables, the e_s / ln / adiabat-family tables -- to that
 *     device, and every call runs there whatever the calling thread's current device is (which
 *     is restored on return).  Calls from several host threads are safe against each other;
 *     replacing tables (xp_set_tables, xp_set_family_table, xp_init on another device) waits for
 *     the device to drain first and must not race with other calls;
 *   - work is enqueued on the hipStream_t passed as `stream` (NULL = the default stream), which
 *     must belong to the library's device.  Device-resident calls return without synchronising
 *     (an asynchronous kernel fault surfaces at the caller's next synchronisation); calls with
 *     host buffers synchronise the stream before returning.
 */
#ifndef XPARCEL_H
#define XPARCEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XP_VERSION 100 /* 0.1.0 */

enum { XP_F32 = 0, XP_F64 = 1 };
enum { XP_MEM_HOST = 0, XP_MEM_DEVICE = 1 };

/* which parcel is lifted (pf.py:1477 / 1557 / 1651 / 1394) */
enum { XP_PARCEL_SURFACE = 0, XP_PARCEL_MOST_UNSTABLE = 1, XP_PARCEL_MIXED_LAYER = 2, XP_PARCEL_EXPLICIT = 3 };
/* XP_PARCEL_OVER_GROUND, a flag OR-ed into xp_parcel.mode: the views are ISOBARIC levels -- what reanalyses and climate
   archives deliver, with values extrapolated below the terrain -- and the surface comes separately: xp_parcel.pressure /
   temperature / dewpoint hold ncol surface values each (hPa, K, K; the views' dtype and mem; the third is always a dewpoint,
   as for explicit parcels, also under XP_HUM_SPECIFIC).  Valid with XP_PARCEL_SURFACE, XP_PARCEL_MOST_UNSTABLE and
   XP_PARCEL_MIXED_LAYER; with XP_PARCEL_EXPLICIT, with any other bit, or with one of the three pointers NULL: XP_E_ARG.
   The RE-BASED COLUMN of column c with the surface values ps, Ts, Tds has nlev + 1 rows:
     k0 = the first level index with p[k0] < ps (plain comparison: a NaN pressure compares false and is dropped with the
          levels below the ground; a level with p == ps is replaced by the surface);
     row 0 = (ps, Ts, Tds);  row 1 + j = level k0 + j;  the remaining rows NaN in all three arrays;
     no level above the ground: row 0 alone;  ps, Ts or Tds NaN: every row NaN.
   With the flag the call IS the same call without it on the re-based (nlev + 1, ncol) arrays, bit for bit: every scalar,
   every status bit, every profile row.  The parcel mode is mode & 3; parcel_index, lfc_index and el_index count re-based
   rows; a profile needs nlev_out >= nlev + 2.  XP_HUM_SPECIFIC: the kept levels are converted as
   xp_dewpoint_from_specific_humidity converts them (stored in the views' dtype) and the call equals that function followed
   by the dewpoint-input call.  The views are read in place whatever their strides -- col_stride == 0 is a device pressure of
   nlev isobars shared by all columns -- by one streaming kernel (csrc/xp_ground.hpp) that writes the re-based grid to
   internal scratch: three (nlev + 1, ncol) arrays for the duration of the call.
   Honoured by xp_cape_cin, xp_cape_cin_multi (every parcel flagged and carrying the same three pointers, or none: XP_E_ARG
   otherwise; the grid is re-based once per call, XP_OPT_FUSE_PARCELS works on it like on any other) and xp_select_parcel.
   xp_rebase_profile and xp_cape_cin_layers, whose outputs would change shape, reject it with XP_E_ARG;
   xp_opts.compute = XP_F32 rejects it by its own rule (mode must be exactly XP_PARCEL_SURFACE). */
enum { XP_PARCEL_OVER_GROUND = 16 };
/* XP_PARCEL_MAX_CAPE, a fifth parcel kind: the departure level with the LARGEST CAPE in the lowest xp_parcel.depth hPa --
   the "most unstable" of the archives that lift a parcel from every level of the window, where XP_PARCEL_MOST_UNSTABLE is
   the reference's rule, the level of highest theta-e.  The two usually agree and part on elevated convection.
   CANDIDATES, those of xp_effective_inflow_layer: a level is valid when p, T and Td are all non-NaN; p0 is the pressure of
     the lowest valid level; the candidates are the valid levels with p >= p0 - depth (plain comparison), in level order.
     depth [hPa] not finite or not > 0: XP_E_ARG.
   CANDIDATE CAPE: CAPE_k = what xp_cape_cin(XP_PARCEL_SURFACE) writes as cape for the views p[k:], T[k:], Td[k:] with the
     call's four CAPE / CIN options; the moist adiabat by the lookup tables under XP_MOIST_TABLE and by the RK4 stepper
     otherwise -- XP_MOIST_FAMILY is treated as exact FOR THE SELECTION ONLY.  Every candidate is lifted: no early stop.
   SELECTION: k* = the lowest candidate whose CAPE_k is the largest.  Walking the candidates upward the first one is taken
     and then replaced only when CAPE_k > best, so a NaN CAPE_k never wins, and when every CAPE is 0 the lowest valid level
     wins: the surface parcel.  A column without candidates has k* = 0.
   The RE-BASED COLUMN has nlev rows: row j = level k* + j for j < nlev - k*, the remaining rows NaN in all three arrays.
   With this mode the call IS the call with XP_PARCEL_SURFACE on the re-based arrays, with the caller's own options --
   XP_MOIST_FAMILY and its transparent exact redo included -- bit for bit: every scalar, every status bit, every profile row
   (nlev_out >= nlev + 1, as for any call).  The one exception: parcel_index = k*, the convention of the most-unstable
   parcel; parcel_pressure / temperature / dewpoint are level k*'s values, lfc_index / el_index count re-based rows, as
   they do for XP_PARCEL_MOST_UNSTABLE.
   Honoured by xp_cape_cin, xp_cape_cin_multi (in any mix with the other kinds, one selection per such parcel; with
   XP_OPT_FUSE_PARCELS the call takes the per-parcel path, as for explicit parcels) and xp_select_parcel (no options: the
   selection runs with the default options and RK4; it writes parcel_index and the three parcel values).  XP_HUM_SPECIFIC
   with this kind: XP_E_ARG; xp_opts.compute = XP_F32 rejects it by its own rule; it does not combine with
   XP_PARCEL_OVER_GROUND (4 | 16 is a bad mode); every other entry point that takes an xp_parcel rejects it.
   COST: one ascent per candidate and column (csrc/xp_max_cape.hpp; ~the open-threshold xp_effective_inflow_layer call)
   plus three (nlev, ncol) scratch arrays for the duration of the call, per such parcel. */
enum { XP_PARCEL_MAX_CAPE = 4 };

/* moist adiabat: XP_MOIST_EXACT integrates MetPy's pseudo-adiabat ODE (what the reference's
   KATs are run with, unit_tests.py:114-140) by RK4 in ln p with steps <= 0.1;
   XP_MOIST_TABLE emulates the reference's lookup tables (pf.py:525-607) against tables given
   to xp_set_tables(). */
enum { XP_MOIST_EXACT = 0, XP_MOIST_TABLE = 1, XP_MOIST_FAMILY = 2 };
/* XP_HUM_SPECIFIC: the moisture view holds specific humidity [kg/kg] (what the reference's data files provide) and is
   converted to dewpoint on load with the xp_dewpoint_from_specific_humidity chain (parcel_test.py:262-266), saving the
   separate pass and the (nlev, ncol) dewpoint array.  Explicit parcels (xp_parcel.dewpoint) stay dewpoints.
   XP_HUM_RELATIVE and XP_HUM_MIXING_RATIO: the moisture m as the archives without a dewpoint deliver it.
     XP_HUM_RELATIVE: the view holds relative humidity over liquid water as a FRACTION (1 = saturated; not percent):
       e = m * e_s(T), e_s Bolton's formula as everywhere in the library.
     XP_HUM_MIXING_RATIO: the view holds the water-vapour mixing ratio [kg/kg]: e = p * m / (eps + m).
     Both: D = 273.15 + 243.5 v / (17.67 - v) with v = ln(e / 6.112) -- MetPy's dewpoint -- evaluated in double.
     VALIDITY: D is NaN unless m > 0 by plain comparison, so a NaN, zero or negative moisture gives NaN.  There is no upper
       bound: rh > 1 gives D > T, exactly as a dewpoint view may hold it.  The IEEE arithmetic of the formula decides
       everything else (infinities, a NaN T or p); the relative kind needs T and not p, the mixing-ratio kind p and not T.
     D is stored in the views' dtype, rounded once, and with either kind the call IS the XP_HUM_DEWPOINT call on D, bit for
     bit: every scalar, every status bit, every profile row, environment_dewpoint included.  Explicit parcels stay
     dewpoints, and so does the surface dewpoint of XP_PARCEL_OVER_GROUND: the levels are converted first and the ground
     cut runs on the result.
     Honoured by xp_cape_cin, xp_cape_cin_multi (converted once per call; XP_OPT_FUSE_PARCELS works on D like on any
     dewpoint grid), xp_cape_cin_layers and xp_effective_inflow_layer.  XP_PARCEL_MAX_CAPE accepts both (its selection
     sees a dewpoint grid); xp_opts.compute = XP_F32 rejects them by its own rule; xp_conv_properties (specific humidity
     by construction) and xp_hydrostatic_height (its own two kinds) do not take them.
     COST: one streaming pass over the moisture and T or p in front of the call (csrc/xp_humidity.hpp; the views are read
     in place whatever their strides, the caller's moisture view is never written) plus one dense (nlev, ncol) scratch
     array for the duration of the call.  Measured on 64 x 1 Mi columns, surface parcel, XP_MOIST_FAMILY:
     the call costs 1.6 x the dewpoint call in fp64 and 1.5 x in fp32. */
enum { XP_HUM_DEWPOINT = 0, XP_HUM_SPECIFIC = 1, XP_HUM_RELATIVE = 2, XP_HUM_MIXING_RATIO = 3 };
/* XP_MOIST_FAMILY: the same pseudo-adiabat ODE, served from a piecewise-polynomial table of its solutions: the parcel's
   VIRTUAL temperature along the adiabat, Tv(ln p ; psi) = T (1 + 0.608 w_s(p, T)) (what pf.py:760-775 feed the CAPE / CIN
   integration), psi = the adiabat's temperature at 1000 hPa (8 pieces of 0.5 in ln p from 1100 hPa to ~20 hPa x 9 pieces
   in psi from 215 to 312 K, degree 8 x 8, 46.7 KB, built at xp_init; specification: oracle/family.py).  Within 1e-6 K
   of the ODE (the RK4 stepper of XP_MOIST_EXACT: 2e-5 K; MetPy's LSODA: 4e-5 ... 4e-4 K), a level costs one Horner
   evaluation instead of an RK4 step, and all of the reference's known-answer tests pass in this mode too.  The parcel
   TEMPERATURE, where asked for (profile output, virtual_temperature_correction off), is the T with that virtual
   temperature at that pressure (Newton on the reference's own formula).  Above the table's top the adiabat continues dry.
   Columns whose label or LCL leave the table (psi outside 215.05 ... 311.95 K, p_lcl outside ~20 ... 1100 hPa) are
   transparently redone with XP_MOIST_EXACT.  Honoured by xp_cape_cin; the component entry points treat it as
   XP_MOIST_EXACT. */
enum { XP_LCL_INTERP_LINEAR = 0, XP_LCL_INTERP_LOG = 1 };
/* xp_opts.flags.  XP_OPT_FUSE_PARCELS: xp_cape_cin_multi lifts its parcels in ONE pass over the grid where it can (see
   there); same results bit for bit, measured SLOWER than one pass per parcel on MI355X, so off by default. */
enum { XP_OPT_FUSE_PARCELS = 1 };
/* xp_opts.flags, bits 4-6: WHICH POSITIVE LAYER the CAPE / CIN and the LFC / EL of a call describe.  The reference's rule
   (lfc_el, pf.py:1124-1138) takes the bottom LFC and the top EL: on a sounding with several separate positive areas --
   capping inversions, elevated convection, dry intrusions -- it adds them all up.  MetPy lets the caller say which one is
   meant (which_lfc / which_el = 'bottom' | 'top' | 'wide' | 'most_cape'); this field does the same for a whole LFC / EL pair.
   The rule is defined on exactly the nodes xp_cape_cin scans for the chosen parcel (the LCL-augmented profile from the parcel
   on), with F+ and F- the running sums of the positive and the negative area of parcel minus environment over ln p
   (xp_cape_cin_layers' formalism, below).
   EVENTS, in the order of the ascent: an UP is an increasing crossing that qualifies as an LFC candidate of lfc_el (above
     the LCL, in the selected set of pf.py:1117-1120), a DOWN a decreasing crossing that qualifies as an EL candidate (above
     the LCL, not in the first interval) -- every one of them, not only the bottom UP and the top DOWN.  A crossing lies at
     the ln p, with the parcel temperature and the interval index, that xp_cape_cin computes for it; F+ and F- "at" a
     crossing are the sums up to it (the interval's triangle below the crossing included).
   POSITIVE LAYERS, numbered 1 ... K upward: an UP while no layer is open opens one: its bottom is this crossing, with
     cL = F+ and nL = F- there; an UP while one is open is ignored.  A DOWN while a layer is open closes it: its top is this
     crossing, with cE = F+ there.  A DOWN while none is open and none has been opened before closes a layer whose bottom is
     the LCL: L = the LCL pressure, lfc_temperature = the LCL's (virtual) temperature, lfc_index = -2, cL and nL the sums at
     the LCL node -- the existing replacement of pf.py:1161-1180 -- unless the crossing lies ON the LCL, within 2e-9 in ln p
     (the window in which xp_cape_cin itself decides "above the LCL" on the last bit of exp / log: a saturated parcel that
     turns negative right above its own level): that layer would have no depth, and the DOWN is ignored.  Any other DOWN is
     ignored.  A layer still open after the
     last node closes at the lowest valid pressure: cE = the final F+, el_pressure / el_temperature NaN, el_index = -1, as
     the existing rule has it when there is no EL.
   SELECTION (K >= 2): XP_OPT_LAYER_LOWEST layer 1, XP_OPT_LAYER_HIGHEST layer K, XP_OPT_LAYER_DEEPEST the largest
     ln L - ln E -- depth in ln p, roughly geometric depth, NOT MetPy's difference in hPa, which favours low layers --
     XP_OPT_LAYER_MOST_CAPE the largest cE - cL.  Walking upward the first layer is taken and then replaced only on a strictly
     greater metric: the lower of equals wins, a NaN metric never wins.
   RESULT (K >= 2): cape = (E < L) ? Rd (cE - cL) : 0, cin = Rd nL (post_zero_cin as ever), lfc_* / el_* the chosen
     layer's, the pressures through the routine that forms xp_cape_cin's; every other scalar -- lcl_*, parcel_*,
     parcel_index, status -- what the default call writes.  Equivalently: cape and cin are xp_cape_cin_base's for the chosen
     lfc_pressure / el_pressure (the lowest valid pressure for an open layer).
   K <= 1: there is nothing to choose, and every choice stores exactly what the default call stores, fallbacks of
     pf.py:1161-1180 included -- bit for bit in XP_MOIST_EXACT and XP_MOIST_TABLE.  (One class apart: a saturated parcel's
     crossing ON its LCL, where xp_cape_cin's own answer hangs on the last bit of exp / log and on the other columns of
     the wavefront; this call always breaks that tie as the reference's expressions do.)
   Honoured by xp_cape_cin and xp_cape_cin_multi (one choice per call; every parcel takes the per-parcel path,
   XP_OPT_FUSE_PARCELS is ignored as for explicit parcels), with all five parcel kinds, XP_PARCEL_OVER_GROUND, and every
   XP_HUM_* (XP_HUM_RELATIVE, XP_HUM_MIXING_RATIO and the ground cut are passes in front: the call IS the call on what they
   produce, bit for bit; XP_HUM_SPECIFIC is converted on load by xp_dewpoint_from_specific_humidity's chain).
   XP_MOIST_EXACT and XP_MOIST_TABLE; XP_MOIST_FAMILY is treated as exact, as in xp_cape_cin_layers.  f32 views are
   converted exactly, all arithmetic is fp64.  pos_cape_neg_cin must be set (F+ and F- are the sign-filtered sums).
   XP_E_ARG, nothing written, for a non-zero field with: a value 5 ... 7; pos_cape_neg_cin == 0; a non-NULL profile (the
   profile does not depend on the choice: the default call provides it); compute = XP_F32; or any other entry point that
   takes an xp_opts (xp_cape_cin_layers, xp_effective_inflow_layer, xp_conv_properties, xp_cape_cin_base).
   With the field 0 nothing changes by a bit and the same kernels run.
   COST (csrc/xp_cape_pick.hpp): one ascent in xp_cape_cin_layers' kernel form, at half the exact-mode kernels' occupancy.
   Measured on 64 x 1 Mi fp64 columns, surface parcel: 1.7 x the XP_MOIST_EXACT default call. */
enum { XP_OPT_LAYER_SHIFT = 4, XP_OPT_LAYER_MASK = 7 << 4,
       XP_OPT_LAYER_ENVELOPE = 0 << 4,   /* bottom LFC, top EL: the reference's rule, the default */
       XP_OPT_LAYER_LOWEST = 1 << 4, XP_OPT_LAYER_HIGHEST = 2 << 4, XP_OPT_LAYER_DEEPEST = 3 << 4, XP_OPT_LAYER_MOST_CAPE = 4 << 4 };

/* error codes */
enum {
    XP_OK = 0,
    XP_E_ARG = -1,          /* null / inconsistent arguments (shape, dtype, mem mismatch)       */
    XP_E_NOT_INIT = -2,     /* xp_init not called                                              */
    XP_E_NO_TABLES = -3,    /* table mode without tables: 'Call load_moist_adiabat_lookups first' (pf.py:60) */
    XP_E_INTERP = -4,       /* 'interpolator must be linear or log' (pf.py:878)                */
    XP_E_HIP = -5,          /* HIP runtime error (message in xp_last_error)                    */
    XP_E_NO_DEVICE = -6     /* no usable gfx950 device                                         */
};

/* per-column status bits (xp_scalars_out.status) */
enum {
    XP_ST_TOP_NAN = 1,          /* 'Top temperature is NaN' condition of pf.py:1149 */
    XP_ST_LCL_NOT_CONVERGED = 2,/* LCL fixed point hit 50 iterations (MetPy raises)  */
    XP_ST_BAD_PRESSURE = 8,     /* a pressure higher than the level below it: outside the input contract (README.md:9,
                                   pf.py:2319-2320); the column's other outputs are unspecified.  (A pressure <= 0 has no
                                   logarithm: it is not tested for as such, but in practice trips this test too.) */
    XP_ST_NAN_PRESSURE = 4,     /* a NaN pressure below the LCL.  The level is treated as MISSING -- exactly as if its
                                   temperature and dewpoint were NaN too: the two intervals that touch it drop out of
                                   every sum and the LCL bracket skips it -- not as the reference's insert_level does
                                   (pf.py:962-966 puts a copy of the LCL into the NaN slot and integrates over the
                                   out-of-order profile).  Contract: tests/test_gpu_parity.py::test_nan_pressure_levels */
    XP_ST_NO_LAYER = 16,        /* xp_downdraft_cape, xp_bunkers_storm_motion: the column does not span the layer (MetPy
                                   raises), every output NaN; xp_storm_relative_helicity: some depth is not spanned, that
                                   depth's outputs NaN */
    XP_ST_BAD_HEIGHT = 32,      /* xp_bunkers_storm_motion, xp_storm_relative_helicity: a height not above the valid level
                                   below it (heights must increase strictly); every output NaN */
    XP_ST_LAYER_OPEN = 64,      /* xp_effective_inflow_layer: the last candidate of the search window passes, i.e.
                                   search_depth (or the column top) cut the layer, which might extend further */
    XP_ST_NO_CCL = 128,         /* xp_sounding_indices: the dewpoint line of the CCL's mixing ratio never crosses the
                                   environment temperature; the three CCL outputs NaN */
    XP_ST_NOT_CONVERGED = 256   /* xp_isentropic_interpolation: the Newton iteration of some target took max_iters steps
                                   without meeting eps; that target's outputs NaN */
};

typedef struct {
    const void *data;
    int32_t dtype;      /* XP_F32 | XP_F64 */
    int32_t mem;        /* XP_MEM_HOST | XP_MEM_DEVICE */
    int64_t nlev, ncol;
    int64_t lev_stride, col_stride; /* in elements.  xp_cape_cin is fastest when its three views share their strides
                                       (non-negative, < 4 GiB per level row): anything else is copied to dense scratch first */
} xp_view;

typedef struct {
    int32_t mode;       /* XP_PARCEL_* (XP_PARCEL_MAX_CAPE included), the first three optionally | XP_PARCEL_OVER_GROUND */
    int32_t reserved;
    double depth;       /* hPa: MU search depth (default 300, pf.py:1558) / ML mixing depth (100, pf.py:1652) */
    /* XP_PARCEL_EXPLICIT: the per-column parcel; XP_PARCEL_OVER_GROUND: the surface.  ncol elements each, same dtype/mem as
       the views; unused otherwise */
    const void *pressure, *temperature, *dewpoint;
} xp_parcel;

typedef struct {
    int32_t virtual_temperature_correction; /* default 1 (pf.py:1396) */
    int32_t lcl_interp;                     /* XP_LCL_INTERP_*; default log (pf.py:1396) */
    int32_t pos_cape_neg_cin;               /* default 1 (pf.py:1293) */
    int32_t post_zero_cin;                  /* default 0 (pf.py:1293) */
    int32_t moist_mode;                     /* XP_MOIST_* */
    int32_t compute;                        /* arithmetic type: XP_F64 (the default), or XP_F32 in xp_cape_cin's one case below */
    int32_t humidity;                       /* XP_HUM_*: what the `dewpoint` view of xp_cape_cin holds */
    int32_t flags;                          /* XP_OPT_* bits; 0 by default */
} xp_opts;

/* xp_opts.compute == XP_F32: fp32 arithmetic in the level walk of xp_cape_cin (csrc/xp_cape_f32.hpp).  Honoured in exactly
   this case, and XP_E_ARG -- the message names the offending argument -- in every other one:
     views      all three XP_F32, in host or device memory, dense or strided (staged like any other call);
     parcel     parcel->mode == XP_PARCEL_SURFACE;
     opts       moist_mode == XP_MOIST_FAMILY, humidity == XP_HUM_DEWPOINT, and virtual_temperature_correction, lcl_interp,
                pos_cape_neg_cin, post_zero_cin at their defaults (1, XP_LCL_INTERP_LOG, 1, 0);
     profile    NULL;
     scalars    CAPE/CIN-only in the sense of xp_scalars_out below: lfc_temperature, el_temperature, lfc_index, el_index and
                status all NULL.  Supported: cape, cin, lcl_pressure, lcl_temperature, lcl_virtual_temperature, lfc_pressure,
                el_pressure, parcel_index, parcel_pressure, parcel_temperature, parcel_dewpoint.
   Every other entry point that takes an xp_opts (xp_cape_cin_multi, xp_conv_properties, xp_effective_inflow_layer,
   xp_cape_cin_layers) rejects XP_F32 with XP_E_ARG.  Nothing that passes XP_F64, or no opts, changes by a bit.
   What fp32 arithmetic promises, against the same call with XP_F64:
     (a) classification  the same decisions for every column: which levels are valid, where parcel minus environment
                         changes sign, which crossing is the LFC and which the EL, whether they exist -- so cape, cin,
                         lfc_pressure and el_pressure are NaN in the same columns.  A node whose fp32 difference is smaller
                         than XP_F32_GUARD (4e-4 K, a derived bound on the fp32 error of that difference), the first node
                         above the LCL where the LCL node's own difference is below 1e-5 of its (the XP_F64 path's tie
                         window at the LCL), a node within 8e-6 (relative) of the LCL pressure, and every node at or below
                         the LCL are evaluated in fp64 by the XP_F64 path's own code.  The bound is derived for levels with
                         1 hPa <= p <= 1100 hPa, 150 K <= Td <= T <= 330 K, e_s(T) <= 0.1 p and a mixing ratio up to 0.04
                         (csrc/xp_cape_f32.hpp); (a) and (b) are promised for columns whose levels lie inside that domain;
     (b) values          cape and cin within 0.5 J/kg (measured: 0.02 J/kg); an LFC / EL that lies in the interval
                         between the nodes a and b within 2 XP_F32_GUARD |ln p_b - ln p_a| / |y_b - y_a| + 2e-7 in ln p, y the
                         parcel-minus-environment virtual temperature; an LFC on the LCL is the LCL bit for bit.
   The LCL and parcel outputs are bit-identical: the column prologue (parcel, LCL, the adiabat's label) stays fp64.  Columns
   the family table cannot serve are redone with XP_MOIST_EXACT in fp64, as for XP_F64.
   Unlike XP_F64, the XP_F32 values of a column are NOT bitwise invariant under a permutation, a slicing or a sharding of
   the columns: which of its nodes take the fp64 code depends on the 63 columns it shares a wavefront with.  The
   classification (a) is invariant; cape, cin, lfc_pressure and el_pressure move within (b). */

/* Per-column outputs; every pointer is nullable (not written when NULL).  Floating outputs have
   `dtype`, all buffers live in `mem`, ncol elements each.  `dtype` and `mem` are this struct's own: for xp_cape_cin,
   xp_cape_cin_multi (per parcel), xp_lfc_el, xp_select_parcel and xp_rebase_profile they need not match the views' (fp32
   grids with fp64 CAPE / CIN, device grids with host scalars, ...); a value is the fp64 result rounded once to `dtype`.
   Anything but XP_F32 / XP_F64 and XP_MEM_HOST / XP_MEM_DEVICE is XP_E_ARG.  The other output structs below
   (xp_dcape_out, xp_effective_layer_out, xp_cape_layers_out, xp_storm_motion_out, xp_srh_out, xp_srh_layers_out,
   xp_wind_layers_out, xp_thermo_layers_out, xp_sounding_out, xp_isentropic_out, xp_hydrostatic_out, xp_ncape_out) must
   match the views' dtype and mem: XP_E_ARG otherwise.
   lfc_index / el_index: index i of the interval (levels i, i+1 of the LCL-augmented profile)
   that holds the chosen crossing; -1 = none; lfc_index -2 = LFC replaced by the LCL (pf.py:1161-1185).
   parcel_index: source level of the lifted parcel (0 for surface, MU level for most-unstable, -1 otherwise).
   Cost: with default options and lfc_temperature, el_temperature, lfc_index, el_index and status all NULL the
   pass runs the CAPE/CIN-only kernels (3-5 % faster); any of the five selects the all-outputs kernels.  Values
   of the arrays that are written do not depend on which kernel ran. */
typedef struct {
    void *cape, *cin;                                   /* J/kg (pf.py:1361-1385) */
    void *lcl_pressure, *lcl_temperature, *lcl_virtual_temperature; /* pf.py:609-682 */
    void *lfc_pressure, *lfc_temperature, *el_pressure, *el_temperature; /* pf.py:1066-1198 */
    int32_t *lfc_index, *el_index, *status, *parcel_index;
    void *parcel_pressure, *parcel_temperature, *parcel_dewpoint; /* the lifted parcel (MU: pf.py:133, ML: pf.py:268-287) */
    int32_t dtype, mem;
} xp_scalars_out;

/* Optional lifted profile with the LCL inserted as an extra level (pf.py:806-931): six
   (nlev_out, ncol) arrays, nlev_out >= nlev + 1.  For MU / ML parcels the profile is re-based
   (levels below the parcel removed, pf.py:1551-1553, 1636-1644) and padded with NaN on top.  Any of the six
   pointers may be NULL: that array is not written (lifted_index, pf.py:1722, reads three of them).  `dtype` and `mem`
   are the profile's own: they need not match the views', nor the xp_scalars_out's of the same call.  Element (j, c) of
   each array lives at [j*lev_stride + c*col_stride]; a device profile may have any non-negative strides (padded rows,
   column-major, every second column: only the addressed elements are written), a host profile must be dense
   (lev_stride == ncol, col_stride == 1); negative strides are XP_E_ARG. */
typedef struct {
    void *pressure, *temperature, *virtual_temperature;                 /* parcel */
    void *environment_temperature, *environment_virtual_temperature, *environment_dewpoint;
    int32_t dtype, mem;
    int64_t nlev_out, lev_stride, col_stride;
    /* lifted_index (pf.py:1722): environment minus parcel temperature of THIS profile at `lifted_index_pressure` hPa
       (the reference: 500), by the log_interp rule of pf.py:1813 applied to the profile's rows -- ncol values of the
       profile's dtype / mem, written in the same pass; NULL = not wanted.  With all six arrays NULL the pass costs
       little more than CAPE / CIN alone -- in family mode, with the default options and a CAPE/CIN-only xp_scalars_out
       (see there), 10 % more: the parcel's plain temperature is then derived from the table's virtual temperature only at
       the two nodes around the level (any other request in family mode derives it at every node: + 65 %). */
    void *lifted_index;
    double lifted_index_pressure;
} xp_profile_out;

/* reference-format moist-adiabat lookup tables (pf.py:447-523), host memory, copied to the device */
typedef struct {
    int64_t n_pressure, n_temperature, n_adiabat;
    double p_max, p_step;       /* index-grid pressures  p_max - i*p_step   (1100 ... 2.5, pf.py:447-448) */
    double t_min, t_step;       /* index-grid temperatures t_min + j*t_step (173 ... 315.98, pf.py:449-450) */
    const uint16_t *index;      /* [n_pressure][n_temperature] adiabat number, 0 = NaN */
    const float *adiabats;      /* [n_adiabat][n_pressure], pressure ASCENDING (pf.py:54) */
} xp_tables;

int xp_version(void);

/* Select the device and create the library state; idempotent.  Replaces the module-global set-up of
   pf.py:18-21.  device = HIP device ordinal. */
int xp_init(int device);

/* pf.py:39-61 load_moist_adiabat_lookups: hand over tables (generated by
   xarray_parcel_amd.adiabat_tables or loaded from its cache file). */
int xp_set_tables(const xp_tables *tables);
int xp_tables_loaded(void);

/* The coefficient table of XP_MOIST_FAMILY as [n_lnp][n_label] doubles: n_lnp = 648 rows (x-piece, power of z, power of s,
   C-order), n_label = 9 psi-pieces (no reference counterpart: the reference's tables are the XP_MOIST_TABLE ones).  Read
   it back (out may be NULL to query the shape) or replace it, e.g. with the oracle's independently built copy in the
   parity tests. */
int xp_family_table(double *out, int64_t *n_lnp, int64_t *n_label);
int xp_set_family_table(const double *table, int64_t n_lnp, int64_t n_label);

/* pf.py:1394-1475 cape_cin and its three drivers: surface_based_cape_cin (pf.py:1477),
   most_unstable_cape_cin (pf.py:1557), mixed_layer_cape_cin (pf.py:1651); with `profile` non-NULL
   also parcel_profile_with_lcl (pf.py:806) + lfc_el (pf.py:1066) in the same pass. */
int xp_cape_cin(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                const xp_parcel *parcel, const xp_opts *opts,
                xp_scalars_out *scalars, xp_profile_out *profile, void *stream);

/* Several parcels of the SAME grid in one call -- what the reference's products do with three calls over the same three
   arrays: most_unstable_cape_cin + mixed_layer_cape_cin (BASELINE config 5; pf.py:1557, 1651), and the most-unstable,
   100 hPa and 50 hPa mixed-layer parcels of conv_properties (pf.py:1984-2006).  parcels[i] / scalars[i] / profiles[i]
   (profiles may be NULL) describe parcel i, nparcel = 1...3.  Results are bit-identical to nparcel separate xp_cape_cin
   calls; by default that is also how the work is done (one pass per parcel, back to back on the stream).  With
   XP_OPT_FUSE_PARCELS in opts->flags, and XP_MOIST_FAMILY, dewpoint input, two surface / most-unstable / mixed-layer
   parcels and no profiles, the parcels are lifted in ONE pass (csrc/xp_multi.hpp): every level above the LCLs is read
   once and its ln p and environment virtual temperature evaluated once for both. */
int xp_cape_cin_multi(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                      int32_t nparcel, const xp_parcel *parcels, const xp_opts *opts,
                      xp_scalars_out *scalars, xp_profile_out *profiles, void *stream);

/* --- component entry points (used by the KATs and by the host-side mirrors) ------------------- */

/* pf.py:609-682 lcl: n parcels -> LCL pressure / temperature / virtual temperature. */
int xp_lcl(int64_t n, int32_t dtype, int32_t mem, const void *parcel_pressure, const void *parcel_temperature,
           const void *parcel_dewpoint, void *lcl_pressure, void *lcl_temperature,
           void *lcl_virtual_temperature, int32_t *status, void *stream);

/* pf.py:291-316 dry_lapse and pf.py:525-607 moist_lapse: parcel (ncol values) lifted to every level of
   `pressure`; out has the layout of `pressure`.  parcel_pressure NULL = level 0 (pf.py:549-550). */
int xp_dry_lapse(const xp_view *pressure, const void *parcel_temperature, const void *parcel_pressure,
                 void *out, void *stream);
int xp_moist_lapse(const xp_view *pressure, const void *parcel_temperature, const void *parcel_pressure,
                   int32_t moist_mode, void *out, void *stream);

/* pf.py:712-780 parcel_profile (no LCL level): parcel temperature and virtual temperature on the
   levels of `pressure` + LCL scalars (nullable). */
int xp_parcel_profile(const xp_view *pressure, const void *parcel_pressure, const void *parcel_temperature,
                      const void *parcel_dewpoint, int32_t moist_mode, void *temperature_out,
                      void *virtual_temperature_out, void *lcl_pressure, void *lcl_temperature,
                      void *lcl_virtual_temperature, void *stream);

/* pf.py:1066-1198 lfc_el on caller-supplied profiles (parcel / environment temperature of any kind). */
int xp_lfc_el(const xp_view *pressure, const xp_view *parcel_temperature, const xp_view *temperature,
              const void *lcl_pressure, const void *lcl_temperature, xp_scalars_out *out, void *stream);

/* pf.py:1291-1392 cape_cin_base on caller-supplied profiles and LFC / EL pressures. */
int xp_cape_cin_base(const xp_view *pressure, const xp_view *temperature, const xp_view *parcel_temperature,
                     const void *lfc_pressure, const void *el_pressure, const xp_opts *opts,
                     void *cape, void *cin, void *stream);

/* pf.py:102-135 most_unstable_parcel, pf.py:229-289 mixed_parcel: parcels only (scalars->parcel_*,
   parcel_index). */
int xp_select_parcel(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                     const xp_parcel *parcel, xp_scalars_out *out, void *stream);

/* pf.py:137-162 mixed_layer: pressure-weighted layer mean of one variable over the lowest `depth` hPa. */
int xp_mixed_layer(const xp_view *pressure, const xp_view *variable, double depth, void *out, void *stream);

/* --- SURVEY 8(f) "next" items built on the same device code ------------------------------------------ */

/* pf.py:389-445 wet_bulb_temperature (Normand's rule): for every element, lift to the LCL (pf.py:609) and come back down
   the moist adiabat to the element's own pressure (pf.py:525).  out has the layout of `pressure`. */
int xp_wet_bulb_temperature(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                            int32_t moist_mode, void *out, void *stream);

/* metpy.calc.downdraft_cape (MetPy 1.4; the reference has no counterpart): downdraft CAPE of every column.  Levels where
   p, T or Td is NaN are dropped.  The layer runs from layer_bottom (b, MetPy: 700 hPa) up layer_depth (MetPy: 200 hPa) to
   u = b - layer_depth: every level with u <= p <= b (np.isclose counting as equal), plus b and u themselves where no layer
   level is close to them, with T and Td interpolated linearly in ln p.  The start point p0 is the first layer point, in
   order of decreasing pressure, with the smallest Bolton theta_e; its wet-bulb temperature wb0 (xp_wet_bulb_temperature's
   chain) starts a moist descent (xp_moist_lapse from (p0, wb0)) through every level with p >= p0, and
       DCAPE = -Rd * trapz(Tv_env - Tv_parcel, ln p)  [J/kg]  over those levels,
   Tv in MetPy's form T (w + eps) / (eps (1 + w)) -- not the T (1 + 0.608 w) of the CAPE path -- with w the saturation
   mixing ratio at Td (environment) or at the parcel temperature (the parcel is saturated).  Moist modes as in
   xp_wet_bulb_temperature (XP_MOIST_FAMILY runs the RK4 descent).  Every output may be NULL; the outputs share the views'
   dtype and mem.  Strided device views are read in place. */
typedef struct {
    void *dcape;              /* J/kg, ncol */
    void *start_pressure;     /* hPa: p0 (a level's pressure or an added bound) */
    void *start_temperature;  /* K: wb0 */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_LCL_NOT_CONVERGED (the start point's LCL) */
    void *parcel_temperature; /* dense C-order (nlev, ncol): Tp on the down levels, NaN elsewhere */
    int32_t dtype, mem;
} xp_dcape_out;
int xp_downdraft_cape(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                      double layer_bottom, double layer_depth, int32_t moist_mode, xp_dcape_out *out, void *stream);

/* The effective inflow layer of Thompson et al. (2007; the reference and MetPy 1.4 have no counterpart): the lowest
   contiguous run of levels whose lifted parcels have CAPE >= cape_min (100 J/kg) and CIN >= cin_min (-250 J/kg; CIN is
   <= 0 in this library).  `height` (same shape, dtype and mem as the other views) may be NULL.
   A level is VALID when p, T and Td are all non-NaN.  With p0 the pressure of the lowest valid level, the CANDIDATES are
   the valid levels with p >= p0 - search_depth (plain comparison; 300 hPa is the library's most-unstable default), in
   level order.  Invalid levels are skipped: they neither start, extend nor close the layer.
   Candidate k is lifted exactly as xp_cape_cin lifts the surface parcel of the column cut off below k:
       CAPE_k, CIN_k = xp_cape_cin(XP_PARCEL_SURFACE) on the views p[k:], T[k:], Td[k:] with the same options,
   NaN handling above k included, and passes when CAPE_k >= cape_min && CIN_k >= cin_min.  A candidate without a level
   above it is lifted like any other (a one-level view: CAPE 0).
   base = the first passing candidate; top = the last passing candidate before the first failing candidate above base, or
   the last candidate if none fails.  Candidates above the first failure after base are not lifted.
   base_height / top_height: the height of that level MINUS the height of the lowest valid level (a surface-based layer has
   base_height == 0.0 exactly; NaN without `height`) -- the height convention of xp_storm_relative_helicity_layers.
   base_index / top_index: level indices, -1 = none.  candidate_cape / candidate_cin: dense C-order (nlev, ncol), what was
   computed for every level that was lifted -- bit for bit what xp_cape_cin writes for that view -- and NaN elsewhere.
   status: XP_ST_NO_LAYER when no candidate passes (floats NaN, indices -1); XP_ST_LAYER_OPEN when the last candidate of the
   window passes; XP_ST_LCL_NOT_CONVERGED ORed over the candidates lifted; XP_ST_BAD_PRESSURE as in xp_cape_cin (ORed likewise).
   opts: the four CAPE / CIN options and moist_mode (XP_MOIST_EXACT, XP_MOIST_TABLE; XP_MOIST_FAMILY is treated as exact);
   humidity XP_HUM_DEWPOINT, XP_HUM_RELATIVE or XP_HUM_MIXING_RATIO.  Non-finite thresholds, search_depth <= 0 or not finite,
   mismatched views and XP_HUM_SPECIFIC return XP_E_ARG.  Every output may be NULL; the outputs share the views' dtype and
   mem.  Strided device views are read in place. */
typedef struct {
    void *base_pressure, *top_pressure;   /* hPa, ncol: the pressures of the levels base_index / top_index */
    void *base_height, *top_height;       /* m above the lowest valid level, ncol */
    int32_t *base_index, *top_index, *status;
    void *candidate_cape, *candidate_cin; /* J/kg, dense C-order (nlev, ncol), NaN where the level was not lifted */
    int32_t dtype, mem;
} xp_effective_layer_out;
int xp_effective_inflow_layer(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                              const xp_view *height, double cape_min, double cin_min, double search_depth,
                              const xp_opts *opts, xp_effective_layer_out *out, void *stream);

/* CAPE and CIN over 1 ... 4 per-column pressure layers of ONE ascent (0-3 km CAPE, hail-growth-zone CAPE; the reference
   and MetPy 1.4 have no counterpart).  Views, parcel and options as in xp_cape_cin; bottom and top are arrays of nlayer
   pointers to ncol pressures each [hPa], in the views' dtype and mem; `bottom`, or any bottom[i], may be NULL.
   The NODES are exactly the nodes xp_cape_cin scans for the chosen parcel: the levels from the parcel's first level, the
   LCL node, and the prepended mixed-layer parcel where there is one; each with X = ln p and y = parcel - environment
   (virtual temperatures under the correction switch).  y(x) is piecewise linear in ln p through the nodes, with its zeros
   where the scan puts them; F+(x) and F-(x) are the positive and the negative area of y from the first node up to x (an
   interval with a NaN end contributes nothing): at every node the running sums xp_cape_cin itself keeps.  With L the LFC
   (or the LCL that replaces it), E the EL (or the lowest valid pressure when there is none) and cL = F+(ln L),
   cE = F+(ln E), nL = F-(ln L) -- the terms of xp_cape_cin's own CAPE = Rd (cE - cL), CIN = Rd nL -- layer i with the
   bounds pb > pt has
       cape[i] = (E < L)  ? Rd * max(0, min(cE, F+(ln pt)) - max(cL, F+(ln pb))) : 0.0
       cin[i]  = isnan(L) ? 0.0 : Rd * min(0, max(nL, F-(ln pt)) - F-(ln pb))
   i.e. the positive area inside the layer between LFC and EL, and the negative area inside the layer below the LFC
   (F+ never decreases and F- never increases with height, so the min / max form is exact).
   Bottom bound: a NULL array, a NaN pb, or a pb above the first node's pressure means "from the first node" (F = 0).
   Top bound: a pt below the last valid node's pressure means "to the top" (F = the final sums): bottom NULL and a tiny pt
   give total_cape / total_cin bit for bit.  A NaN pt, or pt >= pb with both non-NaN, gives NaN for that layer and
   XP_ST_NO_LAYER for the column; the other layers are unaffected.  A NaN parcel or LCL gives 0.0 for every (valid) layer,
   as xp_cape_cin gives the column.  A bound inside an interval: F there is the sum below plus the area of the part of
   the interval up to the bound, y at the bound linear in ln p between the two nodes -- one trapezoid, or the lower
   triangle plus part of the upper one when the bound lies above the interval's zero; ln of a bound is the library log.
   F is continuous, so on which side of a node a bound within an ulp of it falls does not matter (nothing bit-exact is
   promised there).
   total_cape, total_cin, lfc_pressure, el_pressure, lcl_pressure and the other status bits are what xp_cape_cin writes
   for the same arguments.  opts: pos_cape_neg_cin must be set (cin[i] <= 0 by construction, so post_zero_cin changes
   nothing); moist_mode XP_MOIST_EXACT or XP_MOIST_TABLE (XP_MOIST_FAMILY is treated as exact); humidity XP_HUM_DEWPOINT,
   XP_HUM_RELATIVE or XP_HUM_MIXING_RATIO.  nlayer outside 1 ... 4, a NULL top or top[i], mismatched views, XP_HUM_SPECIFIC,
   pos_cape_neg_cin == 0 and an unknown moist_mode return XP_E_ARG; a bad lcl_interp XP_E_INTERP.  Every output may be
   NULL; the outputs share the views' dtype and mem. */
typedef struct {
    void *cape[4], *cin[4];               /* J/kg, ncol each, per layer (entries past nlayer unused) */
    void *total_cape, *total_cin;         /* J/kg, ncol: the whole ascent, as xp_cape_cin */
    void *lfc_pressure, *el_pressure, *lcl_pressure;   /* hPa, ncol */
    int32_t *status;          /* xp_cape_cin's bits | XP_ST_NO_LAYER */
    int32_t dtype, mem;
} xp_cape_layers_out;
int xp_cape_cin_layers(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint, const xp_parcel *parcel,
                       const xp_opts *opts, int32_t nlayer, const void *const *bottom, const void *const *top,
                       xp_cape_layers_out *out, void *stream);

/* pf.py:1758-1811 linear_interp / pf.py:1813-1828 log_interp: value of `variable` at coordinate `at` (one value per
   column, or a single value for all when at_is_scalar) between the bracketing levels of `coords`; duplicates of a
   bracketing coordinate are averaged, no extrapolation (NaN).  log_coords != 0 interpolates in ln(coords), ln(at).
   Used by lifted_index (pf.py:1722), deep_convective_index (pf.py:1830), isobar_temperature (pf.py:2193). */
int xp_interp_level(const xp_view *coords, const xp_view *variable, const void *at, int32_t at_is_scalar,
                    int32_t log_coords, void *out, void *stream);
/* The same rule for nvar (1..4) variables at ntarget (1..4) coordinates in one pass over the column: what conv_properties
   (pf.py:1951) needs of deep_convective_index (pf.py:1830: T, Td at 850 hPa), lapse_rate (pf.py:2102: T, z at 700 and 500)
   and isobar_temperature (pf.py:2193: T at 500) is one call instead of seven.  out[v * ntarget + j] (ncol values each,
   NULL = not wanted) = variable v at coordinate at[j]. */
int xp_interp_levels(const xp_view *coords, int32_t nvar, const xp_view *const *variables, int32_t ntarget, const double *at,
                     int32_t log_coords, void *const *out, void *stream);

/* metpy.calc.dewpoint_from_specific_humidity in its MetPy 1.4.1 form, the front step of the reference's harness and
   products (parcel_test.py:262-266, pf.py:1889-1894, 1969-1974): w = q/(1-q), RH = w / w_s(p, T),
   Td = dewpoint(RH e_s(T)) [K].  Element-wise; out has the layout of `pressure`.  No reference fixture pins this
   function: parity unpinned beyond the oracle's restatement. */
int xp_dewpoint_from_specific_humidity(const xp_view *pressure, const xp_view *temperature,
                                       const xp_view *specific_humidity, void *out, void *stream);

/* pf.py:2137-2158 freezing_level_height (and melting_level_height, pf.py:2160-2191, on the wet-bulb field): the
   smallest x over all intersections (find_intersections pf.py:992-1064, linear in x) of the profile a(x) with the
   constant `value`; NaN where the profile never crosses it.  One value per column. */
int xp_crossing_level(const xp_view *x, const xp_view *a, double value, void *out, void *stream);

/* pf.py:684-710 mixing_ratio: w = RH(T, Td) * w_s(p, T) [kg/kg], element-wise (MetPy 1.4.1 forms, pf.py:698-704); out has
   the layout of `temperature`.  (virtual_temperature, pf.py:782-804, is T (1 + 0.608 w): plain arithmetic in the mirror.) */
int xp_mixing_ratio(const xp_view *temperature, const xp_view *dewpoint, const xp_view *pressure, void *out, void *stream);

/* pf.py:1951-2100 conv_properties, the reference's product bundle, in ONE call: the q -> dewpoint front step and the NaN mask,
   most-unstable (250 hPa), 100 hPa and 50 hPa mixed-layer CAPE / CIN with their lifted indices (pf.py:1722) out of the same
   passes, the three deep convective indices (pf.py:1830), the 700-500 hPa lapse rate (pf.py:2102), the 500 hPa temperature
   (pf.py:2193), freezing and melting level (pf.py:2137, 2160 with the 1/3-rule wet bulb), the 0-6 km shear (pf.py:2216) and the
   mixing ratio of the most-unstable parcel (pf.py:2053-2059); points with a NaN anywhere in pressure / temperature / humidity /
   dewpoint are blanked unless ignore_nans (pf.py:2097-2098).  Everything that is not parcel lifting is one pass over the four
   grids plus one per-point kernel (csrc/xp_bundle.hpp); scratch (the dewpoint array, per-point temporaries) is stream-ordered
   and internal.  The four (nlev, ncol) views share dtype and mem; the wind views are (nwind, ncol) on their own vertical;
   all seven views live in one mem and the options are checked on an empty grid too (XP_E_ARG / XP_E_INTERP otherwise);
   surface winds and every output are ncol values of that dtype in that mem (positive_shear: int32 0 / 1); NULL outputs are
   skipped.  opts: moist_mode and the CAPE / CIN options of xp_cape_cin (humidity is ignored: the input IS specific humidity). */
typedef struct {
    const xp_view *pressure, *temperature, *specific_humidity, *height_asl;
    const xp_view *wind_u, *wind_v, *wind_height_above_surface;
    const void *surface_wind_u, *surface_wind_v;
} xp_conv_in;
typedef struct {
    void *mu_cape, *mu_cin, *mu_mixing_ratio, *mu_lifted_index, *mu_dci;
    void *mixed_100_cape, *mixed_100_cin, *mixed_100_lifted_index, *mixed_100_dci;
    void *mixed_50_cape, *mixed_50_cin, *mixed_50_lifted_index, *mixed_50_dci;
    void *lapse_rate_700_500, *temp_500, *freezing_level, *melting_level;
    void *shear_u, *shear_v, *shear_magnitude;
    int32_t *positive_shear;
} xp_conv_out;
int xp_conv_properties(const xp_conv_in *in, const xp_opts *opts, int32_t ignore_nans, xp_conv_out *out, void *stream);

/* ---- Per-point products on top of the bundle (no parcel lifting: array arithmetic in the reference) --------------------
   n values each, of `dtype`, in `mem`; flags are int32 0 / 1. */

/* pf.py:2216-2259 wind_shear: the wind at shear_height [m] (linear interpolation in height over the (nwind, ncol) views,
   pf.py:1758 rule) minus the surface wind; outputs nullable. */
int xp_wind_shear(const xp_view *wind_u, const xp_view *wind_v, const xp_view *height, const void *surface_wind_u,
                  const void *surface_wind_v, double shear_height, void *shear_u, void *shear_v, void *shear_magnitude,
                  int32_t *positive_shear, void *stream);

/* pf.py:2261-2306 significant_hail_parameter (SPC SHIP) with the reference's validity windows. */
int xp_significant_hail_parameter(int64_t n, int32_t dtype, int32_t mem, const void *mucape, const void *mixing_ratio,
                                  const void *lapse, const void *temp_500, const void *shear, const void *flh, void *out,
                                  void *stream);

/* pf.py:2323-2407 storm_proxies from the outputs of xp_conv_properties: nine flags (each nullable) and SHIP. */
typedef struct {
    const void *mu_cape, *mu_mixing_ratio, *mixed_100_cape, *mixed_100_cin, *mixed_100_lifted_index, *mixed_100_dci;
    const void *mixed_50_cape, *mixed_50_cin, *lapse_rate_700_500, *temp_500, *freezing_level, *shear_magnitude;
    const int32_t *positive_shear;
} xp_proxies_in;
typedef struct {
    int32_t *craven2004, *kunz2007, *trapp2007, *marsh2009, *allen2011, *allen2014, *eccel2012, *mohr2013, *ship_0_1;
    void *ship;
} xp_proxies_out;
int xp_storm_proxies(int64_t n, int32_t dtype, int32_t mem, const xp_proxies_in *in, xp_proxies_out *out, void *stream);

/* ---- Kinematics: storm motion, helicity and the composites built on them (MetPy 1.4; the reference has none) ----------
   Column entry points: (nlev, ncol) views of one shape, dtype and mem, level 0 at the surface.  A level where any input is
   NaN is dropped.  Ordering is checked on the levels read -- up to and including the first level beyond the deepest top:
   a height not above the valid level below it gives XP_ST_BAD_HEIGHT, a pressure not below it XP_ST_BAD_PRESSURE, and
   the column's outputs are NaN.  "close" is np.isclose with its defaults, |x - y| <= 1e-8 + 1e-5 |y|.  Arithmetic is
   fp64.  Every output may be NULL; the outputs share the views' dtype and mem; per-column inputs are ncol elements in
   that dtype and mem.  Strided device views are read in place. */

/* metpy.calc.bunkers_storm_motion: right mover, left mover and 0-6 km mean wind of every column, from pressure, u, v and
   height on one vertical (the caller supplies the pressure on the wind levels).  With z0, p0 the lowest valid level,
   M(zb, d) is the layer mean of MetPy's weighted_continuous_average / get_layer:
     pb = np.interp(zb, z, p), pt = np.interp(zb + d, z, p) (linear in height, exact at a level); the points are the levels
     with pt <= p <= pb (close counting as inside), plus pb and pt where no point is close to them, u and v there linear
     in ln p between the levels on either side; M = trapz(u, p) / (p_last - p_first) in order of decreasing pressure.
   mean = M(z0, 6000 m), low = M(z0, 500 m), high = M(z0 + 5500 m, 500 m), shear = high - low,
   rdev = (shear_v, -shear_u) * 7.5 / hypot(shear), right = mean + rdev, left = mean - rdev [m/s].
   A column with z0 + 6000 > max z (plain comparison: MetPy raises) gets XP_ST_NO_LAYER and NaN.  Zero shear gives NaN
   movers (0/0).  One pass: a level below the one that brackets z0 + 5500 m is not looked back at, which matters only
   for levels closer than 1e-5 (relative) in pressure. */
typedef struct {
    void *right_u, *right_v, *left_u, *left_v, *mean_u, *mean_v;   /* m/s, ncol each */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_HEIGHT | XP_ST_BAD_PRESSURE */
    int32_t dtype, mem;
} xp_storm_motion_out;
int xp_bunkers_storm_motion(const xp_view *pressure, const xp_view *u, const xp_view *v, const xp_view *height,
                            xp_storm_motion_out *out, void *stream);

/* metpy.calc.storm_relative_helicity (get_layer_heights with_agl) for 1 ... 4 depths in one pass.  Heights are made
   relative to the lowest valid level, h = z - z_first; with surface_u / surface_v (both or neither; dropped where NaN)
   the point (0 m, su, sv) comes first and heights are used as given (wind_height_above_surface).  For depth d, top =
   bottom + d: the points are the levels with bottom <= h <= top (close counting as inside), plus bottom and top where no
   such level EQUALS them (MetPy tests with `in`, not isclose), u and v there linear in height.  With the storm motion
   (storm_u, storm_v; NULL = 0, MetPy's default) term_i = (u[i+1]-cu)(v[i]-cv) - (u[i]-cu)(v[i+1]-cv); positive = sum of
   the terms > 0, negative = sum of the terms < 0, total = positive + negative [m^2/s^2].  A depth with top > max h or
   bottom < min h (plain comparison; MetPy returns a partial sum) is not spanned: its outputs are NaN and the column's
   status gets XP_ST_NO_LAYER.  A NaN storm motion gives NaN.  bottom >= 0 and every depth > 0, finite. */
typedef struct {
    void *positive[4], *negative[4], *total[4];   /* m^2/s^2, ncol each, per depth (entries past ndepth unused) */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_HEIGHT */
    int32_t dtype, mem;
} xp_srh_out;
int xp_storm_relative_helicity(const xp_view *height, const xp_view *u, const xp_view *v, const void *surface_u,
                               const void *surface_v, const void *storm_u, const void *storm_v, double bottom,
                               int32_t ndepth, const double *depth, xp_srh_out *out, void *stream);

/* Helicity and bulk wind difference between PER-COLUMN bounds: 1 ... 4 layers that share a bottom, one upward pass.  Views,
   surface wind and storm motion as in xp_storm_relative_helicity; bottom and top[i] are ncol values each (the views' dtype
   and mem) in that function's own height convention -- above the lowest valid level, or as given when surface winds are
   passed: what xp_effective_inflow_layer writes to base_height / top_height.  Point selection, the linear-in-height
   interpolation, the `in`-not-isclose rule for added bound points, the term and the sign-filtered sums are those of
   xp_storm_relative_helicity with bottom[c], top[i][c] in place of bottom, bottom + depth[i]: with constant arrays the
   helicity outputs are bit-identical to it.  shear_u[i] / shear_v[i] = the ground-relative wind at top[i][c] minus the wind
   at bottom[c], each linear in HEIGHT between the levels on either side (a level exactly on the bound gives its own wind):
   the rule of xp_wind_shear, NOT MetPy's bulk_shear, which interpolates in ln p.  A NaN bound, top <= bottom, bottom < 0 or
   a layer the column does not span gives NaN for that layer and XP_ST_NO_LAYER; XP_ST_BAD_HEIGHT as above.  A NaN storm
   motion gives NaN helicity (the shear does not depend on it). */
typedef struct {
    void *positive[4], *negative[4], *total[4];   /* m^2/s^2, ncol each, per layer (entries past nlayer unused) */
    void *shear_u[4], *shear_v[4];                /* m/s, ncol each, per layer */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_HEIGHT */
    int32_t dtype, mem;
} xp_srh_layers_out;
int xp_storm_relative_helicity_layers(const xp_view *height, const xp_view *u, const xp_view *v, const void *surface_u,
                                      const void *surface_v, const void *storm_u, const void *storm_v, const void *bottom,
                                      int32_t nlayer, const void *const *top, xp_srh_layers_out *out, void *stream);

/* metpy.calc.significant_tornado, per point in MetPy's operation order (NaN propagates):
   lcl_term = (2000 - clip(lcl_height, 1000, 2000)) / 1000; shr = (shear < 12.5 ? 0 : min(shear, 30)) / 20;
   stp = (sbcape * lcl_term * srh * shr) / (1500 * 150).  n elements of dtype in mem each; no argument may be NULL. */
int xp_significant_tornado(int64_t n, int32_t dtype, int32_t mem, const void *sbcape, const void *lcl_height,
                           const void *srh, const void *shear, void *out, void *stream);

/* metpy.calc.supercell_composite, per point (NaN propagates): shr = (shear < 10 ? 0 : min(shear, 20)) / 20;
   scp = (mucape / 1000) * (srh / 50) * shr.  As xp_significant_tornado. */
int xp_supercell_composite(int64_t n, int32_t dtype, int32_t mem, const void *mucape, const void *srh, const void *shear,
                           void *out, void *stream);

/* The wind over 1 ... 4 caller-chosen layers in one upward pass: metpy.calc.mean_pressure_weighted and bulk_shear (the ln p
   one), the wind at each layer's bottom and the layer's strongest wind.  pressure, u, v and (nullable) height on one vertical;
   a supplied height takes part in the NaN drop and in the ordering check.  With p0, z0 the lowest valid level, layer i is
     XP_LAYER_PRESSURE        pb = bottom hPa (NaN: p0), pt = top hPa;
     XP_LAYER_PRESSURE_DEPTH  pb as above, pt = pb - top: MetPy's bottom=, depth= in hPa;
     XP_LAYER_HEIGHT          bottom, top in metres above z0 (NaN bottom: 0): pb = np.interp(z0 + bottom, z, p),
                              pt = np.interp(z0 + top, z, p), linear in height and exact at a level (the bound rule of
                              xp_bunkers_storm_motion); needs height.
   The layer's points are those of MetPy's get_layer: the valid levels with pt <= p <= pb (close counting as inside), plus pb
   and pt themselves where no selected level is close to them, u and v there linear in ln p between the levels on either
   side, in order of decreasing pressure (P, U, V).  Per layer, ncol values each:
     mean_u, mean_v      trapz(U P, P) / (0.5 (P_last^2 - P_first^2));
     shear_u, shear_v    the wind at the last point (the top) minus the wind at the first (the bottom);
     bottom_u, bottom_v  the wind at the first point;
     max_u, max_v, max_pressure   the point of largest hypot(u, v), the first such point winning ties: the layer's strongest
                         wind, since speed is convex along a linearly interpolated segment.
   A layer with pt >= pb, with pb > p0, with pt below the smallest valid pressure (plain comparisons: MetPy raises) or, by
   height, with a bound above the highest valid height gets NaN and the column XP_ST_NO_LAYER; the other layers are not
   affected.  Levels are read up to and including the first one beyond the deepest top (every level, while some layer's top
   has not been reached).  One pass: only the level just below the one that first reaches a bottom bound is looked back at,
   which matters for levels closer than 1e-5 (relative) in pressure.  XP_E_ARG: nlayer outside 1 ... 4, an unknown kind, a
   non-finite top, an infinite bottom, a depth <= 0 (XP_LAYER_PRESSURE_DEPTH's top; top <= bottom by height), a negative
   bottom height, a layer by height without height. */
enum { XP_LAYER_PRESSURE = 0, XP_LAYER_PRESSURE_DEPTH = 1, XP_LAYER_HEIGHT = 2 };
typedef struct { int32_t kind; int32_t reserved; double bottom, top; } xp_wind_layer;
typedef struct {
    void *mean_u[4], *mean_v[4], *shear_u[4], *shear_v[4], *bottom_u[4], *bottom_v[4];   /* m/s, ncol each, per layer */
    void *max_u[4], *max_v[4], *max_pressure[4];                                         /* m/s, m/s, hPa */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_HEIGHT | XP_ST_BAD_PRESSURE */
    int32_t dtype, mem;
} xp_wind_layers_out;
int xp_wind_layers(const xp_view *pressure, const xp_view *u, const xp_view *v, const xp_view *height, int32_t nlayer,
                   const xp_wind_layer *layers, xp_wind_layers_out *out, void *stream);

/* Temperature and humidity over 1 ... 4 caller-chosen layers in one upward pass: metpy.calc.precipitable_water, the layer means
   of mixing ratio and relative humidity, thickness and lapse rate between the bounds, and the layer's extremes of equivalent
   potential temperature.  pressure [hPa] and the nullable temperature, dewpoint [K] and height [m] on one vertical, as
   (nlev, ncol) views of one shape, dtype and mem.  A level is valid when every SUPPLIED view is non-NaN there; the others
   are dropped.  p0, z0: the lowest valid level.  A supplied height takes part in the ordering check.  All arithmetic is fp64,
   without contraction.
   At every valid level, once, shared by the layers: e = e_s(Td), es = e_s(T) (Bolton's formula, as everywhere in the
   library), w = eps e / (p - e), rh = e / es, th = theta_e(p, T, Td) (Bolton's eq. 39, metpy.calc.equivalent_potential_
   temperature).
   The layer kinds and the points are those of xp_wind_layers: XP_LAYER_PRESSURE, XP_LAYER_PRESSURE_DEPTH, XP_LAYER_HEIGHT give
   pb and pt as there; the points are the valid levels with pt <= p <= pb (close counting as inside) plus pb and pt themselves
   where no selected level is close to them, in order of decreasing pressure.  At an added bound point T, Td and z are each
   linear in ln p between the levels on either side, and e, es, w, rh, th are evaluated FROM THE INTERPOLATED T, Td -- what
   MetPy's precipitable_water does with get_layer on the dewpoint.  Two extensions:
     open top            a NaN scalar top with XP_LAYER_PRESSURE: to the highest valid level (precipitable_water's default).
                         The whole column is read and its last valid level closes the layer: pt is that level's pressure;
     per-column bounds   bottom_columns / top_columns (each nullable): nlayer pointers, each NULL or ncol values [hPa] in the
                         views' dtype and mem.  A non-NULL entry needs XP_LAYER_PRESSURE and replaces that layer's scalar.  A NaN
                         element of a bottom array is p0; a NaN element of a top array gives NaN for that layer and
                         XP_ST_NO_LAYER (xp_cape_cin_layers' rules).  A column whose layer is empty (pt >= pb, or pb > p0) is
                         finished with that layer at its first level, as with scalar bounds.
   With the points P, T, Td, z (first ... last), S = trapz(w, P) (negative), R = trapz(rh, P), D = P_last - P_first, per layer,
   ncol values each:
     precipitable_water [mm]          (-S) * (1e5 / (g rho_l)): hPa -> Pa, m -> mm, g = 9.80665, rho_l = 999.97495 kg m^-3
                                      (MetPy 1.4's metpy.constants.rho_l; part of this definition);
     mean_mixing_ratio [kg/kg]        S / D;
     mean_relative_humidity [0 ... 1] R / D;
     thickness [m]                    z_last - z_first;
     lapse_rate [K/km]                -(T_last - T_first) / thickness * 1000: positive where it cools upward;
     theta_e_min, theta_e_min_pressure   the smallest th over the layer's points and its P, the first of equals winning;
     theta_e_max, theta_e_max_pressure   the largest, likewise.
   The extremes are over the POINTS, not over the continuous profile between them (the convention of xp_downdraft_cape's
   source-level search).  A layer of one point has D = 0: its means are 0/0.
   A layer with pt >= pb, with pb > p0, with pt below the smallest valid pressure or, by height, with a bound above the highest
   valid height gets NaN and the column XP_ST_NO_LAYER; XP_ST_BAD_HEIGHT / XP_ST_BAD_PRESSURE and the levels read as in
   xp_wind_layers.  XP_E_ARG, outputs untouched: everything xp_wind_layers rejects except the NaN top of an
   XP_LAYER_PRESSURE layer (a scalar that a per-column array replaces is not looked at); a NULL pressure; a per-column array
   on a layer of another kind; a wanted output whose input view is NULL -- temperature is needed by mean_relative_humidity,
   lapse_rate and theta_e_*, dewpoint by everything except thickness and lapse_rate, height by thickness, lapse_rate and
   layers by height.  Every output may be NULL; strided device views are read in place. */
typedef struct {
    void *precipitable_water[4], *mean_mixing_ratio[4], *mean_relative_humidity[4];   /* mm, kg/kg, 0 ... 1; ncol each, per layer */
    void *thickness[4], *lapse_rate[4];                                               /* m, K/km */
    void *theta_e_min[4], *theta_e_min_pressure[4], *theta_e_max[4], *theta_e_max_pressure[4];   /* K, hPa, K, hPa */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_HEIGHT | XP_ST_BAD_PRESSURE */
    int32_t dtype, mem;
} xp_thermo_layers_out;
int xp_thermo_layers(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint, const xp_view *height,
                     int32_t nlayer, const xp_wind_layer *layers, const void *const *bottom_columns,
                     const void *const *top_columns, xp_thermo_layers_out *out, void *stream);

/* The classic sounding indices and the convective condensation level of every column in ONE upward pass: MetPy 1.4's k_index,
   total_totals_index, cross_totals, vertical_totals, showalter_index, sweat_index and ccl (the reference has no counterpart),
   carried over to gridded columns whose levels are not the mandatory ones.  Parity with MetPy itself is UNPINNED: MetPy selects
   the mandatory levels by equality, the interpolation to the isobars is this library's extension, and the tests hold the kernel
   to a NumPy restatement of the rules below only (tests/sounding_indices_restatement.py).
   Inputs: pressure [hPa], temperature, dewpoint [K] as (nlev, ncol) views of one shape, dtype and mem, level 0 lowest, pressure
   decreasing; u, v [m/s] on the same vertical, nullable, both or neither: only sweat_index reads them.
   Valid levels: a level is THERMODYNAMICALLY VALID when p, T and Td are all non-NaN, and WIND-VALID when p, u and v are.  Invalid
   levels are dropped (MetPy's _remove_nans); nothing is interpolated through them.
   Value at an isobar P* (850, 700, 500 hPa): a valid level with p == P* gives its values as they are; otherwise the value is
   linear in ln p between the nearest valid level below and the nearest above (MetPy's log_interpolate_1d), NaN without both.
   T and Td use the thermodynamically valid levels, u and v the wind-valid ones.
   Span: if the thermodynamically valid levels do not bracket both 850 and 500 hPa (one with p >= 850 and one with p <= 500), the
   six indices are NaN and the status carries XP_ST_NO_LAYER; sweat_index is NaN too when the wind-valid levels do not.  The CCL
   outputs do not depend on the span.
   Indices (differences in K; [degC] = minus 273.15), in double, in this operation order, without contraction:
     vertical_totals  VT = T850 - T500
     cross_totals     CT = Td850 - T500
     total_totals     TT = VT + CT
     k_index          (VT + Td850[degC]) - (T700 - Td700)
     showalter_index  T500 - Tp500: the parcel (850 hPa, T850, Td850) is lifted to its LCL (xp_lcl); with an LCL pressure
                      <= 500 hPa it rises on the dry adiabat alone, Tp500 = T850 (500 / 850)^kappa; otherwise on the moist
                      adiabat from the LCL to 500 hPa (xp_moist_lapse from (p_lcl, T_lcl), bit for bit) in the call's moist mode:
                      XP_MOIST_EXACT and XP_MOIST_FAMILY both run RK4, XP_MOIST_TABLE the lookup tables.  No virtual temperature
                      correction.  An LCL that did not converge gives NaN and XP_ST_LCL_NOT_CONVERGED.
     sweat_index      (((12 max(Td850[degC], 0) + 20 max(TT - 49, 0)) + 2 f850) + f500) + shear
                      f = sqrt(u u + v v) / (1852 / 3600) [kt] and dir = 90 - atan2(-v, -u) [degrees], plus 360 where that is <= 0
                      (so in (0, 360]), both from the INTERPOLATED u, v;  shear = 125 (sin(dir500 - dir850) + 0.2) when
                      130 <= dir850 <= 250, 210 <= dir500 <= 310, dir500 - dir850 > 0, f850 >= 15 and f500 >= 15 all hold,
                      otherwise 0.
   CCL (metpy.calc.ccl): the start level (p0, T0, Td0) is the lowest thermodynamically valid level.  The mixing ratio r is
   w_s(p0, Td0) with ccl_mixed_layer_depth == 0, otherwise the mixed-layer mean mixing ratio over the lowest
   ccl_mixed_layer_depth hPa, exactly the one of xp_select_parcel's mixed-layer parcel (pf.py:137-162, 229-289; on the column
   as given).  rt(p) = dewpoint(e = p r / (eps + r)) at every thermodynamically valid level -- except that with depth 0 rt at
   the start level IS Td0, not the round trip through r, so that a saturated surface has rt - T == 0 exactly there.  With
   d = rt - T, every pair of consecutive valid levels whose sign(d) differ (zero being a sign of its own, as for np.sign; a NaN
   d is no sign and its pairs hold no crossing) holds a crossing: at ln p and rt value given by xp_find_intersections' two
   expressions (pf.py:1046, 1050) with x = ln p, a = rt, b = T, ccl_pressure = exp(x) -- or, where d is exactly 0 at one end of
   the pair, at that level itself (its p and rt as they are).  ccl_which = XP_CCL_TOP (MetPy's default)
   takes the last crossing, XP_CCL_BOTTOM the first.  ccl_temperature = rt at the crossing; convective_temperature =
   ccl_temperature (p0 / ccl_pressure)^kappa.  Without a crossing the three are NaN and the status carries XP_ST_NO_CCL.
   Every output may be NULL and NULL outputs skip their work: levels are read up to the first valid level at or above 500 hPa
   (wind levels likewise, and u, v only while they are needed), up to the first crossing for XP_CCL_BOTTOM, and to the top of
   the column only for XP_CCL_TOP.  Values do not depend on which other outputs are asked for.  The status bits belong to
   outputs: XP_ST_NO_LAYER is reported when one of the six indices is wanted, XP_ST_LCL_NOT_CONVERGED when showalter_index is,
   XP_ST_NO_CCL when a CCL output is.  The outputs share the views' dtype and mem; strided device views are read in place.
   opts NULL: XP_MOIST_EXACT, XP_CCL_TOP, depth 0.  XP_E_ARG: a NULL or mismatched view; u without v or v without u;
   sweat_index wanted without u and v; a NULL out or one whose dtype or mem differs from the views'; an unknown moist_mode or
   ccl_which; a ccl_mixed_layer_depth that is negative or not finite.  XP_E_NO_TABLES: XP_MOIST_TABLE without tables. */
enum { XP_CCL_TOP = 0, XP_CCL_BOTTOM = 1 };
typedef struct {
    int32_t moist_mode;             /* XP_MOIST_* */
    int32_t ccl_which;              /* XP_CCL_* */
    double ccl_mixed_layer_depth;   /* hPa; 0 = the surface parcel */
} xp_sounding_opts;
typedef struct {
    void *k_index, *total_totals, *cross_totals, *vertical_totals, *showalter_index;   /* K, ncol each */
    void *sweat_index;                                                                 /* dimensionless */
    void *ccl_pressure, *ccl_temperature, *convective_temperature;                     /* hPa, K, K */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_LCL_NOT_CONVERGED | XP_ST_NO_CCL */
    int32_t dtype, mem;
} xp_sounding_out;
int xp_sounding_indices(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint,
                        const xp_view *u, const xp_view *v, const xp_sounding_opts *opts,
                        xp_sounding_out *out, void *stream);

/* Isentropic interpolation (metpy.calc.isentropic_interpolation; the reference has no counterpart): pressure, temperature and up
   to four further variables of every column on up to XP_ISEN_MAX_LEVELS surfaces of constant potential temperature, in ONE read
   of pressure and temperature.  Parity with MetPy itself is UNPINNED: MetPy is not installed where this library is tested, and
   the tests hold the kernel to a NumPy restatement of the rules below only (tests/isentropic_restatement.py).  Three deliberate
   differences from MetPy: (1) the solver and its stopping rule -- MetPy solves the same equation with SciPy's
   Steffensen-accelerated fixed_point and a RELATIVE test on ln p; here it is Newton with an ABSOLUTE test on ln p, under
   MetPy's names and default values (max_iters, eps); (2) ONE bracketing pair serves the pressure and the further variables --
   on a column whose theta does not increase strictly MetPy sorts theta for its interpolate_1d and may read other levels there
   than it used for the pressure; (3) NaN plus a status bit instead of raising (MetPy raises only when a target exceeds the
   whole grid's maximum theta).
   Inputs: pressure [hPa] and temperature [K] as (nlev, ncol) views of one shape, dtype and mem, level 0 lowest, pressure
   decreasing; nvar in 0 ... 4 further variables on the same vertical, same shape, dtype and mem; nlevel in
   1 ... XP_ISEN_MAX_LEVELS target potential temperatures [K] as host doubles, finite and strictly increasing (64: one 64-bit
   word holds a per-target flag).  f32 inputs are converted exactly; all arithmetic is in double, without contraction.
   Valid levels: a level is valid when p and T are both non-NaN.  Invalid levels are dropped, as everywhere in this library;
   nothing is interpolated through them.  A NaN in a further variable does not invalidate a level.
   Potential temperature of a valid level: x_k = ln p_k, theta_k = T_k exp(kappa (ln 1000 - x_k)), kappa = 2 / 7.
   Bracketing pair of a target theta* (MetPy's find_bounding_indices): a pair of consecutive valid levels (k, k + 1) holds a
   crossing when (theta_k <= theta*) differs from (theta_k+1 <= theta*); either direction counts (an unstable layer crosses
   downward).  from_below != 0 (the default; MetPy's bottom_up_search=True) takes the lowest such pair, from_below == 0 the
   highest.  No such pair: every output of that target is NaN in that column and the column's status carries XP_ST_NO_LAYER.
   Pressure on the surface: T is linear in ln p on the pair, a = (T_k+1 - T_k) / (x_k+1 - x_k), b = T_k+1 - a x_k+1.  Newton on
   f(x) = theta* - (a x + b) exp(kappa (ln 1000 - x)) starts at the midpoint x = 0.5 (x_k + x_k+1); with
   e = exp(kappa (ln 1000 - x)), t = a x + b, f = theta* - e t and f' = e (kappa t - a) the step is x <- x - f / f'.  The
   iteration is converged after the step with |x_new - x| <= eps (absolute in ln p, i.e. relative in p) and the result is
   x_new; at most max_iters steps are taken.  Without convergence the target's outputs are NaN and the status carries
   XP_ST_NOT_CONVERGED.  pressure[j] = exp(x); temperature[j] = theta* exp(-kappa (ln 1000 - x)) (MetPy's temperature_out).
   Further variables: linear in theta between the same two levels, v = v_k + (v_k+1 - v_k) (theta* - theta_k) / (theta_k+1 -
   theta_k); NaN where either end is NaN.  On columns whose theta increases strictly this is MetPy's interpolate_1d over theta.
   Outputs: pressure, temperature and vars[0 ... 3] are dense (nlevel, ncol) arrays, level-major, each nullable, of the views'
   dtype and mem; status is int32 per column, the OR over the column's targets.  Values do not depend on which other outputs
   are asked for.  Host views are staged; strided device views are read in place.
   opts NULL: from_below 1, max_iters 50, eps 1e-6.  XP_E_ARG: a NULL or mismatched view; nvar outside 0 ... 4 or a NULL variable
   below nvar; vars[i] set for i >= nvar; nlevel outside 1 ... XP_ISEN_MAX_LEVELS; levels NULL, not finite or not strictly
   increasing; max_iters < 1; eps not finite or <= 0; a NULL out or one whose dtype or mem differs from the views'. */
enum { XP_ISEN_MAX_LEVELS = 64 };
typedef struct {
    int32_t from_below;       /* != 0: the lowest bracketing pair; 0: the highest */
    int32_t max_iters;        /* Newton steps at most, >= 1 */
    double eps;               /* |x_new - x| <= eps in ln p */
} xp_isentropic_opts;
typedef struct {
    void *pressure, *temperature;   /* hPa, K; (nlevel, ncol) each */
    void *vars[4];                  /* the further variables on the surfaces, (nlevel, ncol) each */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_NOT_CONVERGED, ncol */
    int32_t dtype, mem;
} xp_isentropic_out;
int xp_isentropic_interpolation(const xp_view *pressure, const xp_view *temperature, int32_t nvar,
                                const xp_view *const *variables, int32_t nlevel, const double *levels,
                                const xp_isentropic_opts *opts, xp_isentropic_out *out, void *stream);

/* Hydrostatic heights and layer thickness from pressure, temperature and humidity (metpy.calc.thickness_hydrostatic, accumulated
   level by level; the reference has no counterpart): the height of every valid level of every column and the thickness of up to
   four layers by pressure, in ONE upward pass.  Parity with MetPy itself is UNPINNED: MetPy is not installed where this library is
   tested, and the tests hold the kernel to a NumPy restatement of the rules below only (tests/hydrostatic_restatement.py).  One
   deliberate difference from MetPy: the moisture is given as dewpoint or as specific humidity, not as mixing ratio.
   Inputs: pressure [hPa] and temperature [K] as (nlev, ncol) views of one shape, dtype and mem, level 0 lowest, pressure
   decreasing; moisture on the same vertical, same shape, dtype and mem, nullable: dewpoint [K] with XP_HUM_DEWPOINT, specific
   humidity [kg/kg] with XP_HUM_SPECIFIC (opts->humidity; opts NULL: XP_HUM_DEWPOINT); NULL: a dry atmosphere, Tv = T.
   base_height, nullable: ncol values [m] in the views' dtype and mem, the height of each column's lowest valid level; NULL: 0,
   i.e. heights above the lowest valid level, the convention of every height bound in this library.  A NaN element makes that
   column's heights NaN and sets no status bit.  f32 inputs are converted exactly; all arithmetic is fp64, without contraction.
   Valid levels: p, T and the supplied moisture are all non-NaN.  Invalid levels are dropped: their height is NaN and nothing
   is interpolated through them.  p0: the pressure of the lowest valid level.
   Virtual temperature of a point (p, T, moisture): Tv = T (w + eps) / (eps (1 + w)) -- MetPy's form, xp_downdraft_cape's, not the
   reference's 0.608 form -- with w = eps e / (p - e), e = e_s(Td) by Bolton's formula (as everywhere in the library) from a
   dewpoint, w = q / (1 - q) from a specific humidity (no dewpoint in between), w = 0 without moisture.
   Heights: x = ln p.  The lowest valid level gets base_height; every further valid level b after the previous valid level a
       z_b = z_a + (Rd / g) * (0.5 * (Tv_a + Tv_b)) * (x_a - x_b),      Rd = 287.04749097718457, g = 9.80665,
   in that operation order: the trapezoid of Tv over ln p, level by level.
   Layer thickness: nlayer in 0 ... 4 xp_wind_layer structs of kind XP_LAYER_PRESSURE or XP_LAYER_PRESSURE_DEPTH, with the
   vocabulary and the points of xp_thermo_layers: a NaN bottom is p0; a NaN top with XP_LAYER_PRESSURE is open, to the highest
   valid level; the points are the valid levels with pt <= p <= pb (close counting as inside) plus pb and pt themselves where no
   selected level is close to them.  At an added bound point T and the moisture are each linear in ln p between the levels on
   either side, and Tv is evaluated FROM THE INTERPOLATED values.  thickness[j] is the sum of the same (Rd / g) * (0.5 * (Tv_a +
   Tv_b)) * (x_a - x_b) terms over consecutive points of the layer, from 0 at its first point: it does not depend on
   base_height, and a layer of one point has thickness 0.  A layer with pt >= pb, with pb > p0 or with pt below the smallest
   valid pressure gets NaN and the column XP_ST_NO_LAYER; other layers are unaffected.
   Ordering and empty columns: the whole column is always read.  A valid level whose pressure is not below the previous valid
   level's sets XP_ST_BAD_PRESSURE (alone: no layer is judged); heights from that level upward are NaN, and so is every thickness
   of the column.  A column without a valid level gets all NaN and XP_ST_NO_LAYER.
   Outputs: height is dense (nlev, ncol), level-major, nullable; thickness[j] ncol values each, nullable; status int32 per
   column, nullable; all in the views' dtype and mem.  Values do not depend on which other outputs are asked for.  Host views
   are staged; strided device views are read in place; a device call stages nothing and synchronises nothing.
   XP_E_ARG: a NULL or mismatched pressure or temperature; a moisture of another shape, dtype or mem; an unknown humidity;
   nlayer outside 0 ... 4, or layers NULL with nlayer > 0; a layer of kind XP_LAYER_HEIGHT or of an unknown kind; a depth <= 0 or
   not finite, an infinite bound; thickness[j] set for j >= nlayer; a NULL out, or one whose dtype or mem differs from the
   views'. */
typedef struct {
    int32_t humidity;         /* XP_HUM_*: what the moisture view holds */
    int32_t reserved;         /* 0 */
} xp_hydrostatic_opts;
typedef struct {
    void *height;             /* m; (nlev, ncol) */
    void *thickness[4];       /* m; ncol each, per layer */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_PRESSURE, ncol */
    int32_t dtype, mem;
} xp_hydrostatic_out;
int xp_hydrostatic_height(const xp_view *pressure, const xp_view *temperature, const xp_view *moisture,
                          const void *base_height, int32_t nlayer, const xp_wind_layer *layers,
                          const xp_hydrostatic_opts *opts, xp_hydrostatic_out *out, void *stream);

/* metpy.calc.geopotential_to_height and height_to_geopotential per point, with Re = 6371008.7714 m (metpy.constants.Re) and
   g = 9.80665: height [m] = (geopotential * Re) / (g * Re - geopotential); geopotential [m^2 s^-2] = (g * Re * height) /
   (Re + height), each in that operation order, without contraction.  NaN propagates.  n elements of dtype in mem each; no
   argument may be NULL. */
int xp_geopotential_to_height(int64_t n, int32_t dtype, int32_t mem, const void *geopotential, void *out, void *stream);
int xp_height_to_geopotential(int64_t n, int32_t dtype, int32_t mem, const void *height, void *out, void *stream);

/* metpy.calc.critical_angle per point [degrees]: the angle between a = (shear_u, shear_v), the 0-500 m ln p bulk shear, and
   b = (storm_u - surface_u, storm_v - surface_v), evaluated as atan2(|a x b|, a . b) -- mathematically MetPy's
   arccos(a . b / (|a| |b|)), but well conditioned near 0 and 180 degrees, where that form can leave [-1, 1] by rounding.
   NaN where either vector is exactly zero; NaN propagates.  n elements of dtype in mem each; no argument may be NULL. */
int xp_critical_angle(int64_t n, int32_t dtype, int32_t mem, const void *shear_u, const void *shear_v, const void *surface_u,
                      const void *surface_v, const void *storm_u, const void *storm_v, void *out, void *stream);

/* Corfidi (2003) MCS motion per point: upwind = mean - llj, downwind = mean + upwind, in that operation order; mean the
   850-300 hPa pressure-weighted mean wind, llj the low-level jet.  Inputs as above; every output may be NULL. */
int xp_corfidi_storm_motion(int64_t n, int32_t dtype, int32_t mem, const void *mean_u, const void *mean_v, const void *llj_u,
                            const void *llj_v, void *upwind_u, void *upwind_v, void *downwind_u, void *downwind_v,
                            void *stream);

/* SPC's effective-layer significant tornado parameter per point.  With clip(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x)
   (NaN passes through): lcl_term = (2000 - clip(lcl_height, 1000, 2000)) / 1000; cin_term = (200 + clip(mlcin, -200, -50))
   / 150 (CIN <= 0 as everywhere in this library); shr = (ebwd < 12.5 ? 0 : min(ebwd, 30)) / 20;
   stp = ((((mlcape / 1500) * lcl_term) * (esrh / 150)) * shr) * cin_term.  base_height (nullable): the height of the effective
   inflow base (xp_effective_inflow_layer); where it is > 0 the layer is not surface based and the result is 0, whatever the
   other arguments (SPC's rule).  Otherwise NaN propagates.  The other arguments may not be NULL. */
int xp_significant_tornado_effective(int64_t n, int32_t dtype, int32_t mem, const void *mlcape, const void *mlcin,
                                     const void *lcl_height, const void *esrh, const void *ebwd, const void *base_height,
                                     void *out, void *stream);

/* The buoyancy-dilution potential NCAPE of entraining CAPE (Peters, Chavas, Su, Morrison and Coffer 2023, J. Atmos. Sci.; the
   reference and MetPy 1.4 have no counterpart) for every column: an integral over the environment alone, between the LFC and
   the EL that xp_cape_cin wrote for the parcel of interest.  pressure [hPa], temperature, dewpoint [K] and height [m] on one
   vertical; lfc_pressure (L) and el_pressure (E) [hPa]: ncol values each, in the views' dtype and mem.  All arithmetic is in
   double, in the order written here, without contraction.
   A level is valid when p, T, Td and z are all non-NaN; the others are dropped.  z0, p0: the lowest valid level; p_top: the
   pressure of the highest.  With g = 9.80665 and the library's cp, Lv, at every valid level k:
       w = w_s(p, Td), q = w / (1 + w);   ws = w_s(p, T), qs = ws / (1 + ws)          (Bolton's e_s, as everywhere)
       h = (cp T + Lv q) + g z,   hs = (cp T + Lv qs) + g z                            moist static energy, and saturated
       I_0 = 0, I_k = I_(k-1) + (0.5 (h_k + h_(k-1))) (z_k - z_(k-1))                  trapz(h, z) from z0
       hbar_0 = h_0, hbar_k = I_k / (z_k - z0)                                         the mean of h below the level
       b_k = -(g / (cp T_k)) (hbar_k - hs_k).
   The bounds, in this order:
     - L NaN (no LFC: CAPE is 0): ncape = 0.0, both heights NaN, no status bit -- whatever the column holds;
     - L and E both non-NaN and E >= L: the outputs NaN, XP_ST_NO_LAYER;
     - E NaN with L valid: the integral runs to the highest valid level;
     - otherwise both are clamped into [p_top, p0]; a layer that is empty after clamping gives 0.0 (and equal heights);
     - fewer than two valid levels: the outputs NaN, XP_ST_NO_LAYER.
   A bound pb that lies between the valid level below (pp, zp, bp) and the valid level above (p, z, b), pp > pb > p, is the point
       f = (ln pb - ln p) / (ln pp - ln p);   z_b = z + f (zp - z);   b_b = b + f (bp - b)
   -- z linear in ln p, b linear in z; a bound equal to a level's pressure is that level.  Then
       ncape = trapz(b, z) over z_L, the valid levels strictly between, and z_E     [J/kg],
   which is continuous in the bounds: on which side of a level a bound within an ulp of it falls does not matter, and nothing
   bit-exact is promised there.  lfc_height, el_height: z_L - z0, z_E - z0 [m above the lowest valid level: the height
   convention of xp_storm_relative_helicity_layers].
   Levels are read up to and including the first valid level at or beyond E (p <= E), and at least two of them; among the
   valid levels read, a height not above the level below gives XP_ST_BAD_HEIGHT, a pressure not below it XP_ST_BAD_PRESSURE,
   and the outputs are NaN.  Every output may be NULL; the outputs share the views' dtype and mem.  Strided device views are
   read in place.  XP_E_ARG: a NULL or mismatched view, a NULL lfc_pressure or el_pressure, a NULL out or one whose dtype or
   mem differs from the views'. */
typedef struct {
    void *ncape;              /* J/kg, ncol */
    void *lfc_height;         /* m above the lowest valid level */
    void *el_height;          /* the same */
    int32_t *status;          /* XP_ST_NO_LAYER | XP_ST_BAD_HEIGHT | XP_ST_BAD_PRESSURE */
    int32_t dtype, mem;
} xp_ncape_out;
int xp_ncape(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint, const xp_view *height,
             const void *lfc_pressure, const void *el_pressure, xp_ncape_out *out, void *stream);

/* Entraining CAPE per point: the dimensional form of Peters et al.'s (2023) analytic E_A.  cape, ncape [J/kg], el_height [m
   above the lowest valid level: xp_ncape's], sr_u, sr_v [m/s]: the storm-relative 0-1 km mean wind.  A NaN in any input, or
   el_height <= 0, gives NaN in every output.  Otherwise, in double and in this order, without contraction:
       C = k^2 a^2 pi^2 Lmix / (4 Pr s^2) = 82.87727046436741    (k = 0.42, a = 0.8, Lmix = 120 m, Pr = 1/3, s = 1.1)
       psi = C / el_height
       cape <= 0: ecape = ecape_a = 0
       V = max(hypot(sr_u, sr_v), 1e-3);  K = 0.5 (V V);  e = psi / (V V)
       B = (1 + psi) + (2 e) ncape;  x = (8 e) (cape - psi ncape);  r = B B + x
       r < 0: ecape = ecape_a = 0                                 (entrainment leaves no updraft)
       s = sqrt(r);  num = B >= 0 ? (B + s == 0 ? 0 : x / (B + s)) : s - B        (no cancellation)
       ecape_a = max(0, K + num / (4 e));  ecape = max(0, ecape_a - K)
   ecape_a includes the inflow's kinetic energy K, ecape does not.  The floor on V is a definition: the expression is
   continuous there and tends to max(0, -ncape) as V -> 0.  n elements of dtype in mem each; no input may be NULL, every output
   may. */
int xp_ecape(int64_t n, int32_t dtype, int32_t mem, const void *cape, const void *ncape, const void *el_height,
             const void *sr_u, const void *sr_v, void *ecape, void *ecape_a, void *psi, void *stream);

/* ---- Array primitives of the reference's implementation -------------------------------------------------------------
   The CAPE / CIN kernels stream a column once and never build the arrays these functions return, but the reference
   exposes them (and its tests call two of them), so a caller of the reference finds them here too.  One variable per
   call; every view of a call shares shape, dtype and mem; outputs are DENSE C-order (rows, ncol) arrays of that dtype
   in that mem, allocated by the caller.  Arithmetic follows the reference's expressions operation by operation. */

/* pf.py:933-990 insert_level, one variable: out (nlev + 1, ncol) = `variable` with level_value inserted after every
   level whose coordinate is >= level_coord (an equal coordinate stays BELOW the new level, pf.py:950-954).  For the
   coordinate itself pass variable = coords, level_value = level_coord.  Rows whose coordinate is NaN come out NaN in
   every variable, and so does a value equal to fill_value (the reference's -999 trick, pf.py:962-966, 988; its assert
   that the data holds no fill_value is not evaluated). */
int xp_insert_level(const xp_view *coords, const xp_view *variable, const void *level_coord, const void *level_value,
                    double fill_value, void *out, void *stream);

/* pf.py:992-1064 find_intersections of a(x) and b(x) (b NULL = zero): six (nlev - 1, ncol) arrays, each nullable --
   all_intersect_x, all_intersect_y, increasing_x, increasing_y, decreasing_x, decreasing_y; row i describes the interval
   between levels i and i + 1 (the reference's label i + 1 on 'offset_dim'); log_x: interpolate in ln x (pf.py:1014, 1053). */
int xp_find_intersections(const xp_view *x, const xp_view *a, const xp_view *b, int32_t log_x, void *const out[6], void *stream);

/* pf.py:164-206 trapz of one variable: out[c] = sum over intervals of |dx| * mean(dat), NaN areas skipped; mask
   (nullable): (nlev - 1, ncol) bytes in the views' mem, interval i counts when non-zero. */
int xp_trapz(const xp_view *dat, const xp_view *x, const uint8_t *mask, int32_t only_positive, int32_t only_negative,
             void *out, void *stream);

/* pf.py:1200-1289 trap_around_zeros (start = 0): areas = area, dx, x, x_from, x_to, each (2 nlev - 1, ncol), nullable:
   rows 0 .. nlev-1 the areas just BEFORE a zero of y (level k and the zero in (k, k+1)), rows nlev .. 2 nlev-2 the areas
   just AFTER (the zero of interval i and level i + 1) -- the reference's concat of the two families (pf.py:1273).
   mask (nullable): (nlev, ncol) bytes, 1 where the "before" area is NaN (pf.py:1282-1287). */
int xp_trap_around_zeros(const xp_view *x, const xp_view *y, int32_t log_x, void *const areas[5], uint8_t *mask, void *stream);

/* pf.py:208-227 bound_pressure: the pressure of the column closest to bound[c] (the larger of two equally close). */
int xp_bound_pressure(const xp_view *pressure, const void *bound, void *out, void *stream);

/* pf.py:63-100 get_layer, one variable: the lowest `depth` hPa of the column (from its highest pressure), NaN outside.
   interpolate != 0: the layer top is inserted as a level (variable interpolated in ln p; the pressure variable --
   variable_is_pressure -- takes the top pressure itself): out (nlev + 1, ncol).  interpolate == 0: the top is the
   nearest existing level (bound_pressure): out (nlev, ncol). */
int xp_get_layer(const xp_view *pressure, const xp_view *variable, double depth, int32_t interpolate,
                 int32_t variable_is_pressure, void *out, void *stream);

/* pf.py:1699-1720 shift_out_nans, one variable: every column moved down by the number of leading NaNs of `name`. */
int xp_shift_out_nans(const xp_view *name, const xp_view *variable, void *out, void *stream);

/* pf.py:1517-1555 from_most_unstable_parcel (XP_PARCEL_MOST_UNSTABLE) / pf.py:1604-1649 mix_layer
   (XP_PARCEL_MIXED_LAYER): the profile re-based on its parcel.  Levels below the most-unstable parcel / inside the
   mixed layer are masked, levels left without a value in every column of the grid are dropped (dropna(how='all')),
   every column is shifted onto its first remaining level and, for the mixed layer, the parcel is put underneath.
   out_*: (nlev [+ 1 for the mixed layer], ncol), rows >= *nlev_out NaN; parcel: parcel_pressure / temperature /
   dewpoint / parcel_index of xp_scalars_out (nullable, in its own dtype / mem; the parcel row of out_* does not depend
   on them); level_kept (nullable, HOST, nlev
   int32): 1 for every input level that survived the drop.  *nlev_out (HOST) = rows in use.  Synchronises the stream. */
int xp_rebase_profile(const xp_view *pressure, const xp_view *temperature, const xp_view *dewpoint, const xp_parcel *parcel,
                      void *out_pressure, void *out_temperature, void *out_dewpoint, xp_scalars_out *parcel_out,
                      int32_t *level_kept, int64_t *nlev_out, void *stream);

/* pf.py:23-37 interp1d_numba = numpy.interp along the levels: at (m, ncol); xp, fp (n, ncol) with xp increasing along
   the levels (col_stride 0 shares one set of points between the columns); out (m, ncol). */
int xp_interp1d(const xp_view *at, const xp_view *xp, const xp_view *fp, void *out, void *stream);

const char *xp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* XPARCEL_H */
