// xp_humidity.hpp -- XP_HUM_RELATIVE and XP_HUM_MIXING_RATIO (include/xparcel.h): the moisture view of a CAPE / CIN call holds
// relative humidity (a fraction over liquid water) or the water-vapour mixing ratio [kg/kg].  One kernel in front of the CAPE /
// CIN kernels turns it into the dewpoint D of the header, a dense (nlev, ncol) array in the views' dtype; everything
// downstream -- the ground cut, the maximum-CAPE selection, the level walks -- runs on D as on any dewpoint view.
//   relative:      e = m e_s(T)           (Bolton's e_s; the pressure is not read)
//   mixing ratio:  e = p m / (eps + m)    (the temperature is not read)
//   both:          D = 273.15 + 243.5 v / (17.67 - v), v = ln(e / 6.112) -- NaN unless m > 0 (plain comparison)
// restated in NumPy in tests/humidity_restatement.py.
//
// A pure streaming pass: two reads and one write per element.  The work item is (level row, run of adjacent columns): a
// block's x index names 256 runs of W columns of one row, its y index the row (and, past the grid's y limit, every
// gridDim.y-th row after it), so an element's address is row * stride + column -- no division -- and a wavefront's loads
// and stores of a row are dense requests.  W = 16 bytes of T (2 fp64 / 4 fp32 columns per lane, one 16-byte load per view
// and one 16-byte store) where the launcher finds every view it reads and the output laid out for it; W = 1, any strides,
// otherwise.  A pressure with col_stride == 0 (shared isobars) is read by lane 0 of the wavefront and broadcast.
// Arithmetic: the library's fast fp64 forms for physically sane arguments; everything else -- where IEEE infinities and
// the library's edge cases decide between a value and NaN -- takes the reference spelling with the library exp / log, out
// of line behind a ballot (dewpoint_from_q's pattern).  A moisture that is not > 0 is NaN by the rule and needs neither.
// No LDS, no scratch (tests/test_humidity_cpu.py; the register counts are in _lib.py).  It lives in a translation unit of
// its own (xp_humidity_tu.hip).
#pragma once
#include "xp_lcl_node.hpp"

namespace xp {

constexpr int HUM_RELATIVE = 2, HUM_MIXING_RATIO = 3;        // what the moisture view holds: the ABI's XP_HUM_*

struct HumidityArgs {
    View p, t, m;                         // the call's views, read in place whatever their strides (p.cs == 0: shared isobars)
    int64_t nlev, ncol;
    void *out;                            // D: dense (nlev, ncol) of the views' dtype; every element is written
};

// kind: HUM_RELATIVE or HUM_MIXING_RATIO; a call in the views' dtype on stream s
void launch_dewpoint_from(const HumidityArgs &a, bool f64, int kind, hipStream_t s);

// the header's formulas as the oracle spells them (oracle/thermo.py), library exp / log and IEEE division; m > 0
template <int KIND> __device__ __attribute__((noinline)) double dewpoint_from_slow(double p, double t, double m) {
    return dewpoint_of_e(KIND == HUM_RELATIVE ? m * es_ref(t) : p * m / (EPS + m));
}
template <int KIND> XP_DEV double dewpoint_from(double p, double t, double m) {
    bool sane;
    double e;
    if constexpr (KIND == HUM_RELATIVE) {
        sane = (t > 150.0) && (t < 350.0) && (m > 1e-9) && (m < 100.0);
        e = m * sat_vapor_pressure(t);
    } else {
        sane = (p > 1.0) && (p < 2000.0) && (m > 1e-12) && (m < 10.0);
        e = vapor_pressure(p, m);
    }
    const bool wet = m > 0.0;
    double td = wet ? dewpoint_fast(e) : qnan();
    const bool slow = wet && !sane;
    if (__builtin_amdgcn_ballot_w64(slow) != 0ull && slow) td = dewpoint_from_slow<KIND>(p, t, m);
    return td;
}

// W adjacent elements of T; 16 bytes where W > 1
template <typename T, int W> struct alignas(sizeof(T) * W) Run { T e[W]; };

// the W columns from c of row k: one 16-byte load (W > 1: the launcher vouches for col_stride == 1 and the alignment)
template <typename T, int W> XP_DEV Run<T, W> load_run(const View &v, int64_t k, int64_t c) {
    if constexpr (W > 1) return *(const Run<T, W> *)((const T *)v.data + (k * v.ls + c));
    else return Run<T, W>{{ldr<T>(v, k, c)}};
}
// one value for the whole wavefront: lane 0 loads it, every lane receives it (called by all live lanes; lane 0 is one of them)
template <typename T> XP_DEV double load_wave(const T *p) {
    double v = 0.0;
    if ((threadIdx.x & 63u) == 0u) v = (double)*p;
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// VEC: 16-byte runs (ncol is a multiple of W then, so a run never crosses the end of a row)
template <typename T, int KIND, bool VEC> __global__ __launch_bounds__(256) void k_dewpoint_from(HumidityArgs a) {
    constexpr int W = VEC ? 16 / (int)sizeof(T) : 1;
    const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (c >= a.ncol) return;             // (lane 0 holds the wavefront's lowest column: it lives as long as any lane does)
    const View &x = KIND == HUM_RELATIVE ? a.t : a.p;        // the view read next to the moisture
    const bool shared = KIND == HUM_MIXING_RATIO && a.p.cs == 0;
    for (int64_t k = blockIdx.y; k < a.nlev; k += gridDim.y) {
        const Run<T, W> m = load_run<T, W>(a.m, k, c);
        Run<T, W> xr{}, d;
        double xs = 0.0;
        if (shared) xs = load_wave((const T *)x.data + k * x.ls);
        else xr = load_run<T, W>(x, k, c);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const double xv = shared ? xs : (double)xr.e[i];
            d.e[i] = (T)dewpoint_from<KIND>(xv, xv, (double)m.e[i]);
        }
        *(Run<T, W> *)((T *)a.out + (k * a.ncol + c)) = d;
    }
}

}  // namespace xp
