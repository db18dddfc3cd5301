// xp_ground.hpp -- XP_PARCEL_OVER_GROUND (include/xparcel.h): isobaric levels cut at the ground.  One kernel in front of
// the CAPE / CIN kernels turns the three views and the three surface arrays into the re-based column of the header --
// row 0 the surface, then the levels above it, then NaN -- as three dense (nlev + 1, ncol) arrays; everything downstream
// runs on those as on any other grid.
//
// A pure streaming copy.  One lane per column, so a wavefront owns 64 adjacent columns: the stores of an output row are
// one dense request per array, and the loads of a row coalesce within runs of columns that share k0 (smooth terrain).
// The search for k0 reads the pressure alone; temperature and moisture of a dropped level are never read.  A lane whose
// column has run out of levels re-reads its top level (a cache hit) and stores NaN instead, so the loads of a row are
// unconditional and the rows of one trip of the unrolled loop are in flight together.
#pragma once
#include "xp_lcl_node.hpp"

namespace xp {

struct GroundArgs {
    View p, t, m;                         // the call's views, read in place whatever their strides (cs == 0: shared isobars)
    const void *ps, *ts, *tds;            // surface pressure, temperature, dewpoint: ncol each, the views' dtype
    int64_t nlev, ncol;
    void *op, *ot, *otd;                  // dense (nlev + 1, ncol) of the views' dtype; every element is written
};

template <typename T> XP_DEV T tnan() { return (T)qnan(); }

// HUM: the moisture view holds specific humidity; a kept level is stored as k_dewpoint_from_q stores it (the surface is a
// dewpoint already)
template <typename T, bool HUM> __global__ __launch_bounds__(256) void k_ground_rebase(GroundArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    const T ps = ((const T *)a.ps)[c], ts = ((const T *)a.ts)[c], tds = ((const T *)a.tds)[c];
    const bool bad = ps != ps || ts != ts || tds != tds;     // a NaN surface value: the whole column is NaN
    T *op = (T *)a.op + c, *ot = (T *)a.ot + c, *otd = (T *)a.otd + c;
    op[0] = bad ? tnan<T>() : ps;
    ot[0] = bad ? tnan<T>() : ts;
    otd[0] = bad ? tnan<T>() : tds;
    int64_t k0 = 0;                                          // the first level with p < ps: plain comparison, NaN is false
    if (bad) k0 = a.nlev;
    else while (k0 < a.nlev && !(ldr<T>(a.p, k0, c) < ps)) ++k0;
    const int64_t last = a.nlev - 1;
#pragma unroll HUM ? 1 : 4                                   // (the conversion's out-of-line slow path does not unroll)
    for (int64_t j = 0; j < a.nlev; ++j) {
        const int64_t k = k0 + j, kk = k < last ? k : last;
        const bool live = k <= last;
        const T p = ldr<T>(a.p, kk, c), t = ldr<T>(a.t, kk, c), m = ldr<T>(a.m, kk, c);
        const T td = HUM ? (T)dewpoint_from_q((double)p, (double)t, (double)m) : m;
        const int64_t o = (j + 1) * a.ncol;
        op[o] = live ? p : tnan<T>();
        ot[o] = live ? t : tnan<T>();
        otd[o] = live ? td : tnan<T>();
    }
}

}  // namespace xp
