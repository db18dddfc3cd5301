// xp_max_cape.hpp -- XP_PARCEL_MAX_CAPE (include/xparcel.h): the parcel with the largest CAPE among the departure levels of
// the lowest `depth` hPa.  Two kernels in front of the CAPE / CIN kernels:
//   k_max_cape_select lifts every candidate of every column -- the candidates of xp_effective_inflow_layer, by its lifter,
//     xp::lift_candidate, unchanged -- and keeps the lowest level k* whose CAPE is the largest;
//   k_rebase_from copies each column from its level k* on into three dense (nlev, ncol) arrays, NaN behind it.
// Everything downstream then runs the SURFACE parcel on those arrays as on any other grid, so the call is, bit for bit,
// the surface call on the re-based column (the pattern of xp_ground.hpp).
//
// The selection kernel is k_effective_inflow with another bookkeeping: one thread per column, the e_s / ln table and the
// Scan slots in LDS, the candidate index WAVE-UNIFORM -- the outer loop runs k = 0, 1, ... for the whole wavefront, a lane
// whose level k is invalid or beyond its window sits the candidate out, and a ballot ends the loop when no lane has work
// left.  There is no early stop: every candidate of the window is lifted.  The LCL iteration sits inside the candidate loop,
// so the unit (xp_max_cape_tu.hip) is compiled with -disable-machine-licm for the reason written at k_effective_inflow.
#pragma once
#include "xp_effective.hpp"

namespace xp {

struct MaxCapeArgs {
    EffectiveArgs e;                      // views, shape, depth, the four CAPE / CIN options, tables: what lift_candidate reads
    int32_t *kstar;                       // per column: k*, 0 for a column without a candidate (may be null)
    ScalarsOut s;                         // xp_select_parcel: parcel_idx and par_p / par_t / par_td (each may be null)
};

template <typename T, bool TABLE> __global__ __launch_bounds__(256)
void k_max_cape_select(MaxCapeArgs a) {
    struct Lds { double es[LDS_TAB]; double slot[SLOT_FIELDS * SLOT_STRIDE]; };   // the table first (see k_cape_cin)
    __shared__ Lds l;
    static_assert(SLOT_STRIDE == 256, "one Scan slot column per thread of the workgroup");
    const double *es = stage_es_table(a.e.es_tab, l.es);
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.e.ncol) return;
    const int nlev = (int)a.e.nlev;
    double *const slot = l.slot + threadIdx.x;

    double bound = qnan(), best = qnan();        // p0 - depth, once the lowest valid level is known; the holder's CAPE
    int kstar = -1;
    bool done = false;                           // the first valid level beyond the window has been seen
    for (int k = 0; k < nlev; ++k) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        bool lift = false;
        double p = qnan(), t = qnan(), td = qnan();
        if (!done) {
            p = ld<T>(a.e.p, k, c); t = ld<T>(a.e.t, k, c); td = ld<T>(a.e.td, k, c);
            if (!(isnan_(p) || isnan_(t) || isnan_(td))) {                 // an invalid level is skipped
                if (isnan_(bound)) bound = p - a.e.depth;
                lift = p >= bound;
                done = !lift;
            }
        }
        if (lift) {
            double cape, cin;
            int cst;
            lift_candidate<T, TABLE>(a.e, es, slot, c, k, nlev, p, t, td, cape, cin, cst);
            if (kstar < 0 || cape > best) { kstar = k; best = cape; }      // the first candidate, then only a larger CAPE: NaN never wins
        }
    }
    if (kstar < 0) kstar = 0;
    sti(a.kstar, c, kstar);
    sti(a.s.parcel_idx, c, kstar);
    if (a.s.par_p) st(a.s.par_p, a.s.f64, c, ld<T>(a.e.p, kstar, c));
    if (a.s.par_t) st(a.s.par_t, a.s.f64, c, ld<T>(a.e.t, kstar, c));
    if (a.s.par_td) st(a.s.par_td, a.s.f64, c, ld<T>(a.e.td, kstar, c));
}

struct RebaseFromArgs {
    View p, t, td;                        // the call's views, read in place whatever their strides
    const int32_t *kstar;                 // per column, 0 ... nlev - 1
    int64_t nlev, ncol;
    void *op, *ot, *otd;                  // dense (nlev, ncol) of the views' dtype; every element is written
};

// A pure streaming copy, k_ground_rebase's shape: one lane per column, so the stores of an output row are one dense request
// per array, and the loads of row j -- level k* + j -- coalesce within runs of columns that share k*.  The scattered side is
// the loads: a partly covered line costs a read the same as a full one and is read again from L2 by the neighbours one row on,
// while a partly covered store would cost a read-modify-write of the line.  A lane whose column has run out of levels re-reads
// its top level (a cache hit) and stores NaN instead, so the loads of a row are unconditional.
template <typename T> __global__ __launch_bounds__(256) void k_rebase_from(RebaseFromArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    const int64_t last = a.nlev - 1;
    int64_t k0 = a.kstar[c];
    k0 = k0 < 0 ? 0 : k0 > last ? last : k0;                 // (k* lies in 0 ... nlev - 1 by construction)
    const T nan = (T)qnan();
    T *op = (T *)a.op + c, *ot = (T *)a.ot + c, *otd = (T *)a.otd + c;
#pragma unroll 4
    for (int64_t j = 0; j < a.nlev; ++j) {
        const int64_t k = k0 + j, kk = k < last ? k : last;
        const bool live = k <= last;
        const T p = ldr<T>(a.p, kk, c), t = ldr<T>(a.t, kk, c), td = ldr<T>(a.td, kk, c);
        const int64_t o = j * a.ncol;
        op[o] = live ? p : nan;
        ot[o] = live ? t : nan;
        otd[o] = live ? td : nan;
    }
}

// defined in xp_max_cape_tu.hip
void launch_max_cape_select(const MaxCapeArgs &a, bool f64, bool table, hipStream_t s);
void launch_rebase_from(const RebaseFromArgs &a, bool f64, hipStream_t s);

}  // namespace xp
