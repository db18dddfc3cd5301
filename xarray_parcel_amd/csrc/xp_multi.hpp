// xp_multi.hpp -- several parcels of ONE grid lifted in one pass (adiabat-family moist mode).
//
// The reference's products lift two or three parcels from the same three arrays -- most-unstable and mixed-layer CAPE / CIN
// of BASELINE config 5 (pf.py:1557, 1651), most-unstable + 100 hPa + 50 hPa mixed-layer in conv_properties (pf.py:1984-2006) --
// and every single-parcel launch of k_cape_cin re-reads p / T / Td and recomputes what does not depend on the parcel: ln p
// and the environment's virtual temperature, the two e_s evaluations of pf.py:839-843 -- about 60 of the ~150 fp64
// instructions a level costs.  Here one thread still owns one column, but carries NP parcel "chains" (LCL, dry-adiabat
// constants, xp::Family coefficients, xp::Scan state, LDS slots) through ONE walk over the levels:
//
//   * first every chain, one after the other, does what depends on its parcel alone: the parcel search, the LCL, the
//     adiabat's label, and the levels up to the LCL with the LCL node in their midst (xp::below_lcl_node of xp_lcl_node.hpp,
//     on per-lane level indices: ~10-15 iterations until the whole wavefront is past its LCLs);
//   * then ONE walk up the remaining levels (k_cape_cin's phase B, ~85 % of a column): every level is loaded once, with a
//     wave-uniform index (one coalesced row request per array), its environment node (ln p, Tv) is evaluated once, and each
//     chain that has reached it feeds it to its scan with its own moist-adiabat value.  A chain that resumes higher up sits
//     out until the walk reaches its level.
// (A first version walked all chains through their LCLs in the shared loop as well: with the most-unstable parcels of
// 18 % of the columns starting at levels 12-43 some lane of nearly every wavefront was below its LCL up to level ~50, the
// expensive below-LCL node ran there for everybody, and the fused c5 step took 39 ms against 24.3 for two separate calls.)
//
// Every chain performs exactly the floating-point operations of the single-parcel kernel on its nodes (up to the LCL the
// pieces of xp_lcl_node.hpp that k_cape_cin composes as well, above it the same device functions in the same order), so
// the results are bit-identical to separate xp_cape_cin calls (tests/test_gpu_multi.py).
// Columns a chain's family table cannot serve are flagged per chain and redone by the single-parcel RK4 kernel.
// Workgroups: XP_CAPE_THREADS threads, one per CU (LDS: e_s / ln tables 11.8 KB + family table 46.7 KB + NP x
// SLOT_FIELDS x XP_CAPE_THREADS slot doubles); two parcels at 512 threads = 156.9 KB, two wavefronts per SIMD with up
// to 256 VGPRs each -- the chains of a thread are independent dependency chains, which is where the latency hiding
// that the lower occupancy gives up comes back from.
#pragma once
#include "xp_kernels.hpp"

namespace xp {

constexpr int MULTI_MAX = 3;
struct MultiArgs {
    CapeArgs base;                    // views, shape, options, tables, persist (base.s / base.flags / base.depth / base.prof unused)
    int np;
    int mode[MULTI_MAX];              // PM_SURFACE | PM_MU | PM_ML
    double depth[MULTI_MAX];
    ScalarsOut s[MULTI_MAX];
    int32_t *flags[MULTI_MAX];        // 1 = the column of this chain must be redone by the RK4 kernel
};

struct Lev { double P, X, T, Td, tve; };      // one level with its environment node: pressure, ln p, T, Td, Tv (or T)

struct Chain {
    BelowLcl n;            // the LCL and the dry adiabat below it
    double lt;             // LCL temperature
    int first;             // first level of the grid that belongs to this chain's profile (INT_MAX: blank chain)
    int status;
    bool done;             // the LCL node has been fed: the chain consumes `prev` from now on
    Scan sc;
    Family fam;
};

template <typename T, int NP, bool PERSIST>
__global__ __launch_bounds__(XP_CAPE_THREADS) void k_cape_cin_multi(MultiArgs a) {
    static_assert(NP >= 1 && NP <= MULTI_MAX, "1..3 parcels");
    __shared__ double s_es[LDS_TAB];
    __shared__ double s_fam[FAM_SIZE];
    for (int i = threadIdx.x; i < FAM_SIZE; i += blockDim.x) s_fam[i] = a.base.fam_tab[i];
    __shared__ int s_next;
    if (PERSIST && threadIdx.x == 0) s_next = (int)(blockDim.x >> 6);
    stage_es_table(a.base.es_tab, s_es);
    const int64_t c0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!PERSIST && c0 >= a.base.ncol) return;
    const double *es = s_es;
    __shared__ double s_slot[NP * SLOT_FIELDS * SLOT_STRIDE];
    constexpr int DEAD = 0x7fffffff;

    auto column = [&](const int64_t c) __attribute__((always_inline)) {
    const CapeArgs &b = a.base;
    const bool vtc = b.vtc != 0, pos_neg = b.pos_neg != 0;
    const bool need_w = vtc;
    const int nlev = (int)b.nlev;
    Chain h0, h1, h2;
    auto each = [&](auto f) __attribute__((always_inline)) {
        f(h0, std::integral_constant<int, 0>{});
        if constexpr (NP > 1) f(h1, std::integral_constant<int, 1>{});
        if constexpr (NP > 2) f(h2, std::integral_constant<int, 2>{});
    };
    // One node of chain h at / below / just above its LCL, on one level (P, T_, Td_): xp::below_lcl_node with the family's
    // adiabat -- the table holds the parcel's VIRTUAL temperature, and on the LCL the adiabat's temperature is the LCL's.
    auto feed = [&](Chain &h, double P, double T_, double Td_, const bool skew, const bool last) __attribute__((always_inline)) {
        h.done = below_lcl_node(es, h.sc, h.n, vtc, b.log_interp != 0, P, T_, Td_, skew, last, h.status,
                                [&](bool above, double P_, double X, double &tp, double &tvp) __attribute__((always_inline)) {
            if (above) { tvp = h.fam.at(X); tp = !vtc ? Family::temperature_of(es, P_, tvp) : tvp; }
            else tp = h.lt;
        });
    };

    // three per-lane row pointers that walk up the levels with a one-level look-ahead (xp_level_reader.hpp)
    LevelReader<T> rd(b.p, b.t, b.td, c);

    // ---- per chain, one after the other: parcel, LCL, label, and the levels up to the LCL ---------------------------------
    // (every lane walks from ITS first level with its own row pointers until the whole wavefront is past its LCLs -- ~10-15
    // iterations; these rows are read again by the shared walk below, out of L2)
    each([&](Chain &h, auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        const Parcel pc = choose_parcel<T, false>(b, a.mode[i], c, es, a.depth[i]);
        const ScalarsOut &s = a.s[i];
        Lcl l;
        h.done = true; h.first = DEAD;
        h.fam.tab = s_fam; h.fam.q = 0; h.fam.s = 0.0; h.fam.bad = false; h.fam.poison();
        if (!start_column(es, pc, need_w, vtc, pos_neg, s_slot + i * (SLOT_FIELDS * SLOT_STRIDE) + threadIdx.x, l, h.n, h.sc, h.status)) {
            store_blank_column(s, c, pc, l, h.status);                              // (a blank chain: its scan is never fed nor finished)
            a.flags[i][c] = 0;
        } else {
            store_parcel_and_lcl(s, c, pc, l);
            h.fam.start(s_fam, es, l.p, h.n.x_lcl, l.t, l.tv);
            h.done = false;
            h.first = (int)pc.first;
        }
        h.lt = l.t;
        // mixed layer: the parcel is the new level 0 of its profile (pf.py:1641-1644)
        const bool pre = pc.prepend && h.first != DEAD;
        if (__builtin_amdgcn_ballot_w64(pre) != 0ull && pre) {
            feed(h, pc.p, pc.t, pc.td, false, false);
            // a supersaturated mixed parcel lies above its own LCL: the LCL node went first and the parcel node follows it
            const bool again = h.done;
            if (__builtin_amdgcn_ballot_w64(again) != 0ull && again) feed(h, pc.p, pc.t, pc.td, true, false);
        }
        // levels first, first + 1, ... while some lane of the wavefront is at or below its LCL; a lane past its LCL is one
        // level behind its loads (the level that crossed waits in wP, wT, wM)
        int k = h.first == DEAD ? nlev + 1 : h.first;
        rd.start(k, nlev);
        double wP = qnan(), wT = qnan(), wM = qnan();
        for (; k <= nlev; ++k) {
            if (__ballot(!h.done) == 0ull) break;
            const bool in = k < nlev;
            double P, T_, M_;
            rd.peek(P, T_, M_);
            P = in ? P : qnan(); T_ = in ? T_ : qnan(); M_ = in ? M_ : qnan();
            if (k + 1 < nlev) rd.request();
            const bool skew = h.done;
            if (!skew || k > h.first) feed(h, skew ? wP : P, skew ? wT : T_, skew ? wM : M_, skew, !in);
            wP = P; wT = T_; wM = M_;
        }
        // the next level this chain takes is the one that is waiting (k - 1), or its first one if it has not loaded any:
        // the shared walk feeds level j to a chain in iteration j + 1
        h.first = h.first == DEAD ? DEAD : (k > h.first ? k : h.first + 1);
    });

    // ---- the shared walk: every chain of every lane is above its LCL (k_cape_cin's phase B) ------------------------------
    // h.first now is the iteration in which the chain resumes; the wavefront walks up from the lowest of them, every level
    // is loaded once (one coalesced row request per array) and its environment node -- ln p, Tv(T, Td, p): two e_s behind
    // one wave-uniform range test -- evaluated once for all chains.
    int fmin = h0.first;
    if constexpr (NP > 1) fmin = h1.first < fmin ? h1.first : fmin;
    if constexpr (NP > 2) fmin = h2.first < fmin ? h2.first : fmin;
    int ku = nlev + 1;
    for (int probe = 1; probe <= nlev; ++probe) if (__ballot(fmin <= probe) != 0ull) { ku = probe - 1; break; }
    rd.start(ku, nlev);
    Lev cur, prev;
    prev.P = prev.X = prev.T = prev.Td = prev.tve = qnan();
    for (int k = ku; k <= nlev; ++k) {
        each([&](Chain &h, auto ic) __attribute__((always_inline)) {
            if (k >= h.first) {
                const double tvp = h.fam.at(prev.X);
                const double tp = !vtc ? Family::temperature_of(es, prev.P, tvp) : tvp;
                h.sc.template node<false, true>(prev.P, prev.X, vtc ? tvp : tp, vtc ? prev.tve : prev.T, false);
            }
        });
        if (k < nlev) {
            rd.peek(cur.P, cur.T, cur.Td);
            if (k + 1 < nlev) rd.request();
            cur.X = log_tab<true>(es, cur.P);
            cur.tve = need_w ? virt_env_ranged(es, cur.T, cur.Td, cur.P) : cur.T;
            prev = cur;
        }
    }

    // ---- results -------------------------------------------------------------------------------------------------------
    // (output pointers fetched from the kernel arguments only now, as in k_cape_cin: not carried across the walk)
    const auto late = late_kernargs<MultiArgs>();
    const bool post_zero = late->base.post_zero != 0;
    each([&](Chain &h, auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        if (h.first != DEAD) {
            Scan::Result r = h.sc.finish(post_zero);
            late->flags[i][c] = h.fam.bad ? 1 : 0;
            store_scan_result(late->s[i], c, r, h.status | r.status);
        }
    });
    };   // column

    if (PERSIST) persistent_tiles(a.base.ncol, s_next, column);
    else column(c0);
}

// one translation unit per (T, NP): xp_multi_tu.hip
template <typename T, int NP> void launch_cape_multi(const MultiArgs &a, hipStream_t s);

}  // namespace xp
