// xp_isentropic.hpp -- isentropic interpolation (metpy.calc.isentropic_interpolation) of every column of a grid: pressure,
// temperature and up to four further variables on up to 64 surfaces of constant potential temperature, in ONE read of p and T.
// One thread per column, level-major coalesced loads through the two-view look-ahead reader (xp_level_reader.hpp); no moist
// tables and no e_s table: the only LDS is the sorted target list (at most 512 B).
// The rules are stated in include/xparcel.h and restated in NumPy in tests/isentropic_restatement.py.
// One walk over the valid levels (p, T non-NaN) -- upward for from_below, the same walk from the top level downward otherwise,
// so that the first pair a target meets is the one the rule names:
//   - cursor: n(theta) = the number of targets below theta = the first target index with theta <= target.  Per lane, carried
//     from level to level and moved by comparing against the LDS list (indexed per lane): free on a stable column, where it
//     only ever advances, and at most nlevel steps over the whole column.
//   - the targets that flip over the pair (theta_k, theta_k+1) are those with min <= target < max, i.e. the index range
//     [min(n_k, n_k+1), max(n_k, n_k+1)); minus the lane's 64-bit found mask it is the set of targets the pair closes.
//   - each target that closes runs its Newton steps right there, per lane (the lanes of a wavefront that close something at
//     this level step together under one ballot-ended loop, each on its own target), and stores its (j, c) outputs as soon
//     as it closes: the level-major outputs coalesce where neighbouring columns close the same target at the same level.
//     (Tried and dropped: closing per TARGET -- the wavefront takes one pending target at a time and every lane that has it
//     pending solves it -- which makes every store coalesce but runs the Newton loop once per DISTINCT target of the
//     wavefront and level: on columns that do not resemble their neighbours 2.18 ms instead of 0.73 ms for 16 targets on
//     64 x 1 Mi)
//   - the extras are NOT streamed: a closing lane reads the two ends of its pair (2 nvar loads per closed target) where the
//     intended shape had every level of every extra go through registers.  On a 64-level column with 16 targets and two
//     extras that is half the loads, none of them for a target that does not resolve, and the walk's registers are those of the
//     call without extras; the instantiation on HAS-EXTRAS only keeps the pair's level indices out of the latter.
//   - a lane is done when every target is found; the wavefront leaves the loop by ballot.  Unfound targets get NaN at the end.
// Instantiated on dtype x {extras or not}; no instantiation may spill or use scratch (tests/test_isentropic_cpu.py).  It lives
// in a translation unit of its own (xp_isentropic_tu.hip).  The targets reach the kernel as an argument of their own (512 B of
// the kernel-argument segment, read by the first nlevel threads): a device call stages nothing and synchronises nothing.
#pragma once
#include "xp_level_reader.hpp"

namespace xp {

constexpr int ST_NOT_CONVERGED = 256;
constexpr int ISEN_MAX_LEVELS = 64, ISEN_MAX_VARS = 4;
constexpr double LN1000 = 6.907755278982137;                     // ln 1000

struct IsentropicArgs {
    View p, t, v[ISEN_MAX_VARS];
    int64_t nlev, ncol;
    int nlevel, from_below, max_iters;
    double eps;
    void *pressure, *temperature, *vars[ISEN_MAX_VARS];          // dense (nlevel, ncol), the inputs' dtype, nullable
    int32_t *status;
};

// the nlevel targets [K], strictly increasing: a kernel argument of their own, copied into LDS by the first nlevel threads
struct IsentropicLevels { double v[ISEN_MAX_LEVELS]; };

void launch_isentropic(const IsentropicArgs &a, const IsentropicLevels &lv, bool f64, hipStream_t s);

XP_DEV double theta_at(double x, double t) {
#pragma clang fp contract(off)
    return t * fexp(KAPPA * (LN1000 - x));
}

// Newton on f(x) = target - (a x + b) exp(kappa (ln 1000 - x)) over the pair (x0, t0) -- level k -- and (x1, t1) -- level
// k + 1 -- from the midpoint; converged after the step with |x_new - x| <= eps.  All lanes of the group step together.
XP_DEV double isentropic_root(double target, double x0, double t0, double x1, double t1, int max_iters, double eps, bool &conv) {
#pragma clang fp contract(off)
    const double a = fdiv(t1 - t0, x1 - x0), b = t1 - a * x1;
    double x = 0.5 * (x0 + x1);
    conv = false;
    for (int it = 0; it < max_iters; ++it) {
        if (__builtin_amdgcn_ballot_w64(!conv) == 0ull) break;
        const double e = fexp(KAPPA * (LN1000 - x)), t = a * x + b;
        const double f = target - e * t, fp = e * (KAPPA * t - a);
        const double xn = x - fdiv(f, fp);
        if (!conv) {
            conv = fabs(xn - x) <= eps;
            x = xn;
        }
    }
    return conv ? x : qnan();
}

template <typename T, bool EXTRAS> __global__ __launch_bounds__(256)
void k_isentropic(IsentropicArgs a, IsentropicLevels lv) {
#pragma clang fp contract(off)
    __shared__ double s_th[ISEN_MAX_LEVELS];
    const int n = a.nlevel;
    if ((int)threadIdx.x < n) s_th[threadIdx.x] = lv.v[threadIdx.x];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    constexpr int f64 = sizeof(T) == 8;
    const bool up = a.from_below != 0;
    const uint64_t all = n == 64 ? ~0ull : (1ull << n) - 1ull;

    uint64_t found = 0;
    int status = 0, cur = 0;                                     // cur: n(theta) of the last valid level
    double xq = qnan(), tq = qnan(), thq = qnan();               // the last valid level
    int64_t kq = 0;
    bool have = false, done = false;

    const int64_t k0 = up ? 0 : a.nlev - 1, step = up ? 1 : -1;
    LookAhead2<T> next(a.p, a.t, c, k0);
    for (int64_t i = 0; i < a.nlev; ++i) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        if (done) continue;
        const int64_t k = k0 + step * i;
        double p, t;
        next.take(k + step, i + 1 < a.nlev, p, t);
        if (isnan_(p) || isnan_(t)) continue;
        const double x = flog(p), th = theta_at(x, t);
        int nb = cur;
        while (nb < n && s_th[nb] < th) ++nb;
        while (nb > 0 && s_th[nb - 1] >= th) --nb;
        if (have) {
            const int lo = nb < cur ? nb : cur, hi = nb < cur ? cur : nb;        // lo <= hi <= n <= 64
            uint64_t m = ((hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << (lo & 63)) - 1ull)) & ~found;
            if (lo == hi) m = 0;
            // level k of the pair is the lower one whichever way the walk runs
            const double x0 = up ? xq : x, t0 = up ? tq : t, th0 = up ? thq : th;
            const double x1 = up ? x : xq, t1 = up ? t : tq, th1 = up ? th : thq;
            const int64_t ka = up ? kq : k, kb = up ? k : kq;
            // every lane closes its own pending targets, lowest first; the wavefront stays until the last lane has none left
            while (__builtin_amdgcn_ballot_w64(m != 0ull) != 0ull) {
                if (m != 0ull) {
                    const int j = (int)__builtin_ctzll(m);                                   // < n
                    const double target = s_th[j];
                    bool conv;
                    const double xs = isentropic_root(target, x0, t0, x1, t1, a.max_iters, a.eps, conv);
                    if (!conv) status |= ST_NOT_CONVERGED;
                    const int64_t o = (int64_t)j * a.ncol + c;
                    st(a.pressure, f64, o, conv ? fexp(xs) : qnan());
                    st(a.temperature, f64, o, conv ? target * fexp(-(KAPPA * (LN1000 - xs))) : qnan());
                    if constexpr (EXTRAS) {
                        const double w = fdiv(target - th0, th1 - th0);
#pragma unroll
                        for (int q = 0; q < ISEN_MAX_VARS; ++q) {
                            if (a.vars[q] == nullptr) continue;                 // (null at and above nvar)
                            const double v0 = ld<T>(a.v[q], ka, c), v1 = ld<T>(a.v[q], kb, c);
                            st(a.vars[q], f64, o, conv ? v0 + (v1 - v0) * w : qnan());
                        }
                    }
                    m &= m - 1ull;
                    found |= 1ull << j;
                }
            }
        }
        cur = nb; xq = x; tq = t; thq = th; kq = k; have = true;
        done = found == all;
    }

    if (found != all) status |= ST_NO_LAYER;
    for (int j = 0; j < n; ++j) {
        if ((found >> j) & 1ull) continue;
        const int64_t o = (int64_t)j * a.ncol + c;
        st(a.pressure, f64, o, qnan());
        st(a.temperature, f64, o, qnan());
        if constexpr (EXTRAS) {
#pragma unroll
            for (int q = 0; q < ISEN_MAX_VARS; ++q) st(a.vars[q], f64, o, qnan());
        }
    }
    sti(a.status, c, status);
}

}  // namespace xp
