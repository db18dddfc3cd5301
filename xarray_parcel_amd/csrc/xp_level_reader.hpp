// xp_level_reader.hpp -- how the lifting kernels read a column's levels, once: LevelReader, the pointer walk with a one-level
// look-ahead of k_cape_cin (xp_kernels.hpp) and the fused kernel (xp_multi.hpp), and LookAhead, the simpler indexed
// look-ahead of the parcel searches and the effective inflow layer (xp_effective.hpp), with LookAhead2, its two-view sibling.
// Both keep the look-ahead values in the INPUT type until they are used: converting an fp32 value at the load makes the
// wavefront wait for the load right there, and the prefetch hides nothing (it made every fp32 kernel run without any
// prefetch).  None of this is arithmetic: float -> double is exact wherever it happens.
#pragma once
#include "xp_lcl_node.hpp"

namespace xp {

// One-level software prefetch by level index: a loop over the levels is otherwise a chain of dependent HBM round trips.
template <typename T> struct LookAhead {
    const View &pv, &tv, &mv;
    const int64_t c;
    T p, t, m;
    XP_DEV LookAhead(const View &pv_, const View &tv_, const View &mv_, int64_t c_, int64_t k0) : pv(pv_), tv(tv_), mv(mv_), c(c_) { request(k0); }
    XP_DEV void request(int64_t k) { p = ldr<T>(pv, k, c); t = ldr<T>(tv, k, c); m = ldr<T>(mv, k, c); }
    // the level in the buffer, converted now; level `next` is requested if the column has it
    template <typename I> XP_DEV void take(I next, I nlev, double &P, double &T_, double &M_) {
        P = (double)p; T_ = (double)t; M_ = (double)m;
        if (next < nlev) request(next);
    }
};

// The same for the kernels that read pressure and temperature alone (xp_isentropic.hpp), whose walk may also run downward:
// the caller names the level to request next and says whether the column has it.
template <typename T> struct LookAhead2 {
    const View &pv, &tv;
    const int64_t c;
    T p, t;
    XP_DEV LookAhead2(const View &pv_, const View &tv_, int64_t c_, int64_t k0) : pv(pv_), tv(tv_), c(c_) { request(k0); }
    XP_DEV void request(int64_t k) { p = ldr<T>(pv, k, c); t = ldr<T>(tv, k, c); }
    XP_DEV void take(int64_t next, bool more, double &P, double &T_) {
        P = (double)p; T_ = (double)t;
        if (more) request(next);
    }
};

// Three per-lane row pointers that WALK up the levels: set once (64-bit multiply-add, a quarter-rate instruction),
// then advanced by the row stride with two full-rate adds per array and level.  The three views share their strides
// (CapeArgs::off32).
template <typename T> struct LevelReader {
    // (address space 1 = global, spelled out: behind the asm barrier below the compiler would otherwise fall back to
    // flat loads, which also count against the LDS counter and so make every LDS wait a memory wait)
    typedef const char __attribute__((address_space(1))) *GPtr;
    typedef const T __attribute__((address_space(1))) *GT;
    const View &pv, &tv, &dv;
    const int64_t lane_off, row_step;
    GPtr lp = nullptr, lt = nullptr, ld_ = nullptr;
    // (the look-ahead buffer, in the input type: an fp32 level is converted when it is TAKEN; declared in the order they are
    // copied out, the value requested last first: with pressure first one fp32 profile kernel of k_cape_cin gained a
    // scratch store)
    T ntd_ = (T)qnan(), nt_ = (T)qnan(), np_ = (T)qnan();

    XP_DEV LevelReader(const View &p, const View &t, const View &td, int64_t c)
        : pv(p), tv(t), dv(td), lane_off(c * p.cs * (int64_t)sizeof(T)), row_step(p.ls * (int64_t)sizeof(T)) {}
    XP_DEV void seek(int64_t kk) {                                         // the next request() reads level kk
        const int64_t o = kk * row_step + lane_off;
        lp = (GPtr)pv.data + o; lt = (GPtr)tv.data + o; ld_ = (GPtr)dv.data + o;
    }
    XP_DEV void request() {
        np_ = *(GT)lp; nt_ = *(GT)lt; ntd_ = *(GT)ld_;
        lp += row_step; lt += row_step; ld_ += row_step;
        asm volatile("" : "+v"(lp), "+v"(lt), "+v"(ld_));                  // (keeps the walk: no re-derivation from the level index)
    }
    // The buffer itself holds NaN once the levels are used up (no select per level)
    XP_DEV void refill_nan() { np_ = (T)qnan(); nt_ = (T)qnan(); ntd_ = (T)qnan(); }
    // start (or start again) at level k: its values are requested if the column has it
    XP_DEV void start(int k, int nlev) {
        seek(k);
        refill_nan();
        if (k < nlev) request();
    }
    // (one wait for the three values: left alone the compiler waits for each one just before its copy)
    static XP_DEV void wait() { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0x0F70); __builtin_amdgcn_sched_barrier(0); }
    // the level in the buffer as it stands, no wait of its own (the value requested last is copied first, so that the
    // compiler's one wait covers all three)
    XP_DEV void peek(double &P_, double &T2_, double &M_) const { M_ = (double)ntd_; T2_ = (double)nt_; P_ = (double)np_; }
    XP_DEV double peek_p() const { return (double)np_; }
    // Level out of the look-ahead buffer behind the one wait, the next one requested (`more`) or the buffer refilled with NaN.
    XP_DEV void take(bool more, double &P_, double &T2_, double &M_) {
        wait();
        peek(P_, T2_, M_);
        if (more) request();
        else refill_nan();
    }
    XP_DEV void step_back() { lp -= row_step; lt -= row_step; ld_ -= row_step; }
    // a LEVEL (exact in T) goes back into the buffer
    XP_DEV void put_back(double P_, double T2_, double M_) { np_ = (T)P_; nt_ = (T)T2_; ntd_ = (T)M_; }
};

}  // namespace xp
