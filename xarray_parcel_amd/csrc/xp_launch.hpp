// xp_launch.hpp -- how every launcher of libxparcel turns run-time values into the template arguments of one kernel, and
// the launch geometry.  A launcher is a nest of with_*() calls around a single mention of its kernel template:
//     with_type(f64, [&](auto z) { with_bool(flag, [&](auto FLAG) { with_int<1, 4>(n, [&](auto N) {
//         launch_columns(k<decltype(z), N(), FLAG()>, ncol, s, a); }); }); });
// Each with_*() calls the generic lambda exactly once, with a value that carries the choice in its type.  A value that is
// none of the choices takes the LAST one (with_int: HI), as the default: of a switch would.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace xp {

// f(double()) or f(float())
template <typename F> void with_type(bool f64, F &&f) {
    if (f64) f(double());
    else f(float());
}
// f(std::true_type()) or f(std::false_type())
template <typename F> void with_bool(bool b, F &&f) {
    if (b) f(std::true_type());
    else f(std::false_type());
}
// f(std::integral_constant<int, K>()) with K the enumerator of the list that v equals, else the last of the list
template <int K, int... REST, typename F> void with_one_of(int v, F &&f) {
    if constexpr (sizeof...(REST) > 0) {
        if (v != K) { with_one_of<REST...>(v, f); return; }
    }
    f(std::integral_constant<int, K>());
}
// the same over LO ... HI: a v outside the range takes HI
template <int LO, int HI, typename F> void with_int(int v, F &&f) {
    static_assert(LO <= HI, "with_int<LO, HI>: an empty range");
    if constexpr (LO < HI) {
        if (v != LO) { with_int<LO + 1, HI>(v, f); return; }
    }
    f(std::integral_constant<int, LO>());
}

// workgroups of `threads` that cover n elements (none for n <= 0)
inline unsigned blocks_for(int64_t n, int threads = 256) { return n > 0 ? (unsigned)((n + threads - 1) / threads) : 0u; }
// one thread per column (or element) of an n-column grid, 256 per workgroup, on stream s; n <= 0 launches nothing
template <typename... P, typename... A> void launch_columns(void (*k)(P...), int64_t n, hipStream_t s, const A &...args) {
    if (n > 0) hipLaunchKernelGGL(k, dim3(blocks_for(n)), dim3(256), 0, s, args...);
}

// Persistent wavefronts: at most workgroups_per_cu workgroups on each of n_cu compute units walk the grid between them.
inline unsigned capped_blocks(int64_t ncol, int threads, int workgroups_per_cu, int n_cu) {
    const unsigned nblk = blocks_for(ncol, threads), cap = (unsigned)(n_cu * workgroups_per_cu);
    return nblk > cap ? cap : nblk;
}
// ... with the current device's CU count, asked once (256 where the query fails)
inline unsigned persistent_blocks(int64_t ncol, int threads, int workgroups_per_cu = 1) {
    static const int n_cu = [] { int d = 0; hipDeviceProp_t pr; return (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&pr, d) == hipSuccess) ? pr.multiProcessorCount : 256; }();
    return capped_blocks(ncol, threads, workgroups_per_cu, n_cu);
}

}  // namespace xp
