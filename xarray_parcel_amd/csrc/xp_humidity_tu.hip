// The translation unit of k_dewpoint_from (xp_humidity.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_humidity.hpp"

namespace xp {

namespace {
constexpr unsigned MAX_GRID_Y = 65535;
// a view the 16-byte path can read: adjacent columns, base and row pitch on 16 bytes
bool runs16(const View &v, size_t es) {
    return v.cs == 1 && (uintptr_t)v.data % 16 == 0 && (uint64_t)v.ls * es % 16 == 0;
}
template <typename T, int KIND, bool VEC> void launch_v(const HumidityArgs &a, hipStream_t s) {
    constexpr int64_t per_block = 256 * (VEC ? 16 / (int64_t)sizeof(T) : 1);
    const dim3 gr((unsigned)((a.ncol + per_block - 1) / per_block), (unsigned)(a.nlev < MAX_GRID_Y ? a.nlev : MAX_GRID_Y)), bl(256);
    hipLaunchKernelGGL((k_dewpoint_from<T, KIND, VEC>), gr, bl, 0, s, a);
}
template <typename T, int KIND> void launch_k(const HumidityArgs &a, hipStream_t s) {
    const View &x = KIND == HUM_RELATIVE ? a.t : a.p;
    const bool shared = KIND == HUM_MIXING_RATIO && x.cs == 0;
    // the output rows are ncol elements apart: they keep the alignment when ncol is a whole number of runs
    const bool vec = a.ncol * sizeof(T) % 16 == 0 && (uintptr_t)a.out % 16 == 0 && runs16(a.m, sizeof(T)) && (shared || runs16(x, sizeof(T)));
    if (vec) launch_v<T, KIND, true>(a, s); else launch_v<T, KIND, false>(a, s);
}
template <typename T> void launch_t(const HumidityArgs &a, int kind, hipStream_t s) {
    if (kind == HUM_RELATIVE) launch_k<T, HUM_RELATIVE>(a, s); else launch_k<T, HUM_MIXING_RATIO>(a, s);
}
}  // namespace

void launch_dewpoint_from(const HumidityArgs &a, bool f64, int kind, hipStream_t s) {
    if (a.ncol <= 0 || a.nlev <= 0) return;
    if (f64) launch_t<double>(a, kind, s); else launch_t<float>(a, kind, s);
}

}  // namespace xp
