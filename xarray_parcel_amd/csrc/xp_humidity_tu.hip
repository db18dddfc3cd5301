// The translation unit of k_dewpoint_from (xp_humidity.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_humidity.hpp"

namespace xp {

namespace {
constexpr unsigned MAX_GRID_Y = 65535;
// a view the 16-byte path can read: adjacent columns, base and row pitch on 16 bytes
bool runs16(const View &v, size_t es) {
    return v.cs == 1 && (uintptr_t)v.data % 16 == 0 && (uint64_t)v.ls * es % 16 == 0;
}
}  // namespace

void launch_dewpoint_from(const HumidityArgs &a, bool f64, int kind, hipStream_t s) {
    if (a.ncol <= 0 || a.nlev <= 0) return;
    with_type(f64, [&](auto z) { with_one_of<HUM_RELATIVE, HUM_MIXING_RATIO>(kind, [&](auto KIND) {
        using T = decltype(z);
        const View &x = KIND() == HUM_RELATIVE ? a.t : a.p;
        const bool shared = KIND() == HUM_MIXING_RATIO && x.cs == 0;
        // the output rows are ncol elements apart: they keep the alignment when ncol is a whole number of runs
        const bool vec = a.ncol * sizeof(T) % 16 == 0 && (uintptr_t)a.out % 16 == 0 && runs16(a.m, sizeof(T)) && (shared || runs16(x, sizeof(T)));
        with_bool(vec, [&](auto VEC) {
            const dim3 gr(blocks_for(a.ncol, 256 * (VEC() ? 16 / (int)sizeof(T) : 1)), (unsigned)(a.nlev < MAX_GRID_Y ? a.nlev : MAX_GRID_Y));
            hipLaunchKernelGGL((k_dewpoint_from<T, KIND(), VEC()>), gr, dim3(256), 0, s, a);
        });
    }); });
}

}  // namespace xp
