// The translation unit of k_wind_layers (xp_wind_layers.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_wind_layers.hpp"

namespace xp {

namespace {
dim3 grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

template <typename T, bool MAXW> void launch_nl(const WindLayersArgs &a, hipStream_t s) {
    const dim3 gr = grid(a.ncol), bl(256);
    switch (a.n) {
        case 1: hipLaunchKernelGGL((k_wind_layers<T, 1, MAXW>), gr, bl, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_wind_layers<T, 2, MAXW>), gr, bl, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_wind_layers<T, 3, MAXW>), gr, bl, 0, s, a); break;
        default: hipLaunchKernelGGL((k_wind_layers<T, 4, MAXW>), gr, bl, 0, s, a); break;
    }
}
}  // namespace

void launch_wind_layers(const WindLayersArgs &a, bool f64, bool want_max, hipStream_t s) {
    if (a.ncol <= 0) return;
    if (f64) { if (want_max) launch_nl<double, true>(a, s); else launch_nl<double, false>(a, s); }
    else { if (want_max) launch_nl<float, true>(a, s); else launch_nl<float, false>(a, s); }
}

}  // namespace xp
