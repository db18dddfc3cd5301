// The translation unit of k_hydrostatic (xp_hydrostatic.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_hydrostatic.hpp"

namespace xp {

namespace {
template <typename T, int HUM> void launch_h(const HydrostaticArgs &a, hipStream_t s) {
    const dim3 gr((unsigned)((a.ncol + 255) / 256)), bl(256);
    switch (a.n) {
        case 0: hipLaunchKernelGGL((k_hydrostatic<T, HUM, 0>), gr, bl, 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_hydrostatic<T, HUM, 1>), gr, bl, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_hydrostatic<T, HUM, 2>), gr, bl, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_hydrostatic<T, HUM, 3>), gr, bl, 0, s, a); break;
        default: hipLaunchKernelGGL((k_hydrostatic<T, HUM, 4>), gr, bl, 0, s, a); break;
    }
}
template <typename T> void launch_t(const HydrostaticArgs &a, int hum, hipStream_t s) {
    if (hum == HY_DEWPOINT) launch_h<T, HY_DEWPOINT>(a, s);
    else if (hum == HY_SPECIFIC) launch_h<T, HY_SPECIFIC>(a, s);
    else launch_h<T, HY_DRY>(a, s);
}
}  // namespace

void launch_hydrostatic(const HydrostaticArgs &a, bool f64, int hum, hipStream_t s) {
    if (a.ncol <= 0) return;
    if (f64) launch_t<double>(a, hum, s); else launch_t<float>(a, hum, s);
}

}  // namespace xp
