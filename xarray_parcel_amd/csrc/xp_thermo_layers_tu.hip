// The translation unit of k_thermo_layers (xp_thermo_layers.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "xp_thermo_layers.hpp"

namespace xp {

namespace {
dim3 grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

template <typename T, bool MOIST, bool THETA, bool COLB> void launch_nl(const ThermoLayersArgs &a, hipStream_t s) {
    const dim3 gr = grid(a.ncol), bl(256);
    switch (a.n) {
        case 1: hipLaunchKernelGGL((k_thermo_layers<T, 1, MOIST, THETA, COLB>), gr, bl, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_thermo_layers<T, 2, MOIST, THETA, COLB>), gr, bl, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_thermo_layers<T, 3, MOIST, THETA, COLB>), gr, bl, 0, s, a); break;
        default: hipLaunchKernelGGL((k_thermo_layers<T, 4, MOIST, THETA, COLB>), gr, bl, 0, s, a); break;
    }
}
template <typename T, bool MOIST, bool THETA> void launch_colb(const ThermoLayersArgs &a, bool colb, hipStream_t s) {
    if (colb) launch_nl<T, MOIST, THETA, true>(a, s); else launch_nl<T, MOIST, THETA, false>(a, s);
}
template <typename T> void launch_t(const ThermoLayersArgs &a, bool moist, bool theta, bool colb, hipStream_t s) {
    if (moist) { if (theta) launch_colb<T, true, true>(a, colb, s); else launch_colb<T, true, false>(a, colb, s); }
    else { if (theta) launch_colb<T, false, true>(a, colb, s); else launch_colb<T, false, false>(a, colb, s); }
}
}  // namespace

void launch_thermo_layers(const ThermoLayersArgs &a, bool f64, bool moist, bool theta, bool colb, hipStream_t s) {
    if (a.ncol <= 0) return;
    if (f64) launch_t<double>(a, moist, theta, colb, s); else launch_t<float>(a, moist, theta, colb, s);
}

}  // namespace xp
