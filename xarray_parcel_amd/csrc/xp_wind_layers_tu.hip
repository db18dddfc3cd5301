// The translation unit of k_wind_layers and the per-point kernels of xp_wind_layers.hpp, and their launchers.
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

void launch_critical_angle(int64_t n, bool f64, const void *const in[6], void *out, hipStream_t s) {
    if (n <= 0) return;
    if (f64) hipLaunchKernelGGL(k_critical_angle<double>, grid(n), dim3(256), 0, s, n, in[0], in[1], in[2], in[3], in[4], in[5], out);
    else hipLaunchKernelGGL(k_critical_angle<float>, grid(n), dim3(256), 0, s, n, in[0], in[1], in[2], in[3], in[4], in[5], out);
}

void launch_corfidi(int64_t n, bool f64, const void *const in[4], void *const out[4], hipStream_t s) {
    if (n <= 0) return;
    if (f64) hipLaunchKernelGGL(k_corfidi_storm_motion<double>, grid(n), dim3(256), 0, s, n, in[0], in[1], in[2], in[3], out[0], out[1], out[2], out[3]);
    else hipLaunchKernelGGL(k_corfidi_storm_motion<float>, grid(n), dim3(256), 0, s, n, in[0], in[1], in[2], in[3], out[0], out[1], out[2], out[3]);
}

void launch_stp_effective(int64_t n, bool f64, const void *const in[6], void *out, hipStream_t s) {
    if (n <= 0) return;
    if (f64) hipLaunchKernelGGL(k_significant_tornado_effective<double>, grid(n), dim3(256), 0, s, n, in[0], in[1], in[2], in[3], in[4], in[5], out);
    else hipLaunchKernelGGL(k_significant_tornado_effective<float>, grid(n), dim3(256), 0, s, n, in[0], in[1], in[2], in[3], in[4], in[5], out);
}

}  // namespace xp
