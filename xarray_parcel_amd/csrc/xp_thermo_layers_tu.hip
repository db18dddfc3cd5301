// The translation unit of k_thermo_layers (xp_thermo_layers.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_thermo_layers.hpp"

namespace xp {

void launch_thermo_layers(const ThermoLayersArgs &a, bool f64, bool moist, bool theta, bool colb, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(moist, [&](auto MOIST) { with_bool(theta, [&](auto THETA) {
        with_bool(colb, [&](auto COLB) { with_int<1, 4>(a.n, [&](auto N) {
            launch_columns(k_thermo_layers<decltype(z), N(), MOIST(), THETA(), COLB()>, a.ncol, s, a);
        }); }); }); }); });
}

}  // namespace xp
