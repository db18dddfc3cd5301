// The translation unit of k_wind_layers (xp_wind_layers.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_wind_layers.hpp"

namespace xp {

void launch_wind_layers(const WindLayersArgs &a, bool f64, bool want_max, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(want_max, [&](auto MAXW) { with_int<1, 4>(a.n, [&](auto N) {
        launch_columns(k_wind_layers<decltype(z), N(), MAXW()>, a.ncol, s, a);
    }); }); });
}

}  // namespace xp
