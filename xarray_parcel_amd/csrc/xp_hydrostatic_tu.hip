// The translation unit of k_hydrostatic (xp_hydrostatic.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_hydrostatic.hpp"

namespace xp {

void launch_hydrostatic(const HydrostaticArgs &a, bool f64, int hum, hipStream_t s) {
    with_type(f64, [&](auto z) { with_one_of<HY_DEWPOINT, HY_SPECIFIC, HY_DRY>(hum, [&](auto HUM) {
        with_int<0, 4>(a.n, [&](auto N) { launch_columns(k_hydrostatic<decltype(z), HUM(), N()>, a.ncol, s, a); });
    }); });
}

}  // namespace xp
