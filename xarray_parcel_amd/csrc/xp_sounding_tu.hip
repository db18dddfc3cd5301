// The translation unit of k_sounding (xp_sounding.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_sounding.hpp"

namespace xp {

void launch_sounding(const SoundingArgs &a, bool f64, bool wind, int ccl, hipStream_t s) {
    with_type(f64, [&](auto z) { with_bool(wind, [&](auto WIND) { with_one_of<CCL_NONE, CCL_SURFACE, CCL_MIXED>(ccl, [&](auto CCL) {
        launch_columns(k_sounding<decltype(z), WIND(), CCL()>, a.ncol, s, a);
    }); }); });
}

}  // namespace xp
