// The translation unit of k_ncape (xp_ecape.hpp) and its launcher.
#include "xp_launch.hpp"
#include "xp_ecape.hpp"

namespace xp {

void launch_ncape(const NcapeArgs &a, bool f64, hipStream_t s) {
    with_type(f64, [&](auto z) { launch_columns(k_ncape<decltype(z)>, a.ncol, s, a); });
}

}  // namespace xp
