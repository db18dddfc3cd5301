// A stand-alone check of csrc/xp_launch.hpp on the host (tests/test_launch_cpu.py builds and runs it; no device is touched):
// every with_*() calls its functor exactly once, with the value asked for or, outside the choices, with the last one; the
// block counts of launch_columns' geometry; the persistent grid below, at and above its cap.
#include <cstdio>
#include <type_traits>

#include "xp_launch.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// what a dispatcher called: how often, and with which compile-time value
struct Seen {
    int calls = 0, value = -999;
    template <typename V> void operator()(V) { ++calls; value = (int)V::value; }
};
struct SeenType {
    int calls = 0, size = 0;
    bool floating = false;
    template <typename T> void operator()(T) { ++calls; size = (int)sizeof(T); floating = std::is_floating_point<T>::value; }
};

template <int LO, int HI> void check_int() {
    for (int v = LO - 2; v <= HI + 2; ++v) {
        Seen s;
        xp::with_int<LO, HI>(v, s);
        const int want = (v >= LO && v <= HI) ? v : HI;
        CHECK(s.calls == 1 && s.value == want, "with_int<%d, %d>(%d): %d call(s), value %d, want %d", LO, HI, v, s.calls, s.value, want);
    }
}

int main() {
    check_int<1, 4>();          // layer, variable and target counts
    check_int<0, 4>();          // the hydrostatic layers
    check_int<0, 3>();
    check_int<-1, 1>();
    check_int<7, 7>();

    enum { A = 5, B = 2, C = 9 };                        // not contiguous, not ordered: the last one is the default
    for (int v = 0; v <= 11; ++v) {
        Seen s;
        xp::with_one_of<A, B, C>(v, s);
        const int want = (v == A || v == B) ? v : C;
        CHECK(s.calls == 1 && s.value == want, "with_one_of<5, 2, 9>(%d): %d call(s), value %d, want %d", v, s.calls, s.value, want);
        Seen one;
        xp::with_one_of<A>(v, one);
        CHECK(one.calls == 1 && one.value == A, "with_one_of<5>(%d): %d call(s), value %d", v, one.calls, one.value);
    }

    for (int b = 0; b <= 1; ++b) {
        Seen s;
        xp::with_bool(b != 0, s);
        CHECK(s.calls == 1 && s.value == b, "with_bool(%d): %d call(s), value %d", b, s.calls, s.value);
        SeenType t;
        xp::with_type(b != 0, t);
        CHECK(t.calls == 1 && t.floating && t.size == (b ? 8 : 4), "with_type(%d): %d call(s), size %d", b, t.calls, t.size);
    }
    {                                                    // an int flag (CapeArgs::hum, ::persist) is true when non-zero
        Seen s;
        xp::with_bool(2, s);
        CHECK(s.calls == 1 && s.value == 1, "with_bool(2): %d call(s), value %d", s.calls, s.value);
    }

    const long long n[] = {-1, 0, 1, 256, 257}, want256[] = {0, 0, 1, 1, 2};
    for (int i = 0; i < 5; ++i)
        CHECK(xp::blocks_for(n[i]) == (unsigned)want256[i], "blocks_for(%lld) = %u, want %lld", n[i], xp::blocks_for(n[i]), want256[i]);
    CHECK(xp::blocks_for(1025, 1024) == 2 && xp::blocks_for(1024, 1024) == 1 && xp::blocks_for(0, 1024) == 0, "blocks_for(n, 1024)");
    CHECK(xp::blocks_for((1ll << 36) - 1) == (1u << 28), "blocks_for(2^36 - 1) = %u", xp::blocks_for((1ll << 36) - 1));

    // an assumed 10 CUs.  1024-thread workgroups, one per CU: the cap is 10 workgroups
    const int cu = 10;
    CHECK(xp::capped_blocks(9 * 1024 + 1, 1024, 1, cu) == 10, "1024 threads, at the cap from a partial workgroup");
    CHECK(xp::capped_blocks(9 * 1024, 1024, 1, cu) == 9, "1024 threads, below the cap");
    CHECK(xp::capped_blocks(10 * 1024, 1024, 1, cu) == 10, "1024 threads, at the cap");
    CHECK(xp::capped_blocks(10 * 1024 + 1, 1024, 1, cu) == 10, "1024 threads, above the cap");
    CHECK(xp::capped_blocks(1ll << 30, 1024, 1, cu) == 10, "1024 threads, far above the cap");
    CHECK(xp::capped_blocks(1, 1024, 1, cu) == 1 && xp::capped_blocks(0, 1024, 1, cu) == 0, "1024 threads, one column and none");
    // 256-thread workgroups, four per CU (1024 / 256, the k_cape_cin units' rule): the cap is 40
    CHECK(xp::capped_blocks(39 * 256, 256, 4, cu) == 39, "256 threads, below the cap");
    CHECK(xp::capped_blocks(40 * 256, 256, 4, cu) == 40, "256 threads, at the cap");
    CHECK(xp::capped_blocks(40 * 256 + 1, 256, 4, cu) == 40, "256 threads, above the cap");
    CHECK(xp::capped_blocks(1ll << 30, 256, 1, cu) == 10, "256 threads, one workgroup per CU");

    printf(failures ? "%d check(s) failed\n" : "xp_launch.hpp: all checks passed\n", failures);
    return failures ? 1 : 0;
}
