// dispatch.cpp -- the launchers' run-time to template selection (poseestimation_amd/csrc/so3_dispatch.h: with_flags, with_value,
// kernel_label) and the cloud kernels' launch shape (so3_device.h: clouds_per_wave, cloud_blocks) compiled for the host, so that
// tests/test_dispatch_host.py checks them without a GPU.  TEST INFRASTRUCTURE ONLY.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "../../poseestimation_amd/csrc/so3_dispatch.h"

extern "C" {

// with_flags over the low n bits of `bits` (flag i = bit i, in argument order).  *calls counts the calls of the callable; *seen is
// rebuilt from the CONSTANTS it received, constant i at bit i, and bit 8 + j is set when j constants arrived.
void model_with_flags(int n, int bits, int *calls, int *seen) {
    const bool a = bits & 1, b = bits & 2, c = bits & 4, d = bits & 8;
    *calls = 0;
    *seen = 0;
    if (n == 1) so3::with_flags([&](auto A) { ++*calls; *seen = (1 << 9) | A(); }, a);
    if (n == 2) so3::with_flags([&](auto A, auto B) { ++*calls; *seen = (1 << 10) | A() | B() << 1; }, a, b);
    if (n == 3) so3::with_flags([&](auto A, auto B, auto C) { ++*calls; *seen = (1 << 11) | A() | B() << 1 | C() << 2; }, a, b, c);
    if (n == 4)
        so3::with_flags([&](auto A, auto B, auto C, auto D) {
            static_assert(std::is_same_v<decltype(A), std::bool_constant<A()>>, "a constant, not a bool");
            ++*calls;
            *seen = (1 << 12) | A() | B() << 1 | C() << 2 | D() << 3;
        }, a, b, c, d);
}

// with_value<1, 2, 4>: returns what it returns; *got is the constant the callable received (untouched without a call).
int model_with_value(int v, int *calls, int *got) {
    *calls = 0;
    return so3::with_value<1, 2, 4>(v, [&](auto V) {
        static_assert(std::is_same_v<decltype(V), std::integral_constant<int, V()>>, "a constant, not an int");
        ++*calls;
        *got = V();
    }) ? 1 : 0;
}

// kernel_label into buf[0, n); the bytes from buf[n] on are the caller's and must stay untouched.  The arguments are the constants the
// dispatchers hand out (cases 0-2), plain values (3, 4), none (5).
void model_kernel_label(int which, char *buf, size_t n) {
    switch (which) {
        case 0:
            so3::with_flags([&](auto W, auto T, auto S) {
                so3::with_value<4, 2, 1>(4, [&](auto U) { so3::kernel_label(buf, n, "k_icp_step", W, T, S, U); });
            }, false, false, false);
            break;
        case 1: so3::with_flags([&](auto CF) { so3::kernel_label(buf, n, "k_group_bwd", CF, 64, 16); }, true); break;
        case 2:
            so3::with_value<8>(8, [&](auto PP) { so3::kernel_label(buf, n, "k_fps", PP, std::integral_constant<int, 1024>{}); });
            break;
        case 3: so3::kernel_label(buf, n, "k_sym_add", 2, false, 16); break;
        case 4: so3::kernel_label(buf, n, "k_three_nn", 1, true); break;
        default: so3::kernel_label(buf, n, "k_three_interp_bwd_cf"); break;
    }
}

int32_t model_clouds_per_wave(int64_t B, int64_t cus) { return so3::clouds_per_wave(B, cus); }
int64_t model_cloud_blocks(int64_t B, int32_t per_wave) { return so3::cloud_blocks(B, per_wave); }

}  // extern "C"
