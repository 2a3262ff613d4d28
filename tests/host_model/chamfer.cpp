// chamfer.cpp -- the device functions of the Chamfer kernels (poseestimation_amd/csrc/so3_device.h: add_s_pair, chamfer_length,
// chamfer_term, chamfer_phi, chamfer_own, chamfer_hit, chamfer_points_per_lane) compiled for the host (SO3_HOST_MODEL) and driven by
// loops that keep the kernels' order of operations, so that tests/test_chamfer_host.py measures the float32 arithmetic without a GPU.
// TEST INFRASTRUCTURE ONLY.
// Differences from the device: libm's correctly rounded sqrt / division stand in for v_sqrt_f32 / v_rcp_f32 (1 ulp).  A forward work
// item is kIcpBlock * U source points: slot u * 256 + tid of the chunk on lane tid % 64 of wave tid / 64; a lane adds its slots in
// order, the wave's sum is the xor butterfly (as wave_allsum: its DPP mirrors add the same partners' sums), the four waves in wave
// order, a cloud's records in chunk order in float64 -- k_chamfer_fwd and k_chamfer_rows at the U the launcher picks for `cus`
// compute units.  The backward is one chain per point: the own term, then the hits in ascending index (k_chamfer_bwd).
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <algorithm>
#include <limits>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "wave_model.h"

namespace {

// one direction of one cloud's gradient: P's points own, Q's points hit
template <bool SQUARED>
void gradient(const float *P, const float *Q, int32_t full, int32_t len_p, int32_t len_q, const int32_t *near_own, const int32_t *near_hit,
              const float *s_own, const float *s_hit, float *out) {
    const bool live_cloud = len_p > 0 && len_q > 0;
    for (int i = 0; i < full; ++i) {
        float acc[3] = {0.f, 0.f, 0.f};
        const bool keep = live_cloud && i < len_p;
        if (keep) {
            if (s_own != nullptr && near_own != nullptr) {
                const int j = std::min(std::max(near_own[i], 0), len_q - 1);
                so3::chamfer_own<SQUARED>(*s_own, P[i * 3] - Q[j * 3], P[i * 3 + 1] - Q[j * 3 + 1], P[i * 3 + 2] - Q[j * 3 + 2], acc);
            }
            if (s_hit != nullptr && near_hit != nullptr) {
                for (int j = 0; j < len_q; ++j) {
                    if (near_hit[j] != i) continue;
                    float ux, uy, uz;
                    so3::chamfer_phi<SQUARED>(P[i * 3] - Q[j * 3], P[i * 3 + 1] - Q[j * 3 + 1], P[i * 3 + 2] - Q[j * 3 + 2], ux, uy, uz);
                    so3::chamfer_hit(*s_hit, ux, uy, uz, acc);
                }
            }
        }
        for (int k = 0; k < 3; ++k) out[i * 3 + k] = keep ? acc[k] : 0.f;
    }
}

}  // namespace

extern "C" {

int model_chamfer_points_per_lane(int64_t B, int32_t N, int32_t M, int32_t single, int64_t cus) {
    return so3::chamfer_points_per_lane(B, N, M, single != 0, cus);
}

// so3_chamfer_fwd_f32 on a device of `cus` compute units (flags: 1 unsquared, 2 single direction)
void model_chamfer_fwd(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, float *dist_x, int32_t *nearest_x, float *dist_y,
                       int32_t *nearest_y, float *rows, uint32_t flags, int64_t B, int32_t N, int32_t M, int64_t cus) {
    const bool squared = (flags & 1u) == 0, single = (flags & 2u) != 0;
    const int u = so3::chamfer_points_per_lane(B, N, M, single, cus);
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *x = X + b * N * 3, *y = Y + b * M * 3;
        float *dx = dist_x != nullptr ? dist_x + b * N : nullptr, *dy = dist_y != nullptr ? dist_y + b * M : nullptr;
        int32_t *ix = nearest_x != nullptr ? nearest_x + b * N : nullptr, *iy = nearest_y != nullptr ? nearest_y + b * M : nullptr;
        double sx[2], sy[2] = {0.0, 0.0};
        if (squared) chamfer_direction<true, false>(x, y, nullptr, nullptr, N, nb, mb, dx, ix, nullptr, false, u, sx);
        else chamfer_direction<false, false>(x, y, nullptr, nullptr, N, nb, mb, dx, ix, nullptr, false, u, sx);
        if (!single) {
            if (squared) chamfer_direction<true, false>(y, x, nullptr, nullptr, M, mb, nb, dy, iy, nullptr, false, u, sy);
            else chamfer_direction<false, false>(y, x, nullptr, nullptr, M, mb, nb, dy, iy, nullptr, false, u, sy);
        }
        const bool live = nb > 0 && mb > 0;
        rows[b * 2 + 0] = live ? static_cast<float>(sx[0] / static_cast<double>(nb)) : 0.f;
        rows[b * 2 + 1] = live && !single ? static_cast<float>(sy[0] / static_cast<double>(mb)) : 0.f;
    }
}

// so3_chamfer_bwd_f32 (scale_y and nearest_y NULL: the x direction alone)
void model_chamfer_bwd(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, const int32_t *nearest_x,
                       const int32_t *nearest_y, const float *scale_x, const float *scale_y, float *dX, float *dY, uint32_t flags, int64_t B, int32_t N,
                       int32_t M) {
    const bool squared = (flags & 1u) == 0;
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *x = X + b * N * 3, *y = Y + b * M * 3;
        const int32_t *ix = nearest_x + b * N, *iy = nearest_y != nullptr ? nearest_y + b * M : nullptr;
        const float *sx = scale_x + b, *sy = scale_y != nullptr ? scale_y + b : nullptr;
        if (dX != nullptr) {
            if (squared) gradient<true>(x, y, N, nb, mb, ix, iy, sx, sy, dX + b * N * 3);
            else gradient<false>(x, y, N, nb, mb, ix, iy, sx, sy, dX + b * N * 3);
        }
        if (dY != nullptr) {
            if (squared) gradient<true>(y, x, M, mb, nb, iy, ix, sy, sx, dY + b * M * 3);
            else gradient<false>(y, x, M, mb, nb, iy, ix, sy, sx, dY + b * M * 3);
        }
    }
}

}  // extern "C"
