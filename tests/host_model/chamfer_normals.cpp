// chamfer_normals.cpp -- the device functions of the Chamfer kernels with the normal term (poseestimation_amd/csrc/so3_device.h:
// add_s_pair, chamfer_length, chamfer_term, chamfer_cosine, chamfer_normal_term, chamfer_normal_psi, chamfer_normal_own, chamfer_hit,
// chamfer_points_per_lane) compiled for the host (SO3_HOST_MODEL) and driven by loops that keep the kernels' order of operations, so
// that tests/test_chamfer_normals_host.py measures the float32 arithmetic without a GPU.  TEST INFRASTRUCTURE ONLY.
// Differences from the device: libm's correctly rounded 1 / sqrt stands in for v_rsq_f32 (1 ulp).  The forward's work items, lane
// sums, butterfly, wave order and float64 chunk-order sums are wave_model.h's chamfer_direction, with a second sum for the term beside
// the distance's (k_chamfer_normals_fwd, k_chamfer_normals_rows); the backward is one chain per normal: the own pair, then the hits in
// ascending index (k_chamfer_normals_bwd).
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <algorithm>
#include <limits>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "wave_model.h"

namespace {

// one direction of one cloud's gradient: P's normals own, Q's hit
void gradient(const float *P, const float *Q, int32_t full, int32_t len_p, int32_t len_q, const int32_t *near_own, const int32_t *near_hit,
              const float *s_own, const float *s_hit, bool signed_cos, float *out) {
    const bool live_cloud = len_p > 0 && len_q > 0;
    for (int i = 0; i < full; ++i) {
        float acc[3] = {0.f, 0.f, 0.f};
        const bool keep = live_cloud && i < len_p;
        if (keep) {
            float ux, uy, uz;
            if (s_own != nullptr && near_own != nullptr) {
                const int j = std::min(std::max(near_own[i], 0), len_q - 1);
                so3::chamfer_normal_psi(P[i * 3], P[i * 3 + 1], P[i * 3 + 2], Q[j * 3], Q[j * 3 + 1], Q[j * 3 + 2], signed_cos, ux, uy, uz);
                so3::chamfer_normal_own(*s_own, ux, uy, uz, acc);
            }
            if (s_hit != nullptr && near_hit != nullptr) {
                for (int j = 0; j < len_q; ++j) {
                    if (near_hit[j] != i) continue;
                    so3::chamfer_normal_psi(P[i * 3], P[i * 3 + 1], P[i * 3 + 2], Q[j * 3], Q[j * 3 + 1], Q[j * 3 + 2], signed_cos, ux, uy, uz);
                    so3::chamfer_hit(*s_hit, ux, uy, uz, acc);
                }
            }
        }
        for (int k = 0; k < 3; ++k) out[i * 3 + k] = keep ? acc[k] : 0.f;
    }
}

}  // namespace

extern "C" {

// so3_chamfer_normals_fwd_f32 on a device of `cus` compute units (flags: 1 unsquared, 2 single direction, 4 signed cosine);
// u_override > 0 sets the points per lane instead of the launcher's rule
void model_chamfer_normals_fwd(const float *X, const float *Y, const float *NX, const float *NY, const int32_t *x_len, const int32_t *y_len,
                               float *dist_x, int32_t *nearest_x, float *dist_y, int32_t *nearest_y, float *term_x, float *term_y, float *rows,
                               float *rows_n, uint32_t flags, int64_t B, int32_t N, int32_t M, int64_t cus, int32_t u_override) {
    const bool squared = (flags & 1u) == 0, single = (flags & 2u) != 0, sc = (flags & 4u) != 0;
    const int u = u_override > 0 ? u_override : so3::chamfer_points_per_lane(B, N, M, single, cus);
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *x = X + b * N * 3, *y = Y + b * M * 3, *nx = NX + b * N * 3, *ny = NY + b * M * 3;
        float *dx = dist_x != nullptr ? dist_x + b * N : nullptr, *dy = dist_y != nullptr ? dist_y + b * M : nullptr;
        float *tx = term_x != nullptr ? term_x + b * N : nullptr, *ty = term_y != nullptr ? term_y + b * M : nullptr;
        int32_t *ix = nearest_x != nullptr ? nearest_x + b * N : nullptr, *iy = nearest_y != nullptr ? nearest_y + b * M : nullptr;
        double sx[2], sy[2] = {0.0, 0.0};
        if (squared) chamfer_direction<true, true>(x, y, nx, ny, N, nb, mb, dx, ix, tx, sc, u, sx);
        else chamfer_direction<false, true>(x, y, nx, ny, N, nb, mb, dx, ix, tx, sc, u, sx);
        if (!single) {
            if (squared) chamfer_direction<true, true>(y, x, ny, nx, M, mb, nb, dy, iy, ty, sc, u, sy);
            else chamfer_direction<false, true>(y, x, ny, nx, M, mb, nb, dy, iy, ty, sc, u, sy);
        }
        const bool live = nb > 0 && mb > 0;
        for (int k = 0; k < 2; ++k) {
            float *r = k == 0 ? rows : rows_n;
            r[b * 2 + 0] = live ? static_cast<float>(sx[k] / static_cast<double>(nb)) : 0.f;
            r[b * 2 + 1] = live && !single ? static_cast<float>(sy[k] / static_cast<double>(mb)) : 0.f;
        }
    }
}

// so3_chamfer_normals_bwd_f32 (scale_y and nearest_y NULL: the x direction alone)
void model_chamfer_normals_bwd(const float *NX, const float *NY, const int32_t *x_len, const int32_t *y_len, const int32_t *nearest_x,
                               const int32_t *nearest_y, const float *scale_x, const float *scale_y, float *dNX, float *dNY, uint32_t flags, int64_t B,
                               int32_t N, int32_t M) {
    const bool sc = (flags & 4u) != 0;
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *nx = NX + b * N * 3, *ny = NY + b * M * 3;
        const int32_t *ix = nearest_x + b * N, *iy = nearest_y != nullptr ? nearest_y + b * M : nullptr;
        const float *sx = scale_x + b, *sy = scale_y != nullptr ? scale_y + b : nullptr;
        if (dNX != nullptr) gradient(nx, ny, N, nb, mb, ix, iy, sx, sy, sc, dNX + b * N * 3);
        if (dNY != nullptr) gradient(ny, nx, M, mb, nb, iy, ix, sy, sx, sc, dNY + b * M * 3);
    }
}

}  // extern "C"
