// add_metrics.cpp -- the device functions of the ADD / ADD-S / diameter kernels (poseestimation_amd/csrc/so3_device.h: pose_point,
// pair_dist2, add_s_pair, unit_scale) compiled for the host (SO3_HOST_MODEL) and driven by loops that keep the kernels' order of
// operations, so that tests/test_add_metrics_host.py measures the float32 arithmetic without a GPU.  TEST INFRASTRUCTURE ONLY.
// Differences from the device: libm's correctly rounded sqrt / division stand in for v_sqrt_f32 / v_rcp_f32 (1 ulp), and the build
// does not contract a * b + c.  A "wave" is 64 float accumulators filled lane-strided and summed by the xor butterfly, as
// wave_allsum does (its DPP mirrors add the same partners' sums).
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <limits>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "wave_model.h"

namespace {

void top_rows(const float *T, float (&m)[12]) {
    for (int k = 0; k < 12; ++k) m[k] = T[k];
}

// k_add_s: every outer point against the inner cloud in index order (tiles and their padding do not change the order or the result)
template <bool DIAMETER>
void add_s(const float *Tgt, const float *Tpred, const float *pts, float *point_dist, int32_t *nearest, float *rows, int64_t B, int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        const float *cloud = pts + b * N * 3;
        float mg[12] = {0}, mp[12] = {0};
        if (!DIAMETER) { top_rows(Tgt + b * 16, mg); top_rows(Tpred + b * 16, mp); }
        double sum = 0.0;
        float mx = 0.f;
        for (int i = 0; i < N; ++i) {
            float x = cloud[i * 3], y = cloud[i * 3 + 1], z = cloud[i * 3 + 2];
            if (!DIAMETER) so3::pose_point(mg, cloud[i * 3], cloud[i * 3 + 1], cloud[i * 3 + 2], x, y, z);
            float best = DIAMETER ? 0.f : std::numeric_limits<float>::infinity();
            int idx = 0;
            for (int j = 0; j < N; ++j) {
                float qx = cloud[j * 3], qy = cloud[j * 3 + 1], qz = cloud[j * 3 + 2];
                if (!DIAMETER) so3::pose_point(mp, cloud[j * 3], cloud[j * 3 + 1], cloud[j * 3 + 2], qx, qy, qz);
                so3::add_s_pair<!DIAMETER, DIAMETER>(x, y, z, qx, qy, qz, j, best, idx);
            }
            const float d = so3::hw::sqrt(best);
            point_dist[b * N + i] = d;
            if (nearest != nullptr) nearest[b * N + i] = idx;
            sum += static_cast<double>(d);
            mx = std::max(mx, d);
        }
        rows[b] = DIAMETER ? mx : static_cast<float>(sum / static_cast<double>(N));       // k_add_s_rows
    }
}

}  // namespace

extern "C" {

void model_add_s_fwd(const float *Tgt, const float *Tpred, const float *pts, float *point_dist, int32_t *nearest, float *dists, int64_t B,
                     int32_t N) {
    add_s<false>(Tgt, Tpred, pts, point_dist, nearest, dists, B, N);
}

void model_cloud_diameter(const float *pts, float *work, float *diam, int64_t B, int32_t N) {
    add_s<true>(nullptr, nullptr, pts, work, nullptr, diam, B, N);
}

// k_add_s_bwd
void model_add_s_bwd(const float *Tgt, const float *Tpred, const float *pts, const int32_t *nearest, const float *grad_rows, float grad_scale,
                     float *dT, int64_t B, int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        const float *cloud = pts + b * N * 3;
        float mg[12], mp[12];
        top_rows(Tgt + b * 16, mg);
        top_rows(Tpred + b * 16, mp);
        float acc[12][64] = {};
        for (int i = 0; i < N; ++i) {
            const int lane = i & 63;
            const int j = std::min(std::max(nearest[b * N + i], 0), N - 1);
            float ex, ey, ez, qx, qy, qz;
            so3::pose_point(mg, cloud[i * 3], cloud[i * 3 + 1], cloud[i * 3 + 2], ex, ey, ez);
            const float px = cloud[j * 3], py = cloud[j * 3 + 1], pz = cloud[j * 3 + 2];
            so3::pose_point(mp, px, py, pz, qx, qy, qz);
            ex -= qx; ey -= qy; ez -= qz;
            const float inv = so3::unit_scale(so3::pair_dist2(ex, ey, ez));
            const float u[3] = {ex * inv, ey * inv, ez * inv};
            for (int c = 0; c < 3; ++c) {
                acc[4 * c + 0][lane] = std::fma(u[c], px, acc[4 * c + 0][lane]);
                acc[4 * c + 1][lane] = std::fma(u[c], py, acc[4 * c + 1][lane]);
                acc[4 * c + 2][lane] = std::fma(u[c], pz, acc[4 * c + 2][lane]);
                acc[4 * c + 3][lane] += u[c];
            }
        }
        const float k = -grad_scale * (grad_rows != nullptr ? grad_rows[b] : 1.f) / static_cast<float>(N);
        for (int e = 0; e < 12; ++e) dT[b * 16 + e] = k * wave_allsum(acc[e]);
        for (int e = 12; e < 16; ++e) dT[b * 16 + e] = 0.f;
    }
}

// k_add_l1<false, U, L2>: d = (R_gt - R_pred) p + (t_gt - t_pred)
void model_add_l2(const float *Tgt, const float *Tpred, const float *pts, float *dists, float *dT, float grad_scale, int64_t B, int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        const float *cloud = pts + b * N * 3, *tg = Tgt + b * 16, *tp = Tpred + b * 16;
        float dr[9], dt[3];
        for (int c = 0; c < 3; ++c) {
            for (int k = 0; k < 3; ++k) dr[3 * c + k] = tg[4 * c + k] - tp[4 * c + k];
            dt[c] = tg[4 * c + 3] - tp[4 * c + 3];
        }
        float acc[13][64] = {};
        for (int i = 0; i < N; ++i) {
            const int lane = i & 63;
            const float px = cloud[i * 3], py = cloud[i * 3 + 1], pz = cloud[i * 3 + 2];
            const float dx = std::fma(dr[0], px, std::fma(dr[1], py, std::fma(dr[2], pz, dt[0])));
            const float dy = std::fma(dr[3], px, std::fma(dr[4], py, std::fma(dr[5], pz, dt[1])));
            const float dz = std::fma(dr[6], px, std::fma(dr[7], py, std::fma(dr[8], pz, dt[2])));
            const float d2 = so3::pair_dist2(dx, dy, dz);
            const float inv = so3::unit_scale(d2);
            acc[0][lane] += so3::hw::sqrt(d2);
            const float s[3] = {dx * inv, dy * inv, dz * inv};
            for (int c = 0; c < 3; ++c) {
                acc[1 + 3 * c][lane] = std::fma(s[c], px, acc[1 + 3 * c][lane]);
                acc[2 + 3 * c][lane] = std::fma(s[c], py, acc[2 + 3 * c][lane]);
                acc[3 + 3 * c][lane] = std::fma(s[c], pz, acc[3 + 3 * c][lane]);
                acc[10 + c][lane] += s[c];
            }
        }
        const float inv_n = 1.0f / static_cast<float>(N);
        dists[b] = wave_allsum(acc[0]) * inv_n;
        const float k = -grad_scale * inv_n;
        for (int c = 0; c < 3; ++c) {
            for (int j = 0; j < 3; ++j) dT[b * 16 + 4 * c + j] = k * wave_allsum(acc[1 + 3 * c + j]);
            dT[b * 16 + 4 * c + 3] = k * wave_allsum(acc[10 + c]);
        }
        for (int e = 12; e < 16; ++e) dT[b * 16 + e] = 0.f;
    }
}

}  // extern "C"
