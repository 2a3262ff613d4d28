// icp.cpp -- the device functions of the ICP kernels (poseestimation_amd/csrc/so3_device.h: pose_point, add_s_pair, icp_accumulate,
// icp_finish and what they call, icp_points_per_lane) compiled for the host (SO3_HOST_MODEL) and driven by loops that keep the
// kernels' order of operations, so that tests/test_icp_host.py measures the float32 arithmetic without a GPU.  TEST INFRASTRUCTURE ONLY.
// Differences from the device: libm's correctly rounded sqrt / division stand in for v_sqrt_f32 / v_rcp_f32 (1 ulp), and the build
// does not contract a * b + c.  A work item is kIcpBlock * U source points: point u * 256 + tid of the chunk on lane tid % 64 of wave
// tid / 64, the waves' sums by the xor butterfly (as wave_allsum: its DPP mirrors add the same partners' sums), the four waves in wave
// order, the chunks in chunk order -- k_icp_step and k_icp_finish at the U the launcher picks for `cus` compute units.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <limits>
#include <vector>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "wave_model.h"

namespace {

// the search of one source point: the target in index order (tiles and their padding change neither the order nor the result)
void search(const float *pose, const float *p, const float *tgt, int32_t M, float &best, int &idx) {
    float x = p[0], y = p[1], z = p[2];
    if (pose != nullptr) {
        float m[12];
        for (int k = 0; k < 12; ++k) m[k] = pose[k];
        so3::pose_point(m, p[0], p[1], p[2], x, y, z);
    }
    best = std::numeric_limits<float>::infinity();
    idx = 0;
    for (int j = 0; j < M; ++j) so3::add_s_pair<true, false>(x, y, z, tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], j, best, idx);
    idx = std::min(idx, M - 1);
}

// k_icp_step<.., SUMS = true, U> over one cloud: records (chunks, kIcpRecord)
template <bool TRIMMED>
void step(const float *src, const float *tgt, const float *w, const float *pose, float max_distance, float *rec, float *dist, int32_t *nearest,
          int32_t N, int32_t M, int u) {
    const int per = so3::kIcpBlock * u, chunks = (N + per - 1) / per;
    const float p0[3] = {src[0], src[1], src[2]}, q0[3] = {tgt[0], tgt[1], tgt[2]};
    for (int c = 0; c < chunks; ++c) {
        static float acc[so3::kIcpBlock][so3::kIcpSums];
        for (int t = 0; t < so3::kIcpBlock; ++t)
            for (int k = 0; k < so3::kIcpSums; ++k) acc[t][k] = 0.f;
        for (int uu = 0; uu < u; ++uu) {
            for (int t = 0; t < so3::kIcpBlock; ++t) {
                const int i = c * per + uu * so3::kIcpBlock + t;
                const bool in = i < N;
                const int ic = std::min(i, N - 1);
                float best;
                int j;
                search(pose, src + ic * 3, tgt, M, best, j);
                const float d = so3::hw::sqrt(best);
                if (in) {
                    if (dist != nullptr) dist[i] = d;
                    if (nearest != nullptr) nearest[i] = j;
                }
                const float wi = in ? (w != nullptr ? w[ic] : 1.f) : 0.f;
                so3::icp_accumulate<TRIMMED>(wi, best, d, max_distance, src[ic * 3] - p0[0], src[ic * 3 + 1] - p0[1], src[ic * 3 + 2] - p0[2],
                                             tgt[j * 3] - q0[0], tgt[j * 3 + 1] - q0[1], tgt[j * 3 + 2] - q0[2], acc[t]);
            }
        }
        for (int k = 0; k < so3::kIcpRecord; ++k) {
            float v = 0.f;
            if (k < so3::kIcpSums) {
                for (int wv = 0; wv < so3::kIcpBlock / 64; ++wv) {
                    float lane[64];
                    for (int l = 0; l < 64; ++l) lane[l] = acc[wv * 64 + l][k];
                    const float tot = wave_allsum(lane);
                    v = wv == 0 ? tot : v + tot;
                }
            }
            rec[c * so3::kIcpRecord + k] = v;
        }
    }
}

}  // namespace

extern "C" {

// so3_nearest_f32
void model_nearest(const float *X, const float *Y, int64_t y_stride, float *dist, int32_t *nearest, int64_t B, int32_t N, int32_t M) {
    for (int64_t b = 0; b < B; ++b) {
        for (int i = 0; i < N; ++i) {
            float best;
            int j;
            search(nullptr, X + (b * N + i) * 3, Y + b * y_stride, M, best, j);
            dist[b * N + i] = so3::hw::sqrt(best);
            if (nearest != nullptr) nearest[b * N + i] = j;
        }
    }
}

int model_icp_points_per_lane(int64_t B, int32_t N, int64_t cus) { return so3::icp_points_per_lane(B, N, cus); }

// so3_icp_f32 on a device of `cus` compute units (iterations >= 1; the outputs as the C ABI's, each optional but R and t)
void model_icp(const float *P, const float *Q, int64_t q_stride, const float *w, const float *T_init, float max_distance, int32_t iterations,
               float *R, float *t, float *rmse, int32_t *inliers, int32_t *nearest, float *dist, int64_t B, int32_t N, int32_t M, int64_t cus) {
    const int u = so3::icp_points_per_lane(B, N, cus);
    const int per = so3::kIcpBlock * u, chunks = (N + per - 1) / per;
    std::vector<float> rec(static_cast<size_t>(chunks) * so3::kIcpRecord);
    for (int64_t b = 0; b < B; ++b) {
        const float *src = P + b * N * 3, *tgt = Q + b * q_stride, *wb = w != nullptr ? w + b * N : nullptr;
        float cur[12], next[12];
        bool have = T_init != nullptr;
        for (int k = 0; k < 12; ++k) cur[k] = have ? T_init[b * 12 + k] : ((k % 5) == 0 ? 1.f : 0.f);
        for (int32_t it = 0; it < iterations; ++it) {
            const bool last = it + 1 == iterations;
            float *dd = last && dist != nullptr ? dist + b * N : nullptr;
            int32_t *nn = last && nearest != nullptr ? nearest + b * N : nullptr;
            if (max_distance >= 0.f) step<true>(src, tgt, wb, have ? cur : nullptr, max_distance, rec.data(), dd, nn, N, M, u);
            else step<false>(src, tgt, wb, have ? cur : nullptr, max_distance, rec.data(), dd, nn, N, M, u);
            float s[so3::kIcpSums];
            for (int k = 0; k < so3::kIcpSums; ++k) {
                float v = 0.f;
                for (int c = 0; c < chunks; ++c) v += rec[c * so3::kIcpRecord + k];
                s[k] = v;
            }
            const float p0[3] = {src[0], src[1], src[2]}, q0[3] = {tgt[0], tgt[1], tgt[2]};
            float e, cnt;
            so3::icp_finish(s, p0, q0, cur, next, e, cnt);
            for (int k = 0; k < 12; ++k) cur[k] = next[k];
            have = true;
            if (rmse != nullptr) rmse[it * B + b] = e;
            if (inliers != nullptr) inliers[it * B + b] = static_cast<int32_t>(cnt);
        }
        for (int c = 0; c < 3; ++c) {
            for (int k = 0; k < 3; ++k) R[b * 9 + 3 * c + k] = cur[4 * c + k];
            t[b * 3 + c] = cur[4 * c + 3];
        }
    }
}

}  // extern "C"
