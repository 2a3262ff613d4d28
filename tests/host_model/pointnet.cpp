// pointnet.cpp -- the device functions of the sampling and grouping kernels (poseestimation_amd/csrc/so3_device.h: pointnet_dist2,
// fps_update, fps_key, fps_key_index, ball_radius2, ball_member, fps_shape) compiled for the host (SO3_HOST_MODEL) and driven by loops
// that compute what k_fps and k_ball_query compute, so that tests/test_pointnet_host.py checks the definition without a GPU.  TEST
// INFRASTRUCTURE ONLY.  The build switches contraction off, as the header does for these functions on the device.  Nothing here is
// approximate: a maximum of unique keys does not depend on the order the lanes, waves and slots are combined in, so the plain loop over
// j below gives the kernel's answer bit for bit.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../poseestimation_amd/csrc/so3_device.h"

extern "C" {

// so3_fps_f32
void model_fps(const float *xyz, const int32_t *start, int32_t *out, int64_t B, int32_t N, int32_t npoint) {
    std::vector<float> dist(N);
    for (int64_t b = 0; b < B; ++b) {
        const float *src = xyz + b * N * 3;
        for (int j = 0; j < N; ++j) dist[j] = so3::kFpsInit;
        int cur = std::min(std::max(start[b], 0), N - 1);
        for (int i = 0; i < npoint; ++i) {
            out[b * npoint + i] = cur;
            if (i + 1 == npoint) break;
            const float cx = src[cur * 3], cy = src[cur * 3 + 1], cz = src[cur * 3 + 2];
            unsigned long long best = 0;
            for (int j = 0; j < N; ++j) {
                so3::fps_update(so3::pointnet_dist2(src[j * 3], src[j * 3 + 1], src[j * 3 + 2], cx, cy, cz), dist[j]);
                best = std::max(best, so3::fps_key(dist[j], j));
            }
            cur = so3::fps_key_index(best);
        }
    }
}

// so3_ball_query_f32 (count optional; the early exit of the scan changes nothing that is written)
void model_ball_query(const float *xyz, const float *centres, float radius, int32_t nsample, int32_t *idx, int32_t *count, int64_t B,
                      int32_t N, int32_t S) {
    const int32_t width = std::min(nsample, N);
    const float r2 = so3::ball_radius2(radius);
    for (int64_t item = 0; item < B * S; ++item) {
        const float *src = xyz + item / S * N * 3, *c = centres + item * 3;
        int32_t *row = idx + item * width;
        int found = 0, first = N;
        for (int j = 0; j < N; ++j) {
            if (!so3::ball_member(so3::pointnet_dist2(src[j * 3], src[j * 3 + 1], src[j * 3 + 2], c[0], c[1], c[2]), r2)) continue;
            if (found == 0) first = j;
            if (found < width) row[found] = j;
            ++found;
        }
        for (int k = std::min(found, width); k < width; ++k) row[k] = first;
        if (count != nullptr) count[item] = found;
    }
}

// the instantiation k_fps's launcher picks for N
void model_fps_shape(int32_t N, int32_t *ppl, int32_t *block) {
    int p, b;
    so3::fps_shape(N, p, b);
    *ppl = p;
    *block = b;
}

}  // extern "C"
