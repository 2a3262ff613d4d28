// grouping.cpp -- the device functions of the grouping kernels (poseestimation_amd/csrc/so3_device.h: group_valid, group_relative,
// group_bwd_add, group_channel, group_bwd_narrow) compiled for the host (SO3_HOST_MODEL) and driven by loops that compute what
// k_group_fwd, k_group_bwd and k_group_centres_bwd compute, so that tests/test_grouping_host.py checks the definition without a GPU.
// TEST INFRASTRUCTURE ONLY.  The backward walks grad_out's slots in their ascending memory order and adds each valid one to the point
// it selected -- per point that is the order in which the kernel's owning lane meets its hits, whatever the tile and the owner group.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include "../../poseestimation_amd/csrc/so3_device.h"

extern "C" {

static inline int64_t out_offset(int32_t cf, int64_t b, int64_t s, int64_t k, int64_t c, int64_t S, int64_t K, int64_t C) {
    return cf ? ((b * C + c) * K + k) * S + s : ((b * S + s) * K + k) * C + c;
}

// so3_group_points_f32
void model_group_points(const float *xyz, const float *centres, const float *feat, const int32_t *idx, float *out, int32_t features_first,
                        int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t K, int32_t D) {
    const int32_t C = 3 + D;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t s = 0; s < S; ++s)
            for (int64_t k = 0; k < K; ++k) {
                const int32_t i = idx[(b * S + s) * K + k];
                const bool ok = so3::group_valid(i, N);
                for (int32_t c = 0; c < C; ++c) {
                    int32_t d;
                    const int j = so3::group_channel(features_first != 0, D, c, d);
                    float v = 0.f;
                    if (ok) {
                        if (j >= 0) v = so3::group_relative(xyz[(b * N + i) * 3 + j], centres[(b * S + s) * 3 + j]);
                        else v = channels_first ? feat[(b * D + d) * N + i] : feat[(b * N + i) * D + d];
                    }
                    out[out_offset(channels_first, b, s, k, c, S, K, C)] = v;
                }
            }
}

// so3_group_points_bwd_f32: each of the three outputs may be null
void model_group_points_bwd(const float *grad_out, const int32_t *idx, float *grad_xyz, float *grad_centres, float *grad_feat,
                            int32_t features_first, int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t K, int32_t D) {
    const int32_t C = 3 + D;
    if (D == 0) grad_feat = nullptr;
    for (int64_t e = 0; grad_xyz != nullptr && e < B * N * 3; ++e) grad_xyz[e] = 0.f;
    for (int64_t e = 0; grad_feat != nullptr && e < B * N * D; ++e) grad_feat[e] = 0.f;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t slot = 0; slot < static_cast<int64_t>(S) * K; ++slot) {
            const int64_t s = channels_first ? slot % S : slot / K, k = channels_first ? slot / S : slot % K;
            const int32_t i = idx[(b * S + s) * K + k];
            if (!so3::group_valid(i, N)) continue;
            for (int32_t c = 0; c < C; ++c) {
                int32_t d;
                const int j = so3::group_channel(features_first != 0, D, c, d);
                const float g = grad_out[out_offset(channels_first, b, s, k, c, S, K, C)];
                if (j >= 0) {
                    if (grad_xyz != nullptr) grad_xyz[(b * N + i) * 3 + j] = so3::group_bwd_add(grad_xyz[(b * N + i) * 3 + j], g);
                } else if (grad_feat != nullptr) {
                    float &acc = channels_first ? grad_feat[(b * D + d) * N + i] : grad_feat[(b * N + i) * D + d];
                    acc = so3::group_bwd_add(acc, g);
                }
            }
        }
    if (grad_centres == nullptr) return;
    const int32_t xb = features_first ? D : 0;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t s = 0; s < S; ++s)
            for (int j = 0; j < 3; ++j) {
                float acc = 0.f;
                for (int64_t k = 0; k < K; ++k)
                    if (so3::group_valid(idx[(b * S + s) * K + k], N)) acc = so3::group_bwd_add(acc, grad_out[out_offset(channels_first, b, s, k, xb + j, S, K, C)]);
                grad_centres[(b * S + s) * 3 + j] = 0.f - acc;
            }
}

// the dispatch of so3_group_points_bwd_f32: 1 = the narrow kernel (eight owner groups x eight channels per wave)
int32_t model_group_bwd_narrow(int32_t D) { return so3::group_bwd_narrow(D) ? 1 : 0; }

}  // extern "C"
