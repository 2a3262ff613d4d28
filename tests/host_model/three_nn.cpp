// three_nn.cpp -- the device functions of the feature-propagation kernels (poseestimation_amd/csrc/so3_device.h: pointnet_dist2,
// three_nn_put, three_nn_finish, three_nn_weights, three_interp, three_interp_bwd_add, three_nn_waves_per_point) compiled for the host
// (SO3_HOST_MODEL) and driven by loops that compute what k_three_nn, k_three_interp and the two backward kernels compute, so that
// tests/test_three_nn_host.py checks the definition without a GPU.  TEST INFRASTRUCTURE ONLY.  The build switches contraction off, as
// the header does for these functions on the device.  Nothing here is approximate: the three smallest under a total order do not
// depend on how the kernel splits the known cloud over tiles and waves (model_three_nn takes `slices` to show exactly that: the scan
// dealt to that many lists, merged as the kernel merges them), and the backward's sum is defined with its order.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../poseestimation_amd/csrc/so3_device.h"

extern "C" {

// so3_three_nn_f32 (weight optional); slices in {1, 2, 4}: blocks of eight known points dealt to the lists in turn, as k_three_nn<WPP> deals them
void model_three_nn(const float *unknown, const float *known, float *dist2, int32_t *idx, float *weight, int64_t B, int32_t N, int32_t S,
                    int32_t slices) {
    for (int64_t row = 0; row < B * N; ++row) {
        const float *p = unknown + row * 3, *tgt = known + row / N * S * 3;
        float D[4][3];
        int J[4][3];
        for (int w = 0; w < 4; ++w)
            for (int k = 0; k < 3; ++k) { D[w][k] = __builtin_huge_valf(); J[w][k] = so3::kThreeNnNone; }
        for (int j = 0; j < S; ++j) {
            const int w = (j % so3::kThreeNnTile) / 8 % slices;
            so3::three_nn_put<false>(so3::pointnet_dist2(tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], p[0], p[1], p[2]), j, D[w], J[w]);
        }
        for (int w = 1; w < slices; ++w)
            for (int k = 0; k < 3; ++k) so3::three_nn_put<true>(D[w][k], J[w][k], D[0], J[0]);
        so3::three_nn_finish(S, D[0], J[0]);
        for (int k = 0; k < 3; ++k) { dist2[row * 3 + k] = D[0][k]; idx[row * 3 + k] = J[0][k]; }
        if (weight != nullptr) {
            float W[3];
            so3::three_nn_weights(S, D[0], W);
            for (int k = 0; k < 3; ++k) weight[row * 3 + k] = W[k];
        }
    }
}

static inline int64_t clamp_index(int32_t i, int32_t S) { return std::min(std::max(i, 0), S - 1); }

// so3_three_interpolate_f32
void model_three_interpolate(const float *feat, const int32_t *idx, const float *weight, float *out, int32_t channels_first, int64_t B, int32_t N,
                             int32_t S, int32_t D) {
    for (int64_t row = 0; row < B * N; ++row) {
        const int64_t b = row / N, n = row - b * N;
        const int64_t i0 = clamp_index(idx[row * 3], S), i1 = clamp_index(idx[row * 3 + 1], S), i2 = clamp_index(idx[row * 3 + 2], S);
        const float w0 = weight[row * 3], w1 = weight[row * 3 + 1], w2 = weight[row * 3 + 2];
        for (int64_t c = 0; c < D; ++c) {
            if (channels_first) {
                const float *f = feat + (b * D + c) * S;
                out[(b * D + c) * N + n] = so3::three_interp(w0, w1, w2, f[i0], f[i1], f[i2]);
            } else {
                const float *f = feat + b * S * D + c;
                out[row * D + c] = so3::three_interp(w0, w1, w2, f[i0 * D], f[i1 * D], f[i2 * D]);
            }
        }
    }
}

// so3_three_interpolate_bwd_f32: every sum from 0 in ascending (n, k)
void model_three_interpolate_bwd(const float *grad_out, const int32_t *idx, const float *weight, float *grad_feat, int32_t channels_first, int64_t B,
                                 int32_t N, int32_t S, int32_t D) {
    for (int64_t e = 0; e < B * S * D; ++e) grad_feat[e] = 0.f;
    for (int64_t row = 0; row < B * N; ++row) {
        const int64_t b = row / N, n = row - b * N;
        for (int k = 0; k < 3; ++k) {
            const int64_t s = clamp_index(idx[row * 3 + k], S);
            const float w = weight[row * 3 + k];
            for (int64_t c = 0; c < D; ++c) {
                float &acc = channels_first ? grad_feat[(b * D + c) * S + s] : grad_feat[(b * S + s) * D + c];
                acc = so3::three_interp_bwd_add(w, channels_first ? grad_out[(b * D + c) * N + n] : grad_out[row * D + c], acc);
            }
        }
    }
}

// the waves per point k_three_nn's launcher picks
int32_t model_three_nn_waves_per_point(int64_t B, int32_t N, int32_t S) { return so3::three_nn_waves_per_point(B, N, S); }

}  // extern "C"
