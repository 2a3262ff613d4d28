// fpfh.cpp -- the device functions of k_spfh and k_fpfh (poseestimation_amd/csrc/so3_device.h: group_valid, chamfer_length, fpfh_pair,
// fpfh_bin, spfh_value, fpfh_slot, fpfh_finish) compiled for the host (SO3_HOST_MODEL) and driven by loops in the kernels' order: one
// query at a time, its row's slots in ascending order, so that tests/test_fpfh_host.py checks the counts and the definition without a
// GPU.  The ballots become a plain histogram (the counts are integers: the order of counting does not matter).  libm's 1 / sqrt
// stands in for v_rsq_f32.  TEST INFRASTRUCTURE ONLY.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include "../../poseestimation_amd/csrc/so3_device.h"

namespace {

so3::V3<float> at(const float *p, int j) { return so3::mk<float>(p[j * 3], p[j * 3 + 1], p[j * 3 + 2]); }

}  // namespace

extern "C" {

int32_t model_fpfh_slots() { return so3::kFpfhSlots; }

// so3_spfh_f32; g (B*N*K*3 float32, optional) receives every slot's g1, g2, g3 and pair (B*N*K uint8, optional) whether it is a pair.
int32_t model_spfh(const float *X, const float *normals, const int32_t *idx, const int32_t *len, float *spfh, int32_t *pairs, float *g, uint8_t *pair,
                   int32_t K, int64_t B, int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(len, b, N);
        const float *pts = X + b * N * 3, *nrm = normals + b * N * 3;
        for (int i = 0; i < N; ++i) {
            const int64_t q = b * N + i;
            int32_t hist[so3::kFpfhSlots] = {0}, r = 0;
            for (int k = 0; k < K; ++k) {
                const int32_t j = idx[q * K + k];
                const bool slot = i < nb && so3::group_valid(j, nb) && j != i;
                const int jc = slot ? j : 0;
                float g1, g2, g3;
                const bool is_pair = so3::fpfh_pair(slot, at(pts, i), at(nrm, i), at(pts, jc), at(nrm, jc), g1, g2, g3);
                if (g != nullptr) { g[(q * K + k) * 3] = g1; g[(q * K + k) * 3 + 1] = g2; g[(q * K + k) * 3 + 2] = g3; }
                if (pair != nullptr) pair[q * K + k] = is_pair ? 1 : 0;
                if (!is_pair) continue;
                ++r;
                ++hist[so3::fpfh_bin(g1)];
                ++hist[so3::kFpfhBins + so3::fpfh_bin(g2)];
                ++hist[2 * so3::kFpfhBins + so3::fpfh_bin(g3)];
            }
            if (spfh != nullptr) for (int s = 0; s < so3::kFpfhSlots; ++s) spfh[q * so3::kFpfhSlots + s] = so3::spfh_value(hist[s], r);
            if (pairs != nullptr) pairs[q] = r;
        }
    }
    return 0;
}

// so3_fpfh_f32
int32_t model_fpfh(const float *X, const int32_t *idx, const int32_t *len, const float *spfh, const int32_t *pairs, float *fpfh, int32_t K, int64_t B,
                   int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(len, b, N);
        const float *pts = X + b * N * 3, *hist = spfh + b * N * so3::kFpfhSlots;
        const int32_t *cnt = pairs + b * N;
        for (int i = 0; i < N; ++i) {
            const int32_t *row = idx + (b * N + i) * K;
            for (int s = 0; s < so3::kFpfhSlots; ++s) {
                float out = 0.f;
                if (i < nb) {
                    float W = 0.f, A = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const int32_t j = row[k];
                        const bool slot = so3::group_valid(j, nb) && j != i;
                        const int jc = slot ? j : 0;
                        so3::fpfh_slot(slot, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], pts[jc * 3], pts[jc * 3 + 1], pts[jc * 3 + 2], cnt[jc],
                                       hist[jc * so3::kFpfhSlots + s], W, A);
                    }
                    out = so3::fpfh_finish(hist[i * so3::kFpfhSlots + s], W, A);
                }
                fpfh[(b * N + i) * so3::kFpfhSlots + s] = out;
            }
        }
    }
    return 0;
}

}  // extern "C"
