// ransac.cpp -- the device functions of k_ransac_score and k_ransac_select (poseestimation_amd/csrc/so3_device.h: ransac_valid,
// ransac_admissible, ransac_pose, ransac_score_pair, ransac_better, ransac_inlier, ransac_rmse, ransac_identity) compiled for the host
// (SO3_HOST_MODEL) and driven by loops in the kernels' order: one hypothesis at a time, the cloud's pairs in ascending order, and the
// selection as one ascending scan (the order is total, so the device's tree gives the same winner).  tests/test_ransac_host.py checks
// the definitions against tests/ransac_ref.py without a GPU.  libm's 1 / sqrt stands in for v_rsq_f32 in the projection: the pose is
// not part of the bit contract.  TEST INFRASTRUCTURE ONLY.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <cmath>

#include "../../poseestimation_amd/csrc/so3_device.h"

namespace {

so3::V3<float> at(const float *p, int j) { return so3::mk<float>(p[j * 3], p[j * 3 + 1], p[j * 3 + 2]); }

}  // namespace

extern "C" {

int32_t model_ransac_tile() { return so3::kRansacTile; }
int32_t model_ransac_max_hypotheses() { return so3::kRansacMaxHypotheses; }

// so3_ransac_score_f32
int32_t model_ransac_score(const float *P, const float *Q, const int32_t *corr, const int32_t *x_len, const int32_t *y_len, const int32_t *samples,
                           float max_distance, float edge_similarity, float *T_hyp, int32_t *count, float *err, int64_t B, int32_t N, int32_t M,
                           int32_t H) {
    const float r2 = max_distance * max_distance;
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *src = P + b * N * 3, *tgt = Q + b * M * 3;
        const int32_t *cr = corr + b * N;
        for (int32_t h = 0; h < H; ++h) {
            const int32_t *tri = samples + (b * H + h) * 3;
            int32_t si[3], sc[3];
            so3::V3<float> p[3], q[3];
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                si[k] = tri[k];
                const int ic = so3::group_valid(si[k], N) ? si[k] : 0;
                sc[k] = cr[ic];
                const bool valid = so3::group_valid(si[k], N) && so3::ransac_valid(si[k], nb, sc[k], mb);
                const int jc = valid ? sc[k] : 0;
                p[k] = at(src, ic);
                q[k] = at(tgt, jc);
                ok = ok && valid;
            }
            const bool admissible = so3::ransac_admissible(ok, si, sc, p, q, edge_similarity);
            float T[12];
            so3::ransac_pose(admissible, p, q, T);
            int32_t cnt = 0;
            float e = 0.f;
            for (int i = 0; i < nb; ++i) {
                const int32_t c = cr[i];
                const bool valid = so3::ransac_valid(i, nb, c, mb);
                const int jc = valid ? c : 0;
                so3::ransac_score_pair(T, src[i * 3], src[i * 3 + 1], src[i * 3 + 2], valid ? tgt[jc * 3] : std::nanf(""), tgt[jc * 3 + 1],
                                       tgt[jc * 3 + 2], r2, cnt, e);
            }
            const int64_t o = b * H + h;
            for (int k = 0; k < 12; ++k) T_hyp[o * 12 + k] = T[k];
            count[o] = admissible ? cnt : -1;
            err[o] = admissible ? e : 0.f;
        }
    }
    return 0;
}

// so3_ransac_select_f32
int32_t model_ransac_select(const float *P, const float *Q, const int32_t *corr, const int32_t *x_len, const int32_t *y_len, const float *T_hyp,
                            const int32_t *count, const float *err, float max_distance, int32_t *best, float *T_best, int32_t *inliers, float *rmse,
                            float *weights, float *targets, int64_t B, int32_t N, int32_t M, int32_t H) {
    const float r2 = max_distance * max_distance;
    for (int64_t b = 0; b < B; ++b) {
        int32_t bc = -1, bh = -1;
        float be = 0.f;
        for (int32_t h = 0; h < H; ++h) {
            if (so3::ransac_better(count[b * H + h], err[b * H + h], h, bc, be, bh)) { bc = count[b * H + h]; be = err[b * H + h]; bh = h; }
        }
        const bool found = bh >= 0;
        float T[12];
        so3::ransac_identity(T);
        if (found) for (int k = 0; k < 12; ++k) T[k] = T_hyp[(b * H + bh) * 12 + k];
        best[b] = bh;
        inliers[b] = bc > 0 ? bc : 0;
        rmse[b] = so3::ransac_rmse(bc, be);
        for (int k = 0; k < 12; ++k) T_best[b * 12 + k] = T[k];
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *src = P + b * N * 3, *tgt = Q + b * M * 3;
        for (int i = 0; i < N; ++i) {
            const int32_t c = corr[b * N + i];
            const bool valid = so3::ransac_valid(i, nb, c, mb);
            const int jc = valid ? c : 0;
            float x, y, z, d2;
            const bool in = so3::ransac_inlier(T, src[i * 3], src[i * 3 + 1], src[i * 3 + 2], tgt[jc * 3], tgt[jc * 3 + 1], tgt[jc * 3 + 2], r2, x, y, z, d2) &&
                            valid && found;
            weights[b * N + i] = in ? 1.f : 0.f;
            const bool row = i < nb;
            targets[(b * N + i) * 3 + 0] = valid ? tgt[jc * 3 + 0] : (row ? x : 0.f);
            targets[(b * N + i) * 3 + 1] = valid ? tgt[jc * 3 + 1] : (row ? y : 0.f);
            targets[(b * N + i) * 3 + 2] = valid ? tgt[jc * 3 + 2] : (row ? z : 0.f);
        }
    }
    return 0;
}

}  // extern "C"
