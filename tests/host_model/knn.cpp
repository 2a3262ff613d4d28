// knn.cpp -- the device functions of the K-nearest-neighbour kernels (poseestimation_amd/csrc/so3_device.h: pointnet_dist2, knn_insert,
// knn_finish, chamfer_length, chamfer_phi, chamfer_hit, knn_queries_per_wave) compiled for the host (SO3_HOST_MODEL) and driven by loops
// that keep k_knn's order of operations, so that tests/test_knn_host.py checks the definition without a GPU.  model_knn_bwd is a second
// restatement of the definition's order through chamfer_phi / chamfer_hit (every target's entries in ascending (i, k)), NOT a simulation
// of k_knn_bwd's owner scan with its ballot walk and clamped loads; in the forward, Q only changes how queries are dealt to waves.
// TEST INFRASTRUCTURE ONLY.  The build switches contraction off, as the header does for pointnet_dist2 on the device.
// A wave is 64 array slots: lane k holds entry k of a query's sorted list.  One block of 64 candidates is tested against tau = entry
// K - 1 as a whole (the ballot), then the hits are inserted in ascending j; an insertion reads every lane's entry and the entry of the
// lane below (lane 0: -inf) before any lane is written, as the DPP move does.  A work item is the four waves' 4 Q consecutive queries.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <algorithm>
#include <limits>

#include "../../poseestimation_amd/csrc/so3_device.h"

extern "C" {

int32_t model_knn_queries_per_wave(int64_t B, int32_t N, int32_t M) { return so3::knn_queries_per_wave(B, N, M); }

// so3_knn_f32 with Q queries per wave (dist2 optional)
void model_knn(const float *X, const float *Y, int64_t y_stride, const int32_t *x_len, const int32_t *y_len, float *dist2, int32_t *idx, int32_t K,
               int64_t B, int32_t N, int32_t M, int32_t Q) {
    const float inf = std::numeric_limits<float>::infinity();
    const int per = 4 * Q, chunks = (N + per - 1) / per;
    for (int64_t item = 0; item < B * chunks; ++item) {
        const int64_t b = item / chunks;
        for (int wave = 0; wave < 4; ++wave) {
            const int first = (static_cast<int>(item - b * chunks) * 4 + wave) * Q;
            if (first >= N) continue;
            const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
            const float *src = X + b * N * 3, *tgt = Y + b * y_stride;
            const bool live = mb > 0 && first < nb;
            for (int q = 0; q < Q && first + q < N; ++q) {
                float D[64];
                int J[64];
                for (int l = 0; l < 64; ++l) { D[l] = inf; J[l] = so3::kKnnNone; }
                const int i = first + q;
                if (live) {
                    const int ic = std::min(i, nb - 1);
                    for (int j0 = 0; j0 < mb; j0 += 64) {
                        float d[64];
                        bool hit[64];
                        const float tau = D[K - 1];
                        for (int l = 0; l < 64; ++l) {
                            const int j = std::min(j0 + l, mb - 1);
                            d[l] = so3::pointnet_dist2(tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], src[ic * 3], src[ic * 3 + 1], src[ic * 3 + 2]);
                            hit[l] = j0 + l < mb && d[l] < tau;
                        }
                        for (int h = 0; h < 64; ++h) {
                            if (!hit[h]) continue;
                            float pD[64];
                            int pJ[64];
                            pD[0] = -inf; pJ[0] = so3::kKnnNone;
                            for (int l = 1; l < 64; ++l) { pD[l] = D[l - 1]; pJ[l] = J[l - 1]; }
                            for (int l = 0; l < 64; ++l) so3::knn_insert(d[h], j0 + h, D[l], J[l], pD[l], pJ[l]);
                        }
                    }
                }
                const int32_t r = live && i < nb ? std::min(K, mb) : 0;
                for (int l = 0; l < K; ++l) {
                    so3::knn_finish(l, r, mb, D[l], J[l]);
                    const int64_t at = (b * N + i) * K + l;
                    if (dist2 != nullptr) dist2[at] = D[l];
                    idx[at] = J[l];
                }
            }
        }
    }
}

// so3_knn_bwd_f32 (dX, dY each optional)
void model_knn_bwd(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, const int32_t *idx, const float *grad, float *dX,
                   float *dY, int32_t K, int64_t B, int32_t N, int32_t M) {
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *xs = X + b * N * 3, *ys = Y + b * M * 3;
        const int32_t *rows = idx + b * N * K;
        const float *gs = grad + b * N * K;
        const bool live = nb > 0 && mb > 0;
        const int32_t r = std::min(K, mb);
        if (dX != nullptr) {
            for (int i = 0; i < N; ++i) {
                float acc[3] = {0.f, 0.f, 0.f};
                if (live && i < nb) {
                    for (int k = 0; k < r; ++k) {
                        const int jr = rows[static_cast<int64_t>(i) * K + k];
                        if (jr < 0) continue;
                        const int j = std::min(jr, mb - 1);
                        float ux, uy, uz;
                        so3::chamfer_phi<true>(xs[i * 3] - ys[j * 3], xs[i * 3 + 1] - ys[j * 3 + 1], xs[i * 3 + 2] - ys[j * 3 + 2], ux, uy, uz);
                        so3::chamfer_hit(gs[static_cast<int64_t>(i) * K + k], ux, uy, uz, acc);
                    }
                }
                for (int c = 0; c < 3; ++c) dX[(b * N + i) * 3 + c] = acc[c];
            }
        }
        if (dY != nullptr) {
            float *out = dY + b * M * 3;
            for (int64_t e = 0; e < static_cast<int64_t>(M) * 3; ++e) out[e] = 0.f;
            if (!live) continue;
            for (int64_t e = 0; e < static_cast<int64_t>(nb) * K; ++e) {            // ascending (i, k): every owner's hits in its order
                const int32_t j = rows[e];
                if (static_cast<uint32_t>(j) >= static_cast<uint32_t>(mb)) continue;
                const int i = static_cast<int>(e / K);
                float ux, uy, uz, acc[3] = {out[j * 3], out[j * 3 + 1], out[j * 3 + 2]};
                so3::chamfer_phi<true>(ys[j * 3] - xs[i * 3], ys[j * 3 + 1] - xs[i * 3 + 1], ys[j * 3 + 2] - xs[i * 3 + 2], ux, uy, uz);
                so3::chamfer_hit(gs[e], ux, uy, uz, acc);
                for (int c = 0; c < 3; ++c) out[j * 3 + c] = acc[c];
            }
        }
    }
}

}  // extern "C"
