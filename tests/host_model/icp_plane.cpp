// icp_plane.cpp -- the device functions of the point-to-plane ICP kernels (poseestimation_amd/csrc/so3_device.h: pose_point, add_s_pair,
// plane_accumulate, plane_solve, plane_retraction, plane_finish and what they call) compiled for the host (SO3_HOST_MODEL) and driven by
// loops that keep the kernels' order of operations, so that tests/test_icp_plane_host.py measures the float32 arithmetic without a GPU.
// TEST INFRASTRUCTURE ONLY.  Differences from the device and the layout of a work item: as tests/host_model/icp.cpp.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <limits>
#include <vector>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "wave_model.h"

namespace {

// the posed point and its search: the target in index order (tiles and their padding change neither the order nor the result)
void search(const float *pose, const float *p, const float *tgt, int32_t M, float (&x)[3], float &best, int &idx) {
    x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
    if (pose != nullptr) {
        float m[12];
        for (int k = 0; k < 12; ++k) m[k] = pose[k];
        so3::pose_point(m, p[0], p[1], p[2], x[0], x[1], x[2]);
    }
    best = std::numeric_limits<float>::infinity();
    idx = 0;
    for (int j = 0; j < M; ++j) so3::add_s_pair<true, false>(x[0], x[1], x[2], tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], j, best, idx);
    idx = std::min(idx, M - 1);
}

// k_icp_plane_step<.., U> over one cloud: records (chunks, kPlaneRecord)
template <bool TRIMMED>
void step(const float *src, const float *tgt, const float *nrm, const float *w, const float *pose, float max_distance, float *rec, float *dist,
          int32_t *nearest, int32_t N, int32_t M, int u) {
    const int per = so3::kIcpBlock * u, chunks = (N + per - 1) / per;
    float c[3], best0;
    int j0;
    search(pose, src, tgt, 1, c, best0, j0);                     // the pivot: the posed first source point
    for (int ch = 0; ch < chunks; ++ch) {
        static float acc[so3::kIcpBlock][so3::kPlaneSums];
        for (int t = 0; t < so3::kIcpBlock; ++t)
            for (int k = 0; k < so3::kPlaneSums; ++k) acc[t][k] = 0.f;
        for (int uu = 0; uu < u; ++uu) {
            for (int t = 0; t < so3::kIcpBlock; ++t) {
                const int i = ch * per + uu * so3::kIcpBlock + t;
                const bool in = i < N;
                const int ic = std::min(i, N - 1);
                float x[3], best;
                int j;
                search(pose, src + ic * 3, tgt, M, x, best, j);
                const float d = so3::hw::sqrt(best);
                if (in) {
                    if (dist != nullptr) dist[i] = d;
                    if (nearest != nullptr) nearest[i] = j;
                }
                const float wi = in ? (w != nullptr ? w[ic] : 1.f) : 0.f;
                so3::plane_accumulate<TRIMMED>(wi, best, d, max_distance, x[0] - c[0], x[1] - c[1], x[2] - c[2], x[0] - tgt[j * 3], x[1] - tgt[j * 3 + 1],
                                               x[2] - tgt[j * 3 + 2], nrm[j * 3], nrm[j * 3 + 1], nrm[j * 3 + 2], acc[t]);
            }
        }
        for (int k = 0; k < so3::kPlaneRecord; ++k) {
            float v = 0.f;
            if (k < so3::kPlaneSums) {
                for (int wv = 0; wv < so3::kIcpBlock / 64; ++wv) {
                    float lane[64];
                    for (int l = 0; l < 64; ++l) lane[l] = acc[wv * 64 + l][k];
                    const float tot = wave_allsum(lane);
                    v = wv == 0 ? tot : v + tot;
                }
            }
            rec[ch * so3::kPlaneRecord + k] = v;
        }
    }
}

}  // namespace

extern "C" {

float model_plane_pivot_eps() { return so3::kPlanePivotEps; }

// plane_solve on a full row-major 6x6 (its upper triangle is read) with the diagonal scaled by (1 + damping), as plane_finish does:
// returns whether it was solved; delta (6) and ratio (1) out
int model_plane_solve(const float *A, const float *g, float damping, float *delta, float *ratio) {
    float a[21], gg[6], d[6];
    const float lm = 1.f + damping;
    for (int k = 0; k < 6; ++k) {
        for (int l = k; l < 6; ++l) a[so3::plane_tri(k, l)] = k == l ? A[k * 6 + l] * lm : A[k * 6 + l];
        gg[k] = g[k];
    }
    const bool ok = so3::plane_solve(a, gg, damping > 0.f, d, *ratio);
    for (int k = 0; k < 6; ++k) delta[k] = d[k];
    return ok ? 1 : 0;
}

void model_plane_retraction(const float *omega, float *dr) {
    float r[9];
    so3::plane_retraction(omega[0], omega[1], omega[2], r);
    for (int k = 0; k < 9; ++k) dr[k] = r[k];
}

// so3_icp_plane_f32 on a device of `cus` compute units (iterations >= 0; the outputs as the C ABI's, each optional but R and t);
// ratio: optional iterations*B, plane_solve's smallest pivot ratio of each step
void model_icp_plane(const float *P, const float *Q, const float *Nrm, int64_t q_stride, const float *w, const float *T_init, float max_distance,
                     float damping, int32_t iterations, float *R, float *t, float *rmse, float *rmse_point, int32_t *inliers, int32_t *solved,
                     int32_t *nearest, float *dist, float *ratio, int64_t B, int32_t N, int32_t M, int64_t cus) {
    const int u = so3::icp_points_per_lane(B, N, cus);
    const int per = so3::kIcpBlock * u, chunks = (N + per - 1) / per;
    std::vector<float> rec(static_cast<size_t>(chunks) * so3::kPlaneRecord);
    for (int64_t b = 0; b < B; ++b) {
        const float *src = P + b * N * 3, *tgt = Q + b * q_stride, *nrm = Nrm + b * q_stride, *wb = w != nullptr ? w + b * N : nullptr;
        float cur[12], next[12];
        bool have = T_init != nullptr;
        for (int k = 0; k < 12; ++k) cur[k] = have ? T_init[b * 12 + k] : ((k % 5) == 0 ? 1.f : 0.f);
        if (iterations == 0 && (dist != nullptr || nearest != nullptr)) {
            for (int i = 0; i < N; ++i) {
                float x[3], best;
                int j;
                search(have ? cur : nullptr, src + i * 3, tgt, M, x, best, j);
                if (dist != nullptr) dist[b * N + i] = so3::hw::sqrt(best);
                if (nearest != nullptr) nearest[b * N + i] = j;
            }
        }
        for (int32_t it = 0; it < iterations; ++it) {
            const bool last = it + 1 == iterations;
            float *dd = last && dist != nullptr ? dist + b * N : nullptr;
            int32_t *nn = last && nearest != nullptr ? nearest + b * N : nullptr;
            if (max_distance >= 0.f) step<true>(src, tgt, nrm, wb, have ? cur : nullptr, max_distance, rec.data(), dd, nn, N, M, u);
            else step<false>(src, tgt, nrm, wb, have ? cur : nullptr, max_distance, rec.data(), dd, nn, N, M, u);
            float s[so3::kPlaneSums];
            for (int k = 0; k < so3::kPlaneSums; ++k) {
                float v = 0.f;
                for (int c = 0; c < chunks; ++c) v += rec[c * so3::kPlaneRecord + k];
                s[k] = v;
            }
            float c[3] = {src[0], src[1], src[2]}, e, ep, cnt;
            if (have) so3::pose_point(cur, src[0], src[1], src[2], c[0], c[1], c[2]);
            bool ok;
            so3::plane_finish(s, c, cur, damping, next, e, ep, cnt, ok);
            if (ratio != nullptr) {
                float A[36], dl[6], rt;
                for (int k = 0; k < 6; ++k)
                    for (int l = k; l < 6; ++l) A[k * 6 + l] = s[1 + so3::plane_tri(k, l)];
                model_plane_solve(A, s + 22, damping, dl, &rt);
                ratio[it * B + b] = rt;
            }
            for (int k = 0; k < 12; ++k) cur[k] = next[k];
            have = true;
            if (rmse != nullptr) rmse[it * B + b] = e;
            if (rmse_point != nullptr) rmse_point[it * B + b] = ep;
            if (inliers != nullptr) inliers[it * B + b] = static_cast<int32_t>(cnt);
            if (solved != nullptr) solved[it * B + b] = ok ? 1 : 0;
        }
        for (int c = 0; c < 3; ++c) {
            for (int k = 0; k < 3; ++k) R[b * 9 + 3 * c + k] = cur[4 * c + k];
            t[b * 3 + c] = cur[4 * c + 3];
        }
    }
}

}  // extern "C"

#ifdef SO3_ICP_PLANE_MAIN
// A stand-alone run for -fsanitize=address,undefined (tests/test_icp_plane_host.py): one ragged-edge case -- N one past a chunk, M one
// past a tile, a shared target, weights, trimming, an initial pose -- in heap buffers of exactly the sizes the C ABI documents.
#include <stdio.h>
int main() {
    const int64_t B = 2;
    const int32_t N = 257, M = 1025, iterations = 2;
    std::vector<float> P(B * N * 3), Q(M * 3), Nrm(M * 3), w(B * N), T0(B * 12), R(B * 9), t(B * 3), rmse(iterations * B), rmse_point(iterations * B),
        dist(B * N), ratio(iterations * B);
    std::vector<int32_t> inliers(iterations * B), solved(iterations * B), nearest(B * N);
    uint32_t state = 30;
    auto next = [&state] { state = state * 1664525u + 1013904223u; return static_cast<float>(state >> 8) * (1.0f / 16777216.0f) - 0.5f; };
    for (int j = 0; j < M; ++j) {
        float v[3] = {next(), next(), next()};
        const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-6f;
        for (int k = 0; k < 3; ++k) { Nrm[j * 3 + k] = j % 5 == 4 ? 0.f : v[k] / len; Q[j * 3 + k] = v[k] / len * (k == 0 ? 1.0f : k == 1 ? 0.7f : 0.5f); }
    }
    for (int64_t i = 0; i < B * N; ++i) {
        const int j = static_cast<int>((i * 7) % M);
        for (int k = 0; k < 3; ++k) P[i * 3 + k] = Q[j * 3 + k] + 0.01f * next();
        w[i] = i % 3 == 0 ? 0.f : 1.f;
    }
    for (int64_t b = 0; b < B; ++b)
        for (int k = 0; k < 12; ++k) T0[b * 12 + k] = (k % 5) == 0 ? 1.f : (k % 4) == 3 ? 0.01f : 0.f;
    for (int64_t cus : {256, 1, 0})
        model_icp_plane(P.data(), Q.data(), Nrm.data(), 0, w.data(), T0.data(), 0.05f, 0.0f, iterations, R.data(), t.data(), rmse.data(), rmse_point.data(),
                        inliers.data(), solved.data(), nearest.data(), dist.data(), ratio.data(), B, N, M, cus);
    model_icp_plane(P.data(), Q.data(), Nrm.data(), 0, nullptr, nullptr, -1.0f, 0.5f, 0, R.data(), t.data(), nullptr, nullptr, nullptr, nullptr,
                    nearest.data(), dist.data(), nullptr, B, N, M, 256);
    printf("SANITIZE OK inliers %d solved %d rmse %.3e\n", inliers[0], solved[0], rmse[0]);
    return 0;
}
#endif
