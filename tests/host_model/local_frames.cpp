// local_frames.cpp -- the device functions of k_local_frames (poseestimation_amd/csrc/so3_device.h: group_valid, chamfer_length,
// frames_sum_slot, frames_mean, frames_cov_slot, frames_cov_finish, sym_eigen3, frames_flat, frames_orient) compiled for the host (SO3_HOST_MODEL)
// and driven by loops in the kernel's order: one query at a time, two passes over its row, then the eigen stage, so that
// tests/test_local_frames_host.py checks the definition and measures the eigen stage's bounds without a GPU.  libm's sqrt and
// 1 / sqrt stand in for v_sqrt_f32 and v_rsq_f32.  TEST INFRASTRUCTURE ONLY.
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include "../../poseestimation_amd/csrc/so3_device.h"

namespace {

template <int SWEEPS>
void run(const float *Y, int64_t y_stride, const int32_t *idx, const int32_t *x_len, const int32_t *y_len, const float *viewpoint, float *cov,
         float *eigenvalues, float *normals, float *frames, int32_t K, int64_t B, int32_t N, int32_t M) {
    for (int64_t b = 0; b < B; ++b) {
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *tgt = Y + b * y_stride;
        for (int i = 0; i < N; ++i) {
            const int64_t q = b * N + i;
            const int32_t *row = idx + q * K;
            float C[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, lam[3] = {0.f, 0.f, 0.f}, F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int32_t r = 0;
            float px = 0.f, py = 0.f, pz = 0.f;
            if (i < nb && mb > 0) {
                float s[3] = {0.f, 0.f, 0.f};
                for (int k = 0; k < K; ++k) {
                    const int32_t j = row[k];
                    if (!so3::group_valid(j, mb)) continue;
                    if (r == 0) { px = tgt[j * 3]; py = tgt[j * 3 + 1]; pz = tgt[j * 3 + 2]; }
                    so3::frames_sum_slot(tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], px, py, pz, s);
                    ++r;
                }
                if (r > 0) {
                    float m[3], S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    so3::frames_mean(s, r, m);
                    for (int k = 0; k < K; ++k) {
                        const int32_t j = row[k];
                        if (so3::group_valid(j, mb)) so3::frames_cov_slot(tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], px, py, pz, m, S);
                    }
                    so3::frames_cov_finish(S, r, C);
                    so3::V3<float> e0, e1, e2;
                    so3::sym_eigen3<SWEEPS>(C, lam, e0, e1, e2);
                    const bool view = viewpoint != nullptr && !so3::frames_flat(C);
                    const float wx = view ? viewpoint[b * 3] - px : 0.f, wy = view ? viewpoint[b * 3 + 1] - py : 0.f,
                                wz = view ? viewpoint[b * 3 + 2] - pz : 0.f;
                    so3::frames_orient(e0, e1, e2, view, wx, wy, wz);
                    F[0] = e0.x; F[1] = e1.x; F[2] = e2.x;
                    F[3] = e0.y; F[4] = e1.y; F[5] = e2.y;
                    F[6] = e0.z; F[7] = e1.z; F[8] = e2.z;
                }
            }
            if (cov != nullptr) for (int a = 0; a < 6; ++a) cov[q * 6 + a] = C[a];
            if (eigenvalues != nullptr) for (int a = 0; a < 3; ++a) eigenvalues[q * 3 + a] = lam[a];
            if (normals != nullptr) for (int a = 0; a < 3; ++a) normals[q * 3 + a] = F[3 * a];
            if (frames != nullptr) for (int a = 0; a < 9; ++a) frames[q * 9 + a] = F[a];
        }
    }
}

}  // namespace

extern "C" {

int32_t model_local_frames_sweeps() { return so3::kFramesSweeps; }

// so3_local_frames_f32 with `sweeps` Jacobi sweeps (the shipped count, one fewer and one more); -1: a count that is not compiled
int32_t model_local_frames(const float *Y, int64_t y_stride, const int32_t *idx, const int32_t *x_len, const int32_t *y_len, const float *viewpoint,
                           float *cov, float *eigenvalues, float *normals, float *frames, int32_t K, int64_t B, int32_t N, int32_t M, int32_t sweeps) {
    if (sweeps == so3::kFramesSweeps) run<so3::kFramesSweeps>(Y, y_stride, idx, x_len, y_len, viewpoint, cov, eigenvalues, normals, frames, K, B, N, M);
    else if (sweeps == so3::kFramesSweeps - 1) run<so3::kFramesSweeps - 1>(Y, y_stride, idx, x_len, y_len, viewpoint, cov, eigenvalues, normals, frames, K, B, N, M);
    else if (sweeps == so3::kFramesSweeps + 1) run<so3::kFramesSweeps + 1>(Y, y_stride, idx, x_len, y_len, viewpoint, cov, eigenvalues, normals, frames, K, B, N, M);
    else return -1;
    return 0;
}

}  // extern "C"
