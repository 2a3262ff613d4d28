// rigid_align.cpp -- the device functions of the rigid_align kernels (poseestimation_amd/csrc/so3_device.h: align_accumulate,
// align_finish, align_translation, align_rotation_grad, align_bwd_consts, align_bwd_dq / _dp / _dw, and the projection and its
// backward they feed) compiled for the host (SO3_HOST_MODEL) and driven by loops that keep the kernels' order of operations, so that
// tests/test_rigid_align_host.py measures the float32 arithmetic without a GPU.  TEST INFRASTRUCTURE ONLY.
// Differences from the device: libm's correctly rounded sqrt / division stand in for v_sqrt_f32 / v_rcp_f32 (1 ulp), and the build
// does not contract a * b + c.  A "wave" is 64 sets of accumulators filled lane-strided (point i on lane i % 64, in index order) and
// summed by the xor butterfly, as wave_allsum does (its DPP mirrors add the same partners' sums).
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include "../../poseestimation_amd/csrc/so3_device.h"
#include "wave_model.h"

namespace {

}  // namespace

extern "C" {

// k_rigid_align: w may be null (all ones).  R (B,9), t (B,3), H (B,9), stats (B,7).
void model_rigid_align(const float *P, const float *Q, const float *w, float *R, float *t, float *H, float *stats, int64_t B, int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        const float *pc = P + b * N * 3, *qc = Q + b * N * 3;
        float p0[3] = {0.f, 0.f, 0.f}, q0[3] = {0.f, 0.f, 0.f};
        if (N > 0) {
            for (int k = 0; k < 3; ++k) { p0[k] = pc[k]; q0[k] = qc[k]; }
        }
        static float acc[64][so3::kAlignSums];
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < so3::kAlignSums; ++i) acc[l][i] = 0.f;
        for (int i = 0; i < N; ++i)
            so3::align_accumulate(w != nullptr ? w[b * N + i] : 1.f, pc[i * 3] - p0[0], pc[i * 3 + 1] - p0[1], pc[i * 3 + 2] - p0[2],
                                  qc[i * 3] - q0[0], qc[i * 3 + 1] - q0[1], qc[i * 3 + 2] - q0[2], acc[i & 63]);
        float s[so3::kAlignSums];
        for (int i = 0; i < so3::kAlignSums; ++i) {
            float lane[64];
            for (int l = 0; l < 64; ++l) lane[l] = acc[l][i];
            s[i] = wave_allsum(lane);
        }
        float h[9], st[7], r[9], tt[3];
        so3::align_finish(s, p0, q0, h, st);
        so3::project_rotation<float>(h, r);
        so3::align_translation(r, st, tt);
        for (int i = 0; i < 9; ++i) { R[b * 9 + i] = r[i]; H[b * 9 + i] = h[i]; }
        for (int i = 0; i < 3; ++i) t[b * 3 + i] = tt[i];
        for (int i = 0; i < 7; ++i) stats[b * 7 + i] = st[i];
    }
}

// k_rigid_align_bwd: gR, gt, gH, w and each of dP, dQ, dw may be null.
void model_rigid_align_bwd(const float *P, const float *Q, const float *w, const float *H, const float *R, const float *stats,
                           const float *gR, const float *gt, const float *gH, float *dP, float *dQ, float *dw, int64_t B, int32_t N) {
    for (int64_t b = 0; b < B; ++b) {
        float st[7], r[9], g3[3], dh[9], k[so3::kAlignBwdConsts];
        for (int i = 0; i < 7; ++i) st[i] = stats[b * 7 + i];
        for (int i = 0; i < 9; ++i) { r[i] = R[b * 9 + i]; dh[i] = 0.f; }
        for (int i = 0; i < 3; ++i) g3[i] = gt != nullptr ? gt[b * 3 + i] : 0.f;
        if (gR != nullptr || gt != nullptr) {
            float h[9], g[9];
            for (int i = 0; i < 9; ++i) { h[i] = H[b * 9 + i]; g[i] = gR != nullptr ? gR[b * 9 + i] : 0.f; }
            so3::align_rotation_grad(g3, st, g);
            so3::project_backward_rows<float>(h, g, dh);
        }
        if (gH != nullptr) {
            for (int i = 0; i < 9; ++i) dh[i] += gH[b * 9 + i];
        }
        so3::align_bwd_consts(dh, r, g3, st, k);
        for (int i = 0; i < N; ++i) {
            const int64_t e = b * N + i;
            const float wi = w != nullptr ? w[e] : 1.f;
            const float ax = P[e * 3] - k[9], ay = P[e * 3 + 1] - k[10], az = P[e * 3 + 2] - k[11];
            const float cx = Q[e * 3] - k[12], cy = Q[e * 3 + 1] - k[13], cz = Q[e * 3 + 2] - k[14];
            if (dQ != nullptr) so3::align_bwd_dq(k, wi, ax, ay, az, dQ[e * 3], dQ[e * 3 + 1], dQ[e * 3 + 2]);
            if (dP != nullptr) so3::align_bwd_dp(k, wi, cx, cy, cz, dP[e * 3], dP[e * 3 + 1], dP[e * 3 + 2]);
            if (dw != nullptr) dw[e] = so3::align_bwd_dw(k, ax, ay, az, cx, cy, cz);
        }
    }
}

}  // extern "C"
