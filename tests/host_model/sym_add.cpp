// sym_add.cpp -- the device functions of k_sym_add (poseestimation_amd/csrc/so3_device.h: sym_add_difference, sym_add_residual,
// sym_add_term, sym_add_join, sym_add_finish, sym_add_direction, sym_add_rotate_back) compiled for the host (SO3_HOST_MODEL) and driven
// by loops that keep the kernel's order of operations, so that tests/test_sym_add_host.py measures the float32 arithmetic of
// so3_sym_add_f32 without a GPU.  TEST INFRASTRUCTURE ONLY.
// Differences from the device: libm's correctly rounded sqrt / division stand in for v_sqrt_f32 / v_rcp_f32 (1 ulp), and the build
// does not contract a * b + c.  A "wave" is 64 float accumulators filled lane-strided and joined by the xor butterfly, as
// sym_add_wave_join does (its DPP mirrors join the same partners' results).
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include <limits>

#include "../../poseestimation_amd/csrc/so3_device.h"

namespace {

template <int MODE> float wave_join(const float (&lane)[64]) {
    float v[64], w[64];
    for (int l = 0; l < 64; ++l) v[l] = lane[l];
    for (int off = 1; off < 64; off <<= 1) {
        for (int l = 0; l < 64; ++l) w[l] = so3::sym_add_join<MODE>(v[l], v[l ^ off]);
        for (int l = 0; l < 64; ++l) v[l] = w[l];
    }
    return v[0];
}

template <int MODE>
void sym_add(const float *Tgt, const float *Tpred, const float *pts, const float *S, const int32_t *class_id, int32_t C, int32_t K,
             float *dists, int32_t *index, float *all, float *dT, float grad_scale, int64_t B, int32_t N) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t b = 0; b < B; ++b) {
        const float *cloud = pts + b * N * 3, *tg = Tgt + b * 16, *tp = Tpred + b * 16;
        float rg[9], rp[9], dt[3];
        for (int c = 0; c < 3; ++c) {
            for (int j = 0; j < 3; ++j) { rg[3 * c + j] = tg[4 * c + j]; rp[3 * c + j] = tp[4 * c + j]; }
            dt[c] = tg[4 * c + 3] - tp[4 * c + 3];
        }
        const int cls = class_id != nullptr ? class_id[b] : 0;
        const bool bad = static_cast<unsigned>(cls) >= static_cast<unsigned>(C);
        const float *tab = S + static_cast<int64_t>(bad ? 0 : cls) * K * 9;
        float best = 0.f;
        int kb = 0;
        for (int k = 0; k < K; ++k) {
            float s[9], d[9];
            for (int i = 0; i < 9; ++i) s[i] = tab[k * 9 + i];
            so3::sym_add_difference(rg, rp, s, k, d);
            float stat = 0.f;
            for (int i0 = 0; i0 < N; i0 += so3::kSymAddSweep) {                      // a sweep: per lane in index order, then the butterfly
                float part[64] = {};
                for (int i = i0; i < std::min(N, i0 + so3::kSymAddSweep); ++i) {
                    float dx, dy, dz;
                    so3::sym_add_residual(d, dt, cloud[i * 3], cloud[i * 3 + 1], cloud[i * 3 + 2], dx, dy, dz);
                    part[i & 63] = so3::sym_add_join<MODE>(part[i & 63], so3::sym_add_term<MODE>(dx, dy, dz));
                }
                stat = so3::sym_add_join<MODE>(stat, wave_join<MODE>(part));
            }
            const float val = so3::sym_add_finish<MODE>(stat, N);
            if (all != nullptr) all[b * K + k] = val;
            if (k == 0 || val < best) { best = val; kb = k; }                       // strict <, ascending k
        }
        if (dists != nullptr) dists[b] = bad ? nan : best;
        if (index != nullptr) index[b] = bad ? -1 : kb;
        if (dT == nullptr) continue;
        float s[9], d[9];
        for (int i = 0; i < 9; ++i) s[i] = tab[kb * 9 + i];
        so3::sym_add_difference(rg, rp, s, kb, d);
        float acc[12][64] = {};
        for (int i = 0; i < N; ++i) {
            const int lane = i & 63;
            const float px = cloud[i * 3], py = cloud[i * 3 + 1], pz = cloud[i * 3 + 2];
            float dx, dy, dz, u[3];
            so3::sym_add_residual(d, dt, px, py, pz, dx, dy, dz);
            so3::sym_add_direction<MODE>(dx, dy, dz, u[0], u[1], u[2]);
            for (int c = 0; c < 3; ++c) {
                acc[3 * c + 0][lane] = std::fma(u[c], px, acc[3 * c + 0][lane]);
                acc[3 * c + 1][lane] = std::fma(u[c], py, acc[3 * c + 1][lane]);
                acc[3 * c + 2][lane] = std::fma(u[c], pz, acc[3 * c + 2][lane]);
                acc[9 + c][lane] += u[c];
            }
        }
        float g[9], gs[9], gt[3];
        for (int i = 0; i < 9; ++i) g[i] = wave_join<so3::kSymAddL2>(acc[i]);
        for (int c = 0; c < 3; ++c) gt[c] = wave_join<so3::kSymAddL2>(acc[9 + c]);
        so3::sym_add_rotate_back(g, s, kb, gs);
        const float c = bad ? nan : -grad_scale * (MODE == so3::kSymAddL1 ? 1.0f / (3.0f * static_cast<float>(N)) : 1.0f / static_cast<float>(N));
        for (int r = 0; r < 3; ++r) {
            for (int j = 0; j < 3; ++j) dT[b * 16 + 4 * r + j] = c * gs[3 * r + j];
            dT[b * 16 + 4 * r + 3] = c * gt[r];
        }
        for (int e = 12; e < 16; ++e) dT[b * 16 + e] = 0.f;
    }
}

}  // namespace

extern "C" {

// so3_sym_add_f32's arguments without loss_sum and the stream; `all` (optional, B*K): every candidate's statistic.  mode: SO3_SYM_ADD_*.
// Returns 0, or -1 for dT with the maximum or an unknown mode.
int model_sym_add(const float *Tgt, const float *Tpred, const float *pts, const float *S, const int32_t *class_id, int32_t C, int32_t K,
                  float *dists, int32_t *index, float *all, float *dT, float grad_scale, unsigned mode, int64_t B, int32_t N) {
    if (mode == 0) sym_add<so3::kSymAddL2>(Tgt, Tpred, pts, S, class_id, C, K, dists, index, all, dT, grad_scale, B, N);
    else if (mode == 1) sym_add<so3::kSymAddL1>(Tgt, Tpred, pts, S, class_id, C, K, dists, index, all, dT, grad_scale, B, N);
    else if (mode == 2 && dT == nullptr) sym_add<so3::kSymAddMax>(Tgt, Tpred, pts, S, class_id, C, K, dists, index, all, nullptr, grad_scale, B, N);
    else return -1;
    return 0;
}

}  // extern "C"
