// knn_paths: how many queries should one wave of k_knn serve side by side (poseestimation_amd/csrc/so3proj.hip)?  The kernel below is
// a COPY of the library's skeleton (full lengths only: no ragged / padding path, no y_stride; to be kept in step by hand) on the
// library's arithmetic from so3_device.h (pointnet_dist2, knn_insert, knn_finish) with
// Q in {1, 2, 4, 8}: a wave loads a block of 64 candidates once and offers it to Q lists that live across its lanes; a work item is the
// four waves' 4 Q consecutive queries.  More Q: fewer candidate loads and block steps per query, fewer waves to fill the chip.
// Shapes: 32 x 1024 <- 1024 K = 16, 32 x 512 <- 128 K = 8, 8 x 4096 <- 4096 K = 20.  Prints the median of 20 launches per Q and checks
// that every Q wrote the same bits.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -fno-slp-vectorize -o tools/ubench/knn_paths tools/ubench/knn_paths.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../poseestimation_amd/csrc/so3_device.h"
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
constexpr int kBlock = 256, kMaxGrid = 8192;

__device__ __forceinline__ float lane_below(float v, float below0) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(below0), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int lane_below(int v, int below0) { return __builtin_amdgcn_update_dpp(below0, v, 0x138, 0xf, 0xf, false); }

template <int Q>
__global__ __launch_bounds__(kBlock) void knn(const float *__restrict__ X, const float *__restrict__ Y, float *__restrict__ dist2, int32_t *__restrict__ idx,
                                              int32_t K, int64_t B, int32_t N, int32_t M, int32_t chunks) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int first = (static_cast<int>(item - b * chunks) * (kBlock / 64) + wave) * Q;
        if (first >= N) continue;
        const float *src = X + b * N * 3, *tgt = Y + b * M * 3;
        float D[Q], qx[Q], qy[Q], qz[Q];
        int J[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            D[q] = __builtin_huge_valf(); J[q] = so3::kKnnNone;
            const int i = min(first + q, N - 1);
            qx[q] = src[i * 3 + 0]; qy[q] = src[i * 3 + 1]; qz[q] = src[i * 3 + 2];
        }
        int jn = min(lane, M - 1);
        float nx = tgt[jn * 3 + 0], ny = tgt[jn * 3 + 1], nz = tgt[jn * 3 + 2];
        for (int j0 = 0; j0 < M; j0 += 64) {
            const float cx = nx, cy = ny, cz = nz;
            jn = min(j0 + 64 + lane, M - 1);
            nx = tgt[jn * 3 + 0]; ny = tgt[jn * 3 + 1]; nz = tgt[jn * 3 + 2];
            const bool valid = j0 + lane < M;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float d = so3::pointnet_dist2(cx, cy, cz, qx[q], qy[q], qz[q]);
                const float tau = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(D[q]), K - 1));
                unsigned long long mask = __ballot(valid && d < tau);
                while (mask != 0) {
                    const int h = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const float dh = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), h));
                    so3::knn_insert(dh, j0 + h, D[q], J[q], lane_below(D[q], -__builtin_huge_valf()), lane_below(J[q], so3::kKnnNone));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = first + q;
            if (i >= N) break;
            so3::knn_finish(lane, min(K, M), M, D[q], J[q]);
            if (lane < K) { dist2[(b * N + i) * K + lane] = D[q]; idx[(b * N + i) * K + lane] = J[q]; }
        }
    }
}

template <int Q>
void launch(const float *x, const float *y, float *d, int32_t *i, int K, int B, int N, int M) {
    const int chunks = (N + 4 * Q - 1) / (4 * Q);
    hipLaunchKernelGGL(knn<Q>, dim3(static_cast<unsigned>(std::min<int64_t>(static_cast<int64_t>(B) * chunks, kMaxGrid))), dim3(kBlock), 0, 0, x, y, d, i, K,
                       static_cast<int64_t>(B), N, M, chunks);
}

int run(int B, int N, int M, int K) {
    std::vector<float> hx(static_cast<size_t>(B) * N * 3), hy(static_cast<size_t>(B) * M * 3);
    srand(7);
    for (auto &v : hx) v = rand() / static_cast<float>(RAND_MAX) - 0.5f;
    for (auto &v : hy) v = rand() / static_cast<float>(RAND_MAX) - 0.5f;
    float *x, *y, *d[4];
    int32_t *idx[4];
    CHECK(hipMalloc(&x, hx.size() * 4)); CHECK(hipMalloc(&y, hy.size() * 4));
    CHECK(hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); CHECK(hipMemcpy(y, hy.data(), hy.size() * 4, hipMemcpyHostToDevice));
    const size_t words = static_cast<size_t>(B) * N * K;
    for (int p = 0; p < 4; ++p) {
        CHECK(hipMalloc(&d[p], words * 4)); CHECK(hipMalloc(&idx[p], words * 4));
        CHECK(hipMemset(d[p], 0xFF, words * 4)); CHECK(hipMemset(idx[p], 0xFF, words * 4));
    }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int p = 0; p < 4; ++p) {
        std::vector<float> ms;
        for (int rep = 0; rep < 25; ++rep) {
            CHECK(hipEventRecord(e0));
            if (p == 0) launch<1>(x, y, d[p], idx[p], K, B, N, M);
            else if (p == 1) launch<2>(x, y, d[p], idx[p], K, B, N, M);
            else if (p == 2) launch<4>(x, y, d[p], idx[p], K, B, N, M);
            else launch<8>(x, y, d[p], idx[p], K, B, N, M);
            CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); CHECK(hipGetLastError());
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (rep >= 5) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        printf("%d x %d <- %d K=%d  Q=%d %8.2f us (median of 20; min %.2f)\n", B, N, M, K, 1 << p, 1e3f * ms[ms.size() / 2], 1e3f * ms[0]);
    }
    std::vector<int32_t> got[4][2];
    for (int p = 0; p < 4; ++p) {
        void *from[2] = {d[p], idx[p]};
        for (int q = 0; q < 2; ++q) { got[p][q].resize(words); CHECK(hipMemcpy(got[p][q].data(), from[q], words * 4, hipMemcpyDeviceToHost)); }
    }
    bool same = true;
    for (int p = 1; p < 4; ++p)
        for (int q = 0; q < 2; ++q) same = same && got[p][q] == got[0][q];
    printf("%d x %d <- %d K=%d  the same bits for every Q: %s\n", B, N, M, K, same ? "yes" : "NO");
    for (int p = 0; p < 4; ++p) { CHECK(hipFree(d[p])); CHECK(hipFree(idx[p])); }
    CHECK(hipFree(x)); CHECK(hipFree(y));
    return same ? 0 : 1;
}

int main() {
    int bad = run(32, 1024, 1024, 16);
    bad |= run(32, 512, 128, 8);
    bad |= run(8, 4096, 4096, 20);
    return bad;
}
