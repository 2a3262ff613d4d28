// ball_query_paths: how should k_ball_query (poseestimation_amd/csrc/so3proj.hip) read its cloud?  One wave per centre scans the cloud 64
// points per step in ascending j; both kernels below compute the library's rows with the library's arithmetic (so3_device.h).
//   l2  : every wave reads the points straight from global memory (12 B per lane; a cloud's 12 N bytes stay in L2); a wave leaves as
//         soon as its row is full
//   lds : a workgroup of four waves serves four centres of ONE cloud and stages the cloud through LDS in tiles of 1024 points, as
//         k_icp_step does; the waves share every tile, so the workgroup leaves only when all four rows are full
// Shape: the reference model's first level, 32 clouds x 1024 points, 512 centres (cloud points), r = 0.2 of the bounding-box diagonal,
// 64 samples.  Prints the median of 20 launches per path and checks that both wrote the same rows.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -o tools/ubench/ball_query_paths tools/ubench/ball_query_paths.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../poseestimation_amd/csrc/so3_device.h"
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)
constexpr int kBlock = 256, kUnroll = 4, kTile = 1024;

// One step of a wave's scan: the ballot of the members, their slots, the running count.
__device__ __forceinline__ void take(bool in, int j, int base, int width, int32_t *row, int &found, int &first) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(in);
    if (mask == 0) return;
    const int lane = threadIdx.x & 63;
    if (found == 0) first = base + __builtin_ctzll(mask);
    const int at = found + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
    if (in && at < width) row[at] = j;
    found += __builtin_popcountll(mask);
}

__global__ __launch_bounds__(kBlock) void ball_l2(const float *__restrict__ xyz, const float *__restrict__ centres, float radius, int width,
                                                  int32_t *__restrict__ idx, int B, int N, int S) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (item >= B * S) return;
    const float *src = xyz + static_cast<int64_t>(item / S) * N * 3;
    const float cx = centres[item * 3], cy = centres[item * 3 + 1], cz = centres[item * 3 + 2], r2 = so3::ball_radius2(radius);
    int32_t *row = idx + static_cast<int64_t>(item) * width;
    int found = 0, first = N;
    for (int j0 = 0; j0 < N && found < width; j0 += 64 * kUnroll) {
        float x[kUnroll], y[kUnroll], z[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const int j = min(j0 + 64 * k + lane, N - 1);
            x[k] = src[j * 3]; y[k] = src[j * 3 + 1]; z[k] = src[j * 3 + 2];
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const int j = j0 + 64 * k + lane;
            take(j < N && so3::ball_member(so3::pointnet_dist2(x[k], y[k], z[k], cx, cy, cz), r2), j, j0 + 64 * k, width, row, found, first);
        }
    }
    for (int k = min(found, width) + lane; k < width; k += 64) row[k] = first;
}

__global__ __launch_bounds__(kBlock) void ball_lds(const float *__restrict__ xyz, const float *__restrict__ centres, float radius, int width,
                                                   int32_t *__restrict__ idx, int B, int N, int S) {          // S % 4 == 0
    __shared__ float tile[3][kTile];
    const int tid = threadIdx.x, lane = tid & 63;
    const int item = blockIdx.x * (kBlock / 64) + (tid >> 6);
    const float *src = xyz + static_cast<int64_t>(item / S) * N * 3;
    const float cx = centres[item * 3], cy = centres[item * 3 + 1], cz = centres[item * 3 + 2], r2 = so3::ball_radius2(radius);
    int32_t *row = idx + static_cast<int64_t>(item) * width;
    int found = 0, first = N;
    for (int t0 = 0; t0 < N; t0 += kTile) {
        const int cnt = min(kTile, N - t0);
        if (__syncthreads_and(found >= width)) break;                      // also: the previous tile has been read
        for (int k = tid; k < cnt; k += kBlock) {
            tile[0][k] = src[(t0 + k) * 3]; tile[1][k] = src[(t0 + k) * 3 + 1]; tile[2][k] = src[(t0 + k) * 3 + 2];
        }
        __syncthreads();
        for (int k0 = 0; k0 < cnt && found < width; k0 += 64) {
            const int k = min(k0 + lane, cnt - 1);
            take(k0 + lane < cnt && so3::ball_member(so3::pointnet_dist2(tile[0][k], tile[1][k], tile[2][k], cx, cy, cz), r2), t0 + k0 + lane, t0 + k0,
                 width, row, found, first);
        }
    }
    for (int k = min(found, width) + lane; k < width; k += 64) row[k] = first;
}

int main() {
    const int B = 32, N = 1024, S = 512, K = 64;
    const float radius = 0.2f;
    std::vector<float> h(static_cast<size_t>(B) * N * 3), c(static_cast<size_t>(B) * S * 3);
    srand(7);
    for (auto &v : h) v = (rand() / static_cast<float>(RAND_MAX) - 0.5f) / 1.7320508f;      // a unit bounding-box diagonal, as pc_normalize
    for (int b = 0; b < B; ++b) std::copy(h.begin() + static_cast<size_t>(b) * N * 3, h.begin() + (static_cast<size_t>(b) * N + S) * 3, c.begin() + static_cast<size_t>(b) * S * 3);
    float *xyz, *cen;
    int32_t *out[2];
    CHECK(hipMalloc(&xyz, h.size() * 4)); CHECK(hipMalloc(&cen, c.size() * 4));
    CHECK(hipMemcpy(xyz, h.data(), h.size() * 4, hipMemcpyHostToDevice)); CHECK(hipMemcpy(cen, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    const size_t words = static_cast<size_t>(B) * S * K;
    for (auto &o : out) { CHECK(hipMalloc(&o, words * 4)); CHECK(hipMemset(o, 0xFF, words * 4)); }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const dim3 grid(B * S / (kBlock / 64)), block(kBlock);
    for (int path = 0; path < 2; ++path) {
        std::vector<float> ms;
        for (int rep = 0; rep < 25; ++rep) {
            CHECK(hipEventRecord(e0));
            if (path == 0) hipLaunchKernelGGL(ball_l2, grid, block, 0, 0, xyz, cen, radius, K, out[0], B, N, S);
            else hipLaunchKernelGGL(ball_lds, grid, block, 0, 0, xyz, cen, radius, K, out[1], B, N, S);
            CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); CHECK(hipGetLastError());
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (rep >= 5) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        printf("%-4s %8.2f us (median of 20; min %.2f)\n", path == 0 ? "l2" : "lds", 1e3f * ms[ms.size() / 2], 1e3f * ms[0]);
    }
    std::vector<int32_t> a(words), b(words);
    CHECK(hipMemcpy(a.data(), out[0], words * 4, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(b.data(), out[1], words * 4, hipMemcpyDeviceToHost));
    size_t full = 0;
    for (size_t r = 0; r < words; r += K) full += a[r + K - 1] != a[r] || K == 1;
    printf("rows equal: %s; rows with >= %d points: %.1f %%\n", a == b ? "yes" : "NO", K, 100.0 * full / (words / K));
    return a == b ? 0 : 1;
}
