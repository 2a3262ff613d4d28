// so3proj.hip -- C ABI of libso3proj.so (gfx950 only) and the small-batch kernels.  See include/so3proj.h.
//
// Large, 16-byte-aligned batches run on the row-streaming engine of so3_rows.h (persistent waves, packed
// two-matrices-per-lane arithmetic, branch-free buffer I/O).  What is left -- a remainder of < 64 rows,
// pointers that are not 16-byte aligned, and the Kabsch kernel -- lives here: 256-thread workgroups own a
// contiguous tile of 256 rows (9216 B), move it with coalesced accesses through LDS, and each lane picks its
// nine floats out of LDS at a 9-dword stride (odd stride -> conflict-free ds_read_b32 / ds_write_b32).
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <algorithm>
#include <atomic>
#include <stdlib.h>
#include <string>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>

#include "../../include/so3proj.h"
#include "so3_device.h"
#include "so3_dispatch.h"
#include "so3_rows.h"

namespace {



constexpr int kBlock = 256;                 // lanes (= 3x3 blocks) per workgroup tile
constexpr int kTileFloats = kBlock * 9;     // 2304 floats = 9216 B
constexpr int kTileVec4 = kTileFloats / 4;  // 576 float4

thread_local char g_err[256] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, code == SO3_ERR_INVALID ? "invalid argument" : hipGetErrorString((hipError_t)code));
    return code;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail((int)e, what);
}

__host__ __device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- tile movers ----------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(uint16_t b) { return __uint_as_float(static_cast<uint32_t>(b) << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const __bf16 h = static_cast<__bf16>(f);   // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}

// Global (f32) -> LDS tile.  `n` = valid blocks in this tile (<= 256).  VEC: 16-byte path allowed.
template <bool VEC>
__device__ __forceinline__ void tile_in_f32(const float *__restrict__ g, int n, float *tile) {
    const int tid = threadIdx.x;
    if (VEC && n == kBlock) {
        const float4 *src = reinterpret_cast<const float4 *>(g);
        float4 *dst = reinterpret_cast<float4 *>(tile);
        const float4 a = src[tid], b = src[tid + kBlock];
        float4 c;
        if (tid < kTileVec4 - 2 * kBlock) c = src[tid + 2 * kBlock];
        dst[tid] = a;
        dst[tid + kBlock] = b;
        if (tid < kTileVec4 - 2 * kBlock) dst[tid + 2 * kBlock] = c;
    } else {
        for (int i = tid; i < n * 9; i += kBlock) tile[i] = g[i];
    }
}

template <bool VEC>
__device__ __forceinline__ void tile_out_f32(float *__restrict__ g, int n, const float *tile) {
    const int tid = threadIdx.x;
    if (VEC && n == kBlock) {
        float4 *dst = reinterpret_cast<float4 *>(g);
        const float4 *src = reinterpret_cast<const float4 *>(tile);
        dst[tid] = src[tid];
        dst[tid + kBlock] = src[tid + kBlock];
        if (tid < kTileVec4 - 2 * kBlock) dst[tid + 2 * kBlock] = src[tid + 2 * kBlock];
    } else {
        for (int i = tid; i < n * 9; i += kBlock) g[i] = tile[i];
    }
}

// bf16 in global <-> f32 in the LDS tile (conversion on the way through).
__device__ __forceinline__ void tile_in_bf16(const uint16_t *__restrict__ g, int n, float *tile) {
    for (int i = threadIdx.x; i < n * 9; i += kBlock) tile[i] = bf16_to_f32(g[i]);
}
__device__ __forceinline__ void tile_out_bf16(uint16_t *__restrict__ g, int n, const float *tile) {
    for (int i = threadIdx.x; i < n * 9; i += kBlock) g[i] = f32_to_bf16(tile[i]);
}

template <bool BF16, bool VEC>
__device__ __forceinline__ void tile_in(const void *base, int64_t first, int n, float *tile) {
    if (BF16) tile_in_bf16(static_cast<const uint16_t *>(base) + first * 9, n, tile);
    else tile_in_f32<VEC>(static_cast<const float *>(base) + first * 9, n, tile);
}
template <bool BF16, bool VEC>
__device__ __forceinline__ void tile_out(void *base, int64_t first, int n, const float *tile) {
    if (BF16) tile_out_bf16(static_cast<uint16_t *>(base) + first * 9, n, tile);
    else tile_out_f32<VEC>(static_cast<float *>(base) + first * 9, n, tile);
}

__device__ __forceinline__ void lane_get(const float *tile, bool active, float (&m)[9]) {
    const float *p = tile + threadIdx.x * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = active ? p[i] : ((i & 3) == 0 ? 1.f : 0.f);   // idle lanes: identity
}
__device__ __forceinline__ void lane_put(float *tile, const float (&m)[9]) {
    float *p = tile + threadIdx.x * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = m[i];
}

// ---- K1 -------------------------------------------------------------------------------------------
template <bool BF16, bool VEC, bool FLIP>
__global__ __launch_bounds__(kBlock) void k_project_fwd(const void *__restrict__ M, float *__restrict__ R,
                                                        uint8_t *__restrict__ flip, int64_t B) {
    __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int n = static_cast<int>(min<int64_t>(kBlock, B - first));
    tile_in<BF16, VEC>(M, first, n, tile);
    __syncthreads();
    float m[9], r[9];
    const bool active = static_cast<int>(threadIdx.x) < n;
    lane_get(tile, active, m);
    so3::project_rotation<float>(m, r);
    if (FLIP && active) flip[first + threadIdx.x] = so3::det_negative(m) ? 1 : 0;
    lane_put(tile, r);          // each lane overwrites only the nine words it alone has read
    __syncthreads();
    tile_out<false, VEC>(R, first, n, tile);
}


// ---- K2 -------------------------------------------------------------------------------------------
template <bool BF16, bool VEC>
__global__ __launch_bounds__(kBlock) void k_project_bwd(const void *__restrict__ M, const float *__restrict__ G,
                                                        void *__restrict__ dM, int64_t B) {
    __shared__ __attribute__((aligned(16))) float tile_m[kTileFloats];
    __shared__ __attribute__((aligned(16))) float tile_g[kTileFloats];
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int n = static_cast<int>(min<int64_t>(kBlock, B - first));
    tile_in<BF16, VEC>(M, first, n, tile_m);
    tile_in<false, VEC>(G, first, n, tile_g);
    __syncthreads();
    float m[9], g[9], dm[9];
    const bool active = static_cast<int>(threadIdx.x) < n;
    lane_get(tile_m, active, m);
    lane_get(tile_g, active, g);
    so3::project_backward_rows<float>(m, g, dm);
    lane_put(tile_m, dm);
    __syncthreads();
    tile_out<BF16, VEC>(dM, first, n, tile_m);
}

// ---- block reduction of one double (sum) --------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double block_sum(double v, double *scratch /* >= 4 doubles of LDS */) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) scratch[wave] = v;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// A remainder kernel's share of a workspace reduction (so3_rows.h): its workgroups fill slots [0, gridDim.x) and take no
// ticket; the engine launch that follows on the stream sums them with its own.
__device__ __forceinline__ void publish_partial(so3::ReduceWs *ws, double total, bool flag) {
    so3::slot_publish(ws, blockIdx.x, total);
    if (flag) atomicOr(&ws->flag, 1);
}

// ---- K3 -------------------------------------------------------------------------------------------
template <bool BF16, bool VEC, bool WANT_R, bool WANT_DM>
__global__ __launch_bounds__(kBlock) void k_frob_fwd_bwd(const void *__restrict__ M, const float *__restrict__ Rtrue,
                                                         float *__restrict__ R, void *__restrict__ dM,
                                                         double *__restrict__ loss_sum, int64_t B, float inv_b, so3::ReduceWs *ws) {
    __shared__ __attribute__((aligned(16))) float tile_m[kTileFloats];
    __shared__ __attribute__((aligned(16))) float tile_t[kTileFloats];
    __shared__ double red[4];
    const int64_t ntiles = (B + kBlock - 1) / kBlock;
    double acc = 0.0;                                  // per-lane partial of sum_b ||.||_F over this workgroup's tiles
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t first = tile * kBlock;
        const int n = static_cast<int>(min<int64_t>(kBlock, B - first));
        tile_in<BF16, VEC>(M, first, n, tile_m);
        tile_in<false, VEC>(Rtrue, first, n, tile_t);
        __syncthreads();
        float m[9], t[9], r[9], g[9], dm[9];
        const bool active = static_cast<int>(threadIdx.x) < n;
        lane_get(tile_m, active, m);
        lane_get(tile_t, active, t);
        so3::HardRows<float> hard;
        so3::project_rotation_frames<WANT_DM, float>(m, r, hard);
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = r[i] - t[i];   // d||Rtrue - R||/dR = (R - Rtrue)/||.||
        const so3::FrobRow<float> fr = so3::frob_row<float>(g, inv_b);      // the engine's arithmetic (so3_rows.h)
        if (active) acc += static_cast<double>(fr.nrm);
        if (WANT_DM) {
#pragma unroll
            for (int i = 0; i < 9; ++i) g[i] *= fr.gs;
            so3::backward_given_rotation<float>(m, r, g, hard, dm);
            lane_put(tile_m, dm);
        }
        if (WANT_R) lane_put(tile_t, r);
        __syncthreads();
        if (WANT_DM) tile_out<BF16, VEC>(dM, first, n, tile_m);
        if (WANT_R) tile_out<false, VEC>(R, first, n, tile_t);
        __syncthreads();                               // the tiles are reused by the next iteration
    }
    // one float64 atomic per workgroup: same-address atomics cost ~12 ns each (one per 256-row tile made this
    // kernel atomic-bound: 59 us per 1M rows)
    const double total = block_sum(acc, red);
    if (threadIdx.x == 0) {
        if (ws != nullptr) publish_partial(ws, total, false);
        else atomicAdd(loss_sum, total);
    }
}

// K3 for a batch that fits ONE workgroup (config #4: B = 512): one row per thread, rows read and written straight from
// global memory (9 KB in all: latency-bound, not a streaming problem), the loss reduced inside the workgroup and written
// with a plain store -- no zero-fill launch before the kernel and no atomic.  The call is then a single launch.
constexpr int kSmallBatch = 1024;
template <bool BF16, bool WANT_R, bool WANT_DM>
__global__ __launch_bounds__(kSmallBatch) void k_frob_small(const void *__restrict__ M, const float *__restrict__ Rtrue,
                                                            float *__restrict__ R, void *__restrict__ dM,
                                                            double *__restrict__ loss_sum, float *__restrict__ loss_mean, int B, float inv_b,
                                                            bool add) {
    __shared__ double red[kSmallBatch / 64];
    const int b = threadIdx.x;
    const bool active = b < B;
    float m[9], t[9], r[9], g[9], dm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        m[i] = (i & 3) == 0 ? 1.f : 0.f;              // idle lanes: identity
        t[i] = m[i];
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            m[i] = BF16 ? bf16_to_f32(static_cast<const uint16_t *>(M)[b * 9 + i]) : static_cast<const float *>(M)[b * 9 + i];
            t[i] = Rtrue[b * 9 + i];
        }
    }
    so3::HardRows<float> hard;
    so3::project_rotation_frames<WANT_DM, float>(m, r, hard);
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = r[i] - t[i];
    const so3::FrobRow<float> fr = so3::frob_row<float>(g, inv_b);
    const float nrm = fr.nrm;
    if (WANT_DM) {
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] *= fr.gs;
        so3::backward_given_rotation<float>(m, r, g, hard, dm);
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (WANT_DM) {
                if (BF16) static_cast<uint16_t *>(dM)[b * 9 + i] = f32_to_bf16(dm[i]);
                else static_cast<float *>(dM)[b * 9 + i] = dm[i];
            }
            if (WANT_R) R[b * 9 + i] = r[i];
        }
    }
    const double v = wave_sum(active ? static_cast<double>(nrm) : 0.0);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) total += red[w];
        if (loss_sum != nullptr) *loss_sum = add ? *loss_sum + total : total;        // SO3_PREZEROED: added to, as the atomics do
        if (loss_mean != nullptr) *loss_mean = static_cast<float>(total * (1.0 / static_cast<double>(B)));   // float64 sum / B, rounded once
    }
}

// ---- K3', stand-alone Frobenius loss (3D-Pose/loss.py:7-11) for callers that already hold R_pred -----
// loss_sum += sum_b ||Rtrue_b - Rpred_b||_F ;  optional dRpred_b = (Rpred_b - Rtrue_b) / (B ||.||_F).
// Element-wise over flat float4s is not possible (the norm is per 9-float row), so the same 256-row tile
// staging as the other block kernels is used.
template <bool VEC, bool WANT_GRAD>
__global__ __launch_bounds__(kBlock) void k_frob_loss(const float *__restrict__ Rpred, const float *__restrict__ Rtrue,
                                                      float *__restrict__ dRpred, double *__restrict__ loss_sum,
                                                      int64_t B, float inv_b, so3::ReduceWs *ws) {
    __shared__ __attribute__((aligned(16))) float tile_p[kTileFloats];
    __shared__ __attribute__((aligned(16))) float tile_t[kTileFloats];
    __shared__ double red[4];
    const int64_t ntiles = (B + kBlock - 1) / kBlock;
    double acc = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t first = tile * kBlock;
        const int n = static_cast<int>(min<int64_t>(kBlock, B - first));
        tile_in<false, VEC>(Rpred, first, n, tile_p);
        tile_in<false, VEC>(Rtrue, first, n, tile_t);
        __syncthreads();
        float p[9], t[9], g[9];
        const bool active = static_cast<int>(threadIdx.x) < n;
        lane_get(tile_p, active, p);
        lane_get(tile_t, active, t);
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = p[i] - t[i];
        const so3::FrobRow<float> fr = so3::frob_row<float>(g, inv_b);
        if (active) acc += static_cast<double>(fr.nrm);
        __syncthreads();
        if (WANT_GRAD) {
#pragma unroll
            for (int i = 0; i < 9; ++i) g[i] *= fr.gs;
            lane_put(tile_p, g);
            __syncthreads();
            tile_out<false, VEC>(dRpred, first, n, tile_p);
            __syncthreads();
        }
    }
    const double total = block_sum(acc, red);          // one atomic per workgroup
    if (threadIdx.x == 0) {
        if (ws != nullptr) publish_partial(ws, total, false);
        else atomicAdd(loss_sum, total);
    }
}

// K3' for a launch-bound batch (B <= kSmallBatch): one workgroup, one row per thread, loss_sum written with a plain
// store -- no zero-fill before the kernel.  Row arithmetic as in k_frob_loss / OpFrobLoss.
template <bool WANT_GRAD>
__global__ __launch_bounds__(kSmallBatch) void k_frob_loss_small(const float *__restrict__ Rpred, const float *__restrict__ Rtrue,
                                                                 float *__restrict__ dRpred, double *__restrict__ loss_sum,
                                                                 float *__restrict__ loss_mean, int B, float inv_b, bool add) {
    __shared__ double red[kSmallBatch / 64];
    const int b = threadIdx.x;
    const bool active = b < B;
    float g[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = active ? Rpred[b * 9 + i] - Rtrue[b * 9 + i] : 0.f;
    const so3::FrobRow<float> fr = so3::frob_row<float>(g, inv_b);
    const float nrm = fr.nrm;
    if (WANT_GRAD && active) {
#pragma unroll
        for (int i = 0; i < 9; ++i) dRpred[b * 9 + i] = g[i] * fr.gs;
    }
    const double v = wave_sum(active ? static_cast<double>(nrm) : 0.0);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) total += red[w];
        *loss_sum = add ? *loss_sum + total : total;
        if (loss_mean != nullptr) *loss_mean = static_cast<float>(total * (1.0 / static_cast<double>(B)));
    }
}

// dst[i] = src[i] * (*factor): the chain rule's last step for a gradient that was computed at unit upstream scale in the forward
// launch (K3 stores d loss / dM; autograd hands loss.backward() the upstream factor as a 0-dim DEVICE tensor).  One launch
// instead of torch's float() / mul / to(bfloat16) chain around a 4-us kernel.  16 bytes per thread; n counts elements.
template <bool BF16>
__global__ __launch_bounds__(kBlock) void k_scale(const void *__restrict__ src, const float *__restrict__ factor, void *__restrict__ dst, int64_t n) {
    const float f = *factor;
    constexpr int kPer = BF16 ? 8 : 4;
    const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kPer;
    if (i0 + kPer <= n && aligned16(static_cast<const char *>(src) + i0 * (BF16 ? 2 : 4)) && aligned16(static_cast<char *>(dst) + i0 * (BF16 ? 2 : 4))) {
        if constexpr (BF16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(src) + i0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = static_cast<uint32_t>(f32_to_bf16(bf16_to_f32(static_cast<uint16_t>(w[k] & 0xFFFFu)) * f))
                       | static_cast<uint32_t>(f32_to_bf16(bf16_to_f32(static_cast<uint16_t>(w[k] >> 16)) * f)) << 16;
            *reinterpret_cast<uint4 *>(static_cast<uint16_t *>(dst) + i0) = uint4{o[0], o[1], o[2], o[3]};
        } else {
            float4 v = *reinterpret_cast<const float4 *>(static_cast<const float *>(src) + i0);
            v.x *= f; v.y *= f; v.z *= f; v.w *= f;
            *reinterpret_cast<float4 *>(static_cast<float *>(dst) + i0) = v;
        }
    } else {
        for (int64_t i = i0; i < n && i < i0 + kPer; ++i) {
            if constexpr (BF16) static_cast<uint16_t *>(dst)[i] = f32_to_bf16(bf16_to_f32(static_cast<const uint16_t *>(src)[i]) * f);
            else static_cast<float *>(dst)[i] = static_cast<const float *>(src)[i] * f;
        }
    }
}

// float32 mean from the float64 sum once the kernels before it on the stream are done (batches too large for one workgroup,
// no workspace: the atomics' total is only complete at the end of the launch)
__global__ void k_mean_from_sum(const double *__restrict__ loss_sum, float *__restrict__ loss_mean, double inv_b) {
    *loss_mean = static_cast<float>(*loss_sum * inv_b);
}

// ---- K4 -------------------------------------------------------------------------------------------
template <bool VEC, bool WANT_DEG, bool WANT_SUM>
__global__ __launch_bounds__(kBlock) void k_angle_error(const float *__restrict__ R1, const float *__restrict__ R2,
                                                        double *__restrict__ out, double *__restrict__ sum_count,
                                                        int32_t *__restrict__ range_flag, double unit, int64_t B, so3::ReduceWs *ws) {
    __shared__ __attribute__((aligned(16))) float tile_a[kTileFloats];
    __shared__ __attribute__((aligned(16))) float tile_b[kTileFloats];
    __shared__ double red[4];
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int n = static_cast<int>(min<int64_t>(kBlock, B - first));
    tile_in<false, VEC>(R1, first, n, tile_a);
    tile_in<false, VEC>(R2, first, n, tile_b);
    __syncthreads();
    float a[9], b[9];
    const bool active = static_cast<int>(threadIdx.x) < n;
    lane_get(tile_a, active, a);
    lane_get(tile_b, active, b);
    double tr = 0.0;                                   // tr(R1^T R2) = sum_ij R1_ij R2_ij, float64
#pragma unroll
    for (int i = 0; i < 9; ++i) tr = fma(static_cast<double>(a[i]), static_cast<double>(b[i]), tr);
    const double c_raw = (tr - 1.0) * 0.5;
    const bool bad = active && (c_raw < -1.1 || c_raw > 1.1);  // NaN compares false, as torch.any(...) does
    double c = fmin(fmax(c_raw, -1.0), 1.0);                   // torch.clamp ...
    if (c_raw != c_raw) c = c_raw;                             // ... which keeps NaN (fmin/fmax drop it)
    const double ang = so3::acos_f64(c) * unit;
    if (__any(bad) && (threadIdx.x & 63) == 0) {
        if (ws != nullptr) atomicOr(&ws->flag, 1);
        else if (range_flag != nullptr) atomicOr(range_flag, 1);
    }
    if (WANT_DEG && active) out[first + threadIdx.x] = ang;
    if (WANT_SUM) {
        const double total = block_sum(active ? ang : 0.0, red);
        if (threadIdx.x == 0) {
            if (ws != nullptr) publish_partial(ws, total, false);
            else atomicAdd(sum_count, total);  // the row count is written once by k_angle_init
        }
    }
}

// Batches of up to kSmallBatch rows (the per-batch metric of a training loop, 3D-Pose/main.py:60-62: B = 512) are
// launch-latency-bound, and the accumulators' initialisation was a launch of its own.  One workgroup, one row per thread:
// the kernel writes (sum, count) and the range flag with plain stores (with SO3_PREZEROED it adds to the sum and ORs the flag, as the
// atomics do) -- one launch, no atomics.  PROJECT: the first
// operand is the head's input M and the angle is taken of its projection (the fused evaluation step).
template <bool PROJECT, bool WANT_R, bool WANT_DEG>
__global__ __launch_bounds__(kSmallBatch) void k_angle_small(const float *__restrict__ A, const float *__restrict__ Bm,
                                                             float *__restrict__ R, double *__restrict__ deg,
                                                             double *__restrict__ sum_count, int32_t *__restrict__ range_flag,
                                                             double unit, int B, bool add) {
    __shared__ double red[kSmallBatch / 64];
    __shared__ int red_bad[kSmallBatch / 64];
    const int b = threadIdx.x;
    const bool active = b < B;
    float a[9], t[9], r[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        a[i] = (i & 3) == 0 ? 1.f : 0.f;              // idle lanes: identity
        t[i] = a[i];
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            a[i] = A[b * 9 + i];
            t[i] = Bm[b * 9 + i];
        }
    }
    if (PROJECT) {
        so3::project_rotation<float>(a, r);
        if (WANT_R && active) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[b * 9 + i] = r[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) r[i] = a[i];
    }
    double tr = 0.0;                                   // the arithmetic of OpAngle / k_angle_error, operation for operation
#pragma unroll
    for (int i = 0; i < 9; ++i) tr = fma(static_cast<double>(r[i]), static_cast<double>(t[i]), tr);
    const double c_raw = (tr - 1.0) * 0.5;
    const bool bad = active && (c_raw < -1.1 || c_raw > 1.1);
    double c = fmin(fmax(c_raw, -1.0), 1.0);
    if (c_raw != c_raw) c = c_raw;
    const double ang = so3::acos_f64(c) * unit;
    if (WANT_DEG && active) deg[b] = ang;
    const double v = wave_sum(active ? ang : 0.0);
    const bool any_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = v; red_bad[threadIdx.x >> 6] = any_bad ? 1 : 0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        int flag = 0;
        for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) { total += red[w]; flag |= red_bad[w]; }
        if (sum_count) { sum_count[0] = add ? sum_count[0] + total : total; sum_count[1] = static_cast<double>(B); }   // add: SO3_PREZEROED
        if (range_flag) *range_flag = add ? (*range_flag | flag) : flag;
    }
}

__global__ void k_angle_init(double *sum_count, int32_t *range_flag, double count) {
    if (sum_count) { sum_count[0] = 0.0; sum_count[1] = count; }
    if (range_flag) *range_flag = 0;
}

// float32 radians variant (rotation_representation.py:209-227; point_cloud/main.py:61-73): tr(m1 m2^T) in float32, clamp to [lo, hi];
// `sum` (nullable): the block's angles are added to it (one atomic per workgroup); theta nullable then.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_geodesic_f32(const float *__restrict__ R1, const float *__restrict__ R2,
                                                         float *__restrict__ theta, double *__restrict__ sum, float lo, float hi, int64_t B,
                                                         so3::ReduceWs *__restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float tile_a[kTileFloats];
    __shared__ __attribute__((aligned(16))) float tile_b[kTileFloats];
    __shared__ double part[kBlock / 64];
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int n = static_cast<int>(min<int64_t>(kBlock, B - first));
    tile_in<false, VEC>(R1, first, n, tile_a);
    tile_in<false, VEC>(R2, first, n, tile_b);
    __syncthreads();
    float a[9], b[9];
    const bool active = static_cast<int>(threadIdx.x) < n;
    lane_get(tile_a, active, a);
    lane_get(tile_b, active, b);
    // diagonal of m1 m2^T, summed in the reference's order: m00 + m11 + m22
    const float d0 = fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]));
    const float d1 = fmaf(a[5], b[5], fmaf(a[4], b[4], a[3] * b[3]));
    const float d2 = fmaf(a[8], b[8], fmaf(a[7], b[7], a[6] * b[6]));
    float c = (d0 + d1 + d2 - 1.f) * 0.5f;
    c = (c > hi) ? hi : c;     // torch.min / torch.max with a constant, torch.clamp: NaN stays NaN
    c = (c < lo) ? lo : c;
    const float th = acosf(c);
    if (active && theta != nullptr) theta[first + threadIdx.x] = th;
    if (sum != nullptr) {
        double v = active ? static_cast<double>(th) : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) t += part[w];
            if (ws != nullptr) publish_partial(ws, t, false);
            else atomicAdd(sum, t);
        }
    }
}

// ---- K4b: backward of the metrics, one row per thread: the remainder (< 64 rows) and unaligned views of the streaming kernel; the
// arithmetic is the engine operation's own (so3::OpAngleBwd::compute, one matrix per lane).  `g` = the per-row upstream gradient
// (float32, or float64 with F64MATH) when the operation takes one.
template <class Op>
__global__ __launch_bounds__(kBlock) void k_angle_bwd_rows(Op op, const void *__restrict__ g, float *__restrict__ d1, float *__restrict__ d2, int64_t B) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (row >= B) return;
    so3::RowCtx<1> ctx{};
    so3::Rows<float, Op> rows;
    const float *a = static_cast<const float *>(op.in0) + row * 9, *b = static_cast<const float *>(op.in1) + row * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) { rows.a[i] = a[i]; rows.b[i] = b[i]; }
    if constexpr (Op::kIn2 != 0) {
        const float *gw = static_cast<const float *>(g) + row * Op::kIn2N;
#pragma unroll
        for (int i = 0; i < Op::kIn2N; ++i) rows.c[i] = gw[i];
    }
    op.template compute<float, 1>(rows, ctx);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        d1[row * 9 + i] = rows.o0[i];
        if constexpr (Op::kOut1 != 0) d2[row * 9 + i] = rows.o1[i];
    }
}

// The same gradient from float64 data (so3_angle_bwd_f64): one row per thread, grid-stride.  g: per-row, or one shared value (scalar).
__global__ __launch_bounds__(kBlock) void k_angle_bwd_f64(const double *__restrict__ R1, const double *__restrict__ R2, const double *__restrict__ g,
                                                          bool scalar, double div, double unit, double lo, double hi, double *__restrict__ d1,
                                                          double *__restrict__ d2, int64_t B) {
#pragma clang fp contract(off)
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; row < B; row += static_cast<int64_t>(gridDim.x) * kBlock) {
        double a[9], b[9], tr = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) { a[i] = R1[row * 9 + i]; b[i] = R2[row * 9 + i]; tr = fma(a[i], b[i], tr); }
        const double c = (tr - 1.0) * 0.5;
        const double up = (scalar ? g[0] : g[row]) / div;
        const double om = 1.0 - c * c;
        double h = (c >= lo && c <= hi && om > 0.0) ? (up * unit) * (-1.0 / __builtin_sqrt(om)) * 0.5 : 0.0;
        if (c != c) h = c;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (d1 != nullptr) d1[row * 9 + i] = h * b[i];
            if (d2 != nullptr) d2[row * 9 + i] = h * a[i];
        }
    }
}

// ---- K5 -------------------------------------------------------------------------------------------
// One wave per cloud at a time; lane i takes points i, i+64, ... as 12-byte (dwordx3) loads, so each
// wave-instruction reads 768 contiguous bytes.  The nine partial sums are reduced across the wave
// (DPP within rows of 16, then two cross-row exchanges); lane j of the wave keeps the H of the j-th
// cloud the wave has processed, and after its last cloud the wave runs the K1 body once with one
// cloud per lane.
__device__ __forceinline__ float dpp_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
}
__device__ __forceinline__ float dpp_xor2(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
}
__device__ __forceinline__ float dpp_half_mirror(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
}
__device__ __forceinline__ float dpp_mirror(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));  // row_mirror
}
__device__ __forceinline__ float wave_allsum(float v) {
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
constexpr int kKabschUnroll = 8;           // 8 x 2 x 768 B = 12 KB of loads in flight per wave

__global__ __launch_bounds__(kBlock) void k_kabsch(const float *__restrict__ P, const float *__restrict__ Q,
                                                   float *__restrict__ R, float *__restrict__ H, int64_t B, int32_t N,
                                                   int clouds_per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // SGPR: cloud indices stay scalar
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * clouds_per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(clouds_per_wave, B - c0));
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (i & 3) == 0 ? 1.f : 0.f;
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        // One buffer descriptor per cloud (num_records = N*12 B): lanes past the last point read zeros, which add
        // nothing to the sums, so the point loop needs no tail and no exec-masked branch.  Streamed once: nt.
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        const so3::rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Q) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        float acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = 0.f;
        for (int i0 = 0; i0 < N; i0 += 64 * kKabschUnroll) {
            u32x3 pp[kKabschUnroll], qq[kKabschUnroll];
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const int off = (i0 + 64 * u + lane) * 12;
                pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, off, 0, so3::kStreamNt);
                qq[u] = __builtin_amdgcn_raw_buffer_load_b96(rq, off, 0, so3::kStreamNt);
            }
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                const float qx = __uint_as_float(qq[u].x), qy = __uint_as_float(qq[u].y), qz = __uint_as_float(qq[u].z);
                acc[0] = fmaf(qx, px, acc[0]); acc[1] = fmaf(qx, py, acc[1]); acc[2] = fmaf(qx, pz, acc[2]);
                acc[3] = fmaf(qy, px, acc[3]); acc[4] = fmaf(qy, py, acc[4]); acc[5] = fmaf(qy, pz, acc[5]);
                acc[6] = fmaf(qz, px, acc[6]); acc[7] = fmaf(qz, py, acc[7]); acc[8] = fmaf(qz, pz, acc[8]);
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float tot = wave_allsum(acc[i]);
            h[i] = (lane == j) ? tot : h[i];
        }
    }
    const bool active = lane < nc;
    float r[9];
    so3::project_rotation<float>(h, r);
    if (active) {
        float *out = R + (c0 + lane) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = r[i];
        if (H != nullptr) {
            float *ho = H + (c0 + lane) * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) ho[i] = h[i];
        }
    }
}

// ---- K5b: Kabsch backward ---------------------------------------------------------------------------------------
// Forward H = sum_i q_i p_i^T, R = proj(H).  Given gR and gH (either may be null):
//     dH = K2(H, gR) + gH,   dQ_i = dH p_i,   dP_i = dH^T q_i.
// k_kabsch's skeleton turned round: the K2 body runs once per lane (lane j: the wave's j-th cloud; idle lanes take an
// identity H and a zero gR) BEFORE the point loop, then each cloud's dH is broadcast from its lane (readlane, j is
// wave-uniform) and the cloud is streamed.  dQ needs only P and dP only Q: a one-sided gradient reads half the bytes.
template <bool WANT_DP, bool WANT_DQ>
__global__ __launch_bounds__(kBlock) void k_kabsch_bwd(const float *__restrict__ P, const float *__restrict__ Q,
                                                       const float *__restrict__ H, const float *__restrict__ gR,
                                                       const float *__restrict__ gH, float *__restrict__ dP, float *__restrict__ dQ,
                                                       int64_t B, int32_t N, int clouds_per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * clouds_per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(clouds_per_wave, B - c0));
    const bool active = lane < nc;
    float dh[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) dh[i] = 0.f;
    if (gR != nullptr) {
        float h[9], g[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            h[i] = active ? H[(c0 + lane) * 9 + i] : ((i & 3) == 0 ? 1.f : 0.f);
            g[i] = active ? gR[(c0 + lane) * 9 + i] : 0.f;
        }
        so3::project_backward_rows<float>(h, g, dh);
    }
    if (gH != nullptr) {
#pragma unroll
        for (int i = 0; i < 9; ++i) dh[i] += active ? gH[(c0 + lane) * 9 + i] : 0.f;
    }
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        float d[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) d[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dh[i]), j));
        const int64_t base = (c0 + j) * N * 3;
        so3::rsrc_t rp, rq, rdp, rdq;
        if (WANT_DQ) {
            rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + base, 0, cloud_bytes, so3::kRsrcFlags);
            rdq = __builtin_amdgcn_make_buffer_rsrc(dQ + base, 0, cloud_bytes, so3::kRsrcFlags);
        }
        if (WANT_DP) {
            rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Q) + base, 0, cloud_bytes, so3::kRsrcFlags);
            rdp = __builtin_amdgcn_make_buffer_rsrc(dP + base, 0, cloud_bytes, so3::kRsrcFlags);
        }
        for (int i0 = 0; i0 < N; i0 += 64 * kKabschUnroll) {
            u32x3 pp[kKabschUnroll], qq[kKabschUnroll];
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const int off = (i0 + 64 * u + lane) * 12;
                if (WANT_DQ) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, off, 0, so3::kStreamNt);
                if (WANT_DP) qq[u] = __builtin_amdgcn_raw_buffer_load_b96(rq, off, 0, so3::kStreamNt);
            }
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const int off = (i0 + 64 * u + lane) * 12;       // lanes past the cloud's end: the range check drops the store
                if (WANT_DQ) {
                    const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                    const float x = fmaf(d[2], pz, fmaf(d[1], py, d[0] * px));
                    const float y = fmaf(d[5], pz, fmaf(d[4], py, d[3] * px));
                    const float z = fmaf(d[8], pz, fmaf(d[7], py, d[6] * px));
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(x), __float_as_uint(y), __float_as_uint(z)}, rdq, off, 0, so3::kStreamNt);
                }
                if (WANT_DP) {
                    const float qx = __uint_as_float(qq[u].x), qy = __uint_as_float(qq[u].y), qz = __uint_as_float(qq[u].z);
                    const float x = fmaf(d[6], qz, fmaf(d[3], qy, d[0] * qx));
                    const float y = fmaf(d[7], qz, fmaf(d[4], qy, d[1] * qx));
                    const float z = fmaf(d[8], qz, fmaf(d[5], qy, d[2] * qx));
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(x), __float_as_uint(y), __float_as_uint(z)}, rdp, off, 0, so3::kStreamNt);
                }
            }
        }
    }
}

// ---- K5c: rigid_align, the weighted and centred Kabsch giving a pose (R | t) -------------------------------------------
//     W = sum w_i,  pbar = sum w_i p_i / W,  qbar = sum w_i q_i / W,  H = sum w_i (q_i - qbar)(p_i - pbar)^T,
//     R = proj(H),  t = qbar - R pbar.
// k_kabsch's skeleton with a third, coalesced b32 stream for the weights.  ONE pass over the clouds: the sums are taken
// relative to the cloud's first point pair (so3_device.h: the pivot rule), sixteen of them instead of nine, and
// align_finish turns them into H and the centroids -- on every lane alike (the sums are wave-uniform after wave_allsum);
// lane j keeps cloud j's H, centroids and W.  Lanes past the cloud's end read zeros from the descriptor: a zero weight
// (WEIGHTED), or the index test (unweighted), keeps their pivot-shifted coordinates out of the sums.
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_rigid_align(const float *__restrict__ P, const float *__restrict__ Q, const float *__restrict__ Wt,
                                                        float *__restrict__ R, float *__restrict__ T, float *__restrict__ H,
                                                        float *__restrict__ S, int64_t B, int32_t N, int clouds_per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * clouds_per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(clouds_per_wave, B - c0));
    float h[9], st[7];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (i & 3) == 0 ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) st[i] = 0.f;
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        const float *pc = P + (c0 + j) * N * 3, *qc = Q + (c0 + j) * N * 3;
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pc), 0, cloud_bytes, so3::kRsrcFlags);
        const so3::rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(qc), 0, cloud_bytes, so3::kRsrcFlags);
        so3::rsrc_t rw;
        if (WEIGHTED) rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wt) + (c0 + j) * N, 0, static_cast<unsigned>(N) * 4u, so3::kRsrcFlags);
        float p0[3] = {0.f, 0.f, 0.f}, q0[3] = {0.f, 0.f, 0.f};               // the pivot: wave-uniform addresses
        if (N > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { p0[k] = pc[k]; q0[k] = qc[k]; }
        }
        float acc[so3::kAlignSums];
#pragma unroll
        for (int i = 0; i < so3::kAlignSums; ++i) acc[i] = 0.f;
        for (int i0 = 0; i0 < N; i0 += 64 * kKabschUnroll) {
            u32x3 pp[kKabschUnroll], qq[kKabschUnroll];
            float ww[kKabschUnroll];
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const int i = i0 + 64 * u + lane;
                pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, i * 12, 0, so3::kStreamNt);
                qq[u] = __builtin_amdgcn_raw_buffer_load_b96(rq, i * 12, 0, so3::kStreamNt);
                if (WEIGHTED) ww[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, i * 4, 0, so3::kStreamNt));
                else ww[u] = i < N ? 1.f : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u)
                so3::align_accumulate(ww[u], __uint_as_float(pp[u].x) - p0[0], __uint_as_float(pp[u].y) - p0[1], __uint_as_float(pp[u].z) - p0[2],
                                      __uint_as_float(qq[u].x) - q0[0], __uint_as_float(qq[u].y) - q0[1], __uint_as_float(qq[u].z) - q0[2], acc);
        }
#pragma unroll
        for (int i = 0; i < so3::kAlignSums; ++i) acc[i] = wave_allsum(acc[i]);
        float hj[9], sj[7];
        so3::align_finish(acc, p0, q0, hj, sj);
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = (lane == j) ? hj[i] : h[i];
#pragma unroll
        for (int i = 0; i < 7; ++i) st[i] = (lane == j) ? sj[i] : st[i];
    }
    const bool active = lane < nc;
    float r[9], t[3];
    so3::project_rotation<float>(h, r);
    so3::align_translation(r, st, t);
    if (active) {
        const int64_t c = c0 + lane;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[c * 9 + i] = r[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) T[c * 3 + i] = t[i];
        if (H != nullptr) {
#pragma unroll
            for (int i = 0; i < 9; ++i) H[c * 9 + i] = h[i];
        }
        if (S != nullptr) {
#pragma unroll
            for (int i = 0; i < 7; ++i) S[c * 7 + i] = st[i];
        }
    }
}

// ---- K5d: rigid_align backward ----------------------------------------------------------------------------------------
// Given gR, g_t, gH (each may be null).  With a_i = p_i - pbar, c_i = q_i - qbar, u = R^T g_t:
//     gR' = gR - g_t pbar^T        (t = qbar - R pbar depends on R)
//     dH  = K2(H, gR') + gH
//     dQ_i = w_i dH a_i + (w_i / W) g_t,   dP_i = w_i dH^T c_i - (w_i / W) u,   dw_i = c_i^T dH a_i + (g_t . c_i - u . a_i) / W.
// Why one pass suffices.  H depends on q_i directly, dH_i = w_i (dq_i) a_i^T, and through qbar: -(sum_j w_j a_j)^T-terms,
// d(qbar) (sum_j w_j a_j)^T -- but sum_j w_j a_j = sum_j w_j p_j - W pbar = 0, and likewise sum_j w_j c_j = 0 kills the
// pbar-terms; the w_i-derivative of H is c_i a_i^T plus the same two vanishing centroid terms.  What is left of the centroids
// is t's own dependence: d(qbar)/d(q_i) = w_i / W, d(qbar)/d(w_i) = c_i / W, d(pbar)/d(w_i) = a_i / W, with dL/d(qbar) = g_t
// and dL/d(pbar) = -R^T g_t = -u.  So every per-point gradient needs only per-cloud constants known before the point loop.
// k_kabsch_bwd's skeleton: K2 once per lane, the cloud's 21 constants broadcast from its lane, then one stream over the
// cloud.  dQ alone reads only P (and w), dP alone only Q (and w); dw reads both.  Wt may be null (all ones).
template <bool WANT_DP, bool WANT_DQ, bool WANT_DW>
__global__ __launch_bounds__(kBlock) void k_rigid_align_bwd(const float *__restrict__ P, const float *__restrict__ Q, const float *__restrict__ Wt,
                                                            const float *__restrict__ H, const float *__restrict__ R, const float *__restrict__ S,
                                                            const float *__restrict__ gR, const float *__restrict__ gT, const float *__restrict__ gH,
                                                            float *__restrict__ dP, float *__restrict__ dQ, float *__restrict__ dW,
                                                            int64_t B, int32_t N, int clouds_per_wave) {
    constexpr bool NEED_P = WANT_DQ || WANT_DW, NEED_Q = WANT_DP || WANT_DW;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * clouds_per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(clouds_per_wave, B - c0));
    const bool active = lane < nc;
    const int64_t c = c0 + lane;
    float kk[so3::kAlignBwdConsts];
    {
        float st[7], r[9], gt[3], dh[9];
#pragma unroll
        for (int i = 0; i < 7; ++i) st[i] = active ? S[c * 7 + i] : 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) { r[i] = active ? R[c * 9 + i] : 0.f; dh[i] = 0.f; }
#pragma unroll
        for (int i = 0; i < 3; ++i) gt[i] = (active && gT != nullptr) ? gT[c * 3 + i] : 0.f;
        if (gR != nullptr || gT != nullptr) {
            float h[9], g[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                h[i] = active ? H[c * 9 + i] : ((i & 3) == 0 ? 1.f : 0.f);
                g[i] = (active && gR != nullptr) ? gR[c * 9 + i] : 0.f;
            }
            so3::align_rotation_grad(gt, st, g);
            so3::project_backward_rows<float>(h, g, dh);
        }
        if (gH != nullptr) {
#pragma unroll
            for (int i = 0; i < 9; ++i) dh[i] += active ? gH[c * 9 + i] : 0.f;
        }
        so3::align_bwd_consts(dh, r, gt, st, kk);
    }
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        float k[so3::kAlignBwdConsts];
#pragma unroll
        for (int i = 0; i < so3::kAlignBwdConsts; ++i) k[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(kk[i]), j));
        const int64_t base = (c0 + j) * N * 3;
        so3::rsrc_t rp, rq, rw, rdp, rdq, rdw;
        if (NEED_P) rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + base, 0, cloud_bytes, so3::kRsrcFlags);
        if (NEED_Q) rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Q) + base, 0, cloud_bytes, so3::kRsrcFlags);
        if (Wt != nullptr) rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wt) + (c0 + j) * N, 0, static_cast<unsigned>(N) * 4u, so3::kRsrcFlags);
        if (WANT_DP) rdp = __builtin_amdgcn_make_buffer_rsrc(dP + base, 0, cloud_bytes, so3::kRsrcFlags);
        if (WANT_DQ) rdq = __builtin_amdgcn_make_buffer_rsrc(dQ + base, 0, cloud_bytes, so3::kRsrcFlags);
        if (WANT_DW) rdw = __builtin_amdgcn_make_buffer_rsrc(dW + (c0 + j) * N, 0, static_cast<unsigned>(N) * 4u, so3::kRsrcFlags);
        for (int i0 = 0; i0 < N; i0 += 64 * kKabschUnroll) {
            u32x3 pp[kKabschUnroll], qq[kKabschUnroll];
            float ww[kKabschUnroll];
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const int i = i0 + 64 * u + lane;
                if (NEED_P) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, i * 12, 0, so3::kStreamNt);
                if (NEED_Q) qq[u] = __builtin_amdgcn_raw_buffer_load_b96(rq, i * 12, 0, so3::kStreamNt);
                if (WANT_DP || WANT_DQ) ww[u] = Wt != nullptr ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, i * 4, 0, so3::kStreamNt)) : 1.f;
            }
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const int i = i0 + 64 * u + lane;                  // lanes past the cloud's end: the range check drops the stores
                float ax = 0.f, ay = 0.f, az = 0.f, cx = 0.f, cy = 0.f, cz = 0.f, x, y, z;
                if (NEED_P) { ax = __uint_as_float(pp[u].x) - k[9]; ay = __uint_as_float(pp[u].y) - k[10]; az = __uint_as_float(pp[u].z) - k[11]; }
                if (NEED_Q) { cx = __uint_as_float(qq[u].x) - k[12]; cy = __uint_as_float(qq[u].y) - k[13]; cz = __uint_as_float(qq[u].z) - k[14]; }
                if (WANT_DQ) {
                    so3::align_bwd_dq(k, ww[u], ax, ay, az, x, y, z);
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(x), __float_as_uint(y), __float_as_uint(z)}, rdq, i * 12, 0, so3::kStreamNt);
                }
                if (WANT_DP) {
                    so3::align_bwd_dp(k, ww[u], cx, cy, cz, x, y, z);
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(x), __float_as_uint(y), __float_as_uint(z)}, rdp, i * 12, 0, so3::kStreamNt);
                }
                if (WANT_DW)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(so3::align_bwd_dw(k, ax, ay, az, cx, cy, cz)), rdw, i * 4, 0, so3::kStreamNt);
            }
        }
    }
}

// ---- next row f4: on-device pair synthesis for Kabsch (point_cloud/prepare.py:21-49, point_cloud/main.py:173-181) --
// (a) the reference's rotation sampler as a kernel: quaternion (cos t, axis sin t) -> matrix, given the random draws;
// (b) Kabsch with the second cloud synthesised on the fly, q_i = R_gt p_i + sigma n_i, so only P is read from HBM.
// The noise is a counter-based generator (no state): a 32-bit mix of (seed, cloud, point, pair) -> two uniforms ->
// Box-Muller; restated by the test oracle (synth_normal_np).
__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// Six standard normals for a PAIR of points from three Box-Muller pairs (round 6; rounds 2-5: two pairs per point, the second one's sine
// thrown away -- seven transcendentals and five quarter-rate integer multiplies per point, now six and three and a half):
//     point a: (r_A cos, r_A sin)(2 pi u_A), r_C cos(2 pi u_C)        point b: (r_B cos, r_B sin)(2 pi u_B), r_C sin(2 pi u_C),   r = sqrt(-2 ln u_r).
// The pair of point p is j = (p >> 7) * 64 + (p & 63) and p is its point a or b by bit 6: the two points a lane holds in neighbouring trips of
// the kernel's loop (p and p + 64), whatever the cloud's length or the loop's unrolling.  Hardware transcendentals: v_log_f32 (log2),
// v_cos_f32 / v_sin_f32 (argument in turns).
// The integer side is what the generator costs (rounds 2-4: six full mixes per point, 80 us of the kernel's 223 per 65 536 x 1024
// points; the transcendentals were the smaller half), so:
//   * ONE full mix per pair, h0 = mix(cloud's key ^ pair's counter), and four single-multiply rounds of it with different shifts,
//     multipliers and pre-whitening, h1..h4 -- pairwise 64 x 64 and 256-fold-magnified chi-square of the six uniforms, against each
//     other and against the next pair's / cloud's, stay within 3.1 sigma over 4 seeds x 4M pairs (tests/test_oracle_golden.py holds a
//     reduced form; two rounds of the SAME shape fail it at 9 sigma);
//   * a uniform is 23 bits dropped into the mantissa of a float in [1, 2) by one v_alignbit_b32: the radii take 2 - x in (0, 1], the
//     angles take x as it is (cosine and sine have period one turn);
//   * u_rA, u_A, u_rB, u_B, u_rC = the high 23 bits of h0 .. h4; u_C = the high 23 bits of the four low bytes of h0 .. h3 (bits no other
//     uniform uses).
__device__ __forceinline__ unsigned synth_cloud_key(unsigned seed, unsigned cloud) { return mix32(seed ^ mix32(cloud * 0x9e3779b9u + 0x85ebca6bu)); }
__device__ __forceinline__ float synth_unit_float(unsigned h) { return __uint_as_float(__builtin_amdgcn_alignbit(0x7fu, h, 9u)); }   // 0x3f800000 | h >> 9
__device__ __forceinline__ void synth_normal3x2(unsigned cloud_key, unsigned pair, float (&na)[3], float (&nb)[3]) {
    const unsigned h0 = mix32(cloud_key ^ (pair * 0x9e3779b9u + 0xc2b2ae35u));
    unsigned h1 = h0 + 0x27d4eb2fu; h1 ^= h1 >> 16; h1 *= 0x7feb352du; h1 ^= h1 >> 15;
    unsigned h2 = h0 ^ 0x165667b1u; h2 ^= h2 >> 15; h2 *= 0x2c1b3c6du; h2 ^= h2 >> 16;
    unsigned h3 = h0 + 0x9e3779b1u; h3 ^= h3 >> 17; h3 *= 0x297a2d39u; h3 ^= h3 >> 14;
    unsigned h4 = h0 ^ 0x85ebca77u; h4 ^= h4 >> 14; h4 *= 0xc2b2ae3du; h4 ^= h4 >> 17;
    const unsigned low = __builtin_amdgcn_perm(__builtin_amdgcn_perm(h0, h1, 0x04000c0cu), __builtin_amdgcn_perm(h2, h3, 0x0c0c0400u), 0x07060100u);
    const float ra = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(2.0f - synth_unit_float(h0)));     // -2 ln2 log2(u), u in (0, 1]
    const float rb = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(2.0f - synth_unit_float(h2)));
    const float rc = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(2.0f - synth_unit_float(h4)));
    const float ta = synth_unit_float(h1), tb = synth_unit_float(h3), tc = synth_unit_float(low);                            // [1, 2) turns
    na[0] = ra * __builtin_amdgcn_cosf(ta); na[1] = ra * __builtin_amdgcn_sinf(ta); na[2] = rc * __builtin_amdgcn_cosf(tc);
    nb[0] = rb * __builtin_amdgcn_cosf(tb); nb[1] = rb * __builtin_amdgcn_sinf(tb); nb[2] = rc * __builtin_amdgcn_sinf(tc);
}

__global__ __launch_bounds__(kBlock) void k_rotations_axis_angle(const float *__restrict__ theta, const float *__restrict__ axis,
                                                                 float *__restrict__ R, int64_t B) {
    const int64_t b = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (b >= B) return;
    const float t = theta[b];
    float ax = axis[3 * b], ay = axis[3 * b + 1], az = axis[3 * b + 2];
    const float mag = fmaxf(sqrtf(ax * ax + ay * ay + az * az), 1e-8f);        // normalize_vector, prepare.py:12-18
    ax /= mag; ay /= mag; az /= mag;
    const float sn = sinf(t), qw = cosf(t);                                        // :24,27
    const float qx = ax * sn, qy = ay * sn, qz = az * sn;                          // :28-30
    const float xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
    const float xw = qx * qw, yw = qy * qw, zw = qz * qw;
    float *o = R + 9 * b;
    o[0] = 1 - 2 * yy - 2 * zz; o[1] = 2 * xy - 2 * zw;     o[2] = 2 * xz + 2 * yw;      // :43
    o[3] = 2 * xy + 2 * zw;     o[4] = 1 - 2 * xx - 2 * zz; o[5] = 2 * yz - 2 * xw;      // :44
    o[6] = 2 * xz - 2 * yw;     o[7] = 2 * yz + 2 * xw;     o[8] = 1 - 2 * xx - 2 * yy;  // :45
}

template <bool NOISE>
__global__ __launch_bounds__(kBlock) void k_kabsch_synth(const float *__restrict__ P, const float *__restrict__ Rgt, float sigma,
                                                         unsigned seed, float *__restrict__ R, float *__restrict__ H, int64_t B,
                                                         int32_t N, int clouds_per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * clouds_per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(clouds_per_wave, B - c0));
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (i & 3) == 0 ? 1.f : 0.f;
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        float g[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = Rgt[(c0 + j) * 9 + i];                   // wave-uniform: scalar loads
        float acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = 0.f;
        const unsigned cloud_key = synth_cloud_key(seed, static_cast<unsigned>(c0 + j));      // wave-uniform: the scalar unit's
        for (int i0 = 0; i0 < N; i0 += 64 * kKabschUnroll) {
            u32x3 pp[kKabschUnroll];
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u)
                pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, (i0 + 64 * u + lane) * 12, 0, so3::kStreamNt);
            static_assert(kKabschUnroll % 2 == 0, "the noise is drawn for the lane's points of two neighbouring trips at a time");
            float nz[kKabschUnroll][3];
            if constexpr (NOISE) {          // (a lane past the cloud's end draws too: its p is the range check's zero, and so is q p^T)
#pragma unroll
                for (int u = 0; u < kKabschUnroll; u += 2)              // points i0 + 64 u + lane and 64 further: pair (i0 / 128 + u / 2) * 64 + lane
                    synth_normal3x2(cloud_key, static_cast<unsigned>(((i0 >> 7) + (u >> 1)) * 64 + lane), nz[u], nz[u + 1]);
            }
#pragma unroll
            for (int u = 0; u < kKabschUnroll; ++u) {
                const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                float qx = fmaf(g[2], pz, fmaf(g[1], py, g[0] * px));               // q = R_gt p   (main.py:176-181)
                float qy = fmaf(g[5], pz, fmaf(g[4], py, g[3] * px));
                float qz = fmaf(g[8], pz, fmaf(g[7], py, g[6] * px));
                if constexpr (NOISE) {
                    qx = fmaf(sigma, nz[u][0], qx);
                    qy = fmaf(sigma, nz[u][1], qy);
                    qz = fmaf(sigma, nz[u][2], qz);
                }
                acc[0] = fmaf(qx, px, acc[0]); acc[1] = fmaf(qx, py, acc[1]); acc[2] = fmaf(qx, pz, acc[2]);
                acc[3] = fmaf(qy, px, acc[3]); acc[4] = fmaf(qy, py, acc[4]); acc[5] = fmaf(qy, pz, acc[5]);
                acc[6] = fmaf(qz, px, acc[6]); acc[7] = fmaf(qz, py, acc[7]); acc[8] = fmaf(qz, pz, acc[8]);
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float tot = wave_allsum(acc[i]);
            h[i] = (lane == j) ? tot : h[i];
        }
    }
    const bool active = lane < nc;
    float r[9];
    so3::project_rotation<float>(h, r);
    if (active) {
        float *out = R + (c0 + lane) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = r[i];
        if (H != nullptr) {
            float *ho = H + (c0 + lane) * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) ho[i] = h[i];
        }
    }
}

// Clouds of a few points (N <= kSynthFew): the same skeleton, one point per lane, with q = R_gt p + sigma n formed in float64 -- the noise
// included: log, sqrt, cospi / sinpi on the same six uniforms -- and rounded to float32 ONCE.  H = sum q p^T of so few terms has no slack to
// hide the roundings of q's three products where they cancel (a q_a of 1e-4 from products of 0.3 carries 3e-8, three hundred times
// u |q_a|); with q correctly rounded, |dH_ab| <= 2 N u sum_i |q_ia| |p_ib| holds for every N.  Eight points a cloud: the cost does not matter.
constexpr int kSynthFew = 8;
__device__ __forceinline__ double synth_unit_double(unsigned h) { return static_cast<double>(h >> 9) * (1.0 / 8388608.0); }   // [0, 1)
template <bool NOISE>
__global__ __launch_bounds__(kBlock) void k_kabsch_synth_few(const float *__restrict__ P, const float *__restrict__ Rgt, float sigma,
                                                             unsigned seed, float *__restrict__ R, float *__restrict__ H, int64_t B,
                                                             int32_t N, int clouds_per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * clouds_per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(clouds_per_wave, B - c0));
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (i & 3) == 0 ? 1.f : 0.f;
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        const u32x3 pp = __builtin_amdgcn_raw_buffer_load_b96(rp, lane * 12, 0, so3::kStreamNt);     // lanes past the cloud's end: zeros
        const float p[3] = {__uint_as_float(pp.x), __uint_as_float(pp.y), __uint_as_float(pp.z)};
        double nz[3] = {0.0, 0.0, 0.0};
        if constexpr (NOISE) {          // point `lane` < 64 is point a of pair `lane` (synth_normal3x2): (r_A cos, r_A sin)(u_A), r_C cos(u_C)
            const unsigned cloud_key = synth_cloud_key(seed, static_cast<unsigned>(c0 + j));
            const unsigned h0 = mix32(cloud_key ^ (static_cast<unsigned>(lane) * 0x9e3779b9u + 0xc2b2ae35u));
            unsigned h1 = h0 + 0x27d4eb2fu; h1 ^= h1 >> 16; h1 *= 0x7feb352du; h1 ^= h1 >> 15;
            unsigned h2 = h0 ^ 0x165667b1u; h2 ^= h2 >> 15; h2 *= 0x2c1b3c6du; h2 ^= h2 >> 16;
            unsigned h3 = h0 + 0x9e3779b1u; h3 ^= h3 >> 17; h3 *= 0x297a2d39u; h3 ^= h3 >> 14;
            unsigned h4 = h0 ^ 0x85ebca77u; h4 ^= h4 >> 14; h4 *= 0xc2b2ae3du; h4 ^= h4 >> 17;
            const unsigned low = ((h0 & 0xffu) << 24) | ((h1 & 0xffu) << 16) | ((h2 & 0xffu) << 8) | (h3 & 0xffu);
            const double ra = sqrt(-2.0 * log(1.0 - synth_unit_double(h0))), rc = sqrt(-2.0 * log(1.0 - synth_unit_double(h4)));
            const double ta = 2.0 * synth_unit_double(h1), tc = 2.0 * synth_unit_double(low);        // half turns
            nz[0] = ra * cospi(ta); nz[1] = ra * sinpi(ta); nz[2] = rc * cospi(tc);
        }
        float q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float *g = Rgt + (c0 + j) * 9 + 3 * a;                         // wave-uniform: scalar loads
            double s = static_cast<double>(g[0]) * p[0];                          // products of two floats are exact in float64
            s = fma(static_cast<double>(g[1]), static_cast<double>(p[1]), s);
            s = fma(static_cast<double>(g[2]), static_cast<double>(p[2]), s);
            if constexpr (NOISE) s = fma(static_cast<double>(sigma), nz[a], s);
            q[a] = static_cast<float>(s);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float tot = wave_allsum(q[i / 3] * p[i % 3]);
            h[i] = (lane == j) ? tot : h[i];
        }
    }
    const bool active = lane < nc;
    float r[9];
    so3::project_rotation<float>(h, r);
    if (active) {
        float *out = R + (c0 + lane) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = r[i];
        if (H != nullptr) {
            float *ho = H + (c0 + lane) * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) ho[i] = h[i];
        }
    }
}

// ---- row a7 (cloud side of the Kabsch / PointNet path) ----------------------------------------------------------
// (a) the training loop's pairing rule, point_cloud/main.py:173-181: q_i = R_b p_i for every point of cloud b, written
//     either as (B,N,3) or already transposed to the (B,3,N) layout the network consumes (`gg = pc_out.transpose(1,2)`);
// (b) pc_normalize, point_cloud/prepare.py:51-56: subtract the bounding-box centre, divide by the box diagonal.
// One wave per cloud at a time, 12-byte nt loads with a per-cloud descriptor (lanes past the end read zeros and their
// stores are dropped by the range check).
constexpr int kCloudUnroll = 8;
typedef float f32x3 __attribute__((ext_vector_type(3)));

template <bool TRANSPOSED>
__global__ __launch_bounds__(kBlock) void k_rotate_clouds(const float *__restrict__ P, const float *__restrict__ R,
                                                          float *__restrict__ out, int64_t B, int32_t N, int per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * per_wave;
    const int nc = c0 < B ? static_cast<int>(min<int64_t>(per_wave, B - c0)) : 0;
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    for (int j = 0; j < nc; ++j) {
        const float *r = R + (c0 + j) * 9;                       // wave-uniform: scalar loads
        const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5], r6 = r[6], r7 = r[7], r8 = r[8];
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        float *ob = out + (c0 + j) * N * 3;
        const so3::rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(ob, 0, cloud_bytes, so3::kRsrcFlags);
        const so3::rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(ob, 0, static_cast<unsigned>(N) * 4u, so3::kRsrcFlags);
        const so3::rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(ob + N, 0, static_cast<unsigned>(N) * 4u, so3::kRsrcFlags);
        const so3::rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(ob + 2 * static_cast<int64_t>(N), 0, static_cast<unsigned>(N) * 4u, so3::kRsrcFlags);
        for (int i0 = 0; i0 < N; i0 += 64 * kCloudUnroll) {
            u32x3 pp[kCloudUnroll];
#pragma unroll
            for (int u = 0; u < kCloudUnroll; ++u) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, (i0 + 64 * u + lane) * 12, 0, so3::kStreamNt);
#pragma unroll
            for (int u = 0; u < kCloudUnroll; ++u) {
                const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                const float qx = fmaf(r0, px, fmaf(r1, py, r2 * pz));
                const float qy = fmaf(r3, px, fmaf(r4, py, r5 * pz));
                const float qz = fmaf(r6, px, fmaf(r7, py, r8 * pz));
                const int i = i0 + 64 * u + lane;
                if (TRANSPOSED) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(qx), rx, i * 4, 0, so3::kStreamNt);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(qy), ry, i * 4, 0, so3::kStreamNt);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(qz), rz, i * 4, 0, so3::kStreamNt);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(qx), __float_as_uint(qy), __float_as_uint(qz)}, ro, i * 12, 0, so3::kStreamNt);
                }
            }
        }
    }
}

// a7b: the pairing rule's backward.  Forward q_i = R p_i; given G in the forward's output layout ((B,N,3), or (B,3,N) when
// TRANSPOSED):  dP_i = R^T g_i,  dR = sum_i g_i p_i^T.  G is read once; P only for dR, which is accumulated as k_kabsch
// accumulates H (lane j keeps cloud j's sum, the wave stores them at the end).  N == 0 still writes dR = 0.
template <bool TRANSPOSED, bool WANT_DP, bool WANT_DR>
__global__ __launch_bounds__(kBlock) void k_rotate_clouds_bwd(const float *__restrict__ P, const float *__restrict__ R,
                                                              const float *__restrict__ G, float *__restrict__ dP,
                                                              float *__restrict__ dR, int64_t B, int32_t N, int per_wave) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * per_wave;
    if (c0 >= B) return;
    const int nc = static_cast<int>(min<int64_t>(per_wave, B - c0));
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    const unsigned row_bytes = static_cast<unsigned>(N) * 4u;
    float dr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) dr[i] = 0.f;
    for (int j = 0; j < nc; ++j) {
        float r[9];
        if (WANT_DP) {
#pragma unroll
            for (int i = 0; i < 9; ++i) r[i] = R[(c0 + j) * 9 + i];             // wave-uniform: scalar loads
        }
        const int64_t base = (c0 + j) * N * 3;
        float *gb = const_cast<float *>(G) + base;
        const so3::rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(gb, 0, cloud_bytes, so3::kRsrcFlags);
        const so3::rsrc_t rgx = __builtin_amdgcn_make_buffer_rsrc(gb, 0, row_bytes, so3::kRsrcFlags);
        const so3::rsrc_t rgy = __builtin_amdgcn_make_buffer_rsrc(gb + N, 0, row_bytes, so3::kRsrcFlags);
        const so3::rsrc_t rgz = __builtin_amdgcn_make_buffer_rsrc(gb + 2 * static_cast<int64_t>(N), 0, row_bytes, so3::kRsrcFlags);
        so3::rsrc_t rp, rdp;
        if (WANT_DR) rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + base, 0, cloud_bytes, so3::kRsrcFlags);
        if (WANT_DP) rdp = __builtin_amdgcn_make_buffer_rsrc(dP + base, 0, cloud_bytes, so3::kRsrcFlags);
        float acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = 0.f;
        for (int i0 = 0; i0 < N; i0 += 64 * kCloudUnroll) {
            f32x3 gg[kCloudUnroll];
            u32x3 pp[kCloudUnroll];
#pragma unroll
            for (int u = 0; u < kCloudUnroll; ++u) {
                const int i = i0 + 64 * u + lane;                 // lanes past the cloud's end read zeros
                if (TRANSPOSED) {
                    gg[u].x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rgx, i * 4, 0, so3::kStreamNt));
                    gg[u].y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rgy, i * 4, 0, so3::kStreamNt));
                    gg[u].z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rgz, i * 4, 0, so3::kStreamNt));
                } else {
                    const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(rg, i * 12, 0, so3::kStreamNt);
                    gg[u] = f32x3{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z)};
                }
                if (WANT_DR) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, i * 12, 0, so3::kStreamNt);
            }
#pragma unroll
            for (int u = 0; u < kCloudUnroll; ++u) {
                const float gx = gg[u].x, gy = gg[u].y, gz = gg[u].z;
                if (WANT_DP) {
                    const float x = fmaf(r[6], gz, fmaf(r[3], gy, r[0] * gx));
                    const float y = fmaf(r[7], gz, fmaf(r[4], gy, r[1] * gx));
                    const float z = fmaf(r[8], gz, fmaf(r[5], gy, r[2] * gx));
                    __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(x), __float_as_uint(y), __float_as_uint(z)}, rdp,
                                                          (i0 + 64 * u + lane) * 12, 0, so3::kStreamNt);
                }
                if (WANT_DR) {
                    const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                    acc[0] = fmaf(gx, px, acc[0]); acc[1] = fmaf(gx, py, acc[1]); acc[2] = fmaf(gx, pz, acc[2]);
                    acc[3] = fmaf(gy, px, acc[3]); acc[4] = fmaf(gy, py, acc[4]); acc[5] = fmaf(gy, pz, acc[5]);
                    acc[6] = fmaf(gz, px, acc[6]); acc[7] = fmaf(gz, py, acc[7]); acc[8] = fmaf(gz, pz, acc[8]);
                }
            }
        }
        if (WANT_DR) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const float tot = wave_allsum(acc[i]);
                dr[i] = (lane == j) ? tot : dr[i];
            }
        }
    }
    if (WANT_DR && lane < nc) {
        float *out = dR + (c0 + lane) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = dr[i];
    }
}

__device__ __forceinline__ float wave_allmax(float v) {
    v = fmaxf(v, dpp_xor1(v));
    v = fmaxf(v, dpp_xor2(v));
    v = fmaxf(v, dpp_half_mirror(v));
    v = fmaxf(v, dpp_mirror(v));
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// HOLD > 0: the whole cloud (N <= 64 * HOLD points) stays in registers between the two passes: one HBM read.
template <int HOLD>
__global__ __launch_bounds__(kBlock) void k_pc_normalize(const float *__restrict__ P, float *__restrict__ out,
                                                         float *__restrict__ centroid, float *__restrict__ scale_out,
                                                         int64_t B, int32_t N, int per_wave) {
    constexpr int kU = HOLD > 0 ? HOLD : kCloudUnroll;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * per_wave;
    const int nc = c0 < B ? static_cast<int>(min<int64_t>(per_wave, B - c0)) : 0;
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    const float inf = __builtin_huge_valf();
    for (int j = 0; j < nc; ++j) {
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        const so3::rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(out + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        // pass 1: bounding box.  Out-of-range lanes read zeros, which must not enter the box: they are masked by index.
        // fmaxf / fminf drop a NaN operand where numpy's max / min (prepare.py:52) hand it on: the last NaN coordinate a lane has seen
        // on an axis is kept beside the box (a select; a zero-filled slot is no NaN) and given back to the box after the wave's reduction.
        float hi[3] = {-inf, -inf, -inf}, lo[3] = {inf, inf, inf}, bad[3] = {0.f, 0.f, 0.f};
        u32x3 pp[kU];
        for (int i0 = 0; i0 < N; i0 += 64 * kU) {
#pragma unroll
            for (int u = 0; u < kU; ++u) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, (i0 + 64 * u + lane) * 12, 0, HOLD > 0 ? so3::kStreamNt : 0);
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const bool in = i0 + 64 * u + lane < N;
                const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                hi[0] = fmaxf(hi[0], in ? px : -inf); hi[1] = fmaxf(hi[1], in ? py : -inf); hi[2] = fmaxf(hi[2], in ? pz : -inf);
                lo[0] = fminf(lo[0], in ? px : inf);  lo[1] = fminf(lo[1], in ? py : inf);  lo[2] = fminf(lo[2], in ? pz : inf);
                bad[0] = px != px ? px : bad[0]; bad[1] = py != py ? py : bad[1]; bad[2] = pz != pz ? pz : bad[2];
            }
        }
        float c[3], ext2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool nan_k = so3::hw::any_lane(bad[k] != bad[k]);    // wave-uniform: a select on the scalar unit's condition, no branch
            const float nan = __builtin_nanf("");
            const float mx = nan_k ? nan : wave_allmax(hi[k]), mn = nan_k ? nan : -wave_allmax(-lo[k]);
            c[k] = (mx + mn) * 0.5f;                                   // prepare.py:52
            const float e = (mx - c[k]) - (mn - c[k]);                 // :54 on the centred cloud
            ext2 = fmaf(e, e, ext2);
        }
        const float sc = __builtin_amdgcn_sqrtf(ext2);
        const float inv = 1.0f / sc;
        if (lane == 0) {
            if (centroid != nullptr) { centroid[(c0 + j) * 3 + 0] = c[0]; centroid[(c0 + j) * 3 + 1] = c[1]; centroid[(c0 + j) * 3 + 2] = c[2]; }
            if (scale_out != nullptr) scale_out[c0 + j] = sc;
        }
        // pass 2: from the registers when the cloud fits, otherwise a second read (mostly served by L2 / Infinity Cache)
        for (int i0 = 0; i0 < N; i0 += 64 * kU) {
            if (HOLD == 0) {
#pragma unroll
                for (int u = 0; u < kU; ++u) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, (i0 + 64 * u + lane) * 12, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const float qx = (__uint_as_float(pp[u].x) - c[0]) * inv, qy = (__uint_as_float(pp[u].y) - c[1]) * inv,
                            qz = (__uint_as_float(pp[u].z) - c[2]) * inv;
                __builtin_amdgcn_raw_buffer_store_b96(u32x3{__float_as_uint(qx), __float_as_uint(qy), __float_as_uint(qz)}, ro,
                                                      (i0 + 64 * u + lane) * 12, 0, so3::kStreamNt);
            }
        }
    }
}

// ---- next row f6: the ADD-L1 losses that consume calculate_T_pred's output (Iterative/loss.py:10-48) ------------
// dist_b = mean_{i,c} |(T_gt p_i - T_pred p_i)_c| = mean |dR p_i + dt|,  dR = R_gt - R_pred, dt = t_gt - t_pred, and
// its gradient  dL/dR_pred[c][j] = -k sum_i sgn(d_ic) p_ij,  dL/dt_pred[c] = -k sum_i sgn(d_ic),  k = scale / (3 N),
// in one pass over the points (the K5 skeleton: one wave per sample at a time, 12-byte loads, lane j of the wave
// keeps the results of its j-th sample).  DISENT = compute_disentangled_ADD_L1_loss: the rotation term is the same
// sum with dt = 0; the translation and depth terms do not depend on the points at all -- (|dtx| + |dty|)/3 and
// |dtz|/3 -- because the two transformed clouds differ by a constant vector.
__device__ __forceinline__ float sgn_of(float d) { return __builtin_amdgcn_fmed3f(d * 0x1p127f, -1.f, 1.f); }   // -1, 0, +1

// kAddUnroll = 12-byte loads in flight per lane: 16 for large clouds (12 KB per wave, what K5 has with two arrays),
// fewer for small ones, whose zero-filled slots would only cost arithmetic.
// L2 = compute_ADD_loss (the ADD metric): the same pass with |d|_2 in place of the L1 sum and u = d / |d| (0 where d = 0) in place of
// the signs; dist_b = mean_i |d_i|, k = scale / N.  Its zero-filled slots are masked, so they contribute exactly zero.
template <bool DISENT, int kAddUnroll, bool L2 = false>
__global__ __launch_bounds__(kBlock) void k_add_l1(const float *__restrict__ Tgt, const float *__restrict__ Tpred,
                                                   const float *__restrict__ pts, float *__restrict__ dists,
                                                   double *__restrict__ loss_sum, float *__restrict__ dT, float grad_scale,
                                                   int64_t B, int32_t N, int per_wave) {
    __shared__ double red[kBlock / 64][3];
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave_in_block;
    const int64_t c0 = wave * per_wave;
    const int nc = c0 < B ? static_cast<int>(min<int64_t>(per_wave, B - c0)) : 0;
    const float inv3n = 1.0f / (3.0f * static_cast<float>(N));
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    const int slots = ((N + 64 * kAddUnroll - 1) / (64 * kAddUnroll)) * kAddUnroll;      // loads per lane and sample
    const int valid = N > lane ? (N - lane + 63) / 64 : 0;
    const float npad = static_cast<float>(slots - valid);     // zero-filled slots of this lane: each adds |dt|, sgn(dt)
    float keep[13];                                            // lane j: dist, G (9), gt (3) of sample c0 + j
    float keep_dt[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 13; ++i) keep[i] = 0.f;
    for (int j = 0; j < nc; ++j) {
        const float *tg = Tgt + (c0 + j) * 16, *tp = Tpred + (c0 + j) * 16;      // wave-uniform: scalar loads
        float dr[9], dt[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dr[3 * c + k] = tg[4 * c + k] - tp[4 * c + k];
            dt[c] = tg[4 * c + 3] - tp[4 * c + 3];
        }
        const float ax = DISENT ? 0.f : dt[0], ay = DISENT ? 0.f : dt[1], az = DISENT ? 0.f : dt[2];
        const so3::rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pts) + (c0 + j) * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        float acc[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) acc[i] = 0.f;
        for (int i0 = 0; i0 < N; i0 += 64 * kAddUnroll) {
            u32x3 pp[kAddUnroll];
#pragma unroll
            for (int u = 0; u < kAddUnroll; ++u) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rp, (i0 + 64 * u + lane) * 12, 0, so3::kStreamNt);
#pragma unroll
            for (int u = 0; u < kAddUnroll; ++u) {
                const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                const float dx = fmaf(dr[0], px, fmaf(dr[1], py, fmaf(dr[2], pz, ax)));
                const float dy = fmaf(dr[3], px, fmaf(dr[4], py, fmaf(dr[5], pz, ay)));
                const float dz = fmaf(dr[6], px, fmaf(dr[7], py, fmaf(dr[8], pz, az)));
                float sx, sy, sz;
                if (L2) {
                    const bool in = i0 + 64 * u + lane < N;
                    const float d2 = so3::pair_dist2(dx, dy, dz);
                    const float inv = in ? so3::unit_scale(d2) : 0.f;
                    acc[0] += in ? so3::hw::sqrt(d2) : 0.f;
                    sx = dx * inv; sy = dy * inv; sz = dz * inv;
                } else {
                    acc[0] += fabsf(dx) + fabsf(dy) + fabsf(dz);
                    sx = sgn_of(dx); sy = sgn_of(dy); sz = sgn_of(dz);
                }
                acc[1] = fmaf(sx, px, acc[1]); acc[2] = fmaf(sx, py, acc[2]); acc[3] = fmaf(sx, pz, acc[3]);
                acc[4] = fmaf(sy, px, acc[4]); acc[5] = fmaf(sy, py, acc[5]); acc[6] = fmaf(sy, pz, acc[6]);
                acc[7] = fmaf(sz, px, acc[7]); acc[8] = fmaf(sz, py, acc[8]); acc[9] = fmaf(sz, pz, acc[9]);
                acc[10] += sx; acc[11] += sy; acc[12] += sz;
            }
        }
        if (!DISENT && !L2) {      // take the zero-filled slots back out (they saw d = dt exactly)
            acc[0] = fmaf(-npad, fabsf(ax) + fabsf(ay) + fabsf(az), acc[0]);
            acc[10] = fmaf(-npad, sgn_of(ax), acc[10]);
            acc[11] = fmaf(-npad, sgn_of(ay), acc[11]);
            acc[12] = fmaf(-npad, sgn_of(az), acc[12]);
        }
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            const float tot = wave_allsum(acc[i]);
            keep[i] = (lane == j) ? tot : keep[i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) keep_dt[c] = (lane == j) ? dt[c] : keep_dt[c];
    }
    // lane j < nc finishes sample c0 + j
    const bool active = lane < nc;
    const float inv_n = L2 ? 1.0f / static_cast<float>(N) : inv3n;
    const float dist = keep[0] * inv_n;
    double part[3] = {0.0, 0.0, 0.0};
    if (active) {
        const int64_t b = c0 + lane;
        part[0] = dist;
        if (DISENT) {
            part[1] = (fabsf(keep_dt[0]) + fabsf(keep_dt[1])) * (1.0f / 3.0f);
            part[2] = fabsf(keep_dt[2]) * (1.0f / 3.0f);
        }
        if (dists != nullptr) dists[b] = dist;
        if (dT != nullptr) {
            const float k = -grad_scale * inv_n, kt = -grad_scale * (1.0f / 3.0f);
            float *o = dT + b * 16;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[4 * c + 0] = k * keep[1 + 3 * c]; o[4 * c + 1] = k * keep[2 + 3 * c]; o[4 * c + 2] = k * keep[3 + 3 * c];
                o[4 * c + 3] = DISENT ? kt * sgn_of(keep_dt[c]) : k * keep[10 + c];
            }
            o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
        }
    }
    if (loss_sum != nullptr) {
        constexpr int kTerms = DISENT ? 3 : 1;
#pragma unroll
        for (int t = 0; t < kTerms; ++t) {
            const double v = wave_sum(part[t]);
            if (lane == 0) red[wave_in_block][t] = v;
        }
        __syncthreads();
        if (threadIdx.x < kTerms) {
            double tot = 0.0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) tot += red[w][threadIdx.x];
            atomicAdd(loss_sum + threadIdx.x, tot);
        }
    }
}

// ---- ADD-S and the cloud diameter: the N^2 kernel -----------------------------------------------------------------------------------
// ADDS_b = (1/N) sum_i min_j |x_i - y_j|,  x = T_gt p (outer cloud), y = T_pred p (inner cloud);  diam_b = max_ij |p_i - p_j|.
// One work item = kBlock * U outer points of one cloud (a cloud is split over workgroups when B is small); a lane keeps U outer points
// in registers.  The inner cloud goes through tile_search, posed once per work item by the same pose_point as the outer points; one
// broadcast read feeds U pairs.  A copy of the tile's last point in the padding never beats the original (strict <, the minimum and
// the maximum are unchanged).
// The per-point result sqrt(best) goes to point_dist (B,N); k_add_s_rows finishes the rows in a fixed order.  No atomics anywhere.
constexpr int kAddsTile = 1024;         // 16 KB of LDS per workgroup
constexpr int kAddsUnroll = 8;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

// The tiled broadcast search of k_add_s and k_chamfer_fwd: the workgroup walks a target cloud of `len` points through LDS in tiles of
// kAddsTile float4, fetch(j) gives target point j for the tile.  A tile's tail is padded to kAddsUnroll with copies of its last point,
// which never beat the original (strict <; the minimum and the maximum are unchanged).  Every thread then visits every point of the
// tile in ascending order with the U points (x, y, z) it keeps: add_s_pair leaves the best squared distance and (WANT_INDEX) its
// index, t0 + k + kk, the point's index in the cloud, not in the tile.  The read is the same address in every lane, a broadcast, and
// volatile keeps the unused fourth dword in the load: one ds_read_b128 (4 LDS cycles) where the compiler would pick ds_read_b96 (8),
// which one point per lane cannot hide.  Two barriers per tile: the first also covers whatever the caller kept in the tile after the
// previous search (item_record).  The search runs in copies of best and idx, as owner_scan's chain does: through the caller's arrays
// k_chamfer_fwd<., 4> gets the registers of two slots exchanged and its pair loop scheduled around them.
// k_icp_step and k_three_nn keep this loop written out: called from them, the helper leaves k_icp_step<false, false, false, 4> with an
// s_nop inside the pair loop and k_three_nn with its selects in another order (profiles/tile_search_refactor_isa.txt).
// Who uses what: tile_search -- k_add_s, k_icp_plane_step, chamfer_search (both Chamfer forwards); item_record -- k_icp_step,
// k_icp_plane_step, chamfer_search; owner_scan -- k_chamfer_bwd, k_chamfer_normals_bwd, k_knn_bwd's dY; two_way_item -- chamfer_search,
// k_chamfer_bwd, k_chamfer_normals_bwd; record_sum / pose_entry / store_pose -- both ICP finish kernels (profiles/cloud_skeletons_isa.txt).
template <bool WANT_INDEX, bool DIAMETER, int U, class Fetch>
__device__ __forceinline__ void tile_search(float4 *tile, int tid, int len, Fetch fetch, const float (&x)[U], const float (&y)[U], const float (&z)[U],
                                            float (&best)[U], int (&idx)[U]) {
    float d[U];
    int n[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { d[u] = best[u]; n[u] = idx[u]; }
    for (int t0 = 0; t0 < len; t0 += kAddsTile) {
        const int cnt = min(kAddsTile, len - t0);
        const int cntp = (cnt + kAddsUnroll - 1) / kAddsUnroll * kAddsUnroll;      // <= kAddsTile
        __syncthreads();                                                         // the previous tile has been read
        for (int k = tid; k < cntp; k += kBlock) tile[k] = fetch(t0 + min(k, cnt - 1));
        __syncthreads();
        for (int k = 0; k < cntp; k += kAddsUnroll) {
#pragma unroll
            for (int kk = 0; kk < kAddsUnroll; ++kk) {
                const f32x4 q = *(const volatile lds_f32x4 *)(&tile[k + kk]);
#pragma unroll
                for (int u = 0; u < U; ++u) so3::add_s_pair<WANT_INDEX, DIAMETER>(x[u], y[u], z[u], q.x, q.y, q.z, t0 + k + kk, d[u], n[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { best[u] = d[u]; idx[u] = n[u]; }
}
__device__ __forceinline__ float4 tile_point(const float *cloud, int j) { return make_float4(cloud[j * 3 + 0], cloud[j * 3 + 1], cloud[j * 3 + 2], 0.f); }

// A work item's record of W floats in wave order: lane k < W of every wave brings its wave's sum k, the waves' sums go through the
// tile the search has finished with, and thread k adds entry k in wave order and writes out[k].
template <int W>
__device__ __forceinline__ void item_record(float4 *tile, int tid, float mine, float *out) {
    float *red = reinterpret_cast<float *>(tile);
    const int lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                         // every wave has left the last tile
    if (lane < W) red[wave * W + lane] = mine;
    __syncthreads();
    if (tid < W) {
        float v = red[tid];
#pragma unroll
        for (int wv = 1; wv < kBlock / 64; ++wv) v += red[wv * W + tid];          // in wave order
        out[tid] = v;
    }
}

template <bool WANT_INDEX, bool DIAMETER, int U>
__global__ __launch_bounds__(kBlock) void k_add_s(const float *__restrict__ Tgt, const float *__restrict__ Tpred, const float *__restrict__ pts,
                                                  float *__restrict__ point_dist, int32_t *__restrict__ nearest, int64_t B, int32_t N,
                                                  int32_t chunks) {
    __shared__ float4 tile[kAddsTile];
    const int tid = threadIdx.x;
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int i_base = static_cast<int>(item - b * chunks) * (kBlock * U);
        const float *cloud = pts + b * N * 3;
        float mg[12], mp[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {                       // wave-uniform: scalar loads
            mg[k] = DIAMETER ? 0.f : Tgt[b * 16 + k];
            mp[k] = DIAMETER ? 0.f : Tpred[b * 16 + k];
        }
        float x[U], y[U], z[U], best[U];
        int idx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(i_base + u * kBlock + tid, N - 1);             // a slot beyond the cloud repeats its last point; not stored
            const float px = cloud[i * 3 + 0], py = cloud[i * 3 + 1], pz = cloud[i * 3 + 2];
            if (DIAMETER) { x[u] = px; y[u] = py; z[u] = pz; }
            else so3::pose_point(mg, px, py, pz, x[u], y[u], z[u]);
            best[u] = DIAMETER ? 0.f : __builtin_huge_valf();
            idx[u] = 0;
        }
        tile_search<WANT_INDEX, DIAMETER>(tile, tid, N,
            [&](int j) {
                float4 q = tile_point(cloud, j);
                if (!DIAMETER) so3::pose_point(mp, q.x, q.y, q.z, q.x, q.y, q.z);
                return q;
            }, x, y, z, best, idx);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i_base + u * kBlock + tid;
            if (i < N) {
                point_dist[b * N + i] = so3::hw::sqrt(best[u]);
                if (WANT_INDEX) nearest[b * N + i] = min(idx[u], N - 1);
            }
        }
    }
}

// The rows of k_add_s's (B,N) result, one wave per sample at a time, in a fixed order: lane-strided float64 partial sums (or float
// maxima), a butterfly, out[b] = float(sum / N) (or the maximum).  With ONE workgroup it also leaves sum_b out[b] in total[0].
template <bool MAX>
__global__ __launch_bounds__(kBlock) void k_add_s_rows(const float *__restrict__ work, float *__restrict__ out, double *__restrict__ total,
                                                       int64_t B, int32_t N) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    double mine = 0.0;
    for (int64_t b = wave; b < B; b += nwaves) {
        const float *row = work + b * N;
        float r;
        if (MAX) {
            float m = 0.f;
            for (int i = lane; i < N; i += 64) m = fmaxf(m, row[i]);
            r = wave_allmax(m);
        } else {
            double acc = 0.0;
            for (int i = lane; i < N; i += 64) acc += static_cast<double>(row[i]);
            r = static_cast<float>(wave_sum(acc) / static_cast<double>(N));          // the butterfly leaves the same bits in every lane
        }
        if (out != nullptr && lane == 0) out[b] = r;
        mine += static_cast<double>(r);
    }
    if (total != nullptr) {                    // gridDim.x == 1
        const double t = block_sum(lane == 0 ? mine : 0.0, red);
        if (threadIdx.x == 0) total[0] = t;
    }
}

// sum_b v[b] in float64 by one workgroup, in a fixed order
__global__ __launch_bounds__(kBlock) void k_sum_f32_to_f64(const float *__restrict__ v, double *__restrict__ total, int64_t B) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kBlock) acc += static_cast<double>(v[b]);
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) total[0] = t;
}

// ---- ADD / ADD-L1 / MSSD up to a symmetry group (so3_sym_add_f32) -----------------------------------------------------------------
// dist_b = min_k stat(T_gt, T_pred S_k), the smallest minimising k, and (GRAD) the selected branch's gradient w.r.t. T_pred, in one
// launch.  k_add_l1's skeleton: one wave per sample at a time, 12-byte buffer loads, poses and table entries wave-uniform.  A sweep of
// 64 * kU points is loaded into registers once and every candidate is walked over it in a wave-uniform loop: D_k = R_gt - R_pred S_k
// from scalar loads, the lanes' partial statistic, one butterfly per candidate; LANE k keeps candidate k's statistic across the sweeps
// (K <= 64), so no per-lane array is indexed by k.  The minimum and its first index are one more butterfly and a ballot.  The gradient
// phase recomputes D_k* and runs k_add_l1's twelve sums over the points -- still in registers when the cloud is one sweep, read again
// (L2) when it is longer.  kU < 16 is only launched for clouds that fit 64 * kU points: a sweep is kSymAddSweep points for every N,
// so the order of a row's sum depends on N alone.
// `total` (one workgroup only): sum_b dist_b in float64, in the order the four waves met the rows.
template <int MODE> __device__ __forceinline__ float sym_add_wave_join(float v) {      // wave_allsum's partners
    v = so3::sym_add_join<MODE>(v, dpp_xor1(v));
    v = so3::sym_add_join<MODE>(v, dpp_xor2(v));
    v = so3::sym_add_join<MODE>(v, dpp_half_mirror(v));
    v = so3::sym_add_join<MODE>(v, dpp_mirror(v));
    v = so3::sym_add_join<MODE>(v, __shfl_xor(v, 16, 64));
    v = so3::sym_add_join<MODE>(v, __shfl_xor(v, 32, 64));
    return v;
}
template <int MODE, bool GRAD, int kU>
__global__ __launch_bounds__(kBlock) void k_sym_add(const float *__restrict__ Tgt, const float *__restrict__ Tpred, const float *__restrict__ pts,
                                                    const float *__restrict__ S, const int32_t *__restrict__ class_id, int32_t C, int32_t K,
                                                    float *__restrict__ dists, int32_t *__restrict__ index, double *__restrict__ total,
                                                    float *__restrict__ dT, float grad_scale, int64_t B, int32_t N) {
    static_assert(64 * kU <= so3::kSymAddSweep && !(GRAD && MODE == so3::kSymAddMax), "");
    __shared__ double red[4];
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const unsigned cloud_bytes = static_cast<unsigned>(N) * 12u;
    const float nan = __int_as_float(0x7fc00000);
    double mine = 0.0;
    for (int64_t b = wave; b < B; b += nwaves) {
        const float *tg = Tgt + b * 16, *tp = Tpred + b * 16;                   // wave-uniform: scalar loads
        float rg[9], rp[9], dt[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { rg[3 * c + j] = tg[4 * c + j]; rp[3 * c + j] = tp[4 * c + j]; }
            dt[c] = tg[4 * c + 3] - tp[4 * c + 3];
        }
        const int cls = class_id != nullptr ? class_id[b] : 0;
        const bool bad = static_cast<unsigned>(cls) >= static_cast<unsigned>(C);
        const float *tab = S + static_cast<int64_t>(bad ? 0 : cls) * K * 9;
        const so3::rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pts) + b * N * 3, 0, cloud_bytes, so3::kRsrcFlags);
        u32x3 pp[kU];
        float stat = 0.f;                                                        // lane k: candidate k
        for (int i0 = 0; i0 < N; i0 += 64 * kU) {
#pragma unroll
            for (int u = 0; u < kU; ++u) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (i0 + 64 * u + lane) * 12, 0, 0);
            for (int k = 0; k < K; ++k) {
                float s[9], d[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) s[i] = tab[k * 9 + i];
                so3::sym_add_difference(rg, rp, s, k, d);
                float part = 0.f;
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    float dx, dy, dz;
                    so3::sym_add_residual(d, dt, __uint_as_float(pp[u].x), __uint_as_float(pp[u].y), __uint_as_float(pp[u].z), dx, dy, dz);
                    const float term = so3::sym_add_term<MODE>(dx, dy, dz);
                    part = so3::sym_add_join<MODE>(part, i0 + 64 * u + lane < N ? term : 0.f);      // a zero-filled slot adds exactly 0
                }
                const float tot = sym_add_wave_join<MODE>(part);
                stat = lane == k ? so3::sym_add_join<MODE>(stat, tot) : stat;
            }
        }
        // min_k by strict < in ascending k: a NaN candidate never wins, a NaN candidate 0 is never beaten
        const float val = lane < K ? so3::sym_add_finish<MODE>(stat, N) : __builtin_huge_valf();
        const float v0 = __builtin_amdgcn_readfirstlane(val);
        float best = -wave_allmax(-val);
        int kb = __builtin_ctzll(__builtin_amdgcn_ballot_w64(val == best) | (1ull << 63));
        if (v0 != v0) { best = v0; kb = 0; }
        if (bad) { best = nan; }
        if (lane == 0) {
            if (dists != nullptr) dists[b] = best;
            if (index != nullptr) index[b] = bad ? -1 : kb;
        }
        mine += static_cast<double>(best);
        if (GRAD) {
            float s[9], d[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) s[i] = tab[kb * 9 + i];
            so3::sym_add_difference(rg, rp, s, kb, d);
            float acc[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] = 0.f;
            for (int i0 = 0; i0 < N; i0 += 64 * kU) {
                if (N > 64 * kU) {                                               // more than one sweep: the registers hold the last one
#pragma unroll
                    for (int u = 0; u < kU; ++u) pp[u] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (i0 + 64 * u + lane) * 12, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const float px = __uint_as_float(pp[u].x), py = __uint_as_float(pp[u].y), pz = __uint_as_float(pp[u].z);
                    const bool in = i0 + 64 * u + lane < N;
                    float dx, dy, dz, ux, uy, uz;
                    so3::sym_add_residual(d, dt, px, py, pz, dx, dy, dz);
                    so3::sym_add_direction<MODE>(dx, dy, dz, ux, uy, uz);
                    ux = in ? ux : 0.f; uy = in ? uy : 0.f; uz = in ? uz : 0.f;
                    acc[0] = fmaf(ux, px, acc[0]); acc[1] = fmaf(ux, py, acc[1]); acc[2] = fmaf(ux, pz, acc[2]);
                    acc[3] = fmaf(uy, px, acc[3]); acc[4] = fmaf(uy, py, acc[4]); acc[5] = fmaf(uy, pz, acc[5]);
                    acc[6] = fmaf(uz, px, acc[6]); acc[7] = fmaf(uz, py, acc[7]); acc[8] = fmaf(uz, pz, acc[8]);
                    acc[9] += ux; acc[10] += uy; acc[11] += uz;
                }
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] = wave_allsum(acc[i]);
            float g[9], gs[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) g[i] = acc[i];
            so3::sym_add_rotate_back(g, s, kb, gs);
            if (lane == 0) {
                const float c = bad ? nan : -grad_scale * (MODE == so3::kSymAddL1 ? 1.0f / (3.0f * static_cast<float>(N)) : 1.0f / static_cast<float>(N));
                float *o = dT + b * 16;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    o[4 * r + 0] = c * gs[3 * r + 0]; o[4 * r + 1] = c * gs[3 * r + 1]; o[4 * r + 2] = c * gs[3 * r + 2];
                    o[4 * r + 3] = c * acc[9 + r];
                }
                o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
            }
        }
    }
    if (total != nullptr) {                    // gridDim.x == 1
        const double t = block_sum(lane == 0 ? mine : 0.0, red);
        if (threadIdx.x == 0) total[0] = t;
    }
}

// ADD-S backward through the stored indices: with e_i = x_i - y_nn(i), u_i = e_i / |e_i| (0 where e_i = 0),
// dL/dR_pred = -k sum_i u_i p_nn(i)^T,  dL/dt_pred = -k sum_i u_i,  k = grad_scale * grad_rows[b] / N.  One pass over (B,N), one wave per
// sample at a time (the k_add_l1 skeleton); an index outside [0, N) is clamped, so a bad index buffer cannot read out of bounds.
__global__ __launch_bounds__(kBlock) void k_add_s_bwd(const float *__restrict__ Tgt, const float *__restrict__ Tpred, const float *__restrict__ pts,
                                                      const int32_t *__restrict__ nearest, const float *__restrict__ grad_rows, float grad_scale,
                                                      float *__restrict__ dT, int64_t B, int32_t N) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    for (int64_t b = wave; b < B; b += nwaves) {
        float mg[12], mp[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { mg[k] = Tgt[b * 16 + k]; mp[k] = Tpred[b * 16 + k]; }
        const float *cloud = pts + b * N * 3;
        const int32_t *nn = nearest + b * N;
        float acc[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] = 0.f;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const bool in = i0 + lane < N;
            const int i = min(i0 + lane, N - 1);
            const int j = min(max(nn[i], 0), N - 1);
            float ex, ey, ez, qx, qy, qz;
            so3::pose_point(mg, cloud[i * 3 + 0], cloud[i * 3 + 1], cloud[i * 3 + 2], ex, ey, ez);
            const float px = cloud[j * 3 + 0], py = cloud[j * 3 + 1], pz = cloud[j * 3 + 2];
            so3::pose_point(mp, px, py, pz, qx, qy, qz);
            ex -= qx; ey -= qy; ez -= qz;
            const float inv = in ? so3::unit_scale(so3::pair_dist2(ex, ey, ez)) : 0.f;
            const float ux = ex * inv, uy = ey * inv, uz = ez * inv;
            acc[0] = fmaf(ux, px, acc[0]); acc[1] = fmaf(ux, py, acc[1]); acc[2] = fmaf(ux, pz, acc[2]); acc[3] += ux;
            acc[4] = fmaf(uy, px, acc[4]); acc[5] = fmaf(uy, py, acc[5]); acc[6] = fmaf(uy, pz, acc[6]); acc[7] += uy;
            acc[8] = fmaf(uz, px, acc[8]); acc[9] = fmaf(uz, py, acc[9]); acc[10] = fmaf(uz, pz, acc[10]); acc[11] += uz;
        }
        const float k = -grad_scale * (grad_rows != nullptr ? grad_rows[b] : 1.f) / static_cast<float>(N);
        float mine = 0.f;                                    // lane l < 12 keeps entry l of the top three rows
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const float tot = wave_allsum(acc[e]);
            mine = lane == e ? tot : mine;
        }
        if (lane < 16) dT[b * 16 + lane] = lane < 12 ? k * mine : 0.f;
    }
}

// ---- ICP: nearest neighbours between two clouds, fused with rigid_align's sums ------------------------------------------------------
// k_icp_step is k_add_s over two DIFFERENT clouds: one work item = kBlock * U source points of one cloud, the target cloud (M points,
// its own or one shared by the batch) goes through LDS raw, in tile_search's loop written out.  The source points are posed by the current pose (pose ==
// nullptr: the identity, nothing is multiplied); distances come from coordinate differences.  SUMS = false is nearest_neighbors: dist
// and nearest are all it writes.  SUMS = true is one ICP iteration's first half: after the search a lane gathers q_j(i) (12 B per
// point, an L2 hit), trims its weight and adds the point to rigid_align's sixteen pivot-relative sums (of the UNPOSED p_i), sum w' d^2
// and the inlier count; wave_allsum, then item_record leaves one record per work item in rec[b][chunk][.].  k_icp_finish adds a
// cloud's records in chunk order and writes the next pose.  No atomics anywhere: the same inputs give the same bits.
template <bool WEIGHTED, bool TRIMMED, bool SUMS, int U>
__global__ __launch_bounds__(kBlock) void k_icp_step(const float *__restrict__ P, const float *__restrict__ Q, int64_t q_stride,
                                                     const float *__restrict__ Wt, const float *__restrict__ pose, float max_distance,
                                                     float *__restrict__ rec, float *__restrict__ dist, int32_t *__restrict__ nearest,
                                                     int64_t B, int32_t N, int32_t M, int32_t chunks) {
    static_assert(kBlock == so3::kIcpBlock, "the host model's chunking");
    __shared__ float4 tile[kAddsTile];
    const int tid = threadIdx.x;
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int chunk = static_cast<int>(item - b * chunks);
        const int i_base = chunk * (kBlock * U);
        const float *src = P + b * N * 3, *tgt = Q + b * q_stride;
        float m[12];
        if (pose != nullptr) {
#pragma unroll
            for (int k = 0; k < 12; ++k) m[k] = pose[b * 12 + k];          // wave-uniform: scalar loads
        }
        float x[U], y[U], z[U], best[U];
        int idx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(i_base + u * kBlock + tid, N - 1);             // a slot beyond the cloud repeats its last point; weight 0, not stored
            const float px = src[i * 3 + 0], py = src[i * 3 + 1], pz = src[i * 3 + 2];
            if (pose != nullptr) so3::pose_point(m, px, py, pz, x[u], y[u], z[u]);
            else { x[u] = px; y[u] = py; z[u] = pz; }
            best[u] = __builtin_huge_valf();
            idx[u] = 0;
        }
        for (int t0 = 0; t0 < M; t0 += kAddsTile) {
            const int cnt = min(kAddsTile, M - t0);
            const int cntp = (cnt + kAddsUnroll - 1) / kAddsUnroll * kAddsUnroll;      // <= kAddsTile
            __syncthreads();                                                         // the previous tile (and the waves' sums in it) has been read
            for (int k = tid; k < cntp; k += kBlock) {
                const int j = t0 + min(k, cnt - 1);
                float4 q;
                q.x = tgt[j * 3 + 0]; q.y = tgt[j * 3 + 1]; q.z = tgt[j * 3 + 2]; q.w = 0.f;
                tile[k] = q;
            }
            __syncthreads();
            for (int k = 0; k < cntp; k += kAddsUnroll) {
#pragma unroll
                for (int kk = 0; kk < kAddsUnroll; ++kk) {
                    const f32x4 q = *(const volatile lds_f32x4 *)(&tile[k + kk]);     // tile_search: the ds_read_b128 broadcast
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        so3::add_s_pair<true, false>(x[u], y[u], z[u], q.x, q.y, q.z, t0 + k + kk, best[u], idx[u]);
                }
            }
        }
        float acc[so3::kIcpSums];
        float p0[3], q0[3];
        if (SUMS) {
#pragma unroll
            for (int k = 0; k < so3::kIcpSums; ++k) acc[k] = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { p0[k] = src[k]; q0[k] = tgt[k]; }             // the pivot: wave-uniform addresses
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i_base + u * kBlock + tid;
            const bool in = i < N;
            const int j = min(idx[u], M - 1);
            const float d = so3::hw::sqrt(best[u]);
            if (in) {
                if (dist != nullptr) dist[b * N + i] = d;
                if (nearest != nullptr) nearest[b * N + i] = j;
            }
            if (SUMS) {
                const int ic = min(i, N - 1);
                const float w = in ? (WEIGHTED ? Wt[b * N + ic] : 1.f) : 0.f;
                so3::icp_accumulate<TRIMMED>(w, best[u], d, max_distance, src[ic * 3 + 0] - p0[0], src[ic * 3 + 1] - p0[1], src[ic * 3 + 2] - p0[2],
                                             tgt[j * 3 + 0] - q0[0], tgt[j * 3 + 1] - q0[1], tgt[j * 3 + 2] - q0[2], acc);
            }
        }
        if (SUMS) {
            const int lane = tid & 63;
            float mine = 0.f;                                    // lane k < kIcpSums keeps sum k of its wave, the record's padding 0
#pragma unroll
            for (int k = 0; k < so3::kIcpSums; ++k) {
                const float tot = wave_allsum(acc[k]);
                mine = lane == k ? tot : mine;
            }
            item_record<so3::kIcpRecord>(tile, tid, lane < so3::kIcpSums ? mine : 0.f, rec + (b * chunks + chunk) * so3::kIcpRecord);
        }
    }
}

// What the finish kernels of both ICPs share.  record_sum: lane k < W adds entry k of a cloud's records in chunk order (the other lanes
// keep 0).  pose_entry: entry k of the (3,4) pose a cloud starts an iteration from -- prev == nullptr is the identity.  store_pose:
// lanes 0..11 each hold one entry of the new pose, write it to next (when given) and scatter it to the caller's R | T (when given).
template <int W> __device__ __forceinline__ float record_sum(const float *r, int lane, int chunks) {
    float v = 0.f;
    if (lane < W) {
        for (int c = 0; c < chunks; ++c) v += r[c * W + lane];
    }
    return v;
}
__device__ __forceinline__ float pose_entry(const float *prev, int64_t at, int k) { return prev != nullptr ? prev[at] : ((k % 5) == 0 ? 1.f : 0.f); }
__device__ __forceinline__ void scatter_pose(float *R, float *T, int64_t b, int k, float v) {
    const int c = k >> 2, j = k & 3;
    if (j < 3) R[b * 9 + 3 * c + j] = v; else T[b * 3 + c] = v;
}
__device__ __forceinline__ void store_pose(int lane, const float (&mn)[12], float *next, float *R, float *T, int64_t b) {
    float out = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) out = lane == k ? mn[k] : out;
    if (lane < 12) {
        next[b * 12 + lane] = out;
        if (R != nullptr) scatter_pose(R, T, b, lane, out);
    }
}

// One wave per cloud.  Lane k < kIcpRecord adds entry k of the cloud's records in chunk order; the sums are then broadcast and every
// lane finishes the same cloud (icp_finish: align_finish, the projection, align_translation), lane 0..11 write the next pose.
// prev == nullptr: the iteration started from the identity.  R, t (the caller's results) are written when given: the last iteration.
__global__ __launch_bounds__(kBlock) void k_icp_finish(const float *__restrict__ P, const float *__restrict__ Q, int64_t q_stride,
                                                       const float *__restrict__ rec, const float *__restrict__ prev, float *__restrict__ next,
                                                       float *__restrict__ R, float *__restrict__ T, float *__restrict__ rmse,
                                                       int32_t *__restrict__ inliers, int64_t B, int32_t N, int32_t chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    for (int64_t b = wave; b < B; b += nwaves) {
        const float v = record_sum<so3::kIcpRecord>(rec + b * chunks * so3::kIcpRecord, lane, chunks);
        float s[so3::kIcpSums], p0[3], q0[3], mp[12], mn[12], e, cnt;
#pragma unroll
        for (int k = 0; k < so3::kIcpSums; ++k) s[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
#pragma unroll
        for (int k = 0; k < 3; ++k) { p0[k] = P[b * N * 3 + k]; q0[k] = Q[b * q_stride + k]; }
#pragma unroll
        for (int k = 0; k < 12; ++k) mp[k] = pose_entry(prev, b * 12 + k, k);
        so3::icp_finish(s, p0, q0, mp, mn, e, cnt);
        store_pose(lane, mn, next, R, T, b);
        if (lane == 0) {
            if (rmse != nullptr) rmse[b] = e;
            if (inliers != nullptr) inliers[b] = static_cast<int32_t>(cnt);
        }
    }
}

// iterations == 0: the initial pose is the result
__global__ __launch_bounds__(kBlock) void k_icp_initial_pose(const float *__restrict__ init, float *__restrict__ R, float *__restrict__ T, int64_t B) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= B * 12) return;
    const int64_t b = e / 12;
    const int k = static_cast<int>(e - b * 12);
    scatter_pose(R, T, b, k, pose_entry(init, e, k));
}

// ---- point-to-plane ICP: k_icp_step's search, then the 31 sums of the Gauss-Newton system over the target's normals ----------------
// The search is k_icp_step's through tile_search (the same add_s_pair in the same order: the same nearest and dist bits).  The 31
// accumulators are declared after it, so the pair loop holds what k_icp_step's holds.  Per point the epilogue gathers q_j and n_j
// (12 B each, L2 hits) and REUSES the posed x_i the search kept: 3 U registers stay live past the loop instead of 3 reloads and 9 FMAs
// per point, and x_i - c, x_i - q_j are then formed from the very bits the search compared.  c = the posed p_0, wave-uniform.
// wave_allsum per sum, item_record<32> through the tile: one record per work item in rec[b][chunk][.], no atomics.
// It shares no helper with k_icp_step: a common prologue (pose load, U posed points) flipped the polarity of every k_icp_step's
// pose != nullptr branches, a common epilogue (wave_allsum per sum, item_record) rescheduled 800-1400 lines of this kernel.
template <bool WEIGHTED, bool TRIMMED, int U>
__global__ __launch_bounds__(kBlock) void k_icp_plane_step(const float *__restrict__ P, const float *__restrict__ Q,
                                                           const float *__restrict__ Nrm, int64_t q_stride, const float *__restrict__ Wt,
                                                           const float *__restrict__ pose, float max_distance, float *__restrict__ rec,
                                                           float *__restrict__ dist, int32_t *__restrict__ nearest, int64_t B, int32_t N,
                                                           int32_t M, int32_t chunks) {
    static_assert(kBlock == so3::kIcpBlock, "the host model's chunking");
    __shared__ float4 tile[kAddsTile];
    const int tid = threadIdx.x;
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int chunk = static_cast<int>(item - b * chunks);
        const int i_base = chunk * (kBlock * U);
        const float *src = P + b * N * 3, *tgt = Q + b * q_stride, *nrm = Nrm + b * q_stride;
        float m[12];
        if (pose != nullptr) {
#pragma unroll
            for (int k = 0; k < 12; ++k) m[k] = pose[b * 12 + k];          // wave-uniform: scalar loads
        }
        float x[U], y[U], z[U], best[U];
        int idx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(i_base + u * kBlock + tid, N - 1);             // a slot beyond the cloud repeats its last point; weight 0, not stored
            const float px = src[i * 3 + 0], py = src[i * 3 + 1], pz = src[i * 3 + 2];
            if (pose != nullptr) so3::pose_point(m, px, py, pz, x[u], y[u], z[u]);
            else { x[u] = px; y[u] = py; z[u] = pz; }
            best[u] = __builtin_huge_valf();
            idx[u] = 0;
        }
        tile_search<true, false, U>(tile, tid, M, [&](int j) { return tile_point(tgt, j); }, x, y, z, best, idx);
        float c[3] = {src[0], src[1], src[2]};                               // the pivot: the posed first source point, wave-uniform
        if (pose != nullptr) so3::pose_point(m, src[0], src[1], src[2], c[0], c[1], c[2]);
        float acc[so3::kPlaneSums];
#pragma unroll
        for (int k = 0; k < so3::kPlaneSums; ++k) acc[k] = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i_base + u * kBlock + tid;
            const bool in = i < N;
            const int j = min(idx[u], M - 1);
            const float d = so3::hw::sqrt(best[u]);
            if (in) {
                if (dist != nullptr) dist[b * N + i] = d;
                if (nearest != nullptr) nearest[b * N + i] = j;
            }
            const float w = in ? (WEIGHTED ? Wt[b * N + min(i, N - 1)] : 1.f) : 0.f;
            so3::plane_accumulate<TRIMMED>(w, best[u], d, max_distance, x[u] - c[0], y[u] - c[1], z[u] - c[2], x[u] - tgt[j * 3 + 0],
                                           y[u] - tgt[j * 3 + 1], z[u] - tgt[j * 3 + 2], nrm[j * 3 + 0], nrm[j * 3 + 1], nrm[j * 3 + 2], acc);
        }
        const int lane = tid & 63;
        float mine = 0.f;                                        // lane k < kPlaneSums keeps sum k of its wave, the record's padding 0
#pragma unroll
        for (int k = 0; k < so3::kPlaneSums; ++k) {
            const float tot = wave_allsum(acc[k]);
            mine = lane == k ? tot : mine;
        }
        item_record<so3::kPlaneRecord>(tile, tid, lane < so3::kPlaneSums ? mine : 0.f, rec + (b * chunks + chunk) * so3::kPlaneRecord);
    }
}

// One wave per cloud.  Lane k < kPlaneRecord adds entry k of the cloud's records in chunk order; the sums are broadcast by readlane and
// every lane runs the same solve (plane_finish: the damped Cholesky, the Cayley retraction, the projection); lanes 0..11 write the next
// pose, lane 0 the iteration's figures.  prev == nullptr: the iteration started from the identity.  R, T when given: the last iteration.
__global__ __launch_bounds__(kBlock) void k_icp_plane_finish(const float *__restrict__ P, const float *__restrict__ rec,
                                                             const float *__restrict__ prev, float damping, float *__restrict__ next,
                                                             float *__restrict__ R, float *__restrict__ T, float *__restrict__ rmse,
                                                             float *__restrict__ rmse_point, int32_t *__restrict__ inliers,
                                                             int32_t *__restrict__ solved, int64_t B, int32_t N, int32_t chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    for (int64_t b = wave; b < B; b += nwaves) {
        const float v = record_sum<so3::kPlaneRecord>(rec + b * chunks * so3::kPlaneRecord, lane, chunks);
        float s[so3::kPlaneSums], c[3], mp[12], mn[12], e, ep, cnt;
        bool ok;
#pragma unroll
        for (int k = 0; k < so3::kPlaneSums; ++k) s[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
#pragma unroll
        for (int k = 0; k < 12; ++k) mp[k] = pose_entry(prev, b * 12 + k, k);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = P[b * N * 3 + k];
        if (prev != nullptr) so3::pose_point(mp, P[b * N * 3 + 0], P[b * N * 3 + 1], P[b * N * 3 + 2], c[0], c[1], c[2]);
        so3::plane_finish(s, c, mp, damping, mn, e, ep, cnt, ok);
        store_pose(lane, mn, next, R, T, b);
        if (lane == 0) {
            if (rmse != nullptr) rmse[b] = e;
            if (rmse_point != nullptr) rmse_point[b] = ep;
            if (inliers != nullptr) inliers[b] = static_cast<int32_t>(cnt);
            if (solved != nullptr) solved[b] = ok ? 1 : 0;
        }
    }
}

// ---- Chamfer distance: both searches in one launch, both gradients in one gather ---------------------------------------------------
// k_chamfer_fwd is k_icp_step<.., SUMS = false, U> over the work items of BOTH directions: a cloud has chunks_x items that search Y
// for kBlock * U points of X, then chunks_y items that search X for points of Y (chunks_y = 0: x direction only).  The clouds are
// ragged: a cloud uses its first n_b / m_b points (wave-uniform, scalar loads), tile_search runs to the target's own length, slots
// past the source's length read dist 0 and nearest -1.  A work item leaves the sum of its points' terms in rec[item]: lane-wise in
// slot order, wave_allsum, item_record.  k_chamfer_rows adds a cloud's records in chunk order in float64 and WRITES rows (B,2) = the
// two directions' means.  No atomics, no zero-fill.
//
// One work item of a two-direction kernel (the Chamfer forwards, the gather backwards): of a cloud's chunks_x + chunks_y items the
// first chunks_x serve the x direction -- X's points search or own, Y's are searched or hit -- the others the y direction (rev: the
// roles exchanged).  two_way_lengths reads the cloud's ragged lengths, wave-uniform scalar loads; the gather backwards call it after
// their early exit.
struct TwoWayItem {
    int64_t b;
    bool rev;
    int chunk;                                   // within its direction
    int32_t full, qfull, len_p, len_q;           // the own and the other cloud's padded extents and live lengths
};
__device__ __forceinline__ TwoWayItem two_way_item(int64_t item, int per, int32_t chunks_x, int32_t N, int32_t M) {
    TwoWayItem it;
    it.b = item / per;
    const int c = static_cast<int>(item - it.b * per);
    it.rev = c >= chunks_x;
    it.chunk = it.rev ? c - chunks_x : c;
    it.full = it.rev ? M : N; it.qfull = it.rev ? N : M;
    return it;
}
__device__ __forceinline__ void two_way_lengths(TwoWayItem &it, const int32_t *x_len, const int32_t *y_len, int32_t N, int32_t M) {
    const int32_t nb = so3::chamfer_length(x_len, it.b, N), mb = so3::chamfer_length(y_len, it.b, M);
    it.len_p = it.rev ? mb : nb; it.len_q = it.rev ? nb : mb;
}

// The work-item loop of both Chamfer forwards.  NORMALS adds k_chamfer_normals_fwd's epilogue per kept slot and a second lane sum; the
// record is then two floats (sum of e, sum of t), item_record<2>, whose entry 0 adds the waves' sums in item_record<1>'s order.
template <bool SQUARED, int U, bool NORMALS>
__device__ __forceinline__ void chamfer_search(float4 *tile, const float *X, const float *Y, const float *NX, const float *NY, const int32_t *x_len,
                                               const int32_t *y_len, float *dist_x, int32_t *nearest_x, float *dist_y, int32_t *nearest_y,
                                               float *term_x, float *term_y, float *rec, int32_t signed_cos, int64_t B, int32_t N, int32_t M,
                                               int32_t chunks_x, int32_t chunks_y) {
    static_assert(kBlock == so3::kIcpBlock, "the host model's chunking");
    constexpr int W = NORMALS ? 2 : 1;
    const int tid = threadIdx.x;
    const int per = chunks_x + chunks_y;
    const int64_t items = B * per;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        TwoWayItem it = two_way_item(item, per, chunks_x, N, M);     // rev, the y direction: Y's points search X
        two_way_lengths(it, x_len, y_len, N, M);
        const int64_t b = it.b;
        const bool rev = it.rev;
        const int i_base = it.chunk * (kBlock * U);
        const int32_t full = it.full, len_p = it.len_p, len_q = it.len_q;
        const float *src = rev ? Y + b * M * 3 : X + b * N * 3, *tgt = rev ? X + b * N * 3 : Y + b * M * 3;
        const float *own = rev ? NY + b * M * 3 : NX + b * N * 3, *other = rev ? NX + b * N * 3 : NY + b * M * 3;      // NORMALS
        float *dist = rev ? dist_y : dist_x, *term = rev ? term_y : term_x;
        int32_t *nearest = rev ? nearest_y : nearest_x;
        const bool live = len_q > 0 && i_base < len_p;              // the same in every lane of the workgroup
        float x[U], y[U], z[U], best[U];
        int idx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { x[u] = 0.f; y[u] = 0.f; z[u] = 0.f; best[u] = 0.f; idx[u] = 0; }
        if (live) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = min(i_base + u * kBlock + tid, len_p - 1);    // a slot beyond the cloud repeats its last point; not summed, not stored
                x[u] = src[i * 3 + 0]; y[u] = src[i * 3 + 1]; z[u] = src[i * 3 + 2];
                best[u] = __builtin_huge_valf();
            }
            tile_search<true, false>(tile, tid, len_q, [=](int j) { return tile_point(tgt, j); }, x, y, z, best, idx);
        }
        float mine = 0.f, mine_n = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i_base + u * kBlock + tid;
            const bool valid = live && i < len_p;
            const float e = valid ? so3::chamfer_term<SQUARED>(best[u]) : 0.f;
            mine += e;
            float t = 0.f;
            if (NORMALS && live) {                                   // both indices clamped into the live part before they address anything
                const int ic = min(i, len_p - 1), j = min(max(idx[u], 0), len_q - 1);
                const float tt = so3::chamfer_normal_term(own[ic * 3 + 0], own[ic * 3 + 1], own[ic * 3 + 2], other[j * 3 + 0], other[j * 3 + 1],
                                                          other[j * 3 + 2], signed_cos != 0);
                t = valid ? tt : 0.f;
            }
            mine_n += t;
            if (i < full) {
                if (dist != nullptr) dist[b * full + i] = e;
                if (nearest != nullptr) nearest[b * full + i] = valid ? min(idx[u], len_q - 1) : -1;
                if (NORMALS && term != nullptr) term[b * full + i] = t;
            }
        }
        float sum = wave_allsum(mine);                               // every lane runs both butterflies
        if (NORMALS) { const float sum_t = wave_allsum(mine_n); sum = (tid & 63) == 0 ? sum : sum_t; }
        item_record<W>(tile, tid, sum, rec + item * W);
    }
}

// The rows of both forwards, W floats per record: a thread per (cloud, direction) adds each of the W entries of the cloud's records in
// chunk order in float64, divides by the length and writes rows[w][2 b + direction].
template <int W>
__device__ __forceinline__ void chamfer_rows(const float *rec, const int32_t *x_len, const int32_t *y_len, float *const (&rows)[W], int64_t B,
                                             int32_t N, int32_t M, int32_t chunks_x, int32_t chunks_y) {
    const int per = chunks_x + chunks_y;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < 2 * B; t += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = t >> 1;
        const bool rev = (t & 1) != 0;
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *r = rec + (b * per + (rev ? chunks_x : 0)) * W;
        const int chunks = rev ? chunks_y : chunks_x;
        double acc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = 0.0;
        for (int c = 0; c < chunks; ++c) {
#pragma unroll
            for (int w = 0; w < W; ++w) acc[w] += static_cast<double>(r[c * W + w]);
        }
        const bool scored = nb > 0 && mb > 0 && chunks > 0;
        const double len = static_cast<double>(rev ? mb : nb);
#pragma unroll
        for (int w = 0; w < W; ++w) rows[w][t] = scored ? static_cast<float>(acc[w] / len) : 0.f;
    }
}

template <bool SQUARED, int U>
__global__ __launch_bounds__(kBlock) void k_chamfer_fwd(const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ x_len,
                                                        const int32_t *__restrict__ y_len, float *__restrict__ dist_x, int32_t *__restrict__ nearest_x,
                                                        float *__restrict__ dist_y, int32_t *__restrict__ nearest_y, float *__restrict__ rec,
                                                        int64_t B, int32_t N, int32_t M, int32_t chunks_x, int32_t chunks_y) {
    __shared__ float4 tile[kAddsTile];
    chamfer_search<SQUARED, U, false>(tile, X, Y, nullptr, nullptr, x_len, y_len, dist_x, nearest_x, dist_y, nearest_y, nullptr, nullptr, rec, 0, B,
                                      N, M, chunks_x, chunks_y);
}

// rows[b] = (cham_x, cham_y): a thread per (cloud, direction) adds the records in chunk order in float64 and divides by the length.
// A cloud with an empty side scores 0 in both; without the y items (chunks_y = 0) cham_y is written as 0.
__global__ __launch_bounds__(kBlock) void k_chamfer_rows(const float *__restrict__ rec, const int32_t *__restrict__ x_len,
                                                         const int32_t *__restrict__ y_len, float *__restrict__ rows, int64_t B, int32_t N, int32_t M,
                                                         int32_t chunks_x, int32_t chunks_y) {
    float *const out[1] = {rows};
    chamfer_rows<1>(rec, x_len, y_len, out, B, N, M, chunks_x, chunks_y);
}

// The owner scan of the gather backwards (k_chamfer_bwd, k_knn_bwd's dY).  A wave owns `owners` <= 64 consecutive points from
// `first`, lane l the point (px, py, pz) = first + l and its accumulator.  The wave reads the `entries` index entries load(e) 64 per
// block, kChamferScanBlocks blocks in flight, once for all its owners: an entry names one of them when idx - first < owners (one
// unsigned compare: -1 and every other owner fall out), a ballot collects the block's hits.  The lanes that hold a hit call
// term(e, ox, oy, oz, ux, uy, uz, g) side by side with their owner's point (ds_bpermute): it gathers the entry's point, forms u and
// may leave a coefficient in g.  The wave then walks the ballot in ascending e and the owner a hit names takes it with
// chamfer_hit(coef(g, h), u) -- readlane moves, no memory, one statically indexed accumulator per lane; coef gives a wave-uniform
// coefficient as it is, or fetches the hit lane h's g.  No loop bound depends on the data.  The chain runs in a copy of the caller's
// accumulator: through the reference, k_knn_bwd's owner takes a hit under a branch where it was three selects.
template <class Count, class Load, class Term, class Coef>
__device__ __forceinline__ void owner_scan(int lane, int first, unsigned owners, Count entries, float px, float py, float pz, Load load,
                                           Term term, Coef coef, float (&acc)[3]) {
    float a[3] = {acc[0], acc[1], acc[2]};
    for (Count e0 = 0; e0 < entries; e0 += 64 * so3::kChamferScanBlocks) {
        int named[so3::kChamferScanBlocks];
#pragma unroll
        for (int s = 0; s < so3::kChamferScanBlocks; ++s) {
            const Count e = e0 + 64 * s + lane;
            named[s] = e < entries ? load(e) : -1;
        }
#pragma unroll
        for (int s = 0; s < so3::kChamferScanBlocks; ++s) {
            const unsigned rel = static_cast<unsigned>(named[s] - first);
            const bool hit = rel < owners;
            unsigned long long mask = __ballot(hit);
            if (mask == 0) continue;
            const Count e = min(e0 + 64 * s + lane, entries - 1);
            const int owner = static_cast<int>(rel & 63u);
            const float ox = __shfl(px, owner, 64), oy = __shfl(py, owner, 64), oz = __shfl(pz, owner, 64);
            float ux = 0.f, uy = 0.f, uz = 0.f, g = 0.f;
            if (hit) term(e, ox, oy, oz, ux, uy, uz, g);
            while (mask != 0) {                                  // ascending e
                const int h = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int o = __builtin_amdgcn_readlane(owner, h);
                const float hc = coef(g, h);
                const float hx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ux), h));
                const float hy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uy), h));
                const float hz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uz), h));
                if (lane == o) so3::chamfer_hit(hc, hx, hy, hz, a);
            }
        }
    }
    acc[0] = a[0]; acc[1] = a[1]; acc[2] = a[2];
}

// The three gather backwards (k_chamfer_bwd, k_chamfer_normals_bwd, k_knn_bwd) keep their frame written out.  One frame taking the
// kernel's chain as a callable (own term, then owner_scan) was tried with the decode as a struct, as plain locals, by value and by
// reference, its lambdas forced inline: every spelling left the three with one or three SGPRs fewer or more, the scan blocks' eight
// e < entries compares signed where they were unsigned and k_knn_bwd 16 instructions longer (profiles/cloud_skeletons_isa.txt).
// k_chamfer_bwd: both gradients as a gather.  A wave owns kChamferOwners = 64 consecutive points of one cloud, one per lane, and a
// work item is the four waves' 256 points; the items of dX come first, then dY's, as in k_chamfer_fwd.  A lane opens its chain with
// its own term (its neighbour's 12 bytes gathered from L2).  The wave then takes the OTHER direction's `nearest` through owner_scan:
// a hit lane gathers its point and forms phi against the owner's point, the coefficient is the cloud's.
// No LDS, no barrier: the waves of a work item do not meet.  Padded slots and clouds with an empty side get a row of zeros.
template <bool SQUARED>
__global__ __launch_bounds__(kBlock) void k_chamfer_bwd(const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ x_len,
                                                        const int32_t *__restrict__ y_len, const int32_t *__restrict__ nearest_x,
                                                        const int32_t *__restrict__ nearest_y, const float *__restrict__ scale_x,
                                                        const float *__restrict__ scale_y, float *__restrict__ dX, float *__restrict__ dY, int64_t B,
                                                        int32_t N, int32_t M, int32_t chunks_x, int32_t chunks_y) {
    static_assert(so3::kChamferOwners == 64 && kBlock % 64 == 0, "one owner per lane");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per = chunks_x + chunks_y;
    const int64_t items = B * per;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        TwoWayItem it = two_way_item(item, per, chunks_x, N, M);     // rev, dY: Y's points own, X's points hit
        const int64_t b = it.b;
        const bool rev = it.rev;
        const int32_t full = it.full, qfull = it.qfull;
        const int first = it.chunk * kBlock + wave * 64;
        float *out = rev ? dY : dX;
        if (out == nullptr || first >= full) continue;
        two_way_lengths(it, x_len, y_len, N, M);
        const int32_t len_p = it.len_p, len_q = it.len_q;
        const float *P = rev ? Y + b * M * 3 : X + b * N * 3, *Q = rev ? X + b * N * 3 : Y + b * M * 3;
        const int32_t *near_own = rev ? nearest_y : nearest_x, *near_hit = rev ? nearest_x : nearest_y;
        const float *s_own = rev ? scale_y : scale_x, *s_hit = rev ? scale_x : scale_y;
        const int i = first + lane;
        float acc[3] = {0.f, 0.f, 0.f};
        const bool live = len_q > 0 && first < len_p;                // wave-uniform
        if (live) {
            const int ic = min(i, len_p - 1);
            const float px = P[ic * 3 + 0], py = P[ic * 3 + 1], pz = P[ic * 3 + 2];
            if (s_own != nullptr && near_own != nullptr) {
                const int j = min(max(near_own[b * full + ic], 0), len_q - 1);
                so3::chamfer_own<SQUARED>(s_own[b], px - Q[j * 3 + 0], py - Q[j * 3 + 1], pz - Q[j * 3 + 2], acc);
            }
            if (s_hit != nullptr && near_hit != nullptr) {
                const float cb = s_hit[b];
                const unsigned owners = static_cast<unsigned>(min(64, len_p - first));
                const int32_t *hits = near_hit + b * qfull;
                owner_scan(lane, first, owners, len_q, px, py, pz, [&](int j) { return hits[j]; },
                    [&](int j, float ox, float oy, float oz, float &ux, float &uy, float &uz, float &) {
                        so3::chamfer_phi<SQUARED>(ox - Q[j * 3 + 0], oy - Q[j * 3 + 1], oz - Q[j * 3 + 2], ux, uy, uz);
                    },
                    [&](float, int) { return cb; }, acc);
            }
        }
        if (i < full) {
            const bool keep = live && i < len_p;
            float *o = out + (b * full + i) * 3;
            o[0] = keep ? acc[0] : 0.f; o[1] = keep ? acc[1] : 0.f; o[2] = keep ? acc[2] : 0.f;
        }
    }
}

// ---- Chamfer's normal term: the cosine loss on the pairs the searches return ---------------------------------------------------------
// k_chamfer_normals_fwd is k_chamfer_fwd with an epilogue per kept slot: the search has left the nearest index in a register, the
// lane loads its own normal (coalesced, 12 bytes) and gathers its neighbour's (12 bytes from L2), forms t = chamfer_normal_term and
// keeps a second lane sum in slot order.  The search's x, y, z are dead by then.  A work item leaves TWO floats, rec[item] = (sum of
// e, sum of t): item_record<2>, whose entry 0 adds the waves' sums in item_record<1>'s order -- dist, nearest and the distance rows
// are k_chamfer_fwd's bits.  signed_cos is wave-uniform (an SGPR), not a template parameter.  No atomics, no zero-fill.
template <bool SQUARED, int U>
__global__ __launch_bounds__(kBlock) void k_chamfer_normals_fwd(const float *__restrict__ X, const float *__restrict__ Y, const float *__restrict__ NX,
                                                                const float *__restrict__ NY, const int32_t *__restrict__ x_len,
                                                                const int32_t *__restrict__ y_len, float *__restrict__ dist_x,
                                                                int32_t *__restrict__ nearest_x, float *__restrict__ dist_y,
                                                                int32_t *__restrict__ nearest_y, float *__restrict__ term_x,
                                                                float *__restrict__ term_y, float *__restrict__ rec, int32_t signed_cos, int64_t B,
                                                                int32_t N, int32_t M, int32_t chunks_x, int32_t chunks_y) {
    __shared__ float4 tile[kAddsTile];
    chamfer_search<SQUARED, U, true>(tile, X, Y, NX, NY, x_len, y_len, dist_x, nearest_x, dist_y, nearest_y, term_x, term_y, rec, signed_cos, B, N,
                                     M, chunks_x, chunks_y);
}

// rows[b] = (cham_x, cham_y) from the records' first floats, k_chamfer_rows' bits, and rows_n[b] the same from their second.
__global__ __launch_bounds__(kBlock) void k_chamfer_normals_rows(const float *__restrict__ rec, const int32_t *__restrict__ x_len,
                                                                 const int32_t *__restrict__ y_len, float *__restrict__ rows,
                                                                 float *__restrict__ rows_n, int64_t B, int32_t N, int32_t M, int32_t chunks_x,
                                                                 int32_t chunks_y) {
    float *const out[2] = {rows, rows_n};
    chamfer_rows<2>(rec, x_len, y_len, out, B, N, M, chunks_x, chunks_y);
}

// k_chamfer_normals_bwd: both normals' gradients as a gather, at k_chamfer_bwd's geometry (64 owners per wave, one per lane, dNX's
// items first, no LDS, no barrier).  A lane opens its chain with its own pair (its neighbour's normal gathered through the clamped
// index), then the wave takes the OTHER direction's `nearest` through owner_scan: the owner's three floats are its normal, a hit lane
// gathers its own normal and forms psi(owner, hit), the coefficient is the cloud's.  The points themselves are not read.
__global__ __launch_bounds__(kBlock) void k_chamfer_normals_bwd(const float *__restrict__ NX, const float *__restrict__ NY,
                                                                const int32_t *__restrict__ x_len, const int32_t *__restrict__ y_len,
                                                                const int32_t *__restrict__ nearest_x, const int32_t *__restrict__ nearest_y,
                                                                const float *__restrict__ scale_x, const float *__restrict__ scale_y,
                                                                float *__restrict__ dNX, float *__restrict__ dNY, int32_t signed_cos, int64_t B,
                                                                int32_t N, int32_t M, int32_t chunks_x, int32_t chunks_y) {
    static_assert(so3::kChamferOwners == 64 && kBlock % 64 == 0, "one owner per lane");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per = chunks_x + chunks_y;
    const int64_t items = B * per;
    const bool sc = signed_cos != 0;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        TwoWayItem it = two_way_item(item, per, chunks_x, N, M);     // rev, dNY: Y's normals own, X's hit
        const int64_t b = it.b;
        const bool rev = it.rev;
        const int32_t full = it.full, qfull = it.qfull;
        const int first = it.chunk * kBlock + wave * 64;
        float *out = rev ? dNY : dNX;
        if (out == nullptr || first >= full) continue;
        two_way_lengths(it, x_len, y_len, N, M);
        const int32_t len_p = it.len_p, len_q = it.len_q;
        const float *P = rev ? NY + b * M * 3 : NX + b * N * 3, *Q = rev ? NX + b * N * 3 : NY + b * M * 3;
        const int32_t *near_own = rev ? nearest_y : nearest_x, *near_hit = rev ? nearest_x : nearest_y;
        const float *s_own = rev ? scale_y : scale_x, *s_hit = rev ? scale_x : scale_y;
        const int i = first + lane;
        float acc[3] = {0.f, 0.f, 0.f};
        const bool live = len_q > 0 && first < len_p;                // wave-uniform
        if (live) {
            const int ic = min(i, len_p - 1);
            const float px = P[ic * 3 + 0], py = P[ic * 3 + 1], pz = P[ic * 3 + 2];
            if (s_own != nullptr && near_own != nullptr) {
                const int j = min(max(near_own[b * full + ic], 0), len_q - 1);
                float ux, uy, uz;
                so3::chamfer_normal_psi(px, py, pz, Q[j * 3 + 0], Q[j * 3 + 1], Q[j * 3 + 2], sc, ux, uy, uz);
                so3::chamfer_normal_own(s_own[b], ux, uy, uz, acc);
            }
            if (s_hit != nullptr && near_hit != nullptr) {
                const float cb = s_hit[b];
                const unsigned owners = static_cast<unsigned>(min(64, len_p - first));
                const int32_t *hits = near_hit + b * qfull;
                owner_scan(lane, first, owners, len_q, px, py, pz, [&](int j) { return hits[j]; },
                    [&](int j, float ox, float oy, float oz, float &ux, float &uy, float &uz, float &) {
                        so3::chamfer_normal_psi(ox, oy, oz, Q[j * 3 + 0], Q[j * 3 + 1], Q[j * 3 + 2], sc, ux, uy, uz);
                    },
                    [&](float, int) { return cb; }, acc);
            }
        }
        if (i < full) {
            const bool keep = live && i < len_p;
            float *o = out + (b * full + i) * 3;
            o[0] = keep ? acc[0] : 0.f; o[1] = keep ? acc[1] : 0.f; o[2] = keep ? acc[2] : 0.f;
        }
    }
}

// ---- PointNet++ sampling and grouping: farthest-point sampling and ball query ----------------------------------------------------
// The maximum of a 64-bit key over the wave, in every lane (wave_allmax's partners).
__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned int lo, unsigned int hi) {
    const unsigned long long b = (static_cast<unsigned long long>(hi) << 32) | lo;
    return b > a ? b : a;
}
template <int STEPS>                    // STEPS = 6: the whole wave; fewer: aligned groups of 2^STEPS lanes (STEPS <= 4)
__device__ __forceinline__ unsigned long long wave_allmax_key(unsigned long long k) {
#define SO3_KEY_STEP(MOVE) k = key_max(k, __float_as_uint(MOVE(__uint_as_float(static_cast<unsigned int>(k)))), \
                                       __float_as_uint(MOVE(__uint_as_float(static_cast<unsigned int>(k >> 32)))))
    if (STEPS >= 1) SO3_KEY_STEP(dpp_xor1);
    if (STEPS >= 2) SO3_KEY_STEP(dpp_xor2);
    if (STEPS >= 3) SO3_KEY_STEP(dpp_half_mirror);
    if (STEPS >= 4) SO3_KEY_STEP(dpp_mirror);
#undef SO3_KEY_STEP
    if (STEPS >= 5) k = key_max(k, __shfl_xor(static_cast<unsigned int>(k), 16, 64), __shfl_xor(static_cast<unsigned int>(k >> 32), 16, 64));
    if (STEPS >= 6) k = key_max(k, __shfl_xor(static_cast<unsigned int>(k), 32, 64), __shfl_xor(static_cast<unsigned int>(k >> 32), 32, 64));
    return k;
}

// k_fps<PPL, BLOCK>: one workgroup per cloud, all npoint iterations in one launch.  Point j lives in slot j / BLOCK of lane
// j % BLOCK, with its running minimum, for the whole launch.  One iteration: every lane updates its minima with the current centre
// (so3::pointnet_dist2, fps_update) and keeps its largest minimum and that point's slot, which give its key (so3::fps_key: largest
// minimum, lowest index); the wave's maximum (wave_allmax_key) is unique to one lane, which writes the key and its point's coordinates to
// the wave's LDS slot; one barrier; every wave reduces the slots redundantly and reads the winner's coordinates from the winner's slot, so the
// next centre never comes from global memory.  The slots are double-buffered by the parity of a counter that runs on across the
// clouds a workgroup serves: a wave can only be one barrier ahead of another, so it writes the buffer nobody is still reading.
// Loop bounds and barriers are uniform across the workgroup.  No atomics, no workspace, no scratch.
constexpr int kFpsMaxGrid = 4096;        // workgroups of a launch; a larger batch is strided over
template <int PPL, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_fps(const float *__restrict__ xyz, const int32_t *__restrict__ start, int32_t *__restrict__ out,
                                               int64_t B, int32_t N, int32_t npoint) {
    constexpr int kWaves = BLOCK / 64;
    constexpr int kSlotSteps = kWaves == 16 ? 4 : 2;
    static_assert(kWaves == 4 || kWaves == 16, "the slots are reduced within a DPP row");
    __shared__ unsigned long long slot_key[2][kWaves];
    __shared__ float4 slot_xyz[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int turn = 0;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const float *src = xyz + b * N * 3;
        float x[PPL], y[PPL], z[PPL], dist[PPL];
#pragma unroll
        for (int u = 0; u < PPL; ++u) {
            const int j = u * BLOCK + tid, jc = min(j, N - 1);
            x[u] = src[jc * 3 + 0]; y[u] = src[jc * 3 + 1]; z[u] = src[jc * 3 + 2];
            dist[u] = j < N ? so3::kFpsInit : -1.f;                         // a slot beyond the cloud: no d is below -1, and no point's minimum is
        }
        int cur = min(max(start[b], 0), N - 1);                             // workgroup-uniform
        float cx = src[cur * 3 + 0], cy = src[cur * 3 + 1], cz = src[cur * 3 + 2];
        asm volatile("" : "+v"(cx), "+v"(cy), "+v"(cz));                    // values, not addresses: otherwise the loop reads its centre through one
        for (int i = 0; i < npoint; ++i) {                                  // flat load whose pointer is this global one or the LDS slot's
            if (tid == 0) out[b * npoint + i] = cur;
            if (i + 1 == npoint) break;
            float bestd = -1.f;                                             // the lane's largest minimum and its slot: the lowest slot (= the
            int bu = 0;                                                     // lowest j of this lane) among equal values
#pragma unroll
            for (int u = 0; u < PPL; ++u) {
                so3::fps_update(so3::pointnet_dist2(x[u], y[u], z[u], cx, cy, cz), dist[u]);
                const bool up = dist[u] > bestd;
                bestd = up ? dist[u] : bestd;
                bu = up ? u : bu;
            }
            const unsigned long long best = bestd < 0.f ? 0ull : so3::fps_key(bestd, bu * BLOCK + tid);      // 0: a lane without a point
            const unsigned long long top = wave_allmax_key<6>(best);
            const int par = turn & 1;
            ++turn;
            if (top != 0 ? best == top : lane == 0) {                      // one lane: a point's key is unique
                float bx = x[0], by = y[0], bz = z[0];
#pragma unroll
                for (int u = 1; u < PPL; ++u) {
                    const bool mine = u == bu;
                    bx = mine ? x[u] : bx; by = mine ? y[u] : by; bz = mine ? z[u] : bz;
                }
                slot_key[par][wave] = top;
                slot_xyz[par][wave] = make_float4(bx, by, bz, 0.f);
            }
            __syncthreads();
            const unsigned long long win = wave_allmax_key<kSlotSteps>(slot_key[par][lane & (kWaves - 1)]);
            cur = so3::fps_key_index(win);
            const float4 c = slot_xyz[par][(cur & (BLOCK - 1)) >> 6];       // the wave that holds point cur
            cx = c.x; cy = c.y; cz = c.z;
        }
    }
}

// k_ball_query<COUNT>: one wave per centre, the cloud scanned 64 points per step in ascending j, kBallUnroll steps' loads in flight.
// The cloud is read straight from global memory (12 B per lane, a wave's 768 B contiguous; every centre of a cloud reads the same
// 12 * N bytes, which stay in L2): waves that have filled their row leave early, which tiles shared through LDS by a workgroup
// would not allow.  Membership gives a ballot; a lane's slot is count + popcount(mask below it), so stores ascend by construction.
// COUNT = true scans the whole cloud and writes the number of points in the ball.
constexpr int kBallUnroll = 4;
template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_ball_query(const float *__restrict__ xyz, const float *__restrict__ centres, float radius,
                                                       int32_t width, int32_t *__restrict__ idx, int32_t *__restrict__ count,
                                                       int64_t B, int32_t N, int32_t S) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const float r2 = so3::ball_radius2(radius);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t item = wave; item < B * S; item += nwaves) {
        const int64_t b = item / S;
        const float *src = xyz + b * N * 3;
        const float cx = centres[item * 3 + 0], cy = centres[item * 3 + 1], cz = centres[item * 3 + 2];      // wave-uniform
        int32_t *row = idx + item * width;
        int found = 0, first = N;
        for (int j0 = 0; j0 < N; j0 += 64 * kBallUnroll) {
            float x[kBallUnroll], y[kBallUnroll], z[kBallUnroll];
#pragma unroll
            for (int k = 0; k < kBallUnroll; ++k) {
                const int j = min(j0 + 64 * k + lane, N - 1);
                x[k] = src[j * 3 + 0]; y[k] = src[j * 3 + 1]; z[k] = src[j * 3 + 2];
            }
#pragma unroll
            for (int k = 0; k < kBallUnroll; ++k) {
                const int j = j0 + 64 * k + lane;
                const bool in = j < N && so3::ball_member(so3::pointnet_dist2(x[k], y[k], z[k], cx, cy, cz), r2);
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(in);
                if (mask != 0) {                                           // wave-uniform
                    if (found == 0) first = j0 + 64 * k + __builtin_ctzll(mask);
                    const int at = found + __builtin_popcountll(mask & below);
                    if (in && at < width) row[at] = j;
                    found += __builtin_popcountll(mask);
                }
            }
            if (!COUNT && found >= width) break;
        }
        for (int k = min(found, width) + lane; k < width; k += 64) row[k] = first;
        if (COUNT && lane == 0) count[item] = found;
    }
}

// ---- PointNet++ feature propagation: three nearest known points, inverse-distance interpolation and its backward -------------------
constexpr int kThreeMaxGrid = 8192;      // workgroups of a launch; more work items are strided over

// k_three_nn<WPP, WEIGHT>: tile_search's loop, written out, with a sorted top three per lane.  One work item = kBlock / WPP unknown points
// of one cloud; the known cloud goes through LDS in tiles of kAddsTile float4 and every lane of a wave reads the same float4 per step.
// Thread tid keeps point tid % (kBlock / WPP) and scans slice tid / (kBlock / WPP): the tile's blocks of kAddsUnroll entries are dealt
// to the WPP slices in turn, so a wave's lanes share their slice and the LDS read stays a broadcast.  A tile's tail is padded with
// x = +inf, whose d is +inf (or NaN) and never enters a list.  Slices 1.. hand their lists to slice 0 through LDS, which merges them
// lexicographically on (d, j) (so3::three_nn_put<true>), finishes the row and writes it.  No atomics, no workspace, no scratch.
template <int WPP, bool WEIGHT>
__global__ __launch_bounds__(kBlock) void k_three_nn(const float *__restrict__ unknown, const float *__restrict__ known, float *__restrict__ dist2,
                                                     int32_t *__restrict__ idx, float *__restrict__ weight, int64_t B, int32_t N, int32_t S,
                                                     int32_t chunks) {
    static_assert(kAddsTile == so3::kThreeNnTile && kBlock == so3::kIcpBlock, "the dispatch's constants");
    constexpr int kPts = kBlock / WPP;
    __shared__ float4 tile[kAddsTile];
    __shared__ float part_d[WPP > 1 ? WPP - 1 : 1][3][kPts];
    __shared__ int part_j[WPP > 1 ? WPP - 1 : 1][3][kPts];
    const int tid = threadIdx.x, pt = tid % kPts, slice = tid / kPts;
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int i = static_cast<int>(item - b * chunks) * kPts + pt;
        const float *src = unknown + b * N * 3, *tgt = known + b * S * 3;
        const int ic = min(i, N - 1);                                              // a slot beyond the cloud repeats its last point; not stored
        const float x = src[ic * 3 + 0], y = src[ic * 3 + 1], z = src[ic * 3 + 2];
        float D[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
        int J[3] = {so3::kThreeNnNone, so3::kThreeNnNone, so3::kThreeNnNone};
        for (int t0 = 0; t0 < S; t0 += kAddsTile) {
            const int cnt = min(kAddsTile, S - t0);
            const int cntp = (cnt + kAddsUnroll - 1) / kAddsUnroll * kAddsUnroll;      // <= kAddsTile
            __syncthreads();                                                         // the previous tile has been read
            for (int k = tid; k < cntp; k += kBlock) {
                const int j = t0 + min(k, cnt - 1);
                float4 q;
                q.x = k < cnt ? tgt[j * 3 + 0] : __builtin_huge_valf(); q.y = tgt[j * 3 + 1]; q.z = tgt[j * 3 + 2]; q.w = 0.f;
                tile[k] = q;
            }
            __syncthreads();
            for (int k = slice * kAddsUnroll; k < cntp; k += WPP * kAddsUnroll) {
#pragma unroll
                for (int kk = 0; kk < kAddsUnroll; ++kk) {
                    const f32x4 q = *(const volatile lds_f32x4 *)(&tile[k + kk]);     // tile_search: the ds_read_b128 broadcast
                    so3::three_nn_put<false>(so3::pointnet_dist2(q.x, q.y, q.z, x, y, z), t0 + k + kk, D, J);
                }
            }
        }
        if (WPP > 1) {
            if (slice > 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { part_d[slice - 1][k][pt] = D[k]; part_j[slice - 1][k][pt] = J[k]; }
            }
            __syncthreads();                                                         // the next write to part comes two barriers later
            if (slice > 0) continue;
#pragma unroll
            for (int w = 0; w < WPP - 1; ++w) {
#pragma unroll
                for (int k = 0; k < 3; ++k) so3::three_nn_put<true>(part_d[w][k][pt], part_j[w][k][pt], D, J);
            }
        }
        so3::three_nn_finish(S, D, J);
        if (i < N) {
            const int64_t at = (b * N + i) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) { dist2[at + k] = D[k]; idx[at + k] = J[k]; }
            if (WEIGHT) {
                float W[3];
                so3::three_nn_weights(S, D, W);
#pragma unroll
                for (int k = 0; k < 3; ++k) weight[at + k] = W[k];
            }
        }
    }
}

// k_three_interp<CF>: out = fma(w2, f2, fma(w1, f1, w0 * f0)) (so3::three_interp).  An index outside [0, S) is clamped, so a bad index
// buffer cannot read out of bounds.
// CF = false, (B,S,D) -> (B,N,D): a group of gw = min(64, D rounded up to a power of two) lanes per unknown point, 64 / gw points per
//   wave; the lanes run over the channels, so the three feature rows are read and the output row is written contiguously.
// CF = true, (B,D,S) -> (B,D,N): one work item = kBlock unknown points x kThreeCfChannels channels of one cloud; a lane keeps its
//   point's indices and weights and walks the channels, so every store is contiguous over n and every load is a gather inside one
//   feature row of S floats.
constexpr int kThreeCfChannels = 16;
template <bool CF>
__global__ __launch_bounds__(kBlock) void k_three_interp(const float *__restrict__ feat, const int32_t *__restrict__ idx, const float *__restrict__ weight,
                                                         float *__restrict__ out, int64_t B, int32_t N, int32_t S, int32_t D, int32_t gw) {
    if (!CF) {
        const int lane = threadIdx.x & 63, sub = lane / gw, c0 = lane % gw, rpw = 64 / gw;
        const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
        const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64), rows = B * N;
        for (int64_t row0 = wave * rpw; row0 < rows; row0 += nwaves * rpw) {
            const int64_t row = row0 + sub;
            if (row >= rows) continue;
            const float *f = feat + row / N * S * D;
            const int64_t i0 = min(max(idx[row * 3 + 0], 0), S - 1), i1 = min(max(idx[row * 3 + 1], 0), S - 1), i2 = min(max(idx[row * 3 + 2], 0), S - 1);
            const float w0 = weight[row * 3 + 0], w1 = weight[row * 3 + 1], w2 = weight[row * 3 + 2];
            for (int c = c0; c < D; c += gw) out[row * D + c] = so3::three_interp(w0, w1, w2, f[i0 * D + c], f[i1 * D + c], f[i2 * D + c]);
        }
    } else {
        const int nchunks = (N + kBlock - 1) / kBlock, cchunks = (D + kThreeCfChannels - 1) / kThreeCfChannels;
        const int64_t items = B * nchunks * cchunks;
        for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
            const int64_t b = item / (static_cast<int64_t>(nchunks) * cchunks);
            const int rest = static_cast<int>(item - b * nchunks * cchunks);
            const int n = rest % nchunks * kBlock + static_cast<int>(threadIdx.x), cbase = rest / nchunks * kThreeCfChannels;
            if (n >= N) continue;
            const int64_t row = b * N + n;
            const int i0 = min(max(idx[row * 3 + 0], 0), S - 1), i1 = min(max(idx[row * 3 + 1], 0), S - 1), i2 = min(max(idx[row * 3 + 2], 0), S - 1);
            const float w0 = weight[row * 3 + 0], w1 = weight[row * 3 + 1], w2 = weight[row * 3 + 2];
            const int cend = min(cbase + kThreeCfChannels, D);
            for (int c = cbase; c < cend; ++c) {
                const float *f = feat + (b * D + c) * S;
                out[(b * D + c) * N + n] = so3::three_interp(w0, w1, w2, f[i0], f[i1], f[i2]);
            }
        }
    }
}

// The backward as a gather: grad_feat[b][s][c] = sum of w(n,k) * grad_out[b][n][c] over the (n, k) with idx[b][n][k] == s, taken in
// ascending (n, k) through acc = fma(w, g, acc) (so3::three_interp_bwd_add).  A wave owns known points; it scans the cloud's 3N
// indices (clamped into [0, S) as the forward clamps them) 64 at a time from LDS, takes the ballot of idx == s and walks the set bits
// upwards.  Every element of grad_feat is written once, zeros included: no atomics, no memset, no workspace, the same bits every call.
// k_three_interp_bwd_cl, (B,N,D) -> (B,S,D): one work item = kThreeBwdS known points of one cloud, kThreeBwdS / 4 per wave; the lanes
//   run over the channels, four per lane (so3::kThreeBwdChannels per pass, further passes scan again), so a hit reads a contiguous row
//   of grad_out.  Indices and weights go through LDS in tiles of kThreeBwdTile unknown points.
constexpr int kThreeBwdS = 16;
constexpr int kThreeBwdTile = 1024;
__global__ __launch_bounds__(kBlock) void k_three_interp_bwd_cl(const float *__restrict__ grad_out, const int32_t *__restrict__ idx,
                                                                const float *__restrict__ weight, float *__restrict__ grad_feat, int64_t B, int32_t N,
                                                                int32_t S, int32_t D) {
    constexpr int kPerWave = kThreeBwdS / (kBlock / 64), kPerLane = so3::kThreeBwdChannels / 64;
    __shared__ int32_t t_idx[3 * kThreeBwdTile];
    __shared__ float t_w[3 * kThreeBwdTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int groups = (S + kThreeBwdS - 1) / kThreeBwdS;
    const int64_t items = B * groups;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / groups;
        const int s0 = static_cast<int>(item - b * groups) * kThreeBwdS + wave * kPerWave;
        const int32_t *ib = idx + b * N * 3;
        const float *wb = weight + b * N * 3, *gb = grad_out + b * N * D;
        for (int c0 = 0; c0 < D; c0 += so3::kThreeBwdChannels) {
            float acc[kPerWave][kPerLane];
#pragma unroll
            for (int u = 0; u < kPerWave; ++u)
#pragma unroll
                for (int q = 0; q < kPerLane; ++q) acc[u][q] = 0.f;
            for (int n0 = 0; n0 < N; n0 += kThreeBwdTile) {
                const int cnt = 3 * min(kThreeBwdTile, N - n0), cntp = (cnt + 63) / 64 * 64;
                __syncthreads();                                                     // the previous tile has been read
                for (int k = tid; k < cntp; k += kBlock) {
                    const int64_t e = static_cast<int64_t>(n0) * 3 + min(k, cnt - 1);
                    t_idx[k] = k < cnt ? min(max(ib[e], 0), S - 1) : -1;
                    t_w[k] = wb[e];
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < kPerWave; ++u) {
                    const int s = s0 + u;                                            // s >= S matches nothing: the indices are clamped
                    for (int k = 0; k < cntp; k += 64) {
                        unsigned long long mask = __builtin_amdgcn_ballot_w64(t_idx[k + lane] == s);
                        while (mask != 0) {                                          // wave-uniform
                            const int e = k + __builtin_ctzll(mask);
                            mask &= mask - 1;
                            const float w = t_w[e];
                            const float *g = gb + static_cast<int64_t>(n0 + e / 3) * D + c0 + lane;
#pragma unroll
                            for (int q = 0; q < kPerLane; ++q)
                                if (c0 + lane + 64 * q < D) acc[u][q] = so3::three_interp_bwd_add(w, g[64 * q], acc[u][q]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kPerWave; ++u)
#pragma unroll
                for (int q = 0; q < kPerLane; ++q)
                    if (s0 + u < S && c0 + lane + 64 * q < D) grad_feat[(b * S + s0 + u) * D + c0 + lane + 64 * q] = acc[u][q];
        }
    }
}

// k_three_interp_bwd_cf, (B,D,N) -> (B,D,S): one work item = 64 known points x 64 channels of one cloud, sixteen known points per wave,
//   a lane per channel.  grad_out is contiguous over n, so a tile of 64 unknown points x 64 channels is read row by row (lanes over n)
//   and stored transposed in LDS (stride 65: no bank conflicts either way); a hit then reads its row with the lanes over the channels.
//   The sums leave through the same LDS array, transposed back, so the stores to grad_feat are contiguous over s.
__global__ __launch_bounds__(kBlock) void k_three_interp_bwd_cf(const float *__restrict__ grad_out, const int32_t *__restrict__ idx,
                                                                const float *__restrict__ weight, float *__restrict__ grad_feat, int64_t B, int32_t N,
                                                                int32_t S, int32_t D) {
    constexpr int kPerWave = 64 / (kBlock / 64);
    __shared__ float gt[64][65];
    __shared__ int32_t t_idx[192];
    __shared__ float t_w[192];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sgroups = (S + 63) / 64, cgroups = (D + 63) / 64;
    const int64_t items = B * sgroups * cgroups;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / (static_cast<int64_t>(sgroups) * cgroups);
        const int rest = static_cast<int>(item - b * sgroups * cgroups);
        const int sbase = rest % sgroups * 64, c0 = rest / sgroups * 64;
        const int32_t *ib = idx + b * N * 3;
        const float *wb = weight + b * N * 3;
        float acc[kPerWave];
#pragma unroll
        for (int u = 0; u < kPerWave; ++u) acc[u] = 0.f;
        for (int n0 = 0; n0 < N; n0 += 64) {
            const int cnt = min(64, N - n0);
            __syncthreads();                                                         // the previous tile (or the previous item's sums) has been read
            for (int r = wave; r < 64; r += kBlock / 64)
                gt[lane][r] = (c0 + r < D && lane < cnt) ? grad_out[(b * D + c0 + r) * N + n0 + lane] : 0.f;
            if (tid < 192) {
                const int64_t e = static_cast<int64_t>(n0) * 3 + min(tid, 3 * cnt - 1);
                t_idx[tid] = tid < 3 * cnt ? min(max(ib[e], 0), S - 1) : -1;
                t_w[tid] = wb[e];
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kPerWave; ++u) {
                const int s = sbase + wave * kPerWave + u;
#pragma unroll
                for (int k = 0; k < 192; k += 64) {
                    unsigned long long mask = __builtin_amdgcn_ballot_w64(t_idx[k + lane] == s);
                    while (mask != 0) {                                              // wave-uniform
                        const int e = k + __builtin_ctzll(mask);
                        mask &= mask - 1;
                        acc[u] = so3::three_interp_bwd_add(t_w[e], gt[e / 3][lane], acc[u]);
                    }
                }
            }
        }
        __syncthreads();                                                             // the last tile has been read
#pragma unroll
        for (int u = 0; u < kPerWave; ++u) gt[wave * kPerWave + u][lane] = acc[u];
        __syncthreads();
        for (int r = wave; r < 64; r += kBlock / 64)
            if (c0 + r < D && sbase + lane < S) grad_feat[(b * D + c0 + r) * S + sbase + lane] = gt[lane][r];
    }
}

// ---- K nearest neighbours: a sorted list across the lanes of a wave, and both gradients in one gather -------------------------------
// The entry of the lane below (wave_shr:1 DPP); lane 0 keeps `below0`.
__device__ __forceinline__ float lane_below(float v, float below0) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(below0), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int lane_below(int v, int below0) { return __builtin_amdgcn_update_dpp(below0, v, 0x138, 0xf, 0xf, false); }

// k_knn<Q>: one wave serves Q queries of one cloud at a time; a work item is the four waves' 4 Q consecutive queries, and the waves of
// a work item do not meet (no LDS, no barrier).  Lane k holds entry k of every query's sorted list (so3::knn_insert), so K is a
// run-time, wave-uniform value.  The wave walks the target in blocks of 64 candidates, one per lane, straight from global memory
// (coalesced; a cloud's target stays in L2 for all its waves) with the next block's loads in flight; the Q query points are
// wave-uniform.  Per query a lane forms d and tests d < tau = entry K - 1, a ballot collects the block's hits and the wave inserts
// them in ascending j, each with one DPP move per list register and no memory access.  A hit is not tested again against the tau an
// earlier hit of its block lowered: inserting a d >= tau changes no lane below K.  Rows past n_b and clouds without a target skip the
// scan and write the padding (dist2 0, idx -1); lane k < K stores slot k, a row is one contiguous store.
template <int Q>
__global__ __launch_bounds__(kBlock) void k_knn(const float *__restrict__ X, const float *__restrict__ Y, int64_t y_stride, const int32_t *__restrict__ x_len,
                                                const int32_t *__restrict__ y_len, float *__restrict__ dist2, int32_t *__restrict__ idx, int32_t K,
                                                int64_t B, int32_t N, int32_t M, int32_t chunks) {
    static_assert(so3::kKnnMaxK == 64 && kBlock % 64 == 0, "one list entry per lane");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int first = (static_cast<int>(item - b * chunks) * (kBlock / 64) + wave) * Q;          // wave-uniform
        if (first >= N) continue;
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *src = X + b * N * 3, *tgt = Y + b * y_stride;
        const bool live = mb > 0 && first < nb;
        float D[Q];
        int J[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) { D[q] = __builtin_huge_valf(); J[q] = so3::kKnnNone; }
        if (live) {
            float qx[Q], qy[Q], qz[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int i = min(first + q, nb - 1);                // a slot beyond the cloud repeats its last point; not stored
                qx[q] = src[i * 3 + 0]; qy[q] = src[i * 3 + 1]; qz[q] = src[i * 3 + 2];
            }
            int jn = min(lane, mb - 1);
            float nx = tgt[jn * 3 + 0], ny = tgt[jn * 3 + 1], nz = tgt[jn * 3 + 2];
            for (int j0 = 0; j0 < mb; j0 += 64) {
                const float cx = nx, cy = ny, cz = nz;
                jn = min(j0 + 64 + lane, mb - 1);                    // the next block, clamped into the cloud
                nx = tgt[jn * 3 + 0]; ny = tgt[jn * 3 + 1]; nz = tgt[jn * 3 + 2];
                const bool valid = j0 + lane < mb;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float d = so3::pointnet_dist2(cx, cy, cz, qx[q], qy[q], qz[q]);
                    const float tau = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(D[q]), K - 1));
                    unsigned long long mask = __ballot(valid && d < tau);
                    while (mask != 0) {                              // ascending j
                        const int h = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const float dh = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), h));
                        so3::knn_insert(dh, j0 + h, D[q], J[q], lane_below(D[q], -__builtin_huge_valf()), lane_below(J[q], so3::kKnnNone));
                    }
                }
            }
        }
        const int32_t r = min(K, mb);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = first + q;
            if (i >= N) break;
            so3::knn_finish(lane, live && i < nb ? r : 0, mb, D[q], J[q]);
            if (lane < K) {
                const int64_t at = (b * N + i) * K + lane;
                if (dist2 != nullptr) dist2[at] = D[q];
                idx[at] = J[q];
            }
        }
    }
}

// k_knn_bwd: both gradients of dist2 as a gather, one launch; the items of dX come first, then dY's, as in k_chamfer_bwd.
// dX: a lane per query; its chain takes the slots k < r in ascending k (K gathers of 12 bytes), a padded slot (-1) contributes nothing.
// dY: a wave owns 64 consecutive target points, one per lane, and takes the cloud's n_b * K index entries through owner_scan in
//   ascending (i, k): a hit lane gathers its query point and forms the term against the owner's point, the coefficient is the
//   entry's own g.
// An index is clamped before it addresses anything; no loop bound depends on the data.  No LDS, no atomics, no zero-fill.
__global__ __launch_bounds__(kBlock) void k_knn_bwd(const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ x_len,
                                                    const int32_t *__restrict__ y_len, const int32_t *__restrict__ idx, const float *__restrict__ grad,
                                                    float *__restrict__ dX, float *__restrict__ dY, int32_t K, int64_t B, int32_t N, int32_t M,
                                                    int32_t chunks_x, int32_t chunks_y) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per = chunks_x + chunks_y;
    const int64_t items = B * per;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / per;
        const int c = static_cast<int>(item - b * per);
        const bool rev = c >= chunks_x;                              // dY: Y's points own
        const int32_t full = rev ? M : N;
        const int first = (rev ? c - chunks_x : c) * kBlock + wave * 64;
        float *out = rev ? dY : dX;
        if (out == nullptr || first >= full) continue;
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const int32_t len_p = rev ? mb : nb;
        const float *xs = X + b * N * 3, *ys = Y + b * M * 3;
        const int32_t *rows = idx + b * N * K;
        const float *gs = grad + b * N * K;
        const int i = first + lane;
        float acc[3] = {0.f, 0.f, 0.f};
        const bool live = nb > 0 && mb > 0 && first < len_p;         // wave-uniform
        if (live && !rev) {
            const int ic = min(i, nb - 1);
            const float px = xs[ic * 3 + 0], py = xs[ic * 3 + 1], pz = xs[ic * 3 + 2];
            const int32_t r = min(K, mb);
            for (int k = 0; k < r; ++k) {
                const int jr = rows[static_cast<int64_t>(ic) * K + k];
                const int j = min(max(jr, 0), mb - 1);
                float ux, uy, uz;
                so3::chamfer_phi<true>(px - ys[j * 3 + 0], py - ys[j * 3 + 1], pz - ys[j * 3 + 2], ux, uy, uz);
                if (jr >= 0) so3::chamfer_hit(gs[static_cast<int64_t>(ic) * K + k], ux, uy, uz, acc);
            }
        }
        if (live && rev) {
            const int jc = min(i, mb - 1);
            const float px = ys[jc * 3 + 0], py = ys[jc * 3 + 1], pz = ys[jc * 3 + 2];
            const unsigned owners = static_cast<unsigned>(min(64, mb - first));
            const int64_t entries = static_cast<int64_t>(nb) * K;
            owner_scan(lane, first, owners, entries, px, py, pz, [&](int64_t e) { return rows[e]; },
                [&](int64_t e, float ox, float oy, float oz, float &ux, float &uy, float &uz, float &g) {
                    const int q = static_cast<int>(e / K);           // the entry's query point, < n_b
                    so3::chamfer_phi<true>(ox - xs[q * 3 + 0], oy - xs[q * 3 + 1], oz - xs[q * 3 + 2], ux, uy, uz);
                    g = gs[e];
                },
                [&](float g, int h) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g), h)); }, acc);
        }
        if (i < full) {
            const bool keep = live && i < len_p;
            float *o = out + (b * full + i) * 3;
            o[0] = keep ? acc[0] : 0.f; o[1] = keep ? acc[1] : 0.f; o[2] = keep ? acc[2] : 0.f;
        }
    }
}

// ---- Local frames: the covariance of a point's neighbourhood and its eigen-decomposition, one query per lane -------------------------
// k_local_frames: a lane serves one row of idx (k_knn_bwd's dX mapping).  It reads the row's K indices from its own contiguous row
// and gathers 12 bytes per valid slot twice: the first pass finds the pivot (the first valid slot) and the chains of s, the second
// the six covariance chains about the mean -- the order the definition prescribes; a cloud of a few thousand points stays in L1 / L2
// between the passes.  A slot is valid when idx < m_b as ONE unsigned compare; an invalid slot loads point 0 of the cloud (m_b > 0
// here) and its values are dropped by selects, so no index addresses anything before it is tested.  Then the eigen stage in
// registers (so3::sym_eigen3: a fixed number of Jacobi sweeps, no data-dependent loop, no indexed private array).  Rows past n_b,
// rows without a valid slot and clouds with m_b == 0 write zeros; every element of every requested output is written.
// No LDS, no atomics, no workspace; the grid is capped and strided over.
__global__ __launch_bounds__(kBlock) void k_local_frames(const float *__restrict__ Y, int64_t y_stride, const int32_t *__restrict__ idx,
                                                         const int32_t *__restrict__ x_len, const int32_t *__restrict__ y_len,
                                                         const float *__restrict__ viewpoint, float *__restrict__ cov, float *__restrict__ eigenvalues,
                                                         float *__restrict__ normals, float *__restrict__ frames, int32_t K, int64_t B, int32_t N,
                                                         int32_t M, int32_t chunks) {
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int i = static_cast<int>(item - b * chunks) * kBlock + static_cast<int>(threadIdx.x);
        if (i >= N) continue;
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *tgt = Y + b * y_stride;
        const int64_t q = b * N + i;
        const int32_t *row = idx + q * K;
        float C[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, lam[3] = {0.f, 0.f, 0.f};
        so3::V3<float> e0 = so3::mk<float>(0.f, 0.f, 0.f), e1 = e0, e2 = e0;
        if (i < nb && mb > 0) {
            int32_t r = 0;
            float px = 0.f, py = 0.f, pz = 0.f, s[3] = {0.f, 0.f, 0.f};
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const int32_t j = row[k];
                const bool valid = so3::group_valid(j, mb);
                const int jc = valid ? j : 0;
                const float yx = tgt[jc * 3 + 0], yy = tgt[jc * 3 + 1], yz = tgt[jc * 3 + 2];
                const bool first = valid && r == 0;
                px = first ? yx : px; py = first ? yy : py; pz = first ? yz : pz;
                float t[3] = {s[0], s[1], s[2]};
                so3::frames_sum_slot(yx, yy, yz, px, py, pz, t);
                s[0] = valid ? t[0] : s[0]; s[1] = valid ? t[1] : s[1]; s[2] = valid ? t[2] : s[2];
                r += valid ? 1 : 0;
            }
            if (r > 0) {
                float m[3], S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                so3::frames_mean(s, r, m);
#pragma unroll 4
                for (int k = 0; k < K; ++k) {
                    const int32_t j = row[k];
                    const bool valid = so3::group_valid(j, mb);
                    const int jc = valid ? j : 0;
                    float T[6] = {S[0], S[1], S[2], S[3], S[4], S[5]};
                    so3::frames_cov_slot(tgt[jc * 3 + 0], tgt[jc * 3 + 1], tgt[jc * 3 + 2], px, py, pz, m, T);
#pragma unroll
                    for (int a = 0; a < 6; ++a) S[a] = valid ? T[a] : S[a];
                }
                so3::frames_cov_finish(S, r, C);
                if (eigenvalues != nullptr || normals != nullptr || frames != nullptr) {
                    so3::sym_eigen3(C, lam, e0, e1, e2);
                    const bool view = viewpoint != nullptr && !so3::frames_flat(C);
                    float wx = 0.f, wy = 0.f, wz = 0.f;
                    if (view) { wx = viewpoint[b * 3 + 0] - px; wy = viewpoint[b * 3 + 1] - py; wz = viewpoint[b * 3 + 2] - pz; }
                    so3::frames_orient(e0, e1, e2, view, wx, wy, wz);
                }
            }
        }
        if (cov != nullptr) {
#pragma unroll
            for (int a = 0; a < 6; ++a) cov[q * 6 + a] = C[a];
        }
        if (eigenvalues != nullptr) { eigenvalues[q * 3 + 0] = lam[0]; eigenvalues[q * 3 + 1] = lam[1]; eigenvalues[q * 3 + 2] = lam[2]; }
        if (normals != nullptr) { normals[q * 3 + 0] = e0.x; normals[q * 3 + 1] = e0.y; normals[q * 3 + 2] = e0.z; }
        if (frames != nullptr) {
            float *f = frames + q * 9;
            f[0] = e0.x; f[1] = e1.x; f[2] = e2.x;
            f[3] = e0.y; f[4] = e1.y; f[5] = e2.y;
            f[6] = e0.z; f[7] = e1.z; f[8] = e2.z;
        }
    }
}

// ---- FPFH: point feature histograms over a cloud's own neighbourhoods (include/so3proj.h holds the definition) ------------------------
// k_spfh<G>: G = the power of two >= K, 1 .. 64.  A group of G lanes serves one query, one neighbour per lane, a wave 64 / G queries,
// a work item kBlock / G consecutive queries of one cloud.  The group's lanes read the row's K indices side by side and gather the
// neighbour's point and normal; the query's own point and normal are one address for the whole group, which the memory pipeline
// serves as one request.  A lane forms its three bin numbers or "no pair" (so3::fpfh_pair, fpfh_bin); the histogram is 33 ballots,
// a slot's count the population count of the ballot under the group's lanes.  Lane k keeps the counts of the slots k, k + G, ... in
// registers (compile-time positions), so the 33 floats of a query leave as ceil(33 / G) stores of G consecutive floats.  An invalid
// slot reads point 0 and is dropped by selects: no index addresses anything before it is tested.  Every lane of a wave runs every
// ballot: the only loop bounds are the work item's and compile-time ones.  No LDS, no scratch, no atomics.
template <int G>
__global__ __launch_bounds__(kBlock) void k_spfh(const float *__restrict__ X, const float *__restrict__ normals, const int32_t *__restrict__ idx,
                                                 const int32_t *__restrict__ len, float *__restrict__ spfh, int32_t *__restrict__ pairs,
                                                 int32_t K, int64_t B, int32_t N, int32_t chunks) {
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a group is a power of two of lanes inside one wave");
    constexpr int kQueries = kBlock / G, kMine = (so3::kFpfhSlots + G - 1) / G;
    const int tid = threadIdx.x, lane = tid & 63, k = tid & (G - 1);
    const unsigned long long group = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull) << (lane & ~(G - 1));
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int i0 = static_cast<int>(item - b * chunks) * kQueries + tid / G;
        const bool row = i0 < N;
        const int i = row ? i0 : N - 1;
        const int32_t nb = so3::chamfer_length(len, b, N);
        const float *pts = X + b * N * 3, *nrm = normals + b * N * 3;
        const int64_t q = b * N + i;
        const int32_t j = k < K ? idx[q * K + k] : -1;
        const bool slot = row && i < nb && so3::group_valid(j, nb) && j != i;
        const int jc = slot ? j : 0;
        const so3::V3<float> pi = so3::mk<float>(pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]);
        const so3::V3<float> ni = so3::mk<float>(nrm[i * 3 + 0], nrm[i * 3 + 1], nrm[i * 3 + 2]);
        const so3::V3<float> pj = so3::mk<float>(pts[jc * 3 + 0], pts[jc * 3 + 1], pts[jc * 3 + 2]);
        const so3::V3<float> nj = so3::mk<float>(nrm[jc * 3 + 0], nrm[jc * 3 + 1], nrm[jc * 3 + 2]);
        float g1, g2, g3;
        const bool pair = so3::fpfh_pair(slot, pi, ni, pj, nj, g1, g2, g3);
        const int h1 = so3::fpfh_bin(g1), h2 = so3::kFpfhBins + so3::fpfh_bin(g2), h3 = 2 * so3::kFpfhBins + so3::fpfh_bin(g3);
        const int32_t r = __popcll(__builtin_amdgcn_ballot_w64(pair) & group);
        int32_t mine[kMine];
#pragma unroll
        for (int s = 0; s < so3::kFpfhSlots; ++s) {
            const int h = s < so3::kFpfhBins ? h1 : (s < 2 * so3::kFpfhBins ? h2 : h3);
            const int32_t c = __popcll(__builtin_amdgcn_ballot_w64(pair && h == s) & group);
            mine[s / G] = (s % G) == k ? c : ((s % G) == 0 ? 0 : mine[s / G]);
        }
        if (row && spfh != nullptr) {
#pragma unroll
            for (int t = 0; t < kMine; ++t) {
                const int s = t * G + k;
                if (s < so3::kFpfhSlots) spfh[q * so3::kFpfhSlots + s] = so3::spfh_value(mine[t], r);
            }
        }
        if (row && pairs != nullptr && k == 0) pairs[q] = r;
    }
}

// k_fpfh: one output element per lane, e = i * 33 + s inside a cloud, so consecutive lanes write consecutive floats.  A lane walks
// its query's K slots in ascending order -- the index and the neighbour's point are one address for the query's lanes, the 33
// floats of the neighbour's spfh row lie side by side across them -- and keeps the two chains of the definition (so3::fpfh_slot,
// fpfh_finish); w is recomputed per lane from the two points.  No cross-lane operation, no LDS, no atomics.
__global__ __launch_bounds__(kBlock) void k_fpfh(const float *__restrict__ X, const int32_t *__restrict__ idx, const int32_t *__restrict__ len,
                                                 const float *__restrict__ spfh, const int32_t *__restrict__ pairs, float *__restrict__ fpfh,
                                                 int32_t K, int64_t B, int32_t N, int32_t chunks) {
    const int32_t E = N * so3::kFpfhSlots;
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int e = static_cast<int>(item - b * chunks) * kBlock + static_cast<int>(threadIdx.x);
        if (e >= E) continue;
        const int i = e / so3::kFpfhSlots, s = e - i * so3::kFpfhSlots;
        const int32_t nb = so3::chamfer_length(len, b, N);
        float out = 0.f;
        if (i < nb) {
            const float *pts = X + b * N * 3, *hist = spfh + b * N * so3::kFpfhSlots;
            const int32_t *row = idx + (b * N + i) * K, *cnt = pairs + b * N;
            const float px = pts[i * 3 + 0], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
            float W = 0.f, A = 0.f;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const int32_t j = row[k];
                const bool slot = so3::group_valid(j, nb) && j != i;
                const int jc = slot ? j : 0;
                so3::fpfh_slot(slot, px, py, pz, pts[jc * 3 + 0], pts[jc * 3 + 1], pts[jc * 3 + 2], cnt[jc], hist[jc * so3::kFpfhSlots + s], W, A);
            }
            out = so3::fpfh_finish(hist[i * so3::kFpfhSlots + s], W, A);
        }
        fpfh[b * N * so3::kFpfhSlots + e] = out;
    }
}

// ---- RANSAC over feature matches (include/so3proj.h holds the definition; so3_device.h the arithmetic) --------------------------------
// k_ransac_score: one hypothesis per lane, a work item = kBlock consecutive hypotheses of one cloud.  A lane gathers its three sampled
// pairs, decides admissibility and keeps its pose in twelve registers (so3::ransac_pose: every lane runs the projection, an
// inadmissible one on the identity).  The workgroup then streams the cloud's first n_b pairs through LDS in tiles of kRansacTile: each
// lane stages its share (p_i, and q_i or NaN for an invalid pair, so that d2 <= r2 drops it without a branch); after the barrier every
// lane walks the tile in ascending i, all 64 lanes of a wave at one LDS address (two ds_read_b128 broadcasts per pair).  count and err
// stay in registers, in the definition's order by construction: no cross-lane operation, no atomics, no indexed private array.
__global__ __launch_bounds__(kBlock) void k_ransac_score(const float *__restrict__ P, const float *__restrict__ Q, const int32_t *__restrict__ corr,
                                                         const int32_t *__restrict__ x_len, const int32_t *__restrict__ y_len,
                                                         const int32_t *__restrict__ samples, float max_distance, float edge_similarity,
                                                         float *__restrict__ T_hyp, int32_t *__restrict__ count, float *__restrict__ err,
                                                         int64_t B, int32_t N, int32_t M, int32_t H, int32_t chunks) {
    __shared__ float4 tile_p[so3::kRansacTile];
    __shared__ float4 tile_q[so3::kRansacTile];
    const int tid = threadIdx.x;
    const float r2 = max_distance * max_distance;
    const int64_t items = B * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / chunks;
        const int h0 = static_cast<int>(item - b * chunks) * kBlock + tid;
        const bool live = h0 < H;
        const int h = live ? h0 : H - 1;
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *src = P + b * N * 3, *tgt = Q + b * M * 3;
        const int32_t *cr = corr + b * N, *tri = samples + (b * H + h) * 3;
        int32_t si[3], sc[3];
        so3::V3<float> p[3], q[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            si[k] = tri[k];
            const int ic = so3::group_valid(si[k], N) ? si[k] : 0;          // no index addresses anything before it is tested
            sc[k] = cr[ic];
            const bool valid = so3::group_valid(si[k], N) && so3::ransac_valid(si[k], nb, sc[k], mb);
            const int jc = valid ? sc[k] : 0;
            p[k] = so3::mk<float>(src[ic * 3 + 0], src[ic * 3 + 1], src[ic * 3 + 2]);
            q[k] = so3::mk<float>(tgt[jc * 3 + 0], tgt[jc * 3 + 1], tgt[jc * 3 + 2]);
            ok = ok && valid;
        }
        const bool admissible = so3::ransac_admissible(ok, si, sc, p, q, edge_similarity);
        float T[12];
        so3::ransac_pose(admissible, p, q, T);
        int32_t cnt = 0;
        float e = 0.f;
        for (int t0 = 0; t0 < nb; t0 += so3::kRansacTile) {
            const int len = min(so3::kRansacTile, nb - t0);
            __syncthreads();                                                    // the previous tile has been read
            for (int k = tid; k < len; k += kBlock) {
                const int i = t0 + k;
                const int32_t c = cr[i];
                const bool valid = so3::ransac_valid(i, nb, c, mb);
                const int jc = valid ? c : 0;
                float4 a, t;
                a.x = src[i * 3 + 0]; a.y = src[i * 3 + 1]; a.z = src[i * 3 + 2]; a.w = 0.f;
                t.x = valid ? tgt[jc * 3 + 0] : __builtin_nanf(""); t.y = tgt[jc * 3 + 1]; t.z = tgt[jc * 3 + 2]; t.w = 0.f;
                tile_p[k] = a;
                tile_q[k] = t;
            }
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < len; ++k) {
                const f32x4 a = *(const volatile lds_f32x4 *)(&tile_p[k]);      // wave-uniform addresses: broadcasts
                const f32x4 t = *(const volatile lds_f32x4 *)(&tile_q[k]);
                so3::ransac_score_pair(T, a.x, a.y, a.z, t.x, t.y, t.z, r2, cnt, e);
            }
        }
        if (live) {
            const int64_t at = b * H + h0;
#pragma unroll
            for (int k = 0; k < 12; ++k) T_hyp[at * 12 + k] = T[k];
            count[at] = admissible ? cnt : -1;
            err[at] = admissible ? e : 0.f;
        }
    }
}

// k_ransac_select: one workgroup per cloud.  Lanes stride over the H hypotheses and keep their best under so3::ransac_better, a tree
// through LDS joins the 256 candidates (the order is total: the tree's shape cannot change the answer), every lane reads the winner's
// pose as it was WRITTEN (nothing is recomputed from the samples) and the workgroup walks the N rows for weights and targets.
__global__ __launch_bounds__(kBlock) void k_ransac_select(const float *__restrict__ P, const float *__restrict__ Q, const int32_t *__restrict__ corr,
                                                          const int32_t *__restrict__ x_len, const int32_t *__restrict__ y_len,
                                                          const float *__restrict__ T_hyp, const int32_t *__restrict__ count,
                                                          const float *__restrict__ err, float max_distance, int32_t *__restrict__ best,
                                                          float *__restrict__ T_best, int32_t *__restrict__ inliers, float *__restrict__ rmse,
                                                          float *__restrict__ weights, float *__restrict__ targets, int64_t B, int32_t N,
                                                          int32_t M, int32_t H) {
    __shared__ int32_t s_c[kBlock], s_h[kBlock];
    __shared__ float s_e[kBlock];
    const int tid = threadIdx.x;
    const float r2 = max_distance * max_distance;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        int32_t bc = -1, bh = -1;
        float be = 0.f;
        for (int h = tid; h < H; h += kBlock) {
            const int32_t c = count[b * H + h];
            const float e = err[b * H + h];
            const bool take = so3::ransac_better(c, e, h, bc, be, bh);
            bc = take ? c : bc; be = take ? e : be; bh = take ? h : bh;
        }
        __syncthreads();                                                        // the previous cloud's winner has been read
        s_c[tid] = bc; s_e[tid] = be; s_h[tid] = bh;
        __syncthreads();
        for (int s = kBlock / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const bool take = so3::ransac_better(s_c[tid + s], s_e[tid + s], s_h[tid + s], s_c[tid], s_e[tid], s_h[tid]);
                if (take) { s_c[tid] = s_c[tid + s]; s_e[tid] = s_e[tid + s]; s_h[tid] = s_h[tid + s]; }
            }
            __syncthreads();
        }
        bc = s_c[0]; be = s_e[0]; bh = s_h[0];
        const bool found = bh >= 0;
        float T[12];
        so3::ransac_identity(T);
        if (found) {
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = T_hyp[(b * H + bh) * 12 + k];      // wave-uniform: scalar loads
        }
        if (tid == 0) {
            best[b] = bh;
            inliers[b] = bc > 0 ? bc : 0;
            rmse[b] = so3::ransac_rmse(bc, be);
#pragma unroll
            for (int k = 0; k < 12; ++k) T_best[b * 12 + k] = T[k];
        }
        const int32_t nb = so3::chamfer_length(x_len, b, N), mb = so3::chamfer_length(y_len, b, M);
        const float *src = P + b * N * 3, *tgt = Q + b * M * 3;
        for (int i = tid; i < N; i += kBlock) {
            const int32_t c = corr[b * N + i];
            const bool valid = so3::ransac_valid(i, nb, c, mb);
            const int jc = valid ? c : 0;
            const float px = src[i * 3 + 0], py = src[i * 3 + 1], pz = src[i * 3 + 2];
            const float qx = tgt[jc * 3 + 0], qy = tgt[jc * 3 + 1], qz = tgt[jc * 3 + 2];
            float x, y, z, d2;
            const bool in = so3::ransac_inlier(T, px, py, pz, qx, qy, qz, r2, x, y, z, d2) && valid && found;
            weights[b * N + i] = in ? 1.f : 0.f;
            const bool row = i < nb;
            targets[(b * N + i) * 3 + 0] = valid ? qx : (row ? x : 0.f);
            targets[(b * N + i) * 3 + 1] = valid ? qy : (row ? y : 0.f);
            targets[(b * N + i) * 3 + 2] = valid ? qz : (row ? z : 0.f);
        }
    }
}

// ---- PointNet++ set abstraction: the grouping gather and its backward -------------------------------------------------------------
// What sample_and_group does between the ball query and the first Conv2d: gather the grouped coordinates and
// features, subtract the centre, concatenate, in the layout the caller asks for.  A slot whose index lies outside [0, N) -- an empty
// ball's N, or a negative index -- is 0 in every channel and takes no gradient; no index can make a kernel leave a buffer.
// k_group_fwd<CF>:
// CF = false, -> (B,S,K,C): a group of gw = min(64, C rounded up to a power of two) lanes per slot, 64 / gw slots per wave; the
//   lanes run over the channels, so the point's row is read and the slot's row is written contiguously (k_three_interp<false>).
// CF = true, -> (B,C,K,S): one work item = kBlock centres x kGroupFwdCfChannels channels of one (cloud, k); a lane keeps its slot's
//   index and walks the channels, so every store is contiguous over s and every load is a gather inside the cloud's coordinates or
//   inside one feature row of N floats.
template <bool CF>
__global__ __launch_bounds__(kBlock) void k_group_fwd(const float *__restrict__ xyz, const float *__restrict__ centres, const float *__restrict__ feat,
                                                      const int32_t *__restrict__ idx, float *__restrict__ out, int32_t features_first, int64_t B,
                                                      int32_t N, int32_t S, int32_t K, int32_t D, int32_t gw) {
    const int32_t C = 3 + D;
    const bool ff = features_first != 0;
    if (!CF) {
        const int lane = threadIdx.x & 63, sub = lane / gw, c0 = lane % gw, rpw = 64 / gw;
        const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
        const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / 64), rows = B * S * K;
        for (int64_t row0 = wave * rpw; row0 < rows; row0 += nwaves * rpw) {
            const int64_t row = row0 + sub;
            if (row >= rows) continue;
            const int64_t bs = row / K, b = bs / S;
            const int32_t i = idx[row];
            const bool ok = so3::group_valid(i, N);
            const int64_t src = b * N + (ok ? i : 0);
            for (int32_t c = c0; c < C; c += gw) {
                int32_t d;
                const int j = so3::group_channel(ff, D, c, d);
                float v = 0.f;
                if (ok) v = j >= 0 ? so3::group_relative(xyz[src * 3 + j], centres[bs * 3 + j]) : feat[src * D + d];
                out[row * C + c] = v;
            }
        }
    } else {
        const int schunks = (S + kBlock - 1) / kBlock, cchunks = (C + so3::kGroupFwdCfChannels - 1) / so3::kGroupFwdCfChannels;
        const int64_t items = B * K * schunks * cchunks;
        for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
            const int sc = static_cast<int>(item % schunks);
            int64_t rest = item / schunks;
            const int32_t k = static_cast<int32_t>(rest % K);
            rest /= K;
            const int32_t cbase = static_cast<int32_t>(rest % cchunks) * so3::kGroupFwdCfChannels;
            const int64_t b = rest / cchunks;
            const int32_t s = sc * kBlock + static_cast<int32_t>(threadIdx.x);
            if (s >= S) continue;
            const int64_t bs = b * S + s;
            const int32_t i = idx[bs * K + k];
            const bool ok = so3::group_valid(i, N);
            const int64_t src = ok ? i : 0;
            const int32_t cend = min(cbase + so3::kGroupFwdCfChannels, C);
            for (int32_t c = cbase; c < cend; ++c) {
                int32_t d;
                const int j = so3::group_channel(ff, D, c, d);
                float v = 0.f;
                if (ok) v = j >= 0 ? so3::group_relative(xyz[(b * N + src) * 3 + j], centres[bs * 3 + j]) : feat[(b * D + d) * N + src];
                out[((b * C + c) * K + k) * S + s] = v;
            }
        }
    }
}

// The backward as a gather (k_three_interp_bwd_* above, with the scan shared): grad_xyz[b][n][j] and grad_feat[b][n][d] are the sums
// of the matching channel of grad_out over the slots that selected n, by plain float32 additions from 0 in the ascending MEMORY order
// of the slots -- (s, k) channel-last, (k, s) channel-first.  Every requested element is written once, zeros included: no atomics, no
// memset, no workspace, the same bits every call.
// k_group_bwd<CF, CW, R>: one work item = 4 * (64 / CW) * R points x CW channels of one cloud.  grad_out streams through LDS in
//   memory order, T slots x CW channels per tile (channel-first: read with the lanes over the slots and stored transposed, stride
//   CW + 1, so neither side has bank conflicts), with the tile's indices beside it (invalid ones as -1).  A wave then scans the
//   indices 64 at a time ONCE for all its owners: idx - (its first owner) against its owner count, one ballot; a step without a hit
//   costs nothing more.  A hit is walked in ascending order; lane (u, c) adds the slot's channel c to the owner it keeps if the hit is
//   that owner's (R > 1: one ballot per r, so the accumulator's index is static).
//   <CF, 8, 2>: 3 + D <= 8, eight owner groups x eight channels per wave.  <CF, 64, 16>: a lane per channel, sixteen owners per lane.
//   A wave's owners are the points n = w (mod WT), WT the waves that share the cloud, not a run of neighbours: a ball query pads its
//   rows with their FIRST hit, the lowest index in the ball, so the low indices of a cloud take most of the hits and a wave that owned
//   points 0..15 would walk many times the average wave's hits, one after the other.  The scan sees idx % WT * 16 + idx / WT.
//   A work item whose channels hold no requested output is skipped, so a subset of the outputs gives the bits of the whole.
template <bool CF, int CW, int R>
__global__ __launch_bounds__(kBlock) void k_group_bwd(const float *__restrict__ grad_out, const int32_t *__restrict__ idx, float *__restrict__ grad_xyz,
                                                      float *__restrict__ grad_feat, int32_t features_first, int64_t B, int32_t N, int32_t S,
                                                      int32_t K, int32_t D) {
    constexpr int T = CW == so3::kGroupNarrowC ? so3::kGroupNarrowTile : so3::kGroupWideTile;
    constexpr int PW = 64 / CW * R, PG = PW * (kBlock / 64);
    constexpr int NL = T * CW / kBlock, NI = (T + kBlock - 1) / kBlock;             // loads of one lane per tile: 32 values, 4 or 1 indices
    static_assert(PG == (CW == so3::kGroupNarrowC ? so3::kGroupNarrowOwners : so3::kGroupWideOwners) && (R & (R - 1)) == 0 && T % 64 == 0 &&
                      T * CW % kBlock == 0, "so3_device.h");
    __shared__ float gt[T * (CW + 1)];
    __shared__ int32_t t_i[T];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u = lane / CW, cl = lane % CW;
    const int32_t C = 3 + D;
    const bool ff = features_first != 0;
    const int32_t xb = ff ? D : 0, fb = ff ? 0 : 3;              // the first coordinate channel, the first feature channel
    const int64_t E = static_cast<int64_t>(S) * K;
    const int ngroups = (N + PG - 1) / PG, cchunks = (C + CW - 1) / CW;
    const int32_t WT = ngroups * (kBlock / 64);                  // the waves that share a cloud's points: wave w owns the points n = w (mod WT)
    const int64_t items = B * ngroups * cchunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / (static_cast<int64_t>(ngroups) * cchunks);
        const int rest = static_cast<int>(item - b * ngroups * cchunks);
        const int32_t c0 = rest / ngroups * CW, cw = min(CW, C - c0);
        const bool has_xyz = grad_xyz != nullptr && c0 < xb + 3 && c0 + cw > xb;
        const bool has_feat = grad_feat != nullptr && c0 < fb + D && c0 + cw > fb;
        if (!has_xyz && !has_feat) continue;                                         // workgroup-uniform
        const int32_t nw0 = rest % ngroups * PG + wave * PW;                         // the wave's first owner
        const int32_t *ib = idx + b * E;
        const float *gb = grad_out + b * E * C;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        // A tile's loads: NL values and NI indices per lane, every address clamped into the buffer (no branch around a load), all in
        // flight together; the next tile's are issued before the current tile is scanned and wait in registers.
        float pre[NL];
        int32_t pi[NI];
        auto load_tile = [&](int64_t t0) {
            const int cnt = static_cast<int>(min(static_cast<int64_t>(T), E - t0));
            const int64_t k0 = CF ? t0 / S : 0;
            const int32_t s0 = CF ? static_cast<int32_t>(t0 - k0 * S) : 0;                 // s0 + q < S + T: int32
#pragma unroll
            for (int m = 0; m < NI; ++m) {
                const int q = min(tid + m * kBlock, cnt - 1);
                const int32_t kq = CF ? (s0 + q) / S : 0, sq = s0 + q - kq * S;
                pi[m] = ib[CF ? static_cast<int64_t>(sq) * K + k0 + kq : t0 + q];
            }
#pragma unroll
            for (int m = 0; m < NL; ++m) {
                const int q = tid + m * kBlock;
                const int cc = min(CF ? q / T : q % CW, cw - 1), jj = min(CF ? q % T : q / CW, cnt - 1);
                pre[m] = gb[CF ? static_cast<int64_t>(c0 + cc) * E + t0 + jj : (t0 + jj) * C + c0 + cc];
            }
        };
        load_tile(0);
        for (int64_t t0 = 0; t0 < E; t0 += T) {
            const int cnt = static_cast<int>(min(static_cast<int64_t>(T), E - t0)), cntp = (cnt + 63) / 64 * 64;
            __syncthreads();                                                         // the previous tile has been read
#pragma unroll
            for (int m = 0; m < NI; ++m) {
                const int q = tid + m * kBlock;
                if (q < T) t_i[q] = q < cnt && so3::group_valid(pi[m], N) ? pi[m] % WT * PW + pi[m] / WT : -1;   // the point's place among the owners
            }
#pragma unroll
            for (int m = 0; m < NL; ++m) {
                const int q = tid + m * kBlock;
                gt[(CF ? q % T : q / CW) * (CW + 1) + (CF ? q / T : q % CW)] = pre[m];   // a clamped load lands in a slot or channel nobody reads
            }
            __syncthreads();
            if (t0 + T < E) load_tile(t0 + T);                                       // workgroup-uniform
            for (int k0 = 0; k0 < cntp; k0 += 64) {
                const int32_t v = t_i[k0 + lane] - nw0;
                const bool in = static_cast<uint32_t>(v) < static_cast<uint32_t>(PW);
                if (__builtin_amdgcn_ballot_w64(in) == 0) continue;                  // wave-uniform: nobody here owns any of the 64 slots
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    unsigned long long mask = __builtin_amdgcn_ballot_w64(in && (v & (R - 1)) == r);
                    while (mask != 0) {                                              // wave-uniform
                        const int e = k0 + __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const int32_t vh = (t_i[e] - nw0) / R;
                        const float g = gt[e * (CW + 1) + cl];
                        acc[r] = vh == u ? so3::group_bwd_add(acc[r], g) : acc[r];
                    }
                }
            }
        }
        const int32_t c = c0 + cl;
        if (c >= C) continue;                                                        // no barrier follows in this iteration
        int32_t d;
        const int j = so3::group_channel(ff, D, c, d);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t n = static_cast<int64_t>((u * R + r) % PW) * WT + (nw0 + u * R + r) / PW;
            if (n >= N) continue;
            if (j >= 0) {
                if (grad_xyz != nullptr) grad_xyz[(b * N + n) * 3 + j] = acc[r];
            } else if (grad_feat != nullptr) {
                grad_feat[CF ? (b * D + d) * N + n : (b * N + n) * D + d] = acc[r];
            }
        }
    }
}

// grad_centres[b][s][j] = 0 - (the sum over ascending k of coordinate channel j of the valid slots of row (b, s)): a thread per centre.
template <bool CF>
__global__ __launch_bounds__(kBlock) void k_group_centres_bwd(const float *__restrict__ grad_out, const int32_t *__restrict__ idx,
                                                              float *__restrict__ grad_centres, int32_t features_first, int64_t B, int32_t N,
                                                              int32_t S, int32_t K, int32_t D) {
    const int32_t C = 3 + D, xb = features_first != 0 ? D : 0;
    const int64_t rows = B * S, step = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; row < rows; row += step) {
        const int64_t b = row / S, s = row - b * S;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        const int64_t cs = CF ? static_cast<int64_t>(K) * S : 1;
#pragma unroll 8
        for (int32_t k = 0; k < K; ++k) {                                            // no load depends on the index: no branch, the loads overlap
            const bool ok = so3::group_valid(idx[row * K + k], N);
            const float *g = CF ? grad_out + ((b * C + xb) * K + k) * S + s : grad_out + (row * K + k) * C + xb;
            const float g0 = g[0], g1 = g[cs], g2 = g[2 * cs];
            a0 = ok ? so3::group_bwd_add(a0, g0) : a0;
            a1 = ok ? so3::group_bwd_add(a1, g1) : a1;
            a2 = ok ? so3::group_bwd_add(a2, g2) : a2;
        }
        grad_centres[row * 3 + 0] = 0.f - a0;
        grad_centres[row * 3 + 1] = 0.f - a1;
        grad_centres[row * 3 + 2] = 0.f - a2;
    }
}

// ---- float64 head and backward (the reference's functions accept double tensors): the same templates over
// T = double, one row per thread with plain loads -- a convenience path, not a benchmark configuration.
// Four fixed sweeps, then sweeps until the wave-wide residual is below 1e-14 (at most six more).
// Diagnostic twin of K1 (tests/test_gpu_parity.py: the adversarial search on the fast path's certificate): one row per thread,
// R as every forward kernel computes it (project_rotation<float>: the same IEEE operations as the packed engine) and, beside it,
// the DEVICE's own verdict -- did the fast path settle the row, or did it hand it to the Jacobi path.
__global__ __launch_bounds__(kBlock) void k_project_diag(const float *__restrict__ M, float *__restrict__ R, uint8_t *__restrict__ hard, int64_t B) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool active = row < B;
    float m[9], r[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = active ? M[row * 9 + i] : ((i & 3) == 0 ? 1.f : 0.f);
    const bool h = so3::project_rotation<float>(m, r);
    if (active) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[row * 9 + i] = r[i];
        hard[row] = h ? 1 : 0;
    }
}

// ---- float64 arguments of the metrics and the loss (the reference's functions accept double tensors and, for the metrics,
// cast to double themselves: rotation_representation.py:232-233) -- one row per thread straight from global memory: not a
// benchmark path, but no ATen arithmetic either.  MODE 0: angle_error (float64, range flag, unit = 180/pi or 1);
// MODE 1: compute_geodesic_distance_from_two_matrices (radians, hard clamp, no flag);  MODE 2: geodesic(R1, R2, reduction)
// (point_cloud/main.py:61-73: clamp to [lo, hi], the angles' sum added onto a zeroed accumulator).
// Grid-stride (at most 2048 workgroups).  How the reduction is finished -- `how`: 0 = atomics onto accumulators an init launch has
// zeroed; 1 = ONE workgroup (B <= 1024): it writes sum, count and flag itself; 2 = caller's workspace: partial per workgroup, a ticket,
// the last one writes everything (so3_rows.h, ticket_finish).  1 and 2 are one launch per call.
template <int MODE, bool WANT_ROWS, bool WANT_SUM>
__global__ __launch_bounds__(kBlock) void k_angle_f64(const double *__restrict__ R1, const double *__restrict__ R2, double *__restrict__ out,
                                                      double *__restrict__ sum_count, int32_t *__restrict__ range_flag, double unit, int64_t B,
                                                      so3::ReduceWs *ws, int how, double lo = -1.0, double hi = 1.0) {
    __shared__ double red[4];
    double acc = 0.0;
    bool bad = false;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; row < B; row += static_cast<int64_t>(gridDim.x) * kBlock) {
        double tr = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) tr = fma(R1[row * 9 + i], R2[row * 9 + i], tr);
        const double c_raw = (tr - 1.0) * 0.5;
        bad |= MODE == 0 && (c_raw < -1.1 || c_raw > 1.1);
        double c = fmin(fmax(c_raw, lo), hi);
        if (c_raw != c_raw) c = c_raw;                          // clamp keeps NaN
        const double ang = so3::acos_f64(c) * unit;
        if (WANT_ROWS) out[row] = ang;
        acc += ang;
    }
    const bool any_bad = MODE == 0 && __syncthreads_or(bad ? 1 : 0) != 0;
    const double total = WANT_SUM ? block_sum(acc, red) : 0.0;
    if (MODE == 2 && WANT_SUM && threadIdx.x == 0) atomicAdd(sum_count, total);
    if (MODE != 0) return;
    if (how == 2) {
        so3::ticket_finish<kBlock>(ws, blockIdx.x, gridDim.x, gridDim.x, total, any_bad, [&](double t, bool any) {
            if (WANT_SUM) { sum_count[0] = t; sum_count[1] = static_cast<double>(B); }
            if (range_flag != nullptr) *range_flag = any ? 1 : 0;
        });
    } else if (threadIdx.x == 0) {
        if (how == 1) {
            if (WANT_SUM) { sum_count[0] = total; sum_count[1] = static_cast<double>(B); }
            if (range_flag != nullptr) *range_flag = any_bad ? 1 : 0;
        } else {
            if (WANT_SUM) atomicAdd(sum_count, total);
            if (any_bad && range_flag != nullptr) atomicOr(range_flag, 1);
        }
    }
}

// loss_frobenius in float64: sum_b ||Rtrue_b - Rpred_b||_F, optional dRpred_b = (Rpred_b - Rtrue_b) / (B ||.||_F); `how` as above
// (1 / 2: loss_sum and, if asked for, loss_mean = loss_sum / B are written by the kernel).
template <bool WANT_GRAD>
__global__ __launch_bounds__(kBlock) void k_frob_loss_f64(const double *__restrict__ Rpred, const double *__restrict__ Rtrue,
                                                          double *__restrict__ dRpred, double *__restrict__ loss_sum, double *__restrict__ loss_mean,
                                                          int64_t B, double inv_b, so3::ReduceWs *ws, int how) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; row < B; row += static_cast<int64_t>(gridDim.x) * kBlock) {
        double g[9], n2 = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            g[i] = Rpred[row * 9 + i] - Rtrue[row * 9 + i];
            n2 = fma(g[i], g[i], n2);
        }
        const double nrm = __builtin_sqrt(n2);
        if (WANT_GRAD) {
            const double gs = n2 > 0.0 ? inv_b / nrm : 0.0;     // zero difference -> zero gradient (the reference: NaN)
#pragma unroll
            for (int i = 0; i < 9; ++i) dRpred[row * 9 + i] = g[i] * gs;
        }
        acc += nrm;
    }
    const double total = block_sum(acc, red);
    auto write = [&](double t) {
        *loss_sum = t;
        if (loss_mean != nullptr) *loss_mean = t * inv_b;
    };
    if (how == 2) so3::ticket_finish<kBlock>(ws, blockIdx.x, gridDim.x, gridDim.x, total, false, [&](double t, bool) { write(t); });
    else if (threadIdx.x == 0) { if (how == 1) write(total); else atomicAdd(loss_sum, total); }
}
__global__ void k_mean_from_sum_f64(const double *__restrict__ loss_sum, double *__restrict__ loss_mean, double inv_b) {
    *loss_mean = *loss_sum * inv_b;
}

template <bool BWD>
__global__ __launch_bounds__(kBlock) void k_project_f64(const double *__restrict__ M, const double *__restrict__ G,
                                                        double *__restrict__ out, uint8_t *__restrict__ flip, int64_t B) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = row < B;
    const int64_t rr_ = live ? row : 0;                         // idle lanes recompute row 0: keeps the sweep loop wave-uniform
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = M[rr_ * 9 + i];
    if (!BWD) {
        const auto f = so3::signed_svd<false, double, 4, true, 6>(m);
        double r[9];
        so3::rotation_from(f, r);
        if (live) {
#pragma unroll
            for (int i = 0; i < 9; ++i) out[row * 9 + i] = r[i];
            if (flip != nullptr) {
                const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
                flip[row] = det < 0.0 ? 1 : 0;
            }
        }
    } else {
        double g[9], dm[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = G[rr_ * 9 + i];
        const auto f = so3::signed_svd<true, double, 4, true, 6>(m);
        so3::project_backward(f, g, dm);
        if (live) {
#pragma unroll
            for (int i = 0; i < 9; ++i) out[row * 9 + i] = dm[i];
        }
    }
}

// ---- 6D head, one row per thread: remainder (< 64 rows) and unaligned input of the streaming kernels ----------
template <bool BWD>
__global__ __launch_bounds__(kBlock) void k_ortho6d_rows(const float *__restrict__ X, const float *__restrict__ G,
                                                         float *__restrict__ out, int64_t B) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (row >= B) return;
    so3::RowCtx<1> ctx{};
    if (BWD) {
        so3::Rows<float, so3::OpOrtho6dBwd> rows;
#pragma unroll
        for (int i = 0; i < 6; ++i) rows.a[i] = X[row * 6 + i];
#pragma unroll
        for (int i = 0; i < 9; ++i) rows.b[i] = G[row * 9 + i];
        so3::OpOrtho6dBwd op;
        op.compute<float, 1>(rows, ctx);
#pragma unroll
        for (int i = 0; i < 6; ++i) out[row * 6 + i] = rows.o0[i];
    } else {
        so3::Rows<float, so3::OpOrtho6d> rows;
#pragma unroll
        for (int i = 0; i < 6; ++i) rows.a[i] = X[row * 6 + i];
        so3::OpOrtho6d op;
        op.compute<float, 1>(rows, ctx);
#pragma unroll
        for (int i = 0; i < 9; ++i) out[row * 9 + i] = rows.o0[i];
    }
}

// ---- any float32 row operation, one row per thread: remainder (< 64 rows) and unaligned input of the streaming kernels
template <class Op>
__global__ __launch_bounds__(kBlock) void k_op_rows(Op op, int64_t B) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (row >= B) return;
    so3::RowCtx<1> ctx{};
    so3::Rows<float, Op> rows;
    const float *a = static_cast<const float *>(op.in0) + row * Op::kIn0N;
#pragma unroll
    for (int i = 0; i < Op::kIn0N; ++i) rows.a[i] = a[i];
    if constexpr (Op::kIn1 != 0) {
        const float *b = static_cast<const float *>(op.in1) + row * Op::kIn1N;
#pragma unroll
        for (int i = 0; i < Op::kIn1N; ++i) rows.b[i] = b[i];
    }
    if constexpr (Op::kIn2 != 0) {
        const float *c = static_cast<const float *>(op.in2) + row * Op::kIn2N;
#pragma unroll
        for (int i = 0; i < Op::kIn2N; ++i) rows.c[i] = c[i];
    }
    op.template compute<float, 1>(rows, ctx);
    float *o = static_cast<float *>(op.out0) + row * Op::kOut0N;
#pragma unroll
    for (int i = 0; i < Op::kOut0N; ++i) o[i] = rows.o0[i];
    if constexpr (Op::kOut1 != 0) {
        float *o1 = static_cast<float *>(op.out1) + row * Op::kOut1N;
#pragma unroll
        for (int i = 0; i < Op::kOut1N; ++i) o1[i] = rows.o1[i];
    }
}

// ---- K4s / K3s one row per thread: a batch of up to kSmallBatch rows (one workgroup) and the remainder (< 64 rows) or unaligned input
// of the streaming kernels.  The arithmetic is the engine operation's own (compute<float, 1>).  Every thread runs the operation (idle ones
// on identities, exists = false), so its wave-wide votes see whole waves.  A wave's rows are one 64-row unit of the pointers it was given
// (blockDim is a multiple of 64).  `mode` (operations with a reduction): 1 = this launch is the whole batch, its one workgroup writes the
// loss and the mean; 2 = publish into the workspace's slot blockIdx.x (the engine launch behind it sums); 3 = add to *loss_sum.
template <class Op>
__global__ __launch_bounds__(kSmallBatch) void k_sym_rows(Op op, int64_t B, int mode, so3::ReduceWs *ws) {
    __shared__ double red[kSmallBatch / 64];
    so3::RowCtx<1> ctx{};
    ctx.lane = static_cast<int>(threadIdx.x & 63);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t row0 = static_cast<int64_t>(blockIdx.x) * blockDim.x; row0 < B; row0 += stride) {
        const int64_t row = row0 + threadIdx.x;
        const bool active = row < B;
        so3::Rows<float, Op> rows;
        const float *a = static_cast<const float *>(op.in0) + row * 9, *b = static_cast<const float *>(op.in1) + row * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            rows.a[i] = active ? a[i] : ((i & 3) == 0 ? 1.f : 0.f);
            rows.b[i] = active ? b[i] : ((i & 3) == 0 ? 1.f : 0.f);
        }
        if constexpr (Op::kIn2 != 0) rows.c[0] = __int_as_float(active ? static_cast<const int32_t *>(op.in2)[row] : 0);
        ctx.unit[0] = row >> 6;
        ctx.exists[0] = active;
        op.template compute<float, 1>(rows, ctx);
        if (active) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                if constexpr (Op::kOut0 != 0) static_cast<float *>(op.out0)[row * 9 + i] = rows.o0[i];
                if constexpr (Op::kOut1 != 0) static_cast<float *>(op.out1)[row * 9 + i] = rows.o1[i];
            }
        }
    }
    if constexpr (Op::kReduce) {
        const double v = wave_sum(ctx.acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double total = 0.0;
            for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) total += red[w];
            if (mode == 1) {
                *op.loss_sum = total;
                if (op.loss_mean != nullptr) *op.loss_mean = static_cast<float>(total * op.inv_b_f64);
            } else if (mode == 2) {
                publish_partial(ws, total, false);
            } else {
                atomicAdd(op.loss_sum, total);
            }
        }
    }
}

// ---- SE(3) update, one row per thread: remainder and unaligned input of the streaming kernels -----------------
template <bool BWD>
__global__ __launch_bounds__(kBlock) void k_se3_rows(const float *__restrict__ out12, const float *__restrict__ Tinit,
                                                     const float *__restrict__ G, float *__restrict__ res, float inv_fx,
                                                     float inv_fy, int64_t B) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (row >= B) return;
    so3::RowCtx<1> ctx{};
    if (BWD) {
        so3::Rows<float, so3::OpSe3UpdateBwd> rows;
#pragma unroll
        for (int i = 0; i < 12; ++i) rows.a[i] = out12[row * 12 + i];
#pragma unroll
        for (int i = 0; i < 16; ++i) { rows.b[i] = Tinit[row * 16 + i]; rows.c[i] = G[row * 16 + i]; }
        so3::OpSe3UpdateBwd op; op.inv_fx = inv_fx; op.inv_fy = inv_fy;
        op.compute<float, 1>(rows, ctx);
#pragma unroll
        for (int i = 0; i < 12; ++i) res[row * 12 + i] = rows.o0[i];
    } else {
        so3::Rows<float, so3::OpSe3Update> rows;
#pragma unroll
        for (int i = 0; i < 12; ++i) rows.a[i] = out12[row * 12 + i];
#pragma unroll
        for (int i = 0; i < 16; ++i) rows.b[i] = Tinit[row * 16 + i];
        so3::OpSe3Update op; op.inv_fx = inv_fx; op.inv_fy = inv_fy;
        op.compute<float, 1>(rows, ctx);
#pragma unroll
        for (int i = 0; i < 16; ++i) res[row * 16 + i] = rows.o0[i];
    }
}

// ---- next row f3: per-class evaluation statistics of K4's angles (3D-Pose/test_per_class.py:174-216) ----------
// Count, mean, std, max, three accuracy thresholds and an EXACT median (the two middle elements averaged, as np.median) with TWO
// passes over the rows in TWO launches (rounds 2 / 3: a radix select of eight launches, 152 us per 1M rows; round 4: four launches, 41 us):
//   1. k_stats_window (all rows): per class the sum, the sum of squares, the maximum, and a histogram of the angles over a WINDOW of
//      bins on the top bits of the float64 pattern (non-negative doubles order like their bits): sixteen bins per octave from 2^-23 to
//      2^9 degrees (sixty-four for at most four classes, Win<FINE>), one bin below and one above.  The thresholds 7.5, 15 and 30 are
//      bin edges (1.875 x 2^k), so the three accuracies and the count are sums over bins -- no atomics of their own.  Workgroup-private
//      in LDS, flushed once -- into kStatReplicas copies by the workgroup's XCD: flushing into one copy, 256 same-address atomics in a
//      row on each of a few thousand words, was the larger half of the launch (tools/stats_anatomy.py; a same-address atomic at the
//      memory side takes 30-80 ns).
//   2. k_stats_collect (all rows): first the replicas' sum and, per class, the bins holding the lower and the upper middle element
//      (every workgroup for itself); then the rows of those bins (a few per cent of a class) are compacted:
//      staged in LDS (a cursor: no global atomic, no barrier in the loop), grouped by class, and appended to the class's stretch of
//      the candidate buffer -- the histogram says exactly how long each stretch is; one atomic per workgroup and class takes a share.
//      Then the workgroup draws a ticket, and workgroup c (c < ncls; further classes wrap around) FINISHES class c once every ticket
//      is drawn: the class's candidates -- a contiguous list -- go into LDS (when more than 16 384: after the first digit has thinned
//      them out), ONE 8-bit digit is voted on, and the <= 64 candidates per selection that share it are ranked by a wave (more: further
//      digits); the class's row of the result is written.  What crosses workgroups inside the launch -- the candidates -- is written with agent-scope stores (performed past the
//      XCDs' L2s before the ticket is drawn: no release fence, which round 4 measured at 4-9 us per launch) and read with agent-scope
//      loads.  The wait is bounded: a finishing workgroup whose launch-mates do not all arrive in time (they can only be queued behind
//      another kernel: the finishers hold ncls of the device's CUs, not all) selects over the rows of its class themselves -- slow, never
//      wrong, and no wave ever waits on a condition that cannot come.
// The workspace is ZERO-FILLED ONCE by the caller and every call leaves it zeroed (the finishers clear what their class used): round
// 4's zero-fill launch in front of every call is gone.
// Exact for every input: an edge bin (zeros, denormals, angles above 512 degrees) is selected on all 64 bits, and if a workgroup's
// staging overflows (more than 4096 of its rows inside the selected bins: e.g. two million equal angles -- one million over 256
// workgroups are exactly 4096 each and fit) the finishing workgroups select over the rows themselves (two sweeps, then from LDS).
// An empty class reports count 0 and NaN elsewhere; -0.0 counts as +0.0; negative angles are outside the contract (include/so3proj.h).
// What does NOT pay (measured, tools/stats_anatomy.py): one launch for both passes with the rows kept in registers -- the two grid-wide
// waits it needs cost what the launch boundary does (a ticket takes 3.5 us from the last workgroup's store to the first reader's
// load); the candidates' first digit voted by the collecting workgroups into a global sub-histogram -- 74 000 same-address atomics
// on 256 words added 24 us.
constexpr int kStatFields = 8;                     // count, mean, std, max, median, acc<30, acc<15, acc<7.5
constexpr int kMaxClasses = 64;
// The window at two widths: sixteen bins per octave (the top 16 bits of the pattern) for up to kMaxClasses classes, or -- FINE, for at most
// kFineClasses classes, whose histograms then take the same LDS -- sixty-four per octave (the top 18 bits): the rows of a selected bin are
// the candidates every later step handles, and with ONE class of a million rows a sixteenth of an octave held 22 000-74 000 of them
// (the class's single finishing workgroup: 30-63 us); a sixty-fourth holds a quarter of that.
constexpr int kFineClasses = 4;
template <bool FINE> struct Win {
    static constexpr int kShift = FINE ? 46 : 48;
    static constexpr int kBase = FINE ? 0x3E80 << 2 : 0x3E80;          // (bits >> kShift) of 2^-23
    static constexpr int kBins = FINE ? 2048 : 512;
    static constexpr int kHist = kBins + 2;                            // [0]: below the window, [kHist - 1]: above it (and +inf)
    static constexpr int kRow = (kHist + 3) / 4 * 4;                   // (rows padded to whole 16-byte loads)
    // bins [0, edge) hold exactly the angles below the threshold: 30, 15 and 7.5 are 1.875 x 2^k, i.e. edges of the 1/16-octave bins
    static constexpr int kEdge30 = ((0x403E - 0x3E80) << (FINE ? 2 : 0)) + 1, kEdge15 = ((0x402E - 0x3E80) << (FINE ? 2 : 0)) + 1,
                         kEdge7p5 = ((0x401E - 0x3E80) << (FINE ? 2 : 0)) + 1;
    static __device__ __forceinline__ int bin(unsigned long long key) {
        const int top = static_cast<int>(key >> kShift);
        return top < kBase ? 0 : (top >= kBase + kBins ? kHist - 1 : top - kBase + 1);
    }
    static __device__ __forceinline__ unsigned long long top16(int b) { return static_cast<unsigned long long>(kBase + b - 1) >> (FINE ? 2 : 0); }   // of an inner bin
};
constexpr int kHistWords = kMaxClasses * Win<false>::kRow;            // one replica's histograms (either width)
static_assert(kFineClasses * Win<true>::kRow <= kHistWords, "the fine histograms fit a replica");
constexpr unsigned int kCandCap = 1u << 20;
constexpr int kStatMaxWgs = 1024;
constexpr int kStatLdsKeys = 16384;                // candidates of one class that k_stats_finish keeps in LDS (128 KB + 16 KB of tags)
// The window pass's per-class sums and histograms exist kStatReplicas times, a workgroup adds into replica (its XCD's id) % kStatReplicas:
// 256 workgroups flushing ~100 bins per class into ONE copy were 256 atomics in a row on every address -- the flush was issued 3.9 us
// into the launch and performed 9-12.6 us into it, the larger half of the pass (stamps, docs/history/profiles/r05_stats_anatomy.txt).
#ifndef SO3_STAT_REPLICAS
#define SO3_STAT_REPLICAS 4
#endif
constexpr int kStatReplicas = SO3_STAT_REPLICAS;
static_assert(kStatReplicas >= 1 && kStatReplicas <= 16 && (kStatReplicas & (kStatReplicas - 1)) == 0, "SO3_STAT_REPLICAS: a power of two (stat_replica masks the XCD id with it)");
// Layout of the caller's workspace.  `acc` and `hist` are zero-filled once by the caller and left zeroed by every call (only
// k_stats_window adds into them, only a class's own finishing workgroup clears them).  The CONTROL words -- overflow, ticket,
// class_cursor -- are put to zero by the FIRST launch of every call (k_stats_window, workgroup 0): stream order puts that after every
// workgroup of the previous call, late ones included.  Round 5 cleared them at the END of the second launch, by the last class to
// finish: a finishing workgroup whose launch-mates had not arrived within its wait then cleared the words while those mates were
// still queued, and they added to the cleared words afterwards -- the next call started with a ticket above zero and trusted a
// half-filled candidate buffer (the advisor's finding; tests/test_gpu_parity.py::test_angle_stats_survives_timed_out_waits).
struct StatWork {
    double acc[kStatReplicas][kMaxClasses][4];     // sum, sumsq, max (bits), nan_count
    unsigned int overflow, ticket;                 // bit 0: some collecting workgroup's staging overflowed, bit 2: some finishing workgroup's wait timed out; collecting workgroups that have published their candidates
    unsigned int unused, pad;
    unsigned int class_cursor[kMaxClasses];        // k_stats_collect: how much of class c's stretch of the candidate buffer is taken
    unsigned int hist[kStatReplicas][kHistWords];  // class c's bins from c * Win<FINE>::kRow on
    unsigned char tag[kCandCap];                   // bit 0: counts for the lower middle element, bit 1: for the upper
    unsigned long long cand[kCandCap];             // class c's candidates: the rows of its selected bins, in a stretch whose place and length the histogram gives
};
constexpr unsigned int kStatRegion = 4096;         // candidates one workgroup of k_stats_collect can stage in LDS (48 KB)
static_assert(kStatRegion * 256u <= kCandCap, "what 256 workgroups can stage fits the buffer");

// (a <= 0: -0.0, whose pattern 0x8000... would order above every angle, counts as +0.0 too; negative angles are outside the contract)
__device__ __forceinline__ unsigned long long angle_key(double a) { return static_cast<unsigned long long>(__double_as_longlong(a <= 0 ? 0.0 : a)); }

#ifdef SO3_STATS_STAMP
#define STAT_STAMP(w, idx) do { if ((blockIdx.x == 0 || blockIdx.x == 100) && threadIdx.x == 0) (w)->cand[kCandCap - 64 + (blockIdx.x ? 32 : 0) + (idx)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define STAT_STAMP(w, idx) do { } while (0)
#endif
constexpr int kStatLdsClasses = 16;
constexpr int kStatBlock = 1024;
// Every row once: body(angle, class) -- two rows per thread and trip: one 16-byte and one 8-byte load where both arrays allow it
// from row `head` on (mode 0 / 1: head = 0 / 1 -- views like deg[1:], cls[1:] are 8 / 4 bytes off), two scalar loads each otherwise
// (mode 2); a leading and an odd last row by themselves.
template <class F>
__device__ __forceinline__ void stats_rows(const double *__restrict__ deg, const int32_t *__restrict__ cls, int64_t B, int mode, F &&body) {
    const int64_t head = mode == 1 ? 1 : 0;
    const int64_t pairs = B > head ? (B - head) / 2 : 0;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kStatBlock;
    auto fetch = [&](int64_t i, double2 &a, int2 &c) {
        c = make_int2(0, 0);
        if (mode == 2) {
            a.x = deg[2 * i]; a.y = deg[2 * i + 1];
            if (cls) { c.x = cls[2 * i]; c.y = cls[2 * i + 1]; }
        } else {
            a = reinterpret_cast<const double2 *>(deg + head)[i];
            if (cls) c = reinterpret_cast<const int2 *>(cls + head)[i];
        }
    };
    // two trips' loads in flight per thread: a million rows are two trips of the grid, and one at a time the second trip's loads waited
    // for the first one's LDS atomics (the launch is a few microseconds long: a memory round trip is a quarter of it)
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kStatBlock + threadIdx.x; i < pairs; i += 2 * stride) {
        double2 a0, a1 = make_double2(0.0, 0.0);
        int2 c0, c1 = make_int2(-1, -1);
        const bool second = i + stride < pairs;
        fetch(i, a0, c0);
        if (second) fetch(i + stride, a1, c1);
        body(a0.x, c0.x);
        body(a0.y, c0.y);
        if (second) { body(a1.x, c1.x); body(a1.y, c1.y); }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head == 1 && B > 0) body(deg[0], cls ? cls[0] : 0);
        if (B > head && ((B - head) & 1)) body(deg[B - 1], cls ? cls[B - 1] : 0);
    }
}

// Which replica of the sums and histograms this workgroup adds into: the id of the XCD it runs on (a speed matter only: any spread
// over the replicas gives the same totals).
__device__ __forceinline__ int stat_replica() {
    return static_cast<int>(__builtin_amdgcn_s_getreg((4 - 1) << 11 | 20) & (kStatReplicas - 1));        // hwreg(HW_REG_XCC_ID, 0, 4)
}

// LCLS = how many classes the workgroup's histograms hold: 16 (33 KB of counters) or all 64 the interface allows (132 KB of the CU's
// 160 KB).  The float64 sums go to 32 (8) lane-private LDS slots per class and field, the slot index fastest: a wave's 64 lanes then
// fall on 32 distinct bank pairs whatever their classes (sixteen slots were four-way conflicts: 11 us of a 30-us launch).
template <int LCLS, bool FINE>
__global__ __launch_bounds__(kStatBlock) void k_stats_window(const double *__restrict__ deg, const int32_t *__restrict__ cls, int ncls, StatWork *w,
                                                             int64_t B, int mode) {
    constexpr int kSlots = LCLS <= 16 ? 32 : 8;
    constexpr int kHistBins = Win<FINE>::kHist;
    static_assert(sizeof(unsigned int) * LCLS * kHistBins + sizeof(double) * LCLS * 4 * kSlots + 64 <= 160 * 1024, "k_stats_window: LDS budget of a gfx950 CU");
    __shared__ unsigned int sh[LCLS][kHistBins];
    __shared__ double sacc[LCLS][4][kSlots];
    STAT_STAMP(w, 16);
    if (blockIdx.x == 0) {        // the call's control words (StatWork): whatever the previous call's last workgroups left in them
        if (threadIdx.x < kMaxClasses) w->class_cursor[threadIdx.x] = 0u;
        if (threadIdx.x == kMaxClasses) { w->overflow = 0u; w->ticket = 0u; w->unused = 0u; }
    }
    for (int i = threadIdx.x; i < LCLS * kHistBins; i += kStatBlock) (&sh[0][0])[i] = 0;
    for (int i = threadIdx.x; i < ncls * 4 * kSlots; i += kStatBlock) (&sacc[0][0][0])[i] = 0.0;
    __syncthreads();
    STAT_STAMP(w, 17);
    const int slot = threadIdx.x & (kSlots - 1);
    stats_rows(deg, cls, B, mode, [&](double a, int c) {
        if (c < 0 || c >= ncls) return;
        if (a != a) { atomicAdd(&sacc[c][3][slot], 1.0); return; }
        atomicAdd(&sacc[c][0][slot], a);
        atomicAdd(&sacc[c][1][slot], a * a);
        const unsigned long long key = angle_key(a);
        atomicMax(reinterpret_cast<unsigned long long *>(&sacc[c][2][slot]), key);
        atomicAdd(&sh[c][Win<FINE>::bin(key)], 1u);
    });
    __syncthreads();
    STAT_STAMP(w, 18);
    const int rep = stat_replica();
    for (int i = threadIdx.x; i < ncls * kHistBins; i += kStatBlock) {
        const unsigned int v = sh[i / kHistBins][i % kHistBins];
        if (v) atomicAdd(&w->hist[rep][i / kHistBins * Win<FINE>::kRow + i % kHistBins], v);
    }
    for (int i = threadIdx.x; i < ncls * 4; i += kStatBlock) {
        const int c = i / 4, f = i % 4;
        if (f == 2) {
            unsigned long long m = 0;
            for (int k = 0; k < kSlots; ++k) { const unsigned long long v = static_cast<unsigned long long>(__double_as_longlong(sacc[c][2][k])); m = v > m ? v : m; }
            if (m) atomicMax(reinterpret_cast<unsigned long long *>(&w->acc[rep][c][2]), m);
        } else {
            double v = 0.0;
            for (int k = 0; k < kSlots; ++k) v += sacc[c][f][k];
            if (v != 0.0) atomicAdd(&w->acc[rep][c][f], v);
        }
    }
    STAT_STAMP(w, 19);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAT_STAMP(w, 20);
}

// What every workgroup of k_stats_collect derives for itself from the histograms (20 KB per ten classes, L2-resident): per class the
// window bins of the lower / upper middle element and the rank inside, the counts that are sums over bins, the class's stretch of
// the candidate buffer.
struct StatSel {
    int bin[2][kMaxClasses];                       // the window bin of the lower / upper middle element (-1: empty class)
    long long krem[2][kMaxClasses];                // its rank inside that bin
    double count[kMaxClasses];                     // rows of the class (NaN included)
    double acc[4][kMaxClasses];                    // sum, sum of squares, maximum, NaN count: the replicas' totals
    unsigned int below[3][kMaxClasses];            // non-NaN rows below 30 / 15 / 7.5
    unsigned int base[kMaxClasses], total[kMaxClasses];   // class c's candidates: cand[base, base + total)
};
// The replicas of the histograms are added up into LDS first (`scratch`: room for kSelChunk classes), every load a wave's 256
// consecutive bytes -- read by the lanes that scan them (nine bins apiece, 36 bytes apart, eight replicas: 72 loads of 18 cache lines
// each per class) the selection took 15 us.  Then a wave per class: both selections from one reading of the class's summed histogram,
// and how many candidates the class has in all (the rows of its one or two selected bins).
constexpr int kSelChunk = 32;
constexpr int kSelAhead = 2;
template <bool FINE>
__device__ __forceinline__ void stats_select(int ncls, const StatWork *w, StatSel &sel, unsigned int *scratch) {
    constexpr int kHistBins = Win<FINE>::kHist, kHistRow = Win<FINE>::kRow, kEdge30 = Win<FINE>::kEdge30, kEdge15 = Win<FINE>::kEdge15, kEdge7p5 = Win<FINE>::kEdge7p5;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int kPerLane = (kHistBins + 63) / 64;                         // 9 (33) bins per lane
    for (int c0 = 0; c0 < ncls; c0 += kSelChunk) {
        const int nc = ncls - c0 < kSelChunk ? ncls - c0 : kSelChunk;
        __syncthreads();
        const int quads = nc * kHistRow / 4;
        for (int i0 = threadIdx.x; i0 < quads; i0 += kSelAhead * kStatBlock) {        // 16 bytes per lane and load, kSelAhead x kStatReplicas loads in flight
            uint4 v[kSelAhead][kStatReplicas];
#pragma unroll
            for (int a = 0; a < kSelAhead; ++a) {
                const int i = i0 + a * kStatBlock;
#pragma unroll
                for (int r = 0; r < kStatReplicas; ++r) v[a][r] = reinterpret_cast<const uint4 *>(&w->hist[r][c0 * kHistRow])[i < quads ? i : i0];
            }
#pragma unroll
            for (int a = 0; a < kSelAhead; ++a) {
                const int i = i0 + a * kStatBlock;
                uint4 sum = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int r = 0; r < kStatReplicas; ++r) { sum.x += v[a][r].x; sum.y += v[a][r].y; sum.z += v[a][r].z; sum.w += v[a][r].w; }
                if (i < quads) reinterpret_cast<uint4 *>(scratch)[i] = sum;
            }
        }
        __syncthreads();
        for (int c = c0 + wave; c < c0 + nc; c += kStatBlock / 64) {
            const unsigned int *hc = scratch + (c - c0) * kHistRow;
            // (a lane's bins are read out of LDS again where it owns a selection: held in registers, the fine width's 33 spilled)
            auto count_of = [&](int j) { const int bin = kPerLane * lane + j; return bin < kHistBins ? hc[bin] : 0u; };
            unsigned int mine = 0, b30 = 0, b15 = 0, b7 = 0;
#pragma unroll 3
            for (int j = 0; j < kPerLane; ++j) {
                const int bin = kPerLane * lane + j;
                const unsigned int hj = count_of(j);
                mine += hj;
                b30 += bin < kEdge30 ? hj : 0u; b15 += bin < kEdge15 ? hj : 0u; b7 += bin < kEdge7p5 ? hj : 0u;
            }
            unsigned int incl = mine;                                       // inclusive prefix sum over the lanes
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            const long long n = static_cast<long long>(__shfl(incl, 63, 64));   // the non-NaN rows of the class
            const long long before = static_cast<long long>(incl - mine);
            int bin_of[2] = {-1, -1};
            unsigned int rows_of[2] = {0u, 0u};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long k = n > 0 ? (t == 0 ? (n - 1) / 2 : n / 2) : 0;
                const bool owner = n > 0 && k >= before && k < before + static_cast<long long>(mine);   // exactly one lane (the counts add up to n > k)
                int d = 0;
                long long kk = k - before;
                unsigned int hd = 0;
                if (owner) {
                    for (; d < kPerLane - 1; ++d) { const unsigned int v = count_of(d); if (kk < static_cast<long long>(v)) break; kk -= v; }
                    hd = count_of(d);
                    sel.bin[t][c] = kPerLane * lane + d;
                    sel.krem[t][c] = kk;
                }
                if (n <= 0 && lane == 0) { sel.bin[t][c] = -1; sel.krem[t][c] = 0; }
                const unsigned long long who = __builtin_amdgcn_ballot_w64(owner);
                if (who != 0) {                                             // (wave-uniform)
                    const int src = __builtin_ctzll(who);
                    bin_of[t] = __shfl(kPerLane * lane + d, src, 64);
                    rows_of[t] = __shfl(hd, src, 64);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { b30 += __shfl_xor(b30, off, 64); b15 += __shfl_xor(b15, off, 64); b7 += __shfl_xor(b7, off, 64); }
            if (lane == 0) {
                double a0 = 0.0, a1 = 0.0, a3 = 0.0;
                unsigned long long a2 = 0;
                for (int r = 0; r < kStatReplicas; ++r) {
                    a0 += w->acc[r][c][0]; a1 += w->acc[r][c][1]; a3 += w->acc[r][c][3];
                    const unsigned long long v = static_cast<unsigned long long>(__double_as_longlong(w->acc[r][c][2]));
                    a2 = v > a2 ? v : a2;
                }
                sel.acc[0][c] = a0; sel.acc[1][c] = a1; sel.acc[2][c] = __longlong_as_double(static_cast<long long>(a2)); sel.acc[3][c] = a3;
                sel.count[c] = static_cast<double>(n) + a3;
                sel.below[0][c] = b30; sel.below[1][c] = b15; sel.below[2][c] = b7;
                sel.total[c] = rows_of[0] + (bin_of[1] != bin_of[0] ? rows_of[1] : 0u);
            }
        }
    }
    __syncthreads();
}

// agent-scope accesses to the candidate buffer: written and read inside ONE launch by workgroups on different XCDs
__device__ __forceinline__ void put_candidate(StatWork *w, unsigned int at, unsigned long long key, unsigned char tag) {
    __hip_atomic_store(&w->cand[at], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&w->tag[at], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long get_candidate(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned int get_tag(const unsigned char *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

#ifndef SO3_STAT_SPINS
#define SO3_STAT_SPINS 16384                       // x ~0.6 us: how long a finishing workgroup waits for its launch-mates' tickets before it helps itself
#endif                                             // (0 in the test build poseestimation_amd/libso3proj_spins0.so: every wait times out at once)
constexpr unsigned int kStatSpins = SO3_STAT_SPINS;
#ifndef SO3_STAT_GRID_MULT
#define SO3_STAT_GRID_MULT 1
#endif

// One class, by the whole workgroup: the class's candidates (a contiguous stretch of the buffer; into LDS when they fit), both middle
// elements by ONE radix select of 8-bit digits -- two (prefix, rank) states side by side, they part where the two elements differ --
// then the class's row of the result (np.mean / np.std / np.max / np.median / the thresholds), and the class's part of the workspace
// back to zero.  `overflow`: the candidate buffer is not to be trusted (a staging overflow somewhere, or launch-mates that did not
// arrive): select over the rows of the class themselves.
template <bool FINE>
__device__ __forceinline__ void stats_finish_class(int c, const double *__restrict__ deg, const int32_t *__restrict__ cls, StatWork *w, int64_t B,
                                                   double *__restrict__ stats, const StatSel &sel, bool overflow_in, unsigned long long *lkey,
                                                   unsigned char *ltag, unsigned int (*hh)[256]) {
    __shared__ unsigned long long s_prefix[2];
    __shared__ long long s_k[2];
    __shared__ unsigned int s_rem[2], s_cur, s_nsurv[2];
    __shared__ unsigned long long s_surv[2][64];
    const double n = sel.count[c], nan = sel.acc[3][c], m = n - nan;
    const int bins[2] = {sel.bin[0][c], sel.bin[1][c]};
    const unsigned int total = sel.total[c];                            // the class's candidates
    const unsigned long long *cand = w->cand + sel.base[c];
    const unsigned char *ctag = w->tag + sel.base[c];
    // (a stretch that would leave the buffer can only belong to a call in which some workgroup overflowed; the flag is set then)
    const bool overflow = overflow_in || static_cast<unsigned long long>(sel.base[c]) + total > kCandCap;
    constexpr int kAhead = 8;                                           // loads in flight per thread: the workgroup is alone on its CU
    bool cached = m > 0 && !overflow && total <= static_cast<unsigned int>(kStatLdsKeys);      // (workgroup-uniform throughout)
    unsigned int held = total;                                                                // how many candidates LDS holds once cached
    __syncthreads();                                                    // (LDS of the previous phase / class is free from here)
    STAT_STAMP(w, 8);
    if (cached) {
        // (eight candidates' loads in flight per thread, as in every_far_candidate below: one at a time -- each agent-scope load followed by
        // its LDS store -- a class's 7 400 candidates took eight round trips to memory, 4.4 us)
        for (unsigned int i0 = threadIdx.x; i0 < total; i0 += kAhead * kStatBlock) {
            unsigned long long key[kAhead];
            unsigned int which[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const unsigned int i = i0 + j * kStatBlock;
                key[j] = get_candidate(cand + (i < total ? i : i0));
                which[j] = get_tag(ctag + (i < total ? i : i0));
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const unsigned int i = i0 + j * kStatBlock;
                if (i < total) { lkey[i] = key[j]; ltag[i] = static_cast<unsigned char>(which[j]); }
            }
        }
        __syncthreads();
    }
    STAT_STAMP(w, 9);
    double middle[2] = {0.0, 0.0};
    if (m > 0) {
        const bool edge[2] = {bins[0] == 0 || bins[0] == Win<FINE>::kHist - 1, bins[1] == 0 || bins[1] == Win<FINE>::kHist - 1};
        if (threadIdx.x < 2) {
            const int t = threadIdx.x;
            s_prefix[t] = edge[t] ? 0ull : Win<FINE>::top16(bins[t]);     // (FINE: the candidates share two more bits; the first digit finds them out)
            s_k[t] = sel.krem[t][c];
        }
        __syncthreads();
        // digits from bit 56 down when an edge bin is involved (it does not fix the top 16 bits), else from bit 40; a selection whose
        // bin fixes them sits out the two top digits
        for (int shift = (edge[0] || edge[1]) ? 56 : 40; shift >= 0; shift -= 8) {
            for (int i = threadIdx.x; i < 512; i += kStatBlock) (&hh[0][0])[i] = 0;
            __syncthreads();
            const bool active[2] = {edge[0] || shift <= 40, edge[1] || shift <= 40};
            const unsigned long long prefix[2] = {s_prefix[0], s_prefix[1]};
            auto vote = [&](unsigned long long key, unsigned int which) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (active[t] && (which >> t & 1u) && (shift == 56 || (key >> (shift + 8)) == prefix[t])) atomicAdd(&hh[t][(key >> shift) & 0xFF], 1u);
            };
            // every candidate of the class (or, after an overflow, every row of it inside the selected bins): f(key, which selections it counts for)
            // (eight loads in flight per thread: the workgroup is alone on its CU, and one load at a time -- the votes' LDS atomics keep the
            // compiler from overlapping iterations -- made a pass over 44 000 candidates 43 round trips to memory, 20 us)
            auto every_far_candidate = [&](auto &&f) {
                if (!overflow) {
                    for (unsigned int i0 = threadIdx.x; i0 < total; i0 += kAhead * kStatBlock) {
                        unsigned long long key[kAhead];
                        unsigned int which[kAhead];
#pragma unroll
                        for (int j = 0; j < kAhead; ++j) {
                            const unsigned int i = i0 + j * kStatBlock;
                            key[j] = get_candidate(cand + (i < total ? i : i0));
                            which[j] = i < total ? get_tag(ctag + i) : 0u;
                        }
#pragma unroll
                        for (int j = 0; j < kAhead; ++j)
                            if (which[j]) f(key[j], which[j]);
                    }
                } else {
                    for (int64_t i0 = threadIdx.x; i0 < B; i0 += kAhead * kStatBlock) {
                        double a[kAhead];
                        int cc[kAhead];
#pragma unroll
                        for (int j = 0; j < kAhead; ++j) {
                            const int64_t i = i0 + j * kStatBlock;
                            a[j] = deg[i < B ? i : i0];
                            cc[j] = i < B ? (cls ? cls[i] : 0) : -1;
                        }
#pragma unroll
                        for (int j = 0; j < kAhead; ++j) {
                            if (cc[j] != c || a[j] != a[j]) continue;
                            const unsigned long long key = angle_key(a[j]);
                            const int bin = Win<FINE>::bin(key);
                            const unsigned int which = (bin == bins[0] ? 1u : 0u) | (bin == bins[1] ? 2u : 0u);
                            if (which) f(key, which);
                        }
                    }
                }
            };
            if (cached) {
                for (unsigned int i = threadIdx.x; i < held; i += kStatBlock) vote(lkey[i], ltag[i]);
            } else {
                every_far_candidate(vote);
            }
            __syncthreads();
            if (shift == 40) STAT_STAMP(w, 10);
            if (threadIdx.x < 128) {                                    // wave t: the digit holding selection t's rank -- 256 bins, four per lane, a wave prefix sum
                const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
                unsigned int h[4], mine = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = hh[t][4 * lane + j]; mine += h[j]; }
                unsigned int incl = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned int up = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += up;
                }
                const long long before = static_cast<long long>(incl - mine), k = s_k[t];
                if (active[t] && k >= before && k < before + static_cast<long long>(mine)) {
                    long long kk = k - before;
                    unsigned int d = 0;
                    for (; d < 3; ++d) { if (kk < static_cast<long long>(h[d])) break; kk -= h[d]; }
                    s_k[t] = kk;
                    s_prefix[t] = (prefix[t] << 8) | static_cast<unsigned long long>(4 * lane + d);
                    s_rem[t] = h[d];                                    // how many candidates share the element's digits so far
                }
            }
            if (threadIdx.x == 0) s_cur = 0;
            if (threadIdx.x < 2) s_nsurv[threadIdx.x] = 0;
            __syncthreads();
            // Few enough left (a digit of 4 400 candidates leaves ~17): the candidates that share the digits chosen so far -- at most 64 per
            // selection -- are gathered, and ONE wave per selection ranks them directly (a lane per survivor, 64 comparisons each): the
            // remaining four or five digit passes, a microsecond each, are not run.
            auto rank_survivors = [&]() {
                const unsigned long long np[2] = {s_prefix[0], s_prefix[1]};
                for (unsigned int i = threadIdx.x; i < held; i += kStatBlock) {
                    const unsigned long long key = lkey[i];
                    const unsigned int which = ltag[i];
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        if ((which >> t & 1u) && (key >> shift) == np[t]) s_surv[t][atomicAdd(&s_nsurv[t], 1u)] = key;     // (<= s_rem[t] <= 64 of them)
                }
                __syncthreads();
                if (threadIdx.x < 128) {
                    const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
                    const unsigned int cnt = __builtin_amdgcn_readfirstlane(s_nsurv[t]);
                    const unsigned long long mine = lane < static_cast<int>(cnt) ? s_surv[t][lane] : ~0ull;
                    const unsigned int mine_lo = static_cast<unsigned int>(mine), mine_hi = static_cast<unsigned int>(mine >> 32);
                    long long rank = 0;
                    for (unsigned int j = 0; j < cnt; ++j) {            // lane j's key through the scalar unit (out of LDS: one ~100-cycle read per step, 3 us for 30 survivors)
                        const unsigned long long other = static_cast<unsigned long long>(static_cast<unsigned int>(__builtin_amdgcn_readlane(mine_hi, j))) << 32 |
                                                         static_cast<unsigned int>(__builtin_amdgcn_readlane(mine_lo, j));
                        rank += (other < mine || (other == mine && static_cast<int>(j) < lane)) ? 1 : 0;
                    }
                    if (lane < static_cast<int>(cnt) && rank == s_k[t]) s_prefix[t] = mine;       // exactly one lane: the ranks are a permutation of 0 .. cnt-1
                }
                __syncthreads();
            };
            if (cached && shift > 0 && active[0] && active[1] && s_rem[0] <= 64u && s_rem[1] <= 64u) {
                rank_survivors();
                break;                                                  // s_prefix holds both elements, all 64 bits
            }
            // Candidates that did not fit LDS (one class of a million rows: 44 000 in its middle bin; or the rows themselves after an
            // overflow): once the digits chosen so far leave few enough, those move into LDS and the remaining digits are read there --
            // two passes over the far candidates instead of six (eight).
            if (!cached && active[0] && active[1] && shift > 0 && s_rem[0] + s_rem[1] <= static_cast<unsigned int>(kStatLdsKeys)) {
                const unsigned long long np[2] = {s_prefix[0], s_prefix[1]};
                every_far_candidate([&](unsigned long long key, unsigned int which) {
                    const unsigned int keep = ((which & 1u) && (key >> shift) == np[0] ? 1u : 0u) | ((which & 2u) && (key >> shift) == np[1] ? 2u : 0u);
                    if (keep) {
                        const unsigned int at = atomicAdd(&s_cur, 1u);
                        lkey[at] = key;                                 // (at < s_rem[0] + s_rem[1] <= kStatLdsKeys)
                        ltag[at] = static_cast<unsigned char>(keep);
                    }
                });
                __syncthreads();
                held = s_cur;
                cached = true;
                if (s_rem[0] <= 64u && s_rem[1] <= 64u) {
                    rank_survivors();
                    break;
                }
            }
        }
        STAT_STAMP(w, 11);
        middle[0] = __longlong_as_double(static_cast<long long>(s_prefix[0]));
        middle[1] = __longlong_as_double(static_cast<long long>(s_prefix[1]));
    }
    if (threadIdx.x == 0) {
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        double *o = stats + c * kStatFields;
        // an empty class (m == 0 == n): count 0 and NaN for every other field, as the oracle reports it (0/0 below); a class holding
        // +inf: mean and max +inf, var = inf - inf = NaN and std NaN, as np.std
        const double mean = sel.acc[0][c] / m;
        o[0] = n;
        o[1] = nan > 0 ? qnan : mean;
        const double var = sel.acc[1][c] / m - mean * mean;
        o[2] = nan > 0 ? o[1] : sqrt(var < 0 ? 0.0 : var);                       // np.std: population standard deviation (a NaN stays one)
        o[3] = (nan > 0 || m <= 0) ? qnan : sel.acc[2][c];
        o[4] = (nan > 0 || m <= 0) ? qnan : 0.5 * (middle[0] + middle[1]);
        o[5] = sel.below[0][c] / n; o[6] = sel.below[1][c] / n; o[7] = sel.below[2][c] / n;   // (x < t).sum() / len(x)
    }
    __syncthreads();
    // the class's part of the workspace back to zero (the next call's launches come later on the stream: plain stores)
    for (int i = threadIdx.x; i < kStatReplicas * Win<FINE>::kHist; i += kStatBlock) w->hist[i / Win<FINE>::kHist][c * Win<FINE>::kRow + i % Win<FINE>::kHist] = 0u;
    if (threadIdx.x < 4 * kStatReplicas) w->acc[threadIdx.x >> 2][c][threadIdx.x & 3] = 0.0;
}

// The rows of the selected bins: staged in LDS (a cursor: no global atomic, no barrier in the loop), then grouped by class -- a
// counting sort in LDS -- and appended to the class's stretch of the candidate buffer.  The stretches are exact: the histogram says how
// many rows each class has in its selected bins, every workgroup derives the same offsets from it, and a workgroup takes its share of
// a stretch with ONE atomic per class it holds; a finishing workgroup then reads a contiguous list.  Then the ticket, and the
// finishing of the classes this workgroup answers for (see the head of this section).
template <bool FINE>
__global__ __launch_bounds__(kStatBlock) void k_stats_collect(const double *__restrict__ deg, const int32_t *__restrict__ cls, int ncls, StatWork *w,
                                                              int64_t B, int mode, double *__restrict__ stats) {
    // the finishing phase's candidates (128 KB + 16 KB); the collecting phase stages its own rows in the front of the same arrays
    __shared__ __attribute__((aligned(16))) unsigned long long lkey[kStatLdsKeys];
    __shared__ __attribute__((aligned(8))) unsigned char ltag[kStatLdsKeys];
    __shared__ unsigned int hh[2][256];
    __shared__ StatSel sel;
    __shared__ unsigned int ccount[kMaxClasses], cstart[kMaxClasses], ccur[kMaxClasses], gbase[kMaxClasses];
    __shared__ unsigned int cur, s_state;
    static_assert(kStatRegion <= kStatLdsKeys && kStatRegion * 2 <= kStatLdsKeys, "the staging area fits the finishing phase's arrays");
    unsigned long long *skey = lkey;
    unsigned short *stag = reinterpret_cast<unsigned short *>(ltag);
    STAT_STAMP(w, 0);
    static_assert((FINE ? kFineClasses : kSelChunk) * Win<FINE>::kRow * sizeof(unsigned int) <= sizeof(unsigned long long) * kStatLdsKeys, "the selection's scratch fits the candidates' array");
    stats_select<FINE>(ncls, w, sel, reinterpret_cast<unsigned int *>(lkey));
    for (int i = threadIdx.x; i < ncls; i += kStatBlock) ccount[i] = 0;
    if (threadIdx.x == 0) cur = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int at = 0;
        for (int c = 0; c < ncls; ++c) {
            sel.base[c] = at;
            at = at + sel.total[c] < at ? 0xFFFFFFFFu : at + sel.total[c];      // (saturating: beyond the buffer nothing is written anyway)
        }
    }
    STAT_STAMP(w, 1);
    stats_rows(deg, cls, B, mode, [&](double a, int c) {
        if (c < 0 || c >= ncls || a != a) return;
        const unsigned long long key = angle_key(a);
        const int bin = Win<FINE>::bin(key);
        const unsigned int t0 = bin == sel.bin[0][c] ? 1u : 0u, t1 = bin == sel.bin[1][c] ? 1u : 0u;
        if (t0 | t1) {
            const unsigned int at = atomicAdd(&cur, 1u);
            if (at < kStatRegion) { skey[at] = key; stag[at] = static_cast<unsigned short>(c | t0 << 8 | t1 << 9); }
        }
    });
    __syncthreads();
    STAT_STAMP(w, 2);
    const unsigned int n = cur < kStatRegion ? cur : kStatRegion;
    if (threadIdx.x == 0 && cur > kStatRegion) atomicOr(&w->overflow, 1u);     // (the finishing workgroups then select over the rows themselves)
    for (unsigned int i = threadIdx.x; i < n; i += kStatBlock) atomicAdd(&ccount[stag[i] & 0xFF], 1u);
    __syncthreads();
    if (threadIdx.x < static_cast<unsigned>(ncls)) {
        const int c = threadIdx.x;
        gbase[c] = ccount[c] ? sel.base[c] + atomicAdd(&w->class_cursor[c], ccount[c]) : 0u;
    }
    if (threadIdx.x == 0) {
        unsigned int at = 0;
        for (int c = 0; c < ncls; ++c) { cstart[c] = at; ccur[c] = at; at += ccount[c]; }
    }
    __syncthreads();
    for (unsigned int i = threadIdx.x; i < n; i += kStatBlock) {
        const int c = stag[i] & 0xFF;
        const unsigned int at = gbase[c] + (atomicAdd(&ccur[c], 1u) - cstart[c]);
        if (at < kCandCap) put_candidate(w, at, skey[i], static_cast<unsigned char>(stag[i] >> 8));     // (past the buffer only after some workgroup has overflowed)
    }
    // every store of this workgroup has been performed (agent scope: past the L2) before its ticket is drawn
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    STAT_STAMP(w, 3);
    if (static_cast<int>(blockIdx.x) >= ncls) {                          // not a finishing workgroup: ticket and out
        if (threadIdx.x == 0) atomicAdd(&w->ticket, 1u);
        return;
    }
    if (threadIdx.x == 0) {
        atomicAdd(&w->ticket, 1u);
        unsigned int spins = 0;
        while (__hip_atomic_load(&w->ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x && spins < kStatSpins) {
            __builtin_amdgcn_s_sleep(4);
            ++spins;
        }
        const bool all_in = __hip_atomic_load(&w->ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= gridDim.x;
        // A wait that timed out is made known to every finishing workgroup that comes later, BEFORE this one clears anything (the
        // returning atomic has been performed when its value is here): a launch-mate that starts after this workgroup has put its
        // class's histogram back to zero derives other stretches of the candidate buffer than everyone else did, and a finishing
        // workgroup that then finds all tickets in must not trust that buffer.
        unsigned int flags = all_in ? 0u : atomicOr(&w->overflow, 4u) | 4u;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        flags |= __hip_atomic_load(&w->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_state = flags;
    }
    __syncthreads();
    STAT_STAMP(w, 4);
    const bool overflow = s_state != 0u;
    for (int c = blockIdx.x; c < ncls; c += gridDim.x) {
        stats_finish_class<FINE>(c, deg, cls, w, B, stats, sel, overflow, lkey, ltag, hh);
        __syncthreads();
        STAT_STAMP(w, 5);
    }
    // (ticket, overflow and the cursors stay as they are: the next call's first launch clears them, see StatWork)
}

inline unsigned grid_for(int64_t B) { return static_cast<unsigned>((B + kBlock - 1) / kBlock); }
inline unsigned capped_grid(int64_t B, unsigned cap) { const unsigned t = grid_for(B); return t < cap ? t : cap; }
inline unsigned persistent_grid(int64_t B) { return capped_grid(B, 2048u); }

// Resident waves per SIMD the two-input kernels K2 / K3 / K1+K4 are built for (K1 runs at 3): their rare Jacobi branch keeps the frames
// live across the backward (190-216 VGPRs).  Round 4 measured what three waves would buy with that branch out of the loop
// (docs/history/profiles/r04_row_number_queue_ab.txt): K2 at 168 VGPRs, spill-free, 22.10 us against 22.01 us at two -- occupancy is not what bounds it.
#ifndef SO3_BLOCK_K1
#define SO3_BLOCK_K1 256
#endif
#ifndef SO3_WPS_K1
#define SO3_WPS_K1 3
#endif
#ifndef SO3_BLOCK_K3
#define SO3_BLOCK_K3 256
#endif
#ifndef SO3_BLOCK_K14
#define SO3_BLOCK_K14 256
#endif
#ifndef SO3_WPS_K2
#define SO3_WPS_K2 2
#endif
#ifndef SO3_WPS_K3
#define SO3_WPS_K3 2
#endif
#ifndef SO3_WPS_K14
#define SO3_WPS_K14 2
#endif
#ifndef SO3_K4B_NPL                  // K4b's launch shape (the metrics' backward)
#define SO3_K4B_NPL 2
#define SO3_K4B_WPS 3
#define SO3_K4B_BLOCK 256
#endif

#ifndef SO3_INV_NPL                  // the inverse maps' launch shape (so3_mat_to_quat_*, so3_logmap_*, so3_mat_to_euler_*, so3_relative_log_*)
#define SO3_INV_NPL 2
#define SO3_INV_WPS 4
#define SO3_RELLOG_BWD_WPS 3
#endif

#define SO3_CHECK_ARGS(cond, name) \
    do { if (!(cond)) return fail(SO3_ERR_INVALID, name); } while (0)
#define SO3_MAX_B (INT64_C(2147483647) * kBlock)
// The cloud entry points' dimensions: up to 2^31 clouds of 1..max points and, where there is one, a second extent of 1..max; and K.
inline bool cloud_dims_ok(int64_t B, int32_t N, int32_t M = 1, int32_t max = SO3_ADD_S_MAX_N) {
    return B >= 0 && B <= (INT64_C(1) << 31) && N >= 1 && N <= max && M >= 1 && M <= max;
}
inline bool knn_k_ok(int32_t K) { return K >= 1 && K <= SO3_KNN_MAX_K; }

// Compute units of the current device (queried once per device; 256 on an MI355X in SPX mode, fewer in CPX / DPX partitions).
inline int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

using so3::with_flags;
using so3::with_value;
using so3::kernel_label;
constexpr double kDegPerRad = 57.295779513082320876798154814105;      // 180/pi

// A wave per row at a time: the workgroups B rows need, at most per_cu per compute unit.
inline unsigned wave_rows_grid(int64_t B, int per_cu) {
    return static_cast<unsigned>(std::min<int64_t>((B + kBlock / 64 - 1) / (kBlock / 64), static_cast<int64_t>(device_cus()) * per_cu));
}
// The cloud kernels' launch shape on this device (so3::clouds_per_wave).
struct CloudShape { int per_wave; int64_t blocks; };
inline CloudShape cloud_shape(int64_t B) {
    const int per_wave = so3::clouds_per_wave(B, device_cus());
    return {per_wave, so3::cloud_blocks(B, per_wave)};
}
// Zero `bytes` at p in stream order; `what` names the call in so3_last_error() when the runtime refuses.
inline int zero_async(void *p, size_t bytes, hipStream_t s, const char *what) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, s);
    return e == hipSuccess ? 0 : fail(static_cast<int>(e), what);
}

// Launch an operation on the streaming engine: NPL matrices per lane, WPS resident waves per SIMD, BLOCK threads.
// The name of a k_rows instantiation as a profiler prints it: the runtime's own (mangled) name of the kernel behind the host
// stub, demangled, without the "void " in front and the parameter list behind.
thread_local const char *g_last_kernel = "";
thread_local char g_kernel_label[64] = "";        // so3_last_kernel() of the launchers outside the engine: kernel_label writes it
template <class... Args> inline void name_kernel(const char *name, Args... args) {
    g_last_kernel = kernel_label(g_kernel_label, sizeof g_kernel_label, name, args...);
}
template <class Op, int NPL, int WPS, int BLOCK>
const char *rows_kernel_name(hipStream_t s) {
    static const std::string name = [s] {
        const char *mangled = hipKernelNameRefByPtr(reinterpret_cast<const void *>(&so3::k_rows<Op, NPL, WPS, BLOCK, false>), s);
        if (mangled == nullptr) return std::string("so3::k_rows<?>");
        int status = 0;
        char *d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
        std::string full = (status == 0 && d != nullptr) ? d : mangled;
        free(d);
        if (full.rfind("void ", 0) == 0) full.erase(0, 5);
        int depth = 0;                                         // cut at the '(' that opens the parameter list
        for (size_t i = 0; i < full.size(); ++i) {
            if (full[i] == '<') ++depth;
            else if (full[i] == '>') --depth;
            else if (full[i] == '(' && depth == 0) { full.erase(i); break; }
        }
        return full;
    }();
    return name.c_str();
}

// The grid of a launch of `rounds` rounds: a wave per round up to the CUs' wave slots.
template <int NPL, int WPS, int BLOCK, class Op>
unsigned rows_grid(int64_t rounds) {
    constexpr int kWaves = BLOCK / 64;
    const int64_t want = (rounds + kWaves - 1) / kWaves;
    int64_t cap = static_cast<int64_t>(device_cus()) * 4 * WPS / kWaves;          // CUs x 4 SIMDs x WPS wave slots
    if (Op::kFixedRounds > 0) {                                                    // not persistent: a wave per k consecutive rounds, back-filled
        const int64_t waves = (rounds + Op::kFixedRounds - 1) / Op::kFixedRounds;
        cap = (waves + kWaves - 1) / kWaves;
    }
    return static_cast<unsigned>(want < cap ? want : cap);
}

// `rounds` < 0: the rounds of one array of nunits units; a segmented operation (Op::kSegmented) passes its table's total.
template <int NPL, int WPS, int BLOCK, class Op>
void launch_rows(const Op &op, int64_t nunits, hipStream_t s, int64_t rounds = -1) {
    g_last_kernel = rows_kernel_name<Op, NPL, WPS, BLOCK>(s);
    if (rounds < 0) rounds = (nunits + NPL - 1) / NPL;
    const dim3 grid(rows_grid<NPL, WPS, BLOCK, Op>(rounds)), block(BLOCK);
    hipLaunchKernelGGL((so3::k_rows<Op, NPL, WPS, BLOCK, false>), grid, block, 0, s, op, nunits, nullptr);
}

// Rows [0, 64*nunits) go to the engine when every pointer is dword aligned (every float32 array is; a bfloat16 view that
// starts at an odd row is not); the rest to the tile kernels.  The engine's 16-byte buffer loads and stores need dword
// alignment only: a view that starts at row 1 of a tensor (36 B in: 4 mod 16) streams like an aligned one -- round 1
// sent such views, e.g. the shards of an uneven split, to the one-row-per-thread kernels.
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline int64_t stream_units(int64_t B, std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (p != nullptr && !aligned4(p)) return 0;
    if (B / so3::kUnitRows > 0x7fffffff - 4096) return 0;      // the engine numbers its rounds in 32 bits (1.3e11 rows: 5 TB of float32 input)
    return B / so3::kUnitRows;
}
// A call's rows between the two: nunits whole units = rows [0, done) on the engine, the last `rest` rows on the tile kernels.
struct Split {
    int64_t nunits, done, rest;
    Split(int64_t B, std::initializer_list<const void *> ptrs)
        : nunits(B > 0 ? stream_units(B, ptrs) : 0), done(nunits * so3::kUnitRows), rest(B - done) {}
};

// A float32 row operation with up to three inputs and up to two outputs: whole units on the streaming engine, the rest
// (and everything when a pointer is not 16-byte aligned) one row per thread.
template <int NPL, int WPS, int BLOCK, class Op>
int run_row_op(Op op, int64_t B, hipStream_t s, const char *what) {
    const Split sp(B, {op.in0, op.in1, op.in2, op.out0, op.out1});
    if (sp.nunits > 0) launch_rows<NPL, WPS, BLOCK>(op, sp.nunits, s);
    if (sp.rest > 0) {
        const int64_t done = sp.done, rest = sp.rest;
        Op t = op;
        t.in0 = static_cast<const float *>(op.in0) + done * Op::kIn0N;
        if (Op::kIn1 != 0) t.in1 = static_cast<const float *>(op.in1) + done * Op::kIn1N;
        if (Op::kIn2 != 0) t.in2 = static_cast<const float *>(op.in2) + done * Op::kIn2N;
        t.out0 = static_cast<float *>(op.out0) + done * Op::kOut0N;
        if (Op::kOut1 != 0) t.out1 = static_cast<float *>(op.out1) + done * Op::kOut1N;
        hipLaunchKernelGGL((k_op_rows<Op>), dim3(grid_for(rest)), dim3(kBlock), 0, s, t, rest);
    }
    return check_launch(what);
}

template <class T> inline T *advance(T *p, int64_t elems) { return p ? p + elems : nullptr; }
inline const void *advance_bytes(const void *p, int64_t bytes) { return p ? static_cast<const char *>(p) + bytes : nullptr; }
inline void *advance_bytes(void *p, int64_t bytes) { return p ? static_cast<char *>(p) + bytes : nullptr; }

// ---- K1 --------------------------------------------------------------------------------------------
// The buffer pairs of one launch of K1's engine kernel as the host keeps them (so3::OpProject's segment table is built from it).
struct K1Run {
    const void *in[so3::kMaxSegments];
    float *out[so3::kMaxSegments];
    int64_t rows[so3::kMaxSegments];          // whole units each
    int n = 0;
    int elem_bytes = 4;                       // of the input: 4 = float32, 2 = bfloat16 (different kernels)
};
constexpr int64_t kMaxRounds32 = (INT64_C(1) << 30) - 2048;      // what stream_units admits for one array: round numbers stay 32-bit
inline int64_t k1_rounds(int64_t rows) { return (rows / so3::kUnitRows + 1) / 2; }
inline int64_t k1_rounds(const K1Run &run) {
    int64_t r = 0;
    for (int i = 0; i < run.n; ++i) r += k1_rounds(run.rows[i]);
    return r;
}
inline bool bytes_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) && b0 < a0 + static_cast<uintptr_t>(na);
}

// What this thread's last engine-only K1 call left in the graph being captured: the kernel node and the segments it runs.
struct K1Captured {
    unsigned long long capture_id = 0;
    hipGraphNode_t node = nullptr;
    K1Run run;
};
thread_local K1Captured g_k1_captured;
thread_local int64_t g_k1_fused = 0;
std::atomic<int> g_capture_fusion{1};

// May the call (M, R, B rows, elem_bytes) on a stream whose capture is `capture_id` and whose capture dependencies are `ndeps` nodes
// (the first one `dep0`) be folded into the recorded node?  Pure logic: no runtime call, no pointer is dereferenced.
//   * same capture, and the recorded node is the stream's ONLY dependency: nothing was captured on this stream since, and whatever must
//     precede this call is upstream of that node already (anything else would be a second dependency);
//   * same instantiation, room in the table, round numbers still 32-bit;
//   * no hazard between the segments, which run concurrently inside the kernel: the new input overlaps no recorded output (read after
//     write), the new output overlaps no recorded output (write after write) and no recorded input (write after read).
bool k1_may_fuse(const K1Captured &rec, unsigned long long capture_id, size_t ndeps, hipGraphNode_t dep0, int elem_bytes,
                 const void *M, const void *R, int64_t B) {
    if (rec.node == nullptr || rec.run.n < 1 || rec.capture_id != capture_id) return false;
    if (ndeps != 1 || dep0 != rec.node) return false;
    if (rec.run.elem_bytes != elem_bytes) return false;
    if (rec.run.n >= so3::kMaxSegments) return false;
    if (k1_rounds(rec.run) + k1_rounds(B) > kMaxRounds32) return false;
    const int64_t in_bytes = B * 9 * elem_bytes, out_bytes = B * 9 * 4;
    for (int i = 0; i < rec.run.n; ++i) {
        const int64_t rin = rec.run.rows[i] * 9 * rec.run.elem_bytes, rout = rec.run.rows[i] * 9 * 4;
        if (bytes_overlap(M, in_bytes, rec.run.out[i], rout)) return false;
        if (bytes_overlap(R, out_bytes, rec.run.out[i], rout)) return false;
        if (bytes_overlap(R, out_bytes, rec.run.in[i], rin)) return false;
    }
    return true;
}

template <int EB> so3::OpProject<EB, false> k1_op(const K1Run &run) {
    so3::OpProject<EB, false> op;
    for (int i = 0; i < run.n; ++i) op.template add_segment<2>(run.in[i], run.out[i], run.rows[i] / so3::kUnitRows);
    return op;
}
template <int EB> void k1_launch(const K1Run &run, hipStream_t s) {
    const so3::OpProject<EB, false> op = k1_op<EB>(run);
    int64_t units = 0;
    for (int i = 0; i < run.n; ++i) units += run.rows[i] / so3::kUnitRows;
    launch_rows<2, SO3_WPS_K1, SO3_BLOCK_K1>(op, units, s, op.total_rounds);
}
// The recorded kernel node runs `run` from now on: a new argument block and the grid of its rounds.
template <int EB> hipError_t k1_rewrite_node(hipGraphNode_t node, const K1Run &run, hipStream_t s) {
    typedef so3::OpProject<EB, false> Op;
    Op op = k1_op<EB>(run);
    int64_t units = 0;
    for (int i = 0; i < run.n; ++i) units += run.rows[i] / so3::kUnitRows;
    unsigned long long *stamps = nullptr;
    void *args[3] = {&op, &units, &stamps};
    hipKernelNodeParams p;
    memset(&p, 0, sizeof p);
    p.func = reinterpret_cast<void *>(&so3::k_rows<Op, 2, SO3_WPS_K1, SO3_BLOCK_K1, false>);
    p.gridDim = dim3(rows_grid<2, SO3_WPS_K1, SO3_BLOCK_K1, Op>(op.total_rounds));
    p.blockDim = dim3(SO3_BLOCK_K1);
    p.sharedMemBytes = 0;
    p.kernelParams = args;
    p.extra = nullptr;
    const hipError_t e = hipGraphKernelNodeSetParams(node, &p);
    if (e == hipSuccess) g_last_kernel = rows_kernel_name<Op, 2, SO3_WPS_K1, SO3_BLOCK_K1>(s);
    return e;
}

// The capture state of `s`: true while it is being captured (then id and the stream's capture dependencies are set).
inline bool capture_state(hipStream_t s, unsigned long long *id, const hipGraphNode_t **deps, size_t *ndeps) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    hipGraph_t graph = nullptr;
    *id = 0; *deps = nullptr; *ndeps = 0;
    if (hipStreamGetCaptureInfo_v2(s, &status, id, &graph, deps, ndeps) != hipSuccess) {
        (void)hipGetLastError();              // (a query the runtime refuses is not this call's failure: launch as ever)
        return false;
    }
    return status == hipStreamCaptureStatusActive;
}

template <bool BF16>
int project_fwd(const void *M, float *R, uint8_t *flip, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_project_fwd: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(M != nullptr && R != nullptr, "so3_project_fwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr int EB = BF16 ? 2 : 4;
    const Split sp(B, {M, R});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    if (nunits > 0) {
        // two matrices per lane, three waves per SIMD: against one matrix per lane at four / five / six / eight waves (round 3, the fast
        // path, one device): 14.6-14.9 us against 15.6 / 14.9 / 16.6 (spills) / 18.4
        if (flip) {
            so3::OpProject<EB, true> op; op.template add_segment<2>(M, R, nunits); op.flip = flip;
            launch_rows<2, SO3_WPS_K1, SO3_BLOCK_K1>(op, nunits, s);
        } else if (nunits * so3::kUnitRows == B && g_capture_fusion.load(std::memory_order_relaxed) != 0) {
            // Engine only (no flags, no remainder).  Under capture the call may join the kernel node this thread's previous such call
            // created: adjacent independent launches then replay as ONE persistent launch over several segments, and the tail of one
            // overlaps the fill of the next inside the kernel instead of draining at a launch boundary.
            K1Captured &rec = g_k1_captured;
            unsigned long long id;
            const hipGraphNode_t *deps;
            size_t ndeps;
            const bool capturing = capture_state(s, &id, &deps, &ndeps);
            if (capturing && k1_may_fuse(rec, id, ndeps, ndeps > 0 ? deps[0] : nullptr, EB, M, R, B)) {
                K1Run wider = rec.run;
                wider.in[wider.n] = M; wider.out[wider.n] = R; wider.rows[wider.n] = B; ++wider.n;
                if (k1_rewrite_node<EB>(rec.node, wider, s) == hipSuccess) {
                    rec.run = wider;
                    ++g_k1_fused;
                    return 0;
                }
                (void)hipGetLastError();      // the runtime refused: a node of its own, below
            }
            K1Run run;
            run.in[0] = M; run.out[0] = R; run.rows[0] = B; run.n = 1; run.elem_bytes = EB;
            k1_launch<EB>(run, s);
            rec.node = nullptr;
            if (capturing && capture_state(s, &id, &deps, &ndeps) && ndeps == 1) {       // the node the launch has just created
                rec.capture_id = id;
                rec.node = deps[0];
                rec.run = run;
            }
        } else {
            so3::OpProject<EB, false> op; op.template add_segment<2>(M, R, nunits);
            launch_rows<2, SO3_WPS_K1, SO3_BLOCK_K1>(op, nunits, s);
        }
    }
    if (rest > 0) {
        const void *Mt = advance_bytes(M, done * 9 * EB);
        float *Rt = R + done * 9;
        uint8_t *ft = advance(flip, done);
        const bool vec = (BF16 || aligned16(Mt)) && aligned16(Rt);      // for bf16 input VEC only governs the R store
        const dim3 grid(grid_for(rest)), block(kBlock);
        with_flags([&](auto VE, auto FL) { hipLaunchKernelGGL((k_project_fwd<BF16, VE(), FL()>), grid, block, 0, s, Mt, Rt, ft, rest); }, vec,
                   flip != nullptr);
    }
    return check_launch("so3_project_fwd");
}

// ---- K2 --------------------------------------------------------------------------------------------
template <bool BF16>
int project_bwd(const void *M, const float *G, void *dM, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_project_bwd: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(M != nullptr && G != nullptr && dM != nullptr, "so3_project_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr int EB = BF16 ? 2 : 4;
    const Split sp(B, {M, G, dM});
    const int64_t done = sp.done, rest = sp.rest;
    if (sp.nunits > 0) {
        so3::OpProjectBwd<EB> op; op.in0 = M; op.in1 = G; op.out0 = dM;
        launch_rows<2, SO3_WPS_K2, 256>(op, sp.nunits, s);
    }
    if (rest > 0) {
        const void *Mt = advance_bytes(M, done * 9 * EB);
        const float *Gt = G + done * 9;
        void *dt = advance_bytes(dM, done * 9 * EB);
        const bool vec = aligned16(Gt) && (BF16 || (aligned16(Mt) && aligned16(dt)));
        const dim3 grid(grid_for(rest)), block(kBlock);
        with_flags([&](auto VE) { hipLaunchKernelGGL((k_project_bwd<BF16, VE()>), grid, block, 0, s, Mt, Gt, dt, rest); }, vec);
    }
    return check_launch("so3_project_bwd");
}

// ---- K3 --------------------------------------------------------------------------------------------
// How a reduction over a large batch is finished.  With a workspace (and whole units on the engine): the remainder kernel,
// if any, runs FIRST and fills slots [0, tile_wgs); the engine launch then takes tickets and its last workgroup writes the
// result.  Without: the accumulators are zeroed by a memset / init launch and every workgroup adds to them atomically.
inline so3::ReduceWs *reduce_workspace(void *workspace, const Split &sp, unsigned tile_wgs) {
    const bool use = workspace != nullptr && sp.nunits > 0 && tile_wgs <= 1024u;        // + at most 1024 engine workgroups <= kMaxPartials
    return use ? static_cast<so3::ReduceWs *>(workspace) : nullptr;
}

template <bool BF16>
int frob(const void *M, const float *Rtrue, float *R, void *dM, double *loss_sum, float *loss_mean, void *workspace, unsigned flags, int64_t B,
         void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_PREZEROED)) == 0, "so3_frob_fwd_bwd: unknown flag");
    const bool prezeroed = (flags & SO3_PREZEROED) != 0;
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_frob_fwd_bwd: B");
    SO3_CHECK_ARGS(loss_sum != nullptr || (loss_mean != nullptr && B > 0 && B <= kSmallBatch), "so3_frob_fwd_bwd: loss_sum is null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B > 0 && B <= kSmallBatch) {                    // one workgroup, one launch: the kernel writes loss_sum and / or the mean itself
        SO3_CHECK_ARGS(M != nullptr && Rtrue != nullptr, "so3_frob_fwd_bwd: null pointer");
        const dim3 grid(1), block(static_cast<unsigned>((B + 63) / 64 * 64));
        const float inv = 1.0f / static_cast<float>(B);
        with_flags([&](auto WR, auto WD) {
            hipLaunchKernelGGL((k_frob_small<BF16, WR(), WD()>), grid, block, 0, s, M, Rtrue, R, dM, loss_sum, loss_mean, static_cast<int>(B), inv, prezeroed);
        }, R != nullptr, dM != nullptr);
        return check_launch("so3_frob_fwd_bwd");
    }
    constexpr int EB = BF16 ? 2 : 4;
    const Split sp(B, {M, Rtrue, R, dM});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    const unsigned tile_wgs = rest > 0 ? persistent_grid(rest) : 0u;
    so3::ReduceWs *ws = reduce_workspace(workspace, sp, tile_wgs);
    if (ws == nullptr && !prezeroed) if (int e = zero_async(loss_sum, sizeof(double), s, "so3_frob_fwd_bwd: memset")) return e;
    if (B == 0) {
        if (loss_mean != nullptr) if (int e = zero_async(loss_mean, sizeof(float), s, "so3_frob_fwd_bwd: memset")) return e;
        return 0;
    }
    SO3_CHECK_ARGS(M != nullptr && Rtrue != nullptr, "so3_frob_fwd_bwd: null pointer");
    const float inv_b = 1.0f / static_cast<float>(B);
    if (rest > 0) {
        const void *Mt = advance_bytes(M, done * 9 * EB);
        const float *Tt = Rtrue + done * 9;
        float *Rt = advance(R, done * 9);
        void *dt = advance_bytes(dM, done * 9 * EB);
        bool vec = aligned16(Tt) && (Rt == nullptr || aligned16(Rt));
        if (!BF16) vec = vec && aligned16(Mt) && (dt == nullptr || aligned16(dt));
        const dim3 grid(tile_wgs), block(kBlock);
        with_flags([&](auto VE, auto WR, auto WD) {
            hipLaunchKernelGGL((k_frob_fwd_bwd<BF16, VE(), WR(), WD()>), grid, block, 0, s, Mt, Tt, Rt, dt, loss_sum, rest, inv_b, ws);
        }, vec, R != nullptr, dM != nullptr);
    }
    if (nunits > 0) {
        with_flags([&](auto WR, auto WD) {
            so3::OpFrobHead<EB, WD(), WR()> op; op.in0 = M; op.in1 = Rtrue; op.out0 = dM; op.out1 = R;
            op.loss_sum = loss_sum; op.inv_b = inv_b; op.loss_mean = loss_mean; op.inv_b_f64 = 1.0 / static_cast<double>(B);
            op.ws = ws; op.ws_slot0 = tile_wgs;
            launch_rows<2, SO3_WPS_K3, SO3_BLOCK_K3>(op, nunits, s);
        }, R != nullptr, dM != nullptr);
    }
    if (ws == nullptr && loss_mean != nullptr) k_mean_from_sum<<<1, 1, 0, s>>>(loss_sum, loss_mean, 1.0 / static_cast<double>(B));
    return check_launch("so3_frob_fwd_bwd");
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
namespace {
// The model points a lane of k_add_l1 / k_sym_add keeps in flight.
inline int add_points_unroll(int32_t N) { return N > 512 ? 16 : (N > 128 ? 8 : 2); }

template <bool DISENT, bool L2 = false>
int launch_add_l1(const float *Tgt, const float *Tpred, const float *points, float *dists, double *loss_sum, float *dTpred,
                  float grad_scale, int64_t B, int32_t N, hipStream_t s, const char *what) {
    if (loss_sum != nullptr) if (int e = zero_async(loss_sum, (DISENT ? 3 : 1) * sizeof(double), s, what)) return e;
    if (B == 0) return 0;
    const CloudShape shape = cloud_shape(B);
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    with_value<16, 8, 2>(add_points_unroll(N), [&](auto U) {
        hipLaunchKernelGGL((k_add_l1<DISENT, U(), L2>), grid, block, 0, s, Tgt, Tpred, points, dists, loss_sum, dTpred, grad_scale, B, N, shape.per_wave);
    });
    return check_launch(what);
}

// The search kernels' launch: at most 64 workgroups per compute unit, which stride over the work items.
inline unsigned search_grid(int64_t items) { return static_cast<unsigned>(std::min<int64_t>(items, static_cast<int64_t>(device_cus()) * 64)); }
// The work items of one cloud of N source points in k_add_s and k_icp_step, and the points per lane u they are cut for.
inline int32_t icp_chunks(int64_t B, int32_t N, int &u) {
    u = so3::icp_points_per_lane(B, N, device_cus());
    return so3::search_chunks(N, u);
}

// k_add_s over B clouds, then its rows.  The instantiation's name goes to so3_last_kernel; the rows' launches leave it there.
template <bool DIAMETER>
int launch_add_s(const float *Tgt, const float *Tpred, const float *points, float *point_dist, int32_t *nearest, float *rows, double *total,
                 int64_t B, int32_t N, hipStream_t s, const char *what) {
    int u;
    const int32_t chunks = icp_chunks(B, N, u);
    const dim3 grid(search_grid(B * chunks)), block(kBlock);
    with_flags([&](auto WI) {
        constexpr bool kIndex = WI() && !DIAMETER;             // a diameter has no nearest index: no such instantiation
        with_value<4, 2, 1>(u, [&](auto U) {
            name_kernel("k_add_s", kIndex, DIAMETER, U);
            hipLaunchKernelGGL((k_add_s<kIndex, DIAMETER, U()>), grid, block, 0, s, Tgt, Tpred, points, point_dist, nearest, B, N, chunks);
        });
    }, !DIAMETER && nearest != nullptr);
    if (rows != nullptr) {
        hipLaunchKernelGGL((k_add_s_rows<DIAMETER>), dim3(wave_rows_grid(B, 8)), block, 0, s, point_dist, rows, static_cast<double *>(nullptr), B, N);
        if (total != nullptr) hipLaunchKernelGGL(k_sum_f32_to_f64, dim3(1), block, 0, s, rows, total, B);
    } else if (total != nullptr) {            // no per-sample buffer to go through: one workgroup finishes rows and batch
        hipLaunchKernelGGL((k_add_s_rows<DIAMETER>), dim3(1), block, 0, s, point_dist, static_cast<float *>(nullptr), total, B, N);
    }
    return check_launch(what);
}

// k_sym_add over B clouds: a wave per sample at a time, at most eight workgroups per compute unit.  With `rows` the batch total is a
// second, one-workgroup launch over them; without, one workgroup does the whole call and sums as it goes (k_add_s_rows's rule).
// The instantiation's name goes to so3_last_kernel.
template <int MODE, bool GRAD>
void launch_sym_add(const float *Tgt, const float *Tpred, const float *points, const float *S, const int32_t *class_id, int32_t C, int32_t K,
                    float *rows, int32_t *index, double *total, float *dT, float grad_scale, int64_t B, int32_t N, hipStream_t s) {
    const bool one_group = rows == nullptr && total != nullptr;
    const dim3 grid(one_group ? 1u : wave_rows_grid(B, 8)), block(kBlock);
    double *in_kernel = one_group ? total : nullptr;
    with_value<16, 8, 2>(add_points_unroll(N), [&](auto U) {
        name_kernel("k_sym_add", MODE, GRAD, U);
        hipLaunchKernelGGL((k_sym_add<MODE, GRAD, U()>), grid, block, 0, s, Tgt, Tpred, points, S, class_id, C, K, rows, index, in_kernel, dT,
                           grad_scale, B, N);
    });
    if (rows != nullptr && total != nullptr) hipLaunchKernelGGL(k_sum_f32_to_f64, dim3(1), block, 0, s, rows, total, B);
}

// k_icp_step over B clouds at k_add_s's launch shape.  The instantiation's name goes to so3_last_kernel.
template <bool SUMS>
void launch_icp_step(const float *P, const float *Q, int64_t q_stride, const float *w, const float *pose, float max_distance, float *rec,
                     float *dist, int32_t *nearest, int64_t B, int32_t N, int32_t M, int u, int32_t chunks, hipStream_t s) {
    const dim3 grid(search_grid(B * chunks)), block(kBlock);
    with_flags([&](auto WW, auto TT) {
        constexpr bool kWeighted = WW() && SUMS, kTrimmed = TT() && SUMS;       // the search alone has neither: no such instantiation
        with_value<4, 2, 1>(u, [&](auto U) {
            name_kernel("k_icp_step", kWeighted, kTrimmed, SUMS, U);
            hipLaunchKernelGGL((k_icp_step<kWeighted, kTrimmed, SUMS, U()>), grid, block, 0, s, P, Q, q_stride, w, pose, max_distance, rec, dist,
                               nearest, B, N, M, chunks);
        });
    }, SUMS && w != nullptr, SUMS && max_distance >= 0.f);
}

// The work items of one cloud in the Chamfer kernels: kBlock * u points per item, x items first, then the y items (none: x direction only).
struct ChamferChunks { int32_t x, y; };
inline ChamferChunks chamfer_chunks(int32_t N, int32_t M, bool single, int u) {
    return {so3::search_chunks(N, u), single ? 0 : so3::search_chunks(M, u)};
}
inline unsigned chamfer_grid(int64_t B, ChamferChunks ch) { return search_grid(B * (ch.x + ch.y)); }
inline int chamfer_invalid(const char *name, const char *what) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, what);
    return fail(SO3_ERR_INVALID, msg);
}
#define SO3_CHAMFER_CHECK(cond, what) \
    do { if (!(cond)) return chamfer_invalid(name, what); } while (0)

// so3_chamfer_fwd_f32 and so3_chamfer_normals_fwd_f32 (NORMALS: the normals, term_x / term_y, rows_n and the signed-cosine flag come
// with it): the checks, the search over the work items of both directions, the rows.  Both take u from the same rule, so the
// distance's partial sums are the same.
template <bool NORMALS>
int launch_chamfer_fwd(const char *name, const float *X, const float *Y, const float *NX, const float *NY, const int32_t *x_len, const int32_t *y_len,
                       float *dist_x, int32_t *nearest_x, float *dist_y, int32_t *nearest_y, float *term_x, float *term_y, float *rows,
                       float *rows_n, void *work, uint32_t flags, int64_t B, int32_t N, int32_t M, void *stream) {
    const unsigned known = SO3_CHAMFER_UNSQUARED | SO3_CHAMFER_SINGLE | (NORMALS ? SO3_CHAMFER_SIGNED_COSINE : 0);
    SO3_CHAMFER_CHECK((flags & ~known) == 0, "unknown flag");
    SO3_CHAMFER_CHECK(cloud_dims_ok(B, N, M), "B/N/M");
    if (B == 0) return 0;
    const bool single = (flags & SO3_CHAMFER_SINGLE) != 0;
    SO3_CHAMFER_CHECK(X != nullptr && Y != nullptr && rows != nullptr && work != nullptr &&
                          (!NORMALS || (NX != nullptr && NY != nullptr && rows_n != nullptr)), "null pointer");
    SO3_CHAMFER_CHECK(!single || (dist_y == nullptr && nearest_y == nullptr && term_y == nullptr),
                      NORMALS ? "dist_y / nearest_y / term_y with SO3_CHAMFER_SINGLE" : "dist_y / nearest_y with SO3_CHAMFER_SINGLE");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int u = so3::chamfer_points_per_lane(B, N, M, single, device_cus());
    const ChamferChunks ch = chamfer_chunks(N, M, single, u);
    float *rec = static_cast<float *>(work);
    const dim3 grid(chamfer_grid(B, ch)), block(kBlock);
    const dim3 rows_grid(static_cast<unsigned>(std::min<int64_t>((2 * B + kBlock - 1) / kBlock, static_cast<int64_t>(device_cus()) * 64)));
    const int32_t signed_cos = (flags & SO3_CHAMFER_SIGNED_COSINE) != 0 ? 1 : 0;
    with_flags([&](auto SQ) {
        constexpr bool kSquared = SQ();
        with_value<4, 2, 1>(u, [&](auto U) {
            if constexpr (NORMALS) {
                name_kernel("k_chamfer_normals_fwd", kSquared, U);
                hipLaunchKernelGGL((k_chamfer_normals_fwd<kSquared, U()>), grid, block, 0, s, X, Y, NX, NY, x_len, y_len, dist_x, nearest_x, dist_y,
                                   nearest_y, term_x, term_y, rec, signed_cos, B, N, M, ch.x, ch.y);
            } else {
                name_kernel("k_chamfer_fwd", kSquared, U);
                hipLaunchKernelGGL((k_chamfer_fwd<kSquared, U()>), grid, block, 0, s, X, Y, x_len, y_len, dist_x, nearest_x, dist_y, nearest_y, rec, B,
                                   N, M, ch.x, ch.y);
            }
        });
    }, (flags & SO3_CHAMFER_UNSQUARED) == 0);
    if (NORMALS) hipLaunchKernelGGL(k_chamfer_normals_rows, rows_grid, block, 0, s, rec, x_len, y_len, rows, rows_n, B, N, M, ch.x, ch.y);
    else hipLaunchKernelGGL(k_chamfer_rows, rows_grid, block, 0, s, rec, x_len, y_len, rows, B, N, M, ch.x, ch.y);
    return check_launch(name);
}

// What both Chamfer backwards ask of their arguments (A, Bq: the two clouds' points or normals).  0: go on; B == 0 is the caller's.
inline int check_chamfer_bwd(const char *name, unsigned known, const void *A, const void *Bq, const int32_t *nearest_x, const int32_t *nearest_y,
                             const float *scale_x, const float *scale_y, const void *dA, const void *dB, uint32_t flags, int64_t B, int32_t N,
                             int32_t M) {
    SO3_CHAMFER_CHECK((flags & ~known) == 0, "unknown flag");
    SO3_CHAMFER_CHECK(cloud_dims_ok(B, N, M), "B/N/M");
    if (B == 0) return 0;
    const bool single = (flags & SO3_CHAMFER_SINGLE) != 0;
    SO3_CHAMFER_CHECK(A != nullptr && Bq != nullptr && nearest_x != nullptr && scale_x != nullptr && (dA != nullptr || dB != nullptr), "null pointer");
    SO3_CHAMFER_CHECK(single ? (nearest_y == nullptr && scale_y == nullptr) : (nearest_y != nullptr && scale_y != nullptr),
                      "nearest_y and scale_y go with both directions, NULL with SO3_CHAMFER_SINGLE");
    return 0;
}
#undef SO3_CHAMFER_CHECK
}  // namespace

// ---- K4b: the metrics' backward (include/so3proj.h) ------------------------------------------------------------------
namespace {
template <int GRAD, bool F64MATH, bool BOTH>
void angle_bwd_launch(const float *R1, const float *R2, const void *grad, double div, double unit, double lo, double hi, float *d1, float *d2,
                      int64_t B, hipStream_t s) {
    so3::OpAngleBwd<GRAD, F64MATH, BOTH> op;
    op.in0 = R1; op.in1 = R2; op.out0 = d1; op.out1 = d2;
    op.lo = lo; op.hi = hi; op.unit = unit; op.div = div;
    if (GRAD == 0) op.gscalar = grad; else op.in2 = grad;
    const Split sp(B, {R1, R2, GRAD != 0 ? grad : nullptr, d1, d2});
    const int64_t done = sp.done, rest = sp.rest;
    // light arithmetic, 108-152 B per row: two rows per lane, three waves per SIMD (11 KB of LDS per wave)
    if (sp.nunits > 0) launch_rows<SO3_K4B_NPL, SO3_K4B_WPS, SO3_K4B_BLOCK>(op, sp.nunits, s);
    if (rest > 0) {
        so3::OpAngleBwd<GRAD, F64MATH, BOTH> t = op;
        t.in0 = R1 + done * 9; t.in1 = R2 + done * 9;
        const void *g = GRAD != 0 ? advance_bytes(grad, done * (F64MATH ? 8 : 4)) : nullptr;
        hipLaunchKernelGGL((k_angle_bwd_rows<so3::OpAngleBwd<GRAD, F64MATH, BOTH>>), dim3(grid_for(rest)), dim3(kBlock), 0, s, t, g, d1 + done * 9,
                           advance(d2, done * 9), rest);
    }
}
}  // namespace

extern "C" {

int so3_version(void) { return SO3PROJ_VERSION; }
const char *so3_last_error(void) { return g_err; }
const char *so3_last_kernel(void) { return g_last_kernel; }

int so3_project_fwd_f32(const float *M, float *R, uint8_t *flip, int64_t B, void *stream) {
    return project_fwd<false>(M, R, flip, B, stream);
}
int so3_project_fwd_bf16(const void *M, float *R, uint8_t *flip, int64_t B, void *stream) {
    return project_fwd<true>(M, R, flip, B, stream);
}
int so3_project_fwd_segments_f32(const float *const *M, float *const *R, const int64_t *B, int n, void *stream) {
    SO3_CHECK_ARGS(n >= 1 && n <= so3::kMaxSegments, "so3_project_fwd_segments_f32: n");
    SO3_CHECK_ARGS(M != nullptr && R != nullptr && B != nullptr, "so3_project_fwd_segments_f32: null pointer");
    K1Run run;
    for (int i = 0; i < n; ++i) {
        SO3_CHECK_ARGS(B[i] > 0 && B[i] % so3::kUnitRows == 0, "so3_project_fwd_segments_f32: B[i] must be a positive multiple of 64");
        SO3_CHECK_ARGS(M[i] != nullptr && R[i] != nullptr, "so3_project_fwd_segments_f32: null pointer");
        SO3_CHECK_ARGS(aligned4(M[i]) && aligned4(R[i]), "so3_project_fwd_segments_f32: pointers must be dword aligned");
        run.in[i] = M[i]; run.out[i] = R[i]; run.rows[i] = B[i];
        run.n = i + 1;
        SO3_CHECK_ARGS(k1_rounds(run) <= kMaxRounds32, "so3_project_fwd_segments_f32: too many rows in all");
    }
    k1_launch<4>(run, static_cast<hipStream_t>(stream));
    g_k1_captured.node = nullptr;
    return check_launch("so3_project_fwd_segments_f32");
}
int so3_capture_fusion(int enable) { return g_capture_fusion.exchange(enable != 0 ? 1 : 0); }
int64_t so3_capture_fused_launches(void) { return g_k1_fused; }
int so3_capture_fusion_would_fuse(const void *const *rec_M, void *const *rec_R, const int64_t *rec_B, int rec_n, int rec_elem_bytes,
                                  int same_capture, int ndeps, int dep_is_recorded_node, int elem_bytes, const void *M, const void *R,
                                  int64_t B) {
    SO3_CHECK_ARGS(rec_n >= 0 && rec_n <= so3::kMaxSegments && (rec_n == 0 || (rec_M != nullptr && rec_R != nullptr && rec_B != nullptr)),
                   "so3_capture_fusion_would_fuse: record");
    int marks[2];                              // two distinct addresses stand for the recorded node and for any other (never dereferenced)
    K1Captured rec;
    rec.capture_id = 1;
    rec.node = rec_n > 0 ? reinterpret_cast<hipGraphNode_t>(&marks[0]) : nullptr;
    rec.run.n = rec_n;
    rec.run.elem_bytes = rec_elem_bytes;
    for (int i = 0; i < rec_n; ++i) { rec.run.in[i] = rec_M[i]; rec.run.out[i] = static_cast<float *>(rec_R[i]); rec.run.rows[i] = rec_B[i]; }
    return k1_may_fuse(rec, same_capture != 0 ? 1 : 2, static_cast<size_t>(ndeps < 0 ? 0 : ndeps),
                       reinterpret_cast<hipGraphNode_t>(&marks[dep_is_recorded_node != 0 ? 0 : 1]), elem_bytes, M, R, B) ? 1 : 0;
}
int so3_project_bwd_f32(const float *M, const float *G, float *dM, int64_t B, void *stream) {
    return project_bwd<false>(M, G, dM, B, stream);
}
int so3_project_bwd_bf16(const void *M, const float *G, void *dM, int64_t B, void *stream) {
    return project_bwd<true>(M, G, dM, B, stream);
}
size_t so3_reduce_workspace_bytes(void) { return sizeof(so3::ReduceWs); }
int so3_frob_fwd_bwd_v2_f32(const float *M, const float *Rtrue, float *R, float *dM, double *loss_sum, float *loss_mean, void *workspace,
                            unsigned flags, int64_t B, void *stream) {
    return frob<false>(M, Rtrue, R, dM, loss_sum, loss_mean, workspace, flags, B, stream);
}
int so3_frob_fwd_bwd_v2_bf16(const void *M, const float *Rtrue, float *R, void *dM, double *loss_sum, float *loss_mean, void *workspace,
                             unsigned flags, int64_t B, void *stream) {
    return frob<true>(M, Rtrue, R, dM, loss_sum, loss_mean, workspace, flags, B, stream);
}

int so3_frob_loss_v2_f32(const float *Rpred, const float *Rtrue, float *dRpred, double *loss_sum, float *loss_mean, void *workspace,
                         unsigned flags, int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_PREZEROED)) == 0, "so3_frob_loss_f32: unknown flag");
    const bool prezeroed = (flags & SO3_PREZEROED) != 0;
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_frob_loss_f32: B");
    SO3_CHECK_ARGS(loss_sum != nullptr, "so3_frob_loss_f32: loss_sum is null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B > 0 && B <= kSmallBatch) {                     // one workgroup, one launch: the kernel writes loss_sum (and the mean) itself
        SO3_CHECK_ARGS(Rpred != nullptr && Rtrue != nullptr, "so3_frob_loss_f32: null pointer");
        const dim3 grid(1), block(static_cast<unsigned>((B + 63) / 64 * 64));
        const float inv = 1.0f / static_cast<float>(B);
        with_flags([&](auto WG) {
            hipLaunchKernelGGL((k_frob_loss_small<WG()>), grid, block, 0, s, Rpred, Rtrue, dRpred, loss_sum, loss_mean, static_cast<int>(B), inv, prezeroed);
        }, dRpred != nullptr);
        return check_launch("so3_frob_loss_f32");
    }
    const Split sp(B, {Rpred, Rtrue, dRpred});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    const unsigned tile_wgs = rest > 0 ? persistent_grid(rest) : 0u;
    so3::ReduceWs *ws = reduce_workspace(workspace, sp, tile_wgs);
    if (ws == nullptr && !prezeroed) if (int e = zero_async(loss_sum, sizeof(double), s, "so3_frob_loss_f32: memset")) return e;
    if (B == 0) {
        if (loss_mean != nullptr) if (int e = zero_async(loss_mean, sizeof(float), s, "so3_frob_loss_f32: memset")) return e;
        return 0;
    }
    SO3_CHECK_ARGS(Rpred != nullptr && Rtrue != nullptr, "so3_frob_loss_f32: null pointer");
    const float inv_b = 1.0f / static_cast<float>(B);
    if (rest > 0) {
        const float *Pt = Rpred + done * 9, *Tt = Rtrue + done * 9;
        float *gt = advance(dRpred, done * 9);
        const bool vec = aligned16(Pt) && aligned16(Tt) && (gt == nullptr || aligned16(gt));
        const dim3 grid(tile_wgs), block(kBlock);
        with_flags([&](auto VE, auto WG) {
            hipLaunchKernelGGL((k_frob_loss<VE(), WG()>), grid, block, 0, s, Pt, Tt, gt, loss_sum, rest, inv_b, ws);
        }, vec, dRpred != nullptr);
    }
    if (nunits > 0) {
        with_flags([&](auto WG) {
            so3::OpFrobLoss<WG()> op; op.in0 = Rpred; op.in1 = Rtrue; op.out0 = dRpred; op.loss_sum = loss_sum; op.inv_b = inv_b;
            op.loss_mean = loss_mean; op.inv_b_f64 = 1.0 / static_cast<double>(B); op.ws = ws; op.ws_slot0 = tile_wgs;
            launch_rows<1, 4, 1024>(op, nunits, s);
        }, dRpred != nullptr);
    }
    if (ws == nullptr && loss_mean != nullptr) k_mean_from_sum<<<1, 1, 0, s>>>(loss_sum, loss_mean, 1.0 / static_cast<double>(B));
    return check_launch("so3_frob_loss_f32");
}
// `prezeroed`: sum_count[0] and *range_flag are zero on entry (the caller hands out fresh slots of a zero-filled pool): no
// init launch, the kernels add to them as they are and one workgroup stores the row count.
int so3_angle_error_v2(const float *R1, const float *R2, double *deg, double *sum_count, int32_t *range_flag, void *workspace, unsigned flags,
                       int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_RADIANS | SO3_PREZEROED | SO3_EXACT_F64)) == 0, "so3_angle_error: unknown flag");
    const bool radians = (flags & SO3_RADIANS) != 0, prezeroed = (flags & SO3_PREZEROED) != 0;      // (K4 alone is float64 on every row: SO3_EXACT_F64 changes nothing)
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_angle_error: B");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double unit = radians ? 1.0 : kDegPerRad;
    if (B > 0 && B <= kSmallBatch && (sum_count || range_flag)) {       // one workgroup: the accumulators need no launch of their own
        SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr, "so3_angle_error: null pointer");
        const dim3 grid(1), block(static_cast<unsigned>((B + 63) / 64 * 64));
        with_flags([&](auto WD) {
            hipLaunchKernelGGL((k_angle_small<false, false, WD()>), grid, block, 0, s, R1, R2, nullptr, deg, sum_count, range_flag, unit, static_cast<int>(B), prezeroed);
        }, deg != nullptr);
        return check_launch("so3_angle_error");
    }
    const Split sp(B, {R1, R2, deg});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    const unsigned tile_wgs = rest > 0 ? grid_for(rest) : 0u;
    so3::ReduceWs *ws = (sum_count || range_flag) ? reduce_workspace(workspace, sp, tile_wgs) : nullptr;
    // without a workspace one tiny launch zeroes the accumulators and writes the row count (instead of two memsets + a store)
    if (ws == nullptr && (sum_count || range_flag) && !(prezeroed && B > 0)) k_angle_init<<<1, 1, 0, s>>>(sum_count, range_flag, static_cast<double>(B));
    if (B == 0) return check_launch("so3_angle_error");
    const bool store_count = prezeroed && ws == nullptr;
    if (store_count && sum_count != nullptr && nunits == 0) k_angle_init<<<1, 1, 0, s>>>(sum_count, nullptr, static_cast<double>(B));   // no engine launch to store the count
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr, "so3_angle_error: null pointer");
    if (rest > 0) {                                            // remainder (< 64 rows) or unaligned input
        const float *A1 = R1 + done * 9, *A2 = R2 + done * 9;
        double *dg = advance(deg, done);
        const bool vec = aligned16(A1) && aligned16(A2);
        const dim3 grid(tile_wgs), block(kBlock);
        with_flags([&](auto VE, auto WD, auto WS) {
            hipLaunchKernelGGL((k_angle_error<VE(), WD(), WS()>), grid, block, 0, s, A1, A2, dg, sum_count, range_flag, unit, rest, ws);
        }, vec, deg != nullptr, sum_count != nullptr);
    }
    if (nunits > 0) {
        // 1024-thread workgroups: 256 partials (or, without a workspace, 256 same-address float64 atomics at ~9 ns) at the end
        with_flags([&](auto WD, auto WS) {
            so3::OpAngle<WD(), WS()> op; op.in0 = R1; op.in1 = R2; op.deg = deg; op.sum_count = sum_count;
            op.range_flag = range_flag; op.unit_scale = unit; op.count = static_cast<double>(B); op.ws = ws; op.ws_slot0 = tile_wgs;
            op.store_count = store_count;
            launch_rows<1, 4, 1024>(op, nunits, s);
        }, deg != nullptr, sum_count != nullptr);
    }
    return check_launch("so3_angle_error");
}
int so3_project_angle_error_v2_f32(const float *M, const float *Rtrue, float *R, double *deg, double *sum_count, int32_t *range_flag,
                                   void *workspace, unsigned flags, int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_RADIANS | SO3_PREZEROED | SO3_EXACT_F64)) == 0, "so3_project_angle_error_f32: unknown flag");
    const bool radians = (flags & SO3_RADIANS) != 0, prezeroed = (flags & SO3_PREZEROED) != 0, exact = (flags & SO3_EXACT_F64) != 0;
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_project_angle_error_f32: B");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double unit = radians ? 1.0 : kDegPerRad;
    if (B > 0 && B <= kSmallBatch && (sum_count || range_flag)) {       // one workgroup, one launch
        SO3_CHECK_ARGS(M != nullptr && Rtrue != nullptr, "so3_project_angle_error_f32: null pointer");
        const dim3 grid(1), block(static_cast<unsigned>((B + 63) / 64 * 64));
        with_flags([&](auto WR, auto WD) {
            hipLaunchKernelGGL((k_angle_small<true, WR(), WD()>), grid, block, 0, s, M, Rtrue, R, deg, sum_count, range_flag, unit, static_cast<int>(B), prezeroed);
        }, R != nullptr, deg != nullptr);
        return check_launch("so3_project_angle_error_f32");
    }
    const Split sp(B, {M, Rtrue, R, deg});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    const unsigned tile_wgs = rest > 0 ? grid_for(rest) : 0u;
    so3::ReduceWs *ws = (sum_count || range_flag) ? reduce_workspace(workspace, sp, tile_wgs) : nullptr;
    if (ws == nullptr && (sum_count || range_flag) && !(prezeroed && B > 0)) k_angle_init<<<1, 1, 0, s>>>(sum_count, range_flag, static_cast<double>(B));
    if (B == 0) return check_launch("so3_project_angle_error_f32");
    const bool store_count = prezeroed && ws == nullptr;
    if (store_count && sum_count != nullptr && nunits == 0) k_angle_init<<<1, 1, 0, s>>>(sum_count, nullptr, static_cast<double>(B));
    SO3_CHECK_ARGS(M != nullptr && Rtrue != nullptr, "so3_project_angle_error_f32: null pointer");
    if (rest > 0) {
        // remainder / unaligned input: the two-kernel spelling (K1 -> R -> K4) on the tail, which needs the caller's R buffer
        SO3_CHECK_ARGS(R != nullptr, "so3_project_angle_error_f32: a < 64-row remainder or unaligned input needs the R buffer");
        const float *Mt = M + done * 9, *Tt = Rtrue + done * 9;
        float *Rt = R + done * 9;
        double *dg = advance(deg, done);
        const dim3 grid(tile_wgs), block(kBlock);
        with_flags([&](auto VE) {
            hipLaunchKernelGGL((k_project_fwd<false, VE(), false>), grid, block, 0, s, static_cast<const void *>(Mt), Rt, nullptr, rest);
        }, aligned16(Mt) && aligned16(Rt));
        with_flags([&](auto WD, auto WS) {
            hipLaunchKernelGGL((k_angle_error<false, WD(), WS()>), grid, block, 0, s, Rt, Tt, dg, sum_count, range_flag, unit, rest, ws);
        }, deg != nullptr, sum_count != nullptr);
    }
    if (nunits > 0) {
        // the sum without per-row angles: float32 trace and acos outside the band around +-1 (so3::angle_sum_f32) unless SO3_EXACT_F64
        const bool f32 = sum_count != nullptr && deg == nullptr && !exact;
        with_flags([&](auto WR, auto WD, auto WS, auto F32) {
            if constexpr (!F32() || (!WD() && WS())) {        // (F32 exists for the sum alone)
                so3::OpProjectAngle<4, WR(), WD(), WS(), F32()> op; op.in0 = M; op.in1 = Rtrue; op.out0 = R; op.deg = deg;
                op.sum_count = sum_count; op.range_flag = range_flag; op.unit_scale = unit; op.count = static_cast<double>(B);
                op.ws = ws; op.ws_slot0 = tile_wgs; op.store_count = store_count;
                launch_rows<2, SO3_WPS_K14, SO3_BLOCK_K14>(op, nunits, s);
            }
        }, R != nullptr, deg != nullptr, sum_count != nullptr, f32);
    }
    return check_launch("so3_project_angle_error_f32");
}
int so3_project_fwd_diag_f32(const float *M, float *R, uint8_t *hard, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_project_fwd_diag_f32: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(M != nullptr && R != nullptr && hard != nullptr, "so3_project_fwd_diag_f32: null pointer");
    hipLaunchKernelGGL(k_project_diag, dim3(grid_for(B)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), M, R, hard, B);
    return check_launch("so3_project_fwd_diag_f32");
}

int so3_scale_f32(const float *src, const float *factor, float *dst, int64_t n, void *stream) {
    SO3_CHECK_ARGS(n >= 0, "so3_scale_f32: n");
    if (n == 0) return 0;
    SO3_CHECK_ARGS(src != nullptr && factor != nullptr && dst != nullptr, "so3_scale_f32: null pointer");
    hipLaunchKernelGGL((k_scale<false>), dim3(static_cast<unsigned>((n + 4 * kBlock - 1) / (4 * kBlock))), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const void *>(src), factor, static_cast<void *>(dst), n);
    return check_launch("so3_scale_f32");
}
int so3_scale_bf16(const void *src, const float *factor, void *dst, int64_t n, void *stream) {
    SO3_CHECK_ARGS(n >= 0, "so3_scale_bf16: n");
    if (n == 0) return 0;
    SO3_CHECK_ARGS(src != nullptr && factor != nullptr && dst != nullptr, "so3_scale_bf16: null pointer");
    hipLaunchKernelGGL((k_scale<true>), dim3(static_cast<unsigned>((n + 8 * kBlock - 1) / (8 * kBlock))), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       src, factor, dst, n);
    return check_launch("so3_scale_bf16");
}

// one launch for B <= 1024 (one workgroup) and with a workspace; else init / memset launch + kernel (+ the mean's)
static int reduce_how(void *workspace, int64_t B, unsigned *grid) {
    // two workgroups' worth per CU, grid-stride: the ticket at the end is one same-address atomic per workgroup (~12 ns each,
    // serialised at the memory side -- 2048 of them were 7 us on top of a 37-us kernel)
    *grid = B <= kSmallBatch ? 1u : capped_grid(B, 2u * static_cast<unsigned>(device_cus()));
    return B <= kSmallBatch ? 1 : (workspace != nullptr ? 2 : 0);
}

int so3_angle_error_v2_f64(const double *R1, const double *R2, double *deg, double *sum_count, int32_t *range_flag, void *workspace,
                           unsigned flags, int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_RADIANS)) == 0, "so3_angle_error_v2_f64: unknown flag (SO3_RADIANS only)");
    const bool radians = (flags & SO3_RADIANS) != 0;
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_angle_error_v2_f64: B");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned grid = 1;
    const int how = B > 0 ? reduce_how(workspace, B, &grid) : 0;
    if (how == 0 && (sum_count || range_flag)) k_angle_init<<<1, 1, 0, s>>>(sum_count, range_flag, static_cast<double>(B));
    if (B == 0) return check_launch("so3_angle_error_v2_f64");
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr, "so3_angle_error_v2_f64: null pointer");
    const double unit = radians ? 1.0 : kDegPerRad;
    const dim3 block(kBlock);
    so3::ReduceWs *ws = static_cast<so3::ReduceWs *>(workspace);
    with_flags([&](auto WD, auto WS) {
        hipLaunchKernelGGL((k_angle_f64<0, WD(), WS()>), dim3(grid), block, 0, s, R1, R2, deg, sum_count, range_flag, unit, B, ws, how);
    }, deg != nullptr, sum_count != nullptr);
    return check_launch("so3_angle_error_v2_f64");
}

int so3_geodesic_f64(const double *R1, const double *R2, double *theta, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_geodesic_f64: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && theta != nullptr, "so3_geodesic_f64: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((k_angle_f64<1, true, false>), dim3(capped_grid(B, 2048u)), dim3(kBlock), 0, s, R1, R2, theta, nullptr, nullptr, 1.0, B, nullptr, 0);
    return check_launch("so3_geodesic_f64");
}

int so3_frob_loss_v2_f64(const double *Rpred, const double *Rtrue, double *dRpred, double *loss_sum, double *loss_mean, void *workspace,
                         unsigned flags, int64_t B, void *stream) {
    SO3_CHECK_ARGS(flags == 0, "so3_frob_loss_v2_f64: unknown flag (none is defined for it)");
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_frob_loss_v2_f64: B");
    SO3_CHECK_ARGS(loss_sum != nullptr, "so3_frob_loss_v2_f64: loss_sum is null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned grid = 1;
    const int how = B > 0 ? reduce_how(workspace, B, &grid) : 0;
    if (how == 0) {
        if (int e = zero_async(loss_sum, sizeof(double), s, "so3_frob_loss_v2_f64: memset")) return e;
        if (B == 0) {
            if (loss_mean != nullptr) if (int e = zero_async(loss_mean, sizeof(double), s, "so3_frob_loss_v2_f64: memset")) return e;
            return 0;
        }
    }
    SO3_CHECK_ARGS(Rpred != nullptr && Rtrue != nullptr, "so3_frob_loss_v2_f64: null pointer");
    const double inv_b = 1.0 / static_cast<double>(B);
    const dim3 block(kBlock);
    so3::ReduceWs *ws = static_cast<so3::ReduceWs *>(workspace);
    with_flags([&](auto WG) {
        hipLaunchKernelGGL((k_frob_loss_f64<WG()>), dim3(grid), block, 0, s, Rpred, Rtrue, dRpred, loss_sum, loss_mean, B, inv_b, ws, how);
    }, dRpred != nullptr);
    if (how == 0 && loss_mean != nullptr) k_mean_from_sum_f64<<<1, 1, 0, s>>>(loss_sum, loss_mean, inv_b);
    return check_launch("so3_frob_loss_v2_f64");
}

static int geodesic_f32(const float *R1, const float *R2, float *theta, double *sum, float *result, int mean, float eps, void *workspace, int64_t B,
                        void *stream, const char *what) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B && eps >= 0.f && eps < 1.f, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Split sp(B, {R1, R2, theta});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    const unsigned tile_wgs = rest > 0 ? grid_for(rest) : 0u;
    // with a workspace: ONE launch (two with a remainder) -- the last workgroup writes the sum and the reduced result
    so3::ReduceWs *ws = sum != nullptr ? reduce_workspace(workspace, sp, tile_wgs) : nullptr;
    if (sum != nullptr && ws == nullptr) if (int e = zero_async(sum, sizeof(double), s, what)) return e;
    const double scale = mean ? 1.0 / static_cast<double>(B) : 1.0;
    if (B > 0) {
        SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && (theta != nullptr || sum != nullptr), what);
        const float lo = -1.f + eps, hi = 1.f - eps;          // float32 arithmetic, like torch.clamp's scalars on a float32 tensor
        if (rest > 0) {                                       // (first: its partials are in the workspace when the engine's last workgroup sums)
            const float *A1 = R1 + done * 9, *A2 = R2 + done * 9;
            const dim3 grid(tile_wgs), block(kBlock);
            with_flags([&](auto VE) {
                hipLaunchKernelGGL((k_geodesic_f32<VE()>), grid, block, 0, s, A1, A2, advance(theta, done), sum, lo, hi, rest, ws);
            }, aligned16(A1) && aligned16(A2));
        }
        if (nunits > 0) {
            if (sum) {
                so3::OpGeodesic<true> op; op.in0 = R1; op.in1 = R2; op.theta = theta; op.sum = sum; op.lo = lo; op.hi = hi;
                op.ws = ws; op.ws_slot0 = tile_wgs; op.result = result; op.scale = scale;
                // 1024-thread workgroups as K4: 256 partials / same-address atomics at the end, not 768 (at ~12 ns each the
                // <2, 3, 256> shape spent 5 us of its 18.5 queueing on one address: docs/history/profiles/r04_all_kernels_stats.csv)
                launch_rows<1, 4, 1024>(op, nunits, s);
            } else { so3::OpGeodesic<false> op; op.in0 = R1; op.in1 = R2; op.theta = theta; op.lo = lo; op.hi = hi; launch_rows<2, 3, 256>(op, nunits, s); }
        }
    }
    // (torch's mean of an empty tensor is NaN, its sum 0: 0 * inf / 0 * 1)
    if (result != nullptr && ws == nullptr) k_mean_from_sum<<<1, 1, 0, s>>>(sum, result, scale);
    return check_launch(what);
}
int so3_geodesic_f32(const float *R1, const float *R2, float *theta, int64_t B, void *stream) {
    if (B == 0) return 0;
    SO3_CHECK_ARGS(theta != nullptr, "so3_geodesic_f32: null pointer");
    return geodesic_f32(R1, R2, theta, nullptr, nullptr, 0, 0.f, nullptr, B, stream, "so3_geodesic_f32");
}
int so3_geodesic_eps_f32(const float *R1, const float *R2, float *theta, double *sum, float *result, int mean, float eps, void *workspace, int64_t B,
                         void *stream) {
    SO3_CHECK_ARGS(result == nullptr || sum != nullptr, "so3_geodesic_eps_f32: result needs the float64 scratch `sum`");
    return geodesic_f32(R1, R2, theta, sum, result, mean, eps, workspace, B, stream, "so3_geodesic_eps_f32");
}

int so3_angle_bwd_f32(const float *R1, const float *R2, const void *grad, double grad_div, double eps, unsigned flags, float *dR1, float *dR2,
                      int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_RADIANS | SO3_GRAD_SCALAR | SO3_F64_MATH)) == 0, "so3_angle_bwd_f32: unknown flag");
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_angle_bwd_f32: B");
    SO3_CHECK_ARGS(eps >= 0.0 && eps < 1.0 && grad_div != 0.0, "so3_angle_bwd_f32: eps / grad_div");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && grad != nullptr && (dR1 != nullptr || dR2 != nullptr), "so3_angle_bwd_f32: null pointer");
    const bool f64 = (flags & SO3_F64_MATH) != 0, scalar = (flags & SO3_GRAD_SCALAR) != 0;
    SO3_CHECK_ARGS((reinterpret_cast<uintptr_t>(grad) & (f64 ? 7u : 3u)) == 0, "so3_angle_bwd_f32: grad is not aligned to its element");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double unit = (flags & SO3_RADIANS) != 0 ? 1.0 : kDegPerRad;
    // the clamp's bounds in the arithmetic of the spelling (torch.clamp's scalars on a float32 tensor are float32)
    const double lo = f64 ? -1.0 + eps : static_cast<double>(-1.f + static_cast<float>(eps));
    const double hi = f64 ? 1.0 - eps : static_cast<double>(1.f - static_cast<float>(eps));
    // one gradient alone: tr(R1 R2^T) is symmetric in its arguments, so dR2 is dR1 of the swapped pair
    const bool both = dR1 != nullptr && dR2 != nullptr;
    const float *A = dR1 != nullptr ? R1 : R2, *Bm = dR1 != nullptr ? R2 : R1;
    float *d1 = dR1 != nullptr ? dR1 : dR2, *d2 = both ? dR2 : nullptr;
    with_flags([&](auto F6, auto SC, auto BO) {
        constexpr int kGrad = SC() ? 0 : (F6() ? 2 : 1);          // the upstream gradient: one scalar, or per row in float32 / float64
        angle_bwd_launch<kGrad, F6(), BO()>(A, Bm, grad, grad_div, unit, lo, hi, d1, d2, B, s);
    }, f64, scalar, both);
    return check_launch("so3_angle_bwd_f32");
}

int so3_angle_bwd_f64(const double *R1, const double *R2, const double *grad, double grad_div, double eps, unsigned flags, double *dR1, double *dR2,
                      int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_RADIANS | SO3_GRAD_SCALAR)) == 0, "so3_angle_bwd_f64: unknown flag");
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_angle_bwd_f64: B");
    SO3_CHECK_ARGS(eps >= 0.0 && eps < 1.0 && grad_div != 0.0, "so3_angle_bwd_f64: eps / grad_div");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && grad != nullptr && (dR1 != nullptr || dR2 != nullptr), "so3_angle_bwd_f64: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double unit = (flags & SO3_RADIANS) != 0 ? 1.0 : kDegPerRad;
    hipLaunchKernelGGL(k_angle_bwd_f64, dim3(capped_grid(B, 2048u)), dim3(kBlock), 0, s, R1, R2, grad, (flags & SO3_GRAD_SCALAR) != 0, grad_div,
                       unit, -1.0 + eps, 1.0 - eps, dR1, dR2, B);
    return check_launch("so3_angle_bwd_f64");
}

int so3_geodesic_eps_f64(const double *R1, const double *R2, double *theta, double *sum, double *result, int mean, double eps, int64_t B,
                         void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B && eps >= 0.0 && eps < 1.0, "so3_geodesic_eps_f64: B / eps");
    SO3_CHECK_ARGS(result == nullptr || sum != nullptr, "so3_geodesic_eps_f64: result needs the scratch `sum`");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (sum != nullptr) if (int e = zero_async(sum, sizeof(double), s, "so3_geodesic_eps_f64: memset")) return e;
    if (B > 0) {
        SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && (theta != nullptr || sum != nullptr), "so3_geodesic_eps_f64: null pointer");
        const dim3 grid(capped_grid(B, 2048u)), block(kBlock);
        with_flags([&](auto WD, auto WS) {
            if constexpr (WD() || WS())                         // (neither output: refused above)
                hipLaunchKernelGGL((k_angle_f64<2, WD(), WS()>), grid, block, 0, s, R1, R2, theta, sum, nullptr, 1.0, B, nullptr, 0, -1.0 + eps, 1.0 - eps);
        }, theta != nullptr, sum != nullptr);
    }
    // (torch's mean of an empty tensor is NaN, its sum 0)
    if (result != nullptr) k_mean_from_sum_f64<<<1, 1, 0, s>>>(sum, result, mean ? 1.0 / static_cast<double>(B) : 1.0);
    return check_launch("so3_geodesic_eps_f64");
}

int so3_ortho6d_fwd_f32(const float *X, float *R, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_ortho6d_fwd_f32: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(X != nullptr && R != nullptr, "so3_ortho6d_fwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Split sp(B, {X, R});
    const int64_t done = sp.done, rest = sp.rest;
    if (sp.nunits > 0) { so3::OpOrtho6d op; op.in0 = X; op.out0 = R; launch_rows<2, 4, 256>(op, sp.nunits, s); }
    if (rest > 0) hipLaunchKernelGGL((k_ortho6d_rows<false>), dim3(grid_for(rest)), dim3(kBlock), 0, s, X + done * 6, nullptr, R + done * 9, rest);
    return check_launch("so3_ortho6d_fwd_f32");
}

int so3_ortho6d_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_ortho6d_bwd_f32: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(X != nullptr && G != nullptr && dX != nullptr, "so3_ortho6d_bwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Split sp(B, {X, G, dX});
    const int64_t done = sp.done, rest = sp.rest;
    if (sp.nunits > 0) { so3::OpOrtho6dBwd op; op.in0 = X; op.in1 = G; op.out0 = dX; launch_rows<2, 4, 256>(op, sp.nunits, s); }
    if (rest > 0) hipLaunchKernelGGL((k_ortho6d_rows<true>), dim3(grid_for(rest)), dim3(kBlock), 0, s, X + done * 6, G + done * 9, dX + done * 6, rest);
    return check_launch("so3_ortho6d_bwd_f32");
}

// The other heads of the reference's dispatch tables (include/so3proj.h, "next row f5").
#define SO3_DEFINE_HEAD(NAME, OP)                                                                                   \
    int so3_##NAME##_fwd_f32(const float *X, float *R, int64_t B, void *stream) {                                    \
        SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_" #NAME "_fwd_f32: B");                                        \
        if (B == 0) return 0;                                                                                        \
        SO3_CHECK_ARGS(X != nullptr && R != nullptr, "so3_" #NAME "_fwd_f32: null pointer");                         \
        so3::OP<false> op; op.in0 = X; op.out0 = R;                                                                  \
        return run_row_op<1, 6, 256>(op, B, static_cast<hipStream_t>(stream), "so3_" #NAME "_fwd_f32");              \
    }                                                                                                                \
    int so3_##NAME##_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream) {                   \
        SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_" #NAME "_bwd_f32: B");                                        \
        if (B == 0) return 0;                                                                                        \
        SO3_CHECK_ARGS(X != nullptr && G != nullptr && dX != nullptr, "so3_" #NAME "_bwd_f32: null pointer");        \
        so3::OP<true> op; op.in0 = X; op.in1 = G; op.out0 = dX;                                                      \
        return run_row_op<1, 6, 256>(op, B, static_cast<hipStream_t>(stream), "so3_" #NAME "_bwd_f32");              \
    }
SO3_DEFINE_HEAD(quat, OpQuat)
SO3_DEFINE_HEAD(euler, OpEuler)
SO3_DEFINE_HEAD(ortho5d, OpOrtho5d)
SO3_DEFINE_HEAD(expmap, OpExpMap)
#undef SO3_DEFINE_HEAD

// The inverse maps (include/so3proj.h, "inverse maps"): R (B,9) -> W numbers per row, and the tangent-space gradient back.
#define SO3_DEFINE_INVERSE(NAME, OP)                                                                                \
    int so3_##NAME##_fwd_f32(const float *R, float *Y, int64_t B, void *stream) {                                    \
        SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_" #NAME "_fwd_f32: B");                                        \
        if (B == 0) return 0;                                                                                        \
        SO3_CHECK_ARGS(R != nullptr && Y != nullptr, "so3_" #NAME "_fwd_f32: null pointer");                         \
        so3::OP<false> op; op.in0 = R; op.out0 = Y;                                                                  \
        return run_row_op<SO3_INV_NPL, SO3_INV_WPS, 256>(op, B, static_cast<hipStream_t>(stream), "so3_" #NAME "_fwd_f32"); \
    }                                                                                                                \
    int so3_##NAME##_bwd_f32(const float *R, const float *G, float *dR, int64_t B, void *stream) {                   \
        SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_" #NAME "_bwd_f32: B");                                        \
        if (B == 0) return 0;                                                                                        \
        SO3_CHECK_ARGS(R != nullptr && G != nullptr && dR != nullptr, "so3_" #NAME "_bwd_f32: null pointer");        \
        so3::OP<true> op; op.in0 = R; op.in1 = G; op.out0 = dR;                                                      \
        return run_row_op<SO3_INV_NPL, SO3_INV_WPS, 256>(op, B, static_cast<hipStream_t>(stream), "so3_" #NAME "_bwd_f32"); \
    }
SO3_DEFINE_INVERSE(mat_to_quat, OpMatToQuat)
SO3_DEFINE_INVERSE(logmap, OpLogMap)
SO3_DEFINE_INVERSE(mat_to_euler, OpMatToEuler)
#undef SO3_DEFINE_INVERSE

int so3_relative_log_fwd_f32(const float *R1, const float *R2, float *V, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_relative_log_fwd_f32: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && V != nullptr, "so3_relative_log_fwd_f32: null pointer");
    so3::OpRelLog<false, false> op; op.in0 = R1; op.in1 = R2; op.out0 = V;
    return run_row_op<SO3_INV_NPL, SO3_INV_WPS, 256>(op, B, static_cast<hipStream_t>(stream), "so3_relative_log_fwd_f32");
}

int so3_relative_log_bwd_f32(const float *R1, const float *R2, const float *G, float *dR1, float *dR2, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_relative_log_bwd_f32: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R1 != nullptr && R2 != nullptr && G != nullptr && (dR1 != nullptr || dR2 != nullptr), "so3_relative_log_bwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dR1 != nullptr && dR2 != nullptr) {
        so3::OpRelLog<true, true> op; op.in0 = R1; op.in1 = R2; op.in2 = G; op.out0 = dR2; op.out1 = dR1;
        return run_row_op<SO3_INV_NPL, SO3_RELLOG_BWD_WPS, 256>(op, B, s, "so3_relative_log_bwd_f32");
    }
    // one gradient alone: log(R1^T R2) = -log(R2^T R1), so dR1 is the second argument's gradient of the swapped pair under -g
    so3::OpRelLog<true, false> op; op.in2 = G;
    if (dR2 != nullptr) { op.in0 = R1; op.in1 = R2; op.out0 = dR2; }
    else { op.in0 = R2; op.in1 = R1; op.out0 = dR1; op.gsign = -1.f; }
    return run_row_op<SO3_INV_NPL, SO3_RELLOG_BWD_WPS, 256>(op, B, s, "so3_relative_log_bwd_f32");
}

int so3_add_l1_f32(const float *Tgt, const float *Tpred, const float *points, float *dists, double *loss_sum, float *dTpred,
                   float grad_scale, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, 1, 150000000), "so3_add_l1_f32: B/N");
    SO3_CHECK_ARGS(B == 0 || (Tgt != nullptr && Tpred != nullptr && points != nullptr), "so3_add_l1_f32: null pointer");
    return launch_add_l1<false>(Tgt, Tpred, points, dists, loss_sum, dTpred, grad_scale, B, N, static_cast<hipStream_t>(stream), "so3_add_l1_f32");
}

int so3_add_l2_f32(const float *Tgt, const float *Tpred, const float *points, float *dists, double *loss_sum, float *dTpred,
                   float grad_scale, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, 1, 150000000), "so3_add_l2_f32: B/N");
    SO3_CHECK_ARGS(B == 0 || (Tgt != nullptr && Tpred != nullptr && points != nullptr), "so3_add_l2_f32: null pointer");
    return launch_add_l1<false, true>(Tgt, Tpred, points, dists, loss_sum, dTpred, grad_scale, B, N, static_cast<hipStream_t>(stream), "so3_add_l2_f32");
}

int so3_add_s_fwd_f32(const float *Tgt, const float *Tpred, const float *points, float *point_dist, int32_t *nearest, float *dists,
                      double *loss_sum, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N), "so3_add_s_fwd_f32: B/N");
    SO3_CHECK_ARGS(B == 0 || (Tgt != nullptr && Tpred != nullptr && points != nullptr && point_dist != nullptr), "so3_add_s_fwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B == 0) {
        if (loss_sum != nullptr) if (int e = zero_async(loss_sum, sizeof(double), s, "so3_add_s_fwd_f32")) return e;
        return 0;
    }
    return launch_add_s<false>(Tgt, Tpred, points, point_dist, nearest, dists, loss_sum, B, N, s, "so3_add_s_fwd_f32");
}

int so3_add_s_bwd_f32(const float *Tgt, const float *Tpred, const float *points, const int32_t *nearest, const float *grad_rows,
                      float grad_scale, float *dTpred, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N), "so3_add_s_bwd_f32: B/N");
    SO3_CHECK_ARGS(B == 0 || (Tgt != nullptr && Tpred != nullptr && points != nullptr && nearest != nullptr && dTpred != nullptr),
                   "so3_add_s_bwd_f32: null pointer");
    if (B == 0) return 0;
    hipLaunchKernelGGL(k_add_s_bwd, dim3(wave_rows_grid(B, 8)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), Tgt, Tpred, points,
                       nearest, grad_rows, grad_scale, dTpred, B, N);
    return check_launch("so3_add_s_bwd_f32");
}

int so3_cloud_diameter_f32(const float *points, float *work, float *diam, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N), "so3_cloud_diameter_f32: B/N");
    SO3_CHECK_ARGS(B == 0 || (points != nullptr && work != nullptr && diam != nullptr), "so3_cloud_diameter_f32: null pointer");
    if (B == 0) return 0;
    return launch_add_s<true>(nullptr, nullptr, points, work, nullptr, diam, nullptr, B, N, static_cast<hipStream_t>(stream), "so3_cloud_diameter_f32");
}

int so3_nearest_f32(const float *X, const float *Y, int64_t y_stride, float *dist, int32_t *nearest, int64_t B, int32_t N, int32_t M,
                    void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_nearest_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(y_stride == 0 || y_stride >= static_cast<int64_t>(M) * 3, "so3_nearest_f32: y_stride");
    SO3_CHECK_ARGS(X != nullptr && Y != nullptr && dist != nullptr, "so3_nearest_f32: null pointer");
    int u;
    const int32_t chunks = icp_chunks(B, N, u);
    launch_icp_step<false>(X, Y, y_stride, nullptr, nullptr, -1.f, nullptr, dist, nearest, B, N, M, u, chunks, static_cast<hipStream_t>(stream));
    return check_launch("so3_nearest_f32");
}

size_t so3_icp_workspace_bytes(int64_t B, int32_t N) {
    if (!cloud_dims_ok(B, N)) return 0;
    // two pose buffers and one record per work item at the smallest work item (U = 1), whatever the device
    return static_cast<size_t>(B) * (2 * 12 + static_cast<size_t>((N + kBlock - 1) / kBlock) * so3::kIcpRecord) * sizeof(float);
}

int so3_icp_f32(const float *P, const float *Q, int64_t q_stride, const float *w, const float *T_init, float max_distance, int32_t iterations,
                float *R, float *t, float *rmse, int32_t *inliers, int32_t *nearest, float *dist, void *workspace, int64_t B, int32_t N,
                int32_t M, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_icp_f32: B/N");
    SO3_CHECK_ARGS(iterations >= 0 && iterations <= SO3_ICP_MAX_ITERATIONS, "so3_icp_f32: iterations");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(q_stride == 0 || q_stride >= static_cast<int64_t>(M) * 3, "so3_icp_f32: q_stride");
    SO3_CHECK_ARGS(P != nullptr && Q != nullptr && R != nullptr && t != nullptr && (iterations == 0 || workspace != nullptr), "so3_icp_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kBlock);
    int u;
    const int32_t chunks = icp_chunks(B, N, u);
    if (iterations == 0) {
        hipLaunchKernelGGL(k_icp_initial_pose, dim3(static_cast<unsigned>((B * 12 + kBlock - 1) / kBlock)), block, 0, s, T_init, R, t, B);
        if (nearest != nullptr || dist != nullptr)           // the search at the initial pose, so that the outputs are defined
            launch_icp_step<false>(P, Q, q_stride, nullptr, T_init, -1.f, nullptr, dist, nearest, B, N, M, u, chunks, s);
        return check_launch("so3_icp_f32");
    }
    float *poses[2] = {static_cast<float *>(workspace), static_cast<float *>(workspace) + B * 12};
    float *rec = static_cast<float *>(workspace) + B * 24;
    const unsigned fin_blocks = wave_rows_grid(B, 16);
    const float *cur = T_init;
    for (int32_t k = 0; k < iterations; ++k) {
        const bool last = k + 1 == iterations;
        float *next = poses[k & 1];
        launch_icp_step<true>(P, Q, q_stride, w, cur, max_distance, rec, last ? dist : nullptr, last ? nearest : nullptr, B, N, M, u, chunks, s);
        hipLaunchKernelGGL(k_icp_finish, dim3(fin_blocks), block, 0, s, P, Q, q_stride, rec, cur, next, last ? R : nullptr,
                           last ? t : nullptr, rmse != nullptr ? rmse + k * B : nullptr, inliers != nullptr ? inliers + k * B : nullptr, B, N, chunks);
        cur = next;
    }
    return check_launch("so3_icp_f32");
}

size_t so3_icp_plane_workspace_bytes(int64_t B, int32_t N) {
    if (!cloud_dims_ok(B, N)) return 0;
    // two pose buffers and one record per work item at the smallest work item (U = 1), whatever the device
    return static_cast<size_t>(B) * (2 * 12 + static_cast<size_t>((N + kBlock - 1) / kBlock) * so3::kPlaneRecord) * sizeof(float);
}

int so3_icp_plane_f32(const float *P, const float *Q, const float *normals, int64_t q_stride, const float *w, const float *T_init,
                      float max_distance, float damping, int32_t iterations, float *R, float *t, float *rmse, float *rmse_point,
                      int32_t *inliers, int32_t *solved, int32_t *nearest, float *dist, void *workspace, int64_t B, int32_t N, int32_t M,
                      void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_icp_plane_f32: B/N");
    SO3_CHECK_ARGS(iterations >= 0 && iterations <= SO3_ICP_MAX_ITERATIONS, "so3_icp_plane_f32: iterations");
    SO3_CHECK_ARGS(damping >= 0.f, "so3_icp_plane_f32: damping");                      // a NaN fails the comparison
    if (B == 0) return 0;
    SO3_CHECK_ARGS(q_stride == 0 || q_stride >= static_cast<int64_t>(M) * 3, "so3_icp_plane_f32: q_stride");
    SO3_CHECK_ARGS(P != nullptr && Q != nullptr && normals != nullptr && R != nullptr && t != nullptr && (iterations == 0 || workspace != nullptr),
                   "so3_icp_plane_f32: null pointer");
    static_assert(so3::kPlanePivotEps == SO3_ICP_PLANE_PIVOT_EPS, "include/so3proj.h");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kBlock);
    int u;
    const int32_t chunks = icp_chunks(B, N, u);
    if (iterations == 0) {
        hipLaunchKernelGGL(k_icp_initial_pose, dim3(static_cast<unsigned>((B * 12 + kBlock - 1) / kBlock)), block, 0, s, T_init, R, t, B);
        if (nearest != nullptr || dist != nullptr)           // the search at the initial pose, so that the outputs are defined
            launch_icp_step<false>(P, Q, q_stride, nullptr, T_init, -1.f, nullptr, dist, nearest, B, N, M, u, chunks, s);
        return check_launch("so3_icp_plane_f32");
    }
    float *poses[2] = {static_cast<float *>(workspace), static_cast<float *>(workspace) + B * 12};
    float *rec = static_cast<float *>(workspace) + B * 24;
    const dim3 grid(search_grid(B * chunks)), fin_grid(wave_rows_grid(B, 16));
    const float *cur = T_init;
    for (int32_t k = 0; k < iterations; ++k) {
        const bool last = k + 1 == iterations;
        float *next = poses[k & 1];
        with_flags([&](auto WW, auto TT) {
            constexpr bool kWeighted = WW(), kTrimmed = TT();
            with_value<4, 2, 1>(u, [&](auto U) {
                name_kernel("k_icp_plane_step", kWeighted, kTrimmed, U);
                hipLaunchKernelGGL((k_icp_plane_step<kWeighted, kTrimmed, U()>), grid, block, 0, s, P, Q, normals, q_stride, w, cur, max_distance, rec,
                                   last ? dist : nullptr, last ? nearest : nullptr, B, N, M, chunks);
            });
        }, w != nullptr, max_distance >= 0.f);
        hipLaunchKernelGGL(k_icp_plane_finish, fin_grid, block, 0, s, P, rec, cur, damping, next, last ? R : nullptr, last ? t : nullptr,
                           rmse != nullptr ? rmse + k * B : nullptr, rmse_point != nullptr ? rmse_point + k * B : nullptr,
                           inliers != nullptr ? inliers + k * B : nullptr, solved != nullptr ? solved + k * B : nullptr, B, N, chunks);
        cur = next;
    }
    return check_launch("so3_icp_plane_f32");
}

size_t so3_chamfer_workspace_bytes(int64_t B, int32_t N, int32_t M) {
    if (!cloud_dims_ok(B, N, M)) return 0;
    // one float per work item at the smallest work item (U = 1), both directions, whatever the device
    const ChamferChunks ch = chamfer_chunks(N, M, false, 1);
    return static_cast<size_t>(B) * (static_cast<size_t>(ch.x) + static_cast<size_t>(ch.y)) * sizeof(float);
}

int so3_chamfer_fwd_f32(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, float *dist_x, int32_t *nearest_x,
                        float *dist_y, int32_t *nearest_y, float *rows, void *work, uint32_t flags, int64_t B, int32_t N, int32_t M,
                        void *stream) {
    return launch_chamfer_fwd<false>("so3_chamfer_fwd_f32", X, Y, nullptr, nullptr, x_len, y_len, dist_x, nearest_x, dist_y, nearest_y, nullptr, nullptr,
                                     rows, nullptr, work, flags, B, N, M, stream);
}

int so3_chamfer_bwd_f32(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, const int32_t *nearest_x,
                        const int32_t *nearest_y, const float *scale_x, const float *scale_y, float *dX, float *dY, uint32_t flags, int64_t B,
                        int32_t N, int32_t M, void *stream) {
    if (int e = check_chamfer_bwd("so3_chamfer_bwd_f32", SO3_CHAMFER_UNSQUARED | SO3_CHAMFER_SINGLE, X, Y, nearest_x, nearest_y, scale_x, scale_y, dX, dY,
                                  flags, B, N, M)) return e;
    if (B == 0) return 0;
    const ChamferChunks ch = chamfer_chunks(N, M, false, 1);
    with_flags([&](auto SQ) {
        name_kernel("k_chamfer_bwd", SQ);
        hipLaunchKernelGGL((k_chamfer_bwd<SQ()>), dim3(chamfer_grid(B, ch)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), X, Y, x_len, y_len,
                           nearest_x, nearest_y, scale_x, scale_y, dX, dY, B, N, M, ch.x, ch.y);
    }, (flags & SO3_CHAMFER_UNSQUARED) == 0);
    return check_launch("so3_chamfer_bwd_f32");
}

size_t so3_chamfer_normals_workspace_bytes(int64_t B, int32_t N, int32_t M) {
    // two floats per work item (the distance's sum and the normal term's) at the smallest work item (U = 1), both directions
    return 2 * so3_chamfer_workspace_bytes(B, N, M);
}

int so3_chamfer_normals_fwd_f32(const float *X, const float *Y, const float *NX, const float *NY, const int32_t *x_len, const int32_t *y_len,
                                float *dist_x, int32_t *nearest_x, float *dist_y, int32_t *nearest_y, float *term_x, float *term_y, float *rows,
                                float *rows_n, void *work, uint32_t flags, int64_t B, int32_t N, int32_t M, void *stream) {
    return launch_chamfer_fwd<true>("so3_chamfer_normals_fwd_f32", X, Y, NX, NY, x_len, y_len, dist_x, nearest_x, dist_y, nearest_y, term_x, term_y, rows,
                                    rows_n, work, flags, B, N, M, stream);
}

int so3_chamfer_normals_bwd_f32(const float *NX, const float *NY, const int32_t *x_len, const int32_t *y_len, const int32_t *nearest_x,
                                const int32_t *nearest_y, const float *scale_x, const float *scale_y, float *dNX, float *dNY, uint32_t flags,
                                int64_t B, int32_t N, int32_t M, void *stream) {
    if (int e = check_chamfer_bwd("so3_chamfer_normals_bwd_f32", SO3_CHAMFER_UNSQUARED | SO3_CHAMFER_SINGLE | SO3_CHAMFER_SIGNED_COSINE, NX, NY, nearest_x,
                                  nearest_y, scale_x, scale_y, dNX, dNY, flags, B, N, M)) return e;
    if (B == 0) return 0;
    const ChamferChunks ch = chamfer_chunks(N, M, false, 1);
    name_kernel("k_chamfer_normals_bwd");
    hipLaunchKernelGGL(k_chamfer_normals_bwd, dim3(chamfer_grid(B, ch)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), NX, NY, x_len, y_len,
                       nearest_x, nearest_y, scale_x, scale_y, dNX, dNY, (flags & SO3_CHAMFER_SIGNED_COSINE) != 0 ? 1 : 0, B, N, M, ch.x, ch.y);
    return check_launch("so3_chamfer_normals_bwd_f32");
}

int so3_knn_f32(const float *X, const float *Y, int64_t y_stride, const int32_t *x_len, const int32_t *y_len, float *dist2, int32_t *idx, int32_t K,
                int64_t B, int32_t N, int32_t M, void *stream) {
    static_assert(SO3_KNN_MAX_K == so3::kKnnMaxK, "the header's limit is the kernel's");
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_knn_f32: B/N/M");
    SO3_CHECK_ARGS(knn_k_ok(K), "so3_knn_f32: K");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(y_stride == 0 || y_stride >= static_cast<int64_t>(M) * 3, "so3_knn_f32: y_stride");
    SO3_CHECK_ARGS(X != nullptr && Y != nullptr && idx != nullptr, "so3_knn_f32: null pointer");
    with_value<so3::kKnnWideQ, so3::kKnnNarrowQ>(so3::knn_queries_per_wave(B, N, M), [&](auto QQ) {
        constexpr int kPer = kBlock / 64 * QQ();
        const int32_t chunks = (N + kPer - 1) / kPer;
        name_kernel("k_knn", QQ);
        hipLaunchKernelGGL((k_knn<QQ()>), dim3(static_cast<unsigned>(std::min<int64_t>(B * chunks, kThreeMaxGrid))), dim3(kBlock), 0,
                           static_cast<hipStream_t>(stream), X, Y, y_stride, x_len, y_len, dist2, idx, K, B, N, M, chunks);
    });
    return check_launch("so3_knn_f32");
}

int so3_knn_bwd_f32(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, const int32_t *idx, const float *grad_dist2,
                    float *dX, float *dY, int32_t K, int64_t B, int32_t N, int32_t M, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_knn_bwd_f32: B/N/M");
    SO3_CHECK_ARGS(knn_k_ok(K), "so3_knn_bwd_f32: K");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(X != nullptr && Y != nullptr && idx != nullptr && grad_dist2 != nullptr && (dX != nullptr || dY != nullptr),
                   "so3_knn_bwd_f32: null pointer");
    const ChamferChunks ch = chamfer_chunks(N, M, false, 1);
    name_kernel("k_knn_bwd");
    hipLaunchKernelGGL(k_knn_bwd, dim3(chamfer_grid(B, ch)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), X, Y, x_len, y_len, idx, grad_dist2, dX,
                       dY, K, B, N, M, ch.x, ch.y);
    return check_launch("so3_knn_bwd_f32");
}

int so3_local_frames_f32(const float *Y, int64_t y_stride, const int32_t *idx, const int32_t *x_len, const int32_t *y_len, const float *viewpoint,
                         float *cov, float *eigenvalues, float *normals, float *frames, int32_t K, int64_t B, int32_t N, int32_t M, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_local_frames_f32: B/N/M");
    SO3_CHECK_ARGS(knn_k_ok(K), "so3_local_frames_f32: K");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(y_stride == 0 || y_stride >= static_cast<int64_t>(M) * 3, "so3_local_frames_f32: y_stride");
    SO3_CHECK_ARGS(Y != nullptr && idx != nullptr && (cov != nullptr || eigenvalues != nullptr || normals != nullptr || frames != nullptr),
                   "so3_local_frames_f32: null pointer");
    const int32_t chunks = (N + kBlock - 1) / kBlock;
    name_kernel("k_local_frames");
    hipLaunchKernelGGL(k_local_frames, dim3(static_cast<unsigned>(std::min<int64_t>(B * chunks, kThreeMaxGrid))), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), Y, y_stride, idx, x_len, y_len, viewpoint, cov, eigenvalues, normals, frames, K, B, N, M, chunks);
    return check_launch("so3_local_frames_f32");
}

int so3_spfh_f32(const float *X, const float *normals, const int32_t *idx, const int32_t *len, float *spfh, int32_t *pairs, int32_t K, int64_t B,
                 int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N), "so3_spfh_f32: B/N");
    SO3_CHECK_ARGS(knn_k_ok(K), "so3_spfh_f32: K");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(X != nullptr && normals != nullptr && idx != nullptr && (spfh != nullptr || pairs != nullptr), "so3_spfh_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int width = 1;                                               // the power of two >= K
    while (width < K) width *= 2;
    with_value<1, 2, 4, 8, 16, 32, 64>(width, [&](auto GG) {
        constexpr int G = GG();
        const int32_t chunks = (N + kBlock / G - 1) / (kBlock / G);
        name_kernel("k_spfh", GG);
        hipLaunchKernelGGL((k_spfh<G>), dim3(static_cast<unsigned>(std::min<int64_t>(B * chunks, kThreeMaxGrid))), dim3(kBlock), 0, s, X, normals, idx,
                           len, spfh, pairs, K, B, N, chunks);
    });
    return check_launch("so3_spfh_f32");
}

int so3_fpfh_f32(const float *X, const int32_t *idx, const int32_t *len, const float *spfh, const int32_t *pairs, float *fpfh, int32_t K, int64_t B,
                 int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N), "so3_fpfh_f32: B/N");
    SO3_CHECK_ARGS(knn_k_ok(K), "so3_fpfh_f32: K");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(X != nullptr && idx != nullptr && spfh != nullptr && pairs != nullptr && fpfh != nullptr, "so3_fpfh_f32: null pointer");
    const int32_t chunks = (N * so3::kFpfhSlots + kBlock - 1) / kBlock;
    name_kernel("k_fpfh");
    hipLaunchKernelGGL(k_fpfh, dim3(static_cast<unsigned>(std::min<int64_t>(B * chunks, kThreeMaxGrid))), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), X, idx, len, spfh, pairs, fpfh, K, B, N, chunks);
    return check_launch("so3_fpfh_f32");
}

inline bool ransac_hypotheses_ok(int32_t H) {
    static_assert(SO3_RANSAC_MAX_HYPOTHESES == so3::kRansacMaxHypotheses, "the header's limit is the device header's");
    return H >= 1 && H <= SO3_RANSAC_MAX_HYPOTHESES;
}
inline bool ransac_distance_ok(float max_distance) { return max_distance >= 0.f && max_distance < __builtin_inff(); }   // a NaN fails

int so3_ransac_score_f32(const float *P, const float *Q, const int32_t *corr, const int32_t *x_len, const int32_t *y_len, const int32_t *samples,
                         float max_distance, float edge_similarity, float *T_hyp, int32_t *count, float *err, int64_t B, int32_t N, int32_t M,
                         int32_t H, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_ransac_score_f32: B/N/M");
    SO3_CHECK_ARGS(ransac_hypotheses_ok(H), "so3_ransac_score_f32: H");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(ransac_distance_ok(max_distance), "so3_ransac_score_f32: max_distance");
    SO3_CHECK_ARGS(edge_similarity >= 0.f && edge_similarity <= 1.f, "so3_ransac_score_f32: edge_similarity");
    SO3_CHECK_ARGS(P != nullptr && Q != nullptr && corr != nullptr && samples != nullptr && T_hyp != nullptr && count != nullptr && err != nullptr,
                   "so3_ransac_score_f32: null pointer");
    const int32_t chunks = (H + kBlock - 1) / kBlock;
    name_kernel("k_ransac_score");
    hipLaunchKernelGGL(k_ransac_score, dim3(static_cast<unsigned>(std::min<int64_t>(B * chunks, kThreeMaxGrid))), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), P, Q, corr, x_len, y_len, samples, max_distance, edge_similarity, T_hyp, count, err, B, N, M, H,
                       chunks);
    return check_launch("so3_ransac_score_f32");
}

int so3_ransac_select_f32(const float *P, const float *Q, const int32_t *corr, const int32_t *x_len, const int32_t *y_len, const float *T_hyp,
                          const int32_t *count, const float *err, float max_distance, int32_t *best, float *T_best, int32_t *inliers, float *rmse,
                          float *weights, float *targets, int64_t B, int32_t N, int32_t M, int32_t H, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, M), "so3_ransac_select_f32: B/N/M");
    SO3_CHECK_ARGS(ransac_hypotheses_ok(H), "so3_ransac_select_f32: H");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(ransac_distance_ok(max_distance), "so3_ransac_select_f32: max_distance");
    SO3_CHECK_ARGS(P != nullptr && Q != nullptr && corr != nullptr && T_hyp != nullptr && count != nullptr && err != nullptr && best != nullptr &&
                       T_best != nullptr && inliers != nullptr && rmse != nullptr && weights != nullptr && targets != nullptr,
                   "so3_ransac_select_f32: null pointer");
    name_kernel("k_ransac_select");
    hipLaunchKernelGGL(k_ransac_select, dim3(static_cast<unsigned>(std::min<int64_t>(B, kThreeMaxGrid))), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), P, Q, corr, x_len, y_len, T_hyp, count, err, max_distance, best, T_best, inliers, rmse, weights,
                       targets, B, N, M, H);
    return check_launch("so3_ransac_select_f32");
}

int so3_fps_f32(const float *xyz, const int32_t *start, int32_t *out, int64_t B, int32_t N, int32_t npoint, void *stream) {
    static_assert(SO3_FPS_MAX_N == so3::kFpsMaxN, "the header's limit is the dispatch's");
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, npoint, SO3_FPS_MAX_N), "so3_fps_f32: B/N/npoint");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(xyz != nullptr && start != nullptr && out != nullptr, "so3_fps_f32: null pointer");
    int ppl, block;
    so3::fps_shape(N, ppl, block);
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(B, kFpsMaxGrid)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch = [&](auto PP, auto BB) {
        name_kernel("k_fps", PP, BB);
        hipLaunchKernelGGL((k_fps<PP(), BB()>), grid, dim3(BB()), 0, s, xyz, start, out, B, N, npoint);
    };
    // the shapes so3::fps_shape hands out: up to eight points per lane of 256, then four to sixteen of 1024
    const bool found = block == 256    ? with_value<1, 2, 4, 8>(ppl, [&](auto PP) { launch(PP, std::integral_constant<int, 256>{}); })
                       : block == 1024 ? with_value<4, 8, 16>(ppl, [&](auto PP) { launch(PP, std::integral_constant<int, 1024>{}); })
                                       : false;
    if (!found) return fail(SO3_ERR_INVALID, "so3_fps_f32: no kernel for this N");
    return check_launch("so3_fps_f32");
}

int so3_ball_query_f32(const float *xyz, const float *centres, float radius, int32_t nsample, int32_t *idx, int32_t *count, int64_t B,
                       int32_t N, int32_t S, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, S) && nsample >= 1,
                   "so3_ball_query_f32: B/N/S/nsample");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(xyz != nullptr && centres != nullptr && idx != nullptr, "so3_ball_query_f32: null pointer");
    const int32_t width = std::min(nsample, N);
    const dim3 grid(wave_rows_grid(B * S, 32)), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_flags([&](auto COUNT) {
        name_kernel("k_ball_query", COUNT);
        hipLaunchKernelGGL(k_ball_query<COUNT()>, grid, block, 0, s, xyz, centres, radius, width, idx, count, B, N, S);
    }, count != nullptr);
    return check_launch("so3_ball_query_f32");
}

int so3_three_nn_f32(const float *unknown, const float *known, float *dist2, int32_t *idx, float *weight, int64_t B, int32_t N, int32_t S,
                     void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, S), "so3_three_nn_f32: B/N/S");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(unknown != nullptr && known != nullptr && dist2 != nullptr && idx != nullptr, "so3_three_nn_f32: null pointer");
    const int wpp = so3::three_nn_waves_per_point(B, N, S);
    const int32_t chunks = (N + kBlock / wpp - 1) / (kBlock / wpp);
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(B * chunks, kThreeMaxGrid))), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_flags([&](auto WEIGHT) {
        constexpr bool kWeight = WEIGHT();
        with_value<4, 1>(wpp, [&](auto WPP) {
            name_kernel("k_three_nn", WPP, kWeight);
            hipLaunchKernelGGL((k_three_nn<WPP(), kWeight>), grid, block, 0, s, unknown, known, dist2, idx, weight, B, N, S, chunks);
        });
    }, weight != nullptr);
    return check_launch("so3_three_nn_f32");
}

int so3_three_interpolate_f32(const float *feat, const int32_t *idx, const float *weight, float *out, int32_t channels_first, int64_t B,
                              int32_t N, int32_t S, int32_t D, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, S) && D >= 1 && D <= SO3_THREE_MAX_D,
                   "so3_three_interpolate_f32: B/N/S/D");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(feat != nullptr && idx != nullptr && weight != nullptr && out != nullptr, "so3_three_interpolate_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t gw = 64;
    while (gw > 1 && gw / 2 >= D) gw >>= 1;
    int64_t blocks;
    if (channels_first) {
        blocks = B * ((N + kBlock - 1) / kBlock) * ((D + kThreeCfChannels - 1) / kThreeCfChannels);
    } else {
        const int64_t rows_per_block = (kBlock / 64) * (64 / gw);
        blocks = (B * N + rows_per_block - 1) / rows_per_block;
    }
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(blocks, kThreeMaxGrid))), block(kBlock);
    with_flags([&](auto CF) {
        name_kernel("k_three_interp", CF);
        hipLaunchKernelGGL(k_three_interp<CF()>, grid, block, 0, s, feat, idx, weight, out, B, N, S, D, gw);
    }, channels_first != 0);
    return check_launch("so3_three_interpolate_f32");
}

int so3_three_interpolate_bwd_f32(const float *grad_out, const int32_t *idx, const float *weight, float *grad_feat, int32_t channels_first,
                                  int64_t B, int32_t N, int32_t S, int32_t D, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, S) && D >= 1 && D <= SO3_THREE_MAX_D,
                   "so3_three_interpolate_bwd_f32: B/N/S/D");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(grad_out != nullptr && idx != nullptr && weight != nullptr && grad_feat != nullptr, "so3_three_interpolate_bwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t blocks = channels_first ? B * ((S + 63) / 64) * ((D + 63) / 64) : B * ((S + kThreeBwdS - 1) / kThreeBwdS);
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(blocks, kThreeMaxGrid))), block(kBlock);
    g_last_kernel = channels_first ? "k_three_interp_bwd_cf" : "k_three_interp_bwd_cl";
    if (channels_first) hipLaunchKernelGGL(k_three_interp_bwd_cf, grid, block, 0, s, grad_out, idx, weight, grad_feat, B, N, S, D);
    else hipLaunchKernelGGL(k_three_interp_bwd_cl, grid, block, 0, s, grad_out, idx, weight, grad_feat, B, N, S, D);
    return check_launch("so3_three_interpolate_bwd_f32");
}

int so3_group_points_f32(const float *xyz, const float *centres, const float *feat, const int32_t *idx, float *out, int32_t features_first,
                         int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t K, int32_t D, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, S) && K >= 1 &&
                       K <= SO3_GROUP_MAX_K && D >= 0 && D <= SO3_THREE_MAX_D,
                   "so3_group_points_f32: B/N/S/K/D");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(xyz != nullptr && centres != nullptr && idx != nullptr && out != nullptr && (D == 0 || feat != nullptr),
                   "so3_group_points_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int32_t C = 3 + D;
    int32_t gw = 64;
    while (gw > 1 && gw / 2 >= C) gw >>= 1;
    int64_t blocks;
    if (channels_first) {
        blocks = B * K * ((S + kBlock - 1) / kBlock) * ((C + so3::kGroupFwdCfChannels - 1) / so3::kGroupFwdCfChannels);
    } else {
        const int64_t rows_per_block = (kBlock / 64) * (64 / gw);
        blocks = (B * S * K + rows_per_block - 1) / rows_per_block;
    }
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(blocks, kThreeMaxGrid))), block(kBlock);
    with_flags([&](auto CF) {
        name_kernel("k_group_fwd", CF);
        hipLaunchKernelGGL(k_group_fwd<CF()>, grid, block, 0, s, xyz, centres, feat, idx, out, features_first, B, N, S, K, D, gw);
    }, channels_first != 0);
    return check_launch("so3_group_points_f32");
}

int so3_group_points_bwd_f32(const float *grad_out, const int32_t *idx, float *grad_xyz, float *grad_centres, float *grad_feat,
                             int32_t features_first, int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t K, int32_t D, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, S) && K >= 1 &&
                       K <= SO3_GROUP_MAX_K && D >= 0 && D <= SO3_THREE_MAX_D,
                   "so3_group_points_bwd_f32: B/N/S/K/D");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(grad_out != nullptr && idx != nullptr, "so3_group_points_bwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kBlock);
    if (D == 0) grad_feat = nullptr;
    if (grad_centres != nullptr) {
        const dim3 grid(static_cast<unsigned>(std::min<int64_t>((B * S + kBlock - 1) / kBlock, kThreeMaxGrid)));
        with_flags([&](auto CF) {
            name_kernel("k_group_centres_bwd", CF);
            hipLaunchKernelGGL(k_group_centres_bwd<CF()>, grid, block, 0, s, grad_out, idx, grad_centres, features_first, B, N, S, K, D);
        }, channels_first != 0);
    }
    if (grad_xyz != nullptr || grad_feat != nullptr) {
        const bool narrow = so3::group_bwd_narrow(D);
        const int owners = narrow ? so3::kGroupNarrowOwners : so3::kGroupWideOwners, cw = narrow ? so3::kGroupNarrowC : so3::kGroupWideChannels;
        const int64_t blocks = B * ((N + owners - 1) / owners) * ((3 + D + cw - 1) / cw);
        const dim3 grid(static_cast<unsigned>(std::min<int64_t>(blocks, kThreeMaxGrid)));
        with_flags([&](auto CF, auto NARROW) {
            // channels per owner group and owners per lane (so3_device.h, k_group_bwd<CF, CW, R>)
            constexpr int kCw = NARROW() ? so3::kGroupNarrowC : so3::kGroupWideChannels, kR = NARROW() ? 2 : 16;
            name_kernel("k_group_bwd", CF, kCw, kR);
            hipLaunchKernelGGL((k_group_bwd<CF(), kCw, kR>), grid, block, 0, s, grad_out, idx, grad_xyz, grad_feat, features_first, B, N, S, K, D);
        }, channels_first != 0, narrow);
    }
    return check_launch("so3_group_points_bwd_f32");
}

int so3_add_l1_disentangled_f32(const float *Tpred, const float *Tgt, const float *points, double *loss_sum, float *dTpred,
                                float grad_scale, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, 1, 150000000), "so3_add_l1_disentangled_f32: B/N");
    SO3_CHECK_ARGS(B == 0 || (Tgt != nullptr && Tpred != nullptr && points != nullptr), "so3_add_l1_disentangled_f32: null pointer");
    return launch_add_l1<true>(Tgt, Tpred, points, nullptr, loss_sum, dTpred, grad_scale, B, N, static_cast<hipStream_t>(stream),
                               "so3_add_l1_disentangled_f32");
}

int so3_rotate_clouds_f32(const float *P, const float *R, float *out, int transposed, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 31) && N >= 0 && N <= 150000000, "so3_rotate_clouds_f32: B/N");
    if (B == 0 || N == 0) return 0;
    SO3_CHECK_ARGS(P != nullptr && R != nullptr && out != nullptr, "so3_rotate_clouds_f32: null pointer");
    const CloudShape shape = cloud_shape(B);
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_flags([&](auto T) { hipLaunchKernelGGL((k_rotate_clouds<T()>), grid, block, 0, s, P, R, out, B, N, shape.per_wave); }, transposed != 0);
    return check_launch("so3_rotate_clouds_f32");
}

int so3_pc_normalize_f32(const float *P, float *out, float *centroid, float *scale, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, 1, 150000000), "so3_pc_normalize_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(P != nullptr && out != nullptr, "so3_pc_normalize_f32: null pointer");
    const CloudShape shape = cloud_shape(B);
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the points a lane holds in registers between the two passes (N <= 64 * HOLD), or 0: the cloud is read twice
    with_value<4, 16, 0>(N <= 256 ? 4 : (N <= 1024 ? 16 : 0), [&](auto HOLD) {
        hipLaunchKernelGGL((k_pc_normalize<HOLD()>), grid, block, 0, s, P, out, centroid, scale, B, N, shape.per_wave);
    });
    return check_launch("so3_pc_normalize_f32");
}

int so3_project_fwd_f64(const double *M, double *R, uint8_t *flip, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_project_fwd_f64: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(M != nullptr && R != nullptr, "so3_project_fwd_f64: null pointer");
    hipLaunchKernelGGL((k_project_f64<false>), dim3(grid_for(B)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), M, nullptr, R, flip, B);
    return check_launch("so3_project_fwd_f64");
}

int so3_project_bwd_f64(const double *M, const double *G, double *dM, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_project_bwd_f64: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(M != nullptr && G != nullptr && dM != nullptr, "so3_project_bwd_f64: null pointer");
    hipLaunchKernelGGL((k_project_f64<true>), dim3(grid_for(B)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), M, G, dM, nullptr, B);
    return check_launch("so3_project_bwd_f64");
}

size_t so3_angle_stats_workspace_bytes(void) { return sizeof(StatWork); }

int so3_angle_stats(const double *deg, const int32_t *cls, int32_t ncls, double *stats, void *workspace, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && ncls >= 1 && ncls <= kMaxClasses, "so3_angle_stats: B / ncls (1..64)");
    SO3_CHECK_ARGS(stats != nullptr && workspace != nullptr && (B == 0 || deg != nullptr), "so3_angle_stats: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    StatWork *w = static_cast<StatWork *>(workspace);
    // (the sums, the overflow flag and the histograms of the classes in use; a memset node of this size costs two fill kernels, ~5 us each)
    // 16-byte loads of deg and 8-byte loads of cls from row 0 (mode 0) or row 1 (mode 1) on, wherever both arrays are aligned there
    auto vec_ok = [&](int64_t head) {
        return (reinterpret_cast<uintptr_t>(deg + head) & 15u) == 0 && (cls == nullptr || (reinterpret_cast<uintptr_t>(cls + head) & 7u) == 0);
    };
    const int mode = vec_ok(0) ? 0 : (vec_ok(1) ? 1 : 2);
    // one 1024-thread workgroup per CU, two rows per thread and trip (two per CU measured slower: twice the flushes and LDS histograms)
    // (SO3_STAT_GRID_MULT > 1, test builds only: more workgroups than CUs, so that the later ones START when the first ones have finished --
    // with SO3_STAT_SPINS=0 the launch-mates of every finishing workgroup then arrive after it has cleared its class)
    int64_t cap = static_cast<int64_t>(device_cus()) * SO3_STAT_GRID_MULT;
    if (cap > kStatMaxWgs) cap = kStatMaxWgs;
    const int64_t want = (B / 2 + kStatBlock - 1) / kStatBlock;
    const unsigned grid = static_cast<unsigned>(want < 1 ? 1 : (want < cap ? want : cap));
    if (ncls <= kFineClasses) {                          // few classes: bins of 1/64 octave
        k_stats_window<kFineClasses, true><<<grid, kStatBlock, 0, s>>>(deg, cls, ncls, w, B, mode);
        k_stats_collect<true><<<grid, kStatBlock, 0, s>>>(deg, cls, ncls, w, B, mode, stats);
    } else {
        if (ncls <= kStatLdsClasses) k_stats_window<kStatLdsClasses, false><<<grid, kStatBlock, 0, s>>>(deg, cls, ncls, w, B, mode);
        else k_stats_window<kMaxClasses, false><<<grid, kStatBlock, 0, s>>>(deg, cls, ncls, w, B, mode);
        k_stats_collect<false><<<grid, kStatBlock, 0, s>>>(deg, cls, ncls, w, B, mode, stats);
    }
    return check_launch("so3_angle_stats");
}

int so3_se3_update_f32(const float *out12, const float *Tinit, float *Tpred, float fx, float fy, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B && fx != 0.f && fy != 0.f, "so3_se3_update_f32: B / fx / fy");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(out12 != nullptr && Tinit != nullptr && Tpred != nullptr, "so3_se3_update_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Split sp(B, {out12, Tinit, Tpred});
    const int64_t done = sp.done, rest = sp.rest;
    if (sp.nunits > 0) { so3::OpSe3Update op; op.in0 = out12; op.in1 = Tinit; op.out0 = Tpred; op.inv_fx = 1.f / fx; op.inv_fy = 1.f / fy; launch_rows<2, 2, 256>(op, sp.nunits, s); }
    if (rest > 0) hipLaunchKernelGGL((k_se3_rows<false>), dim3(grid_for(rest)), dim3(kBlock), 0, s, out12 + done * 12, Tinit + done * 16, nullptr, Tpred + done * 16, 1.f / fx, 1.f / fy, rest);
    return check_launch("so3_se3_update_f32");
}

int so3_se3_update_bwd_f32(const float *out12, const float *Tinit, const float *G, float *dout12, float fx, float fy, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B && fx != 0.f && fy != 0.f, "so3_se3_update_bwd_f32: B / fx / fy");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(out12 != nullptr && Tinit != nullptr && G != nullptr && dout12 != nullptr, "so3_se3_update_bwd_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Split sp(B, {out12, Tinit, G, dout12});
    const int64_t done = sp.done, rest = sp.rest;
    if (sp.nunits > 0) { so3::OpSe3UpdateBwd op; op.in0 = out12; op.in1 = Tinit; op.in2 = G; op.out0 = dout12; op.inv_fx = 1.f / fx; op.inv_fy = 1.f / fy; launch_rows<1, 3, 256>(op, sp.nunits, s); }
    if (rest > 0) hipLaunchKernelGGL((k_se3_rows<true>), dim3(grid_for(rest)), dim3(kBlock), 0, s, out12 + done * 12, Tinit + done * 16, G + done * 16, dout12 + done * 12, 1.f / fx, 1.f / fy, rest);
    return check_launch("so3_se3_update_bwd_f32");
}

int so3_rotations_axis_angle_f32(const float *theta, const float *axis, float *R, int64_t B, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, "so3_rotations_axis_angle_f32: B");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(theta != nullptr && axis != nullptr && R != nullptr, "so3_rotations_axis_angle_f32: null pointer");
    hipLaunchKernelGGL(k_rotations_axis_angle, dim3(grid_for(B)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), theta, axis, R, B);
    return check_launch("so3_rotations_axis_angle_f32");
}

int so3_kabsch_synth_f32(const float *P, const float *Rgt, float sigma, uint32_t seed, float *R, float *H, int64_t B, int32_t N,
                         void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 31) && N >= 0 && N <= 150000000, "so3_kabsch_synth_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R != nullptr && Rgt != nullptr && (N == 0 || P != nullptr), "so3_kabsch_synth_f32: null pointer");
    const CloudShape shape = cloud_shape(B);
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_flags([&](auto NOISE) {
        if (N <= kSynthFew)      // a few points a cloud: q rounded once (k_kabsch_synth_few)
            hipLaunchKernelGGL((k_kabsch_synth_few<NOISE()>), grid, block, 0, s, P, Rgt, sigma, seed, R, H, B, N, shape.per_wave);
        else
            hipLaunchKernelGGL((k_kabsch_synth<NOISE()>), grid, block, 0, s, P, Rgt, sigma, seed, R, H, B, N, shape.per_wave);
    }, sigma != 0.f);
    return check_launch("so3_kabsch_synth_f32");
}

int so3_kabsch_f32(const float *P, const float *Q, float *R, float *H, int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 40) && N >= 0 && N <= 150000000, "so3_kabsch_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R != nullptr && (N == 0 || (P != nullptr && Q != nullptr)), "so3_kabsch_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CloudShape shape = cloud_shape(B);
    SO3_CHECK_ARGS(shape.blocks <= 2147483647, "so3_kabsch_f32: B too large");
    hipLaunchKernelGGL(k_kabsch, dim3(static_cast<unsigned>(shape.blocks)), dim3(kBlock), 0, s, P, Q, R, H, B, N, shape.per_wave);
    return check_launch("so3_kabsch_f32");
}

int so3_kabsch_bwd_f32(const float *P, const float *Q, const float *H, const float *gR, const float *gH, float *dP, float *dQ,
                       int64_t B, int32_t N, void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 40) && N >= 0 && N <= 150000000, "so3_kabsch_bwd_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(H != nullptr && (N == 0 || (P != nullptr && Q != nullptr)), "so3_kabsch_bwd_f32: null pointer");
    if (N == 0 || (dP == nullptr && dQ == nullptr)) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CloudShape shape = cloud_shape(B);
    SO3_CHECK_ARGS(shape.blocks <= 2147483647, "so3_kabsch_bwd_f32: B too large");
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    with_flags([&](auto DP, auto DQ) {
        if constexpr (DP() || DQ())                              // (no gradient asked for: returned above)
            hipLaunchKernelGGL((k_kabsch_bwd<DP(), DQ()>), grid, block, 0, s, P, Q, H, gR, gH, dP, dQ, B, N, shape.per_wave);
    }, dP != nullptr, dQ != nullptr);
    return check_launch("so3_kabsch_bwd_f32");
}

int so3_rigid_align_f32(const float *P, const float *Q, const float *w, float *R, float *t, float *H, float *stats, int64_t B, int32_t N,
                        void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 40) && N >= 0 && N <= 150000000, "so3_rigid_align_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(R != nullptr && t != nullptr && (N == 0 || (P != nullptr && Q != nullptr)), "so3_rigid_align_f32: null pointer");
    const CloudShape shape = cloud_shape(B);
    SO3_CHECK_ARGS(shape.blocks <= 2147483647, "so3_rigid_align_f32: B too large");
    with_flags([&](auto WEIGHTED) {
        hipLaunchKernelGGL((k_rigid_align<WEIGHTED()>), dim3(static_cast<unsigned>(shape.blocks)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                           P, Q, w, R, t, H, stats, B, N, shape.per_wave);
    }, w != nullptr);
    return check_launch("so3_rigid_align_f32");
}

int so3_rigid_align_bwd_f32(const float *P, const float *Q, const float *w, const float *H, const float *R, const float *stats,
                            const float *gR, const float *gt, const float *gH, float *dP, float *dQ, float *dw, int64_t B, int32_t N,
                            void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 40) && N >= 0 && N <= 150000000, "so3_rigid_align_bwd_f32: B/N");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(H != nullptr && R != nullptr && stats != nullptr && (N == 0 || (P != nullptr && Q != nullptr)),
                   "so3_rigid_align_bwd_f32: null pointer");
    if (N == 0 || (dP == nullptr && dQ == nullptr && dw == nullptr)) return 0;
    const CloudShape shape = cloud_shape(B);
    SO3_CHECK_ARGS(shape.blocks <= 2147483647, "so3_rigid_align_bwd_f32: B too large");
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_flags([&](auto DP, auto DQ, auto DW) {
        if constexpr (DP() || DQ() || DW())                      // (no gradient asked for: returned above)
            hipLaunchKernelGGL((k_rigid_align_bwd<DP(), DQ(), DW()>), grid, block, 0, s, P, Q, w, H, R, stats, gR, gt, gH, dP, dQ, dw, B, N,
                               shape.per_wave);
    }, dP != nullptr, dQ != nullptr, dw != nullptr);
    return check_launch("so3_rigid_align_bwd_f32");
}

int so3_rotate_clouds_bwd_f32(const float *P, const float *R, const float *G, float *dP, float *dR, int transposed, int64_t B, int32_t N,
                              void *stream) {
    SO3_CHECK_ARGS(B >= 0 && B <= (INT64_C(1) << 31) && N >= 0 && N <= 150000000, "so3_rotate_clouds_bwd_f32: B/N");
    if (B == 0) return 0;
    if (N == 0) dP = nullptr;                                      // (N == 0: dR = 0 is the only output)
    SO3_CHECK_ARGS((dP == nullptr || R != nullptr) && (N == 0 || (G != nullptr && (dR == nullptr || P != nullptr))),
                   "so3_rotate_clouds_bwd_f32: null pointer");                 // R for dP, P for dR, G for either
    if (dR == nullptr && dP == nullptr) return 0;
    const CloudShape shape = cloud_shape(B);
    const dim3 grid(static_cast<unsigned>(shape.blocks)), block(kBlock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_flags([&](auto T, auto WP, auto WR) {
        if constexpr (WP() || WR())                              // (no gradient asked for: returned above)
            hipLaunchKernelGGL((k_rotate_clouds_bwd<T(), WP(), WR()>), grid, block, 0, s, P, R, G, dP, dR, B, N, shape.per_wave);
    }, transposed != 0, dP != nullptr, dR != nullptr);
    return check_launch("so3_rotate_clouds_bwd_f32");
}

// ---- K4s / K3s: the metric and the loss up to a symmetry group ------------------------------------------------------------------
// Arguments both entries share.  `ENTRY` names the entry in so3_last_error().
#define SO3_SYM_CHECK(ENTRY) do { \
        SO3_CHECK_ARGS(B >= 0 && B <= SO3_MAX_B, ENTRY ": B"); \
        SO3_CHECK_ARGS(K >= 1 && K <= 64, ENTRY ": K must be in [1, 64]"); \
        SO3_CHECK_ARGS(num_classes >= 1, ENTRY ": num_classes must be >= 1"); \
        SO3_CHECK_ARGS(static_cast<int64_t>(num_classes) * K <= 256, ENTRY ": num_classes * K must be <= 256"); \
        SO3_CHECK_ARGS((class_id != nullptr) == (num_classes > 1), ENTRY ": class_id must be given exactly when num_classes > 1"); \
        SO3_CHECK_ARGS(S != nullptr, ENTRY ": S is null"); \
    } while (0)

}  // extern "C"

template <bool MULTI>
static void sym_angle_launch(so3::OpSymAngle<MULTI> op, int64_t B, hipStream_t s) {
    const Split sp(B, {op.in0, op.in1, op.in2, op.deg, op.index});
    const int64_t done = sp.done, rest = sp.rest;
    if (sp.nunits > 0) launch_rows<1, 4, 1024>(op, sp.nunits, s);
    if (rest > 0) {
        so3::OpSymAngle<MULTI> t = op;
        t.in0 = static_cast<const float *>(op.in0) + done * 9;
        t.in1 = static_cast<const float *>(op.in1) + done * 9;
        if (MULTI) t.in2 = static_cast<const int32_t *>(op.in2) + done;
        t.deg = op.deg + done;
        t.index = advance(op.index, done);
        hipLaunchKernelGGL((k_sym_rows<so3::OpSymAngle<MULTI>>), dim3(persistent_grid(rest)), dim3(kBlock), 0, s, t, rest, 0, nullptr);
    }
}

extern "C" {

int so3_sym_angle_error_f32(const float *Rpred, const float *Rtrue, const float *S, const int32_t *class_id, int32_t num_classes, int32_t K,
                            double *deg, int32_t *index, int32_t *flags_out, unsigned flags, int64_t B, void *stream) {
    SO3_CHECK_ARGS((flags & ~static_cast<unsigned>(SO3_RADIANS)) == 0, "so3_sym_angle_error_f32: unknown flag");
    SO3_SYM_CHECK("so3_sym_angle_error_f32");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(Rpred != nullptr && Rtrue != nullptr && deg != nullptr, "so3_sym_angle_error_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags_out != nullptr) if (int e = zero_async(flags_out, sizeof(int32_t), s, "so3_sym_angle_error_f32: memset")) return e;
    with_flags([&](auto MULTI) {
        so3::OpSymAngle<MULTI()> op; op.in0 = Rpred; op.in1 = Rtrue; op.in2 = class_id; op.sym.table = S; op.sym.K = K;
        op.sym.C = num_classes; op.deg = deg; op.index = index; op.flags_out = flags_out;
        op.unit_scale = (flags & SO3_RADIANS) ? 1.0 : kDegPerRad;
        sym_angle_launch<MULTI()>(op, B, s);
    }, num_classes > 1);
    return check_launch("so3_sym_angle_error_f32");
}

}  // extern "C"

template <bool MULTI, bool DP, bool DT>
static int sym_loss_launch(so3::OpSymFrobLoss<MULTI, DP, DT> op, int64_t B, void *workspace, hipStream_t s) {
    typedef so3::OpSymFrobLoss<MULTI, DP, DT> Op;
    if (B <= kSmallBatch) {                              // one workgroup, one launch: the kernel writes loss_sum and the mean itself
        hipLaunchKernelGGL((k_sym_rows<Op>), dim3(1), dim3(static_cast<unsigned>((B + 63) / 64 * 64)), 0, s, op, B, 1, nullptr);
        return 0;
    }
    const Split sp(B, {op.in0, op.in1, op.in2, op.out0, op.out1, op.index});
    const int64_t nunits = sp.nunits, done = sp.done, rest = sp.rest;
    const unsigned tile_wgs = rest > 0 ? persistent_grid(rest) : 0u;
    so3::ReduceWs *ws = reduce_workspace(workspace, sp, tile_wgs);
    if (ws == nullptr) if (int e = zero_async(op.loss_sum, sizeof(double), s, "so3_sym_frob_loss_f32: memset")) return e;
    if (rest > 0) {
        Op t = op;
        t.in0 = static_cast<const float *>(op.in0) + done * 9;
        t.in1 = static_cast<const float *>(op.in1) + done * 9;
        if (MULTI) t.in2 = static_cast<const int32_t *>(op.in2) + done;
        t.out0 = advance(static_cast<float *>(op.out0), done * 9);
        t.out1 = advance(static_cast<float *>(op.out1), done * 9);
        t.index = advance(op.index, done);
        hipLaunchKernelGGL((k_sym_rows<Op>), dim3(tile_wgs), dim3(kBlock), 0, s, t, rest, ws != nullptr ? 2 : 3, ws);
    }
    if (nunits > 0) {
        op.ws = ws;
        op.ws_slot0 = tile_wgs;
        launch_rows<1, 4, 1024>(op, nunits, s);
    }
    if (ws == nullptr && op.loss_mean != nullptr) k_mean_from_sum<<<1, 1, 0, s>>>(op.loss_sum, op.loss_mean, op.inv_b_f64);
    return 0;
}

extern "C" {

int so3_sym_frob_loss_f32(const float *Rpred, const float *Rtrue, const float *S, const int32_t *class_id, int32_t num_classes, int32_t K,
                          float *dRpred, float *dRtrue, int32_t *index, double *loss_sum, float *loss_mean, void *workspace, unsigned flags,
                          int64_t B, void *stream) {
    SO3_CHECK_ARGS(flags == 0, "so3_sym_frob_loss_f32: unknown flag (none is defined for it)");
    SO3_SYM_CHECK("so3_sym_frob_loss_f32");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(Rpred != nullptr && Rtrue != nullptr && loss_sum != nullptr, "so3_sym_frob_loss_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int err = 0;
    with_flags([&](auto MULTI, auto DP, auto DT) {
        so3::OpSymFrobLoss<MULTI(), DP(), DT()> op; op.in0 = Rpred; op.in1 = Rtrue; op.in2 = class_id; op.out0 = dRpred;
        op.out1 = dRtrue; op.sym.table = S; op.sym.K = K; op.sym.C = num_classes; op.index = index;
        op.loss_sum = loss_sum; op.loss_mean = loss_mean; op.inv_b = 1.0f / static_cast<float>(B);
        op.inv_b_f64 = 1.0 / static_cast<double>(B);
        err = sym_loss_launch(op, B, workspace, s);
    }, num_classes > 1, dRpred != nullptr, dRtrue != nullptr);
    if (err != 0) return err;                           // (the memset's: so3_last_error() is set)
    return check_launch("so3_sym_frob_loss_f32");
}

int so3_sym_add_f32(const float *Tgt, const float *Tpred, const float *points, const float *S, const int32_t *class_id, int32_t num_classes,
                    int32_t K, float *dists, int32_t *index, double *loss_sum, float *dTpred, float grad_scale, unsigned flags, int64_t B,
                    int32_t N, void *stream) {
    SO3_CHECK_ARGS(flags <= static_cast<unsigned>(SO3_SYM_ADD_MAX), "so3_sym_add_f32: unknown flag (the mode: SO3_SYM_ADD_L2, _L1 or _MAX)");
    SO3_CHECK_ARGS(cloud_dims_ok(B, N, 1, 150000000), "so3_sym_add_f32: B/N");
    SO3_SYM_CHECK("so3_sym_add_f32");
    SO3_CHECK_ARGS(flags != static_cast<unsigned>(SO3_SYM_ADD_MAX) || dTpred == nullptr, "so3_sym_add_f32: dTpred must be null with SO3_SYM_ADD_MAX (no gradient)");
    if (B == 0) return 0;
    SO3_CHECK_ARGS(Tgt != nullptr && Tpred != nullptr && points != nullptr, "so3_sym_add_f32: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    static_assert(SO3_SYM_ADD_L2 == so3::kSymAddL2 && SO3_SYM_ADD_L1 == so3::kSymAddL1 && SO3_SYM_ADD_MAX == so3::kSymAddMax, "the flag is the mode");
    with_value<so3::kSymAddL2, so3::kSymAddL1, so3::kSymAddMax>(static_cast<int>(flags), [&](auto MODE) {
        constexpr int kMode = MODE();
        with_flags([&](auto GRAD) {
            if constexpr (kMode != so3::kSymAddMax || !GRAD())   // (the maximum has no gradient: refused above)
                launch_sym_add<kMode, GRAD()>(Tgt, Tpred, points, S, class_id, num_classes, K, dists, index, loss_sum, dTpred, grad_scale, B, N, s);
        }, dTpred != nullptr);
    });
    return check_launch("so3_sym_add_f32");
}
#undef SO3_SYM_CHECK

}  // extern "C"

