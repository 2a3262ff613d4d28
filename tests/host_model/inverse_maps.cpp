// inverse_maps.cpp -- the inverse-map operations of poseestimation_amd/csrc/so3_rows.h (OpMatToQuat, OpLogMap, OpMatToEuler, OpRelLog)
// and Tr<T>::atan2 compiled for the host (SO3_HOST_MODEL), so that tests/test_inverse_maps_host.py runs the kernels' own templates
// without a GPU.  TEST INFRASTRUCTURE ONLY.  Differences from the device: libm's correctly rounded sqrt / division stand in for
// v_rsq_f32 / v_sqrt_f32 / v_rcp_f32 (1 ulp), and the build does not contract a * b + c.  Needs clang++ (ext_vector_type).
#define SO3_HOST_MODEL 1
#include <stdint.h>

#include "../../poseestimation_amd/csrc/so3_rows.h"

namespace {

// One operation over B rows; PACKED: two rows per "lane" (T = f32x2, what the streaming engine instantiates), an odd last row is
// paired with itself.  Absent arrays are null.
template <class Op, bool PACKED>
void run(Op op, const float *in0, const float *in1, const float *in2, float *out0, float *out1, int64_t B) {
    typedef typename so3::LaneT<PACKED ? 2 : 1>::type T;
    typedef so3::Tr<T> R;
    constexpr int L = PACKED ? 2 : 1;
    for (int64_t b = 0; b < B; b += L) {
        so3::Rows<T, Op> rows;
        so3::RowCtx<L> ctx{};
        for (int k = 0; k < L; ++k) {
            const int64_t row = b + k < B ? b + k : b;
            for (int i = 0; i < Op::kIn0N; ++i) R::set(rows.a[i], k, in0[row * Op::kIn0N + i]);
            if (Op::kIn1 != 0) for (int i = 0; i < Op::kIn1N; ++i) R::set(rows.b[i], k, in1[row * Op::kIn1N + i]);
            if (Op::kIn2 != 0) for (int i = 0; i < Op::kIn2N; ++i) R::set(rows.c[i], k, in2[row * Op::kIn2N + i]);
        }
        op.template compute<T, L>(rows, ctx);
        for (int k = 0; k < L; ++k) {
            const int64_t row = b + k < B ? b + k : b;
            for (int i = 0; i < Op::kOut0N; ++i) out0[row * Op::kOut0N + i] = R::get(rows.o0[i], k);
            if (Op::kOut1 != 0) for (int i = 0; i < Op::kOut1N; ++i) out1[row * Op::kOut1N + i] = R::get(rows.o1[i], k);
        }
    }
}

template <class Op>
void run_either(Op op, int packed, const float *in0, const float *in1, const float *in2, float *out0, float *out1, int64_t B) {
    if (packed) run<Op, true>(op, in0, in1, in2, out0, out1, B);
    else run<Op, false>(op, in0, in1, in2, out0, out1, B);
}

}  // namespace

extern "C" {

#define INVERSE(NAME, OP)                                                                                         \
    void model_##NAME##_fwd(const float *R, float *Y, int64_t B, int packed) {                                    \
        run_either(so3::OP<false>(), packed, R, nullptr, nullptr, Y, nullptr, B);                                 \
    }                                                                                                             \
    void model_##NAME##_bwd(const float *R, const float *G, float *dR, int64_t B, int packed) {                   \
        run_either(so3::OP<true>(), packed, R, G, nullptr, dR, nullptr, B);                                       \
    }
INVERSE(mat_to_quat, OpMatToQuat)
INVERSE(logmap, OpLogMap)
INVERSE(mat_to_euler, OpMatToEuler)
#undef INVERSE

void model_relative_log_fwd(const float *R1, const float *R2, float *V, int64_t B, int packed) {
    run_either(so3::OpRelLog<false, false>(), packed, R1, R2, nullptr, V, nullptr, B);
}

// as so3_relative_log_bwd_f32: either output may be null; one alone runs the swapped pair under -g
void model_relative_log_bwd(const float *R1, const float *R2, const float *G, float *dR1, float *dR2, int64_t B, int packed) {
    if (dR1 != nullptr && dR2 != nullptr) {
        run_either(so3::OpRelLog<true, true>(), packed, R1, R2, G, dR2, dR1, B);
    } else if (dR2 != nullptr) {
        run_either(so3::OpRelLog<true, false>(), packed, R1, R2, G, dR2, nullptr, B);
    } else {
        so3::OpRelLog<true, false> op;
        op.gsign = -1.f;
        run_either(op, packed, R2, R1, G, dR1, nullptr, B);
    }
}

void model_atan2(const float *y, const float *x, float *out, int64_t n, int packed) {
    if (packed) {
        for (int64_t i = 0; i + 1 < n; i += 2) {
            const so3::f32x2 a = so3::Tr<so3::f32x2>::atan2(so3::f32x2{y[i], y[i + 1]}, so3::f32x2{x[i], x[i + 1]});
            out[i] = a.x;
            out[i + 1] = a.y;
        }
        if (n % 2) out[n - 1] = so3::Tr<float>::atan2(y[n - 1], x[n - 1]);
    } else {
        for (int64_t i = 0; i < n; ++i) out[i] = so3::Tr<float>::atan2(y[i], x[i]);
    }
}

// max_i |atan2 - atan2l| / max(|atan2l|, tiny) and the largest absolute error over a sweep of n points on `rings` circles of radii
// 2^-20 .. 2^20 (angles uniform in (-pi, pi], the axes and the diagonals included), against long double
void model_atan2_sweep(int64_t n, int rings, double *max_rel, double *max_abs) {
    double worst_rel = 0.0, worst_abs = 0.0;
    const long double pi = 3.14159265358979323846264338327950288L;
    const int64_t per = n / rings;
    for (int r = 0; r < rings; ++r) {
        const float radius = std::ldexp(1.0f, -20 + (40 * r) / (rings > 1 ? rings - 1 : 1));
        for (int64_t i = 0; i < per; ++i) {
            const long double ang = -pi + 2 * pi * (static_cast<long double>(i) + 1) / per;
            const float y = radius * static_cast<float>(std::sin(ang)), x = radius * static_cast<float>(std::cos(ang));
            const long double want = std::atan2(static_cast<long double>(y), static_cast<long double>(x));
            const double err = static_cast<double>(std::fabs(static_cast<long double>(so3::Tr<float>::atan2(y, x)) - want));
            // (y = -0 next to the cut: the sign of zero decides between +pi and -pi; both are the same angle)
            const double e = err > 6.0 ? std::fabs(err - static_cast<double>(2 * pi)) : err;
            if (e > worst_abs) worst_abs = e;
            const double rel = e / static_cast<double>(std::fabs(want) > 1e-30L ? std::fabs(want) : 1e-30L);
            if (std::fabs(want) > 0 && rel > worst_rel) worst_rel = rel;
        }
    }
    *max_rel = worst_rel;
    *max_abs = worst_abs;
}

}  // extern "C"
