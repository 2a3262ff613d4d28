// wave_model.h -- what the host models share of a wave's and a work item's order of operations.  Included after so3_device.h
// (SO3_HOST_MODEL).  TEST INFRASTRUCTURE ONLY.
#pragma once

namespace {

// the xor butterfly over a wave's 64 lanes, as the device's wave_allsum: its DPP mirrors add the same partners' sums
[[maybe_unused]] float wave_allsum(const float (&lane)[64]) {
    float v[64], w[64];
    for (int l = 0; l < 64; ++l) v[l] = lane[l];
    for (int off = 1; off < 64; off <<= 1) {
        for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; ++l) v[l] = w[l];
    }
    return v[0];
}

// one entry of a work item's record: thread tid = lane tid % 64 of wave tid / 64, each wave's butterfly, the four waves in wave order
[[maybe_unused]] float item_sum(const float (&mine)[so3::kIcpBlock]) {
    float v = 0.f;
    for (int wv = 0; wv < so3::kIcpBlock / 64; ++wv) {
        float lane[64];
        for (int l = 0; l < 64; ++l) lane[l] = mine[wv * 64 + l];
        const float tot = wave_allsum(lane);
        v = wv == 0 ? tot : v + tot;
    }
    return v;
}

// One direction of one cloud in the Chamfer forwards (the device's chamfer_search): the points src[0 .. len_p) search tgt[0 .. len_q);
// NORMALS pairs their normals own[i], other[j(i)] as well.  sums[0], sums[1] = the float64 sums of the records (distance, normal term).
template <bool SQUARED, bool NORMALS>
[[maybe_unused]] void chamfer_direction(const float *src, const float *tgt, const float *own, const float *other, int32_t full, int32_t len_p,
                                        int32_t len_q, float *dist, int32_t *nearest, float *term, bool signed_cos, int u, double (&sums)[2]) {
    const int per = so3::kIcpBlock * u, chunks = (full + per - 1) / per;
    sums[0] = sums[1] = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const int i_base = c * per;
        const bool live = len_q > 0 && i_base < len_p;
        float mine[so3::kIcpBlock], mine_n[so3::kIcpBlock];
        for (int t = 0; t < so3::kIcpBlock; ++t) mine[t] = mine_n[t] = 0.f;
        for (int uu = 0; uu < u; ++uu) {
            for (int t = 0; t < so3::kIcpBlock; ++t) {
                const int i = i_base + uu * so3::kIcpBlock + t;
                const bool valid = live && i < len_p;
                float best = 0.f, tn = 0.f;
                int idx = 0;
                if (valid) {
                    best = std::numeric_limits<float>::infinity();
                    for (int j = 0; j < len_q; ++j)
                        so3::add_s_pair<true, false>(src[i * 3], src[i * 3 + 1], src[i * 3 + 2], tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], j, best, idx);
                    if (NORMALS) {
                        const int j = std::min(std::max(idx, 0), len_q - 1);
                        tn = so3::chamfer_normal_term(own[i * 3], own[i * 3 + 1], own[i * 3 + 2], other[j * 3], other[j * 3 + 1], other[j * 3 + 2],
                                                      signed_cos);
                    }
                }
                const float e = valid ? so3::chamfer_term<SQUARED>(best) : 0.f;
                mine[t] += e;
                mine_n[t] += tn;
                if (i < full) {
                    if (dist != nullptr) dist[i] = e;
                    if (nearest != nullptr) nearest[i] = valid ? std::min(idx, len_q - 1) : -1;
                    if (NORMALS && term != nullptr) term[i] = tn;
                }
            }
        }
        sums[0] += static_cast<double>(item_sum(mine));
        if (NORMALS) sums[1] += static_cast<double>(item_sum(mine_n));
    }
}

}  // namespace
