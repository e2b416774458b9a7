// nearest_sanitize.cpp -- a stand-alone host program for the sanitizers: the host twin of nearest_kernel (packed_nearest;
// csrc/packed_host.cpp) on generated matrices, with and without an allow-mask, for every list length and for counts around it, checked
// against a stable sort of packed_score_rows' scores; and packed_assign, which calls it, with and without `best`. No GPU, no Python. Build and run once on the CPU (from the repository's root):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o /tmp/nearest_sanitize \
//       tools/nearest_sanitize.cpp approximate-spmv-topk_amd/csrc/{packed_host,wbscsr,host_utils,options}.cpp -pthread && /tmp/nearest_sanitize
// Exit status 0 and "nearest_sanitize: ok" when the twin equals the sorted scores and no sanitizer spoke.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "../approximate-spmv-topk_amd/csrc/host_utils.hpp"
#include "../approximate-spmv-topk_amd/csrc/packed_host.hpp"
#include "../approximate-spmv-topk_amd/csrc/wbscsr.hpp"
#include "../include/tkspmv.h"

using namespace tkspmv;

static int fail(const char *what) {
    std::fprintf(stderr, "nearest_sanitize: FAILED: %s\n", what);
    return 1;
}

static int one_matrix(uint32_t rows, uint32_t cols, uint32_t C, uint32_t hint, uint64_t &mix) {
    CooMatrix m;
    generate_matrix(rows, cols, 20, DIST_GAMMA, 7 + cols, m);
    // signed values; every 11th row loses its entries (rows without entries, the last rows among them)
    size_t keep = 0;
    for (size_t i = 0; i < m.val.size(); ++i) {
        if (m.row[i] % 11u == 10u) continue;
        m.row[keep] = m.row[i];
        m.col[keep] = m.col[i];
        m.val[keep] = (i & 1u) ? -m.val[i] : m.val[i];
        ++keep;
    }
    m.row.resize(keep), m.col.resize(keep), m.val.resize(keep);
    PackedMatrix pm;
    int kind = 0;
    const std::string e = pack_wbscsr(rows, cols, m.nnz(), m.row.data(), m.col.data(), m.val.data(), Precision::F32, C, hint, 1u, pm, kind);
    if (!e.empty()) return fail(e.c_str());
    const int32_t max_count = 20;
    std::vector<float> xs((size_t)max_count * cols);
    uint32_t state = 12345u + cols;
    for (float &x : xs) {
        state = state * 1664525u + 1013904223u;
        x = (float)(int32_t)(state >> 8 & 0xFFFFu) / 32768.0f - 1.0f;
    }
    for (uint32_t c = 0; c < cols; ++c) xs[(size_t)7 * cols + c] = xs[(size_t)2 * cols + c];  // a duplicate: ties by index
    std::vector<uint32_t> ids(rows), mask((rows + 31u) / 32u + 1u, 0u);
    std::iota(ids.begin(), ids.end(), 0u);
    for (uint32_t r = 0; r < rows; ++r)
        if ((r * 2654435761u >> 9) & 1u) mask[r >> 5] |= 1u << (r & 31u);
    std::string err;
    std::vector<float> y((size_t)max_count * rows);
    for (int32_t q = 0; q < max_count; ++q)
        if (packed_score_rows(pm, xs.data() + (size_t)q * cols, ids.data(), (int32_t)rows, y.data() + (size_t)q * rows, err) != TKSPMV_OK) return fail(err.c_str());
    const float none = -std::numeric_limits<float>::infinity();
    for (const int32_t count : {1, 2, 3, 4, 5, 20})
        for (int32_t n = 1; n <= TKSPMV_NEAREST_MAX_N; ++n)
            for (const bool masked : {false, true}) {
                // exactly rows * n words each: guard words behind the outputs
                std::vector<uint32_t> labels((size_t)rows * n + 1u, 0xAAAAAAAAu);
                std::vector<float> scores((size_t)rows * n + 1u, -7.0f);
                if (packed_nearest(pm, xs.data(), count, n, masked ? mask.data() : nullptr, labels.data(), scores.data(), err) != TKSPMV_OK) return fail(err.c_str());
                if (labels.back() != 0xAAAAAAAAu || scores.back() != -7.0f) return fail("the twin wrote behind its outputs");
                std::vector<int32_t> order(count);
                for (uint32_t r = 0; r < rows; ++r) {
                    const bool in = !masked || ((mask[r >> 5] >> (r & 31u)) & 1u) != 0u;
                    std::iota(order.begin(), order.end(), 0);
                    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return y[(size_t)a * rows + r] > y[(size_t)b * rows + r]; });
                    for (int32_t j = 0; j < n; ++j) {
                        const bool have = in && j < count;
                        const uint32_t want_l = have ? (uint32_t)order[j] : TKSPMV_NEAREST_NONE;
                        const float want_s = have ? y[(size_t)order[j] * rows + r] : none;
                        if (labels[(size_t)r * n + j] != want_l || std::memcmp(&scores[(size_t)r * n + j], &want_s, 4) != 0)
                            return fail("the twin's lists differ from the stable sort of packed_score_rows' scores");
                        mix += want_l;
                    }
                }
            }
    // packed_assign is packed_nearest's lists of one entry: with best given and with best = NULL (the scores then go to an array of
    // the call), exactly rows words each, equal to the first of the sorted scores
    for (const int32_t count : {1, 5, 20})
        for (const bool with_best : {true, false}) {
            std::vector<uint32_t> labels((size_t)rows + 1u, 0xAAAAAAAAu);
            std::vector<float> best((size_t)rows + 1u, -7.0f);
            if (packed_assign(pm, xs.data(), count, labels.data(), with_best ? best.data() : nullptr, err) != TKSPMV_OK) return fail(err.c_str());
            if (labels.back() != 0xAAAAAAAAu || best.back() != -7.0f) return fail("packed_assign wrote behind its outputs");
            for (uint32_t r = 0; r < rows; ++r) {
                int32_t first = 0;
                for (int32_t q = 1; q < count; ++q)
                    if (y[(size_t)q * rows + r] > y[(size_t)first * rows + r]) first = q;
                const float want_s = with_best ? y[(size_t)first * rows + r] : -7.0f;
                if (labels[r] != (uint32_t)first || std::memcmp(&best[r], &want_s, 4) != 0) return fail("packed_assign differs from the first of packed_score_rows' scores");
                mix += labels[r];
            }
        }
    return 0;
}

int main() {
    uint64_t mix = 0;
    if (one_matrix(2500, 300, 4, 7, mix)) return 1;
    if (one_matrix(2500, 1024, 8, 64, mix)) return 1;
    if (one_matrix(600, 5000, 4, 7, mix)) return 1;
    if (one_matrix(40, 64, 4, 1, mix)) return 1;
    std::printf("nearest_sanitize: ok (%llx)\n", (unsigned long long)mix);
    return 0;
}
