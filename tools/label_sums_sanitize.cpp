// label_sums_sanitize.cpp -- a stand-alone host program for the sanitizers: the host twin of label_sums_kernel (packed_label_sums,
// packed_sums_exponent, sums_close_host; csrc/packed_host.cpp) and quantise (csrc/quantise.hpp) on generated matrices, checked
// against a direct sum over the COO. No GPU, no Python. Build and run once on the CPU (from the repository's root):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o /tmp/label_sums_sanitize \
//       tools/label_sums_sanitize.cpp approximate-spmv-topk_amd/csrc/{packed_host,wbscsr,host_utils,options}.cpp -pthread && /tmp/label_sums_sanitize
// Exit status 0 and "label_sums_sanitize: ok" when the twin equals the direct sums and no sanitizer spoke.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../approximate-spmv-topk_amd/csrc/host_utils.hpp"
#include "../approximate-spmv-topk_amd/csrc/packed_host.hpp"
#include "../approximate-spmv-topk_amd/csrc/quantise.hpp"
#include "../approximate-spmv-topk_amd/csrc/wbscsr.hpp"
#include "../include/tkspmv.h"

using namespace tkspmv;

static int fail(const char *what) {
    std::fprintf(stderr, "label_sums_sanitize: FAILED: %s\n", what);
    return 1;
}

static int one_matrix(uint32_t rows, uint32_t cols, uint32_t C, uint32_t hint, uint32_t n_bins) {
    CooMatrix m;
    generate_matrix(rows, cols, 20, DIST_GAMMA, 7 + cols, m);
    for (size_t i = 0; i < m.val.size(); ++i) m.val[i] = std::ldexp((i & 1u) ? -m.val[i] : m.val[i], -(int)(i % 21u));
    PackedMatrix pm;
    int kind = 0;
    const std::string e = pack_wbscsr(rows, cols, m.nnz(), m.row.data(), m.col.data(), m.val.data(), Precision::F32, C, hint, 1u, pm, kind);
    if (!e.empty()) return fail(e.c_str());
    std::vector<uint32_t> labels(rows);
    for (uint32_t r = 0; r < rows; ++r) labels[r] = (r * 2654435761u >> 7) % (n_bins + 2u);  // some rows have no bin
    std::string err;
    int32_t E = 0;
    if (packed_sums_exponent(pm, &E, err) != TKSPMV_OK) return fail(err.c_str());
    for (const int32_t exp : {E, -12, -3, 200, -2000000000, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
        std::vector<int64_t> sums((size_t)n_bins * cols, -7), want((size_t)n_bins * cols, 0);
        std::vector<float> out((size_t)n_bins * cols, -7.0f);
        for (const int32_t mode : {TKSPMV_SUMS_RAW, TKSPMV_SUMS_FLOAT, TKSPMV_SUMS_UNIT})
            if (packed_label_sums(pm, labels.data(), n_bins, exp, mode, sums.data(), mode == TKSPMV_SUMS_RAW ? nullptr : out.data(), err) != TKSPMV_OK)
                return fail(err.c_str());
        if (exp < -100) continue;  // (shifts beyond 38: unspecified words; the calls above only had to stay defined behaviour)
        for (size_t i = 0; i < m.val.size(); ++i) {
            uint32_t bits;
            std::memcpy(&bits, &m.val[i], 4);
            if (labels[m.row[i]] < n_bins)
                want[(size_t)labels[m.row[i]] * cols + m.col[i]] = (int64_t)((uint64_t)want[(size_t)labels[m.row[i]] * cols + m.col[i]] + (uint64_t)quantise(bits, exp));
        }
        if (sums != want) return fail("the twin's sums differ from the direct sums over the COO");
    }
    return 0;
}

int main() {
    // quantise at its edges: every exponent field, both signs, exponents at and beyond the int32 range's ends
    uint64_t mix = 0;
    for (uint32_t e = 0; e < 256u; ++e)
        for (const uint32_t frac : {0u, 1u, 0x400000u, 0x7FFFFFu})
            for (const int32_t E : {0, -149, -190, 104, 168, 1000, -1000, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
                const uint32_t bits = e << 23 | frac;
                const int64_t q = quantise(bits, E);
                if (quantise(bits | 0x80000000u, E) != (int64_t)(0ull - (uint64_t)q)) return fail("quantise(-v) != -quantise(v)");
                mix += (uint64_t)q;
            }
    if (one_matrix(2500, 300, 4, 7, 9)) return 1;
    if (one_matrix(2500, 1024, 8, 64, 17)) return 1;
    if (one_matrix(600, 5000, 4, 7, 3)) return 1;
    if (one_matrix(40, 64, 4, 1, 1)) return 1;
    std::printf("label_sums_sanitize: ok (%llx)\n", (unsigned long long)mix);
    return 0;
}
