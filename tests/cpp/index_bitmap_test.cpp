// index_bitmap_test.cpp -- Index::SearchBitmap / SearchBatchBitmap of the C++ host mirror (include/longbow_gpu.hpp): a search under
// a row bitmap given with the call ("call bitmap" in include/longbow_gpu.h).  Argument validation needs no device; with one, a
// bitmap search is compared with the CPU oracle (oracle/longbow_oracle.h) under the unpacked bits, bit for bit.
//
// exit code 0 = all passed, 77 = skipped (no GPU: NewIndexWithConfig returned ErrGPUNotAvailable), anything else = failure.
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "longbow_gpu.hpp"
extern "C" {
#include "longbow_oracle.h"
}

using longbow::gpu::GPUConfig;
using longbow::gpu::Index;
using longbow::gpu::NewIndexWithConfig;

static int failures = 0;
#define REQUIRE(cond, ...)                                                      \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                  \
            std::fprintf(stderr, "\n");                                         \
            failures++;                                                         \
            return;                                                             \
        }                                                                       \
    } while (0)

// the C entry points refuse a NULL handle before a device is touched, with nothing written
static void TestIndexBitmap_NullHandle()
{
    std::vector<float> q(8, 0.5f), dist(3, -3.0f);
    std::vector<int64_t> lab(3, -9);
    const uint8_t bits[2] = {0xA5, 0xA5};
    REQUIRE(lb_gpu_index_search_bitmap_ctx(nullptr, 1, q.data(), 3, bits, 16, dist.data(), lab.data(), nullptr) == LB_ERR_INVALID_ARG, "host");
    REQUIRE(lb_gpu_index_search_bitmap_device_ctx(nullptr, 1, q.data(), 3, bits, 16, dist.data(), lab.data(), nullptr, nullptr) == LB_ERR_INVALID_ARG,
            "device");
    REQUIRE(lb_gpu_index_search_bitmap_ctx(nullptr, 1, q.data(), 3, nullptr, 0, dist.data(), lab.data(), nullptr) == LB_ERR_INVALID_ARG,
            "NULL bitmap");
    REQUIRE(lb_gpu_index_nvisible(nullptr) == 0, "nvisible");
    for (int i = 0; i < 3; i++) REQUIRE(dist[(size_t)i] == -3.0f && lab[(size_t)i] == -9, "written at %d", i);
    std::printf("ok   TestIndexBitmap_NullHandle\n");
}

// the wrapper's own checks: the query's dimension and the bitmap's length
static void TestIndexBitmap_Validation(bool &skipped)
{
    auto [raw, err] = NewIndexWithConfig(GPUConfig{0, 8});
    if (err) { std::printf("SKIP GPU not available: %s\n", err.message.c_str()); skipped = true; return; }
    std::unique_ptr<Index> idx(raw);
    const int n = 19;
    std::vector<float> X((size_t)n * 8);
    for (size_t i = 0; i < X.size(); i++) X[i] = (float)((i * 37) % 101) * 0.01f;
    std::vector<int64_t> ids((size_t)n);
    for (int i = 0; i < n; i++) ids[(size_t)i] = 100 + i;
    err = idx->Add(ids, X);
    REQUIRE(!err, "%s", err.message.c_str());
    std::vector<float> q(X.begin(), X.begin() + 8);
    std::vector<int64_t> rids;
    std::vector<float> dist;
    err = idx->SearchBitmap(std::vector<float>(7, 0.f), 3, std::vector<uint8_t>(3, 0xFF), rids, dist);
    REQUIRE(err && err.message == "query vector dimension 7 does not match index dimension 8", "%s", err.message.c_str());
    err = idx->SearchBitmap(q, 3, std::vector<uint8_t>(2, 0xFF), rids, dist);
    REQUIRE(err && err.code == LB_ERR_INVALID_ARG && err.message == "a bitmap of 2 bytes, 3 are read for 19 rows", "%s", err.message.c_str());
    err = idx->SearchBitmap(q, 3, std::vector<uint8_t>(4, 0xFF), rids, dist);
    REQUIRE(err && err.code == LB_ERR_INVALID_ARG, "a long bitmap");
    // the batched form hands nbits through: the library names both numbers
    std::vector<int64_t> lab(3, -9);
    std::vector<float> d3(3, -3.0f);
    const std::vector<uint8_t> all(3, 0xFF);
    err = idx->SearchBatchBitmap(q.data(), 1, 3, all.data(), n + 1, lab.data(), d3.data());
    REQUIRE(err && err.code == LB_ERR_INVALID_ARG && err.message.find("20") != std::string::npos && err.message.find("19") != std::string::npos,
            "%s", err.message.c_str());
    REQUIRE(lab[0] == -9 && d3[0] == -3.0f, "written by a refused call");
    // row 0 hidden: its id does not come back, everything else does in order; padding is trimmed
    std::vector<uint8_t> bits(3, 0);
    bits[0] = 0x06; // rows 1 and 2
    err = idx->SearchBitmap(q, 5, bits, rids, dist);
    REQUIRE(!err, "%s", err.message.c_str());
    REQUIRE(rids.size() == 2 && dist.size() == 2, "len %zu", rids.size());
    REQUIRE((rids[0] == 101 || rids[0] == 102) && (rids[1] == 101 || rids[1] == 102) && rids[0] != rids[1], "ids %lld %lld", (long long)rids[0],
            (long long)rids[1]);
    // the index is as it was
    err = idx->Search(q, 1, rids, dist);
    REQUIRE(!err && rids.size() == 1 && rids[0] == 100 && dist[0] == 0.f, "plain search after a bitmap search");
    REQUIRE(!idx->Close(), "close");
    err = idx->SearchBitmap(q, 3, all, rids, dist);
    REQUIRE(err && err.message == "index is closed", "%s", err.message.c_str());
    std::printf("ok   TestIndexBitmap_Validation\n");
}

// one bitmap search against the oracle: 5,003 x 24, 9 queries, k = 10, about a third of the rows visible, ones behind the last bit
static void TestIndexBitmap_MatchesOracle()
{
    const int n = 5003, d = 24, nq = 9, k = 10;
    auto [raw, err] = NewIndexWithConfig(GPUConfig{0, d});
    REQUIRE(!err, "%s", err.message.c_str());
    std::unique_ptr<Index> idx(raw);
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::vector<float> X((size_t)n * d), Q((size_t)nq * d);
    for (auto &v : X) v = u(rng);
    for (auto &v : Q) v = u(rng);
    std::vector<int64_t> ids((size_t)n);
    for (int i = 0; i < n; i++) ids[(size_t)i] = (int64_t)i;
    err = idx->Add(ids, X);
    REQUIRE(!err, "%s", err.message.c_str());
    std::vector<uint8_t> mask((size_t)n), bits((size_t)(n + 7) / 8, 0);
    for (int r = 0; r < n; r++) {
        mask[(size_t)r] = (rng() % 3) == 0;
        if (mask[(size_t)r]) bits[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7));
    }
    bits.back() |= (uint8_t)(0xFFu << (n & 7)); // n % 8 == 3: five bits that are no rows
    std::vector<int64_t> lab((size_t)nq * k), olab((size_t)nq * k);
    std::vector<float> dist((size_t)nq * k), odist((size_t)nq * k);
    err = idx->SearchBatchBitmap(Q.data(), nq, k, bits.data(), n, lab.data(), dist.data());
    REQUIRE(!err, "%s", err.message.c_str());
    lbo_search_batch(LB_METRIC_EUCLIDEAN, 0, Q.data(), nq, X.data(), n, d, k, mask.data(), nullptr, olab.data(), odist.data(), 1);
    REQUIRE(std::memcmp(lab.data(), olab.data(), lab.size() * sizeof(int64_t)) == 0, "labels differ from the oracle");
    REQUIRE(std::memcmp(dist.data(), odist.data(), dist.size() * sizeof(float)) == 0, "distances differ from the oracle");
    // a NULL bitmap is the plain search
    err = idx->SearchBatchBitmap(Q.data(), nq, k, nullptr, -5, lab.data(), dist.data());
    REQUIRE(!err, "%s", err.message.c_str());
    lbo_search_batch(LB_METRIC_EUCLIDEAN, 0, Q.data(), nq, X.data(), n, d, k, nullptr, nullptr, olab.data(), odist.data(), 1);
    REQUIRE(std::memcmp(lab.data(), olab.data(), lab.size() * sizeof(int64_t)) == 0 && std::memcmp(dist.data(), odist.data(), dist.size() * sizeof(float)) == 0,
            "NULL bitmap differs from the plain search");
    std::printf("ok   TestIndexBitmap_MatchesOracle\n");
}

int main()
{
    bool skipped = false;
    TestIndexBitmap_NullHandle();
    TestIndexBitmap_Validation(skipped);
    if (!skipped) TestIndexBitmap_MatchesOracle();
    if (failures) { std::printf("FAILED (%d)\n", failures); return 1; }
    if (skipped) return 77;
    std::printf("PASS\n");
    return 0;
}
