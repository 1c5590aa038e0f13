/*
 * wblank_gate_test.cpp -- the wideband blanker's integer arithmetic (csrc/ddc_wblank_gate.h, what k_wblank_* and
 * ddc_wblank.cpp both use) on vectors written out here: a program of its own for a host compiler, built and run under
 * AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_wblank_gate_cpu.py.  Prints "ok: <checks>" and returns 0,
 * or says which check failed and returns 1.
 */
#include "ddc_wblank_gate.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pddc;

static long checks = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond);                                         \
            exit(1);                                                                                                   \
        }                                                                                                              \
    } while (0)

/* the contract's scaling in 64-bit, the slow way */
static int32_t scale_ref(int32_t v, int num, int r)
{
    const int64_t mag = v < 0 ? -(int64_t)v : (int64_t)v;
    const int64_t s = (mag * num) >> r;
    return (int32_t)(v < 0 ? -s : s);
}

/* six bytes per sample, little-endian, I first: the stream's format written out byte by byte */
static void bytes_of(const int32_t (&c)[4], uint8_t (&out)[12])
{
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j)
            out[3 * k + j] = (uint8_t)(((uint32_t)c[k] >> (8 * j)) & 0xffu);
}

int main()
{
    const int32_t lo = -(1 << 23), hi = (1 << 23) - 1;

    /* parameters */
    CHECK(wb_log2_block(64) == 6 && wb_log2_block(4096) == 12 && wb_log2_block(32) < 0 && wb_log2_block(8192) < 0 &&
          wb_log2_block(96) < 0 && wb_log2_block(0) < 0 && wb_log2_block(-64) < 0);
    CHECK(wb_ramp(0) == 0 && wb_ramp(3) == 7 && wb_ramp(7) == 127);
    CHECK(wb_delay(128, 7) == kWbMaxDelay && wb_delay(0, 0) == 0);
    CHECK(wb_params_ok(64, 1, 0, 0) && wb_params_ok(4096, 16, 128, 7) && !wb_params_ok(4096, 17, 128, 7) &&
          !wb_params_ok(4096, 0, 0, 0) && !wb_params_ok(64, 1, 129, 0) && !wb_params_ok(64, 1, -1, 0) &&
          !wb_params_ok(64, 1, 0, 8) && !wb_params_ok(64, 1, 0, -1) && !wb_params_ok(128 + 64, 1, 0, 0));
    CHECK(wb_thr_ok(16) && wb_thr_ok(65536) && !wb_thr_ok(15) && !wb_thr_ok(65537) && !wb_thr_ok(0) && !wb_thr_ok(~0u));

    /* what is carried: D = 0, 1, 255 and every D between */
    CHECK(wb_tail_len(0) == 0 && wb_tail_bit_bytes(0) == 0);
    CHECK(wb_tail_len(1) == 8 && wb_tail_bit_bytes(1) == 1);
    CHECK(wb_tail_len(4) == 8 && wb_tail_len(5) == 16);
    CHECK(wb_tail_len(255) == 512 && wb_tail_bit_bytes(255) == 64);
    for (int D = 0; D <= kWbMaxDelay; ++D) {
        const int tl = wb_tail_len(D);
        CHECK(tl % 8 == 0 && tl >= 2 * D && tl < 2 * D + 8 && tl - D >= D && wb_tail_bit_bytes(D) * 8 == tl);
    }

    /* the block grid at stream positions beyond 2^32 and at the top of uint64 */
    const uint64_t big = (1ull << 32) + 8;
    CHECK(wb_block_of(big, 6) == (1ull << 26) && wb_block_offset(big, 6) == 8);
    CHECK(wb_block_of(big, 12) == (1ull << 20) && wb_block_offset(big, 12) == 8);
    CHECK(wb_block_of((1ull << 40) + 4095, 12) == (1ull << 28) && wb_block_offset((1ull << 40) + 4095, 12) == 4095);
    CHECK(wb_block_of(~0ull - 7, 6) == (~0ull >> 6) && wb_block_offset(~0ull - 7, 6) == 56);
    CHECK(wb_blocks_touched(0, 0, 6) == 0 && wb_blocks_touched(0, 8, 6) == 1 && wb_blocks_touched(56, 8, 6) == 1 &&
          wb_blocks_touched(56, 16, 6) == 2 && wb_blocks_touched(big, 64, 6) == 2 && wb_blocks_touched(big, 56, 6) == 1 &&
          wb_blocks_touched((1ull << 33), 1ull << 23, 6) == (1ull << 17) &&
          wb_blocks_touched((1ull << 33) + 4088, 1ull << 23, 12) == (1ull << 11) + 1);

    /* codes and powers at the ends of the range */
    CHECK(wb_code((int32_t)0x80000000u) == lo && wb_code(0x7fffff00) == hi && wb_code(-256) == -1 && wb_code(0) == 0);
    CHECK(wb_power(lo, lo) == (1ull << 47));
    CHECK(wb_power(hi, hi) == 2ull * (uint64_t)hi * (uint64_t)hi);
    CHECK(wb_power(lo, 0) == (1ull << 46) && wb_power(0, 0) == 0 && wb_power(-1, 1) == 2);
    /* a block of 4096 such samples: 2^59 */
    uint64_t S = 0;
    for (int k = 0; k < 4096; ++k)
        S += wb_power(lo, lo);
    CHECK(S == (1ull << 59) && (S >> 12) == (1ull << 47));

    /* the limit: mean thr16 at 2^63 */
    CHECK(wb_limit(1ull << 47, 65536) == (1ull << 59));
    CHECK(wb_limit(1ull << 47, 16) == (1ull << 47));
    CHECK(wb_limit(1, 16) == 1 && wb_limit(1, 17) == 1 && wb_limit(3, 24) == 4 && wb_limit(0, 65536) == 0);
    CHECK(!wb_trigger(true, 1ull << 47, 1ull << 47, 16));              /* p > limit, not >= */
    CHECK(!wb_trigger(true, 1ull << 47, 1ull << 47, 65536));
    CHECK(wb_trigger(true, (1ull << 47) - 1, 1ull << 47, 16));
    CHECK(!wb_trigger(true, 0, 1ull << 47, 16));                       /* no reference yet */
    CHECK(!wb_trigger(false, 1, 1ull << 47, 16));
    CHECK(wb_trigger(true, 1, 2, 16) && !wb_trigger(true, 1, 1, 16));

    /* the gate numerator */
    CHECK(wb_num(0, 0) == 0 && wb_num(1, 0) == 1 && wb_num(4, 4) == 0 && wb_num(5, 4) == 1 && wb_num(11, 4) == 7 &&
          wb_num(255, 128) == 127 && wb_num(128, 128) == 0);

    /* the scaling: every (num, r), the ends of the range, +-1, toward zero on both sides */
    const int32_t vals[] = { lo, lo + 1, -12345, -3, -2, -1, 0, 1, 2, 3, 12345, hi - 1, hi };
    for (int r = 0; r <= kWbMaxRampLog2; ++r)
        for (int num = 0; num <= wb_ramp(r); ++num)
            for (const int32_t v : vals) {
                const int32_t s = wb_scale(v, num, r);
                CHECK(s == scale_ref(v, num, r));
                CHECK((v >= 0 ? s >= 0 && s <= v : s <= 0 && s >= v) && wb_scale(-v, num, r) == -s);
            }
    CHECK(wb_scale(lo, 127, 7) == -8323072 && wb_scale(hi, 127, 7) == 8323071 && wb_scale(-1, 7, 3) == 0 &&
          wb_scale(-8, 7, 3) == -7 && wb_scale(-9, 7, 3) == -7 && wb_scale(9, 7, 3) == 7 && wb_scale(lo, 0, 0) == 0);

    /* the re-pack: negative values, the ends, and the way back */
    const int32_t sets[][4] = { { lo, hi, -1, 0 }, { -1, -1, -1, -1 }, { 0x123456, -0x123456, 0x7f00ff, -0x7f00ff },
                                { hi, lo, hi, lo }, { 1, -2, 3, -4 }, { 0, 0, 0, 0 }, { -256, 255, -65536, 65535 } };
    for (const auto &c : sets) {
        uint32_t w[3];
        wb_pack2(c[0], c[1], c[2], c[3], w[0], w[1], w[2]);
        uint8_t want[12];
        bytes_of(c, want);
        for (int k = 0; k < 12; ++k)
            CHECK(((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == want[k]);
        int32_t i0, q0, i1, q1;
        wb_unpack2_msb(w[0], w[1], w[2], i0, q0, i1, q1);
        CHECK(wb_code(i0) == c[0] && wb_code(q0) == c[1] && wb_code(i1) == c[2] && wb_code(q1) == c[3]);
        CHECK((i0 & 0xff) == 0 && (q0 & 0xff) == 0 && (i1 & 0xff) == 0 && (q1 & 0xff) == 0);
    }
    /* a scaled negative sample through the pack: bytes of -7 */
    {
        uint32_t w[3];
        wb_pack2(wb_scale(-9, 7, 3), wb_scale(9, 7, 3), 0, 0, w[0], w[1], w[2]);
        CHECK(w[0] == 0x07fffff9u && w[1] == 0u && w[2] == 0u);
    }

    /* a gate over a short series, the slow way against wb_num: W = 1, r = 2 (R = 3, D = 4), triggers at 10 and 13 */
    {
        const int W = 1, r = 2, D = wb_delay(W, r);
        std::vector<int> num(24, -1);
        const int trig[] = { 10, 13 };
        for (int m = 0; m < 24; ++m) {
            int dist = -1;
            for (const int u : trig) {
                const int d = m > u ? m - u : u - m;
                if (d <= D && (dist < 0 || d < dist))
                    dist = d;
            }
            if (dist >= 0)
                num[m] = wb_num(dist, W);
        }
        const int want[24] = { -1, -1, -1, -1, -1, -1, 3, 2, 1, 0, 0, 0, 0, 0, 0, 1, 2, 3, -1, -1, -1, -1, -1, -1 };
        for (int m = 0; m < 24; ++m)
            CHECK(num[m] == want[m]);
    }

    printf("ok: %ld checks\n", checks);
    return 0;
}
