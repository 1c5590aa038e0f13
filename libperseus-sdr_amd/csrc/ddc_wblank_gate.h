/*
 * ddc_wblank_gate.h -- the wideband blanker's arithmetic as plain integer functions: the parameter limits, the power of
 * a sample, the trigger's limit, the gate numerator, the scaling, the re-pack of two samples and the lengths of what is
 * carried.  k_wblank_* (ddc_wblank.hip) and the host side (ddc_wblank.cpp) both use them, and tests/wblank_gate_test.cpp
 * runs them under the sanitizers with a host compiler: no HIP header here.
 */
#ifndef PDDC_DDC_WBLANK_GATE_H
#define PDDC_DDC_WBLANK_GATE_H

#include <stdint.h>

#ifdef __HIPCC__
#define PDDC_WB_FN __host__ __device__ inline
#else
#define PDDC_WB_FN inline
#endif

namespace pddc {

static constexpr int kWbMinBlock = 64, kWbMaxBlock = 4096, kWbMaxHistory = 16, kWbMaxGuard = 128, kWbMaxRampLog2 = 7;
static constexpr int kWbMaxDelay = 255;
static constexpr uint32_t kWbMinThr16 = 16, kWbMaxThr16 = 65536;
static constexpr uint64_t kWbNoBlock = ~0ull;       /* the sum of a block in front of the stream: never the minimum */

/* log2 of a power of two in [64, 4096]; -1 for anything else */
PDDC_WB_FN constexpr int wb_log2_block(int B)
{
    for (int b = 6; b <= 12; ++b)
        if (B == (1 << b))
            return b;
    return -1;
}
/* R = 2^r - 1 */
PDDC_WB_FN constexpr int wb_ramp(int r) { return (1 << r) - 1; }
/* D = W + R */
PDDC_WB_FN constexpr int wb_delay(int W, int r) { return W + wb_ramp(r); }
PDDC_WB_FN constexpr bool wb_params_ok(int B, int H, int W, int r)
{
    return wb_log2_block(B) >= 0 && H >= 1 && H <= kWbMaxHistory && W >= 0 && W <= kWbMaxGuard && r >= 0 &&
           r <= kWbMaxRampLog2 && wb_delay(W, r) <= kWbMaxDelay;
}
PDDC_WB_FN constexpr bool wb_thr_ok(uint32_t thr16) { return thr16 >= kWbMinThr16 && thr16 <= kWbMaxThr16; }

/* samples carried between batches: the last 2 D inputs, rounded up to whole groups of 8 (0, 8, .. 512) */
PDDC_WB_FN constexpr int wb_tail_len(int D) { return (2 * D + 7) & ~7; }
/* ... and the bytes of their trigger bits, one byte per group */
PDDC_WB_FN constexpr int wb_tail_bit_bytes(int D) { return wb_tail_len(D) / 8; }

/* the block of stream sample m, and m's place in it */
PDDC_WB_FN constexpr uint64_t wb_block_of(uint64_t m, int b) { return m >> b; }
PDDC_WB_FN constexpr uint64_t wb_block_offset(uint64_t m, int b) { return m & ((1ull << b) - 1); }
/* sums a batch of n samples that starts at stream sample N adds to or completes: blocks (N mod B + n - 1) >> b, + 1 */
PDDC_WB_FN constexpr uint64_t wb_blocks_touched(uint64_t N, uint64_t n, int b)
{
    return n ? ((wb_block_offset(N, b) + n - 1) >> b) + 1 : 0;
}

/* the 24-bit code of an MSB-aligned sample (value * 256, as pddc_unpack24_i32 gives it) */
PDDC_WB_FN constexpr int32_t wb_code(int32_t msb) { return msb >> 8; }
/* p = I^2 + Q^2 of two codes in [-2^23, 2^23): at most 2^47 */
PDDC_WB_FN constexpr uint64_t wb_power(int32_t i, int32_t q)
{
    return (uint64_t)((int64_t)i * i) + (uint64_t)((int64_t)q * q);
}
/* the trigger's limit: (mean thr16) >> 4; mean <= 2^47 and thr16 <= 2^16, so the product is at most 2^63 */
PDDC_WB_FN constexpr uint64_t wb_limit(uint64_t mean, uint32_t thr16) { return (mean * thr16) >> 4; }
PDDC_WB_FN constexpr bool wb_trigger(bool on, uint64_t mean, uint64_t p, uint32_t thr16)
{
    return on && mean > 0 && p > wb_limit(mean, thr16);
}
/* the gate numerator at distance dist <= D from the nearest trigger: 0 inside the guard, 1 .. R on the ramp */
PDDC_WB_FN constexpr int wb_num(int dist, int W) { return dist <= W ? 0 : dist - W; }
/* sign(v) ((|v| num) >> r): toward zero; |v| <= 2^23 and num < 2^7, so the product is below 2^31 */
PDDC_WB_FN constexpr int32_t wb_scale(int32_t v, int num, int r)
{
    const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    const int32_t s = (int32_t)((mag * (uint32_t)num) >> r);
    return v < 0 ? -s : s;
}
/* two samples' codes -> their 12 bytes as three little-endian dwords (I0 Q0 I1 Q1, three bytes each) */
PDDC_WB_FN void wb_pack2(int32_t i0, int32_t q0, int32_t i1, int32_t q1, uint32_t &a, uint32_t &b, uint32_t &c)
{
    const uint32_t ui0 = (uint32_t)i0 & 0xffffffu, uq0 = (uint32_t)q0 & 0xffffffu, ui1 = (uint32_t)i1 & 0xffffffu,
                   uq1 = (uint32_t)q1 & 0xffffffu;
    a = ui0 | (uq0 << 24);
    b = (uq0 >> 8) | (ui1 << 16);
    c = (ui1 >> 16) | (uq1 << 8);
}
/* ... and back, to MSB-aligned values: what unpack2_msb (ddc_dev.h) does with byte selectors */
PDDC_WB_FN void wb_unpack2_msb(uint32_t a, uint32_t b, uint32_t c, int32_t &i0, int32_t &q0, int32_t &i1, int32_t &q1)
{
    i0 = (int32_t)(a << 8);
    q0 = (int32_t)(((a >> 24) | (b << 8)) << 8);
    i1 = (int32_t)(((b >> 16) | (c << 16)) << 8);
    q1 = (int32_t)(c & 0xffffff00u);
}

} // namespace pddc
#endif
