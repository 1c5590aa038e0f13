/*
 * ddc_fir_i8.hip -- the first stages on the INT8 matrix cores of gfx950 (MI355X, CDNA4): k_fir_i8x.
 *
 * The wire bytes are the operand planes (a 24-bit sample IS three bytes), the taps four planes of balanced base-256 digits,
 * int32 accumulation is exact.  Without NCO one tap table; with it the NCO is folded into the TAPS:
 *       y[m] = LO(n0 + 8 m) * sum_k (h[k] e^{+j theta k}) x_raw[8 m - k],   theta = 2 pi freg / 2^32,
 * i.e. complex taps on the raw integer planes (four real band products instead of one) and ONE float rotation per output,
 * with the exact 32-bit phase; optionally a second decimate-by-8 stage fused behind it (the cascades' pair: the 1 B/sample
 * intermediate never reaches HBM); a decimate-by-10 form.  Tiles are handed round the blocks in chunks of C (1:
 * tile-interleaved, what streams best; the pair: 4, or 8 with two matrix + two finishing waves from 2^23 samples on), NOTEBOOK.md R4.2.
 * (Round 3's k_fir_i8 -- the same product without NCO, eight matrix waves -- lived here until round 5; what it alone
 * offered, binary16-STORED taps quantised by the matrix waves themselves, is now the plain form's FirI8xArgs::taps16.)
 *
 * Reference anchors: the samples are the 24-bit wire format of examples/perseustest.c:449-455, the tuning word is
 * perseus-sdr.c:584; the arithmetic itself has no reference source (FPGA bitstreams), DESIGN.md 3.
 */
#include "ddc_kernels.h"
#include "ddc_dev.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace pddc {

/* ---- the formulation (round 3; what every form below shares) ----------------------------------------------------------
 * int8 MFMA has thirty times the vector unit's multiply-add peak, and this data fits it exactly: a 24-bit sample is three
 * bytes, a tap quantised to 2^-E (E = 30 - ceil(log2 max|h|), i.e. 31 significant bits on the largest tap) is four
 * balanced base-256 digits, every digit x byte-plane product sum over 256 taps stays below 2^24, so int32 accumulation is
 * EXACT; products of equal weight 256^(i+j) share an accumulator, the three lightest (i + j < 2: below 1.2e-7 of full
 * scale even if every term had the same sign, 2e-9 typical) are dropped, and the four sums are recombined in fp32 once
 * per output.  The unpack is gone: the loaders only de-interleave bytes (v_perm, 24 per 8 samples) into six planes (the two
 * low bytes of each component xor 0x80: unsigned -> signed, the offset comes back as one constant per filter).
 *   out[16 n + r] = sum_c T[r][c] X[c][n],  T[r][c] = h[HIST - (c - 8 r)] (banded Toeplitz, 16 x (120 + HIST)),
 *   X[c][n] = xp[8192 tile + 128 n + c],    xp = the HIST history samples followed by the batch.
 * v_mfma_i32_16x16x64_i8: 16 output rows, 16 columns, k-steps of 64; 9 plane products per step.  LDS rows are padded (lane
 * stride 144 B / 20 floats): conflict-free.  Measured as stand-alone prototypes first (tools/ubench/fir_i8_planes*.hip). */
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));
namespace i8 {
__device__ __forceinline__ int swz(int p) { return p + 16 * (p >> 7); }

/* the 8 bytes at offsets 6 s + O and the 8 at 6 s + O + 1 (s = 0..7; O = 0, 2, 4) of the 48 bytes w[0..11]: planes O and
 * O + 1, a[0] / b[0] samples 0..3, a[1] / b[1] samples 4..7.  In each 24-byte half the two planes live in the same dwords
 * -- samples 0, 1 in dwords (O >> 2, (O + 6) >> 2), samples 2, 3 three dwords on -- so ONE perm per dword pair picks two
 * bytes for each plane ([a0 a1 b0 b1], [a2 a3 b2 b3]) and two more put the planes' dwords together: 4 perms per plane pair
 * and half, 24 per group (one plane at a time took 36) */
template <int O>
__device__ __forceinline__ void plane_pair_bytes(const uint32_t (&w)[12], uint32_t (&a)[2], uint32_t (&b)[2])
{
    static_assert(O == 0 || O == 2 || O == 4, "an even plane and its neighbour");
    constexpr uint32_t sel = (uint32_t)(O & 3) | ((uint32_t)(4 + ((O + 6) & 3)) << 8) | ((uint32_t)((O + 1) & 3) << 16) |
                             ((uint32_t)(4 + ((O + 7) & 3)) << 24);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int d = 6 * half;
        const uint32_t p = __builtin_amdgcn_perm(w[d + ((O + 6) >> 2)], w[d + (O >> 2)], sel);
        const uint32_t q = __builtin_amdgcn_perm(w[d + ((O + 18) >> 2)], w[d + ((O + 12) >> 2)], sel);
        a[half] = __builtin_amdgcn_perm(q, p, 0x05040100u);
        b[half] = __builtin_amdgcn_perm(q, p, 0x07060302u);
    }
}

} // namespace i8

/* host: the binary16 array the plain form reads with FirI8xArgs::taps16 (values must be binary16-representable):
 * G[128 + tt] = h[hist - tt] for tt = 1 .. hist, zeros elsewhere */
void fir_i8_taps16(const float *taps, int ntaps, int hist, uint16_t *out)
{
    for (int i = 0; i < kFirI8Taps16Len; ++i)
        out[i] = 0;
    for (int tt = 1; tt <= hist; ++tt) {
        const int k = hist - tt;
        if (k < ntaps) {
            const _Float16 hv = (_Float16)taps[k];
            __builtin_memcpy(&out[128 + tt], &hv, 2);
        }
    }
}


/* ======================================================================== */
/* k_fir_i8x : decimate by 8 on the int8 matrix cores WITH the NCO, [+ a fused second decimate-by-8 stage]              */
/* ======================================================================== */
/* The mix commutes with the filter once it is moved into the taps (file header): what k_fir_i8 multiplies by h[k] this
 * kernel multiplies by gc[k] = h[k] cos(theta k) and gs[k] = h[k] sin(theta k),
 *     uI = gc * xI - gs * xQ,   uQ = gs * xI + gc * xQ     (* = the band product of k_fir_i8, exact in int32),
 * and y[m] = (uI + j uQ)[m] (cos phi_m - j sin phi_m), phi_m = the exact 32-bit phase of input sample n0 + 8 m, one
 * nco_lo and four multiplies per OUTPUT.  The samples stay the integers of the wire: no per-sample mix, no rounding
 * before the accumulation.  Three forms of one kernel (MODE):
 *   0  no NCO            waves = component x half of the columns, one tap set                    (k_fir_i8's arithmetic)
 *   1  NCO, 129..256 taps waves = tap set (c / s) x half of the columns, BOTH components each: four partial products
 *                        P[c|s][I|Q] meet in LDS, uI = P[c][I] - P[s][Q], uQ = P[s][I] + P[c][Q] at the stores
 *                        (two tap sets in one wave would need 2 x 96 registers)
 *   2  NCO, <= 128 taps  ONE operand holds both tap sets: rows 0..7 the band of eight outputs for one set, rows 8..15 the
 *                        band of the same eight outputs for the other (columns of 8 outputs, 64 samples apart; the band is
 *                        56 + HIST wide: 2 k-steps up to 64 taps, 3 up to 128).  [c ; s] meets the I planes, [-s ; c] the Q
 *                        planes, both into the SAME int32 accumulators: rows 0..7 come out as uI, rows 8..15 as uQ --
 *                        complete, one rounding -- and every wave makes both rails of its columns.  A third fewer matrix
 *                        instructions than two 16-row bands per rail (the dead corners of a band shrink with its height):
 *                        same box, 2^28 samples, 48 taps 0.3406 -> 0.3272 ms, 127 taps 0.3865 -> 0.3513 (it replaced a form
 *                        with both 16-row tables per wave for <= 64 taps and took 65..128 taps over from mode 1)
 * The tuned form 2 also DECIMATES BY 10 (template D = 10, hist = 64; the 1.6 / 2 / 1 MS/s plans' first stage,
 * launch_fir_i8x_d10): columns of 8 outputs 80 samples apart, a band of 70 + 64 samples = 3 k-steps, tiles of 10240 samples =
 * 1024 outputs, 1280 loader groups (two and a half rounds).  A stream's decimation phase makes a batch's first window end on
 * any sample 0 .. 9; the loaders' groups sit on multiples of 8, so the taps are delayed by (-first) mod 8 samples (one table
 * set per delay, built on the host) and the windows end on in_off = first + delay; the rotation takes that sample's phase.
 * Walk: the batch is cut into chunks of C tiles and block b takes chunks b, b + G, b + 2 G, ...  C = 1 is k_fir_i8's
 * tile-interleaved walk -- all CUs read one compact window of the batch, which is what this chip's HBM likes (same
 * kernel, 2^28 samples: contiguous ranges per block 0.380 ms, interleaved 0.332) --; inside a chunk the HIST samples in
 * front of a tile are the last ones of the tile before it and come over from the previous plane set inside LDS, only a
 * chunk's first tile loads them.
 * FUSE2 (modes 0 and 2): the tile's 1024 first-stage values u stay in LDS behind a 64-entry porch that holds the 64 values
 * in front of the tile; thread p of waves 0/1 computes second-stage output p of the tile,
 *     z = LO(n0 + 64 P) sum_k (h2[k] e^{+j 8 theta k}) u[8 P - k],
 * from float4 reads of both rails (packed FMAs, taps through the scalar cache) and stores it; still ONE barrier per tile.
 * Inside a chunk the porch is the previous tile's tail (copied by the two waves that do not filter); a chunk's first tile
 * computes it itself: four more columns in front of the tile (one extra pass of the matrix waves 2/3 over 512 + HIST more
 * samples, loaded by 72 loader lanes) -- no tile depends on another block, no warm-up tile; the batch's first tile takes
 * the stream's second-stage history (the 64 mixed first-stage outputs k_fir8's fused pair keeps too) instead.        */
namespace i8x {
using i8::plane_pair_bytes;
using i8::swz;
constexpr int TILE = 8192;
constexpr int kTaps2Len = 68;                  /* floats per rail of the second stage's tap table (65 used) */

/* D: the decimation -- 8, or 10 for the tuned form with paired rows (mode 2): a tile is 1024 outputs = 1024 D samples */
template <int HIST, int MODE, bool FUSE2, int D = 8>
struct Geo {
    static constexpr int EXTRA = FUSE2 ? 512 : 0;                   /* samples in front of the history: the porch's columns */
    static constexpr int FRONT = EXTRA + HIST;
    static constexpr int TILE_S = 1024 * D;                         /* samples per tile */
    static constexpr int SPAN = TILE_S + FRONT, PLANE = SPAN + 16 * ((SPAN + 127) / 128);
    /* the band of a row block: 16 outputs (modes 0, 1) or 8 outputs x the two tap sets (mode 2), D samples apart, + HIST */
    static constexpr int KSTEPS = ((MODE == 2 ? 7 : 15) * D + HIST + 63) / 64;
    static constexpr int HG = HIST / 8, FG = FRONT / 8;              /* history groups of 8 samples; with the extra ones */
    static constexpr int NARR = MODE == 1 ? 4 : 2;
    static constexpr int PORCH = FUSE2 ? 64 : 0;
    static constexpr int AS = 20 * ((1024 + PORCH) / 16);            /* floats per output array (16 values per 20) */
    static constexpr size_t LDS_BYTES = 12 * (size_t)PLANE + 2 * (size_t)NARR * AS * sizeof(float);
    static constexpr int NTAB = MODE == 0 ? 1 : 2;
    static constexpr int TABV = 4 * KSTEPS * 64;                     /* v4i entries per tap table */
    static_assert(MODE != 2 || HIST <= 128, "two paired tables of 5 k-steps do not fit the registers");
    static_assert(D == 8 || (D == 10 && MODE == 2 && !FUSE2), "decimate-by-10: the tuned paired-rows form only");
    static_assert(!(FUSE2 && MODE == 1), "the fused second stage reads complete u values");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(FG <= 128, "front groups are loaded by the first loader waves");
};

/* a block's tile sequence: chunk b, b + G, ... of C tiles each */
struct Cursor {
    long long chunk;
    int k;
};
struct Walk {
    long long ntiles, G;
    int C;
    __device__ __forceinline__ long long tile(const Cursor &c) const
    {
        const long long t = c.chunk * C + c.k;
        return t < ntiles ? t : -1;
    }
    __device__ __forceinline__ Cursor next(Cursor c) const
    {
        if (++c.k == C) {
            c.k = 0;
            c.chunk += G;
        }
        return c;
    }
};

/* 8 samples (48 bytes) -> 8 bytes in each of the six planes; `p`: this lane's (swizzled) position in the set's plane 0 --
 * the planes then lie at constant offsets below 64 KB, inside the LDS store's offset field */
__device__ __forceinline__ void put_planes(const uint4 (&r)[3], uint8_t *p, int PLANE)
{
    const uint32_t w[12] = { r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w };
    uint32_t lo[2], hi[2];
    /* planes O and O + 1 of the wire = plane sets' planes PA and PB; XA / XB: unsigned -> signed for the two low bytes */
#define PDDC_PL(O, PA, XA, PB, XB)                                                                \
    plane_pair_bytes<O>(w, lo, hi);                                                               \
    *reinterpret_cast<uint2 *>(p + (PA) * PLANE) = make_uint2(lo[0] ^ XA, lo[1] ^ XA);            \
    *reinterpret_cast<uint2 *>(p + (PB) * PLANE) = make_uint2(hi[0] ^ XB, hi[1] ^ XB);
    PDDC_PL(0, 0, 0x80808080u, 1, 0x80808080u)
    PDDC_PL(2, 2, 0u, 3, 0x80808080u)
    PDDC_PL(4, 4, 0x80808080u, 5, 0u)
#undef PDDC_PL
}

/* The main groups of a tile come through a buffer descriptor of the TILE (built from wave-uniform values: the batch, the
 * tile): base = the tile's first sample, records = the bytes of its groups that lie WHOLLY inside the batch -- none for "no
 * tile" (t < 0) --, so that the loads need neither a branch nor a zero fill: a group behind the batch comes back as zeros
 * from the range check.  hipcc answers a load under a runtime condition with s_waitcnt vmcnt(0) -- with the branches the
 * loader waves waited for every group right behind issuing it and nothing ran two tiles ahead (NOTEBOOK R26) --, loads it
 * can count it waits for at their first use.  Rebased per tile the record count stays below 64 KB whatever the batch.
 * (Cached loads: a lane's three 16-byte loads share their cache lines with its neighbours' -- as NONTEMPORAL loads the lines
 * are fetched again and again: 0.3205 -> 0.4293 ms for the untuned 127-tap stage, same box, tools/ab_i8x.sh.)          */
/* a wave-uniform 64-bit value, in scalar registers for what is computed from it (the descriptors' words) */
__device__ __forceinline__ long long uniform64(long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, long long byte_off, int bytes)
{
    const long long p = uniform64((long long)(static_cast<const uint8_t *>(base) + byte_off));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(p), 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
template <int TILE_S, int NGRP>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t group_rsrc(const FirI8xArgs &a, long long t)
{
    const long long s0 = uniform64(t < 0 ? 0 : t * TILE_S + a.in_off);
    long long left = (uniform64(a.n_in) - s0) >> 3;                  /* (n_in and in_off are multiples of 8) */
    left = t < 0 || left < 0 ? 0 : left > NGRP ? NGRP : left;
    return make_rsrc(a.in, s0 * 6, 48 * (int)left);
}

/* the three 16-byte loads of the group at byte `voff` of the descriptor's range (48 g for group g) */
__device__ __forceinline__ void issue_group(__amdgpu_buffer_rsrc_t rs, int voff, uint4 (&r)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 16 * i, 0, 0);
        r[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

/* ONE group per wave in flight: the step waits for the group it issued last before it issues the next -- behind that group's
 * conversion time, not right behind its issue.  Measured, not designed (NOTEBOOK R26): with two groups per wave in flight --
 * what hipcc's counted waits alone allow -- the untuned 127-tap stage at 2^28 samples takes 0.3203 ms, with one 0.3013, with
 * the wait right behind every issue (what the branches used to force) 0.3149; same box, alternating builds.  (Supposed: the
 * three loads of a group share every cache line, eight waves x 3 KB are 24 KB of lines in flight in a 32 KB L1, twice that
 * evicts lines between a group's first load and its third.  Not separated from it: vmcnt counts this wave's stores too, so
 * where the loaders finish tiles -- LAYOUT 1 -- the wait also drains their result stores.) */
__device__ __forceinline__ void loads_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

/* the descriptor of the FG front groups of tile t > 0 (all of them lie in the batch: samples TILE_S t - FRONT .. TILE_S t);
 * no records unless the tile starts a chunk */
template <int FRONT, int TILE_S>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t front_rsrc(const FirI8xArgs &a, long long t, bool wanted)
{
    const bool some = wanted && t > 0;
    return make_rsrc(a.in, some ? (uniform64(t * TILE_S + a.in_off) - FRONT) * 6 : 0, some ? 6 * FRONT : 0);
}

/* the groups in front of a chunk's first tile t: front group g (0 .. FG) = samples 8192 t - FRONT + 8 g ..; groups below
 * `g0` are not needed (no porch columns: not FUSE2, or the batch's first tile).  From the stream's history for t = 0.
 * (The block's FIRST tile only, once per launch: two sources and a zero fill, under branches -- every later tile's front
 * groups come from the batch alone, through front_rsrc.) */
template <int HIST, int FRONT, int TILE_S = TILE>
__device__ __forceinline__ void issue_front(const FirI8xArgs &a, long long t, int g, uint4 (&r)[3])
{
    const long long b = t * TILE_S - FRONT + 8LL * g + a.in_off;
    const int hl = a.hist_len ? a.hist_len : HIST;                   /* samples the history buffer holds (in front of a.in) */
    if (b < -(long long)hl) {                                       /* in front of the history: only zero taps reach there */
        r[0] = r[1] = r[2] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint4 *p = b < 0 ? reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(a.hist) + (b + hl) * 6)
                           : reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(a.in) + b * 6);
    r[0] = p[0];
    r[1] = p[1];
    r[2] = p[2];
}

/* A float2 store whose data registers stay untouched for two more issue slots.  Measured on MI355X (ROCm 7.2): when a wave
 * stores (global_store_dwordx2) while ANOTHER wave on its SIMD is issuing matrix instructions, and the wave's next vector
 * instruction overwrites one of the store's data registers, the last quarter of the wave (lanes 48..63) now and then stores
 * the new value of that register -- once per few thousand tiles with post waves beside two matrix waves, never seen without
 * a matrix wave beside the storing one.  hipcc pads only stores of more than 64 bits; the pad has to sit inside the statement,
 * or the scheduler moves vector instructions in front of it.
 * All result stores of this file are NONTEMPORAL: the outputs are written once and read by another kernel much later, and
 * keeping them out of the L2's way is worth 5.7 % on the untuned 127-tap stage (same box, two rounds: 0.3383 / 0.3359 ->
 * 0.3191 / 0.3166 ms), 2 % on the tuned 48-tap one, nothing where the matrix work bounds (tools/ab_i8x.sh).           */
__device__ __forceinline__ void store_f2_padded(float2 *p, float x, float y)
{
    const f32x2 v = { x, y };
    asm volatile("global_store_dwordx2 %0, %1, off nt\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

/* y = sum_s acc[s] 256^(s+2) as floats */
__device__ __forceinline__ float recombine(const v4i_t (&acc)[4], int v)
{
    return ((float)acc[0][v] * 65536.0f + (float)acc[1][v] * 16777216.0f) +
           ((float)acc[2][v] * 4294967296.0f + (float)acc[3][v] * 1099511627776.0f);
}
} // namespace i8x

/* Who does what (LAYOUT).  The matrix waves' chain per tile -- operand reads, matrix instructions, recombination, and then
 * the tile's finish (rotation and stores, or the second stage) -- was the longest in the block: the loaders sat in the
 * barrier for a third to a half of every tile while waves 0..3 finished it (in-kernel clock probe: tuned 48 taps, matrix pass
 * 2800 cycles + finish 2700 against 3650..4300 of loader work; the finish is slow because its stores queue behind the
 * loaders' loads in the CU's one memory pipeline).
 *   0  matrix waves 0..3 finish their tile themselves, behind its barrier (k_fir_i8's scheme)
 *   1  the LOADERS finish the tile before while the matrix waves work on this one: every wave of the block then has about
 *      the same work per tile; stores from a loader wave sit beside a matrix wave's instructions on its SIMD and need the
 *      padded form (store_f2_padded)
 *   2  TWO matrix waves (0, 1: one component -- or tap set -- each, all four column blocks) and two FINISHING waves (2, 3:
 *      the tile before, while the matrix waves work on this one).  Waves w, w + 4, w + 8 share a SIMD
 *      (tools/ubench/wave_simd.hip): the finishing waves have no matrix wave beside them (packed fp32 is safe there) and,
 *      without tap operands, the registers to keep a second stage's LDS reads in flight
 * (Tried: matrix and dedicated post waves on two SIMDs, six loader waves with the vector port to themselves on the other
 * two -- a matrix instruction holds its SIMD's vector issue port for 8 of its 16 cycles, which costs the loaders beside it
 * 0.05 ms per 2^28 samples -- but six loader waves stream worse than eight: 0.39 ms for every form.)                 */
template <int LAYOUT, int D = 8>
struct Roles {
    static constexpr int NLT = 512;                            /* loader threads */
    static constexpr int NPT = LAYOUT == 0 ? 256 : LAYOUT == 1 ? 512 : 128;       /* threads that finish a tile */
    static constexpr int NGRP = 128 * D;                       /* main groups of 8 samples per tile */
    static constexpr int NQ = (NGRP + NLT - 1) / NLT;          /* ... per loader thread (the last round may be partial) */
};

/* the block's work; `nblk` blocks walk this stream's tiles, this is block `blk` of them (k_fir_i8x: the grid; k_fir_i8x_many:
 * the grid's x dimension, one stream per y).
 * NCH > 1 (k_fir_i8x_bank; tuned paired rows, layout 0 only): NCH channels over ONE plane set per tile.  Matrix wave w works
 * for channel w / (4 / NCH) -- `a` is that channel's record, the loaders get channel 0's -- and takes 2 NCH of the tile's 8
 * column blocks; each channel has ONE value array pair (no double buffer: 4 x 10 KB beside the planes' 109 KB), and the wave
 * finishes exactly the outputs it computed, so only its own LDS writes are read back and no other wave waits for them.
 * Decimate by 10 (D = 10): 2 channels only -- the planes of a 10240-sample tile take 136 KB, two value array pairs (20 KB)
 * fit beside them in the CU's 160 KB, four (40 KB) do not. */
template <int HIST, int MODE, bool FUSE2, int LAYOUT, int D = 8, int NCH = 1>
__device__ __forceinline__ void fir_i8x_block(const FirI8xArgs &a, long long ntiles, int C, long long nblk, long long blk)
{
    using namespace i8x;
    using G = Geo<HIST, MODE, FUSE2, D>;
    using R = Roles<LAYOUT, D>;
    static_assert(NCH == 1 || (MODE == 2 && !FUSE2 && LAYOUT == 0 && ((D == 8 && (NCH == 2 || NCH == 4)) || (D == 10 && NCH == 2))),
                  "the bank: tuned paired rows, matrix waves finish; decimate by 8 with 2 or 4 channels, by 10 with 2");
    static_assert(12 * (size_t)G::PLANE + (size_t)NCH * G::NARR * G::AS * sizeof(float) <= 160 * 1024, "bank LDS");
    constexpr int TILE_S = G::TILE_S, NGRP = R::NGRP;
    constexpr bool PART = NGRP % R::NLT != 0;                  /* the last round of main groups is a partial one */
    constexpr int PLANE = G::PLANE, KSTEPS = G::KSTEPS, AS = G::AS, NARR = G::NARR, PORCH = G::PORCH, EXTRA = G::EXTRA,
                  FRONT = G::FRONT, NLT = R::NLT, NPT = R::NPT, NQ = R::NQ;
    constexpr bool MIX = MODE != 0;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_i8x[];
    /* [2 buffers][2 components][3 planes][PLANE], then [2 buffers][NARR][AS] first-stage values */
    float *arr_base = reinterpret_cast<float *>(lds_i8x + 12 * PLANE);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   /* (an SGPR: role branches are uniform) */
    const Walk wk{ ntiles, nblk, C };
    Cursor cur{ blk, 0 };
    const uint32_t n0lo = (uint32_t)a.n0;
    const long long n_out = a.n_out ? a.n_out : a.n_in >> 3;

    /* ---- finishing a tile whose values are in `arr` (after its barrier): non-FUSE2 combine, rotate, store float2 (thread
     * pt of NPT); FUSE2 the second stage and the porch copy.  GUARD: the batch's last tile (ragged end, hist2_out). */
    /* (u + j v) (c + j s) in place.  NO packed fp32 in code that loader waves run (this TU is compiled without the SLP
     * vectoriser, and the finishing code below uses no 2-vectors): on MI355X a v_pk_fma_f32 / v_pk_mul_f32 result consumed
     * one or two instructions later came out wrong in lanes 48..63 now and then -- only in waves that share their SIMD with
     * a wave issuing matrix instructions (tools/i8x_debug.py, 20..27 of 40 runs of 600 tiles; none with plain v_fma_f32) */
    auto rotate = [](float &u, float &v, float c, float s) __attribute__((always_inline)) {
        const float x = __builtin_fmaf(-v, s, u * c), y = __builtin_fmaf(v, c, u * s);
        u = x;
        v = y;
    };
    auto put_f2 = [&](float2 *p, float x, float y) __attribute__((always_inline)) {
        if (LAYOUT == 0 && NCH == 1) {
            const f32x2 v = { x, y };
            __builtin_nontemporal_store(v, reinterpret_cast<f32x2 *>(p));
        } else
            store_f2_padded(p, x, y);
    };
    /* outputs pt + STRIDE o4 (o4 = 0 .. COUNT) of tile t from their values in `arr`: combine, rotate, store (NPT finishing
     * threads: STRIDE = NPT, COUNT = 1024 / NPT; the bank's matrix waves: their own outputs, STRIDE = 64) */
    auto post_store = [&](long long t, const float *arr, int pt, auto guard_c, auto stride_c, auto count_c) __attribute__((always_inline)) {
        constexpr bool GUARD = decltype(guard_c)::value;
        constexpr int STRIDE = decltype(stride_c)::value, COUNT = decltype(count_c)::value;
        float2 *dst = reinterpret_cast<float2 *>(a.out) + t * 1024;
        const long long left = n_out - t * 1024;
#pragma unroll
        for (int o4 = 0; o4 < COUNT; ++o4) {
            const int o = pt + STRIDE * o4;
            const int q = 20 * (o >> 4) + (o & 15);
            float uI, uQ;
            if (MODE == 1) {
                uI = (arr[q] - arr[3 * AS + q]) + a.ct[0];
                uQ = (arr[2 * AS + q] + arr[AS + q]) + a.ct[1];
            } else {
                uI = arr[q];
                uQ = arr[AS + q];
            }
            if (MIX) {
                float c, s;
                nco_lo((n0lo + (uint32_t)D * (uint32_t)(t * 1024 + o)) * a.freg + a.phase_off, c, s);
                rotate(uI, uQ, c, s);
            }
            if (!GUARD || o < left)
                put_f2(dst + o, uI, uQ);
        }
    };
    /* second stage, output p of the tile from u[8 p - 64 .. 8 p] (array positions 8 p .. 8 p + 64 behind the porch); the tap
     * tables are in descending order, gre[i] = Re g2[64 - i], so that a float4 of u meets a float4 of taps.
     * WHOLE: one thread forms the complex output.  Otherwise a PAIR of neighbouring lanes forms it: lane `comp` = 0 the real
     * part gr * uI - gi * uQ, lane 1 the imaginary part gr * uQ + gi * uI (the same code on swapped rails), one quad
     * permute brings the halves together for the rotation, and each lane stores its own float.                        */
    auto post_stage2 = [&](long long t, const float *arr, int p) __attribute__((always_inline)) {
        constexpr bool WHOLE = true;
        const float *uA = arr, *uB = arr + AS;
        const f32x2 PDDC_CONSTANT *gre = (const f32x2 PDDC_CONSTANT *)a.taps2;
        const f32x2 PDDC_CONSTANT *gim = (const f32x2 PDDC_CONSTANT *)(a.taps2 + kTaps2Len);
        /* Packed fp32 only where the wave that runs this issues the matrix instructions itself (LAYOUT 0).  The finishing
         * waves of LAYOUT 2 take ONE float per instruction, like the loaders of LAYOUT 1: that they have no matrix wave on
         * their SIMD rests on waves w, w + 4, w + 8 sharing one (tools/ubench/wave_simd.hip) -- measured, not guaranteed
         * (round 5 advisor) -- and packed fp32 beside a matrix wave is the code shape that delivered wrong lanes 48..63
         * (`rotate` above).  The same four partial sums in the same order: the same bits either way.                     */
        constexpr bool PK = LAYOUT == 0;
        f32x2 ra_[2] = { { 0.f, 0.f }, { 0.f, 0.f } }, ib_[2] = { { 0.f, 0.f }, { 0.f, 0.f } };
        f32x2 ia_[2] = { { 0.f, 0.f }, { 0.f, 0.f } }, rb_[2] = { { 0.f, 0.f }, { 0.f, 0.f } };
        float sra[4] = { 0.f, 0.f, 0.f, 0.f }, srb[4] = { 0.f, 0.f, 0.f, 0.f }, sia[4] = { 0.f, 0.f, 0.f, 0.f },
              sib[4] = { 0.f, 0.f, 0.f, 0.f };
        const float PDDC_CONSTANT *gref = (const float PDDC_CONSTANT *)a.taps2;
        const float PDDC_CONSTANT *gimf = (const float PDDC_CONSTANT *)(a.taps2 + kTaps2Len);
        /* (hipcc waits for every float4 pair: sixteen exposed LDS latencies, 4200 cycles per tile on the clock probe -- the
         * reason why LAYOUT 1 gives this work to waves that can keep the reads in flight) */
        constexpr int S2B = LAYOUT == 2 ? 8 : 1;  /* (matrix waves: no registers for more -- batches of 4 spill 12, of 8 47) */
#pragma unroll
        for (int jb = 0; jb < 16; jb += S2B) {
            float4 xA[S2B], xB[S2B];
#pragma unroll
            for (int jj = 0; jj < S2B; ++jj) {
                const int op = 8 * p + 4 * (jb + jj), q = 20 * (op >> 4) + (op & 15);
                xA[jj] = *reinterpret_cast<const float4 *>(uA + q);
                xB[jj] = *reinterpret_cast<const float4 *>(uB + q);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int jj = 0; jj < S2B; ++jj) {
                const int j = jb + jj;
                if (PK) {
                    const f32x2 xa[2] = { { xA[jj].x, xA[jj].y }, { xA[jj].z, xA[jj].w } },
                                xb[2] = { { xB[jj].x, xB[jj].y }, { xB[jj].z, xB[jj].w } };
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const f32x2 gr = gre[2 * j + e];
                        ra_[e] = __builtin_elementwise_fma(gr, xa[e], ra_[e]);
                        if (WHOLE)
                            rb_[e] = __builtin_elementwise_fma(gr, xb[e], rb_[e]);
                        if (MIX) {
                            const f32x2 gi = gim[2 * j + e];
                            ib_[e] = __builtin_elementwise_fma(gi, xb[e], ib_[e]);
                            if (WHOLE)
                                ia_[e] = __builtin_elementwise_fma(gi, xa[e], ia_[e]);
                        }
                    }
                } else {
                    const float *xa = &xA[jj].x, *xb = &xB[jj].x;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float gr = gref[4 * j + e];
                        sra[e] = __builtin_fmaf(gr, xa[e], sra[e]);
                        srb[e] = __builtin_fmaf(gr, xb[e], srb[e]);
                        if (MIX) {
                            const float gi = gimf[4 * j + e];
                            sib[e] = __builtin_fmaf(gi, xb[e], sib[e]);
                            sia[e] = __builtin_fmaf(gi, xa[e], sia[e]);
                        }
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!PK) {
            ra_[0] = f32x2{ sra[0], sra[1] };
            ra_[1] = f32x2{ sra[2], sra[3] };
            rb_[0] = f32x2{ srb[0], srb[1] };
            rb_[1] = f32x2{ srb[2], srb[3] };
            ia_[0] = f32x2{ sia[0], sia[1] };
            ia_[1] = f32x2{ sia[2], sia[3] };
            ib_[0] = f32x2{ sib[0], sib[1] };
            ib_[1] = f32x2{ sib[2], sib[3] };
        }
        const int op = 8 * p + 64, q = 20 * (op >> 4) + (op & 15);
        const float g0r = a.taps2[64], g0i = a.taps2[kTaps2Len + 64];
        const float x0A = uA[q], x0B = uB[q];
        const uint32_t ph = (n0lo + 64u * (uint32_t)(t * 128 + p)) * a.freg + a.phase_off;
        if (WHOLE) {
            float zr = ((ra_[0].x + ra_[0].y) + (ra_[1].x + ra_[1].y)) + g0r * x0A;
            float zi = ((rb_[0].x + rb_[0].y) + (rb_[1].x + rb_[1].y)) + g0r * x0B;
            if (MIX) {
                zr -= ((ib_[0].x + ib_[0].y) + (ib_[1].x + ib_[1].y)) + g0i * x0B;
                zi += ((ia_[0].x + ia_[0].y) + (ia_[1].x + ia_[1].y)) + g0i * x0A;
                float c, s;
                nco_lo(ph, c, s);
                const float yr = zr * c - zi * s, yi = zr * s + zi * c;
                zr = yr;
                zi = yi;
            }
            put_f2(reinterpret_cast<float2 *>(a.out) + t * 128 + p, zr, zi);
        }
    };
    /* the same output by a PAIR of neighbouring loader lanes (LAYOUT 1): lane `comp` = 0 the real part gr * uI - gi * uQ,
     * lane 1 the imaginary part gr * uQ + gi * uI -- the same code on swapped rails --, scalar FMAs (see rotate()), the
     * window's LDS reads in batches that are in flight before the first FMA (these waves have the registers the matrix waves
     * lack), one quad permute brings the halves together for the rotation, each lane stores its own float.  A wave takes
     * outputs of ONE parity (B: p = 2 (32 h + i) + B for lane pair i of wave 2 h + B): the window of output p starts at
     * array position 8 p = 16 a + 8 B, so with the parity fixed every read is the lane's base 20 a plus a constant (the 16
     * values of a block lie 20 floats apart), and the taps stay wave-uniform (scalar loads).                           */
    auto post_stage2_pair = [&](long long t, const float *arr, int h, int lane_, auto parity_c) __attribute__((always_inline)) {
        constexpr int B = decltype(parity_c)::value;
        const int comp = lane_ & 1, ap = 32 * h + (lane_ >> 1), p = 2 * ap + B;
        const float *uA = arr + comp * AS + 20 * ap, *uB = arr + (comp ^ 1) * AS + 20 * ap;
        const float PDDC_CONSTANT *gre = (const float PDDC_CONSTANT *)a.taps2;
        const float PDDC_CONSTANT *gim = (const float PDDC_CONSTANT *)(a.taps2 + kTaps2Len);
        float s1[4] = { 0.f, 0.f, 0.f, 0.f }, s2[4] = { 0.f, 0.f, 0.f, 0.f };
        constexpr int NB = 4;
#pragma unroll
        for (int jb = 0; jb < 16; jb += NB) {
            float4 xA[NB], xB[NB];
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                constexpr int dummy = 0;
                (void)dummy;
                const int m = jb + jj + 2 * B, q = 4 * m + 4 * (m >> 2);          /* float4 m of the lane's blocks */
                xA[jj] = *reinterpret_cast<const float4 *>(uA + q);
                if (MIX)
                    xB[jj] = *reinterpret_cast<const float4 *>(uB + q);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int i = 4 * (jb + jj);
                const float *xa = &xA[jj].x, *xb = &xB[jj].x;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s1[e] = __builtin_fmaf(gre[i + e], xa[e], s1[e]);
                    if (MIX)
                        s2[e] = __builtin_fmaf(gim[i + e], xb[e], s2[e]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        constexpr int ml = 16 + 2 * B, ql = 4 * ml + 4 * (ml >> 2);
        float z = ((s1[0] + s1[1]) + (s1[2] + s1[3])) + gre[64] * uA[ql];
        if (MIX) {
            const float w = ((s2[0] + s2[1]) + (s2[2] + s2[3])) + gim[64] * uB[ql];
            z = comp ? z + w : z - w;
            const float other = __builtin_bit_cast(
                float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, z), 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, true));
            const float zr = comp ? other : z, zi = comp ? z : other;
            float c, s;
            nco_lo((n0lo + 64u * (uint32_t)(t * 128 + p)) * a.freg + a.phase_off, c, s);
            z = comp ? __builtin_fmaf(zi, c, zr * s) : __builtin_fmaf(-zi, s, zr * c);
        }
        float *dst = a.out + 2 * (t * 128 + p) + comp;
        asm volatile("global_store_dword %0, %1, off nt\n\ts_nop 1" ::"v"(dst), "v"(z) : "memory");
    };
    auto post_porch = [&](long long t, const float *arr, float *other, int c, bool chain, auto guard_c) __attribute__((always_inline)) {
        constexpr bool GUARD = decltype(guard_c)::value;
        const int comp = c >> 6, e = c & 63;
        const int qs = 20 * (64 + (e >> 4)) + (e & 15), qd = 20 * (e >> 4) + (e & 15);
        if (chain)                                           /* inside a chunk the tile's last 64 values are the next one's porch */
            other[comp * AS + qd] = arr[comp * AS + qs];
        if (GUARD && t == ntiles - 1 && a.hist2_out && comp == 0) {
            /* ... and the batch's last 64 the next call's second-stage history: mixed floats, y = u LO */
            float uI = arr[qs], uQ = arr[AS + qs];
            if (MIX) {
                float c, s;
                nco_lo((n0lo + 8u * (uint32_t)(t * 1024 + 960 + e)) * a.freg + a.phase_off, c, s);
                rotate(uI, uQ, c, s);
            }
            put_f2(static_cast<float2 *>(a.hist2_out) + e, uI, uQ);
        }
    };
    /* `next_first`: the tile behind t starts a chunk (it makes its own porch, or takes the stream's history); pt: the
     * finishing thread, 0 .. NPT */
    auto post = [&](long long t, float *arr, float *other, bool next_first, int pt, auto guard_c) __attribute__((always_inline)) {
        const int pw = __builtin_amdgcn_readfirstlane(pt >> 6);
        if (!FUSE2) {
            post_store(t, arr, pt, guard_c, std::integral_constant<int, NPT>{}, std::integral_constant<int, 1024 / NPT>{});
        } else if (LAYOUT == 0) {
            if (pw < 2)
                post_stage2(t, arr, pt);
            else
                post_porch(t, arr, other, pt - 128, !next_first, guard_c);
        } else if (LAYOUT == 2) {
            post_stage2(t, arr, pt);
            post_porch(t, arr, other, pt, !next_first, guard_c);
        } else {
            if (pw < 4) {
                if (pw & 1)
                    post_stage2_pair(t, arr, pw >> 1, pt & 63, std::integral_constant<int, 1>{});
                else
                    post_stage2_pair(t, arr, pw >> 1, pt & 63, std::integral_constant<int, 0>{});
            }
            else if (pw < 6)
                post_porch(t, arr, other, pt - 256, !next_first, guard_c);
        }
    };
    if (wave >= 4) {
        /* ---- loaders (waves 4..11): main groups two tiles ahead in two register sets, front groups one tile ahead of their
         * conversion in a third;
         * LAYOUT 1: they also finish the tile before the one the matrix waves are working on */
        const int lt = tid - 256;
        if (blk == 0 && a.hist_out) {             /* the next call's history: the batch's last HIST (hist_len) samples */
            const int hl = a.hist_len ? a.hist_len : HIST;
            const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(a.in) + (a.n_in - hl) * 6);
            if (lt < hl * 6 / 16)
                static_cast<uint4 *>(a.hist_out)[lt] = src[lt];
        }
        /* front groups a chunk's first tile t needs: all FG with the porch columns (FUSE2, t > 0), else the last HG */
        auto front_lo = [&](long long t) __attribute__((always_inline)) { return FUSE2 && t > 0 ? 0 : G::FG - G::HG; };
        uint4 ra[NQ][3], rb[NQ][3], rf[3];
        Cursor c0 = cur, c1 = wk.next(c0), c2 = wk.next(c1);
        long long t = wk.tile(c0), t1 = wk.tile(c1), t2 = wk.tile(c2), tp = -1;
        /* (the last round of a tile whose groups are no multiple of the loader threads: every lane LOADS -- its group lies
         * behind the descriptor's range and costs no traffic --, only the lanes with a group convert) */
        auto has = [&](int q) __attribute__((always_inline)) { return !PART || q < NQ - 1 || lt + NLT * q < NGRP; };
        /* this lane's main groups: their bytes in a tile's descriptor, and their positions in the two plane sets -- kept in
         * registers (the second set's planes lie beyond the LDS store's 16-bit offset field: from one base per set every
         * plane is a constant offset, from one base for both the compiler adds the rest again in front of every store) */
        int voff[NQ];
        uint32_t at0[NQ], at1[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            voff[q] = 48 * (lt + NLT * q);
            at0[q] = (uint32_t)swz(FRONT + 8 * (lt + NLT * q));
            at1[q] = at0[q] + 6 * PLANE;
            asm volatile("" : "+v"(at0[q]), "+v"(at1[q]));
        }
        const bool front_wave = wave < 4 + (G::FG + 63) / 64;        /* (uniform) the loader waves that hold front lanes */
        {
            const __amdgpu_buffer_rsrc_t rs = group_rsrc<TILE_S, NGRP>(a, t), rs1 = group_rsrc<TILE_S, NGRP>(a, t1);
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                issue_group(rs, voff[q], ra[q]);
            if (lt < G::FG && lt >= front_lo(t)) {
                issue_front<HIST, FRONT, TILE_S>(a, t, lt, rf);
                put_planes(rf, lds_i8x + swz(8 * lt), PLANE);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (has(q))
                    put_planes(ra[q], lds_i8x + at0[q], PLANE);
            if (front_wave)
                issue_group(front_rsrc<FRONT, TILE_S>(a, t1, c1.k == 0), 48 * lt, rf);
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                issue_group(rs1, voff[q], ra[q]);
        }
        __syncthreads();
        /* one step: tile `tn` > 0 (already in `cur_r`) goes into plane set `dst` (this lane's positions in it: `at`) while the
         * matrix waves work on `src`; the loads of the tile after it (`tnn`; no tile: a descriptor without records) go out
         * group by group BETWEEN the conversions (k_fir_i8's pacing), all of them unconditional, each once the group before
         * it has landed (loads_landed): a group is in flight while the group before it is converted.  The front groups of a
         * chunk's first tile (C = 1: every tile) lie in the batch, tile 0 being a prologue's: a descriptor of their own,
         * without records inside a chunk, loaded by every lane of the first loader wave(s) -- tn's were requested at the
         * start of the step before (same box, same build otherwise: requested and converted inside one step, as until round
         * 26, 0.3189 ms against 0.3011) and are converted first; tnn's follow */
        auto step = [&](long long tn, bool tn_first, long long tnn, bool tnn_first, uint4 (&nxt)[NQ][3], const uint4 (&cur_r)[NQ][3],
                        auto set_c) {
            /* the plane set tn goes into (0 / 1): its base, the other set's, and this lane's main-group positions in it */
            constexpr int SET = decltype(set_c)::value;
            uint8_t *const dst = lds_i8x + SET * 6 * PLANE;
            const uint8_t *const src = lds_i8x + (SET ^ 1) * 6 * PLANE;
            const uint32_t(&at)[NQ] = SET ? at1 : at0;
            const bool ff = tn_first && lt < G::FG;
            if (ff) {
                put_planes(rf, dst + swz(8 * lt), PLANE);
            } else if (!tn_first && lt < G::HG) {
                /* inside a chunk: the history comes over from the plane set of the tile before */
                const int s_at = swz(FRONT + TILE_S - HIST + 8 * lt), d_at = swz(EXTRA + 8 * lt);
#pragma unroll
                for (int pl = 0; pl < 6; ++pl)
                    *reinterpret_cast<uint2 *>(dst + pl * PLANE + d_at) = *reinterpret_cast<const uint2 *>(src + pl * PLANE + s_at);
            }
            if (front_wave)
                issue_group(front_rsrc<FRONT, TILE_S>(a, tnn, tnn_first), 48 * lt, rf);
            const __amdgpu_buffer_rsrc_t rs = group_rsrc<TILE_S, NGRP>(a, tnn);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                /* (decimate by 10, three rounds of groups, the last half empty: no wait in front of the step's FIRST issue --
                 * with it the form's 2^26-sample batches took 0.0857-0.0864 ms against 0.0809-0.0816 without and 0.0822-0.0825
                 * before round 26; the decimate-by-8 forms were measured with it) */
                if (D == 8 || q >= 1)
                    loads_landed();
                issue_group(rs, voff[q], nxt[q]);
                __builtin_amdgcn_sched_barrier(0);
                if (has(q))
                    put_planes(cur_r[q], lds_i8x + at[q], PLANE);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        float *arr0 = arr_base, *arr1 = arr_base + NARR * AS;
        int lastbuf;
        for (;;) {
            /* the matrix waves compute tile t from plane set 0 into value set 0; t1 (in ra) goes to plane set 1, t2 starts
             * towards rb; the tile before t (values in set 1) is finished */
            if (t1 >= 0)
                step(t1, c1.k == 0, t2, c2.k == 0, rb, ra, std::integral_constant<int, 1>{});
            if (LAYOUT == 1 && tp >= 0)
                post(tp, arr1, arr0, c0.k == 0, lt, std::false_type{});
            __syncthreads();
            lastbuf = 0;
            if (t1 < 0)
                break;
            tp = t;
            c0 = c1;
            c1 = c2;
            c2 = wk.next(c2);
            t = t1;
            t1 = t2;
            t2 = wk.tile(c2);
            if (t1 >= 0)
                step(t1, c1.k == 0, t2, c2.k == 0, ra, rb, std::integral_constant<int, 0>{});
            if (LAYOUT == 1)
                post(tp, arr0, arr1, c0.k == 0, lt, std::false_type{});
            __syncthreads();
            lastbuf = 1;
            if (t1 < 0)
                break;
            tp = t;
            c0 = c1;
            c1 = c2;
            c2 = wk.next(c2);
            t = t1;
            t1 = t2;
            t2 = wk.tile(c2);
        }
        if (LAYOUT == 1)
            post(t, lastbuf ? arr1 : arr0, lastbuf ? arr0 : arr1, true, lt, std::true_type{});
        return;
    }
    if (LAYOUT == 2 && wave >= 2) {
        /* ---- finishing waves (LAYOUT 2): tile t - 1 is finished while the matrix waves work on tile t */
        const int pt = tid - 128;
        if (FUSE2 && blk == 0 && pt < 64) {
            /* the batch's first tile: the stream's second-stage history -- the 64 first-stage outputs in front of this batch,
             * mixed floats -- taken back into the frame of this call's u values: u = y conj(LO) */
            const float2 y = static_cast<const float2 *>(a.hist2)[pt];
            float uI = y.x, uQ = y.y;
            if (MIX) {
                float c, s;
                nco_lo((n0lo + 8u * (uint32_t)(pt - 64)) * a.freg + a.phase_off, c, s);
                uI = y.x * c + y.y * s;
                uQ = y.y * c - y.x * s;
            }
            const int q = 20 * (pt >> 4) + (pt & 15);
            arr_base[q] = uI;
            arr_base[AS + q] = uQ;
        }
        __syncthreads();
        int buf = 0;
        long long t = wk.tile(cur), tprev = -1;
        while (t >= 0) {
            const bool first = cur.k == 0;
            cur = wk.next(cur);
            if (tprev >= 0)
                post(tprev, arr_base + (buf ^ 1) * NARR * AS, arr_base + buf * NARR * AS, first, pt, std::false_type{});
            __syncthreads();
            tprev = t;
            t = wk.tile(cur);
            buf ^= 1;
        }
        post(tprev, arr_base + (buf ^ 1) * NARR * AS, arr_base + buf * NARR * AS, true, pt, std::true_type{});
        return;
    }
    /* ---- matrix waves (0..3; LAYOUT 2: 0 and 1, both halves of the columns each) */
    const int w0 = wave & 1, half = wave >> 1;
    const int n = lane & 15, kq = lane >> 4;
    const v4i_t *atab = static_cast<const v4i_t *>(a.atab);
    /* tap operand(s): mode 0 the one table; mode 1 table w0 (c or s); mode 2 both paired tables -- [c ; s] meets the I planes,
     * [-s ; c] the Q planes */
    v4i_t A0[KSTEPS][4];
    v4i_t A1[MODE == 2 ? KSTEPS : 1][4];
    if (MODE == 0 && a.taps16 != nullptr) {                 /* uniform */
        /* binary16 tap storage: this lane's 16 columns of every k-step, quantised here exactly as build_tables_core does on
         * the host (H = llround(h 2^E), four balanced base-256 digits).  The device array is laid out for this read:
         * G[128 + tt] = h[HIST - tt] for tt = 1 .. HIST, zeros around it (kFirI8Taps16Len entries), so that the 16 values of
         * a k-step -- T[r][c] = G[128 + c - 8 r] -- are two aligned 16-byte loads */
        const uint4 *g16 = static_cast<const uint4 *>(a.taps16);
        const float two_e = a.two_e;                        /* a power of two: h 2^E is exact in binary32 */
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int i0 = (128 + 64 * ks + 16 * kq - 8 * n) >> 3;      /* in units of 8 values */
            const uint4 lo = g16[i0], hi = g16[i0 + 1];
            const uint32_t hw[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
            int w[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                w[0][q] = w[1][q] = w[2][q] = w[3][q] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int jj = 4 * q + b;
                    const uint32_t bits = (jj & 1) ? hw[jj >> 1] >> 16 : hw[jj >> 1] & 0xffffu;
                    _Float16 hv;
                    const uint16_t b16 = (uint16_t)bits;
                    __builtin_memcpy(&hv, &b16, 2);
                    const float x = (float)hv * two_e;
                    int r = (int)(x + __builtin_copysignf(0.5f, x));   /* llround: exact, |x| <= 2^30 and 11 bits wide */
                    /* balanced digits: d = the low byte, signed; what is left is (r - d) / 256 = (r + 128) >> 8.  Byte b of
                     * plane j's word takes the low byte as it is (one v_perm_b32) */
                    const uint32_t sel = 0x03020100u ^ ((0x04u ^ (uint32_t)b) << (8 * b));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        w[j][q] = (int)__builtin_amdgcn_perm((uint32_t)r, (uint32_t)w[j][q], sel);
                        r = (r + 128) >> 8;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                A0[ks][j] = v4i_t{ w[j][0], w[j][1], w[j][2], w[j][3] };
        }
    } else {
        const int tab0 = MODE == 1 ? w0 : 0;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                A0[ks][j] = atab[tab0 * G::TABV + (j * KSTEPS + ks) * 64 + lane];
                if (MODE == 2)
                    A1[ks][j] = atab[G::TABV + (j * KSTEPS + ks) * 64 + lane];
            }
    }
    if (LAYOUT != 2 && FUSE2 && blk == 0 && tid < 64) {
        /* the batch's first tile: the stream's second-stage history -- the 64 first-stage outputs in front of this batch,
         * mixed floats -- taken back into the frame of this call's u values: u = y conj(LO) */
        const float2 y = static_cast<const float2 *>(a.hist2)[tid];
        float uI = y.x, uQ = y.y;
        if (MIX) {
            float c, s;
            nco_lo((n0lo + 8u * (uint32_t)(tid - 64)) * a.freg + a.phase_off, c, s);
            uI = y.x * c + y.y * s;
            uQ = y.y * c - y.x * s;
        }
        const int q = 20 * (tid >> 4) + (tid & 15);
        arr_base[q] = uI;
        arr_base[AS + q] = uQ;
    }
    /* one band pass of this wave over 16 columns whose operand bytes start at plane position `pos` (per lane: + 16 kq + 64 ks) */
    auto band = [&](const uint8_t *pb, int pos, float *dst) __attribute__((always_inline)) {
        if (MODE == 1) {
#pragma unroll
            for (int comp = 0; comp < 2; ++comp) {
                v4i_t acc[4];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc[s] = v4i_t{ 0, 0, 0, 0 };
                /* The operand reads run ONE k-step ahead of the matrix instructions that use them, in two register sets:
                 * hipcc left to itself issues a k-step's reads three or four matrix instructions (50-60 cycles) before their
                 * first use and waits -- the 216 matrix instructions of a tile filled 57 % of these waves' 6000 ticks of work
                 * (clock probe, NOTEBOOK R5.7), and these waves are the chain the block waits for in this form */
                constexpr bool PF1 = LAYOUT == 1;               /* (the form's default layout; the others have no registers left) */
                v4i_t B[PF1 ? 2 : 1][3];
                auto read_b1 = [&](int ks, v4i_t (&b)[3]) __attribute__((always_inline)) {
                    const int at = swz(pos + 64 * ks);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        b[i] = *reinterpret_cast<const v4i_t *>(pb + (3 * comp + i) * PLANE + at);
                };
                if (PF1)
                    read_b1(0, B[0]);
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    if (!PF1)
                        read_b1(ks, B[0]);
                    else if (ks + 1 < KSTEPS)
                        read_b1(ks + 1, B[(ks + 1) & 1]);
                    if (PF1)
                        __builtin_amdgcn_sched_barrier(0);
                    const v4i_t(&b)[3] = B[PF1 ? ks & 1 : 0];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (i + j >= 2)
                                acc[i + j - 2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0[ks][j], b[i], acc[i + j - 2], 0, 0, 0);
                    if (PF1)
                        __builtin_amdgcn_sched_barrier(0);
                }
                float4 y;
                float *yp = &y.x;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    yp[v] = recombine(acc, v) * a.scale;
                *reinterpret_cast<float4 *>(dst + (2 * w0 + comp) * AS) = y;
            }
        } else {
            v4i_t acc[4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[s] = v4i_t{ 0, 0, 0, 0 };
            /* (operand reads one k-step ahead of their matrix instructions, two register sets: see mode 1 above) -- for the long
             * untuned first stage only (six k-steps: there these waves' chain is what the block waits for, 255 taps 0.3451 ->
             * 0.3369 ms).  Where the loaders are the longer chain the pinned order costs 2 % (two-k-step tuned form 0.3260 ->
             * 0.3320), and the three-k-step tuned form has no registers for a second set (profiles/r05/f_ab_operand_prefetch.txt) */
            constexpr bool PF = MODE == 0 && KSTEPS > 4 && !FUSE2;
            if (PF) {
                v4i_t B[2][3];
                auto read_b = [&](int ks, v4i_t (&b)[3]) __attribute__((always_inline)) {
                    const int at = swz(pos + 64 * ks);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        b[i] = *reinterpret_cast<const v4i_t *>(pb + (3 * w0 + i) * PLANE + at);
                };
                read_b(0, B[0]);
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    if (ks + 1 < KSTEPS)
                        read_b(ks + 1, B[(ks + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (i + j >= 2)
                                acc[i + j - 2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0[ks][j], B[ks & 1][i], acc[i + j - 2], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const int at = swz(pos + 64 * ks);
                if (MODE == 0) {
                    v4i_t B[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        B[i] = *reinterpret_cast<const v4i_t *>(pb + (3 * w0 + i) * PLANE + at);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (i + j >= 2)
                                acc[i + j - 2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0[ks][j], B[i], acc[i + j - 2], 0, 0, 0);
                } else {
                    v4i_t BI[3], BQ[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        BI[i] = *reinterpret_cast<const v4i_t *>(pb + i * PLANE + at);
                        BQ[i] = *reinterpret_cast<const v4i_t *>(pb + (3 + i) * PLANE + at);
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (i + j >= 2) {
                                acc[i + j - 2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0[ks][j], BI[i], acc[i + j - 2], 0, 0, 0);
                                acc[i + j - 2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1[MODE == 2 ? ks : 0][j], BQ[i], acc[i + j - 2], 0, 0, 0);
                            }
                }
            }
            }
            /* this lane: its column, rows 4 kq + v -> four consecutive values; mode 2: rows 0..7 are uI, rows 8..15 uQ of the
             * column's eight outputs */
            const int rail = MODE == 2 ? kq >> 1 : w0;
            float4 y;
            float *yp = &y.x;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                yp[v] = recombine(acc, v) * a.scale + (rail ? a.ct[1] : a.ct[0]);
            *reinterpret_cast<float4 *>(dst + rail * AS) = y;
        }
    };
    __syncthreads();
    /* the bank: this wave's channel and its share of the columns (NCH = 1: the wave's share of the tile) */
    const int mw = NCH > 1 ? wave % (4 / NCH) : wave;
    float *const arr_ch = arr_base + (NCH > 1 ? wave / (4 / NCH) : 0) * NARR * AS;
    int buf = 0;
    long long t = wk.tile(cur);
    while (t >= 0) {
        const bool first = cur.k == 0;
        cur = wk.next(cur);
        const uint8_t *pb = lds_i8x + buf * 6 * PLANE;
        float *arr = NCH > 1 ? arr_ch : arr_base + buf * NARR * AS, *arr_o = arr_base + (buf ^ 1) * NARR * AS;
        if (MODE == 2) {
            /* columns of 8 outputs, 8 D = 64 (80) samples apart: 128 of them in a tile, 16 per pass; every matrix wave makes both rails.
             * Output o = 8 col + 4 (kq & 1) + v lies at array position o + PORCH. */
            constexpr int NMW = LAYOUT == 2 ? 2 : 4;
            constexpr int CPW = 8 / NMW * NCH;              /* column blocks per wave */
            if (FUSE2 && first && t > 0 && wave == NMW - 1) {
                /* a chunk's first tile computes its own porch: columns -8 .. -1 in lanes 8..15; the other lanes repeat column
                 * -8 (same operand bytes, same results, same address: the whole wave runs the matrix instructions) */
                const int colx = n < 8 ? -8 : n - 16, pp = 64 + 8 * colx + 4 * (kq & 1);
                band(pb, EXTRA + 8 * D * colx + 16 * kq, arr + 20 * (pp >> 4) + (pp & 15));
            }
#pragma unroll
            for (int cb = 0; cb < CPW; ++cb) {
                const int col = 16 * (CPW * mw + cb) + n, pp = PORCH + 8 * col + 4 * (kq & 1);
                band(pb, EXTRA + 8 * D * col + 16 * kq, arr + 20 * (pp >> 4) + (pp & 15));
            }
        } else {
        if (FUSE2 && first && t > 0 && (LAYOUT == 2 || half == 1)) {
            /* a chunk's first tile computes its own porch: columns -4 .. -1 in lanes 12..15; the other lanes repeat column -4
             * (same operand bytes, same results, same address: the whole wave runs the matrix instructions) */
            const int colx = n < 12 ? -4 : n - 16;
            band(pb, EXTRA + 128 * colx + 16 * kq, arr + 20 * (colx + 4) + 4 * kq);
        }
#pragma unroll
        for (int cb = 0; cb < (LAYOUT == 2 ? 4 : 2); ++cb) {
            const int col = 16 * (LAYOUT == 2 ? cb : 2 * half + cb) + n;
            band(pb, EXTRA + 128 * col + 16 * kq, arr + 20 * (col + PORCH / 16) + 4 * kq);
        }
        }
        __syncthreads();                 /* ONE barrier per tile: the next tile's planes are written, this tile's values are in LDS */
        if (NCH > 1) {                   /* the bank: this wave's own 256 NCH outputs of its channel, 64 consecutive per store */
            /* (in rounds of 256 outputs, not unrolled: sixteen outputs' addresses and phases at once do not fit beside the
             * tables) */
#pragma unroll 1
            for (int h = 0; h < NCH; ++h)
                post_store(t, arr, 256 * (NCH * mw + h) + lane, std::true_type{}, std::integral_constant<int, 64>{},
                           std::integral_constant<int, 4>{});
            /* (the next tile's values go to the same array: the LDS unit keeps one wave's accesses in order, this keeps the
             * compiler from moving them) */
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        } else if (LAYOUT == 0) {        /* ... and these waves finish it themselves */
            post(t, arr, arr_o, cur.k == 0, tid, std::true_type{});
        }
        t = wk.tile(cur);
        buf ^= 1;
    }
}

template <int HIST, int MODE, bool FUSE2, int LAYOUT, int D = 8>
__global__ __launch_bounds__(768, 1) void k_fir_i8x(FirI8xArgs a, long long ntiles, int C)
{
    fir_i8x_block<HIST, MODE, FUSE2, LAYOUT, D>(a, ntiles, C, (long long)gridDim.x, (long long)blockIdx.x);
}

/* several streams, one launch (the gang: receivers that share a GPU): blockIdx.y is the stream, every record its own --
 * buffers, history, tuning word, tap tables; the same block body, so the same bits as a launch of its own */
template <int HIST, int MODE, bool FUSE2, int LAYOUT>
__global__ __launch_bounds__(768, 1) void k_fir_i8x_many(FirI8xMany m, long long ntiles, int C)
{
    /* this stream's record, field by field through the scalar cache (indexing the by-value array puts a copy on the stack) */
    const FirI8xArgs PDDC_CONSTANT &r = ((const FirI8xArgs PDDC_CONSTANT *)__builtin_amdgcn_kernarg_segment_ptr())[blockIdx.y];
    (void)m;
    FirI8xArgs a;
    a.in = r.in;
    a.hist = r.hist;
    a.hist_out = r.hist_out;
    a.out = r.out;
    a.atab = r.atab;
    a.n_in = r.n_in;
    a.scale = r.scale;
    a.ct[0] = r.ct[0];
    a.ct[1] = r.ct[1];
    a.n0 = r.n0;
    a.freg = r.freg;
    a.phase_off = r.phase_off;
    a.taps2 = r.taps2;
    a.hist2 = r.hist2;
    a.hist2_out = r.hist2_out;
    a.taps16 = r.taps16;
    a.two_e = r.two_e;
    fir_i8x_block<HIST, MODE, FUSE2, LAYOUT>(a, ntiles, C, (long long)gridDim.x, (long long)blockIdx.x);
}

/* The channel bank (ddc_kernels.h FirI8xBank): NCH tuned first stages from one read of the input.  The loaders are
 * k_fir_i8x's, one plane set per tile for every channel; matrix wave w is channel w / (4 / NCH) over 2 NCH column blocks,
 * with that channel's tables resident (64 registers, as in the solo form) and finishes its own outputs (fir_i8x_block).
 * Which LDS option: the four channels' double-buffered value arrays (80 KB) do not fit beside the planes (109 KB); single
 * buffers do (40 KB), because each matrix wave reads back only what it wrote itself -- no wave waits for another's values,
 * and the tile keeps its ONE barrier.  Finishing straight from the accumulators would save the LDS round trip but needs
 * rows 0..7 (uI) and 8..15 (uQ) of a column brought together across lane halves, and a combine / rotation in another
 * order than the solo form's -- the outputs must be the solo form's bits, so the bank shares its finishing code instead.
 * D = 10 (the tuned decimate-by-10 form, hist 64, NCH = 2): the same scheme on k_fir_i8x's 10240-sample tiles; the two
 * channels share one decimation phase (in_off, n_out) and may differ in the history they keep (hist_len). */
template <int HIST, int NCH, int D = 8>
__global__ __launch_bounds__(768, 1) void k_fir_i8x_bank(FirI8xBank b, long long ntiles, int C)
{
    /* the record through the scalar cache, the channel by a wave-uniform index (see k_fir_i8x_many) */
    const FirI8xBank PDDC_CONSTANT &r = *(const FirI8xBank PDDC_CONSTANT *)__builtin_amdgcn_kernarg_segment_ptr();
    (void)b;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ch = wave < 4 ? wave / (4 / NCH) : 0;
    FirI8xArgs a;
    a.in = r.a.in;
    a.hist = r.a.hist;
    a.n_in = r.a.n_in;
    a.atab = r.ch[ch].atab;
    a.out = r.ch[ch].out;
    a.hist_out = r.ch[ch].hist_out;
    a.scale = r.ch[ch].scale;
    a.ct[0] = r.ch[ch].ct[0];
    a.ct[1] = r.ch[ch].ct[1];
    a.n0 = r.ch[ch].n0;
    a.freg = r.ch[ch].freg;
    a.phase_off = r.ch[ch].phase_off;
    if (D == 10) {
        /* decimate by 10: the group's one phase (every channel's windows end on in_off + 10 m, n_out of them), and the
         * loaders read channel 0's history -- the longest; the other channels' taps are zero where it reaches further */
        a.n_out = r.a.n_out;
        a.in_off = r.a.in_off;
        a.hist_len = r.ch[ch].hist_len;
    }
    if (blockIdx.x == 0 && wave >= 4) {
        /* the loaders write channel 0's next history (fir_i8x_block); the other channels get their own last samples here
         * (decimate by 8: the same HIST bytes; by 10: each its own hist_len) */
        const int lt = threadIdx.x - 256;
        const int hl = D == 8 ? HIST : r.ch[1].hist_len;              /* (decimate by 10: channel 1 is the only other) */
        const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(a.in) + (a.n_in - hl) * 6);
        for (int c = 1; c < NCH; ++c)
            if (r.ch[c].hist_out && lt < hl * 6 / 16)
                static_cast<uint4 *>(r.ch[c].hist_out)[lt] = src[lt];
    }
    fir_i8x_block<HIST, 2, false, 0, D, NCH>(a, ntiles, C, (long long)gridDim.x, (long long)blockIdx.x);
}

/* ---- host side: the tap operands ------------------------------------------------------------------------------------ */
/* H[k] (k = 0 .. hist-1, |H| <= 2^30) -> four planes of balanced base-256 digits in the matrix instruction's lane order:
 * lane l of k-step ks holds A[row l & 15][k = 16 (l >> 4) + jj], T[r][c] = H[hist - (c - 8 r)] */
static bool i8_fill_table(const long long *H, int hist, int8_t *table)
{
    std::vector<int8_t> dig(4 * (size_t)hist);
    for (int k = 0; k < hist; ++k) {
        long long r = H[k];
        for (int j = 0; j < 4; ++j) {
            const long long d = j == 3 ? r : ((r + 128) & 255) - 128;
            if (d < -128 || d > 127)
                return false;
            dig[(size_t)j * hist + k] = (int8_t)d;
            r = (r - d) / 256;
        }
    }
    const int ksteps = (120 + hist + 63) / 64;
    for (int j = 0; j < 4; ++j)
        for (int ks = 0; ks < ksteps; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int jj = 0; jj < 16; ++jj) {
                    const int r = l & 15, c = 64 * ks + 16 * (l >> 4) + jj, tt = c - 8 * r;
                    table[(((size_t)j * ksteps + ks) * 64 + l) * 16 + jj] =
                        (tt >= 1 && tt <= hist) ? dig[(size_t)j * hist + (hist - tt)] : 0;
                }
    return true;
}

/* mode 2: the same digits with the two tap sets of a row block in ONE operand -- rows 0..7 the band of `top` over eight
 * outputs, rows 8..15 the band of `bot` over the same eight: lane l of k-step ks holds A[row l & 15][k = 16 (l >> 4) + jj],
 * T[r][c] = H_(r >> 3)[hist - (c - 8 (r & 7))] */
static bool i8_fill_table_paired(const long long *top, const long long *bot, int hist, int8_t *table, int D = 8)
{
    std::vector<int8_t> dig(8 * (size_t)hist);
    for (int set = 0; set < 2; ++set)
        for (int k = 0; k < hist; ++k) {
            long long r = (set ? bot : top)[k];
            for (int j = 0; j < 4; ++j) {
                const long long d = j == 3 ? r : ((r + 128) & 255) - 128;
                if (d < -128 || d > 127)
                    return false;
                dig[((size_t)set * 4 + j) * hist + k] = (int8_t)d;
                r = (r - d) / 256;
            }
        }
    const int ksteps = (7 * D + hist + 63) / 64;
    for (int j = 0; j < 4; ++j)
        for (int ks = 0; ks < ksteps; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int jj = 0; jj < 16; ++jj) {
                    const int r = l & 15, c = 64 * ks + 16 * (l >> 4) + jj, tt = c - D * (r & 7);
                    table[(((size_t)j * ksteps + ks) * 64 + l) * 16 + jj] =
                        (tt >= 1 && tt <= hist) ? dig[((size_t)(r >> 3) * 4 + j) * hist + (hist - tt)] : 0;
                }
    return true;
}

int fir_i8x_mode(int hist, bool mix) { return !mix ? 0 : hist <= 128 ? 2 : 1; }

static int fir_i8x_ksteps(int hist, int mode) { return ((mode == 2 ? 56 : 120) + hist + 63) / 64; }

size_t fir_i8x_table_bytes(int hist, bool mix)
{
    const int mode = fir_i8x_mode(hist, mix), ksteps = fir_i8x_ksteps(hist, mode);
    return (size_t)(mode == 0 ? 1 : 2) * 4 * ksteps * 64 * 16;
}

static bool build_tables_core(const float *taps, int ntaps, int hist, bool mix, uint32_t freg, int8_t *tables, float *scale,
                              float ct[2], int *exp2, int D, int delay);

bool fir_i8x_build_tables(const float *taps, int ntaps, int hist, bool mix, uint32_t freg, int8_t *tables, float *scale,
                          float ct[2], int *exp2)
{
    return build_tables_core(taps, ntaps, hist, mix, freg, tables, scale, ct, exp2, 8, 0);
}

size_t fir_i8x_d10_table_bytes() { return (size_t)2 * 4 * ((70 + kFirI8xD10Hist + 63) / 64) * 64 * 16; }

bool fir_i8x_d10_build_tables(const float *taps, int ntaps, int delay, uint32_t freg, int8_t *tables, float *scale, float ct[2])
{
    return build_tables_core(taps, ntaps, kFirI8xD10Hist, true, freg, tables, scale, ct, nullptr, 10, delay);
}

/* taps h[0 .. ntaps) delayed by `delay` samples: g[k] = h[k - delay] e^{+j theta k} (D = 8: delay = 0) */
static bool build_tables_core(const float *taps, int ntaps, int hist, bool mix, uint32_t freg, int8_t *tables, float *scale,
                              float ct[2], int *exp2, int D, int delay)
{
    if (!taps || ntaps < 1 || (hist != 32 && hist != 64 && hist != 128 && hist != 256) || delay < 0 || ntaps + delay > hist || !tables)
        return false;
    if (D != 8 && !(D == 10 && mix && hist == kFirI8xD10Hist))
        return false;
    double hmax = 0.0;
    for (int k = 0; k < ntaps; ++k)
        hmax = std::fmax(hmax, std::fabs((double)taps[k]));
    if (!(hmax > 0.0) || !std::isfinite(hmax))
        return false;
    const int E = 30 - (int)std::ceil(std::log2(hmax));            /* |H| <= 2^30 for h, a fortiori for h cos, h sin */
    if (exp2)
        *exp2 = E;
    const int mode = fir_i8x_mode(hist, mix);
    const size_t tb = (size_t)4 * (D == 8 ? fir_i8x_ksteps(hist, mode) : (7 * D + hist + 63) / 64) * 64 * 16;
    /* sample = v24 / 8388607 (perseustest.c:466-502); planes 0 and 1 are stored minus 128: V = planes + 32896 */
    const double unit = std::ldexp(1.0, -E) / 8388607.0;
    *scale = (float)unit;
    std::vector<long long> Hc((size_t)hist, 0), Hs((size_t)hist, 0), Hm((size_t)hist, 0);
    long long sc = 0, ss = 0;
    const double w = 6.283185307179586476925286766559 / 4294967296.0;
    for (int kk = 0; kk < ntaps; ++kk) {
        const int k = kk + delay;
        const double hk = std::ldexp((double)taps[kk], E);
        if (mix) {
            const double th = w * (double)(uint32_t)((uint64_t)k * freg);
            Hc[k] = std::llround(hk * std::cos(th));
            Hs[k] = std::llround(hk * std::sin(th));
        } else {
            Hc[k] = std::llround(hk);
        }
        Hm[k] = -Hs[k];
        sc += Hc[k];
        ss += Hs[k];
    }
    if (mode == 2) {
        /* [c ; s] meets the I planes, [-s ; c] the Q planes, both into the same accumulators: rows 0..7 uI, rows 8..15 uQ */
        if (!i8_fill_table_paired(Hc.data(), Hs.data(), hist, tables, D) ||
            !i8_fill_table_paired(Hm.data(), Hc.data(), hist, tables + tb, D))
            return false;
    } else {
        if (!i8_fill_table(Hc.data(), hist, tables))
            return false;
        if (mix && !i8_fill_table(Hs.data(), hist, tables + tb))
            return false;
    }
    ct[0] = (float)((double)(sc - ss) * 32896.0 * unit);           /* uI = gc xI - gs xQ */
    ct[1] = (float)((double)(ss + sc) * 32896.0 * unit);           /* uQ = gs xI + gc xQ */
    return true;
}

void fir_i8x_taps2(const float *taps2, int ntaps2, bool mix, uint32_t freg, float *out)
{
    /* out[i] = Re g2[64 - i], out[kFirI8xTaps2Len / 2 + i] = Im g2[64 - i]; g2[k] = h2[k] e^{+j 8 theta k}: a first-stage
     * output is 8 input samples */
    for (int i = 0; i < kFirI8xTaps2Len; ++i)
        out[i] = 0.0f;
    const double w = 6.283185307179586476925286766559 / 4294967296.0;
    for (int k = 0; k < ntaps2 && k < 64; ++k) {
        double c = 1.0, s = 0.0;
        if (mix) {
            const double th = w * (double)(uint32_t)((uint64_t)(8 * k) * freg);
            c = std::cos(th);
            s = std::sin(th);
        }
        out[64 - k] = (float)((double)taps2[k] * c);
        out[kFirI8xTaps2Len / 2 + 64 - k] = (float)((double)taps2[k] * s);
    }
}

/* what every k_fir_i8x launcher does first: the device's CU count, looked up once per kernel (`cus` is that kernel's own
 * cache, per device), and the LDS attribute of its kernels set on the same occasion */
static hipError_t i8x_cus(int (&cus)[64], const void *k0, const void *k1, size_t lds, long long &ncu)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (cus[dev & 63] == 0) {
        int v = 0;
        hipError_t e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess)
            return e;
        for (const void *k : { k0, k1 })
            if (k && (e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
                return e;
        cus[dev & 63] = v > 0 ? v : 256;
    }
    ncu = cus[dev & 63];
    return hipSuccess;
}

/* the walk: chunks of C tiles (c_default unless asked) round at most nblk blocks, never more than a block's fair share,
 * so that every CU has work -> the grid and C */
static void i8x_walk(long long nblk, long long ntiles, int max_blocks, int chunk, long long c_default, long long &grid, long long &C)
{
    if (max_blocks > 0 && nblk > max_blocks)
        nblk = max_blocks;
    C = chunk > 0 ? chunk : c_default;
    if (C > (ntiles + nblk - 1) / nblk)
        C = (ntiles + nblk - 1) / nblk;
    const long long nchunks = (ntiles + C - 1) / C;
    grid = nchunks < nblk ? nchunks : nblk;
}

template <int HIST, int MODE, bool FUSE2, int LAYOUT, int D = 8>
static hipError_t launch_fir_i8x_l(const FirI8xArgs &a, int max_blocks, int chunk, hipStream_t s, const FirI8xMany *many = nullptr,
                                   int nmany = 0)
{
    using G = i8x::Geo<HIST, MODE, FUSE2, D>;
    const long long ntiles = D == 8 ? (a.n_in + i8x::TILE - 1) / i8x::TILE : (a.n_out + 1023) / 1024;
    static int cus[64] = { 0 };
    long long nblk = 0, grid = 0, C = 0;
    const hipError_t e = i8x_cus(cus, reinterpret_cast<const void *>(&k_fir_i8x<HIST, MODE, FUSE2, LAYOUT, D>),
                                 D == 8 ? reinterpret_cast<const void *>(&k_fir_i8x_many<HIST, MODE, FUSE2, LAYOUT>) : nullptr,
                                 G::LDS_BYTES, nblk);
    if (e != hipSuccess)
        return e;
    /* chunks of C tiles go round the blocks: C = 1 (tile-interleaved) unless asked otherwise */
    if (many && nmany > 1)
        nblk = (nblk + nmany - 1) / nmany;        /* the streams of a round share the CUs */
    i8x_walk(nblk, ntiles, max_blocks, chunk, FUSE2 ? (LAYOUT == 2 ? 8 : 4) : 1, grid, C);
    if (many && D == 8)
        hipLaunchKernelGGL((k_fir_i8x_many<HIST, MODE, FUSE2, LAYOUT>), dim3((unsigned)grid, (unsigned)nmany), dim3(768), G::LDS_BYTES, s,
                           *many, ntiles, (int)C);
    else
        hipLaunchKernelGGL((k_fir_i8x<HIST, MODE, FUSE2, LAYOUT, D>), dim3((unsigned)grid), dim3(768), G::LDS_BYTES, s, a, ntiles, (int)C);
    return hipGetLastError();
}

struct I8xManyRef {
    const FirI8xMany *m = nullptr;
    int n = 0;
};
static thread_local I8xManyRef t_many;       /* (set by launch_fir_i8x_many around its dispatch through the same switch) */
template <int HIST, int MODE, bool FUSE2>
static hipError_t launch_fir_i8x_t(const FirI8xArgs &a, int max_blocks, int chunk, int layout, hipStream_t s)
{
    return layout == 0   ? launch_fir_i8x_l<HIST, MODE, FUSE2, 0>(a, max_blocks, chunk, s, t_many.m, t_many.n)
           : layout == 1 ? launch_fir_i8x_l<HIST, MODE, FUSE2, 1>(a, max_blocks, chunk, s, t_many.m, t_many.n)
                         : launch_fir_i8x_l<HIST, MODE, FUSE2, 2>(a, max_blocks, chunk, s, t_many.m, t_many.n);
}

template <int HIST>
static hipError_t launch_fir_i8x_h(const FirI8xArgs &a, bool mix, bool fuse2, int max_blocks, int chunk, int layout, hipStream_t s)
{
    constexpr int MM = HIST <= 128 ? 2 : 1;
    if (!mix)
        return fuse2 ? launch_fir_i8x_t<HIST, 0, true>(a, max_blocks, chunk, layout, s) : launch_fir_i8x_t<HIST, 0, false>(a, max_blocks, chunk, layout, s);
    if (!fuse2)
        return launch_fir_i8x_t<HIST, MM, false>(a, max_blocks, chunk, layout, s);
    if constexpr (MM == 2)
        return launch_fir_i8x_t<HIST, 2, true>(a, max_blocks, chunk, layout, s);
    else
        return hipErrorInvalidValue;
}


bool fir_i8x_supported(int hist, bool mix, bool fuse2)
{
    if (hist != 32 && hist != 64 && hist != 128 && hist != 256)
        return false;
    return !(fuse2 && mix && hist > 128);
}

hipError_t launch_fir_i8x(const FirI8xArgs &a, int hist, bool mix, bool fuse2, hipStream_t s, int max_blocks, int chunk, int layout)
{
    if (a.n_in <= 0)
        return hipSuccess;
    if ((a.n_in & 7) || !a.in || !a.hist || !a.out || (!a.atab && !(a.taps16 && !mix)) || (a.hist_out && a.n_in < hist) ||
        !fir_i8x_supported(hist, mix, fuse2))
        return hipErrorInvalidValue;
    if (a.taps16 && (mix || !(a.two_e > 0.0f)))            /* binary16-stored taps: the untuned form only (tuned tables come from the host) */
        return hipErrorInvalidValue;
    if (fuse2 && ((a.n_in % i8x::TILE) || !a.taps2 || !a.hist2))
        return hipErrorInvalidValue;
    /* by form: the loaders finish the tile where the finish is heavy -- the four partial products of 129..256 tuned taps, and
     * the fused pair's second stage for SMALL batches; from 1024 tiles on (2^23 samples: four tiles per block and more) the
     * pair runs on two matrix + two finishing waves with chunks of 8 tiles.  Same box, the API's 250 kS/s pair, layout 1 /
     * chunks of 4 against layout 2 / chunks of 8: 2^22 7.6 / 7.7 us, 2^24 23.9 / 21.4, 2^26 99.7 / 88.5 (k_fir8's pair: 93.7),
     * 2^28 374 / 336 (profiles/r05/c_pair_layouts.txt) */
    if (layout < 0)
        layout = fuse2 ? (a.n_in >= (1LL << 23) ? 2 : 1) : (mix && hist > 128) ? 1 : 0;
    switch (hist) {
    case 32:
        return launch_fir_i8x_h<32>(a, mix, fuse2, max_blocks, chunk, layout, s);
    case 64:
        return launch_fir_i8x_h<64>(a, mix, fuse2, max_blocks, chunk, layout, s);
    case 128:
        return launch_fir_i8x_h<128>(a, mix, fuse2, max_blocks, chunk, layout, s);
    default:
        return launch_fir_i8x_h<256>(a, mix, fuse2, max_blocks, chunk, layout, s);
    }
}

hipError_t launch_fir_i8x_d10(const FirI8xArgs &a, hipStream_t s, int max_blocks, int chunk, int layout)
{
    if (a.n_out <= 0)
        return hipSuccess;
    if ((a.n_in & 7) || (a.in_off & 7) || a.in_off < 0 || !a.in || !a.hist || !a.out || !a.atab || a.taps2 ||
        (a.hist_out && a.n_in < a.hist_len) ||
        a.hist_len < 8 || (a.hist_len & 7) || (long long)a.in_off - 7 + 10 * (a.n_out - 1) >= a.n_in)
        return hipErrorInvalidValue;
    return layout == 1   ? launch_fir_i8x_l<kFirI8xD10Hist, 2, false, 1, 10>(a, max_blocks, chunk, s)
           : layout == 2 ? launch_fir_i8x_l<kFirI8xD10Hist, 2, false, 2, 10>(a, max_blocks, chunk, s)
                         : launch_fir_i8x_l<kFirI8xD10Hist, 2, false, 0, 10>(a, max_blocks, chunk, s);
}

template <int HIST, int NCH, int D = 8>
static hipError_t launch_fir_i8x_bank_l(const FirI8xBank &b, int max_blocks, int chunk, hipStream_t s)
{
    using G = i8x::Geo<HIST, 2, false, D>;
    constexpr size_t lds = 12 * (size_t)G::PLANE + (size_t)NCH * G::NARR * G::AS * sizeof(float);
    const long long ntiles = D == 8 ? (b.a.n_in + i8x::TILE - 1) / i8x::TILE : (b.a.n_out + 1023) / 1024;
    static int cus[64] = { 0 };
    long long nblk = 0, grid = 0, C = 0;
    const hipError_t e = i8x_cus(cus, reinterpret_cast<const void *>(&k_fir_i8x_bank<HIST, NCH, D>), nullptr, lds, nblk);
    if (e != hipSuccess)
        return e;
    i8x_walk(nblk, ntiles, max_blocks, chunk, 1, grid, C);      /* launch_fir_i8x_l's walk: one block per CU, C = 1 */
    hipLaunchKernelGGL((k_fir_i8x_bank<HIST, NCH, D>), dim3((unsigned)grid), dim3(768), lds, s, b, ntiles, (int)C);
    return hipGetLastError();
}

hipError_t launch_fir_i8x_bank(const FirI8xBank &b, int nch, int hist, hipStream_t s, int max_blocks, int chunk)
{
    const FirI8xArgs &a = b.a;
    if (a.n_in <= 0)
        return hipSuccess;
    if ((nch != 1 && nch != 2 && nch != 4) || (hist != 32 && hist != 64) || (a.n_in & 7) || !a.in || !a.hist)
        return hipErrorInvalidValue;
    for (int c = 0; c < nch; ++c)
        if (!b.ch[c].atab || !b.ch[c].out || (b.ch[c].hist_out && a.n_in < hist))
            return hipErrorInvalidValue;
    if (nch == 1) {                                      /* one channel: the solo kernel itself */
        FirI8xArgs q;
        q.in = a.in;
        q.hist = a.hist;
        q.n_in = a.n_in;
        q.atab = b.ch[0].atab;
        q.out = b.ch[0].out;
        q.hist_out = b.ch[0].hist_out;
        q.scale = b.ch[0].scale;
        q.ct[0] = b.ch[0].ct[0];
        q.ct[1] = b.ch[0].ct[1];
        q.n0 = b.ch[0].n0;
        q.freg = b.ch[0].freg;
        q.phase_off = b.ch[0].phase_off;
        return launch_fir_i8x(q, hist, true, false, s, max_blocks, chunk, 0);
    }
    if (hist == 32)
        return nch == 2 ? launch_fir_i8x_bank_l<32, 2>(b, max_blocks, chunk, s) : launch_fir_i8x_bank_l<32, 4>(b, max_blocks, chunk, s);
    return nch == 2 ? launch_fir_i8x_bank_l<64, 2>(b, max_blocks, chunk, s) : launch_fir_i8x_bank_l<64, 4>(b, max_blocks, chunk, s);
}

hipError_t launch_fir_i8x_bank_d10(const FirI8xBank &b, int nch, hipStream_t s, int max_blocks, int chunk)
{
    const FirI8xArgs &a = b.a;
    if (a.n_out <= 0)
        return hipSuccess;
    /* launch_fir_i8x_d10's checks on the shared part and on every channel; channel 0's history is the one the loaders read */
    if ((nch != 1 && nch != 2) || (a.n_in & 7) || (a.in_off & 7) || a.in_off < 0 || !a.in || !a.hist ||
        (long long)a.in_off - 7 + 10 * (a.n_out - 1) >= a.n_in)
        return hipErrorInvalidValue;
    for (int c = 0; c < nch; ++c) {
        const FirI8xBankCh &h = b.ch[c];
        if (!h.atab || !h.out || (h.hist_out && a.n_in < h.hist_len) || h.hist_len < 8 || (h.hist_len & 7) ||
            h.hist_len > b.ch[0].hist_len || h.hist_len > kFirI8xD10Hist)
            return hipErrorInvalidValue;
    }
    if (nch == 1) {                                      /* one channel: the solo kernel itself */
        FirI8xArgs q;
        q.in = a.in;
        q.hist = a.hist;
        q.n_in = a.n_in;
        q.n_out = a.n_out;
        q.in_off = a.in_off;
        q.hist_len = b.ch[0].hist_len;
        q.atab = b.ch[0].atab;
        q.out = b.ch[0].out;
        q.hist_out = b.ch[0].hist_out;
        q.scale = b.ch[0].scale;
        q.ct[0] = b.ch[0].ct[0];
        q.ct[1] = b.ch[0].ct[1];
        q.n0 = b.ch[0].n0;
        q.freg = b.ch[0].freg;
        q.phase_off = b.ch[0].phase_off;
        return launch_fir_i8x_d10(q, s, max_blocks, chunk, 0);
    }
    return launch_fir_i8x_bank_l<kFirI8xD10Hist, 2, 10>(b, max_blocks, chunk, s);
}

hipError_t launch_fir_i8x_many(const FirI8xMany &m, int n, int hist, bool mix, bool fuse2, hipStream_t s, int max_blocks, int chunk,
                               int layout)
{
    if (n < 1 || n > kFir8ManyMax)
        return hipErrorInvalidValue;
    for (int i = 1; i < n; ++i)
        if (m.a[i].n_in != m.a[0].n_in)
            return hipErrorInvalidValue;
    t_many = I8xManyRef{ &m, n };
    const hipError_t e = launch_fir_i8x(m.a[0], hist, mix, fuse2, s, max_blocks, chunk, layout);
    t_many = I8xManyRef{};
    return e;
}

} // namespace pddc
