/*
 * ddc_eq.hip -- the equaliser: per receiver a cascade of up to S second-order sections over the audio, in binary64
 * (gfx950 only).
 *
 *   k_eq        per receiver j and sample m: v = (double)x[m]; for s < nsec_j: y = (b0 v) + s1, s1 = ((b1 v) - (a1 y)) + s2,
 *               s2 = (b2 v) - (a2 y), v = y; out[m] = (float)v.  nsec_j = 0 passes the words.  DESIGN.md 8 has the
 *               definition.
 *
 * Layout: a block is kEqWaves = 1 wave (with more, each wave is what follows with rows of its own).  A receiver has
 * L = S lanes of it, side by side inside a row of 16, and a wave G = min(64 / L, kEqGroup) receivers; lane s of a
 * receiver holds section s's five coefficients and two states in registers for the whole launch.  The sections are a
 * systolic pipeline: at step t lane s does the definition's three lines for sample m = t - s, where 0 <= m < n, on the y
 * that lane s - 1 made at step t - 1: two 32-bit DPP row_shr:1 moves.  Elsewhere a select leaves its states alone; the
 * chunks of C steps that find every lane inside its n samples -- all but the launch's first and last few -- run without
 * that select.  Lane 0 takes (double)x[m] from the receiver's LDS row; lane L - 1 leaves (float)y in the output row at
 * step m + L - 1.  Lanes s >= nsec_j pass what they are given by select, with no arithmetic; with nsec_j = 0 what
 * travels is the input word itself, which lane L - 1 writes as it is.  So S sections take n + S - 1 steps, not S n.
 * Walk: the wave takes its receivers through the launch tile by tile, TT = 256 steps a time.
 *   1. the tile's inputs, loaded a tile ahead into registers (coalesced 4-byte loads), go to sx; the NEXT tile's loads
 *      are issued here and stay in registers over the chain.
 *   2. the chain, step by step, C = 4 samples of lane 0's input read a chunk ahead.
 *   3. so is stored coalesced, once per tile: step i of the tile at offset o finished output o + i - (L - 1), so a
 *      tile's store covers the outputs finished during it, and the last tile runs L - 1 more steps (up to the next
 *      multiple of C: the steps beyond find every lane past its n samples).
 *   The states go to the new record at the end; those of sections s >= nsec_j as 0.
 * Bits: every value is made by the definition's operation sequence (contraction is off in this file, binary64 and
 * float32 denormals are kept, the conversions round to nearest even: the target's default mode) from the receiver's own
 * series, states and table entry, so nothing depends on the batch cut, K, j's index, the other receivers, S or the
 * layout.  No atomics, no scratch.
 * In place (out == a): a tile's inputs are in registers before the tile before it is stored, a tile's store ends below
 * the next tile's first input, and a wave alone reads and writes its receivers' rows.
 * Bounds: a and out are indexed by receivers < nrx and samples < n only; the record by receivers < nrx and sections < S;
 * sx and so by rows < G and places < TT + L - 1 + C <= 267 < the row's length.
 */
#include "ddc_eq.h"
#include "ddc_dev.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace pddc {

/* the word of the lane before in the row of 16 (row_shr:1); lane 0 of a row reads 0 */
__device__ __forceinline__ uint32_t eq_from_left(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
}

template <int L> __global__ __launch_bounds__(kEqThreads) void k_eq(EqArgs a)
{
    constexpr int G = eq_group(L), TT = kEqTile, C = 4;
    constexpr int GS = TT + 17;         /* a row: TT places, the drain's L - 1 + C, and an odd length: rows on different banks */
    constexpr int RT = TT / 64;
    static_assert(L >= 1 && L <= kEqMaxSections && 16 % L == 0 && G * L <= 64 && kEqThreads == 64 * kEqWaves, "the lanes of one wave");
    static_assert(TT % 64 == 0 && TT % C == 0 && GS >= TT + L - 1 + 2 * C, "row layout");
    __shared__ uint32_t sxw[kEqWaves][G * GS];
    __shared__ uint32_t sow[kEqWaves][G * GS];
    const int lane = (int)threadIdx.x % 64, wave = (int)threadIdx.x / 64;
    uint32_t *const sx = sxw[wave], *const so = sow[wave];
    const int l = lane % L;
    const bool mine = lane / L < G;                 /* lanes behind the wave's G receivers idle */
    const int grp = mine ? lane / L : G - 1;
    const int j0 = ((int)blockIdx.x * kEqWaves + wave) * G;
    const int j = j0 + grp;
    const bool live = mine && j < a.nrx;

    int nsec = 0;
    bool keep = false;                              /* the carried states are read */
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, a1 = 0.0, a2 = 0.0;
    if (live) {
        const EqRx *const r = a.rx + j;
        nsec = (int)r->nsec;
        keep = !a.fresh && !(r->flags & kEqRestart);
        if (l < nsec) {
            b0 = r->c[l][0];
            b1 = r->c[l][1];
            b2 = r->c[l][2];
            a1 = r->c[l][3];
            a2 = r->c[l][4];
        }
    }
    const bool run = l < nsec, off = nsec == 0;
    double s1 = 0.0, s2 = 0.0;
    if (run && keep) {
        s1 = a.old_state[((long long)j * L + l) * 2];
        s2 = a.old_state[((long long)j * L + l) * 2 + 1];
    }

    uint32_t pre[G][RT];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int i = r * 64 + lane;
            pre[g][r] = 0u;
            if (j0 + g < a.nrx && i < a.n)
                pre[g][r] = a.a[(long long)(j0 + g) * a.a_stride + i];
        }

    const uint32_t *const xb = sx + grp * GS;
    uint32_t *const ob = so + grp * GS;
    const bool writer = mine && l == L - 1;
    uint32_t ylo = 0u, yhi = 0u;                    /* what this lane made at the step before */
    for (long long o = 0;; o += TT) {
        const bool last = o + TT >= a.n;
        const int cnt = last ? (int)(a.n - o) : TT;
        const int nst = last ? cnt + L - 1 : TT;    /* steps of this tile */
        /* this lane's sample at step i is m = o + i - l: it runs where 0 <= m < n */
        const int lo = o == 0 ? l : 0, hi = cnt + l;
        /* 1. this tile into its rows; the next tile's loads */
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RT; ++r)
                sx[g * GS + r * 64 + lane] = pre[g][r];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const long long i = o + TT + r * 64 + lane;
                pre[g][r] = 0u;
                if (j0 + g < a.nrx && i < a.n)
                    pre[g][r] = a.a[(long long)(j0 + g) * a.a_stride + i];
            }
        __syncthreads();

        /* 2. the chain */
        uint32_t xn[C];
#pragma unroll
        for (int s = 0; s < C; ++s)
            xn[s] = xb[s];
        /* one step; `inside`: every lane of the wave is inside its n samples at this step, and the states move without a
         * select (those of a lane whose section does not run are never read: the record gets 0 for them) */
        auto step = [&](auto inside, int i, uint32_t xw) {
            uint32_t vlo = ylo, vhi = yhi;
            if constexpr (L > 1) {
                vlo = eq_from_left(ylo);
                vhi = eq_from_left(yhi);
            }
            if (l == 0) {
                const double d = (double)__uint_as_float(xw);
                vlo = off ? xw : (uint32_t)__double2loint(d);
                vhi = off ? 0u : (uint32_t)__double2hiint(d);
            }
            const double v = __hiloint2double((int)vhi, (int)vlo);
            const double y = (b0 * v) + s1;
            const double n1 = ((b1 * v) - (a1 * y)) + s2;
            const double n2 = (b2 * v) - (a2 * y);
            if constexpr (decltype(inside)::value) {
                s1 = n1;
                s2 = n2;
            } else {
                const bool upd = run && i >= lo && i < hi;
                s1 = upd ? n1 : s1;
                s2 = upd ? n2 : s2;
            }
            /* the sections differ from lane group to lane group: selects */
            ylo = run ? (uint32_t)__double2loint(y) : vlo;
            yhi = run ? (uint32_t)__double2hiint(y) : vhi;
            if (writer)
                ob[i] = off ? ylo : __float_as_uint((float)__hiloint2double((int)yhi, (int)ylo));
        };
        /* the steps from `full` on and below cnt find every lane inside: lane l's window is lo <= i < hi = cnt + l */
        const int full = o == 0 ? L - 1 : 0;
        for (int i0 = 0; i0 < nst; i0 += C) {
            uint32_t x[C];
#pragma unroll
            for (int s = 0; s < C; ++s)
                x[s] = xn[s];
            if (i0 + C < nst) {
#pragma unroll
                for (int s = 0; s < C; ++s)
                    xn[s] = xb[i0 + C + s];
            }
            if (i0 >= full && i0 + C <= cnt) {
#pragma unroll
                for (int s = 0; s < C; ++s)
                    step(std::true_type{}, i0 + s, x[s]);
            } else {
#pragma unroll
                for (int s = 0; s < C; ++s)
                    step(std::false_type{}, i0 + s, x[s]);
            }
        }
        __syncthreads();

        /* 3. the outputs this tile finished: step i made output o + i - (L - 1) */
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r <= RT; ++r) {
                const int i = r * 64 + lane;
                const long long m = o + i - (L - 1);
                if (j0 + g < a.nrx && i < nst && m >= 0 && m < a.n)
                    a.out[(long long)(j0 + g) * a.out_stride + m] = so[g * GS + i];
            }
        if (last)
            break;
        /* the next tile's chain writes so, which the store has read, only after its own barrier */
        __syncthreads();
    }

    /* the record: sections that did not run are at rest */
    if (live) {
        a.new_state[((long long)j * L + l) * 2] = run ? s1 : 0.0;
        a.new_state[((long long)j * L + l) * 2 + 1] = run ? s2 : 0.0;
    }
}

template <int L> static hipError_t launch_eq_l(const EqArgs &a, hipStream_t s)
{
    constexpr int G = eq_group(L) * kEqWaves;
    hipLaunchKernelGGL((k_eq<L>), dim3((unsigned)((a.nrx + G - 1) / G)), dim3(kEqThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_eq(const EqArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kEqMaxRx || a.a_stride < a.n || a.out_stride < a.n || !a.a || !a.out || !a.rx ||
        !a.old_state || !a.new_state)
        return hipErrorInvalidValue;
    switch (a.S) {
    case 1: return launch_eq_l<1>(a, s);
    case 2: return launch_eq_l<2>(a, s);
    case 4: return launch_eq_l<4>(a, s);
    case 8: return launch_eq_l<8>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace pddc
