/*
 * ddc_rxfilter.hip -- the receiver filter: every receiver's complex series through one of a bank of real FIR filters,
 * one output per input (gfx950 only).
 *
 *   k_rxfilter   per receiver j and output m of the launch: acc = (0, 0); over t = 0 .. T-1 ascending
 *                acc.re = fmaf(h_f[t], z_j[m - t].re, acc.re), the same for im; out_j[m] = acc, f = f_j.
 *                DESIGN.md 8 has the definition.
 *
 * Walk: every output is independent.  A block takes a tile of TT = 1024 consecutive outputs of G = 2 consecutive
 * receivers; thread i makes the O = 4 outputs 4 i .. 4 i + 3 of the tile, one receiver after the other:
 *   1. all threads stage, per receiver of the group, the tile's input span from S = (T - 1 rounded up to a multiple of
 *      O) inputs before its first output to its last output: consecutive threads, consecutive inputs, coalesced
 *      8-byte loads; an input before the batch's first comes from the carried record (zero where the receiver is marked
 *      fresh, and before the record's T - 1 values), one past the batch's last is zero.
 *   2. the tap loop walks the inputs, not the taps: step k = 0 .. T + O - 2 reads ONE value, staged element
 *      S + (O - 1) + 4 i - k, and gives it to output o as tap t = k - (O - 1) + o where 0 <= t < T -- O fmaf pairs per
 *      ds_read_b64.  Output o meets its taps in ascending t with an accumulator of its own, so its bits are those
 *      of the definition whatever O is.  The loop runs in passes of 8 steps; a pass whose 11 taps all lie in 0 .. T-1
 *      runs without a test, the first and last passes test every tap (uniform, scalar).
 *   3. h: the filter index comes from the receiver table through the scalar cache and through readfirstlane, the
 *      window of 11 taps of a pass is loaded with scalar loads into SGPRs: no per-lane loads of h, no LDS for h.
 *   4. four 8-byte stores per thread and receiver.
 *   The blocks of the last tile also write their receivers' new carried record, the last T - 1 values of
 *   [old record | batch], from global memory into the other buffer: a batch shorter than T - 1 keeps part of the old
 *   record, and no launch reads what it writes.
 * LDS layout: a receiver's row is O planes of PL float2 slots; staged element e lies in plane e mod O at slot e div O.
 *   At step k = O u + r every lane reads plane O - 1 - r at slot i + S / O - u: the 32 lanes of a ds_read_b64 group
 *   read 32 consecutive slots = 64 consecutive dwords = each of the 64 banks once (interleaved in one plane the lanes
 *   would lie 8 dwords apart, 8 lanes to a bank).  The staging store of 16 consecutive elements (a ds_write_b64
 *   group) goes to 4 consecutive slots of each plane; PL = 4 mod 16 puts the planes 8 dwords apart modulo 32, so
 *   the 16 slots cover the 32 store banks once.
 * Bits: one thread makes each value with one operation sequence (contraction is off in this file, every fmaf is
 * spelled); so out_j[m] does not depend on the batch cut, nrx, j's index, the other receivers, the strides or the tile
 * and lane a value falls into.  No atomics, no scratch.
 * Bounds: z and out are indexed by receivers < nrx and 0 <= i < n only; the records by receivers < nrx and
 * 0 <= e < T - 1; a staged element index is < S + TT <= O PL, a read one lies in S - (T - 1) .. S + TT - 1; the bank
 * row is read at taps -(O - 1) .. T + 7 + O - 2, inside its pads of 16; the filter index is checked by the host.
 */
#include "ddc_rxfilter.h"
#include "ddc_dev.h"
#include "ddc_host.h"

#pragma clang fp contract(off)

namespace pddc {

/* input idx of receiver row `zr`: before the batch's first from the carried record `old` (H = T - 1 values, the newest
 * last), zero before that and where the receiver is fresh; zero past the batch's last */
__device__ __forceinline__ float2 rxf_input(const float2 *zr, const float2 *old, long long idx, long long n, int H, bool fresh)
{
    if (idx < 0)
        return (fresh || idx < -(long long)H) ? make_float2(0.0f, 0.0f) : old[H + idx];
    return idx < n ? zr[idx] : make_float2(0.0f, 0.0f);
}

/* one pass of kRxfStep steps from step k0 (a multiple of kRxfStep): hw[i] = h[k0 - (O - 1) + i]; p points at the
 * thread's slot of step 0 in plane 0 */
template <bool Guard>
__device__ __forceinline__ void rxf_pass(const float2 *p, int PL, int k0, int T, const float (&hw)[kRxfStep + kRxfOut - 1],
                                         float2 (&acc)[kRxfOut])
{
    constexpr int O = kRxfOut, U = kRxfStep;
    const float2 *q = p - k0 / O;
    const int t0 = k0 - (O - 1);
#pragma unroll
    for (int s = 0; s < U; ++s) {
        if (Guard && k0 + s >= T + O - 1)
            break;
        const float2 z = q[(O - 1 - s % O) * PL - s / O];
#pragma unroll
        for (int o = 0; o < O; ++o) {
            if (!Guard || (unsigned)(t0 + s + o) < (unsigned)T) {
                acc[o].x = fmaf(hw[s + o], z.x, acc[o].x);
                acc[o].y = fmaf(hw[s + o], z.y, acc[o].y);
            }
        }
    }
}

__global__ __launch_bounds__(kRxfThreads) void k_rxfilter(RxfArgs a)
{
    constexpr int G = kRxfGroup, O = kRxfOut, TT = kRxfTile, U = kRxfStep;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int tid = (int)threadIdx.x;
    const int T = a.taps, H = T - 1;
    const int S = rxf_lead(T), PL = rxf_plane(T);
    const int g0 = (int)blockIdx.y * G;
    const int ng = a.nrx - g0 < G ? a.nrx - g0 : G;
    const long long o0 = (long long)blockIdx.x * TT;
    const int cnt = (int)(a.n - o0 < TT ? a.n - o0 : TT);
    const int len = S + (cnt + O - 1) / O * O;
    const RxfRx PDDC_CONSTANT *rx = (const RxfRx PDDC_CONSTANT *)a.rx + g0;

    for (int g = 0; g < ng; ++g) {
        const int j = g0 + g;
        const bool fresh = rx[g].fresh != 0u;
        const float2 *zr = a.z + (long long)j * a.z_stride;
        const float2 *old = a.state + (long long)j * H;
        float2 *row = lds2 + g * O * PL;
        for (int e = tid; e < len; e += kRxfThreads)
            row[(e % O) * PL + e / O] = rxf_input(zr, old, o0 - S + e, a.n, H, fresh);
    }
    __syncthreads();

    for (int g = 0; g < ng; ++g) {
        const int j = g0 + g;
        const int f = __builtin_amdgcn_readfirstlane(rx[g].filter);
        const float PDDC_CONSTANT *h = (const float PDDC_CONSTANT *)a.bank + (long long)f * (T + 2 * kRxfPad) + kRxfPad;
        const float2 *p = lds2 + g * O * PL + tid + S / O;
        float2 acc[O];
#pragma unroll
        for (int o = 0; o < O; ++o)
            acc[o] = make_float2(0.0f, 0.0f);
        for (int k0 = 0; k0 < T + O - 1; k0 += U) {
            const int t0 = k0 - (O - 1);
            float hw[U + O - 1];
#pragma unroll
            for (int i = 0; i < U + O - 1; ++i)
                hw[i] = h[t0 + i];
            if (t0 >= 0 && t0 + U + O - 2 < T)
                rxf_pass<false>(p, PL, k0, T, hw, acc);
            else
                rxf_pass<true>(p, PL, k0, T, hw, acc);
        }
        float2 *outr = a.out + (long long)j * a.out_stride + o0;
#pragma unroll
        for (int o = 0; o < O; ++o)
            if (O * tid + o < cnt)
                outr[O * tid + o] = acc[o];
    }

    /* the new carried record: the last T - 1 values of [old record | batch] */
    if (blockIdx.x == gridDim.x - 1) {
        for (int g = 0; g < ng; ++g) {
            const int j = g0 + g;
            const bool fresh = rx[g].fresh != 0u;
            for (int e = tid; e < H; e += kRxfThreads)
                a.new_state[(long long)j * H + e] =
                    rxf_input(a.z + (long long)j * a.z_stride, a.state + (long long)j * H, a.n - H + e, a.n, H, fresh);
        }
    }
}

hipError_t launch_rxfilter(const RxfArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.nrx <= 0 || a.nrx > kRxfMaxRx || a.nfilters < 1 || a.nfilters > kRxfMaxFilters || a.taps < 1 ||
        a.taps > kRxfMaxTaps || !a.z || !a.out || a.z_stride < a.n || a.out_stride < a.n || !a.bank || !a.rx || !a.state ||
        !a.new_state)
        return hipErrorInvalidValue;
    const long long nx = (a.n + kRxfTile - 1) / kRxfTile;
    if (nx > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nx, (unsigned)((a.nrx + kRxfGroup - 1) / kRxfGroup));
    return launch_dynamic_lds<&k_rxfilter>(kRxfLdsCap, grid, dim3(kRxfThreads), rxf_lds_bytes(a.taps), s, a);
}

} // namespace pddc
