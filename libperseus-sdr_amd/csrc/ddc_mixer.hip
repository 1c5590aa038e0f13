/*
 * ddc_mixer.hip -- the mixer: the active receivers' real series summed into Q output buses through per-receiver gains
 * with ramps, and per bus a block peak limiter (gfx950 only).
 *
 *   k_mix       per sample i and bus q: the active receivers p (ascending j) in chunks of C = 32; chunk m starts at +0 and
 *               takes s_m = fmaf(g_pq(i), a_p[i], s_m) in ascending p; y = s_0, then y = y + s_m in ascending m.  The gain
 *               is to_q once the ramp counter c = min(c0 + i + 1, R) has reached R, else fmaf(to_q - from_q, float(c) invR,
 *               from_q).  DESIGN.md 8 has the definition.
 *   k_mix_bus   per bus: the peak of |y| for read(); with the limiter, over blocks of Lb samples P[k] = max |y|,
 *               t[k] = ceil / max(P[k], P[k+1]) above the ceiling else 1, E[k] = fminf(t[k], fmaf(rel, 1 - E[k-1], E[k-1])),
 *               the gain interpolated from E[k-1] to E[k] across block k, out = clamp(y g, +-ceil); block k is written once
 *               block k + 1 is complete.
 *
 * k_mix: a block takes one tile of 64 samples, lane l of every wave sample l of the tile, so a receiver's row is read
 * with coalesced 4-byte loads of 256 bytes.  Chunk m runs on wave m mod waves (up to 16 waves): the wave loads its
 * receivers eight at a time, the next eight issued before the chain over the eight in hand, and every loaded value
 * feeds all Q accumulators.  The active list with the gain records is the uploaded table, read through the scalar
 * cache.  The chunk sums go to LDS, s[m][q][l]; behind a barrier wave q mod waves adds bus q's in ascending m; the tile's
 * y then leaves from LDS: planar rows (the limiter's workspace, or the float32 output), the interleaved int16 frames
 * as consecutive 2-byte stores, and the tile's peak per bus.
 * k_mix_bus: one block of 1024 threads per bus.  The tiles' peaks are reduced with fmaxf (exact, no order).  The
 * limiter sees the carried samples followed by the launch's: groups of up to 64 lanes take P of one block each, all
 * threads the t[k], one lane walks E over the blocks that are written, all threads the gain, the clamp and the stores,
 * and the samples not yet written go to the other carried record.
 * Bits: every chunk sum is made by one lane in ascending p from +0 and every bus sum by one lane in ascending m
 * (contraction is off in this file, every fmaf is spelled), the maxima are exact, E is one lane's chain; so nothing
 * depends on n, the batch cut, the grid or the tile -- only on the active set, which the host keeps constant within a
 * launch.  No atomics, no scratch.
 * In flight: nothing on the device is cleared from the host.  A launch reads one carried record and writes the other;
 * `fresh` tells k_mix_bus not to read the record (create, reset), `clear` to take the carried peak as 0 and the
 * smallest gain as 1.  The workspace y and the tiles' peaks are written by k_mix and read by the k_mix_bus behind it on
 * the same stream.
 * Bounds: a is indexed by the table's receivers (< nrx, the host's) and samples < n; the table by p < nact; LDS by
 * chunks < ceil(nact / C) <= 32, buses < QP and lanes < 64; y, f32 and i16 by buses < Q and samples < n (k_mix) or <
 * write_blocks Lb (k_mix_bus), which the host checked against the capacities; the carried samples by e < 2 Lb; sP and
 * sE by blocks <= (held + n) / Lb <= kMixMaxBlocks.
 */
#include "ddc_mixer.h"
#include "ddc_dev.h"
#include "ddc_host.h"

#pragma clang fp contract(off)

namespace pddc {

static constexpr int kMixLoads = 8;                     /* receivers whose loads a wave keeps in flight */

template <int QP> __global__ __launch_bounds__(kMixTile * kMixMaxWaves) void k_mix(MixArgs a)
{
    constexpr int C = kMixChunk, U = kMixLoads, TT = kMixTile;
    static_assert(C % U == 0 && TT == 64, "a chunk is whole groups of loads; a tile is one wave wide");
    extern __shared__ __attribute__((aligned(16))) float s[];         /* [max(chunks, 1)][QP][TT] */
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int waves = (int)blockDim.x >> 6;
    const int i0 = (int)blockIdx.x * TT;
    const int i = i0 + lane;
    const bool in = i < a.n;
    const int nch = (a.nact + C - 1) / C;
    const MixRx PDDC_CONSTANT *rx = (const MixRx PDDC_CONSTANT *)a.rx;
    const uint32_t R = a.R;

    for (int m = wave; m < nch; m += waves) {
        const int p0 = m * C;
        const int cnt = a.nact - p0 < C ? a.nact - p0 : C;
        float acc[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q)
            acc[q] = 0.0f;
        float cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cur[u] = 0.0f;
            nxt[u] = 0.0f;
            if (u < cnt && in)
                cur[u] = a.a[(long long)rx[p0 + u].j * a.a_stride + i];
        }
        for (int g = 0; g < cnt; g += U) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (g + U + u < cnt && in)
                    nxt[u] = a.a[(long long)rx[p0 + g + U + u].j * a.a_stride + i];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (g + u < cnt) {
                    const MixRx PDDC_CONSTANT *r = rx + (p0 + g + u);
                    const float v = cur[u];
                    const uint32_t c0 = r->c;
                    if (c0 >= R) {
#pragma unroll
                        for (int q = 0; q < QP; ++q)
                            acc[q] = fmaf(r->to[q], v, acc[q]);
                    } else {
                        uint32_t c = c0 + (uint32_t)i + 1u;
                        c = c < R ? c : R;
                        const float t = (float)c * a.invR;
#pragma unroll
                        for (int q = 0; q < QP; ++q) {
                            const float to = r->to[q], from = r->from[q];
                            const float gq = c == R ? to : fmaf(to - from, t, from);
                            acc[q] = fmaf(gq, v, acc[q]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                cur[u] = nxt[u];
        }
#pragma unroll
        for (int q = 0; q < QP; ++q)
            s[(m * QP + q) * TT + lane] = acc[q];
    }
    __syncthreads();

    /* the bus sums, in chunk order; y takes chunk 0's place, which this lane alone reads */
    for (int q = wave; q < QP; q += waves) {
        float y = 0.0f;
        if (nch > 0) {
            y = s[q * TT + lane];
            for (int m = 1; m < nch; ++m)
                y = y + s[(m * QP + q) * TT + lane];
        }
        s[q * TT + lane] = y;
    }
    __syncthreads();

    /* the tile leaves: planar rows, interleaved frames, the peak */
    const int cnt = a.n - i0 < TT ? a.n - i0 : TT;
    float *planar = a.y ? a.y : a.f32;
    const long long pstride = a.y ? a.y_stride : a.f32_stride;
    for (int e = (int)threadIdx.x; e < a.Q * TT; e += (int)blockDim.x) {
        const int q = e >> 6, l = e & 63;
        if (planar && l < cnt)
            planar[(long long)q * pstride + i0 + l] = s[q * TT + l];
    }
    if (a.i16) {
        /* (one frame a pass: two frames' y scale side by side come out as one packed multiply) */
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int e = (int)threadIdx.x; e < a.Q * cnt; e += (int)blockDim.x) {
            const int fr = e / a.Q, q = e - fr * a.Q;
            a.i16[(long long)(i0 + fr) * a.Q + q] = pcm16(s[q * TT + fr], a.scale);
        }
    }
    for (int q = wave; q < a.Q; q += waves) {
        float pk = in ? fmaxf(0.0f, fabsf(s[q * TT + lane])) : 0.0f;
#pragma unroll
        for (int o = 32; o; o >>= 1)
            pk = fmaxf(pk, __shfl_xor(pk, o));
        if (lane == 0)
            a.tile_peak[(long long)blockIdx.x * kMixMaxBus + q] = pk;
    }
}

__global__ __launch_bounds__(kMixBusThreads) void k_mix_bus(MixBusArgs a)
{
    __shared__ float sP[kMixMaxBlocks];
    __shared__ float sE[kMixMaxBlocks];
    __shared__ float sred[kMixBusThreads / 64];
    const int tid = (int)threadIdx.x, q = (int)blockIdx.x;
    constexpr int NT = kMixBusThreads;

    MixBus st;
    st.peak = 0.0f;
    st.gain = 1.0f;
    st.min_gain = 1.0f;
    st.pad = 0u;
    if (!a.fresh)
        st = a.old[q];
    if (a.clear) {
        st.peak = 0.0f;
        st.min_gain = 1.0f;
    }

    /* the peak: fmaxf over the tiles' */
    float pk = 0.0f;
    for (int t = tid; t < a.tiles; t += NT)
        pk = fmaxf(pk, a.tile_peak[(long long)t * kMixMaxBus + q]);
#pragma unroll
    for (int o = 32; o; o >>= 1)
        pk = fmaxf(pk, __shfl_xor(pk, o));
    if ((tid & 63) == 0)
        sred[tid >> 6] = pk;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < NT / 64; ++w)
            st.peak = fmaxf(st.peak, sred[w]);
    }
    if (!a.limit) {
        if (tid == 0)
            a.next[q] = st;
        return;
    }

    const int Lb = a.Lb, H = a.held, T = H + a.n, cb = T / Lb, wn = a.write_blocks;
    const float *ho = a.held_old + (long long)q * 2 * Lb;
    float *hn = a.held_next + (long long)q * 2 * Lb;
    const float *yq = a.y + (long long)q * a.y_stride;
    /* sample t of [the carried samples | this launch's] */
    auto v = [&](int t) { return t < H ? ho[t] : yq[t - H]; };

    /* P[k] of the complete blocks: a group of G <= 64 lanes (a power of two, G <= Lb) per block */
    int G = 64;
    while (G > Lb)
        G >>= 1;
    const int groups = NT / G, gi = tid / G, gl = tid - gi * G;
    for (int k0 = 0; k0 < cb; k0 += groups) {
        const int k = k0 + gi;
        float m = 0.0f;
        if (k < cb)
            for (int r = gl; r < Lb; r += G)
                m = fmaxf(m, fabsf(v(k * Lb + r)));
        for (int o = G >> 1; o; o >>= 1)
            m = fmaxf(m, __shfl_xor(m, o));
        if (k < cb && gl == 0)
            sP[k] = m;
    }
    __syncthreads();
    for (int k = tid; k < wn; k += NT) {
        const float m = fmaxf(sP[k], sP[k + 1]);
        sE[k] = m > a.ceil ? a.ceil / m : 1.0f;
    }
    __syncthreads();
    const float E0 = st.gain;               /* E of the block before the first one written here */
    if (tid == 0) {
        float E = E0, mn = st.min_gain;
        for (int k = 0; k < wn; ++k) {
            E = fminf(sE[k], fmaf(a.rel, 1.0f - E, E));
            sE[k] = E;
            mn = fminf(mn, E);
        }
        st.gain = E;
        st.min_gain = mn;
        a.next[q] = st;
    }
    __syncthreads();
    const int nout = wn * Lb;
    for (int t = tid; t < nout; t += NT) {
        const int k = t / Lb, r = t - k * Lb;
        const float Ek = sE[k], Ep = k ? sE[k - 1] : E0;
        const float g = r == Lb - 1 ? Ek : fmaf(Ek - Ep, (float)(r + 1) * a.invLb, Ep);
        const float o = fminf(fmaxf(v(t) * g, -a.ceil), a.ceil);
        if (a.f32)
            a.f32[(long long)q * a.f32_stride + t] = o;
        if (a.i16)
            a.i16[(long long)t * a.Q + q] = pcm16(o, a.scale);
    }
    for (int e = tid; e < T - nout; e += NT)
        hn[e] = v(nout + e);
}

static size_t mix_lds_bytes(int nact, int QP)
{
    const int nch = (nact + kMixChunk - 1) / kMixChunk;
    return (size_t)(nch > 0 ? nch : 1) * (size_t)QP * kMixTile * sizeof(float);
}

template <int QP> static hipError_t launch_mix_q(const MixArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    return launch_dynamic_lds<&k_mix<QP>>(mix_lds_bytes(kMixMaxRx, QP), grid, block, mix_lds_bytes(a.nact, QP), s, a);
}

hipError_t launch_mix(const MixArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.n > kMixMaxPiece || a.nact < 0 || a.nact > kMixMaxRx || a.Q < 1 || a.Q > kMixMaxBus || !a.a ||
        a.a_stride < a.n || !a.rx || !a.tile_peak || a.R < 1u || a.R > (uint32_t)kMixMaxRamp)
        return hipErrorInvalidValue;
    if (a.y ? (a.y_stride < a.n || a.f32 || a.i16) : ((!a.f32 && !a.i16) || (a.f32 && a.f32_stride < a.n)))
        return hipErrorInvalidValue;
    const int nch = (a.nact + kMixChunk - 1) / kMixChunk;
    const int waves = nch < 1 ? 1 : nch > kMixMaxWaves ? kMixMaxWaves : nch;
    const dim3 grid((unsigned)((a.n + kMixTile - 1) / kMixTile)), block((unsigned)(waves * 64));
    switch (a.Q) {
    case 1:
        return launch_mix_q<1>(a, grid, block, s);
    case 2:
        return launch_mix_q<2>(a, grid, block, s);
    case 3:
    case 4:
        return launch_mix_q<4>(a, grid, block, s);
    default:
        return launch_mix_q<8>(a, grid, block, s);
    }
}

hipError_t launch_mix_bus(const MixBusArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.n > kMixMaxPiece || a.Q < 1 || a.Q > kMixMaxBus || !a.tile_peak ||
        a.tiles != (a.n + kMixTile - 1) / kMixTile || !a.old || !a.next)
        return hipErrorInvalidValue;
    if (a.limit) {
        if (a.Lb < kMixMinBlock || a.Lb > kMixMaxBlock || a.held < 0 || a.held >= 2 * a.Lb || !a.y || a.y_stride < a.n ||
            !a.held_old || !a.held_next || !(a.ceil > 0.0f) || !(a.rel > 0.0f && a.rel <= 1.0f))
            return hipErrorInvalidValue;
        const int cb = (a.held + a.n) / a.Lb;
        if (cb > kMixMaxBlocks || a.write_blocks != (cb > 1 ? cb - 1 : 0))
            return hipErrorInvalidValue;
        if (a.write_blocks && ((!a.f32 && !a.i16) || (a.f32 && a.f32_stride < (long long)a.write_blocks * a.Lb)))
            return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_mix_bus, dim3((unsigned)a.Q), dim3(kMixBusThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
