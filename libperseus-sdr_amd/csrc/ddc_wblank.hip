/*
 * ddc_wblank.hip -- the wideband blanker's gfx950 kernels (include/perseus_ddc.h, pddc_wblank_*): impulse blanking on the
 * packed 24-bit ADC stream, 6 bytes in and 6 bytes out per sample, integers only.
 *
 *   k_wblank_sums    a thread takes a group of 8 samples (48 bytes, three nontemporal 16-byte loads), adds their powers,
 *                    the lanes of one metering block add up by shuffles, one integer atomic add per block and wave.
 *                    Threads are placed on the stream's block grid, so a block never straddles such a lane set.
 *   k_wblank_means   a thread per metering block: its reference, the least of the H sums in front of it.  The launch's
 *                    last block writes what the device carries on: the last H sums, the open block's partial sum, the
 *                    reference, the counters as they stood.
 *   k_wblank_gate    tiles of 2048 outputs, a workgroup walks a run of them.  Per tile ONE pass of global loads: the
 *                    tile's samples and the 2 D in front of them (a group per thread, the first threads one more), with
 *                    the reference of each group's block.  Their trigger bits go into LDS, a byte per group -- taken
 *                    again from the samples, or from the carried bits where the samples lie in the tail -- and so do the
 *                    bytes themselves.  Then a thread makes a group of 8 outputs from the input D samples earlier: 13
 *                    dwords from LDS, shifted by 0 or 2 bytes to the output's place, stored as they are when no
 *                    trigger bit lies within D of them (almost always).  Only a group with a gate value in it unpacks,
 *                    scales and re-packs.  Counters: one atomic add per workgroup and counter; an output in front
 *                    of the stream's first input (n < D) is not counted as blanked, whatever lies near it.
 *                    The blocks behind the tiles' copy the tail and the carried trigger bits for the next batch.
 *
 * No floating point, so every bit is independent of grid, run, tile and cut.  Nothing waits for another workgroup.
 */
#include "ddc_wblank.h"

namespace pddc {

static constexpr int kWbSpanGroups = (kWbTile + 512) / 8;                /* a tile's own groups and the most in front of them */
static constexpr int kWbTrigWords = (kWbTile + 512) / 32 + 2;

/* the sum of block k0 + j as this batch sees it: carried for j < 0, the scratch's (with the carried partial sum in the
 * open block) for j >= 0 */
__device__ __forceinline__ uint64_t wb_block_sum(const WbArgs &a, long long j)
{
    if (j < 0)
        return a.H + j >= 0 ? a.st->hist[a.H + j] : kWbNoBlock;
    return a.sums[j] + (j == 0 ? a.st->partial : 0);
}

/* the reference of block k0 + i: the minimum of the H sums in front of it, >> b; 0 for the stream's first block */
__device__ __forceinline__ uint64_t wb_block_mean(const WbArgs &a, uint64_t k0, long long i)
{
    if (k0 + (uint64_t)i == 0)
        return 0;
    uint64_t m = kWbNoBlock;
    for (int h = 1; h <= a.H; ++h) {
        const uint64_t s = wb_block_sum(a, i - h);
        m = s < m ? s : m;
    }
    return m >> a.b;
}

/* the powers of the 8 samples of a loaded group */
__device__ __forceinline__ void wb_group_powers(const u32x4 (&raw)[3], uint64_t (&p)[8])
{
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        PDDC_UNPACK_GROUP_MSB(raw, h, i0, q0, i1, q1);
        p[2 * h] = wb_power(wb_code(i0), wb_code(q0));
        p[2 * h + 1] = wb_power(wb_code(i1), wb_code(q1));
    }
}

__global__ __launch_bounds__(256) void k_wblank_sums(WbArgs a)
{
    const long long off = (long long)wb_block_offset(a.N, a.b);
    const long long w0 = off & ~511ll;                      /* a wave's 512 samples lie on the block grid */
    const long long ngroups = (off - w0 + a.n) >> 3;
    const int L = (1 << (a.b - 3)) < 64 ? (1 << (a.b - 3)) : 64;       /* lanes that share a block */
    const int lane = threadIdx.x & 63;
    for (long long g0 = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); g0 < ngroups; g0 += (long long)gridDim.x * 256) {
        const long long w = w0 + ((g0 + lane) << 3), u = w - off;
        unsigned long long s = 0;
        if (u >= 0 && u < a.n) {
            u32x4 raw[3];
            a.in.load_group(u + a.TL, raw);
            uint64_t p[8];
            wb_group_powers(raw, p);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                s += p[j];
        }
        for (int m = 1; m < L; m <<= 1)
            s += __shfl_xor(s, m);
        if (!(lane & (L - 1)) && s)
            atomicAdd(reinterpret_cast<unsigned long long *>(a.sums + (w >> a.b)), s);
    }
}

/* the references of the blocks the batch touches, means[i] for block k0 + i; and, in the launch's last block, what the
 * device carries on: the sums, the open block's partial sum, the reference, the counters as they stand in front of the
 * batch (k_wblank_gate adds to them) */
__global__ __launch_bounds__(256) void k_wblank_means(WbArgs a)
{
    const long long off = (long long)wb_block_offset(a.N, a.b);
    const uint64_t k0 = wb_block_of(a.N, a.b);
    const int t = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        const long long done = (off + a.n) >> a.b;          /* blocks this batch completed */
        if (t < kWbMaxHistory)
            a.new_st->hist[t] = t < a.H ? wb_block_sum(a, done - a.H + t) : kWbNoBlock;
        if (t == 16)
            a.new_st->partial = wb_block_sum(a, done);
        if (t == 17)
            a.new_st->triggers = a.st->triggers;
        if (t == 18)
            a.new_st->blanked = a.st->blanked;
        if (t == 19)
            a.new_st->mean = wb_block_mean(a, k0, done);
        return;
    }
    const long long i = (long long)blockIdx.x * 256 + t;
    if (i < a.nblocks)
        a.means[i] = wb_block_mean(a, k0, i);
}

__global__ __launch_bounds__(256) void k_wblank_gate(WbArgs a)
{
    __shared__ u32x4 s_raw[kWbSpanGroups * 3 + 1];          /* the span's bytes as they lie in the stream, and a spare chunk */
    __shared__ uint32_t s_trig[kWbTrigWords];
    __shared__ unsigned s_cnt[2];
    const int tid = threadIdx.x;

    if ((int)blockIdx.x >= a.tile_blocks) {
        /* the carried trigger bits of tail samples that stay in the tail (a batch shorter than the tail) */
        if ((int)blockIdx.x == a.tile_blocks)
            for (long long v = a.n + 8ll * tid; v < a.TL; v += 8 * 256)
                a.new_bits[(v - a.n) >> 3] = a.bits[v >> 3];
        PDDC_CARRY_TAIL(a.carry, a.tile_blocks)
        return;
    }

    const long long off = (long long)wb_block_offset(a.N, a.b);
    const int delta = a.TL - a.D;                           /* output n is sample n + delta of tail-then-batch */
    const int own = a.TL >> 3;                              /* the span's groups in front of the tile's own     */
    const int q = (6 * delta) >> 2, rr = (6 * delta) & 3;   /* the outputs' place in the span: dwords, and 0 or 2 bytes */
    uint8_t *trig_bytes = reinterpret_cast<uint8_t *>(s_trig);
    const uint32_t *raw_words = reinterpret_cast<const uint32_t *>(s_raw);
    unsigned ntrig = 0, nblank = 0;
    for (int i = tid; i < kWbTrigWords; i += 256)
        s_trig[i] = 0;
    if (tid < 2)
        s_cnt[tid] = 0;
    if (tid == 0)
        s_raw[kWbSpanGroups * 3] = u32x4{ 0, 0, 0, 0 };

    const long long r0 = (long long)blockIdx.x * a.run;
    const long long r1 = r0 + a.run < a.n ? r0 + a.run : a.n;
    for (long long t0 = r0; t0 < r1; t0 += kWbTile) {
        /* the span: samples t0 .. t0 + kWbTile + TL of tail-then-batch, i.e. inputs t0 - TL .. t0 + kWbTile: a group per
         * thread, the first `own` threads one more; all loads first, then what hangs on them */
        u32x4 raw[2][3];
        uint64_t mean[2];
        int kind[2];                                        /* -1 no group, 0 behind the batch, 1 in the tail, 2 in the batch */
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int gi = tid + 256 * s;
            const long long v = t0 + 8ll * gi, u = v - a.TL;
            kind[s] = gi >= 256 + own ? -1 : u >= a.n ? 0 : u < 0 ? 1 : 2;
            raw[s][0] = raw[s][1] = raw[s][2] = u32x4{ 0, 0, 0, 0 };
            mean[s] = 0;
            if (kind[s] > 0)
                a.in.load_group(v, raw[s]);
            if (kind[s] == 2)
                mean[s] = a.means[(off + u) >> a.b];
        }
        __syncthreads();                                    /* the tile before is done with the LDS */
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (kind[s] < 0)
                continue;
            const int gi = tid + 256 * s;
            const long long v = t0 + 8ll * gi;
            unsigned byte = 0;
            if (kind[s] == 1) {
                byte = a.bits[v >> 3];
            } else if (kind[s] == 2) {
                uint64_t p[8];
                wb_group_powers(raw[s], p);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    byte |= wb_trigger(a.on != 0, mean[s], p[j], a.thr16) ? 1u << j : 0u;
                if (gi >= own) {                            /* the tile's own samples: counted and carried once */
                    ntrig += __popc(byte);
                    if (v >= a.n)
                        a.new_bits[(v - a.n) >> 3] = (uint8_t)byte;
                }
            }
            trig_bytes[gi] = (uint8_t)byte;
            s_raw[3 * gi] = raw[s][0], s_raw[3 * gi + 1] = raw[s][1], s_raw[3 * gi + 2] = raw[s][2];
        }
        __syncthreads();

        const long long n0 = t0 + 8ll * tid;
        if (n0 < a.n) {
            /* bit i of s_trig is the trigger of span sample i; output n0 + j looks at i = 8 tid + j + delta -+ D */
            const int lo = 8 * tid + a.TL - 2 * a.D, hi = 8 * tid + 7 + a.TL;
            uint32_t any = 0;
            for (int wd = lo >> 5; wd <= hi >> 5; ++wd)
                any |= s_trig[wd];

            /* the 48 bytes from span sample 8 tid + delta on: 13 dwords, shifted by rr bytes */
            uint32_t w[13], o[12];
#pragma unroll
            for (int i = 0; i < 13; ++i)
                w[i] = raw_words[12 * tid + q + i];
#pragma unroll
            for (int i = 0; i < 12; ++i)
                o[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], rr);

            if (any) {
                int num[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 8 * tid + j + delta;
                    int dist = -1;
                    for (int d = 0; d <= a.D; ++d) {
                        const int i0 = c - d, i1 = c + d;
                        if (((s_trig[i0 >> 5] >> (i0 & 31)) | (s_trig[i1 >> 5] >> (i1 & 31))) & 1u) {
                            dist = d;
                            break;
                        }
                    }
                    num[j] = dist < 0 ? -1 : wb_num(dist, a.W);
                    /* counted as the contract counts: outputs made from an input, c = n - D >= 0 */
                    nblank += dist >= 0 && a.N + (uint64_t)(n0 + j) >= (uint64_t)a.D;
                }
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    if (num[2 * h] >= 0 || num[2 * h + 1] >= 0) {
                        int32_t i0, q0, i1, q1;
                        unpack2_msb(o[3 * h], o[3 * h + 1], o[3 * h + 2], i0, q0, i1, q1);
                        i0 = wb_code(i0), q0 = wb_code(q0), i1 = wb_code(i1), q1 = wb_code(q1);
                        if (num[2 * h] >= 0)
                            i0 = wb_scale(i0, num[2 * h], a.r), q0 = wb_scale(q0, num[2 * h], a.r);
                        if (num[2 * h + 1] >= 0)
                            i1 = wb_scale(i1, num[2 * h + 1], a.r), q1 = wb_scale(q1, num[2 * h + 1], a.r);
                        wb_pack2(i0, q0, i1, q1, o[3 * h], o[3 * h + 1], o[3 * h + 2]);
                    }
                }
            }
            u32x4 *dst = reinterpret_cast<u32x4 *>(a.out + n0 * 6);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                u32x4 x;
                x[0] = o[4 * c], x[1] = o[4 * c + 1], x[2] = o[4 * c + 2], x[3] = o[4 * c + 3];
                __builtin_nontemporal_store(x, dst + c);
            }
        }
    }

    if (ntrig)
        atomicAdd(&s_cnt[0], ntrig);
    if (nblank)
        atomicAdd(&s_cnt[1], nblank);
    __syncthreads();
    if (tid == 0 && s_cnt[0])
        atomicAdd(reinterpret_cast<unsigned long long *>(&a.new_st->triggers), (unsigned long long)s_cnt[0]);
    if (tid == 1 && s_cnt[1])
        atomicAdd(reinterpret_cast<unsigned long long *>(&a.new_st->blanked), (unsigned long long)s_cnt[1]);
}

hipError_t launch_wblank_sums(const WbArgs &a, int max_blocks, hipStream_t s)
{
    const long long groups = (a.n + 512) >> 3;
    long long blocks = (groups + 255) / 256;
    blocks = blocks < max_blocks ? blocks : max_blocks;
    hipLaunchKernelGGL(k_wblank_sums, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wblank_means(const WbArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wblank_means, dim3((unsigned)((a.nblocks + 255) / 256 + 1)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wblank_gate(const WbArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wblank_gate, dim3((unsigned)(a.tile_blocks + carry_tail_blocks(a.carry.new_len))), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace pddc
