/*
 * ddc_mixer.cpp -- host side of the mixer (include/perseus_ddc.h, pddc_mixer_*): the object, the receivers' gains with
 * their ramps, the cut of a batch into launches, the output counts and the status read.  The kernels are in
 * ddc_mixer.hip.
 * The gain state (from, to and the ramp counter c of every receiver) lives HERE: it is host arithmetic (fmaf is
 * correctly rounded on both sides), and the kernel gets, per launch, the table of the ACTIVE receivers in ascending j
 * with their counters in front of the launch's first sample.  The table is uploaded in stream order whenever it
 * changed: a set_rx, a reset, a ramp under way, a receiver gone silent.
 * A launch has one active set.  A receiver on its way to all-zero gains goes silent at the sample where its counter
 * reaches R, so process() cuts the batch in front of that sample (and every kMixMaxPiece samples, the size of the
 * limiter's workspace); each piece is a batch of its own: upload, k_mix, k_mix_bus, and only then do the counters move.
 * The outputs do not depend on the cut, so neither do they on this one.
 * What is carried on the device, per bus in two records read and written in turn: the status (peak, latest and
 * smallest limiter gain) and, with the limiter, the samples not written yet (fewer than 2 Lb; the count is host
 * arithmetic).  Nothing on the device is cleared from the host: create and reset set `fresh`, read(clear) sets `clear`.
 */
#include "ddc_stage.h"
#include "ddc_mixer.h"

#include <algorithm>
#include <cmath>

using namespace pddc;

typedef unsigned __int128 u128;

struct pddc_mixer : StageBase {
    PDDC_LOCAL ~pddc_mixer() = default;
    pddc_mixer_params par{};
    int Q = 0;
    uint32_t R = 1;
    float invR = 1.0f, invLb = 1.0f;
    bool limit = false;
    /* per receiver, [nrx][kMixMaxBus] with the buses >= Q zero */
    std::vector<float> from, to;
    std::vector<uint32_t> c;                        /* the ramp counter behind the last sample processed, 0 .. R  */
    std::vector<uint8_t> pending;                   /* a set_rx since the last accepted launch: from and c are set */
    RxTable<MixRx> table;                           /* the active receivers first; host.size() == nrx             */
    int nact = 0;
    uint32_t piece_cap = 0;                         /* samples until the table's active set changes (0: no limit) */
    Carried<MixBus> bus;                            /* [Q]                                                        */
    Carried<float> held;                            /* [Q][2 Lb] (limiter)                                        */
    DevBuf<float> y;                                /* [Q][kMixMaxPiece] (limiter)                                */
    DevBuf<float> tile_peak;                        /* [kMixMaxTiles][kMixMaxBus]                                 */
    MixBus host_bus[kMixMaxBus] = {};               /* where read() lands the records                             */
    bool fresh = true;                              /* no launch since create / reset                             */
    bool clear = false;                             /* read(clear) since the last launch                          */
    int held_count = 0;                             /* samples of a bus not written yet, < 2 Lb                   */
    uint64_t N = 0;                                 /* samples since create / reset                               */
};

static_assert(PDDC_MIX_LIMIT == kMixLimit, "the kernel's flag bit is the header's");

/* written so that a NaN fails them */
static bool mix_finite(float v) { return v >= -3.4028234e38f && v <= 3.4028234e38f; }
static bool mix_block_ok(int Lb) { return Lb >= kMixMinBlock && Lb <= kMixMaxBlock; }

/* outputs after N samples: the blocks before the last complete one */
static u128 mix_written(uint64_t Lb, u128 N)
{
    const u128 blocks = N / Lb;
    return blocks > 1 ? (blocks - 1) * Lb : 0;
}

static bool mix_all_zero(const float *g)
{
    for (int q = 0; q < kMixMaxBus; ++q)
        if (g[q] != 0.0f)
            return false;
    return true;
}

/* the gain of receiver j on bus q at its counter: what the last sample processed was given */
static float mix_gain(const pddc_mixer *s, int j, int q)
{
    const size_t at = (size_t)j * kMixMaxBus + (size_t)q;
    if (s->c[(size_t)j] >= s->R)
        return s->to[at];
    return std::fmaf(s->to[at] - s->from[at], (float)s->c[(size_t)j] * s->invR, s->from[at]);
}

/* the table of the receivers that are active at the next sample, and how long that set holds */
static void mix_build_table(pddc_mixer *s)
{
    int p = 0;
    uint32_t cap = 0;
    for (int j = 0; j < s->nrx; ++j) {
        const float *to = &s->to[(size_t)j * kMixMaxBus];
        const uint32_t cj = s->c[(size_t)j];
        if (mix_all_zero(to)) {
            /* silent once the counter is R: at the sample R - c - 1 from here */
            if (cj + 1u >= s->R)
                continue;
            const uint32_t left = s->R - cj - 1u;
            cap = cap ? std::min(cap, left) : left;
        }
        MixRx &r = s->table.host[(size_t)p++];
        r.j = (uint32_t)j;
        r.c = cj;
        for (int q = 0; q < kMixMaxBus; ++q) {
            r.from[q] = s->from[(size_t)j * kMixMaxBus + (size_t)q];
            r.to[q] = to[q];
        }
    }
    s->nact = p;
    s->piece_cap = cap;
    s->table.dirty = true;
}

extern "C" {

int pddc_mixer_chunk(void) { return kMixChunk; }

int pddc_mixer_tile_outputs(void) { return kMixTile; }

uint64_t pddc_mixer_outputs(int block, uint64_t samples_before, size_t n)
{
    if (!mix_block_ok(block))
        return 0;
    const u128 c = mix_written((uint64_t)block, (u128)samples_before + n) - mix_written((uint64_t)block, samples_before);
    return c > (u128)UINT64_MAX ? 0 : (uint64_t)c;
}

int pddc_mixer_create(pddc_mixer **out, int device, int nrx, const pddc_mixer_params *par, const float *gains)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kMixMaxRx || !gains)
        return pddc_set_error_(PDDC_EINVAL, "mixer: %d receivers (1 .. %d) and their gains", nrx, kMixMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "mixer: null parameters");
    if (par->nbus < 1 || par->nbus > kMixMaxBus || par->ramp < 1 || par->ramp > kMixMaxRamp || (par->flags & ~kMixLimit))
        return pddc_set_error_(PDDC_EINVAL, "mixer: %d buses (1 .. %d), ramp %d (1 .. %d), flags 0x%x", par->nbus, kMixMaxBus,
                               par->ramp, kMixMaxRamp, par->flags);
    const bool limit = (par->flags & kMixLimit) != 0u;
    if (limit && (!mix_block_ok(par->block) || !(par->ceil > 0.0f && par->ceil <= 3.4028234e38f) ||
                  !(par->rel > 0.0f && par->rel <= 1.0f)))
        return pddc_set_error_(PDDC_EINVAL, "mixer: limiter block %d (%d .. %d), ceiling %g (finite, > 0), release %g (0 < rel <= 1)",
                               par->block, kMixMinBlock, kMixMaxBlock, (double)par->ceil, (double)par->rel);
    if (!(par->scale > 0.0f && par->scale <= 3.0e38f))
        return pddc_set_error_(PDDC_EINVAL, "mixer: scale %g (finite, > 0)", (double)par->scale);
    const int Q = par->nbus;
    for (int e = 0; e < nrx * Q; ++e)
        if (!mix_finite(gains[e]))
            return pddc_set_error_(PDDC_EINVAL, "mixer: receiver %d: the gain of bus %d is not finite", e / Q, e % Q);
    return stage_create(out, device, nrx, [&](pddc_mixer &s) {
        s.par = *par;
        s.Q = Q;
        s.R = (uint32_t)par->ramp;
        s.invR = 1.0f / (float)par->ramp;
        s.limit = limit;
        s.invLb = limit ? 1.0f / (float)par->block : 1.0f;
        s.to.assign((size_t)nrx * kMixMaxBus, 0.0f);
        for (int j = 0; j < nrx; ++j)
            for (int q = 0; q < Q; ++q)
                s.to[(size_t)j * kMixMaxBus + (size_t)q] = gains[(size_t)j * (size_t)Q + (size_t)q];
        s.from = s.to;
        s.c.assign((size_t)nrx, s.R);
        s.pending.assign((size_t)nrx, 0);
        s.table.host.resize((size_t)nrx);
        mix_build_table(&s);
        PDDC_TRY(s.table.alloc());
        PDDC_TRY(s.bus.alloc(kMixMaxBus));
        PDDC_TRY(s.tile_peak.alloc((size_t)kMixMaxTiles * kMixMaxBus, true));
        if (limit) {
            PDDC_TRY(s.held.alloc((size_t)Q * 2 * (size_t)par->block));
            PDDC_TRY(s.y.alloc((size_t)Q * kMixMaxPiece, true));
        }
        return (int)PDDC_OK;
    });
}

int pddc_mixer_destroy(pddc_mixer *s) { return stage_destroy(s); }

int pddc_mixer_reset(pddc_mixer *s)
{
    PDDC_TRY(stage_quiesce(s));
    s->N = 0;
    s->held_count = 0;
    s->fresh = true;
    s->clear = false;
    std::fill(s->c.begin(), s->c.end(), s->R);
    std::fill(s->pending.begin(), s->pending.end(), (uint8_t)0);
    s->from = s->to;
    mix_build_table(s);
    return PDDC_OK;
}

int pddc_mixer_set_rx(pddc_mixer *s, int rx, const float *gains)
{
    PDDC_TRY(stage_rx_ok(s, "mixer", rx));
    if (!gains)
        return null_argument();
    for (int q = 0; q < s->Q; ++q)
        if (!mix_finite(gains[q]))
            return pddc_set_error_(PDDC_EINVAL, "mixer: the gain of bus %d is not finite", q);
    /* the first call since the last sample fixes where the ramp starts; a later one only moves its end */
    if (!s->pending[(size_t)rx]) {
        float g[kMixMaxBus] = {};
        for (int q = 0; q < s->Q; ++q)
            g[q] = mix_gain(s, rx, q);
        for (int q = 0; q < kMixMaxBus; ++q)
            s->from[(size_t)rx * kMixMaxBus + (size_t)q] = g[q];
        s->c[(size_t)rx] = 0u;
        s->pending[(size_t)rx] = 1;
    }
    for (int q = 0; q < s->Q; ++q)
        s->to[(size_t)rx * kMixMaxBus + (size_t)q] = gains[q];
    mix_build_table(s);
    return PDDC_OK;
}

int pddc_mixer_next_outputs(const pddc_mixer *s, size_t n, size_t *count)
{
    if (!s || !count)
        return null_argument();
    *count = s->limit ? (size_t)pddc_mixer_outputs(s->par.block, s->N, n) : n;
    return PDDC_OK;
}

int pddc_mixer_process(pddc_mixer *s, const void *d_a, size_t n, size_t a_stride, void *d_f32, size_t f32_stride, void *d_i16,
                       size_t i16_cap_frames, size_t *count, void *stream)
{
    if (!s)
        return null_argument();
    const size_t total = s->limit ? (size_t)pddc_mixer_outputs(s->par.block, s->N, n) : n;
    if (n)
        PDDC_TRY(device_ptr_ok(d_a, 4, "d_a"));
    if (total && !d_f32 && !d_i16)
        return pddc_set_error_(PDDC_EINVAL, "mixer: one of d_f32 and d_i16 must be given");
    if (total && !(aligned_or_null(d_f32, 4) && aligned_or_null(d_i16, 2)))
        return pddc_set_error_(PDDC_EINVAL, "d_f32 must be a 4-byte, d_i16 a 2-byte aligned device pointer");
    if (n > a_stride || (d_f32 && total > f32_stride) || (d_i16 && total > i16_cap_frames))
        return pddc_set_error_(PDDC_ECAPACITY, "mixer: %zu samples and %zu outputs, a_stride %zu, f32_stride %zu, %zu int16 frames",
                               n, total, a_stride, f32_stride, i16_cap_frames);
    if (n && total) {
        const size_t ab = rows_extent(s->nrx, n, a_stride, 4);
        if (d_f32 && ranges_overlap(d_f32, rows_extent(s->Q, total, f32_stride, 4), d_a, ab))
            return pddc_set_error_(PDDC_EINVAL, "mixer: f32 overlaps a");
        if (d_i16 && ranges_overlap(d_i16, total * (size_t)s->Q * 2, d_a, ab))
            return pddc_set_error_(PDDC_EINVAL, "mixer: i16 overlaps a");
    }
    if (!n) {
        if (count)
            *count = 0;
        return PDDC_OK;
    }
    PDDC_TRY(set_device(s->device));
    hipStream_t st = (hipStream_t)stream;
    const int Lb = s->limit ? s->par.block : 1;
    size_t done = 0, written = 0;
    while (done < n) {
        size_t len = std::min(n - done, (size_t)kMixMaxPiece);
        if (s->piece_cap)
            len = std::min(len, (size_t)s->piece_cap);
        PDDC_TRY(s->table.upload(st));
        const int tiles = (int)((len + kMixTile - 1) / kMixTile);
        const int cb = s->limit ? (int)(((size_t)s->held_count + len) / (size_t)Lb) : 0;
        const int wn = cb > 1 ? cb - 1 : 0;
        MixArgs a{};
        a.a = static_cast<const float *>(d_a) + done;
        a.a_stride = (long long)a_stride;
        a.n = (int)len;
        a.rx = s->table.dev();
        a.nact = s->nact;
        a.Q = s->Q;
        a.R = s->R;
        a.invR = s->invR;
        a.scale = s->par.scale;
        a.tile_peak = s->tile_peak.get();
        if (s->limit) {
            a.y = s->y.get();
            a.y_stride = kMixMaxPiece;
        } else {
            a.f32 = d_f32 ? static_cast<float *>(d_f32) + done : nullptr;
            a.f32_stride = (long long)f32_stride;
            a.i16 = d_i16 ? static_cast<int16_t *>(d_i16) + done * (size_t)s->Q : nullptr;
        }
        MixBusArgs b{};
        b.y = a.y;
        b.y_stride = a.y_stride;
        b.n = (int)len;
        b.tile_peak = a.tile_peak;
        b.tiles = tiles;
        b.Q = s->Q;
        b.old = s->bus.old();
        b.next = s->bus.next();
        b.fresh = s->fresh ? 1u : 0u;
        b.clear = s->clear ? 1u : 0u;
        b.limit = s->limit ? 1u : 0u;
        b.scale = s->par.scale;
        if (s->limit) {
            b.held_old = s->held.old();
            b.held_next = s->held.next();
            b.held = s->held_count;
            b.write_blocks = wn;
            b.Lb = Lb;
            b.invLb = s->invLb;
            b.ceil = s->par.ceil;
            b.rel = s->par.rel;
            b.f32 = d_f32 ? static_cast<float *>(d_f32) + written : nullptr;
            b.f32_stride = (long long)f32_stride;
            b.i16 = d_i16 ? static_cast<int16_t *>(d_i16) + written * (size_t)s->Q : nullptr;
        }
        PDDC_HIP_TRY(launch_mix(a, st));
        PDDC_HIP_TRY(launch_mix_bus(b, st));
        /* the launches were accepted: only now do the host-side counters move */
        bool moved = false;
        for (int j = 0; j < s->nrx; ++j) {
            uint32_t &cj = s->c[(size_t)j];
            if (cj < s->R) {
                cj = (uint32_t)std::min<uint64_t>((uint64_t)cj + len, s->R);
                moved = true;
            }
            s->pending[(size_t)j] = 0;
        }
        if (moved)
            mix_build_table(s);
        s->bus.turn();
        if (s->limit) {
            s->held.turn();
            s->held_count = (int)((size_t)s->held_count + len - (size_t)wn * (size_t)Lb);
            written += (size_t)wn * (size_t)Lb;
        } else {
            written += len;
        }
        s->N += len;
        s->fresh = false;
        s->clear = false;
        done += len;
    }
    if (count)
        *count = written;
    return PDDC_OK;
}

int pddc_mixer_read(pddc_mixer *s, pddc_mixer_status *host, int clear, void *stream)
{
    if (!s || !host)
        return null_argument();
    PDDC_TRY(set_device(s->device));
    PDDC_TRY(read_back(s->host_bus, s->fresh ? nullptr : s->bus.old(), (size_t)kMixMaxBus, (hipStream_t)stream));
    for (int q = 0; q < s->Q; ++q) {
        const MixBus &r = s->host_bus[q];
        pddc_mixer_status v{ 0.0f, 1.0f, 1.0f };
        if (!s->fresh)
            v = pddc_mixer_status{ s->clear ? 0.0f : r.peak, r.gain, s->clear ? 1.0f : r.min_gain };
        host[q] = v;
    }
    if (clear)
        s->clear = true;
    return PDDC_OK;
}

} // extern "C"
