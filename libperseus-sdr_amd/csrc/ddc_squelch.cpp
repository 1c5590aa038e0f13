/*
 * ddc_squelch.cpp -- host side of the squelch (include/perseus_ddc.h, pddc_squelch_*): the object, its receiver table,
 * the sample counter, the launch of a batch and the status read.  The kernel is in ddc_squelch.hip.
 * What is carried per receiver (partial sum, floor, level, peak, open, run, opens, ramp counter) lives on the device in
 * two records, read and written in turn; nothing on the device is cleared from the host: create and reset set `fresh`
 * (the next launch does not read the record, its values are the create values), read(clear_peak) sets `clear_peak` (the
 * next launch takes the carried peak as 0).  Thresholds and flags live in the table, which is uploaded in stream order
 * when it changed.
 */
#include "ddc_stage.h"
#include "ddc_squelch.h"

#include <cmath>
#include <limits>

using namespace pddc;

struct pddc_squelch : StageBase {
    PDDC_LOCAL ~pddc_squelch() = default;
    pddc_squelch_params par{};
    float invB = 0.0f, invR = 0.0f;
    RxTable<SquelchRx> table;
    std::vector<SquelchState> host_state;           /* where read() lands the records                              */
    bool fresh = true;                              /* no launch since create / reset                              */
    bool clear_peak = false;                        /* read(clear_peak) since the last launch                      */
    Carried<SquelchState> state;
    uint64_t N = 0;                                 /* samples per receiver since create / reset                   */
};

static_assert(PDDC_SQL_GATE == kSquelchGate && PDDC_SQL_RELATIVE == kSquelchRelative, "the kernel's flag bits are the header's");

/* written so that a NaN fails it */
static bool squelch_rx_ok(float open_thr, float close_thr, uint32_t flags)
{
    return !(flags & ~(kSquelchGate | kSquelchRelative)) && close_thr >= 0.0f && close_thr <= open_thr && open_thr <= 3.4028234e38f;
}

static bool squelch_block_ok(int B) { return B >= 1 && B <= kSquelchMaxBlock; }

extern "C" {

int pddc_squelch_tile_outputs(void) { return kSquelchTile; }

uint64_t pddc_squelch_blocks(int block, uint64_t samples_before, size_t n)
{
    return squelch_block_ok(block) ? squelch_blocks((uint64_t)block, samples_before, (uint64_t)n) : 0;
}

int pddc_squelch_create(pddc_squelch **out, int device, int nrx, const pddc_squelch_params *par, const pddc_squelch_rx *rx)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nrx < 1 || nrx > kSquelchMaxRx || !rx)
        return pddc_set_error_(PDDC_EINVAL, "squelch: %d receivers (1 .. %d) and their thresholds", nrx, kSquelchMaxRx);
    if (!par)
        return pddc_set_error_(PDDC_EINVAL, "squelch: null parameters");
    if (!squelch_block_ok(par->block) || par->attack < 1 || par->attack > kSquelchMaxCount || par->hang < 1 ||
        par->hang > kSquelchMaxCount || par->ramp < 1 || par->ramp > kSquelchMaxRamp)
        return pddc_set_error_(PDDC_EINVAL, "squelch: block %d (1 .. %d), attack %d, hang %d (1 .. %d), ramp %d (1 .. %d)",
                               par->block, kSquelchMaxBlock, par->attack, par->hang, kSquelchMaxCount, par->ramp, kSquelchMaxRamp);
    if (!(par->up >= 1.0f && par->up <= 3.4028234e38f))
        return pddc_set_error_(PDDC_EINVAL, "squelch: up %g (finite, >= 1)", (double)par->up);
    for (int j = 0; j < nrx; ++j)
        if (!squelch_rx_ok(rx[j].open_thr, rx[j].close_thr, rx[j].flags))
            return pddc_set_error_(PDDC_EINVAL, "squelch: receiver %d: thresholds %g, %g (finite, 0 <= close <= open), flags 0x%x",
                                   j, (double)rx[j].open_thr, (double)rx[j].close_thr, rx[j].flags);
    return stage_create(out, device, nrx, [&](pddc_squelch &s) {
        s.par = *par;
        s.invB = 1.0f / (float)par->block;
        s.invR = 1.0f / (float)par->ramp;
        s.host_state.resize((size_t)nrx);
        for (int j = 0; j < nrx; ++j)
            s.table.host.push_back(SquelchRx{ rx[j].open_thr, rx[j].close_thr, rx[j].flags,
                                              (rx[j].flags & kSquelchGate) ? 0u : (uint32_t)par->ramp });
        PDDC_TRY(s.table.alloc());
        return s.state.alloc((size_t)nrx);
    });
}

int pddc_squelch_destroy(pddc_squelch *s) { return stage_destroy(s); }

int pddc_squelch_reset(pddc_squelch *s)
{
    PDDC_TRY(stage_quiesce(s));
    s->N = 0;
    s->fresh = true;
    s->clear_peak = false;
    for (SquelchRx &r : s->table.host)
        r.c0 = (r.flags & kSquelchGate) ? 0u : (uint32_t)s->par.ramp;
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_squelch_set_rx(pddc_squelch *s, int rx, float open_thr, float close_thr, uint32_t flags)
{
    PDDC_TRY(stage_rx_ok(s, "squelch", rx));
    if (!squelch_rx_ok(open_thr, close_thr, flags))
        return pddc_set_error_(PDDC_EINVAL, "squelch: thresholds %g, %g (finite, 0 <= close <= open), flags 0x%x",
                               (double)open_thr, (double)close_thr, flags);
    SquelchRx &r = s->table.host[(size_t)rx];
    /* nothing carried is reset: c0 is what create / reset made it */
    r.open_thr = open_thr;
    r.close_thr = close_thr;
    r.flags = flags;
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_squelch_next_blocks(const pddc_squelch *s, size_t n, size_t *count)
{
    if (!s || !count)
        return null_argument();
    *count = (size_t)squelch_blocks((uint64_t)s->par.block, s->N, (uint64_t)n);
    return PDDC_OK;
}

int pddc_squelch_process(pddc_squelch *s, const void *d_z, const void *d_a, size_t n, size_t z_stride, size_t a_stride,
                         void *d_out, size_t out_stride, void *d_level, void *d_state, size_t blk_stride, size_t *blocks,
                         void *stream)
{
    if (!s)
        return null_argument();
    const size_t nblk = (size_t)squelch_blocks((uint64_t)s->par.block, s->N, (uint64_t)n);
    if (n) {
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
        PDDC_TRY(device_ptr_ok(d_a, 4, "d_a"));
        PDDC_TRY(device_ptr_ok(d_out, 4, "d_out"));
    }
    if (nblk)
        PDDC_TRY(device_ptr_ok(d_level, 4, "d_level", true));
    if (over_capacity(n, z_stride, a_stride, out_stride))
        return pddc_set_error_(PDDC_ECAPACITY, "squelch: %zu samples per receiver, z_stride %zu, a_stride %zu, out_stride %zu", n,
                               z_stride, a_stride, out_stride);
    if ((d_level || d_state) && nblk > blk_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "squelch: %zu blocks per receiver, blk_stride %zu", nblk, blk_stride);
    if (n) {
        const size_t zb = rows_extent(s->nrx, n, z_stride, 8), ab = rows_extent(s->nrx, n, a_stride, 4),
                     ob = rows_extent(s->nrx, n, out_stride, 4);
        if (ranges_overlap(d_out, ob, d_z, zb))
            return pddc_set_error_(PDDC_EINVAL, "squelch: out overlaps z");
        if (!(d_out == d_a && out_stride == a_stride) && ranges_overlap(d_out, ob, d_a, ab))
            return pddc_set_error_(PDDC_EINVAL, "squelch: out overlaps a (in place is out == a with equal strides)");
    }
    if (!n) {
        if (blocks)
            *blocks = 0;
        return PDDC_OK;
    }
    PDDC_TRY(set_device(s->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(s->table.upload(st));
    SquelchArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.a = static_cast<const float *>(d_a);
    a.a_stride = (long long)a_stride;
    a.out = static_cast<float *>(d_out);
    a.out_stride = (long long)out_stride;
    a.level = nblk ? static_cast<float *>(d_level) : nullptr;
    a.state = nblk ? static_cast<uint8_t *>(d_state) : nullptr;
    a.blk_stride = (long long)blk_stride;
    a.n = (long long)n;
    a.rx = s->table.dev();
    a.nrx = s->nrx;
    a.old = s->state.old();
    a.new_state = s->state.next();
    a.B = (uint32_t)s->par.block;
    a.attack = (uint32_t)s->par.attack;
    a.hang = (uint32_t)s->par.hang;
    a.R = (uint32_t)s->par.ramp;
    a.ph0 = (uint32_t)(s->N % (uint64_t)s->par.block);
    a.magic = meter_magic(a.B);
    a.invB = s->invB;
    a.invR = s->invR;
    a.up = s->par.up;
    a.fresh = s->fresh ? 1u : 0u;
    a.clear_peak = s->clear_peak ? 1u : 0u;
    PDDC_HIP_TRY(launch_squelch(a, st));
    /* the launch was accepted: only now do the host-side counters move */
    s->state.turn();
    s->N += n;
    s->fresh = false;
    s->clear_peak = false;
    if (blocks)
        *blocks = nblk;
    return PDDC_OK;
}

int pddc_squelch_read(pddc_squelch *s, pddc_squelch_status *host, int clear_peak, void *stream)
{
    if (!s || !host)
        return null_argument();
    PDDC_TRY(set_device(s->device));
    PDDC_TRY(read_back(s->host_state.data(), s->fresh ? nullptr : s->state.old(), (size_t)s->nrx, (hipStream_t)stream));
    for (int j = 0; j < s->nrx; ++j) {
        const SquelchState &r = s->host_state[(size_t)j];
        pddc_squelch_status v{ 0.0f, std::numeric_limits<float>::infinity(), 0.0f, 0u, 0u };
        if (!s->fresh)
            v = pddc_squelch_status{ r.level, r.f, s->clear_peak ? 0.0f : r.peak, r.open, r.opens };
        host[j] = v;
    }
    if (clear_peak)
        s->clear_peak = true;
    return PDDC_OK;
}

} // extern "C"
