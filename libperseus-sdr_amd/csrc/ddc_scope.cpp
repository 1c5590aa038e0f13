/*
 * ddc_scope.cpp -- host side of the scope (include/perseus_ddc.h, pddc_scope_*): the object, its slot table, the sample
 * counter, the segment and line arithmetic of a batch and its one launch.  The kernel is in ddc_scope.hip.
 * What is carried per slot (the samples from the start of the first incomplete segment, fewer than nfft; the partial sum
 * of the line under way) lives on the device in two sets of buffers, read and written in turn; nothing on the device is
 * cleared from the host: at create and reset no sample is carried and no line is under way, so the next launch reads
 * neither, and a retargeted slot carries `fresh` in the table, which is uploaded in stream order, until a launch has
 * written its buffers anew.
 */
#include "ddc_stage.h"
#include "ddc_scope.h"

using namespace pddc;

struct pddc_scope : StageBase {                     /* nrx: the slots */
    PDDC_LOCAL ~pddc_scope() = default;
    int nsrc = 0, nfft = 0, hop = 0, avg = 0;
    uint32_t flags = 0;
    FrameTables tables;
    RxTable<ScopeSlot> table;
    Carried<float2> carry;                          /* [nslots][nfft]                                              */
    Carried<float> part;                            /* [nslots][nfft]                                              */
    uint64_t N = 0;                                 /* samples per row since create / reset                        */
};

static_assert(PDDC_SCOPE_CENTERED == kScopeCentered, "the kernel's flag bit is the header's");

static bool scope_sizes_ok(int nfft, int hop, int avg)
{
    if (nfft != 256 && nfft != 512 && nfft != 1024 && nfft != 2048 && nfft != 4096)
        return false;
    return hop >= nfft / kScopeMinHopDiv && hop <= nfft && avg >= 1 && avg <= kScopeMaxAvg;
}

extern "C" {

uint64_t pddc_scope_lines(int nfft, int hop, int avg, uint64_t samples_before, size_t n)
{
    if (!scope_sizes_ok(nfft, hop, avg))
        return 0;
    return windows_complete(nfft, hop, samples_before + n) / (uint64_t)avg - windows_complete(nfft, hop, samples_before) / (uint64_t)avg;
}

uint64_t pddc_scope_next_lines(const pddc_scope *s, size_t n) { return s ? pddc_scope_lines(s->nfft, s->hop, s->avg, s->N, n) : 0; }

int pddc_scope_block_items(int nfft) { return scope_sizes_ok(nfft, nfft, 1) ? scope_items_per_block(nfft) : 0; }

int pddc_scope_create(pddc_scope **out, int device, int nsrc, int nslots, const int *rows, int nfft, int hop, int avg,
                      const float *window, uint32_t flags)
{
    if (!out)
        return null_argument();
    *out = nullptr;
    if (nsrc < 1 || nsrc > kScopeMaxSrc || nslots < 1 || nslots > kScopeMaxSlots || !rows)
        return pddc_set_error_(PDDC_EINVAL, "scope: %d rows (1 .. %d), %d slots (1 .. %d) and their rows", nsrc, kScopeMaxSrc,
                               nslots, kScopeMaxSlots);
    if (!scope_sizes_ok(nfft, hop, avg))
        return pddc_set_error_(PDDC_EINVAL, "scope: nfft %d (256, 512, 1024, 2048 or 4096), hop %d (nfft/16 .. nfft), avg %d (1 .. %d)",
                               nfft, hop, avg, kScopeMaxAvg);
    if (flags & ~kScopeCentered)
        return pddc_set_error_(PDDC_EINVAL, "scope: unknown flags 0x%x", flags);
    if (!window)
        return pddc_set_error_(PDDC_EINVAL, "scope: null window");
    if (const int i = FrameTables::bad_window(window, nfft); i >= 0)
        return pddc_set_error_(PDDC_EINVAL, "scope: window[%d] is not finite", i);
    for (int j = 0; j < nslots; ++j)
        if (rows[j] < -1 || rows[j] >= nsrc)
            return pddc_set_error_(PDDC_EINVAL, "scope: slot %d: row %d (-1: off, 0 .. %d)", j, rows[j], nsrc - 1);
    return stage_create(out, device, nslots, [&](pddc_scope &s) {
        s.nsrc = nsrc;
        s.nfft = nfft;
        s.hop = hop;
        s.avg = avg;
        s.flags = flags;
        for (int j = 0; j < nslots; ++j)
            s.table.host.push_back(ScopeSlot{ rows[j], 0u });
        PDDC_TRY(s.tables.alloc(nfft, window));
        PDDC_TRY(s.table.alloc());
        PDDC_TRY(s.carry.alloc((size_t)nslots * (size_t)nfft));
        return s.part.alloc((size_t)nslots * (size_t)nfft);
    });
}

int pddc_scope_destroy(pddc_scope *s) { return stage_destroy(s); }

int pddc_scope_reset(pddc_scope *s)
{
    PDDC_TRY(stage_quiesce(s));
    s->N = 0;
    return PDDC_OK;
}

int pddc_scope_set_slot(pddc_scope *s, int slot, int row)
{
    if (!s)
        return null_argument();
    if (slot < 0 || slot >= s->nrx || row < -1 || row >= s->nsrc)
        return pddc_set_error_(PDDC_EINVAL, "scope: slot %d (0 .. %d), row %d (-1: off, 0 .. %d)", slot, s->nrx - 1, row,
                               s->nsrc - 1);
    if (s->table.host[(size_t)slot].row == row)
        return PDDC_OK;
    s->table.host[(size_t)slot] = ScopeSlot{ row, 1u };
    s->table.dirty = true;
    return PDDC_OK;
}

int pddc_scope_process(pddc_scope *s, const void *d_z, size_t n, size_t z_stride, void *d_lines, size_t line_stride,
                       size_t *n_lines, void *stream)
{
    if (!s)
        return null_argument();
    const uint64_t S0 = windows_complete(s->nfft, s->hop, s->N), S1 = windows_complete(s->nfft, s->hop, s->N + n);
    const uint64_t A = (uint64_t)s->avg, due = S1 / A - S0 / A;
    if (n)
        PDDC_TRY(device_ptr_ok(d_z, 8, "d_z"));
    PDDC_TRY(device_ptr_ok(d_lines, 16, "d_lines", due == 0));
    if (over_capacity(n, z_stride) || due > line_stride)
        return pddc_set_error_(PDDC_ECAPACITY, "scope: %zu samples per row, z_stride %zu; %llu lines due, line_stride %zu", n,
                               z_stride, (unsigned long long)due, line_stride);
    if (due && ranges_overlap(d_lines, rows_extent(s->nrx, (size_t)due, line_stride, sizeof(float) * (size_t)s->nfft), d_z,
                              rows_extent(s->nsrc, n, z_stride, 8)))
        return pddc_set_error_(PDDC_EINVAL, "scope: lines overlap z");
    const uint64_t nseg = S1 - S0, i0 = S0 % A;
    const uint64_t nunits = due + ((i0 + nseg) % A ? 1 : 0);
    if (n && (nunits > 0x7fffffffull || !scope_blocks(s->nfft, s->nrx, (int)nunits)))
        return pddc_set_error_(PDDC_ECAPACITY, "scope: %llu lines of %d slots are more than one launch holds", (unsigned long long)due,
                               s->nrx);
    if (!n) {
        if (n_lines)
            *n_lines = 0;
        return PDDC_OK;
    }
    PDDC_TRY(set_device(s->device));
    hipStream_t st = (hipStream_t)stream;
    PDDC_TRY(s->table.upload(st));
    ScopeArgs a{};
    a.z = static_cast<const float2 *>(d_z);
    a.z_stride = (long long)z_stride;
    a.n = (long long)n;
    a.slots = s->table.dev();
    a.nslots = s->nrx;
    a.lines = static_cast<float *>(d_lines);
    a.line_stride = (long long)line_stride;
    a.old_carry = s->carry.old();
    a.new_carry = s->carry.next();
    a.old_part = s->part.old();
    a.new_part = s->part.next();
    a.window = s->tables.window.get();
    a.twiddles = s->tables.twiddles.get();
    a.hop = s->hop;
    a.avg = s->avg;
    a.clen = (int)(s->N - S0 * (uint64_t)s->hop);
    a.new_clen = (int)(s->N + n - S1 * (uint64_t)s->hop);
    a.i0 = (int)i0;
    a.nseg = (long long)nseg;
    a.nlines = (long long)due;
    a.nunits = (int)nunits;
    a.flags = s->flags;
    PDDC_HIP_TRY(launch_scope(s->nfft, a, st));
    /* the launch was accepted: only now do the host-side marks move */
    s->carry.turn();
    s->part.turn();
    s->N += n;
    for (ScopeSlot &sl : s->table.host)
        if (sl.fresh) {
            sl.fresh = 0u;
            s->table.dirty = true;
        }
    if (n_lines)
        *n_lines = (size_t)due;
    return PDDC_OK;
}

} // extern "C"
