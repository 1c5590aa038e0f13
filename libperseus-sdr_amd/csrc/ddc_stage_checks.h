/*
 * ddc_stage_checks.h -- the arithmetic behind the argument tests of the per-receiver stages' process() (ddc_stage.h):
 * pointers, capacities, the bytes a set of rows spans, whether two spans meet, the squelch's block count and the block
 * meter's division constant.  No HIP header: a host compiler builds it alone (tests/stage_checks_test.cpp).  Internal;
 * nothing here is exported.
 */
#ifndef PDDC_DDC_STAGE_CHECKS_H
#define PDDC_DDC_STAGE_CHECKS_H

#include <stddef.h>
#include <stdint.h>

namespace pddc {

/* p is a multiple of `align` (a power of two) ... */
inline bool aligned_or_null(const void *p, size_t align) { return !((uintptr_t)p & (align - 1)); }
/* ... and not NULL */
inline bool aligned_ptr(const void *p, size_t align) { return p && aligned_or_null(p, align); }

/* n items per row do not fit one of the row strides */
template <class... S> inline bool over_capacity(size_t n, S... strides) { return ((n > (size_t)strides) || ...); }

/* bytes from the first item of row 0 to the end of row nrx - 1: nrx >= 1 rows of n items of `item` bytes, `stride` items
 * apart.  Not bounded: it can wrap for absurd strides (the receiver filter alone limits them before it asks) */
inline size_t rows_extent(int nrx, size_t n, size_t stride, size_t item) { return ((size_t)(nrx - 1) * stride + n) * item; }

/* byte ranges [p, p + bytes) and [q, q + qbytes) share a byte.  With rows_extent() this compares the hulls of two row
 * sets: interleaved rows that share no byte meet as well */
inline bool ranges_overlap(const void *p, size_t bytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + bytes;
}

/* blocks of B samples that n samples after `before` complete */
inline uint64_t squelch_blocks(uint64_t B, uint64_t before, uint64_t n) { return (before + n) / B - before / B; }

/* The block meter's division (ddc_meter_dev.h; squelch and blanker): x / B = (x * meter_magic(B)) >> kMeterDivShift for
 * x < 512 (two tiles) and B < 256 (a tile).  Host and device; a launcher refuses arguments whose magic is another number. */
static constexpr int kMeterDivShift = 20;
constexpr uint32_t meter_magic(uint32_t B) { return ((1u << kMeterDivShift) + B - 1u) / B; }

} // namespace pddc
#endif
