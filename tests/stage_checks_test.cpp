/* tests/stage_checks_test.cpp -- the arithmetic behind the argument tests of the per-receiver stages' process()
 * (csrc/ddc_stage_checks.h: no HIP header, so a host compiler builds it alone): whether two byte ranges meet, the bytes a
 * set of rows spans, pointer alignment, the squelch's completed blocks against a counting loop, and the block meter's
 * multiply-and-shift against the division.
 * usage: stage_checks_test   -> prints "ok: <checks> checks", exit 0; the first failed check is printed, exit 1 */
#include <stdio.h>
#include <stdlib.h>
#include "ddc_stage_checks.h"

using namespace pddc;

static long checks = 0;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        ++checks;                                                                                               \
        if (!(cond)) {                                                                                          \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                                                    \
            exit(1);                                                                                            \
        }                                                                                                       \
    } while (0)

/* both orders of the arguments must agree */
static bool meet(const void *p, size_t pb, const void *q, size_t qb)
{
    const bool a = ranges_overlap(p, pb, q, qb), b = ranges_overlap(q, qb, p, pb);
    CHECK(a == b);
    return a;
}

static void test_ranges_overlap()
{
    alignas(8) static char buf[64];
    CHECK(!meet(buf, 8, buf + 16, 8));          /* disjoint */
    CHECK(!meet(buf, 16, buf + 16, 8));         /* touch end to start */
    CHECK(meet(buf, 17, buf + 16, 8));          /* share exactly one byte */
    CHECK(meet(buf + 8, 8, buf + 8, 8));        /* identical */
    CHECK(meet(buf, 64, buf + 24, 4));          /* one inside the other */
    CHECK(meet(buf, 64, buf, 1) && meet(buf, 64, buf + 63, 1));
    /* hulls: rows of 3 items at a stride of 7 and the rows that lie in their gaps share no byte, and meet */
    CHECK(meet(buf, rows_extent(3, 3, 7, 1), buf + 3, rows_extent(3, 3, 7, 1)));
}

static void test_rows_extent()
{
    const size_t strides[] = { 0, 1, 3, 7, 1000 }, items[] = { 2, 4, 8 };
    for (size_t stride : strides)
        for (size_t item : items)
            CHECK(rows_extent(1, 3, stride, item) == 3 * item);     /* one row: n items whatever the stride */
    for (size_t item : items)
        CHECK(rows_extent(5, 3, 7, item) == (4 * 7 + 3) * item);
    CHECK(rows_extent(5, 3, 7, 1) == 31);
    CHECK(rows_extent(2, 0, 9, 4) == 36);
}

static void test_alignment()
{
    alignas(8) static char buf[16];
    const size_t aligns[] = { 2, 4, 8 };
    for (size_t al : aligns) {
        CHECK(!aligned_ptr(nullptr, al));
        CHECK(aligned_or_null(nullptr, al));
        CHECK(aligned_ptr(buf, al) && aligned_or_null(buf, al));
        CHECK(aligned_ptr(buf + 8, al));
        CHECK(!aligned_ptr(buf + 1, al) && !aligned_or_null(buf + 1, al));
        CHECK(aligned_ptr(buf + al, al));
        CHECK(!aligned_ptr(buf + al / 2, al) && !aligned_or_null(buf + al / 2, al));
    }
    CHECK(aligned_ptr(buf + 4, 4) && !aligned_ptr(buf + 4, 8) && aligned_ptr(buf + 2, 2) && !aligned_ptr(buf + 2, 4));
}

static void test_over_capacity()
{
    CHECK(!over_capacity(0, (size_t)0) && !over_capacity(5, (size_t)5, (size_t)9) && over_capacity(5, (size_t)4));
    CHECK(over_capacity(5, (size_t)9, (size_t)4) && over_capacity(5, (size_t)9, (size_t)9, (size_t)4));
}

static void test_squelch_blocks()
{
    const uint64_t Bs[] = { 1, 2, 48, 4095, 4096 };
    for (uint64_t B : Bs) {
        const uint64_t ks[] = { 0, 1, 7, ((uint64_t)1 << 63) / B, (((uint64_t)1 << 63) + ((uint64_t)1 << 62)) / B };
        const uint64_t ns[] = { 0, 1, B - 1, B, B + 1, 2 * B + 1, 3 * B };
        for (uint64_t k : ks)
            for (int d = -2; d <= 2; ++d) {
                if (k == 0 && d < 0)
                    continue;
                const uint64_t before = k * B + (uint64_t)(int64_t)d;
                for (uint64_t n : ns) {
                    uint64_t count = 0;
                    for (uint64_t i = 1; i <= n; ++i)
                        count += (before + i) % B == 0;
                    CHECK(squelch_blocks(B, before, n) == count);
                }
            }
    }
}

/* every x a kernel divides (below two tiles of 256) by every B that takes the multiply (below a tile) */
static void test_meter_magic()
{
    for (uint32_t B = 1; B < 256; ++B)
        for (uint32_t x = 0; x < 512; ++x)
            CHECK((x * meter_magic(B)) >> kMeterDivShift == x / B);
}

int main()
{
    test_ranges_overlap();
    test_rows_extent();
    test_alignment();
    test_over_capacity();
    test_squelch_blocks();
    test_meter_magic();
    printf("ok: %ld checks\n", checks);
    return 0;
}
