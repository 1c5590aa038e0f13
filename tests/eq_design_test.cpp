/* tests/eq_design_test.cpp -- the equaliser's host arithmetic (csrc/ddc_eq_design.h: no HIP header, so a host compiler
 * builds it alone): the stability triangle on, just inside and just outside its edges, values that are not finite, the
 * designs' argument tests, and the designs at the ends of their argument ranges -- every section they give is stable, or
 * the design says that it has none.
 * usage: eq_design_test   -> prints "ok: <checks> checks", exit 0; the first failed check is printed, exit 1 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "ddc_eq_design.h"

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

static bool ok(double a1, double a2) { return eq_section_ok(EqSection{ 1.0, 0.0, 0.0, a1, a2 }); }

static void test_triangle()
{
    const double e = 2.220446049250313e-16;        /* 2^-52 */
    CHECK(ok(0.0, 0.0));
    /* the edge a2 = 1, and the corners */
    CHECK(!ok(0.0, 1.0) && ok(0.0, 1.0 - e) && !ok(0.0, 1.0 + e));
    CHECK(!ok(2.0, 1.0) && !ok(-2.0, 1.0) && !ok(0.0, -1.0));
    CHECK(ok(0.0, -1.0 + e) && !ok(0.0, -1.0 - e));
    /* the edges |a1| = 1 + a2 */
    const double a2s[] = { -0.5, 0.0, 0.25, 0.5, 0.96875 };
    for (double a2 : a2s) {
        const double edge = 1.0 + a2;              /* exact for these */
        CHECK(!ok(edge, a2) && !ok(-edge, a2));
        CHECK(ok(nextafter(edge, 0.0), a2) && ok(-nextafter(edge, 0.0), a2));
        CHECK(!ok(nextafter(edge, 4.0), a2) && !ok(-nextafter(edge, 4.0), a2));
    }
    CHECK(!ok(2.0, 0.5) && !ok(1.5, 0.5) && ok(1.4999, 0.5));
    /* the issue's two: a1 = 2, a2 = 1 */
    CHECK(!ok(2.0, 0.99) && !ok(0.5, 1.0));
    /* not finite, in every place */
    const double bad[] = { NAN, INFINITY, -INFINITY };
    for (double v : bad) {
        CHECK(!eq_section_ok(EqSection{ v, 0.0, 0.0, 0.0, 0.0 }));
        CHECK(!eq_section_ok(EqSection{ 1.0, v, 0.0, 0.0, 0.0 }));
        CHECK(!eq_section_ok(EqSection{ 1.0, 0.0, v, 0.0, 0.0 }));
        CHECK(!eq_section_ok(EqSection{ 1.0, 0.0, 0.0, v, 0.0 }));
        CHECK(!eq_section_ok(EqSection{ 1.0, 0.0, 0.0, 0.0, v }));
    }
    /* large but finite numerators are the caller's business */
    CHECK(eq_section_ok(EqSection{ 1e300, -1e300, 1e300, 0.0, 0.0 }));
}

static void test_arguments()
{
    EqSection c{ 7.0, 7.0, 7.0, 7.0, 7.0 };
    const double rate = 48000.0;
    CHECK(!eq_design(-1, rate, 1000.0, 1.0, 0.0, &c) && !eq_design(kEqKinds, rate, 1000.0, 1.0, 0.0, &c));
    CHECK(!eq_design(kEqPeak, rate, 0.0, 1.0, 0.0, &c) && !eq_design(kEqPeak, rate, -1.0, 1.0, 0.0, &c));
    CHECK(!eq_design(kEqPeak, rate, 24000.0, 1.0, 0.0, &c) && !eq_design(kEqPeak, rate, 30000.0, 1.0, 0.0, &c));
    CHECK(!eq_design(kEqPeak, rate, 1000.0, 0.0, 0.0, &c) && !eq_design(kEqPeak, rate, 1000.0, -1.0, 0.0, &c));
    CHECK(!eq_design(kEqPeak, 0.0, 1000.0, 1.0, 0.0, &c) && !eq_design(kEqPeak, -rate, 1000.0, 1.0, 0.0, &c));
    const double bad[] = { NAN, INFINITY, -INFINITY };
    for (double v : bad) {
        CHECK(!eq_design(kEqPeak, v, 1000.0, 1.0, 0.0, &c) && !eq_design(kEqPeak, rate, v, 1.0, 0.0, &c));
        CHECK(!eq_design(kEqPeak, rate, 1000.0, v, 0.0, &c) && !eq_design(kEqPeak, rate, 1000.0, 1.0, v, &c));
    }
    CHECK(!eq_design(kEqPeak, rate, 1000.0, 1.0, 0.0, nullptr));
    /* a refusal leaves *out alone */
    CHECK(c.b0 == 7.0 && c.b1 == 7.0 && c.b2 == 7.0 && c.a1 == 7.0 && c.a2 == 7.0);
    CHECK(eq_design(kEqPeak, rate, 1000.0, 1.0, 0.0, &c) && c.b0 != 7.0);
}

/* every kind over the ends of the ranges: a section that comes out is stable, and in the ordinary range one comes out */
static void test_ends()
{
    const double rates[] = { 9765.625, 48000.0 };
    const double rel[] = { 1e-12, 1e-9, 1e-6, 1e-4, 2e-3, 0.01, 0.1, 0.25, 0.4, 0.49, 0.4999, 0.4999999, 0.5 - 1e-12 };
    const double qs[] = { 1e-6, 1e-3, 0.1, 0.5, 0.70710678118654752, 1.0, 10.0, 30.0, 1000.0, 1e6, 1e12 };
    const double gains[] = { -400.0, -60.0, -18.0, -1.0, 0.0, 1.0, 18.0, 60.0, 400.0, 20000.0 };
    long made = 0;
    for (int kind = 0; kind < kEqKinds; ++kind)
        for (double rate : rates)
            for (double r : rel)
                for (double q : qs)
                    for (double g : gains) {
                        EqSection c{ 7.0, 7.0, 7.0, 7.0, 7.0 };
                        const bool got = eq_design(kind, rate, r * rate, q, g, &c);
                        if (got) {
                            ++made;
                            CHECK(eq_section_ok(c));
                        } else {
                            CHECK(c.b0 == 7.0 && c.a2 == 7.0);
                        }
                        const bool ordinary = r >= 2e-3 && r <= 0.49 && q >= 0.1 && q <= 30.0 && g >= -60.0 && g <= 60.0;
                        if (ordinary)
                            CHECK(got);
                    }
    CHECK(made > 10000);
    /* the one-pole sections have no second-order part, and unity at their pass end */
    EqSection c{};
    CHECK(eq_design(kEqLowpass1, 48000.0, 2122.0, 1.0, 0.0, &c) && c.b2 == 0.0 && c.a2 == 0.0 && c.b0 == c.b1);
    CHECK(fabs((c.b0 + c.b1) / (1.0 + c.a1) - 1.0) < 1e-15);
    CHECK(eq_design(kEqHighpass1, 48000.0, 100.0, 1.0, 0.0, &c) && c.b2 == 0.0 && c.a2 == 0.0 && c.b0 == -c.b1);
    CHECK(fabs((c.b0 - c.b1) / (1.0 - c.a1) - 1.0) < 1e-15);
}

int main()
{
    test_triangle();
    test_arguments();
    test_ends();
    printf("ok: %ld checks\n", checks);
    return 0;
}
