/*
 * ddc_eq_design.h -- the equaliser's host arithmetic (include/perseus_ddc.h, pddc_eq_*): the stability test a section
 * passes at create and set_rx, and the second-order sections of pddc_eq_design -- the RBJ cookbook's, and two one-pole
 * sections through the bilinear transform -- in double.  No HIP header and nothing of the library: a host compiler builds
 * it alone (tests/eq_design_test.cpp).  Internal; nothing here is exported.
 */
#ifndef PDDC_DDC_EQ_DESIGN_H
#define PDDC_DDC_EQ_DESIGN_H

#include <cmath>

namespace pddc {

/* pddc_eq_section's layout: y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y (a0 = 1) */
struct EqSection {
    double b0, b1, b2, a1, a2;
};

/* PDDC_EQ_LOWPASS .. PDDC_EQ_HIGHPASS1 */
enum EqKind {
    kEqLowpass = 0,
    kEqHighpass = 1,
    kEqBandpass = 2,
    kEqNotch = 3,
    kEqPeak = 4,
    kEqLowshelf = 5,
    kEqHighshelf = 6,
    kEqLowpass1 = 7,
    kEqHighpass1 = 8,
    kEqKinds = 9
};

/* Both poles inside the unit circle -- the triangle |a2| < 1, |a1| < 1 + a2 -- and all five values finite; written so
 * that a NaN fails it */
inline bool eq_section_ok(const EqSection &c)
{
    if (!(std::isfinite(c.b0) && std::isfinite(c.b1) && std::isfinite(c.b2) && std::isfinite(c.a1) && std::isfinite(c.a2)))
        return false;
    return std::fabs(c.a2) < 1.0 && std::fabs(c.a1) < 1.0 + c.a2;
}

/* the arguments pddc_eq_design takes: a kind, 0 < f < rate / 2, q > 0, all finite */
inline bool eq_design_args_ok(int kind, double rate, double f, double q, double gain_db)
{
    if (kind < 0 || kind >= kEqKinds)
        return false;
    if (!(std::isfinite(rate) && std::isfinite(f) && std::isfinite(q) && std::isfinite(gain_db)))
        return false;
    return rate > 0.0 && f > 0.0 && f < 0.5 * rate && q > 0.0;
}

/* The section of `kind` at f Hz of rate Hz -> *out; false, and *out untouched, for arguments outside the above or a
 * result that fails eq_section_ok (a corner so low, or a gain so large, that double does not hold the section).
 * q: the cookbook's Q (for the shelves its slope Q, 1/sqrt(2) the steepest without overshoot); gain_db: PEAK and the
 * shelves.  The one-pole sections take neither. */
inline bool eq_design(int kind, double rate, double f, double q, double gain_db, EqSection *out)
{
    if (!out || !eq_design_args_ok(kind, rate, f, q, gain_db))
        return false;
    const double pi = 3.14159265358979323846;
    EqSection c{};
    if (kind == kEqLowpass1 || kind == kEqHighpass1) {
        /* H(s) = 1 / (1 + s) and s / (1 + s) with s = (1 - z^-1) / (K (1 + z^-1)), K = tan(pi f / rate): half power at f */
        const double K = std::tan(pi * f / rate);
        const double d = 1.0 / (1.0 + K);
        c.a1 = (K - 1.0) * d;
        c.a2 = 0.0;
        c.b2 = 0.0;
        if (kind == kEqLowpass1) {
            c.b0 = K * d;
            c.b1 = K * d;
        } else {
            c.b0 = d;
            c.b1 = -d;
        }
    } else {
        const double w = 2.0 * pi * f / rate;
        const double cs = std::cos(w), sn = std::sin(w);
        const double alpha = sn / (2.0 * q);
        const double A = std::pow(10.0, gain_db / 40.0);
        double b0, b1, b2, a0, a1, a2;
        switch (kind) {
        case kEqLowpass:
            b0 = 0.5 * (1.0 - cs); b1 = 1.0 - cs; b2 = b0;
            a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case kEqHighpass:
            b0 = 0.5 * (1.0 + cs); b1 = -(1.0 + cs); b2 = b0;
            a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case kEqBandpass:
            b0 = alpha; b1 = 0.0; b2 = -alpha;
            a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case kEqNotch:
            b0 = 1.0; b1 = -2.0 * cs; b2 = 1.0;
            a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case kEqPeak:
            b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A;
            a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
            break;
        case kEqLowshelf: {
            const double r = 2.0 * std::sqrt(A) * alpha;
            b0 = A * ((A + 1.0) - (A - 1.0) * cs + r); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs);
            b2 = A * ((A + 1.0) - (A - 1.0) * cs - r);
            a0 = (A + 1.0) + (A - 1.0) * cs + r; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs);
            a2 = (A + 1.0) + (A - 1.0) * cs - r;
            break;
        }
        default: {                                  /* kEqHighshelf */
            const double r = 2.0 * std::sqrt(A) * alpha;
            b0 = A * ((A + 1.0) + (A - 1.0) * cs + r); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs);
            b2 = A * ((A + 1.0) + (A - 1.0) * cs - r);
            a0 = (A + 1.0) - (A - 1.0) * cs + r; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs);
            a2 = (A + 1.0) - (A - 1.0) * cs - r;
            break;
        }
        }
        c.b0 = b0 / a0;
        c.b1 = b1 / a0;
        c.b2 = b2 / a0;
        c.a1 = a1 / a0;
        c.a2 = a2 / a0;
    }
    if (!eq_section_ok(c))
        return false;
    *out = c;
    return true;
}

} // namespace pddc
#endif
