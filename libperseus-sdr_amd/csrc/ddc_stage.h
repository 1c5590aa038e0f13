/*
 * ddc_stage.h -- what the host files of the per-receiver stages (blanker, receiver filter, demodulator, squelch,
 * adaptive filter, audio, and the mixer behind them) share: device buffers that free themselves, the pair of carried records a batch reads and
 * writes in turn, the receiver table with its upload, the window and twiddles of the stages that transform frames (scope,
 * noise reduction), and the common ends of create / destroy / reset / set_rx / process / read.  A stage's own file keeps its parameters, its table entries, its kernel arguments and its counters.
 * Host only (no kernel includes it); internal, nothing here is exported.
 */
#ifndef PDDC_DDC_STAGE_H
#define PDDC_DDC_STAGE_H

#include "ddc_host.h"
#include "ddc_stage_checks.h"

#include <cmath>
#include <new>
#include <vector>

/* return a PDDC_E* code that is not PDDC_OK */
#define PDDC_TRY(expr)                                                                                          \
    do {                                                                                                        \
        if (const int rc__ = (expr))                                                                            \
            return rc__;                                                                                        \
    } while (0)

namespace pddc {

/* `count` items on the device that is current at alloc(), freed with the object */
template <class T> class DevBuf {
    T *p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)hipFree(p_); }

    int alloc(size_t count, bool zero)
    {
        PDDC_HIP_TRY(hipMalloc(&p_, sizeof(T) * count));
        if (zero)
            PDDC_HIP_TRY(hipMemset(p_, 0, sizeof(T) * count));
        return PDDC_OK;
    }
    /* ... holding v from the start (a prototype, a bank: uploaded once, at create) */
    int alloc_copy(const std::vector<T> &v)
    {
        PDDC_TRY(alloc(v.size(), false));
        PDDC_HIP_TRY(hipMemcpy(p_, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
        return PDDC_OK;
    }
    T *get() const { return p_; }
};

/* The window and the twiddle table of a stage that transforms frames of nfft samples (the scope, the noise reduction:
 * the framed transform of ddc_fft_dev.h), uploaded once, at create.  The twiddles are the panorama's, ddc_spectrum.h: */
int spectrum_twiddle_len(int nfft);
void spectrum_build_twiddles(int nfft, float *tw);

struct FrameTables {
    DevBuf<float> window, twiddles;

    /* the first window value that is not finite, or -1: create tests it before it asks for a device, with its own message */
    static int bad_window(const float *w, int nfft)
    {
        for (int i = 0; i < nfft; ++i)
            if (!std::isfinite(w[i]))
                return i;
        return -1;
    }
    int alloc(int nfft, const float *w)
    {
        std::vector<float> tw((size_t)spectrum_twiddle_len(nfft));
        spectrum_build_twiddles(nfft, tw.data());
        PDDC_TRY(window.alloc_copy(std::vector<float>(w, w + nfft)));
        return twiddles.alloc_copy(tw);
    }
};

/* what a stage carries from batch to batch, twice: a launch reads old() and writes next(); once it was accepted, turn().
 * Nothing on the device is cleared from the host after alloc(): a stage's `fresh` mark tells the kernel not to read. */
template <class T> class Carried {
    DevBuf<T> buf_[2];
    int cur_ = 0;

public:
    int alloc(size_t count)
    {
        PDDC_TRY(buf_[0].alloc(count, true));
        return buf_[1].alloc(count, true);
    }
    T *old() const { return buf_[cur_].get(); }
    T *next() const { return buf_[cur_ ^ 1].get(); }
    void turn() { cur_ ^= 1; }
};

/* One entry per receiver, edited on the host (`host`: create, reset, set_rx, marks that go after an accepted launch) and
 * read by the kernel from the device.  Whoever edits `host` sets `dirty`; process() calls upload() in front of its
 * launch, so the change takes effect in stream order.  `dirty` clears once the copy is enqueued: the bytes are on their
 * way whether or not the launch behind them is accepted.
 * The copy does not read `host` but `staged_`, which upload() alone writes: the runtime may read the source of an
 * asynchronous copy after the call returns, and the host goes on editing `host` meanwhile. */
template <class Rx> class RxTable {
    std::vector<Rx> staged_;
    DevBuf<Rx> dev_;

public:
    std::vector<Rx> host;
    bool dirty = true;

    int alloc() { return dev_.alloc(host.size(), false); }
    int upload(hipStream_t st)
    {
        if (!dirty)
            return PDDC_OK;
        staged_ = host;
        PDDC_HIP_TRY(hipMemcpyAsync(dev_.get(), staged_.data(), sizeof(Rx) * staged_.size(), hipMemcpyHostToDevice, st));
        dirty = false;
        return PDDC_OK;
    }
    const Rx *dev() const { return dev_.get(); }
};

/* What every stage's handle begins with.  The handle types are declared in the public header, under its default
 * visibility, so a handle's destructor says PDDC_LOCAL: the library exports the C ABI and no member of a handle. */
#define PDDC_LOCAL __attribute__((visibility("hidden")))
struct StageBase {
    int device = 0;
    int nrx = 0;
};

inline int null_argument() { return pddc_set_error_(PDDC_EINVAL, "null argument"); }

inline int set_device(int device)
{
    PDDC_HIP_TRY(hipSetDevice(device));
    return PDDC_OK;
}

/* waits for the device's work, then frees; NULL is fine */
template <class S> int stage_destroy(S *s)
{
    if (!s)
        return PDDC_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
    return PDDC_OK;
}

/* The end of create, for a caller that has tested its arguments (so that a bad argument is PDDC_EINVAL with or without
 * a device): the device check, the object, the stage's own `fill` (its members, its allocations on the then current
 * device; -> PDDC_OK or a code) and the hand-over.  A failed create leaves nothing behind: the members free themselves. */
template <class S, class Fill> int stage_create(S **out, int device, int nrx, Fill fill)
{
    PDDC_TRY(pddc_check_device_(device));
    S *s = new (std::nothrow) S;
    if (!s)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    s->device = device;
    s->nrx = nrx;
    int rc = set_device(device);
    if (!rc)
        rc = fill(*s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return PDDC_OK;
}

/* what reset begins with: no batch of this stage is in flight when the host-side marks change */
inline int stage_quiesce(const StageBase *s)
{
    if (!s)
        return null_argument();
    PDDC_TRY(set_device(s->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    return PDDC_OK;
}

/* what set_rx begins with; `stage` as the messages spell it */
inline int stage_rx_ok(const StageBase *s, const char *stage, int rx)
{
    if (!s)
        return null_argument();
    if (rx < 0 || rx >= s->nrx)
        return pddc_set_error_(PDDC_EINVAL, "%s: receiver %d (0 .. %d)", stage, rx, s->nrx - 1);
    return PDDC_OK;
}

/* process(): `p`, the argument called `name`, is a device pointer aligned to 2, 4 or 8 bytes (or NULL, if that may be) */
inline int device_ptr_ok(const void *p, size_t align, const char *name, bool or_null = false)
{
    if (or_null ? aligned_or_null(p, align) : aligned_ptr(p, align))
        return PDDC_OK;
    return pddc_set_error_(PDDC_EINVAL, "%s must be %s %zu-byte aligned device pointer%s", name, align == 8 ? "an" : "a", align,
                           or_null ? " or NULL" : "");
}

/* read(): `count` items at `dev` (NULL: nothing was written yet, and `host` stays as it is) to `host`, behind the
 * batches submitted on `st` so far, and waits for them */
template <class T> int read_back(T *host, const T *dev, size_t count, hipStream_t st)
{
    if (dev)
        PDDC_HIP_TRY(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, st));
    PDDC_HIP_TRY(hipStreamSynchronize(st));
    return PDDC_OK;
}

} // namespace pddc
#endif
