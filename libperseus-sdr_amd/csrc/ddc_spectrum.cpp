/*
 * ddc_spectrum.cpp -- host side of the panorama (include/perseus_ddc.h, pddc_spectrum_*): the object, its counters, and
 * the two launches of a batch.  The carried tail is a PackedCarry (ddc_packed.h); the kernels are in ddc_spectrum.hip.
 */
#include "ddc_spectrum.h"

#include <new>
#include <vector>

using namespace pddc;

struct pddc_spectrum {
    int device = 0;
    int nfft = 0, hop = 0;
    uint32_t flags = 0;
    int max_blocks = 0;
    float *d_window = nullptr, *d_tw = nullptr;
    PackedCarry in;                                 /* the carried tail (a window of nfft) and the stream length */
    uint64_t segments = 0;                          /* accumulated since the last clear        */
    float *d_part_sum = nullptr, *d_part_peak = nullptr;
    double *d_acc_sum = nullptr;
    float *d_acc_peak = nullptr;
};

static bool spec_sizes_ok(int nfft, int hop)
{
    if (nfft != 1024 && nfft != 2048 && nfft != 4096 && nfft != 8192)
        return false;
    return hop == nfft || hop == nfft / 2;
}

static void spec_free(pddc_spectrum *s)
{
    hipFree(s->d_window);
    hipFree(s->d_tw);
    s->in.free();
    hipFree(s->d_part_sum);
    hipFree(s->d_part_peak);
    hipFree(s->d_acc_sum);
    hipFree(s->d_acc_peak);
    delete s;
}

static int spec_create(pddc_spectrum *s, const float *window)
{
    const size_t n = (size_t)s->nfft;
    PDDC_HIP_TRY(hipSetDevice(s->device));
    int ncu = 0;
    PDDC_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device));
    s->max_blocks = spectrum_max_blocks(s->nfft, ncu > 0 ? ncu : 256);
    std::vector<float> tw((size_t)spectrum_twiddle_len(s->nfft));
    spectrum_build_twiddles(s->nfft, tw.data());
    PDDC_HIP_TRY(hipMalloc(&s->d_window, n * sizeof(float)));
    PDDC_HIP_TRY(hipMalloc(&s->d_tw, tw.size() * sizeof(float)));
    PDDC_HIP_TRY(s->in.alloc(n));
    PDDC_HIP_TRY(hipMalloc(&s->d_part_sum, (size_t)s->max_blocks * n * sizeof(float)));
    PDDC_HIP_TRY(hipMalloc(&s->d_acc_sum, n * sizeof(double)));
    if (s->flags & PDDC_SPEC_PEAK) {
        PDDC_HIP_TRY(hipMalloc(&s->d_part_peak, (size_t)s->max_blocks * n * sizeof(float)));
        PDDC_HIP_TRY(hipMalloc(&s->d_acc_peak, n * sizeof(float)));
        PDDC_HIP_TRY(hipMemset(s->d_acc_peak, 0, n * sizeof(float)));
    }
    PDDC_HIP_TRY(hipMemcpy(s->d_window, window, n * sizeof(float), hipMemcpyHostToDevice));
    PDDC_HIP_TRY(hipMemcpy(s->d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
    PDDC_HIP_TRY(hipMemset(s->d_acc_sum, 0, n * sizeof(double)));
    return PDDC_OK;
}

extern "C" {

uint64_t pddc_spectrum_segments(int nfft, int hop, uint64_t samples_before, size_t nsamples)
{
    if (!spec_sizes_ok(nfft, hop))
        return 0;
    return windows_complete(nfft, hop, samples_before + nsamples) - windows_complete(nfft, hop, samples_before);
}

uint64_t pddc_spectrum_next_segments(const pddc_spectrum *s, size_t nsamples)
{
    return s ? pddc_spectrum_segments(s->nfft, s->hop, s->in.samples, nsamples) : 0;
}

int pddc_spectrum_create(pddc_spectrum **out, int device, int nfft, int hop, const float *window, uint32_t flags)
{
    if (!out)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    *out = nullptr;
    if (!spec_sizes_ok(nfft, hop))
        return pddc_set_error_(PDDC_EINVAL, "spectrum: nfft %d (1024, 2048, 4096 or 8192), hop %d (nfft or nfft/2)", nfft,
                               hop);
    if (!window)
        return pddc_set_error_(PDDC_EINVAL, "spectrum: null window");
    if (flags & ~PDDC_SPEC_PEAK)
        return pddc_set_error_(PDDC_EINVAL, "spectrum: unknown flags 0x%x", flags);
    if (const int rc = pddc_check_device_(device))
        return rc;
    pddc_spectrum *s = new (std::nothrow) pddc_spectrum;
    if (!s)
        return pddc_set_error_(PDDC_ENOMEM, "out of memory");
    s->device = device;
    s->nfft = nfft;
    s->hop = hop;
    s->flags = flags;
    const int rc = spec_create(s, window);
    if (rc) {
        spec_free(s);
        return rc;
    }
    *out = s;
    return PDDC_OK;
}

int pddc_spectrum_destroy(pddc_spectrum *s)
{
    if (!s)
        return PDDC_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    spec_free(s);
    return PDDC_OK;
}

int pddc_spectrum_reset(pddc_spectrum *s)
{
    if (!s)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    PDDC_HIP_TRY(hipSetDevice(s->device));
    PDDC_HIP_TRY(hipDeviceSynchronize());
    PDDC_HIP_TRY(hipMemset(s->d_acc_sum, 0, (size_t)s->nfft * sizeof(double)));
    if (s->d_acc_peak)
        PDDC_HIP_TRY(hipMemset(s->d_acc_peak, 0, (size_t)s->nfft * sizeof(float)));
    s->in.reset();
    s->segments = 0;
    return PDDC_OK;
}

int pddc_spectrum_process(pddc_spectrum *s, const void *d_packed, size_t nsamples, void *stream)
{
    if (!s)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (const int rc = PackedCarry::check(d_packed, nsamples))
        return rc;
    if (!nsamples)
        return PDDC_OK;
    PDDC_HIP_TRY(hipSetDevice(s->device));
    const PackedCarry::Plan plan = s->in.plan(nsamples, s->nfft, s->hop);
    const uint64_t nseg = plan.n_complete;
    const int blocks = (int)(nseg < (uint64_t)s->max_blocks ? nseg : (uint64_t)s->max_blocks);
    hipStream_t st = (hipStream_t)stream;
    if (nseg) {
        SpectrumArgs a{};
        a.in = s->in.stream(d_packed);
        a.nseg = (long long)nseg;
        a.hop = s->hop;
        a.window = s->d_window;
        a.twiddles = s->d_tw;
        a.part_sum = s->d_part_sum;
        a.part_peak = s->d_part_peak;
        PDDC_HIP_TRY(launch_spectrum(s->nfft, a, blocks, st));
    }
    SpectrumFoldArgs f{};
    f.part_sum = s->d_part_sum;
    f.part_peak = s->d_part_peak;
    f.nparts = blocks;
    f.nfft = s->nfft;
    f.acc_sum = s->d_acc_sum;
    f.acc_peak = s->d_acc_peak;
    f.carry = s->in.carry(plan, d_packed);
    PDDC_HIP_TRY(launch_spectrum_fold(f, st));
    /* both launches were accepted: only now do the host-side counters move */
    s->in.commit(plan, nsamples);
    s->segments += nseg;
    return PDDC_OK;
}

int pddc_spectrum_read(pddc_spectrum *s, void *d_sum, void *d_peak, uint64_t *nsegments, int clear, void *stream)
{
    if (!s)
        return pddc_set_error_(PDDC_EINVAL, "null argument");
    if (d_peak && !(s->flags & PDDC_SPEC_PEAK))
        return pddc_set_error_(PDDC_EINVAL, "spectrum: created without PDDC_SPEC_PEAK");
    PDDC_HIP_TRY(hipSetDevice(s->device));
    if (d_sum || d_peak || clear)
        PDDC_HIP_TRY(launch_spectrum_read(s->nfft, s->d_acc_sum, s->d_acc_peak, static_cast<float *>(d_sum),
                                          static_cast<float *>(d_peak), clear, (hipStream_t)stream));
    if (nsegments)
        *nsegments = s->segments;
    if (clear)
        s->segments = 0;
    return PDDC_OK;
}

} // extern "C"
