// call_util.hpp — what the two-call entry points with caller-allocated outputs share (ewise.hip, coo.hip, g4s_csr_row_indices): an owned block of the
// caching allocator, the overlap check of host arrays, the capture refusal, the upload of a host array and the combiners.
#pragma once
#include "common.hpp"

namespace {   // (one copy per translation unit, as the kernels of prims.hpp)

struct BigBuf {
    void *p = nullptr;
    bool idle = false;
    BigBuf() = default;
    BigBuf(const BigBuf &) = delete;
    BigBuf &operator=(const BigBuf &) = delete;
    ~BigBuf() { if (p) (void)g4s::big_free(p, idle); }
    int alloc(size_t bytes) { return g4s::big_alloc(&p, bytes); }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const char *x = static_cast<const char *>(a), *y = static_cast<const char *>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

struct Span {
    const void *p;
    size_t bytes;
};

template <size_t NO, size_t NI>
bool any_overlap(const Span (&outs)[NO], const Span (&ins)[NI])
{
    for (const Span &o : outs)
        for (const Span &i : ins)
            if (overlap(o.p, o.bytes, i.p, i.bytes)) return true;
    for (size_t x = 0; x < NO; ++x)
        for (size_t y = x + 1; y < NO; ++y)
            if (overlap(outs[x].p, outs[x].bytes, outs[y].p, outs[y].bytes)) return true;
    return false;
}

inline int not_capturing(const char *fn, hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    G4S_HIP_TRY(hipStreamIsCapturing(s, &cs));
    if (cs != hipStreamCaptureStatusNone) return g4s::set_error(G4S_ERR_INVALID, "%s: the call reads counts back and cannot be captured", fn);
    return G4S_OK;
}

inline int upload(BigBuf &b, const void *src, size_t bytes, hipStream_t s)
{
    G4S_TRY(b.alloc(bytes));
    if (bytes && src) G4S_HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
    return G4S_OK;
}

inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

// x ⊕ y of a G4S_COMBINE_* value: one IEEE operation or a copy
__device__ __forceinline__ double combine_values(int combine, double x, double y)
{
    switch (combine) {
    case G4S_COMBINE_PLUS: return x + y;
    case G4S_COMBINE_TIMES: return x * y;
    case G4S_COMBINE_MIN: return y < x ? y : x;
    case G4S_COMBINE_MAX: return x < y ? y : x;
    case G4S_COMBINE_FIRST: return x;
    default: return y;
    }
}

} // namespace
