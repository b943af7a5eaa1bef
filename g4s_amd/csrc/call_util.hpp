// call_util.hpp — what the entry points that take host or device arrays and read a verdict back share (ewise.hip, extract.hip, coo.hip, spgemm_masked.hip,
// transpose.hip's g4s_csr_row_indices, pagerank.hip, traverse.hip, betweenness.hip and the graph calls on raw CSR arrays: components.hip, kcore.hip, color.hip,
// ktruss.hip, scc.hip, msf.hip, and trsv.hip): an owned block of the caching allocator, the carver of a work block, the staging frame of a call with host pointers, the overlap
// check of host arrays, the capture refusal, the capped grid, the combiners, and for the graph calls the environment switch, the launch counts and the
// text of a refused pattern.
#pragma once
#include "common.hpp"
#include <algorithm>
#include <cstdlib>

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

// why: what the call reads back, for the refusal's message
inline int not_capturing(const char *fn, hipStream_t s, const char *why = "counts")
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    G4S_HIP_TRY(hipStreamIsCapturing(s, &cs));
    if (cs != hipStreamCaptureStatusNone) return g4s::set_error(G4S_ERR_INVALID, "%s: the call reads %s back and cannot be captured", fn, why);
    return G4S_OK;
}

inline int upload(BigBuf &b, const void *src, size_t bytes, hipStream_t s)
{
    G4S_TRY(b.alloc(bytes));
    if (bytes && src) G4S_HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
    return G4S_OK;
}

inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

// the workgroups of a grid-stride kernel over n elements: at least one, at most cap
template <int WG_>
inline int grid_for(long long n, long long cap) { return (int)std::max(1LL, std::min((n + WG_ - 1) / WG_, cap)); }

// an A/B switch of the environment clamped to [lo, hi]; dflt when it is not set
inline int env_int(const char *name, int dflt, int lo, int hi)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    return std::max(lo, std::min(hi, atoi(e)));
}

// what a stepped graph call reports of its own host loop (g4s_*_info: launches, resumes, host_waits)
struct Counts {
    int launches = 0, resumes = 0, waits = 0;
};

// The bits an opening pass (frontier.hpp) leaves in a state block's `invalid` word, as the refusal's text: 1 rowptr, 2 an id, 4 the order inside a row.
// NULL when none of them is set: the caller's own bits.
inline const char *csr_invalid_text(int bits)
{
    return (bits & 1) ? "rowptr must start at 0 and never decrease" : (bits & 2) ? "a column id is outside [0, n)" : (bits & 4) ? "a row is not strictly ascending" : nullptr;
}

// One work block cut into arrays. piece() declares them in order, each padded to 256 bytes (tail(): unpadded, for the last one); alloc() makes the one
// big_alloc of their sum and sets the pointers. idle(): the stream that used the block has been synchronised — without it the block is released behind a
// device-wide wait, which is what an early return gets. A call with a staging frame says it right behind Staged::finish, whatever the status.
class Carver {
    struct Piece {
        void *slot;
        void (*set)(void *slot, char *at);
        size_t off;
    };
    static constexpr int kMax = 16;
    Piece pc_[kMax];
    int n_ = 0;
    size_t bytes_ = 0;
    BigBuf buf_;
    template <typename T>
    void add(T **p, size_t bytes)
    {
        if (n_ < kMax) pc_[n_] = Piece{p, [](void *slot, char *at) { *static_cast<T **>(slot) = reinterpret_cast<T *>(at); }, bytes_};
        ++n_;
        bytes_ += bytes;
    }
public:
    template <typename T> void piece(T **p, size_t bytes) { add(p, pad256(bytes)); }
    template <typename T> void tail(T **p, size_t bytes) { add(p, bytes); }
    int alloc()
    {
        if (n_ > kMax) return g4s::set_error(G4S_ERR_INVALID, "internal: a work block of %d pieces", n_);
        G4S_TRY(buf_.alloc(bytes_));
        for (int i = 0; i < n_; ++i) pc_[i].set(pc_[i].slot, buf_.as<char>() + pc_[i].off);
        return G4S_OK;
    }
    void idle() { buf_.idle = true; }
};

// The device copies of a call with host pointers. The rule it owns: a block may go back to the cache as idle only after the stream that used it has been
// synchronised — otherwise the next caller of big_alloc gets memory with a copy still in flight. finish() is the only place that marks the blocks idle, and
// it synchronises first unless the status says that the device form already has — so behind it the stream is idle whatever the status, and the caller's
// own work blocks (Carver::idle) are too. A frame destroyed without finish() leaves its blocks not idle: they are released behind a device-wide wait.
class Staged {
    static constexpr int kMax = 12;
    BigBuf b_[kMax];
    int n_ = 0, err_ = G4S_OK;
    hipStream_t s_;
    void *block(const void *src, size_t bytes)
    {
        if (err_ != G4S_OK) return nullptr;
        err_ = n_ < kMax ? upload(b_[n_], src, bytes, s_) : g4s::set_error(G4S_ERR_INVALID, "internal: more than %d staged arrays", kMax);
        return err_ == G4S_OK ? b_[n_++].p : nullptr;
    }
public:
    explicit Staged(hipStream_t s) : s_(s) {}
    // the device copy of a host array; NULL for NULL, and after a failure (error())
    template <typename T> const T *in(const T *src, size_t bytes) { return src ? static_cast<const T *>(block(src, bytes)) : nullptr; }
    template <typename T> T *out(size_t bytes) { return static_cast<T *>(block(nullptr, bytes)); }
    int error() const { return err_; }                             // the first failure of in() / out(): nothing was staged behind it
    int to_host(void *dst, const void *src, size_t bytes)          // enqueues only
    {
        if (bytes) G4S_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s_));
        return G4S_OK;
    }
    int wait()
    {
        G4S_HIP_TRY(hipStreamSynchronize(s_));
        return G4S_OK;
    }
    // status: G4S_OK only behind a wait on the stream with nothing enqueued since
    int finish(int status)
    {
        if (status != G4S_OK) (void)hipStreamSynchronize(s_);
        for (int i = 0; i < n_; ++i) b_[i].idle = true;
        return status;
    }
};

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
