// readback.hpp — small device→host reads (a count, a total, a flag) through a pinned block of the calling thread (runtime.cpp, read_ledger.hpp).
// hipMemcpyAsync into pageable memory — a stack variable — goes through the runtime's staging buffer and costs 40–100 µs of host time per read on this stack; a
// SpGEMM call makes ten of them (round 5: profiles/r05_small_sizes.txt). A ReadScope enqueues the copy into the pinned block and NOTES where the value belongs;
// a wait hands the noted values out.
//
// The contract. A noted read belongs to the ReadScope that made it, and ends with it. The scope lives in the block that holds the destinations it notes — on
// the stack of the function (or lambda) that notes, or as a member of the object that holds the destination — so that leaving the block by ANY path ends the
// notes: no record outlives its destination. A scope that dies with notes still undelivered (an early return between note and wait) synchronises its stream
// and drops them; it never delivers, destinations declared behind it are gone by then. On the success path its destructor does nothing and makes no HIP call.
// A scope is used and destroyed on the thread that made it: the ledger is thread-local.
//
// reads_sync(s) synchronises s and hands out every note of the calling thread for s, whoever owns it (ReadScope::wait() is the same). That is safe by
// construction — every note in the list has a live owner further up the stack, or in a live object — and it is what lets a callee's wait, or the caller's own
// wait on the stream, settle a read noted elsewhere.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <type_traits>
namespace g4s {
hipError_t reads_sync(hipStream_t s);

class ReadScope {
public:
    explicit ReadScope(hipStream_t s) : s_(s) {}
    ReadScope(const ReadScope &) = delete;
    ReadScope &operator=(const ReadScope &) = delete;
    ~ReadScope();

    // Enqueues the copy of `bytes` from device memory `src` and notes `dst` for it. Without a free slot (block full, no pinned memory) the value is copied
    // straight to dst and the stream synchronised: correct, only slower, and no write to dst is in flight that the ledger does not know of. After a failed
    // enqueue the note stays with the scope, which drops it: return the error.
    hipError_t note(void *dst, const void *src, size_t bytes);
    template <typename T> hipError_t note(T &dst, const void *src)
    {
        static_assert(std::is_trivially_copyable<T>::value && !std::is_pointer<T>::value, "note(dst, src) takes the destination itself — a value or an array of values");
        return note(&dst, src, sizeof(T));
    }
    template <typename T> hipError_t fetch(T &dst, const void *src)   // note + wait: one value, now
    {
        const hipError_t e = note(dst, src);
        return e != hipSuccess ? e : wait();
    }
    hipError_t mark(hipEvent_t ev);      // records ev on the stream, behind every note made by this scope so far
    hipError_t wait() { return reads_sync(s_); }
    hipError_t wait(hipEvent_t ev);      // waits for the marked event only, and hands out what was noted for the stream up to the mark — nothing enqueued behind it

private:
    uintptr_t owner() const { return reinterpret_cast<uintptr_t>(this); }
    hipStream_t s_;
    uint64_t last_ = 0, mark_ = 0;       // sequence numbers (read_ledger.hpp): of this scope's latest note, and of that note when mark() was called
};
} // namespace g4s
