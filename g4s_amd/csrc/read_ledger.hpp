// read_ledger.hpp — the bookkeeping behind readback.hpp, in plain C++ (no HIP: tests/cpp/read_ledger_test.cpp runs it on the host under a sanitizer).
// A note says: `bytes` at offset `off` of the staging block belong at `dst` once the copy enqueued on `stream` has landed. Every note has an owner (a
// ReadScope) and a sequence number, rising in the order of the notes. Slots are handed out front to back and never twice while anything is noted: `used`
// returns to 0 exactly when the list is empty. The ledger never touches the block except to copy a landed value out of it; the block is passed in.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
namespace g4s {
class ReadLedger {
public:
    static constexpr size_t kBlockBytes = 4096;
    static constexpr uint64_t kNoMark = ~(uint64_t)0;

    // A slot for `bytes`, noted for `dst`; *seq becomes the note's sequence number. nullptr (and nothing noted) when there is no block or it is full.
    char *reserve(char *block, void *dst, size_t bytes, const void *stream, uintptr_t owner, uint64_t *seq)
    {
        const size_t need = (bytes + 15) & ~(size_t)15;
        if (!block || need > kBlockBytes - used_) return nullptr;
        notes_.push_back(Note{dst, used_, bytes, stream, owner, *seq = ++seq_});
        used_ += need;
        return block + notes_.back().off;
    }
    // Hands out every note of `stream`, whoever owns it — up to sequence number `mark` when one is given; later ones stay noted.
    void deliver(const char *block, const void *stream, uint64_t mark = kNoMark)
    {
        retain([&](const Note &r) {
            if (r.stream != stream || r.seq > mark) return true;
            std::memcpy(r.dst, block + r.off, r.bytes);
            return false;
        });
    }
    void drop(uintptr_t owner) { retain([&](const Note &r) { return r.owner != owner; }); }   // the owner's notes end; nothing is written
    size_t count(uintptr_t owner) const
    {
        size_t n = 0;
        for (const Note &r : notes_) n += r.owner == owner;
        return n;
    }
    size_t pending() const { return notes_.size(); }
    size_t used() const { return used_; }

private:
    struct Note { void *dst; size_t off, bytes; const void *stream; uintptr_t owner; uint64_t seq; };
    template <typename Keep> void retain(Keep keep)
    {
        size_t n = 0;
        for (const Note &r : notes_) if (keep(r)) notes_[n++] = r;
        notes_.resize(n);
        if (!n) used_ = 0;
    }
    std::vector<Note> notes_;
    size_t used_ = 0;
    uint64_t seq_ = 0;
};
} // namespace g4s
