// Host test of g4s::ReadLedger (g4s_amd/csrc/read_ledger.hpp), built with -fsanitize=address,undefined by tests/test_read_ledger_cpu.py.
// A malloc'ed block stands in for the pinned one, small integers for streams and owners; "the copy lands" is a memcpy into the reserved slot.
#include "read_ledger.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using g4s::ReadLedger;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static const void *stream(int i) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(i)); }

struct Fixture {
    char *block = static_cast<char *>(std::malloc(ReadLedger::kBlockBytes));
    ReadLedger l;
    Fixture() { std::memset(block, 0xEE, ReadLedger::kBlockBytes); }
    ~Fixture() { std::free(block); }
    // notes `dst` and lets the "copy" of `value` land in its slot; 0 when no slot was to be had
    uint64_t note(int *dst, int value, int s, uintptr_t owner)
    {
        uint64_t seq = 0;
        char *slot = l.reserve(block, dst, sizeof(int), stream(s), owner, &seq);
        if (!slot) return 0;
        std::memcpy(slot, &value, sizeof(int));
        return seq;
    }
};

// (a) a scope's notes are delivered by a wait on its stream and not by a wait on another stream
static void a_stream_selects()
{
    Fixture f;
    int x = -1, y = -1;
    CHECK(f.note(&x, 11, 1, 100));
    CHECK(f.note(&y, 22, 2, 100));
    f.l.deliver(f.block, stream(3));
    CHECK(x == -1 && y == -1 && f.l.count(100) == 2);
    f.l.deliver(f.block, stream(2));
    CHECK(x == -1 && y == 22 && f.l.count(100) == 1 && f.l.used() != 0);
    f.l.deliver(f.block, stream(1));
    CHECK(x == 11 && y == 22 && f.l.count(100) == 0 && f.l.used() == 0);
}

// (b) an owner dropped with notes pending: a later deliver on that stream writes nothing to the old destinations (freed here: the sanitizer sees a write)
static void b_dropped_owner_writes_nothing()
{
    Fixture f;
    int *heap = static_cast<int *>(std::malloc(3 * sizeof(int)));
    heap[0] = heap[2] = 0x5A5A5A5A;                                // canaries around the destination
    heap[1] = -1;
    int other = -1;
    CHECK(f.note(&heap[1], 33, 1, 100));
    CHECK(f.note(&other, 44, 1, 200));
    f.l.drop(100);
    CHECK(heap[0] == 0x5A5A5A5A && heap[1] == -1 && heap[2] == 0x5A5A5A5A);
    CHECK(f.l.count(100) == 0 && f.l.count(200) == 1 && f.l.used() != 0);
    std::free(heap);
    f.l.deliver(f.block, stream(1));                               // would write into the freed block if the note were still there
    CHECK(other == 44 && f.l.count(100) == 0 && f.l.pending() == 0 && f.l.used() == 0);
    // the same with the dropped owner alone in the list: used is 0 right after the drop
    int *lone = static_cast<int *>(std::malloc(sizeof(int)));
    CHECK(f.note(lone, 55, 1, 300));
    f.l.drop(300);
    CHECK(f.l.count(300) == 0 && f.l.used() == 0);
    std::free(lone);
    f.l.deliver(f.block, stream(1));
}

// (c) A, A, mark, A, then an event deliver: exactly the first two are delivered and the third stays pending
static void c_mark_bounds_the_delivery()
{
    Fixture f;
    int a = -1, b = -1, c = -1;
    CHECK(f.note(&a, 1, 1, 100));
    const uint64_t mark = f.note(&b, 2, 1, 100);
    CHECK(mark != 0);
    const uint64_t later = f.note(&c, 3, 1, 100);
    CHECK(later > mark);
    f.l.deliver(f.block, stream(1), mark);
    CHECK(a == 1 && b == 2 && c == -1 && f.l.count(100) == 1 && f.l.used() != 0);
    f.l.deliver(f.block, stream(1));
    CHECK(c == 3 && f.l.count(100) == 0 && f.l.used() == 0);
    // an owner that has noted nothing before its mark (sequence number 0) is handed nothing
    CHECK(f.note(&a, 4, 1, 100));
    f.l.deliver(f.block, stream(1), 0);
    CHECK(a == 1 && f.l.count(100) == 1);
    f.l.drop(100);
}

// (d) slots are never handed out twice while pending; a full block refuses instead of wrapping; used resets only when the list is empty
static void d_slots_and_the_full_block()
{
    Fixture f;
    CHECK(f.l.reserve(nullptr, nullptr, 4, stream(1), 100, nullptr) == nullptr);   // no block: refused before anything is touched
    static int dst[ReadLedger::kBlockBytes];
    std::vector<std::pair<char *, char *>> slots;                  // [first, last) of every slot handed out
    size_t n = 0;
    for (;; ++n) {                                                 // two owners and two streams interleaved, 4- and 24-byte reads in turn
        uint64_t seq = 0;
        const size_t bytes = n % 2 ? 24 : 4;
        char *slot = f.l.reserve(f.block, &dst[n], bytes, stream(1 + (int)(n % 2)), 100 + n % 2, &seq);
        if (!slot) break;
        CHECK(slot >= f.block && slot + bytes <= f.block + ReadLedger::kBlockBytes);
        CHECK((slot - f.block) % 16 == 0);
        for (const auto &other : slots) CHECK(slot >= other.second || slot + bytes <= other.first);
        slots.emplace_back(slot, slot + bytes);
        CHECK(seq == n + 1);
    }
    CHECK(n == 2 * (ReadLedger::kBlockBytes / (16 + 32)) + 1);     // 85 pairs of 16 + 32 bytes and one more 16
    CHECK(f.l.pending() == n && f.l.used() <= ReadLedger::kBlockBytes);
    uint64_t seq = 0;
    CHECK(f.l.reserve(f.block, &dst[0], 32, stream(1), 100, &seq) == nullptr && f.l.pending() == n);   // still full: no wrap
    f.l.deliver(f.block, stream(1));                               // owner 100's reads: gone, but owner 101's are pending — nothing is reused
    CHECK(f.l.count(100) == 0 && f.l.count(101) == n / 2 && f.l.used() != 0);
    CHECK(f.l.reserve(f.block, &dst[0], 32, stream(1), 100, &seq) == nullptr);
    f.l.drop(101);
    CHECK(f.l.pending() == 0 && f.l.used() == 0);
    char *again = f.l.reserve(f.block, &dst[0], 4, stream(1), 100, &seq);
    CHECK(again == f.block && seq == n + 1);                       // the block starts over; sequence numbers go on rising
    f.l.drop(100);
    CHECK(f.l.reserve(f.block, &dst[0], ReadLedger::kBlockBytes + 1, stream(1), 100, &seq) == nullptr && f.l.used() == 0);   // larger than the block
}

// (e) a nested owner's deliver for the stream also delivers the outer owner's notes
static void e_nested_wait_delivers_the_outer_notes()
{
    Fixture f;
    int outer = -1, inner = -1;
    CHECK(f.note(&outer, 7, 1, 100));
    CHECK(f.note(&inner, 8, 1, 200));
    f.l.deliver(f.block, stream(1));                               // the inner owner's wait
    CHECK(outer == 7 && inner == 8 && f.l.count(100) == 0 && f.l.count(200) == 0 && f.l.used() == 0);
}

int main()
{
    a_stream_selects();
    b_dropped_owner_writes_nothing();
    c_mark_bounds_the_delivery();
    d_slots_and_the_full_block();
    e_nested_wait_delivers_the_outer_notes();
    if (g_failed) { std::fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    std::puts("read_ledger_test: ok");
    return 0;
}
