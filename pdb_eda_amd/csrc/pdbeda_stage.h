// pdbeda_stage.h -- the host library's staging arithmetic: the carve that lays out an arena, the pinned block's allocator, the host block that
// mirrors a row of a carve, and the copy a setup leaves to its job's first launch.  Pointers and sizes only -- no HIP call, no device: the file
// compiles with the host compiler alone and runs under its sanitizers (tests/stage_harness.cpp); the callers are in pdbeda_hip.hip.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace pdbeda {

// The sizes the host's path choices hang on (tests/test_cloud_host.py, tests/contacts_cases.py and tests/test_gpu_batch_limits.py restate them)
constexpr size_t PINNED_BLOCK_BYTES = (size_t)4 << 20;      // a context's pinned block
constexpr size_t DEV_STAGE_BYTES = (size_t)2 << 20;         // a context's device staging block (d2h_many without copy kernels)
constexpr size_t STAGED_ROW_LIMIT = (size_t)1 << 20;        // the largest row of inputs that is staged in the pinned block whole
constexpr size_t H2D_ROW_SPAN = (size_t)256 << 10;          // h2d_row's default limit on the span it stages

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The rule: an arena's layout and its size come from ONE carve -- a callable that takes a Carver & and names every piece.  arena_carve() (or
// with_scratch() on top of it) runs the carve on a null base for the size and again on the arena's base; never size an arena by hand.
// A piece occupies whole 256-byte units: an EMPTY piece occupies none and has the address of its successor.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(char *b) : base(b) {}
    template <typename T> T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += align_up(n * sizeof(T));
        return p;
    }
    template <typename T> void take(T *&p, size_t n) { p = take<T>(n); }      // (T from the pointer it fills)
};

// The pinned block's ONE allocator: everything staged in it -- inputs the host writes, results kernels write -- is a take, handed out until the
// wait that has seen the stream drain rewinds the block.  A take occupies whole 64-byte lines ((bytes + 63) & ~63: an EMPTY take occupies none and
// shares its address with the next one; a caller whose kernel wants a place of its own for an empty item takes a byte), so the room left is always a
// multiple of 64 and "N bytes fit" is plainly N <= room().
struct PinnedBlock {
    struct Pending { void *dst; size_t off, bytes; };
    char *base = nullptr;
    size_t cap = 0, used = 0;
    std::vector<Pending> pending;      // what the next successful wait copies out of the block, in the order it was registered
    static size_t span(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
    size_t room() const { return cap - used; }      // (0 without a block)
    // The next rewind_delivering() copies `bytes` at `from` (inside a take) to `dst`.
    void deliver(const char *from, void *dst, size_t bytes) { pending.push_back({dst, (size_t)(from - base), bytes}); }
    // nullptr: no block, or no room.  deliver_to: where the take's bytes go (nothing for an empty take).
    char *take(size_t bytes, void *deliver_to = nullptr) {
        if (!base || span(bytes) > room()) return nullptr;
        char *p = base + used;
        if (deliver_to && bytes) deliver(p, deliver_to, bytes);
        used += span(bytes);
        return p;
    }
    // A caller whose launch failed (or that found it cannot use what it took) hands back `first` and every take after it, deliveries included: the
    // block and the pending list are as they were before `first` was taken -- a failed call delivers nothing.
    void untake(const char *first) {
        used = (size_t)(first - base);
        while (!pending.empty() && pending.back().off >= used) pending.pop_back();
    }
    void rewind() { pending.clear(); used = 0; }      // a wait that failed: nothing is delivered, everything is handed out again
    void rewind_delivering() { for (const Pending &p : pending) memcpy(p.dst, base + p.off, p.bytes); rewind(); }      // a wait that saw the stream drain
    // A failed call delivers nothing.  Its takes are NOT handed out again: copies queued by an earlier call may still read them.
    void drop_deliveries() { pending.clear(); }
};

// A host block laid out as a run of consecutive Carver pieces of a device arena: `bytes` from `dev_base` on the device, the same bytes from `stage` on
// the host, every piece at the same offset in both.  twin() is the block's address of a device piece; put() copies into it (nothing: a no-op).
struct StagedRow {
    char *stage = nullptr;
    const char *dev_base = nullptr;
    size_t bytes = 0;
    template <typename T> T *twin(const T *dev) const { return reinterpret_cast<T *>(stage + (reinterpret_cast<const char *>(dev) - dev_base)); }
    void put(const void *dev, const void *src, size_t n) const { if (n) memcpy(twin(static_cast<const char *>(dev)), src, n); }
    // The span in whole 16-byte units (k_job_init copies uint4s).  A row ends on a carve boundary or inside a piece: the round-up stays within that
    // piece's 256-byte padding, on the device and -- a take is whole 64-byte lines -- in the pinned block.
    size_t bytes16() const { return (bytes + 15) & ~(size_t)15; }
};

// A staged row whose copy into device scratch has not been launched yet.  Whoever launches it (or reads the row where it lies) take()s it: it cannot
// be launched twice, or left behind by a path that forgot to clear it.
struct PendingCopy {
    char *src = nullptr, *dst = nullptr;
    size_t bytes = 0;
    PendingCopy take() { const PendingCopy p = *this; *this = PendingCopy(); return p; }
};

}  // namespace pdbeda
