// tests/stage_harness.cpp -- the host library's staging arithmetic (pdb_eda_amd/csrc/pdbeda_stage.h) as a stand-alone program.
//
// Test infrastructure (CPU): tests/test_stage_host.py writes cases into a text file, builds this file with the host compiler under
// AddressSanitizer + UBSan, runs it and compares what it prints with a restatement in Python integers.  Every buffer has exactly the size the
// case names, so a read or write past it is the sanitizer's to report.  One record a line:
//   block CAP                  a PinnedBlock over CAP bytes, byte i of which holds (7 i + 3) mod 256 (CAP 0: no block)   -> state
//   take BYTES DELIVER         take(BYTES, DELIVER ? a destination of BYTES bytes : nullptr)                             -> "take OFF" or "take null", state
//   deliver K OFF BYTES        deliver(take K + OFF, a destination of BYTES bytes, BYTES)                                -> state
//   untake K                   untake(take K)                                                                            -> state
//   rewind_delivering | rewind | drop                                                                                    -> state, "dest I HEX" per destination
//   carve SIZE N...            pieces of N elements of SIZE bytes: a Carver on a null base, then on a buffer of the size that pass found
//                                                                                                                        -> "carve END_NULL END_BASED OFF..."
//   row END SIZE...            pieces of SIZE bytes in a stand-in for device memory, a StagedRow over the first END bytes of them, each piece put() with
//                              bytes (13 i + piece) mod 256          -> "twin STAGE_OFF DEV_OFF" per piece, "row BYTES16 HEX"
//   pending SRC DST BYTES      a PendingCopy of BYTES from offset SRC to offset DST of a buffer, taken twice                -> two "pending" lines
// state: "used U room R pending OFF:BYTES ..." (a destination's number is its place in the pending list's history: destinations are never reused).
#include "pdbeda_stage.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

using namespace pdbeda;

namespace {

long long integer(std::istream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "stage_harness: an integer is missing\n"); exit(2); }
    return v;
}
void print_hex(const char *p, size_t n) {
    if (n == 0) printf("-");
    for (size_t i = 0; i < n; ++i) printf("%02x", (unsigned)(unsigned char)p[i]);
}
struct Elem48 { char b[48]; };

struct BlockCase {
    std::unique_ptr<char[]> mem;
    PinnedBlock blk;
    std::vector<char *> takes;                  // successful takes, in order
    std::vector<std::vector<char>> dests;       // every destination ever registered
    void state() const {
        printf("used %zu room %zu pending", blk.used, blk.room());
        for (const PinnedBlock::Pending &p : blk.pending) printf(" %zu:%zu", p.off, p.bytes);
        printf("\n");
    }
    void print_dests() const {
        for (size_t i = 0; i < dests.size(); ++i) { printf("dest %zu ", i); print_hex(dests[i].data(), dests[i].size()); printf("\n"); }
    }
    char *new_dest(size_t bytes) {
        dests.emplace_back(bytes, (char)0xEE);
        return dests.back().data();      // (the inner vector's storage does not move when the outer one grows)
    }
};

template <typename T>
void carve_pass(Carver &cv, const std::vector<size_t> &counts, std::vector<size_t> *offs) {
    for (size_t n : counts) {
        T *p = cv.take<T>(n);
        if (cv.base) {
            offs->push_back((size_t)(reinterpret_cast<char *>(p) - cv.base));
            if (n) memset(static_cast<void *>(p), 0x5A, n * sizeof(T));      // (every piece is the caller's to write whole)
        }
    }
}
void carve_sized(size_t size, Carver &cv, const std::vector<size_t> &counts, std::vector<size_t> *offs) {
    if (size == 1) carve_pass<uint8_t>(cv, counts, offs);
    else if (size == 4) carve_pass<uint32_t>(cv, counts, offs);
    else if (size == 8) carve_pass<uint64_t>(cv, counts, offs);
    else if (size == 48) carve_pass<Elem48>(cv, counts, offs);
    else { fprintf(stderr, "stage_harness: no element of %zu bytes\n", size); exit(2); }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: stage_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "stage_harness: cannot read %s\n", argv[1]); return 2; }
    std::unique_ptr<BlockCase> bc;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind) || kind[0] == '#') continue;
        if (kind == "block") {
            const size_t cap = (size_t)integer(in);
            bc.reset(new BlockCase());
            if (cap) {
                bc->mem.reset(new char[cap]);
                for (size_t i = 0; i < cap; ++i) bc->mem[i] = (char)((7 * i + 3) & 255);
                bc->blk.base = bc->mem.get();
                bc->blk.cap = cap;
            }
            bc->state();
        } else if (kind == "take") {
            const size_t bytes = (size_t)integer(in);
            const bool deliver = integer(in) != 0;
            char *p = bc->blk.take(bytes, deliver ? bc->new_dest(bytes) : nullptr);
            if (p) { bc->takes.push_back(p); printf("take %zu\n", (size_t)(p - bc->blk.base)); }
            else printf("take null\n");
            bc->state();
        } else if (kind == "deliver") {
            const size_t k = (size_t)integer(in), off = (size_t)integer(in), bytes = (size_t)integer(in);
            bc->blk.deliver(bc->takes.at(k) + off, bc->new_dest(bytes), bytes);
            bc->state();
        } else if (kind == "untake") {
            const size_t k = (size_t)integer(in);
            bc->blk.untake(bc->takes.at(k));
            bc->takes.resize(k);
            bc->state();
        } else if (kind == "rewind_delivering" || kind == "rewind" || kind == "drop") {
            if (kind == "rewind_delivering") bc->blk.rewind_delivering();
            else if (kind == "rewind") bc->blk.rewind();
            else bc->blk.drop_deliveries();
            if (kind != "drop") bc->takes.clear();
            bc->state();
            bc->print_dests();
        } else if (kind == "carve") {
            const size_t size = (size_t)integer(in);
            std::vector<size_t> counts, offs;
            for (long long n; in >> n;) counts.push_back((size_t)n);
            Carver sizing(nullptr);
            carve_sized(size, sizing, counts, &offs);
            // (a base on a 256-byte boundary, as hipMalloc's: what is tested is that every piece keeps it)
            char *mem = sizing.off ? static_cast<char *>(aligned_alloc(256, sizing.off)) : nullptr;
            alignas(256) char dummy = 0;
            Carver cv(mem ? mem : &dummy);      // (nothing to lay out: a base all the same, so that the pieces' addresses are taken)
            carve_sized(size, cv, counts, &offs);
            printf("carve %zu %zu", sizing.off, cv.off);
            for (size_t o : offs) printf(" %zu", o);
            printf("\n");
            free(mem);
        } else if (kind == "row") {
            const size_t end = (size_t)integer(in);
            std::vector<size_t> sizes;
            for (long long n; in >> n;) sizes.push_back((size_t)n);
            Carver sizing(nullptr);
            for (size_t n : sizes) sizing.take<char>(n);
            std::vector<char> dev(sizing.off), stage(end, (char)0xCC);
            Carver cv(dev.data());
            const StagedRow row{stage.data(), dev.data(), end};
            for (size_t k = 0; k < sizes.size(); ++k) {
                const char *piece = cv.take<char>(sizes[k]);
                std::vector<char> src(sizes[k]);
                for (size_t i = 0; i < sizes[k]; ++i) src[i] = (char)((13 * i + k) & 255);
                printf("twin %zu %zu\n", (size_t)(row.twin(piece) - stage.data()), (size_t)(piece - dev.data()));
                row.put(piece, sizes[k] ? src.data() : nullptr, sizes[k]);      // (nothing to put: no source either)
            }
            printf("row %zu ", row.bytes16());
            print_hex(stage.data(), stage.size());
            printf("\n");
        } else if (kind == "pending") {
            const size_t src = (size_t)integer(in), dst = (size_t)integer(in), bytes = (size_t)integer(in);
            std::vector<char> mem(src + dst + bytes + 1);
            PendingCopy pc{mem.data() + src, mem.data() + dst, bytes};
            for (int k = 0; k < 2; ++k) {
                const PendingCopy t = pc.take();
                if (t.src) printf("pending %zu %zu %zu\n", (size_t)(t.src - mem.data()), (size_t)(t.dst - mem.data()), t.bytes);
                else printf("pending null %d %zu\n", t.dst ? 1 : 0, t.bytes);
            }
        } else {
            fprintf(stderr, "stage_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
