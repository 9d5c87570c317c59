"""The host library's staging arithmetic (pdb_eda_amd/csrc/pdbeda_stage.h) on a CPU: tests/stage_harness.cpp, built with the host compiler
under AddressSanitizer + UBSan (nothing recovered, nothing preloaded, nothing loaded into Python), against a restatement in Python integers.
Everything is compared with ==.

What the header promises: a take of the pinned block occupies whole 64-byte lines and an empty one none; a take that does not fit changes
nothing; untake(first) puts the block and the pending list back to where they were before `first`; a wait that succeeded delivers every
pending range and rewinds, one that failed only rewinds, a failed call drops its deliveries and keeps its takes.  A carve ends at the same
offset on a null base as on a real one, every non-empty piece on a 256-byte boundary, an empty piece at its successor's address.  A staged
row has every piece at its device offset, put() of nothing touches nothing, and the row's 16-byte round-up stays inside the last piece's
padding.  A pending copy is taken once.  The harness is one process over one file of cases; a sanitizer report ends it with a non-zero
status."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE, PIECE = 64, 256


def span(n):
    return (n + LINE - 1) // LINE * LINE


def hexs(b):
    return bytes(b).hex() if len(b) else "-"


class Cases(object):
    def __init__(self):
        self.lines, self.want, self.where = [], [], []
        self.name = ""

    def emit(self, record, want):
        self.lines.append(record)
        self.want += want
        self.where += [self.name] * len(want)

    # ---- PinnedBlock: the model ----
    def block(self, name, cap):
        self.name = name
        self.cap, self.used, self.pending, self.takes, self.dests = cap, 0, [], [], []      # pending: (dest, off, bytes)
        self.mem = bytes((7 * i + 3) & 255 for i in range(cap))
        self.emit("block %d" % cap, [self.state()])

    def state(self):
        room = self.cap - self.used
        assert room % LINE == 0 and 0 <= self.used <= self.cap, (self.name, self.used)
        return "used %d room %d pending" % (self.used, room) + "".join(" %d:%d" % (off, n) for _, off, n in self.pending)

    def take(self, n, deliver):
        if deliver:
            self.dests.append(bytes([0xEE]) * n)
        if self.cap == 0 or span(n) > self.cap - self.used:
            self.emit("take %d %d" % (n, deliver), ["take null", self.state()])
            return None
        off = self.used
        if deliver and n:
            self.pending.append((len(self.dests) - 1, off, n))
        self.used += span(n)
        self.takes.append(off)
        self.emit("take %d %d" % (n, deliver), ["take %d" % off, self.state()])
        return off

    def deliver(self, k, off, n):
        self.dests.append(bytes([0xEE]) * n)
        self.pending.append((len(self.dests) - 1, self.takes[k] + off, n))
        self.emit("deliver %d %d %d" % (k, off, n), [self.state()])

    def untake(self, k):
        self.used = self.takes[k]
        while self.pending and self.pending[-1][1] >= self.used:
            self.pending.pop()
        del self.takes[k:]
        self.emit("untake %d" % k, [self.state()])

    def end(self, how):
        if how == "rewind_delivering":
            for d, off, n in self.pending:
                self.dests[d] = self.mem[off:off + n]
        self.pending = []
        if how != "drop":
            self.used, self.takes = 0, []
        self.emit(how, [self.state()] + ["dest %d %s" % (i, hexs(d)) for i, d in enumerate(self.dests)])

    # ---- Carver, StagedRow, PendingCopy ----
    def carve(self, size, counts):
        self.name = "carve %d x %s" % (size, counts)
        offs, off = [], 0
        for n in counts:
            offs.append(off)
            off += (n * size + PIECE - 1) // PIECE * PIECE
        for k, n in enumerate(counts):
            assert offs[k] % PIECE == 0
            if n == 0:
                assert offs[k] == (offs[k + 1] if k + 1 < len(counts) else off)      # an empty piece: its successor's address
        self.emit("carve %d %s" % (size, " ".join(map(str, counts))), ["carve %d %d" % (off, off) + "".join(" %d" % o for o in offs)])
        return off

    def row(self, sizes):
        """A row over pieces of `sizes` bytes that ends behind the last piece's bytes, inside its padding."""
        self.name = "row %s" % (sizes,)
        offs, off = [], 0
        for n in sizes:
            offs.append(off)
            off += (n + PIECE - 1) // PIECE * PIECE
        end = offs[-1] + sizes[-1]
        stage = bytearray([0xCC]) * end
        want = []
        for k, n in enumerate(sizes):
            want.append("twin %d %d" % (offs[k], offs[k]))
            stage[offs[k]:offs[k] + n] = bytes((13 * i + k) & 255 for i in range(n))      # the by-hand layout
        bytes16 = (end + 15) // 16 * 16
        assert end <= bytes16 <= off and bytes16 - end < 16      # within the last piece's 256-byte padding
        self.emit("row %d %s" % (end, " ".join(map(str, sizes))), want + ["row %d %s" % (bytes16, hexs(stage))])

    def pending_copy(self, src, dst, n):
        self.name = "pending copy"
        self.emit("pending %d %d %d" % (src, dst, n), ["pending %d %d %d" % (src, dst, n), "pending null 0 0"])


def _build_cases():
    cs = Cases()
    cs.block("spans", 256)
    assert [cs.take(n, 1) for n in (0, 1, 63, 64)] == [0, 0, 64, 128] and cs.used == 192      # spans 0, 64, 64, 64
    assert len(cs.pending) == 3                                                                # the empty take registered no delivery
    before = (cs.used, list(cs.pending))
    assert cs.take(65, 1) is None and (cs.used, cs.pending) == before                          # larger than the room: nothing changes
    cs.end("rewind_delivering")
    assert cs.used == 0 and not cs.pending and cs.dests[0] == b"" and cs.dests[1] == cs.mem[0:1] and cs.dests[3] == cs.mem[128:192]
    assert cs.dests[4] == bytes([0xEE]) * 65                                                   # the take that failed delivers nothing
    cs.block("span of 65", 256)
    assert cs.take(65, 0) == 0 and cs.used == 128
    assert cs.take(128, 1) == 128 and cs.used == 256
    assert cs.take(1, 1) is None and cs.take(0, 1) == 256                                      # full: an empty take still fits
    cs.end("rewind")
    assert cs.dests[0] == bytes([0xEE]) * 128                                                  # a wait that failed delivers nothing
    cs.block("no block", 0)
    for n in (0, 1, 64):
        assert cs.take(n, 1) is None
    cs.end("rewind_delivering")
    cs.block("untake the second of three", 256)
    offs = [cs.take(n, 1) for n in (10, 70, 3)]
    assert offs == [0, 64, 192]
    cs.untake(1)
    assert cs.used == 64 and [p[1:] for p in cs.pending] == [(0, 10)]
    assert cs.take(64, 1) == 64                                                                # handed out again
    cs.end("rewind_delivering")
    assert cs.dests[1] == bytes([0xEE]) * 70 and cs.dests[3] == cs.mem[64:128]
    cs.block("untake the first", 256)
    cs.take(0, 1), cs.take(5, 1), cs.take(64, 0)
    cs.untake(0)
    assert cs.used == 0 and not cs.pending
    cs.end("rewind_delivering")
    cs.block("deliveries inside a take, dropped and kept", 256)
    cs.take(48, 0)
    cs.deliver(0, 0, 16), cs.deliver(0, 32, 16)      # (two ranges of one take, as the map statistics deliver theirs)
    cs.take(8, 1)
    cs.untake(1)                                      # the later take goes, the deliveries inside the earlier one stay
    assert [p[1:] for p in cs.pending] == [(0, 16), (32, 16)]
    cs.end("drop")
    assert cs.used == 64 and not cs.pending           # a failed call: the list is cleared, the takes are kept
    cs.take(8, 1)
    cs.end("rewind_delivering")
    assert cs.dests[0] == bytes([0xEE]) * 16 and cs.dests[3] == cs.mem[64:72]
    for size in (1, 4, 8, 48):
        for counts in ([0], [1], [257], [0, 1, 257], [257, 0, 1], [1, 0, 0, 257, 0]):
            cs.carve(size, counts)
    assert cs.carve(48, [257]) == 12544 and cs.carve(1, [257]) == 512
    cs.row([0, 1, 257, 24])
    cs.row([24])
    cs.row([256, 0, 16])      # (a row that ends ON a 16-byte unit)
    cs.pending_copy(3, 40, 4096)
    return cs


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage")
    exe, case_file = str(d / "stage_harness"), str(d / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"), os.path.join(ROOT, "tests", "stage_harness.cpp"), "-o", exe])
    cs = _build_cases()
    with open(case_file, "w") as f:
        f.write("\n".join(cs.lines) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    return cs, proc


def test_the_harness_ends_clean_under_the_sanitizers(run):
    cs, proc = run
    assert proc.returncode == 0 and proc.stderr == "", proc.stderr[-4000:]


def test_staging_equals_the_restatement(run):
    cs, proc = run
    got = proc.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, cs.want)):
        assert g == w, (cs.where[i], i)
    assert len(got) == len(cs.want)
