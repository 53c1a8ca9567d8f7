"""csrc/arena.h, the bump allocator every pass cuts its scratch with: a small host program compiled against the header (no HIP include:
plain C++), whose takes are printed and checked here."""
import os
import subprocess

import pytest

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "arena.h"
using yoho::Arena;

struct Big { char b[4096]; };
struct Odd { char b[112]; };

// one take sequence with mixed types, counts and alignments (an empty buffer among them)
static const size_t ALIGN[8] = {256, 256, 64, 16, 256, 8, 256, 4096};
static int lay(Arena& ar, const char* tag, uintptr_t* ptr) {
    int k = 0;
    ptr[k++] = (uintptr_t)ar.take<float>(1000);
    ptr[k++] = (uintptr_t)ar.take<double>(37);
    ptr[k++] = (uintptr_t)ar.take<char>(5, 64);
    ptr[k++] = (uintptr_t)ar.take<unsigned long long>(3, 16);
    ptr[k++] = (uintptr_t)ar.take<int>(0);
    ptr[k++] = (uintptr_t)ar.take<Odd>(3, 8);
    ptr[k++] = (uintptr_t)ar.take<unsigned char>(777);
    ptr[k++] = (uintptr_t)ar.take<Big>(2, 4096);
    std::printf("%s off %zu over %d\n", tag, ar.off, (int)ar.over);
    return k;
}

int main() {
    alignas(4096) static char block[65536];
    uintptr_t pm[8], pb[8];
    Arena measure;
    const int n = lay(measure, "measure", pm);
    for (int k = 0; k < n; ++k) std::printf("measured_ptr %d %llu\n", k, (unsigned long long)pm[k]);
    Arena bound{block, 0, measure.off};
    lay(bound, "bound", pb);
    for (int k = 0; k < n; ++k) std::printf("take %d offset %llu align %zu\n", k, (unsigned long long)(pb[k] - (uintptr_t)block), ALIGN[k]);

    // one byte short: the take that does not fit is the last one
    Arena tight{block, 0, measure.off - 1};
    uintptr_t pt[8];
    lay(tight, "short", pt);
    for (int k = 0; k < n; ++k) std::printf("short_ptr %d %llu\n", k, pt[k] ? (unsigned long long)(pt[k] - (uintptr_t)block) : ~0ull);
    std::printf("short_cap %zu\n", tight.cap);
    void* after = tight.take<char>(1, 1);          // sticky: nothing is handed out behind an overrun
    std::printf("short_after %d over %d\n", after ? 1 : 0, (int)tight.over);

    // count * sizeof(T) beyond size_t, in both modes
    Arena big;
    void* p = big.take<double>(SIZE_MAX / 8 + 1);
    std::printf("overflow_measure ptr %d over %d\n", p ? 1 : 0, (int)big.over);
    Arena bigb{block, 0, sizeof(block)};
    bigb.take<int>(10);
    p = bigb.take<Big>(SIZE_MAX / 4096 + 1);
    std::printf("overflow_bound ptr %d over %d\n", p ? 1 : 0, (int)bigb.over);
    Arena wrap;
    wrap.take<char>(SIZE_MAX - 100, 1);
    p = wrap.take<char>(200, 1);                   // the sum, not the product, overflows
    std::printf("overflow_sum ptr %d over %d\n", p ? 1 : 0, (int)wrap.over);
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    from yoho_amd import build
    d = tmp_path_factory.mktemp("arena")
    src, exe = d / "arena_test.cpp", d / "arena_test"
    src.write_text(PROGRAM)
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", build.CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def rows(lines, tag):
    return [ln[1:] for ln in lines if ln[0] == tag]


def test_header_needs_no_hip_include():
    from yoho_amd import build
    text = open(os.path.join(build.CSRC, "arena.h")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text


def test_measuring_and_bound_runs_take_the_same_offsets(lines):
    (m,), (b,) = rows(lines, "measure"), rows(lines, "bound")
    assert m == b and m[3] == "0" and int(m[1]) > 0              # same end offset, nothing over
    assert all(p[1] == "0" for p in rows(lines, "measured_ptr"))    # a measuring arena hands out null
    takes = rows(lines, "take")
    offs = [int(t[2]) for t in takes]
    assert len(takes) == 8 and offs == sorted(offs) and offs[0] == 0
    # the offsets are what the sizes and alignments say, so a measuring run (which returns no addresses) took them too
    sizes = [4000, 296, 5, 24, 0, 336, 777, 8192]
    off = 0
    for t, size in zip(takes, sizes):
        a = int(t[4])
        off = (off + a - 1) // a * a
        assert int(t[2]) == off
        off += size
    assert off == int(m[1])


def test_every_pointer_honours_its_alignment(lines):
    for t in rows(lines, "take"):
        assert int(t[2]) % int(t[4]) == 0, t


def test_one_byte_short_is_over_and_hands_out_nothing_past_the_block(lines):
    (s,) = rows(lines, "short")
    assert s[3] == "1"
    cap = int(rows(lines, "short_cap")[0][0])
    ptrs = [int(p[1]) for p in rows(lines, "short_ptr")]
    assert ptrs[-1] == 2 ** 64 - 1                                  # the take that did not fit: null
    assert all(p < cap for p in ptrs[:-1])                          # the others: inside the block
    assert rows(lines, "short_after") == [["0", "over", "1"]]


def test_overflowing_sizes_are_over(lines):
    for tag in ("overflow_measure", "overflow_bound", "overflow_sum"):
        assert rows(lines, tag) == [["ptr", "0", "over", "1"]], tag
