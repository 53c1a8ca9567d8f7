"""The FCGF backbone without a GPU: (a) csrc/rklayout.h, the host arithmetic from a cloud's box of voxels to its bitmap descriptors,
through a small host program compiled against the header (no HIP include: plain C++) and checked against a restatement in Python;
(b) the compiler's resource report for the three translation units of the backbone: no kernel spills, and the hot kernels keep the
register counts recorded in profiles/sparse_split.md."""
import os
import re
import subprocess

import pytest

PROGRAM = r"""
#include <cstdio>
#include "rklayout.h"
using namespace yoho;

static void show(const char* tag, const RkDesc& d) {
    std::printf("%s %lld %d %d %d %d %d %d %lld %d %d %d\n", tag, d.base, d.x0, d.y0, d.z0, d.wx, d.ny, d.nz, d.rbase, d.nyb, d.nrank, d.blk0);
}

// commands on stdin:  R = forget the running totals;  L margin bb[6] = the four levels of one cloud of a forward pass;
// K x0 y0 z0 dx dy dz = one rank-ordered box;  M x0 y0 z0 dx dy dz = one plain bitmap
int main() {
    RkRun run[4];
    long long words = 0;
    char c;
    while (std::scanf(" %c", &c) == 1) {
        if (c == 'R') { for (RkRun& r : run) r = RkRun(); words = 0; std::printf("reset\n"); continue; }
        if (c == 'L') {
            int margin, bb[6];
            if (std::scanf("%d %d %d %d %d %d %d", &margin, bb, bb + 1, bb + 2, bb + 3, bb + 4, bb + 5) != 7) return 2;
            RkDesc d[4 * 3];                                   // stride 3: the levels of one cloud are not neighbours in the caller's array
            const bool ok = rk_layout_levels(bb, margin, d, 3, run);
            std::printf("levels %d\n", ok ? 1 : 0);
            if (ok) for (int l = 0; l < 4; ++l) show("level", d[3 * l]);
        } else {
            long long v[6];
            if (std::scanf("%lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5) != 6) return 2;
            if (c == 'K') {
                RkDesc d;
                const bool ok = rk_layout(d, run[0], (int)v[0], (int)v[1], (int)v[2], v[3], v[4], v[5]);
                std::printf("box %d\n", ok ? 1 : 0);
                if (ok) { show("level", d); const BmDesc b = bm_of(d); std::printf("bm %lld %d %d %d %d %d %d\n", b.base, b.x0, b.y0, b.z0, b.wx, b.ny, b.nz); }
            } else {
                BmDesc b;
                const bool ok = bm_layout(b, words, (int)v[0], (int)v[1], (int)v[2], v[3], v[4], v[5]);
                std::printf("plain %d\n", ok ? 1 : 0);
                if (ok) std::printf("bm %lld %d %d %d %d %d %d\n", b.base, b.x0, b.y0, b.z0, b.wx, b.ny, b.nz);
            }
        }
        for (int l = 0; l < 4; ++l) std::printf("run %d %lld %lld %d\n", l, run[l].words, run[l].ranks, run[l].blocks);
        std::printf("words %lld\n", words);
    }
    return 0;
}
"""

MAX_WORDS = 1 << 24


class Run:
    def __init__(self):
        self.words = self.ranks = self.blocks = 0


def rk_layout(run, x0, y0, z0, dx, dy, dz):
    """the descriptor as the kernels read it (spmaps.hip rk_index / rk_lookup): words of 32 x-cells, ranks over 8 x 8 (y, z) bricks of
    words padded to whole bricks, scan blocks of 1024 ranks"""
    wx = -(-dx // 32)
    if wx * dy * dz > MAX_WORDS:
        return None
    nyb, nzb = -(-dy // 8), -(-dz // 8)
    d = [run.words, x0, y0, z0, wx, dy, dz, run.ranks, nyb, nzb * nyb * wx * 64, run.blocks]
    run.words += wx * dy * dz
    run.ranks += d[9]
    run.blocks += -(-d[9] // 1024)
    return d


def rk_layout_levels(runs, bb, margin):
    if bb[0] > bb[3]:
        org, dim = [0, 0, 0], [1, 1, 1]
    else:
        org = [(bb[a] - margin) // 16 * 16 for a in range(3)]                 # floor division: towards minus infinity
        dim = [bb[3 + a] + margin + 1 - org[a] for a in range(3)]
    out = []
    for l in range(4):
        d = rk_layout(runs[l], *org, *dim)
        if d is None:
            return None
        out.append(d)
        dim = [-(-v // 2) for v in dim]
    return out


def drive(exe, commands):
    r = subprocess.run([str(exe)], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from yoho_amd import build
    d = tmp_path_factory.mktemp("rklayout")
    src, out = d / "rklayout_test.cpp", d / "rklayout_test"
    src.write_text(PROGRAM)
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", build.CSRC, str(src), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_header_needs_no_hip_include():
    from yoho_amd import build
    text = open(os.path.join(build.CSRC, "rklayout.h")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text and "#include" not in text


# (margin, box): an empty cloud, a one-voxel box, a negative origin that is no multiple of 16, x extents of 31, 32 and 33 voxels
# (margin 0 and an origin on a multiple of 16, so that the extent is the number of cells), a box with odd sizes on every level
SINGLE = [(3, (5, 5, 5, 4, 4, 4)), (3, (7, -9, 40, 7, -9, 40)), (3, (-37, -100, -1, 60, 11, 300)), (0, (16, 0, -16, 46, 9, -3)),
          (0, (16, 0, -16, 47, 9, -3)), (0, (16, 0, -16, 48, 9, -3)), (2, (-250, -131, 3, 211, 77, 160))]


def test_levels_of_one_cloud(exe):
    cmds = []
    for margin, bb in SINGLE:
        cmds += ["R", "L %d %s" % (margin, " ".join(map(str, bb)))]
    out = drive(exe, cmds)
    blocks = [i for i, ln in enumerate(out) if ln[0] == "levels"]
    assert len(blocks) == len(SINGLE)
    for (margin, bb), i in zip(SINGLE, blocks):
        runs = [Run() for _ in range(4)]
        want = rk_layout_levels(runs, bb, margin)
        assert out[i] == ["levels", "1"]
        got = [[int(v) for v in ln[1:]] for ln in out[i + 1:i + 5]]
        assert got == want, (bb, got, want)
        assert [[int(v) for v in ln[2:]] for ln in out[i + 5:i + 9]] == [[r.words, r.ranks, r.blocks] for r in runs]
        # what the kernels rely on, stated without the restatement: one origin for all levels, a multiple of 16 at or below the box
        # minus the margin; the cells of level l hold the box plus the margin; a level halves the cells of the one before (rounded up)
        for l, d in enumerate(got):
            assert d[1:4] == got[0][1:4] and all(v % 16 == 0 for v in d[1:4])
            if l:
                assert d[5] == (got[l - 1][5] + 1) // 2 and d[6] == (got[l - 1][6] + 1) // 2
        if bb[0] <= bb[3]:
            d = got[0]
            assert all(d[1 + a] <= bb[a] - margin and bb[a] - margin - d[1 + a] < 16 for a in range(3))
            assert d[4] * 32 > bb[3] + margin - d[1] and d[5] == bb[4] + margin - d[2] + 1 and d[6] == bb[5] + margin - d[3] + 1
        else:
            assert got[0][1:7] == [0, 0, 0, 1, 1, 1]
    # the x extents: 31 and 32 cells are one word per row, 33 are two
    assert [out[i + 1][5] for i in blocks[3:6]] == ["1", "1", "2"]


def test_fifteen_clouds_accumulate_their_bases(exe):
    boxes = [(-40 - 3 * b, -17 + b, 5 * b, 70 + 11 * b, 90 - 2 * b, 5 * b + 33 + b) for b in range(15)]
    boxes[6] = (1, 1, 1, 0, 0, 0)                                             # an empty cloud in the middle takes its one cell
    out = drive(exe, ["R"] + ["L 3 " + " ".join(map(str, bb)) for bb in boxes])
    runs = [Run() for _ in range(4)]
    blocks = [i for i, ln in enumerate(out) if ln[0] == "levels"]
    assert len(blocks) == 15
    last = None
    for bb, i in zip(boxes, blocks):
        want = rk_layout_levels(runs, bb, 3)
        got = [[int(v) for v in ln[1:]] for ln in out[i + 1:i + 5]]
        assert got == want, bb
        if last is not None:                                                  # a cloud starts where the one before it ends, on every level
            for l in range(4):
                p = last[l]
                assert got[l][0] == p[0] + p[4] * p[5] * p[6] and got[l][7] == p[7] + p[9] and got[l][10] == p[10] + (p[9] + 1023) // 1024
        last = got
    assert [[int(v) for v in ln[2:]] for ln in out[-5:-1]] == [[r.words, r.ranks, r.blocks] for r in runs]


def test_single_boxes_plain_bitmaps_and_the_word_limit(exe):
    # 2^24 words exactly is taken, one row more is refused and leaves the totals alone; the voxelisation's boxes (any origin)
    full = (0, 0, 0, 32 * 256, 256, 256)
    over = (0, 0, 0, 32 * 256, 256, 257)
    out = drive(exe, ["R", "K -5 7 -1000 33 9 17", "K 3 3 3 1 1 1", "K %d %d %d %d %d %d" % full, "K %d %d %d %d %d %d" % over,
                      "M -5 7 -1000 33 9 17", "M %d %d %d %d %d %d" % over, "M 1 2 3 64 2 2",
                      "R", "L 3 0 0 0 %d 300 300" % (32 * 256)])
    run = Run()
    want = [rk_layout(run, -5, 7, -1000, 33, 9, 17), rk_layout(run, 3, 3, 3, 1, 1, 1), rk_layout(run, *full)]
    assert rk_layout(Run(), *over) is None
    k = [i for i, ln in enumerate(out) if ln[0] == "box"]
    assert [out[i][1] for i in k] == ["1", "1", "1", "0"]
    for i, w in zip(k[:3], want):
        assert [int(v) for v in out[i + 1][1:]] == w
        assert [int(v) for v in out[i + 2][1:]] == w[:7]                      # bm_of: the plain bitmap of a rank-ordered one
    assert [int(v) for v in out[k[3] + 1][2:]] == [run.words, run.ranks, run.blocks]      # refused: the totals are those of the third box
    m = [i for i, ln in enumerate(out) if ln[0] == "plain"]
    assert [out[i][1] for i in m] == ["1", "0", "1"]
    assert [int(v) for v in out[m[0] + 1][1:]] == [0, -5, 7, -1000, 2, 9, 17]
    assert [int(v) for v in out[m[2] + 1][1:]] == [2 * 9 * 17, 1, 2, 3, 2, 2, 2]          # the refused one in between added nothing
    lv = [i for i, ln in enumerate(out) if ln[0] == "levels"]
    assert out[lv[0]] == ["levels", "0"]                                      # a forward-pass cloud over the limit: the hash-table path
    assert [ln[2:] for ln in out[lv[0] + 1:lv[0] + 5]] == [["0", "0", "0"]] * 4


# next_free_vgpr of the hot kernels (profiles/sparse_split.md: the parent's assembly); by mangled-name fragment
HOT = {"spconv16w_kernelILi1EEE": 112, "spconv16w_kernelILi2EEE": 102, "spconv16w_kernelILi4EEE": 156,
       "spconv16s_kernelILi2ELi2EEE": 176, "spconv16s_kernelILi1ELi3EEE": 144,
       "13spconv_kernelILi1ELb0EEE": 112, "13spconv_kernelILi1ELb1EEE": 120, "13spconv_kernelILi2ELb0EEE": 176, "13spconv_kernelILi2ELb1EEE": 184,
       "heads_fused_kernelILi3EEE": 169, "conv1_mfma_kernel": 152}
UNITS = ("sparse.hip", "spmaps.hip", "spconv.hip")


def test_backbone_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
    """the three units compiled for gfx950 with the flags of the build (none of them has an EXTRA entry: default FP contraction)"""
    from yoho_amd import build
    assert all(u in build.SOURCES and u not in build.EXTRA for u in UNITS)
    procs = [(u, subprocess.Popen(build.asm_command(u, str(tmp_path / (u + ".s"))) + ["-Rpass-analysis=kernel-resource-usage"],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for u in UNITS]
    scratch, vgpr = {}, {}
    for u, p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
        names = re.findall(r"Function Name: (\S+)", err)
        sizes = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
        assert len(names) == len(sizes), u
        scratch.update(zip(names, sizes))
        asm = open(tmp_path / (u + ".s")).read()
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S):
            vgpr[name] = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    assert len(scratch) == 49 and set(scratch) == set(vgpr), len(scratch)
    assert not [n for n, s in scratch.items() if s], {n: s for n, s in scratch.items() if s}
    for frag, want in HOT.items():
        hits = [n for n in vgpr if frag in n]
        assert len(hits) == 1, (frag, hits)
        print(hits[0], vgpr[hits[0]])
        assert vgpr[hits[0]] == want, (hits[0], vgpr[hits[0]], want)
