// Layout of the backbone's occupancy bitmaps on the host: from a cloud's box of voxels to its descriptor, and the running totals of a
// pass (words, rank entries, scan blocks) that give the next cloud its bases.  One definition for the four levels of a forward pass,
// for the batched voxelisation and for the hash path's first-convolution bitmaps.  No HIP include (plain C++, as arena.h): a host
// program can compile it (tests/test_sparse_cpu.py).
#pragma once

namespace yoho {

// Dense occupancy bitmap of the voxels of one cloud (x fastest, 32 voxels per word)
struct BmDesc {
    long long base;          // first word of this cloud's bitmap
    int x0, y0, z0;          // voxel coordinate of bit 0
    int wx, ny, nz;          // words per x row, rows per z slice, slices
};
// A bitmap with a prefix popcount over 32 (x) x 8 x 8 bricks of words: row(voxel) = rank[word] + popcount(bits below it) (spmaps.hip)
struct RkDesc {
    long long base;          // first word of this cloud's bitmap at this level (row-major: x words fastest, then y, then z)
    int x0, y0, z0;          // voxel coordinate of cell (0,0,0): the same multiples of 16 at every level
    int wx, ny, nz;          // words per x row, rows, slices at this level
    long long rbase;         // first entry of this cloud's rank array at this level
    int nyb, nrank;          // y bricks; rank entries of this cloud = nzb * nyb * wx * 64
    int blk0;                // first 1024-entry scan block of this cloud
};
struct RkRun { long long words = 0, ranks = 0; int blocks = 0; };       // totals of the clouds laid out so far (one per level)

constexpr long long BM_MAX_WORDS = 1ll << 24;        // 64 MiB for one cloud: larger boxes go to the hash tables (and keep word indices in an int)

// a box of dx x dy x dz cells at (x0, y0, z0) behind `words`; false (nothing written) when it is over BM_MAX_WORDS
inline bool bm_layout(BmDesc& d, long long& words, int x0, int y0, int z0, long long dx, long long dy, long long dz) {
    const long long wx = (dx + 31) / 32;
    if (wx * dy * dz > BM_MAX_WORDS) return false;
    d = BmDesc{words, x0, y0, z0, (int)wx, (int)dy, (int)dz};
    words += wx * dy * dz;
    return true;
}
inline bool rk_layout(RkDesc& d, RkRun& run, int x0, int y0, int z0, long long dx, long long dy, long long dz) {
    BmDesc b;
    if (!bm_layout(b, run.words, x0, y0, z0, dx, dy, dz)) return false;
    d.base = b.base; d.x0 = x0; d.y0 = y0; d.z0 = z0; d.wx = b.wx; d.ny = b.ny; d.nz = b.nz;
    d.nyb = (int)((dy + 7) / 8);
    d.nrank = (int)(((dz + 7) / 8) * d.nyb * b.wx * 64);
    d.rbase = run.ranks; d.blk0 = run.blocks;
    run.ranks += d.nrank; run.blocks += (d.nrank + 1023) / 1024;
    return true;
}
inline BmDesc bm_of(const RkDesc& d) { return BmDesc{d.base, d.x0, d.y0, d.z0, d.wx, d.ny, d.nz}; }

// The four levels of one cloud of a forward pass: bb = (min x, y, z, max x, y, z) of its voxels (min > max: empty cloud, one cell at
// 0), margin = reach of the first convolution.  The origin is floored to a multiple of 16, so flooring a coordinate to a coarser
// stride is a shift of its cell index; level l + 1 halves the cells (rounded up).  d[l * stride] is level l's descriptor.
inline bool rk_layout_levels(const int* bb, int margin, RkDesc* d, int stride, RkRun* run) {
    auto floor16 = [](int v) { return v >= 0 ? v / 16 * 16 : -((-v + 15) / 16 * 16); };
    const bool empty = bb[0] > bb[3];
    const int x0 = empty ? 0 : floor16(bb[0] - margin), y0 = empty ? 0 : floor16(bb[1] - margin), z0 = empty ? 0 : floor16(bb[2] - margin);
    long long dx = empty ? 1 : (long long)bb[3] + margin + 1 - x0, dy = empty ? 1 : (long long)bb[4] + margin + 1 - y0,
              dz = empty ? 1 : (long long)bb[5] + margin + 1 - z0;
    for (int l = 0; l < 4; ++l) {
        if (!rk_layout(d[l * stride], run[l], x0, y0, z0, dx, dy, dz)) return false;      // (level 0 decides: the coarser ones are smaller)
        dx = (dx + 1) / 2; dy = (dy + 1) / 2; dz = (dz + 1) / 2;
    }
    return true;
}

}  // namespace yoho
