"""numpy restatement of the contract of yoho_radius_pairs (include/yoho_trainset.h), used by the CPU and the GPU tests:

    dx = a_i.x - b_j.x (same for y, z), d2 = (dx*dx + dy*dy) + dz*dz, d = sqrt(d2), pair iff d < radius      all in f32

numpy's f32 operators round every step to f32 and never fuse, and np.sqrt of an f32 array is the correctly rounded IEEE square root,
so this IS the contract bit for bit.  Pairs come in np.where's order (ascending i, then ascending j) as (M,2) int64."""
import numpy as np


def radius_pairs_ref(a, b, radius, rows_per_block=256):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
    r = np.float32(radius)
    assert not np.isnan(r), "a NaN radius is refused by the entry"
    out = [np.zeros((0, 2), np.int64)]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i0 in range(0, a.shape[0], rows_per_block):
            blk = a[i0:i0 + rows_per_block]
            dx = blk[:, None, 0] - b[None, :, 0]
            dy = blk[:, None, 1] - b[None, :, 1]
            dz = blk[:, None, 2] - b[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            i, j = np.where(np.sqrt(d2) < r)
            out.append(np.stack([i.astype(np.int64) + i0, j.astype(np.int64)], 1))
    return np.concatenate(out, 0)


def threshold_points(radius, n=64):
    """`n` points on the x axis at distances from the origin that straddle `radius` ulp by ulp: radius - n/2 ulps ... radius + n/2 - 1
    ulps.  Against the single query (0,0,0) the f32 sum d2 is x*x rounded once, so sqrt(d2) is x itself or a neighbour of it - the
    exact-path band of the kernel, on and one ulp beside the threshold."""
    r = np.float32(radius)
    x = np.empty(n, np.float32)
    v = r
    for _ in range(n // 2):
        v = np.nextafter(v, np.float32(0))
    for k in range(n):
        x[k] = v
        v = np.nextafter(v, np.float32(np.inf))
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0] = x
    return pts
