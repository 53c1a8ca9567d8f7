"""The host-side plans that depend on the input size, restated, and the inputs that pin both sides of every threshold (helper of
tests/test_sizes_cpu.py and tests/test_gpu_sizes.py, not a conftest).

  grid_bits, grid_passes     rf_grid_layout / rf_build_grid (yoho_amd/csrc/rfgrid.hip): the table has 2^bits slots, bits the smallest
                             value in [8, 23] with 2^bits >= 2 Nt, and the sort runs ceil(bits / 8) digit passes
  fuse_scan_levels           fu_scan_layout (yoho_amd/csrc/fuse.hip): one level of tile sums per factor of FU_TILE = 2048, two at most

tests/test_sizes_cpu.py holds the constants these rest on against the two sources.  Below them the seeded inputs of the two test
files and their references, each computed once per process and shared: the callers do not modify them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as CR  # noqa: E402
import cluster_ref as CL  # noqa: E402
import fuse_ref as FR  # noqa: E402
import multiway_ref as MR  # noqa: E402
import plane_ref as PR  # noqa: E402
import refine_ref as RR  # noqa: E402
import verify_ref as VR  # noqa: E402

f32, f64 = np.float32, np.float64
GRID_MIN_BITS, GRID_MAX_BITS, GRID_FILL, FU_TILE, FU_MAX_LEVELS = 8, 23, 2, 2048, 2


# ---- the plans ---------------------------------------------------------------------------------------------------------------------------
def grid_bits(Nt):
    bits = GRID_MIN_BITS
    while bits < GRID_MAX_BITS and (1 << bits) < GRID_FILL * Nt:
        bits += 1
    return bits


def grid_passes(Nt):
    return (grid_bits(Nt) + 7) // 8


def fuse_scan_levels(n):
    levels = 0
    while n > FU_TILE and levels < FU_MAX_LEVELS:
        n = (n + FU_TILE - 1) // FU_TILE
        levels += 1
    return levels


# ---- the sizes ---------------------------------------------------------------------------------------------------------------------------
NQ = 4097
NT_GRID = 32769                                                         # the first target size with three digit passes
# (Nt, radius): both sides of the one / two and the two / three pass thresholds and a size with 18 bits, at the radii 0.2 (small sizes) and
# 0.02 (large ones).  In the unit cube a query has a partner with probability 1 - exp(-Nt 4/3 pi r^3) away from the faces: two thirds at
# 32 768 targets, but 95 % at 128 targets under 0.2 and 96 % at 100 003 under 0.02.  WITHIN_WINDOW adds, at those three sizes, the radius
# at which between 10 % and 90 % of the queries have a partner; at the radii above both kinds of query are there, at least 100 of each
WITHIN = ((128, 0.2), (129, 0.2), (32768, 0.02), (32769, 0.02), (100003, 0.02))
WITHIN_WINDOW = ((128, 0.1), (129, 0.1), (32768, 0.02), (32769, 0.02), (100003, 0.0138))
CHAIN_N, CHAIN_EPS, CHAIN_ORDERS = 65537, 0.05, ("shuffled_row0_middle", "descending")
FUSE_S = (4194304, 4194305)                                             # a full 2048-entry top tile at one level; the first two-level size
FUSE_RUNS = ((1.0, 1), (1.0, 2), (0.25, 1))                             # (voxel, min_frags)

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def cube(n, seed):
    return np.random.RandomState(seed).rand(n, 3).astype(f32)


# ---- yoho_nn_within --------------------------------------------------------------------------------------------------------------------
def within_case(Nt):
    """-> (q (4097,3), tgt (Nt,3)) uniform in the unit cube, seed 0"""
    def make():
        rs = np.random.RandomState(0)
        q = rs.rand(NQ, 3).astype(f32)
        return q, rs.rand(Nt, 3).astype(f32)
    return cached(("within", Nt), make)


TIES_RADIUS = 1e-3


def ties_case():
    """32 769 targets and 920 queries under the radius 1e-3, whose cells clamp at |x| ~ 1049:
      targets   300 base points, test_nn_within_ties_gate_non_finite_and_clamp's 200 far points (around x = +-5000, z = 2000 on the f32
                lattice of step 2^-11 there) and 250 near ones (a 1 cm cube), 31 719 of the unit cube, and the 300 base points again
      queries   the first 100 base points (two targets at d2 = 0: the lower index wins), the other 200 far points, the other 250 near
                ones, the first 20 far targets themselves, 350 of the unit cube
    -> dict(q, tgt, far = the rows of the 200 far queries, own = the rows of the 20 targets asked for themselves, own_idx)"""
    def make():
        rs = np.random.RandomState(8)
        base = rs.rand(300, 3).astype(f32)
        far = np.zeros((400, 3), f32)
        far[:, 0] = np.where(np.arange(400) % 2 == 0, 5000.0, -5000.0) + rs.randint(-14, 15, 400) * 2.0 ** -11
        far[:, 1] = rs.randint(-3, 4, 400) * 2.0 ** -11
        far[:, 2] = 2000.0 + rs.randint(-3, 4, 400) * 2.0 ** -11
        near = rs.rand(500, 3).astype(f32) * f32(0.01)
        fill = rs.rand(NT_GRID - 300 - 200 - 250 - 300, 3).astype(f32)
        tgt = np.concatenate([base, far[:200], near[:250], fill, base])
        q = np.concatenate([base[:100], far[200:], near[250:], far[:20], rs.rand(350, 3).astype(f32)])
        assert tgt.shape[0] == NT_GRID
        return {"q": q, "tgt": tgt, "far": np.arange(100, 300), "own": np.arange(550, 570), "own_idx": 300 + np.arange(20)}
    return cached("ties", make)


# ---- the clean scans, the normals, DBSCAN ------------------------------------------------------------------------------------------------
KNN_RADIUS, KNN_K = 0.03, 8


def knn_cloud():
    return cached("knn cloud", lambda: cube(NT_GRID, 2))


def statistical():
    """-> statistical_ref of knn_cloud() at the radius 0.03 with k = 8, min_found 1 and ratio 2"""
    return cached("statistical", lambda: CR.statistical_ref(knn_cloud(), KNN_RADIUS, KNN_K, 1, 2.0))


NORMAL_RADIUS = 0.025


def surface():
    """32 769 points of synth.surface_cloud (four planes and a sphere with 2 mm of noise), f32: about 10 neighbours inside 2.5 cm
    on a plane, fewer at the edges"""
    def make():
        from yoho_amd import synth
        return np.ascontiguousarray(synth.surface_cloud(NT_GRID, seed=5), f32)
    return cached("surface", make)


def surface_normals():
    return cached("surface normals", lambda: PR.normals_ref(surface(), NORMAL_RADIUS))


DBSCAN_EPS, DBSCAN_MIN_PTS = 0.025, 4


def dbscan_cloud():
    return cached("dbscan cloud", lambda: cube(NT_GRID, 1))


def dbscan():
    return cached("dbscan", lambda: CL.dbscan_ref(dbscan_cloud(), DBSCAN_EPS, DBSCAN_MIN_PTS))


def chain(order):
    """the 65 537-point snake in one of snake_orders' row orders -> (pts, ends = the rows of the two chain ends)"""
    def make():
        perm = CL.snake_orders(CHAIN_N)[order]
        return CL.snake(CHAIN_N, CHAIN_EPS)[perm], np.nonzero((perm == 0) | (perm == CHAIN_N - 1))[0]
    return cached(("chain", order), make)


def chain_expected(order):
    """the analytic answer at min_pts = 3: one cluster, every row but the two ends core (two neighbours and itself), no noise"""
    _, ends = chain(order)
    count = np.full((CHAIN_N,), 2, np.int32)
    count[ends] = 1
    sizes = np.zeros((CHAIN_N,), np.int32)
    sizes[0] = CHAIN_N
    return {"labels": np.zeros((CHAIN_N,), np.int32), "count": count, "core": (count == 2).astype(np.uint8), "sizes": sizes,
            "n": np.array([1, CHAIN_N - 2, 0], np.int32)}


# ---- the sums over pairs -----------------------------------------------------------------------------------------------------------------
PAIR_GATE = 0.02
EDGE_LENGTHS = (4097, 63, 1025)


def pair_case():
    """a 32 769-point target in the unit cube, 4097 + 63 + 1025 source points drawn from it with 3 cm of noise (test_gpu_verify's
    cloud_pair) and three transforms up to 2 degrees / 1 cm off the identity; under the gate 0.02 about two thirds of a source have a
    partner -> dict(tgt, srcs, src, soff, T)"""
    def make():
        rs = np.random.RandomState(41)
        tgt = rs.rand(NT_GRID, 3).astype(f32)
        srcs = [(tgt[rs.randint(NT_GRID, size=m)] + 0.03 * rs.randn(m, 3)).astype(f32) for m in EDGE_LENGTHS]
        T = np.stack([RR.perturbed(VR.IDENTITY, rs, 2.0 * rs.rand(), 0.01 * rs.rand()) for _ in EDGE_LENGTHS])
        return {"tgt": tgt, "srcs": srcs, "src": np.concatenate(srcs), "soff": FR.soff_of(srcs), "T": T}
    return cached("pairs", make)


def edge_info():
    c = pair_case()
    return cached("edge info", lambda: MR.edge_info_ref(c["src"], c["soff"], c["tgt"], c["T"], PAIR_GATE))


def eval_two():
    """K = 2: the first source under the first two transforms"""
    c = pair_case()
    return cached("eval", lambda: VR.eval_ref(c["srcs"][0], c["tgt"], c["T"][:2], PAIR_GATE))


ICP_GATE = 0.03


def icp_case():
    """refine_ref.icp_case's recipe on surface(): the target is the cloud, the source every eighth point of it (4097) moved by the
    inverse of a known transform, the start 1 degree / 1 cm off; normals = surface_normals() -> dict(src, tgt, T0, max_dist, normals)"""
    def make():
        rs = np.random.RandomState(2003)
        pc = surface()
        T_gt = np.concatenate([RR.rot_axis_angle(rs.randn(3), 35.0), np.array([[0.3], [-0.2], [0.5]])], axis=1)
        src = (pc[::8].astype(f64) - T_gt[:, 3]) @ T_gt[:, :3]
        return {"src": np.ascontiguousarray(src, f32), "tgt": pc, "T_gt": T_gt, "T0": RR.perturbed(T_gt, rs, 1.0, 0.01), "max_dist": ICP_GATE,
                "normals": surface_normals()["normals"]}
    return cached("icp", make)


def icp_point_step():
    c = icp_case()
    return cached("icp point step", lambda: RR.icp_step(c["src"], c["tgt"], c["T0"], c["max_dist"]))


def icp_plane_step():
    c = icp_case()
    return cached("icp plane step", lambda: PR.plane_step(c["src"], c["tgt"], c["normals"], c["T0"], c["max_dist"]))


# ---- yoho_fuse_clouds --------------------------------------------------------------------------------------------------------------------
def fuse_case(S):
    """S points of a 40 m cube in three fragments cut at S // 3 and 2 S // 3, each under a generic pose -> (src, soff, T (3,3,4))"""
    def make():
        rs = np.random.RandomState(0)
        src = (rs.rand(S, 3) * 40).astype(f32)
        T = np.stack([FR.pose(rs.randn(3), 70.0 * rs.rand(), rs.randn(3)) for _ in range(3)])[:, :3, :]
        return src, np.array([0, S // 3, 2 * S // 3, S], np.int32), np.ascontiguousarray(T)
    return cached(("fuse", S), make)


def fuse_expected(S, voxel, min_frags):
    return cached(("fuse ref", S, voxel, min_frags), lambda: FR.fuse_ref(*fuse_case(S), voxel, 1, min_frags))
