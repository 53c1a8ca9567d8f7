"""yoho_edge_information and the scene pass on the GPU (-m gpu): against the numpy restatement of the contract (tests/multiway_ref.py) -
pair counts exactly, rmse by its bits, the matrix by its values -, row by row against the one-edge call and against
yoho_eval_transforms, over poisoned scratch, its refusals through raw ctypes, and one scene end to end.  Nothing here has a tolerance:
the entry is an exact contract, and the host solve is deterministic given the matrices."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiway_ref as MR  # noqa: E402
from test_gpu_verify import PATTERNS, bits64, cloud_pair, cu, eval_rows  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 513)
GATE = 0.1


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


_RAGGED = {}


def ragged_case(Nt):
    """one target of Nt points and 64 sources whose lengths cycle through LENGTHS, each with its own points (test_gpu_verify.cloud_pair's
    recipe on the shared target: Nt-point unit cube, sources drawn from it with 3 cm of noise); 64 transforms as eval_rows builds them:
    the identity, one 100 m away, one with a NaN entry, one with an infinite entry, twelve generic ones, repeated.  The reference of
    all 64 rows is computed once per Nt and shared; the callers do not modify it."""
    if Nt in _RAGGED:
        return _RAGGED[Nt]
    _, tgt = cloud_pair(1, Nt, 300 + Nt)
    rs = np.random.RandomState(400 + Nt)
    lens = [LENGTHS[k % 8] for k in range(64)]
    srcs = [(tgt[rs.randint(Nt, size=m)] + 0.03 * rs.randn(m, 3)).astype(f32) for m in lens]
    T = eval_rows(Nt)
    # rows 0 .. 3 (identity, far, NaN, inf) sit on the lengths 1, 63, 64, 65; give the four larger lengths their special rows too
    T[4 + 16], T[5 + 16], T[6 + 16], T[7 + 16] = T[0], T[1], T[2], T[3]
    soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    src = np.concatenate(srcs)
    n, r, M = MR.edge_info_ref(src, soff, tgt, T, GATE)
    _RAGGED[Nt] = {"tgt": tgt, "srcs": srcs, "src": src, "soff": soff, "T": T, "npairs": n, "rmse": r, "info": M, "tgt_d": cu(tgt)}
    return _RAGGED[Nt]


def call(c, srcs, tgt_d, T, max_dist=GATE):
    soff = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.int32)
    n, r, M = c.edge_information(cu(np.concatenate(srcs)), soff, tgt_d, cu(T), max_dist)
    K = len(srcs)
    assert n.dtype == torch.int32 and r.dtype == M.dtype == torch.float64 and tuple(n.shape) == tuple(r.shape) == (K,) and tuple(M.shape) == (K, 6, 6)
    return n.cpu().numpy(), r.cpu().numpy(), M.cpu().numpy()


def check(got, case, rows, what):
    n, r, M = got
    assert np.array_equal(n, case["npairs"][rows]), (what, "npairs", n, case["npairs"][rows])
    assert np.array_equal(bits64(r), bits64(case["rmse"][rows])), (what, "rmse bits")
    assert np.array_equal(M, case["info"][rows]), (what, "info", np.nonzero(M != case["info"][rows]))


@pytest.mark.parametrize("Nt", [1, 65, 4097])
def test_ragged_sources_against_the_reference(ctx, Nt):
    """K = 8 (one source of every length), K = 64 (the lengths cycling) and K = 1, on one reference per target size"""
    c = ragged_case(Nt)
    n = c["npairs"]
    # the special rows do what the header says, the generic ones differ
    for k in (1, 2, 3, 21, 22, 23):
        assert n[k] == 0 and c["rmse"][k] == np.inf and not c["info"][k].any(), k
    assert n[0] == 1 and n[20] > 128 and len(set(n[4:16].tolist())) > 1
    check(call(ctx, c["srcs"][:8], c["tgt_d"], c["T"][:8]), c, slice(0, 8), (Nt, 8))
    check(call(ctx, c["srcs"], c["tgt_d"], c["T"]), c, slice(0, 64), (Nt, 64))
    for k in (7, 20, 22):
        check(call(ctx, c["srcs"][k:k + 1], c["tgt_d"], c["T"][k:k + 1]), c, slice(k, k + 1), (Nt, 1, k))


@pytest.mark.parametrize("Nt", [1, 65, 4097])
def test_row_of_a_batch_is_the_call_on_that_source_alone(ctx, Nt):
    """every row of the K = 64 call equals, as bytes, the K = 1 call on its source: a row depends neither on soff[k] nor on its
    neighbours; and npairs and rmse of every row are yoho_eval_transforms' on that source, bit for bit"""
    c = ragged_case(Nt)
    n, r, M = call(ctx, c["srcs"], c["tgt_d"], c["T"])
    for k in range(64):
        n1, r1, M1 = call(ctx, c["srcs"][k:k + 1], c["tgt_d"], c["T"][k:k + 1])
        assert n1.tobytes() == n[k:k + 1].tobytes() and r1.tobytes() == r[k:k + 1].tobytes() and M1.tobytes() == M[k:k + 1].tobytes(), (Nt, k)
        en, er, _ = ctx.eval_transforms(cu(c["srcs"][k]), c["tgt_d"], cu(c["T"][k:k + 1]), GATE)
        assert en.cpu().numpy().tobytes() == n[k:k + 1].tobytes() and er.cpu().numpy().tobytes() == r[k:k + 1].tobytes(), (Nt, k, "eval_transforms")


def test_bits_repeat_over_poisoned_scratch_and_contexts(hip):
    c = ragged_case(4097)
    first = None
    for rep in range(6):
        if rep in (0, 5):
            cx = hip.Context()                                           # the last repeat on a context of its own
        cx.poison_scratch(PATTERNS[rep % 5])
        a = call(cx, c["srcs"], c["tgt_d"], c["T"])
        cx.poison_scratch(PATTERNS[(rep + 1) % 5])
        b = call(cx, c["srcs"][:8], c["tgt_d"], c["T"][:8])
        cx.poison_scratch(PATTERNS[(rep + 2) % 5])
        d = call(cx, c["srcs"][7:8], c["tgt_d"], c["T"][7:8])
        got = [x.tobytes() for x in list(a) + list(b) + list(d)]
        if first is None:
            first = got
            check(a, c, slice(0, 64), "poisoned, K = 64")
        assert got == first, rep


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    s, t = cu(rs.rand(30, 3).astype(f32)), cu(rs.rand(41, 3).astype(f32))
    T = cu(np.tile(np.eye(4)[:3], (8, 1, 1)))
    npr = torch.full((80,), -7, dtype=torch.int32, device="cuda")
    rm = torch.full((80,), -3.0, dtype=torch.float64, device="cuda")
    inf = torch.full((80 * 36,), -3.0, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)           # noqa: E731
    N, f = None, C.c_float
    big = hip.REFINE_MAX_POINTS + 1
    keep = []

    def so(*v):
        a = np.array(v, np.int32)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def ei(ctx_=h, src=p(s), soff=None, K=2, tgt=p(t), Nt=41, T_=p(T), md=f(0.1), n_=p(npr), r_=p(rm), i_=p(inf)):
        return (ctx_, src, so(0, 9, 30) if soff is None else soff, K, tgt, Nt, T_, md, n_, r_, i_, N)

    rows = [
        (ei(ctx_=N), "bad argument"),
        (ei(src=N), "NULL"), (ei(soff=C.c_void_p(None)), "NULL"), (ei(tgt=N), "NULL"), (ei(T_=N), "NULL"), (ei(n_=N), "NULL"), (ei(r_=N), "NULL"), (ei(i_=N), "NULL"),
        (ei(K=0), "K=0"), (ei(K=-1), "K=-1"), (ei(K=65, soff=so(*range(66))), "YOHO_MULTIWAY_MAX_K"),
        (ei(soff=so(1, 9, 30)), "soff[0]=1"),
        (ei(soff=so(0, 9, 9)), "strictly increasing"),                  # an empty source
        (ei(soff=so(0, 0, 30)), "strictly increasing"),
        (ei(soff=so(0, 20, 9)), "strictly increasing"),                 # decreasing
        (ei(soff=so(0, -5, 30)), "strictly increasing"),
        (ei(soff=so(0, big, big + 1)), "YOHO_REFINE_MAX_POINTS"),         # a source above the limit
        (ei(Nt=0), "Nt=0"), (ei(Nt=-2), "Nt=-2"), (ei(Nt=big), "YOHO_REFINE_MAX_POINTS"),
        (ei(md=f(0.0)), "max_dist"), (ei(md=f(-1.0)), "max_dist"), (ei(md=f(np.inf)), "max_dist"), (ei(md=f(np.nan)), "max_dist"),
        (ei(src=off(s, 2)), "4-byte aligned"), (ei(tgt=off(t, 1), Nt=40), "4-byte aligned"), (ei(T_=off(T, 4)), "8-byte aligned"),
        (ei(n_=off(npr, 2)), "4-byte aligned"), (ei(r_=off(rm, 4)), "8-byte aligned"), (ei(i_=off(inf, 4)), "8-byte aligned"),
    ]
    # soff[K] above YOHO_MULTIWAY_MAX_SOURCE_POINTS: 17 sources of 2^22 points
    many = so(*[k * hip.REFINE_MAX_POINTS for k in range(18)])
    rows.append((ei(K=17, soff=many), "YOHO_MULTIWAY_MAX_SOURCE_POINTS"))
    assert hip.MULTIWAY_SYMBOLS == ["yoho_edge_information"]
    for args, text in rows:
        rc = lib.yoho_edge_information(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_edge_information" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((npr == -7).all()) and bool((rm == -3.0).all()) and bool((inf == -3.0).all())
    # the context works as before: rows of 12 bytes that are not 16-byte aligned, outputs written inside their K rows only
    assert lib.yoho_edge_information(*ei(src=off(s, 12), soff=so(0, 9, 29), tgt=off(t, 12), Nt=40, T_=off(T, 96), n_=off(npr, 4), r_=off(rm, 8),
                                         i_=off(inf, 36 * 8), md=f(0.3))) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    rn, rr, rM = MR.edge_info_ref(s.cpu().numpy()[1:], [0, 9, 29], t.cpu().numpy()[1:], np.tile(np.eye(4)[:3], (2, 1, 1)), 0.3)
    assert rn.min() > 0
    assert np.array_equal(npr[1:3].cpu().numpy(), rn) and np.array_equal(bits64(rm[1:3]), bits64(rr))
    assert np.array_equal(inf[36:108].cpu().numpy().reshape(2, 6, 6), rM)
    assert npr[0] == -7 and bool((npr[3:] == -7).all()) and rm[0] == -3.0 and bool((rm[3:] == -3.0).all())
    assert bool((inf[:36] == -3.0).all()) and bool((inf[108:] == -3.0).all())
    # the binding refuses a table that does not cover src before the library sees it
    with pytest.raises(ValueError):
        ctx.edge_information(s, np.array([0, 9, 29], np.int32), t, T[:2], 0.1)


def test_workspace_refusal_is_enomem_and_leaves_the_context_usable(hip, monkeypatch):
    """the grid over 200 000 target points and the slab of 782 blocks ask for more than the 1 MiB this context may hold"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    cx = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    big = cu(np.random.RandomState(0).rand(200000, 3).astype(f32))
    c = ragged_case(65)
    with pytest.raises(hip.YohoError) as e:
        cx.edge_information(big, np.array([0, 100000, 200000], np.int32), big, cu(c["T"][:2]), 0.01)
    assert e.value.code == ENOMEM and "workspace" in str(e.value)
    check(call(cx, c["srcs"][:8], c["tgt_d"], c["T"][:8]), c, slice(0, 8), "after ENOMEM")


# ---- a scene -----------------------------------------------------------------------------------------------------------------------------
def test_scene_end_to_end(ctx):
    """multiway_ref.scene_case: six fragments of 3000 points cut with overlap from one 12 000-point surface, twelve registrations 0.5
    degrees / 1 cm off and one of them (1, 3) replaced by a transform 40 degrees off.  register_scene prunes exactly that pair; its
    matrices are the reference's, hence its poses are, as bytes, those of optimize run on the reference's matrices"""
    from yoho_amd import multiway as MW
    c = MR.scene_case()
    clouds_d = [cu(x) for x in c["clouds"]]
    ed, res = MW.register_scene(ctx, clouds_d, c["pairs"], c["T"], max_dist=c["max_dist"])
    ref = MR.scene_edges_ref(c["clouds"], c["pairs"], c["T"], c["max_dist"])
    assert np.array_equal(ed["npairs"], ref["npairs"]) and ed["rmse"].tobytes() == ref["rmse"].tobytes() and ed["overlap"].tobytes() == ref["overlap"].tobytes()
    assert np.array_equal(ed["info"], ref["info"])
    assert ref["npairs"].min() >= 100 and ref["npairs"][c["bad"]] < ref["npairs"].max() // 4
    want = MW.optimize(6, c["pairs"], c["T"], ref["info"])
    assert res["pruned"].tolist() == [e == c["bad"] for e in range(len(c["pairs"]))] and not res["dropped"].any() and res["reached"].all()
    for k in ("poses", "weights", "rbar"):
        assert res[k].tobytes() == want[k].tobytes(), k
    assert res["history"] == want["history"]
    deg, m = MR.pose_error(res["poses"], c["Xg"])
    print(f"scene: pairs {ed['npairs'].tolist()}, weights {np.round(res['weights'], 3).tolist()}, {deg:.3f} degrees / {m:.4f} m from the ground truth")
    assert deg < 1.0 and m < 0.03                                       # the registrations were 0.5 degrees / 1 cm off each
    # f64 clouds are taken too (converted once), and give the same bytes
    ed2 = MW.scene_edges(ctx, [x.to(torch.float64) for x in clouds_d], c["pairs"], c["T"], c["max_dist"])
    assert ed2["info"].tobytes() == ed["info"].tobytes()
