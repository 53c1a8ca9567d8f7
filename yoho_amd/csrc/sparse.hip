// FCGF backbone: sparse 3-D ResUNet forward pass on a voxelised cloud.  Reference: fcgf_model/resunet.py:10-190
// (ResUNet2 family), residual_block.py:9-52, simple_yoho/fcgf_feat.py:33-49, written against MinkowskiEngine 0.5.x; the sparse-tensor
// semantics implemented here are those listed in oracle/fcgf_oracle.py.  This file holds the weights and the driver; the kernels are in
// spmaps.hip (integer tables) and spconv.hip (convolutions), the shared types in sparse.h.
//
//   FcgfNet, fcgf_load     the weights as fp32 kernels and, by default, fp16x2 planes in MFMA B-fragment order (YOHO_FCGF=f32: fp32 only);
//   fcgf_forward           up to three attempts of one pass (a larger workspace, then the hash tables, when the bitmaps do not fit);
//   one attempt            a FcgfPass walked through its stages: level-0 rows and boxes -> the levels' coordinate maps as rank-ordered
//                          bitmaps (default) or hash tables -> the first convolution's lookup -> kernel maps -> parity orders -> the
//                          network.  The internal row order of a level is free (a row's sum is taken in kernel-offset order whatever
//                          its number); level 0 is handed back in the caller's order through operm.
#include <vector>
#include <algorithm>
#include <cstring>
#include <cmath>

#include "sparse.h"

namespace yoho {

struct BnAff { float* s = nullptr; float* t = nullptr; };
struct ConvW { float* w = nullptr; void* wh = nullptr; float descale = 1.f; };      // fp32 kernel, fp16x2 planes (or null)

struct FcgfNet {
    int C[5] = {0, 32, 64, 128, 256}, T[5] = {0, 64, 64, 64, 128};
    int out_ch = 32, k1 = 7, in_ch = 1, normalize = 1;
    // kernels in spec order
    ConvW conv[4];                                               // conv1..conv4
    BnAff norm[4];
    ConvW bconv[4][2];                                           // block1..4 conv1/conv2
    BnAff bnorm[4][2];
    ConvW conv_tr[3];                                            // conv4_tr, conv3_tr, conv2_tr
    BnAff norm_tr[3];
    ConvW bconv_tr[3][2];                                        // block4_tr, block3_tr, block2_tr
    BnAff bnorm_tr[3][2];
    ConvW conv1_tr;
    ConvW final_k;
    float* final_b = nullptr;
    void* c1planes = nullptr; float c1descale = 1.f;             // first convolution as an MFMA product (conv1_mfma_kernel)
    std::vector<void*> owned;
};

static int up(FcgfNet* n, const float* h, size_t cnt, float** d) {
    HIPCHK(hipMalloc((void**)d, cnt * sizeof(float)));
    n->owned.push_back(*d);
    HIPCHK(hipMemcpy(*d, h, cnt * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

static inline unsigned short f16bits(float x) {
    const _Float16 hh = (_Float16)x;
    unsigned short u;
    std::memcpy(&u, &hh, 2);
    return u;
}

// kernel (K, cin, cout) fp32 -> device copy + (if the shape fits the MFMA path) fp16x2 planes in B-fragment order
static int up_conv(FcgfNet* n, const float* h, int K, int cin, int cout, ConvW* o, bool use16) {
    int rc;
    if ((rc = up(n, h, (size_t)K * cin * cout, &o->w))) return rc;
    if (!use16 || cin % 32 || cout % 32 || K > 27) return 0;
    float wmax = 0.f;
    for (size_t i = 0; i < (size_t)K * cin * cout; ++i) wmax = std::fmax(wmax, std::fabs(h[i]));
    int ex = 0;
    if (wmax > 0.f && std::isfinite(wmax)) (void)std::frexp(wmax, &ex);
    const float wscale = std::ldexp(1.f, 10 - ex);
    o->descale = 1.f / (wscale * 16.f);
    const int nch = cin / 32, ncbt = cout / 32;
    std::vector<unsigned short> pl((size_t)K * cin * cout * 2);
    for (int k = 0; k < K; ++k)
        for (int cc = 0; cc < nch; ++cc)
            for (int st = 0; st < 2; ++st)
                for (int cb = 0; cb < ncbt; ++cb)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const int c = cc * 32 + st * 16 + (lane >> 5) * 8 + e, co = cb * 32 + (lane & 31);
                            const float x = h[((size_t)k * cin + c) * cout + co] * wscale;
                            const _Float16 hi = (_Float16)x;
                            const size_t it = (size_t)k * nch + cc;
                            const size_t base = (((it * 2 + st) * 2) * ncbt) * 512;              // plane 0 of (it, st)
                            pl[base + ((size_t)0 * ncbt + cb) * 512 + lane * 8 + e] = f16bits(x);
                            pl[base + ((size_t)1 * ncbt + cb) * 512 + lane * 8 + e] = f16bits(x - (float)hi);
                        }
    HIPCHK(hipMalloc(&o->wh, pl.size() * 2));
    n->owned.push_back(o->wh);
    HIPCHK(hipMemcpy(o->wh, pl.data(), pl.size() * 2, hipMemcpyHostToDevice));
    return 0;
}

static int up_bn(FcgfNet* n, const float* const* p, int c, BnAff* o) {      // p: weight, bias, running_mean, running_var
    std::vector<float> s(c), t(c);
    for (int i = 0; i < c; ++i) {
        const float sc = p[0][i] / std::sqrt(p[3][i] + 1e-5f);
        s[i] = sc; t[i] = p[1][i] - p[2][i] * sc;
    }
    int rc;
    if ((rc = up(n, s.data(), c, &o->s)) || (rc = up(n, t.data(), c, &o->t))) return rc;
    return 0;
}

void fcgf_free(FcgfNet* n) {
    if (!n) return;
    for (void* p : n->owned) (void)hipFree(p);
    delete n;
}

// tensors: host pointers in the order of yoho_amd.weights.fcgf_spec() with the num_batches_tracked entries left out
int fcgf_load(FcgfNet** out, const yoho_fcgf_config* cfg, const float* const* t, int ntensors, bool f32_kernels) {
    FcgfNet* n = new FcgfNet();
    for (int i = 1; i < 5; ++i) { n->C[i] = cfg->channels[i]; n->T[i] = cfg->tr_channels[i]; }
    n->out_ch = cfg->out_channels; n->k1 = cfg->conv1_kernel_size; n->in_ch = cfg->in_channels; n->normalize = cfg->normalize_feature;
    const int expect = 4 * (1 + 4 + 2 * (1 + 4)) + 3 * (1 + 4 + 2 * (1 + 4)) + 3;
    if (ntensors != expect) { fcgf_free(n); set_error("yoho_load_fcgf: expected %d tensors, got %d", expect, ntensors); return YOHO_EINVAL; }
    if (n->k1 % 2 == 0 || n->out_ch > 64 || n->in_ch > 31) { fcgf_free(n); set_error("yoho_load_fcgf: unsupported configuration"); return YOHO_EINVAL; }
    int ti = 0, rc = 0;
    auto fail = [&](int r) { fcgf_free(n); return r; };
    const bool use16 = !f32_kernels;                              // default: fp16x2 split MFMA; a context created under YOHO_FCGF=f32 keeps the fp32 MFMA kernels
    const int* C = n->C; const int* T = n->T;
    const int cin_enc[4] = {n->in_ch, C[1], C[2], C[3]};
    for (int l = 0; l < 4 && !rc; ++l) {
        const int kv = l == 0 ? n->k1 * n->k1 * n->k1 : 27, co = C[l + 1];
        if ((rc = up_conv(n, t[ti], kv, cin_enc[l], co, &n->conv[l], use16))) break; ti += 1;
        if ((rc = up_bn(n, t + ti, co, &n->norm[l]))) break; ti += 4;
        for (int j = 0; j < 2 && !rc; ++j) {
            if ((rc = up_conv(n, t[ti], 27, co, co, &n->bconv[l][j], use16))) break; ti += 1;
            if ((rc = up_bn(n, t + ti, co, &n->bnorm[l][j]))) break; ti += 4;
        }
    }
    if (rc) return fail(rc);
    const int cin_tr[3] = {C[4], C[3] + T[4], C[2] + T[3]}, cout_tr[3] = {T[4], T[3], T[2]};
    for (int l = 0; l < 3 && !rc; ++l) {
        if ((rc = up_conv(n, t[ti], 27, cin_tr[l], cout_tr[l], &n->conv_tr[l], use16))) break; ti += 1;
        if ((rc = up_bn(n, t + ti, cout_tr[l], &n->norm_tr[l]))) break; ti += 4;
        for (int j = 0; j < 2 && !rc; ++j) {
            if ((rc = up_conv(n, t[ti], 27, cout_tr[l], cout_tr[l], &n->bconv_tr[l][j], use16))) break; ti += 1;
            if ((rc = up_bn(n, t + ti, cout_tr[l], &n->bnorm_tr[l][j]))) break; ti += 4;
        }
    }
    if (rc) return fail(rc);
    if (use16 && n->in_ch == 1 && C[1] == 32 && n->k1 <= 7) {
        // weight planes of the first convolution in the order conv1_mfma_kernel walks: step s, lane half kg -> (y, z) line
        // 2 s + kg, element e -> x offset e (zero for e >= k1 and for the line past the end)
        const float* w = t[0];                                       // (k1^3, 1, 32), kernel index x fastest
        const int k1 = n->k1, kv = k1 * k1 * k1, nsteps = (k1 * k1 + 1) / 2;
        float wmax = 0.f;
        for (int i = 0; i < kv * 32; ++i) wmax = std::fmax(wmax, std::fabs(w[i]));
        int ex = 0;
        if (wmax > 0.f && std::isfinite(wmax)) (void)std::frexp(wmax, &ex);
        const float wscale = std::ldexp(1.f, 10 - ex);
        n->c1descale = 1.f / wscale;
        std::vector<unsigned short> pl((size_t)nsteps * 2 * 64 * 8, 0);
        for (int st = 0; st < nsteps; ++st)
            for (int lane = 0; lane < 64; ++lane) {
                const int line = 2 * st + (lane >> 5), ch = lane & 31;
                if (line >= k1 * k1) continue;
                for (int e = 0; e < k1; ++e) {
                    const float x = w[((size_t)line * k1 + e) * 32 + ch] * wscale;          // line = z * k1 + y
                    const _Float16 hi = (_Float16)x;
                    pl[(((size_t)st * 2 + 0) * 64 + lane) * 8 + e] = f16bits(x);
                    pl[(((size_t)st * 2 + 1) * 64 + lane) * 8 + e] = f16bits(x - (float)hi);
                }
            }
        HIPCHK(hipMalloc(&n->c1planes, pl.size() * 2));
        n->owned.push_back(n->c1planes);
        HIPCHK(hipMemcpy(n->c1planes, pl.data(), pl.size() * 2, hipMemcpyHostToDevice));
    }
    if ((rc = up_conv(n, t[ti], 1, C[1] + T[2], T[1], &n->conv1_tr, use16))) return fail(rc);
    ti += 1;
    if ((rc = up_conv(n, t[ti], 1, T[1], n->out_ch, &n->final_k, use16))) return fail(rc);
    ti += 1;
    if ((rc = up(n, t[ti++], n->out_ch, &n->final_b))) return fail(rc);
    *out = n;
    return 0;
}

constexpr size_t C1BM_BUDGET = (size_t)64 << 20;
size_t fcgf_workspace_bytes(const FcgfNet* net, int n0) {
    // generous bound: every level sized like level 0
    const size_t N = (size_t)n0 + 256;
    const int k1 = net->k1 * net->k1 * net->k1;
    size_t b = 0;
    b += 4 * (N * 4 * 4 + (size_t)table_cap(n0) * 12) + 8192;                 // coords + tables
    b += ((size_t)k1 + 27 * 10) * N * 4;                                      // kernel maps
    b += 3 * (N + 8 * 128 + 256) * 4;                                         // parity-sorted row orders
    b += N * 20 + (size_t)64 * 4096 * 8 + 8192;                               // cell-sorted level-0 rows
    const int* C = net->C; const int* T = net->T;
    size_t feat = 1 + 2 * C[1] + (T[2] + C[1]) + 2 * T[2] + T[1] + net->out_ch;
    feat += 2 * C[2] + (T[3] + C[2]) + 2 * T[3] + 2 * C[3] + (T[4] + C[3]) + 2 * T[4] + 3 * C[4];
    b += feat * N * 4 + 64 * 256;
    b += C1BM_BUDGET;                                                         // occupancy bitmaps of the first convolution (hash-table path)
    return b;
}

// coords0: (n0,3) int32 device, the distinct voxels of nb clouds stored one after the other (host row offsets off[0..nb],
// null = one cloud); out: (n0, out_ch).  The clouds share every launch (cloud index = 4th key component).
// One attempt.  ws_extra: bytes on top of fcgf_workspace_bytes (the rank-ordered bitmaps of a pass whose clouds are sparse in large
// boxes: their size hangs on the bounding boxes, which are only known once the pass has started).  Returns FCGF_RETRY with *rank_need
// set when the bitmaps would eat into the budget of the maps and features behind them - nothing of the pass has been kept then, and
// the caller starts it again on a workspace grown by that much (or on the hash-table path when allow_rank is false).
static constexpr int FCGF_RETRY = 2;
// What the stages of one attempt share: the workspace arena (takes in a fixed order: the scratch tests depend on it), the four levels,
// the coordinate path they live on and its lookups, the kernel maps and row orders, the flags.
struct FcgfPass {
    yoho_ctx* ctx; const FcgfNet* net; hipStream_t s;
    int n0, nb;
    Arena ar; size_t ws_base;
    int gather_ld[4];                                        // widest gathered feature matrix per level (window_ok)
    int* dcount;                                             // 4 device counters: level sizes / the duplicate flag
    Level L[4];
    CloudOff ho; int bb_rpw, bb_nblk; int* dbb; int* dbbpart; int hbb[64 * 6];      // bounding boxes: runs, device partials, host result
    bool boxes_pending;                                      // dbbpart holds the partial boxes of the rows as they are now
    bool conv1_fused;                                        // constant-one input: the first convolution needs no kernel map
    bool rank_mode = false;                                  // the levels are rank-ordered bitmaps (rk), else hash tables (L[].keys)
    bool has_dups = false;                                   // the caller's rows repeat voxels: every row is then mapped by its own probes (full maps)
    RkLevel rk[4];
    BmDesc* ddesc = nullptr; unsigned* dbm = nullptr; long long dbm_words = 0;      // level-0 occupancy bitmaps (rank mode: rk[0]'s)
    int* operm = nullptr;                                    // internal level-0 row -> caller's row (null: same order)
    int* M1 = nullptr; int* Msame[4]; int* Mdown[3]; int* Mup[3];
    int* perm[3]; int nperm[3];                              // parity-sorted row orders of levels 0..2
};

// The gathers address a feature matrix through a 2 GiB buffer window.  Level 0 is checked at the start, the coarser levels as their
// sizes come back (they hold a fraction of the rows, so in practice the level-0 matrices - 96 columns: 5.5 M voxels - limit a pass).
static bool window_ok(const FcgfPass& P, int level, long long rows) {
    if (rows * P.gather_ld[level] * 4 >= (1ll << 31)) {
        set_error("fcgf_forward: %lld voxels at level %d exceed the 2 GiB gather window (%d columns); split the batch", rows, level, P.gather_ld[level]);
        return false;
    }
    return true;
}

// workspace, (n,3) -> (n,4) level-0 rows with the cloud index, and the partial bounding boxes of the clouds on the way
static int level0_rows(FcgfPass& P, const int* coords0, const int* off_host, size_t ws_extra) {
    const FcgfNet* net = P.net;
    const int n0 = P.n0, nb = P.nb;
    const int ld[4] = {std::max(net->T[2] + net->C[1], net->C[1]), std::max(net->T[3] + net->C[2], net->C[2]),
                       std::max(net->T[4] + net->C[3], net->C[3]), net->C[4]};
    std::copy(ld, ld + 4, P.gather_ld);
    if (!window_ok(P, 0, n0)) return YOHO_EINVAL;
    int rc;
    P.ws_base = fcgf_workspace_bytes(net, n0);
    if ((rc = ensure_ws(P.ctx, P.ws_base + ws_extra, P.s))) return rc;
    P.ar = Arena{(char*)P.ctx->ws.p, 0, P.ctx->ws.bytes};
    P.dcount = P.ar.take<int>(4);
    phase_mark(P.ctx, 1, P.s);
    P.L[0].n = n0; P.L[0].ts = 1; P.L[0].coords = P.ar.take<int>((size_t)n0 * 4);
    P.dbb = P.ar.take<int>(64 * 6);
    P.dbbpart = P.ar.take<int>(7 * 1100);               // per-workgroup partial boxes of bbox_kernel (<= 1024 + nb <= 1088 runs)
    if (P.ar.over) return arena_overrun(P.ar, "fcgf_forward: level-0 rows");
    // <= 1024 + nb workgroups, each a run of rows of one cloud
    P.ho.off[0] = 0; P.ho.off[1] = n0;
    if (off_host) for (int b = 0; b <= nb; ++b) P.ho.off[b] = off_host[b];
    P.bb_rpw = std::max(1024, (n0 + 1023) / 1024);
    P.bb_nblk = 0;
    for (int b = 0; b < nb; ++b) P.bb_nblk += (P.ho.off[b + 1] - P.ho.off[b] + P.bb_rpw - 1) / P.bb_rpw;
    P.boxes_pending = true;
    P.conv1_fused = net->in_ch == 1 && net->C[1] == 32 && net->k1 * net->k1 * net->k1 <= C1O_MAXK;
    launch_bbox(coords0, true, P.bb_rpw, P.dbbpart, P.ho, nb, P.L[0].coords, P.bb_nblk, P.s);
    HIPCHK(hipGetLastError());
    return 0;
}

// per-cloud boxes of the voxel indices -> P.hbb (waits for the stream).  The boxes do not depend on the order of the rows: the
// partials taken while the rows were written serve the first call, a second one (the table path behind a bitmap path that handed
// over) reduces the rows again
static int bounding_boxes(FcgfPass& P, const int* c4) {
    if (!P.boxes_pending) launch_bbox(c4, false, P.bb_rpw, P.dbbpart, P.ho, P.nb, nullptr, P.bb_nblk, P.s);
    P.boxes_pending = false;
    launch_bbox_reduce(P.dbbpart, P.bb_nblk, P.nb, P.dbb, P.s);
    HIPCHK(hipMemcpyAsync(P.hbb, P.dbb, sizeof(int) * 6 * P.nb, hipMemcpyDeviceToHost, P.s));
    HIPCHK(hipStreamSynchronize(P.s));
    // the packed 64-bit voxel keys hold 19 bits per axis: indices outside +-(2^18 - 16) (16 = reach of the coarsest kernel
    // offsets) would alias other voxels and give wrong kernel maps without any error - refuse them here
    for (int b = 0; b < P.nb; ++b) {
        const int* bb = P.hbb + 6 * b;
        if (bb[0] > bb[3]) continue;                        // empty cloud
        for (int a = 0; a < 3; ++a)
            if (bb[a] < -VOX_LIM || bb[3 + a] > VOX_LIM) {
                set_error("FCGF backbone: voxel index %d of cloud %d is outside +-%d (cloud extent / voxel size too large, or a non-finite point)",
                          bb[a] < -VOX_LIM ? bb[a] : bb[3 + a], b, VOX_LIM);
                return YOHO_EINVAL;
            }
    }
    return 0;
}

// Rank-ordered bitmaps (spmaps.hip): every level's coordinate map without a hash table, when every cloud fits one.  Leaves
// P.rank_mode set, or unset with nothing taken when the pass belongs on the tables (a cloud too large for a bitmap, duplicate voxels,
// no room); FCGF_RETRY with *rank_need when a larger workspace would do.
static int coords_rank(FcgfPass& P, size_t* rank_need) {
    int rc;
    const int n0 = P.n0, nb = P.nb;
    hipStream_t s = P.s;
    Arena& ar = P.ar;
    if ((rc = bounding_boxes(P, P.L[0].coords))) return rc;
    RkDesc hrk[4][64];
    RkRun run[4];
    bool ok = true;
    for (int b = 0; b < nb && ok; ++b) ok = rk_layout_levels(P.hbb + 6 * b, P.net->k1 / 2, &hrk[0][b], 64, run);      // false: the hash-table path
    const size_t mark = ar.off;
    int* lcoords[4];
    if (ok) {
        // The estimate behind the workspace knows n0 only; the bitmaps and rank arrays follow the VOLUME of the boxes (sparse clouds
        // in large boxes: 15 copies of 5 k voxels over 800 x 800 x 240 cells are 660 MB of ranks).  They must fit ON TOP of that
        // estimate, or the kernel maps and features taken later run out of room: ask for a larger workspace and start again.
        size_t rb = 22 * 256 + 2 * sizeof(RkDesc) * 64 + sizeof(BmDesc) * 64 + (size_t)n0 * 4;
        for (int l = 0; l < 4; ++l)
            rb += ((size_t)run[l].words + 2) * 4 + ((size_t)run[l].ranks + 1) * 4 + ((size_t)run[l].blocks + 2) * 4 + (size_t)n0 * 16 + sizeof(RkDesc) * 64;
        if (P.ws_base + rb > ar.cap) {
            if (rank_need) { *rank_need = rb; return FCGF_RETRY; }
            ok = false;
        }
    }
    if (ok) {
        for (int l = 0; l < 4; ++l) {
            RkLevel& k = P.rk[l];
            k.d = reinterpret_cast<RkDesc*>(ar.take<char>(sizeof(RkDesc) * 64));
            k.bm = ar.take<unsigned>((size_t)run[l].words + 2);        // + spare zero words: conv1_mfma_kernel reads word pairs
            k.rank = ar.take<int>((size_t)run[l].ranks + 1);
            k.btot = ar.take<int>((size_t)run[l].blocks + 2);
            k.blocks = run[l].blocks;
            lcoords[l] = ar.take<int>((size_t)n0 * 4);
            for (int b = 0; b < nb; ++b) {
                k.maxw = std::max(k.maxw, (long long)hrk[l][b].wx * hrk[l][b].ny * hrk[l][b].nz);
                k.maxr = std::max(k.maxr, hrk[l][b].nrank);
            }
        }
        P.ddesc = reinterpret_cast<BmDesc*>(ar.take<char>(sizeof(BmDesc) * 64));
        P.operm = ar.take<int>((size_t)n0);
        if (ar.over) ok = false;
    }
    if (ok) {
        BmDesc hdesc[64];
        for (int b = 0; b < nb; ++b) hdesc[b] = bm_of(hrk[0][b]);
        // (the host arrays live on this frame; the copies complete with the synchronisation behind the level sizes below)
        for (int l = 0; l < 4; ++l) {
            HIPCHK(hipMemcpyAsync(P.rk[l].d, hrk[l], sizeof(RkDesc) * nb, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(P.rk[l].bm, 0, ((size_t)run[l].words + 2) * 4, s));
        }
        HIPCHK(hipMemcpyAsync(P.ddesc, hdesc, sizeof(BmDesc) * nb, hipMemcpyHostToDevice, s));
        launch_rk_fill(P.L[0].coords, n0, P.rk[0], s);
        for (int l = 0; l < 3; ++l) launch_rk_coarsen(P.rk[l], P.rk[l + 1], nb, s);
        for (int l = 0; l < 4; ++l) launch_rk_count(P.rk[l], nb, P.dcount + l, s);
        int hn[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(hn, P.dcount, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        P.has_dups = hn[0] != n0;
        if (!P.has_dups) {                                   // else: duplicate voxels in the input - the hash-table path keeps the first of each
            P.rank_mode = true;
            for (int l = 0; l < 4; ++l) {
                P.L[l].ts = 1 << l; P.L[l].n = hn[l];
                if (!window_ok(P, l, hn[l])) return YOHO_EINVAL;
                launch_rk_rows(P.rk[l], nb, 1 << l, lcoords[l], s);
            }
            launch_rk_operm(P.L[0].coords, n0, P.rk[0], P.operm, s);
            for (int l = 0; l < 4; ++l) P.L[l].coords = lcoords[l];
            P.dbm = P.rk[0].bm; P.dbm_words = run[0].words;
            HIPCHK(hipGetLastError());
        }
    }
    if (!P.rank_mode) { ar.off = mark; ar.over = false; P.operm = nullptr; P.ddesc = nullptr; }      // (nothing was over at `mark`: checked above)
    return 0;
}

// Hash tables: level 0 from the rows (optionally grouped by cell first), each coarser level by inserting the quantised rows of the
// finer one and compacting the first occurrences
static int coords_hash(FcgfPass& P) {
    int rc;
    const int n0 = P.n0;
    hipStream_t s = P.s;
    Arena& ar = P.ar;
    Level* L = P.L;
    if (P.ctx->fcgf_cell_sort > 1 || (P.ctx->fcgf_cell_sort == 1 && n0 >= CELL_SORT_MIN_ROWS)) {
        const int ncell = P.nb * CELL_PER_CLOUD;
        int* cnt = ar.take<int>((size_t)2 * ncell);            // histogram -> in-block prefix | cursors
        int* btot = ar.take<int>(ncell / 1024 + 1);
        int* sorted = ar.take<int>((size_t)n0 * 4);
        P.operm = ar.take<int>((size_t)n0);
        if (ar.over) return arena_overrun(ar, "fcgf_forward: cell sort");
        launch_cell_sort(L[0].coords, n0, P.nb, cnt, btot, P.operm, sorted, s);
        HIPCHK(hipGetLastError());
        L[0].coords = sorted;
    }
    // (the bounding boxes again when the rank path was tried: the rows may have been cell-sorted since - same boxes, one more
    // reduction on the rare path)
    if ((rc = bounding_boxes(P, L[0].coords))) return rc;
    HIPCHK(hipMemsetAsync(P.dcount, 0, sizeof(int) * 4, s));       // [0]: raised when the level-0 insert meets a voxel twice
    for (int l = 0; l < 4; ++l) {
        L[l].ts = 1 << l;
        const int nprev = l == 0 ? n0 : L[l - 1].n;
        L[l].mask = table_cap(nprev) - 1;
        L[l].keys = ar.take<u64>(L[l].mask + 1);
        L[l].vals = ar.take<int>(L[l].mask + 1);
        if (ar.over) return arena_overrun(ar, "fcgf_forward: hash tables");
        if (l == 0) {
            CoordSrc src{L[0].coords, nullptr, 1.0, 1, 0, {0}, nullptr, P.dcount};
            if ((rc = build_table(src, n0, L[0], s))) return rc;
            continue;                                          // value = first row of the voxel (atomicMin); the input voxels are normally distinct
        }
        CoordSrc src{L[l - 1].coords, nullptr, 1.0, L[l].ts, 0, {0}};
        if ((rc = build_table(src, nprev, L[l], s))) return rc;
        L[l].coords = ar.take<int>((size_t)nprev * 4);
        int* bsum = ar.take<int>((size_t)(nprev + 1023) / 1024 + 1);
        if (ar.over) return arena_overrun(ar, "fcgf_forward: coarse rows");
        if ((rc = launch_first_compact(src, nprev, L[l].keys, L[l].vals, L[l].mask, bsum, L[l].coords, 4, nullptr, P.dcount + l, s))) return rc;
        int hd[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(hd, P.dcount + l - 1, sizeof(int) * 2, hipMemcpyDeviceToHost, s));      // l = 1: [duplicate flag, n1]
        HIPCHK(hipStreamSynchronize(s));
        L[l].n = hd[1];
        if (l == 1 && hd[0]) P.has_dups = true;
        if (!window_ok(P, l, L[l].n)) return YOHO_EINVAL;
        launch_hash_set_rows(L[l], s);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static LevelLookup lookup_of(const FcgfPass& P, int l) {
    if (P.rank_mode) return LevelLookup{nullptr, nullptr, 0u, nullptr, P.rk[l].bm, P.rk[l].d, P.rk[l].rank, l};
    const bool filter = P.dbm && l == 0;                       // the occupancy bitmap holds the level-0 voxels
    return LevelLookup{P.L[l].keys, P.L[l].vals, P.L[l].mask, filter ? P.ddesc : nullptr, filter ? P.dbm : nullptr, nullptr, nullptr, 0};
}
// the map of level lo's rows onto level li through ksize^3 offsets of stride ts; null with nothing launched when the arena is over
// (the caller checks it)
static int* make_map(FcgfPass& P, int lo, int li, int ksize, int ts, int sign) {
    int* m = P.ar.take<int>((size_t)ksize * ksize * ksize * P.L[lo].n);
    if (!P.ar.over) launch_build_map(P.L[lo].coords, P.L[lo].n, lookup_of(P, li), ksize, ts, sign, P.L[li].ts, m, P.s);
    return m;
}

// What the first convolution looks its neighbours up in: its kernel map (general input), or the level-0 occupancy bitmaps (constant-
// one input on the hash path; the rank path has them already; skipped if a cloud's bounding box is too large: hash probes then)
static int conv1_lookup(FcgfPass& P, size_t* rank_need) {
    const int n0 = P.n0, nb = P.nb;
    Arena& ar = P.ar;
    phase_mark(P.ctx, 2, P.s);
    if (!P.conv1_fused) P.M1 = make_map(P, 0, 0, P.net->k1, 1, +1);
    if (ar.over) return arena_overrun(ar, "fcgf_forward: first kernel map");
    if (!P.conv1_fused || P.rank_mode) return 0;
    const int hk = P.net->k1 / 2;
    BmDesc hdesc[64];
    long long words = 0;
    bool ok = true;
    for (int b = 0; b < nb && ok; ++b) {
        const int* bb = P.hbb + 6 * b;
        if (bb[0] > bb[3]) { hdesc[b] = BmDesc{words, 0, 0, 0, 1, 1, 1}; continue; }       // empty cloud
        ok = bm_layout(hdesc[b], words, bb[0] - hk, bb[1] - hk, bb[2] - hk, (long long)bb[3] - bb[0] + 1 + 2 * hk, (long long)bb[4] - bb[1] + 1 + 2 * hk,
                       (long long)bb[5] - bb[2] + 1 + 2 * hk);
    }
    // optional, and budgeted: fcgf_workspace_bytes reserves 64 MiB for these bitmaps (C1BM_BUDGET).  Sparse clouds in large boxes
    // need more than that (15 x 5 k voxels over 800 x 800 x 240 cells: 310 MB) - they are taken only if the workspace has that much
    // ON TOP of the estimate, or the maps and features allocated below would run out of room ("workspace estimate too small")
    const size_t bm_bytes = (size_t)words * 4 + 8192 + sizeof(BmDesc) * 64 + 512;
    const bool fits = bm_bytes <= C1BM_BUDGET || P.ws_base + (bm_bytes - C1BM_BUDGET) <= ar.cap;
    if (ok && words > 0 && !fits && rank_need) { *rank_need = bm_bytes - C1BM_BUDGET; return FCGF_RETRY; }      // once more on a workspace with room for them
    if (!(ok && words > 0 && fits)) return 0;
    P.dbm_words = words;
    P.dbm = ar.take<unsigned>((size_t)words + 2);            // + spare words: conv1_mfma_kernel reads word pairs
    P.ddesc = reinterpret_cast<BmDesc*>(ar.take<char>(sizeof(BmDesc) * 64));
    if (ar.over) return arena_overrun(ar, "fcgf_forward: occupancy bitmaps");
    HIPCHK(hipMemsetAsync(P.dbm, 0, ((size_t)words + 2) * 4, P.s));
    HIPCHK(hipMemcpyAsync(P.ddesc, hdesc, sizeof(BmDesc) * nb, hipMemcpyHostToDevice, P.s));
    launch_bitmap_fill(P.L[0].coords, n0, P.ddesc, P.dbm, P.s);
    HIPCHK(hipStreamSynchronize(P.s));                  // hdesc lives on this frame
    return 0;
}

// (the launches of this stage are checked behind the parity orders)
static int kernel_maps(FcgfPass& P) {
    hipStream_t s = P.s;
    Arena& ar = P.ar;
    const Level* L = P.L;
    // every map by its own probes: A/B switch, and whenever the caller's rows repeat voxels - the mirrored entries of the symmetric
    // build and the inverted maps are only ever written for the FIRST row of a voxel
    const bool full_maps = P.ctx->env.fcgf_full_maps || P.has_dups;
    for (int l = 0; l < 4; ++l) {
        // symmetric 3^3 map: offsets 0..12 looked up, 14..26 mirrored, 13 = identity (build_map_sym_kernel)
        P.Msame[l] = full_maps ? make_map(P, l, l, 3, L[l].ts, +1) : ar.take<int>((size_t)27 * L[l].n);
        if (ar.over) return arena_overrun(ar, "fcgf_forward: same-level kernel maps");
        if (full_maps || L[l].n == 0) continue;
        HIPCHK(hipMemsetAsync(P.Msame[l] + (size_t)14 * L[l].n, 0xFF, sizeof(int) * (size_t)13 * L[l].n, s));
        launch_build_map_sym(L[l].coords, L[l].n, lookup_of(P, l), L[l].ts, P.Msame[l], s);
    }
    for (int l = 0; l < 3; ++l) {
        P.Mdown[l] = make_map(P, l + 1, l, 3, L[l].ts, +1);           // strided conv: offsets on the input (finer) stride
        // transposed: coarse row at coord(fine) - offset ... which is the strided map with input and output exchanged
        // (invert_map_kernel): no second probe pass
        P.Mup[l] = full_maps ? make_map(P, l, l + 1, 3, L[l].ts, -1) : ar.take<int>((size_t)27 * L[l].n);
        if (ar.over) return arena_overrun(ar, "fcgf_forward: strided kernel maps");
        if (full_maps || L[l].n == 0) continue;
        HIPCHK(hipMemsetAsync(P.Mup[l], 0xFF, sizeof(int) * (size_t)27 * L[l].n, s));
        if (L[l + 1].n > 0) launch_invert_map(P.Mdown[l], L[l + 1].n, L[l].n, P.Mup[l], s);
    }
    return 0;
}

// parity-sorted row orders of levels 0..2 for the transposed convolutions
static int parity_orders(FcgfPass& P) {
    for (int l = 0; l < 3; ++l) {
        P.nperm[l] = P.L[l].n + 8 * PAR_PAD;
        P.perm[l] = P.ar.take<int>((size_t)P.nperm[l]);
        int* pc = P.ar.take<int>(16);
        if (P.ar.over) return arena_overrun(P.ar, "fcgf_forward: parity orders");
        if (P.L[l].n == 0) continue;
        HIPCHK(hipMemsetAsync(P.perm[l], 0xFF, sizeof(int) * (size_t)P.nperm[l], P.s));
        HIPCHK(hipMemsetAsync(pc, 0, sizeof(int) * 16, P.s));
        launch_parity_order(P.L[l].coords, P.L[l].n, l, pc, P.perm[l], P.s);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the network (resunet.py:142-187) over the levels, maps and orders of the pass
static int run_network(FcgfPass& P, float* out) {
    int rc;
    yoho_ctx* ctx = P.ctx;
    const FcgfNet* net = P.net;
    hipStream_t s = P.s;
    Arena& ar = P.ar;
    const Level* L = P.L;
    const int n0 = P.n0;
    const int* C = net->C; const int* T = net->T;
    float* ones = ar.take<float>((size_t)n0 * net->in_ch);
    if (ar.over) return arena_overrun(ar, "fcgf_forward: input features");
    launch_fill_ones(ones, n0 * net->in_ch, s);
    float* x[4]; float* tmp[4]; float* cat[3]; float* enc3;
    const int catw[3] = {T[2] + C[1], T[3] + C[2], T[4] + C[3]}, catoff[3] = {T[2], T[3], T[4]};
    for (int l = 0; l < 4; ++l) {
        x[l] = ar.take<float>((size_t)L[l].n * C[l + 1]);
        tmp[l] = ar.take<float>((size_t)L[l].n * C[l + 1]);
        if (l < 3) cat[l] = ar.take<float>((size_t)L[l].n * catw[l]);
    }
    enc3 = ar.take<float>((size_t)L[3].n * C[4]);
    if (ar.over) return arena_overrun(ar, "fcgf_forward: encoder features");

    int conv_cat = -1;                          // phase category of the next conv() calls (yoho_phase_read)
    int conv_norm = 0;                          // > 0: the next conv() normalises its output rows in its epilogue (and hands them back in the caller's order)
    auto conv = [&](const float* in, int ldin, int cin, const int* map, int K, int nout, const ConvW& W, int cout, float* o, int ldout,
                    int ocoff, const BnAff* bn, const float* bias, const float* res, int ldres, int rcoff, int relu,
                    const int* rowperm = nullptr, int nslots = 0) -> int {
        phase_mark(ctx, conv_cat, s);
        // fp16 MFMA flops the launch issues: every 32-row tile walks all K offsets x cin x cout, 3 split products (the
        // parity-sorted transposed convolutions skip offsets by data: not counted)
        if (W.wh && !rowperm && cin % 32 == 0 && cout % 32 == 0) phase_work(ctx, conv_cat, 2.0 * 3.0 * (double)((nout + 31) / 32 * 32) * K * cin * cout);
        SpConvArgs a;
        a.rowperm = rowperm; a.nslots = rowperm ? nslots : nout;
        a.in = in; a.ldin = ldin; a.cin = cin; a.map = map; a.K = K; a.nout = nout; a.W = W.w; a.Wh = W.wh; a.descale = W.descale; a.cout = cout;
        a.out = o; a.ldout = ldout; a.ocoff = ocoff; a.aff_s = bn ? bn->s : nullptr; a.aff_t = bn ? bn->t : bias;
        a.res = res; a.ldres = ldres; a.rcoff = rcoff; a.relu = relu;
        a.norm = conv_norm; a.operm = conv_norm ? P.operm : nullptr;
        a.debug = 0;
        return launch_spconv(a, s);
    };
    // BasicBlockBN: out = relu(bn2(conv2(relu(bn1(conv1(x))))) + x), written at column `ocoff` of `o`
    auto block = [&](int l, const float* xin, int c, const ConvW* Wc, const BnAff* bnc, float* scratch, float* o, int ldout, int ocoff) -> int {
        int r;
        if ((r = conv(xin, c, c, P.Msame[l], 27, L[l].n, Wc[0], c, scratch, c, 0, &bnc[0], nullptr, nullptr, 0, 0, 1))) return r;
        return conv(scratch, c, c, P.Msame[l], 27, L[l].n, Wc[1], c, o, ldout, ocoff, &bnc[1], nullptr, xin, c, 0, 1);
    };

    // encoder (resunet.py:142-160).  The block outputs land in the decoder's concatenation buffers (right-hand columns).
    const int k1v = net->k1 * net->k1 * net->k1;
    phase_mark(ctx, 3, s);
    conv_cat = 3;
    if (P.conv1_fused) {
        const Conv1Args c1{L[0].coords, n0, P.ddesc, P.dbm, P.dbm_words, L[0].keys, L[0].mask, net->k1, net->c1planes, net->c1descale, net->conv[0].w,
                           net->norm[0].s, net->norm[0].t, x[0]};
        launch_conv1(c1, ctx->nCU, s);
        HIPCHK(hipGetLastError());
    } else if ((rc = conv(ones, net->in_ch, net->in_ch, P.M1, k1v, n0, net->conv[0], C[1], x[0], C[1], 0, &net->norm[0], nullptr, nullptr, 0, 0, 0)))
        return rc;
    conv_cat = 4;
    if ((rc = block(0, x[0], C[1], net->bconv[0], net->bnorm[0], tmp[0], cat[0], catw[0], catoff[0]))) return rc;
    for (int l = 1; l < 4; ++l) {
        const float* in = cat[l - 1] + catoff[l - 1];
        conv_cat = 7 + l;
        if ((rc = conv(in, catw[l - 1], C[l], P.Mdown[l - 1], 27, L[l].n, net->conv[l], C[l + 1], x[l], C[l + 1], 0, &net->norm[l], nullptr, nullptr,
                       0, 0, 0))) return rc;
        float* o = l < 3 ? cat[l] : enc3;
        conv_cat = 4 + l;
        if ((rc = block(l, x[l], C[l + 1], net->bconv[l], net->bnorm[l], tmp[l], o, l < 3 ? catw[l] : C[4], l < 3 ? catoff[l] : 0))) return rc;
    }
    // decoder (resunet.py:162-181): conv_tr -> norm -> block -> left-hand columns of the concatenation buffer
    const float* din = enc3; int dld = C[4], dcin = C[4];
    for (int j = 0; j < 3; ++j) {
        const int l = 2 - j;                       // output level of conv{4,3,2}_tr
        const int co = j == 0 ? T[4] : (j == 1 ? T[3] : T[2]);
        float* u = ar.take<float>((size_t)L[l].n * co);
        float* sc = ar.take<float>((size_t)L[l].n * co);
        if (ar.over) return arena_overrun(ar, "fcgf_forward: decoder features");
        conv_cat = 11 + l;
        if ((rc = conv(din, dld, dcin, P.Mup[l], 27, L[l].n, net->conv_tr[j], co, u, co, 0, &net->norm_tr[j], nullptr, nullptr, 0, 0, 0,
                       ctx->fcgf_parity_sort ? P.perm[l] : nullptr, P.nperm[l]))) return rc;
        conv_cat = 4 + l;
        if ((rc = block(l, u, co, net->bconv_tr[j], net->bnorm_tr[j], sc, cat[l], catw[l], 0))) return rc;
        din = cat[l]; dld = catw[l]; dcin = catw[l];
    }
    float* f1 = ar.take<float>((size_t)n0 * T[1]);
    float* f2 = ar.take<float>((size_t)n0 * net->out_ch);
    if (ar.over) return arena_overrun(ar, "fcgf_forward: head features");
    conv_cat = 14;
    // both heads in one launch where the fused kernel exists (96 -> 64 -> 32 channels, fp16x2 packs, a pass large enough for the fused
    // normalisation): the 64-channel intermediate never leaves the CU (YOHO_FCGF_HEADS=staged: the two launches below)
    const bool heads_fused = !ctx->env.fcgf_heads_staged && !ctx->env.fcgf_norm_staged && net->out_ch == 32 && T[1] == 64 && catw[0] == 96 &&
                             net->conv1_tr.wh && net->final_k.wh && (n0 + 31) / 32 >= 1024;
    if (heads_fused) {
        phase_mark(ctx, conv_cat, s);
        HeadsArgs ha{cat[0], catw[0], n0, net->conv1_tr.wh, net->conv1_tr.descale, net->final_k.wh, net->final_k.descale, net->final_b, out,
                     net->normalize ? 2 : 1, P.operm};
        launch_heads_fused(ha, ctx->nCU, s);
        HIPCHK(hipGetLastError());
        phase_mark(ctx, -1, s);
        return 0;
    }
    if ((rc = conv(cat[0], catw[0], catw[0], nullptr, 1, n0, net->conv1_tr, T[1], f1, T[1], 0, nullptr, nullptr, nullptr, 0, 0, 1))) return rc;
    // the feature head: 1 x 1 convolution to out_ch, rows /= |row| (once more for fcgf_feat.py:48), the caller's row order.  Fused into
    // the convolution's epilogue where that kernel exists (32 features, fp16x2 fine-level kernel: passes of >= 32768 voxels); the
    // pass over the (n0, 32) matrix was 0.16 ms per 15-copy pass
    const bool fuse_norm = !ctx->env.fcgf_norm_staged && net->out_ch == 32 && net->final_k.wh && T[1] % 32 == 0 && (n0 + 31) / 32 >= 1024;
    conv_norm = fuse_norm ? (net->normalize ? 2 : 1) : 0;
    if ((rc = conv(f1, T[1], T[1], nullptr, 1, n0, net->final_k, net->out_ch, fuse_norm ? out : f2, net->out_ch, 0, nullptr, net->final_b, nullptr, 0, 0, 0))) return rc;
    conv_norm = 0;
    if (!fuse_norm) launch_row_normalize(f2, n0, net->out_ch, out, net->normalize ? 1 : 0, P.operm, s);
    HIPCHK(hipGetLastError());
    phase_mark(ctx, -1, s);
    return 0;
}

static int fcgf_forward_attempt(yoho_ctx* ctx, const FcgfNet* net, const int* coords0, int n0, const int* off_host, int nb, float* out, hipStream_t s,
                                size_t ws_extra, bool allow_rank, size_t* rank_need) {
    FcgfPass P;
    P.ctx = ctx; P.net = net; P.s = s; P.n0 = n0; P.nb = nb;
    int rc;
    if ((rc = level0_rows(P, coords0, off_host, ws_extra))) return rc;
    if (P.conv1_fused && !ctx->fcgf_hash_coords && allow_rank && (rc = coords_rank(P, rank_need))) return rc;
    if (!P.rank_mode && (rc = coords_hash(P))) return rc;
    if ((rc = conv1_lookup(P, rank_need))) return rc;
    if ((rc = kernel_maps(P))) return rc;
    if ((rc = parity_orders(P))) return rc;
    return run_network(P, out);
}

int fcgf_forward(yoho_ctx* ctx, const FcgfNet* net, const int* coords0, int n0, const int* off_host, int nb, float* out, hipStream_t s) {
    if (nb < 1 || nb > 64) { set_error("fcgf_forward: 1..64 clouds per call"); return YOHO_EINVAL; }
    if (n0 == 0) return 0;
    size_t need = 0;
    int rc = fcgf_forward_attempt(ctx, net, coords0, n0, off_host, nb, out, s, 0, true, &need);
    if (rc != FCGF_RETRY) return rc;
    // the bitmaps of this pass do not fit beside the budget of the maps and features: once more on a workspace with room for both (it
    // stays that size, so the next pass of the same shape starts there), and on the hash tables if even that cannot be had
    rc = fcgf_forward_attempt(ctx, net, coords0, n0, off_host, nb, out, s, need, true, nullptr);
    if (rc != YOHO_ENOMEM) return rc;
    rc = fcgf_forward_attempt(ctx, net, coords0, n0, off_host, nb, out, s, 0, false, nullptr);
    if (rc == 0) clear_error();             // recovered: the failed allocation's message must not outlive the pass that succeeded
    return rc;
}

}  // namespace yoho
