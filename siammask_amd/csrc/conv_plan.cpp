// conv_plan.cpp -- the kernel / workgroup-shape choice for one convolution, the marks on a sequence list (conv_plan.h).  Host
// code, no HIP runtime call.
#include "conv_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace smk;

// code: bits 0-3 tile (0 auto, 1 128x128, 2 128x64, 3 64x128, 4 64x64), bits 4-5 K tile
// (0 auto, 1 128 B, 2 256 B), bits 6-7 ring depth (0 auto, 1..3 -> 2..4 stages)
TileChoice tile_from_code(int code, const ConvParams &p, int dtype) {
    TileChoice t = choose_tile(p, dtype);
    static const int tb[6][2] = {{0, 0}, {128, 128}, {128, 64}, {64, 128}, {64, 64}, {256, 128}};
    const int tile = code & 15, kt = (code >> 4) & 3, st = (code >> 6) & 3;
    if (tile >= 1 && tile <= 5) {
        t.bm = tb[tile][0]; t.bn = tb[tile][1];
        t.kt = (t.bm == 64 && t.bn == 64) ? 256 : 128;
        t.stages = (t.bm == 128 && t.bn == 128) ? 2 : 3;
    }
    if (kt) t.kt = kt == 2 ? 256 : 128;
    if (t.bm == 64 && t.bn == 64) t.kt = 256;
    if (t.bm == 256) t.kt = 128;
    if (st) t.stages = st + 1;
    return t;
}

// conv3x3_halo_kernel or the generic kernel?  Returns the halo workgroup height (128 / 64) or 0.
// Measured on MI355X (profiles/r01_v6_halo_ab.txt): the halo kernel wins on every 3x3 stride-1 layer of the
// path except the long-K wide-N projection (l3.0.downsample, K=4608 N=1024), where the 256x128 generic tile
// amortises the weight stream better; BM=128 once the launch has >= 300 such tiles, else BM=64.
int halo_choice(const PackedConv &pc, const ConvParams &p, const ConvOpt &o, int dtype) {
    const int mode = o.halo ? o.halo : g_tune.halo;
    if (!mode || !pc.w_halo || p.out_mode != OUT_NHWC || p.kh != 3 || p.kw != 3 || p.stride != 1 || p.ups) return 0;
    if (mode != 1) return mode;
    if (dtype != DT_F16) return 0;            // fp32 (32-channel chunks, 32x32x2 MFMA): measured slower, 1.33 vs 1.09 ms at B=1
    if (p.Ci * 9 > 2304 && p.Nst >= 512) return 0;
    const long tiles128 = (long)p.B * ((p.Ho * p.Wo + 127) / 128) * ((p.Nst + 127) / 128);
    return tiles128 >= 300 ? 128 : 64;
}

// the patch-sharing tile of the sequences (wreg_halo_tile.inc): can this 3x3 convolution run on whole-row tiles of bm pixels?
bool seq_halo_ok(const ConvParams &p, int bm) {
    if (!p.wgt_frag_halo || p.kh != 3 || p.kw != 3 || p.stride != 1 || p.stride_x != 1 || p.pad != p.dil || p.dil < 1 || p.dil > 4) return false;
    if (p.Hl != p.Hs || p.Wl != p.Ws || p.org_y || p.org_x || p.Ho != p.Hl || p.Wo != p.Wl) return false;
    if (p.Ci % 128 || p.Kpad != 9 * p.Ci || p.Wo > bm) return false;       // an even number of 64-channel chunks
    const int rpt = bm / p.Wo;
    return (rpt + 2 * p.dil) * (p.Wl + 2 * p.dil) * 9 <= 10 * 256;         // patch pieces (HALO_NRMAX rounds of 256; 144-byte rows)
}
// force_halo: 0 = the rule below, 128 / 64 = that tile or fail, -1 = never (per-op tests that force another tile)
bool seq_layer_from(const ConvParams &p, int dtype, SeqLayer &L, int force_halo) {
    if (!conv_wreg_eligible(p, dtype) || p.groups > 1 || p.pos || p.ups || p.Kpad % 128) return false;
    if (p.ci_shift < 0 || p.Ci < 64) return false;       // (wreg_tile compiles the general tap arithmetic out of the sequence's routines)
    if (p.kh > 15 || p.kw > 15 || p.stride > 15 || p.pad > 15 || p.dil > 15) return false;
    // the packed record keeps the geometry in 16-bit fields
    const int u16[] = {p.Hs, p.Ws, p.Cs, p.cin_off, p.Ci, p.Hl, p.Wl, p.Ho, p.Wo, p.Kpad, p.Nst, p.Cos, p.cout_off, p.res_Cs, p.res_coff};
    for (int v : u16)
        if (v < 0 || v > 65535) return false;
    if (p.org_y < -32768 || p.org_y > 32767 || p.org_x < -32768 || p.org_x > 32767) return false;
    memset(&L, 0, sizeof(L));
    L.in = p.in; L.wgt_frag = p.wgt_frag; L.bias = p.bias; L.res = p.res; L.out = p.out;
    L.in_bytes = p.in_bytes; L.w_bytes = p.w_bytes;
    L.Hs = (unsigned short)p.Hs; L.Ws = (unsigned short)p.Ws; L.Cs = (unsigned short)p.Cs; L.cin_off = (unsigned short)p.cin_off;
    L.Ci = (unsigned short)p.Ci; L.Hl = (unsigned short)p.Hl; L.Wl = (unsigned short)p.Wl;
    L.org_y = (short)p.org_y; L.org_x = (short)p.org_x; L.Ho = (unsigned short)p.Ho; L.Wo = (unsigned short)p.Wo;
    L.Kpad = (unsigned short)p.Kpad; L.Nst = (unsigned short)p.Nst; L.Cos = (unsigned short)p.Cos;
    L.cout_off = (unsigned short)p.cout_off; L.res_Cs = (unsigned short)p.res_Cs; L.res_coff = (unsigned short)p.res_coff;
    L.kw_magic = p.kw_magic;
    L.kh = (signed char)p.kh; L.kw = (signed char)p.kw; L.stride = (signed char)p.stride; L.stride_x = (signed char)p.stride_x;
    L.pad = (signed char)p.pad; L.dil = (signed char)p.dil; L.relu = (signed char)p.relu; L.res_mode = (signed char)p.res_mode;
    L.ci_shift = (signed char)p.ci_shift;
    L.a_stage = (signed char)p.a_stage;
    L.res_nt = (signed char)p.res_nt;
    // workgroup tile: the widest that still gives the 32 workgroups of an XCD a tile each per image
    L.cfg = p.Nst >= 512 ? 0 : (p.Nst >= 192 ? 1 : 2);
    // Short-K layers are dominated by the fixed cost of a tile (operand first touch, residual fetch, accumulator hand-over:
    // ~5 us against ~0.45 us per K tile, SMK_SEQ_CLK), so when the 64-row tiling needs more than one round of the team's
    // 32 workgroups per image, ONE 128-row tile per workgroup beats two 64-row tiles in sequence
    // (bottleneck conv3: 2 x 64x256 -> 1 x 128x256; layer2.0 conv1 on the 63x63 input: 4 rounds of 64x64 -> 1 of 128x128)
    // (seq_tall = 2, A/B knob: also for long-K layers -- l3.0.downsample, 64 tiles of 64x256 = two rounds -- now that four
    //  producer waves feed a 128-row tile)
    if (g_tune.seq_tall && ((long)p.kh * p.kw * p.Ci <= 512 || g_tune.seq_tall == 2)) {
        const int hw = p.Ho * p.Wo;
        const int bn64 = L.cfg == 0 ? 256 : (L.cfg == 1 ? 128 : 64);
        const int tiles64 = ((hw + 63) / 64) * ((p.Nst + bn64 - 1) / bn64);
        if (tiles64 > 32) {
            if (p.Nst >= 512) L.cfg = 3;
            else if (p.Nst >= 96) L.cfg = 4;
            else L.cfg = 9;                              // 128x64 (layer1's 64-channel convolutions on 63x63 images)
        }
        if (tiles64 > 64 && p.Nst >= 192 && p.Nst < 512) L.cfg = 3;      // N = 256 on 63x63 images: 128x256, one round (layer1 conv3)
    }
    // N = 512 with 16 row tiles (layer2.0's 3x3 stride-2 shortcut on a 31x31 output): 32 tiles either as 64x256 or as 128x128 --
    // the square tile stages 32 KB per K tile instead of 40 KB for the same flops, and these loops run at the CU's 64 B/clk
    // (smk_tune "seq_ds128", A/B knob)
    if (g_tune.seq_ds128 && L.cfg == 0 && p.Nst == 512 && (long)p.kh * p.kw * p.Ci >= 1024) {
        const int hw = p.Ho * p.Wo;
        if (((hw + 127) / 128) * 4 <= 32) L.cfg = 4;
    }
    // 3x3 stride-1 layers with N <= 256 (every Bottleneck's conv2): whole-row tiles x 64 channels with the activation patch shared
    // by the nine taps -- half the bytes per flop of the 64 x 128 / 64 x 64 im2col tiles (smk_tune "seq_halo").  128 pixels where that
    // gives the team (nearly) a tile per workgroup (256 channels on 31 x 31: 8 x 4), else 64 (128 channels: 16 x 2).  The long-K
    // wide-N shortcut of layer3.0 stays on 128 x 256 tiles (same bytes per flop, four times fewer tiles).
    if (force_halo > 0 || (force_halo == 0 && g_tune.seq_halo && p.Nst <= 256)) {
        const int tn = (p.Nst + 63) / 64;
        int bm = force_halo > 0 ? force_halo : 0;
        if (!bm) {
            const bool ok128 = seq_halo_ok(p, 128), ok64 = seq_halo_ok(p, 64);
            const int t128 = ok128 ? ((p.Ho + 128 / p.Wo - 1) / (128 / p.Wo)) * tn : 0;
            bm = (ok128 && (t128 >= 28 || !ok64)) ? 128 : (ok64 ? 64 : 0);
        } else if (!seq_halo_ok(p, bm)) return false;
        if (bm) {
            L.cfg = (signed char)(bm == 128 ? SEQ_CFG_HALO128 : SEQ_CFG_HALO64);
            L.wgt_frag = p.wgt_frag_halo;
        }
    }
    L.sync = 1;
    // K-loop stagger (smk_tune "seq_kstag": 0 off, 1 = layers whose weights fit the XCD's L2 beside the activations, 2 = all)
    L.kstag = (signed char)((g_tune.seq_kstag == 2 || (g_tune.seq_kstag == 1 && (size_t)p.Nst * p.Kpad * 2 <= (3u << 19))) ? 1 : 0);
    if (g_tune.seq_deep && L.cfg == 1) L.cfg = 5;         // measurement variant (smk_tune "seq_deep")
    {   // (smk_tune "seq_kstag_mask": which tile routines stagger -- 1 fused pairs, 2 patch-sharing tiles, 4 the im2col tiles)
        const bool is_halo = L.cfg == SEQ_CFG_HALO128 || L.cfg == SEQ_CFG_HALO64;
        if (is_halo && !(g_tune.seq_kstag_mask & 2)) L.kstag = 0;
        if (!is_halo && !(g_tune.seq_kstag_mask & 4)) L.kstag = 0;
    }
    return true;
}

// Pairs (conv3 of a Bottleneck, the 1x1 convolution that reads its output) -> one fused tile routine (c3c1_tile.inc): the 1x1
// needs every channel of a pixel and no neighbour, so the workgroup that owns 32 whole rows of conv3's output runs it from LDS.
// Marks the two records of every pair the routine has a shape for; the list itself (tensors, order, barriers behind the pair)
// stays as recorded.  smk_tune "seq_fuse" 0 leaves the list alone.
static bool seq_pair_fusable_why(const SeqLayer *L, int i, int *code, int *why);
bool seq_pair_fusable(const SeqLayer *L, int i, int *code) {
    int why = 0;
    const bool ok = seq_pair_fusable_why(L, i, code, &why);
    // SMK_SEQ_DEBUG=1: why is a (1x1 + residual + ReLU, 1x1) pair of records NOT fused?  (stderr, once per list walk)
    if (!ok && why > 1 && getenv("SMK_SEQ_DEBUG"))
        fprintf(stderr, "[seq fuse] records %d, %d: not fusable, reason %d (Kpad %d Nst %d -> Nst %d, res %p relu %d, b.relu %d b.Ho %d Hs %d)\n", i, i + 1, why,
                (int)L[i].Kpad, (int)L[i].Nst, (int)L[i + 1].Nst, L[i].res, (int)L[i].relu, (int)L[i + 1].relu, (int)L[i + 1].Ho, (int)L[i + 1].Hs);
    return ok;
}
static bool seq_pair_fusable_why(const SeqLayer *L, int i, int *code, int *why) {
    const SeqLayer &a = L[i], &b = L[i + 1];
    auto plain1x1 = [](const SeqLayer &l) {
        return l.kh == 1 && l.kw == 1 && l.stride == 1 && l.stride_x == 1 && l.pad == 0 && l.org_y == 0 && l.org_x == 0 &&
               l.Hl == l.Hs && l.Wl == l.Ws && l.Ho == l.Hs && l.Wo == l.Ws && l.Ci == l.Kpad;
    };
    if (!plain1x1(a) || !a.sync) { *why = 1; return false; }
    if (!plain1x1(b)) { *why = 2; return false; }
    if (!a.res || a.res_mode != RES_PRE_RELU || !a.relu) { *why = 1; return false; }
    if (b.res || b.res_mode != RES_NONE) { *why = 3; return false; }
    if (b.in != a.out) { *why = 1; return false; }
    if (b.cin_off != a.cout_off || b.Cs != a.Cos || b.Ci != a.Nst || b.Hs != a.Ho || b.Ws != a.Wo) { *why = 4; return false; }
    if (b.out == a.out || b.out == a.res || b.out == a.in) { *why = 5; return false; }
    // The routine fetches the residual BEFORE it waits at its hoist point.  The barrier still pending there is the one behind
    // the LAST layer before i that carries one (`pend`; layer i - 1 when it has sync = 1, an earlier one when smk_op_conv_seq's
    // caller chained independent members with sync = 0).  Whoever wrote the residual inside this list must be separated from
    // layer i by a barrier the workgroup has already PASSED, i.e. one behind a layer j' with writer <= j' < pend.
    // (The first record of an already marked pair carries no barrier of its own.)
    auto has_bar = [&](int k) { return L[k].sync && L[k].cfg != SEQ_CFG_C3C1_L3 && L[k].cfg != SEQ_CFG_C3C1_L2 && L[k].cfg != SEQ_CFG_C3C1P_L3 && L[k].cfg != SEQ_CFG_C3C1P_L2; };
    int pend = -1;
    for (int k = i - 1; k >= 0; --k)
        if (has_bar(k)) { pend = k; break; }
    for (int j = i - 1; j >= 0; --j)
        if (L[j].out == a.res) {
            bool passed = false;
            for (int k = j; k < pend; ++k) passed = passed || has_bar(k);
            if (!passed) { *why = 6; return false; }
            break;
        }
    // conv3's own input must be behind the pending barrier too (the hoist point is the only wait in front of its loads)
    for (int j = i - 1; j >= 0; --j)
        if (L[j].out == a.in) {
            if (j > pend) { *why = 7; return false; }
            break;
        }
    if (a.Kpad == 256 && a.Nst == 1024 && b.Nst == 256) *code = SEQ_CFG_C3C1_L3;
    else if (a.Kpad == 128 && a.Nst == 512 && b.Nst == 128) *code = SEQ_CFG_C3C1_L2;
    else { *why = 8; return false; }
    return true;
}

bool seq_pair_fits(const SeqLayer *L, int i, int B, int *code) {
    if (!seq_pair_fusable(L, i, code)) return false;
    // the routine switches rows beyond the image off with a buffer offset of 0x7ffff000: every tensor must end below it
    const size_t px = (size_t)B * L[i].Ho * L[i].Wo;
    const size_t widest = std::max(std::max((size_t)L[i].Cs, (size_t)L[i].Cos), std::max((size_t)L[i].res_Cs, (size_t)L[i + 1].Cos));
    return px * widest * 2 < 0x7fff0000u && L[i].in_bytes < 0x7fff0000u;
}

// ---- plan_seq: the marks on a recorded list -------------------------------------------------------------------------
// The passes mark the records of one launch [i0, i1) of the list L[0, n).

// Pairs (seq_pair_fusable).  L: the launch's first record.
static int seq_fuse_pairs(SeqLayer *L, int n, int B, const char *locked, bool have_xch) {
    if (!g_tune.seq_fuse) return 0;
    int fused = 0;
    for (int i = 0; i + 1 < n; ++i) {
        int code = 0;
        if (locked && (locked[i] || locked[i + 1])) continue;        // (per-op tests: the caller forced a tile)
        if (L[i].cfg >= SEQ_CFG_C3C1_L3 || L[i + 1].cfg >= SEQ_CFG_C3C1_L3 || !seq_pair_fits(L, i, B, &code)) continue;
        if (g_tune.seq_fuse == 2 && code != SEQ_CFG_C3C1_L3) continue;      // (2: layer3's pairs only, A/B knob)
        // Measured (profiles/r03h_*): -4.3 .. -5.5 % on the B = 8 step, -2.0 % at B = 16, -2.7 % at B = 24.  (What looked like a race of
        // this routine at B = 12 was a buffer shared by two layouts inside the launch, see build_arena; profiles/r03h_b12_race.txt.)
        // smk_tune "seq_pair2d": the pair split over two CUs (needs the exchange scratch: f16 contexts / smk_op_conv_seq have it)
        if (have_xch && g_tune.seq_pair2d && (g_tune.seq_pair2d == 1 || code == SEQ_CFG_C3C1_L3))
            code = code == SEQ_CFG_C3C1_L3 ? SEQ_CFG_C3C1P_L3 : SEQ_CFG_C3C1P_L2;
        L[i].cfg = (signed char)code;
        L[i + 1].cfg = (signed char)SEQ_CFG_C3C1_2ND;
        if (!(g_tune.seq_kstag_mask & 1)) L[i].kstag = 0;
        ++fused;
        ++i;
    }
    return fused;
}

static bool read_after_list(const std::vector<const void *> &read_after, const void *y) {
    return std::find(read_after.begin(), read_after.end(), y) != read_after.end();
}

// Triples (round 4): [conv2 (3x3, stride 1, pad = dilation), conv3, the next 1x1] of a Bottleneck as ONE tile routine on image-row
// tiles (c3c1_tile.inc, FRONT = 1).  Runs behind seq_fuse_pairs: a marked pair (i + 1, i + 2) whose first record reads what record i --
// the block's 3x3 convolution -- writes, and nobody else reads it.  The barrier between conv2 and the pair disappears with the
// tensor.  wstd[i] = the (kh, kw, cin)-ordered fragment pack of record i (the record itself carries the chunk-major pack of the
// patch-sharing tile).  smk_tune "seq_fuse3": 0 off, 1 on, 2 layer3's blocks only.
static int seq_fuse_triples(SeqLayer *L, int i0, int i1, int n, const void *const *wstd, const char *locked,
                            const std::vector<const void *> &read_after) {
    if (!g_tune.seq_fuse3) return 0;
    auto group_has_bar = [&](int k) {            // a barrier stands behind record k (pairs / triples: behind their LAST record only)
        const int cf = L[k].cfg;
        if (cf == SEQ_CFG_C3C1_L3 || cf == SEQ_CFG_C3C1_L2 || cf == SEQ_CFG_C3C1P_L3 || cf == SEQ_CFG_C3C1P_L2 || cf == SEQ_CFG_C2C3C1_L3 ||
            cf == SEQ_CFG_C2C3C1_L2 || cf == SEQ_CFG_C2C3C1_MID)
            return false;
        return L[k].sync != 0;
    };
    int fused = 0;
    for (int i = i0; i + 2 < i1; ++i) {
        SeqLayer &c2 = L[i], &c3 = L[i + 1], &c1 = L[i + 2];
        if (locked && (locked[i] || locked[i + 1] || locked[i + 2])) continue;
        if ((c3.cfg != SEQ_CFG_C3C1_L3 && c3.cfg != SEQ_CFG_C3C1_L2) || c1.cfg != SEQ_CFG_C3C1_2ND) continue;
        if (c2.cfg != SEQ_CFG_HALO128 && c2.cfg != SEQ_CFG_HALO64 && c2.cfg > 9) continue;     // (a plain tile or the patch-sharing one)
        const int code = c3.cfg == SEQ_CFG_C3C1_L3 ? SEQ_CFG_C2C3C1_L3 : SEQ_CFG_C2C3C1_L2;
        if (g_tune.seq_fuse3 == 2 && code != SEQ_CFG_C2C3C1_L3) continue;
        const int kc = c3.Kpad;                  // 256 / 128: conv2 is kc -> kc
        if (c2.kh != 3 || c2.kw != 3 || c2.stride != 1 || c2.stride_x != 1 || c2.pad != c2.dil || c2.dil < 1 || c2.dil > 2) continue;
        if (c2.Ci != kc || c2.Nst != kc || c2.Kpad != 9 * kc || !c2.relu || c2.res || c2.res_mode != RES_NONE || !c2.sync) continue;
        if (c2.org_y || c2.org_x || c2.Hl != c2.Hs || c2.Wl != c2.Ws || c2.Ho != c2.Hs || c2.Wo != c2.Ws) continue;
        if (c2.Wo > 32 || c2.Wo < 24 || c2.Wo + 2 * c2.dil > 35) continue;      // one image row per 32-row tile; short rows (the template's 15 x 15) stay pairs
        if (c3.in != c2.out || c3.cin_off != c2.cout_off || c3.Cs != c2.Cos || c3.Hs != c2.Ho || c3.Ws != c2.Wo) continue;
        if (!wstd[i]) continue;
        // conv2's output never reaches memory: nobody else may read it, in this launch, a later one or behind the list, until a
        // later record writes that buffer again (the blocks of a layer share their intermediates)
        bool other_reader = read_after_list(read_after, c2.out);
        for (int j = i + 2; j < n; ++j) {
            if (L[j].in == c2.out || L[j].res == c2.out) { other_reader = true; break; }
            if (L[j].out == c2.out) { other_reader = false; break; }
        }
        if (other_reader || c2.out == c3.res || c2.out == c1.out || c2.out == c3.out) continue;
        // conv2's input must have been written in front of the barrier this routine waits for (the last one before record i)
        int pend = -1;
        for (int k = i - 1; k >= i0; --k)
            if (group_has_bar(k)) { pend = k; break; }
        bool in_ok = true;
        for (int j = i - 1; j >= i0; --j)
            if (L[j].out == c2.in) { in_ok = j <= pend; break; }
        if (!in_ok) continue;
        // the residual rows: in front of the wait when their writer is separated from record i by a barrier ALREADY passed, or when it
        // is the previous triple's conv3 on the same row tiles (then this very workgroup wrote them); behind the wait otherwise
        int res_late = 0;
        for (int j = i - 1; j >= i0; --j)
            if (L[j].out == c3.res) {
                bool passed = false;
                for (int k = j; k < pend; ++k) passed = passed || group_has_bar(k);
                const bool own_rows = L[j].cfg == SEQ_CFG_C2C3C1_MID && L[j].Ho == c3.Ho && L[j].Wo == c3.Wo;
                if (!passed && !own_rows) res_late = 1;
                break;
            }
        c2.cfg = (signed char)code;
        c2.wgt_frag = wstd[i];
        c2.sync = 0;
        c3.cfg = (signed char)SEQ_CFG_C2C3C1_MID;
        c3.a_stage = (signed char)res_late;
        ++fused;
        i += 2;
    }
    return fused;
}

// Resident trunk (round 6; smk_kernels.h SEQ_YRES_*): consecutive fused pairs of one ResNet layer -- [conv3 k + conv1 k+1], conv2 k+1 on a
// patch-sharing tile, [conv3 k+1 + conv1 k+2] -- run on the same 32-row tiles; with ONE image per team and a tile per workgroup the
// same workgroup owns the same rows in both, and the second pair's residual is the Y image the first one left in its LDS
// (experiments/siammask_sharp/resnet.py:80-103: `out += residual`, residual = the previous block's output).  Marks: the second
// pair does not fetch its residual rows (64 KB per CU "usually from beyond the L2", profiles/r05_seq_phase_clocks.txt: 3.0-3.5 of a
// layer3 pair's 17-18 us), the first one does not store Y when nobody else reads the tensor, the 3x3 convolution between them works
// in the LDS behind the image.  Values and summation orders are unchanged: bit-identical (tests/test_gpu_seq.py).
static int seq_mark_resident(SeqLayer *L, int i0, int i1, int n, const SeqPlanEnv &env, const std::vector<const void *> &read_after) {
    if (!g_tune.seq_yres || env.B > 8) return 0;         // (image b runs on team b % 8: from nine images on a workgroup owns two tiles per pair)
    int prev = -1, marked = 0;
    for (int i = i0; i + 1 < i1; ++i) {
        const int cfg = L[i].cfg;
        if (cfg != SEQ_CFG_C3C1_L3 && cfg != SEQ_CFG_C3C1_L2) continue;
        const int p = prev;
        prev = i;
        if (p < 0 || L[p].cfg != cfg || i != p + 3) continue;
        const int mid = L[p + 2].cfg;
        if (mid != SEQ_CFG_HALO64 && mid != SEQ_CFG_HALO128) continue;
        if ((L[i].Ho * L[i].Wo + 31) / 32 > env.nslots || L[i].Ho != L[p].Ho || L[i].Wo != L[p].Wo) continue;
        if (L[i].res != L[p].out || L[i].res_Cs != L[p].Cos || L[i].res_coff != L[p].cout_off) continue;
        L[i].a_stage |= SEQ_YRES_IN;
        L[p + 2].a_stage |= SEQ_LDS_HI;
        ++marked;
        // the store of Y: does anything but the pair's own second record (from LDS) and this residual read the tensor, anywhere in
        // the list or behind it?  (Conservative: a reader behind a later write of the buffer counts too.)
        bool others = read_after_list(read_after, L[p].out);
        for (int j = 0; j < n && !others; ++j) {
            if (j != p + 1 && L[j].in == L[p].out) others = true;
            if (j != i && L[j].res == L[p].out) others = true;
        }
        if (!others) L[p].a_stage |= SEQ_YRES_NOSTORE;
    }
    return marked;
}

SeqPlanStats plan_seq(std::vector<SeqRec> &rec, const SeqPlanEnv &env, const char *locked, const std::vector<const void *> &read_after) {
    const int n = (int)rec.size();
    std::vector<SeqLayer> L(n);
    std::vector<const void *> wstd(n);
    for (int i = 0; i < n; ++i) { L[i] = rec[i].L; wstd[i] = rec[i].wstd; }
    // the pair split over two CUs trades partial sums through the scratch: an even team, at most SEQ_XCH_PAIRS pairs per team
    const bool xch = env.have_xch && env.nslots % 2 == 0 && env.nslots / 2 <= SEQ_XCH_PAIRS;
    SeqPlanStats st;
    for (int i0 = 0; i0 < n; i0 += SEQ_MAX) {
        const int i1 = std::min(n, i0 + SEQ_MAX);
        st.pairs = seq_fuse_pairs(L.data() + i0, i1 - i0, env.B, locked ? locked + i0 : nullptr, xch);
        st.triples = seq_fuse_triples(L.data(), i0, i1, n, wstd.data(), locked, read_after);
        st.resident = seq_mark_resident(L.data(), i0, i1, n, env, read_after);
    }
    for (int i = 0; i < n; ++i) rec[i].L = L[i];
    return st;
}

double seq_fabric_bytes(const SeqLayer *L, int n, int B, const void *late_read) {
    double ext = 0.0;
    for (int i = 0; i < n; ++i) {
        const SeqLayer &l = L[i];
        bool in_inside = false, res_inside = l.res == nullptr, out_read = false;
        for (int j = 0; j < n; ++j) {
            if (j < i && L[j].out == l.in) in_inside = true;
            if (j < i && l.res && L[j].out == l.res) res_inside = true;
            if (j > i && (L[j].in == l.out || L[j].res == l.out)) out_read = true;
        }
        bool in_counted = false, res_counted = false;          // a tensor several layers read is fetched once
        for (int j = 0; j < i; ++j) {
            if (L[j].in == l.in || L[j].res == l.in) in_counted = true;
            if (l.res && (L[j].in == l.res || L[j].res == l.res)) res_counted = true;
        }
        const double px_in = (double)B * l.Hs * l.Ws, px_out = (double)B * l.Ho * l.Wo;
        ext += (double)l.Nst * l.Kpad * 2.0;
        if (!in_inside && !in_counted) ext += px_in * l.Cs * 2.0;
        if (!res_inside && !res_counted) ext += px_out * l.res_Cs * 2.0;
        if (!out_read || l.out == late_read) ext += px_out * l.Nst * 2.0;
    }
    return ext;
}

// conv_wreg_kernel (weights global -> VGPR) or the LDS-staged kernels?  Returns the tile code 1..8 (WREG_TILE) or 0.
const int WREG_TILE[9][2] = {{0, 0}, {64, 256}, {64, 128}, {64, 64}, {128, 256}, {128, 128}, {128, 64}, {96, 256}, {32, 64}};
int wreg_choice(const ConvParams &p, const ConvOpt &o, int dtype, long ncu) {
    if (o.algo_naive || !conv_wreg_eligible(p, dtype)) return 0;
    if (o.wreg) return o.wreg;
    if (g_tune.wreg >= 2) return g_tune.wreg - 1;
    if (!g_tune.wreg) return 0;
    // per-shape choice, fitted to profiles/r02_wregbench_b8_b64.json (A/B against the best LDS-staged instantiation in
    // one process): the register path wins where the weight stream is long and the tile is N-wide -- the two strided /
    // wide 3x3 projections (l2.0.ds x1.10-1.15, l3.0.ds x1.05-1.08) and, while M is small (B <= ~16), the 1x1
    // reductions with K >= 512 (l3.c1 x1.13, l3.0.c1 x1.10, l2.c1 x1.07) and the strided 3x3 of l2.0 (x1.06).
    // It loses on layer1 (short K, large M: x0.5-0.9) and against the halo kernel on 3x3 stride-1 layers.
    const long K = (long)p.kh * p.kw * p.Ci;
    if (g_tune.wreg_policy == 1) {
        // With four producer waves (smk_tune npw, round 2) the register-fed kernel beats the best LDS-staged instantiation on
        // almost every fp16 NHWC layer of the path at B = 1, 8 and 64 (profiles/r02_producer_waves_2_vs_4.txt,
        // r02_producer_waves_layers_b1_b64.json).  Exceptions, kept on the LDS-staged kernels: the 7x7 stem, the short-K 3x3
        // stride-1 layers (the patch-sharing kernel wins or ties: l1.c2, l2.c2, Refine's small convolutions), and at
        // large M the narrow / short-K layers (128-row LDS-staged tiles at two workgroups per CU win: layer1, l2.c1, head0,
        // v1.0 at B = 64).
        if (p.kh > 3) return 0;
        if (p.kh == 3 && p.stride == 1 && K <= 1152) return 0;
        if (p.M > 16384 && !(p.Nst >= 512 || (K >= 2304 && p.Nst >= 128) || (K >= 1024 && p.Nst >= 256) ||
                             (p.kh == 3 && p.stride == 2)))
            return 0;
        // the largest workgroup shape that still hands the chip >= 150 workgroups (N-wide first: 128x256, 64x256, 64x128, 64x64)
        static const int cand[4] = {4, 1, 2, 3};
        const int nr = (p.Nst + 63) / 64 * 64, ng = p.groups > 0 ? p.groups : 1;
        for (int ci = 0; ci < 4; ++ci) {
            const int bm = WREG_TILE[cand[ci]][0], bn = WREG_TILE[cand[ci]][1];
            if (bn > nr && bn > 64) continue;
            if ((long)((p.M + bm - 1) / bm) * ((p.Nst + bn - 1) / bn) * ng >= 150) {
                // 128 x 256 with 129 .. 255 workgroups leaves CUs idle for a whole tile time (conv_search at B = 8: 53 x 3 = 159
                // tiles on 256 CUs); 96 rows (code 7) = 213 tiles, still one round, each 3/4 as long (smk_tune "wreg96", round 5)
                if (cand[ci] == 4 && g_tune.wreg96) {
                    const long tn = (p.Nst + 255) / 256 * ng;
                    const long t128 = (long)((p.M + 127) / 128) * tn, t96 = (long)((p.M + 95) / 96) * tn;
                    if (((t128 + ncu - 1) / ncu) * 128 > ((t96 + ncu - 1) / ncu) * 96 && t96 <= 4 * ncu) return 7;
                }
                return cand[ci];
            }
        }
        // nothing fills the chip: 64 x 64 -- or 32 x 64 (code 8, smk_tune "wreg32") while even that leaves CUs idle: the narrow tiles' K loops wait for
        // their activation refills (profiles/r06t_wreg_ring_depth.txt), and a 32-row workgroup asks for half of them
        if (g_tune.wreg32 && (long)((p.M + 63) / 64) * ((p.Nst + 63) / 64) * ng < g_tune.wreg32) return 8;
        return 3;
    }
    if (p.M < 4096) return 0;                  // not measured below B ~ 5: keep the fitted LDS-staged choice
    if (p.kh == 3 && K >= 2304 && p.Nst >= 512)
        return ((long)((p.M + 127) / 128) * ((p.Nst + 255) / 256) >= 200) ? 4 : 1;       // 128x256 once it fills the chip
    if (p.M > 16384) return 0;
    if (p.kh == 1 && K >= 512 && p.Nst <= 256) return p.Nst >= 192 ? 2 : 3;               // 64x128 / 64x64
    if (p.kh == 3 && p.stride == 2 && K >= 1152 && p.Nst <= 128) return 3;
    return 0;
}
// depth of conv_wreg_kernel's activation ring: three K tiles; four in split-operand contexts (their K loops are three times as long and mostly on the
// narrow tiles: +2.3 .. 2.6 % on the B = 8 step) and for one or two streams (every layer on 64 x 64 tiles: +1.8 % on the B = 1 step).  Deeper rings (5 .. 7)
// lose everywhere, and so does running the WEIGHT stream further ahead: profiles/r06q_x3_ring_depth_b1_levers.txt, r06t_wreg_ring_depth.txt, r06r_wreg_deep_prefetch.txt
int wreg_stages(int ctx_dtype, int B) {
    if (g_tune.wreg_stages) return g_tune.wreg_stages;
    return (ctx_dtype == DT_F16X3 || (B >= 1 && B <= 2)) ? 4 : 3;
}
// per-op entry points: bits 6-7 of the tile code -- 0 the library's choice, 1 eight k-steps ahead on every shape (conv_wreg.hip WregDepth; MEASURE builds,
// otherwise the three-deep ring), 2 / 3 a 3- / 4-deep ring
int wreg_stages_from_code(int code) {
    const int st = (code >> 6) & 3;
    return st == 0 ? wreg_stages(DT_F16, 0) : (st == 1 ? 8 : (st == 2 ? 3 : 4));
}

// conv_pp_kernel (conv_pp.hip: 256 x 256 tiles, two wave groups alternating between fetching and multiplying) takes the long-K
// convolutions once 256-row tiles fill the chip in (nearly) whole rounds -- the 3x3 shortcuts and layer3's conv2 from B ~ 53 (BASELINE
// configs[4]): +1.3..3.8 % per launch over the register-fed 128 x 256 tile; conv_search's 633 tiles are 2.47 rounds (0.82 of three) and
// stay on the register-fed kernel (-6 %); profiles/r06a_pp_first_contact.txt.  Below ~200 tiles the launch is a partial round of a few
// long tiles and the smaller tiles win (B = 32: -6..-60 %).  pp = 2 (A/B knob): any K, e.g. the Bottlenecks' 1x1 convolutions.
bool pp_choice(const ConvParams &p, const ConvOpt &o, int dtype, long ncu) {
    if (!g_tune.pp || o.algo_naive || o.halo || o.wreg || o.tile_code || !conv_pp_eligible(p, dtype)) return false;
    const long K = (long)p.kh * p.kw * p.Ci;
    const long tiles = (long)((p.M + 255) / 256) * ((p.Nst + 255) / 256);
    const long rounds = (tiles + ncu - 1) / ncu;
    if (tiles < 200 || tiles * 10 < rounds * ncu * 9 || p.Nst < 256 || (p.Nst % 256) != 0) return false;
    return g_tune.pp == 2 || K >= 2304;
}

ConvPlan plan_conv(const ConvParams &p, const ConvOpt &o, const PackedConv &pc, int dtype, int B, long ncu) {
    const int kd = kdtype(dtype);
    ConvPlan pl;
    pl.tile = tile_from_code(o.tile_code, p, kd);
    if (o.algo_naive) { pl.kind = CK_NAIVE; return pl; }
    // the 63x63 mask head as its own launch (depth-2 pipelining, B > 16) in fp16 contexts: the stationary-pixel tile (smk_tune "chain_mask" = 2,
    // fp32 and split-operand contexts: the generic tiles)
    if (dtype == DT_F16 && g_tune.chain_mask != 2 && !o.tile_code && !o.halo && !o.wreg && mask_head_eligible(p, kd)) { pl.kind = CK_MHEAD; return pl; }
    // halo_choice's own answer is also an input of the rules below, whether or not the halo kernel then takes the geometry
    int bm = halo_choice(pc, p, o, kd);
    if (bm && !o.halo && conv_ksplit(p, kd, pl.tile) > 1) bm = 0;       // under-filled: split-K on the generic kernel wins
    if (pp_choice(p, o, kd, ncu)) { pl.kind = CK_PP; return pl; }
    // (policy 1 decides between the register-fed and the patch-sharing kernel itself; the round-2 table only covered the
    //  layers the patch-sharing kernel does not take)
    const int wr = (o.halo || (bm && !o.wreg && g_tune.wreg < 2 && g_tune.wreg_policy == 0)) ? 0 : wreg_choice(p, o, kd, ncu);
    if (wr) {
        pl.kind = CK_WREG; pl.wreg = wr; pl.stages = wreg_stages(dtype, B);
    } else if (bm && conv_halo_eligible(p, kd, bm)) {
        // 3x3 stride-1: the activation patch is staged once per channel chunk and shared by the nine taps
        pl.kind = CK_HALO; pl.halo_bm = bm;
    }
    return pl;
}

ConvPlan plan_conv_batch(const ConvBatch &cb, const ConvOpt *const o[], int lead, int dtype, int B, long ncu) {
    const int kd = kdtype(dtype);
    ConvPlan pl;
    int wr = wreg_choice(cb.p[lead], *o[lead], kd, ncu);
    for (int i = 0; i < cb.n && wr; ++i)
        if (!wreg_choice(cb.p[i], *o[i], kd, ncu) || (cb.p[i].groups > 1) != (cb.p[0].groups > 1)) wr = 0;
    if (wr) {
        pl.kind = CK_WREG; pl.wreg = wr; pl.stages = wreg_stages(dtype, B);
    } else {
        pl.tile = tile_from_code(o[lead]->tile_code, cb.p[lead], kd);
    }
    return pl;
}

std::string plan_kernel_name(const ConvPlan &pl, int dtype, int out_mode, int merged) {
    const char *dt = dtname(kdtype(dtype));
    char kn[80], mg[16] = "";
    if (merged) snprintf(mg, sizeof(mg), ",merged%d", merged);
    switch (pl.kind) {
    case CK_NAIVE: return "conv_naive";
    case CK_PP: return "conv_pp<f16,256x256>";
    case CK_MHEAD: return "mask_head<f16,128px,nchw>";
    case CK_HALO: snprintf(kn, sizeof(kn), "conv3x3_halo<%s,%dx128>", dt, pl.halo_bm); break;
    case CK_WREG: snprintf(kn, sizeof(kn), "conv_wreg<%s,%dx%d,s%d%s>", dt, WREG_TILE[pl.wreg][0], WREG_TILE[pl.wreg][1], pl.stages, mg); break;
    default:
        snprintf(kn, sizeof(kn), "conv_igemm<%s,%dx%dx%d,s%d,%s%s>", dt, pl.tile.bm, pl.tile.bn, pl.tile.kt, pl.tile.stages,
                 out_mode == OUT_NCHW_F32 ? "nchw" : "nhwc", mg);
    }
    return kn;
}
