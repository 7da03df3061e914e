// conv_launch.cpp -- from (pack, tensors, options) to the kernels' ConvParams, and from a plan (conv_plan.h) to a launch.
// Context-free: the engine passes what it takes from its context as a ConvEnv, the per-op entries of op_api.cpp their own.
#include <cstring>

#include "engine_internal.h"

namespace smk {

int conv_params(const ConvEnv &env, const PackedConv &pc, const Act &in, const Act *out, int B, const ConvOpt &o, ConvParams &p) {
    memset(&p, 0, sizeof(p));
    p.in = in.p;
    p.wgt = pc.w;
    p.wgt_frag = pc.w_frag;
    p.wgt_frag_halo = pc.w_frag_halo;
    p.bias = pc.bias;
    p.oscale = pc.oscale;
    p.pos = o.pos;
    p.B = B;
    p.Hs = in.H; p.Ws = in.W; p.Cs = in.C;
    p.cin_off = o.cin_off;
    p.Ci = pc.Ci;
    p.x3_ct = pc.x3_ct; p.x3_nreal = pc.x3_nreal;
    p.x3_in = pc.x3 ? pc.Ci / 3 : 0;      // split tensor in: the operand's [hi | hi | lo] channels of a tap are gathered from the stored [hi | lo] planes
    p.Hl = (o.win || o.ups) ? o.Hl : in.H;
    p.Wl = (o.win || o.ups) ? o.Wl : in.W;
    p.org_y = o.org_y; p.org_x = o.org_x;
    p.pos_mul = o.pos_mul; p.pos_add = o.pos_add;
    p.ups = o.ups ? 1 : 0;
    p.kh = pc.k;
    p.kw = pc.kw ? pc.kw : pc.k;
    p.stride = o.stride; p.pad = o.pad; p.dil = o.dil;
    p.stride_x = o.stride_x ? o.stride_x : o.stride;
    p.Ho = (p.Hl + 2 * o.pad - o.dil * (p.kh - 1) - 1) / p.stride + 1;
    p.Wo = (p.Wl + 2 * o.pad - o.dil * (p.kw - 1) - 1) / p.stride_x + 1;
    p.K = pc.K; p.Kpad = pc.Kpad;
    p.N = o.n_override ? o.n_override : pc.N;
    p.M = B * p.Ho * p.Wo;
    p.relu = o.relu;
    p.groups = o.groups;
    if (o.groups > 1) {
        p.g_cin_off = pc.x3 ? pc.Ci / 3 * X3_PLANES : pc.Ci;      // branches sit side by side in the channel dimension (split tensors: a branch's
        p.g_wgt_off = pc.group_rows;                               //  two stored planes side by side; pc.Ci is the OPERAND's channel count, 3 per value)
        p.g_cout_off = pc.group_rows * (pc.x3 ? X3_PLANES : 1);
    }
    if (o.nchw_out) {
        p.out = o.nchw_out;
        p.out_mode = OUT_NCHW_F32;
        p.Nst = rup(p.N, 4);
    } else {
        if (!out) return fail(SMK_E_ARG, "conv without output");
        if (out->H != p.Ho || out->W != p.Wo)
            return fail(SMK_E_ARG, "internal: conv output %dx%d != buffer %dx%d", p.Ho, p.Wo, out->H, out->W);
        p.out = out->p;
        p.out_mode = OUT_NHWC;
        p.Cos = out->C;
        p.cout_off = o.cout_off;
        p.Nst = rup(p.N, 8);
        if (pc.x3) {
            // split output: whole-tensor planes (stride = half of the buffer's channels), per-branch planes for a grouped launch
            p.x3_out = o.groups > 1 ? pc.group_rows : out->C / X3_PLANES;
            if (out->C % X3_PLANES || o.cout_off + (o.groups - 1) * X3_PLANES * pc.group_rows + p.x3_out + p.Nst > out->C)
                return fail(SMK_E_ARG, "internal: split conv output channels exceed buffer");
        } else if (o.cout_off + (o.groups - 1) * pc.group_rows + p.Nst > out->C)
            return fail(SMK_E_ARG, "internal: conv output channels exceed buffer");
    }
    p.xcd_mode = g_tune.xcd_mode;
    // NCHW f32 epilogue: a tile writes 128 consecutive positions of each channel plane (512 B at a 4-byte aligned, not
    // line aligned, offset), so the first / last line of every segment is completed by the NEIGHBOURING M tile.  tn-major
    // order runs the M neighbours of one channel block back to back on one XCD: the partial lines meet in that L2
    // before they are evicted (tm-major: the neighbour comes tilesN tiles later -> read-modify-write at the memory side)
    // (measured, profiles/r02_tail_ab.txt: B=64 -1.3 % on the step, B=8 / B=1 within noise -> large launches only)
    if (o.nchw_out && g_tune.nchw_tn_major && p.xcd_mode == 1 && p.M >= 20000 && (double)p.M * p.N * 4 >= 4.0e6) p.xcd_mode = 2;
    p.prio = g_tune.prio;
    p.wave_prio = env.wave_prio;
    {
        const double ib = (double)B * in.H * in.W * in.C * esize(env.dtype), wb = (double)pc.rows * pc.Kpad * esize(env.dtype);
        p.buf_lds = (g_tune.buf_lds && ib < 2.0e9 && wb < 2.0e9) ? 1 : 0;
        p.a_stage = g_tune.a_stage;
        p.res_nt = g_tune.res_nt;
        p.in_bytes = (unsigned)(ib < 4.0e9 ? ib : 0);
        p.w_bytes = (unsigned)(wb < 4.0e9 ? wb : 0);
    }
    p.nt_store = (g_tune.nt_store && o.nchw_out && (double)p.M * p.N * 4 >= 4.0e6) ? 1 : 0;
    p.ci_shift = -1;
    for (int sh = 0; sh < 16; ++sh)
        if ((1 << sh) == p.Ci) p.ci_shift = sh;
    p.kw_magic = 65536 / p.kw + 1;                        // exact for tap < 4096 and kw <= 15
    p.zero = env.device >= 0 ? zero_page() : nullptr;
    if (env.device >= 0 && !p.zero) return fail(SMK_E_HIP, "could not allocate the zero page");
    if (o.res) {
        p.res = o.res->p;
        p.res_Cs = o.res->C;
        p.res_coff = o.res_coff;
        p.res_mode = o.res_mode;
        if (pc.x3) p.x3_res = o.res->C / X3_PLANES;
    }
    p.ksplit = 1;
    p.ks_part = env.ks_part;
    p.ks_cnt = env.ks_cnt;
    p.ks_part_cap = env.ks_part ? KS_PART_FLOATS : 0;
    p.ks_cnt_cap = env.ks_cnt ? KS_CNT : 0;
    return 0;
}

// algorithmic work of one convolution: 2*M*N*K_real flops; bytes = activations read once + weights + output written once
void conv_work(const PackedConv &pc, const ConvParams &p, int B, int dtype, double &flop, double &bytes) {
    const int ng = p.groups > 0 ? p.groups : 1;
    const double kreal = pc.alg_k ? (double)pc.alg_k : (double)p.kh * p.kw * p.Ci;
    const size_t es = esize(kdtype(dtype));
    flop += 2.0 * p.M * (double)p.N * kreal * ng;
    bytes += (double)B * (p.ups ? p.Hs * p.Ws : (double)p.Hl * p.Wl) * p.Ci * es * ng + (double)p.M * p.N * ng * (p.out_mode == OUT_NCHW_F32 ? 4 : es) +
             (double)p.N * kreal * es * ng + (p.res ? (double)p.M * p.N * es : 0.0);
}

// The one place a plan becomes a launch: cb holds the planned problem (CK_PP, CK_HALO, CK_NAIVE: cb.p[0]) or the members of a
// merged one; w_halo is the chunk-major pack of the halo kernel.  A launcher that turns down the geometry it was planned for is
// an internal error, not a fallback.
int launch_plan(const ConvPlan &pl, ConvBatch &cb, const void *w_halo, int dtype, hipStream_t s, const char *what) {
    int rc;
    switch (pl.kind) {
    case CK_PP: rc = launch_conv_pp(cb.p[0], s); break;
    case CK_WREG: rc = launch_conv_wreg_batch(cb, WREG_TILE[pl.wreg][0], WREG_TILE[pl.wreg][1], pl.stages, s); break;
    case CK_HALO: {
        ConvParams ph = cb.p[0];
        ph.wgt = w_halo;
        rc = launch_conv_halo(ph, dtype, pl.halo_bm, s);
        break;
    }
    case CK_NAIVE: rc = launch_conv_naive(cb.p[0], dtype, s); break;
    case CK_MHEAD: rc = launch_mask_head(cb.p[0], s); break;
    default: rc = launch_conv_mfma_batch(cb, dtype, pl.tile, s);
    }
    if (rc == 1) return fail(SMK_E_STATE, "internal: %s is not eligible for the kernel planned for it", what);
    if (rc) return fail(SMK_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // namespace smk
