// op_api.cpp -- the entry points of include/siammask_hip_test.h that need no context: single operations on caller tensors
// (smk_op_*: unit parity of the kernels), smk_bench_conv, and the host-only walks and planners the CPU tests pin the engine's
// choices with (smk_host_conv2d_ex, smk_host_plan_conv, smk_host_plan_seq, smk_host_chain_rows).  They pack, plan and launch through the code the
// engine uses (weight_pack.cpp, conv_plan.cpp, conv_launch.cpp).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/siammask_hip_test.h"
#include "chain_rows.h"
#include "engine_internal.h"

using namespace smk;

extern "C" {

// ---- per-op entry points -------------------------------------------------------------------
struct TmpBufs {
    std::vector<void *> v;
    ~TmpBufs() { for (void *p : v) hipFree(p); }
    int alloc(void **p, size_t bytes) {
        HIPCHK(hipMalloc(p, bytes + 256));
        HIPCHK(hipMemset(*p, 0, bytes + 256));
        v.push_back(*p);
        return 0;
    }
};

static int fill_geom(const smk_conv_geom *g, PackedConv &pc, Act &in, ConvOpt &o, int &Ho, int &Wo) {
    const int cin_len = g->cin_len > 0 ? g->cin_len : g->Cin;
    pc.Ci = rup(cin_len, 8);
    pc.k = g->k;
    pc.K = g->k * g->k * pc.Ci;
    pc.Kpad = rup(pc.K, KPAD_ALIGN);
    pc.groups = 1;
    pc.N = g->Cout;
    pc.group_rows = pc.rows = rup(g->Cout, NPAD_ALIGN);
    in.H = g->H; in.W = g->W; in.C = rup(g->Cin, 8);
    o.stride = g->stride; o.pad = g->pad; o.dil = g->dil; o.relu = g->relu;
    o.cin_off = g->cin_off;
    o.win = g->win != 0; o.ups = g->ups != 0;
    o.Hl = g->Hl; o.Wl = g->Wl; o.org_y = g->org_y; o.org_x = g->org_x;
    o.pos_mul = g->pos_mul; o.pos_add = g->pos_add;
    const int Hl = (o.win || o.ups) ? g->Hl : g->H, Wl = (o.win || o.ups) ? g->Wl : g->W;
    Ho = (Hl + 2 * g->pad - g->dil * (g->k - 1) - 1) / g->stride + 1;
    Wo = (Wl + 2 * g->pad - g->dil * (g->k - 1) - 1) / g->stride + 1;
    if (Ho < 1 || Wo < 1) return fail(SMK_E_ARG, "conv geometry gives empty output");
    if (g->cin_off % 8 != 0) return fail(SMK_E_ARG, "cin_off must be a multiple of 8");
    if (g->cin_off + cin_len > g->Cin) return fail(SMK_E_ARG, "channel slice out of range");
    return 0;
}

static void pack_host(const smk_conv_geom *g, const PackedConv &pc, const float *w, const float *b,
                      std::vector<float> &rows, std::vector<float> &bias) {
    const int cin_len = g->cin_len > 0 ? g->cin_len : g->Cin;
    rows.assign((size_t)pc.rows * pc.Kpad, 0.f);
    bias.assign(pc.rows, 0.f);
    std::vector<double> one(g->Cout, 1.0);
    pack_rows(rows, 0, pc.Kpad, w, one.data(), g->Cout, cin_len, g->k, pc.Ci);
    if (b) for (int n = 0; n < g->Cout; ++n) bias[n] = b[n];
}

// split-K scratch of the context-free entry points (per-op tests, smk_bench_conv): one per device, lazily
static int op_ks_scratch(ConvEnv &env) {
    static float *part[64] = {nullptr};
    static unsigned *cnt[64] = {nullptr};
    const int d = env.device;
    if (d < 0 || d >= 64) return 0;
    if (!part[d]) {
        HIPCHK(hipMalloc((void **)&part[d], KS_PART_FLOATS * sizeof(float)));
        HIPCHK(hipMalloc((void **)&cnt[d], KS_CNT * sizeof(unsigned)));
        HIPCHK(hipMemset(cnt[d], 0, KS_CNT * sizeof(unsigned)));
    }
    env.ks_part = part[d];
    env.ks_cnt = cnt[d];
    return 0;
}

// The kernel a per-op entry point's algo code forces (siammask_hip_test.h: low byte 0 / 2 conv_igemm_kernel, 1 / 3 the naive
// kernel, 4 conv3x3_halo_kernel, 5 conv_wreg_kernel, 6 conv_pp_kernel; bits 8..15 the tile code).  Returns 0, -1 for a wreg tile
// code outside 1..8, 1 when the geometry is not eligible for the kernel.
static int plan_from_algo(int algo, const ConvParams &p, int dtype, ConvPlan &pl) {
    const int mode = algo & 0xff, code = (algo >> 8) & 0xff;
    switch (mode) {
    case 1: case 3: pl.kind = CK_NAIVE; return 0;
    case 4:
        pl.kind = CK_HALO; pl.halo_bm = (code & 15) == 1 ? 128 : 64;
        return conv_halo_eligible(p, dtype, pl.halo_bm) ? 0 : 1;
    case 5:
        pl.kind = CK_WREG; pl.wreg = code & 15; pl.stages = wreg_stages_from_code(code);
        if (pl.wreg < 1 || pl.wreg > 8) return -1;
        return conv_wreg_eligible(p, dtype) ? 0 : 1;
    case 6: pl.kind = CK_PP; return conv_pp_eligible(p, dtype) ? 0 : 1;
    case 7: pl.kind = CK_MHEAD; return mask_head_eligible(p, dtype) ? 0 : 1;
    default: pl.kind = CK_IGEMM; pl.tile = tile_from_code(code, p, dtype); return 0;
    }
}

int smk_op_conv2d_ex(int dtype, int algo, const smk_conv_geom *g, const float *x_dev, const float *w_host,
                     const float *b_host, const float *res_dev, const int32_t *pos_host, float *y_dev,
                     void *stream) {
    if (!g || !x_dev || !w_host || !y_dev) return fail(SMK_E_ARG, "smk_op_conv2d_ex: null argument");
    if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_F16X3) return fail(SMK_E_ARG, "bad dtype");
    // DT_F16X3 (unit parity of the split-operand convolution): x, res -> [hi | lo] planes, the pack tripled per tap ([w_hi | w_lo | w_hi]), conv_igemm_kernel's
    // (or wreg_tile's) splitting epilogue, the output read back as hi + lo.  NHWC epilogue only, whole channel range.
    const bool x3 = dtype == DT_F16X3;
    if (x3 && (((algo & 0xff) != 0 && (algo & 0xff) != 5) || g->cin_off || g->cin_len))
        return fail(SMK_E_ARG, "smk_op_conv2d_ex: split-operand convolutions: algo 0 (conv_igemm_kernel) or 5 (conv_wreg_kernel), no channel slice");
    const int ctx_dtype = dtype;
    dtype = kdtype(dtype);
    hipStream_t s = (hipStream_t)stream;
    PackedConv pc; Act in; ConvOpt o; int Ho, Wo;
    CHK(fill_geom(g, pc, in, o, Ho, Wo));
    std::vector<float> rows, bias;
    pack_host(g, pc, w_host, b_host, rows, bias);
    if (x3) {
        const int Ci0 = pc.Ci, K1 = pc.Kpad;
        pc.x3 = true;
        pc.alg_k = g->k * g->k * Ci0;
        pc.Ci = 3 * Ci0;
        pc.K = g->k * g->k * pc.Ci;
        pc.Kpad = rup(pc.K, KPAD_ALIGN);
        std::vector<float> osc;
        split_rows_x3(rows, pc.rows, K1, pc.Kpad, g->k * g->k, Ci0, osc);
        CHK(upload_oscale(pc, osc));
        in.C *= X3_PLANES;
    }
    std::vector<float> fused;
    if (x3 && g_tune.x3_fused && fuse_rows_x3(rows, pc, g->k * g->k, pc.Ci / 3, fused)) CHK(upload_packed(pc, rows, bias, dtype, &fused));
    else
    CHK(upload_packed(pc, rows, bias, dtype));
    TmpBufs tmp;
    tmp.v.push_back(pc.w); tmp.v.push_back(pc.bias);
    if (pc.w_frag) tmp.v.push_back(pc.w_frag);
    if (pc.w_frag16) tmp.v.push_back(pc.w_frag16);
    if (pc.oscale) tmp.v.push_back(pc.oscale);
    const size_t es = esize(dtype);
    CHK(tmp.alloc(&in.p, (size_t)g->B * g->H * g->W * in.C * es));
    CvtInParams ci{x_dev, in.p, g->B, g->Cin, g->H, g->W, x3 ? in.C / X3_PLANES : in.C, 0, x3 ? 1 : 0};
    if (x3 ? launch_cvt_in_x3(ci, s) : launch_cvt_in(ci, dtype, s)) return fail(SMK_E_HIP, "cvt_in launch failed");
    int *pos_dev = nullptr;
    if (pos_host) {
        CHK(tmp.alloc((void **)&pos_dev, sizeof(int) * 2 * g->B));
        HIPCHK(hipMemcpyAsync(pos_dev, pos_host, sizeof(int) * 2 * g->B, hipMemcpyHostToDevice, s));
        o.pos = pos_dev;
    }
    const int mode = algo & 0xff;
    const bool nchw = (mode == 2 || mode == 3 || mode == 7);
    if (mode == 4) {                                   // halo kernel (3x3 stride 1): its chunk-major pack (f16: + the fragment-order copy)
        CHK(upload_halo_pack(pc, rows, dtype));
        if (pc.w_frag_halo) tmp.v.push_back(pc.w_frag_halo);
        if (pc.w_halo) tmp.v.push_back(pc.w_halo);
    }
    Act out, res;
    out.H = Ho; out.W = Wo; out.C = rup(g->Cout, 8) * (x3 ? X3_PLANES : 1);
    if (res_dev && g->res_mode) {
        if (nchw) return fail(SMK_E_ARG, "residual is not supported with the NCHW epilogue");
        res = out;
        CHK(tmp.alloc(&res.p, (size_t)g->B * Ho * Wo * out.C * es));
        CvtInParams cr{res_dev, res.p, g->B, g->Cout, Ho, Wo, x3 ? out.C / X3_PLANES : out.C, 0, x3 ? 1 : 0};
        if (x3 ? launch_cvt_in_x3(cr, s) : launch_cvt_in(cr, dtype, s)) return fail(SMK_E_HIP, "cvt_in launch failed");
        o.res = &res; o.res_mode = g->res_mode;
    }
    ConvEnv env;
    env.dtype = ctx_dtype;
    HIPCHK(hipGetDevice(&env.device));
    CHK(op_ks_scratch(env));
    ConvParams p;
    if (nchw) {
        o.nchw_out = y_dev;
        CHK(conv_params(env, pc, in, nullptr, g->B, o, p));
    } else {
        CHK(tmp.alloc(&out.p, (size_t)g->B * Ho * Wo * out.C * es));
        CHK(conv_params(env, pc, in, &out, g->B, o, p));
    }
    ConvPlan pl;
    const int prc = plan_from_algo(algo, p, dtype, pl);
    if (prc < 0) return fail(SMK_E_ARG, "smk_op_conv2d_ex: wreg tile code 1..8");
    if (prc)
        return fail(SMK_E_ARG, "smk_op_conv2d_ex: %s", pl.kind == CK_HALO ? "geometry is not eligible for the halo kernel"
                    : (pl.kind == CK_WREG ? "geometry / dtype is not eligible for conv_wreg_kernel"
                       : (pl.kind == CK_MHEAD ? "geometry / dtype is not eligible for mask_head_kernel (fp16, 1x1, Cin = 256, Cout <= 4096, no ReLU)"
                          : "geometry / dtype is not eligible for conv_pp_kernel")));
    ConvBatch cb;
    cb.n = 1;
    cb.p[0] = p;
    CHK(launch_plan(pl, cb, pc.w_halo, dtype, s, "conv"));
    if (!nchw) {
        CvtOutParams co{out.p, y_dev, g->B, g->Cout, Ho, Wo, out.C, 0, x3 ? out.C / X3_PLANES : 0};
        if (x3 ? launch_cvt_out_x3(co, s) : launch_cvt_out(co, dtype, s)) return fail(SMK_E_HIP, "cvt_out launch failed");
    }
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// The layers of an smk_seq_op list as sequence records, with smk_op_conv_seq's validation and errors (smk_host_plan_seq shares
// them): layer i's weights come from pack(i, pc), every output tensor from alloc(&p, bytes); xin is the list input.
static int seq_op_records(const smk_seq_op *ops, int n, const Act &xin, int device, const std::function<int(int, PackedConv &)> &pack,
                          const std::function<int(void **, size_t)> &alloc, std::vector<SeqRec> &rec, std::vector<Act> &outs) {
    const int dtype = DT_F16, B = ops[0].g.B;
    ConvEnv env;
    env.dtype = dtype;
    env.device = device;
    rec.assign(n, SeqRec());
    outs.assign(n, Act());
    for (int i = 0; i < n; ++i) {
        const smk_seq_op &op = ops[i];
        if (!op.w_host) return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d has no weights", i);
        if (op.src >= i || op.res_src >= i) return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d reads a later layer", i);
        if (op.g.B != B || op.g.win || op.g.ups) return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d: one batch, no windows", i);
        const Act &in = op.src < 0 ? xin : outs[op.src];
        const int cin_have = op.src < 0 ? ops[0].g.Cin : ops[op.src].g.Cout;
        if (op.g.H != in.H || op.g.W != in.W || op.g.Cin != cin_have)
            return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d geometry does not match its source", i);
        PackedConv pc; Act gin; ConvOpt o; int Ho, Wo;
        CHK(fill_geom(&op.g, pc, gin, o, Ho, Wo));
        CHK(pack(i, pc));
        outs[i].H = Ho; outs[i].W = Wo; outs[i].C = rup(op.g.Cout, 8);
        CHK(alloc(&outs[i].p, (size_t)B * Ho * Wo * outs[i].C * esize(dtype)));
        Act res;
        if (op.g.res_mode) {
            if (op.res_src < -1) return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d wants a residual without a source", i);
            res = op.res_src < 0 ? xin : outs[op.res_src];
            if (res.H != Ho || res.W != Wo || res.C != outs[i].C)
                return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d: residual shape differs from the output", i);
            o.res = &res; o.res_mode = op.g.res_mode;
        }
        ConvParams p;
        CHK(conv_params(env, pc, in, &outs[i], B, o, p));
        SeqLayer &L = rec[i].L;
        const int force_halo = op.cfg == SEQ_CFG_HALO128 ? 128 : (op.cfg == SEQ_CFG_HALO64 ? 64 : (op.cfg >= 0 ? -1 : 0));
        if (!seq_layer_from(p, dtype, L, force_halo)) return fail(SMK_E_ARG, "smk_op_conv_seq: layer %d cannot run inside a sequence%s", i, force_halo > 0 ? " on the patch-sharing tile" : "");
        if (op.cfg >= 0 && force_halo <= 0) {
#ifdef SMK_MEASURE
            if (op.cfg > 18) return fail(SMK_E_ARG, "smk_op_conv_seq: cfg 0..18");
#else
            if (op.cfg > 9 || (op.cfg >= 6 && op.cfg <= 8))
                return fail(SMK_E_ARG, "smk_op_conv_seq: cfg 0..5, 9 (6..8, 10..18 are measurement tiles: `make MEASURE=1`)");
#endif
            L.cfg = (signed char)op.cfg;
        }
        if (op.kstag >= 0) L.kstag = (signed char)(op.kstag != 0);
        L.sync = (signed char)(op.sync != 0);
        rec[i].wstd = pc.w_frag;
        rec[i].id = "op" + std::to_string(i);
    }
    return 0;
}

// plan_seq on an smk_seq_op list: a layer with a cfg of its own is locked, the outputs the caller reads back are read behind the list
static SeqPlanStats plan_seq_ops(const smk_seq_op *ops, std::vector<SeqRec> &rec, const std::vector<Act> &outs, int grid) {
    std::vector<char> locked(rec.size());
    std::vector<const void *> read_after;
    for (size_t i = 0; i < rec.size(); ++i) {
        locked[i] = ops[i].cfg >= 0;
        if (ops[i].y_dev) read_after.push_back(outs[i].p);
    }
    return plan_seq(rec, {ops[0].g.B, grid >> 3, true}, locked.data(), read_after);
}

// A sequence of convolutions through conv_seq_kernel on caller-described layers (unit parity of the persistent kernel:
// every tile configuration, residual and independent-member cases; micro-benchmarks of its K loop).  fp16 only.
int smk_op_conv_seq(const smk_seq_op *ops, int n, const float *x_dev, int iters, float *usec_out, float *clk_us_out,
                    int *n_fused_out, void *stream) {
    if (!ops || !x_dev || n < 1 || n > SEQ_MAX || iters < 1) return fail(SMK_E_ARG, "smk_op_conv_seq: bad argument (1..%d layers)", SEQ_MAX);
    hipStream_t s = (hipStream_t)stream;
    const int dtype = DT_F16;
    const size_t es = esize(dtype);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev));
    const int grid = seq_grid_for(prop.multiProcessorCount);
    if (!grid) return fail(SMK_E_STATE, "smk_op_conv_seq: the XCD placement / occupancy check failed on this device");
    TmpBufs tmp;
    const int B = ops[0].g.B;
    Act xin;
    xin.H = ops[0].g.H; xin.W = ops[0].g.W; xin.C = rup(ops[0].g.Cin, 8);
    CHK(tmp.alloc(&xin.p, (size_t)B * xin.H * xin.W * xin.C * es));
    CvtInParams ci{x_dev, xin.p, B, ops[0].g.Cin, xin.H, xin.W, xin.C, 0};
    if (launch_cvt_in(ci, dtype, s)) return fail(SMK_E_HIP, "cvt_in launch failed");
    std::vector<PackedConv> packs(n);
    auto pack = [&](int i, PackedConv &pc) -> int {
        const smk_seq_op &op = ops[i];
        int same = -1;                                    // a layer that names the SAME host weights re-uses the device copy
        for (int j = 0; j < i && same < 0; ++j)           // (micro-benchmarks: L2-warm weights)
            if (ops[j].w_host == op.w_host && ops[j].b_host == op.b_host && ops[j].g.Cout == op.g.Cout &&
                ops[j].g.Cin == op.g.Cin && ops[j].g.k == op.g.k && ops[j].g.cin_len == op.g.cin_len) same = j;
        if (same >= 0) {
            pc.w = packs[same].w; pc.bias = packs[same].bias; pc.w_frag = packs[same].w_frag; pc.w_frag_halo = packs[same].w_frag_halo;
        } else {
            std::vector<float> rows, bias;
            pack_host(&op.g, pc, op.w_host, op.b_host, rows, bias);
            CHK(upload_packed(pc, rows, bias, dtype));
            if (pc.k == 3) CHK(upload_halo_pack(pc, rows, dtype));       // (+ its fragment-order form: the patch-sharing tile)
            tmp.v.push_back(pc.w); tmp.v.push_back(pc.bias);
            if (pc.w_frag) tmp.v.push_back(pc.w_frag);
            if (pc.w_frag16) tmp.v.push_back(pc.w_frag16);
            if (pc.w_halo) tmp.v.push_back(pc.w_halo);
            if (pc.w_frag_halo) tmp.v.push_back(pc.w_frag_halo);
        }
        packs[i] = pc;
        return 0;
    };
    std::vector<SeqRec> rec;
    std::vector<Act> outs;
    CHK(seq_op_records(ops, n, xin, dev, pack, [&](void **p, size_t bytes) { return tmp.alloc(p, bytes); }, rec, outs));
    g_seq_last = plan_seq_ops(ops, rec, outs, grid);          // what the engine does with its own lists (smk_tune "seq_fuse", ...)
    SeqArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.B = B;
    a.flags = g_tune.seq_spoll ? 1 : 0;
    for (int i = 0; i < n; ++i) a.L[i] = rec[i].L;
    unsigned *bar = nullptr;
    int *err = nullptr;
    unsigned long long *clk = nullptr, *clk2 = nullptr;
    CHK(tmp.alloc((void **)&bar, 8 * 32 * sizeof(unsigned)));
    CHK(tmp.alloc((void **)&err, sizeof(int)));
    CHK(tmp.alloc((void **)&clk, sizeof(unsigned long long) * (2 * SEQ_MAX + 1)));
    const char *ck = getenv("SMK_SEQ_CLK");
    const bool want2 = ck && !strcmp(ck, "2");
    if (want2) CHK(tmp.alloc((void **)&clk2, sizeof(unsigned long long) * (12 + 32) * SEQ_MAX));
    float *xch = nullptr;
    CHK(tmp.alloc((void **)&xch, SEQ_XCH_BYTES));
    a.bar = bar; a.xch = xch; a.err = err; a.err_host = nullptr; a.clk = clk; a.clk2 = clk2;
    if (n_fused_out) {
        *n_fused_out = 0;
        for (int i = 0; i < n; ++i) *n_fused_out += a.L[i].cfg == SEQ_CFG_C3C1_2ND;
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    // The outputs and the timed launches come from the instantiation the engine's own lists run (no stamp pointers: the stamps
    // live in the CLK build of the kernel); one more launch of the CLK build then writes the per-layer stamps (same results).
    SeqArgs a_run = a;
    a_run.clk = nullptr; a_run.clk2 = nullptr;
    if (launch_conv_seq(a_run, grid, s)) return fail(SMK_E_HIP, "conv_seq launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipEventRecord(e0, s));
    for (int it = 1; it < iters; ++it)
        if (launch_conv_seq(a_run, grid, s)) return fail(SMK_E_HIP, "conv_seq launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipEventRecord(e1, s));
    if (launch_conv_seq(a, grid, s)) return fail(SMK_E_HIP, "conv_seq launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.f;
    if (iters > 1) HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (usec_out) *usec_out = iters > 1 ? ms * 1000.f / (iters - 1) : 0.f;
    int e = 0;
    HIPCHK(hipMemcpy(&e, err, sizeof(int), hipMemcpyDeviceToHost));
    if (e) return fail(SMK_E_HIP, "conv_seq_kernel reported %s", e == 1 ? "an uneven distribution of workgroups over the XCDs" : "a team-barrier time-out");
    {
        unsigned long long h[2 * SEQ_MAX + 1], h2[(12 + 32) * SEQ_MAX];
        HIPCHK(hipMemcpy(h, clk, sizeof(h), hipMemcpyDeviceToHost));
        if (clk_us_out)
            for (int i = 0; i < n; ++i) {
                clk_us_out[2 * i] = (float)((h[1 + 2 * i] - h[2 * i]) / 100.0);
                clk_us_out[2 * i + 1] = (float)((h[2 + 2 * i] - h[1 + 2 * i]) / 100.0);
            }
        if (ck) {
            if (want2) HIPCHK(hipMemcpy(h2, clk2, sizeof(h2), hipMemcpyDeviceToHost));
            seq_print_clk(a, rec.data(), "smk_op_conv_seq", h, want2 ? h2 : nullptr);
        }
    }
    for (int i = 0; i < n; ++i)
        if (ops[i].y_dev) {
            CvtOutParams co{outs[i].p, ops[i].y_dev, B, ops[i].g.Cout, outs[i].H, outs[i].W, outs[i].C, 0};
            if (launch_cvt_out(co, dtype, s)) return fail(SMK_E_HIP, "cvt_out launch failed");
        }
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int smk_op_conv2d(int dtype, int algo, const float *x_dev, int B, int Cin, int H, int W, const float *w_host,
                  const float *b_host, int Cout, int k, int stride, int pad, int dil, int relu,
                  const float *res_dev, float *y_dev, void *stream) {
    smk_conv_geom g;
    memset(&g, 0, sizeof(g));
    g.B = B; g.Cin = Cin; g.H = H; g.W = W; g.Cout = Cout; g.k = k; g.stride = stride; g.pad = pad; g.dil = dil;
    g.relu = relu; g.res_mode = res_dev ? RES_PRE_RELU : RES_NONE;
    return smk_op_conv2d_ex(dtype, algo, &g, x_dev, w_host, b_host, res_dev, nullptr, y_dev, stream);
}

int smk_op_dw_xcorr(int dtype, const float *x_dev, const float *k_dev, int B, int C, int H, int W, int kh, int kw,
                    float *y_dev, void *stream) {
    if (!x_dev || !k_dev || !y_dev) return fail(SMK_E_ARG, "smk_op_dw_xcorr: null argument");
    if (C % 64 != 0) return fail(SMK_E_ARG, "smk_op_dw_xcorr: C must be a multiple of 64");
    if (kh > 5 || kw > 5 || kh > H || kw > W || (W - kw + 1 + 1) / 2 > 13)
        return fail(SMK_E_ARG, "smk_op_dw_xcorr: unsupported geometry");
    hipStream_t s = (hipStream_t)stream;
    TmpBufs tmp;
    const size_t es = esize(dtype);
    const int Ho = H - kh + 1, Wo = W - kw + 1;
    void *x, *k, *y;
    CHK(tmp.alloc(&x, (size_t)B * H * W * C * es));
    CHK(tmp.alloc(&k, (size_t)B * kh * kw * C * es));
    CHK(tmp.alloc(&y, (size_t)B * Ho * Wo * C * es));
    CvtInParams cx{x_dev, x, B, C, H, W, C, 0}, ck{k_dev, k, B, C, kh, kw, C, 0};
    if (launch_cvt_in(cx, dtype, s) || launch_cvt_in(ck, dtype, s)) return fail(SMK_E_HIP, "cvt_in launch failed");
    XcorrParams xp{x, k, y, B, H, W, kh, kw, Ho, Wo, C, C};
    if (launch_xcorr(xp, dtype, s)) return fail(SMK_E_HIP, "xcorr launch failed");
    CvtOutParams co{y, y_dev, B, C, Ho, Wo, C, 0};
    if (launch_cvt_out(co, dtype, s)) return fail(SMK_E_HIP, "cvt_out launch failed");
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int smk_op_maxpool3x3s2(int dtype, const float *x_dev, int B, int C, int H, int W, float *y_dev, void *stream) {
    if (!x_dev || !y_dev) return fail(SMK_E_ARG, "smk_op_maxpool3x3s2: null argument");
    if (C % 8 != 0) return fail(SMK_E_ARG, "smk_op_maxpool3x3s2: C must be a multiple of 8");
    hipStream_t s = (hipStream_t)stream;
    TmpBufs tmp;
    const size_t es = esize(dtype);
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    void *x, *y;
    CHK(tmp.alloc(&x, (size_t)B * H * W * C * es));
    CHK(tmp.alloc(&y, (size_t)B * Ho * Wo * C * es));
    CvtInParams cx{x_dev, x, B, C, H, W, C, 0};
    if (launch_cvt_in(cx, dtype, s)) return fail(SMK_E_HIP, "cvt_in launch failed");
    PoolParams pp{x, y, B, H, W, C, Ho, Wo};
    if (launch_maxpool(pp, dtype, s)) return fail(SMK_E_HIP, "maxpool launch failed");
    CvtOutParams co{y, y_dev, B, C, Ho, Wo, C, 0};
    if (launch_cvt_out(co, dtype, s)) return fail(SMK_E_HIP, "cvt_out launch failed");
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ---- the fused front end on caller tensors: stem_pool_kernel, l1_block_kernel -----------------------------------------
// An output buffer of these two entries: NHWC fp16, every byte 0xFF before the launch (fp16 NaN: a pixel the kernel does not
// write surfaces as NaN in the result) between two guard bands of a fixed byte.  A band that changed means that a tile wrote
// outside its image -- inside this allocation; a write further out is not seen.
constexpr size_t OP_GUARD = 4096;
constexpr int OP_GUARD_BYTE = 0xA5;
struct GuardedBuf {
    unsigned char *base = nullptr;
    size_t bytes = 0;
    void *p() const { return base + OP_GUARD; }
    int alloc(TmpBufs &tmp, size_t n, hipStream_t s) {
        HIPCHK(hipMalloc((void **)&base, n + 2 * OP_GUARD));
        tmp.v.push_back(base);
        bytes = n;
        HIPCHK(hipMemsetAsync(base, OP_GUARD_BYTE, OP_GUARD, s));
        HIPCHK(hipMemsetAsync(base + OP_GUARD, 0xFF, n, s));
        HIPCHK(hipMemsetAsync(base + OP_GUARD + n, OP_GUARD_BYTE, OP_GUARD, s));
        return 0;
    }
    // after the stream has been synchronised: both bands intact?
    int check(const char *entry, const char *name) const {
        std::vector<unsigned char> h(2 * OP_GUARD);
        HIPCHK(hipMemcpy(h.data(), base, OP_GUARD, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h.data() + OP_GUARD, base + OP_GUARD + bytes, OP_GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * OP_GUARD; ++i)
            if (h[i] != OP_GUARD_BYTE)
                return fail(SMK_E_STATE, "%s: the kernel wrote outside the %s buffer (guard band %s it, byte %d)", entry, name,
                            i < OP_GUARD ? "before" : "after", (int)(i % OP_GUARD));
        return 0;
    }
};

// one convolution's weights for a per-op entry: pack_host -> upload_packed (fp16), the device copies owned by tmp
static int op_pack(TmpBufs &tmp, PackedConv &pc, int Cin, int Cout, int k, const float *w, const float *b) {
    smk_conv_geom g;
    memset(&g, 0, sizeof(g));
    g.B = 1; g.Cin = Cin; g.H = g.W = k; g.Cout = Cout; g.k = k; g.stride = 1; g.dil = 1;
    Act in; ConvOpt o; int Ho, Wo;
    CHK(fill_geom(&g, pc, in, o, Ho, Wo));
    std::vector<float> rows, bias;
    pack_host(&g, pc, w, b, rows, bias);
    const int rc = upload_packed(pc, rows, bias, DT_F16);
    for (void *q : {pc.w, (void *)pc.bias, pc.w_frag, pc.w_frag16})
        if (q) tmp.v.push_back(q);
    return rc;
}

int smk_op_stem_pool(const float *x_dev, const float *w_host, const float *b_host, int S, int B, float *p0_dev, float *x1_dev,
                     void *stream) {
    if (!x_dev || !w_host || !b_host || !p0_dev || !x1_dev) return fail(SMK_E_ARG, "smk_op_stem_pool: null argument");
    if (S < 7 || S > 8192) return fail(SMK_E_ARG, "smk_op_stem_pool: S = %d (7 .. 8192)", S);
    if (B < 1 || B > 1024) return fail(SMK_E_ARG, "smk_op_stem_pool: B = %d (1 .. 1024)", B);
    hipStream_t s = (hipStream_t)stream;
    const int s0 = (S - 7) / 2 + 1, s1 = (s0 - 1) / 2 + 1;
    // the context's pack: pixel-pair rows -> upload_packed -> the fragment-order copy the kernel reads
    PackedConv pc = stem_pack_geom();
    std::vector<float> rows((size_t)pc.rows * pc.Kpad, 0.f), bias(pc.rows, 0.f);
    const std::vector<double> one(64, 1.0), shift(b_host, b_host + 64);
    stem_pair_rows(rows, bias, pc.Kpad, w_host, one.data(), shift.data());
    TmpBufs tmp;
    const int rc = upload_packed(pc, rows, bias, DT_F16);
    for (void *q : {pc.w, (void *)pc.bias, pc.w_frag, pc.w_frag16})
        if (q) tmp.v.push_back(q);
    CHK(rc);
    if (!pc.w_frag) return fail(SMK_E_STATE, "smk_op_stem_pool: internal: the stem has no fragment-order pack");
    GuardedBuf p0, x1;
    CHK(p0.alloc(tmp, (size_t)B * s0 * s0 * 64 * 2, s));
    CHK(x1.alloc(tmp, (size_t)B * s1 * s1 * 64 * 2, s));
    StemPoolParams sp{x_dev, pc.w_frag, pc.bias, p0.p(), x1.p(), B, S, s0, s1, pc.Kpad, 0};
    if (launch_stem_pool(sp, s)) return fail(SMK_E_HIP, "stem_pool launch failed: %s", hipGetErrorString(hipGetLastError()));
    CvtOutParams c0{p0.p(), p0_dev, B, 64, s0, s0, 64, 0}, c1{x1.p(), x1_dev, B, 64, s1, s1, 64, 0};
    if (launch_cvt_out(c0, DT_F16, s) || launch_cvt_out(c1, DT_F16, s)) return fail(SMK_E_HIP, "cvt_out launch failed");
    HIPCHK(hipStreamSynchronize(s));
    CHK(p0.check("smk_op_stem_pool", "p0"));
    CHK(x1.check("smk_op_stem_pool", "x1"));
    return 0;
}

int smk_op_l1_block(const float *x_dev, const float *w1_host, const float *b1_host, const float *w2_host, const float *b2_host,
                    const float *w3_host, const float *b3_host, const float *wd_host, const float *bd_host, int Cin, int S, int B,
                    float *y_dev, void *stream) {
    if (!x_dev || !w1_host || !b1_host || !w2_host || !b2_host || !w3_host || !b3_host || !y_dev)
        return fail(SMK_E_ARG, "smk_op_l1_block: null argument");
    if (Cin != 64 && Cin != 256) return fail(SMK_E_ARG, "smk_op_l1_block: Cin = %d (64: block 0 with its projection, 256)", Cin);
    if (Cin == 64 && (!wd_host || !bd_host)) return fail(SMK_E_ARG, "smk_op_l1_block: Cin = 64 needs the projection shortcut wd, bd");
    if (Cin == 256 && (wd_host || bd_host)) return fail(SMK_E_ARG, "smk_op_l1_block: Cin = 256 has an identity shortcut: wd, bd must be null");
    if (S < 1 || S > 4096) return fail(SMK_E_ARG, "smk_op_l1_block: S = %d (1 .. 4096)", S);
    if (B < 1 || B > 1024) return fail(SMK_E_ARG, "smk_op_l1_block: B = %d (1 .. 1024)", B);
    hipStream_t s = (hipStream_t)stream;
    TmpBufs tmp;
    PackedConv p1, p2, p3, pd;
    CHK(op_pack(tmp, p1, Cin, 64, 1, w1_host, b1_host));
    CHK(op_pack(tmp, p2, 64, 64, 3, w2_host, b2_host));
    CHK(op_pack(tmp, p3, 64, 256, 1, w3_host, b3_host));
    if (Cin == 64) CHK(op_pack(tmp, pd, 64, 256, 1, wd_host, bd_host));
    if (!p1.w_frag16 || !p2.w_frag16 || !p3.w_frag16 || (Cin == 64 && !pd.w_frag16))
        return fail(SMK_E_STATE, "smk_op_l1_block: internal: a layer has no 16x16x32 fragment-order pack");
    void *x;
    CHK(tmp.alloc(&x, (size_t)B * S * S * Cin * 2));
    CvtInParams ci{x_dev, x, B, Cin, S, S, Cin, 0};
    if (launch_cvt_in(ci, DT_F16, s)) return fail(SMK_E_HIP, "cvt_in launch failed");
    GuardedBuf y;
    CHK(y.alloc(tmp, (size_t)B * S * S * 256 * 2, s));
    L1BlockParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.x = x; lp.y = y.p();
    lp.w1 = p1.w_frag16; lp.w2 = p2.w_frag16; lp.w3 = p3.w_frag16;
    lp.b1 = p1.bias; lp.b2 = p2.bias; lp.b3 = p3.bias;
    lp.K1pad = p1.Kpad; lp.K2pad = p2.Kpad; lp.K3pad = p3.Kpad;
    if (Cin == 64) { lp.wd = pd.w_frag16; lp.bd = pd.bias; lp.Kdpad = pd.Kpad; }
    lp.B = B; lp.S = S; lp.Cin = Cin;
    if (launch_l1_block(lp, s)) return fail(SMK_E_HIP, "l1_block launch failed: %s", hipGetErrorString(hipGetLastError()));
    CvtOutParams co{y.p(), y_dev, B, 256, S, S, 256, 0};
    if (launch_cvt_out(co, DT_F16, s)) return fail(SMK_E_HIP, "cvt_out launch failed");
    HIPCHK(hipStreamSynchronize(s));
    CHK(y.check("smk_op_l1_block", "y"));
    return 0;
}

// time repeated launches of one conv geometry (operands are pseudo-random, not zeros: DVFS hygiene)
int smk_bench_conv(int dtype, int algo, const smk_conv_geom *g, int with_res, int iters, float *usec_out,
                   void *stream) {
    if (!g || !usec_out || iters < 1) return fail(SMK_E_ARG, "smk_bench_conv: bad argument");
    if (dtype != DT_F32 && dtype != DT_F16) return fail(SMK_E_ARG, "bad dtype");
    hipStream_t s = (hipStream_t)stream;
    PackedConv pc; Act in; ConvOpt o; int Ho, Wo;
    CHK(fill_geom(g, pc, in, o, Ho, Wo));
    const size_t es = esize(dtype);
    TmpBufs tmp;
    // SMK_BENCH_FILL (measurement aid): what the ACTIVATIONS hold -- uniform [-1, 1) (default), "zero", "relu" (negative values -> 0).  The
    // matrix pipes' clock under load depends on the operand bits (MI355X_MICROARCH.md: zero-filled operands +15..21 % TF/s).
    const char *fm = getenv("SMK_BENCH_FILL");
    const int fill_mode = !fm ? 0 : (!strcmp(fm, "zero") ? 1 : (!strcmp(fm, "relu") ? 2 : 0));
    auto fill = [&](void **dst, size_t elems, float scale, unsigned seed) -> int {
        CHK(tmp.alloc(dst, elems * es));
        std::vector<unsigned char> h(elems * es);
        unsigned st = seed * 2654435761u + 12345u;
        for (size_t i = 0; i < elems; ++i) {
            st = st * 1664525u + 1013904223u;
            float v = ((int)((st >> 9) & 0xffff) - 32768) * (scale / 32768.f);
            if (seed == 1 && fill_mode == 1) v = 0.f;                       // SMK_BENCH_FILL=zero: activations all zero
            if (seed == 1 && fill_mode == 2) v = v > 0.f ? v : 0.f;         // SMK_BENCH_FILL=relu: half of them zero, like a ReLU output
            if (dtype == DT_F16) ((_Float16 *)h.data())[i] = (_Float16)v; else ((float *)h.data())[i] = v;
        }
        HIPCHK(hipMemcpy(*dst, h.data(), elems * es, hipMemcpyHostToDevice));
        return 0;
    };
    CHK(fill(&in.p, (size_t)g->B * g->H * g->W * in.C, 1.0f, 1));
    CHK(fill(&pc.w, (size_t)pc.rows * pc.Kpad, 0.05f, 2));
    CHK(tmp.alloc((void **)&pc.bias, (size_t)pc.rows * 4));
    int *pos_dev = nullptr;
    if (g->pos_mul) {
        CHK(tmp.alloc((void **)&pos_dev, sizeof(int) * 2 * g->B));
        std::vector<int> ph(2 * g->B);
        for (int i = 0; i < 2 * g->B; ++i) ph[i] = 8 + (i * 5) % 9;
        HIPCHK(hipMemcpy(pos_dev, ph.data(), ph.size() * 4, hipMemcpyHostToDevice));
        o.pos = pos_dev;
    }
    const int mode = algo & 0xff;
    if (mode == 5 || mode == 7) pc.w_frag = pc.w;       // timing only: the fragment order is irrelevant
    Act out, res;
    out.H = Ho; out.W = Wo; out.C = rup(g->Cout, 8);
    float *nchw = nullptr;
    const bool nchw_mode = mode == 2 || mode == 7;
    if (nchw_mode) {
        CHK(tmp.alloc((void **)&nchw, (size_t)g->B * g->Cout * Ho * Wo * 4));
        o.nchw_out = nchw;
    } else {
        CHK(tmp.alloc(&out.p, (size_t)g->B * Ho * Wo * out.C * es));
        if (with_res) {
            res = out;
            CHK(fill(&res.p, (size_t)g->B * Ho * Wo * out.C, 1.0f, 3));
            o.res = &res; o.res_mode = RES_PRE_RELU;
        }
    }
    ConvEnv env;
    env.dtype = dtype;
    HIPCHK(hipGetDevice(&env.device));
    CHK(op_ks_scratch(env));
    ConvParams p;
    CHK(conv_params(env, pc, in, nchw_mode ? nullptr : &out, g->B, o, p));
    ConvPlan pl;
    const int prc = plan_from_algo(mode == 1 || mode == 3 ? algo & ~0xff : algo, p, dtype, pl);     // (no naive kernel here: 1 / 3 time the MFMA one)
    if (prc < 0) return fail(SMK_E_ARG, "smk_bench_conv: wreg tile code 1..8");
    if (prc && pl.kind == CK_HALO) return fail(SMK_E_HIP, "conv launch failed or geometry not eligible");
    if (prc) return fail(SMK_E_ARG, "smk_bench_conv: not eligible for %s", pl.kind == CK_WREG ? "conv_wreg_kernel" : (pl.kind == CK_MHEAD ? "mask_head_kernel" : "conv_pp_kernel"));
    auto launch = [&]() {
        ConvBatch cb;                                    // (a launcher writes its grid layout into the batch)
        cb.n = 1;
        cb.p[0] = p;
        return launch_plan(pl, cb, p.wgt, dtype, s, "conv");     // (halo kernel, timing only: the K order is irrelevant)
    };
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) CHK(launch());
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) CHK(launch());
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *usec_out = ms * 1000.f / iters;
    return 0;
}

// host-only walk of the packed matrix + the kernels' gather function (no GPU needed)
int smk_host_conv2d_ex(const smk_conv_geom *g, const float *x, const float *w, const float *b, const float *res,
                       const int32_t *pos, float *y) {
    if (!g || !x || !w || !y) return fail(SMK_E_ARG, "smk_host_conv2d_ex: null argument");
    PackedConv pc; Act in; ConvOpt o; int Ho, Wo;
    CHK(fill_geom(g, pc, in, o, Ho, Wo));
    std::vector<float> rows, bias;
    pack_host(g, pc, w, b, rows, bias);
    // NCHW -> NHWC (channel padded) on the host, mirroring cvt_in_kernel
    std::vector<float> xin((size_t)g->B * g->H * g->W * in.C, 0.f);
    for (int bb = 0; bb < g->B; ++bb)
        for (int c = 0; c < g->Cin; ++c)
            for (int yy = 0; yy < g->H; ++yy)
                for (int xx = 0; xx < g->W; ++xx)
                    xin[(((size_t)bb * g->H + yy) * g->W + xx) * in.C + c] =
                        x[(((size_t)bb * g->Cin + c) * g->H + yy) * g->W + xx];
    in.p = xin.data();
    pc.w = rows.data();
    pc.bias = bias.data();
    o.pos = pos;
    Act out;
    out.H = Ho; out.W = Wo; out.C = rup(g->Cout, 8);
    std::vector<float> obuf((size_t)g->B * Ho * Wo * out.C, 0.f);
    out.p = obuf.data();
    ConvEnv env;
    env.device = -1;
    ConvParams p;
    CHK(conv_params(env, pc, in, &out, g->B, o, p));
    for (int m = 0; m < p.M; ++m) {
        const RowInfo r = row_info(p, m, p.pos);
        for (int n = 0; n < g->Cout; ++n) {
            double acc = 0.0;
            for (int kvec = 0; kvec < p.K; kvec += 4) {
                const KDecode d = decode_k(kvec, p.Ci, p.kw);
                const long off = gather_offset(p, r, d, p.cin_off);
                if (off < 0) continue;
                for (int e = 0; e < 4; ++e) acc += (double)xin[off + e] * (double)rows[(size_t)n * p.Kpad + kvec + e];
            }
            double v = acc + bias[n];
            const int hw = Ho * Wo, bb = m / hw, ps = m - bb * hw;
            const double rv = (res && g->res_mode) ? res[((size_t)bb * g->Cout + n) * hw + ps] : 0.0;
            if (g->res_mode == RES_PRE_RELU) v += rv;
            if (g->relu) v = v > 0 ? v : 0;
            if (g->res_mode == RES_POST_RELU) v += rv;
            y[((size_t)bb * g->Cout + n) * hw + ps] = (float)v;
        }
    }
    return 0;
}

// the pack the packer would make, with every derived copy it would make (host-only planning: nothing is dereferenced)
static void fake_pack(PackedConv &pc, int dtype) {
    static float dummy[64];
    pc.w = dummy; pc.bias = dummy;
    if (has_frag_pack(pc, dtype)) pc.w_frag = dummy;
    if (has_frag16_pack(pc, dtype)) pc.w_frag16 = dummy;
    if (has_halo_pack(pc, dtype)) pc.w_halo = dummy;
    if (has_frag_halo_pack(pc, dtype)) pc.w_frag_halo = dummy;
}

// Which kernel and workgroup shape does the engine pick for one convolution of this geometry?  Host only (CPU tests pin the
// measured layer rules with it): plan_conv, as run_conv calls it, on a pack whose derived copies are the ones the packer would
// make, for the MI355X's 256 CUs; *seq_cfg = the conv_seq_kernel tile code the layer gets inside a persistent sequence, or -1
// when it cannot be part of one.
int smk_host_plan_conv(const smk_conv_geom *g, int dtype, int with_res, int *kernel, int *bm, int *bn, int *seq_cfg) {
    if (!g || !kernel || !bm || !bn || !seq_cfg) return fail(SMK_E_ARG, "smk_host_plan_conv: null argument");
    if (dtype != DT_F32 && dtype != DT_F16) return fail(SMK_E_ARG, "smk_host_plan_conv: dtype");
    PackedConv pc; Act in; ConvOpt o; int Ho, Wo;
    CHK(fill_geom(g, pc, in, o, Ho, Wo));
    static float dummy[64];
    in.p = dummy;
    fake_pack(pc, dtype);
    Act out, res;
    out.H = Ho; out.W = Wo; out.C = rup(g->Cout, 8); out.p = dummy;
    res = out;
    if (with_res) { o.res = &res; o.res_mode = RES_PRE_RELU; }
    ConvEnv env;
    env.device = -1;
    env.dtype = dtype;
    ConvParams p;
    CHK(conv_params(env, pc, in, &out, g->B, o, p));
    const ConvPlan pl = plan_conv(p, o, pc, dtype, g->B, MI355X_CUS);
    switch (pl.kind) {
    case CK_PP: *kernel = 3; *bm = 256; *bn = 256; break;
    case CK_WREG: *kernel = 2; *bm = WREG_TILE[pl.wreg][0]; *bn = WREG_TILE[pl.wreg][1]; break;
    case CK_HALO: *kernel = 1; *bm = pl.halo_bm; *bn = 128; break;
    default: *kernel = 0; *bm = pl.tile.bm; *bn = pl.tile.bn;
    }
    SeqLayer L;
    *seq_cfg = seq_layer_from(p, dtype, L) ? (int)L.cfg : -1;
    return 0;
}

// The marks plan_seq puts on an smk_op_conv_seq list of up to 4 * SEQ_MAX layers (launched as SEQ_MAX slices) on a grid of
// `grid` workgroups.  Host only: the records are smk_op_conv_seq's, on distinct fake tensors and fake packs with the copies the
// packer would make.  The "last launch" diagnostics are left alone.
int smk_host_plan_seq(const smk_seq_op *ops, int n, int grid, int *cfg, int *sync, int *a_stage) {
    if (!ops || n < 1 || n > 4 * SEQ_MAX || grid < 8 || grid % 8 || !cfg || !sync || !a_stage)
        return fail(SMK_E_ARG, "smk_host_plan_seq: bad argument (1..%d layers, a grid of whole teams)", 4 * SEQ_MAX);
    static char tensors[4 * SEQ_MAX + 1];             // one address per tensor: the list input, then the layers' outputs
    Act xin;
    xin.H = ops[0].g.H; xin.W = ops[0].g.W; xin.C = rup(ops[0].g.Cin, 8); xin.p = tensors;
    int next = 1;
    std::vector<SeqRec> rec;
    std::vector<Act> outs;
    CHK(seq_op_records(ops, n, xin, -1, [](int, PackedConv &pc) { fake_pack(pc, DT_F16); return 0; },
                       [&](void **p, size_t) { *p = tensors + next++; return 0; }, rec, outs));
    plan_seq_ops(ops, rec, outs, grid);
    for (int i = 0; i < n; ++i) {
        cfg[i] = rec[i].L.cfg;
        sync[i] = rec[i].L.sync;
        a_stage[i] = rec[i].L.a_stage;
    }
    return 0;
}

// the row bands of the split Refine chain: chain_rows.h's function, the one refine_chain_body.inc compiles
int smk_host_chain_rows(int S, int s, int out[8]) {
    if (!out) return fail(SMK_E_ARG, "smk_host_chain_rows: null argument");
    if (!chain_split_valid(S) || s < 0 || s >= S) return fail(SMK_E_ARG, "smk_host_chain_rows: band %d of %d (1, 2 or 4 bands)", s, S);
    const ChainRows r = chain_rows(S, s);
    out[0] = r.post1[0]; out[1] = r.post1[1];
    out[2] = r.h00[0]; out[3] = r.h00[1];
    out[4] = r.h02[0]; out[5] = r.h02[1];
    out[6] = r.post2[0]; out[7] = r.post2[1];
    return 0;
}

}  // extern "C"
