// conv_plan.h -- which kernel runs one convolution, and with which workgroup shape; how a recorded list of convolutions
// becomes persistent sequence launches (internal to libsiammask_hip.so).
// Host code only and no HIP runtime call (the CU count and the grid are arguments): every launch path of the engine, its per-op
// entry points and smk_host_plan_conv plan through plan_conv, and seq_flush, smk_op_conv_seq and smk_host_plan_seq through
// plan_seq, so the CPU tests pin what the GPU runs.  conv_launch.cpp's launch_plan is the only code that turns a plan into a launch.
#pragma once
#include <string>
#include <vector>

#include "smk_kernels.h"

struct Act {
    void *p = nullptr;
    int H = 0, W = 0, C = 0;   // C = channel stride
};

struct PackedConv {
    void *w = nullptr;       // device [rows][Kpad] dtype
    void *w_halo = nullptr;  // same weights, K ordered (chunk, kh, kw, c in chunk) for conv3x3_halo_kernel (3x3 only)
    void *w_frag = nullptr;  // same weights in MFMA-fragment order for conv_wreg_kernel (f16 only)
    void *w_frag_halo = nullptr;  // 3x3, f16: the chunk-major matrix (w_halo's K order) in MFMA-fragment order (wreg_halo_tile, sequences)
    void *w_frag16 = nullptr; // small packs (<= 256 rows, K <= 640: layer1): fragment order of v_mfma_f32_16x16x32_f16 (l1_block_kernel)
    float *bias = nullptr;   // device [rows] f32
    int N = 0;               // real output channels per group
    int rows = 0;            // total rows (all groups), multiple of NPAD_ALIGN
    int group_rows = 0;      // rows per group
    int groups = 1;
    int Ci = 0, k = 1, K = 0, Kpad = 0;
    int kw = 0;              // horizontal taps when != k (pixel-pair stem)
    int alg_k = 0;           // algorithmic K (real multiply-accumulates per output) when the pack pads K
    float *oscale = nullptr; // DT_F16X3: device [rows] f32, the inverse of the power-of-two scale each row of the split pack carries (ConvParams::oscale)
    int x3_ct = 0, x3_nreal = 0;   // DT_F16X3, w_frag in FUSED order (ConvParams::x3_ct): channels / 64, activation tiles per K loop
    bool x3 = false;         // DT_F16X3: K tripled -- per tap [w_hi | w_lo | w_hi] against the operand [hi | hi | lo] gathered from the stored planes [hi | lo]; Ci = 3 x channels
};

struct ConvOpt {
    int stride = 1, pad = 0, dil = 1, relu = 0;
    int stride_x = 0;         // horizontal stride when != stride (pixel-pair stem)
    const Act *res = nullptr;
    int res_mode = smk::RES_NONE;
    int res_coff = 0;
    int cin_off = 0;          // channel slice of the input
    int cout_off = 0;
    int n_override = 0;       // use only the first n rows of a fused pack
    int groups = 1;
    // window / upsample view of the input
    bool win = false;
    int Hl = 0, Wl = 0, org_y = 0, org_x = 0;
    const int *pos = nullptr;
    int pos_mul = 0, pos_add = 0;
    bool ups = false;
    // NCHW f32 output
    float *nchw_out = nullptr;
    int algo_naive = 0;
    int tile_code = 0;
    int halo = 0;             // 128 / 64: force the halo kernel with this BM (per-op tests)
    int wreg = 0;             // 1..8: force conv_wreg_kernel with this tile code (per-op tests, micro-benchmark)
};

// DT_F16X3 contexts (smk_kernels.h): the KERNELS are the fp16 ones; what changes is which packs exist and how many channel planes a tensor has
inline int kdtype(int dtype) { return dtype == smk::DT_F16X3 ? smk::DT_F16 : dtype; }
inline const char *dtname(int dt) { return dt == smk::DT_F16 ? "f16" : "f32"; }

#pragma GCC visibility push(hidden)   // (nothing here is part of the library's ABI)

enum ConvKernel { CK_NAIVE, CK_IGEMM, CK_HALO, CK_WREG, CK_PP, CK_MHEAD };   // CK_MHEAD: mask_head_kernel (mask_head_tile.inc)
struct ConvPlan {
    int kind = CK_IGEMM;
    smk::TileChoice tile{};   // CK_IGEMM
    int halo_bm = 0;          // CK_HALO: workgroup height (128 / 64)
    int wreg = 0;             // CK_WREG: tile code (WREG_TILE), ring depth
    int stages = 0;
};

// conv_wreg_kernel's workgroup shapes by tile code 1..8 (64x256, 64x128, 64x64, 128x256, 128x128, 128x64, 96x256, 32x64)
extern const int WREG_TILE[9][2];

smk::TileChoice tile_from_code(int code, const smk::ConvParams &p, int dtype);
int halo_choice(const PackedConv &pc, const smk::ConvParams &p, const ConvOpt &o, int dtype);
int wreg_choice(const smk::ConvParams &p, const ConvOpt &o, int dtype, long ncu);
int wreg_stages(int ctx_dtype, int B);
int wreg_stages_from_code(int code);
bool pp_choice(const smk::ConvParams &p, const ConvOpt &o, int dtype, long ncu);

// One convolution (dtype: the context's, DT_F16X3 included).  For every knob value the kernel that the engine's fallback chain
// pp -> wreg -> halo -> igemm / naive launched; every launcher accepts what it is planned for.
ConvPlan plan_conv(const smk::ConvParams &p, const ConvOpt &o, const PackedConv &pc, int dtype, int B, long ncu);
// Independent convolutions as ONE launch: conv_wreg_kernel when every member takes it (the lead's tile), else conv_igemm_kernel
// with the lead's tile.
ConvPlan plan_conv_batch(const smk::ConvBatch &cb, const ConvOpt *const *o, int lead, int dtype, int B, long ncu);
// the kernel name a profile record carries (merged > 0: members of a merged launch)
std::string plan_kernel_name(const ConvPlan &pl, int dtype, int out_mode, int merged = 0);

// ---- persistent per-XCD convolution sequences (conv_seq_kernel) ----------------------------------------------------
bool seq_halo_ok(const smk::ConvParams &p, int bm);
bool seq_layer_from(const smk::ConvParams &p, int dtype, smk::SeqLayer &L, int force_halo = 0);
bool seq_pair_fusable(const smk::SeqLayer *L, int i, int *code);
// records i, i + 1 as one pair routine at batch B: seq_pair_fusable, and every tensor ends below the routine's out-of-range offset
bool seq_pair_fits(const smk::SeqLayer *L, int i, int B, int *code);

// One recorded convolution of a sequence list.  wstd: the (kh, kw, cin)-ordered fragment pack (the triples need it where the
// record carries the chunk-major one of the patch-sharing tile).
struct SeqRec {
    smk::SeqLayer L;
    const void *wstd = nullptr;
    std::string id;
};
struct SeqPlanEnv {
    int B = 0;
    int nslots = 0;            // workgroups per team: the launch grid / 8
    bool have_xch = false;     // the pair-split exchange scratch exists
};
struct SeqPlanStats { int pairs = 0, triples = 0, resident = 0; };   // of the LAST launch of the list

// The marks on a recorded list, launched as fixed slices of SEQ_MAX records: pairs (cfg), triples (cfg, sync, a_stage) and the
// resident trunk (a_stage).  Pairs and triples never cross a slice, and the backward scans for writers stay inside it (a launch
// boundary orders every earlier write); the forward scans for readers see the whole list and read_after, the buffers read
// after the list ends.  locked (may be null): records whose tile the caller forced.
SeqPlanStats plan_seq(std::vector<SeqRec> &rec, const SeqPlanEnv &env, const char *locked, const std::vector<const void *> &read_after);
// what one launch of n records must move across the fabric if every tensor produced AND consumed inside it stays in the XCD's
// L2: tensors read but not produced here, every weight pack once, tensors produced here and not read here, and late_read
double seq_fabric_bytes(const smk::SeqLayer *L, int n, int B, const void *late_read);

#pragma GCC visibility pop
