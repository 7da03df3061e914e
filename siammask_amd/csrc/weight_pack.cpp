// weight_pack.cpp -- host packing and upload of ONE convolution's weights: the [rows][Kpad] matrix and its derived copies
// (fragment order, chunk-major, split operands).  Context-free: BN folding and the layer list (fold, pack_conv, pack_deconv,
// pack_stem, build_weights) read the context and live in engine.cpp; the per-op entries of op_api.cpp pack through the same code.
#include <cmath>
#include <cstring>
#include <vector>

#include "engine_internal.h"

namespace smk {

// host-side packing of ONE weight tensor [Cout][Cin][k][k] (already scaled) into rows of a
// [rows][Kpad] matrix with K ordered (ky, kx, cin_padded)
void pack_rows(std::vector<float> &dst, int row0, int Kpad, const float *w, const double *scale, int Cout, int Cin, int k, int Ci) {
    for (int n = 0; n < Cout; ++n)
        for (int ci = 0; ci < Cin; ++ci)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx) {
                    const double v = (double)w[(((size_t)n * Cin + ci) * k + ky) * k + kx] * scale[n];
                    dst[(size_t)(row0 + n) * Kpad + (size_t)(ky * k + kx) * Ci + ci] = (float)v;
                }
}

// Which derived copies of a pack exist (the packer makes them, smk_host_plan_conv fakes them from the same rules)
bool has_frag_pack(const PackedConv &pc, int dtype) { return dtype == DT_F16 && pc.rows % 32 == 0 && pc.Kpad % 16 == 0; }
bool has_frag16_pack(const PackedConv &pc, int dtype) {
    return has_frag_pack(pc, dtype) && pc.rows <= 256 && pc.Kpad <= 640 && pc.Kpad % 32 == 0 && pc.groups == 1;
}
bool has_halo_pack(const PackedConv &pc, int dtype) { return pc.k == 3 && pc.kw == 0 && pc.Ci % (dtype == DT_F16 ? 64 : 32) == 0; }
bool has_frag_halo_pack(const PackedConv &pc, int dtype) { return has_halo_pack(pc, dtype) && has_frag_pack(pc, dtype) && pc.Kpad == 9 * pc.Ci; }

// fragment-order copy of an f16 pack for conv_wreg_kernel: one contiguous KB per (32 rows, 16 k) MFMA operand --
// [rows/32][Kpad/16][lane 0..63][8 halves] with lane = (n % 32) + 32 * ((k % 16) / 8), element e = k % 8
int upload_frag_pack(PackedConv &pc, const std::vector<float> &rows_f32, int dtype) {
    if (!has_frag_pack(pc, dtype)) return 0;
    const int KS16 = pc.Kpad / 16;
    std::vector<_Float16> h((size_t)pc.rows * pc.Kpad);
    for (int n = 0; n < pc.rows; ++n) {
        const float *src = rows_f32.data() + (size_t)n * pc.Kpad;
        const size_t blk = (size_t)(n / 32) * KS16;
        for (int k = 0; k < pc.Kpad; ++k) {
            const int lane = (n % 32) + 32 * ((k % 16) / 8);
            h[((blk + k / 16) * 64 + lane) * 8 + k % 8] = (_Float16)src[k];
        }
    }
    HIPCHK(hipMalloc(&pc.w_frag, h.size() * 2));
    HIPCHK(hipMemcpy(pc.w_frag, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    if (has_frag16_pack(pc, dtype)) {
        // [rows/16][Kpad/32][lane 0..63][8 halves] with lane = (n % 16) + 16 * ((k % 32) / 8), element e = k % 8
        const int KS32 = pc.Kpad / 32;
        std::vector<_Float16> g((size_t)pc.rows * pc.Kpad);
        for (int n = 0; n < pc.rows; ++n) {
            const float *src = rows_f32.data() + (size_t)n * pc.Kpad;
            const size_t blk = (size_t)(n / 16) * KS32;
            for (int k = 0; k < pc.Kpad; ++k) {
                const int lane = (n % 16) + 16 * ((k % 32) / 8);
                g[((blk + k / 32) * 64 + lane) * 8 + k % 8] = (_Float16)src[k];
            }
        }
        HIPCHK(hipMalloc(&pc.w_frag16, g.size() * 2));
        HIPCHK(hipMemcpy(pc.w_frag16, g.data(), g.size() * 2, hipMemcpyHostToDevice));
    }
    return 0;
}

int upload_packed(PackedConv &pc, const std::vector<float> &rows_f32, const std::vector<float> &bias, int dtype,
                  const std::vector<float> *frag_rows) {
    const size_t n = rows_f32.size();
    HIPCHK(hipMalloc(&pc.w, n * esize(dtype)));
    if (dtype == DT_F16) {
        std::vector<_Float16> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = (_Float16)rows_f32[i];
        HIPCHK(hipMemcpy(pc.w, h.data(), n * 2, hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(pc.w, rows_f32.data(), n * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc((void **)&pc.bias, bias.size() * 4));
    HIPCHK(hipMemcpy(pc.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    return upload_frag_pack(pc, frag_rows ? *frag_rows : rows_f32, dtype);       // derived copy for conv_wreg_kernel (f16 only)
}

// chunk-major copy of a 3x3 pack: k = (tap*Ci + c)  ->  k' = ((c / CH)*9 + tap)*CH + c % CH
int upload_halo_pack(PackedConv &pc, const std::vector<float> &rows_f32, int dtype) {
    if (!has_halo_pack(pc, dtype)) return 0;
    const int CH = dtype == DT_F16 ? 64 : 32;
    std::vector<float> hp(rows_f32.size(), 0.f);
    for (int n = 0; n < pc.rows; ++n)
        for (int tap = 0; tap < 9; ++tap)
            for (int ci = 0; ci < pc.Ci; ++ci)
                hp[(size_t)n * pc.Kpad + (size_t)((ci / CH) * 9 + tap) * CH + ci % CH] =
                    rows_f32[(size_t)n * pc.Kpad + (size_t)tap * pc.Ci + ci];
    const size_t cnt = hp.size();
    if (has_frag_halo_pack(pc, dtype)) {
        // the same matrix in fragment order (upload_frag_pack's layout) for the patch-sharing tile of the sequences
        const int KS16 = pc.Kpad / 16;
        std::vector<_Float16> h(cnt);
        for (int n = 0; n < pc.rows; ++n) {
            const float *src = hp.data() + (size_t)n * pc.Kpad;
            const size_t blk = (size_t)(n / 32) * KS16;
            for (int k = 0; k < pc.Kpad; ++k) {
                const int lane = (n % 32) + 32 * ((k % 16) / 8);
                h[((blk + k / 16) * 64 + lane) * 8 + k % 8] = (_Float16)src[k];
            }
        }
        HIPCHK(hipMalloc(&pc.w_frag_halo, cnt * 2));
        HIPCHK(hipMemcpy(pc.w_frag_halo, h.data(), cnt * 2, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&pc.w_halo, cnt * esize(dtype)));
    if (dtype == DT_F16) {
        std::vector<_Float16> h(cnt);
        for (size_t i = 0; i < cnt; ++i) h[i] = (_Float16)hp[i];
        HIPCHK(hipMemcpy(pc.w_halo, h.data(), cnt * 2, hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(pc.w_halo, hp.data(), cnt * 4, hipMemcpyHostToDevice));
    }
    return 0;
}

// x3 (DT_F16X3 contexts, the layers of the track path's trunk): per tap the Ci0 = rup(Cin, 8) channels three times -- [w_hi | w_lo | w_hi]
// with w_hi = fp16(w), w_lo = fp16(w - w_hi) -- against activations stored as [hi | hi | lo] planes
// Every row is first scaled by a power of two that takes its largest |w| into [2^13, 2^14): w_lo = fp16(s w - w_hi) is then a NORMAL fp16
// number for every weight within 2^-16 of the row's maximum, i.e. the pair carries 22 bits where the unscaled, BN-folded weights (1e-2 .. 1e-3)
// leave w_lo in the subnormals (3e-6 .. 3e-5 relative).  oscale[n] = 1 / s_n (exact); the epilogue multiplies the accumulator by it.
void split_rows_x3(std::vector<float> &rows, int nrows, int Kpad1, int Kpad3, int taps, int Ci0, std::vector<float> &oscale) {
    std::vector<float> out((size_t)nrows * Kpad3, 0.f);
    oscale.assign(nrows, 1.f);
    for (int n = 0; n < nrows; ++n) {
        float mx = 0.f;
        for (int k = 0; k < taps * Ci0; ++k) mx = std::max(mx, std::fabs(rows[(size_t)n * Kpad1 + k]));
        int e = 0;
        if (mx > 0.f) {
            e = 13 - (int)std::floor(std::log2(mx));                 // 2^e mx in [2^13, 2^14)
            e = std::max(-8, std::min(e, 40));
        }
        const float sc = std::ldexp(1.f, e);
        oscale[n] = std::ldexp(1.f, -e);
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < Ci0; ++ci) {
                const float v = rows[(size_t)n * Kpad1 + (size_t)t * Ci0 + ci] * sc;
                const float hi = (float)(_Float16)v, lo = (float)(_Float16)(v - hi);
                float *d = out.data() + (size_t)n * Kpad3 + (size_t)t * 3 * Ci0 + ci;
                d[0] = hi; d[Ci0] = lo; d[2 * Ci0] = hi;
            }
    }
    rows.swap(out);
}
// FUSED order of a split pack for conv_wreg_kernel (wreg_tile.inc x3ct): per tap the 3 CT tiles of 64 weights [w_hi_0 .. | w_lo_0 .. | w_hi_0 ..] become
// (w_hi_0, w_lo_0, w_hi_1, w_lo_1, .., w_hi_{CT-1}, w_lo_{CT-1}, then w_hi_0 .. w_hi_{CT-1} for the lo plane): the two products of a hi activation tile are neighbours
// in the weight stream.  Needs Ci0 % 64 == 0.  Sets pc.x3_ct / pc.x3_nreal; returns false (and leaves `out` alone) when the pack cannot be fused.
bool fuse_rows_x3(const std::vector<float> &rows, PackedConv &pc, int taps, int Ci0, std::vector<float> &out) {
    if (Ci0 < 64 || Ci0 % 64) return false;
    const int CT = Ci0 / 64, Kp = pc.Kpad;
    out.assign(rows.size(), 0.f);
    for (int n = 0; n < pc.rows; ++n) {
        const float *s = rows.data() + (size_t)n * Kp;
        float *d = out.data() + (size_t)n * Kp;
        for (int t = 0; t < taps; ++t) {
            const float *st = s + (size_t)t * 3 * Ci0;
            float *dt = d + (size_t)t * 3 * Ci0;
            for (int j = 0; j < CT; ++j) {
                memcpy(dt + (size_t)(2 * j) * 64, st + (size_t)j * 64, 64 * sizeof(float));                       // w_hi_j   (x hi_j)
                memcpy(dt + (size_t)(2 * j + 1) * 64, st + (size_t)Ci0 + (size_t)j * 64, 64 * sizeof(float));     // w_lo_j   (x hi_j again)
                memcpy(dt + (size_t)(2 * CT + j) * 64, st + (size_t)2 * Ci0 + (size_t)j * 64, 64 * sizeof(float)); // w_hi_j   (x lo_j)
            }
        }
    }
    pc.x3_ct = CT;
    pc.x3_nreal = 0;
    for (int w = 0; w < Kp / 64; ++w) {
        const int r = w % (3 * CT);
        if (!(r < 2 * CT && (r & 1))) ++pc.x3_nreal;       // (the same cyclic rule the consumers apply, K padding included)
    }
    return true;
}
int upload_oscale(PackedConv &pc, const std::vector<float> &oscale) {
    HIPCHK(hipMalloc((void **)&pc.oscale, oscale.size() * 4));
    HIPCHK(hipMemcpy(pc.oscale, oscale.data(), oscale.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// features.conv1 (7x7 s2 p0, 3 -> 64) on the pixel-pair input layout [H][ceil(W/2)][2 px x 4 ch]:
// a 7 x 4 convolution over pixel pairs (vertical stride 2, horizontal stride 1 pair), K = 7*4*8 = 224
// instead of 7*7*8 = 392 with the channel-padded layout; the 8th pixel and the 4th channel have zero weights
void stem_pair_rows(std::vector<float> &rows, std::vector<float> &bias, int Kpad, const float *w, const double *scale, const double *shift) {
    for (int n = 0; n < 64; ++n) {
        for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx)
                for (int ci = 0; ci < 3; ++ci) {
                    const double v = (double)w[(((size_t)n * 3 + ci) * 7 + ky) * 7 + kx] * scale[n];
                    rows[(size_t)n * Kpad + (size_t)(ky * 4 + kx / 2) * 8 + (kx & 1) * 4 + ci] = (float)v;
                }
        bias[n] = (float)shift[n];
    }
}

// the stem's pack (without its weights): geometry of the pixel-pair matrix
PackedConv stem_pack_geom() {
    PackedConv pc;
    pc.Ci = 8; pc.k = 7; pc.kw = 4; pc.K = 7 * 4 * 8; pc.Kpad = rup(pc.K, KPAD_ALIGN); pc.alg_k = 3 * 7 * 7;
    pc.groups = 1; pc.N = 64; pc.group_rows = pc.rows = rup(64, NPAD_ALIGN);
    return pc;
}

}  // namespace smk
