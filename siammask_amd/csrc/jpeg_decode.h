// jpeg_decode.h -- a baseline JPEG file to BGR pixels, the arithmetic written ONCE for host and device:
// jpeg_kernels.hip runs these functions one lane per entropy segment / block column and row / pixel, smk_host_jpeg_decode
// (jpeg_parse.cpp) runs them in plain loops on the CPU, and the two agree byte for byte.  The arithmetic is libjpeg's default
// integer path (islow IDCT, "fancy" chroma upsampling, table colour conversion), so the pixels equal what cv2.imread / PIL give.
// The header compiles without HIP too (the parser's stand-alone sanitizer program).
//
// SCOPE.  SOF0 / SOF1, 8-bit samples, Huffman coding, ONE interleaved scan (Ss 0, Se 63, Ah = Al = 0); 1 component (grey, written
// B = G = R) or 3 components YCbCr; luma sampling 1x1, 2x1 or 2x2 with chroma 1x1; 8-bit quantisation tables; DRI / RSTn; APPn / COM
// skipped; fill 0xFF bytes before markers; FF 00 stuffing.  Everything else is refused by the parser (JPEG_UNSUPPORTED), a file
// whose headers are cut or contradict themselves is JPEG_CORRUPT; neither reaches a kernel.
//
// DESCRIPTOR.  One image is JPEG_DESC_WORDS int32 (the JD_* columns).  The parser writes the FORMAT columns; jpeg_layout writes the
// BATCH columns (where the image's file, tables, segment offsets, coefficients, planes and output are).  Segment offsets (int32,
// relative to the file's first byte) point at the first entropy byte of every segment: behind SOS, and behind every RSTn marker
// found in front of the first other marker.  Segment s holds MCUs [s R, min((s + 1) R, M)) with R the restart interval (M when 0);
// of the segments found only the first ceil(M / R) count, and if fewer were found JPEG_ST_MISSING is set and their MCUs stay zero.
//
// TABLES.  struct JpegTables, one per distinct set of DQT / DHT segments: quantisation tables in NATURAL order, and per Huffman
// table a 9-bit first-level lookup (look[first 9 bits] = length << 8 | symbol, 0: longer than 9) plus the canonical
// maxcode[l] (-1: no code of length l) / valptr[l] (index of the first symbol of length l minus its code) / huffval.
//
// ENTROPY SEGMENT (jpeg_decode_segment).  Bytes are read from the file as stored: FF 00 is the byte FF; the data ends at the first
// FF that is followed by anything else, or at the segment's end; from there on the reader delivers 1 bits.  DC predictions start at
// 0 in every segment.  Per block: DC symbol s (<= 15), s bits, EXTEND, added to the prediction; then k = 1; while k < 64: symbol
// (r, s); s = 0: r = 15 skips 16, else the block ends; otherwise k += r, the value goes to natural position ZZ[k], k += 1.  A bit
// pattern that is no code (JPEG_ST_CODE), k > 63 at a value (JPEG_ST_RUN) or a block that ends inside the padding (JPEG_ST_CUT;
// also reported in place of the other two when padding bits were among those looked at) ends the segment.  Coefficients are int16 in natural order in a zeroed workspace: per component a plane of blocks
// [mcu_h * v][mcu_w * h][64], component 0 first.  Every loop is bounded by the segment's end and by k < 64; every table index is
// masked; nothing outside the image's own coefficients is written whatever the bytes are.
//
// IDCT (jpeg_idct_1d).  jpeg_idct_islow after dequantisation: CONST_BITS 13, PASS1_BITS 2; the column pass descales by 11, the
// row pass by 18, both round by adding half; + 128; the 10-bit masked range limit (x & 1023 read as a signed 10-bit number, then
// clamped to 0..255: a plain clamp for valid streams).  The sums run in uint32 (wrap-around, no undefined overflow on hostile
// bytes) and equal the signed ones wherever those do not overflow.
//
// UPSAMPLING (jpeg_chroma).  Over the component's downsampled size cw x ch = ceil(W / 2) x (ceil(H / 2) or H), NOT the padded
// block grid.  2x2: s = 3 near + far, far the row above for the upper output row and the row below for the lower one, replicated
// at the top and at the last real row; even x: (3 s + s_left + 8) >> 4, odd x: (3 s + s_right + 7) >> 4, first column
// (4 s + 8) >> 4, last (4 s + 7) >> 4.  2x1: even (3 p + p_left + 1) >> 2, odd (3 p + p_right + 2) >> 2, first and last output column
// copy their sample.  As in libjpeg, a component with cw <= 2 is replicated instead (no filter in either direction).
//
// COLOUR (jpeg_bgr).  cb, cr minus 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
// B = Y + ((116130 cb + 32768) >> 16), arithmetic shifts, clamped, stored B, G, R.
//
// WORKSPACE (jpeg_layout).  [n int32 status words, rounded up to 256 bytes][int16 coefficients of every image][uint8 planes of every
// image: per component rows * 8 x cols * 8 at the padded block geometry]; status and coefficients are zeroed in-stream by one memset.
#ifndef SMK_JPEG_DECODE_H
#define SMK_JPEG_DECODE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SMK_JPEG_HD __host__ __device__ __forceinline__
#else
#define SMK_JPEG_HD inline
#endif

namespace smk {

constexpr int JPEG_MAX_SIDE = 4096;
constexpr int JPEG_DESC_WORDS = 32;
constexpr int JPEG_META_WORDS = 4;                                    // (status, h, w, segments)

enum {                                                                // ---- format columns (the parser)
    JD_W = 0, JD_H, JD_NCOMP, JD_HS, JD_VS,                           // size; 1 or 3 components; luma sampling
    JD_MCU_W, JD_MCU_H,                                               // MCUs per row and per column
    JD_TQ0, JD_TQ1, JD_TQ2, JD_TD0, JD_TD1, JD_TD2, JD_TA0, JD_TA1, JD_TA2,   // table ids 0..3 per component
    JD_ENT_OFF, JD_ENT_LEN,                                           // entropy data: first byte behind SOS, bytes up to the closing marker
    JD_RESTART, JD_NSEG, JD_STATUS,                                   // restart interval (0: none), segments that count, JPEG_ST_MISSING
    // ---- batch columns (jpeg_layout / the caller)
    JD_FILE_OFF, JD_FILE_LEN,                                         // the file inside the byte buffer
    JD_TABLE_OFF,                                                     // its JpegTables inside the table buffer (bytes)
    JD_SEG_OFF, JD_SEG_BASE,                                          // its offsets inside the segment table; segments of the images before it
    JD_BLK_BASE,                                                      // blocks of the images before it: where its coefficients and planes are
    JD_SPARE0,
    JD_OUT_LO, JD_OUT_HI, JD_PITCH,                                   // output pointer and bytes between rows
    JD_SPARE
};
static_assert(JD_SPARE == JPEG_DESC_WORDS - 1, "descriptor columns");

enum { JPEG_ST_CODE = 1, JPEG_ST_RUN = 2, JPEG_ST_CUT = 4, JPEG_ST_MISSING = 8 };
enum { JPEG_OK = 0, JPEG_UNSUPPORTED = 1, JPEG_CORRUPT = 2 };

struct JpegHuff {
    uint16_t look[512];
    int32_t maxcode[17];                                              // [1..16]
    int32_t valptr[17];
    uint8_t huffval[256];
    int32_t defined;
};
struct JpegTables {
    uint8_t q[4][64];                                                 // natural order
    int32_t qdef[4];
    JpegHuff dc[4], ac[4];
};

struct JpegGeom {                                                     // what the kernels derive from a descriptor row
    int w, h, ncomp, hs, vs, mcu_w, mcu_h;
    int cols0, rows0, cols1, rows1;                                   // blocks per row / column of the luma plane and of a chroma plane
    long blocks, plane_bytes;
    // (accessors instead of arrays: a component index is a run-time value, and an indexed array would live in scratch memory)
    SMK_JPEG_HD int cols(int c) const { return c == 0 ? cols0 : cols1; }
    SMK_JPEG_HD int rows(int c) const { return c == 0 ? rows0 : rows1; }
    SMK_JPEG_HD long blk0(int c) const {                              // first block of a component among the image's blocks
        const long l = (long)cols0 * rows0, k = (long)cols1 * rows1;
        return c == 0 ? 0 : c == 1 ? l : l + k;
    }
    SMK_JPEG_HD long plane0(int c) const { return blk0(c) * 64; }     // first byte of a component's plane among the image's planes
};

SMK_JPEG_HD JpegGeom jpeg_geom(const int32_t *d) {
    JpegGeom g;
    g.w = d[JD_W]; g.h = d[JD_H]; g.ncomp = d[JD_NCOMP]; g.hs = d[JD_HS]; g.vs = d[JD_VS]; g.mcu_w = d[JD_MCU_W]; g.mcu_h = d[JD_MCU_H];
    g.cols0 = g.mcu_w * g.hs; g.rows0 = g.mcu_h * g.vs;
    g.cols1 = g.ncomp == 3 ? g.mcu_w : 0; g.rows1 = g.ncomp == 3 ? g.mcu_h : 0;
    g.blocks = (long)g.cols0 * g.rows0 + 2 * (long)g.cols1 * g.rows1;
    g.plane_bytes = g.blocks * 64;
    return g;
}

// the format columns of a row are in range (what the parser guarantees; smk_jpeg_decode re-checks rows it is handed)
SMK_JPEG_HD bool jpeg_desc_ok(const int32_t *d) {
    if (d[JD_W] < 1 || d[JD_W] > JPEG_MAX_SIDE || d[JD_H] < 1 || d[JD_H] > JPEG_MAX_SIDE) return false;
    if (d[JD_NCOMP] != 1 && d[JD_NCOMP] != 3) return false;
    const int hs = d[JD_HS], vs = d[JD_VS];
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    if (d[JD_NCOMP] == 1 && (hs != 1 || vs != 1)) return false;
    if (d[JD_MCU_W] != (d[JD_W] + 8 * hs - 1) / (8 * hs) || d[JD_MCU_H] != (d[JD_H] + 8 * vs - 1) / (8 * vs)) return false;
    for (int k = JD_TQ0; k <= JD_TA2; ++k)
        if (d[k] < 0 || d[k] > 3) return false;
    const long M = (long)d[JD_MCU_W] * d[JD_MCU_H];
    if (d[JD_RESTART] < 0 || d[JD_RESTART] > 65535 || d[JD_ENT_OFF] < 0 || d[JD_ENT_LEN] < 0) return false;
    const long need = d[JD_RESTART] ? (M + d[JD_RESTART] - 1) / d[JD_RESTART] : 1;
    return d[JD_NSEG] >= 1 && d[JD_NSEG] <= need && (d[JD_STATUS] & ~JPEG_ST_MISSING) == 0;
}

// ---- entropy decoding ---------------------------------------------------------------------------------------------------------
struct JpegBits {
    const uint8_t *p, *end;
    uint64_t buf;
    int cnt, pad;                                                     // valid low bits of buf; bytes of 1s delivered behind the data
};

SMK_JPEG_HD void jpeg_bits_fill(JpegBits &b) {
    while (b.cnt <= 56) {
        unsigned c = 0xFF;
        if (b.pad || b.p >= b.end) {
            b.pad++;
        } else {
            c = *b.p;
            if (c != 0xFF) b.p += 1;
            else if (b.p + 1 < b.end && b.p[1] == 0) b.p += 2;        // a stuffed FF
            else b.pad = 1;                                           // a marker, a fill byte or the cut: the data ends here
        }
        b.buf = (b.buf << 8) | c;
        b.cnt += 8;
    }
}
SMK_JPEG_HD unsigned jpeg_bits_peek(const JpegBits &b, int n) { return (unsigned)(b.buf >> (b.cnt - n)) & ((1u << n) - 1u); }   // n in 1..16 <= cnt
SMK_JPEG_HD unsigned jpeg_bits_get(JpegBits &b, int n) {              // n in 1..15
    jpeg_bits_fill(b);
    const unsigned v = jpeg_bits_peek(b, n);
    b.cnt -= n;
    return v;
}
SMK_JPEG_HD bool jpeg_bits_cut(const JpegBits &b) { return b.pad * 8 > b.cnt; }     // bits of the padding have been consumed
// why a segment ends early: the data's end wins over what the padding looked like (the 16 bits a refused code was sought in count)
SMK_JPEG_HD int jpeg_bits_why(const JpegBits &b, int st) { return b.pad * 8 > b.cnt - (st == JPEG_ST_CODE ? 16 : 0) ? JPEG_ST_CUT : st; }

SMK_JPEG_HD int jpeg_symbol(JpegBits &b, const JpegHuff *t) {         // -> the symbol, -1: no code
    jpeg_bits_fill(b);
    const unsigned look = t->look[jpeg_bits_peek(b, 9)];
    if (look) {
        b.cnt -= (int)(look >> 8);
        return (int)(look & 255u);
    }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)jpeg_bits_peek(b, l);
        if (code <= t->maxcode[l]) {
            b.cnt -= l;
            return t->huffval[(unsigned)(t->valptr[l] + code) & 255u];
        }
    }
    return -1;
}
SMK_JPEG_HD int jpeg_extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// natural position of the k-th coefficient of the scan: each side keeps the 64 bytes where it reads them fastest
#define SMK_JPEG_ZIGZAG                                                                                                        \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// MCUs [mcu0, mcu1) of one image from the bytes [data, end) into the image's coefficients -> JPEG_ST_* bits
SMK_JPEG_HD int jpeg_decode_segment(const uint8_t *data, const uint8_t *end, const int32_t *d, const JpegGeom &g, const JpegTables *T,
                                    int16_t *coef, long mcu0, long mcu1, const uint8_t *zz) {
    JpegBits b;
    b.p = data; b.end = end; b.buf = 0; b.cnt = 0; b.pad = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (long m = mcu0; m < mcu1; ++m) {
        const int my = (int)(m / g.mcu_w), mx = (int)(m - (long)my * g.mcu_w);
        for (int c = 0; c < g.ncomp; ++c) {
            const int hc = c == 0 ? g.hs : 1, vc = c == 0 ? g.vs : 1;
            const JpegHuff *dc = &T->dc[d[JD_TD0 + c] & 3], *ac = &T->ac[d[JD_TA0 + c] & 3];
            for (int by = 0; by < vc; ++by)
                for (int bx = 0; bx < hc; ++bx) {
                    int16_t *blk = coef + (g.blk0(c) + (long)(my * vc + by) * g.cols(c) + (mx * hc + bx)) * 64;
                    int s = jpeg_symbol(b, dc);
                    if (s < 0 || s > 15) return jpeg_bits_why(b, JPEG_ST_CODE);
                    const int diff = s ? jpeg_extend(jpeg_bits_get(b, s), s) : 0;
                    const int pred = (int16_t)((c == 0 ? pred0 : c == 1 ? pred1 : pred2) + diff);
                    if (c == 0) pred0 = pred;
                    else if (c == 1) pred1 = pred;
                    else pred2 = pred;
                    blk[0] = (int16_t)pred;
                    for (int k = 1; k < 64;) {
                        const int rs = jpeg_symbol(b, ac);
                        if (rs < 0) return jpeg_bits_why(b, JPEG_ST_CODE);
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;
                            k += 16;
                            continue;
                        }
                        k += r;
                        if (k > 63) return jpeg_bits_why(b, JPEG_ST_RUN);
                        blk[zz[k]] = (int16_t)jpeg_extend(jpeg_bits_get(b, s), s);
                        k += 1;
                    }
                    if (jpeg_bits_cut(b)) return JPEG_ST_CUT;
                }
        }
    }
    return 0;
}

// ---- IDCT -----------------------------------------------------------------------------------------------------------------------
// one pass of jpeg_idct_islow over 8 values: v[] in, v[] out, descaled by `shift` with rounding (11: columns, 18: rows)
SMK_JPEG_HD void jpeg_idct_1d(uint32_t v[8], int shift) {
    const uint32_t i0 = v[0], i1 = v[1], i2 = v[2], i3 = v[3], i4 = v[4], i5 = v[5], i6 = v[6], i7 = v[7];
    uint32_t z1 = (i2 + i6) * 4433u;
    const uint32_t t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t o0 = i7, o1 = i5, o2 = i3, o3 = i1;
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 = 0u - z1 * 7373u; z2 = 0u - z2 * 20995u; z3 = z5 - z3 * 16069u; z4 = z5 - z4 * 3196u;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    const uint32_t half = 1u << (shift - 1);
    v[0] = (uint32_t)((int32_t)(t10 + o3 + half) >> shift);
    v[7] = (uint32_t)((int32_t)(t10 - o3 + half) >> shift);
    v[1] = (uint32_t)((int32_t)(t11 + o2 + half) >> shift);
    v[6] = (uint32_t)((int32_t)(t11 - o2 + half) >> shift);
    v[2] = (uint32_t)((int32_t)(t12 + o1 + half) >> shift);
    v[5] = (uint32_t)((int32_t)(t12 - o1 + half) >> shift);
    v[3] = (uint32_t)((int32_t)(t13 + o0 + half) >> shift);
    v[4] = (uint32_t)((int32_t)(t13 - o0 + half) >> shift);
}
SMK_JPEG_HD uint32_t jpeg_dequant(int16_t c, uint8_t q) { return (uint32_t)(int32_t)c * (uint32_t)q; }
SMK_JPEG_HD uint8_t jpeg_range_limit(uint32_t x) {                    // x: a row pass output; + 128 through the masked 10-bit table
    const int m = (int)(x & 1023u), s = (m >= 512 ? m - 1024 : m) + 128;
    return (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
}

// ---- upsampling and colour ------------------------------------------------------------------------------------------------------
// the chroma sample of output pixel (x, y) from a component plane p (pitch bytes between rows), downsampled size cw x ch
SMK_JPEG_HD int jpeg_chroma(const uint8_t *p, long pitch, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(long)y * pitch + x];
    const int cx = x >> 1;
    if (vs == 1) {                                                    // 2x1
        const uint8_t *r = p + (long)y * pitch;
        const int v = r[cx];
        if (cw <= 2) return v;
        if (x & 1) return cx == cw - 1 ? v : (3 * v + r[cx + 1] + 2) >> 2;
        return cx == 0 ? v : (3 * v + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                                            // 2x2
    if (cw <= 2) return p[(long)cy * pitch + cx];
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : fy > ch - 1 ? ch - 1 : fy;
    const uint8_t *near = p + (long)cy * pitch, *far = p + (long)fy * pitch;
    const int s = 3 * near[cx] + far[cx];
    if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}
SMK_JPEG_HD uint8_t jpeg_clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
SMK_JPEG_HD void jpeg_bgr(int Y, int cb, int cr, uint8_t *out) {
    cb -= 128; cr -= 128;
    out[0] = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    out[1] = jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    out[2] = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
}
// pixel (x, y) of an image from its planes (the padded block geometry of g)
SMK_JPEG_HD void jpeg_pixel(const uint8_t *planes, const JpegGeom &g, int x, int y, uint8_t *out) {
    const int Y = planes[g.plane0(0) + (long)y * (g.cols0 * 8) + x];
    if (g.ncomp == 1) {
        out[0] = out[1] = out[2] = (uint8_t)Y;
        return;
    }
    const int cw = (g.w + g.hs - 1) / g.hs, ch = (g.h + g.vs - 1) / g.vs;
    const long pitch = (long)g.cols1 * 8;
    jpeg_bgr(Y, jpeg_chroma(planes + g.plane0(1), pitch, cw, ch, g.hs, g.vs, x, y),
             jpeg_chroma(planes + g.plane0(2), pitch, cw, ch, g.hs, g.vs, x, y), out);
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------
SMK_JPEG_HD size_t jpeg_ws_status_bytes(int n) { return ((size_t)n * 4 + 255) & ~(size_t)255; }
SMK_JPEG_HD int32_t *jpeg_ws_status(unsigned char *ws) { return (int32_t *)ws; }
SMK_JPEG_HD int16_t *jpeg_ws_coef(unsigned char *ws, int n, long blk_base) { return (int16_t *)(ws + jpeg_ws_status_bytes(n)) + blk_base * 64; }
SMK_JPEG_HD uint8_t *jpeg_ws_planes(unsigned char *ws, int n, long n_blocks, long blk_base) {
    return ws + jpeg_ws_status_bytes(n) + (size_t)n_blocks * 128 + (size_t)blk_base * 64;
}
SMK_JPEG_HD size_t jpeg_ws_bytes(int n, long n_blocks) { return (jpeg_ws_status_bytes(n) + (size_t)n_blocks * 192 + 255) & ~(size_t)255; }

// ---- what jpeg_kernels.hip launches ---------------------------------------------------------------------------------------------
struct JpegParams {
    const uint8_t *bytes;
    const int32_t *desc;                                              // device rows
    const int32_t *seg;
    const uint8_t *tables;
    unsigned char *ws;
    int32_t *meta;
    int n_images;
    long n_seg;                                                       // segments of the call
    long n_blocks;                                                    // blocks of the call
    long max_blocks, max_pixels;                                      // the largest image's
    size_t zero_bytes;                                                // status words and coefficients: what the memset clears
};
int launch_jpeg(const JpegParams &p, void *stream);

}  // namespace smk
#endif
