// jpeg_parse.cpp -- the host side of the JPEG decoder (jpeg_decode.h states the format): smk_host_jpeg_parse walks
// the markers of one file and fills a descriptor row, the table blob and the segment offsets; smk_jpeg_workspace lays a batch out;
// smk_host_jpeg_decode is the CPU twin of the kernels, the same header code in plain loops.  This is the code that faces untrusted
// bytes: it never reads at or past data + len, and every length field is checked against what is left before it is used.
// Nothing here needs HIP: with -DSMK_JPEG_STANDALONE the file and jpeg_decode.h alone make a program (tests/test_jpeg_host.py
// builds one with the address and undefined-behaviour sanitizers).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/siammask_hip.h"
#include "jpeg_decode.h"

namespace smk {
#ifdef SMK_JPEG_STANDALONE
static char jpeg_err[256];
static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(jpeg_err, sizeof(jpeg_err), fmt, ap);
    va_end(ap);
    return code;
}
#else
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...);       // engine.cpp: the library's error string
#endif

static const uint8_t JPEG_ZZ[64] = SMK_JPEG_ZIGZAG;

static inline int rd16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

static int unsupported(const char *what) { return fail(JPEG_UNSUPPORTED, "jpeg: unsupported: %s", what); }
static int corrupt(const char *what) { return fail(JPEG_CORRUPT, "jpeg: corrupt file: %s", what); }

// one DHT table: counts[16] and the symbols behind them -> look / maxcode / valptr / huffval; false: over-subscribed
static bool build_huff(JpegHuff *t, const uint8_t *counts, const uint8_t *vals, int total) {
    memset(t, 0, sizeof(*t));
    memcpy(t->huffval, vals, (size_t)total);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) return false;
        t->valptr[l] = p - code;
        for (int k = 0; k < n; ++k, ++code, ++p)
            if (l <= 9)
                for (int e = code << (9 - l); e < (code + 1) << (9 - l); ++e) t->look[e] = (uint16_t)((l << 8) | vals[p]);
        t->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[0] = -1;
    t->defined = 1;
    return true;
}

// -> JPEG_OK / JPEG_UNSUPPORTED / JPEG_CORRUPT (the reason through fail); *n_seg: offsets written
static int jpeg_parse(const uint8_t *b, size_t len, int32_t *d, JpegTables *T, int32_t *seg, size_t seg_cap) {
    memset(d, 0, sizeof(int32_t) * JPEG_DESC_WORDS);
    memset(T, 0, sizeof(*T));
    if (len > 0x7fffffffu) return unsupported("a file of 2 GiB or more");
    if (len < 4 || b[0] != 0xFF || b[1] != 0xD8) return corrupt("no SOI");
    size_t i = 2;
    int nc = 0, restart = 0, adobe = 0, transform = 0, jfif = 0;
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    for (;;) {
        if (i >= len || b[i] != 0xFF) return corrupt("a marker is expected");
        while (i < len && b[i] == 0xFF) ++i;                          // fill bytes
        if (i >= len) return corrupt("cut inside a marker");
        const int m = b[i++];
        if (m == 0) return corrupt("FF 00 outside entropy data");
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;     // stand-alone markers
        if (m == 0xD9) return corrupt("EOI before SOS");
        if (len - i < 2) return corrupt("cut inside a segment length");
        const size_t L = (size_t)rd16(b + i);
        if (L < 2 || L > len - i) return corrupt("a segment runs past the end of the file");
        const uint8_t *s = b + i + 2;
        const size_t n = L - 2;
        i += L;
        if (m == 0xDB) {
            for (size_t j = 0; j < n;) {
                const int pq = s[j] >> 4, tq = s[j] & 15;
                if (pq == 1) return unsupported("16-bit quantisation table");
                if (pq || tq > 3) return corrupt("DQT");
                if (n - j < 65) return corrupt("DQT is cut");
                for (int k = 0; k < 64; ++k) T->q[tq][JPEG_ZZ[k]] = s[j + 1 + k];
                T->qdef[tq] = 1;
                j += 65;
            }
        } else if (m == 0xC4) {
            for (size_t j = 0; j < n;) {
                const int tc = s[j] >> 4, th = s[j] & 15;
                if (tc > 1 || th > 3) return corrupt("DHT");
                if (n - j < 17) return corrupt("DHT is cut");
                int total = 0;
                for (int k = 0; k < 16; ++k) total += s[j + 1 + k];
                if (total > 256 || n - j - 17 < (size_t)total) return corrupt("DHT is cut");
                if (!build_huff(tc ? &T->ac[th] : &T->dc[th], s + j + 1, s + j + 17, total)) return corrupt("DHT is over-subscribed");
                j += 17 + (size_t)total;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (nc) return corrupt("two frame headers");
            if (n < 6) return corrupt("SOF is cut");
            if (s[0] != 8) return unsupported("sample precision other than 8 bits");
            const int H = rd16(s + 1), W = rd16(s + 3);
            if (H == 0) return unsupported("DNL (height 0 in the frame header)");
            if (W < 1 || W > JPEG_MAX_SIDE || H > JPEG_MAX_SIDE) return unsupported("width or height outside 1..4096");
            if (s[5] != 1 && s[5] != 3) return unsupported("component count other than 1 or 3");
            nc = s[5];
            if (n < 6 + 3 * (size_t)nc) return corrupt("SOF is cut");
            for (int k = 0; k < nc; ++k) {
                cid[k] = s[6 + 3 * k]; ch[k] = s[7 + 3 * k] >> 4; cv[k] = s[7 + 3 * k] & 15; ctq[k] = s[8 + 3 * k];
                if (ctq[k] > 3) return corrupt("SOF names quantisation table > 3");
            }
            d[JD_W] = W; d[JD_H] = H; d[JD_NCOMP] = nc;
        } else if (m == 0xC2) {
            return unsupported("progressive (SOF2)");
        } else if (m >= 0xC3 && m <= 0xCF) {                          // (C4 was handled above)
            return unsupported(m >= 0xC9 ? "arithmetic coding" : "lossless or hierarchical frame");
        } else if (m == 0xDD) {
            if (n < 2) return corrupt("DRI is cut");
            restart = rd16(s);
        } else if (m == 0xDC) {
            return unsupported("DNL");
        } else if (m == 0xE0) {
            if (n >= 5 && !memcmp(s, "JFIF", 5)) jfif = 1;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(s, "Adobe", 5)) { adobe = 1; transform = s[11]; }
        } else if (m == 0xDA) {
            if (!nc) return corrupt("SOS before SOF");
            if (n < 1) return corrupt("SOS is cut");
            const int ns = s[0];
            if (ns != nc) return unsupported("several scans (a scan that does not hold every component)");
            if (n < 4 + 2 * (size_t)ns) return corrupt("SOS is cut");
            for (int k = 0; k < ns; ++k) {
                if (s[1 + 2 * k] != cid[k]) return unsupported("scan components in another order than the frame's");
                const int td = s[2 + 2 * k] >> 4, ta = s[2 + 2 * k] & 15;
                if (td > 3 || ta > 3) return corrupt("SOS names Huffman table > 3");
                if (!T->qdef[ctq[k]] || !T->dc[td].defined || !T->ac[ta].defined) return corrupt("a table the scan needs is not defined");
                d[JD_TQ0 + k] = ctq[k]; d[JD_TD0 + k] = td; d[JD_TA0 + k] = ta;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return unsupported("a scan that is not 0..63, Ah = Al = 0");
            break;
        }                                                             // APPn, COM and everything else with a length: skipped
    }
    int hs = 1, vs = 1;
    if (nc == 3) {
        hs = ch[0]; vs = cv[0];
        if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))
            return unsupported("sampling other than 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2)");
        if (adobe && transform != 1) return unsupported("Adobe colour transform other than YCbCr");
        if (!adobe && !jfif && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') return unsupported("RGB components");
    }                                                                 // (one component: its scan is not interleaved, an MCU is one block)
    d[JD_HS] = hs; d[JD_VS] = vs;
    d[JD_MCU_W] = (d[JD_W] + 8 * hs - 1) / (8 * hs);
    d[JD_MCU_H] = (d[JD_H] + 8 * vs - 1) / (8 * vs);
    d[JD_RESTART] = restart;
    d[JD_ENT_OFF] = (int32_t)i;
    const long M = (long)d[JD_MCU_W] * d[JD_MCU_H], need = restart ? (M + restart - 1) / restart : 1;
    long found = 1;
    if (seg_cap < 1) return fail(SMK_E_ARG, "smk_host_jpeg_parse: room for %ld segment offsets needed", need);
    seg[0] = (int32_t)i;
    size_t j = i;
    while (j < len) {
        const uint8_t *ff = (const uint8_t *)memchr(b + j, 0xFF, len - j);
        if (!ff) { j = len; break; }
        j = (size_t)(ff - b);
        if (j + 1 >= len) break;                                      // a lone FF closes a cut file
        const int m = b[j + 1];
        if (m == 0) { j += 2; continue; }
        if (m == 0xFF) { ++j; continue; }
        if (m >= 0xD0 && m <= 0xD7) {
            j += 2;
            if (found < need) {
                if ((size_t)found >= seg_cap) return fail(SMK_E_ARG, "smk_host_jpeg_parse: room for %ld segment offsets needed", need);
                seg[found] = (int32_t)j;
            }
            ++found;
            continue;
        }
        if (m == 0xDA) return unsupported("several scans");
        if (m == 0xDC) return unsupported("DNL");
        break;                                                        // EOI or another marker
    }
    d[JD_ENT_LEN] = (int32_t)(j - i);
    d[JD_NSEG] = (int32_t)(found < need ? found : need);
    d[JD_STATUS] = found < need ? JPEG_ST_MISSING : 0;
    d[JD_FILE_LEN] = (int32_t)len;
    return JPEG_OK;
}

// the image's coefficients -> its planes: block by block, columns then rows (what jpeg_idct_kernel does with eight lanes a block)
static void host_idct(const int32_t *d, const JpegGeom &g, const JpegTables *T, const int16_t *coef, uint8_t *planes) {
    for (int c = 0; c < g.ncomp; ++c) {
        const uint8_t *q = T->q[d[JD_TQ0 + c] & 3];
        const long pitch = (long)g.cols(c) * 8;
        for (int by = 0; by < g.rows(c); ++by)
            for (int bx = 0; bx < g.cols(c); ++bx) {
                const int16_t *blk = coef + (g.blk0(c) + (long)by * g.cols(c) + bx) * 64;
                uint32_t ws[64], v[8];
                for (int x = 0; x < 8; ++x) {
                    for (int k = 0; k < 8; ++k) v[k] = jpeg_dequant(blk[8 * k + x], q[8 * k + x]);
                    jpeg_idct_1d(v, 11);
                    for (int k = 0; k < 8; ++k) ws[8 * k + x] = v[k];
                }
                for (int y = 0; y < 8; ++y) {
                    for (int k = 0; k < 8; ++k) v[k] = ws[8 * y + k];
                    jpeg_idct_1d(v, 18);
                    uint8_t *o = planes + g.plane0(c) + ((long)by * 8 + y) * pitch + bx * 8;
                    for (int k = 0; k < 8; ++k) o[k] = jpeg_range_limit(v[k]);
                }
            }
    }
}

}  // namespace smk

using namespace smk;

extern "C" {

size_t smk_jpeg_tables_bytes(void) { return sizeof(JpegTables); }

int smk_host_jpeg_parse(const uint8_t *data, size_t len, int32_t *desc_out, void *tables_out, size_t tables_bytes, int32_t *seg_out,
                        size_t seg_cap) {
    if (!data || !desc_out || !tables_out || !seg_out) return fail(SMK_E_ARG, "smk_host_jpeg_parse: null argument");
    if (tables_bytes < sizeof(JpegTables)) return fail(SMK_E_ARG, "smk_host_jpeg_parse: %zu table bytes, %zu needed", tables_bytes, sizeof(JpegTables));
    if (((uintptr_t)tables_out & 3) != 0) return fail(SMK_E_ARG, "smk_host_jpeg_parse: tables_out must be 4-byte aligned");
    return jpeg_parse(data, len, desc_out, (JpegTables *)tables_out, seg_out, seg_cap);
}

size_t smk_jpeg_workspace(int32_t *desc, int n_images) {
    if (!desc || n_images < 1 || n_images > 65535) return 0;
    long segs = 0, blocks = 0;
    for (int n = 0; n < n_images; ++n) {
        int32_t *d = desc + (size_t)n * JPEG_DESC_WORDS;
        if (!jpeg_desc_ok(d)) return 0;
        const JpegGeom g = jpeg_geom(d);
        if (segs + d[JD_NSEG] > 0x7fffffffL || blocks + g.blocks > 0x7fffffffL) return 0;
        d[JD_SEG_OFF] = d[JD_SEG_BASE] = (int32_t)segs;
        d[JD_BLK_BASE] = (int32_t)blocks;
        segs += d[JD_NSEG];
        blocks += g.blocks;
    }
    return jpeg_ws_bytes(n_images, blocks);
}

int smk_host_jpeg_decode(const uint8_t *data, size_t len, uint8_t *out, int64_t pitch, int out_h, int out_w, int32_t *meta_out) {
    if (!data || !out || !meta_out) return fail(SMK_E_ARG, "smk_host_jpeg_decode: null argument");
    if (out_h < 1 || out_w < 1 || out_h > JPEG_MAX_SIDE || out_w > JPEG_MAX_SIDE || pitch < 3 * (int64_t)out_w)
        return fail(SMK_E_ARG, "smk_host_jpeg_decode: out is %d x %d with %lld bytes between rows", out_h, out_w, (long long)pitch);
    int32_t d[JPEG_DESC_WORDS];
    std::vector<JpegTables> T(1);
    const size_t seg_max = (size_t)(JPEG_MAX_SIDE / 8) * (JPEG_MAX_SIDE / 8);
    std::vector<int32_t> seg(len / 2 + 1 < seg_max ? len / 2 + 1 : seg_max);       // (a restart marker takes two bytes)
    const int rc = jpeg_parse(data, len, d, T.data(), seg.data(), seg.size());
    if (rc) return rc;
    if (d[JD_H] != out_h || d[JD_W] != out_w) return fail(SMK_E_ARG, "smk_host_jpeg_decode: the file is %d x %d, out %d x %d", d[JD_H], d[JD_W], out_h, out_w);
    const JpegGeom g = jpeg_geom(d);
    std::vector<int16_t> coef((size_t)g.blocks * 64, 0);
    std::vector<uint8_t> planes((size_t)g.plane_bytes);
    const long M = (long)g.mcu_w * g.mcu_h, R = d[JD_RESTART] ? d[JD_RESTART] : M;
    const uint8_t *ent_end = data + d[JD_ENT_OFF] + d[JD_ENT_LEN];
    int status = d[JD_STATUS];
    for (int s = 0; s < d[JD_NSEG]; ++s) {
        const long m0 = s * R, m1 = m0 + R < M ? m0 + R : M;
        const uint8_t *p = data + seg[(size_t)s];
        status |= jpeg_decode_segment(p, s + 1 < d[JD_NSEG] ? data + seg[(size_t)s + 1] : ent_end, d, g, T.data(), coef.data(), m0, m1, JPEG_ZZ);
    }
    host_idct(d, g, T.data(), coef.data(), planes.data());
    for (int y = 0; y < g.h; ++y)
        for (int x = 0; x < g.w; ++x) jpeg_pixel(planes.data(), g, x, y, out + (size_t)y * (size_t)pitch + 3 * (size_t)x);
    meta_out[0] = status; meta_out[1] = g.h; meta_out[2] = g.w; meta_out[3] = d[JD_NSEG];
    return 0;
}

}  // extern "C"
