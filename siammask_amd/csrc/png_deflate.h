// png_deflate.h -- the zlib stream of an 8-bit label map (tools/test.py:518-525 --save_mask), written ONCE for host
// and device: png_kernels.hip runs these functions one lane per position / run / output word, smk_host_png_encode (stream_api.cpp)
// runs them in plain loops on the CPU, and the two agree byte for byte.
//
// FORMAT.  The uncompressed data is the PNG scanline stream S of an H x W uint8 map: per row one filter byte 0, then its W bytes;
// N = H * (W + 1); no interlace, filter type 0 only.  The zlib stream is 0x78 0x01, ONE deflate block with fixed Huffman codes
// (header bits 1, 1, 0), zero bits up to a byte, Adler-32 of S big-endian.  S is cut into its MAXIMAL runs of equal bytes (a filter
// byte merges with label 0 on either side).  A run (v, n) is: one literal v; with r = n - 1, r / 258 matches of length 258; with
// m = r % 258, one match of length m if m >= 3, else m literals v.  Every match has distance 1.  End-of-block follows the last run.
// Huffman codes enter the stream most significant bit first, extra bits least significant bit first.
//
// BITS.  The stream is addressed by bit: bit t of byte j is stream bit 8 j + t, and `put(pos, n, val)` sets stream bit pos + t to
// bit t of val -- so a Huffman code is bit-reversed before it is put.  Stream bits 0..15 are the zlib header, the block starts at
// 16.  A run's `off` is its first bit INSIDE the block (3 for the first run): the exclusive prefix sum of the runs' bit counts + 3.
//
// OWNER COMPUTES.  png_word(w, ...) returns the 32 stream bits [32 w, 32 w + 32) from the run table alone: a binary search for the
// last run that starts at or before bit 32 w, then the tokens of the runs that reach into the window, clipped to it.  The 258-matches
// of a long run are identical 13-bit tokens at off + literal bits + 13 k, so a window finds its first one by a division: the
// thousands of matches of a background run are spread over the words they land in, no lane loops over them.  Nothing is zeroed and
// there are no atomics: every byte below min(n_bytes, cap) is written exactly once, nothing at or past cap ever is.
//
// WORKSPACE (smk_png_workspace(B, W, H, cap)): per plane png_ws_stride(W, H, cap) bytes =
//   16 (PngHead) + 8 * (cap + 1) (PngRun table: a run needs >= 8 bits, so run `cap` starts at or past byte cap and only runs
//   0 .. cap - 1, plus one sentinel that holds the next run's start, are kept) + 8 * ceil(N / 64) (transition words) + N rounded
//   up to 8 (the bytes of S); the total is rounded up to 256.  For the grouped forms W x H is the canvas and a group uses the stride
//   of its lowest member slot.
#ifndef SMK_PNG_DEFLATE_H
#define SMK_PNG_DEFLATE_H

#include <hip/hip_runtime.h>

namespace smk {

#define SMK_PNG_HD __host__ __device__ __forceinline__

constexpr int PNG_MAX_SIDE = 4096;
constexpr unsigned PNG_ADLER_MOD = 65521u;

struct PngRun { unsigned off, start; };                               // first bit inside the block; first position in S
struct PngHead { unsigned end_bits, adler, n_runs, n_bytes; };        // block bits with end-of-block; Adler-32(S); runs; stream bytes

SMK_PNG_HD long png_positions(int W, int H) { return (long)H * ((long)W + 1); }
SMK_PNG_HD long png_words(int W, int H) { return (png_positions(W, H) + 63) / 64; }
// the stream's size from the block's bit count (header 3 + runs + end-of-block 7)
SMK_PNG_HD long png_stream_bytes(long end_bits) { return 2 + (end_bits + 7) / 8 + 4; }
// every byte its own run of a 9-bit literal: 3 + 9 N + 7 bits
SMK_PNG_HD long png_worst_bytes(int W, int H) { return png_stream_bytes(10 + 9 * png_positions(W, H)); }
SMK_PNG_HD size_t png_ws_stride(int W, int H, int cap) {
    const size_t n = (size_t)png_positions(W, H);
    return sizeof(PngHead) + sizeof(PngRun) * ((size_t)cap + 1) + 8 * (size_t)png_words(W, H) + ((n + 7) & ~(size_t)7);
}
SMK_PNG_HD PngHead *png_ws_head(unsigned char *ws) { return (PngHead *)ws; }
SMK_PNG_HD PngRun *png_ws_runs(unsigned char *ws) { return (PngRun *)(ws + sizeof(PngHead)); }
SMK_PNG_HD unsigned long long *png_ws_words(unsigned char *ws, int cap) {
    return (unsigned long long *)(ws + sizeof(PngHead) + sizeof(PngRun) * ((size_t)cap + 1));
}
SMK_PNG_HD unsigned char *png_ws_vals(unsigned char *ws, int cap, int W, int H) {
    return (unsigned char *)(png_ws_words(ws, cap) + png_words(W, H));
}

SMK_PNG_HD unsigned png_rev(unsigned code, int bits) {                // the low `bits` bits of code, reversed
    unsigned r = 0;
    for (int k = 0; k < bits; ++k) r |= ((code >> k) & 1u) << (bits - 1 - k);
    return r;
}
SMK_PNG_HD int png_lit_bits(unsigned v) { return v < 144u ? 8 : 9; }
SMK_PNG_HD unsigned png_lit_token(unsigned v) { return v < 144u ? png_rev(0x30u + v, 8) : png_rev(0x190u + (v - 144u), 9); }
// a match of length 3..257 at distance 1: the last length symbol whose base is <= len (257..264: 3..10 without extra bits, then four
// symbols per extra-bit count e = 1..5), its extra bits, and the 5 zero bits of distance symbol 0.  -> the token, *bits its length
SMK_PNG_HD unsigned png_match_token(int len, int *bits) {
    const unsigned x = (unsigned)(len - 3);
    int e = 0;
    if (x >= 8u) e = (31 - __builtin_clz(x)) - 2;
    const unsigned sym = 257u + 4u * e + (x >> e);
    const unsigned extra = x & ((1u << e) - 1u);
    unsigned code;
    int cb;
    if (sym < 280u) { code = png_rev(sym - 256u, 7); cb = 7; }
    else            { code = png_rev(0xC0u + (sym - 280u), 8); cb = 8; }
    *bits = cb + e + 5;
    return code | (extra << cb);
}
constexpr unsigned PNG_M258 = 0xA3u;                                  // symbol 285 = code 0xC5, 8 bits, reversed; no extra; distance 0
constexpr int PNG_M258_BITS = 13;
// the bits of run (v, n): a closed form
SMK_PNG_HD unsigned png_run_bits(unsigned v, unsigned n) {
    const unsigned L = (unsigned)png_lit_bits(v), r = n - 1u, q = r / 258u, m = r - q * 258u;
    unsigned bits = L + PNG_M258_BITS * q;
    if (m >= 3u) {
        int mb;
        png_match_token((int)m, &mb);
        bits += (unsigned)mb;
    } else {
        bits += m * L;
    }
    return bits;
}
// Adler-32 from the runs: a = 1 + sum v n, b = N + sum v (n (N - s) - n (n - 1) / 2), both mod 65521; the terms are exact integers
// (v n (N - s) < 2^8 * 2^49), so the sums do not depend on their order.  -> the run's terms, each already reduced
SMK_PNG_HD void png_adler_terms(unsigned v, unsigned long long n, unsigned long long s, unsigned long long N, unsigned long long *a,
                                unsigned long long *b) {
    *a = ((unsigned long long)v * n) % PNG_ADLER_MOD;
    *b = ((unsigned long long)v * (n * (N - s) - n * (n - 1ull) / 2ull)) % PNG_ADLER_MOD;
}
SMK_PNG_HD unsigned png_adler_finish(unsigned long long a_sum, unsigned long long b_sum, unsigned long long N) {
    const unsigned a = (unsigned)((1ull + a_sum) % PNG_ADLER_MOD), b = (unsigned)((N + b_sum) % PNG_ADLER_MOD);
    return (b << 16) | a;
}

// stream bits [pos, pos + n) = val, clipped to the window [lo, lo + 32) and ORed into word
SMK_PNG_HD unsigned png_put(unsigned word, long lo, long pos, int n, unsigned long long val) {
    if (pos + n <= lo || pos >= lo + 32) return word;
    const long sh = pos - lo;
    return word | (unsigned)(sh >= 0 ? val << sh : val >> -sh);
}

// the 32 stream bits [32 w, 32 w + 32).  runs[0 .. nrec - 1] are the kept runs and runs[nrec] the sentinel (nrec = min(n_runs, cap));
// vals is S; hd the plane's PngHead
SMK_PNG_HD unsigned png_word(long w, const PngRun *runs, int nrec, const unsigned char *vals, const PngHead &hd) {
    const long lo = 32 * w, hi = lo + 32;
    unsigned word = 0;
    word = png_put(word, lo, 0, 16, 0x0178ull);                       // 0x78 0x01
    word = png_put(word, lo, 16, 3, 3ull);                            // BFINAL 1, BTYPE 01 (least significant bit first)
    int a = 0, b = nrec;                                              // the last run with 16 + off <= lo (run 0 if none)
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (16 + (long)runs[mid].off <= lo) a = mid; else b = mid;
    }
    for (int r = a; r < nrec; ++r) {
        const long P = 16 + (long)runs[r].off;
        if (P >= hi) break;
        const unsigned s = runs[r].start, n = runs[r + 1].start - s, v = vals[s];
        const int L = png_lit_bits(v);
        const unsigned lit = png_lit_token(v);
        word = png_put(word, lo, P, L, lit);
        const unsigned rr = n - 1u, q = rr / 258u, m = rr - q * 258u;
        const long Pm = P + L;
        if (q) {
            const long d = lo - Pm;
            for (long k = d > 0 ? d / PNG_M258_BITS : 0; k < (long)q && Pm + PNG_M258_BITS * k < hi; ++k)
                word = png_put(word, lo, Pm + PNG_M258_BITS * k, PNG_M258_BITS, PNG_M258);
        }
        const long Pr = Pm + (long)PNG_M258_BITS * q;
        if (m >= 3u) {
            int mb;
            const unsigned tok = png_match_token((int)m, &mb);
            word = png_put(word, lo, Pr, mb, tok);
        } else {
            for (unsigned j = 0; j < m; ++j) word = png_put(word, lo, Pr + (long)j * L, L, lit);
        }
    }
    // Adler-32 big-endian behind the padded block (end-of-block is 7 zero bits: nothing to put)
    const long pa = 8 * (2 + ((long)hd.end_bits + 7) / 8);
    const unsigned ad = hd.adler;
    const unsigned be = (ad >> 24) | ((ad >> 8) & 0xff00u) | ((ad << 8) & 0xff0000u) | (ad << 24);
    return png_put(word, lo, pa, 32, be);
}

// ---- launchers (png_kernels.hip) ---------------------------------------------------------------------------------------------------
constexpr int PNG_MAX_SLOTS = 32;
// smk_png_encode (grouped == 0): B planes [H][W] of any bytes, one stream each.  The grouped forms (grouped == 1, B <= 32): W x H is
// the canvas, slot b has the size wh[b] and a stream only if bit b of lead is set (the lowest member of a live group); the other
// rows get meta (0, 0, h, w) and nothing else
struct PngParams {
    const unsigned char *planes;    // byte source, or nullptr: the fused source has filled words / vals
    unsigned char *ws;              // workspace, B strides of png_ws_stride(W, H, cap)
    unsigned char *out;             // [B][cap]
    int *meta;                      // [B][4] = (n_bytes, n_runs, h, w)
    int W, H, cap, grouped;
    unsigned lead;
    int wh[PNG_MAX_SLOTS][2];
};
int launch_png(const PngParams &p, int B, void *stream);
struct VosRleVParams;
// smk_vos_png_v / smk_vos_png_dev_v: v as launch_vos_rle_v takes it (v.words unused); the label of every position of every live group
// goes to the stride of the group's lowest slot, then the scan and the emit of launch_png
int launch_vos_png_v(const VosRleVParams &v, const PngParams &p, int B, void *stream);

}  // namespace smk
#endif
