// png_kernels.hip -- the zlib stream of a label map on the device (png_deflate.h has the format and the functions both sides run;
// DESIGN.md 3.22), gfx950.  Three launches per call, none waits for another workgroup:
//   png_bits     one lane per position i of the scanline stream S (row-major, a filter byte 0 in front of every row): the wave
//                keeps its 64 bytes in vals[] and ONE ballot of the transitions S[i] != S[i - 1] in words[].  Lane 0 has no left
//                neighbour in its wave: bit 0 of every word is left clear and png_scan sets it from vals[64 k] != vals[64 k - 1]
//                (bit 0 of word 0 is always a transition: the first run starts there).  The fused form computes the byte as
//                rle_bits_labels_v_kernel computes its label -- the same member walk, warped_prob, given / alive rules, strict > and
//                float32 comparison -- in row-major order, so no label plane is read.
//   png_scan     one workgroup of 1024 per plane walks the words in chunks of 1024, in the style of rle_scan_kernel: a transition at
//                `pos` ENDS the run [prev, pos) of value vals[prev] and STARTS run number (transitions before it).  Two workgroup
//                scans per chunk with running carries -- the exclusive count of transitions with the exclusive maximum of their
//                positions (a word's first run number and the start of the run its first transition ends), then the exclusive sum
//                of the bits of the runs a word ends -- give every run its start and bit offset; the Adler terms are summed per
//                thread and reduced at the end.  Thread 0 closes the last run and writes PngHead, the sentinel and the meta row.
//   png_emit     one lane per 32 output bits (png_word: owner computes, no atomics, nothing zeroed).
// Every exit before a ballot or a barrier is wave- resp. block-uniform: a plane that is not a live group's lowest slot (the block),
// k >= nw (the wave).  No LDS array is indexed by data; nothing spills.
#include <hip/hip_runtime.h>
#include "smk_kernels.h"
#include "tracker_state.h"
#include "warped_prob.h"
#include "png_deflate.h"

namespace smk {

__global__ __launch_bounds__(256) void png_bits_kernel(const PngParams p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int N = (int)png_positions(p.W, p.H), nw = (int)png_words(p.W, p.H);
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), i = k * 64 + lane;
    if (k >= nw) return;
    unsigned v = 0;
    if (i < N) {
        const int y = i / (p.W + 1), c = i - y * (p.W + 1);
        if (c) v = p.planes[((size_t)b * p.H + y) * p.W + (c - 1)];
    }
    const unsigned left = __shfl_up(v, 1);
    const unsigned long long w = __ballot(lane != 0 && i < N && v != left);
    unsigned char *ws = p.ws + (size_t)b * png_ws_stride(p.W, p.H, p.cap);
    if (lane == 0) png_ws_words(ws, p.cap)[k] = w;
    if (i < N) png_ws_vals(ws, p.cap, p.W, p.H)[i] = (unsigned char)v;
}

// the fused source: blockIdx.y is the group; the per-pixel loop is rle_bits_labels_v_kernel's, written out beside it (that kernel
// keeps its instructions), with the position taken row-major over S instead of column-major over the frame
template <bool DEV, bool GIVEN>
__global__ __launch_bounds__(256) void png_bits_labels_v_kernel(const VosRleVParams p, const PngParams q) {
    const int g = blockIdx.y, lane = threadIdx.x & 63;
    if (!((p.live_groups >> g) & 1)) return;
    const unsigned members = p.gmask[g];
    const int W = p.gwh[g][0], H = p.gwh[g][1];
    const int N = (int)png_positions(W, H), nw = (int)png_words(W, H);
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), i = k * 64 + lane;
    if (k >= nw) return;
    int label = 0;
    const int y = i / (W + 1), c = i - y * (W + 1);
    if (i < N && c) {
        const int x = c - 1;
        float best = -1.f;
        int arg = 0, r = 0;
        for (unsigned m = members; m; m &= m - 1, ++r) {
            const int b = __ffs(m) - 1;
            float v = -1.f;
            bool given = false;
            if constexpr (GIVEN) {
                given = (p.given >> b) & 1;
                if (given) v = p.init[g][(size_t)y * W + x] == p.ids[b] ? 1.f : 0.f;
            }
            if (!given && ((p.alive >> b) & 1)) {
                if constexpr (DEV) {
                    const smk_trk_stream *s = p.st + b;
                    const float *lg = p.logits + (size_t)b * p.ms * p.ms;
                    int ls = 1;
                    if (p.head_S) {
                        ls = p.head_S * p.head_S;
                        const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1);
                        const int dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
                        lg = p.logits + (size_t)b * p.ms * p.ms * ls + dy * p.head_S + dx;
                    }
                    v = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y);
                } else {
                    v = warped_prob(p, p.inv_map[b], p.logits + (size_t)b * p.ms * p.ms, 1, x, y);
                }
            }
            if (r == 0 || v > best) { best = v; arg = r; }            // np.argmax keeps the first maximum
        }
        label = best > p.seg_thr ? arg + 1 : 0;
    }
    const int left = __shfl_up(label, 1);
    const unsigned long long w = __ballot(lane != 0 && i < N && label != left);
    unsigned char *ws = q.ws + (size_t)(__ffs(members) - 1) * png_ws_stride(q.W, q.H, q.cap);
    if (lane == 0) png_ws_words(ws, q.cap)[k] = w;
    if (i < N) png_ws_vals(ws, q.cap, q.W, q.H)[i] = (unsigned char)label;
}

__global__ __launch_bounds__(1024) void png_scan_kernel(const PngParams p) {
    __shared__ int s_cnt[16], s_max[16];
    __shared__ unsigned s_bits[16];
    __shared__ unsigned long long s_a[16], s_b[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    int W = p.W, H = p.H;
    if (p.grouped) {
        W = p.wh[b][0]; H = p.wh[b][1];
        if (!((p.lead >> b) & 1)) {                                   // no stream in this row: n_bytes = 0
            if (tid == 0) { int *meta = p.meta + 4 * b; meta[0] = 0; meta[1] = 0; meta[2] = H; meta[3] = W; }
            return;
        }
    }
    const int N = (int)png_positions(W, H), nw = (int)png_words(W, H);
    unsigned char *ws = p.ws + (size_t)b * png_ws_stride(p.W, p.H, p.cap);
    PngRun *runs = png_ws_runs(ws);
    const unsigned long long *words = png_ws_words(ws, p.cap);
    const unsigned char *vals = png_ws_vals(ws, p.cap, p.W, p.H);
    int n_tr = 0, last = 0;                                           // uniform carries: transitions, the last one's position,
    unsigned bits = 0;                                                // the bits of the runs ended so far
    unsigned long long sa = 0, sb = 0;                                // private: Adler terms of the runs this thread ended
    for (int k0 = 0; k0 < nw; k0 += 1024) {
        const int k = k0 + tid;
        unsigned long long t = 0;
        if (k < nw) {
            t = words[k] & ~1ull;
            if (k == 0 || vals[64 * k] != vals[64 * k - 1]) t |= 1ull;
        }
        const int c = __popcll(t);
        int s = c, m = t ? 64 * k + 63 - __clzll((long long)t) : 0;   // inclusive over the wave below
        for (int d = 1; d < 64; d <<= 1) {
            const int s2 = __shfl_up(s, d), m2 = __shfl_up(m, d);
            if (lane >= d) { s += s2; m = max(m, m2); }
        }
        if (lane == 63) { s_cnt[wave] = s; s_max[wave] = m; }
        __syncthreads();
        int o = n_tr + s - c, prev = last, tot = 0, tmax = 0;
        for (int v = 0; v < 16; ++v) {
            const int sv = s_cnt[v], mv = s_max[v];
            if (v < wave) { o += sv; prev = max(prev, mv); }
            tot += sv;
            tmax = max(tmax, mv);
        }
        const int mp = __shfl_up(m, 1);
        if (lane) prev = max(prev, mp);
        unsigned cb = 0;                                              // the bits of the runs this word's transitions end
        {
            int pv = prev;
            for (unsigned long long tt = t; tt; tt &= tt - 1) {
                const int pos = 64 * k + __ffsll((long long)tt) - 1;
                if (pos > 0) {
                    const unsigned v = vals[pv], n = (unsigned)(pos - pv);
                    cb += png_run_bits(v, n);
                    if (v) {
                        unsigned long long ta, tb;
                        png_adler_terms(v, n, (unsigned long long)pv, (unsigned long long)N, &ta, &tb);
                        sa += ta; sb += tb;
                    }
                }
                pv = pos;
            }
        }
        unsigned e = cb;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned e2 = __shfl_up(e, d);
            if (lane >= d) e += e2;
        }
        if (lane == 63) s_bits[wave] = e;
        __syncthreads();
        unsigned acc = bits + e - cb, btot = 0;
        for (int v = 0; v < 16; ++v) {
            const unsigned sv = s_bits[v];
            if (v < wave) acc += sv;
            btot += sv;
        }
        {
            int pv = prev, idx = o;
            for (unsigned long long tt = t; tt; tt &= tt - 1) {
                const int pos = 64 * k + __ffsll((long long)tt) - 1;
                if (pos > 0) acc += png_run_bits(vals[pv], (unsigned)(pos - pv));
                if (idx <= p.cap) { PngRun r; r.off = 3u + acc; r.start = (unsigned)pos; runs[idx] = r; }
                pv = pos;
                ++idx;
            }
        }
        n_tr += tot;
        last = max(last, tmax);
        bits += btot;
    }
    for (int d = 32; d; d >>= 1) { sa += __shfl_down(sa, d); sb += __shfl_down(sb, d); }
    if (lane == 0) { s_a[wave] = sa; s_b[wave] = sb; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long a = 0, bb = 0;
        for (int v = 0; v < 16; ++v) { a += s_a[v]; bb += s_b[v]; }
        const unsigned v = vals[last], n = (unsigned)(N - last);     // the last run: [last, N)
        const unsigned total = bits + png_run_bits(v, n);
        unsigned long long ta, tb;
        png_adler_terms(v, n, (unsigned long long)last, (unsigned long long)N, &ta, &tb);
        PngHead hd;
        hd.end_bits = 3u + total + 7u;
        hd.adler = png_adler_finish(a + ta, bb + tb, (unsigned long long)N);
        hd.n_runs = (unsigned)n_tr;
        hd.n_bytes = (unsigned)png_stream_bytes((long)hd.end_bits);
        *png_ws_head(ws) = hd;
        if (n_tr <= p.cap) { PngRun r; r.off = 3u + total; r.start = (unsigned)N; runs[n_tr] = r; }
        int *meta = p.meta + 4 * b;
        meta[0] = (int)hd.n_bytes; meta[1] = n_tr; meta[2] = H; meta[3] = W;
    }
}

__global__ __launch_bounds__(256) void png_emit_kernel(const PngParams p) {
    const int b = blockIdx.y;
    if (p.grouped && !((p.lead >> b) & 1)) return;
    unsigned char *ws = p.ws + (size_t)b * png_ws_stride(p.W, p.H, p.cap);
    const PngHead hd = *png_ws_head(ws);
    const long lim = min((long)hd.n_bytes, (long)p.cap);
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    if (4 * w >= lim) return;
    const int nrec = (int)min(hd.n_runs, (unsigned)p.cap);
    const unsigned word = png_word(w, png_ws_runs(ws), nrec, png_ws_vals(ws, p.cap, p.W, p.H), hd);
    unsigned char *o = p.out + (size_t)b * p.cap + 4 * w;
    if (4 * w + 4 <= lim && !((size_t)o & 3)) {
        *(unsigned *)o = word;
    } else {
        for (int j = 0; j < 4; ++j)
            if (4 * w + j < lim) o[j] = (unsigned char)(word >> (8 * j));
    }
}

static bool png_params_ok(const PngParams &p, int B) {
    if (p.W < 1 || p.H < 1 || p.W > PNG_MAX_SIDE || p.H > PNG_MAX_SIDE || p.cap < 1 || p.cap > png_worst_bytes(p.W, p.H)) return false;
    if (!p.ws || !p.out || !p.meta || B < 1) return false;
    if (p.grouped) {
        if (B > PNG_MAX_SLOTS) return false;
        for (int b = 0; b < B; ++b)
            if (p.wh[b][0] < 1 || p.wh[b][1] < 1 || p.wh[b][0] > p.W || p.wh[b][1] > p.H) return false;
    } else if (B > 65535) {
        return false;
    }
    return true;
}

static int launch_png_tail(const PngParams &p, int B, hipStream_t s) {
    hipLaunchKernelGGL(png_scan_kernel, dim3(B), dim3(1024), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    const unsigned nwords = (unsigned)(((long)p.cap + 3) / 4);
    hipLaunchKernelGGL(png_emit_kernel, dim3((nwords + 255) / 256, B), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_png(const PngParams &p, int B, void *stream) {
    if (!png_params_ok(p, B) || p.grouped || !p.planes) return -1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(png_bits_kernel, dim3((unsigned)((png_words(p.W, p.H) + 3) / 4), B), dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    return launch_png_tail(p, B, s);
}

int launch_vos_png_v(const VosRleVParams &v, const PngParams &p, int B, void *stream) {
    if (!png_params_ok(p, B) || !p.grouped || v.n_groups < 1 || v.n_groups > B || v.W != p.W || v.H != p.H) return -1;
    if (!v.logits || v.ms < 1) return -1;
    unsigned seen = 0, given = 0, lead = 0;
    for (int g = 0; g < v.n_groups; ++g) {                            // (the entry has said why; nothing out of range is launched)
        const unsigned m = v.gmask[g];
        if (!m || (m & seen) || (B < 32 && (m >> B))) return -1;
        if (v.gwh[g][0] < 1 || v.gwh[g][1] < 1 || v.gwh[g][0] > v.W || v.gwh[g][1] > v.H) return -1;
        if ((v.given & m) && !v.init[g]) return -1;
        const int b0 = __builtin_ctz(m);
        if (p.wh[b0][0] != v.gwh[g][0] || p.wh[b0][1] != v.gwh[g][1]) return -1;
        seen |= m;
        if ((v.live_groups >> g) & 1) { given |= v.given & m; lead |= 1u << b0; }
    }
    if (((v.given | v.alive) & ~seen) || lead != p.lead) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((png_words(p.W, p.H) + 3) / 4), v.n_groups);
    if (given) {
        if (v.st) hipLaunchKernelGGL((png_bits_labels_v_kernel<true, true>), grid, dim3(256), 0, s, v, p);
        else      hipLaunchKernelGGL((png_bits_labels_v_kernel<false, true>), grid, dim3(256), 0, s, v, p);
    } else {
        if (v.st) hipLaunchKernelGGL((png_bits_labels_v_kernel<true, false>), grid, dim3(256), 0, s, v, p);
        else      hipLaunchKernelGGL((png_bits_labels_v_kernel<false, false>), grid, dim3(256), 0, s, v, p);
    }
    if (hipGetLastError() != hipSuccess) return -4;
    return launch_png_tail(p, B, s);
}

}  // namespace smk
