// tracker_init.hip -- starting a stream of the tracker on the device (gfx950): what tools/test.py does on the host between "an
// annotation / a rectangle" and "the stream is planned for its next frame" -- cv2.boundingRect(labels == id) (:494), np.mean(im,
// axis=(0, 1)) (:146), siamese_init's exemplar window (:147-152) -- as launches on one stream with no host read-back
// (DESIGN.md 3.10 / 4.3).  Two one-pass reductions over a frame and one lane-per-stream scalar kernel; the scalar arithmetic is
// tracker_state.h (shared with the host test entry), the exemplar crop is image_kernels.hip's (beside crop_pixel).
#include <hip/hip_runtime.h>
#include "tracker_state.h"

namespace smk {

// ------------------------------------------------------------------------------------------
// label_rects: the bounding rectangles of up to 32 object ids in one pass over a uint8 label map.  A workgroup covers 256 pixels
// of RECT_ROWS consecutive rows (one byte per lane, coalesced along x).  A 256-bit table in LDS says which byte values are asked
// for: a wave whose 64 pixels match nothing (the background of an annotation) does one ballot and moves on.  Otherwise the wave
// groups its matching lanes by value with ballots, as vos_score_kernel does; the lanes of a wave are consecutive x of one row, so a
// group's extent is its lowest / highest set lane, and lane 0 folds it into the workgroup's LDS accumulators.  Per (workgroup,
// object present in it) four global integer atomicMax follow; integer max is order-independent, the result is exact.
// Accumulators (all zero-initialised, all max): BIG - min x, BIG - min y, max x + 1, max y + 1 -- zero means "absent";
// label_rects_finish_kernel turns them into (x, y, w, h) in place.
constexpr int RECT_BIG = 1 << 30;

__global__ __launch_bounds__(256) void label_rects_kernel(const LabelRectsParams p) {
    __shared__ int acc[RECT_MAX_OBJ * 4];
    __shared__ int sid[RECT_MAX_OBJ];
    __shared__ unsigned asked[8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int O = p.n_obj;
    if (tid < RECT_MAX_OBJ * 4) acc[tid] = 0;
    if (tid < 8) asked[tid] = 0;
    __syncthreads();
    if (tid < O) {
        sid[tid] = p.ids[tid];
        atomicOr(&asked[p.ids[tid] >> 5], 1u << (p.ids[tid] & 31));
    }
    __syncthreads();
    const int x = blockIdx.x * 256 + tid, x_wave = x - lane;
    const bool in_x = x < p.W;
    const int y0 = blockIdx.y * RECT_ROWS, y1 = min(y0 + RECT_ROWS, p.H);
    for (int y = y0; y < y1; ++y) {
        int g = -1;
        bool hit = false;
        if (in_x) {
            g = p.labels[(size_t)y * p.W + x];
            hit = (asked[g >> 5] >> (g & 31)) & 1;
        }
        unsigned long long todo = __ballot(hit);
        while (todo) {
            const int gg = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((long long)todo) - 1));
            const unsigned long long m = __ballot(hit && g == gg);
            todo &= ~m;
            if (lane == 0) {
                const int lo = x_wave + __ffsll((long long)m) - 1, hi = x_wave + 63 - __clzll((long long)m);
                for (int j = 0; j < O; ++j) {
                    if (sid[j] != gg) continue;                           // (duplicate ids each get the rectangle)
                    atomicMax(&acc[4 * j], RECT_BIG - lo);
                    atomicMax(&acc[4 * j + 1], RECT_BIG - y);
                    atomicMax(&acc[4 * j + 2], hi + 1);
                    atomicMax(&acc[4 * j + 3], y + 1);
                }
            }
        }
    }
    __syncthreads();
    if (tid < 4 * O) {
        const int v = acc[tid];
        if (v) atomicMax(p.rects + tid, v);
    }
}

__global__ __launch_bounds__(64) void label_rects_finish_kernel(int *rects, int n_obj) {
    const int o = threadIdx.x;
    if (o >= n_obj) return;
    int *r = rects + 4 * o;
    const int a0 = r[0], a1 = r[1], a2 = r[2], a3 = r[3];
    if (a2 == 0) return;                                                  // absent: (0, 0, 0, 0) as the memset left it
    const int x = RECT_BIG - a0, y = RECT_BIG - a1;
    r[0] = x; r[1] = y; r[2] = a2 - x; r[3] = a3 - y;                     // max x - min x + 1, max y - min y + 1
}

int launch_label_rects(const LabelRectsParams &p, void *stream) {
    if (p.n_obj < 1 || p.n_obj > RECT_MAX_OBJ || !p.labels || !p.rects) return -1;
    if (p.W < 1 || p.H < 1 || p.W > 32768 || p.H > 32768) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.rects, 0, sizeof(int) * 4 * p.n_obj, s) != hipSuccess) return -4;
    dim3 grid((p.W + 255) / 256, (p.H + RECT_ROWS - 1) / RECT_ROWS, 1);
    hipLaunchKernelGGL(label_rects_kernel, grid, dim3(256), 0, s, p);
    hipLaunchKernelGGL(label_rects_finish_kernel, dim3(1), dim3(64), 0, s, p.rects, p.n_obj);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ------------------------------------------------------------------------------------------
// frame_sums: per-channel integer sums of n uint8 frames [H][W][3] -> uint64 [n][3].  A frame is `bytes` = H * W * 3 consecutive
// bytes; byte i belongs to channel i % 3.  The 16-byte aligned body is read as uint4 in a grid-stride loop (blockIdx.y = frame);
// the up to 15 bytes before and after it are read one per lane by the first workgroup.  A lane sums into three 32-bit counters
// indexed by (byte position in the chunk) % 3 and rotates them by the chunk's phase with selects (no dynamic register index ->
// no scratch); a chunk adds at most 6 * 255 to a counter and the launcher bounds the chunks per lane, so they cannot wrap.
// Then a 64-bit shuffle reduction per wave, LDS across the four waves, one 64-bit atomic add per workgroup and channel.
constexpr int SUMS_CHUNKS_PER_LANE = 16, SUMS_MAX_BLOCKS = 4096;

__device__ __forceinline__ void sums_add_word(unsigned v, unsigned &t0, unsigned &t1, unsigned &t2) {
    // the four bytes of a little-endian word at chunk position 4 * k: the caller passes the counters rotated by 4 * k % 3
    t0 += v & 255u;
    t1 += (v >> 8) & 255u;
    t2 += (v >> 16) & 255u;
    t0 += v >> 24;
}

__global__ __launch_bounds__(256) void frame_sums_kernel(const FrameSumsParams p) {
    __shared__ unsigned long long part[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char *f = p.frames + (size_t)blockIdx.y * p.stride;
    const long head = min((long)((16 - ((size_t)f & 15)) & 15), p.bytes);
    const long n_chunk = (p.bytes - head) / 16;
    const long tail0 = head + 16 * n_chunk;                               // first byte behind the body
    unsigned c0 = 0, c1 = 0, c2 = 0;                                      // per channel
    const uint4 *body = (const uint4 *)(f + head);
    for (long i = (long)blockIdx.x * 256 + tid; i < n_chunk; i += (long)gridDim.x * 256) {
        const uint4 v = body[i];
        unsigned t0 = 0, t1 = 0, t2 = 0;                                  // indexed by (position in the chunk) % 3
        sums_add_word(v.x, t0, t1, t2);                                   // positions 0..3
        sums_add_word(v.y, t1, t2, t0);                                   // 4..7   (4 % 3 == 1)
        sums_add_word(v.z, t2, t0, t1);                                   // 8..11  (8 % 3 == 2)
        sums_add_word(v.w, t0, t1, t2);                                   // 12..15 (12 % 3 == 0)
        const int ph = (int)((head + 16 * i) % 3);                        // channel of position 0
        c0 += ph == 0 ? t0 : (ph == 1 ? t2 : t1);                         // channel c holds t[(c - ph) mod 3]
        c1 += ph == 0 ? t1 : (ph == 1 ? t0 : t2);
        c2 += ph == 0 ? t2 : (ph == 1 ? t1 : t0);
    }
    if (blockIdx.x == 0 && tid < 32) {                                    // lanes 0..15: the head, 16..31: the tail
        const long i = tid < 16 ? (long)tid : tail0 + (tid - 16);
        const bool on = tid < 16 ? (long)tid < head : i < p.bytes;
        if (on) {
            const unsigned v = f[i];
            const int ch = (int)(i % 3);
            c0 += ch == 0 ? v : 0u;
            c1 += ch == 1 ? v : 0u;
            c2 += ch == 2 ? v : 0u;
        }
    }
    unsigned long long s0 = c0, s1 = c1, s2 = c2;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s0 += __shfl_down(s0, d);
        s1 += __shfl_down(s1, d);
        s2 += __shfl_down(s2, d);
    }
    if (lane == 0) { part[wave][0] = s0; part[wave][1] = s1; part[wave][2] = s2; }
    __syncthreads();
    if (tid < 3) {
        const unsigned long long v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (v) atomicAdd(p.sums + 3 * (size_t)blockIdx.y + tid, v);
    }
}

int launch_frame_sums(const FrameSumsParams &p, void *stream) {
    if (!p.frames || !p.sums || p.n < 1 || p.n > 65535 || p.bytes < 3 || p.stride < 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.sums, 0, sizeof(unsigned long long) * 3 * p.n, s) != hipSuccess) return -4;
    const long per_block = 256L * SUMS_CHUNKS_PER_LANE;
    long blocks = (p.bytes / 16 + per_block - 1) / per_block;
    blocks = blocks < 1 ? 1 : (blocks > SUMS_MAX_BLOCKS ? SUMS_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(frame_sums_kernel, dim3((unsigned)blocks, p.n, 1), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ------------------------------------------------------------------------------------------
// frame_sums_v: the same sums for n frames of DIFFERENT sizes and row pitches (one smk_image_ref each, in the kernarg) in one
// launch.  A pitched frame is not one run of bytes, so the unit is the row: blockIdx.y = frame, a WAVE takes a row (the rows of
// a frame are dealt round-robin to the waves of its workgroups), the channel phase restarts with every row.  Per row: the up
// to 15 bytes in front of the first 16-byte aligned address and behind the last one are read one per lane (lanes 0..15 / 16..31),
// the aligned body as uint4, one chunk per lane and turn, summed and rotated as above.  The 32-bit counters are folded into the
// lane's 64-bit sums after every row -- a row of 32768 pixels gives a lane at most 97 chunks of 6 * 255 -- so nothing can wrap
// at any size.  Reduction and output as frame_sums_kernel: shuffles, LDS, one 64-bit atomic add per workgroup and channel.
constexpr int SUMS_V_ROWS_PER_WAVE = 8, SUMS_V_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void frame_sums_v_kernel(const FrameSumsVParams p) {
    __shared__ unsigned long long part[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const smk_image_ref &im = p.im[blockIdx.y];
    const int h = im.h;
    const long row_len = 3L * im.w;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    for (int y = blockIdx.x * 4 + wave; y < h; y += gridDim.x * 4) {
        const unsigned char *f = im.data + (size_t)y * im.row_bytes;
        const long head = min((long)((16 - ((size_t)f & 15)) & 15), row_len);
        const long n_chunk = (row_len - head) / 16;
        const long tail0 = head + 16 * n_chunk;
        unsigned c0 = 0, c1 = 0, c2 = 0;
        const uint4 *body = (const uint4 *)(f + head);
        for (long i = lane; i < n_chunk; i += 64) {
            const uint4 v = body[i];
            unsigned t0 = 0, t1 = 0, t2 = 0;
            sums_add_word(v.x, t0, t1, t2);
            sums_add_word(v.y, t1, t2, t0);
            sums_add_word(v.z, t2, t0, t1);
            sums_add_word(v.w, t0, t1, t2);
            const int ph = (int)((head + 16 * i) % 3);                    // channel of position 0 (a row starts at channel 0)
            c0 += ph == 0 ? t0 : (ph == 1 ? t2 : t1);
            c1 += ph == 0 ? t1 : (ph == 1 ? t0 : t2);
            c2 += ph == 0 ? t2 : (ph == 1 ? t1 : t0);
        }
        if (lane < 32) {
            const long i = lane < 16 ? (long)lane : tail0 + (lane - 16);
            const bool on = lane < 16 ? (long)lane < head : i < row_len;
            if (on) {
                const unsigned v = f[i];
                const int ch = (int)(i % 3);
                c0 += ch == 0 ? v : 0u;
                c1 += ch == 1 ? v : 0u;
                c2 += ch == 2 ? v : 0u;
            }
        }
        s0 += c0; s1 += c1; s2 += c2;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s0 += __shfl_down(s0, d);
        s1 += __shfl_down(s1, d);
        s2 += __shfl_down(s2, d);
    }
    if (lane == 0) { part[wave][0] = s0; part[wave][1] = s1; part[wave][2] = s2; }
    __syncthreads();
    if (tid < 3) {
        const unsigned long long v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (v) atomicAdd(p.sums + 3 * (size_t)blockIdx.y + tid, v);
    }
}

int launch_frame_sums_v(const FrameSumsVParams &p, void *stream) {
    if (!p.sums || p.n < 1 || p.n > TRK_SET_MAX_B || p.max_h < 1) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.sums, 0, sizeof(unsigned long long) * 3 * p.n, s) != hipSuccess) return -4;
    const int per_block = 4 * SUMS_V_ROWS_PER_WAVE;
    int blocks = (p.max_h + per_block - 1) / per_block;
    blocks = blocks > SUMS_V_MAX_BLOCKS ? SUMS_V_MAX_BLOCKS : blocks;
    hipLaunchKernelGGL(frame_sums_v_kernel, dim3((unsigned)blocks, p.n, 1), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ------------------------------------------------------------------------------------------
// trk_start: one lane per stream; the streams outside `mask` are not touched
__global__ __launch_bounds__(64) void trk_start_kernel(smk_trk_stream *st, double *twh, const TrkStartArgs a) {
    const int b = threadIdx.x;
    if (b >= a.B || !((a.mask >> b) & 1)) return;
    double px, py, w, h;
    if (a.rects) {
        const int *r = a.rects + 4 * b;
        w = (double)r[2]; h = (double)r[3];
        px = t_rect_centre(r[0], r[2]); py = t_rect_centre(r[1], r[3]);
    } else {
        px = a.pos[b][0]; py = a.pos[b][1];
        w = a.sz[b][0]; h = a.sz[b][1];
    }
    double wh[2];
    if (trk_start(st[b], a.cfg, px, py, w, h, a.sums + 3 * (size_t)b * a.sums_stride, a.im_w, a.im_h, a.win + 3 * b,
                  a.res + TRK_START_ROW * b, wh)) {
        twh[2 * b] = wh[0];
        twh[2 * b + 1] = wh[1];
    }
}

// smk_trk_start_v: the same lane with the size of stream b's own frame.  (A kernel of its own and not a shared body: with one,
// the compiler schedules trk_start_kernel differently, and the existing kernels keep their instructions.)
__global__ __launch_bounds__(64) void trk_start_v_kernel(smk_trk_stream *st, double *twh, const TrkStartVArgs v) {
    const int b = threadIdx.x;
    const TrkStartArgs &a = v.a;
    if (b >= a.B || !((a.mask >> b) & 1)) return;
    double px, py, w, h;
    if (a.rects) {
        const int *r = a.rects + 4 * b;
        w = (double)r[2]; h = (double)r[3];
        px = t_rect_centre(r[0], r[2]); py = t_rect_centre(r[1], r[3]);
    } else {
        px = a.pos[b][0]; py = a.pos[b][1];
        w = a.sz[b][0]; h = a.sz[b][1];
    }
    double wh[2];
    if (trk_start(st[b], a.cfg, px, py, w, h, a.sums + 3 * (size_t)b * a.sums_stride, v.im_wh[b][0], v.im_wh[b][1], a.win + 3 * b,
                  a.res + TRK_START_ROW * b, wh)) {
        twh[2 * b] = wh[0];
        twh[2 * b + 1] = wh[1];
    }
}

int launch_trk_start(smk_trk_stream *st, double *twh, const TrkStartArgs &a, void *stream) {
    if (a.B < 1 || a.B > TRK_SET_MAX_B || !st || !twh || !a.sums || !a.win || !a.res) return -1;
    hipLaunchKernelGGL(trk_start_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st, twh, a);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_trk_start_v(smk_trk_stream *st, double *twh, const TrkStartVArgs &v, void *stream) {
    if (v.a.B < 1 || v.a.B > TRK_SET_MAX_B || !st || !twh || !v.a.sums || !v.a.win || !v.a.res) return -1;
    hipLaunchKernelGGL(trk_start_v_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st, twh, v);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk
