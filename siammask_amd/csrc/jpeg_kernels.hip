// jpeg_kernels.hip -- baseline JPEG files to BGR frames on the device (jpeg_decode.h has the format and the functions both sides run;
// DESIGN.md 3.24), gfx950.  One call decodes N images of mixed sizes and samplings with one memset and three launches:
//   jpeg_huff    one lane per entropy segment, all segments of all images in one grid (a binary search over the descriptors'
//                running segment counts finds the lane's image).  The lane reads the stuffed bytes straight from the uploaded file,
//                looks its image's tables up in global memory and writes int16 coefficients into the zeroed workspace.  Its status
//                bits reach the image's status word by one atomic OR, only when there are any.  A wave is a block: the lanes are
//                long serial loops of very different lengths, so waves are spread over the chip instead of sharing a CU's barrier.
//   jpeg_idct    eight lanes per 8x8 block, 32 blocks per workgroup: lane j dequantises and transforms column j into LDS, one
//                barrier, then row j, the range limit and one 8-byte store into the component plane (padded block geometry).
//   jpeg_color   one lane per output pixel: luma, the upsampled chroma (jpeg_chroma reads the four samples it needs), the colour
//                conversion, three byte stores at the image's own pointer and pitch.  Lane 0 of an image writes its meta row.
// blockIdx.y is the image in the last two; an image smaller than the largest leaves whole workgroups at once (block-uniform, before
// the barrier).  Nothing outside an image's own h x w x 3 bytes, coefficients and planes is written whatever its bytes are.
#include <hip/hip_runtime.h>

#include "../../include/siammask_hip_test.h"
#include "jpeg_decode.h"

namespace smk {

__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...);       // engine.cpp

__constant__ uint8_t JPEG_ZZ_DEV[64] = SMK_JPEG_ZIGZAG;

__global__ __launch_bounds__(64) void jpeg_huff_kernel(const JpegParams p) {
    __shared__ uint8_t zz[64];
    zz[threadIdx.x] = JPEG_ZZ_DEV[threadIdx.x];
    __syncthreads();
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= p.n_seg) return;
    int lo = 0, hi = p.n_images - 1;                                  // the last image whose first segment is at or before gid
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long)p.desc[(size_t)mid * JPEG_DESC_WORDS + JD_SEG_BASE] <= gid) lo = mid;
        else hi = mid - 1;
    }
    const int32_t *d = p.desc + (size_t)lo * JPEG_DESC_WORDS;
    const long s = gid - d[JD_SEG_BASE];
    if (s < 0 || s >= d[JD_NSEG]) return;
    const JpegGeom g = jpeg_geom(d);
    const uint8_t *file = p.bytes + (size_t)(uint32_t)d[JD_FILE_OFF];
    const int e0 = d[JD_ENT_OFF], e1 = e0 + d[JD_ENT_LEN];
    int a = p.seg[(size_t)d[JD_SEG_OFF] + s], b = s + 1 < d[JD_NSEG] ? p.seg[(size_t)d[JD_SEG_OFF] + s + 1] : e1;
    a = a < e0 ? e0 : a > e1 ? e1 : a;                                // (offsets are clamped into the image's own entropy data)
    b = b < a ? a : b > e1 ? e1 : b;
    const long M = (long)g.mcu_w * g.mcu_h, R = d[JD_RESTART] ? d[JD_RESTART] : M;
    const long m0 = s * R, m1 = m0 + R < M ? m0 + R : M;
    const JpegTables *T = (const JpegTables *)(p.tables + (size_t)(uint32_t)d[JD_TABLE_OFF]);
    const int st = jpeg_decode_segment(file + a, file + b, d, g, T, jpeg_ws_coef(p.ws, p.n_images, d[JD_BLK_BASE]), m0, m1, zz);
    if (st) atomicOr(jpeg_ws_status(p.ws) + lo, st);
}

constexpr int JPEG_IDCT_BLOCKS = 32;                                  // 8x8 blocks per workgroup of 256

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegParams p) {
    __shared__ uint32_t ws[JPEG_IDCT_BLOCKS][8][9];                   // (rows padded to 9 words)
    const int32_t *d = p.desc + (size_t)blockIdx.y * JPEG_DESC_WORDS;
    const JpegGeom g = jpeg_geom(d);
    if ((long)blockIdx.x * JPEG_IDCT_BLOCKS >= g.blocks) return;      // block-uniform
    const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
    const long blk = (long)blockIdx.x * JPEG_IDCT_BLOCKS + lb;
    const bool on = blk < g.blocks;
    const int c = !on ? 0 : blk >= g.blk0(2) && g.ncomp == 3 ? 2 : blk >= g.blk0(1) && g.ncomp == 3 ? 1 : 0;
    uint32_t v[8];
    if (on) {
        const int16_t *co = jpeg_ws_coef(p.ws, p.n_images, d[JD_BLK_BASE]) + blk * 64;
        const JpegTables *T = (const JpegTables *)(p.tables + (size_t)(uint32_t)d[JD_TABLE_OFF]);
        const uint8_t *q = T->q[d[JD_TQ0 + c] & 3];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = jpeg_dequant(co[8 * k + j], q[8 * k + j]);
        jpeg_idct_1d(v, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[lb][k][j] = v[k];
    }
    __syncthreads();
    if (!on) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = ws[lb][j][k];
    jpeg_idct_1d(v, 18);
    const long rel = blk - g.blk0(c);
    const int by = (int)(rel / g.cols(c)), bx = (int)(rel - (long)by * g.cols(c));
    uint8_t *o = jpeg_ws_planes(p.ws, p.n_images, p.n_blocks, d[JD_BLK_BASE]) + g.plane0(c) + ((long)by * 8 + j) * ((long)g.cols(c) * 8) + bx * 8;
    uint2 w;
    w.x = jpeg_range_limit(v[0]) | (jpeg_range_limit(v[1]) << 8) | (jpeg_range_limit(v[2]) << 16) | ((uint32_t)jpeg_range_limit(v[3]) << 24);
    w.y = jpeg_range_limit(v[4]) | (jpeg_range_limit(v[5]) << 8) | (jpeg_range_limit(v[6]) << 16) | ((uint32_t)jpeg_range_limit(v[7]) << 24);
    *(uint2 *)o = w;                                                  // (planes start at a multiple of 64 bytes, rows and blocks at multiples of 8)
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegParams p) {
    const int n = blockIdx.y;
    const int32_t *d = p.desc + (size_t)n * JPEG_DESC_WORDS;
    const JpegGeom g = jpeg_geom(d);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.w * g.h) return;
    const int y = (int)(i / g.w), x = (int)(i - (long)y * g.w);
    uint8_t *out = (uint8_t *)(((uint64_t)(uint32_t)d[JD_OUT_HI] << 32) | (uint32_t)d[JD_OUT_LO]);
    uint8_t px[3];
    jpeg_pixel(jpeg_ws_planes(p.ws, p.n_images, p.n_blocks, d[JD_BLK_BASE]), g, x, y, px);
    uint8_t *o = out + (size_t)y * (size_t)d[JD_PITCH] + 3 * (size_t)x;
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
    if (i == 0) {
        int32_t *m = p.meta + (size_t)n * JPEG_META_WORDS;
        m[0] = jpeg_ws_status(p.ws)[n] | d[JD_STATUS]; m[1] = g.h; m[2] = g.w; m[3] = d[JD_NSEG];
    }
}

static int jpeg_stages = 7;                                           // smk_test_jpeg_stages: a measurement aid, 7 in the product

int launch_jpeg(const JpegParams &p, void *stream) {
    if (!p.bytes || !p.desc || !p.seg || !p.tables || !p.ws || !p.meta) return -1;
    if (p.n_images < 1 || p.n_images > 65535 || p.n_seg < 1 || p.n_blocks < 1 || p.max_blocks < 1 || p.max_pixels < 1) return -1;
    if (p.max_blocks > p.n_blocks || p.max_pixels > (long)JPEG_MAX_SIDE * JPEG_MAX_SIDE) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.ws, 0, p.zero_bytes, s) != hipSuccess) return -4;
    if (jpeg_stages & 1) hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)((p.n_seg + 63) / 64)), dim3(64), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    if (jpeg_stages & 2)
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((p.max_blocks + JPEG_IDCT_BLOCKS - 1) / JPEG_IDCT_BLOCKS), p.n_images), dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    if (jpeg_stages & 4) hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((p.max_pixels + 255) / 256), p.n_images), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk

using namespace smk;

extern "C" int smk_test_jpeg_stages(int mask) {
    if (mask < 0 || mask > 7) return fail(SMK_E_ARG, "smk_test_jpeg_stages: mask %d (0..7)", mask);
    jpeg_stages = mask;
    return 0;
}

extern "C" int smk_jpeg_decode(const uint8_t *bytes_dev, size_t bytes_len, const int32_t *desc, const int32_t *desc_dev, const int32_t *seg_dev,
                               size_t n_seg, const void *tables_dev, size_t tables_len, int n_images, void *ws_dev, size_t ws_bytes,
                               int32_t *meta_out_dev, void *stream) {
    if (!bytes_dev || !desc || !desc_dev || !seg_dev || !tables_dev || !ws_dev || !meta_out_dev) return fail(SMK_E_ARG, "smk_jpeg_decode: null argument");
    if (n_images < 1 || n_images > 65535) return fail(SMK_E_ARG, "smk_jpeg_decode: n_images %d (1..65535)", n_images);
    if (((uintptr_t)ws_dev & 255) || ((uintptr_t)meta_out_dev & 3) || ((uintptr_t)desc_dev & 3) || ((uintptr_t)seg_dev & 3) || ((uintptr_t)tables_dev & 3))
        return fail(SMK_E_ARG, "smk_jpeg_decode: ws_dev must be 256-byte aligned, descriptors, segment offsets, tables and meta 4-byte aligned");
    JpegParams p;
    p.bytes = bytes_dev; p.desc = desc_dev; p.seg = seg_dev; p.tables = (const uint8_t *)tables_dev; p.ws = (unsigned char *)ws_dev;
    p.meta = meta_out_dev; p.n_images = n_images;
    long segs = 0, blocks = 0, max_blocks = 0, max_pixels = 0;
    for (int n = 0; n < n_images; ++n) {
        const int32_t *d = desc + (size_t)n * JPEG_DESC_WORDS;
        if (!jpeg_desc_ok(d)) return fail(SMK_E_ARG, "smk_jpeg_decode: image %d: the descriptor's format columns are out of range", n);
        const JpegGeom g = jpeg_geom(d);
        if (d[JD_SEG_BASE] != segs || d[JD_SEG_OFF] != segs || d[JD_BLK_BASE] != blocks)
            return fail(SMK_E_ARG, "smk_jpeg_decode: image %d: the batch columns are not those smk_jpeg_workspace wrote", n);
        if (d[JD_FILE_OFF] < 0 || d[JD_FILE_LEN] < 0 || (size_t)d[JD_FILE_OFF] + (size_t)d[JD_FILE_LEN] > bytes_len ||
            (long)d[JD_ENT_OFF] + d[JD_ENT_LEN] > d[JD_FILE_LEN])
            return fail(SMK_E_ARG, "smk_jpeg_decode: image %d: the file or its entropy data lie outside the %zu bytes", n, bytes_len);
        if (d[JD_TABLE_OFF] < 0 || (d[JD_TABLE_OFF] & 3) || (size_t)d[JD_TABLE_OFF] + sizeof(JpegTables) > tables_len)
            return fail(SMK_E_ARG, "smk_jpeg_decode: image %d: its tables lie outside the %zu table bytes", n, tables_len);
        if (!(d[JD_OUT_LO] | d[JD_OUT_HI]) || d[JD_PITCH] < 3 * d[JD_W])
            return fail(SMK_E_ARG, "smk_jpeg_decode: image %d: a null output or fewer than 3 w bytes between rows", n);
        segs += d[JD_NSEG];
        blocks += g.blocks;
        if (segs > 0x7fffffffL || blocks > 0x7fffffffL) return fail(SMK_E_ARG, "smk_jpeg_decode: too many segments or blocks in one call");
        max_blocks = g.blocks > max_blocks ? g.blocks : max_blocks;
        max_pixels = (long)g.w * g.h > max_pixels ? (long)g.w * g.h : max_pixels;
    }
    if ((size_t)segs > n_seg) return fail(SMK_E_ARG, "smk_jpeg_decode: %ld segments, the segment table holds %zu", segs, n_seg);
    if (ws_bytes < jpeg_ws_bytes(n_images, blocks))
        return fail(SMK_E_ARG, "smk_jpeg_decode: workspace of %zu bytes, %zu needed", ws_bytes, jpeg_ws_bytes(n_images, blocks));
    p.n_seg = segs; p.n_blocks = blocks; p.max_blocks = max_blocks; p.max_pixels = max_pixels;
    p.zero_bytes = jpeg_ws_status_bytes(n_images) + (size_t)blocks * 128;
    if (launch_jpeg(p, stream)) return fail(SMK_E_HIP, "jpeg_decode launch failed");
    return 0;
}
