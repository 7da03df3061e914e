// warped_prob.h -- the warped probability of the paste-back (tools/test.py:257-284), shared by the kernels of image_kernels.hip and
// png_kernels.hip: one definition, so every kernel that thresholds or fuses it sees the same bits.
#ifndef SMK_WARPED_PROB_H
#define SMK_WARPED_PROB_H

#include <hip/hip_runtime.h>

namespace smk {

// ------------------------------------------------------------------------------------------
// warped probability of stream b at frame pixel (x, y): WarpAffineInvoker + remapBilinear<float>
// M: the stream's inverse map; lg / ls: its logits and their element stride (1, or S * S for a column of the mask head)
template <class P>
__device__ __forceinline__ float warped_prob(const P &p, const double *M, const float *lg, int ls, int x, int y) {
    constexpr int AB_BITS = 10, INTER_BITS = 5, TAB = 1 << INTER_BITS;
    constexpr double AB_SCALE = 1024.0;
    // X = (X0(y) + adelta(x)) >> (AB_BITS - INTER_BITS), round_delta = AB_SCALE / TAB / 2 = 16
    const long adelta = (long)__builtin_rint(__dmul_rn(__dmul_rn(M[0], (double)x), AB_SCALE));
    const long bdelta = (long)__builtin_rint(__dmul_rn(__dmul_rn(M[3], (double)x), AB_SCALE));
    const long X0 = (long)__builtin_rint(__dmul_rn(__dadd_rn(__dmul_rn(M[1], (double)y), M[2]), AB_SCALE)) + 16;
    const long Y0 = (long)__builtin_rint(__dmul_rn(__dadd_rn(__dmul_rn(M[4], (double)y), M[5]), AB_SCALE)) + 16;
    const long X = (X0 + adelta) >> (AB_BITS - INTER_BITS), Y = (Y0 + bdelta) >> (AB_BITS - INTER_BITS);
    long sxl = X >> INTER_BITS, syl = Y >> INTER_BITS;
    sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);      // saturate_cast<short>
    syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
    const int sx = (int)sxl, sy = (int)syl;
    const float fx = __fmul_rn((float)(X & (TAB - 1)), 1.f / TAB), fy = __fmul_rn((float)(Y & (TAB - 1)), 1.f / TAB);
    const float w00 = __fmul_rn(__fsub_rn(1.f, fy), __fsub_rn(1.f, fx)), w01 = __fmul_rn(__fsub_rn(1.f, fy), fx);
    const float w10 = __fmul_rn(fy, __fsub_rn(1.f, fx)), w11 = __fmul_rn(fy, fx);
    auto tap = [&](int yy, int xx) -> float {
        if ((unsigned)yy < (unsigned)p.ms && (unsigned)xx < (unsigned)p.ms) {
            const float v = lg[(yy * p.ms + xx) * ls];
            return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-v)));        // .sigmoid() (tools/test.py:256)
        }
        return p.border;
    };
    // remapBilinear<float>: sum of four float products, left to right
    float v = __fmul_rn(tap(sy, sx), w00);
    v = __fadd_rn(v, __fmul_rn(tap(sy, sx + 1), w01));
    v = __fadd_rn(v, __fmul_rn(tap(sy + 1, sx), w10));
    v = __fadd_rn(v, __fmul_rn(tap(sy + 1, sx + 1), w11));
    return v;
}

}  // namespace smk
#endif
