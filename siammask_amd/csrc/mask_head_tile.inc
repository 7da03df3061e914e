// mask_head_tile.inc -- the 63x63 mask head (1x1, 256 -> N <= 4096 channels + bias, fp16 in, [B][N][Ho][Wo] f32 NCHW out) as
// C^T = W x A^T with the pixels stationary.  Included by conv_igemm.hip; run by a 1024-thread workgroup (sixteen waves): the mask
// half of chain_mask_kernel and mask_head_kernel.
//
// Against conv_igemm_body<f16, 2, 2, 1, 128, OUT_NCHW_F32, 2> (one 128 x 128 tile per body: both operands through an LDS ring for a
// K loop of four tiles, the accumulators through LDS again for the transposed store, a barrier in between) a tile's lifetime loses
// its steps:
//   * the 128 pixels x 256 channels of a workgroup are staged ONCE (64 KB of LDS, 16-byte slot c of row r at slot c ^ (r & 31): the
//     lane groups of a ds_read_b128 fragment read hit sixteen different slots) and serve every channel block the workgroup owns;
//   * the weights come from the layer's fragment-order pack (ConvParams::wgt_frag) straight into registers, eight k-steps ahead
//     (a ring of eight fragments that wraps into the wave's next channel block, so the next block's first half is in flight
//     under this block's stores);
//   * with the weight fragment as the MFMA's FIRST operand a register of the 32 x 32 accumulator is 32 consecutive pixels of one
//     channel across lanes 0-31 and of a second channel (+ 4) across lanes 32-63: the stores leave from the accumulators, two
//     128-byte runs of two channel planes per instruction, per-lane addresses (runs may straddle an image boundary).  No LDS
//     staging of the output, no barrier behind the K loop.
// Arithmetic: v_mfma_f32_32x32x16_f16, k-steps 0..15 ascending from a zero accumulator, lane half h holding k = 16 s + 8 h + j,
// then + bias in fp32 -- the products and their order of the generic instantiation with the operands swapped, so the logits are
// bit-identical (the bias is NOT folded into the accumulator's start value: that would change the rounding).
//
// Work split: workgroup wg = (pixel tile wg / nsplit, channel-block range wg % nsplit of ceil(N / 32) blocks, split evenly);
// wave w computes the 64-pixel half w & 1 of the blocks c0 + (w >> 1) + 8 i: a unit = 32 channels x 64 pixels = 32 MFMAs and 32
// stores.  VGPRs: 32 accumulators + 32 ring + 16 pixel fragments + addresses (the launch bound of 1024 threads allows 128).

constexpr int MH_PX = 128;                     // pixels per workgroup
constexpr int MH_K = 256;                      // input channels (= K)
constexpr int MH_ROW = MH_K * 2;               // bytes of a staged pixel row
constexpr int MH_KS = MH_K / 16;               // k-steps
constexpr int MH_RING = 8;                     // weight fragments in flight per wave
constexpr int MH_NMAX = 4096;                  // output channels the bias stage is sized for
constexpr int MH_A_BYTES = MH_PX * MH_ROW;     // 64 KB
constexpr int MH_LDS = MH_A_BYTES + MH_NMAX * 4;

typedef unsigned mh_uint4 __attribute__((ext_vector_type(4)));

// The 32 stores of a unit through a buffer resource on the output: the lane's pixel is the (32-bit) vector offset, the channel
// plane the scalar one, so no per-store 64-bit address lives in registers; a lane whose pixel is beyond M carries the
// out-of-range offset and the hardware's range check drops its store (no branch).  NT: streaming stores (ConvParams::nt_store);
// TAIL: the block holds channels >= N (the last block when N % 32 != 0): those lanes get the out-of-range offset per store.
template <bool NT, bool TAIL>
__device__ __forceinline__ void mask_head_store(const floatx16 (&acc)[2], const float *sbias, const __amdgpu_buffer_rsrc_t rs_out,
                                                const int (&opix)[2], const int ch0, const int chs, const int N, const int hw4) {
    constexpr int OOB = 0x7fff0000;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const floatx4 b4 = *(const floatx4 *)(sbias + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e, dch = 8 * g + e;      // register r of a lane: channel ch0 + (r & 3) + 8 (r >> 2)
            const bool live = !TAIL || ch0 + dch < N;
            // (a plane past the tensor for both lane halves: no scalar offset either, whichever way the range check counts it)
            const int plane = (!TAIL || chs + dch < N) ? (chs + dch) * hw4 : 0;
#pragma unroll
            for (int q = 0; q < 2; ++q)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[q][r] + b4[e]), rs_out, live ? opix[q] : OOB, plane, NT ? 2 : 0);
        }
    }
}

__device__ __forceinline__ void mask_head_tile(const ConvParams &p, const int wg, const int nsplit, unsigned char *smem) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pt = wg / nsplit, ns = wg - pt * nsplit;
    const int m0 = pt * MH_PX;
    const int nblk = (p.N + 31) >> 5;
    const int c0 = (int)((long)ns * nblk / nsplit), c1 = (int)((long)(ns + 1) * nblk / nsplit);
    const int half = wave & 1;
    const int cbf = c0 + (wave >> 1);                                  // this wave's first channel block

    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void *)p.wgt_frag, 0, p.w_bytes, 0x00020000);
    constexpr int OOB = 0x7fff0000;                                    // beyond every extent (the launcher checks): the range check returns zeros, no traffic
    auto w_off = [&](int cb) { return cb < c1 ? (cb * MH_KS * 64 + lane) * 16 : OOB; };
    auto load_w = [&](int off, int s) {
        return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, off + s * 1024, 0, 0));
    };
    half8 wf[MH_RING];
    {
        const int off = w_off(cbf);
#pragma unroll
        for (int s = 0; s < MH_RING; ++s) wf[s] = load_w(off, s);
    }

    // ---- the pixel tile and the bias of the workgroup's channel range -> LDS ----
    {
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void *)p.in, 0, p.in_bytes, 0x00020000);
        constexpr int NLD = MH_PX * (MH_ROW / 16) / 1024;              // 4 pieces of 16 bytes per thread
        mh_uint4 v[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int g = i * 1024 + tid, r = g >> 5, c = g & 31;
            const int m = m0 + r;                                      // 1x1, stride 1, no padding: output pixel m IS input pixel m
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, m < p.M ? (m * p.Cs + p.cin_off) * 2 + c * 16 : OOB, 0, 0);
        }
        float *sb = (float *)(smem + MH_A_BYTES);
        for (int i = tid; i < (c1 - c0) * 32; i += 1024) sb[i] = p.bias[c0 * 32 + i];      // (the pack pads the bias to whole blocks)
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int g = i * 1024 + tid, r = g >> 5, c = g & 31;
            *(mh_uint4 *)(smem + r * MH_ROW + ((c ^ (r & 31)) << 4)) = v[i];
        }
    }
    __syncthreads();
    if (cbf >= c1) return;                                             // (fewer blocks than wave pairs)

    const int fr = lane & 31, fh = lane >> 5;
    // fragment of k-step s, pixel row 64 half + 32 q + fr: slot (2 s + fh) ^ fr = (2 s) ^ (fh ^ fr)
    const int aoff = (64 * half + fr) * MH_ROW + ((fh ^ fr) << 4);
    // this lane's two pixels (q = 0, 1) in the NCHW tensor, at channel 4 fh of block 0: byte offsets (the launcher keeps the tensor
    // below the out-of-range offset)
    const int hw = p.Ho * p.Wo;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.M * p.N * 4, 0x00020000);
    int opix[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int m = m0 + 64 * half + 32 * q + fr;
        const int b = m / hw, pos = m - b * hw;
        opix[q] = m < p.M ? ((b * p.N + 4 * fh) * hw + pos) * 4 : OOB;
    }
    const float *sbias = (const float *)(smem + MH_A_BYTES) + 4 * fh;
    const bool nt = p.nt_store != 0;

    for (int cb = cbf; cb < c1; cb += 8) {
        const int offc = w_off(cb), offn = w_off(cb + 8);
        floatx16 acc[2];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        // issue order of a k-step, pinned (left alone the scheduler hoists the sixteen steps' LDS reads and spills): the pixel
        // fragments of step s + 1, the two MFMAs of step s, the refill of the weight slot they freed
        half8 a[2][2];
        a[0][0] = *(const half8 *)(smem + aoff);
        a[0][1] = *(const half8 *)(smem + aoff + 32 * MH_ROW);
#pragma unroll
        for (int s = 0; s < MH_KS; ++s) {
            if (s + 1 < MH_KS) {
                const unsigned char *ap = smem + (aoff ^ ((s + 1) << 5));
                a[(s + 1) & 1][0] = *(const half8 *)ap;
                a[(s + 1) & 1][1] = *(const half8 *)(ap + 32 * MH_ROW);
            }
            __builtin_amdgcn_sched_barrier(0);
            const half8 w = wf[s & (MH_RING - 1)];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w, a[s & 1][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w, a[s & 1][1], acc[1], 0, 0, 0);
            // refill the slot: this block's second half, then the first half of the wave's next block (none: zeros, never used)
            wf[s & (MH_RING - 1)] = s < MH_RING ? load_w(offc, s + MH_RING) : load_w(offn, s - MH_RING);
            __builtin_amdgcn_sched_barrier(0);
        }
        const int ch0 = cb * 32 + 4 * fh;
        const float *sbc = sbias + (cb - c0) * 32;
        if (cb * 32 + 32 <= p.N) {
            if (nt) mask_head_store<true, false>(acc, sbc, rs_out, opix, ch0, cb * 32, p.N, hw * 4);
            else mask_head_store<false, false>(acc, sbc, rs_out, opix, ch0, cb * 32, p.N, hw * 4);
        } else {
            if (nt) mask_head_store<true, true>(acc, sbc, rs_out, opix, ch0, cb * 32, p.N, hw * 4);
            else mask_head_store<false, true>(acc, sbc, rs_out, opix, ch0, cb * 32, p.N, hw * 4);
        }
    }
}
