// chain_rows.h -- the row bands of the split Refine chain: ONE piece of arithmetic for the device code (refine_chain_body.inc), the
// launchers and the host entry smk_host_chain_rows, which lets the CPU tests pin what the device runs.
//
// A stream's chain runs on S workgroups (S = 1, 2, 4).  Every workgroup computes deconv-input .. h1.2 completely; of the four fine
// layers -- post1 (61x61 through the 31 -> 61 upsampling), h0.0, h0.2 (61x61) and post2 (127x127 through 61 -> 127) -- band s
// computes the output rows [y0, y1) below: its share of post2's 127 rows, and for each earlier layer the rows the next layer's
// range reads (the +-1 taps clipped to the image; through the row table of the upsampling, (iy * 61) / 127, for post2).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMK_CHAIN_HD __host__ __device__ inline
#else
#define SMK_CHAIN_HD inline
#endif

namespace smk {

constexpr int CHAIN_H_FINE = 127, CHAIN_H_MID = 61;      // post2's output / post1, h0.0, h0.2's

struct ChainRows {
    int post1[2], h00[2], h02[2], post2[2];              // [y0, y1) of each layer's OUTPUT rows
};

SMK_CHAIN_HD constexpr bool chain_split_valid(int S) { return S == 1 || S == 2 || S == 4; }

SMK_CHAIN_HD constexpr ChainRows chain_rows(int S, int s) {
    ChainRows r{};
    r.post2[0] = s * CHAIN_H_FINE / S;
    r.post2[1] = (s + 1) * CHAIN_H_FINE / S;
    // post2's taps read upsampled rows y0 - 1 .. y1 (clipped): source rows (iy * 61) / 127, monotonic in iy
    const int lo = r.post2[0] > 0 ? r.post2[0] - 1 : 0;
    const int hi = r.post2[1] < CHAIN_H_FINE ? r.post2[1] : CHAIN_H_FINE - 1;
    r.h02[0] = lo * CHAIN_H_MID / CHAIN_H_FINE;
    r.h02[1] = hi * CHAIN_H_MID / CHAIN_H_FINE + 1;
    r.h00[0] = r.h02[0] > 0 ? r.h02[0] - 1 : 0;
    r.h00[1] = r.h02[1] < CHAIN_H_MID ? r.h02[1] + 1 : CHAIN_H_MID;
    r.post1[0] = r.h00[0] > 0 ? r.h00[0] - 1 : 0;
    r.post1[1] = r.h00[1] < CHAIN_H_MID ? r.h00[1] + 1 : CHAIN_H_MID;
    return r;
}

// Workgroups per stream: four while the launch's B * 4 chain workgroups fit one round of the chip's CUs beside whatever else the
// launch carries (`cus` = the CUs the chain may count on), else two, else the unsplit form.  forced = smk_tune "chain_split".
SMK_CHAIN_HD constexpr int chain_split_rule(int B, int cus, int forced) {
    if (chain_split_valid(forced)) return forced;        // (0 = the rule)
    return B * 4 <= cus ? 4 : (B * 2 <= cus ? 2 : 1);
}

}  // namespace smk
