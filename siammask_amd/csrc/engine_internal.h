// engine_internal.h -- what the host translation units of libsiammask_hip.so share (internal, not installed): error reporting
// and the helpers that do not use a context.  struct smk_ctx is private to engine.cpp and stays out of this header.
//   weight_pack.cpp   host packing and upload of one convolution's weights
//   conv_launch.cpp   ConvParams from (pack, tensors, options); the one place a plan becomes a launch
//   engine.cpp        fail / the error string, the sequence helpers, everything that uses a context
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <vector>

#include "../../include/siammask_hip.h"
#include "conv_plan.h"
#include "smk_kernels.h"

#pragma GCC visibility push(hidden)   // (nothing here is part of the library's ABI)

namespace smk {

// ---- errors: one thread-local string (engine.cpp), read by smk_last_error; every translation unit reports through fail ----------
int fail(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(SMK_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                        __FILE__, __LINE__);                                               \
    } while (0)

#define CHK(expr)                     \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != 0) return rc_;     \
    } while (0)

inline int rup(int x, int a) { return (x + a - 1) / a * a; }
inline size_t esize(int dtype) { return dtype == DT_F32 ? 4 : 2; }

constexpr size_t KS_PART_FLOATS = 8u << 20;      // split-K partial tiles, 32 MB: e.g. 256 tiles x 4 parts x 64x128
constexpr int KS_CNT = 8192;                     // ... and their arrival counters
constexpr long MI355X_CUS = 256;                 // what host-only planning (smk_host_plan_conv) plans for

// ---- weight_pack.cpp -----------------------------------------------------------------------------------------------------------
void pack_rows(std::vector<float> &dst, int row0, int Kpad, const float *w, const double *scale, int Cout, int Cin, int k, int Ci);
bool has_frag_pack(const PackedConv &pc, int dtype);
bool has_frag16_pack(const PackedConv &pc, int dtype);
bool has_halo_pack(const PackedConv &pc, int dtype);
bool has_frag_halo_pack(const PackedConv &pc, int dtype);
int upload_frag_pack(PackedConv &pc, const std::vector<float> &rows_f32, int dtype);
int upload_packed(PackedConv &pc, const std::vector<float> &rows_f32, const std::vector<float> &bias, int dtype,
                  const std::vector<float> *frag_rows = nullptr);
int upload_halo_pack(PackedConv &pc, const std::vector<float> &rows_f32, int dtype);
void split_rows_x3(std::vector<float> &rows, int nrows, int Kpad1, int Kpad3, int taps, int Ci0, std::vector<float> &oscale);
bool fuse_rows_x3(const std::vector<float> &rows, PackedConv &pc, int taps, int Ci0, std::vector<float> &out);
int upload_oscale(PackedConv &pc, const std::vector<float> &oscale);
void stem_pair_rows(std::vector<float> &rows, std::vector<float> &bias, int Kpad, const float *w, const double *scale, const double *shift);
PackedConv stem_pack_geom();

// ---- conv_launch.cpp -----------------------------------------------------------------------------------------------------------
// what conv_params takes from its surroundings: a context's (engine.cpp conv_env) or a context-free entry point's own
struct ConvEnv {
    int dtype = DT_F32, device = 0;      // device < 0: host-side walk (CPU tests)
    float *ks_part = nullptr;            // split-K scratch (KS_PART_FLOATS) and arrival counters (KS_CNT), or none
    unsigned *ks_cnt = nullptr;
    int wave_prio = 0;
};
int conv_params(const ConvEnv &env, const PackedConv &pc, const Act &in, const Act *out, int B, const ConvOpt &o, ConvParams &p);
void conv_work(const PackedConv &pc, const ConvParams &p, int B, int dtype, double &flop, double &bytes);
int launch_plan(const ConvPlan &pl, ConvBatch &cb, const void *w_halo, int dtype, hipStream_t s, const char *what);

// ---- engine.cpp: the sequence helpers smk_op_conv_seq shares with seq_flush -----------------------------------------------------
extern SeqPlanStats g_seq_last;   // marks of the launch issued last (smk_tune_get "seq_fused_last" / "seq_fused3_last" / "seq_yres_last", diagnostics)
int seq_grid_for(int ncu);
void seq_print_clk(const SeqArgs &a, const SeqRec *r, const char *idn, const unsigned long long *h, const unsigned long long *h2);

}  // namespace smk

#pragma GCC visibility pop
