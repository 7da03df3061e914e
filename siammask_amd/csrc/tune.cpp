// tune.cpp -- smk_tune / smk_tune_get (include/siammask_hip_test.h): the process-wide knobs of smk_kernels.h Tuning, one table.
#include <cstdlib>
#include <cstring>

#include "../../include/siammask_hip_test.h"
#include "engine_internal.h"

using namespace smk;

extern "C" {

// ---- smk_tune / smk_tune_get: one table --------------------------------------------------------------------------
// accept: the values smk_tune takes -- "*" any, else terms "a", "a..b" or ">=a" joined by '|'; nullptr: a read-only diagnostic.
// conv: what is stored -- KNOB_RAW the value, KNOB_BOOL value != 0, > 0 value & conv.  product: a knob whose other values are
// measured losers that only a `make MEASURE=1` library carries -- the values a product library takes (its default among them).
enum { KNOB_RAW = 0, KNOB_BOOL = -1 };
struct Knob { const char *name; int *slot; const char *accept; int conv; const char *product; };
#ifdef SMK_MEASURE
static int g_measure_build = 1;                  // smk_tune_get "measure_build": the K-loop ablation kernels are present
#else
static int g_measure_build = 0;
#endif
static const Knob KNOBS[] = {
    {"xcd_mode", &g_tune.xcd_mode, "*", KNOB_RAW, nullptr},
    {"force_tile", &g_tune.force_tile, "0..5", KNOB_RAW, nullptr},
    {"min_blocks_x16", &g_tune.min_blocks_x16, "*", KNOB_RAW, nullptr},
    {"stages", &g_tune.stages, "0|2..4", KNOB_RAW, nullptr},
    {"kt", &g_tune.kt, "0|128|256", KNOB_RAW, nullptr},
    {"prio", &g_tune.prio, "-1..3", KNOB_RAW, nullptr},
    {"nt_store", &g_tune.nt_store, "*", KNOB_BOOL, nullptr},
    {"merge", &g_tune.merge, "0..2", KNOB_RAW, nullptr},
    {"merge_max_batch", &g_tune.merge_max_batch, "*", KNOB_RAW, nullptr},
    {"rf_wreg", &g_tune.rf_wreg, "*", KNOB_RAW, nullptr},           // (+ tile codes 0..8 in bits 4..7 and 8..11: smk_tune)
    {"rf_tile2", &g_tune.rf_tile2, "0..5", KNOB_RAW, nullptr},
    {"nchw_tn_major", &g_tune.nchw_tn_major, "*", KNOB_BOOL, nullptr},
    {"chain", &g_tune.chain, "*", KNOB_BOOL, nullptr},
    {"chain_mask", &g_tune.chain_mask, "0..2", KNOB_RAW, nullptr},
    {"corr_head", &g_tune.corr_head, "*", KNOB_BOOL, nullptr},
    {"pair_launch", &g_tune.pair_launch, "0..3", KNOB_RAW, nullptr},
    {"halo", &g_tune.halo, "0|1|64|128", KNOB_RAW, nullptr},
    {"halo_db", &g_tune.halo_db, "*", KNOB_BOOL, nullptr},
    {"ksplit", &g_tune.ksplit, "0|1|2|4", KNOB_RAW, nullptr},
    {"xc_ch", &g_tune.xc_ch, "32|64", KNOB_RAW, nullptr},
    {"xc_full", &g_tune.xc_full, "0..2", KNOB_RAW, nullptr},
    {"stem_fused", &g_tune.stem_fused, "*", KNOB_BOOL, nullptr},
    {"l1_fused", &g_tune.l1_fused, "*", KNOB_BOOL, nullptr},
    {"buf_lds", &g_tune.buf_lds, "*", KNOB_BOOL, nullptr},
    {"a_stage", &g_tune.a_stage, "*", KNOB_BOOL, nullptr},
    {"wreg", &g_tune.wreg, "0..7", KNOB_RAW, nullptr},
    {"wreg_policy", &g_tune.wreg_policy, "0|1", KNOB_RAW, nullptr},
    {"wreg_stages", &g_tune.wreg_stages, "0|3..8", KNOB_RAW, "0|3|4"},
    {"wreg96", &g_tune.wreg96, "*", KNOB_BOOL, nullptr},
    {"wreg32", &g_tune.wreg32, "0..4096", KNOB_RAW, nullptr},
    {"npw", &g_tune.npw, "2|4", KNOB_RAW, nullptr},
    {"res_nt", &g_tune.res_nt, "*", KNOB_BOOL, nullptr},
    {"pp", &g_tune.pp, "0..2", KNOB_RAW, nullptr},
    {"x3_fused", &g_tune.x3_fused, "*", KNOB_BOOL, nullptr},          // (read when a split-operand context packs its weights)
    {"ablate", &g_tune.ablate, "*", 127, "0"},
    {"front_occ1", &g_tune.front_occ1, "*", 3, "0"},
    {"seq", &g_tune.seq, "*", KNOB_BOOL, nullptr},
    {"seq_spoll", &g_tune.seq_spoll, "*", KNOB_BOOL, nullptr},
    {"seq_kstag", &g_tune.seq_kstag, "0..2", KNOB_RAW, nullptr},
    {"seq_kstag_mask", &g_tune.seq_kstag_mask, "*", 7, nullptr},
    {"seq_tall", &g_tune.seq_tall, "0..2", KNOB_RAW, nullptr},
    {"seq_fuse", &g_tune.seq_fuse, "0..3", KNOB_RAW, nullptr},
    {"seq_fuse3", &g_tune.seq_fuse3, "0..2", KNOB_RAW, "0"},
    {"seq_pair2d", &g_tune.seq_pair2d, "0..2", KNOB_RAW, "0"},
    {"seq_deep", &g_tune.seq_deep, "*", KNOB_BOOL, "0"},
    {"seq_ds128", &g_tune.seq_ds128, "*", KNOB_BOOL, nullptr},
    {"seq_halo", &g_tune.seq_halo, "*", KNOB_BOOL, nullptr},
    {"seq_yres", &g_tune.seq_yres, "*", KNOB_BOOL, nullptr},
    {"seq_search", &g_tune.seq_search, "*", KNOB_BOOL, nullptr},
    {"seq_first_stage", &g_tune.seq_first_stage, "0..3", KNOB_RAW, "1..3"},
    {"seq_min_batch", &g_tune.seq_min_batch, ">=1", KNOB_RAW, nullptr},
    {"seq_max_batch", &g_tune.seq_max_batch, ">=1", KNOB_RAW, nullptr},
    {"seq_extra_batch", &g_tune.seq_extra_batch, "*", KNOB_RAW, nullptr},
    {"seq_mult_max", &g_tune.seq_mult_max, ">=0", KNOB_RAW, nullptr},
    {"main_prio", &g_tune.main_prio, "0..3", KNOB_RAW, nullptr},
    {"pipe_late", &g_tune.pipe_late, "*", KNOB_BOOL, nullptr},
    {"seq_fused_last", &g_seq_last.pairs, nullptr, KNOB_RAW, nullptr},     // pairs fused in the sequence launched last
    {"seq_yres_last", &g_seq_last.resident, nullptr, KNOB_RAW, nullptr},
    {"seq_fused3_last", &g_seq_last.triples, nullptr, KNOB_RAW, nullptr},
    {"measure_build", &g_measure_build, nullptr, KNOB_RAW, nullptr},
};

// The Refine tail's geometry knobs (chain_rows.h, conv_igemm.hip) in a table of their own: tests/test_host_logic.py pins the number of rows
// of KNOBS above; these two are read back by tests/test_chain_rows_host.py.
static const Knob TAIL_KNOBS[] = {
    {"chain_split", &g_tune.chain_split, "0|1|2|4", KNOB_RAW, nullptr},
    {"mask_nsplit", &g_tune.mask_nsplit, "0..15", KNOB_RAW, nullptr},
};

static bool knob_accepts(const char *spec, int v) {
    if (!strcmp(spec, "*")) return true;
    for (const char *t = spec; t; t = strchr(t, '|') ? strchr(t, '|') + 1 : nullptr) {
        if (t[0] == '>' && t[1] == '=') {
            if (v >= atoi(t + 2)) return true;
            continue;
        }
        char *e = nullptr;
        const long lo = strtol(t, &e, 10), hi = (e[0] == '.' && e[1] == '.') ? strtol(e + 2, nullptr, 10) : lo;
        if (v >= lo && v <= hi) return true;
    }
    return false;
}

static const Knob *find_knob(const char *key) {
    for (const Knob &k : KNOBS)
        if (!strcmp(key, k.name)) return &k;
    for (const Knob &k : TAIL_KNOBS)
        if (!strcmp(key, k.name)) return &k;
    return nullptr;
}

int smk_tune(const char *key, int value) {
    if (!key) return fail(SMK_E_ARG, "smk_tune: key is NULL");
    const Knob *k = find_knob(key);
    if (!k) return fail(SMK_E_ARG, "smk_tune: unknown key %s", key);
    if (!k->accept) return fail(SMK_E_ARG, "smk_tune: %s is a read-only diagnostic", key);
    if (!knob_accepts(k->accept, value)) return fail(SMK_E_ARG, "smk_tune: %s takes %s, not %d", key, k->accept, value);
#ifndef SMK_MEASURE
    if (k->product && !knob_accepts(k->product, value))
        return fail(SMK_E_ARG, "smk_tune: %s %d is a measured alternative, only in a library built with `make MEASURE=1` (this one takes %s)",
                    key, value, k->product);
#endif
    if (k->slot == &g_tune.rf_wreg && (((value >> 4) & 15) > 8 || ((value >> 8) & 15) > 8))   // (WREG_TILE has codes 1..8)
        return fail(SMK_E_ARG, "smk_tune: rf_wreg tile codes (bits 4..7, 8..11) 0..8");
    *k->slot = k->conv == KNOB_BOOL ? value != 0 : (k->conv > 0 ? value & k->conv : value);
    return 0;
}

int smk_tune_get(const char *key, int *value) {
    if (!key || !value) return fail(SMK_E_ARG, "smk_tune_get: null argument");
    const Knob *k = find_knob(key);
    if (!k) return fail(SMK_E_ARG, "smk_tune_get: unknown key %s", key);
    *value = *k->slot;
    return 0;
}

}  // extern "C"
