// hite_switch.h -- the tri-state "which form runs" switches of a context, in one table: 1 / 0 = a form, -1 = follow the process
// default, which is taken from the environment when it is first asked for.  Plain C++ (no HIP): tests/test_host_switch.py
// compiles it alone.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum HiteSwitch {
    HITE_SW_COPY_INTERVAL,      // copy records carry 1 the aligned interval / 0 the interval of the whole candidate (hite_copies.hip)
    HITE_SW_FILL_TILES,         // the sparse fill 1 by tiles of positions / 0 per cell (hite_msa.hip)
    HITE_SW_GATHER_CHUNKS,      // the window gather 1 in chunks of the destination / 0 a wavefront per row (hite_pipeline.hip)
    HITE_SW_FALLBACK_OVERLAP,   // the fall-back alignment 1 beside the layout of the other candidates / 0 before it (hite_msa.hip)
    HITE_SW_WIDE_TB_RUNS,       // the fall-back's traceback 1 by runs of up to 64 steps / 0 a column per step (hite_align.hip)
    HITE_SW_N
};

// the environment variable of a switch and the values that mean 0; anything else -- unset and empty included -- means 1
struct HiteSwitchRow { const char *env; const char *off[2]; };
static const HiteSwitchRow hite_switch_table[HITE_SW_N] = {
    {"HITE_COPY_INTERVAL", {"0", "whole"}},
    {"HITE_FILL_TILES", {"0", nullptr}},
    {"HITE_GATHER_CHUNKS", {"0", nullptr}},
    {"HITE_FALLBACK_OVERLAP", {"0", nullptr}},
    {"HITE_WIDE_TB_RUNS", {"0", nullptr}},
};

// the process defaults (an inline variable: one copy per process); -1 = not resolved yet
inline int hite_switch_default[HITE_SW_N] = {-1, -1, -1, -1, -1};

// sw: the context's values (hite_ctx::sw), or NULL for the process default alone
inline int hite_switch_resolve(const int32_t *sw, HiteSwitch s) {
    if (sw && sw[s] >= 0) return sw[s];
    int v = __atomic_load_n(&hite_switch_default[s], __ATOMIC_RELAXED);
    if (v < 0) {
        const char *e = getenv(hite_switch_table[s].env);
        v = 1;
        for (const char *off : hite_switch_table[s].off)
            if (e && off && !strcmp(e, off)) v = 0;
        __atomic_store_n(&hite_switch_default[s], v, __ATOMIC_RELAXED);
    }
    return v;
}

inline bool hite_switch_valid(int32_t v) { return v >= -1 && v <= 1; }

// the setters: false (nothing stored) for a value other than -1, 0, 1 or without a context
inline bool hite_switch_set(int32_t *sw, HiteSwitch s, int32_t v) {
    if (!sw || !hite_switch_valid(v)) return false;
    sw[s] = v;
    return true;
}
// -1: the next hite_switch_resolve reads the environment again
inline bool hite_switch_set_default(HiteSwitch s, int32_t v) {
    if (!hite_switch_valid(v)) return false;
    __atomic_store_n(&hite_switch_default[s], (int)v, __ATOMIC_RELAXED);
    return true;
}
