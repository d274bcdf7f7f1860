// ABI version + process-wide tuning knobs of libunsloth_amd.so
#include <stdlib.h>

#include "common.h"

extern "C" int uamd_version(void) { return (0 << 16) | 2; }

namespace {
// One row per UAMD_TUNE_* number, in the header's order. Environment names only for the knobs whose choice still depends on the
// workload (attention forward kernel, fused-activation schedule, GEMM kernel family); the others' A/Bs are settled -- they
// remain `uamd_set_tuning` hooks for the parity tests. `value` < 0: not resolved yet.
struct Knob { const char* env; int dflt; int value; };
Knob g_knob[] = {
    {nullptr, 2, -1},            // UAMD_TUNE_GLU_VAR
    {nullptr, 8, -1},            // UAMD_TUNE_GROUP_M
    {nullptr, 0, -1},            // UAMD_TUNE_STREAM_NT
    {nullptr, 1, -1},            // UAMD_TUNE_DEQUANT_T
    {"UAMD_ATTN_VAR", 0, -1},    // UAMD_TUNE_ATTN_VAR
    {nullptr, 1, -1},            // UAMD_TUNE_RMS_VAR
    {nullptr, 1, -1},            // UAMD_TUNE_GEMM_HALF
    {nullptr, 1, -1},            // UAMD_TUNE_GEMM_PERSIST
    {nullptr, 1, -1},            // UAMD_TUNE_DEQUANT_X4
    {nullptr, 1, -1},            // UAMD_TUNE_GEMM_PLAIN
    {"UAMD_GLU_XA", 3, -1},      // UAMD_TUNE_GLU_XA
    {"UAMD_GEMM_S", 1, -1},      // UAMD_TUNE_GEMM_S
};
static_assert(sizeof(g_knob) / sizeof(g_knob[0]) == UAMD_TUNE_COUNT, "one g_knob row per UAMD_TUNE_* knob");
}  // namespace

// value of a knob: uamd_set_tuning() > environment variable > built-in default (the measured-fastest setting)
int uamd_tuning_get(int knob) {
    if (knob < 0 || knob >= UAMD_TUNE_COUNT) return 0;
    Knob& k = g_knob[knob];
    if (k.value < 0) {
        const char* e = k.env ? getenv(k.env) : nullptr;
        k.value = (e && *e) ? atoi(e) : k.dflt;
        if (k.value < 0) k.value = k.dflt;
    }
    return k.value;
}

extern "C" int uamd_set_tuning(int knob, int value) {
    if (knob < 0 || knob >= UAMD_TUNE_COUNT || value < 0) return UAMD_ERR_ARG;
    g_knob[knob].value = value;
    return UAMD_OK;
}
