// qk_scan_opts.h -- what the body of the tile-form scan (qk_scan_body.inc) expects in scope besides qk_device.h: the compile-time
// experiment switches and the streaming load.  Shared by the translation units that compile that body (qk_scan.hip, qk_after.hip).
#pragma once
#include "qk_device.h"

// Compile-time experiment switches (scripts/scan_ab.sh builds one library per combination)
#ifndef QK_OPT_EARLY_LOAD
#define QK_OPT_EARLY_LOAD 1   // first tile's loads before the query staging
#endif
#ifndef QK_OPT_EARLY_REC
#define QK_OPT_EARLY_REC 0    // reserve record slots at segment start + deferred rec_next store
#endif
#ifndef QK_OPT_ONE_BALLOT
#define QK_OPT_ONE_BALLOT 1   // one ballot per tile in the steady state
#endif

#ifndef QK_OPT_SELECT1
#define QK_OPT_SELECT1 1      // in-loop compaction of one-wave pools (k <= 36) by bisection select instead of the rank sort
#endif
#ifndef QK_OPT_NT
#define QK_OPT_NT 1           // non-temporal loads for the streamed partition rows (measured: loads-only 5.74 -> 6.44 TB/s)
#endif
#ifndef QK_OPT_STEP_DRAIN
#define QK_OPT_STEP_DRAIN 0   // s_waitcnt vmcnt(0) after every step (limits the bytes in flight per wave)
#endif

__device__ __forceinline__ float4 qk_ld_stream(const float4 *p) {
#if QK_OPT_NT
    const f32x4 t = __builtin_nontemporal_load((const f32x4 *)p);
    return make_float4(t[0], t[1], t[2], t[3]);
#else
    return *p;
#endif
}
