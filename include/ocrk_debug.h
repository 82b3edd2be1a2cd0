/* Diagnostics of the tools-only build (`make exp` -> tools/libocrk_exp.so,
 * compiled with -DOCRK_EXPERIMENTS; load it with OCRK_LIB=tools/libocrk_exp.so).
 * NOT part of the product ABI (include/ocrk.h): libocrk.so does not export
 * these, and the tile sweep OCRK_GEMM_NT_CFG that the tools build also reads is
 * inert in it. Instruments only: the routes that measured slower are not kept
 * in the tree (DESIGN.md section 6 names the last commit that holds them). */
#pragma once
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* When buf != NULL the persistent / per-step LSTM forward kernels' workgroups
 * write s_memrealtime stamps ([grid][8] int64) into buf (tools/bench_lstm.py,
 * tools/bench_persist.py). */
int ocrk_lstm_debug_stamps(long long* buf);

#ifdef __cplusplus
}
#endif
