/*
 * pom_batch.hip — the C-ABI of include/pom_batch.h (libpom_batch.so): every entry point the reference-side binding links
 * (INTEGRATION.md).  gfx950 only; there is no CPU path: without a HIP device pom_batch_create fails with POM_E_HIP.
 *
 * This file is the table of contents: one translation unit, its parts by concern.  The order is the order kernels are emitted in,
 * which reaches their register allocation (pom_issue.h step_kernel): pom_kernels.h and pom_chain.h first (through pom_handle.h),
 * then pom_set_word_kernel (pom_issue.h), the copy kernels, pom_bench_policy_kernel, and the search kernels last, each in front of
 * its entry point, pom_step_mixed_kernel behind them, then pom_reach_kernel, pom_view_memory_kernel, pom_imagine_kernel, and pom_deal_kernel the very last.  The entry points between them define no kernel.
 */
#include "pom_handle.h"       /* the handle, its streams, how a call on it begins (begin_call) and how any call refuses (refuse) */
#include "pom_issue.h"        /* a step as launches: the kernel table, runs and who issues them, parts, graphs, several-tick calls */
#include "pom_chain_host.h"   /* chained launches, host half: launch_many_chain, and chain_settle behind every settled call */
#include "pom_copy.h"         /* the kernels of pom_batch_copy_envs */
#include "pom_api_handle.h"   /* entry points: create (options and shape: create_plan), destroy, streams, tick, what the handle reports */
#include "pom_api_transfer.h" /* entry points: upload, download, generate, snapshot, copies by index, the read-backs (one chunk loop) */
#include "pom_api_observe.h"  /* entry points: the observation, alone or fused with a tick, plain and as fogged views */
#include "pom_api_step.h"     /* entry points: ticks from explicit moves, synthetic streams, SimpleAgent; the closed-loop range call */
#include "pom_api_diag.h"     /* entry points: chain statistics and litmus, the diagnostic builds' readers, profiling, pom_bench_policy */
#include "pom_api_one.h"      /* entry points: pom_step / pom_env_step on one State in host memory */
#include "pom_api_search.h"   /* entry points: forecast, rollouts, expand, move safety — with their kernel headers */
#include "pom_api_mixed.h"    /* entry point: pom_batch_step_mixed, the range call with SimpleAgent opponents — with its kernel header */
#include "pom_reach.h"        /* pom_batch_reach's kernel and its launch (the entry point is pom_api_search.h's) */
#include "pom_api_memory.h"   /* entry point: pom_batch_remember_view, the views merged into the agents' memory — with its kernel header */
#include "pom_api_imagine.h"  /* entry point: pom_batch_imagine, games built from an agent's view memory — with its kernel header */
#include "pom_api_deal.h"     /* entry point: pom_batch_deal, Pommerman's standard start boards dealt on the device — with its kernel header, LAST */
