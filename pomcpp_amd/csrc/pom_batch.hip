/*
 * pom_batch.hip — the C-ABI of include/pom_batch.h (libpom_batch.so): every entry point the reference-side binding links
 * (INTEGRATION.md).  gfx950 only; there is no CPU path: without a HIP device pom_batch_create fails with POM_E_HIP.
 *
 * The library is several translation units: this one, the core, and one per kernel family — pom_search.hip, pom_mixed.hip, pom_events.hip,
 * pom_memory.hip, pom_deal.hip — each holding its kernels with their entry points.  The units meet through pom_host.h (the handle and
 * how a call starts, fails and refuses: defined here, hidden from the library's exports) and pom_device.h (what kernels are made of).
 *
 * This file is the core's table of contents, its parts by concern.  The rule that remains: THE ORDER INSIDE THIS UNIT IS PINNED.  The
 * order is the order kernels are emitted in, and kernels of one unit that share a body reach each other's register allocation through
 * it (pom_issue.h step_kernel): pom_kernels.h and pom_chain.h first (through pom_handle.h), then pom_set_word_kernel (pom_issue.h), the
 * copy kernels, pom_bench_policy_kernel.  The headline kernels live here, so nothing is added to, taken from or moved inside this unit
 * without comparing every kernel's instructions before and after (scripts/compare_kernel_isa.py).  A new kernel family does not come
 * here: it gets a unit of its own (pom_host.h, pom_device.h, its kernel header, its entry points; __graft_entry__.HIP_UNITS), where
 * it cannot disturb the code of another unit and no other can disturb its own.
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
