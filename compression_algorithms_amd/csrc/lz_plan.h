// lz_plan.h — how one call of the 64 KiB-block encoder decides HOW to run: the environment switches, the fallback hint of the
// calls before it, and the plan made of the two.  Host only, plain C++17, no HIP and no project header: an entry point reads the
// switches and the hint ONCE (lz_switches_read; lz_hint_read in lz_find.hip), builds the plan, and everything below it takes
// `const LzPlan &` — or, for blocks above 64 KiB, `const LzSwitches &`.  tests/test_lz_plan.py compiles this
// header alone and holds lz_plan() against a restatement of the rules.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#define MI_SETS 3                      // scratch sets (and event sets of a context) the pipeline rotates through
#define LZ_FB_GRID 128u                // workgroups of a fallback launch while few blocks fall back (lz_find.hip, k_lz_sort_home)

// one member per switch; DESIGN.md has the table
struct LzSwitches {
    bool     v2;                       // MI_LZ_V2: off iff the first character is '0' — first pipeline only
    uint32_t batch;                    // MI_LZ_BATCH: blocks per batch, taken for 1..4096; 0 = the rule decides
    bool     no_overlap;               // MI_LZ_NO_OVERLAP set: one stream
    bool     b_split;                  // MI_LZ_B_SPLIT: off iff '0' — one-batch calls: every kernel on the caller's stream
    int      fb2_side;                 // MI_LZ_FB2_SIDE: -1 unset (the rule decides), 1 first character '1', 0 anything else
    bool     prof_fallback;            // MI_LZ_PROF_FALLBACK set: time the fallback chain and the wide finder aside
    bool     rows;                     // MI_LZ_ROWS: atoi, non-zero = on; unset = on
    uint32_t rows_waves;               // MI_LZ_ROWS_WAVES: atol, row-replay waves per CU; unset or negative = 9
    bool     big_split;                // MI_LZ_BIG_SPLIT: off iff '0' — the wave replay in one launch
    uint32_t lanes_kib;                // MI_LZ_LANES_KIB: atol, LDS per wave of k_lz2_lanes; unset or negative = 8; held to 1..32
    bool     prefix;                   // MI_LZ_PREFIX: atoi, non-zero = on; unset = on
    bool     debug;                    // MI_LZ_DEBUG set: phase counters
    bool     lzw_sliced;               // MI_LZW_SLICED: off iff '0' — whole-block finder for blocks above 64 KiB
    bool     lzs_serial;               // MI_LZS_SERIAL set: the sliced finder on one stream
#ifdef MI_MEASURE
    int      skip;                     // MI_LZ_SKIP: atoi — 1: no stage B, 2: no stage C, 3: neither
    uint32_t stop_phase;               // MI_LZ_STOP_PHASE: atoi — k_lz2_find leaves after phase k
    bool     unsafe_no_fallback;       // MI_LZ_UNSAFE_NO_FALLBACK set: the fallback chain left out
#endif
};

// the only place in the library that reads these from the environment
static inline LzSwitches lz_switches_read()
{
    auto not0 = [](const char *name) { const char *e = getenv(name); return !(e && e[0] == '0'); };
    auto is_set = [](const char *name) { return getenv(name) != nullptr; };
    auto nonzero = [](const char *name) { const char *e = getenv(name); return (e ? (uint32_t)atoi(e) : 1u) != 0u; };
    auto u32 = [](const char *name, uint32_t dflt) {
        const char *e = getenv(name);
        if (!e) return dflt;
        const long v = atol(e);
        return v >= 0 ? (uint32_t)v : dflt;
    };
    LzSwitches sw{};
    sw.v2 = not0("MI_LZ_V2");
    if (const char *e = getenv("MI_LZ_BATCH")) { long v = atol(e); if (v >= 1 && v <= 4096) sw.batch = (uint32_t)v; }
    sw.no_overlap = is_set("MI_LZ_NO_OVERLAP");
    sw.b_split = not0("MI_LZ_B_SPLIT");
    { const char *e = getenv("MI_LZ_FB2_SIDE"); sw.fb2_side = e ? (e[0] == '1' ? 1 : 0) : -1; }
    sw.prof_fallback = is_set("MI_LZ_PROF_FALLBACK");
    sw.rows = nonzero("MI_LZ_ROWS");
    sw.rows_waves = u32("MI_LZ_ROWS_WAVES", 9);
    sw.big_split = not0("MI_LZ_BIG_SPLIT");
    { const uint32_t kib = u32("MI_LZ_LANES_KIB", 8); sw.lanes_kib = kib < 1u ? 1u : kib > 32u ? 32u : kib; }
    sw.prefix = nonzero("MI_LZ_PREFIX");
    sw.debug = is_set("MI_LZ_DEBUG");
    sw.lzw_sliced = not0("MI_LZW_SLICED");
    sw.lzs_serial = is_set("MI_LZS_SERIAL");
#ifdef MI_MEASURE
    // measurement builds only (make EXTRA=-DMI_MEASURE)
    sw.skip = getenv("MI_LZ_SKIP") ? atoi(getenv("MI_LZ_SKIP")) : 0;
    sw.stop_phase = getenv("MI_LZ_STOP_PHASE") ? (uint32_t)atoi(getenv("MI_LZ_STOP_PHASE")) : 0u;
    sw.unsafe_no_fallback = is_set("MI_LZ_UNSAFE_NO_FALLBACK");
#endif
    return sw;
}

// one snapshot of the pair k_lz_sort_home leaves in pinned memory: blocks the last finished batch sent to the fallback, blocks of
// that batch
struct LzHint { uint32_t fb, of; };

enum LzOddChain { LZ_ODD_FB, LZ_ODD_FB2, LZ_ODD_STAGE_B };      // the fallback chains of the odd batches: ctx->fb, ctx->fb2, stage B's stream
enum LzBShape { LZ_B_ROWS_SPLIT, LZ_B_SPLIT, LZ_B_ONE };        // stage B's wave / row group: rows with split, split only, one launch

// everything a call decides before it queues anything
struct LzPlan {
    LzSwitches sw;
    LzHint     hint;
    uint32_t   num_cu;
    uint32_t   nbmax;                  // blocks per batch
    bool       overlap;                // three stages on three streams
    int        nsets;                  // scratch sets in rotation
    bool       solo;                   // a call of one batch: the lane replays beside the wave / row replays (lz_stage_b_solo)
    bool       fb_busy;                // blocks do fall back, and the call is pipelined
    LzOddChain odd_chain;
    bool       want_fb2;               // ctx->fb2 should exist after this call
    LzBShape   b_shape;
    int        skip;                   // measurement builds: 1: no stage B, 2: no stage C, 3: neither; else 0
    bool       no_fallback;            // measurement builds: the fallback chain left out; else false
};

static inline LzPlan lz_plan(uint64_t nblocks, uint32_t num_cu, LzHint hint, const LzSwitches &sw)
{
    LzPlan pl{};
    pl.sw = sw; pl.hint = hint; pl.num_cu = num_cu;
    // As few, as large and as EQUAL batches as fit 3840 blocks (round 4).  The three-stream overlap buys 8 % over running every kernel
    // alone, while every batch pays every kernel's tail: 10^8 B (1 526 blocks) in one batch 17.9 GB/s against 16.5 in two (1 024 + 502),
    // 125 MB 18.4 / 17.6, 2 x 10^8 B 19.9 / 18.6, 3 x 10^8 B 20.5 (2 x 2 289) / 18.8 (1 024 x 4 + 482), 5 x 10^8 B 21.5 (2 x 3 815) / 20.8
    // (2 048 x 3 + 1 486), 10^9 B 21.8-21.9 (4 x 3 815) / 21.7 (3 072 x 4 + 2 971) — same box, mode H.  (Until then: 1 024 below 6 144
    // blocks, 2 048 below 9 216, else 3 072 — "as long as three stages have three batches to overlap".)  ~1.6 GB of workspace per 1 024
    // blocks and set, three sets: 288 GB of HBM make that free; k_lz_scan_blocks holds a batch to 4 096 blocks.
    const uint64_t nbat = (nblocks + 3839u) / 3840u;
    uint64_t cap = nbat ? (nblocks + nbat - 1u) / nbat : 1u;
    // ... unless the input lives in the fallback pipeline (the hint an earlier call left, lz_emit.hip: at least a sixteenth of a batch's
    // blocks): its chains are long serial kernels on few workgroups, and what helps THEM is two batches' chains side by side on two
    // streams — "runs" 4.7 GB/s in two batches against 3.8 in one, "pages" 3.5 / 3.4 (10^8 B): the old rule stays for such input
    if (hint.fb > 8u && (uint64_t)hint.fb * 16u >= hint.of) cap = nblocks >= 3u * 3072u ? 3072u : nblocks >= 3u * 2048u ? 2048u : 1024u;
    if (sw.batch) cap = sw.batch;
    pl.nbmax = (uint32_t)(nblocks < cap ? (nblocks ? nblocks : 1) : cap);
    // three stages on three streams, MI_SETS scratch sets in rotation:
    //   `s`          partition + find of batch i+2          (LDS heavy: one / three workgroups per CU)
    //   ctx->side    replay of the exported clusters of i+1 (almost no LDS: runs beside the find)
    //   ctx->parse   parse / emit / concatenate of batch i  (one 150 KiB workgroup per CU; the stream has raised priority)
    // plus ctx->fb for the normally empty fallback chain.  Fork/join with events only: no host synchronisation.
    pl.overlap = nblocks > pl.nbmax && !sw.no_overlap;
    pl.nsets = pl.overlap ? MI_SETS : 1;
#ifdef MI_MEASURE
    // measurement builds only (make EXTRA=-DMI_MEASURE): what would the step cost if a stage were free?  The stream is WRONG.
    pl.skip = sw.skip;
    // MI_LZ_UNSAFE_NO_FALLBACK=1 leaves the fallback chain out, to price its normally empty launches.  The output is WRONG for any
    // block the partition hands back.
    pl.no_fallback = sw.unsafe_no_fallback;
#endif
    pl.solo = !pl.overlap && sw.b_split && sw.v2 && !pl.skip;
    // The fallback chains of consecutive batches go to two streams WHEN the input lives in the fallback: their kernels are long
    // serial chains on few workgroups and overlap well — pages 1.72 -> 2.16, runs 1.65 -> 2.77 GB/s on 10^8 B.  On text a second
    // stream costs 7 % even idle (20.4 -> 19.1 GB/s, whatever GPU_MAX_HW_QUEUES says), so it exists only while the hint says so.
    // The hint (ctx->h_order[1]) is the fallback count of the last batch the GPU has FINISHED — every batch of a call is queued
    // before the first one runs, so in practice it is what an EARLIER call left: a first call on non-text input runs on one
    // fallback stream and small grids, a text call right after such input still carries the second stream (bench.py reports the
    // adversarial families warm AND cold).  Decided once per call; the stream is created here and released here — when a later
    // call finds the hint low and the stream idle (hipStreamQuery: no host wait) — or with the context, never inside the loop
    // (stream create/destroy per batch, skipped on early returns, may block in hipStreamDestroy).
    const uint32_t fb_hint = pl.overlap ? hint.fb : 0u;
    pl.fb_busy = fb_hint > 8u;                                                                                     // (text: 0)
    // When MOST blocks of a batch fall back (zeros, binary pages) stage B has next to nothing to do: the chains of the odd batches
    // then go to ITS stream and no fifth stream is made at all — every stream beyond the four of the pipeline costs all of them
    // (the process has four hardware queues: pages 33.2 -> 29.5 ms, zeros 12.2 -> 8.4 ms per 10^8 B against fb2).  Where stage B has
    // real work beside the fallback (the "runs" family: 17 % of the blocks fall back, the rest export wide clusters) a chain in front
    // of it costs more than the fifth stream (22.5 -> 27.2 ms): there fb2 stays.  MI_LZ_FB2_SIDE=0 / 1 forces either (A/B).
    const uint32_t fb_of = pl.overlap ? hint.of : 0u;                                                              // blocks of the batch the hint is from
    const bool fb2_side = pl.fb_busy && (sw.fb2_side >= 0 ? sw.fb2_side == 1 : fb_hint * 2u >= fb_of);
    pl.odd_chain = fb2_side ? LZ_ODD_STAGE_B : pl.fb_busy ? LZ_ODD_FB2 : LZ_ODD_FB;
    pl.want_fb2 = pl.fb_busy && !fb2_side;
    // stage B's wave / row group (lz2_stage_b has the launches): MI_LZ_BIG_SPLIT=0 one launch for both wave classes, else the
    // 128..511-entry clusters on the row replay or — MI_LZ_ROWS=0 — on the wave replay
    pl.b_shape = !sw.big_split ? LZ_B_ONE : sw.rows ? LZ_B_ROWS_SPLIT : LZ_B_SPLIT;
    return pl;
}

// what the fallback chain of a batch of nb blocks launches (lz_find_batch)
struct LzFbGrids {
    uint32_t fb_want;                  // workgroups the hint asks for
    uint32_t fgrid;                    // k_lz_sort_home, k_lz_sort_cluster, k_lz_emulate (per tile)
    uint32_t giant_cap, giant_grid;    // k_lz_emulate_giant<LZ_GIANT_CAP>
    uint32_t small_grid;               // k_lz_emulate_giant<LZ_GIANT_SMALL>; 0: not launched
};
static inline LzFbGrids lz_plan_fallback_grids(const LzPlan &pl, uint32_t nb)
{
    // fallback: few looping workgroups (see LZ_FB_GRID) — unless the last finished batch (in practice: of an earlier call) had
    // many blocks here (non-text input): the count k_lz_sort_home left in pinned memory sizes the grids (pages family: half the
    // chip sat idle behind 128 workgroups)
    const bool listed = pl.sw.v2;                            // the chain runs a list of blocks; MI_LZ_V2=0: it is the finder, every block
    const uint32_t hint = listed ? pl.hint.fb : 0u;
    LzFbGrids g{};
    g.fb_want = hint > LZ_FB_GRID ? hint : LZ_FB_GRID;
    g.fgrid = (listed && nb > g.fb_want) ? g.fb_want : nb;
    g.giant_cap = listed ? (hint > LZ_FB_GRID ? 512u : LZ_FB_GRID) : 1024u;
    g.giant_grid = nb < g.giant_cap ? nb : g.giant_cap;
    // blocks do fall back: the clusters of <= LZ_GIANT_SMALL entries six workgroups per CU
    if (listed && hint > 8u) g.small_grid = nb * 2u < pl.num_cu * 6u ? nb * 2u : pl.num_cu * 6u;
    return g;
}
