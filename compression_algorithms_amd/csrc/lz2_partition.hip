// lz2_partition.hip — stage 1 of the LDS-resident match finder: cut a block's positions into
// home-bucket ranges ("parts") that no probe cluster can span, and write each part's positions,
// in time order, to one contiguous list.
//
// Why: the first pipeline (lz_find.hip, kept as the fallback) sorts a whole 64 KiB block through
// global scratch; rocprofv3 shows 170x HBM traffic amplification from its scattered 2-byte
// stores (profiles/r01a).  A part of <= LZ2_CAP entries fits in LDS with everything the replay
// needs, so the sorts of stage 2 never leave the CU.
//
// A part boundary must not be crossed by a cluster.  Cluster extents are only known after the
// sort, so the boundary is certified conservatively from per-group counts (group = T/16384
// consecutive buckets, c_g entries):  overflow out of a group is at most
//     out_g = max(in_g + c_g - Gw, c_g - 1, 0)            (all entries on the last bucket)
// a composition of x -> max(x + a, b) maps, i.e. a parallel prefix scan.  Wherever out_g == 0
// no cluster crosses the end of group g.  The deflate flavour's insert wraps modulo T, so its
// bucket space is a ring: the ring is cut at the first certified point and every home is
// re-expressed relative to it (home' = home - base mod T); the lz77 flavour never wraps and
// keeps base = 0.
#include "lz_common.h"
#include "lz2.h"
#include "internal.h"

// (internal linkage, as the kernel had before it was a template: the LDS arrays of a template with external linkage are
//  linkonce symbols the optimiser must keep whole — s_pstart, written and never read, came back as 520 bytes of LDS)
namespace {
#define PT_TICK(k) do { if (sc.dbg && tid == 0) { long long t2 = clock64(); atomicAdd((unsigned long long *)&sc.dbg[32 + (k)], (unsigned long long)(t2 - tk)); tk = t2; } } while (0)

// The LDS of a partition kernel, as the part of the kernel that both of them share takes it.  (The kernels declare the
// arrays: the one that keeps the block in registers lays s_gpart over s_grp, the other has room for both.)
struct Lz2PartLds {
    uint32_t *s_grp;                                 // [LZ2_NG] entries per group on entry; the inclusive prefix from then on
    uint32_t *s_safe;                                // [LZ2_NG / 32] certified groups, zero on entry
    uint64_t *s_scan64;                              // [18]
    uint32_t *s_scan32;                              // [18]
    uint32_t *s_thr;                                 // [LZ2_MAXPARTS + 1] part k = home' in [s_thr[k], s_thr[k+1])
    uint32_t *s_pstart;                              // [LZ2_MAXPARTS + 1]
    uint8_t  *s_gpart;                               // [LZ2_NG] out: part of every rotated group.  May lie over s_grp: its first writer is
                                                     // two barriers behind the last reader of the prefix
    uint8_t  *s_wrank;                               // [LZ2_MAXPARTS]
    uint32_t *s_s0, *s_flag;                         // one word each: the first certified group (~0u on entry), "fall back" (0 on entry)
    uint32_t *s_K, *s_wbase, *s_wbase2;              // one word each
};

// From the counts per group to the part of every group: the overflow certificate, the cuts, the block's record, its parts on
// the work list (or the block on the fallback list) and the table s_gpart.  Called by all 1024 threads behind the barrier that
// ends the counting; returns behind the barrier that ends the tabulation, with the first group of the rotated order in `gstart`
// — or false, with no barrier pending, where the block goes to the fallback pipeline.
__device__ __forceinline__ bool lz2_partition_cuts(const Lz2PartLds &L, const LzP &P, const Lz2Scratch &sc, uint32_t lb, uint32_t n, int tid, long long &tk,
                                                   uint32_t &gstart_out)
{
    uint32_t *const s_grp = L.s_grp, *const s_safe = L.s_safe, *const s_scan32 = L.s_scan32, *const s_thr = L.s_thr, *const s_pstart = L.s_pstart;
    uint64_t *const s_scan64 = L.s_scan64;
    uint8_t *const s_gpart = L.s_gpart, *const s_wrank = L.s_wrank;
    uint32_t &s_s0 = *L.s_s0, &s_flag = *L.s_flag, &s_K = *L.s_K, &s_wbase = *L.s_wbase, &s_wbase2 = *L.s_wbase2;
    const uint32_t T = 1u << P.tbits;
    const uint32_t gshift = P.tbits - LZ2_NG_BITS, Gw = 1u << gshift;

    constexpr uint32_t GPT = LZ2_NG / 1024;            // groups per thread
    static_assert(GPT == 16u, "a thread's part bytes are one 16-byte word");
    // ---- overflow certificate: 16 consecutive groups per thread
    const uint32_t g0 = tid * GPT;
    AffMax mine{0, AM_NEG};
    for (uint32_t k = 0; k < GPT; ++k) {
        const int32_t c = (int32_t)s_grp[g0 + k];
        mine = am_then(mine, AffMax{c - (int32_t)Gw, c > 0 ? c - 1 : 0});
    }
    uint64_t tot64;
    const uint64_t pre64 = block_exclusive_scan<uint64_t>(am_pack(mine), OpAm(), am_pack(AffMax{0, AM_NEG}), s_scan64, &tot64);
    const AffMax pre = am_unpack(pre64), total = am_unpack(tot64);
    // carry into group 0: the ring's fixed point for deflate (F(0) = total.b since total.a = n - T < 0), 0 for lz77
    const int32_t x0 = P.deflate ? (total.b > 0 ? total.b : 0) : 0;
    {
        int32_t x = x0 + pre.a > pre.b ? x0 + pre.a : pre.b;
        if (x < 0) x = 0;
        uint32_t safe_bits = 0;
        for (uint32_t k = 0; k < GPT; ++k) {
            const int32_t c = (int32_t)s_grp[g0 + k];
            int32_t o = x + c - (int32_t)Gw;
            const int32_t o2 = c > 0 ? c - 1 : 0;
            o = o > o2 ? o : o2;
            if (o < 0) o = 0;
            if (o == 0) safe_bits |= 1u << k;
            x = o;
        }
        // 16 groups per thread: two threads share a 32-bit word
        atomicOr(&s_safe[g0 >> 5], safe_bits << (g0 & 31u));
        if (safe_bits) atomicMin(&s_s0, g0 + (uint32_t)__builtin_ctz(safe_bits));
    }
    // inclusive prefix of counts, in place
    {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < GPT; ++k) sum += s_grp[g0 + k];
        uint32_t tot;
        uint32_t run = block_exclusive_scan<uint32_t>(sum, OpAddU32(), 0u, s_scan32, &tot);
        for (uint32_t k = 0; k < GPT; ++k) { run += s_grp[g0 + k]; s_grp[g0 + k] = run; }
    }
    __syncthreads();

    PT_TICK(2);
    // ---- cut the ring / choose the parts
    Lz2BlockMeta *mt = sc.meta + lb;
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_s0);        // (the same for every lane: kept in a scalar register)
    const bool no_safe = (s0 == ~0u);
    // rotated group order starts after s0 (deflate) or at group 0 (lz77: nothing wraps into bucket 0)
    const uint32_t gstart = P.deflate ? (no_safe ? 0u : ((s0 + 1u) & (LZ2_NG - 1u))) : 0u;
    const uint32_t base = gstart << gshift;
    // entries in front of the rotated order: read once, not with every count, and kept in a scalar register
    const uint32_t before = gstart ? (uint32_t)__builtin_amdgcn_readfirstlane((int)s_grp[gstart - 1]) : 0u;
    auto cum_incl = [&](uint32_t gr) -> uint32_t {      // entries in rotated groups 0..gr
        const uint32_t g = (gstart + gr) & (LZ2_NG - 1u);
        return g >= gstart ? s_grp[g] - before : s_grp[g] + (n - before);
    };
    auto is_safe = [&](uint32_t gr) -> bool {
        const uint32_t g = (gstart + gr) & (LZ2_NG - 1u);
        return (s_safe[g >> 5] >> (g & 31u)) & 1u;
    };
    // Greedy cuts: every part takes as many entries as stage 2 can hold (LZ2_CAP), ending at the last certified group
    // that fits.  A fixed target with a fixed margin (parts of TS + "how far back the cut had to move") fails as soon as
    // a block holds one cluster larger than the margin — measured: target 3072 gave +5 % on one corpus and a 6x collapse
    // (every block in the fallback) on another seed whose text has a 1000-entry cluster — while greedy parts only fail when
    // a single cluster exceeds LZ2_CAP.  The cuts depend on each other, so one wave walks them.
    // The walking wave issues ahead of the CU's other waves: fifteen of its own workgroup wait at the barrier below, but the second
    // workgroup on the CU is hashing, and a lone wave of normal priority gets its turn among that one's four on its SIMD.  (The
    // guard is a scalar branch: s_setprio ignores EXEC, so under `tid < 64` alone every wave would raise its priority.)
    const bool walker = __builtin_amdgcn_readfirstlane(tid) < 64;
    if (walker) __builtin_amdgcn_s_setprio(3);
    if (tid < 64) {                                    // wave 0, every lane with the same cur / glo / k
        const uint32_t lane = (uint32_t)tid;
        uint32_t k = 0, cur = 0, glo = 0;               // parts so far, entries before the current part, its first rotated group
        bool bad = false;
        if (lane == 0) s_thr[0] = 0;
        // (a part of a 2^20-bucket table is also kept below 2^16 homes: stage 2 then sorts 16-bit keys in two radix
        //  passes instead of three; a 2^22-bucket table spreads 4096 entries over ~2^18 homes whatever the cut)
        const uint32_t span = (gshift <= 6u) ? (65536u >> gshift) : LZ2_NG;
        // Last certified group g in [glo, .) with at most `limit` entries in rotated groups 0..g, or -1; `upto` gets that count.
        // The boundary is the first rotated group in [glo, hi) whose inclusive count exceeds the limit, else hi.  A cut costs ONE
        // dependent LDS round trip.  The wave keeps 256 checkpoints in registers, four per lane: the count at the end of every
        // 64th group, read once per walk.  How many of them lie within the limit (four ballots) names the 64 groups that hold
        // the first group above it; those 64 groups — or the 64 in front of hi, where hi comes first — are then looked at
        // together, count and certificate bit of a lane's group in one trip: the last certified group lies 0 groups below the
        // boundary in the median and within 10 on text.  Until round 23: two 64-way probes through LDS, a look
        // back and the count, five trips; a first form of the window behind one probe through LDS: two trips, measured slower.
        uint32_t cp[4];                                 // checkpoint lane + 64 q: the entries in rotated groups 0 .. 64 (lane + 64 q) + 63
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) cp[q] = cum_incl(64u * (lane + 64u * q) + 63u);
        auto cut_below = [&](uint32_t limit, uint32_t &upto) -> int32_t {
            // how many of the 256 checkpoints lie within the limit: the first group above it is in the 64 behind them
            uint32_t j = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) j += (uint32_t)__popcll(__ballot(cp[q] <= limit));
            const uint32_t hi0 = (glo + span < LZ2_NG) ? glo + span : LZ2_NG - 1, hi = hi0 < 64u * j + 64u ? hi0 : 64u * j + 64u;
            // the window [hi - 64, hi), lanes below glo off: counts grow with the group, so the first lane over the limit is the
            // boundary (no lane: hi itself) and every group in front of the window is under the limit
            const int32_t w0 = (int32_t)hi - 64, c = w0 + (int32_t)lane;
            const bool on = c >= (int32_t)glo;
            const uint32_t g = (gstart + (uint32_t)c) & (LZ2_NG - 1u);
            uint32_t cum = 0u, sw = 0u;
            if (on) { cum = s_grp[g]; sw = s_safe[g >> 5]; }
            cum = g >= gstart ? cum - before : cum + (n - before);
            const uint64_t mo = __ballot(on && cum > limit);
            const uint64_t ms = __ballot(on && ((sw >> (g & 31u)) & 1u)) & (mo ? (1ull << __builtin_ctzll(mo)) - 1ull : ~0ull);
            if (ms) {
                const uint32_t l = 63u - (uint32_t)__builtin_clzll(ms);
                upto = (uint32_t)__builtin_amdgcn_readlane((int)cum, (int)l);
                return w0 + (int32_t)l;
            }
            // no certified group in the window below the boundary (never on text): further back, 64 groups per look
            for (int32_t gb = w0 - 1; gb >= (int32_t)glo; gb -= 64) {
                const int32_t cb = gb - (int32_t)lane;
                const uint64_t mk = __ballot(cb >= (int32_t)glo && is_safe((uint32_t)cb));
                if (mk) { const int32_t gr = gb - (int32_t)__builtin_ctzll(mk); upto = cum_incl((uint32_t)gr); return gr; }
            }
            return -1;
        };
#ifdef MI_TEST_HOOKS                                       /* lib_test only (MI_LZ_TEST_OLD_CUTS=1): the search as it was, so that a test can compare the */
        auto cut_below_old = [&](uint32_t limit, uint32_t &upto) -> int32_t {        /* parts of both (tests/test_partition_cuts_gpu.py) */
            uint32_t lo = glo, hi = (glo + span < LZ2_NG) ? glo + span : LZ2_NG - 1;
            while (lo < hi) {
                const uint32_t len = hi - lo, step = (len + 63u) / 64u;
                const uint32_t pr = lo + lane * step;
                const bool over = (pr < hi) && cum_incl(pr) > limit;
                const uint64_t mk = __ballot(over);
                if (mk == 0ull) lo = lo + ((len - 1u) / step) * step + 1u;         // every probe is below: continue behind the last one
                else {
                    const uint32_t j = (uint32_t)__builtin_ctzll(mk);
                    hi = lo + j * step;
                    if (j) lo = lo + (j - 1u) * step + 1u;
                }
            }
            // boundary after the last certified group before it, inside this part: 64 groups per look
            for (int32_t g = (int32_t)lo - 1; g >= (int32_t)glo; g -= 64) {
                const int32_t c = g - (int32_t)lane;
                const uint64_t mk = __ballot(c >= (int32_t)glo && is_safe((uint32_t)c));
                if (mk) { const int32_t gr = g - (int32_t)__builtin_ctzll(mk); upto = cum_incl((uint32_t)gr); return gr; }
            }
            return -1;
        };
        const bool old_cuts = (P.flags & LZP_OLD_CUTS) != 0u;
        auto cut = [&](uint32_t limit, uint32_t &upto) -> int32_t { return old_cuts ? cut_below_old(limit, upto) : cut_below(limit, upto); };
#else
        auto cut = cut_below;
#endif
        // parts of at most LZ2_CAP_S entries (four workgroups of stage 2 per CU); where no certified cut lies that close — one
        // cluster of more entries — a part of up to LZ2_CAP entries (k_lz2_find_wide: two per CU)
#ifdef MI_TEST_HOOKS                                       /* lib_test only (MI_LZ_TEST_SMALL_PARTS=1): parts of at most 640 entries — a full block of text */
        const uint32_t cap_s = (P.flags & LZP_SMALL_PARTS) ? 640u : LZ2_CAP_S;   /* gets ~100 of them: the part map's seventh plane, parts beyond stage 2's grid */
#else
        constexpr uint32_t cap_s = LZ2_CAP_S;
#endif
        while (n - cur > cap_s) {
            uint32_t upto = 0u;                                                    // entries in rotated groups 0..gr
            int32_t gr = cut(cur + cap_s, upto);
            if (gr < (int32_t)glo) {
                if (n - cur <= LZ2_CAP) break;                                     // the rest is one wide part
                gr = cut(cur + LZ2_CAP, upto);
            }
            // no certified cut within LZ2_CAP entries: one cluster larger than stage 2 can hold.  (k + 2 > LZ2_MAXPARTS cannot
            // happen — the static_assert in lz2.h has the argument — and stays as a guard.)
            if (gr < (int32_t)glo || k + 2 > LZ2_MAXPARTS) { bad = true; break; }
            cur = upto;
            glo = (uint32_t)gr + 1u;
            ++k;
            if (lane == 0) s_thr[k] = glo << gshift;
        }
#ifdef MI_TEST_HOOKS                                       /* lib_test only (MI_LZ_TEST_FORCE_FALLBACK=1): every block takes the exit above, so a whole */
        if (P.flags & LZP_FORCE_FB) bad = true;                /* batch of ordinary text runs through the fallback chain (tests/test_fallback_chain_gpu.py) */
#endif
        if (lane == 0) {
            s_thr[k + 1] = T;                           // the last part takes everything up to the cut
            s_K = k + 1;
            if (bad) s_flag = 1;
        }
    }
    if (walker) __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    const uint32_t K = s_K;                             // <= LZ2_MAXPARTS
    PT_TICK(3);
    // part sizes; refuse the block if any part exceeds the LDS capacity of stage 2
    if (tid < K) {
        const uint32_t a = s_thr[tid], b = s_thr[tid + 1];
        auto cnt_below = [&](uint32_t h) -> uint32_t {  // entries with home' < h (h is a multiple of Gw or T)
            if (h == 0) return 0u;
            return cum_incl((h >> gshift) - 1u);
        };
        const uint32_t cnt = b > a ? cnt_below(b) - cnt_below(a) : 0u;
        s_pstart[tid] = cnt_below(a);
        if (cnt > LZ2_CAP) atomicOr(&s_flag, 1u);
        mt->part_start[tid] = cnt_below(a);
        mt->part_count[tid] = cnt;
        mt->part_lo[tid] = a;
    }
    if (tid == 0) {
        s_pstart[K] = n;
        mt->n = n; mt->nparts = K; mt->base = base;
        mt->nbig = 0; mt->nbig_entries = 0;
    }
    __syncthreads();
    if (tid == 0) {
        const bool fb = (s_flag != 0) || (P.deflate && no_safe);
        mt->fallback = fb ? 1u : 0u;
        if (fb) { const uint32_t k = atomicAdd(sc.fallback_count, 1u); sc.fallback_list[k] = lb; }
    }
    if (s_flag != 0 || (P.deflate && no_safe)) {
        if (tid == 0 && P.stats) atomicAdd((unsigned long long *)&P.stats[0], 1ull);      // mi_lz_path_stats: blocks sent to the fallback
        return false;
    }
    // this block's parts join the batch's work list: stage 2 runs one workgroup per LISTED part.  (A grid of
    // blocks x "most parts a block can have" interleaved a third of empty workgroups with the real ones; each still had to
    // be given stage 2's 67 KiB of LDS before it could leave: 14.65 -> 11.4 GB/s.)
    {
        if (tid == 0) {
            uint32_t ns = 0, nw = 0;
            for (uint32_t k = 0; k < K; ++k) s_wrank[k] = (uint8_t)(mt->part_count[k] <= LZ2_CAP_S ? ns++ : nw++);
            s_wbase = atomicAdd(sc.work_count, ns);
            s_wbase2 = nw ? atomicAdd(sc.work_count + 1, nw) : 0u;
            if (nw && P.stats) atomicAdd((unsigned long long *)&P.stats[1], (unsigned long long)nw);       // mi_lz_path_stats: wide parts
        }
        __syncthreads();
        if (tid < (int)K) {
            const uint64_t item = (uint64_t)lb | ((uint64_t)tid << 16) | ((uint64_t)mt->part_count[tid] << 24) | ((uint64_t)mt->part_start[tid] << 40);
            if (mt->part_count[tid] <= LZ2_CAP_S) sc.work[s_wbase + s_wrank[tid]] = item;
            else sc.work[sc.work_slots - 1u - (s_wbase2 + s_wrank[tid])] = item;          // the wide list grows from the end (lz2.h)
        }
    }

    // ---- the part of every rotated group (part boundaries are group boundaries): what the kernels look the part of a position
    //      up in.  (s_grp is dead here: its last reader, cum_incl of the part sizes, is two barriers back.)
    {
        // sixteen consecutive groups per thread: one binary search for the first, then a walk along the thresholds
        const uint32_t gr0 = (uint32_t)tid * GPT;
        uint32_t lo = 0, hi = K - 1;                    // last k with thr[k] <= h
        { const uint32_t h = gr0 << gshift; while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (s_thr[mid] <= h) lo = mid; else hi = mid - 1; } }
        uint32_t nxt = lo + 1 < K ? s_thr[lo + 1] : 0xFFFFFFFFu;
        uint32_t pk[GPT / 4u];                          // the sixteen part bytes: one 16-byte store (s_gpart is 16-byte aligned in both kernels)
#pragma unroll
        for (uint32_t k = 0; k < GPT; ++k) {
            const uint32_t h = (gr0 + k) << gshift;
            while (h >= nxt) { ++lo; nxt = lo + 1 < K ? s_thr[lo + 1] : 0xFFFFFFFFu; }
            if (k & 3u) pk[k >> 2] |= lo << (8u * (k & 3u)); else pk[k >> 2] = lo;
        }
        *reinterpret_cast<uint4 *>(s_gpart + gr0) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
    __syncthreads();
    PT_TICK(4);
    gstart_out = gstart;                                // the ring is cut on a group boundary
    return true;
}

template <bool DESC>                                 // DESC: `in` is the batched encoder's descriptor table (lz_block_src)
__global__ __launch_bounds__(1024)
void k_lz2_partition(const uint8_t *__restrict__ in, uint64_t n_total, LzP P, Lz2Scratch sc, uint64_t block0)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_in[LZ_MAX_BLOCK + LZ_TAIL + 16];
    __shared__ __attribute__((aligned(16))) uint32_t s_grp[LZ2_NG];   // counts -> inclusive prefix (read and written 16 bytes at a time); later the staging area
    __shared__ uint32_t s_safe[LZ2_NG / 32];
    __shared__ uint64_t s_scan64[18];
    __shared__ uint32_t s_scan32[18];
    __shared__ uint32_t s_thr[LZ2_MAXPARTS + 1];
    __shared__ uint32_t s_pstart[LZ2_MAXPARTS + 1];
    __shared__ uint32_t s_s0, s_flag, s_K, s_wbase, s_wbase2;
    __shared__ uint8_t s_wrank[LZ2_MAXPARTS];
    __shared__ __attribute__((aligned(16))) uint8_t s_gpart[LZ2_NG];

    const int tid = threadIdx.x;
    const uint32_t lb = blockIdx.x;
    long long tk = clock64();
    const uint8_t *src; uint32_t n;
    lz_block_src<DESC>(in, n_total, P.block, block0, lb, src, n);
    const uint32_t T = 1u << P.tbits, Tmask = T - 1u;
    const uint32_t gshift = P.tbits - LZ2_NG_BITS;

    lz_block_to_lds_of<DESC>(s_in, src, n, (uint32_t)tid);
    for (uint32_t i = tid; i < LZ2_NG; i += 1024) s_grp[i] = 0;
    for (uint32_t i = tid; i < LZ2_NG / 32; i += 1024) s_safe[i] = 0;
    if (tid == 0) { s_s0 = ~0u; s_flag = 0; }
    __syncthreads();
    auto home_of = [&](uint32_t p) -> uint32_t { return lz_mix32(lds_word(s_in, p)) & Tmask; };
    PT_TICK(0);
    // the group of every position stays in registers (two 14-bit numbers per register, 64 positions per thread): the hash is
    // computed once — the pass that tabulates the part of every position further down used to compute it again
    uint32_t gcache[32];
#pragma unroll
    for (uint32_t i = 0; i < 64u; ++i) {
        const uint32_t p = (uint32_t)tid + 1024u * i;
        uint32_t g = 0;
        if (p < n) { g = home_of(p) >> gshift; atomicAdd(&s_grp[g], 1u); }
        if (i & 1u) gcache[i >> 1] |= g << 16; else gcache[i >> 1] = g;
    }
    __syncthreads();
    PT_TICK(1);

    uint32_t gstart_;
    if (!lz2_partition_cuts(Lz2PartLds{s_grp, s_safe, s_scan64, s_scan32, s_thr, s_pstart, s_gpart, s_wrank, &s_s0, &s_flag, &s_K, &s_wbase, &s_wbase2}, P, sc, lb, n, tid, tk, gstart_)) return;

    // ---- positions -> the part map.  The part of every position is tabulated first, one byte each, from the groups in gcache.
    uint8_t *part_in = reinterpret_cast<uint8_t *>(s_grp);              // [65536] part of every position; the group array is dead now
    {
#pragma unroll
        for (uint32_t i = 0; i < 64u; ++i) {
            const uint32_t p = (uint32_t)tid + 1024u * i;
            const uint32_t g = (gcache[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
            part_in[p] = (p < n) ? s_gpart[(g - gstart_) & (LZ2_NG - 1u)] : (uint8_t)PMP_NONE;   // no position: the code no part has (lz2.h)
        }
    }
    __syncthreads();
    PT_TICK(5);
    // The part of every position goes out as seven bit planes (partmap_planes.h), 56 KiB, coalesced: every workgroup of stage 2
    // picks its own positions out of them with a few logic ops per 32 positions and a prefix sum, in time order by construction
    // (lz2_find.hip).  Round 3 sorted the positions into per-part lists here (one stable radix pass over the block: 87 k of this
    // kernel's 205 k cycles — 27 distinct digits, so the lanes of every counting and ranking atomic pile up on a few LDS
    // addresses — and 128 KiB of scattered 2-byte stores); rounds 4 to 19 wrote the map as one byte per position, which each of a
    // block's ~33 workgroups of stage 2 compared byte by byte.
    // Every thread transposes 64 consecutive positions; the planes are staged in s_in (dead since the hashing loop: the groups
    // live in gcache) — not in place, part_in is still being read by other threads.
    {
        uint32_t *stage = reinterpret_cast<uint32_t *>(s_in);
        static_assert(sizeof(s_in) >= PMP_BLOCK_BYTES && LZ_MAX_BLOCK == 64u * 1024u, "the planes of a block are staged in s_in, 64 positions per thread");
        const uint4 *srcv = reinterpret_cast<const uint4 *>(part_in) + 4u * (uint32_t)tid;
        uint32_t w[16], lo[PMP_PLANES], hi[PMP_PLANES];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) { const uint4 v = srcv[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
        pmp_planes_of_bytes(w, lo, hi);
#pragma unroll
        for (uint32_t b = 0; b < PMP_PLANES; ++b)
            *reinterpret_cast<uint2 *>(stage + b * (PMP_PLANE_BYTES / 4u) + 2u * (uint32_t)tid) = make_uint2(lo[b], hi[b]);
        __syncthreads();
        uint4 *dst = reinterpret_cast<uint4 *>(sc.partmap + (size_t)lb * (PMP_BLOCK_BYTES / 4u));
        const uint4 *stv = reinterpret_cast<const uint4 *>(stage);
        for (uint32_t i = tid; i < PMP_BLOCK_BYTES / 16u; i += 1024u) dst[i] = stv[i];
    }
    PT_TICK(6);
    if (sc.dbg && tid == 0) atomicAdd((unsigned long long *)&sc.dbg[47], 1ull);
}

// The same for blocks of ONE buffer that start on 16-byte boundaries (lz2_launch_partition picks), with the block kept in
// registers: thread t owns the positions [64 t, 64 t + 64) from the loads to the stores.  Their 64 words come out of the 17
// dwords that hold the bytes [64 t, 64 t + 68) with one v_alignbyte each, the groups stay in registers as above, and so do the part
// bytes, which the same thread transposes: it holds dwords 2 t and 2 t + 1 of every plane, and a wave stores 512 contiguous bytes
// of a plane with one 8-byte store per lane.  No copy of the block, no byte per position and no staged planes in LDS: 68 KiB
// instead of 147, two workgroups per CU.
// The phase counters keep their numbers: 0 ends behind the zeroing of the counts (the loads are still in flight: their wait is
// in phase 1), 5 is the part of every own position and the transposition, 6 the stores.
__global__ __launch_bounds__(1024, 8)
void k_lz2_partition_direct(const uint8_t *__restrict__ in, uint64_t n_total, LzP P, Lz2Scratch sc, uint64_t block0)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_grp[LZ2_NG];   // counts -> inclusive prefix -> (as bytes) the part of every group
    __shared__ uint32_t s_safe[LZ2_NG / 32];
    __shared__ uint64_t s_scan64[18];
    __shared__ uint32_t s_scan32[18];
    __shared__ uint32_t s_thr[LZ2_MAXPARTS + 1];
    __shared__ uint32_t s_pstart[LZ2_MAXPARTS + 1];
    __shared__ uint32_t s_s0, s_flag, s_K, s_wbase, s_wbase2;
    __shared__ uint8_t s_wrank[LZ2_MAXPARTS];
    static_assert(LZ_MAX_BLOCK == 64u * 1024u, "64 positions per thread");

    const int tid = threadIdx.x;
    const uint32_t lb = blockIdx.x;
    long long tk = clock64();
    const uint8_t *src; uint32_t n;
    lz_block_src<false>(in, n_total, P.block, block0, lb, src, n);
    const uint32_t Tmask = (1u << P.tbits) - 1u;
    const uint32_t gshift = P.tbits - LZ2_NG_BITS;
    const uint32_t p0 = 64u * (uint32_t)tid;

    // The bytes [p0, p0 + 68): four 16-byte words and the first dword of a fifth, issued together.  As in lz_load16_pair, only
    // aligned 16-byte words that hold a byte of the block are read (an offset past the last of them is clamped to it: the
    // loads stay unconditional), and bytes at or past n count as zero — the reference's over-read (lz_block_to_lds).
    uint32_t w[17];
    {
        const uint32_t last = n ? (n - 1u) & ~15u : 0u;
        uint4 v[4] = {};
        uint32_t v4 = 0u;
        if (n) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) { const uint32_t o = p0 + 16u * k; v[k] = *reinterpret_cast<const uint4 *>(src + (o <= last ? o : last)); }
            v4 = *reinterpret_cast<const uint32_t *>(src + (p0 + 64u <= last ? p0 + 64u : last));
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) { w[4 * k] = v[k].x; w[4 * k + 1] = v[k].y; w[4 * k + 2] = v[k].z; w[4 * k + 3] = v[k].w; }
        w[16] = v4;
    }
    for (uint32_t i = tid; i < LZ2_NG; i += 1024) s_grp[i] = 0;
    for (uint32_t i = tid; i < LZ2_NG / 32; i += 1024) s_safe[i] = 0;
    if (tid == 0) { s_s0 = ~0u; s_flag = 0; }
    __syncthreads();
    PT_TICK(0);
    if (p0 + 68u > n) {                              // the thread the block ends in, and the ones behind it
#pragma unroll
        for (uint32_t j = 0; j < 17u; ++j) {
            const uint32_t o = p0 + 4u * j, keep = n > o ? n - o : 0u;          // bytes of this dword below n
            if (keep < 4u) w[j] &= keep ? (1u << (8u * keep)) - 1u : 0u;
        }
    }
    // the group of own position p0 + i (below n): its word is one v_alignbyte of two of the 17 dwords
    auto group_of = [&](uint32_t i) -> uint32_t {
        const uint32_t word = (i & 3u) ? __builtin_amdgcn_alignbyte(w[(i >> 2) + 1], w[i >> 2], i & 3u) : w[i >> 2];
        return (lz_mix32(word) & Tmask) >> gshift;
    };
    // the group of every own position, two per register, as in k_lz2_partition.  (Keeping the 17 dwords instead and hashing a
    // second time below — 48 VGPRs, not 62 — was measured: 2.36 against 1.89 ms of partition per step)
    uint32_t gcache[32];
    // No branch per position: the thread the block ends in adds 0 for its positions at or past n, the threads behind it skip
    // the loop.  Eight positions at a time — all 64 hashes in flight at once do not fit 64 VGPRs.
    if (p0 < n) {
#pragma unroll
        for (uint32_t i = 0; i < 64u; ++i) {
            const uint32_t g = group_of(i);
            atomicAdd(&s_grp[g], p0 + i < n ? 1u : 0u);
            if (i & 1u) gcache[i >> 1] |= g << 16; else gcache[i >> 1] = g;
            if ((i & 7u) == 7u) __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    PT_TICK(1);

    uint8_t *s_gpart = reinterpret_cast<uint8_t *>(s_grp);
    uint32_t gstart_;
    if (!lz2_partition_cuts(Lz2PartLds{s_grp, s_safe, s_scan64, s_scan32, s_thr, s_pstart, s_gpart, s_wrank, &s_s0, &s_flag, &s_K, &s_wbase, &s_wbase2}, P, sc, lb, n, tid, tk, gstart_)) return;

    uint32_t pb[16], lo[PMP_PLANES], hi[PMP_PLANES];   // the part of every own position, four per register, then their planes
#pragma unroll
    for (uint32_t q = 0; q < 16u; ++q) pb[q] = PMP_NONE * 0x01010101u;          // no position: the code no part has (lz2.h)
    if (p0 < n) {
#pragma unroll
        for (uint32_t i = 0; i < 64u; ++i) {
            const uint32_t g = (gcache[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
            const uint32_t look = s_gpart[(g - gstart_) & (LZ2_NG - 1u)], part = (p0 + i < n) ? look : PMP_NONE;
            if (i & 3u) pb[i >> 2] |= part << (8u * (i & 3u)); else pb[i >> 2] = part;
            if ((i & 7u) == 7u) __builtin_amdgcn_sched_barrier(0);
        }
    }
    pmp_planes_of_bytes(pb, lo, hi);
    PT_TICK(5);
    uint2 *dst = reinterpret_cast<uint2 *>(sc.partmap + (size_t)lb * (PMP_BLOCK_BYTES / 4u)) + tid;
#pragma unroll
    for (uint32_t b = 0; b < PMP_PLANES; ++b) dst[b * (PMP_PLANE_BYTES / 8u)] = make_uint2(lo[b], hi[b]);
    PT_TICK(6);
    if (sc.dbg && tid == 0) atomicAdd((unsigned long long *)&sc.dbg[47], 1ull);
}
}  // namespace

void lz2_launch_partition(const uint8_t *d_in, uint64_t n, const LzP &P, const Lz2Scratch &sc, uint64_t block0, uint32_t nb, hipStream_t s)
{
    // one buffer whose blocks all start on 16-byte boundaries: the kernel that keeps the block in registers
    bool direct = !(P.flags & LZP_DESC) && (((uintptr_t)d_in) & 15u) == 0 && P.block % 16u == 0 && P.block <= LZ_MAX_BLOCK;
#ifdef MI_TEST_HOOKS                                       /* lib_test only (MI_LZ_TEST_OLD_PARTITION=1): such input through k_lz2_partition<false> too, */
    if (P.flags & LZP_OLD_PARTITION) direct = false;       /* so that a test can compare what the two kernels write (tests/test_partition_direct_gpu.py) */
#endif
    if (P.flags & LZP_DESC) hipLaunchKernelGGL(k_lz2_partition<true>, dim3(nb), dim3(1024), 0, s, d_in, n, P, sc, block0);
    else if (direct) hipLaunchKernelGGL(k_lz2_partition_direct, dim3(nb), dim3(1024), 0, s, d_in, n, P, sc, block0);
    else hipLaunchKernelGGL(k_lz2_partition<false>, dim3(nb), dim3(1024), 0, s, d_in, n, P, sc, block0);
}

// ---------------------------------------------------------------------------------------------------------------------
// Self-test of block_exclusive_scan with a NON-commutative operator (development / test hook, not in the public header):
// composition of the partition's own x -> max(x + a, b) maps over 1024 threads must equal the serial left-to-right
// composition.  The overflow certificate is only a certificate if earlier maps are applied first.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024)
void k_selftest_scan(const int32_t *__restrict__ ab, uint64_t *__restrict__ out)
{
    __shared__ uint64_t s_tmp[18];
    const int tid = threadIdx.x;
    uint64_t tot;
    const uint64_t pre = block_exclusive_scan<uint64_t>(am_pack(AffMax{ab[2 * tid], ab[2 * tid + 1]}), OpAm(), am_pack(AffMax{0, AM_NEG}), s_tmp, &tot);
    out[tid] = pre;
    if (tid == 0) out[1024] = tot;
}

extern "C" int mi_selftest_scan(mi_ctx *ctx, const int32_t *h_ab /* [1024][2] */, uint64_t *h_out /* [1025] packed a << 32 | b */)
{
    if (!ctx || !h_ab || !h_out) return 0;
    int32_t *d_ab = nullptr; uint64_t *d_out = nullptr;
    if (hipMalloc(&d_ab, 2048 * 4) != hipSuccess || hipMalloc(&d_out, 1025 * 8) != hipSuccess) return 0;
    int ok = hipMemcpy(d_ab, h_ab, 2048 * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) { hipLaunchKernelGGL(k_selftest_scan, dim3(1), dim3(1024), 0, 0, d_ab, d_out); ok = hipDeviceSynchronize() == hipSuccess; }
    if (ok) ok = hipMemcpy(h_out, d_out, 1025 * 8, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_ab); (void)hipFree(d_out);
    return ok;
}
