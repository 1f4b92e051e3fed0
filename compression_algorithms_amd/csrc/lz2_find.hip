// lz2_find.hip — stage 2 and 3 of the LDS-resident match finder.
//
//   k_lz2_find        one workgroup per part (<= LZ2_CAP_S = 2048 positions whose clusters lie inside the part, certified by
//                     stage 1; < 40 KiB of LDS, four per CU.  k_lz2_find_wide: the same body for the rare parts of up to
//                     LZ2_CAP = 4096).  Everything happens in LDS: mixed words (home = mask, equality = equality), positions
//                     sorted by home (2-3 stable 8-bit radix passes), clusters / dense home slots / word ids / "mixed"
//                     bits from the parking sweep, (cluster, time) order by cursor placement.  Then
//                       - a cluster of ONE word is answered by a closed form (anchor chain): most clusters;
//                       - while a cluster has retired nothing, find() is the first occurrence of the word = the word
//                         id: quiet clusters are answered without any replay, and lz77 with a window
//                         that covers the block stops right after the sweep;
//                       - mixed clusters of 2..7 entries are replayed one lane each, their table in two registers;
//                       - larger mixed ones are exported on 16-byte boundaries, by size class.
//   k_lz2_lanes       lane per exported cluster of 8..127 entries (LDS regions per lane, eight entries per load), ONE launch:
//                     the clusters sorted by size (k_lz2_lane_count / k_lz2_lane_place), a wave per group of clusters of one
//                     size, regions sized by it.
//   k_lz2_big         one WAVE per exported cluster of 512..1024 entries (and of what the row replay leaves): occupancy bitmap in
//                     registers, first fit by ballot + v_readlane, 6 bytes of LDS per entry; bound by scalar-instruction issue.
//   k_lz2_rows        FOUR exported clusters of 128..511 entries per wave, one per 16-lane row, 256..511 first (round 4).
//   k_lz2_scatter     lists -> by-position array (test hook and fallback boundary).
//
// Replaces the same reference functions as lz_find.hip (hash / insert_hash_table / find,
// algorithms/lz77/lz77.c:13-108 and algorithms/deflate/lz77.c:14-174).
#include "lz_common.h"
#include "lz2.h"
#include "lz_dom.h"
#include "lz_replay.h"
#include "internal.h"
#include <stdlib.h>

#define RS_HEAD 0x8000u
#define RS_MASK 0x7FFFu

__device__ __forceinline__ bool bm2_test(const uint32_t *bm, uint32_t b) { return (bm[b >> 5] >> (b & 31u)) & 1u; }

// lane-per-cluster replay of a SMALL cluster [s, e) (< LZ2_BIG entries): plain word scan is enough
__device__ void replay_small(const uint16_t *pos, uint16_t *rs, const uint16_t *pid, uint16_t *occ, uint32_t *bm,
                             uint32_t s, uint32_t e, uint32_t W, uint32_t anom, uint32_t limit, uint16_t *cand_i)
{
    uint32_t ev = s;
    bool anom_pending = anom != ~0u;
    const bool plain = (anom == ~0u) && (limit == ~0u);                 // not the cluster that covers bucket 0 / T
    if (plain && (uint32_t)pos[e - 1] <= (uint32_t)pos[s] + W) {
        // a cluster whose entries all lie within one window never evicts: no replay at all, find() = first occurrence
        for (uint32_t i = s; i < e; ++i) { const uint32_t id = pid[i]; cand_i[i] = (id != pos[i]) ? (uint16_t)id : (uint16_t)LZ_NONE16; }
        return;
    }
    for (uint32_t i = s; i < e; ++i) {
        const uint32_t p = pos[i], rsv = rs[i], r = rsv & RS_MASK, id = pid[i];
        while (ev < i && (uint32_t)pos[ev] + W < p) {                   // FIFO retirement, lz77.c:70-76
            const uint32_t b = rs[ev] & RS_MASK;
            atomicAnd(&bm[b >> 5], ~(1u << (b & 31u)));
            ++ev;
        }
        if (anom_pending && p > W - 1u) { atomicAnd(&bm[anom >> 5], ~(1u << (anom & 31u))); anom_pending = false; }
        // the bitmap word and the occupant of the home slot are fetched together, then its id and position together
        uint32_t wi = r >> 5;
        const uint32_t w0 = bm[wi];
        const uint32_t o0 = occ[r];
        uint32_t res = LZ_NONE16;
        if (plain && ev == s) {                                         // nothing evicted yet: the first occurrence (see the sweep)
            if (id != p) res = id;
        } else if ((w0 >> (r & 31u)) & 1u) {
            const uint32_t id0 = pid[o0], pos0 = pos[o0];
            if (id0 == id) res = pos0;
            else {
                for (uint32_t b = r + 1;; ++b) {                         // rare: the home holds another word
                    if (b == limit && r < limit) break;
                    if (!bm2_test(bm, b)) break;
                    const uint32_t o = occ[b];
                    if (pid[o] == id) { res = pos[o]; break; }
                }
            }
        }
        cand_i[i] = (uint16_t)res;
        uint32_t wv = w0 | ((1u << (r & 31u)) - 1u);                     // first fit: word scan (inside the cluster by the parking bound)
        while (wv == 0xFFFFFFFFu) wv = bm[++wi];
        const uint32_t b = (wi << 5) + (uint32_t)__builtin_ctz(~wv);
        atomicOr(&bm[b >> 5], 1u << (b & 31u));
        occ[b] = (uint16_t)i;
        rs[i] = (uint16_t)((rsv & RS_HEAD) | b);
    }
}

// The same replay for a cluster of < 8 entries that does not cover bucket 0 / T, with its whole table in registers:
// 7 occupancy bits, the occupant of every slot and the slot of every entry as 4-bit fields.  LDS is only read for the
// entry records (and for an occupant's word id when a probe has to compare) and written for the result.
// F = uint32_t: up to 8 four-bit fields (clusters below 8 entries); F = uint64_t: up to 16 (below 16).
template <typename F>
__device__ __forceinline__ void replay_small_reg(const uint16_t *pos, const uint16_t *rs, const uint16_t *pid,
                                                 uint32_t s, uint32_t e, uint32_t W, uint16_t *cand_i)
{
    if ((uint32_t)pos[e - 1] <= (uint32_t)pos[s] + W) {
        // a cluster whose entries all lie within one window never evicts: no replay at all, find() = first occurrence
        for (uint32_t i = s; i < e; ++i) { const uint32_t id = pid[i]; cand_i[i] = (id != pos[i]) ? (uint16_t)id : (uint16_t)LZ_NONE16; }
        return;
    }
    const uint32_t n = e - s;
    uint32_t mask = 0;
    F ent = 0, slots = 0;
    uint32_t ev = 0, ev_pos = pos[s];
    for (uint32_t li = 0; li < n; ++li) {
        const uint32_t i = s + li;
        const uint32_t p = pos[i], rr = ((uint32_t)rs[i] & RS_MASK) - s, id = pid[i];
        while (ev < li && ev_pos + W < p) {                              // FIFO retirement, lz77.c:70-76
            mask &= ~(1u << ((uint32_t)(slots >> (4u * ev)) & 15u));
            ++ev; ev_pos = pos[s + ev];
        }
        uint32_t res = LZ_NONE16;
        if (ev == 0) {                                                  // nothing evicted yet: the first occurrence (see the sweep)
            if (id != p) res = id;
        } else if (id != p) {                                           // (a word's first occurrence in the block finds nothing, ever)
            for (uint32_t b = rr; (mask >> b) & 1u; ++b) {              // bits >= n are never set: the probe ends inside the cluster
                const uint32_t o = s + ((uint32_t)(ent >> (4u * b)) & 15u);
                if (pid[o] == id) { res = pos[o]; break; }
            }
        }
        cand_i[i] = (uint16_t)res;
        const uint32_t b = rr + (uint32_t)__builtin_ctz(~(mask >> rr));  // first fit (inside the cluster by the parking bound)
        mask |= 1u << b;
        ent = (ent & ~((F)15u << (4u * b))) | ((F)li << (4u * b));
        slots |= (F)b << (4u * li);
    }
}

// one part: `item` = block | part << 16 | entries << 24 | list start << 40 (lz2.h).  CAP = LDS capacity in entries.
template <uint32_t CAP, bool DESC>
__device__ __forceinline__ void lz2_find_part(const uint8_t *__restrict__ in, uint64_t n_total, const LzP &P, const Lz2Scratch &sc, uint64_t block0, const uint64_t item)
{
    // 16 bytes per entry + radix counters
    __shared__ uint16_t s_pos[CAP];                 // position by time index j
    __shared__ uint32_t s_word[CAP];                // mix32(word) by j; later e_pos / e_rs (replay order)
    __shared__ uint16_t s_j0[CAP], s_j1[CAP];   // sort ping-pong; later e_pid / (free)
    __shared__ __attribute__((aligned(16))) uint16_t s_gr[2 * CAP];   // s_g | s_r; during the home sort: the second pass's counters
    uint16_t *const s_g = s_gr;                          // cluster number by j; later occ
    uint16_t *const s_r = s_gr + CAP;                // dense home slot by j; later cand by replay index
    __shared__ uint16_t s_pid[CAP + 2];             // word id by j (position of the first occurrence); then s_gstart; last cand by j
    // radix counters, [digit][wave + pad] (lz_common.h): a count is at most CAP, so 16 bits hold it — 4.5 KiB instead of 9,
    // part of the budget of four workgroups per CU; the wide instance keeps 32 bits, because the cluster cursors and the
    // export lists that live in the counters after the sorts need 8 KiB there (static_asserts below)
    using Cnt = typename std::conditional<(CAP <= 2048u), uint16_t, uint32_t>::type;
    __shared__ __attribute__((aligned(16))) Cnt s_cnt[LZ2_NWAVES + 1][256];
    __shared__ uint32_t s_bm[CAP / 32 + 2];
    __shared__ uint32_t s_mix[CAP / 32 + 2];        // bit g: cluster g holds more than one home or more than one word ("mixed")
    __shared__ int32_t  s_i32[18];
    __shared__ uint32_t s_zslot, s_zgid, s_nbigl, s_ngroups;
    // LDS diet: four of these workgroups share a CU (two of the wide instance), and whatever they leave is all that the replay
    // kernels of the previous batch can use beside them.  Arrays that are dead by then are reused:
    //   s_gstart (replay index of the head of every cluster) lives in s_pid, dead between the permutation and the final
    //            reordering of the results;
    //   s_big    ({s, e, global dst} of the clusters this part exports) and s_quiet (quiet clusters of >= LZ2_BIG
    //            entries) live in the radix counters, dead after the second sort.
    uint16_t *const s_gstart = s_pid;
    uint32_t *const s_big = reinterpret_cast<uint32_t *>(&s_cnt[0][0]);
    uint16_t *const s_quiet = reinterpret_cast<uint16_t *>(s_big + 3 * (CAP / LZ2_BIG));
    static_assert(3 * (CAP / LZ2_BIG) * 4 + 2 * (CAP / LZ2_BIG) * 2 <= sizeof(s_cnt), "export lists must fit the radix counters");

    const int tid = threadIdx.x;
    const uint32_t lb = (uint32_t)item & 0xFFFFu, part = (uint32_t)(item >> 16) & 0xFFu;
    Lz2BlockMeta *mt = sc.meta + lb;
    long long tk = clock64();
    // stop_phase exists only in a measurement build (make EXTRA=-DMI_MEASURE, scripts/phase_pmc.sh): the shipped library never
    // leaves early, whatever the environment says (a stray MI_LZ_STOP_PHASE produced wrong streams with MI_OK)
// The phase counters (MI_LZ_DEBUG=1) are compiled into measurement builds only, too: the clock and the counter pointer held
// SGPRs across the whole body, and the shipped kernel has to stay within 80 of them (four workgroups per CU, k_lz2_find).
#ifdef MI_MEASURE
#define LZ2_STOP(k) if ((k) < 7 && sc.stop_phase == (uint32_t)(k) + 1u) return
#define LZ2_DBG     sc.dbg
#else
#define LZ2_STOP(k) do { } while (0)
#define LZ2_DBG     ((uint64_t *)nullptr)
#endif
#define LZ2_TICK(k) do { if (LZ2_DBG && tid == 0) { long long t2 = clock64(); atomicAdd((unsigned long long *)&LZ2_DBG[k], (unsigned long long)(t2 - tk)); tk = t2; } \
                         LZ2_STOP(k); } while (0)
    // (only parts of blocks that did not fall back are listed; the list position and length ride in the item, so the list
    //  loads below do not wait for the block's meta record)
    const uint32_t m = (uint32_t)(item >> 24) & 0xFFFFu;
    if (m == 0) return;
    const uint32_t pstart = (uint32_t)(item >> 40), base = mt->base;
    const uint32_t nblk = mt->n;
    const uint8_t *src; uint32_t n_unused;
    lz_block_src<DESC>(in, n_total, P.block, block0, lb, src, n_unused);
    (void)n_unused;
    const uint32_t T = 1u << P.tbits, Tmask = T - 1u, W = 1u << P.wbits;
    uint16_t *plist = sc.plist + (size_t)lb * LZ_MAX_BLOCK + pstart;       // written here (the parse reads position / candidate lists)
    (void)n_total;
    // keys of the home sort are relative to the part's first home; a part of a 2^20-bucket table spans < 2^16 homes, so two
    // 8-bit passes are enough (three otherwise).  For two passes the digits are COUNTED where they are in hand anyway: the first
    // pass's while the words are hashed, the second pass's while the first one scatters — no counting loops of their own.
    const uint32_t plo_ = mt->part_lo[part];
    const uint32_t phi_ = (part + 1 < mt->nparts) ? mt->part_lo[part + 1] : T;
    const bool three = (phi_ - plo_) > 65536u;
    Cnt *const cntA = &s_cnt[0][0];
    Cnt (*const s_cntB)[256] = reinterpret_cast<Cnt (*)[256]>(s_gr);                 // (s_g / s_r are idle until the sweep)
    Cnt *const cntB = &s_cntB[0][0];
    // the second pass's counters must fit s_gr: with 32-bit counters and parts of 2048 entries they did not (9 KiB on 8), and
    // the zeroing and counting ran 1 KiB into whatever LDS array follows — the round-3 A/B build with parts of 2048 entries
    static_assert(sizeof(s_cnt) <= sizeof(s_gr), "the second pass's radix counters must fit s_g | s_r");
    constexpr uint32_t RST = LZ2_NWAVES + 1;                                        // counter stride of radix_pass
    const uint32_t seg = radix_seg<LZ2_NWAVES>(m), seg_inv = (uint32_t)((0x100000000ull + seg - 1u) / seg);   // i / seg = umulhi(i, seg_inv) for i < 2^16
    {   // both sets of counters are zeroed 16 bytes at a time
        static_assert((256u * RST * sizeof(Cnt)) % 16u == 0, "whole 16-byte stores");
        uint4 *const zA = reinterpret_cast<uint4 *>(cntA), *const zB = reinterpret_cast<uint4 *>(cntB);
        for (uint32_t i = tid; i < 256u * RST * (uint32_t)sizeof(Cnt) / 16u; i += LZ2_THREADS) { zA[i] = make_uint4(0, 0, 0, 0); zB[i] = make_uint4(0, 0, 0, 0); }
    }

    bool viol = false;
    // ---- this part's positions, in time order: picked out of the block's part map — seven bit planes, bit p of plane b = bit b
    //      of the part of position p (partmap_planes.h, written by the partition).  Thread t looks at positions [128 t, 128 t + 128)
    //      — one 16-byte load per plane, a wave reads 1 KiB contiguous of each — and a position is this part's where all seven
    //      bits equal the part number's: at most 13 logic ops per 32 positions (rounds 4 to 19: a byte per position and an exact
    //      SWAR zero-byte test per dword, ~350 VALU per thread).  A prefix sum over the threads gives its place,
    //      and it writes its positions there in ascending order: a stable compaction without a single atomic.  (Round 3 read a
    //      list the partition had sorted: item -> list -> words was a chain of three dependent global round trips, 26 % of this
    //      kernel.)
    {
        constexpr uint32_t BPT = LZ_MAX_BLOCK / LZ2_THREADS;                // positions per thread
        static_assert(BPT == 128u, "four dwords of every plane per thread: one 16-byte load each, four match dwords");
        const uint4 *pm = reinterpret_cast<const uint4 *>(sc.partmap + (size_t)lb * (PMP_BLOCK_BYTES / 4u)) + tid;
        // the loads first, all seven; what stays alive across the prefix sum is one match bit per position: four registers
        uint32_t bm[4];
        {
            uint32_t pl[PMP_PLANES][4];
#pragma unroll
            for (uint32_t q = 0; q < PMP_PLANES; ++q) {
                const uint4 v = pm[q * (PMP_PLANE_BYTES / 16u)];
                pl[q][0] = v.x; pl[q][1] = v.y; pl[q][2] = v.z; pl[q][3] = v.w;
            }
            pmp_match_bits(pl, part, bm);
        }
        const uint32_t mine = (uint32_t)(__popc(bm[0]) + __popc(bm[1]) + __popc(bm[2]) + __popc(bm[3]));
        __shared__ uint32_t s_scanp[LZ2_NWAVES + 2];
        uint32_t total_m;
        uint32_t at = block_exclusive_scan<uint32_t>(mine, OpAddU32(), 0u, s_scanp, &total_m);
        (void)total_m;                                                      // == m: the partition counted the same bytes
        const uint32_t p0 = (uint32_t)tid * BPT;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            uint32_t z = bm[k];
            while (z) {
                const uint32_t bpos = (uint32_t)__builtin_ctz(z);
                z &= z - 1u;
                if (at < CAP) s_pos[at] = (uint16_t)(p0 + 32u * k + bpos);
                ++at;
            }
        }
    }
    __syncthreads();
    // ---- gather: the words (4 unaligned bytes each from the block; bytes past the block end read as zero, the parity
    //      definition of the reference's over-read)
    {
        // all of a thread's words first, then the hashing: the loads are in flight together instead of one entry at a time
        constexpr uint32_t GCH = CAP / LZ2_THREADS;
        uint32_t gp[GCH], glo[GCH], ghi[GCH];
        // (a descriptor's block starts anywhere: the two words are the ALIGNED ones around src + p, both inside [src, src + nblk)
        //  rounded out to aligned words, and the shift below is the address's own — no byte-wise gather for an odd item)
        const bool aligned = DESC || (((uintptr_t)src) & 3u) == 0;
#pragma unroll
        for (uint32_t c = 0; c < GCH; ++c) { const uint32_t j = tid + c * LZ2_THREADS; gp[c] = j < m ? (uint32_t)s_pos[j] : 0u; if (j < m) plist[j] = (uint16_t)gp[c]; }
#pragma unroll
        for (uint32_t c = 0; c < GCH; ++c) {
            const uint32_t j = tid + c * LZ2_THREADS, p = gp[c];
            glo[c] = 0; ghi[c] = 0;
            if (j < m) {
                if (p + 8 <= nblk && aligned) {
                    const uintptr_t a = (uintptr_t)(src + p) & ~(uintptr_t)3;
                    glo[c] = *reinterpret_cast<const uint32_t *>(a);
                    ghi[c] = *reinterpret_cast<const uint32_t *>(a + 4);
                } else {
                    // bytes past the block end read as zero (the parity definition of the reference's over-read)
                    uint32_t w = 0;
                    for (uint32_t k = 0; k < 4 && p + k < nblk; ++k) w |= (uint32_t)src[p + k] << (8 * k);
                    glo[c] = w;
                }
            }
        }
        __syncthreads();                                    // the counters are zero (the loads above are in flight across it)
#pragma unroll
        for (uint32_t c = 0; c < GCH; ++c) {
            const uint32_t j = tid + c * LZ2_THREADS, p = gp[c];
            if (j < m) {
                uint32_t w = glo[c];
                if (p + 8 <= nblk && aligned) {
                    const uint32_t sh = ((uint32_t)((uintptr_t)(src + p) & 3u)) * 8u;
                    if (sh) w = (glo[c] >> sh) | (ghi[c] << (32u - sh));
                }
                // every step of the reference hash is invertible (odd multipliers, rotations, xor-shifts), so the mixed
                // value identifies the word: keep it instead of the word — the home is a mask away, equality is equality
                const uint32_t mx = lz_mix32(w);
                s_word[j] = mx;
                radix_cnt_add(cntA, (((((mx & Tmask) - base) & Tmask) - plo_) & 255u) * RST + __umulhi(j, seg_inv), 1u);
            }
        }
    }
    for (uint32_t i = tid; i < CAP / 32 + 2; i += LZ2_THREADS) { s_bm[i] = 0; s_mix[i] = 0; }
    if (tid == 0) { s_zslot = ~0u; s_zgid = ~0u; s_nbigl = 0; }
    __syncthreads();
    auto homep = [&](uint32_t j) -> uint32_t { return ((s_word[j] & Tmask) - base) & Tmask; };
    // (a part's positions are in time order by construction — a compaction, no sort: the order checks start with the home sort)
    LZ2_TICK(0);

    // ---- sort time indices by home', stable
    const uint32_t arank = P.flags & (LZP_ARANK | LZP_BREAK);
    auto keyp = [&](uint32_t j) -> uint32_t { return homep(j) - plo_; };
    uint16_t *srt = s_j0;                                   // where the home order ends up
    if (three) {
        radix_pass<LZ2_NWAVES, 8, uint32_t>(m, s_cnt, [&](uint32_t i) { return i; },
            [&](uint32_t e) { return keyp(e) & 255u; }, [&](uint32_t d, uint32_t e) { s_j0[d] = (uint16_t)e; }, arank, nullptr, true,
            [&](uint32_t d, uint32_t e) { radix_cnt_add(cntB, ((keyp(e) >> 8) & 255u) * RST + __umulhi(d, seg_inv), 1u); });
        for (uint32_t i = tid; i < 256u * RST; i += LZ2_THREADS) cntA[i] = 0;         // (the next pass opens with a barrier)
        radix_pass<LZ2_NWAVES, 8, uint32_t>(m, s_cntB, [&](uint32_t i) { return (uint32_t)s_j0[i]; },
            [&](uint32_t e) { return (keyp(e) >> 8) & 255u; }, [&](uint32_t d, uint32_t e) { s_j1[d] = (uint16_t)e; }, arank, nullptr, true,
            [&](uint32_t d, uint32_t e) { radix_cnt_add(cntA, ((keyp(e) >> 16) & 255u) * RST + __umulhi(d, seg_inv), 1u); });
        radix_pass<LZ2_NWAVES, 8, uint32_t>(m, s_cnt, [&](uint32_t i) { return (uint32_t)s_j1[i]; },
            [&](uint32_t e) { return (keyp(e) >> 16) & 255u; }, [&](uint32_t d, uint32_t e) { s_j0[d] = (uint16_t)e; }, arank, nullptr, true);
    } else {
        radix_pass<LZ2_NWAVES, 8, uint32_t>(m, s_cnt, [&](uint32_t i) { return i; },
            [&](uint32_t e) { return keyp(e) & 255u; }, [&](uint32_t d, uint32_t e) { s_j1[d] = (uint16_t)e; }, arank, LZ2_DBG, true,
            [&](uint32_t d, uint32_t e) { radix_cnt_add(cntB, ((keyp(e) >> 8) & 255u) * RST + __umulhi(d, seg_inv), 1u); });
        radix_pass<LZ2_NWAVES, 8, uint32_t>(m, s_cntB, [&](uint32_t i) { return (uint32_t)s_j1[i]; },
            [&](uint32_t e) { return (keyp(e) >> 8) & 255u; }, [&](uint32_t d, uint32_t e) { s_j0[d] = (uint16_t)e; }, arank, LZ2_DBG, true);
    }
    (void)srt;

    LZ2_TICK(1);
    // ---- parking sweep over the sorted order: CH consecutive entries per thread
    constexpr uint32_t CH = CAP / LZ2_THREADS;
    const uint32_t k0 = tid * CH, k1 = (k0 + CH < m) ? k0 + CH : m;
    {
        // the thread's CH entries live in registers for the three passes below (time index, mixed word, home')
        uint32_t rj[CH], rw[CH]; int32_t rh[CH];
        int32_t mx = INT32_MIN;
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c) {
            const uint32_t k = k0 + c;
            rj[c] = 0; rw[c] = 0; rh[c] = 0;
            if (k < k1) {
                rj[c] = s_j0[k]; rw[c] = s_word[rj[c]]; rh[c] = (int32_t)(((rw[c] & Tmask) - base) & Tmask);
                const int32_t g = rh[c] - (int32_t)k;
                mx = g > mx ? g : mx;
            }
        }
        int32_t gmax_total;
        const int32_t premax = block_exclusive_scan<int32_t>(mx, OpMaxI32(), INT32_MIN, s_i32, &gmax_total);
        int32_t prev_h0 = 0; uint32_t prev_j = 0;
        if (k0 > 0 && k0 < m) { prev_j = s_j0[k0 - 1]; prev_h0 = (int32_t)homep(prev_j); }
        uint32_t nheads = 0; int32_t lasthead = -1, lastrun = -1;
        {
            int32_t run = premax, prev_h = prev_h0;
#pragma unroll
            for (uint32_t c = 0; c < CH; ++c) {
                const uint32_t k = k0 + c;
                if (k < k1) {
                    const int32_t h = rh[c], g = h - (int32_t)k;
                    const bool head = (k == 0) || (g >= run);
                    run = g > run ? g : run;
                    if (head) { ++nheads; lasthead = (int32_t)k; }
                    if (k == 0 || h != prev_h) lastrun = (int32_t)k;
                    prev_h = h;
                }
            }
        }
        // one scan for three carries: heads so far (sum), last head index + 1 (max), last home-run start + 1 (max)
        struct OpHeads {
            __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
                const uint64_t s0 = (a & 0xFFFFu) + (b & 0xFFFFu);
                const uint64_t a1 = (a >> 16) & 0xFFFFu, b1 = (b >> 16) & 0xFFFFu, a2 = (a >> 32) & 0xFFFFu, b2 = (b >> 32) & 0xFFFFu;
                return s0 | ((a1 > b1 ? a1 : b1) << 16) | ((a2 > b2 ? a2 : b2) << 32);
            }
        };
        __shared__ uint64_t s_u64[18];
        uint64_t tot3;
        const uint64_t pre3 = block_exclusive_scan<uint64_t>((uint64_t)nheads | ((uint64_t)(lasthead + 1) << 16) | ((uint64_t)(lastrun + 1) << 32),
                                                            OpHeads(), 0ull, s_u64, &tot3);
        const uint32_t gid_base = (uint32_t)(pre3 & 0xFFFFu), total_heads = (uint32_t)(tot3 & 0xFFFFu);
        const int32_t gs_carry = (int32_t)((pre3 >> 16) & 0xFFFFu) - 1, hs_carry = (int32_t)((pre3 >> 32) & 0xFFFFu) - 1;
        if (tid == 0) s_ngroups = total_heads;
        int32_t run = premax, prev_h = prev_h0;
        uint32_t cur_gs = 0, cur_gid = gid_base; int32_t cur_base = 0;
        uint32_t cur_hs = 0, hs_word = 0, hs_j = 0;
        if (k0 < m) {
            if (gs_carry >= 0) { cur_gs = (uint32_t)gs_carry; cur_base = (int32_t)homep(s_j0[cur_gs]); cur_gid = gid_base - 1u; }
            if (hs_carry >= 0) { cur_hs = (uint32_t)hs_carry; hs_j = s_j0[cur_hs]; hs_word = s_word[hs_j]; }
        }
        uint32_t seen = 0;
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c) {
            const uint32_t k = k0 + c;
            if (k < k1) {
                const uint32_t j = rj[c];
                const int32_t h = rh[c], g = h - (int32_t)k;
                const bool head = (k == 0) || (g >= run);
                run = g > run ? g : run;
                const uint32_t w = rw[c];
                // ... and the home sort must have left (home, time) ascending: the check of every pass at once
                if (k > 0 && (h < prev_h || (h == prev_h && j < prev_j))) viol = true;
                prev_j = j;
                if (head) {
                    cur_gs = k; cur_base = h; cur_gid = gid_base + seen; ++seen;
                    // cursor of the cluster for the one-pass placement below: its first index in replay order (a cluster
                    // keeps its index range in the home order and in the (cluster, time) order)
                    reinterpret_cast<uint16_t *>(&s_cnt[0][0])[cur_gid] = (uint16_t)k;
                }
                uint32_t id;
                if (k == 0 || h != prev_h) { cur_hs = k; hs_word = w; hs_j = j; id = j; }
                else if (w == hs_word) id = hs_j;
                else {                                      // two different words share a home bucket: rare
                    id = j;
                    for (uint32_t kk = cur_hs + 1; kk < k; ++kk) { const uint32_t j2 = s_j0[kk]; if (s_word[j2] == w) { id = j2; break; } }
                    atomicOr(&s_mix[cur_gid >> 5], 1u << (cur_gid & 31u));
                }
                prev_h = h;
                s_g[j] = (uint16_t)cur_gid;
                s_r[j] = (uint16_t)(cur_gs + (uint32_t)(h - cur_base));
                // a cluster whose entries do not all share one home needs its (home, time) order re-sorted by time below;
                // the others (nearly all) are in time order as they stand.  s_bm is free until the replay.
                if (h != cur_base) {
                    if (arank & LZP_ARANK) atomicOr(&s_bm[cur_gid >> 5], 1u << (cur_gid & 31u));
                    atomicOr(&s_mix[cur_gid >> 5], 1u << (cur_gid & 31u));
                }
                // the word's identity is the POSITION of its first occurrence in the block (the home order is stable in
                // time).  While nothing of a cluster has been evicted that position is also what find() returns: the first
                // copy sits at the lowest slot of the word and every slot between the home and it stays occupied.
                s_pid[j] = s_pos[id];
            }
        }
    }
    if (viol) { lz_order_violation(P); viol = false; }
    __syncthreads();
    if (!P.deflate && W >= nblk) {
        // lz77 flavour with a window that covers the block (the 64 KiB-window build): nothing is ever retired, find() never
        // stops at the table end, and the spurious clear of bucket 0 happens at the last insertion — so find() is the
        // first occurrence of the word for EVERY position (2.3 above): no clusters, no second sort, no replay.
        uint16_t *cout = sc.cand + (size_t)lb * LZ_MAX_BLOCK + pstart;
        for (uint32_t j = tid; j < m; j += LZ2_THREADS) { const uint32_t id = s_pid[j]; cout[j] = (id != s_pos[j]) ? (uint16_t)id : (uint16_t)LZ_NONE16; }
        return;
    }
    // bucket 0 (= bucket T on deflate's ring) sits at home' Z: the cluster that covers it gets the one-time
    // spurious clear and, for deflate, the point where find() stops instead of wrapping
    if (tid == 0) {
        const uint32_t Z = (0u - base) & Tmask;
        const uint32_t plo = mt->part_lo[part];
        const uint32_t phi = (part + 1 < mt->nparts) ? mt->part_lo[part + 1] : T;
        if (Z >= plo && (Z < phi || phi == T)) {
            // last sorted entry with home' <= Z
            int32_t lo = -1, hi = (int32_t)m - 1;
            while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (homep(s_j0[mid]) <= Z) lo = mid; else hi = mid - 1; }
            if (lo >= 0) {
                const uint32_t j = s_j0[lo], gid = s_g[j];
                const uint32_t slot = (uint32_t)s_r[j] + (Z - homep(j));
                // last sorted index of that cluster (cluster numbers are non-decreasing along the order)
                int32_t a = lo, b = (int32_t)m - 1;
                while (a < b) { const int32_t mid = (a + b + 1) >> 1; if (s_g[s_j0[mid]] == gid) a = mid; else b = mid - 1; }
                if (slot <= (uint32_t)a) { s_zslot = slot; s_zgid = gid; }
            }
        }
    }
    __syncthreads();

    LZ2_TICK(2);
    // ---- sort time indices by cluster number (they start in time order): identity -> j0 -> j1
    //      (cluster numbers are < CAP <= 4096: two 6-bit passes, fewer ballots and a shorter offset scan than 8 + 8)
    static_assert(CAP <= 8192, "cluster numbers must fit 13 bits");
    constexpr int GB2 = CAP > 4096 ? 7 : 6;          // bits of the second cluster-number pass
    static_assert(2 * CAP <= sizeof(s_cnt), "the cluster cursors live in the radix counters");
    if (arank & LZP_ARANK) {
        // ONE pass, no counting: the sweep left every cluster's first replay index as a 16-bit cursor; an entry's place is its
        // cluster's cursor, post-incremented — in TIME order.  Time order needs every cursor to be advanced by one wave only
        // (a wave's LDS instructions execute in order, and the lanes of one returning add are served in lane order: the
        // property radix_pass uses), so wave w takes the clusters whose cursor PAIR (two 16-bit cursors share a dword, the
        // unit of an LDS atomic) has number = w modulo the wave count, and every wave walks the whole time-ordered list.
        // Replaces two 6-bit radix passes (count, scan, scatter each): 20 k -> ~8 k cycles per part.
        // Only clusters with MORE THAN ONE HOME need it (a cluster of one home is in time order already: the home sort is stable);
        // their entries are compacted first, time order kept, so the eight waves walk a short list instead of the whole part.
        uint32_t *cur32 = reinterpret_cast<uint32_t *>(&s_cnt[0][0]);
        const uint32_t wv = (uint32_t)tid >> 6, ln = (uint32_t)tid & 63u;
        auto multi = [&](uint32_t g) -> bool { return (s_bm[g >> 5] >> (g & 31u)) & 1u; };
        for (uint32_t k = k0; k < k1; ++k) { const uint32_t j = s_j0[k]; if (!multi(s_g[j])) s_j1[k] = (uint16_t)j; }
        __syncthreads();                                     // (s_j0 is dead now: it takes the compacted list)
        uint32_t nm;
        {
            uint32_t mine[CH], cnt = 0;
#pragma unroll
            for (uint32_t c = 0; c < CH; ++c) { const uint32_t j = k0 + c; mine[c] = (j < m && multi(s_g[j])) ? 1u : 0u; cnt += mine[c]; }
            uint32_t at = block_exclusive_scan<uint32_t>(cnt, OpAddU32(), 0u, reinterpret_cast<uint32_t *>(s_i32), &nm);
#pragma unroll
            for (uint32_t c = 0; c < CH; ++c) if (mine[c]) s_j0[at++] = (uint16_t)(k0 + c);
        }
        __syncthreads();
        for (uint32_t x0 = 0; x0 < nm; x0 += 256u) {
            uint32_t jj[4], gg[4], old[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) { const uint32_t x = x0 + 64u * u + ln; jj[u] = x < nm ? (uint32_t)s_j0[x] : 0u; gg[u] = x < nm ? (uint32_t)s_g[jj[u]] : 0xFFFFFFFFu; }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                old[u] = 0;
                if (gg[u] != 0xFFFFFFFFu && ((gg[u] >> 1) % (uint32_t)LZ2_NWAVES) == wv) old[u] = atomicAdd(&cur32[gg[u] >> 1], 1u << (16u * (gg[u] & 1u)));
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                if (gg[u] != 0xFFFFFFFFu && ((gg[u] >> 1) % (uint32_t)LZ2_NWAVES) == wv) s_j1[(old[u] >> (16u * (gg[u] & 1u))) & 0xFFFFu] = (uint16_t)jj[u];
        }
        __syncthreads();
        for (uint32_t i = tid; i < CAP / 32 + 2; i += LZ2_THREADS) s_bm[i] = 0;     // back to the replay's empty bitmap (barriers follow)
    } else {
        radix_pass<LZ2_NWAVES, 6, uint32_t>(m, s_cnt, [&](uint32_t i) { return i; },
            [&](uint32_t e) { return (uint32_t)s_g[e] & 63u; }, [&](uint32_t d, uint32_t e) { s_j0[d] = (uint16_t)e; }, arank);
        radix_pass<LZ2_NWAVES, GB2, uint32_t>(m, s_cnt, [&](uint32_t i) { return (uint32_t)s_j0[i]; },
            [&](uint32_t e) { return (uint32_t)s_g[e] >> 6; }, [&](uint32_t d, uint32_t e) { s_j1[d] = (uint16_t)e; }, arank);
    }

    LZ2_TICK(3);
    // ---- permute into replay order (cluster, time).  e_pos / e_rs overlay the dead word array.
    uint16_t *e_pos = reinterpret_cast<uint16_t *>(s_word);
    uint16_t *e_rs = e_pos + CAP;
    uint16_t *e_pid = s_j0;
    uint32_t regs[CH][3];
    for (uint32_t c = 0; c < CH; ++c) {
        const uint32_t i = tid + c * (uint32_t)LZ2_THREADS;
        if (i < m) {
            const uint32_t j = s_j1[i];
            const bool head = (i == 0) || (s_g[j] != s_g[s_j1[i - 1]]);
            if (i > 0) {                                       // the (cluster, time) order, however it was made
                const uint32_t jp = s_j1[i - 1], gp = s_g[jp], gj = s_g[j];
                if (gp > gj || (gp == gj && jp > j)) viol = true;
            }
            regs[c][0] = s_pos[j];
            regs[c][1] = (uint32_t)s_r[j] | (head ? RS_HEAD : 0u);
            regs[c][2] = (uint32_t)s_pid[j] | ((uint32_t)s_g[j] << 16);
        }
    }
    if (viol) lz_order_violation(P);
    __syncthreads();
    uint16_t *occ = s_g;                    // cluster numbers are dead from here on, except the one remembered in s_zgid
    uint16_t *cand_i = s_r;
    __shared__ uint16_t s_zhead;            // replay index of the head of the cluster that covers bucket 0
    if (tid == 0) { s_zhead = 0xFFFF; s_gstart[s_ngroups] = (uint16_t)m; }
    __syncthreads();
    for (uint32_t c = 0; c < CH; ++c) {
        const uint32_t i = tid + c * (uint32_t)LZ2_THREADS;
        if (i < m) {
            e_pos[i] = (uint16_t)regs[c][0]; e_rs[i] = (uint16_t)regs[c][1]; e_pid[i] = (uint16_t)regs[c][2];
            if (regs[c][1] & RS_HEAD) {
                s_gstart[regs[c][2] >> 16] = (uint16_t)i;
                if ((regs[c][2] >> 16) == s_zgid) s_zhead = (uint16_t)i;
            }
        }
    }
    __syncthreads();

    LZ2_TICK(4);
    __shared__ uint32_t s_cls[LZ2_NCLASS], s_clsbase[LZ2_NCLASS], s_ent, s_entbase;
    uint32_t my_rank[((CAP / LZ2_BIG) + LZ2_THREADS - 1) / LZ2_THREADS], my_dst[((CAP / LZ2_BIG) + LZ2_THREADS - 1) / LZ2_THREADS];
    uint32_t nbig = 0;
    // ---- replay.  Clusters below LZ2_BIG entries: one lane each, lanes sorted by cluster size so that the
    //      64 lanes of a wave run the same number of steps.  Larger clusters are exported by size class.
    {
        // cluster heads -> compact list (order irrelevant), sizes from the next head
        __shared__ uint32_t s_ncl, s_bin[LZ2_BIG + 1], s_nquiet;
        if (tid == 0) { s_ncl = 0; s_nquiet = 0; s_ent = 0; }
        if (tid < (int)LZ2_NCLASS) s_cls[tid] = 0;
        if (tid <= (int)LZ2_BIG) s_bin[tid] = 0;
        __syncthreads();
        uint16_t *c_start = s_j1 + 0;                        // (s_j1 is still needed: cand back to time order) -> use s_pos, dead now
        c_start = s_pos;                                     // [<= m/2] start of each lane-replayed cluster, bucketed by size
        uint32_t my_s[CH], my_n[CH];
        for (uint32_t c = 0; c < CH; ++c) {
            const uint32_t i = tid + c * (uint32_t)LZ2_THREADS;
            my_n[c] = 0; my_s[c] = i;
            if (i < m && (e_rs[i] & RS_HEAD)) {
                const uint32_t g_ = regs[c][2] >> 16;
                const uint32_t e = s_gstart[g_ + 1];                      // clusters are contiguous and in cluster-number order
                const uint32_t size = e - i;
                my_n[c] = size;
                // a cluster whose entries all lie within one window never evicts: no replay, find() = first occurrence
                if (size == 1) cand_i[i] = LZ_NONE16;
                else if (!((s_mix[g_ >> 5] >> (g_ & 31u)) & 1u) && i != s_zhead) my_n[c] = 0;     // ONE word: the closed form below, no replay
                else if (size < LZ2_BIG) atomicAdd(&s_bin[size], 1u);          // (replay_small notices a quiet cluster itself)
                else if ((uint32_t)e_pos[e - 1] <= (uint32_t)e_pos[i] + W && i != s_zhead) { const uint32_t q = atomicAdd(&s_nquiet, 1u); s_quiet[2 * q] = (uint16_t)i; s_quiet[2 * q + 1] = (uint16_t)e; }
                else {
                    const uint32_t q = atomicAdd(&s_nbigl, 1u);
                    if (q < (CAP / LZ2_BIG)) { s_big[3 * q] = i; s_big[3 * q + 1] = e; }
                }
            }
        }
        __syncthreads();
        LZ2_TICK(11);
        if (tid == 0) {                                      // bucket offsets, largest size first
            uint32_t run = 0;
            for (int sz = (int)LZ2_BIG - 1; sz >= 2; --sz) { const uint32_t t = s_bin[sz]; s_bin[sz] = run; run += t; }
            s_ncl = run;
        }
        __syncthreads();
        for (uint32_t c = 0; c < CH; ++c)
            if (my_n[c] >= 2 && my_n[c] < LZ2_BIG) c_start[atomicAdd(&s_bin[my_n[c]], 1u)] = (uint16_t)my_s[c];
        __syncthreads();
        LZ2_TICK(12);
        // reserve the output space of the clusters this part exports NOW — ONE global atomic per part and class (the class
        // counters are shared by every workgroup of the batch), local ranks first in LDS — so that the round trips of
        // those atomics pass while the lanes replay
        nbig = s_nbigl < (CAP / LZ2_BIG) ? s_nbigl : (CAP / LZ2_BIG);          // CAP / LZ2_BIG clusters at most
        {
            uint32_t it = 0;
            for (uint32_t q = tid; q < nbig; q += LZ2_THREADS, ++it) {
                const uint32_t cnt = s_big[3 * q + 1] - s_big[3 * q];
                const uint32_t cls = lz2_class_of(cnt, sc.wave_min);
                my_rank[it] = atomicAdd(&s_cls[cls], 1u);
                my_dst[it] = atomicAdd(&s_ent, LZ2_ALIGN8(cnt));        // every cluster starts on an 8-entry boundary
            }
        }
        __syncthreads();
        // The returns of these global atomics (every part of the batch adds to the same eight class counters: ~12 k cycles
        // under that contention, measured) are only needed by the export below: they stay in a register until the lane
        // replay is through, so the wave that issues them does not stall in front of its share of the replay.
        uint32_t pending_base = 0;
        const bool want_cls = tid < (int)LZ2_NCLASS && s_cls[tid], want_ent = tid == 32 && s_ent;
        // (ONE returning atomic instruction with a per-lane address: on a uniform address the compiler's wave-aggregated
        // form reads the result back with v_readfirstlane at once — wave 0 then stood ~13 k cycles in front of its replay)
        if (want_cls || want_ent) {
            uint32_t *ap = want_ent ? &mt->nbig_entries : &sc.big_count[tid & (int)(LZ2_NCLASS - 1u)];
            pending_base = atomicAdd(ap, want_ent ? s_ent : s_cls[tid & (int)(LZ2_NCLASS - 1u)]);
        }
        if (want_ent) atomicAdd(&mt->nbig, nbig);
        for (uint32_t q = tid >> 6; q < s_nquiet; q += LZ2_NWAVES)
            for (uint32_t k = (uint32_t)s_quiet[2 * q] + (tid & 63u); k < s_quiet[2 * q + 1]; k += 64) {
                const uint32_t id = e_pid[k];
                cand_i[k] = (id != e_pos[k]) ? (uint16_t)id : (uint16_t)LZ_NONE16;
            }
        const uint32_t ncl = s_ncl;
        LZ2_TICK(13);
        if (LZ2_DBG && tid == 0) { atomicAdd((unsigned long long *)&LZ2_DBG[23], (unsigned long long)ncl); atomicAdd((unsigned long long *)&LZ2_DBG[24], (unsigned long long)nbig);
                                  atomicAdd((unsigned long long *)&LZ2_DBG[25], (unsigned long long)s_ent); atomicAdd((unsigned long long *)&LZ2_DBG[26], (unsigned long long)s_nquiet);
                                  atomicAdd((unsigned long long *)&LZ2_DBG[27], (unsigned long long)m); atomicAdd((unsigned long long *)&LZ2_DBG[28], (unsigned long long)s_ngroups); }
        // ---- clusters of ONE word (one home, every entry the same word: most clusters of a text) have a closed form.  find()
        //      for that word only ever looks at the home slot: it holds the "anchor", the copy that was inserted when the slot
        //      was free — the first entry, then, once the anchor has been retired (lz77.c:70-76: its position + W < p), the
        //      next entry, which itself finds the slot empty (nothing) and takes it.  a(0) = first entry, a(k+1) = first entry
        //      after a(k) + W: at most block / W anchors, each a binary search in the cluster's time-ordered positions.  Every
        //      entry on its own, no table, no order: neither the lane replay nor an export (k_lz_emulate_giant uses the same
        //      form for giant clusters).  The cluster that covers bucket 0 / T keeps the general path.
        for (uint32_t c = 0; c < CH; ++c) {
            const uint32_t i = tid + c * (uint32_t)LZ2_THREADS;
            if (i >= m) continue;
            const uint32_t g_ = regs[c][2] >> 16;
            if ((s_mix[g_ >> 5] >> (g_ & 31u)) & 1u) continue;
            const uint32_t s = s_gstart[g_];
            if (s == s_zhead || s_gstart[g_ + 1] - s < 2u) continue;
            const uint32_t p = regs[c][0];
            uint32_t a = e_pos[s], lo = s + 1u;
            while (a + W < p) {                                           // (e_pos[i] = p is beyond a + W: the search ends at i at the latest)
                uint32_t hi = i;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)e_pos[mid] > a + W) hi = mid; else lo = mid + 1u; }
                a = e_pos[lo]; ++lo;
            }
            cand_i[i] = (a == p) ? (uint16_t)LZ_NONE16 : (uint16_t)a;
        }
        for (uint32_t q = tid; q < ncl; q += LZ2_THREADS) {
            const uint32_t s = c_start[q];
            uint32_t e = s + 1;
            while (e < m && !(e_rs[e] & RS_HEAD)) ++e;
            const bool zc = (s == s_zhead);
            if (zc) replay_small(e_pos, e_rs, e_pid, occ, s_bm, s, e, W, s_zslot, P.deflate ? s_zslot : ~0u, cand_i);
            else if (LZ2_BIG > 8u && e - s >= 8u) replay_small_reg<uint64_t>(e_pos, e_rs, e_pid, s, e, W, cand_i);
            else replay_small_reg<uint32_t>(e_pos, e_rs, e_pid, s, e, W, cand_i);
        }
        if (want_cls) s_clsbase[tid] = pending_base;
        if (want_ent) s_entbase = pending_base;
    }
    __syncthreads();
    LZ2_TICK(5);
    // ---- export the larger clusters (cooperatively, coalesced); their space was reserved before the lane replay
    {
        uint32_t it = 0;
        for (uint32_t q = tid; q < nbig; q += LZ2_THREADS, ++it) {
            const uint32_t s = s_big[3 * q], e = s_big[3 * q + 1], cnt = e - s;
            const uint32_t cls = lz2_class_of(cnt, sc.wave_min);
            const uint32_t dst = s_entbase + my_dst[it];
            s_big[3 * q + 2] = dst;
            Lz2BigDesc d;
            d.block = lb; d.start = dst; d.count = cnt;
            const bool zc = (s == s_zhead);
            d.anom = zc ? s_zslot - s : ~0u;
            d.limit = (zc && P.deflate) ? s_zslot - s : ~0u;
            d.pad[0] = pstart; d.pad[1] = d.pad[2] = 0;
            sc.desc[cls][s_clsbase[cls] + my_rank[it]] = d;
        }
    }
    __syncthreads();
    for (uint32_t b = tid >> 6; b < nbig; b += LZ2_NWAVES) {          // a wave per exported cluster
        const uint32_t s = s_big[3 * b], e = s_big[3 * b + 1], dst = s_big[3 * b + 2];
        uint16_t *bp = sc.bigpos + (size_t)lb * LZ2_BIG_STRIDE + dst;
        uint16_t *br = sc.bigrs + (size_t)lb * LZ2_BIG_STRIDE + dst;
        uint16_t *bi = sc.bigpid + (size_t)lb * LZ2_BIG_STRIDE + dst;
        for (uint32_t i = s + (tid & 63); i < e; i += 64) {
            cand_i[i] = e_pos[i];                                // pending (lz2.h)
            bp[i - s] = e_pos[i];
            br[i - s] = (uint16_t)((e_rs[i] & RS_MASK) - s);    // home slot relative to the cluster
            bi[i - s] = e_pid[i];
        }
        uint16_t *bc = sc.bigcand + (size_t)lb * LZ2_BIG_STRIDE + dst;
        for (uint32_t k = (e - s) + (tid & 63); k < LZ2_ALIGN8(e - s); k += 64) { bp[k] = 0; bc[k] = 0; }    // pads: skipped by every consumer
    }
    // ---- cand back to time order and out (coalesced)
    uint16_t *cand_j = s_pid;
    __syncthreads();
    for (uint32_t i = tid; i < m; i += LZ2_THREADS) cand_j[s_j1[i]] = cand_i[i];
    __syncthreads();
    uint16_t *cout = sc.cand + (size_t)lb * LZ_MAX_BLOCK + pstart;
    for (uint32_t j = tid; j < m; j += LZ2_THREADS) cout[j] = cand_j[j];
    LZ2_TICK(6);
    if (LZ2_DBG && tid == 0) atomicAdd((unsigned long long *)&LZ2_DBG[15], 1ull);
}


// The grid covers the worst case (32 parts per block) and the listed parts come first; a surplus workgroup reads the
// count and leaves.  Measured (round 2, same box, 10^9 bytes): a persistent grid of 2 workgroups per CU pulling parts
// off a cursor made this kernel 30.3 -> 51 ms per GB on its own — the loop keeps every scratch pointer live across
// the whole body: 84 -> 176 VGPRs, one workgroup per CU instead of two (forced back to 128 VGPRs it spills) — and the
// hardware dispatcher already IS a dynamic scheduler: ~13 k empty workgroups per batch cost nothing measurable.
// XCD-aware order: workgroup ids go round the 8 XCDs (each with its own L2), the work list holds a block's parts one
// after the other — so give every XCD a CONTIGUOUS eighth of the list: the ~33 parts of a block then gather their
// words from one L2 instead of pulling the block's 64 KiB into all eight (HBM fetch of this kernel: profiles/).
// __launch_bounds__(512, 8): eight waves per SIMD = four workgroups per CU, together with the LDS of lz2_find_part<2048>
// (< 40 KiB): registers above 64 VGPRs / 80 SGPRs would cap the occupancy below that (tests/test_find_budget.py)
template <bool DESC>
__device__ __forceinline__ void lz2_find_listed(const uint8_t *__restrict__ in, uint64_t n_total, const LzP &P, const Lz2Scratch &sc, uint64_t block0)
{
    // the grid is a multiple of 8 (lz2_stage_find) and takes the first gridDim.x listed parts; what a batch lists beyond it
    // (more than LZ2_GRID_PARTS parts per block on average: not seen on any corpus) is k_lz2_find_wide's
    const uint32_t listed = *sc.work_count, nwork = listed < gridDim.x ? listed : gridDim.x;
    const uint32_t cpx = (nwork + 7u) >> 3, item_idx = (blockIdx.x & 7u) * cpx + (blockIdx.x >> 3);
    if ((blockIdx.x >> 3) >= cpx || item_idx >= nwork) return;
    lz2_find_part<LZ2_CAP_S, DESC>(in, n_total, P, sc, block0, sc.work[item_idx]);
}
// (two plain kernels, not a kernel template: tests/test_find_budget.py finds the budgeted kernel by its name)
__global__ __launch_bounds__(LZ2_THREADS, 8)
void k_lz2_find(const uint8_t *__restrict__ in, uint64_t n_total, LzP P, Lz2Scratch sc, uint64_t block0)
{
    lz2_find_listed<false>(in, n_total, P, sc, block0);
}
// ... and over the batched encoder's descriptor table (`in`: lz_block_src)
__global__ __launch_bounds__(LZ2_THREADS, 8)
void k_lz2_find_desc(const uint8_t *__restrict__ in, uint64_t n_total, LzP P, Lz2Scratch sc, uint64_t block0)
{
    lz2_find_listed<true>(in, n_total, P, sc, block0);
}

// the parts above LZ2_CAP_S entries (rare: listed from the end of the work array backwards): a small grid that loops
template <bool DESC>
__global__ __launch_bounds__(LZ2_THREADS)
void k_lz2_find_wide(const uint8_t *__restrict__ in, uint64_t n_total, LzP P, Lz2Scratch sc, uint64_t block0, uint32_t covered)
{
    // `covered` = what k_lz2_find's grid took from the front list; the rest of that list is done here too (a part of <= LZ2_CAP_S
    // entries fits the wide instance)
    const uint32_t nwide = sc.work_count[1], listed = sc.work_count[0], rest = listed > covered ? listed - covered : 0u;
    for (uint32_t k = blockIdx.x; k < nwide + rest; k += gridDim.x) {
        lz2_find_part<LZ2_CAP, DESC>(in, n_total, P, sc, block0, k < nwide ? sc.work[sc.work_slots - 1u - k] : sc.work[covered + (k - nwide)]);
        __syncthreads();
    }
}

// =============================================================================================
// The insert-only prefix of the wave-class clusters, placed in bulk.  A PLAIN cluster (not the one that covers
// bucket 0 / T) retires nothing before the first entry whose position exceeds pos[0] + W; up to there — `pre` entries — find()
// is the word id (or none for the word's first occurrence) and insert is pure first fit, and a maximal run of
// consecutive entries with the same home r takes the next free slots >= r in order: no dependency from entry to entry.  One wave
// per exported cluster of classes 3, 4 and 5 (128..1024 entries), ahead of the replays and with no LDS: the occupancy bitmap
// (<= 1024 slots) is one register per lane as in WaveBitmap<1>; a step finds the first word with a free bit >= r (ballot), the
// lanes that hold a free bit of it rank themselves (popcount below), and the first min(run, free bits) of them store their
// slot for the run's entries.  A run that outlasts the word goes on in the next step.
// Out: the SLOT of every entry i < pre IN PLACE over bigrs[i] (the home of a placed entry is dead: the replays read one array
// for "slot below pre, home from pre on", and the workspace does not grow), bigcand[i] for i < pre, `pre` in the descriptor's
// pad[1]; a cluster with pre == count is finished and flagged like those of k_lz2_dom / k_lz2_rows.  k_lz2_rows and
// big_replay<.., PRE> rebuild their tables from the slots and start at entry `pre`.
// Reference behaviour emulated: insert_hash_table / find, algorithms/lz77/lz77.c:55-108.
// =============================================================================================
#define LZ2_DOM_DONE 0x80000000u
#ifdef MI_TEST_HOOKS                                       /* lib_test only: [0] clusters started from a precomputed prefix (or finished by it), [1] entries it answered */
__device__ unsigned long long g_lz2_prefix_stats[2];
#define LZ2_PREFIX_COUNT(who, entries) do { if (who) { atomicAdd(&g_lz2_prefix_stats[0], 1ull); atomicAdd(&g_lz2_prefix_stats[1], (unsigned long long)(entries)); } } while (0)
#else
#define LZ2_PREFIX_COUNT(who, entries) do { } while (0)
#endif

__global__ __launch_bounds__(64)
void k_lz2_prefix(LzP P, Lz2Scratch sc)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t W = 1u << P.wbits;
    // the long clusters first (their replays are launched first)
    const uint32_t n4 = sc.big_count[4], n5 = sc.big_count[5], ncl = n4 + n5 + sc.big_count[3];
    auto desc_of = [&](uint32_t c) -> Lz2BigDesc * { return c < n4 ? sc.desc[4] + c : c < n4 + n5 ? sc.desc[5] + (c - n4) : sc.desc[3] + (c - n4 - n5); };
    // the cluster that covers bucket 0 / T keeps pre = 0 and the literal replay
    auto ours = [](const uint4 &d, uint32_t limit) -> bool { return d.z != 0u && d.z <= LZ2_BIG_SMALL && d.w == ~0u && limit == ~0u; };
    // (measured: with the descriptor and the first entries of a wave's next cluster prefetched while it works, the span beside
    // k_lz2_partition stayed at 0.29 ms per launch — the steps below, not the loads, are the time; the prefetch was removed)
    for (uint32_t ci = blockIdx.x; ci < ncl; ci += gridDim.x) {
        Lz2BigDesc *dp = desc_of(ci);
        const uint4 c_a = *reinterpret_cast<const uint4 *>(dp);          // block, start, count, anom
        if (!ours(c_a, dp->limit)) continue;
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)c_a.z);
        const size_t at = (size_t)c_a.x * LZ2_BIG_STRIDE + c_a.y;
        const uint16_t *bp = sc.bigpos + at, *bi = sc.bigpid + at;
        uint16_t *br = sc.bigrs + at, *bc = sc.bigcand + at;
        uint32_t bm = 0;                                                // word `lane` of the occupancy bitmap
        uint32_t pre = 0;
        uint32_t n_pos = 0, n_rs = 0, n_pid = 0;
        if (lane < n) { n_pos = bp[lane]; n_rs = br[lane]; n_pid = bi[lane]; }
        const uint32_t last = RLANE(n_pos, 0) + W;                      // entries up to this position see no retirement
        for (uint32_t i0 = 0; i0 < n; i0 += 64) {
            const uint32_t ii = i0 + lane;
            const uint32_t c_pos = n_pos, c_rs = n_rs, c_pid = n_pid;
            if (ii + 64 < n) { n_pos = bp[ii + 64]; n_rs = br[ii + 64]; n_pid = bi[ii + 64]; }
            // positions ascend: the lanes inside the prefix are the lowest ones
            const uint64_t inside = __ballot(ii < n && c_pos <= last);
            const uint32_t lim = ~inside ? (uint32_t)__builtin_ctzll(~inside) : 64u;
            if (lim == 0u) break;
            if (lane < lim) bc[ii] = (uint16_t)(c_pid == c_pos ? (uint32_t)LZ_NONE16 : c_pid);
            const uint32_t below = (uint32_t)__shfl_up((int)c_rs, 1);
            const uint64_t heads = __ballot(lane < lim && (lane == 0u || c_rs != below));   // first entries of the runs of equal homes
            bool stuck = false;
            for (uint32_t t = 0; t < lim;) {
                const uint32_t r = RLANE(c_rs, t);
                const uint64_t rest = t + 1u < 64u ? heads >> (t + 1u) : 0ull;
                const uint32_t run = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : lim - t;
                const uint32_t rw = r >> 5;
                uint32_t v = bm;
                if (lane < rw) v = 0xFFFFFFFFu; else if (lane == rw) v |= (1u << (r & 31u)) - 1u;
                const uint64_t nz = __ballot(v != 0xFFFFFFFFu);
                if (!nz) { stuck = true; break; }                       // (2048 slots for <= 1024 entries: never)
                const uint32_t wl = (uint32_t)__builtin_ctzll(nz);
                const uint32_t f = ~RLANE(v, wl);                       // the free slots of that word, from r on
                const uint32_t fc = (uint32_t)__popc(f), m = run < fc ? run : fc;
                // lane b stands for bit b of the word: the k-th free bit is the slot of the run's k-th entry
                const uint32_t rank = (uint32_t)__popc(f & ((1u << (lane & 31u)) - 1u));
                const bool mine = lane < 32u && ((f >> (lane & 31u)) & 1u) && rank < m;
                const uint32_t taken = (uint32_t)__ballot(mine);
                if (mine) br[i0 + t + rank] = (uint16_t)((wl << 5) + lane);
                if (lane == wl) bm |= taken;
                t += m;
            }
            if (stuck) { lz_order_violation(P); break; }
            pre += lim;
            if (lim < 64u) break;
        }
        if (lane == 0) {
            dp->pad[1] = pre;
            if (pre == n) dp->count = n | LZ2_DOM_DONE;                 // no replay takes it
        }
        LZ2_PREFIX_COUNT(lane == 0 && pre == n, pre);
    }
}

// =============================================================================================
// wave-per-cluster replay
// =============================================================================================
template <int LDS_ENTRIES, int NW>
__global__ __launch_bounds__(64)
void k_lz2_big(LzP P, Lz2Scratch sc, int large)
{
    __shared__ uint32_t s_occ[LDS_ENTRIES];               // slot -> word id | position << 16 of its occupant
    __shared__ uint16_t s_slot[LDS_ENTRIES];              // entry -> slot (for its eviction)
    const uint32_t lane = threadIdx.x;
    // a launch lasts as long as its longest cluster: the 512..1024-entry class is dispatched before the 128..511 one
    // large: 0 = classes 4 (512..1024 entries) and 5 (128..511) in one launch, 1 = class 6, 2 = class 5 alone, 3 = class 4 alone
    const uint32_t nhi = large == 1 ? sc.big_count[6] : (large == 2 || large == 4) ? 0u : sc.big_count[4],
                   ncl = nhi + ((large == 0 || large == 2) ? sc.big_count[5] : large == 4 ? sc.big_count[3] : 0u);
    const uint32_t W = 1u << P.wbits;
    for (uint32_t ci = blockIdx.x; ci < ncl; ci += gridDim.x) {
        const Lz2BigDesc *dp = large == 1 ? &sc.desc[6][ci] : large == 4 ? &sc.desc[3][ci] : (ci < nhi ? &sc.desc[4][ci] : &sc.desc[5][ci - nhi]);
        const uint32_t d_block = dp->block, d_start = dp->start, n = dp->count;
        if (n & 0x80000000u) continue;                       // k_lz2_dom has replayed it (class 6 only: counts are <= LZ2_CAP otherwise)
        const uint32_t d_anom = dp->anom, d_limit = dp->limit;
        const uint16_t *bp = sc.bigpos + (size_t)d_block * LZ2_BIG_STRIDE + d_start;
        const uint16_t *br = sc.bigrs + (size_t)d_block * LZ2_BIG_STRIDE + d_start;
        const uint16_t *bi = sc.bigpid + (size_t)d_block * LZ2_BIG_STRIDE + d_start;
        uint16_t *bc = sc.bigcand + (size_t)d_block * LZ2_BIG_STRIDE + d_start;
        // (in the non-PLAIN version the first-occurrence shortcut is off: that one cluster per block keeps the literal replay)
        // the occupancy bitmap takes one register per lane and 2048 slots: a cluster is replayed with as few as it needs (every
        // first-fit and every clear walks all of them; the wide class was replayed with four whatever its size)
        const bool plain = d_anom == ~0u && d_limit == ~0u;
        if constexpr (NW == 1) {
            // classes 3, 4, 5: k_lz2_prefix has placed and answered the entries below dp->pad[1] (0: it did not run, or not this cluster)
            __shared__ uint32_t s_stage[64];
            const uint32_t pre = dp->pad[1];
            if (plain && pre != 0u && pre < n) {
                LZ2_PREFIX_COUNT(lane == 0, pre);
                big_replay<LDS_ENTRIES, 1, true, true>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc, pre, s_stage);
                continue;
            }
        }
        if constexpr (NW > 1) {
            if (n <= 2048u) {
                if (plain) big_replay<LDS_ENTRIES, 1, true>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc);
                else big_replay<LDS_ENTRIES, 1, false>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc);
                continue;
            }
            if (n <= 4096u) {
                if (plain) big_replay<LDS_ENTRIES, 2, true>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc);
                else big_replay<LDS_ENTRIES, 2, false>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc);
                continue;
            }
        }
        if (plain) big_replay<LDS_ENTRIES, NW, true>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc);
        else big_replay<LDS_ENTRIES, NW, false>(s_occ, s_slot, lane, W, n, d_anom, d_limit, bp, br, bi, bc);
    }
}

// =============================================================================================
// Exported clusters above 1024 entries (class 6: what the wide finder hands over — a run of one byte value with foreign words inside
// its bucket range) that ONE word dominates: the dominated replay of the fallback pipeline (lz_dom.h: occupancy bits, a ring of the
// live entries' slots, a FIFO of the live foreign entries; runs of the dominant word placed up to 64 entries per wave step) instead
// of the general wave replay with a four-dword bitmap per lane, which took 18 of the "runs" family's 34 ms per 10^8 bytes.  A
// cluster it finishes is flagged in its descriptor; k_lz2_big<LZ2_CAP> skips those and replays the rest (not dominated, given up,
// or covering bucket 0 / T).  Reference behaviour emulated: algorithms/lz77/lz77.c:55-108.
// =============================================================================================
__global__ __launch_bounds__(256)
void k_lz2_dom(LzP P, Lz2Scratch sc)
{
    constexpr uint32_t RING = LZ2_CAP;                       // a cluster has at most LZ2_CAP entries: never more alive than that
    static_assert((RING & (RING - 1u)) == 0, "the ring is indexed with a mask");
    __shared__ uint32_t s_occ[LZ2_CAP / 32 + 72 + 264];     // occupancy bits (+ 64 zero words); the closed-form branch keeps <= block / W + 1 anchors here
    __shared__ uint16_t s_ring[RING];
    __shared__ uint16_t s_fid[DOM_FCAP], s_fpos[DOM_FCAP], s_fslot[DOM_FCAP];
    __shared__ uint32_t s_votes[3], s_result, s_next;
    const uint32_t tid = threadIdx.x;
    const uint32_t W = 1u << P.wbits;
    const uint32_t count = sc.big_count[6];
    uint32_t *cursor = sc.big_count + 8;                     // (zeroed with the other counters by stage 1)
    struct Src {                                             // the exported arrays of lz2.h; results aligned with the entries
        const uint16_t *bp, *br, *bi; uint16_t *bc;
        __device__ __forceinline__ uint64_t ent(uint32_t i) const { return ((uint64_t)bp[i] << 16) | ((uint64_t)br[i] << 32) | ((uint64_t)bi[i] << 48); }
        __device__ __forceinline__ void put(uint32_t i, uint32_t, uint32_t res) const { bc[i] = (uint16_t)res; }
    };
    for (;;) {
        __syncthreads();
        if (tid == 0) s_next = atomicAdd(cursor, 1u);
        __syncthreads();
        const uint32_t ci = s_next;
        if (ci >= count) break;
        Lz2BigDesc *dp = &sc.desc[6][ci];
        const uint32_t m = dp->count;
        if (dp->anom != ~0u || dp->limit != ~0u || m > LZ2_CAP) continue;       // the cluster that covers bucket 0 / T: the general replay
        const size_t at = (size_t)dp->block * LZ2_BIG_STRIDE + dp->start;
        Src src{sc.bigpos + at, sc.bigrs + at, sc.bigpid + at, sc.bigcand + at};
        // the replay writes the entries that find something; everything else reads "none" (the general replay writes all of them)
        for (uint32_t i = tid; i < m; i += 256) src.bc[i] = (uint16_t)LZ_NONE16;
        if (tid == 0) { s_votes[0] = s_votes[1] = s_votes[2] = 0; s_result = 0; }
        __syncthreads();
        const bool done = dom_cluster(src, m, W, (W < RING ? W : RING) - 1u, s_occ, s_ring, s_fid, s_fpos, s_fslot, s_votes, s_result, nullptr);
        if (done && tid == 0) dp->count = m | LZ2_DOM_DONE;
    }
}

// =============================================================================================
// Row replay (round 4): SEVERAL exported clusters per wave, one per row of RL = 8 / 16 / 32 lanes (clusters of up to 256 / 512 /
// 1024 entries: eight, four or two per wave).
// The wave replay above spends ~65 wave-uniform instructions per entry and a CU issues one scalar instruction per cycle for all
// its waves: k_lz2_big alone takes 10 of the step's 51 serial milliseconds (10^9 B, one stream).  Here nothing is wave-uniform
// except the step counter: a row owns one cluster — its occupancy bitmap is RL dwords of LDS, one per lane; first fit = every
// lane masks its dword, a ballot, the row's bits of it, ds_bpermute of the winning dword; a step's retirements (FIFO,
// lz77.c:70-76: up to RL at once, a prefix of the live entries because positions ascend) are one LDS `and` per retiring lane;
// the occupant of a slot and the slot + position of an entry are one LDS dword each — so a vector instruction serves all the
// rows.  All global memory traffic happens at BOUNDARIES between passes of RL steps, uses before issues (a wait inside the
// steps, or for a load some other row has just issued, would stall every row): the results of the last RL entries go out, the
// next RL entries of every row were loaded a pass ago, and a three-stage prefetch (cursor -> descriptor -> first entries) has
// the next cluster ready when a row finishes; rows start clusters on boundaries only.  16.25 KiB of LDS per wave for any RL.
// Clusters come off a cursor (descriptor order); the one cluster per block that covers bucket 0 / T (anom / limit) is left to
// k_lz2_big, which skips the descriptors flagged here.  Reference behaviour emulated: algorithms/lz77/lz77.c:55-108.
// =============================================================================================
#define ROW_BPERM(src_lane, v) ((uint32_t)__builtin_amdgcn_ds_bpermute((int)((src_lane) << 2), (int)(v)))

// first free slot at or above `from` of the row's bitmap (lane l of the row holds dword l in v), or ~0u
template <int RL>
__device__ __forceinline__ uint32_t row_first_zero(uint32_t v, uint32_t from, uint32_t l, uint32_t rb)
{
    constexpr uint32_t RMASK = RL == 32 ? 0xFFFFFFFFu : ((1u << (RL & 31)) - 1u);
    const uint32_t rw = from >> 5, lowmask = (1u << (from & 31u)) - 1u;
    if (l < rw) v = 0xFFFFFFFFu; else if (l == rw) v |= lowmask;
    const uint64_t mk = __ballot(v != 0xFFFFFFFFu);
    const uint32_t my = (uint32_t)(mk >> rb) & RMASK;                       // this row's lanes that still have a free slot
    const uint32_t ln = my ? (uint32_t)__builtin_ctz(my) : 0u;
    const uint32_t mv = ROW_BPERM(rb + ln, v);
    const uint32_t fz = (mv != 0xFFFFFFFFu) ? (uint32_t)__builtin_ctz(~mv) : 0u;
    return my ? ((ln << 5) + fz) : ~0u;
}

template <int RL>                                         // lanes per row: 8, 16 or 32 (clusters of up to 256, 512, 1024 entries)
__global__ __launch_bounds__(64)
void k_lz2_rows(LzP P, Lz2Scratch sc, int cls_a, int cls_b, int cursor_slot)
{
    static_assert(RL == 8 || RL == 16 || RL == 32, "rows of 8, 16 or 32 lanes");
    constexpr int NR = 64 / RL, CAPE = 32 * RL;            // rows per wave; slots of a row's bitmap (one dword per lane): 16.25 KiB per wave
    constexpr uint32_t RMASK = RL == 32 ? 0xFFFFFFFFu : ((1u << (RL & 31)) - 1u);
    __shared__ uint32_t s_occ[NR][CAPE];                   // slot -> word id | position << 16 of its occupant
    __shared__ uint32_t s_ent[NR][CAPE];                   // entry -> its slot | its position << 16 (for its eviction)
    __shared__ uint32_t s_bm[NR][RL];
    const uint32_t lane = threadIdx.x, g = lane / (uint32_t)RL, l = lane & (uint32_t)(RL - 1), rb = lane & ~(uint32_t)(RL - 1);
    const uint32_t W = 1u << P.wbits;
    // two descriptor lists behind one cursor, the class of the LONGER clusters first: a launch lasts as long as its last chain
    const uint32_t count_a = sc.big_count[cls_a], count = count_a + sc.big_count[cls_b];
    uint32_t *cursor = sc.big_count + cursor_slot;         // (zeroed with the other counters by stage 1)
    Lz2BigDesc *const descs_a = sc.desc[cls_a], *const descs_b = sc.desc[cls_b];
    auto desc_of = [&](uint32_t ticket) -> Lz2BigDesc * { return ticket < count_a ? descs_a + ticket : descs_b + (ticket - count_a); };
    uint32_t *occ = s_occ[g], *ent = s_ent[g], *bmw = s_bm[g];

    bool active = false, exhausted = false;
    uint32_t n = 0, i0 = 0, ev = 0, pre = 0;                // pre: entries of the cluster that k_lz2_prefix has placed and answered
    size_t at = 0;
    uint32_t cur_a = 0, cur_b = 0, out_acc = LZ_NONE16;
    // the next cluster of this row: 0 = nothing, 1 = cursor value in flight, 2 = descriptor in flight, 3 = first entries in flight / ready
    uint32_t pf_stage = 0, pf_ci = 0, pf_count = 0, pf_pre = 0;
    size_t pf_at = 0;
    // Registers that ONLY loads write (no arithmetic on them before the next boundary, no conditional assignment: either would put
    // a wait for the load right behind its issue).  Every boundary reloads all of them, from a harmless address when a row has
    // nothing to ask for: r_n* = entries i0 + RL .. of the running cluster, r_f* = first RL entries of the prefetched cluster,
    // r_d* = its descriptor, tk = lane 0's ticket from the cursor.  With a precomputed prefix the "first" entries of a cluster are
    // those of the pass that holds entry `pre`.
    uint32_t r_np = 0, r_ni = 0, r_nr = 0, r_fp = 0, r_fi = 0, r_fr = 0, tk = 0;
    uint4 r_d4 = make_uint4(0, 0, 0, 0); uint32_t r_d1 = 0, r_d6 = 0;
    // a zero the compiler cannot see through: on a provably uniform address it turns the cursor's atomic into its wave-aggregated
    // form and reads the result back on the spot
    uint32_t vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));

    for (;;) {
        // ================= boundary: USES (everything read here was loaded at least one pass ago) =================
        const bool flush = active && i0 + l < n && i0 + l >= pre;          // (below pre: k_lz2_prefix has written them)
        uint16_t *const flush_to = sc.bigcand + at + i0 + l;
        if (active) {
            i0 += (uint32_t)RL;
            if (i0 >= n) active = false;
            else { cur_a = r_np | (r_ni << 16); cur_b = r_nr; }
        }
        bool take = false, want_cursor = false;
        uint32_t done_ci = 0, done_n = 0;
        if (!active && pf_stage == 3u) {
            take = true;
            n = pf_count; at = pf_at; pre = pf_pre;
            cur_a = r_fp | (r_fi << 16); cur_b = r_fr; i0 = pre & ~(uint32_t)(RL - 1); ev = 0; active = true; pf_stage = 0;
            bmw[l] = 0;
            done_ci = pf_ci; done_n = n;
        }
        if (pf_stage == 1u) {
            pf_ci = ROW_BPERM(rb, tk);                                      // lane 0 of the row asked the cursor
            if (pf_ci >= count) { exhausted = true; pf_stage = 0; } else pf_stage = 2;
        } else if (pf_stage == 2u) {
            // the cluster that covers bucket 0 / T (and anything that does not fit): not ours, another one
            if (r_d4.w != ~0u || r_d1 != ~0u || r_d4.z > (uint32_t)CAPE || r_d4.z < 2u * RL) pf_stage = 0;
            else { pf_count = r_d4.z; pf_at = (size_t)r_d4.x * LZ2_BIG_STRIDE + r_d4.y; pf_pre = r_d6 < r_d4.z ? r_d6 : 0u; pf_stage = 3; }
        }
        if (pf_stage == 0u && !exhausted) { want_cursor = true; pf_stage = 1; }
        // ================= boundary: ISSUES (all unconditional loads; nothing below waits for them) =================
        {
            const uint32_t k = i0 + (uint32_t)RL + l;
            const size_t na = (active && k < n) ? at + k : 0;
            r_np = sc.bigpos[na]; r_ni = sc.bigpid[na]; r_nr = sc.bigrs[na];
            const uint32_t fk = (pf_pre & ~(uint32_t)(RL - 1)) + l;           // (pre = 0: >= 2 RL entries, the first RL exist)
            const size_t fa = (pf_stage == 3u && fk < pf_count) ? pf_at + fk : 0;
            r_fp = sc.bigpos[fa]; r_fi = sc.bigpid[fa]; r_fr = sc.bigrs[fa];
            const uint32_t *dp = reinterpret_cast<const uint32_t *>(pf_stage == 2u ? desc_of(pf_ci) : descs_a);
            r_d4 = *reinterpret_cast<const uint4 *>(dp); r_d1 = dp[4]; r_d6 = dp[6];
        }
        if (flush) *flush_to = (uint16_t)out_acc;
        if (take && l == 0) desc_of(done_ci)->count = done_n | LZ2_DOM_DONE;     // k_lz2_big skips it
        if (want_cursor && l == 0) tk = atomicAdd(cursor + vzero, 1u);
        // ================= a row that starts behind a precomputed prefix: the whole wave rebuilds its table =================
        // slot (in place of the home, k_lz2_prefix), position and word id of the entries below `pre`, 64 per iteration, the rows
        // that take a cluster at this boundary one after the other.  ONE wait for global memory per 256 entries — at most
        // CAPE / 256 of them per cluster start, where the replay of those entries took pre steps — and every row waits with it.
        {
            uint64_t starts = __ballot(take && l == 0 && pre != 0u);
            while (starts) {
                const uint32_t src = (uint32_t)__builtin_ctzll(starts), g2 = src / (uint32_t)RL;
                starts &= starts - 1ull;
                const uint32_t pre2 = RLANE(pre, src);
                const size_t at2 = (size_t)RLANE((uint32_t)at, src) | ((size_t)RLANE((uint32_t)((uint64_t)at >> 32), src) << 32);
                LZ2_PREFIX_COUNT(lane == 0, pre2);
                for (uint32_t j0 = 0; j0 < pre2; j0 += 256u) {                // (the loads of four iterations in flight together)
                    uint32_t sl[4], pp[4], idw[4];
#pragma unroll
                    for (uint32_t u = 0; u < 4u; ++u) {
                        const uint32_t j = j0 + 64u * u + lane;
                        const size_t ja = j < pre2 ? at2 + j : 0;
                        sl[u] = sc.bigrs[ja]; pp[u] = sc.bigpos[ja]; idw[u] = sc.bigpid[ja];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < 4u; ++u) {
                        const uint32_t j = j0 + 64u * u + lane;
                        if (j < pre2 && sl[u] < (uint32_t)CAPE) {
                            s_occ[g2][sl[u]] = idw[u] | (pp[u] << 16); s_ent[g2][j] = sl[u] | (pp[u] << 16);
                            atomicOr(&s_bm[g2][sl[u] >> 5], 1u << (sl[u] & 31u));    // (behind the row's own bmw[l] = 0, in the LDS queue's order)
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (__ballot(active || pf_stage != 0u) == 0ull) break;
        if (__ballot(active) == 0ull) continue;
        // ================= RL steps: LDS, cross-lane and vector work only =================
        // Software-pipelined: an entry's broadcast, the live entries a step may retire and the bitmap dwords the first fit needs
        // are asked for as early as their addresses are known, and every loaded value is used unconditionally (a load whose
        // only use sits under an `if` is sunk into that block together with the wait for it).
        uint32_t a = ROW_BPERM(rb, cur_a), r = ROW_BPERM(rb, cur_b);
        uint32_t e = ent[(active && ev + l < i0) ? ev + l : 0u];
        for (uint32_t t = 0; t < (uint32_t)RL; ++t) {
            const uint32_t i = i0 + t;
            const bool on = active && i < n && i >= pre;                      // (the pass that holds entry `pre`: the ones below are off)
            const uint32_t p = a & 0xFFFFu, id = a >> 16;
            for (;;) {                                                      // FIFO retirement (lz77.c:70-76): normally one pass
                const bool ret = on && ev + l < i && (e >> 16) + W < p;
                const uint64_t mk = __ballot(ret);
                if (ret) atomicAnd(&bmw[(e & 0xFFFFu) >> 5], ~(1u << (e & 31u)));       // clears the bucket
                const uint32_t cnt = (uint32_t)__popc((uint32_t)(mk >> rb) & RMASK);
                ev += cnt;
                if (__ballot(cnt == (uint32_t)RL) == 0ull) break;           // a row whose every lane retired one may have more
                e = ent[(on && ev + l < i) ? ev + l : 0u];
            }
            // (behind the clears, in the LDS queue's order) the home's dword and occupant, this lane's bitmap dwords
            const uint32_t wr = bmw[r >> 5], h = occ[r], v = bmw[l];
            const uint32_t tn = (t + 1u) & (uint32_t)(RL - 1);
            const uint32_t na = ROW_BPERM(rb + tn, cur_a), nr = ROW_BPERM(rb + tn, cur_b);
            const bool bit = (wr >> (r & 31u)) & 1u, same = (h & 0xFFFFu) == id;
            const bool seek = on && id != p;                                // (the first occurrence of a word in the block finds nothing, ever)
            // nothing evicted yet: the word's first occurrence = the word id; else the occupant of the home, if it is a copy
            uint32_t res = (seek && ev == 0u) ? id : (seek && bit && same) ? (h >> 16) : (uint32_t)LZ_NONE16;
            bool walk = seek && ev != 0u && bit && !same;
            if (__ballot(walk) != 0ull) {
                // the home holds another word: on to the first copy of this word or the first empty bucket, RL occupants per step
                uint32_t e_end = row_first_zero<RL>(v, r + 1u, l, rb);   // (a walk changes no bit)
                if (e_end > (uint32_t)CAPE) e_end = (uint32_t)CAPE;
                uint32_t b0 = r + 1u;
                while (__ballot(walk && b0 < e_end) != 0ull) {
                    const uint32_t bb = b0 + l;
                    const bool in = walk && bb < e_end;
                    const uint32_t o = occ[in ? bb : 0u];
                    const uint64_t mk = __ballot(in && (o & 0xFFFFu) == id);
                    const uint32_t my = (uint32_t)(mk >> rb) & RMASK;
                    const uint32_t src = ROW_BPERM(rb + (my ? (uint32_t)__builtin_ctz(my) : 0u), o);
                    if (walk && my) { res = src >> 16; walk = false; }
                    b0 += (uint32_t)RL;
                }
            }
            // insert: first fit from the home on (inside the cluster by the parking bound)
            const uint32_t b = row_first_zero<RL>(v, r, l, rb);
            const bool put = on && b < (uint32_t)CAPE;
            if (put && l == 0) atomicOr(&bmw[b >> 5], 1u << (b & 31u));
            if (put) { occ[b] = id | (p << 16); ent[i] = b | (p << 16); }
            if (on && l == t) out_acc = res;
            e = ent[(active && i + 1u < n && ev + l < i + 1u) ? ev + l : 0u];     // (behind this step's own record)
            a = na; r = nr;
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Measured alternatives (round 1, same box): staging 16 entries of all 64 clusters through LDS by coalesced loads ran
// 14 % faster alone (7.16 vs 8.35 ms / 400 MB) but its 3x LDS footprint cost the overlapped pipeline 4 % (10.46 vs 10.88
// GB/s) — k_lz2_find needs the whole LDS of a CU for its two workgroups; packing an entry into one 8-byte record
// fetched four steps ahead ran 19 % faster alone (6.76 ms) and cost the pipeline 2 % (11.24 vs 11.46: the export in
// k_lz2_find writes twice the bytes); lane replay of 128..511-entry clusters was 4x slower than the wave replay (one
// wave per CU).  All three were removed.
__device__ __forceinline__ uint32_t u16_of(const uint4 &v, uint32_t k)      // k-th 16-bit element of a 16-byte vector
{
    // two 64-bit halves and a variable shift: a select chain on the four dwords is turned into an indexed scratch access
    const uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    return (uint32_t)(((k & 4u) ? hi : lo) >> ((k & 3u) * 16u)) & 0xFFFFu;
}

// =============================================================================================
// The lane classes in one launch (round 6).  The exported clusters of 8..127 entries become ONE list sorted by size, longest
// first (a counting sort over the sizes: k_lz2_lane_count, k_lz2_lane_place); k_lz2_lanes gives a wave clusters of ONE size,
// as many as its LDS budget holds (at most 64), every lane's region sized by that size: n + 1 occupant dwords, ceil((n + 1) / 32)
// bitmap words, n slot bytes (a slot number fits a byte up to 255), rounded up to an odd number of dwords: the regions of the
// lanes start on different banks.  No lane idles behind a longer cluster, and a wave of 64-entry clusters holds twice the lanes
// that regions sized for the whole 64..127 class would leave it.  Waves are numbered long clusters first; the dispatcher hands them
// out in that order.
// =============================================================================================
constexpr uint32_t LANE_SIZES = LZ2_WAVE;                  // sizes 0..127 (8..127 occur)

__host__ __device__ __forceinline__ uint32_t lz2_lane_region(uint32_t n)      // dwords of the region of an n-entry cluster: odd
{
    return ((n + 1u) + ((n + 32u) >> 5) + ((n + 3u) >> 2)) | 1u;
}
__host__ __device__ __forceinline__ uint32_t lz2_lane_width(uint32_t n, uint32_t budget_dw)    // clusters per wave of n-entry clusters
{
    const uint32_t l = budget_dw / lz2_lane_region(n);
    return l < 64u ? l : 64u;
}

// descriptor v of the four lane classes taken as one array: 8..15 (class 7), 16..31 (0), 32..63 (1), 64..127 (2) entries
__device__ __forceinline__ const Lz2BigDesc *lz2_lane_desc(const Lz2Scratch &sc, uint32_t v, uint32_t n7, uint32_t n0, uint32_t n1)
{
    if (v < n7) return sc.desc[7] + v;
    v -= n7;
    if (v < n0) return sc.desc[0] + v;
    v -= n0;
    if (v < n1) return sc.desc[1] + v;
    return sc.desc[2] + (v - n1);
}

// clusters per size: LDS counters per workgroup, one global add per size
__global__ __launch_bounds__(256)
void k_lz2_lane_count(Lz2Scratch sc)
{
    __shared__ uint32_t s_h[LANE_SIZES];
    const uint32_t tid = threadIdx.x;
    const uint32_t n7 = sc.big_count[7], n0 = sc.big_count[0], n1 = sc.big_count[1], N = n7 + n0 + n1 + sc.big_count[2];
    if (blockIdx.x * 256u >= N) return;
    if (tid < LANE_SIZES) s_h[tid] = 0;
    __syncthreads();
    for (uint32_t v = blockIdx.x * 256u + tid; v < N; v += gridDim.x * 256u)
        atomicAdd(&s_h[lz2_lane_desc(sc, v, n7, n0, n1)->count & (LANE_SIZES - 1u)], 1u);
    __syncthreads();
    if (tid < LANE_SIZES && s_h[tid]) atomicAdd(&sc.lane_hist[tid], s_h[tid]);
}

// the sorted list: a workgroup counts its descriptors per size, reserves a range of every size's bucket with one global add per
// size and ranks inside it by LDS atomics (the order inside a size does not matter: the clusters are independent)
__global__ __launch_bounds__(256)
void k_lz2_lane_place(LzP P, Lz2Scratch sc)
{
    __shared__ uint32_t s_h[LANE_SIZES], s_at[LANE_SIZES];
    const uint32_t tid = threadIdx.x;
    const uint32_t n7 = sc.big_count[7], n0 = sc.big_count[0], n1 = sc.big_count[1], N = n7 + n0 + n1 + sc.big_count[2];
    if (blockIdx.x * 256u >= N) return;
    if (tid < LANE_SIZES) s_h[tid] = 0;
    __syncthreads();
    for (uint32_t v = blockIdx.x * 256u + tid; v < N; v += gridDim.x * 256u)
        atomicAdd(&s_h[lz2_lane_desc(sc, v, n7, n0, n1)->count & (LANE_SIZES - 1u)], 1u);
    __syncthreads();
    if (tid < 64u) {
        // size c's bucket starts behind every cluster of more than c entries; lane l holds sizes 127 - 2l and 126 - 2l
        const uint32_t a = LANE_SIZES - 1u - 2u * tid, b = a - 1u;
        const uint32_t ha = sc.lane_hist[a], hb = sc.lane_hist[b];
        const uint32_t before = wave_inclusive_scan<uint32_t>(ha + hb, OpAddU32(), 0u) - ha - hb;
        if (s_h[a]) s_at[a] = before + atomicAdd(&sc.lane_hist[LANE_SIZES + a], s_h[a]);
        if (s_h[b]) s_at[b] = before + ha + atomicAdd(&sc.lane_hist[LANE_SIZES + b], s_h[b]);
        s_h[a] = 0; s_h[b] = 0;
    }
    __syncthreads();
    for (uint32_t v = blockIdx.x * 256u + tid; v < N; v += gridDim.x * 256u) {
        const Lz2BigDesc *dp = lz2_lane_desc(sc, v, n7, n0, n1);
        const uint32_t c = dp->count & (LANE_SIZES - 1u), at = s_at[c] + atomicAdd(&s_h[c], 1u);
        if (at >= N) { lz_order_violation(P); continue; }             // (the counts are those k_lz2_lane_count saw: never)
        sc.lane_list[at] = make_uint4(dp->block, dp->start, dp->count, (dp->anom & 0xFFFFu) | (dp->limit << 16));
    }
}

// Wave g of the launch replays clusters of one size n in [size_lo, size_hi], the waves of size 127 first.  budget_dw = dynamic
// LDS of the launch in dwords (>= lz2_lane_region(127)).
__global__ __launch_bounds__(64)
void k_lz2_lanes(LzP P, Lz2Scratch sc, uint32_t size_hi, uint32_t size_lo, uint32_t budget_dw)
{
    extern __shared__ uint32_t s_lane[];
    const uint32_t lane = threadIdx.x;
    // lane l: sizes a = 127 - 2l and a - 1, their clusters (for the list offsets: all sizes) and this launch's waves of them
    const uint32_t a = LANE_SIZES - 1u - 2u * lane, b = a - 1u;
    const uint32_t ha = sc.lane_hist[a], hb = sc.lane_hist[b];
    const uint32_t wa = (a <= size_hi && a >= size_lo) ? (ha + lz2_lane_width(a, budget_dw) - 1u) / lz2_lane_width(a, budget_dw) : 0u;
    const uint32_t wb = (b <= size_hi && b >= size_lo) ? (hb + lz2_lane_width(b, budget_dw) - 1u) / lz2_lane_width(b, budget_dw) : 0u;
    const uint32_t hin = wave_inclusive_scan<uint32_t>(ha + hb, OpAddU32(), 0u);
    const uint32_t win = wave_inclusive_scan<uint32_t>(wa + wb, OpAddU32(), 0u);
    const uint32_t g = blockIdx.x;
    if (g >= (uint32_t)__builtin_amdgcn_readlane((int)win, 63)) return;
    // the lane whose sizes hold wave g: the lanes whose waves all lie below g come first
    const uint32_t j = (uint32_t)__popcll(__ballot(win <= g));
    const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)win, (int)j), waj = (uint32_t)__builtin_amdgcn_readlane((int)wa, (int)j),
                   wbj = (uint32_t)__builtin_amdgcn_readlane((int)wb, (int)j), hj = (uint32_t)__builtin_amdgcn_readlane((int)hin, (int)j),
                   haj = (uint32_t)__builtin_amdgcn_readlane((int)ha, (int)j), hbj = (uint32_t)__builtin_amdgcn_readlane((int)hb, (int)j);
    const uint32_t q0 = g - (wj - waj - wbj);
    const bool upper = q0 < waj;
    const uint32_t n = LANE_SIZES - 1u - 2u * j - (upper ? 0u : 1u), q = upper ? q0 : q0 - waj, hn = upper ? haj : hbj;
    const uint32_t first = (hj - haj - hbj) + (upper ? 0u : haj);        // clusters of more than n entries
    const uint32_t width = lz2_lane_width(n, budget_dw), k0 = q * width, nl = (hn - k0 < width) ? hn - k0 : width;
    uint4 dv = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
    if (lane < nl) dv = sc.lane_list[first + k0 + lane];
    // every cluster of the wave has n entries (the list is sorted): anything else would overrun its region
    if (lane < nl && dv.z != n) lz_order_violation(P);
    const uint32_t cnt = (lane < nl && dv.z == n) ? n : 0u, W = 1u << P.wbits;
    const uint32_t anom = (dv.w & 0xFFFFu) == 0xFFFFu ? ~0u : (dv.w & 0xFFFFu), limit = (dv.w >> 16) == 0xFFFFu ? ~0u : (dv.w >> 16);
    // Every lane walks its own cluster, so nothing coalesces, and 2-byte loads cost a cache line each: rocprofv3 showed
    // 1.5 GB of HBM traffic per launch against 60 MB of entries (the lines do not survive in L1 between steps).  Clusters
    // start on 16-byte boundaries (lz2.h), so a lane fetches EIGHT entries per load and stores eight results at once.
    const uint4 *vp = reinterpret_cast<const uint4 *>(sc.bigpos + (size_t)dv.x * LZ2_BIG_STRIDE + dv.y);
    const uint4 *vr = reinterpret_cast<const uint4 *>(sc.bigrs + (size_t)dv.x * LZ2_BIG_STRIDE + dv.y);
    const uint4 *vi = reinterpret_cast<const uint4 *>(sc.bigpid + (size_t)dv.x * LZ2_BIG_STRIDE + dv.y);
    uint4 *vc = reinterpret_cast<uint4 *>(sc.bigcand + (size_t)dv.x * LZ2_BIG_STRIDE + dv.y);
    uint32_t *occ = s_lane + (cnt ? lane : 0u) * lz2_lane_region(n);      // idle lanes (cnt = 0) touch nothing
    uint32_t *bits = occ + (n + 1u);
    uint8_t *slot = reinterpret_cast<uint8_t *>(bits + ((n + 32u) >> 5));
    if (cnt) for (uint32_t k = 0; k < ((n + 32u) >> 5); ++k) bits[k] = 0;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    uint4 evw = zero4;                                     // positions of entries [ev & ~7, +8): the next to retire
    if (cnt) evw = vp[0];
    uint32_t ev = 0, ev_p = evw.x & 0xFFFFu;
    bool anom_pending = anom != ~0u;
    const bool plain = anom == ~0u && limit == ~0u;        // not the cluster that covers bucket 0 / T
    uint4 np = evw, nr = zero4, ni = zero4;                // the group after the current one is in flight
    if (cnt) { nr = vr[0]; ni = vi[0]; }
    for (uint32_t i0 = 0; i0 < n; i0 += 8) {
        const uint4 cp = np, cr = nr, cid = ni;
        if (i0 + 8 < cnt) { np = vp[(i0 >> 3) + 1]; nr = vr[(i0 >> 3) + 1]; ni = vi[(i0 >> 3) + 1]; }
        uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t i = i0 + k;
            if (i < cnt) {
                const uint32_t p = u16_of(cp, k), r = u16_of(cr, k), id = u16_of(cid, k);
                while (ev < i && ev_p + W < p) {           // FIFO retirement
                    const uint32_t sb = slot[ev];
                    bits[sb >> 5] &= ~(1u << (sb & 31u));
                    ++ev;
                    if ((ev & 7u) == 0) evw = vp[ev >> 3];
                    ev_p = u16_of(evw, ev & 7u);
                }
                if (anom_pending && p > W - 1u) { bits[anom >> 5] &= ~(1u << (anom & 31u)); anom_pending = false; }
                uint32_t wi = r >> 5;
                const uint32_t w0 = bits[wi];
                uint32_t res = LZ_NONE16;
                if (plain && ev == 0) {                    // nothing evicted yet: find() = the word's first occurrence,
                    if (id != p) res = id;                 // which is what the word id is (k_lz2_find, the sweep)
                } else if (id != p && ((w0 >> (r & 31u)) & 1u)) {       // (a word's first occurrence in the block finds nothing, ever)
                    for (uint32_t sb = r;; ++sb) {
                        if (sb != r) {
                            if (sb == limit && r < limit) break;
                            if (!((bits[sb >> 5] >> (sb & 31u)) & 1u)) break;
                        }
                        const uint32_t o = occ[sb];
                        if ((o & 0xFFFFu) == id) { res = o >> 16; break; }
                    }
                }
                { const uint32_t v = res << ((k & 1u) * 16u); if (k < 2) o0 |= v; else if (k < 4) o1 |= v; else if (k < 6) o2 |= v; else o3 |= v; }
                uint32_t wv = w0 | ((1u << (r & 31u)) - 1u);
                while (wv == 0xFFFFFFFFu) wv = bits[++wi];
                const uint32_t sb = (wi << 5) + (uint32_t)__builtin_ctz(~wv);
                bits[sb >> 5] |= 1u << (sb & 31u);
                occ[sb] = id | (p << 16); slot[i] = (uint8_t)sb;
            }
        }
        if (i0 < cnt) vc[i0 >> 3] = make_uint4(o0, o1, o2, o3);      // pads of the last group: 0 (= skipped, lz2.h)
    }
}

// lists -> by-position array (test hook mi_lz_find_all_dev and the fallback boundary)
__global__ __launch_bounds__(1024)
void k_lz2_scatter(Lz2Scratch sc, uint16_t *__restrict__ cand_by_pos /* [nb][65536] */)
{
    const uint32_t lb = blockIdx.x;
    const Lz2BlockMeta *mt = sc.meta + lb;
    if (mt->fallback) return;
    const uint32_t n = mt->n;
    const uint16_t *pl = sc.plist + (size_t)lb * LZ_MAX_BLOCK, *cd = sc.cand + (size_t)lb * LZ_MAX_BLOCK;
    uint16_t *out = cand_by_pos + (size_t)lb * LZ_MAX_BLOCK;
    for (uint32_t j = threadIdx.x; j < n; j += 1024) { const uint32_t c = cd[j], p = pl[j]; if (c != p || p == LZ_NONE16) out[p] = (uint16_t)c; }
    __syncthreads();                                                     // position 0xFFFF: "none" first, the exported result over it
    const uint32_t nb = mt->nbig_entries;
    const uint16_t *bp = sc.bigpos + (size_t)lb * LZ2_BIG_STRIDE, *bc = sc.bigcand + (size_t)lb * LZ2_BIG_STRIDE;
    for (uint32_t j = threadIdx.x; j < nb; j += 1024) { const uint32_t p = bp[j], c = bc[j]; if (c != p) out[p] = (uint16_t)c; }    // c == p: a pad
}

template __global__ void k_lz2_big<LZ2_BIG_SMALL, 1>(LzP, Lz2Scratch, int);
template __global__ void k_lz2_big<512, 1>(LzP, Lz2Scratch, int);
template __global__ void k_lz2_big<256, 1>(LzP, Lz2Scratch, int);
template __global__ void k_lz2_big<LZ2_CAP, 4>(LzP, Lz2Scratch, int);
template __global__ void k_lz2_rows<16>(LzP, Lz2Scratch, int, int, int);


// =============================================================================================
// host side
// =============================================================================================
// clusters of class c per block, at most (a block has 65536 entries)
static uint32_t lz2_class_cap(uint32_t c)
{
    static const uint32_t lo[LZ2_NCLASS] = {16, 32, 64, 128, 256, 128, 1025, 8};    // smallest cluster a class can hold (either mode)
    return LZ_MAX_BLOCK / lo[c] + 8;
}

void lz2_carve(mi_carver &cv, uint32_t nb, bool debug, Lz2Scratch *sc)
{
    sc->partmap = cv.take<uint32_t>((size_t)nb * (PMP_BLOCK_BYTES / 4u));
    sc->plist = cv.take<uint16_t>((size_t)nb * LZ_MAX_BLOCK);
    sc->cand = cv.take<uint16_t>((size_t)nb * LZ_MAX_BLOCK);
    sc->meta = cv.take<Lz2BlockMeta>(nb);
    sc->fallback_count = cv.take<uint32_t>(64 + 2 * LANE_SIZES);
    sc->fallback_list = cv.take<uint32_t>(nb);
    sc->bigpos = cv.take<uint16_t>((size_t)nb * LZ2_BIG_STRIDE);
    sc->bigrs = cv.take<uint16_t>((size_t)nb * LZ2_BIG_STRIDE);
    sc->bigpid = cv.take<uint16_t>((size_t)nb * LZ2_BIG_STRIDE);
    sc->bigcand = cv.take<uint16_t>((size_t)nb * LZ2_BIG_STRIDE);
    for (uint32_t c = 0; c < LZ2_NCLASS; ++c) sc->desc[c] = cv.take<Lz2BigDesc>((size_t)nb * lz2_class_cap(c));
    sc->big_count = cv.at(sc->fallback_count, 16);
    sc->work_count = cv.at(sc->fallback_count, 32);      // zeroed with the other counters by stage 1
    sc->lane_hist = cv.at(sc->fallback_count, 64);       // (as are these)
    sc->work = cv.take<uint64_t>((size_t)nb * LZ2_MAXPARTS);
    sc->work_slots = nb * LZ2_MAXPARTS;
    sc->lane_list = cv.take<uint4>((size_t)nb * lz2_class_cap(7));
    sc->dbg = debug ? cv.take<uint64_t>(64) : nullptr;       // the phase counters (MI_LZ_DEBUG)
}

// what the kernels read of the switches, into a carved set (its dbg is the carve's)
void lz2_set_switches(Lz2Scratch *sc, const LzSwitches &sw)
{
    // bits 16..: the row replay's switch (MI_LZ_ROWS, lz2_stage_b): with it the wave classes are three (128..255 apart)
    sc->wave_min = LZ2_WAVE | ((sw.rows ? 1u : 0u) << 16);
    // MI_LZ_PREFIX=0: no k_lz2_prefix, every replay starts at entry 0 (A/B and the parity test, nothing else)
    sc->prefix = sw.prefix ? 1u : 0u;
#ifdef MI_MEASURE
    sc->stop_phase = sw.stop_phase;
#else
    sc->stop_phase = 0u;
#endif
}

// phase cycle counters of the last LZ call of this context (MI_LZ_DEBUG=1; a development hook, not in the public header)
extern "C" int mi_lz_debug_counters(mi_ctx *ctx, uint64_t *out32)
{
    if (!ctx || !ctx->lz_dbg) return 0;
    (void)hipDeviceSynchronize();
    return hipMemcpy(out32, ctx->lz_dbg, 64 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 1 : 0;      // 64 counters: [0..31] find / parse, [32..47] partition
}

#ifdef MI_TEST_HOOKS
// lib_test only (tests/test_prefix_replay_gpu.py): out2[0] = clusters whose replay started from a precomputed prefix or that the
// prefix finished, out2[1] = entries it answered, since the last reset; reset != 0 zeroes both afterwards.  0 on a HIP error.
extern "C" int mi_test_prefix_stats(mi_ctx *ctx, uint64_t *out2, int reset)
{
    if (!ctx || !out2) return 0;
    unsigned long long h[2] = {0, 0};
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lz2_prefix_stats), sizeof h) != hipSuccess) return 0;
    out2[0] = h[0]; out2[1] = h[1];
    if (reset) { h[0] = h[1] = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_lz2_prefix_stats), h, sizeof h) != hipSuccess) return 0; }
    return 1;
}
#endif

#ifdef MI_TEST_HOOKS
// lib_test only (tests/test_partmap_planes_gpu.py): the part map and the block records that the context's LAST partition launch
// wrote (one batch: the caller encodes a small input through any entry point first, which picks the kernel's instance).
// planes: [max_blocks][PMP_BLOCK_BYTES / 4], meta: [max_blocks] Lz2BlockMeta as dwords.  Returns the launch's blocks (at most
// max_blocks are copied), or -1 — no launch yet, or a HIP error.
extern "C" int mi_test_partmap(mi_ctx *ctx, uint32_t *planes, uint32_t *meta, uint32_t max_blocks)
{
    if (!ctx || !planes || !meta || !ctx->test_partmap) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const uint32_t nb = ctx->test_partmap_nb < max_blocks ? ctx->test_partmap_nb : max_blocks;
    if (hipMemcpy(planes, ctx->test_partmap, (size_t)nb * PMP_BLOCK_BYTES, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(meta, ctx->test_partmap_meta, (size_t)nb * sizeof(Lz2BlockMeta), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)ctx->test_partmap_nb;
}
#endif

// stage A1: partition (also decides which blocks go to the fallback pipeline)
mi_status lz2_stage_partition(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                              const Lz2Scratch &sc, hipStream_t s)
{
    MI_HIP(ctx, hipMemsetAsync(sc.fallback_count, 0, (64 + 2 * LANE_SIZES) * 4, s));      // fallback_count, big_count[], lane_hist[]
    if (sc.dbg && ctx->lz_dbg != sc.dbg) { ctx->lz_dbg = sc.dbg; MI_HIP(ctx, hipMemsetAsync(sc.dbg, 0, 512, s)); }
#ifdef MI_TEST_HOOKS
    ctx->test_partmap = sc.partmap; ctx->test_partmap_meta = sc.meta; ctx->test_partmap_nb = nb;      // (mi_test_partmap)
#endif
    mi_prof_scope p(ctx, "k_lz2_partition", s, (uint64_t)nb * P.block);
    lz2_launch_partition(d_in, n, P, sc, block0, nb, s);
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

// stage A2: per-part find (LDS heavy: four workgroups per CU)
static uint32_t lz2_find_grid(const LzP &P, uint32_t nb)
{
    // the partition lists a block's parts (greedy, data dependent: ~33 for a full block of text); the grid covers
    // LZ2_GRID_PARTS per block, rounded up to the 8 XCD slices of the kernel's workgroup mapping (a grid that is not a multiple
    // of 8 would leave items of the last row unassigned: ADVICE r3), the looping wide kernel takes whatever lies beyond
    const uint32_t parts = P.block / 64u + 1u < LZ2_GRID_PARTS ? P.block / 64u + 1u : LZ2_GRID_PARTS;
    return (parts * nb + 7u) & ~7u;
}

mi_status lz2_stage_find(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                         const Lz2Scratch &sc, hipStream_t s)
{
    mi_prof_scope p(ctx, "k_lz2_find", s, (uint64_t)nb * P.block);
    if (P.flags & LZP_DESC) hipLaunchKernelGGL(k_lz2_find_desc, dim3(lz2_find_grid(P, nb)), dim3(LZ2_THREADS), 0, s, d_in, n, P, sc, block0);
    else hipLaunchKernelGGL(k_lz2_find, dim3(lz2_find_grid(P, nb)), dim3(LZ2_THREADS), 0, s, d_in, n, P, sc, block0);
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

// parts of 2049..4096 entries (none in text) and whatever a batch lists beyond k_lz2_find's grid: 256 looping workgroups, gone at
// once when there is nothing to do.  Its own launch and — in the pipelined encoder — NOT on the stream of partition and find: an
// empty launch still has to be given 76 KiB of LDS per workgroup before it can leave, and it waited about a millisecond per batch
// for that behind the parse kernel of the batch before, on the one chain the pipeline is bound by (kernel timeline, round 4:
// partition 3.7 + find 4.45 + this 1.0 ms of a 9.3 ms batch period)
mi_status lz2_stage_find_wide(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                              const Lz2Scratch &sc, hipStream_t s, bool aside, const LzPlan &plan)
{
    // on the side stream this launch is normally empty and merely waits for its LDS behind the other stages (6 ms of "duration"
    // per batch in rocprofv3): timing it would report that wait as the pipeline's dominant kernel (as for the fallback chain,
    // lz_find_batch); MI_LZ_PROF_FALLBACK=1 times it (inputs with wide parts: scripts/adv_profile.py)
    const int saved_prof = ctx->profiling;
    if (aside && !plan.sw.prof_fallback) ctx->profiling = 0;
    {
        mi_prof_scope p(ctx, "k_lz2_find_wide", s, (uint64_t)nb * P.block);
        if (P.flags & LZP_DESC) hipLaunchKernelGGL(k_lz2_find_wide<true>, dim3(256), dim3(LZ2_THREADS), 0, s, d_in, n, P, sc, block0, lz2_find_grid(P, nb));
        else hipLaunchKernelGGL(k_lz2_find_wide<false>, dim3(256), dim3(LZ2_THREADS), 0, s, d_in, n, P, sc, block0, lz2_find_grid(P, nb));
    }
    ctx->profiling = saved_prof;
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

// stage B: replay of the exported clusters (almost no LDS: runs beside the next batch's stage A)
// which: 4 = the lane replays (8..127-entry clusters), 2 = the wave / row replays; 7 = both on `s`
mi_status lz2_stage_b(mi_ctx *ctx, const LzP &P, uint32_t nb, const Lz2Scratch &sc, hipStream_t s, int which, const LzPlan &plan)
{
    // Replay grids cover the worst case and the kernels stride, so any grid is correct.  Measured (round 2, same box):
    // persistent grids sized by LDS (16 / 12 / 7 / 5 / 16 waves per CU) left the lane classes unchanged and made the wave
    // replay 10.9 -> 15.8 ms per GB — a static stride deals a wave whatever chain lengths it draws, the hardware dispatcher
    // hands the next cluster to the first wave that is free.
    const uint32_t ncu = (uint32_t)ctx->num_cu;
    auto grid_of = [](uint64_t worst) -> uint32_t { return (uint32_t)(worst ? worst : 1); };
    // the lane classes: ordering pass + ONE launch of k_lz2_lanes (one-batch calls: on the stream of `which & 4`).
    // MI_LZ_LANES_KIB: LDS per wave of k_lz2_lanes (A/B).
    if (which & 4) {
        const uint32_t budget_dw = plan.sw.lanes_kib * 256u;                     // 1..32 KiB: >= lz2_lane_region(127)
        const uint64_t worst = (uint64_t)nb * lz2_class_cap(7);                  // lane-class clusters of the batch, at most
        const uint32_t og = (uint32_t)((worst + 255u) / 256u < (uint64_t)ncu * 4u ? (worst + 255u) / 256u : (uint64_t)ncu * 4u);
        { mi_prof_scope p(ctx, "k_lz2_lane_order", s, (uint64_t)nb * P.block);
          hipLaunchKernelGGL(k_lz2_lane_count, dim3(og), dim3(256), 0, s, sc);
          hipLaunchKernelGGL(k_lz2_lane_place, dim3(og), dim3(256), 0, s, P, sc); }
        // waves: sum over the sizes of ceil(clusters / width) <= the batch's entries / min(size * width) + one partial wave per size
        uint32_t m = ~0u;
        for (uint32_t c = LZ2_BIG; c < LANE_SIZES; ++c) { const uint32_t x = c * lz2_lane_width(c, budget_dw); m = x < m ? x : m; }
        const uint64_t waves = (uint64_t)nb * LZ_MAX_BLOCK / m + LANE_SIZES;
        { mi_prof_scope p(ctx, "k_lz2_lanes", s, (uint64_t)nb * P.block);
          hipLaunchKernelGGL(k_lz2_lanes, dim3((uint32_t)waves), dim3(64), budget_dw * 4u, s, P, sc, LANE_SIZES - 1u, LZ2_BIG, budget_dw); }
    }
    if (which & 2) {
    // the insert-only prefix of every plain wave-class cluster first (no LDS, a striding grid): the replays below start behind it
    if (sc.prefix) { mi_prof_scope p(ctx, "k_lz2_prefix", s, (uint64_t)nb * P.block);
      const uint64_t worst = (uint64_t)nb * (lz2_class_cap(3) + lz2_class_cap(4) + lz2_class_cap(5));
      hipLaunchKernelGGL(k_lz2_prefix, dim3((unsigned)(worst < (uint64_t)ncu * 32u ? worst : (uint64_t)ncu * 32u)), dim3(64), 0, s, P, sc); }
    { mi_prof_scope p(ctx, "k_lz2_big", s, (uint64_t)nb * P.block);
      // the 512..1024-entry class first and alone on the wave replay (6 KiB of LDS per wave), then the 128..511-entry clusters: on the
      // row replay (below), or — MI_LZ_ROWS=0 — on the wave replay with 3 KiB per wave (MI_LZ_BIG_SPLIT=0: one launch for both wave
      // classes, A/B)
      // row replay (four clusters per wave, off a cursor) of the 128..511-entry clusters, the 256..511 ones first (MI_LZ_ROWS=0: the
      // wave replay for everything, A/B); k_lz2_big then takes what the rows leave (the cluster that covers bucket 0 / T) with
      // small grids that stride over the descriptors
      if (plan.b_shape == LZ_B_ROWS_SPLIT) {
          hipLaunchKernelGGL((k_lz2_big<LZ2_BIG_SMALL, 1>), dim3(grid_of((uint64_t)nb * lz2_class_cap(4))), dim3(64), 0, s, P, sc, 3);
          hipLaunchKernelGGL((k_lz2_rows<16>), dim3(ncu * plan.sw.rows_waves), dim3(64), 0, s, P, sc, 5, 3, 9);
          hipLaunchKernelGGL((k_lz2_big<512, 1>), dim3(ncu * 4u), dim3(64), 0, s, P, sc, 2);
          hipLaunchKernelGGL((k_lz2_big<256, 1>), dim3(ncu * 4u), dim3(64), 0, s, P, sc, 4);
      } else if (plan.b_shape == LZ_B_SPLIT) {
          hipLaunchKernelGGL((k_lz2_big<LZ2_BIG_SMALL, 1>), dim3(grid_of((uint64_t)nb * lz2_class_cap(4))), dim3(64), 0, s, P, sc, 3);
          hipLaunchKernelGGL((k_lz2_big<512, 1>), dim3(grid_of((uint64_t)nb * lz2_class_cap(5))), dim3(64), 0, s, P, sc, 2);
      } else {
          hipLaunchKernelGGL((k_lz2_big<LZ2_BIG_SMALL, 1>), dim3(grid_of((uint64_t)nb * (lz2_class_cap(4) + lz2_class_cap(5)))), dim3(64), 0, s, P, sc, 0);
          // (with the row replay's three classes but MI_LZ_BIG_SPLIT=0: the 128..255 class has its own list)
          if (plan.sw.rows) hipLaunchKernelGGL((k_lz2_big<256, 1>), dim3(grid_of((uint64_t)nb * lz2_class_cap(3))), dim3(64), 0, s, P, sc, 4);
      } }
    { mi_prof_scope p(ctx, "k_lz2_dom", s, (uint64_t)nb * P.block);
      // clusters above 1024 entries that one word dominates (none in text: an empty launch of 13 KiB workgroups); what it leaves
      // goes to the general replay below
      const uint64_t worst = (uint64_t)nb * lz2_class_cap(6);
      hipLaunchKernelGGL(k_lz2_dom, dim3((unsigned)(worst < (uint64_t)ncu * 4u ? worst : (uint64_t)ncu * 4u)), dim3(256), 0, s, P, sc); }
    { mi_prof_scope p(ctx, "k_lz2_big<4096>", s, (uint64_t)nb * P.block);
      hipLaunchKernelGGL((k_lz2_big<LZ2_CAP, 4>), dim3(grid_of((uint64_t)nb * lz2_class_cap(6) < 4096 ? (uint64_t)nb * lz2_class_cap(6) : 4096)), dim3(64), 0, s, P, sc, 1); }   // 24 KiB each, normally none: a small striding grid
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

void lz2_launch_scatter(const Lz2Scratch &sc, uint16_t *cand_by_pos, uint32_t nb, hipStream_t s)
{
    hipLaunchKernelGGL(k_lz2_scatter, dim3(nb), dim3(1024), 0, s, sc, cand_by_pos);
}
