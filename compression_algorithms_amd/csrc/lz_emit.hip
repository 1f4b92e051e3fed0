// lz_emit.hip — greedy parse, token emission and stream concatenation for the LZ77 paths.
//
// Replaces the loop body of lz77_compress (algorithms/lz77/lz77.c:281-338; deflate variant
// algorithms/deflate/lz77.c:215-275) given the match finder's per-position candidates:
//
//   k_lz_parse_emit  per block: match length at every position (lz77.c:302-313), the greedy
//                    chain p -> p+1 | p+len resolved with 64-position chunk exit tables
//                    composed in two levels, token ranks by popcount prefix sums, tokens
//                    bit-packed LSB first through an LDS window (lz77.c:144-174: bit i of the
//                    stream is bit i%8 of byte i/8; deflate byte tokens lz77.c:176-197 are the
//                    same thing with 16/32-bit tokens)
//   k_lz_scan_blocks per-block sizes -> offsets in the batch, and the caller's block table
//   k_lz_concat      block streams -> one stream, bit-contiguous (a funnel-shift gather, one
//                    thread per output dword).  Not in mode H: its record sizes are known before
//                    the records are packed (defh_size.h), so the scan runs first and k_defh_encode
//                    writes every record where it belongs (defh.hip).
//   (decoders: lz_decode.hip)
#include "lz_common.h"
#include "lz2.h"
#include "internal.h"
#include <stdlib.h>


// DICT (with DESC): the first `skip` bytes of the block (LzBlkDesc) are a preset dictionary's tail — there for the finder, whose
// candidates may point into it, and no part of the item: the parse starts at `skip` and only the item's tokens are counted and emitted
// PARSE 1 (mode Z's lazy parse, include/mi_codec.h; token records only): a length is the common prefix up to min(255, n - p) — no
// byte at or past n is compared — and a position whose successor has the longer match becomes a literal; the chain p -> next(p) is
// still a function of the position alone, so the exit tables resolve it, with entry offsets up to 254 instead of 30
template <bool DESC, bool DICT = false, int PARSE = 0>   // DESC: `in` is the batched encoder's descriptor table (lz_block_src)
__global__ __launch_bounds__(1024)
void k_lz_parse_emit(const uint8_t *__restrict__ in, uint64_t n_total, LzP P, LzScratch sc, Lz2Scratch s2, int use_v2,
                     uint64_t block0, uint32_t *__restrict__ trec_all)
{
    // region0: input bytes -> exit tables [64][1024] -> {token base, match base, staging window}
    __shared__ __attribute__((aligned(16))) uint8_t s_r0[LZ_MAX_BLOCK + LZ_TAIL + 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_L[LZ_MAX_BLOCK];
    __shared__ uint64_t s_tok[1024], s_mat[1024];
    __shared__ uint8_t  s_entry[1024];
    __shared__ uint8_t  s_sexit[32][PARSE ? 256 : 32];
    __shared__ uint8_t  s_sentry[32];
    __shared__ uint32_t s_scan[18];

    const int tid = threadIdx.x;
    const uint32_t lb = blockIdx.x;
    long long tk = clock64();
#define PE_TICK(k) do { if (s2.dbg && tid == 0) { long long t2 = clock64(); atomicAdd((unsigned long long *)&s2.dbg[16 + (k)], (unsigned long long)(t2 - tk)); tk = t2; } } while (0)
    const uint8_t *src; uint32_t n;
    static_assert(DESC || !DICT, "a dictionary's tail comes with a descriptor");
    lz_block_src<DESC>(in, n_total, P.block, block0, lb, src, n);
    const uint32_t skip = lz_block_skip<DICT>(in, block0, lb);
    const uint16_t *cand = sc.cand + (size_t)lb * LZ_MAX_BLOCK;
    const uint32_t W = 1u << P.wbits, max_len = (1u << P.lbits) - 1u;
    // a candidate at this distance is no match (deflate lz77.c:223 / lz77.c:290); PARSE 1 is the deflate flavour with wbits 15
    // (defz_check), its rule a constant
    auto too_far = [&](uint32_t dist) -> bool {
        if constexpr (PARSE != 0) return dist >= 32767u;
        else return P.deflate ? (dist >= W - 1u) : (dist == W);
    };

    // ---- block -> LDS with the zero tail
    lz_block_to_lds_of<DESC>(s_r0, src, n, (uint32_t)tid);
    if constexpr (PARSE != 0) {
        // behind the block every length is 0 (phase A writes positions below n only): position n counts as "no match" for the
        // lazy step, and neither that step nor the exit tables need a bound of their own
        for (uint32_t p = n + (uint32_t)tid; p < ((n + 15u) & ~15u); p += 1024u) s_L[p] = 0;
        for (uint32_t q = ((n + 15u) >> 4) + (uint32_t)tid; q < LZ_MAX_BLOCK / 16u; q += 1024u) reinterpret_cast<uint4 *>(s_L)[q] = make_uint4(0, 0, 0, 0);
    }
    if (tid == 0) s_L[LZ_MAX_BLOCK - 1] = 0;     // position 0xFFFF: its "pending" marker equals "none" (lz2.h); none unless a list says otherwise
    __syncthreads();

    PE_TICK(0);
    // ---- A: token length at every position, were a token to start there.  The LDS-resident finder hands
    //      over (position, candidate) LISTS (coalesced); the first pipeline an array indexed by position.
    const bool lists = use_v2 && !s2.meta[lb].fallback;
    // the most a match at p may cover: the length field's, or (PARSE 1) what one byte holds and the block has left
    auto cap_of = [&](uint32_t p) -> uint32_t {
        if constexpr (PARSE != 0) { const uint32_t r = n - p; return r < 255u ? r : 255u; }
        else return max_len;
    };
    auto token_len = [&](uint32_t p, uint32_t c) -> uint32_t {
        const uint32_t cap = cap_of(p);                                     // (PARSE 1: the last compared word ends at n + 2 at most)
        uint32_t len = 0;
        if (c != LZ_NONE16) {
            const uint32_t dist = p - c;
            const bool literal = too_far(dist);
            if (!literal) {
                len = 4;                                                        // the words are equal
                // extend 4 bytes at a time (no `p < size` bound: the zero tail is there); first differing byte by ctz
                while (len < cap) {
                    const uint32_t x = lds_word(s_r0, c + len) ^ lds_word(s_r0, p + len);
                    if (x) { len += (uint32_t)__builtin_ctz(x) >> 3; break; }
                    len += 4;
                }
                if (len > cap) len = cap;
                if constexpr (PARSE != 0) { if (len < 3u) len = 0; }           // (the equal words reach into the zero tail: 1 or 2 real bytes)
            }
        }
        return len;
    };
    const uint16_t *l_pos = s2.plist + (size_t)lb * LZ_MAX_BLOCK, *l_cand = s2.cand + (size_t)lb * LZ_MAX_BLOCK;
    const uint16_t *b_pos = s2.bigpos + (size_t)lb * LZ2_BIG_STRIDE, *b_cand = s2.bigcand + (size_t)lb * LZ2_BIG_STRIDE;
    const uint32_t nbig = lists ? s2.meta[lb].nbig_entries : 0u;
    // (position, candidate) pairs of a list, 8 per lane per step: two 16-byte loads instead of sixteen 2-byte ones
    auto for_each_pair = [&](const uint16_t *lp, const uint16_t *lc, uint32_t cnt, auto &&fn) {
        // the next 8 pairs are in flight while these are worked on (the body is LDS work the compiler will not hoist
        // the loads over: measured, this loop was waiting on HBM, not on LDS)
        uint4 np = make_uint4(0, 0, 0, 0), nc = make_uint4(0, 0, 0, 0);
        uint32_t j0 = tid * 8u;
        if (j0 + 8u <= cnt) { np = *reinterpret_cast<const uint4 *>(lp + j0); nc = *reinterpret_cast<const uint4 *>(lc + j0); }
        for (; j0 < cnt; j0 += 1024u * 8u) {
            if (j0 + 8u <= cnt) {
                const uint4 vp = np, vc = nc;
                const uint32_t j1 = j0 + 1024u * 8u;
                if (j1 + 8u <= cnt) { np = *reinterpret_cast<const uint4 *>(lp + j1); nc = *reinterpret_cast<const uint4 *>(lc + j1); }
                const uint32_t wp[4] = {vp.x, vp.y, vp.z, vp.w}, wc[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) fn((wp[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu, (wc[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu);
            } else {
                for (uint32_t j = j0; j < cnt; ++j) fn((uint32_t)lp[j], (uint32_t)lc[j]);
            }
        }
    };
    // token lengths of a list, eight pairs at a time: the first compare step (bytes 4..7 — where most matches of a text
    // end) of all eight is issued together; a per-pair loop would walk its LDS round trips one pair after the other.
    // Matches that go on past byte 7 are QUEUED and extended 64 at a time: the extension is a data-dependent loop, and run in
    // place every wave paid its longest match (up to seven rounds) for each of its eight pair slots with a handful of lanes
    // alive — the phase was VALU-bound on those rounds (~1000 instructions per thread and step, 4 waves per SIMD: half of
    // this kernel).  The queue is one register per lane: a ballot ranks the lanes that have a pair to extend, ds_permute (the
    // LDS crossbar, no LDS memory) sends pair number r to lane (fill + r) mod 64 — the other lanes send to the slots that are
    // left, so the whole thing is a permutation — and whenever 64 pairs are together they are extended by a full wave.
    uint32_t q_cur = 0, q_nxt = 0, q_fill = 0;                   // queued (position | candidate << 16) of this lane; pairs queued (uniform)
    const uint32_t lane = (uint32_t)tid & 63u;
    auto extend = [&](uint32_t item, bool on) {
        if (on) {
            const uint32_t p = item & 0xFFFFu, c = item >> 16;
            const uint32_t cap = cap_of(p);
            uint32_t len = 8;
            while (len < cap) {
                const uint32_t x = lds_word(s_r0, c + len) ^ lds_word(s_r0, p + len);
                if (x) { len += (uint32_t)__builtin_ctz(x) >> 3; break; }
                len += 4;
            }
            s_L[p] = (uint8_t)(len > cap ? cap : len);
        }
    };
    auto enqueue = [&](bool ext, uint32_t item) {
        const uint64_t mk = __ballot(ext);
        if (mk == 0ull) return;                                    // (uniform)
        const uint32_t cnt = (uint32_t)__popcll(mk);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));   // queued lanes below this one
        const uint32_t slot = ext ? below : cnt + (lane - below);  // a stable partition of the 64 lanes: a permutation
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_permute((int)(((slot + q_fill) & 63u) << 2), (int)item);
        const uint32_t rel = (lane - q_fill) & 63u;                // lane q_fill + r received queued pair r
        if (rel < cnt) { if (lane >= q_fill) q_cur = got; else q_nxt = got; }
        q_fill += cnt;
        if (q_fill >= 64u) { extend(q_cur, true); q_cur = q_nxt; q_fill -= 64u; }
    };
    auto lengths_of_list = [&](const uint16_t *lp, const uint16_t *lc, uint32_t cnt) {
        uint4 np = make_uint4(0, 0, 0, 0), nc = make_uint4(0, 0, 0, 0);
        uint32_t j0 = tid * 8u;
        if (j0 + 8u <= cnt) { np = *reinterpret_cast<const uint4 *>(lp + j0); nc = *reinterpret_cast<const uint4 *>(lc + j0); }
        // (the trip count is the same for every lane of a wave — the queue's ballots need the whole wave: 512 pairs per wave and step)
        for (uint32_t w0 = ((uint32_t)tid & ~63u) * 8u; w0 < cnt; w0 += 1024u * 8u, j0 += 1024u * 8u) {
            const bool full = j0 + 8u <= cnt;                       // (every lane runs the body: the queue works on whole waves)
            {
                const uint4 vp = np, vc = nc;
                const uint32_t j1 = j0 + 1024u * 8u;
                if (j1 + 8u <= cnt) { np = *reinterpret_cast<const uint4 *>(lp + j1); nc = *reinterpret_cast<const uint4 *>(lc + j1); }
                const uint32_t wp[4] = {vp.x, vp.y, vp.z, vp.w}, wc[4] = {vc.x, vc.y, vc.z, vc.w};
                uint32_t pp[8], cc[8], xx[8];
                bool act[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    pp[k] = (wp[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu; cc[k] = (wc[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
                    const uint32_t dist = pp[k] - cc[k];
                    // a candidate that the literal rule does not reject; c == p: pending or pad
                    act[k] = full && cc[k] != LZ_NONE16 && cc[k] != pp[k] && !too_far(dist);
                    xx[k] = 0;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) if (act[k]) xx[k] = lds_word(s_r0, cc[k] + 4u) ^ lds_word(s_r0, pp[k] + 4u);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t cap = cap_of(pp[k]);
                    const bool ext = act[k] && xx[k] == 0u && cap > 8u;
                    if (full && cc[k] != pp[k] && !ext) {              // (pending / pad: the other list, or nobody, writes it)
                        uint32_t len = 0;
                        if (act[k]) {
                            len = xx[k] ? 4u + ((uint32_t)__builtin_ctz(xx[k]) >> 3) : 8u; if (len > cap) len = cap;
                            if constexpr (PARSE != 0) { if (len < 3u) len = 0; }
                        }
                        s_L[pp[k]] = (uint8_t)len;
                    }
                    enqueue(ext, pp[k] | (cc[k] << 16));
                }
            }
            if (!full)
                for (uint32_t j = j0; j < cnt && j < j0 + 8u; ++j) { const uint32_t p = lp[j], c = lc[j]; if (c != p) s_L[p] = (uint8_t)token_len(p, c); }
        }
    };
    auto flush_queue = [&]() { extend(q_cur, lane < q_fill); q_fill = 0; };
    if (lists) {
        lengths_of_list(l_pos, l_cand, n);
        lengths_of_list(b_pos, b_cand, nbig);
        flush_queue();
    } else {
        for (uint32_t p = tid; p < n; p += 1024u) s_L[p] = (uint8_t)token_len(p, cand[p]);
    }
    __syncthreads();
    if constexpr (DICT) {
        // no token starts in front of the item: the exit chain walks to `skip` one position at a time and is greedy from there
        for (uint32_t p = tid; p < skip; p += 1024u) s_L[p] = 0;
        __syncthreads();
    }

    PE_TICK(1);
    // ---- B: exit offset of every position of a 64-position chunk into the next chunk
    uint8_t *ex = s_r0;                       // ex[o * 1024 + chunk]
    {
        // the chunk's 64 lengths come in as four 16-byte LDS reads up front: the backward walk then has ONE dependent LDS
        // read per step (the exit of the position it jumps to) instead of two
        const uint32_t c = tid;
        uint32_t lw[16];
        {
            const uint4 *lp = reinterpret_cast<const uint4 *>(s_L + c * 64u);
#pragma unroll
            for (int q = 0; q < 4; ++q) { const uint4 v = lp[q]; lw[4 * q] = v.x; lw[4 * q + 1] = v.y; lw[4 * q + 2] = v.z; lw[4 * q + 3] = v.w; }
        }
        if constexpr (PARSE != 0) {
            // the lazy step: a match gives way to a literal where the next position's match is longer.  Every thread has its 64
            // lengths and the first of the next chunk in registers BEFORE anyone writes (in place, a neighbour would read a length
            // already rewritten); position n and everything behind it are 0 (filled above), and there is no s_L[65536]
            const uint32_t nx0 = c < 1023u ? (uint32_t)s_L[c * 64u + 64u] : 0u;
            __syncthreads();
            uint32_t ew[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) ew[q] = 0;
#pragma unroll
            for (int o = 0; o < 64; ++o) {
                const uint32_t l = (lw[o >> 2] >> (8 * (o & 3))) & 0xFFu;
                const uint32_t nl = o < 63 ? (lw[(o + 1) >> 2] >> (8 * ((o + 1) & 3))) & 0xFFu : nx0;
                ew[o >> 2] |= (nl > l ? 0u : l) << (8 * (o & 3));
            }
            uint4 *wp = reinterpret_cast<uint4 *>(s_L + c * 64u);
#pragma unroll
            for (int q = 0; q < 4; ++q) { wp[q] = make_uint4(ew[4 * q], ew[4 * q + 1], ew[4 * q + 2], ew[4 * q + 3]); }
#pragma unroll
            for (int q = 0; q < 16; ++q) lw[q] = ew[q];
        }
#pragma unroll
        for (int o = 63; o >= 0; --o) {
            const uint32_t p = c * 64u + (uint32_t)o;
            uint32_t e = 0;
            if (PARSE != 0 || p < n) {                              // (PARSE 1: the lengths behind the block are 0, their exits harmless)
                const uint32_t l = (lw[o >> 2] >> (8 * (o & 3))) & 0xFFu;
                const uint32_t nx = (uint32_t)o + (l ? l : 1u);
                e = nx >= 64u ? nx - 64u : ex[nx * 1024u + c];
            }
            ex[(uint32_t)o * 1024u + c] = (uint8_t)e;
        }
    }
    __syncthreads();
    PE_TICK(2);
    // compose over super-chunks of 32 chunks.  A chunk is entered at offset <= max_len - 1 <= 30 for the
    // reference's length fields (lbits 4 and 5); longer fields take the serial walk below.
    const bool wide = PARSE != 0 ? false : max_len > 31u;
    if constexpr (PARSE != 0) {
        // a chunk is entered at an offset up to 254, and an offset of 64 or more passes the whole chunk: 32 super-chunks x 256
        // entry offsets, eight independent walks per thread (their LDS round trips overlap)
        const uint32_t scn = tid >> 5, o = tid & 31u;
        uint32_t x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = o + 32u * (uint32_t)j;
        for (uint32_t c = scn * 32u; c < scn * 32u + 32u; ++c) {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = x[j] >= 64u ? x[j] - 64u : ex[x[j] * 1024u + c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s_sexit[scn][o + 32u * (uint32_t)j] = (uint8_t)x[j];
        __syncthreads();
        if (tid == 0) {
            uint32_t e = 0;
            for (uint32_t s = 0; s < 32; ++s) { s_sentry[s] = (uint8_t)e; e = s_sexit[s][e]; }
        }
        __syncthreads();
        if (tid < 32) {
            uint32_t xx = s_sentry[tid];
            for (uint32_t c = tid * 32u; c < tid * 32u + 32u; ++c) { s_entry[c] = (uint8_t)xx; xx = xx >= 64u ? xx - 64u : ex[xx * 1024u + c]; }
        }
        __syncthreads();
    } else if (!wide) {
        const uint32_t scn = tid >> 5, o = tid & 31u;
        uint32_t x = o;
        for (uint32_t c = scn * 32u; c < scn * 32u + 32u; ++c) x = ex[x * 1024u + c];
        s_sexit[scn][o] = (uint8_t)x;
        __syncthreads();
        if (tid == 0) {
            uint32_t e = 0;
            for (uint32_t s = 0; s < 32; ++s) { s_sentry[s] = (uint8_t)e; e = s_sexit[s][e]; }
        }
        __syncthreads();
        if (tid < 32) {
            uint32_t xx = s_sentry[tid];
            for (uint32_t c = tid * 32u; c < tid * 32u + 32u; ++c) { s_entry[c] = (uint8_t)xx; xx = ex[xx * 1024u + c]; }
        }
        __syncthreads();
    }

    PE_TICK(3);
    // ---- C: token starts of each chunk
    {
        const uint32_t c = tid;
        uint64_t tok = 0, mat = 0;
        if (!wide) {
            if (c * 64u < n) {
                uint32_t o = s_entry[c];
                while (o < 64u && c * 64u + o < n) {
                    const uint32_t l = s_L[c * 64u + o];
                    tok |= 1ull << o;
                    if (l) mat |= 1ull << o;
                    o += l ? l : 1u;
                }
            }
            if constexpr (DICT) {                                   // the positions in front of the item are no tokens of its
                const uint64_t keep = c * 64u >= skip ? ~0ull : c * 64u + 64u <= skip ? 0ull : ~0ull << (skip - c * 64u);
                tok &= keep; mat &= keep;
            }
            s_tok[c] = tok; s_mat[c] = mat;
        } else {
            s_tok[c] = 0; s_mat[c] = 0;
        }
    }
    __syncthreads();
    if (wide && tid == 0) {
        // lbits > 5: a plain serial walk (not a reference configuration; kept for completeness)
        uint32_t p = DICT ? skip : 0u;
        while (p < n) {
            const uint32_t l = s_L[p];
            s_tok[p >> 6] |= 1ull << (p & 63u);
            if (l) s_mat[p >> 6] |= 1ull << (p & 63u);
            p += l ? l : 1u;
        }
    }
    __syncthreads();
    PE_TICK(4);
    const uint64_t my_tok = s_tok[tid], my_mat = s_mat[tid];
    uint32_t ntok = 0, nmat = 0;
    const uint32_t tbase = block_exclusive_scan<uint32_t>((uint32_t)__popcll(my_tok), OpAddU32(), 0u, s_scan, &ntok);
    const uint32_t mbase = block_exclusive_scan<uint32_t>((uint32_t)__popcll(my_mat), OpAddU32(), 0u, s_scan, &nmat);
    uint32_t *tb = reinterpret_cast<uint32_t *>(s_r0);            // [1025]
    uint32_t *mb = tb + 1026;                                      // [1025]
    uint32_t *stage = mb + 1026;                                   // [TPR * 1024 + 16]
    constexpr uint32_t TPR = 4;                                   // tokens per thread and emit round
    uint16_t *md = reinterpret_cast<uint16_t *>(stage + TPR * 1024 + 16);   // [<= 16384] distance of the k-th match token
    tb[tid] = tbase; mb[tid] = mbase;
    if (tid == 0) { tb[1024] = ntok; mb[1024] = nmat; }
    __syncthreads();
    if (lists) {
        auto put = [&](uint32_t p, uint32_t c) {
            const uint32_t ch = p >> 6, o = p & 63u;
            if ((s_mat[ch] >> o) & 1ull) md[mb[ch] + (uint32_t)__popcll(s_mat[ch] & ((1ull << o) - 1ull))] = (uint16_t)(p - c);
        };
        for_each_pair(l_pos, l_cand, n, [&](uint32_t p, uint32_t c) { if (c != p && c != LZ_NONE16) put(p, c); });
        for_each_pair(b_pos, b_cand, nbig, [&](uint32_t p, uint32_t c) { if (c != LZ_NONE16 && c != p) put(p, c); });
        __syncthreads();
    }

    PE_TICK(5);
    // ---- D: emit, 2048 tokens per barrier round (two per lane: their latencies overlap)
    const uint32_t LB = P.deflate ? 16u : 9u, MB = P.deflate ? 32u : (1u + P.wbits + P.lbits);
    uint32_t *slot = sc.slot + (size_t)lb * LZ_SLOT_WORDS;
    uint32_t carry = 0;
    if (PARSE != 0 || trec_all) {                                  // (PARSE 1 has no packed form)
        // mode H (defh.hip): no packed tokens; one 32-bit record per token, in token order, for the entropy stage:
        //   literal  byte                       match  1<<31 | length << 16 | distance
        // The 286-bin tally of the block (deflate/lz77.c:206,231,273; deflate/huffman.c:49-62) is taken here, where every
        // token passes by anyway, and handed to k_defh_encode at the end of the block's slot: it no longer reads the
        // token records twice.
        uint32_t *trec = trec_all + (size_t)lb * LZ_MAX_BLOCK;
        // eight copies of the tally (a pair of waves each): the frequent symbols of a text serialise on one LDS address
        constexpr uint32_t NH = 8u, HS = 288u;
        static_assert(NH * HS <= TPR * 1024u, "the tallies live in the staging window");
        for (uint32_t i = tid; i < NH * HS; i += 1024u) stage[i] = 0;
        // a literal token's byte goes where its length (0) was: the chunk's 64 bytes come in as four coalesced 16-byte loads
        // instead of one dependent byte load per literal inside the walk
        {
            const uint64_t lit = my_tok & ~my_mat;
            const uint32_t p0 = (uint32_t)tid * 64u;
            if (lit) {
                bool v16 = (((uintptr_t)src) & 15u) == 0 && p0 + 64u <= n;
                // (the chunk's four 16-byte loads first, then their uses: one round trip, not four)
                uint4 v4[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
                if constexpr (DESC) { lz_chunk64_any(src, n, p0, v4); v16 = true; }
                else if (v16) {
#pragma unroll
                    for (uint32_t k4 = 0; k4 < 4u; ++k4) v4[k4] = *reinterpret_cast<const uint4 *>(src + p0 + 16u * k4);
                }
#pragma unroll
                for (uint32_t k4 = 0; k4 < 4u; ++k4) {
                    uint32_t w[4] = {v4[k4].x, v4[k4].y, v4[k4].z, v4[k4].w};
                    if (!v16) { for (uint32_t j = 0; j < 16u; ++j) if (p0 + 16u * k4 + j < n) w[j >> 2] |= (uint32_t)src[p0 + 16u * k4 + j] << (8u * (j & 3u)); }
#pragma unroll
                    for (uint32_t j = 0; j < 16u; ++j)
                        if ((lit >> (16u * k4 + j)) & 1ull) s_L[p0 + 16u * k4 + j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
                }
            }
        }
        __syncthreads();
        // POSITION-driven: thread c walks the token starts of its own chunk (it knows how many tokens and matches lie before
        // it) — no token -> chunk search, no bit selection, nothing but LDS on the walk
        {
            uint64_t tk = my_tok;
            uint32_t t = tbase, mi = mbase;
            const uint32_t p0 = (uint32_t)tid * 64u;
            uint32_t *hist = stage + ((uint32_t)tid >> 7) * HS;
            while (tk) {
                const uint32_t o = (uint32_t)__builtin_ctzll(tk), p = p0 + o;
                tk &= tk - 1ull;
                uint32_t rec = s_L[p], sym = rec;                         // a literal's byte, or a match's length
                if ((my_mat >> o) & 1ull) {
                    const uint32_t d = lists ? (uint32_t)md[mi] : p - cand[p];
                    ++mi;
                    rec = 0x80000000u | (rec << 16) | d;
                    sym = 256u + ((uint32_t)__builtin_clz(d & 0xFFFFu) - 16u);
                }
                atomicAdd(&hist[sym], 1u);
                trec[t++] = rec;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < 288u; i += 1024u) {
            uint32_t v = 0;
            for (uint32_t h = 0; h < NH; ++h) v += stage[h * HS + i];
            slot[LZ_DEFH_HIST_AT + i] = v;
        }
        if (tid == 0) sc.block_bits[lb] = ntok;
        PE_TICK(6);
        if (s2.dbg && tid == 0) atomicAdd((unsigned long long *)&s2.dbg[31], 1ull);
        return;
    }
    // The packed formats, POSITION-driven like the records above: thread c walks the token starts of its own chunk; the bit
    // position of its first token follows from the token and match counts before it.  The output goes through an LDS window
    // of 4096 words per round (tokens are OR-ed in, LSB first: bit i of the stream is bit i%8 of byte i/8, lz77.c:144-174);
    // bit positions grow with the chunk number, so a thread takes part in the one or two rounds its chunk's range meets and
    // resumes where it stopped.  A literal's byte is parked where its length (0) was: four coalesced 16-byte loads per chunk
    // instead of a dependent byte load per literal.  (The token-driven loop this replaces — token -> chunk search, r-th set
    // bit, scattered byte loads, four tokens per thread and round — cost 117 k cycles per block.)
    {
        const uint64_t lit = my_tok & ~my_mat;
        const uint32_t p0 = (uint32_t)tid * 64u;
        if (lit) {
            bool v16 = (((uintptr_t)src) & 15u) == 0 && p0 + 64u <= n;
            uint4 v4[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
            if constexpr (DESC) { lz_chunk64_any(src, n, p0, v4); v16 = true; }
            else if (v16) {
#pragma unroll
                for (uint32_t k4 = 0; k4 < 4u; ++k4) v4[k4] = *reinterpret_cast<const uint4 *>(src + p0 + 16u * k4);
            }
#pragma unroll
            for (uint32_t k4 = 0; k4 < 4u; ++k4) {
                uint32_t w[4] = {v4[k4].x, v4[k4].y, v4[k4].z, v4[k4].w};
                if (!v16) { for (uint32_t j = 0; j < 16u; ++j) if (p0 + 16u * k4 + j < n) w[j >> 2] |= (uint32_t)src[p0 + 16u * k4 + j] << (8u * (j & 3u)); }
#pragma unroll
                for (uint32_t j = 0; j < 16u; ++j)
                    if ((lit >> (16u * k4 + j)) & 1ull) s_L[p0 + 16u * k4 + j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
            }
        }
    }
    {
        constexpr uint32_t WW = TPR * 1024u;                              // window words per round (stage holds WW + 16)
        const uint64_t total = (uint64_t)(ntok - nmat) * LB + (uint64_t)nmat * MB;
        uint64_t tk = my_tok;
        uint64_t q = (uint64_t)(tbase - mbase) * LB + (uint64_t)mbase * MB;   // bit position of this chunk's first token
        uint32_t mi = mbase;
        const uint32_t p0 = (uint32_t)tid * 64u;
        for (uint64_t w0 = 0; (w0 << 5) < total; w0 += WW) {
            for (uint32_t i = tid; i < WW + 2u; i += 1024u) stage[i] = (i == 0) ? carry : 0u;
            __syncthreads();
            const uint64_t hi = (w0 + WW) << 5;
            while (tk && q < hi) {
                const uint32_t o = (uint32_t)__builtin_ctzll(tk), p = p0 + o;
                tk &= tk - 1ull;
                uint32_t v = s_L[p], nbits = LB;                           // a literal's byte, or a match's length
                if ((my_mat >> o) & 1ull) {
                    const uint32_t d = lists ? (uint32_t)md[mi] : p - cand[p];
                    ++mi;
                    v = P.deflate ? (1u | (d << 8) | (v << 24)) : (1u | (d << 1) | (v << (1u + P.wbits)));
                    nbits = MB;
                } else v = P.deflate ? (v << 8) : (v << 1);
                const uint32_t rel = (uint32_t)(q - (w0 << 5)), wi = rel >> 5, sh = rel & 31u;
                atomicOr(&stage[wi], v << sh);
                if (sh + nbits > 32u) atomicOr(&stage[wi + 1], v >> (32u - sh));
                q += nbits;
            }
            __syncthreads();
            // complete words of this window: all of them, or up to the stream's last complete word
            const uint64_t endw = (total >> 5) < w0 + WW ? (total >> 5) : w0 + WW;
            const uint32_t ncomplete = (uint32_t)(endw - w0);
            for (uint32_t i = tid; i < ncomplete; i += 1024u) slot[w0 + i] = stage[i];
            carry = stage[ncomplete];
            __syncthreads();
        }
    }
    PE_TICK(6);
    if (s2.dbg && tid == 0) atomicAdd((unsigned long long *)&s2.dbg[31], 1ull);
    const uint64_t total_bits = (uint64_t)(ntok - nmat) * LB + (uint64_t)nmat * MB;
    if (tid == 0) {
        slot[total_bits >> 5] = (total_bits & 31u) ? carry : 0u;
        slot[(total_bits >> 5) + 1] = 0;
        sc.block_bits[lb] = total_bits;
    }
}

// ---------------------------------------------------------------------------------------------
// single-workgroup exclusive scan of the batch's block bit counts; also publishes the global
// exclusive offsets (base + local) to the caller's array
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_lz_scan_blocks(const uint64_t *bits, uint32_t nb, const uint64_t *__restrict__ base_bits,
                      uint64_t *excl_local /* may alias `bits`: scanned in place */, uint64_t *__restrict__ excl_global)
{
    // one small workgroup (it sits between two LDS-hungry kernels of its stream and must find a free slot quickly):
    // PER consecutive blocks per thread, a batch holds up to 4096 blocks
    __shared__ uint64_t s_tmp[6];
    const uint32_t PER = (nb + 255u) / 256u, a = threadIdx.x * PER, b = a + PER < nb ? a + PER : nb;
    uint64_t v = 0;
    for (uint32_t i = a; i < b; ++i) v += bits[i];
    uint64_t inc = v;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint64_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) s_tmp[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) { uint64_t run = 0; for (int w = 0; w < 4; ++w) { uint64_t t = s_tmp[w]; s_tmp[w] = run; run += t; } s_tmp[4] = run; }
    __syncthreads();
    uint64_t run = s_tmp[wave] + inc - v;
    const uint64_t base = *base_bits;
    for (uint32_t i = a; i < b; ++i) { const uint64_t x = bits[i]; excl_local[i] = run; excl_global[i] = base + run; run += x; }
    __syncthreads();                                    // (in place: every thread has read its own range before anyone writes [nb])
    if (threadIdx.x == 0) { excl_local[nb] = s_tmp[4]; excl_global[nb] = base + s_tmp[4]; }
}

__global__ void k_lz_advance(uint64_t *base_bits, const uint64_t *excl_local, uint32_t nb) { *base_bits += excl_local[nb]; }

// (for defh.hip, whose entropy stage runs the scan between its two kernels: in place over the batch's sizes)
void lz_launch_scan_blocks(uint64_t *block_bits, uint32_t nb, const uint64_t *base_bits, uint64_t *excl_global, hipStream_t s)
{
    hipLaunchKernelGGL(k_lz_scan_blocks, dim3(1), dim3(256), 0, s, block_bits, nb, base_bits, block_bits, excl_global);
}

__device__ __forceinline__ uint32_t extract_bits(const uint32_t *w, uint64_t lo, uint32_t k)   // k in 1..32
{
    const uint64_t wi = lo >> 5; const uint32_t sh = (uint32_t)(lo & 31u);
    const uint64_t two = (uint64_t)w[wi] | ((uint64_t)w[wi + 1] << 32);
    const uint64_t v = two >> sh;
    return k >= 32 ? (uint32_t)v : ((uint32_t)v & ((1u << k) - 1u));
}

// one thread per output dword of the batch's bit range [base, base + total)
__global__ __launch_bounds__(256)
void k_lz_concat(const uint32_t *__restrict__ slots, const uint64_t *__restrict__ excl_local, uint32_t nb,
                 const uint64_t *__restrict__ base_bits, uint32_t *__restrict__ out, uint64_t cap_words, uint32_t slot_words)
{
    const uint64_t base = *base_bits, total = excl_local[nb];
    const uint64_t wfirst = base >> 5;
    uint64_t wlast = (base + total + 31) >> 5;                                 // [wfirst, wlast)
    if (wlast > cap_words) wlast = cap_words;       // never past the caller's buffer (the host checked cap against the bound)
    // grid-stride: the grid is sized for a typical stream, the loop covers the worst case
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + wfirst; j < wlast; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g0 = j << 5, g1 = g0 + 32;
        uint64_t pos = g0 > base ? g0 : base;
        const uint64_t end = g1 < base + total ? g1 : base + total;
        // largest i with base + excl[i] <= pos
        uint32_t lo = 0, hi = nb - 1;
        const uint64_t rel = pos - base;
        while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (excl_local[mid] <= rel) lo = mid; else hi = mid - 1; }
        uint32_t i = lo, word = 0;
        while (pos < end) {
            const uint64_t bs = base + excl_local[i], be = base + excl_local[i + 1];
            const uint64_t se = be < end ? be : end;
            if (se > pos) {
                const uint32_t k = (uint32_t)(se - pos);
                word |= extract_bits(slots + (size_t)i * slot_words, pos - bs, k) << (uint32_t)(pos - g0);
                pos = se;
            }
            if (pos == be) ++i;
        }
        if (j == wfirst && (base & 31u)) atomicOr(&out[j], word);      // shares a dword with the previous batch
        else out[j] = word;
    }
}

// ---------------------------------------------------------------------------------------------
// decode: one wave per block, output staged in LDS.  A block stops at its original length: the
// last match may overshoot (the encoder compares into the zero tail), SURVEY.md A.3.4.
// ---------------------------------------------------------------------------------------------
// k <= 25 stream bits from bit `pos`; bytes at or past `nbytes` read as zero (the table and the stream come from a file
// or a peer: nothing is read outside the buffer the caller described)
__device__ __forceinline__ uint32_t stream_bits(const uint8_t *s, uint64_t nbytes, uint64_t pos, uint32_t k)
{
    const uint64_t byte = pos >> 3;
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) if (byte + i < nbytes) v |= (uint64_t)s[byte + i] << (8 * i);
    return (uint32_t)(v >> (pos & 7u)) & ((1u << k) - 1u);
}

// =============================================================================================
// host side
// =============================================================================================
// The forms of one pipeline (LzForm, internal.h).  LZ_TOKENS: the reference's token stream, packed per block into the block's
// slot, placed by the scan / concatenate kernels.  LZ_H: the same tokens, entropy coded per block (defh.hip); a record's size
// follows from its tally and code lengths and records are whole dwords, so the scan runs BEFORE the pack and the pack writes
// every record where it belongs: no slot, no k_lz_concat, the compressed bytes cross HBM once.  LZ_Z: the same tokens as
// standard DEFLATE records (defz.hip), byte aligned, through slot / scan / concatenate behind the container header; the caller
// has checked the parameters and the capacity.  LZ_BGZF: mode Z's records, each framed as a gzip member in its slot first
// (bgzf.hip).  LZ_BATCH (deflate_batch.hip): mode Z over a batch of independent items — the blocks come from a descriptor table
// built on the device (d_in, n, d_out, cap_bytes and d_block_bits are not used; nblocks is the caller's bound), and stage C
// places every record in its own item's buffer instead of scan / concatenate.  LZ_SNAPPY (snappy_batch.hip): LZ_BATCH with raw
// Snappy records instead of DEFLATE ones — the same descriptor table, tokens and placement, another last stage.  LZ_LZ4
// (lz4_batch.hip): the same again with LZ4 block records, an item being one raw block or a frame of them.

// blocks above 64 KiB (lz77 flavour): the HBM-resident finder of lzw.hip, one stream, batches sized by workspace
static mi_status lz_encode_wide(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap_bytes,
                                uint64_t *d_block_bits, uint64_t nblocks, hipStream_t s, const LzSwitches &sw)
{
    uint32_t nbw = lzw_batch_blocks(ctx, nblocks, P.block);
    LzwScratch ws; uint64_t *base_bits_w;
    mi_status st = lzw_reserve(ctx, &nbw, P.block, &ws, &base_bits_w);
    if (st) return st;
    MI_HIP(ctx, hipMemsetAsync(base_bits_w, 0, 8, s));
    if (nblocks == 0) { MI_HIP(ctx, hipMemsetAsync(d_block_bits, 0, 8, s)); return MI_OK; }
    for (uint64_t b0 = 0; b0 < nblocks; b0 += nbw) {
        const uint32_t nb = (uint32_t)((nblocks - b0) < nbw ? (nblocks - b0) : nbw);
        st = lzw_or_lzs_find(ctx, P, d_in, n, b0, nb, ws, s, sw);
        if (st) return st;
        { mi_prof_scope pr(ctx, "k_lzw_parse_emit", s, (uint64_t)nb * P.block);
          lzw_launch_parse_emit(d_in, n, P, ws, b0, nb, s); }
        hipLaunchKernelGGL(k_lz_scan_blocks, dim3(1), dim3(256), 0, s, ws.block_bits, nb, base_bits_w, ws.block_bits, d_block_bits + b0);
        { mi_prof_scope pr(ctx, "k_lz_concat", s, (uint64_t)nb * P.block);
          const uint64_t typw = (uint64_t)nb * (P.block / 4 + 64);
          hipLaunchKernelGGL(k_lz_concat, dim3((unsigned)((typw + 255) / 256 < 65535 ? (typw + 255) / 256 : 65535)), dim3(256), 0, s, ws.slot, ws.block_bits, nb,
                             base_bits_w, reinterpret_cast<uint32_t *>(d_out), cap_bytes / 4, ws.slot_words); }
        hipLaunchKernelGGL(k_lz_advance, dim3(1), dim3(1), 0, s, base_bits_w, ws.block_bits, nb);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

// The pipeline's workspace: the scratch sets (lz_carve), then the output's running bit position, the token records of every
// form but LZ_TOKENS (one array per set), and what the form keeps for itself (mode Z: the checksum's partials; a batch: its tables)
struct LzWs { LzScratch sc[MI_SETS]; Lz2Scratch sc2[MI_SETS]; uint64_t *base_bits; uint32_t *trec; void *zws; uint8_t *stage[MI_SETS]; };

// stage_bytes: a batch with a preset dictionary stages its items' first blocks behind the dictionary's tail, one cell per block slot of a set
static void lz_carve_all(mi_carver &cv, uint32_t nb, int nsets, bool debug, size_t trec_words, size_t z_bytes, size_t stage_bytes, LzWs *w)
{
    for (int k = 0; k < nsets; ++k) lz_carve(cv, nb, debug, &w->sc[k], &w->sc2[k]);
    for (int k = 0; k < MI_SETS; ++k) w->stage[k] = k < nsets && stage_bytes ? cv.take<uint8_t>(stage_bytes) : nullptr;
    w->base_bits = reinterpret_cast<uint64_t *>(cv.take<uint8_t>(8192));
    w->trec = trec_words ? cv.take<uint32_t>(trec_words) : nullptr;
    w->zws = cv.take<uint8_t>(z_bytes);
}

// The stream of the fallback chains of the ODD batches of a pipelined call (the even ones' is ctx->fb); creates or releases
// ctx->fb2.  `sb`: stage B's stream.
static hipStream_t lz_odd_fallback_stream(mi_ctx *ctx, const LzPlan &plan, hipStream_t sb)
{
    // where the chains go and whether the second stream should exist: lz_plan.h, from the call's one read of the hint
    if (plan.want_fb2 && !ctx->fb2) {
        int lo_ = 0, hi_ = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_, &hi_);
        if (hipStreamCreateWithPriority(&ctx->fb2, hipStreamNonBlocking, lo_) != hipSuccess) { (void)hipGetLastError(); ctx->fb2 = nullptr; }
    } else if (!plan.want_fb2 && ctx->fb2) {
        if (hipStreamQuery(ctx->fb2) == hipSuccess) { (void)hipStreamDestroy(ctx->fb2); ctx->fb2 = nullptr; }
        else (void)hipGetLastError();                     // still draining an earlier call's chains: try again next time
    }
    return plan.odd_chain == LZ_ODD_STAGE_B ? sb : (plan.odd_chain == LZ_ODD_FB2 && ctx->fb2) ? ctx->fb2 : ctx->fb;
}

// Stage B of a call of ONE batch (no pipeline: the side and fallback streams are idle): the lane replays run BESIDE the wave / row
// replays, on the side stream — the two groups are independent, each is a chain of launches with tails, and what follows needs
// both; the (normally empty) fallback chain and the wide finder have left the partition -> find chain for the fallback stream as
// in the pipeline (MI_LZ_B_SPLIT=0: one chain on one stream, A/B)
static mi_status lz_stage_b_solo(mi_ctx *ctx, const LzP &P, uint32_t nb, const Lz2Scratch &sc2, hipStream_t s, const LzPlan &plan)
{
    MI_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_wide[0], 0));                                             // the wide parts' exports
    MI_HIP(ctx, hipEventRecord(ctx->ev_find[0], s));
    MI_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_find[0], 0));
    mi_status st = lz_find_stage_b(ctx, P, nb, sc2, ctx->side, 4, plan);
    if (st) return st;
    MI_HIP(ctx, hipEventRecord(ctx->ev_replay[0], ctx->side));
    st = lz_find_stage_b(ctx, P, nb, sc2, s, 2, plan);
    MI_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_replay[0], 0));
    MI_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_fb[0], 0));                                               // the fallback blocks' candidates
    return st;
}

mi_status lz_encode_impl(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                         uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, void *stream, const LzCall &c)
{
    const bool items = c.form == LZ_BATCH || c.form == LZ_SNAPPY || c.form == LZ_LZ4;  // a batch of independent items brings its own buffers
    if (!ctx || (!items && (!d_out || !d_block_bits || (n && !d_in)))) return MI_ERR_ARG;
    const bool zform = c.form == LZ_Z || c.form == LZ_BGZF || items;                   // mode Z's tokens: the forms that take parse 1
    mi_status st = zform ? defz_check(p, c.form == LZ_SNAPPY || c.form == LZ_LZ4 ? (uint32_t)MI_CONTAINER_RAW : c.container) : lz_check_params(p);
    if (st) return st;
    if (!items && ((uintptr_t)d_out & 3u) != 0) return MI_ERR_ARG;
    if (c.form == LZ_H && (!p->deflate || p->lbits > 5 || p->wbits > 16)) return MI_ERR_ARG;
    if (c.form == LZ_TOKENS && cap_bytes < mi_lz_bound_bytes(n, p)) return MI_ERR_CAPACITY;
    if (c.form == LZ_H && cap_bytes < mi_deflate_h_bound_bytes(n, p)) return MI_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    LzP P = lz_params_of(ctx, p);
    if (items) P.flags |= LZP_DESC;
    const uint64_t nblocks = items ? c.batch->max_blocks : (n + P.block - 1) / P.block;
    // how this call runs: the switches and the hint, read here and nowhere below (lz_plan.h)
    const LzSwitches sw = lz_switches_read();
    const LzHint hint = lz_hint_read(ctx);
    if (P.block > LZ_MAX_BLOCK)
        return c.form == LZ_TOKENS ? lz_encode_wide(ctx, P, d_in, n, d_out, cap_bytes, d_block_bits, nblocks, s, sw) : MI_ERR_ARG;
    const LzPlan plan = lz_plan(nblocks, (uint32_t)ctx->num_cu, hint, sw);
    const uint32_t nbmax = plan.nbmax;
    const bool overlap = plan.overlap, solo = plan.solo;
    const int nsets = plan.nsets, skip = plan.skip, v2 = sw.v2 ? 1 : 0;
    const size_t trec_words = c.form == LZ_TOKENS ? 0 : (size_t)nbmax * LZ_MAX_BLOCK * nsets;
    const size_t z_bytes = items ? dfb_ws_bytes(*c.batch) : (c.form == LZ_Z || c.form == LZ_BGZF) ? defz_ws_bytes() : 0;
    const bool dict = items && c.batch->ulen != 0;                 // a preset dictionary: items' first blocks are staged behind its tail
    const size_t stage_bytes = dict ? dfb_stage_bytes(*c.batch, nbmax, P.block) : 0;
    LzWs t;
    st = mi_ws_carve(ctx, [&](mi_carver &cv) { lz_carve_all(cv, nbmax, nsets, sw.debug, trec_words, z_bytes, stage_bytes, &t); });
    if (st) return st;
    for (int k = 0; k < nsets; ++k) lz2_set_switches(&t.sc2[k], sw);
    DfbCall bc = items ? *c.batch : DfbCall{};                     // the batch with its staging cells in place
    bc.nbmax = nbmax; bc.nsets = (uint32_t)nsets;
    for (int k = 0; k < MI_SETS; ++k) bc.stage[k] = t.stage[k];
    const LzScratch *sc = t.sc; const Lz2Scratch *sc2 = t.sc2;
    // in front of the first block: where the output's bits start, and what the form needs before its blocks
    switch (c.form) {
    case LZ_TOKENS: case LZ_H: MI_HIP(ctx, hipMemsetAsync(t.base_bits, 0, 8, s)); break;
    case LZ_Z: case LZ_BGZF:   st = defz_begin(ctx, c.container, d_in, n, d_out, t.base_bits, t.zws, s); break;   // (the base starts at the header's bits)
    case LZ_BATCH: case LZ_SNAPPY: case LZ_LZ4: st = dfb_begin(ctx, bc, P.block, t.zws, s, &d_in); break;                      // (d_in: the descriptor table from here on)
    }
    if (st) return st;
    // behind the last block.  The table of an empty input is its one closing entry (mode Z's epilogue writes it itself, a batch
    // has no table).
    auto finish = [&]() -> mi_status {
        if (nblocks == 0 && (c.form == LZ_TOKENS || c.form == LZ_H || c.form == LZ_BGZF)) MI_HIP(ctx, hipMemsetAsync(d_block_bits, 0, 8, s));
        switch (c.form) {
        case LZ_TOKENS: case LZ_H: return MI_OK;
        case LZ_Z:                 return defz_end(ctx, c.container, d_out, d_block_bits, nblocks, n, t.zws, c.d_out_bytes, s);
        case LZ_BGZF:              return bgzf_end(ctx, d_out, d_block_bits, nblocks, c.d_out_bytes, s);
        case LZ_BATCH: case LZ_SNAPPY: case LZ_LZ4: return dfb_end(ctx, bc, P.block, t.zws, s);
        }
        return MI_ERR_ARG;
    };
    if (nblocks == 0) return finish();
    hipStream_t sb = overlap ? ctx->side : s, sp = overlap ? ctx->parse : s;
    // stage C of one batch (set k, the seq-th of the call): parse / emit, what the form does with the tokens, then the base moves on
    auto stage_c = [&](int k, uint64_t b0, uint32_t nb, uint64_t seq) {
        const uint64_t pbytes = (uint64_t)nb * P.block;
        uint64_t *excl_local = sc[k].block_bits;                   // reused in place by the scan
        uint32_t *trec = t.trec ? t.trec + (size_t)k * nbmax * LZ_MAX_BLOCK : nullptr;
        {
            mi_prof_scope pr(ctx, "k_lz_parse_emit", sp, pbytes);
            if (P.flags & LZP_LAZY) {                                  // mode Z's parse 1 (forms with token records only: checked at the entry)
                if (dict) hipLaunchKernelGGL((k_lz_parse_emit<true, true, 1>), dim3(nb), dim3(1024), 0, sp, d_in, n, P, sc[k], sc2[k], v2, b0, trec);
                else if (items) hipLaunchKernelGGL((k_lz_parse_emit<true, false, 1>), dim3(nb), dim3(1024), 0, sp, d_in, n, P, sc[k], sc2[k], v2, b0, trec);
                else hipLaunchKernelGGL((k_lz_parse_emit<false, false, 1>), dim3(nb), dim3(1024), 0, sp, d_in, n, P, sc[k], sc2[k], v2, b0, trec);
            }
            else if (dict) hipLaunchKernelGGL((k_lz_parse_emit<true, true>), dim3(nb), dim3(1024), 0, sp, d_in, n, P, sc[k], sc2[k], v2, b0, trec);
            else if (items) hipLaunchKernelGGL(k_lz_parse_emit<true>, dim3(nb), dim3(1024), 0, sp, d_in, n, P, sc[k], sc2[k], v2, b0, trec);
            else hipLaunchKernelGGL(k_lz_parse_emit<false>, dim3(nb), dim3(1024), 0, sp, d_in, n, P, sc[k], sc2[k], v2, b0, trec);
        }
        auto defh = [&] { mi_prof_scope ph(ctx, "k_defh_encode", sp, pbytes);     // mode H's entropy stage, the scan inside it: straight into the stream
                          defh_launch_encode(trec, sc[k].slot, sc[k].block_bits, nb, t.base_bits, d_block_bits + b0, d_out, cap_bytes, sp); };
        auto defz = [&] { mi_prof_scope ph(ctx, "k_defz_encode", sp, pbytes);     // mode Z's entropy stage: records in their slots
                          defz_launch_encode(trec, sc[k].slot, sc[k].block_bits, d_in, n, P.block, b0, nb, items, sp, dict); };
        auto snappy = [&] { mi_prof_scope ph(ctx, "k_snappy_emit", sp, pbytes);   // raw Snappy records in their slots
                            snappy_launch_emit(trec, sc[k].slot, sc[k].block_bits, d_in, P.block, b0, nb, sp); };
        auto lz4 = [&] { mi_prof_scope ph(ctx, "k_lz4_emit", sp, pbytes);         // LZ4 block records in their slots
                         lz4_launch_emit(trec, sc[k].slot, sc[k].block_bits, d_in, P.block, b0, nb, c.container == DFB_LZ4_FRAME, sp); };
        auto frame = [&] { mi_prof_scope pf(ctx, "k_bgzf_frame", sp, pbytes);     // every record a gzip member
                           bgzf_launch_frame(sc[k].slot, sc[k].block_bits, d_in, n, P.block, b0, nb, sp); };
        // every record to its own item (batches reach this stream in order: the item that straddles two of them goes on where the
        // one before stopped)
        auto place = [&] { mi_prof_scope pl(ctx, "k_dfb_place", sp, pbytes);
                           dfb_launch_place(bc, t.zws, sc[k].slot, sc[k].block_bits, b0, nb, seq, sp); };
        auto concat = [&] {                                        // the slots' contents into the one output stream: scan, then concatenate
            hipLaunchKernelGGL(k_lz_scan_blocks, dim3(1), dim3(256), 0, sp, sc[k].block_bits, nb, t.base_bits, excl_local, d_block_bits + b0);
            mi_prof_scope pr(ctx, "k_lz_concat", sp, pbytes);
            const uint64_t typw = (uint64_t)nb * (P.block / 4 + 64);   // about one output byte per input byte; the kernel strides
            hipLaunchKernelGGL(k_lz_concat, dim3((unsigned)((typw + 255) / 256)), dim3(256), 0, sp, sc[k].slot, excl_local, nb,
                               t.base_bits, reinterpret_cast<uint32_t *>(d_out), cap_bytes / 4, (uint32_t)LZ_SLOT_WORDS);
        };
        auto advance = [&] { hipLaunchKernelGGL(k_lz_advance, dim3(1), dim3(1), 0, sp, t.base_bits, excl_local, nb); };
        switch (c.form) {
        case LZ_TOKENS: concat(); advance(); break;
        case LZ_H:      defh(); advance(); break;
        case LZ_Z:      defz(); concat(); advance(); break;
        case LZ_BGZF:   defz(); frame(); concat(); advance(); break;
        case LZ_BATCH:  defz(); place(); break;
        case LZ_SNAPPY: snappy(); place(); break;
        case LZ_LZ4:    lz4(); place(); break;
        }
    };
    const hipStream_t sf_odd = lz_odd_fallback_stream(ctx, plan, sb);
    uint64_t batch = 0; uint32_t nb = 0;
    for (uint64_t b0 = 0; b0 < nblocks; b0 += nb, ++batch) {
        nb = (uint32_t)(nblocks - b0 < nbmax ? nblocks - b0 : nbmax);
        const int k = (int)(batch % (uint64_t)nsets);
        if (overlap && batch >= (uint64_t)nsets) MI_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_done[k], 0));   // set k is free again
        // a dictionary's tail and the items' heads into this set's cells: on `s`, in front of everything that reads a block (the other
        // streams fork from `s` behind it), and behind the wait above for the batch that used the cells last
        if (dict) { mi_prof_scope pr(ctx, "k_dfb_stage", s, (uint64_t)nb * P.block); dfb_launch_stage(bc, P.block, t.zws, b0, nb, s); }
        // stage A: partition + find on `s`, the fallback chain and the wide finder beside them
        const hipStream_t sf = !overlap ? (solo ? ctx->fb : s) : (batch & 1u) ? sf_odd : ctx->fb;
        st = lz_find_stage_a(ctx, P, d_in, n, b0, nb, sc[k], sc2[k], s, sf, ctx->ev_part[k], ctx->ev_fb[k], ctx->ev_wide[k], plan);
        if (st) return st;
        // stage B: the replays, behind the find and the wide parts' exports (lz_find.hip)
        if (overlap) {
            MI_HIP(ctx, hipEventRecord(ctx->ev_find[k], s)); MI_HIP(ctx, hipStreamWaitEvent(sb, ctx->ev_find[k], 0));
            if (v2) MI_HIP(ctx, hipStreamWaitEvent(sb, ctx->ev_wide[k], 0));
        }
        if (solo) st = lz_stage_b_solo(ctx, P, nb, sc2[k], s, plan);
        else if (!(skip & 1)) st = lz_find_stage_b(ctx, P, nb, sc2[k], sb, 7, plan);
        if (st) return st;
        // join: stage C needs the replays' results and the fallback blocks' candidates
        if (overlap) {
            MI_HIP(ctx, hipEventRecord(ctx->ev_replay[k], sb));
            MI_HIP(ctx, hipStreamWaitEvent(sp, ctx->ev_replay[k], 0));
            if (v2) MI_HIP(ctx, hipStreamWaitEvent(sp, ctx->ev_fb[k], 0));
        }
        if (!(skip & 2)) stage_c(k, b0, nb, batch);
        if (overlap) MI_HIP(ctx, hipEventRecord(ctx->ev_done[k], sp));
    }
    if (overlap) {                                                 // join: the last stage finishes everything
        MI_HIP(ctx, hipEventRecord(ctx->ev_fork, sp));
        MI_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_fork, 0));
    }
    MI_HIP(ctx, hipGetLastError());
    return finish();
}

extern "C" mi_status mi_lz_encode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                                      uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, void *stream)
{
    return lz_encode_impl(ctx, p, d_in, n, d_out, cap_bytes, d_block_bits, stream, LzCall{LZ_TOKENS});
}

extern "C" mi_status mi_deflate_h_encode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                                             uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, void *stream)
{
    return lz_encode_impl(ctx, p, d_in, n, d_out, cap_bytes, d_block_bits, stream, LzCall{LZ_H});
}

extern "C" mi_status mi_deflate_z_encode_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, const uint8_t *d_in, uint64_t n,
                                             uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, uint64_t *d_out_bytes, void *stream)
{
    if (!ctx || !d_out || !d_block_bits || !d_out_bytes || (n && !d_in)) return MI_ERR_ARG;
    mi_status st = defz_check(p, container);
    if (st) return st;
    if (cap_bytes < mi_deflate_z_bound_bytes(n, p, container)) return MI_ERR_CAPACITY;
    return lz_encode_impl(ctx, p, d_in, n, d_out, cap_bytes, d_block_bits, stream, LzCall{LZ_Z, container, d_out_bytes});
}

// BGZF (bgzf.hip has the framing): mode Z's records, each in a gzip member of its own
extern "C" mi_status mi_bgzf_encode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n, uint8_t *d_out,
                                        uint64_t cap_bytes, uint64_t *d_member_bits, uint64_t *d_out_bytes, void *stream)
{
    if (!ctx || !d_out || !d_member_bits || !d_out_bytes || (n && !d_in)) return MI_ERR_ARG;
    mi_status st = defz_check(p, MI_CONTAINER_RAW);
    if (st) return st;
    if (p->block > MI_BGZF_MAX_BLOCK) return MI_ERR_ARG;
    if (cap_bytes < mi_bgzf_bound_bytes(n, p)) return MI_ERR_CAPACITY;
    return lz_encode_impl(ctx, p, d_in, n, d_out, cap_bytes, d_member_bits, stream, LzCall{LZ_BGZF, MI_CONTAINER_RAW, d_out_bytes});
}

// launch alone: errors accumulate in *err (an mi_err_slot the caller reads once everything it launched has run)
mi_status mi_lz_decode_launch(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                              const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, uint32_t *err, hipStream_t s)
{
    if (!ctx || !d_stream || !d_block_bits || (n && !d_out) || !err) return MI_ERR_ARG;
    mi_status st = lz_check_params(p);
    if (st) return st;
    if (n == 0) return MI_OK;
    const LzP P = lz_params_of(ctx, p);
    const uint64_t nblocks = (n + P.block - 1) / P.block;
    mi_prof_scope pr(ctx, "k_lz_decode", s, n);
    lz_launch_decode(d_stream, stream_bytes, d_block_bits, P, d_out, n, nblocks, err, s);       // any block size
    return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

extern "C" mi_status mi_lz_decode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                                      const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, void *stream)
{
    if (!ctx || !d_stream || !d_block_bits || (n && !d_out)) return MI_ERR_ARG;
    mi_status st = lz_check_params(p);
    if (st) return st;
    if (n == 0) return MI_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *err = mi_err_slot(ctx, s);
    if (!err) return MI_ERR_HIP;
    st = mi_lz_decode_launch(ctx, p, d_stream, stream_bytes, d_block_bits, d_out, n, err, s);
    if (st) return st;
    uint32_t h_err = 0;
    MI_HIP(ctx, hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return h_err ? MI_ERR_CORRUPT : MI_OK;
}
