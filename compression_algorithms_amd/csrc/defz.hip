// defz.hip — "mode Z": standard DEFLATE (RFC 1951) over the reference's deflate tokens, in a raw, zlib (RFC 1950) or
// gzip (RFC 1952) container, readable by any inflater.
//
// The token sequence is mode T's (same finder, same parse, fresh table per block: k_lz_parse_emit leaves one u32 record per
// token, as for mode H).  One change: a block's last match that runs past the block end (into the zero tail the reference
// reads) is clipped to L' = block_end - pos — a match of L' if L' >= 3, else L' literals.  Each input
// block becomes one RECORD: one DEFLATE block with BFINAL = 0 (dynamic, fixed or stored — whichever is shortest in bits,
// ties in that order; a stored 65 536-byte block is two stored blocks) followed by an empty stored block (a sync flush:
// 000 + pad + 00 00 FF FF).  Records are whole bytes and independent: the block table gives byte-aligned restart points.
// The stream ends with 03 00 (a final fixed block holding only end-of-block).  include/mi_codec.h has the contract.
//
// Code lengths: the reference heap mode H uses (huff_merge in huff_enc.h: leaves in symbol order), then, where a code is longer
// than the limit (15; 7 for the code-length code), a deterministic repair: every length above the limit is clamped, codes
// are moved one level down from the deepest level above the limit that has one until the Kraft sum is <= 1, then one level
// up from the deepest level whose step still fits until it is exactly 1, and the new lengths are dealt out in the order of
// the unlimited ones (length, symbol).  A code with fewer than two used symbols is padded as zlib's encoder pads it.
//
//   k_defz_plan     one wave per block: tally of the RFC alphabets from the token records (with the clip), the three
//                   length-limited codes, the run-length coded header, the block type; tables and header bits -> the slot
//   k_defz_encode   one workgroup per block: header + tokens (BitPacker, huff_enc.h) + end-of-block + sync flush, LSB first, into the slot (or the
//                   stored form from the input); block_bits[lb] = the record's length in bits
//   k_crc32 / k_adler32            per-workgroup partial checksums over contiguous ranges of the input
//   k_crc32_combine / k_adler32_combine   one workgroup: the partials -> the checksum
//   k_defz_finish   one thread: container header, the final 03 00, the trailer, the total byte count
// k_lz_scan_blocks and k_lz_concat (lz_emit.hip) place the records, starting at the container header's bit count.
#include "lz_common.h"
#include "huff_enc.h"               // the heap merge, canonical codes and the pack round, shared with defh.hip
#include "crc32.h"                  // one workgroup's CRC-32 of a byte range, shared with bgzf.hip
#include "adler32.h"                // ... and its Adler-32 sums, shared with inflate_batch.hip
#include "internal.h"

// slot words [DEFZ_AT, ...): what k_defz_plan hands to k_defz_encode (a record is at most 16 388 words: the stored form)
#define DEFZ_AT        17000u
#define DEFZ_TYPE      (DEFZ_AT + 0u)          // 0 stored, 1 fixed, 2 dynamic (BTYPE)
#define DEFZ_HBITS     (DEFZ_AT + 1u)          // header bits (3 for fixed)
#define DEFZ_CLIP      (DEFZ_AT + 2u)          // clipped length of the last match, 0 = no clip
#define DEFZ_LL        (DEFZ_AT + 4u)          // [288] literal/length: bit-reversed code | length << 16
#define DEFZ_DC        (DEFZ_LL + 288u)        // [32]  distance codes, same form
#define DEFZ_HDR       (DEFZ_DC + 32u)         // header bits, LSB first
#define DEFZ_HDR_WORDS 160u                    // 3 + 14 + 19 * 3 + 316 * (7 + 7) bits < 4 500
static_assert((65536u + 5u * 2u + 5u + 3u) / 4u < DEFZ_AT, "the largest record ends before the plan's tables");
static_assert(DEFZ_HDR + DEFZ_HDR_WORDS <= LZ_DEFH_HIST_AT, "the plan's tables end before mode H's tally");
#ifndef DEFZ_THREADS
#define DEFZ_THREADS   256
#endif
#define DEFZ_MAXBITS   48u                     // 15 + 5 (length) + 15 + 13 (distance)

// (ZCK_SEG, ZCK_THREADS, ZCK_PIECE: crc32.h)
#define ZCK_GRID       1024u                   // partials at most (one per workgroup)
#define ZCK_PAIRS_AT   0u                      // checksum workspace: u32 [2 * ZCK_GRID] partials, then the result words
#define ZCK_RESULT_AT  (2u * ZCK_GRID)

__device__ __forceinline__ uint32_t z_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }

// length 3..258 -> code 257..285, extra bits nb with value xv
__device__ __forceinline__ uint32_t z_len_code(uint32_t L, uint32_t &nb, uint32_t &xv)
{
    if (L == 258u) { nb = 0; xv = 0; return 285u; }
    const uint32_t x = L - 3u;
    if (x < 8u) { nb = 0; xv = 0; return 257u + x; }
    nb = z_log2(x) - 2u; xv = x & ((1u << nb) - 1u);
    return 257u + 4u * (nb + 1u) + ((x >> nb) - 4u);
}
// distance 1..32768 -> code 0..29
__device__ __forceinline__ uint32_t z_dist_code(uint32_t d, uint32_t &nb, uint32_t &xv)
{
    const uint32_t x = d - 1u;
    if (x < 4u) { nb = 0; xv = 0; return x; }
    nb = z_log2(x) - 1u; xv = x & ((1u << nb) - 1u);
    return 2u * (nb + 1u) + ((x >> nb) - 2u);
}
__device__ __forceinline__ uint32_t z_len_extra(uint32_t s) { return (s < 265u || s == 285u) ? 0u : (s - 261u) / 4u; }
__device__ __forceinline__ uint32_t z_dist_extra(uint32_t c) { return c < 4u ? 0u : c / 2u - 1u; }
__device__ __forceinline__ uint32_t z_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

// order of the code-length code's lengths in the header (RFC 1951 3.2.7); the gzip header (RFC 1952: no flags, MTIME 0, OS 255)
__constant__ uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__constant__ uint8_t kGzip[10] = {0x1F, 0x8B, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0xFF};

struct ZHeap : HuffHeap<288> {
    uint32_t cnt[24];                         // lengths histogram of the repair
    int      maxlen;
};

// Lengths of a Huffman code over freq[0, nsym), at most `limit` bits, complete.  All 64 lanes of the (one-wave) block call it.
__device__ void z_code_lengths(const uint32_t *freq, int nsym, uint32_t limit, uint8_t *len, ZHeap &h)
{
    const int lane = threadIdx.x;
    for (int s = lane; s < nsym; s += 64) { h.leaf_of[s] = -1; len[s] = 0; }
    __syncthreads();
    if (lane == 0) {
        huff_merge(freq, nsym, h);
        if (h.nnodes < 2) {
            // zlib's build_tree: pad to two codes of length 1 with symbol 0, or 1 (2) when the used one is 0 (1)
            int first = 0;
            while (h.nnodes && h.leaf_of[first] < 0) ++first;
            len[first] = 1; len[h.nnodes == 0 ? 1 : (first < 2 ? first + 1 : 0)] = 1;
        }
        h.maxlen = 0;
        for (int l = 0; l < 24; ++l) h.cnt[l] = 0;
    }
    __syncthreads();
    if (h.root < 0) return;                                            // (uniform) the padded case is complete already
    for (int s = lane; s < nsym; s += 64) {
        const uint32_t l = huff_depth(h, s);
        if (!l) continue;
        len[s] = (uint8_t)l;
        atomicMax(&h.maxlen, (int)l);
        atomicAdd(&h.cnt[l < 23u ? l : 23u], 1u);
    }
    __syncthreads();
    if ((uint32_t)h.maxlen <= limit) return;                          // (uniform)
    if (lane == 0) {
        // clamp, then restore Kraft = 1 (in units of 2^-limit)
        for (int l = (int)limit + 1; l < 24; ++l) { h.cnt[limit] += h.cnt[l]; h.cnt[l] = 0; }
        const uint32_t full = 1u << limit;
        uint32_t K = 0;
        for (uint32_t l = 1; l <= limit; ++l) K += h.cnt[l] << (limit - l);
        while (K > full) {                                             // one code one level deeper: -2^(limit-l-1)
            uint32_t l = limit - 1u;
            while (l > 1u && h.cnt[l] == 0) --l;
            h.cnt[l]--; h.cnt[l + 1]++; K -= 1u << (limit - l - 1u);
        }
        while (K < full) {                                             // one code one level up: +2^(limit-l)
            uint32_t l = limit;
            while (l > 2u && (h.cnt[l] == 0 || (1u << (limit - l)) > full - K)) --l;
            h.cnt[l]--; h.cnt[l - 1]++; K += 1u << (limit - l);
        }
    }
    __syncthreads();
    // deal the new lengths out in (unlimited length, symbol) order
    uint8_t nl[(288 + 63) / 64];
    for (int s = lane, k = 0; s < nsym; s += 64, ++k) {
        nl[k] = 0;
        const uint32_t l = len[s];
        if (!l) continue;
        uint32_t rank = 0;
        for (int t = 0; t < nsym; ++t) { const uint32_t lt = len[t]; rank += lt && (lt < l || (lt == l && t < s)); }
        uint32_t run = 0, newl = limit;
        for (uint32_t q = 1; q <= limit; ++q) { run += h.cnt[q]; if (rank < run) { newl = q; break; } }
        nl[k] = (uint8_t)newl;
    }
    __syncthreads();
    for (int s = lane, k = 0; s < nsym; s += 64, ++k) if (len[s]) len[s] = nl[k];
    __syncthreads();
}

// RFC 1951 3.2.2 canonical codes, bit-reversed for LSB-first packing: tab[s] = rev(code) | len << 16.  All lanes.
__device__ void z_canonical(const uint8_t *len, int nsym, uint32_t *tab, uint32_t *s_cnt /*[16]*/, uint32_t *s_next /*[16]*/)
{
    // (the limiter leaves no length above 15: no bin for longer ones)
    huff_canonical<15, 16>(len, nsym, s_cnt, s_next, [&](int s, uint32_t l, uint32_t code) {
        tab[s] = l ? (__builtin_bitreverse32(code) >> (32u - l)) | (l << 16) : 0u;
    });
}

// (the body of k_defz_plan; DESC: `in` is the batched encoder's descriptor table — lz_block_src; DICT: a block's first `skip` bytes
// (LzBlkDesc) are a preset dictionary's tail — the record is that of the item's bytes behind them, which is what the tokens cover)
template <bool DESC, bool DICT = false>
__device__ __forceinline__ void defz_plan_block(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, const uint64_t *__restrict__ block_bits,
                                                const uint8_t *__restrict__ in, uint64_t n_total, uint32_t block, uint64_t block0)
{
    __shared__ uint32_t f_ll[288], f_dc[32], f_cl[20];
    __shared__ uint8_t  l_ll[288], l_dc[32], l_cl[20];
    __shared__ ZHeap h;
    __shared__ uint32_t s_rle[320];                                    // symbol | extra value << 8
    __shared__ uint32_t s_hdr[DEFZ_HDR_WORDS];
    __shared__ uint32_t s_tab[288];
    __shared__ uint32_t s_cnt[16], s_next[16];
    __shared__ uint32_t s_sum[8];                                      // [0] coverage before the last token, [1..4] bit sums
    const int lane = threadIdx.x;
    const uint32_t lb = blockIdx.x;
    const uint64_t off = (block0 + lb) * (uint64_t)block;
    uint32_t n = (uint32_t)((n_total - off) < block ? (n_total - off) : block);
    const uint8_t *src = nullptr;
    if constexpr (DESC) lz_block_src<true>(in, n_total, block, block0, lb, src, n);      // (a descriptor's block)
    if constexpr (DICT) { const uint32_t skip = lz_block_skip<true>(in, block0, lb); src += skip; n -= skip; }
    const uint32_t ntok = (uint32_t)block_bits[lb];                    // k_lz_parse_emit left the token count here (>= 1)
    const uint32_t *trec = trec_all + (size_t)lb * LZ_MAX_BLOCK;
    uint32_t *out = slots + (size_t)lb * LZ_SLOT_WORDS;

    for (int i = lane; i < 288; i += 64) f_ll[i] = 0;
    if (lane < 32) f_dc[lane] = 0;
    if (lane < 20) f_cl[lane] = 0;
    if (lane < 8) s_sum[lane] = 0;
    for (int i = lane; i < (int)DEFZ_HDR_WORDS; i += 64) s_hdr[i] = 0;
    __syncthreads();
    // ---- tally: every token but the last, which may be clipped
    uint32_t cov = 0;
    for (uint32_t t = lane; t + 1u < ntok; t += 64u) {
        const uint32_t r = trec[t];
        uint32_t nb, xv;
        if (r >> 31) {
            const uint32_t L = (r >> 16) & 0x7FFFu;
            cov += L;
            atomicAdd(&f_ll[z_len_code(L, nb, xv)], 1u);
            atomicAdd(&f_dc[z_dist_code(r & 0xFFFFu, nb, xv)], 1u);
        } else { cov += 1u; atomicAdd(&f_ll[r & 0xFFu], 1u); }
    }
    atomicAdd(&s_sum[0], cov);
    __syncthreads();
    if (lane == 0) {
        const uint32_t r = trec[ntok - 1u], pos = s_sum[0];
        uint32_t clip = 0, nb, xv;
        if (r >> 31) {
            const uint32_t L = (r >> 16) & 0x7FFFu, Lc = n - pos;         // the match starts inside the block: Lc >= 1
            const uint32_t Lk = Lc < L ? Lc : L;
            if (Lc < L) clip = Lc;
            if (Lk >= 3u) { atomicAdd(&f_ll[z_len_code(Lk, nb, xv)], 1u); atomicAdd(&f_dc[z_dist_code(r & 0xFFFFu, nb, xv)], 1u); }
            else for (uint32_t k = 0; k < Lk; ++k) atomicAdd(&f_ll[DESC ? src[n - Lk + k] : in[off + n - Lk + k]], 1u);
        } else atomicAdd(&f_ll[r & 0xFFu], 1u);
        f_ll[256] += 1u;                                               // end-of-block
        out[DEFZ_CLIP] = clip;
    }
    __syncthreads();
    // ---- the two token codes
    z_code_lengths(f_ll, 286, 15u, l_ll, h);
    z_code_lengths(f_dc, 30, 15u, l_dc, h);
    if (lane < 2) { l_ll[286 + lane] = 0; l_dc[30 + lane] = 0; }
    // ---- exact sizes in bits of the token part (extra bits are the same in both Huffman types)
    {
        uint32_t dyn = 0, fix = 0, ext = 0;
        for (int s = lane; s < 286; s += 64) { const uint32_t f = f_ll[s]; dyn += f * l_ll[s]; fix += f * z_fixed_len(s); ext += f * z_len_extra(s); }
        if (lane < 30) { const uint32_t f = f_dc[lane]; dyn += f * l_dc[lane]; fix += f * 5u; ext += f * z_dist_extra(lane); }
        atomicAdd(&s_sum[1], dyn); atomicAdd(&s_sum[2], fix); atomicAdd(&s_sum[3], ext);
    }
    // ---- run-length coded code lengths (one sequence over HLIT + HDIST, RFC 1951 3.2.7), lane 0
    __shared__ uint32_t s_nrle, s_hlit, s_hdist;
    if (lane == 0) {
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257u && !l_ll[hlit - 1]) --hlit;
        while (hdist > 1u && !l_dc[hdist - 1]) --hdist;
        const uint32_t N = hlit + hdist;
        auto seq = [&](uint32_t i) -> uint32_t { return i < hlit ? l_ll[i] : l_dc[i - hlit]; };
        uint32_t k = 0;
        for (uint32_t i = 0; i < N;) {
            const uint32_t v = seq(i);
            uint32_t run = 1;
            while (i + run < N && seq(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11u) { const uint32_t q = run < 138u ? run : 138u; s_rle[k++] = 18u | ((q - 11u) << 8); run -= q; }
                if (run >= 3u) { s_rle[k++] = 17u | ((run - 3u) << 8); run = 0; }
            } else {
                s_rle[k++] = v; --run;
                while (run >= 3u) { const uint32_t q = run < 6u ? run : 6u; s_rle[k++] = 16u | ((q - 3u) << 8); run -= q; }
            }
            while (run) { s_rle[k++] = v; --run; }
        }
        for (uint32_t j = 0; j < k; ++j) f_cl[s_rle[j] & 31u] += 1u;
        s_nrle = k; s_hlit = hlit; s_hdist = hdist;
    }
    __syncthreads();
    z_code_lengths(f_cl, 19, 7u, l_cl, h);
    // ---- choose the block type
    const uint32_t nrle = s_nrle, hlit = s_hlit, hdist = s_hdist;
    uint32_t hclen = 19;
    while (hclen > 4u && !l_cl[kOrder[hclen - 1]]) --hclen;
    uint32_t clbits = 0;
    for (int s = 0; s < 19; ++s) clbits += f_cl[s] * (l_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
    const uint64_t dyn_bits = 3u + 14u + 3u * hclen + clbits + (uint64_t)s_sum[1] + s_sum[3];
    const uint64_t fix_bits = 3u + (uint64_t)s_sum[2] + s_sum[3];
    const uint64_t sto_bits = 40ull * ((n + 65534u) / 65535u) + 8ull * n;
    const uint32_t type = (dyn_bits <= fix_bits && dyn_bits <= sto_bits) ? 2u : (fix_bits <= sto_bits ? 1u : 0u);
    if (type == 0u) { if (lane == 0) out[DEFZ_TYPE] = 0u; return; }
    if (type == 1u) {
        for (int s = lane; s < 288; s += 64) l_ll[s] = (uint8_t)z_fixed_len(s);
        if (lane < 32) l_dc[lane] = 5;
        __syncthreads();
    }
    // ---- header bits: BFINAL 0, BTYPE; for dynamic HLIT, HDIST, HCLEN, the code-length code, the run-length symbols
    if (type == 2u) {
        z_canonical(l_cl, 19, s_tab, s_cnt, s_next);
        if (lane == 0) {
            uint32_t pos = 0;
            auto put = [&](uint32_t v, uint32_t k) {
                if (!k) return;
                const uint32_t wi = pos >> 5, sh = pos & 31u;
                s_hdr[wi] |= v << sh;
                if (sh + k > 32u) s_hdr[wi + 1] |= v >> (32u - sh);
                pos += k;
            };
            put(4u, 3u); put(hlit - 257u, 5u); put(hdist - 1u, 5u); put(hclen - 4u, 4u);
            for (uint32_t i = 0; i < hclen; ++i) put(l_cl[kOrder[i]], 3u);
            for (uint32_t j = 0; j < nrle; ++j) {
                const uint32_t sym = s_rle[j] & 31u, xv = s_rle[j] >> 8, c = s_tab[sym];
                put(c & 0xFFFFu, c >> 16);
                put(xv, sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u);
            }
            out[DEFZ_HBITS] = pos;
        }
    } else if (lane == 0) { s_hdr[0] = 2u; out[DEFZ_HBITS] = 3u; }
    __syncthreads();
    for (int i = lane; i < (int)DEFZ_HDR_WORDS; i += 64) out[DEFZ_HDR + i] = s_hdr[i];
    z_canonical(l_ll, 288, s_tab, s_cnt, s_next);
    for (int i = lane; i < 288; i += 64) out[DEFZ_LL + i] = s_tab[i];
    z_canonical(l_dc, 32, s_tab, s_cnt, s_next);
    if (lane < 32) out[DEFZ_DC + lane] = s_tab[lane];
    if (lane == 0) out[DEFZ_TYPE] = type;
}

__global__ __launch_bounds__(64)
void k_defz_plan(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, const uint64_t *__restrict__ block_bits,
                 const uint8_t *__restrict__ in, uint64_t n_total, uint32_t block, uint64_t block0)
{
    defz_plan_block<false>(trec_all, slots, block_bits, in, n_total, block, block0);
}
__global__ __launch_bounds__(64)
void k_defz_plan_desc(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, const uint64_t *__restrict__ block_bits,
                      const uint8_t *__restrict__ in, uint64_t n_total, uint32_t block, uint64_t block0)
{
    defz_plan_block<true>(trec_all, slots, block_bits, in, n_total, block, block0);
}
__global__ __launch_bounds__(64)
void k_defz_plan_dict(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, const uint64_t *__restrict__ block_bits,
                      const uint8_t *__restrict__ in, uint64_t n_total, uint32_t block, uint64_t block0)
{
    defz_plan_block<true, true>(trec_all, slots, block_bits, in, n_total, block, block0);
}

// byte i of the stored form of a block of n bytes (n >= 1): pieces of <= 65 535 bytes, each 00 LEN NLEN data, then the sync
// flush 00 00 00 FF FF, then zeros
__device__ __forceinline__ uint32_t z_stored_byte(const uint8_t *src, uint32_t n, uint32_t npieces, uint32_t i)
{
    const uint32_t body = 5u * npieces + n;
    if (i >= body) { const uint32_t j = i - body; return (j == 3u || j == 4u) ? 0xFFu : 0u; }
    const uint32_t piece = i / 65540u, r = i - piece * 65540u;
    const uint32_t len = (n - 65535u * piece) < 65535u ? (n - 65535u * piece) : 65535u;
    switch (r) {
        case 0: return 0u;
        case 1: return len & 0xFFu;
        case 2: return len >> 8;
        case 3: return ~len & 0xFFu;
        case 4: return (~len >> 8) & 0xFFu;
        default: return src[65535u * piece + r - 5u];
    }
}

template <bool DESC, bool DICT = false>
__global__ __launch_bounds__(DEFZ_THREADS)
void k_defz_encode(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, uint64_t *__restrict__ block_bits,
                   const uint8_t *__restrict__ in, uint64_t n_total, uint32_t block, uint64_t block0)
{
    __shared__ uint32_t s_ll[288], s_dc[32];
    typedef BitPacker<DEFZ_THREADS, DEFZ_MAXBITS, false, false> Packer;         // LSB first, into the block's own slot
    __shared__ uint32_t s_scan[Packer::SCAN_WORDS], s_stage[Packer::STAGE_WORDS];
    const int tid = threadIdx.x;
    const uint32_t lb = blockIdx.x;
    const uint8_t *src; uint32_t n;
    lz_block_src<DESC>(in, n_total, block, block0, lb, src, n);
    if constexpr (DICT) { const uint32_t skip = lz_block_skip<true>(in, block0, lb); src += skip; n -= skip; }   // the item's bytes
    uint32_t *out = slots + (size_t)lb * LZ_SLOT_WORDS;
    const uint32_t type = out[DEFZ_TYPE];
    if (type == 0u) {
        const uint32_t np = (n + 65534u) / 65535u, bytes = 5u * np + n + 5u;
        for (uint32_t w = tid; w < (bytes + 3u) / 4u; w += DEFZ_THREADS) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) v |= z_stored_byte(src, n, np, 4u * w + j) << (8u * j);
            out[w] = v;
        }
        if (tid == 0) block_bits[lb] = 8ull * bytes;
        return;
    }
    const uint32_t ntok = (uint32_t)block_bits[lb];
    const uint32_t *trec = trec_all + (size_t)lb * LZ_MAX_BLOCK;
    const uint32_t hbits = out[DEFZ_HBITS], clip = out[DEFZ_CLIP];
    for (int i = tid; i < 288; i += DEFZ_THREADS) s_ll[i] = out[DEFZ_LL + i];
    if (tid < 32) s_dc[tid] = out[DEFZ_DC + tid];
    for (uint32_t i = tid; i < (hbits >> 5); i += DEFZ_THREADS) out[i] = out[DEFZ_HDR + i];      // (regions apart)
    const uint32_t hcarry = (hbits & 31u) ? out[DEFZ_HDR + (hbits >> 5)] : 0u;
    __syncthreads();

    Packer pk(s_stage, s_scan, hbits, hcarry, trec, ntok);
    for (uint32_t t0 = 0; t0 < ntok; t0 += DEFZ_THREADS * 4) {
        const uint32_t t = t0 + (uint32_t)tid * 4;
        const uint4 rv = pk.records(trec, t, ntok);
        const uint32_t r[4] = {rv.x, rv.y, rv.z, rv.w};
        uint32_t v[8], nbit[8], mine = 0;                                  // per token: literal or length code, then a second literal or the distance code
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t &a_v = v[2 * k], &a_k = nbit[2 * k], &b_v = v[2 * k + 1], &b_k = nbit[2 * k + 1];
            a_v = 0; a_k = 0; b_v = 0; b_k = 0;
            if (t + k >= ntok) continue;
            const uint32_t rk = r[k];
            if (rk >> 31) {
                uint32_t L = (rk >> 16) & 0x7FFFu;
                if (clip && t + k == ntok - 1u) {
                    L = clip;
                    if (clip < 3u) {                                       // the clipped match becomes 1 or 2 literals
                        const uint32_t c0 = s_ll[src[n - clip]];
                        a_v = c0 & 0xFFFFu; a_k = c0 >> 16;
                        if (clip == 2u) { const uint32_t c1 = s_ll[src[n - 1u]]; b_v = c1 & 0xFFFFu; b_k = c1 >> 16; }
                        mine += a_k + b_k;
                        continue;
                    }
                }
                uint32_t nb, xv;
                const uint32_t cl = s_ll[z_len_code(L, nb, xv)];
                a_v = (cl & 0xFFFFu) | (xv << (cl >> 16)); a_k = (cl >> 16) + nb;
                const uint32_t cd = s_dc[z_dist_code(rk & 0xFFFFu, nb, xv)];
                b_v = (cd & 0xFFFFu) | (xv << (cd >> 16)); b_k = (cd >> 16) + nb;
            } else {
                const uint32_t c = s_ll[rk & 0xFFu];
                a_v = c & 0xFFFFu; a_k = c >> 16;
            }
            mine += a_k + b_k;
        }
        pk.round(v, nbit, mine, out);
    }
    if (tid == 0) {
        // end-of-block, then the sync flush: 000 (an empty stored block), pad to a byte, 00 00 FF FF
        uint64_t w = pk.qbase >> 5, acc = pk.carry;
        uint32_t pos = (uint32_t)(pk.qbase & 31u);
        const uint32_t eob = s_ll[256];
        acc |= (uint64_t)(eob & 0xFFFFu) << pos;
        pos += (eob >> 16) + 3u;
        pos = (pos + 7u) & ~7u;
        if (pos >= 32u) { out[w++] = (uint32_t)acc; acc >>= 32; pos -= 32u; }
        acc |= (uint64_t)0xFFFF0000u << pos;
        pos += 32u;
        out[w] = (uint32_t)acc;
        if (pos > 32u) out[w + 1] = (uint32_t)(acc >> 32);
        block_bits[lb] = w * 32u + pos;
    }
}

void defz_launch_encode(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, const uint8_t *d_in, uint64_t n,
                        uint32_t block, uint64_t b0, uint32_t nb, bool desc, hipStream_t s, bool dict)
{
    if (dict) {
        hipLaunchKernelGGL(k_defz_plan_dict, dim3(nb), dim3(64), 0, s, trec, slots, block_bits, d_in, n, block, b0);
        hipLaunchKernelGGL((k_defz_encode<true, true>), dim3(nb), dim3(DEFZ_THREADS), 0, s, trec, slots, block_bits, d_in, n, block, b0);
        return;
    }
    if (desc) {
        hipLaunchKernelGGL(k_defz_plan_desc, dim3(nb), dim3(64), 0, s, trec, slots, block_bits, d_in, n, block, b0);
        hipLaunchKernelGGL(k_defz_encode<true>, dim3(nb), dim3(DEFZ_THREADS), 0, s, trec, slots, block_bits, d_in, n, block, b0);
        return;
    }
    hipLaunchKernelGGL(k_defz_plan, dim3(nb), dim3(64), 0, s, trec, slots, block_bits, d_in, n, block, b0);
    hipLaunchKernelGGL(k_defz_encode<false>, dim3(nb), dim3(DEFZ_THREADS), 0, s, trec, slots, block_bits, d_in, n, block, b0);
}

// ---------------------------------------------------------------------------------------------
// checksums.  Workgroup g covers pieces [g * ppg, (g + 1) * ppg) of ZCK_PIECE bytes; thread t a ZCK_SEG-byte segment of
// each piece.  Both checksums are linear in the data, so a segment's part moves to the end of the range by a factor that
// depends only on the number of bytes after it:
//   CRC-32 (pure: zero register, no final xor)  crc(A B) = crc(A) * x^(8 |B|) mod P  xor  crc(B)  (GF(2), reflected)
//   Adler-32 (raw sums a = sum b_i, s = sum (|A| - i) b_i)   a(AB) = a(A) + a(B),  s(AB) = s(A) + |B| a(A) + s(B)
// which is the textbook combine of the standard forms: s1 = s1A + s1B - 1, s2 = s2A + s2B + |B| (s1A - 1) (mod 65521).
// The standard values follow at the end: CRC-32 = crc ^ (0xFFFFFFFF * x^(8n) mod P) ^ 0xFFFFFFFF,
// Adler-32 = (s + n) mod 65521 << 16 | (1 + a) mod 65521.
// ---------------------------------------------------------------------------------------------
// (crc_mulmod, crc_xpow8, zck_segment and the walk of one workgroup over its range, crc_range: crc32.h)
__global__ __launch_bounds__(ZCK_THREADS)
void k_crc32(const uint8_t *__restrict__ in, uint64_t n, uint64_t ppg, uint32_t *__restrict__ parts)
{
    __shared__ CrcLds s_crc;
    const uint32_t tid = threadIdx.x;
    crc_lds_init(s_crc, tid);
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * ppg * ZCK_PIECE;
    const uint64_t hi = lo + ppg * ZCK_PIECE < n ? lo + ppg * ZCK_PIECE : n;
    const uint32_t run = crc_range(in + lo, hi > lo ? hi - lo : 0u, s_crc, tid);
    if (tid == 0) parts[blockIdx.x] = run;
}

// (the raw sums of one workgroup over its range, adler_range: adler32.h)
__global__ __launch_bounds__(ZCK_THREADS)
void k_adler32(const uint8_t *__restrict__ in, uint64_t n, uint64_t ppg, uint32_t *__restrict__ parts)
{
    __shared__ AdlerLds s_red;
    const uint32_t tid = threadIdx.x;
    const bool v16 = (((uintptr_t)in) & 15u) == 0;
    const uint64_t lo = (uint64_t)blockIdx.x * ppg * ZCK_PIECE;
    const uint64_t hi = lo + ppg * ZCK_PIECE < n ? lo + ppg * ZCK_PIECE : n;
    uint32_t ra = 0, rs = 0;                                           // (thread 0) raw sums of [lo, hi), mod 65521
    adler_range(in, lo, hi, v16, s_red, tid, ra, rs);
    if (tid == 0) { parts[2 * blockIdx.x] = ra; parts[2 * blockIdx.x + 1] = rs; }
}

// one workgroup of 1024 threads: partial g covers [g * ppg * PIECE, min(...)) and moves by the bytes after its range
__global__ __launch_bounds__(1024)
void k_crc32_combine(const uint32_t *__restrict__ parts, uint32_t nparts, uint64_t n, uint64_t ppg, uint32_t *__restrict__ result)
{
    __shared__ uint32_t s_red[16];
    const uint32_t g = threadIdx.x;
    uint32_t c = 0;
    if (g < nparts) {
        const uint64_t end = (g + 1ull) * ppg * ZCK_PIECE < n ? (g + 1ull) * ppg * ZCK_PIECE : n;
        c = crc_mulmod(parts[g], crc_xpow8(n - end));
    }
    for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o);
    if ((g & 63u) == 0) s_red[g >> 6] = c;
    __syncthreads();
    if (g == 0) {
        uint32_t v = 0;
        for (int w = 0; w < 16; ++w) v ^= s_red[w];
        *result = v ^ crc_mulmod(0xFFFFFFFFu, crc_xpow8(n)) ^ 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(1024)
void k_adler32_combine(const uint32_t *__restrict__ parts, uint32_t nparts, uint64_t n, uint64_t ppg, uint32_t *__restrict__ result)
{
    __shared__ uint64_t s_red[2][16];
    const uint32_t g = threadIdx.x;
    uint64_t a = 0, s = 0;
    if (g < nparts) {
        const uint64_t end = (g + 1ull) * ppg * ZCK_PIECE < n ? (g + 1ull) * ppg * ZCK_PIECE : n;
        a = parts[2 * g];
        s = ((uint64_t)parts[2 * g + 1] + a * ((n - end) % ADLER_MOD)) % ADLER_MOD;
    }
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); s += __shfl_xor(s, o); }
    if ((g & 63u) == 0) { s_red[0][g >> 6] = a; s_red[1][g >> 6] = s; }
    __syncthreads();
    if (g == 0) {
        uint64_t A = 0, S = 0;
        for (int w = 0; w < 16; ++w) { A += s_red[0][w]; S += s_red[1][w]; }
        const uint32_t s1 = (uint32_t)((1ull + A) % ADLER_MOD), s2 = (uint32_t)((S + n % ADLER_MOD) % ADLER_MOD);
        *result = (s2 << 16) | s1;
    }
}

static_assert(ZCK_GRID <= 1024u, "one combine thread per partial");

size_t defz_ws_bytes() { return 4u * (2u * ZCK_GRID + 64u); }

// partials + combine on `s`; the checksum lands in *d_res.  zws: defz_ws_bytes() of device memory, the caller's to place
mi_status defz_checksum(mi_ctx *ctx, bool crc, const uint8_t *d_in, uint64_t n, void *zws, uint32_t *d_res, hipStream_t s)
{
    uint32_t *ws = (uint32_t *)zws;
    const uint64_t npieces = (n + ZCK_PIECE - 1) / ZCK_PIECE;
    const uint64_t ppg = npieces ? (npieces + ZCK_GRID - 1) / ZCK_GRID : 1;
    const uint32_t grid = (uint32_t)((npieces + ppg - 1) / ppg);
    if (grid) {
        mi_prof_scope pr(ctx, crc ? "k_crc32" : "k_adler32", s, n);
        if (crc) hipLaunchKernelGGL(k_crc32, dim3(grid), dim3(ZCK_THREADS), 0, s, d_in, n, ppg, ws + ZCK_PAIRS_AT);
        else hipLaunchKernelGGL(k_adler32, dim3(grid), dim3(ZCK_THREADS), 0, s, d_in, n, ppg, ws + ZCK_PAIRS_AT);
    }
    if (crc) hipLaunchKernelGGL(k_crc32_combine, dim3(1), dim3(1024), 0, s, ws + ZCK_PAIRS_AT, grid, n, ppg, d_res);
    else hipLaunchKernelGGL(k_adler32_combine, dim3(1), dim3(1024), 0, s, ws + ZCK_PAIRS_AT, grid, n, ppg, d_res);
    return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

uint32_t defz_header_bytes(uint32_t container) { return container == MI_CONTAINER_GZIP ? 10u : container == MI_CONTAINER_ZLIB ? 2u : 0u; }
uint32_t defz_trailer_bytes(uint32_t container) { return container == MI_CONTAINER_GZIP ? 8u : container == MI_CONTAINER_ZLIB ? 4u : 0u; }

// Before the pipeline, on `s`: the words the container header shares with the first record are zeroed (k_lz_concat ORs
// into a word it shares with what comes before it), the running base starts at the header's bit count, the checksum runs.
mi_status defz_begin(mi_ctx *ctx, uint32_t container, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t *base_bits,
                     void *zws, hipStream_t s)
{
    const uint32_t hb = defz_header_bytes(container);
    if (hb) MI_HIP(ctx, hipMemsetAsync(d_out, 0, (hb + 3u) & ~3u, s));
    MI_HIP(ctx, hipMemsetAsync(base_bits, 0, 8, s));
    if (hb) MI_HIP(ctx, hipMemsetAsync(base_bits, (int)(8u * hb), 1, s));             // (<= 80: the low byte)
    if (container == MI_CONTAINER_RAW) return MI_OK;
    uint32_t *ws = (uint32_t *)zws;
    return defz_checksum(ctx, container == MI_CONTAINER_GZIP, d_in, n, ws, ws + ZCK_RESULT_AT, s);
}

__global__ void k_defz_finish(uint8_t *__restrict__ out, uint64_t *__restrict__ block_bits, uint64_t nblocks, uint64_t n,
                              uint32_t container, const uint32_t *__restrict__ ck, uint64_t *__restrict__ out_bytes)
{
    uint32_t hb = 0;
    if (container == MI_CONTAINER_ZLIB) { out[0] = 0x78; out[1] = 0x9C; hb = 2; }
    else if (container == MI_CONTAINER_GZIP) { for (int i = 0; i < 10; ++i) out[i] = kGzip[i]; hb = 10; }
    if (nblocks == 0) block_bits[0] = 8ull * hb;
    uint64_t r = block_bits[nblocks] >> 3;
    // The records end at byte r.  k_lz_concat writes whole words and none at or past cap_bytes / 4 words, and cap_bytes may
    // be the bound exactly, with no slack behind the records beyond the 2 bytes of 03 00 (raw container, all blocks stored):
    // with r = 4k + 1 and cap_bytes = r + 2 the word that holds byte r - 1 is not written.  That byte — at most that one, as
    // 4 floor(cap_bytes / 4) >= cap_bytes - 3 >= r - 1 — is the last byte of a sync flush, and every record ends with one:
    // the flush's 00 00 FF FF is written here again, whole.
    if (nblocks) { out[r - 4] = 0x00; out[r - 3] = 0x00; out[r - 2] = 0xFF; out[r - 1] = 0xFF; }
    out[r++] = 0x03; out[r++] = 0x00;                                  // BFINAL = 1, fixed, end-of-block; padding
    if (container == MI_CONTAINER_ZLIB) {
        const uint32_t a = *ck;
        for (int i = 0; i < 4; ++i) out[r++] = (uint8_t)(a >> (24 - 8 * i));
    } else if (container == MI_CONTAINER_GZIP) {
        const uint32_t c = *ck, isz = (uint32_t)n;
        for (int i = 0; i < 4; ++i) out[r++] = (uint8_t)(c >> (8 * i));
        for (int i = 0; i < 4; ++i) out[r++] = (uint8_t)(isz >> (8 * i));
    }
    *out_bytes = r;
}

mi_status defz_end(mi_ctx *ctx, uint32_t container, uint8_t *d_out, uint64_t *d_block_bits, uint64_t nblocks, uint64_t n,
                   void *zws, uint64_t *d_out_bytes, hipStream_t s)
{
    hipLaunchKernelGGL(k_defz_finish, dim3(1), dim3(1), 0, s, d_out, d_block_bits, nblocks, n, container,
                       (const uint32_t *)zws + ZCK_RESULT_AT, d_out_bytes);
    return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

// mode Z takes the deflate flavour with distances and lengths RFC 1951 can code: wbits <= 15, lbits <= 8, blocks <= 64 KiB; the
// lazy parse (its lengths do not come from the length field) with the deflate defaults wbits 15, lbits 5
mi_status defz_check(const mi_lz_params *p, uint32_t container)
{
    mi_status st = lz_check_fields(p);
    if (st) return st;
    if (!p->deflate || p->wbits > 15 || p->lbits > 8 || p->block > LZ_MAX_BLOCK || container > MI_CONTAINER_GZIP) return MI_ERR_ARG;
    if (p->parse > MI_PARSE_LAZY || (p->parse == MI_PARSE_LAZY && (p->wbits != 15 || p->lbits != 5))) return MI_ERR_ARG;
    return MI_OK;
}

extern "C" uint64_t mi_deflate_z_bound_bytes(uint64_t n, const mi_lz_params *p, uint32_t container)
{
    // per block of b bytes the stored form and the sync flush: b + 5 ceil(b / 65535) + 5 (the encoder never writes more:
    // it takes the shortest of three forms); then the container and the closing 03 00
    const uint64_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK;
    const uint64_t nblocks = (n + block - 1) / block;
    const uint64_t last = n - (nblocks ? (nblocks - 1) * block : 0);
    auto rec = [](uint64_t b) -> uint64_t { return b + 5 * ((b + 65534) / 65535) + 5; };
    const uint64_t c = container <= MI_CONTAINER_GZIP ? defz_header_bytes(container) + defz_trailer_bytes(container) : 18u;
    return (nblocks ? (nblocks - 1) * rec(block) + rec(last) : 0) + c + 2;
}

// the two checksums as entry points: the partials in a workspace of their own
static mi_status zck_dev(mi_ctx *ctx, bool crc, const uint8_t *d_in, uint64_t n, uint32_t *d_res, void *stream)
{
    if (!ctx || !d_res || (n && !d_in)) return MI_ERR_ARG;
    uint8_t *zws;
    const mi_status st = mi_ws_carve(ctx, [&](mi_carver &cv) { cv.take(zws, defz_ws_bytes()); });
    return st ? st : defz_checksum(ctx, crc, d_in, n, zws, d_res, (hipStream_t)stream);
}

extern "C" mi_status mi_crc32_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t *d_crc, void *stream)
{
    return zck_dev(ctx, true, d_in, n, d_crc, stream);
}

extern "C" mi_status mi_adler32_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t *d_adler, void *stream)
{
    return zck_dev(ctx, false, d_in, n, d_adler, stream);
}
