// inflate_core.h — what the DEFLATE readers share (inflate.hip: k_inflate over segments of one stream; inflate_batch.hip:
// k_inflate_batch over unrelated streams): the canonical-code tables and their LUTs, the length / distance alphabets, the
// container header, and inf_blocks, the block and token loop of one wave over one byte-aligned range of DEFLATE blocks.
//
// inf_blocks is parameterised by where the range, the output and the limit come from (its arguments) and by what a full
// output means: with FLIP = false the limit is the segment's length and a byte past it is corruption (k_inflate); with
// FLIP = true the limit is a capacity, and the first token that does not fit flips the wave into COUNTING — from there on
// nothing is stored, the ring is left alone, and only the position moves on, with every bit bound and d <= o still checked.
// COUNT_ONLY is counting from the first byte with no ring at all (the size pass).
#pragma once
#include "lz_common.h"
#include "lz_decode.h"

#ifndef INF_LL_BITS
#define INF_LL_BITS 10
#endif
#ifndef INF_D_BITS
#define INF_D_BITS 9
#endif
#define INF_CL_BITS 7                          // the code-length code: at most 7 bits, the LUT covers it whole
#define INF_NONE    0xFFFFu                    // LUT cell: no code of at most LUT-width bits starts with these bits
static_assert(INF_LL_BITS >= 7 && INF_LL_BITS <= 15 && INF_D_BITS >= INF_CL_BITS && INF_D_BITS <= 15, "LUT widths");

#define INF_MAX_POS 0x7FFFFFFFu                // positions inside a range are 32-bit: a counting wave stops above this

static __constant__ uint8_t kInfOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// One canonical Huffman code, ready to decode: symbols sorted by (length, symbol), per length the number of codes, the
// first code and the index of its symbol in `sorted` (k_defh_decode's s_count / s_next / s_first / s_sorted).
template <int NSYM>
struct InfCode {
    uint16_t sorted[NSYM];
    uint16_t count[16], first[16];
    uint32_t next[16];
};

enum { INF_COMPLETE = 0, INF_ONE_OR_NONE = 1 };

// The symbol whose code starts the bit string `rev` (first stream bit in bit 31), lengths lo..hi tried in turn:
// symbol | length << 9, or INF_NONE.  DEFLATE packs codes MSB-first into an LSB-first stream, hence the reversal.
template <int NSYM>
__device__ __forceinline__ uint32_t inf_walk(const InfCode<NSYM> &c, uint32_t rev, uint32_t lo, uint32_t hi)
{
    for (uint32_t l = lo; l <= hi; ++l) {
        const uint32_t code = rev >> (32u - l), rel = code - c.next[l];
        if (code >= c.next[l] && rel < c.count[l]) return (uint32_t)c.sorted[c.first[l] + rel] | (l << 9);
    }
    return INF_NONE;
}

// Build the tables of one code from len[0, nsym) (nsym <= NSYM, lengths 0..15).  All 64 lanes call it with the same
// arguments; the result is wave-uniform: false if the lengths are over-subscribed, or incomplete — except, with
// INF_ONE_OR_NONE (the distance code), a single code of length 1 (RFC 1951 3.2.7) or no code at all (a block of literals).
template <int LUTB, int NSYM>
__device__ bool inf_build(const uint8_t *len, uint32_t nsym, uint32_t kind, InfCode<NSYM> &c, uint16_t *lut, uint32_t lane)
{
    uint32_t cnt[16];
#pragma unroll
    for (int L = 0; L < 16; ++L) cnt[L] = 0;
    for (uint32_t base = 0; base < nsym; base += 64u) {
        const uint32_t l = base + lane < nsym ? len[base + lane] : 0u;
#pragma unroll
        for (int L = 1; L < 16; ++L) cnt[L] += (uint32_t)__popcll(__ballot(l == (uint32_t)L));
    }
    int32_t left = 1;
    uint32_t used = 0, code = 0, run = 0;
    bool over = false;
    uint32_t nx[16], fi[16];
    nx[0] = 0; fi[0] = 0;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
        code = (code + cnt[L - 1]) << 1;
        nx[L] = code; fi[L] = run;
        run += cnt[L]; used += cnt[L];
        left = left * 2 - (int32_t)cnt[L];
        if (left < 0) over = true;
    }
    if (over) return false;
    if (left > 0 && !(kind == INF_ONE_OR_NONE && (used == 0u || (used == 1u && cnt[1] == 1u)))) return false;
    __syncthreads();                                                   // whoever still reads the tables being replaced
    if (lane == 0) {
        c.count[0] = 0; c.first[0] = 0; c.next[0] = 0;
#pragma unroll
        for (int L = 1; L < 16; ++L) { c.count[L] = (uint16_t)cnt[L]; c.first[L] = (uint16_t)fi[L]; c.next[L] = nx[L]; }
    }
    // symbols by (length, symbol): within a round of 64 symbols the rank among equal lengths is a ballot away
#pragma unroll
    for (int L = 0; L < 16; ++L) cnt[L] = 0;
    for (uint32_t base = 0; base < nsym; base += 64u) {
        const uint32_t s = base + lane, l = s < nsym ? len[s] : 0u;
#pragma unroll
        for (int L = 1; L < 16; ++L) {
            const uint64_t m = __ballot(l == (uint32_t)L);
            if (l == (uint32_t)L) c.sorted[fi[L] + cnt[L] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)s;
            cnt[L] += (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    // every LUT cell finds its own symbol: the cell index is the next LUTB stream bits as they lie
    for (uint32_t i = lane; i < (1u << LUTB); i += 64u) lut[i] = (uint16_t)inf_walk(c, __builtin_bitreverse32(i), 1u, (uint32_t)LUTB);
    __syncthreads();
    return true;
}

// length symbol 257..285 -> base and extra bits; distance code 0..29 likewise (RFC 1951 3.2.5)
__device__ __forceinline__ void inf_len_of(uint32_t sym, uint32_t &base, uint32_t &nb)
{
    const uint32_t i = sym - 257u;
    if (i < 8u) { base = 3u + i; nb = 0; }
    else if (i == 28u) { base = 258u; nb = 0; }
    else { nb = (i >> 2) - 1u; base = 3u + ((4u + (i & 3u)) << nb); }
}
__device__ __forceinline__ void inf_dist_of(uint32_t c, uint32_t &base, uint32_t &nb)
{
    if (c < 4u) { base = 1u + c; nb = 0; }
    else { nb = (c >> 1) - 1u; base = 1u + ((2u + (c & 1u)) << nb); }
}

// The container header in front of the DEFLATE data, read through byte(i) (which flags what lies past the stream): its
// length; `bad` is set where it is not one this library reads.  raw none; zlib CM = 8, CINFO <= 7, FCHECK, FDICT = 0; gzip
// 1F 8B, CM = 8, reserved flag bits zero, FEXTRA / FNAME / FCOMMENT / FHCRC skipped by their lengths (FHCRC not verified).
// With DICT (the caller holds a preset dictionary) a zlib header may have FDICT = 1: it is then 6 bytes, *fdict is set and
// *dictid gets the four bytes behind FLG, big-endian; whether they name the caller's dictionary is the caller's to check.
template <bool DICT = false, typename B>
__device__ __forceinline__ uint64_t inf_header_bytes(uint32_t container, B &&byte, bool &bad, bool *fdict = nullptr, uint32_t *dictid = nullptr)
{
    uint64_t hb = 0;
    if (container == MI_CONTAINER_ZLIB) {
        const uint32_t cmf = byte(0), flg = byte(1);
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (!DICT && (flg & 0x20u))) bad = true;
        hb = 2;
        if constexpr (DICT) {
            if (flg & 0x20u) { *fdict = true; *dictid = (byte(2) << 24) | (byte(3) << 16) | (byte(4) << 8) | byte(5); hb = 6; }
        }
    } else if (container == MI_CONTAINER_GZIP) {
        const uint32_t flg = byte(3);
        if (byte(0) != 0x1Fu || byte(1) != 0x8Bu || byte(2) != 8u || (flg & 0xE0u)) bad = true;
        hb = 10;
        if (flg & 4u) { const uint64_t xlen = byte(10) | (byte(11) << 8); hb += 2u + xlen; }                // FEXTRA
        for (uint32_t f = 8u; f <= 16u && !bad; f <<= 1)                                                       // FNAME, FCOMMENT
            if (flg & f) { while (byte(hb) != 0u && !bad) ++hb; ++hb; }
        if (flg & 2u) hb += 2;                                                                                 // FHCRC (not verified)
    }
    return hb;
}

// What a walk leaves behind.  bad: the range is not well-formed (or, big: it is, but inflates past INF_MAX_POS bytes);
// counting: the output limit was passed, `o` went on counting.  Every member is wave-uniform.
struct InfWalk {
    uint64_t pos;                                                      // bits used; a stored range of 2^31 - 1 bytes has 2^34
    uint32_t o;
    bool bad, final_seen, counting, big;
};

// The blocks of the bit range [rb, rb + nbits) of `stream` (rb a multiple of 8), one wave, into the n bytes at outp
// through `ring`.  may_end: a block with BFINAL = 1 may close the range.  Every control value is wave-uniform (lz_decode.h): the
// only memory on a token's critical path is its LUT cell.  The caller checks how the range ended (pos, o, final_seen) and
// calls ring.finish.
// DICT (a FLIP mode): the `dn` <= 32 768 bytes that end at `dend` lie in front of the output as a preset dictionary — a
// distance may be up to o + dn, in all three modes, and positions below 0 are dictionary bytes (OutRing::copy_dict).
// dn = 0: a range that does not use the dictionary, decoded as without DICT.
template <uint32_t RING, bool FLIP, bool COUNT_ONLY, bool DICT = false>
__device__ __forceinline__ InfWalk inf_blocks(const uint8_t *__restrict__ stream, uint64_t rb, uint64_t nbits, uint8_t *outp, uint32_t n,
                                              bool may_end, OutRing<RING> &ring, uint8_t *s_ring, uint16_t *s_llut, uint16_t *s_dlut,
                                              InfCode<288> &s_ll, InfCode<32> &s_dc, uint8_t *s_len, uint8_t *s_cl, uint32_t lane,
                                              const uint8_t *dend = nullptr, uint32_t dn = 0)
{
    static_assert(FLIP || !COUNT_ONLY, "counting is a FLIP mode");
    static_assert(FLIP || !DICT, "a dictionary is a FLIP mode");
    BitsLsb br;
    br.init(stream, rb, nbits, lane);
    ring.init(s_ring, outp, lane);
    if constexpr (DICT && !COUNT_ONLY) {
        ring.preload(dend, dn);
        __builtin_amdgcn_wave_barrier();
    }
    uint64_t pos = 0;
    uint32_t o = 0;
    bool bad = false, fixed_built = false, final_seen = false, counting = COUNT_ONLY, big = false;
    while (pos < nbits && !bad) {
        br.refill();
        const uint32_t hdr = br.peek(3);
        br.skip(3); pos += 3;
        const uint32_t bfinal = hdr & 1u, btype = hdr >> 1;
        if (btype == 3u || (bfinal && !may_end)) { bad = true; break; }
        if (btype == 0u) {
            // ---- stored: to the byte boundary, LEN, NLEN, then LEN bytes straight from the stream, lane-parallel
            const uint32_t pad = (uint32_t)(0u - pos) & 7u;
            br.skip(pad); pos += pad;
            br.refill();
            const uint32_t len = br.peek(16);
            br.skip(16);
            br.refill();
            const uint32_t nlen = br.peek(16);
            br.skip(16); pos += 32;
            if constexpr (FLIP) {
                if ((len ^ nlen) != 0xFFFFu || pos + 8ull * len > nbits) { bad = true; break; }
                if (!COUNT_ONLY && !counting && len > n - o) counting = true;
            } else {
                if ((len ^ nlen) != 0xFFFFu || pos + 8ull * len > nbits || len > n - o) { bad = true; break; }
            }
            if (FLIP && (COUNT_ONLY || counting)) {
                if (len > INF_MAX_POS - o) { bad = true; big = true; break; }
                o += len;
            } else if constexpr (!COUNT_ONLY) {
                const uint8_t *src = stream + ((rb + pos) >> 3);
                for (uint32_t done = 0; done < len;) {                  // (OutRing::advance flushes one quarter per call)
                    const uint32_t piece = len - done < OutRing<RING>::CH ? len - done : OutRing<RING>::CH;
                    for (uint32_t j = lane; j < piece; j += 64u) s_ring[(o + j) & OutRing<RING>::RM] = src[done + j];
                    done += piece; o += piece;
                    __builtin_amdgcn_wave_barrier();
                    ring.advance(o);
                }
            }
            pos += 8ull * len;
            if (pos < nbits && !bfinal) br.init(stream, rb + pos, nbits - pos, lane);
        } else {
            if (btype == 1u) {
                if (!fixed_built) {
                    for (uint32_t s = lane; s < 288u; s += 64u) s_len[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
                    if (lane < 32u) s_len[288u + lane] = 5;
                    __syncthreads();
                    inf_build<INF_LL_BITS>(s_len, 288u, INF_COMPLETE, s_ll, s_llut, lane);
                    inf_build<INF_D_BITS>(s_len + 288u, 32u, INF_COMPLETE, s_dc, s_dlut, lane);
                    fixed_built = true;
                }
            } else {
                // ---- dynamic: HLIT, HDIST, HCLEN, the code-length code in RFC order, then HLIT + HDIST lengths as ONE sequence
                fixed_built = false;
                br.refill();
                const uint32_t h = br.peek(14);
                br.skip(14); pos += 14;
                const uint32_t hlit = (h & 31u) + 257u, hdist = ((h >> 5) & 31u) + 1u, hclen = (h >> 10) + 4u;
                if (hlit > 286u || hdist > 30u) { bad = true; break; }
                if (lane < 20u) s_cl[lane] = 0;
                __syncthreads();
                for (uint32_t i = 0; i < hclen; ++i) {
                    br.refill();
                    if (lane == 0) s_cl[kInfOrder[i]] = (uint8_t)br.peek(3);
                    br.skip(3); pos += 3;
                }
                __syncthreads();
                if (!inf_build<INF_CL_BITS>(s_cl, 19u, INF_COMPLETE, s_dc, s_dlut, lane)) { bad = true; break; }
                const uint32_t total = hlit + hdist;
                uint32_t prev = 0;
                for (uint32_t idx = 0; idx < total;) {                  // every step adds at least one length: <= 316 steps
                    br.refill();
                    const uint32_t e = s_dlut[br.peek(INF_CL_BITS)];
                    if (e == INF_NONE) { bad = true; break; }
                    const uint32_t sym = e & 511u, l = e >> 9;
                    br.skip(l); pos += l;
                    if (sym < 16u) {
                        if (lane == 0) s_len[idx] = (uint8_t)sym;
                        prev = sym; idx += 1u;
                    } else {
                        const uint32_t xb = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
                        const uint32_t rep = (sym == 18u ? 11u : 3u) + br.peek(xb);
                        br.skip(xb); pos += xb;
                        if ((sym == 16u && idx == 0u) || idx + rep > total) { bad = true; break; }
                        const uint32_t v = sym == 16u ? prev : 0u;
                        for (uint32_t j = lane; j < rep; j += 64u) s_len[idx + j] = (uint8_t)v;
                        prev = v; idx += rep;
                    }
                }
                if (bad || pos > nbits) { bad = true; break; }
                __syncthreads();
                if (s_len[256] == 0u) { bad = true; break; }            // no end-of-block code: the block could not end
                if (!inf_build<INF_LL_BITS>(s_len, hlit, INF_COMPLETE, s_ll, s_llut, lane)) { bad = true; break; }
                if (!inf_build<INF_D_BITS>(s_len + hlit, hdist, INF_ONE_OR_NONE, s_dc, s_dlut, lane)) { bad = true; break; }
            }
            // ---- tokens until end-of-block.  Every token uses at least one bit and the loop stops past the range's last.
            for (;;) {
                br.refill();
                uint32_t e = s_llut[br.peek(INF_LL_BITS)];
                if (e == INF_NONE) {
                    e = inf_walk(s_ll, __builtin_bitreverse32((uint32_t)br.buf), INF_LL_BITS + 1u, 15u);
                    if (e == INF_NONE) { bad = true; break; }
                }
                const uint32_t sym = e & 511u, l = e >> 9;
                br.skip(l); pos += l;
                if (sym < 256u) {
                    if constexpr (FLIP) {
                        if (!COUNT_ONLY && !counting && o >= n) counting = true;
                        if (COUNT_ONLY || counting) { if (o >= INF_MAX_POS) { bad = true; big = true; break; } }
                        else ring.put_literal(o, sym);
                    } else {
                        if (o >= n) { bad = true; break; }
                        ring.put_literal(o, sym);
                    }
                    o += 1u;
                } else if (sym == 256u) {
                    break;
                } else {
                    if (sym > 285u) { bad = true; break; }
                    uint32_t base, nb;
                    inf_len_of(sym, base, nb);
                    const uint32_t len = base + br.peek(nb);            // <= 15 + 5 bits since the refill
                    br.skip(nb); pos += nb;
                    br.refill();
                    uint32_t ed = s_dlut[br.peek(INF_D_BITS)];
                    if (ed == INF_NONE) {
                        ed = inf_walk(s_dc, __builtin_bitreverse32((uint32_t)br.buf), INF_D_BITS + 1u, 15u);
                        if (ed == INF_NONE) { bad = true; break; }
                    }
                    const uint32_t dcode = ed & 511u, dl = ed >> 9;
                    br.skip(dl); pos += dl;
                    if (dcode > 29u) { bad = true; break; }
                    inf_dist_of(dcode, base, nb);
                    const uint32_t d = base + br.peek(nb);              // <= 15 + 13 bits since the refill
                    br.skip(nb); pos += nb;
                    if constexpr (FLIP) {
                        if (d > o + (DICT ? dn : 0u)) { bad = true; break; }    // before the range's first byte (the dictionary's)
                        if (!COUNT_ONLY && !counting && len > n - o) counting = true;   // a match is written whole or not at all
                        if (COUNT_ONLY || counting) { if (len > INF_MAX_POS - o) { bad = true; big = true; break; } }
                        else if (DICT && d > o) ring.copy_dict(o, d, len, dend);
                        else ring.copy(o, d, len);
                    } else {
                        if (d > o || len > n - o) { bad = true; break; }    // before the segment's first byte / past its last
                        ring.copy(o, d, len);
                    }
                    o += len;
                }
                if (pos > nbits) { bad = true; break; }
                if (FLIP && (COUNT_ONLY || counting)) continue;         // counting: no ring traffic
                if constexpr (!COUNT_ONLY) {
                    __builtin_amdgcn_wave_barrier();
                    ring.advance(o);
                }
            }
            if (bad) break;
        }
        if (pos > nbits) { bad = true; break; }
        if (bfinal) { final_seen = true; break; }
    }
    return InfWalk{pos, o, bad, final_seen, counting, big};
}
