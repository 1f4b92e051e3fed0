// inflate.hip — standard DEFLATE (RFC 1951) read back on the GPU from a table of restart points.
//
// Mode Z (defz.hip) writes one byte-aligned record per input block that refers to nothing before it, and its table gives
// the bit offset of every record.  Stock zlib writes the same layout when it is given Z_FULL_FLUSH every `block` input
// bytes.  A SEGMENT here is the stream between two table entries: whole DEFLATE blocks of any type that inflate to exactly
// `block` bytes (the last one to the rest).  include/mi_codec.h has the contract.
//
//   k_inflate<RING>   one wave per segment, the shape of k_defh_decode: wave-uniform control flow, the bit buffer in SGPRs
//                     fed from WaveWords (BitsLsb), the last RING bytes of output in an LDS OutRing, far matches read back
//                     from the output buffer.  Stored, fixed and dynamic blocks, the whole RFC alphabet.
//   k_inflate_frame   one lane: the container header, the closing blocks behind the last segment, the trailer, the
//                     comparison of the checksum (mi_crc32_dev / mi_adler32_dev over the decoded bytes) with the trailer.
//
// LDS per wave with the 4 KiB ring: 4096 (ring) + 2048 (10-bit literal/length LUT) + 1024 (9-bit distance LUT) + 640
// (symbols by code) + 256 (count / first code / first index per length, twice) + 344 (code lengths) = 8 420 bytes: 19 waves
// in a CU's 160 KiB (the kernel's 97 VGPRs allow 16).  DESIGN.md 3.5 has the measured figures.
#include "lz_common.h"
#include "lz_decode.h"
#include "internal.h"
#include <stdlib.h>

#ifndef INF_LL_BITS
#define INF_LL_BITS 10
#endif
#ifndef INF_D_BITS
#define INF_D_BITS 9
#endif
#define INF_CL_BITS 7                          // the code-length code: at most 7 bits, the LUT covers it whole
#define INF_NONE    0xFFFFu                    // LUT cell: no code of at most LUT-width bits starts with these bits
static_assert(INF_LL_BITS >= 7 && INF_LL_BITS <= 15 && INF_D_BITS >= INF_CL_BITS && INF_D_BITS <= 15, "LUT widths");

// status words behind the checksum partials in the context workspace
#define INF_WS_CK    0u                        // the checksum of the decoded bytes
#define INF_WS_FINAL 1u                        // set by k_inflate: the (only) segment ended with its BFINAL = 1 block

__constant__ uint8_t kInfOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

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

// DESC (BGZF, bgzf.hip): `seg_bits` points at one InfSeg descriptor per segment instead of the table — the segment's first
// and last bit, output offset and output length; block, nseg and n_total are not used.  Every segment is a whole DEFLATE
// stream then: its last block, and only that one, has BFINAL = 1.
template <uint32_t RING, bool DESC = false>
__global__ __launch_bounds__(64)
void k_inflate(const uint8_t *__restrict__ stream, uint64_t stream_bytes, const uint64_t *__restrict__ seg_bits, uint32_t block,
               uint64_t nseg, uint8_t *__restrict__ out, uint64_t n_total, uint32_t *__restrict__ status, uint32_t *__restrict__ err)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[RING];
    __shared__ uint16_t s_llut[1 << INF_LL_BITS], s_dlut[1 << INF_D_BITS];     // symbol | length << 9
    __shared__ InfCode<288> s_ll;
    __shared__ InfCode<32> s_dc;                                       // the distance code; the code-length code while a header is read
    __shared__ __attribute__((aligned(4))) uint8_t s_len[288 + 32 + 4], s_cl[20];
    const uint32_t lane = threadIdx.x;
    const uint64_t sg = blockIdx.x;
    InfSeg d = {};
    if constexpr (DESC) d = reinterpret_cast<const InfSeg *>(seg_bits)[sg];
    const uint64_t off = DESC ? d.out_off : sg * (uint64_t)block;
    const uint32_t n = DESC ? d.out_len : (uint32_t)((n_total - off) < block ? (n_total - off) : block);
    const uint64_t rb = DESC ? d.first_bit : seg_bits[sg], re = DESC ? d.last_bit : seg_bits[sg + 1];
    // the segment must lie inside the stream, on byte boundaries: every later read is bounded by [rb, re)
    bool bad = ((rb | re) & 7u) || re < rb || re > stream_bytes * 8ull;
    if (bad) { if (lane == 0) atomicOr(err, 1u); return; }
    const uint64_t nbits = re - rb;
    const bool may_end = DESC || nseg == 1u;                           // the one-segment rule: BFINAL = 1 may close the segment

    // every control value below is wave-uniform (lz_decode.h): the only memory on a token's critical path is its LUT cell
    BitsLsb br;
    br.init(stream, rb, nbits, lane);
    OutRing<RING> ring;
    ring.init(s_ring, out + off, lane);
    uint64_t pos = 0;                                                  // bits used; a stored segment of 2^31 - 1 bytes has 2^34
    uint32_t o = 0;
    bool fixed_built = false, final_seen = false;
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
            if ((len ^ nlen) != 0xFFFFu || pos + 8ull * len > nbits || len > n - o) { bad = true; break; }
            const uint8_t *src = stream + ((rb + pos) >> 3);
            for (uint32_t done = 0; done < len;) {                      // (OutRing::advance flushes one quarter per call)
                const uint32_t piece = len - done < OutRing<RING>::CH ? len - done : OutRing<RING>::CH;
                for (uint32_t j = lane; j < piece; j += 64u) s_ring[(o + j) & OutRing<RING>::RM] = src[done + j];
                done += piece; o += piece;
                __builtin_amdgcn_wave_barrier();
                ring.advance(o);
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
            // ---- tokens until end-of-block.  Every token uses at least one bit and the loop stops past the segment's last.
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
                    if (o >= n) { bad = true; break; }
                    ring.put_literal(o, sym);
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
                    if (d > o || len > n - o) { bad = true; break; }    // before the segment's first byte / past its last
                    ring.copy(o, d, len);
                    o += len;
                }
                if (pos > nbits) { bad = true; break; }
                __builtin_amdgcn_wave_barrier();
                ring.advance(o);
            }
            if (bad) break;
        }
        if (pos > nbits) { bad = true; break; }
        if (bfinal) { final_seen = true; break; }
    }
    // the segment's bits are used up exactly (after BFINAL = 1: up to the padding of its last byte), and so is its output
    if (final_seen ? ((pos + 7u) & ~7ull) != nbits : pos != nbits) bad = true;
    if (o != n) bad = true;
    if (DESC && !final_seen) bad = true;
    if (bad) { if (lane == 0) atomicOr(err, 1u); return; }
    ring.finish(n);
    if (!DESC && final_seen && lane == 0) status[INF_WS_FINAL] = 1u;
}

// BGZF: one wave per member descriptor (the caller has checked every descriptor against the stream and the output range)
void inflate_launch_segments(const uint8_t *d_stream, uint64_t stream_bytes, const InfSeg *d_seg, uint32_t nseg, uint8_t *d_out,
                             uint32_t *err, hipStream_t s)
{
    const uint64_t *desc = reinterpret_cast<const uint64_t *>(d_seg);
    if (nseg >= 1024u) hipLaunchKernelGGL((k_inflate<4096u, true>), dim3(nseg), dim3(64), 0, s, d_stream, stream_bytes, desc, 0u, (uint64_t)nseg, d_out, (uint64_t)0, (uint32_t *)nullptr, err);
    else hipLaunchKernelGGL((k_inflate<32768u, true>), dim3(nseg), dim3(64), 0, s, d_stream, stream_bytes, desc, 0u, (uint64_t)nseg, d_out, (uint64_t)0, (uint32_t *)nullptr, err);
}

// The frame around the segments, read by one lane: bytes past the stream read as zero and count as corrupt.
__global__ __launch_bounds__(64)
void k_inflate_frame(const uint8_t *__restrict__ stream, uint64_t stream_bytes, const uint64_t *__restrict__ seg_bits, uint64_t nseg,
                     uint64_t n, uint32_t container, uint32_t flags, const uint32_t *__restrict__ status, uint32_t *__restrict__ err)
{
    if (threadIdx.x != 0) return;
    bool bad = false;
    auto byte = [&](uint64_t i) -> uint32_t { if (i >= stream_bytes) { bad = true; return 0u; } return stream[i]; };
    // ---- header
    uint64_t hb = 0;
    if (container == MI_CONTAINER_ZLIB) {
        const uint32_t cmf = byte(0), flg = byte(1);
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 0x20u)) bad = true;
        hb = 2;
    } else if (container == MI_CONTAINER_GZIP) {
        const uint32_t flg = byte(3);
        if (byte(0) != 0x1Fu || byte(1) != 0x8Bu || byte(2) != 8u || (flg & 0xE0u)) bad = true;
        hb = 10;
        if (flg & 4u) { const uint64_t xlen = byte(10) | (byte(11) << 8); hb += 2u + xlen; }                // FEXTRA
        for (uint32_t f = 8u; f <= 16u && !bad; f <<= 1)                                                       // FNAME, FCOMMENT
            if (flg & f) { while (byte(hb) != 0u && !bad) ++hb; ++hb; }
        if (flg & 2u) hb += 2;                                                                                 // FHCRC (not verified)
    }
    const uint64_t first = seg_bits[0], last = seg_bits[nseg];
    if (first != 8ull * hb || (last & 7u) || last < first || last > stream_bytes * 8ull) bad = true;
    if (bad) { atomicOr(err, 1u); return; }
    // ---- closing part: blocks without bytes up to BFINAL = 1 (stored with LEN 0, or fixed with end-of-block alone),
    // unless the only segment ended with its own BFINAL = 1 block
    uint64_t p = last;                                                 // bit position
    auto bits = [&](uint32_t k) -> uint32_t {                          // k <= 16, LSB first
        uint32_t v = 0;
        for (uint32_t i = 0; i < k; ++i, ++p) v |= ((byte(p >> 3) >> (p & 7u)) & 1u) << i;
        return v;
    };
    if (!status[INF_WS_FINAL]) {
        for (;;) {                                                     // every round uses at least 3 bits of the stream
            const uint32_t bfinal = bits(1), btype = bits(2);
            if (btype == 0u) {
                p = (p + 7u) & ~7ull;
                const uint32_t len = bits(16), nlen = bits(16);
                if (len != 0u || nlen != 0xFFFFu) bad = true;
            } else if (btype == 1u) {
                if (bits(7) != 0u) bad = true;
            } else bad = true;
            if (bad || bfinal) break;
        }
    }
    uint64_t t = (p + 7u) >> 3;
    // ---- trailer, and nothing behind it
    if (container == MI_CONTAINER_ZLIB) {
        const uint32_t a = (byte(t) << 24) | (byte(t + 1) << 16) | (byte(t + 2) << 8) | byte(t + 3);
        if (!(flags & MI_INFLATE_NO_CHECKSUM) && a != status[INF_WS_CK]) bad = true;
        t += 4;
    } else if (container == MI_CONTAINER_GZIP) {
        const uint32_t c = byte(t) | (byte(t + 1) << 8) | (byte(t + 2) << 16) | (byte(t + 3) << 24);
        const uint32_t isz = byte(t + 4) | (byte(t + 5) << 8) | (byte(t + 6) << 16) | (byte(t + 7) << 24);
        if (!(flags & MI_INFLATE_NO_CHECKSUM) && c != status[INF_WS_CK]) bad = true;
        if (isz != (uint32_t)n) bad = true;
        t += 8;
    }
    if (t != stream_bytes) bad = true;
    if (bad) atomicOr(err, 1u);
}

extern "C" mi_status mi_inflate_dev(mi_ctx *ctx, uint32_t container, uint32_t block, const uint8_t *d_stream, uint64_t stream_bytes,
                                    const uint64_t *d_seg_bits, uint8_t *d_out, uint64_t n, uint32_t flags, void *stream)
{
    if (!ctx || !d_stream || !d_seg_bits || (n && !d_out)) return MI_ERR_ARG;
    if (container > MI_CONTAINER_GZIP || block == 0u || block > 0x7FFFFFFFu || (flags & ~MI_INFLATE_NO_CHECKSUM)) return MI_ERR_ARG;
    if (((uintptr_t)d_stream & 3u) || stream_bytes > (UINT64_MAX >> 3)) return MI_ERR_ARG;
    const uint64_t nseg = (n + block - 1) / block;
    if (nseg > 0x7FFFFFFFull) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t ck_bytes = mi_align_up(defz_ws_bytes(), 256);
    mi_status st = mi_ws_reserve(ctx, ck_bytes + 256);
    if (st) return st;
    uint32_t *status = (uint32_t *)((uint8_t *)ctx->ws + ck_bytes);
    MI_HIP(ctx, hipMemsetAsync(status, 0, 8, s));
    uint32_t *err = mi_err_slot(ctx, s);
    if (!err) return MI_ERR_HIP;
    if (nseg) {
        mi_prof_scope pr(ctx, "k_inflate", s, n);
        // a 4 KiB ring (lz_decode.h): far matches read the output buffer.  Few segments cannot fill the CUs anyway and get
        // the whole 32 KiB window in LDS.
        const char *e = getenv("MI_LZ_DECODE_RING");
        const uint32_t want = e ? (uint32_t)atoi(e) : (nseg < 1024u ? 32768u : 4096u);
        if (want <= 4096u) hipLaunchKernelGGL(k_inflate<4096u>, dim3((unsigned)nseg), dim3(64), 0, s, d_stream, stream_bytes, d_seg_bits, block, nseg, d_out, n, status, err);
        else hipLaunchKernelGGL(k_inflate<32768u>, dim3((unsigned)nseg), dim3(64), 0, s, d_stream, stream_bytes, d_seg_bits, block, nseg, d_out, n, status, err);
        if (hipGetLastError() != hipSuccess) return MI_ERR_HIP;
    }
    if (container != MI_CONTAINER_RAW && !(flags & MI_INFLATE_NO_CHECKSUM)) {
        st = container == MI_CONTAINER_GZIP ? mi_crc32_dev(ctx, d_out, n, status + INF_WS_CK, s) : mi_adler32_dev(ctx, d_out, n, status + INF_WS_CK, s);
        if (st) return st;
    }
    hipLaunchKernelGGL(k_inflate_frame, dim3(1), dim3(64), 0, s, d_stream, stream_bytes, d_seg_bits, nseg, n, container, flags, status, err);
    if (hipGetLastError() != hipSuccess) return MI_ERR_HIP;
    uint32_t h_err = 0;
    MI_HIP(ctx, hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return h_err ? MI_ERR_CORRUPT : MI_OK;
}

// host buffers: the table is checked before anything is copied; copy in, decode, copy out
extern "C" mi_status mi_inflate(mi_ctx *ctx, uint32_t container, uint32_t block, const uint8_t *h_stream, uint64_t stream_bytes,
                                const uint64_t *h_seg_bits, uint8_t *h_out, uint64_t n, uint32_t flags)
{
    if (!ctx || !h_stream || !h_seg_bits || (n && !h_out) || block == 0u) return MI_ERR_ARG;
    const uint64_t nseg = (n + block - 1) / block;
    mi_status st = mi_validate_block_table(h_seg_bits, nseg, stream_bytes, 8u);
    if (st) return st;
    hipStream_t s = mi_host_stream(ctx);
    uint8_t *d_stream = nullptr, *d_out = nullptr; uint64_t *d_bits = nullptr;
    if (hipMalloc(&d_stream, stream_bytes + 64) != hipSuccess || hipMalloc(&d_bits, (nseg + 1) * 8) != hipSuccess ||
        hipMalloc(&d_out, n + 16) != hipSuccess) st = MI_ERR_NOMEM;
    if (st == MI_OK && stream_bytes && hipMemcpyAsync(d_stream, h_stream, stream_bytes, hipMemcpyHostToDevice, s) != hipSuccess) st = MI_ERR_HIP;
    if (st == MI_OK && hipMemcpyAsync(d_bits, h_seg_bits, (nseg + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) st = MI_ERR_HIP;
    if (st == MI_OK) st = mi_inflate_dev(ctx, container, block, d_stream, stream_bytes, d_bits, d_out, n, flags, s);
    if (st == MI_OK && n && hipMemcpy(h_out, d_out, n, hipMemcpyDeviceToHost) != hipSuccess) st = MI_ERR_HIP;
    if (st == MI_ERR_HIP && !ctx->last_hip) ctx->last_hip = (int)hipGetLastError();
    (void)hipFree(d_stream); (void)hipFree(d_bits); (void)hipFree(d_out);
    return st;
}
