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
// the LUT widths (inflate_core.h takes them from here and has the same values as its defaults for inflate_batch.hip)
#ifndef INF_LL_BITS
#define INF_LL_BITS 10
#endif
#ifndef INF_D_BITS
#define INF_D_BITS 9
#endif
#include "inflate_core.h"               // the tables, the header rules and the block and token loop, shared with inflate_batch.hip
#include "internal.h"
#include <stdlib.h>

// status words behind the checksum partials in the context workspace
#define INF_WS_CK    0u                        // the checksum of the decoded bytes
#define INF_WS_FINAL 1u                        // set by k_inflate: the (only) segment ended with its BFINAL = 1 block
#define INF_WS_WORDS 2u

// DESC (BGZF, bgzf.hip): `seg_bits` points at one InfSeg descriptor per segment instead of the table — the segment's first
// and last bit, output offset and output length; block, nseg and n_total are not used.  Every segment is a whole DEFLATE
// stream then: its last block, and only that one, has BFINAL = 1.  seg_status (DESC only, may be NULL; bgzf_ranges.hip): one
// word per segment instead of the one `err` word — a segment whose word is not zero on entry is not decoded at all, and a
// segment that fails sets its own word to 1, so that no verdict reaches another segment's owner.
template <uint32_t RING, bool DESC = false>
__global__ __launch_bounds__(64)
void k_inflate(const uint8_t *__restrict__ stream, uint64_t stream_bytes, const uint64_t *__restrict__ seg_bits, uint32_t block,
               uint64_t nseg, uint8_t *__restrict__ out, uint64_t n_total, uint32_t *__restrict__ status, uint32_t *__restrict__ err,
               uint32_t *__restrict__ seg_status)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[RING];
    __shared__ uint16_t s_llut[1 << INF_LL_BITS], s_dlut[1 << INF_D_BITS];     // symbol | length << 9
    __shared__ InfCode<288> s_ll;
    __shared__ InfCode<32> s_dc;                                       // the distance code; the code-length code while a header is read
    __shared__ __attribute__((aligned(4))) uint8_t s_len[288 + 32 + 4], s_cl[20];
    const uint32_t lane = threadIdx.x;
    const uint64_t sg = blockIdx.x;
    if (DESC && seg_status && seg_status[sg] != 0u) return;            // (the whole wave: inert or refused before it got here)
    auto fail = [&]() { if (lane == 0) { if (DESC && seg_status) seg_status[sg] = 1u; else atomicOr(err, 1u); } };
    InfSeg d = {};
    if constexpr (DESC) d = reinterpret_cast<const InfSeg *>(seg_bits)[sg];
    const uint64_t off = DESC ? d.out_off : sg * (uint64_t)block;
    const uint32_t n = DESC ? d.out_len : (uint32_t)((n_total - off) < block ? (n_total - off) : block);
    const uint64_t rb = DESC ? d.first_bit : seg_bits[sg], re = DESC ? d.last_bit : seg_bits[sg + 1];
    // the segment must lie inside the stream, on byte boundaries: every later read is bounded by [rb, re)
    bool bad = ((rb | re) & 7u) || re < rb || re > stream_bytes * 8ull;
    if (bad) { fail(); return; }
    const uint64_t nbits = re - rb;
    const bool may_end = DESC || nseg == 1u;                           // the one-segment rule: BFINAL = 1 may close the segment

    // the block and token loop (inflate_core.h): a byte past the segment's last is corruption here
    OutRing<RING> ring;
    const InfWalk w = inf_blocks<RING, false, false>(stream, rb, nbits, out + off, n, may_end, ring, s_ring, s_llut, s_dlut, s_ll, s_dc, s_len, s_cl, lane);
    const uint64_t pos = w.pos;
    const uint32_t o = w.o;
    const bool final_seen = w.final_seen;
    bad = w.bad;
    // the segment's bits are used up exactly (after BFINAL = 1: up to the padding of its last byte), and so is its output
    if (final_seen ? ((pos + 7u) & ~7ull) != nbits : pos != nbits) bad = true;
    if (o != n) bad = true;
    if (DESC && !final_seen) bad = true;
    if (bad) { fail(); return; }
    ring.finish(n);
    if (!DESC && final_seen && lane == 0) status[INF_WS_FINAL] = 1u;
}

// BGZF: one wave per member descriptor (the caller has checked every descriptor against the stream and the output range)
void inflate_launch_segments(const uint8_t *d_stream, uint64_t stream_bytes, const InfSeg *d_seg, uint32_t nseg, uint8_t *d_out,
                             uint32_t *err, hipStream_t s, uint32_t *seg_status)
{
    const uint64_t *desc = reinterpret_cast<const uint64_t *>(d_seg);
    if (nseg >= 1024u) hipLaunchKernelGGL((k_inflate<4096u, true>), dim3(nseg), dim3(64), 0, s, d_stream, stream_bytes, desc, 0u, (uint64_t)nseg, d_out, (uint64_t)0, (uint32_t *)nullptr, err, seg_status);
    else hipLaunchKernelGGL((k_inflate<32768u, true>), dim3(nseg), dim3(64), 0, s, d_stream, stream_bytes, desc, 0u, (uint64_t)nseg, d_out, (uint64_t)0, (uint32_t *)nullptr, err, seg_status);
}

// The frame around the segments, read by one lane: bytes past the stream read as zero and count as corrupt.
__global__ __launch_bounds__(64)
void k_inflate_frame(const uint8_t *__restrict__ stream, uint64_t stream_bytes, const uint64_t *__restrict__ seg_bits, uint64_t nseg,
                     uint64_t n, uint32_t container, uint32_t flags, const uint32_t *__restrict__ status, uint32_t *__restrict__ err)
{
    if (threadIdx.x != 0) return;
    bool bad = false;
    auto byte = [&](uint64_t i) -> uint32_t { if (i >= stream_bytes) { bad = true; return 0u; } return stream[i]; };
    // ---- header (inflate_core.h)
    const uint64_t hb = inf_header_bytes(container, byte, bad);
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
    uint8_t *zws; uint32_t *status;                      // the checksum's partials, then the status words
    mi_status st = mi_ws_carve(ctx, [&](mi_carver &cv) { cv.take(zws, defz_ws_bytes()); cv.take(status, INF_WS_WORDS); });
    if (st) return st;
    MI_HIP(ctx, hipMemsetAsync(status, 0, INF_WS_WORDS * 4, s));
    uint32_t *err = mi_err_slot(ctx, s);
    if (!err) return MI_ERR_HIP;
    if (nseg) {
        mi_prof_scope pr(ctx, "k_inflate", s, n);
        // a 4 KiB ring (lz_decode.h): far matches read the output buffer.  Few segments cannot fill the CUs anyway and get
        // the whole 32 KiB window in LDS.
        const uint32_t want = lz_decode_ring_want(nseg, 32768u, 4096u);
        if (want <= 4096u) hipLaunchKernelGGL(k_inflate<4096u>, dim3((unsigned)nseg), dim3(64), 0, s, d_stream, stream_bytes, d_seg_bits, block, nseg, d_out, n, status, err, (uint32_t *)nullptr);
        else hipLaunchKernelGGL(k_inflate<32768u>, dim3((unsigned)nseg), dim3(64), 0, s, d_stream, stream_bytes, d_seg_bits, block, nseg, d_out, n, status, err, (uint32_t *)nullptr);
        if (hipGetLastError() != hipSuccess) return MI_ERR_HIP;
    }
    if (container != MI_CONTAINER_RAW && !(flags & MI_INFLATE_NO_CHECKSUM)) {
        st = defz_checksum(ctx, container == MI_CONTAINER_GZIP, d_out, n, zws, status + INF_WS_CK, s);
        if (st) return st;
    }
    hipLaunchKernelGGL(k_inflate_frame, dim3(1), dim3(64), 0, s, d_stream, stream_bytes, d_seg_bits, nseg, n, container, flags, status, err);
    if (hipGetLastError() != hipSuccess) return MI_ERR_HIP;
    uint32_t h_err = 0;
    MI_HIP(ctx, hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return h_err ? MI_ERR_CORRUPT : MI_OK;
}
