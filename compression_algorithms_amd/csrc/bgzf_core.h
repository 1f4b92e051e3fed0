// bgzf_core.h — what the BGZF readers share (bgzf.hip: index and whole members; bgzf_ranges.hip: byte ranges): the member
// header as include/mi_codec.h reads it, and the check of one member of an untrusted table against the stream that turns it
// into an InfSeg descriptor for k_inflate<.., DESC> (inflate.hip).
#pragma once
#include "lz_common.h"
#include "internal.h"

#define BGZF_MIN       28u                     // the shortest member an index accepts: 12 + XLEN (>= 6) + 2 + 8

__device__ __forceinline__ uint32_t bgzf_le16(const uint8_t *s, uint64_t i) { return (uint32_t)s[i] | ((uint32_t)s[i + 1] << 8); }
__device__ __forceinline__ uint32_t bgzf_le32(const uint8_t *s, uint64_t i) { return bgzf_le16(s, i) | (bgzf_le16(s, i + 2) << 16); }

// The member that starts at `pos` and must lie inside [pos, end), end <= the stream's length: nothing outside that range is
// read.  RFC 1952 header with CM = 8 and FLG = FEXTRA alone; the subfields of the XLEN bytes in turn, the first 'B' 'C' of
// length 2 that lies inside them gives BSIZE (a subfield that runs past XLEN ends the search); the member's BSIZE + 1 bytes
// hold at least the header, an empty DEFLATE stream and the trailer; ISIZE, its last four bytes, is at most 65 536.
static __device__ bool bgzf_parse(const uint8_t *__restrict__ s, uint64_t pos, uint64_t end, uint32_t &msize, uint32_t &isize, uint32_t &xlen)
{
    if (end < pos || end - pos < BGZF_MIN) return false;
    if (s[pos] != 0x1Fu || s[pos + 1] != 0x8Bu || s[pos + 2] != 8u || s[pos + 3] != 4u) return false;
    xlen = bgzf_le16(s, pos + 10);
    if (12ull + xlen + 2u + 8u > end - pos) return false;
    bool found = false;
    uint32_t bsize = 0;
    for (uint32_t q = 0; q + 4u <= xlen && !found;) {                  // every round moves on by at least 4 of <= 65 535 bytes
        const uint64_t f = pos + 12u + q;
        const uint32_t slen = bgzf_le16(s, f + 2);
        if (s[f] == 0x42u && s[f + 1] == 0x43u && slen == 2u && q + 6u <= xlen) { bsize = bgzf_le16(s, f + 4); found = true; }
        q += 4u + slen;
    }
    if (!found) return false;
    msize = bsize + 1u;
    if (msize < xlen + 12u + 2u + 8u || msize > end - pos) return false;
    isize = bgzf_le32(s, pos + msize - 4u);
    return isize <= 65536u;
}

// One member of the (untrusted) table — the pairs (s0, o0) and (s1, o1) around it — against the stream of nbytes bytes: the
// pairs do not decrease, lie inside the stream and are at most 65 536 apart both ways; the header read again says the same
// (BSIZE + 1 = s1 - s0, ISIZE = o1 - o0).  True: d holds the member's DEFLATE bits, its length and its trailer's CRC-32
// (d.out_off is the caller's).  Nothing outside [s0, s1) is read.
static __device__ bool bgzf_member_seg(const uint8_t *__restrict__ s, uint64_t nbytes, uint64_t s0, uint64_t o0, uint64_t s1, uint64_t o1,
                                       InfSeg &d)
{
    if (!(s0 <= s1 && s1 <= nbytes && s1 - s0 <= 65536u && o1 >= o0 && o1 - o0 <= 65536u)) return false;
    uint32_t msize = 0, isize = 0, xlen = 0;
    if (!(bgzf_parse(s, s0, s1, msize, isize, xlen) && msize == s1 - s0 && isize == o1 - o0)) return false;
    d.first_bit = 8u * (s0 + 12u + xlen); d.last_bit = 8u * (s1 - 8u);
    d.out_len = isize; d.crc = bgzf_le32(s, s1 - 8u);
    return true;
}
