// defh_size.h — the size of a mode-H record, known before a bit of it is packed.
//
// A token costs its symbol's code plus, for a match, the offset bits below the leading one and the 5-bit length
// (defh.hip: symbol 256 + clz16(d), nx = 15 - clz16(d) offset bits).  Both depend on the symbol alone, so the payload is a
// sum over the block's 286-bin tally:
//     payload = sum over s of hist[s] * (len[s] + extra(s)),   n_tokens = sum over s of hist[s]
// and the record is the 292-byte header plus the payload in whole u32 words.  k_defh_lengths computes this beside the code
// lengths; the scan over the batch's sizes then places every record, and k_defh_encode packs it where it belongs.
// Shared by device and host (tests/defh_size_harness.cpp pins it against the oracle's records).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DEFH_HD __host__ __device__ __forceinline__
#else
#define DEFH_HD inline
#endif

#define DEFH_NSYM     286
#define DEFH_HDR      292u          // bytes before the packed words

// bits that follow a symbol's code: none for a literal, (15 - clz16(d)) offset bits + 5 length bits for a match
DEFH_HD uint32_t defh_extra_bits(uint32_t s) { return (s >= 256u && s <= 271u) ? (15u - (s - 256u)) + 5u : 0u; }

// record size in bytes for a payload of `payload_bits` (<= 65 536 tokens of <= 44 bits: fits 32 bits)
DEFH_HD uint32_t defh_record_bytes(uint32_t payload_bits) { return DEFH_HDR + 4u * ((payload_bits + 31u) >> 5); }

// Payload bits and token count of the symbols first, first + stride, ... < 286: a host caller passes (0, 1), a wave's lane
// (lane, 64) and adds the lanes' results.
DEFH_HD uint32_t defh_payload_bits(const uint32_t *hist, const uint8_t *len, uint32_t first, uint32_t stride, uint32_t *n_tokens)
{
    uint32_t bits = 0, ntok = 0;
    for (uint32_t s = first; s < DEFH_NSYM; s += stride) {
        const uint32_t f = hist[s];
        bits += f * ((uint32_t)len[s] + defh_extra_bits(s));
        ntok += f;
    }
    *n_tokens = ntok;
    return bits;
}
