// partmap_planes.h — the part map of the LDS-resident match finder as seven bit planes.
//
// k_lz2_partition tabulates the part (0..126) of every position of a block; every workgroup of stage 2 (lz2_find.hip) then picks
// its own part's positions out of that map.  As one byte per position the pick was a SWAR byte compare, ~11 VALU per dword of
// four positions, repeated by each of a block's ~33 workgroups.  As bit planes it is a few logic ops per 32 positions:
//
//     plane b (b = 0..6) of a block: 65 536 bits = 8 KiB; bit p of plane b = bit b of the part of position p,
//     little-endian inside a dword (dword p >> 5, bit p & 31); the planes follow each other, 56 KiB per block.
//     A position at or past the block's end carries the code 127 — all seven bits set — which is no part's number.
//
// The two pure functions of the layout live here, for device and host (tests/partmap_planes_harness.cpp checks them against the
// naive bit loops); the kernels call these and nothing else implements the layout.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PMP_HD __host__ __device__ __forceinline__
#define PMP_UNROLL _Pragma("unroll")                // (the arrays are registers on the device)
#else
#define PMP_HD inline
#define PMP_UNROLL
#endif

#define PMP_PLANES       7u
#define PMP_NONE         127u                       // the code of "no position": every plane's bit set
#define PMP_PLANE_BYTES  8192u                      // 65 536 positions, one bit each
#define PMP_BLOCK_BYTES  (PMP_PLANES * PMP_PLANE_BYTES)

// (a) 64 consecutive positions, one code byte each (w[i] holds positions 4 i .. 4 i + 3, lowest byte first; codes < 128)
//     -> their 64 bits of every plane: bit j of lo[b] is bit b of the code of position j, bit j of hi[b] that of position 32 + j.
// Eight positions at a time are an 8 x 8 bit matrix (row = position, column = bit of the code); its transpose (three
// delta swaps) has plane b's eight bits in byte b, and the bytes of eight such groups make the plane's two dwords.
PMP_HD void pmp_planes_of_bytes(const uint32_t w[16], uint32_t lo[PMP_PLANES], uint32_t hi[PMP_PLANES])
{
    uint32_t tl[8], th[8];                          // the transposed groups: planes 0..3 in tl, 4..7 in th
    PMP_UNROLL
    for (uint32_t g = 0; g < 8u; ++g) {
        uint64_t x = (uint64_t)w[2u * g] | ((uint64_t)w[2u * g + 1u] << 32);
        uint64_t t;
        t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;  x ^= t ^ (t << 7);
        t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
        t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
        tl[g] = (uint32_t)x; th[g] = (uint32_t)(x >> 32);
    }
    PMP_UNROLL
    for (uint32_t b = 0; b < PMP_PLANES; ++b) {
        const uint32_t *t = b < 4u ? tl : th;
        const uint32_t sh = 8u * (b & 3u);
        lo[b] = ((t[0] >> sh) & 255u) | (((t[1] >> sh) & 255u) << 8) | (((t[2] >> sh) & 255u) << 16) | (((t[3] >> sh) & 255u) << 24);
        hi[b] = ((t[4] >> sh) & 255u) | (((t[5] >> sh) & 255u) << 8) | (((t[6] >> sh) & 255u) << 16) | (((t[7] >> sh) & 255u) << 24);
    }
}

// (b) one thread's match bits: pl[b][k] is dword k (of the thread's four consecutive ones) of plane b; bit j of bm[k] is set
//     where all seven plane bits equal those of `part` — AND over b of (plane XNOR mask_b), mask_b all ones if bit b of part is
//     set.  part <= 126, so the code 127 matches nothing.
PMP_HD void pmp_match_bits(const uint32_t pl[PMP_PLANES][4], uint32_t part, uint32_t bm[4])
{
    PMP_UNROLL
    for (uint32_t k = 0; k < 4u; ++k) {
        uint32_t m = ~0u;
        PMP_UNROLL
        for (uint32_t b = 0; b < PMP_PLANES; ++b) m &= ~(pl[b][k] ^ (0u - ((part >> b) & 1u)));
        bm[k] = m;
    }
}
