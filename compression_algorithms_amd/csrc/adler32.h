// adler32.h — the Adler-32 sums of a contiguous byte range by one workgroup of ZCK_THREADS threads: what k_adler32 (defz.hip,
// the whole-buffer checksum of the zlib container) and the per-item checksums of the batched inflate (inflate_batch.hip)
// share, as crc32.h is for the CRC-32.
//
// Raw sums a = sum b_i, s = sum (|A| - i) b_i:   a(AB) = a(A) + a(B),  s(AB) = s(A) + |B| a(A) + s(B)
// The standard value follows at the end: Adler-32 = (s + n) mod 65521 << 16 | (1 + a) mod 65521 (adler_standard).
#pragma once
#include "crc32.h"                  // ZCK_SEG / ZCK_THREADS / ZCK_PIECE, zck_segment

#define ADLER_MOD      65521u

// LDS of one workgroup's sums: the per-wave partials
struct AdlerLds { uint64_t red[2][ZCK_THREADS / 64]; };

// Every thread of the workgroup calls it with the same arguments: thread 0 gets the raw sums of in[lo, hi), mod 65521.
// v16: `in` is 16-byte aligned (pieces start at multiples of ZCK_PIECE from it).
__device__ __forceinline__ void adler_range(const uint8_t *__restrict__ in, uint64_t lo, uint64_t hi, bool v16, AdlerLds &sh,
                                            uint32_t tid, uint32_t &ra, uint32_t &rs)
{
    ra = 0; rs = 0;                                                    // (thread 0) raw sums of [lo, base), mod 65521
    for (uint64_t base = lo; base < hi; base += ZCK_PIECE) {
        const uint64_t pend = base + ZCK_PIECE < hi ? base + ZCK_PIECE : hi;
        const uint64_t s0 = base + (uint64_t)tid * ZCK_SEG;
        const uint32_t len = s0 >= pend ? 0u : (uint32_t)((pend - s0) < ZCK_SEG ? (pend - s0) : ZCK_SEG);
        uint32_t a = 0, s = 0;                                         // s = sum of the running a: <= 64 * 65 / 2 * 255
        zck_segment(in + s0, len, v16, [&](uint32_t b) { a += b; s += a; });
        // to the end of the piece: s += a * (bytes after the segment)
        uint64_t A = a, S = (uint64_t)s + (len ? (uint64_t)a * (pend - s0 - len) : 0ull);
        for (int o = 32; o > 0; o >>= 1) { A += __shfl_xor(A, o); S += __shfl_xor(S, o); }
        if ((tid & 63u) == 0) { sh.red[0][tid >> 6] = A; sh.red[1][tid >> 6] = S; }
        __syncthreads();
        if (tid == 0) {
            uint64_t pa = 0, ps = 0;
            for (uint32_t w = 0; w < ZCK_THREADS / 64; ++w) { pa += sh.red[0][w]; ps += sh.red[1][w]; }
            rs = (uint32_t)(((uint64_t)rs + (uint64_t)ra * ((pend - base) % ADLER_MOD) + ps % ADLER_MOD) % ADLER_MOD);
            ra = (uint32_t)(((uint64_t)ra + pa) % ADLER_MOD);
        }
        __syncthreads();
    }
}

// the standard Adler-32 of n bytes from their raw sums
__device__ __forceinline__ uint32_t adler_standard(uint32_t ra, uint32_t rs, uint64_t n)
{
    const uint32_t s1 = (uint32_t)((1ull + ra) % ADLER_MOD), s2 = (uint32_t)(((uint64_t)rs + n % ADLER_MOD) % ADLER_MOD);
    return (s2 << 16) | s1;
}
