// crc32.h — the CRC-32 of a contiguous byte range by one workgroup of ZCK_THREADS threads: what k_crc32 (defz.hip, the
// whole-buffer checksum of the gzip container) and the per-member checksums of BGZF (bgzf.hip) share.
//
// A workgroup walks its range in pieces of ZCK_PIECE bytes; thread t takes a ZCK_SEG-byte segment of each piece.  The CRC
// is linear in the data, so a segment's part moves to the end of the range by a factor that depends only on the number of
// bytes after it:
//   CRC-32 (pure: zero register, no final xor)  crc(A B) = crc(A) * x^(8 |B|) mod P  xor  crc(B)  (GF(2), reflected)
// The standard value follows at the end: CRC-32 = crc ^ (0xFFFFFFFF * x^(8n) mod P) ^ 0xFFFFFFFF (crc_standard).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZCK_SEG        64u                     // checksum bytes per thread and round
#define ZCK_THREADS    256u
#define ZCK_PIECE      (ZCK_SEG * ZCK_THREADS) // bytes per workgroup and round
#define CRC_POLY       0xEDB88320u             // reflected

__device__ inline uint32_t crc_mulmod(uint32_t a, uint32_t b)     // a * b mod P, reflected (bit 31 = x^0)
{
    uint32_t p = 0;
#pragma unroll 8
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}
__device__ inline uint32_t crc_xpow8(uint64_t len)                  // x^(8 len) mod P
{
    uint32_t p = 1u << 31, sq = 1u << 23;                            // 1, x^8
    while (len) {
        if (len & 1u) p = crc_mulmod(sq, p);
        len >>= 1;
        if (len) sq = crc_mulmod(sq, sq);
    }
    return p;
}
// the standard CRC-32 of n bytes from their pure CRC
__device__ inline uint32_t crc_standard(uint32_t pure, uint64_t n) { return pure ^ crc_mulmod(0xFFFFFFFFu, crc_xpow8(n)) ^ 0xFFFFFFFFu; }

// the 64 bytes of one segment (fewer at the end of the input) into a per-byte callback, 16-byte loads where aligned
template <typename F>
__device__ __forceinline__ void zck_segment(const uint8_t *p, uint32_t len, bool v16, F &&fn)
{
    if (v16 && len == ZCK_SEG) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = reinterpret_cast<const uint4 *>(p)[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int j = 0; j < 16; ++j) fn((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        }
    } else {
        for (uint32_t j = 0; j < len; ++j) fn((uint32_t)p[j]);
    }
}

// LDS of one workgroup's CRC: the byte table and the per-wave partials
struct CrcLds {
    uint32_t tab[256];
    uint32_t red[ZCK_THREADS / 64];
};

// Every thread of the workgroup (ZCK_THREADS of them) calls these two with the same arguments.  crc_lds_init fills the
// byte table (the caller's __syncthreads() follows); crc_range returns, in thread 0, the pure CRC of p[0, len).
__device__ __forceinline__ void crc_lds_init(CrcLds &s, uint32_t tid)
{
    uint32_t c = tid;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
    s.tab[tid] = c;
}
__device__ inline uint32_t crc_range(const uint8_t *__restrict__ p, uint64_t len, CrcLds &s, uint32_t tid)
{
    const uint32_t kfull = crc_xpow8((uint64_t)ZCK_SEG * (ZCK_THREADS - 1u - tid));      // segment -> end of a full piece
    const uint32_t xpiece = crc_xpow8(ZCK_PIECE);
    const bool v16 = (((uintptr_t)p) & 15u) == 0;
    uint32_t run = 0;                                                  // (thread 0) crc of [0, base)
    for (uint64_t base = 0; base < len; base += ZCK_PIECE) {
        const uint64_t pend = base + ZCK_PIECE < len ? base + ZCK_PIECE : len;
        const uint64_t s0 = base + (uint64_t)tid * ZCK_SEG;
        const uint32_t n = s0 >= pend ? 0u : (uint32_t)((pend - s0) < ZCK_SEG ? (pend - s0) : ZCK_SEG);
        uint32_t c = 0;
        zck_segment(p + s0, n, v16, [&](uint32_t b) { c = s.tab[(c ^ b) & 0xFFu] ^ (c >> 8); });
        const bool full = pend - base == ZCK_PIECE;
        if (n) c = crc_mulmod(c, full ? kfull : crc_xpow8(pend - s0 - n));
        else c = 0;
        for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o);
        if ((tid & 63u) == 0) s.red[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) {
            uint32_t pc = 0;
            for (uint32_t w = 0; w < ZCK_THREADS / 64; ++w) pc ^= s.red[w];
            run = crc_mulmod(run, full ? xpiece : crc_xpow8(pend - base)) ^ pc;
        }
        __syncthreads();
    }
    return run;
}
