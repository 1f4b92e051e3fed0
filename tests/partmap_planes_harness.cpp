// partmap_planes_harness.cpp — csrc/partmap_planes.h on the host, against the naive bit loops (tests/test_partmap_planes.py).
// Plain C++: no HIP, no library.  Prints "ok <cases>" and exits 0, or the first mismatch and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../compression_algorithms_amd/csrc/partmap_planes.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()                                           // splitmix64
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// (a) against the definition: bit j of plane b = bit b of the code of position j
static int check_planes(const uint8_t code[64], const char *what, uint32_t a, uint32_t b)
{
    uint32_t w[16], lo[PMP_PLANES], hi[PMP_PLANES];
    for (uint32_t i = 0; i < 16; ++i)
        w[i] = (uint32_t)code[4 * i] | ((uint32_t)code[4 * i + 1] << 8) | ((uint32_t)code[4 * i + 2] << 16) | ((uint32_t)code[4 * i + 3] << 24);
    pmp_planes_of_bytes(w, lo, hi);
    for (uint32_t p = 0; p < PMP_PLANES; ++p) {
        uint32_t wl = 0, wh = 0;
        for (uint32_t j = 0; j < 32; ++j) {
            wl |= (uint32_t)((code[j] >> p) & 1u) << j;
            wh |= (uint32_t)((code[32 + j] >> p) & 1u) << j;
        }
        if (wl != lo[p] || wh != hi[p]) {
            printf("planes: %s (%u, %u): plane %u is %08x %08x, want %08x %08x\n", what, a, b, p, lo[p], hi[p], wl, wh);
            return 0;
        }
    }
    return 1;
}

// (b) against the definition: bit j of bm[k] is set iff the seven plane bits at (k, j) spell `part`
static int check_match(const uint32_t pl[PMP_PLANES][4], uint32_t part, const char *what)
{
    uint32_t bm[4];
    pmp_match_bits(pl, part, bm);
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t j = 0; j < 32; ++j) {
            uint32_t code = 0;
            for (uint32_t b = 0; b < PMP_PLANES; ++b) code |= ((pl[b][k] >> j) & 1u) << b;
            if (((bm[k] >> j) & 1u) != (uint32_t)(code == part)) {
                printf("match: %s part %u dword %u bit %u: code %u, match bit %u\n", what, part, k, j, code, (bm[k] >> j) & 1u);
                return 0;
            }
        }
    return 1;
}

int main()
{
    unsigned long cases = 0;
    uint8_t code[64];
    // every code at every position, among zeros and among the code of "no position"
    for (uint32_t bg = 0; bg < 2; ++bg)
        for (uint32_t c = 0; c < 128; ++c)
            for (uint32_t p = 0; p < 64; ++p) {
                memset(code, bg ? (int)PMP_NONE : 0, sizeof code);
                code[p] = (uint8_t)c;
                if (!check_planes(code, "one code", c, p)) return 1;
                ++cases;
            }
    for (uint32_t r = 0; r < 10000; ++r) {
        for (uint32_t p = 0; p < 64; ++p) code[p] = (uint8_t)(rnd() & 127u);
        if (!check_planes(code, "random", r, 0)) return 1;
        ++cases;
    }
    // every part number against random planes, planes of one code everywhere (its own, its neighbours', 127), and planes that
    // the first function made of bytes
    uint32_t pl[PMP_PLANES][4];
    for (uint32_t part = 0; part < PMP_NONE; ++part) {
        for (uint32_t r = 0; r < 64; ++r) {
            for (uint32_t b = 0; b < PMP_PLANES; ++b)
                for (uint32_t k = 0; k < 4; ++k) pl[b][k] = rnd() | (rnd() << 16);
            // a few positions of code 127 and of the part itself among the random ones
            for (uint32_t b = 0; b < PMP_PLANES; ++b) {
                pl[b][r & 3u] |= 0x00010001u << (r & 15u);
                const uint32_t bit = 1u << ((r * 7u) & 31u);
                pl[b][(r >> 2) & 3u] = (pl[b][(r >> 2) & 3u] & ~bit) | (((part >> b) & 1u) ? bit : 0u);
            }
            if (!check_match(pl, part, "random")) return 1;
            ++cases;
        }
        const uint32_t others[4] = {part, (part + 1u) % PMP_NONE, part ^ 64u, PMP_NONE};
        for (uint32_t o = 0; o < 4; ++o) {
            for (uint32_t b = 0; b < PMP_PLANES; ++b)
                for (uint32_t k = 0; k < 4; ++k) pl[b][k] = ((others[o] >> b) & 1u) ? ~0u : 0u;
            if (!check_match(pl, part, "one code everywhere")) return 1;
            uint32_t bm[4];
            pmp_match_bits(pl, part, bm);
            const uint32_t want = (others[o] == part) ? ~0u : 0u;
            if (bm[0] != want || bm[1] != want || bm[2] != want || bm[3] != want) { printf("match: code %u everywhere, part %u\n", others[o], part); return 1; }
            ++cases;
        }
        // 128 positions through (a), then (b): positions p with code[p] == part, and only those
        uint8_t c128[128];
        for (uint32_t p = 0; p < 128; ++p) { const uint32_t x = rnd() & 7u; c128[p] = (uint8_t)(x == 0 ? part : x == 1 ? PMP_NONE : rnd() & 127u); }
        for (uint32_t h = 0; h < 2; ++h) {
            uint32_t w[16], lo[PMP_PLANES], hi[PMP_PLANES];
            for (uint32_t i = 0; i < 16; ++i) memcpy(&w[i], c128 + 64 * h + 4 * i, 4);     // (little-endian hosts, as the GPU)
            pmp_planes_of_bytes(w, lo, hi);
            for (uint32_t b = 0; b < PMP_PLANES; ++b) { pl[b][2 * h] = lo[b]; pl[b][2 * h + 1] = hi[b]; }
        }
        uint32_t bm[4];
        pmp_match_bits(pl, part, bm);
        for (uint32_t p = 0; p < 128; ++p)
            if (((bm[p >> 5] >> (p & 31u)) & 1u) != (uint32_t)(c128[p] == part)) { printf("both: part %u position %u\n", part, p); return 1; }
        ++cases;
    }
    printf("ok %lu\n", cases);
    return 0;
}
