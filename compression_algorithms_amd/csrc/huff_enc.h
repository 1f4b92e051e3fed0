// huff_enc.h — what the two entropy encoders share (defh.hip: mode H, defz.hip: mode Z; they differ in constants and bit order):
//   HuffHeap / huff_merge / huff_depth   the reference's heap merge (algorithms/huffman/huffman.c:100-163,189-211) on one lane and
//                                        a symbol's code length as its leaf's depth.  Its tie-breaking DEFINES the codes of both
//                                        modes (restated by oracle/orc_defh.c and oracle/orc_defz.c): one copy
//   huff_canonical                       canonical codes by (length, symbol): per-length counts, first code per length, rank
//   BitPacker                            the cooperative pack round of k_defh_encode / k_defz_encode, MSB or LSB first
// The callers keep mode Z's padding and length limiter, mode H's one-leaf rule, how a code is stored, how a token record becomes
// pieces, and everything around a record's tokens.  k_huff_build (huffman.hip) keeps its own loop: 64-bit cells, a stored tree.
#pragma once
#include "lz_common.h"
#include "heap_cells.h"

// The reference's array heap (strict '<' on the frequency in both sifts, leaves enqueued in symbol order, first pop = left).  A
// cell holds frequency << 10 | node id (frequencies <= 65 538 tokens, ids < 2 * 288): a comparison is ONE LDS read per node, not
// two dependent ones, and a merged node's frequency comes out of the two cells it pops.  Only the frequency field is compared:
// ties are decided by position alone.  NSYM: the alphabet's size (286 / 288, neither kernel pays LDS for the other's).
template <int NSYM>
struct HuffHeap {
    int16_t  parent[2 * NSYM];
    uint32_t heap[NSYM + 2];             // frequency << 10 | node id
    int16_t  leaf_of[NSYM];              // the caller presets -1: a symbol that is not used has no leaf
    int      nnodes, root;               // leaves + merged nodes; root = -1 when there are fewer than two leaves
};
typedef HeapCells<uint32_t, 10> HuffCells32;
#define HUFF_F(c)  ((c) >> 10)
#define HUFF_ID(c) ((int)((c) & 1023u))

// ONE lane: freq[0, nsym) -> parent / leaf_of / nnodes / root.  This loop is the critical path of the entropy stage (<= 287
// merges behind one lane); its sifts read ahead of their decisions (heap_cells.h), the enqueue loop reads the tally eight
// symbols ahead, and the heap and node counts live in registers (the note on aliasing in heap_cells.h).
template <int NSYM>
__device__ __forceinline__ void huff_merge(const uint32_t *freq, const int nsym, HuffHeap<NSYM> &h)
{
    int nheap = 0, nnodes = 0, root = -1;
    for (int s0 = 0; s0 < nsym; s0 += 8) {
        uint32_t f8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) f8[k] = freq[s0 + k < nsym ? s0 + k : 0];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k;
            const uint32_t f = f8[k];
            if (s >= nsym || !f) continue;
            const int id = nnodes++;
            h.parent[id] = -1; h.leaf_of[s] = (int16_t)id;
            HuffCells32::push(h.heap, nheap, (f << 10) | (uint32_t)id);
        }
    }
    if (nnodes > 1) {
        while (nheap > 1) {
            const uint32_t lc = HuffCells32::pop(h.heap, nheap), rc = HuffCells32::pop(h.heap, nheap);
            const int id = nnodes++;
            h.parent[id] = -1;
            h.parent[HUFF_ID(lc)] = (int16_t)id; h.parent[HUFF_ID(rc)] = (int16_t)id;
            HuffCells32::push(h.heap, nheap, ((HUFF_F(lc) + HUFF_F(rc)) << 10) | (uint32_t)id);
        }
        root = HUFF_ID(HuffCells32::pop(h.heap, nheap));
    }
    h.nnodes = nnodes; h.root = root;
}

// code length of symbol s in a tree of at least two leaves: its leaf's depth; 0 for a symbol that is not used
template <int NSYM>
__device__ __forceinline__ uint32_t huff_depth(const HuffHeap<NSYM> &h, int s)
{
    const int leaf = h.leaf_of[s];
    if (leaf < 0) return 0;
    uint32_t len = 0;
    for (int node = leaf; node != h.root; node = h.parent[node]) ++len;
    return len;
}

// Canonical codes by all blockDim.x threads: store(symbol, length, code), code = first code of the length + rank among the symbols
// of that length (symbol order), 0 where the length is 0 or above MAXLEN.  NBINS = MAXLEN + 2: longer lengths are counted in bin
// MAXLEN + 1; NBINS = MAXLEN + 1: the caller vouches there are none.  s_count[l] and s_next[l] (first code) stay valid.
template <int MAXLEN, int NBINS, typename Store>
__device__ __forceinline__ void huff_canonical(const uint8_t *len, const int nsym, uint32_t *s_count /*[NBINS]*/, uint32_t *s_next /*[NBINS]*/,
                                               Store &&store)
{
    static_assert(NBINS == MAXLEN + 1 || NBINS == MAXLEN + 2, "bins 0..MAXLEN, and maybe one for what is longer");
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < NBINS; i += nt) s_count[i] = 0;
    __syncthreads();
    for (int s = tid; s < nsym; s += nt) if (len[s]) atomicAdd(&s_count[len[s] > NBINS - 1 ? NBINS - 1 : len[s]], 1u);
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
        s_next[0] = 0;
        for (int l = 1; l <= MAXLEN; ++l) { c = (c + s_count[l - 1]) << 1; s_next[l] = c; }
        if (NBINS > MAXLEN + 1) s_next[MAXLEN + 1] = 0;
    }
    __syncthreads();
    for (int s = tid; s < nsym; s += nt) {
        const uint32_t l = len[s];
        uint32_t rank = 0;
        for (int k = 0; k < s; ++k) rank += (len[k] == l);
        store(s, l, (l && l <= (uint32_t)MAXLEN) ? s_next[l] + rank : 0u);
    }
    __syncthreads();
}

// The pack stage of one block's tokens by THREADS threads: a thread owns 4 consecutive tokens per round, each at most two pieces
// of <= 32 bits and MAXBITS bits together.  A round scans the threads' bit counts, zeroes a stage in LDS with the bits left over
// from the round before in front, ORs the pieces in and stores the complete words.  The packer owns the bit position (qbase),
// the incomplete last word (carry) and the read-ahead of the records; its two LDS arrays are the caller's (one struct of both
// padded either kernel by 8 bytes).  The caller makes pieces of a record and writes what surrounds the tokens.  LIMITED: words
// at or past `limit` are not stored (mode H, the caller's buffer); else no compare per word (mode Z, the block's own slot).
template <int THREADS, uint32_t MAXBITS, bool MSB, bool LIMITED>
struct BitPacker {
    static constexpr uint32_t STAGE_WORDS = THREADS * 4 * MAXBITS / 32 + 8, SCAN_WORDS = THREADS / 64 + 2;
    uint32_t *const stage, *const scan;  // LDS of the caller: [STAGE_WORDS], [SCAN_WORDS]
    uint64_t qbase;
    uint32_t carry;
    uint4    ahead;                      // the next round's records, in flight while this round is packed (three barriers, one HBM round trip)

    __device__ __forceinline__ BitPacker(uint32_t *s_stage, uint32_t *s_scan, uint64_t first_bit, uint32_t first_carry, const uint32_t *trec, uint32_t ntok)
        : stage(s_stage), scan(s_scan), qbase(first_bit), carry(first_carry), ahead(make_uint4(0, 0, 0, 0))
    {
        if (threadIdx.x * 4u < ntok) ahead = *reinterpret_cast<const uint4 *>(trec + threadIdx.x * 4u);
    }

    // records t .. t + 3 of this thread (t = round's first token + 4 * threadIdx.x; the token array is 65536 words: in bounds)
    __device__ __forceinline__ uint4 records(const uint32_t *trec, uint32_t t, uint32_t ntok)
    {
        const uint4 rv = ahead;
        if (t + THREADS * 4u < ntok) ahead = *reinterpret_cast<const uint4 *>(trec + t + THREADS * 4u);
        return rv;
    }

    // k <= 32 bits of v at stage bit `rel`
    __device__ __forceinline__ void put(uint32_t &rel, uint32_t v, uint32_t k)
    {
        if (!k) return;
        const uint32_t wi = rel >> 5, sh = rel & 31u;
        if constexpr (MSB) {
            const uint64_t x = (uint64_t)v << (64u - k - sh);
            atomicOr(&stage[wi], (uint32_t)(x >> 32));
            if ((uint32_t)x) atomicOr(&stage[wi + 1], (uint32_t)x);
        } else {
            atomicOr(&stage[wi], v << sh);
            if (sh + k > 32u) atomicOr(&stage[wi + 1], v >> (32u - sh));
        }
        rel += k;
    }

    // one round: this thread's pieces (v[i], k[i] bits) in order, `mine` = the sum of its k[i]; complete words go to dst[their index]
    __device__ __forceinline__ void round(const uint32_t (&v)[8], const uint32_t (&k)[8], uint32_t mine, uint32_t *dst, uint64_t limit = 0)
    {
        const uint32_t tid = threadIdx.x;
        uint32_t total;
        uint32_t rel = block_exclusive_scan<uint32_t>(mine, OpAddU32(), 0u, scan, &total);
        const uint64_t w0 = qbase >> 5;
        const uint32_t sh0 = (uint32_t)(qbase & 31u);
        const uint32_t nwords = (sh0 + total + 31u) >> 5;
        for (uint32_t i = tid; i < nwords + 1; i += THREADS) stage[i] = (i == 0) ? carry : 0u;
        __syncthreads();
        rel += sh0;
#pragma unroll
        for (int i = 0; i < 8; ++i) put(rel, v[i], k[i]);
        __syncthreads();
        const uint32_t ncomplete = (sh0 + total) >> 5;
        for (uint32_t i = tid; i < ncomplete; i += THREADS) if (!LIMITED || w0 + i < limit) dst[w0 + i] = stage[i];
        carry = stage[ncomplete];
        qbase += total;
        __syncthreads();
    }
};
