// defh.hip — "mode H": the entropy stage the reference's deflate leaves as a TODO
// (algorithms/deflate/lz77.c:279 "// TODO: Build huffman tree and encode compressed buffer").
//
// Taken from the reference: the token sequence (algorithms/deflate/lz77.c:199-280, produced by the
// same finder / parse kernels as the byte-token stream), the 286-symbol alphabet
// (deflate/huffman.h:6 NUM_CODES; huffman.c:49-62: literal b -> b, match with offset d ->
// 256 + clz16(d)), the per-block tally (lz77.c:206,231,273), MSB-first u32 packing
// (deflate/huffman.c:16-46) and the heap merge procedure with its tie-breaking
// (algorithms/huffman/huffman.c:100-163,189-211; huff_enc.h holds it, with the canonical-code core and the pack round, for this
// file and defz.hip).  Defined by this project (the bit
// stream is PARITY UNPINNED — the reference has no such encoder; the oracle restatement is
// oracle/orc_defh.c): lengths from that heap, canonical codes by (length, symbol), a match symbol is
// followed by the offset bits below its leading one and the 5-bit length.
//
// Block record, 4-byte aligned:   u32 n_tokens | u8 len[286] + 2 pad | u32 words[] (MSB-first)
//
//   k_defh_lengths  one wave per block: code lengths and canonical codes from the tally k_lz_parse_emit left, and the
//                   record's SIZE (defh_size.h: it follows from the tally and the lengths alone)
//   (k_lz_scan_blocks, lz_emit.hip: sizes -> offsets)
//   k_defh_encode   one workgroup per block over the token records k_lz_parse_emit left: packs the record straight into
//                   its place in the caller's stream — records are whole dwords, so a record's dwords are its own
//   k_defh_decode   one wave per block: record -> tokens -> bytes (LZ copy in LDS), no token stream in HBM
#include "lz_common.h"
#include "lz_decode.h"
#include "huff_enc.h"               // the heap merge, canonical codes and the pack round, shared with defz.hip
#include "internal.h"
#include "defh_size.h"              // DEFH_NSYM, DEFH_HDR, the record's size from tally and lengths
#include <stdlib.h>

// 256 threads per block: the kernel spends its time behind ONE lane (the heap), so what counts is how many blocks a CU holds —
// wave slots, not LDS, are the limit (32 per CU: 8 blocks of 4 waves instead of 4 of 8).  Same box: 512 / 256 / 128 threads
// 17.30 / 17.72 / 17.68 GB/s for the whole mode-H step.
#ifndef DEFH_THREADS
#define DEFH_THREADS  256
#endif
#define DEFH_MAXBITS  44u           // code <= 24 (65536 tokens: Fibonacci bound) + 15 offset bits + 5 length bits
// direct LUT of the decoder: 9 bits = 1 KiB of LDS (more waves per CU beat fewer slow-path symbols: 11 / 10 / 9 / 8 / 7 bits
// decode 17.8 / 19.2 / 19.5 / 18.6 / 18.6 GB/s); decode-side only, the format does not depend on it
#ifndef DEFH_LUT_BITS
#define DEFH_LUT_BITS 9
#endif

__device__ __forceinline__ uint32_t clz16(uint32_t d) { return (uint32_t)__builtin_clz(d & 0xFFFFu) - 16u; }   // d in 1..65535

// canonical codes, MSB first: lengths 1..32 get one, anything longer is counted in bin 33 and gets code 0
__device__ __forceinline__ void defh_canonical(const uint8_t *s_len, uint32_t *s_code, uint32_t *s_count /*[34]*/, uint32_t *s_next /*[34]*/)
{
    huff_canonical<32, 34>(s_len, DEFH_NSYM, s_count, s_next, [&](int s, uint32_t, uint32_t code) { s_code[s] = code; });
}

// Two kernels since round 3.  The code LENGTHS wait ~1.4 M cycles per block behind one lane (the reference heap): that kernel is
// ONE wave per block with 8 KiB of LDS — twenty blocks in flight per CU where the fused kernel (256 threads, the pack stage's
// 5.6 KiB window) held eight.  It leaves the lengths at the head of the block's slot (where the record's header would be), the
// canonical codes and the token count behind the tally, and the record's size in block_bits[lb]; the pack kernel reads the
// first three, the scan between the two kernels turns the sizes into the records' places.
#define DEFH_CODE_AT (LZ_DEFH_HIST_AT + 288u)          // slot words [.., +288): the canonical codes, from k_defh_lengths to k_defh_encode
#define DEFH_NTOK_AT (DEFH_CODE_AT + 288u)             // slot word: the block's token count (the tally's sum)
static_assert(DEFH_NTOK_AT + 1u <= LZ_SLOT_WORDS, "tally, codes and token count live at the end of the slot");

__global__ __launch_bounds__(64)
void k_defh_lengths(uint32_t *__restrict__ slots, uint64_t *__restrict__ block_bits)
{
    // 4.5 KiB of LDS (8 before): the tally's array becomes the codes' once the leaves are enqueued, the heap cells carry the
    // frequencies — the wave holds its LDS for the whole serial merge, and LDS-seconds are what the pipeline's stages compete for
    __shared__ HuffHeap<DEFH_NSYM> h;
    __shared__ uint32_t s_hist[DEFH_NSYM + 2];
    __shared__ __attribute__((aligned(16))) uint8_t s_len[DEFH_NSYM + 2];
    __shared__ uint32_t s_count[34], s_next[34];
    uint32_t *const s_code = s_hist;
    const int tid = threadIdx.x;
    uint32_t *out = slots + (size_t)blockIdx.x * LZ_SLOT_WORDS;
    // ---- tally (lz77.c:206,231,273): taken by k_lz_parse_emit while it wrote the token records, left at the end of the slot
    for (int i = tid; i < DEFH_NSYM + 2; i += 64) { s_hist[i] = out[LZ_DEFH_HIST_AT + i]; s_len[i] = 0; }
    for (int i = tid; i < DEFH_NSYM; i += 64) h.leaf_of[i] = -1;
    __syncthreads();
    // ---- code lengths: the reference heap, leaves enqueued in symbol order (one lane; <= 285 merges); one leaf: one bit
    if (tid == 0) huff_merge(s_hist, DEFH_NSYM, h);
    __syncthreads();
    for (int sy = tid; sy < DEFH_NSYM; sy += 64) s_len[sy] = (uint8_t)(h.nnodes == 1 ? (h.leaf_of[sy] >= 0 ? 1u : 0u) : huff_depth(h, sy));
    __syncthreads();
    // ---- the record's size, while the tally is still there (s_hist becomes s_code below): 286 multiply-adds over the wave
    {
        uint32_t ntok;
        uint32_t bits = defh_payload_bits(s_hist, s_len, (uint32_t)tid, 64u, &ntok);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { bits += __shfl_xor(bits, o); ntok += __shfl_xor(ntok, o); }
        if (tid == 0) {
            block_bits[blockIdx.x] = 8ull * defh_record_bytes(bits);      // replaces the token count k_lz_parse_emit left there
            out[DEFH_NTOK_AT] = ntok;
        }
    }
    defh_canonical(s_len, s_code, s_count, s_next);
    for (int i = tid; i < (DEFH_NSYM + 2) / 4; i += 64) out[1 + i] = reinterpret_cast<const uint32_t *>(s_len)[i];     // the header's lengths
    for (int i = tid; i < DEFH_NSYM + 2; i += 64) out[DEFH_CODE_AT + i] = s_code[i];
}

// The record goes straight to its final place: word (base + excl_local[lb]) / 32 of the caller's stream (base: the bits of the
// batches before this one; both multiples of 32).  Every store is held below cap_words — never past the caller's buffer (the
// host checked the capacity against the bound) — and nothing is written past the record's own last word.
__global__ __launch_bounds__(DEFH_THREADS)
void k_defh_encode(const uint32_t *__restrict__ trec_all, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ excl_local,
                   const uint64_t *__restrict__ base_bits, uint32_t *__restrict__ d_out, uint64_t cap_words)
{
    __shared__ uint32_t s_code[DEFH_NSYM + 2];
    __shared__ __attribute__((aligned(16))) uint8_t s_len[DEFH_NSYM + 2];
    typedef BitPacker<DEFH_THREADS, DEFH_MAXBITS, true, true> Packer;           // MSB first, stores held below wlim
    __shared__ uint32_t s_scan[Packer::SCAN_WORDS], s_stage[Packer::STAGE_WORDS];

    const int tid = threadIdx.x;
    const uint32_t lb = blockIdx.x;
    const uint32_t *trec = trec_all + (size_t)lb * LZ_MAX_BLOCK;
    const uint32_t *slot = slots + (size_t)lb * LZ_SLOT_WORDS;
    const uint32_t ntok = slot[DEFH_NTOK_AT];                         // k_defh_lengths: the tally's sum
    const uint64_t w_rec = (*base_bits + excl_local[lb]) >> 5;        // the record's first word in the stream
    uint32_t *out = d_out + w_rec;
    const uint64_t lim = cap_words > w_rec ? cap_words - w_rec : 0;   // record words [0, lim) are inside the buffer
    auto symbol_of = [](uint32_t r) -> uint32_t { return (r >> 31) ? 256u + clz16(r) : (r & 0xFFu); };

    // ---- lengths and codes: k_defh_lengths left them at the head of the slot and behind the tally
    for (int i = tid; i < DEFH_NSYM + 2; i += DEFH_THREADS) s_code[i] = slot[DEFH_CODE_AT + i];
    for (int i = tid; i < (DEFH_NSYM + 2) / 4; i += DEFH_THREADS) reinterpret_cast<uint32_t *>(s_len)[i] = slot[1 + i];
    __syncthreads();

    // ---- header: token count, the 286 lengths and two zero pad bytes
    if (tid == 0 && lim > 0) out[0] = ntok;
    for (uint32_t i = tid; i < (DEFH_NSYM + 2) / 4; i += DEFH_THREADS) if (1u + i < lim) out[1u + i] = reinterpret_cast<const uint32_t *>(s_len)[i];
    uint32_t *words = out + DEFH_HDR / 4;
    const uint64_t wlim = lim > DEFH_HDR / 4 ? lim - DEFH_HDR / 4 : 0;   // payload words [0, wlim) are inside the buffer

    // ---- pack, DEFH_THREADS * 4 tokens per round; a thread owns 4 consecutive tokens (huff_enc.h)
    Packer pk(s_stage, s_scan, 0, 0u, trec, ntok);
    for (uint32_t t0 = 0; t0 < ntok; t0 += DEFH_THREADS * 4) {
        const uint32_t t = t0 + (uint32_t)tid * 4;
        const uint4 rv = pk.records(trec, t, ntok);
        const uint32_t r[4] = {rv.x, rv.y, rv.z, rv.w};
        uint32_t v[8], nb[8], mine = 0;                                    // per token: the symbol's code, then offset and length bits
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nb[2 * k] = 0; nb[2 * k + 1] = 0; v[2 * k] = 0; v[2 * k + 1] = 0;
            if (t + k < ntok) {
                const uint32_t sym = symbol_of(r[k]);
                v[2 * k] = s_code[sym]; nb[2 * k] = s_len[sym];
                if (r[k] >> 31) {
                    const uint32_t d = r[k] & 0xFFFFu, nx = 15u - clz16(d);
                    v[2 * k + 1] = ((d - (1u << nx)) << 5) | ((r[k] >> 16) & 31u);
                    nb[2 * k + 1] = nx + 5u;
                }
                mine += nb[2 * k] + nb[2 * k + 1];
            }
        }
        pk.round(v, nb, mine, words, wlim);
    }
    if (tid == 0 && (pk.qbase & 31u) && (pk.qbase >> 5) < wlim) words[pk.qbase >> 5] = pk.carry;
}

// The entropy stage of one batch, on one stream: lengths (+ sizes into block_bits), the scan that turns block_bits into offsets
// in place and publishes the block table (lz_emit.hip), then the pack into the caller's stream at *base_bits + offset.
void defh_launch_encode(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, uint32_t nb, const uint64_t *base_bits,
                        uint64_t *excl_global, uint8_t *d_out, uint64_t cap_bytes, hipStream_t s)
{
    hipLaunchKernelGGL(k_defh_lengths, dim3(nb), dim3(64), 0, s, slots, block_bits);
    lz_launch_scan_blocks(block_bits, nb, base_bits, excl_global, s);
    hipLaunchKernelGGL(k_defh_encode, dim3(nb), dim3(DEFH_THREADS), 0, s, trec, slots, block_bits, base_bits,
                       reinterpret_cast<uint32_t *>(d_out), cap_bytes / 4);
}

// ---------------------------------------------------------------------------------------------
// decode: one wave per block.  Every lane reads the same bits (uniform control flow); the LZ copy of a
// match is spread over the lanes, the output block is staged in LDS like k_lz_decode.
// ---------------------------------------------------------------------------------------------
template <uint32_t RING>
__global__ __launch_bounds__(64)
void k_defh_decode(const uint8_t *__restrict__ stream, uint64_t stream_bytes, const uint64_t *__restrict__ block_bits, LzP P,
                   uint8_t *__restrict__ out, uint64_t n_total, uint32_t *__restrict__ err)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[RING];
    __shared__ uint16_t s_lut[1 << DEFH_LUT_BITS];                     // symbol | length << 9; 0xFFFF = longer than the table
    // lengths and codes are only needed while the tables are built: they lie in the (still unused) ring
    static_assert(RING >= 4u * (DEFH_NSYM + 2) + ((DEFH_NSYM + 2 + 3) & ~3u), "the ring holds the build-time tables");
    uint32_t *s_code = reinterpret_cast<uint32_t *>(s_ring);
    uint8_t  *s_len = s_ring + 4u * (DEFH_NSYM + 2);
    __shared__ uint32_t s_count[34], s_next[34];
    __shared__ uint16_t s_sorted[DEFH_NSYM];                           // symbols by (length, symbol)
    __shared__ uint32_t s_first[34];                                   // index into s_sorted of the first symbol of a length
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint64_t off = b * (uint64_t)P.block;
    const uint32_t n = (uint32_t)((n_total - off) < P.block ? (n_total - off) : P.block);
    const uint64_t rb = block_bits[b], re = block_bits[b + 1];
    // the record must lie inside the stream: every later read is bounded by [rb, re)
    bool bad = (rb & 31u) || (re & 31u) || re < rb + DEFH_HDR * 8ull || re > stream_bytes * 8ull;
    if (bad) { if (lane == 0) atomicOr(err, 1u); return; }
    const uint32_t *rec = reinterpret_cast<const uint32_t *>(stream + (rb >> 3));
    const uint32_t ntok = rec[0];
    // n bytes of output need at most n tokens of at most 64 bits
    const uint64_t words64 = ((re - rb) >> 5) - DEFH_HDR / 4;
    const uint32_t nwords = words64 > 2ull * n + 2u ? 2u * n + 2u : (uint32_t)words64;
    const uint32_t *w = rec + DEFH_HDR / 4;
    for (uint32_t i = lane; i < (DEFH_NSYM + 2) / 4; i += 64) reinterpret_cast<uint32_t *>(s_len)[i] = rec[1 + i];
    __syncthreads();
    defh_canonical(s_len, s_code, s_count, s_next);
    // tables: first-code / sorted symbols for the general walk, a direct LUT for codes <= DEFH_LUT_BITS
    for (uint32_t i = lane; i < (1u << DEFH_LUT_BITS); i += 64) s_lut[i] = 0xFFFFu;
    if (lane == 0) { uint32_t run = 0; for (int l = 0; l < 34; ++l) { s_first[l] = run; run += (l >= 1 && l <= 32) ? s_count[l] : 0u; } }
    __syncthreads();
    for (uint32_t s = lane; s < DEFH_NSYM; s += 64) {
        const uint32_t l = s_len[s];
        if (l > 32) bad = true;
        if (l && l <= 32) {
            const uint32_t c = s_code[s];
            s_sorted[s_first[l] + (c - s_next[l])] = (uint16_t)s;
            if (l <= DEFH_LUT_BITS) {
                const uint32_t lo = c << (DEFH_LUT_BITS - l);
                if (lo + (1u << (DEFH_LUT_BITS - l)) > (1u << DEFH_LUT_BITS)) bad = true;       // over-subscribed lengths
                else for (uint32_t k = 0; k < (1u << (DEFH_LUT_BITS - l)); ++k) s_lut[lo + k] = (uint16_t)(s | (l << 9));
            }
        }
    }
    if (__ballot(bad) != 0ull) { if (lane == 0) atomicOr(err, 1u); return; }
    __syncthreads();

    // every control value below is wave-uniform: the bit buffer sits in SGPRs and is refilled from 64 record words held
    // one per lane (lz_decode.h); the only memory on a token's critical path is its LUT cell
    const uint32_t nbits = nwords * 32u;                               // nwords <= 2 n + 2
    BitsMsb br;
    br.init(w, nwords, lane);
    OutRing<RING> ring;
    ring.init(s_ring, out + off, lane);
    uint32_t pos = 0;
    uint32_t o = 0;
    for (uint32_t t = 0; t < ntok && o < n; ++t) {
        br.refill();
        const uint32_t v = br.top32();
        uint32_t sym, l;
        const uint32_t e = s_lut[v >> (32 - DEFH_LUT_BITS)];
        if (e != 0xFFFFu) { sym = e & 511u; l = e >> 9; }
        else {
            sym = DEFH_NSYM; l = DEFH_LUT_BITS + 1;
            for (; l <= 32; ++l) {
                const uint32_t c = v >> (32u - l), rel = c - s_next[l];
                if (c >= s_next[l] && rel < s_count[l]) { sym = s_sorted[s_first[l] + rel]; break; }
            }
            if (sym == DEFH_NSYM) { bad = true; break; }
        }
        br.skip(l); pos += l;
        if (sym < 256u) {
            ring.put_literal(o, sym);
            o += 1;
        } else {
            const uint32_t cz = sym - 256u;
            if (cz < 1u || cz > 15u) { bad = true; break; }
            br.refill();
            const uint32_t nx = 15u - cz, x = br.top32();
            const uint32_t d = (1u << nx) + (nx ? x >> (32u - nx) : 0u);
            const uint32_t len = (x << nx) >> 27;
            br.skip(nx + 5u); pos += nx + 5u;
            if (d > o) { bad = true; break; }
            const uint32_t take = (o + len <= n) ? len : n - o;
            ring.copy(o, d, take);
            o += take;
        }
        if (pos > nbits) { bad = true; break; }
        __builtin_amdgcn_wave_barrier();
        ring.advance(o);
    }
    if (o != n) bad = true;
    if (bad) { if (lane == 0) atomicOr(err, 1u); return; }
    ring.finish(n);
}

extern "C" uint64_t mi_deflate_h_bound_bytes(uint64_t n, const mi_lz_params *p)
{
    // Per block of b bytes: a Huffman code cannot be longer than a fixed 9-bit code over 286 symbols, and a match
    // (code + <= 15 offset bits + 5 length bits <= 29 bits) replaces >= 4 literals (36 bits) — except the block's last
    // token, which may be a match that covers ONE real byte and runs into the zero tail: 9 b + 20 bits at most.
    // Plus the 292-byte header; records are whole words.  Every block pays the header, so the bound depends on p->block.
    const uint64_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK;
    const uint64_t nblocks = (n + block - 1) / block;
    const uint64_t last = n - (nblocks ? (nblocks - 1) * block : 0);
    auto rec = [](uint64_t b) -> uint64_t { return DEFH_HDR + 4 * ((9 * b + 20 + 31) / 32); };
    return (nblocks ? (nblocks - 1) * rec(block) + rec(last) : 0) + 64;
}

// launch alone: errors accumulate in *err (an mi_err_slot the caller reads once everything it launched has run)
mi_status mi_deflate_h_decode_launch(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                                     const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, uint32_t *err, hipStream_t s)
{
    if (!ctx || !d_stream || !d_block_bits || (n && !d_out) || !err) return MI_ERR_ARG;
    mi_status st = lz_check_params(p);
    if (st) return st;
    if (!p->deflate || p->lbits > 5 || p->wbits > 16 || ((uintptr_t)d_stream & 3u)) return MI_ERR_ARG;
    if (n == 0) return MI_OK;
    const LzP P = lz_params_of(ctx, p);
    const uint64_t nblocks = (n + P.block - 1) / P.block;
    {
        mi_prof_scope pr(ctx, "k_defh_decode", s, n);
        // a 4 KiB ring whatever the window (lz_decode.h): far matches read the output buffer
        const uint32_t W = 1u << P.wbits, need = W < P.block ? W : P.block;
        const uint32_t want = lz_decode_ring_want(nblocks, need, 4096u);                      // (few blocks: lz_decode.hip; with the 11-bit LUT 4 KiB: 17 GB/s, 8 KiB: 15, 16 KiB: 12.4, 2 KiB: 16.2; 9-bit LUT: 19.5 at 4 KiB, 19.7 at 8)
        if (want <= 4096u) hipLaunchKernelGGL(k_defh_decode<4096u>, dim3((unsigned)nblocks), dim3(64), 0, s, d_stream, stream_bytes, d_block_bits, P, d_out, n, err);
        else if (want <= 8192u) hipLaunchKernelGGL(k_defh_decode<8192u>, dim3((unsigned)nblocks), dim3(64), 0, s, d_stream, stream_bytes, d_block_bits, P, d_out, n, err);
        else if (need <= 16384u || want <= 16384u) hipLaunchKernelGGL(k_defh_decode<16384u>, dim3((unsigned)nblocks), dim3(64), 0, s, d_stream, stream_bytes, d_block_bits, P, d_out, n, err);
        else if (need <= 32768u || want <= 32768u) hipLaunchKernelGGL(k_defh_decode<32768u>, dim3((unsigned)nblocks), dim3(64), 0, s, d_stream, stream_bytes, d_block_bits, P, d_out, n, err);
        else hipLaunchKernelGGL(k_defh_decode<65536u>, dim3((unsigned)nblocks), dim3(64), 0, s, d_stream, stream_bytes, d_block_bits, P, d_out, n, err);
    }
    return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

extern "C" mi_status mi_deflate_h_decode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                                             const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, void *stream)
{
    if (!ctx || !d_stream || !d_block_bits || (n && !d_out)) return MI_ERR_ARG;
    mi_status st = lz_check_params(p);
    if (st) return st;
    if (!p->deflate || p->lbits > 5 || p->wbits > 16 || ((uintptr_t)d_stream & 3u)) return MI_ERR_ARG;
    if (n == 0) return MI_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *err = mi_err_slot(ctx, s);
    if (!err) return MI_ERR_HIP;
    st = mi_deflate_h_decode_launch(ctx, p, d_stream, stream_bytes, d_block_bits, d_out, n, err, s);
    if (st) return st;
    uint32_t h_err = 0;
    MI_HIP(ctx, hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return h_err ? MI_ERR_CORRUPT : MI_OK;
}
