// snappy_batch.hip — many independent raw Snappy buffers (format_description.txt of google/snappy: a varint32 preamble with the
// uncompressed length, then literal and copy elements; no framing, no checksum) decoded in one launch: every item at its own
// address, of its own size, into its own buffer of a given CAPACITY, with its own verdict and length written on the device.
// The frame is inflate_batch.hip's — one wave per item, parallel across items only — and the token loop is k_inflate's without
// the Huffman tables.  include/mi_codec.h has the contract.
//
//   k_snappy_batch<RING>   one wave per item.  The preamble is read by the wave itself and decides MI_ERR_CAPACITY before any
//                     store (Snappy names its size up front: no counting walk).  Tags and their length / offset bytes come
//                     wave-uniform out of the register window (BitsLsb over WaveWords, lz_decode.h: an item may start at any
//                     byte address, and no dword outside those that cover [in, in + nb) is loaded); a literal's bytes go from
//                     the input into the ring lane-parallel, at most SNP_PIECE per step so that OutRing::advance keeps its
//                     contract; copies are OutRing::copy (near, far, overlapping).  Every bound is checked before the element
//                     stores: a malformed item is MI_ERR_CORRUPT, never a fault, and no byte at or past min(cap, preamble) is
//                     written.
//   k_snappy_batch_size    one thread per item: the preamble alone (snappy::GetUncompressedLength) with the same header
//                     verdicts; the body is not looked at.
//
// LDS per wave: the ring only — 4 096 bytes, or 32 768 in a call of fewer than 1 024 items (lz_decode_ring_want).
#include "lz_common.h"
#include "lz_decode.h"
#include "internal.h"

#define SNP_PIECE 512u                         // literal bytes per step: eight loads per lane in flight, < OutRing<4096>::CH

struct SnapBatch {
    const void *const *in; const uint64_t *in_bytes;
    void *const *out; const uint64_t *out_cap;
    uint64_t *out_bytes; uint32_t *status, *failed;
};

// The preamble of an item of nb >= 1 bytes, byte(i) its byte i < nb: a little-endian base-128 varint of at most five bytes whose
// value fits 32 bits (what snappy's Varint::Parse32WithLimit takes).  -> MI_OK with *n and *hb (its length), MI_ERR_CORRUPT (it
// runs past the item, has a sixth byte or more than 32 bits), MI_ERR_ARG (well-formed, but above the per-item limit).
template <class Byte>
__device__ __forceinline__ uint32_t snappy_preamble(uint64_t nb, Byte byte, uint32_t *n, uint32_t *hb)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < 5u; ++k) {
        if (k >= nb) return MI_ERR_CORRUPT;
        const uint32_t c = byte(k);
        v |= (uint64_t)(c & 0x7Fu) << (7u * k);
        if (c < 0x80u) {
            if (v > 0xFFFFFFFFull) return MI_ERR_CORRUPT;
            if (v > INFB_MAX_BYTES) return MI_ERR_ARG;
            *n = (uint32_t)v; *hb = k + 1u;
            return MI_OK;
        }
    }
    return MI_ERR_CORRUPT;
}

template <uint32_t RING>
__global__ __launch_bounds__(64)
void k_snappy_batch(SnapBatch b)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[RING];
    static_assert(SNP_PIECE <= OutRing<RING>::CH, "a step adds at most one quarter of the ring");
    const uint32_t lane = threadIdx.x, item = blockIdx.x;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(b.in[item]);
    const uint64_t nb = b.in_bytes[item];
    uint8_t *out = reinterpret_cast<uint8_t *>(b.out[item]);
    const uint64_t cap = b.out_cap[item];
    uint32_t st = MI_OK;
    uint64_t size = 0;
    if ((nb && !in) || (cap && !out) || nb > INFB_MAX_BYTES || cap > INFB_MAX_BYTES) st = MI_ERR_ARG;
    else if (nb == 0) st = MI_ERR_CORRUPT;                             // (not even a preamble)
    else {
        BitsLsb br;
        br.init(in, 0, 8ull * nb, lane);
        uint32_t n = 0, ip = 0;
        st = snappy_preamble(nb, [&](uint32_t) -> uint32_t { br.refill(); const uint32_t c = br.peek(8); br.skip(8); return c; }, &n, &ip);
        if (st == MI_OK && n > cap) { st = MI_ERR_CAPACITY; size = n; }    // before any store: nothing is written
        else if (st == MI_OK) {
            OutRing<RING> ring;
            ring.init(s_ring, out, lane);
            const uint32_t end = (uint32_t)nb;
            uint32_t o = 0;
            bool bad = false;
            // every element adds at least one byte, so input behind the n-th byte fails `len > n - o` like an element that is too long
            while (ip < end) {
                br.refill();
                const uint32_t tag = br.peek(8);
                br.skip(8); ++ip;
                const uint32_t kind = tag & 3u;
                // the bytes behind the tag: a literal's length bytes, a copy's offset bytes
                const uint32_t extra = kind == 0u ? ((tag >> 2) >= 60u ? (tag >> 2) - 59u : 0u) : kind == 3u ? 4u : kind;
                if (extra > end - ip) { bad = true; break; }           // the input ends inside the element
                br.refill();
                const uint32_t x = extra == 4u ? (uint32_t)br.buf : (uint32_t)br.buf & ((1u << (8u * extra)) - 1u);
                if (extra) { br.skip(8u * extra); ip += extra; }       // (at most 32 of the more than 32 bits held)
                if (kind == 0u) {
                    const uint64_t len = (extra ? (uint64_t)x : (uint64_t)(tag >> 2)) + 1u;
                    if (len > end - ip || len > n - o) { bad = true; break; }
                    const uint8_t *src = in + ip;
                    for (uint32_t done = 0; done < (uint32_t)len;) {
                        const uint32_t piece = (uint32_t)len - done < SNP_PIECE ? (uint32_t)len - done : SNP_PIECE;
                        uint8_t v[SNP_PIECE / 64u];
#pragma unroll
                        for (uint32_t q = 0; q < SNP_PIECE / 64u; ++q) { const uint32_t j = q * 64u + lane; v[q] = j < piece ? src[done + j] : (uint8_t)0; }
#pragma unroll
                        for (uint32_t q = 0; q < SNP_PIECE / 64u; ++q) { const uint32_t j = q * 64u + lane; if (j < piece) s_ring[(o + j) & OutRing<RING>::RM] = v[q]; }
                        done += piece; o += piece;
                        __builtin_amdgcn_wave_barrier();
                        ring.advance(o);
                    }
                    ip += (uint32_t)len;
                    if (ip < end) bits_seek_bytes(br, in, nb, ip, (uint32_t)len, lane);
                } else {
                    uint32_t len, d;
                    if (kind == 1u) { len = 4u + ((tag >> 2) & 7u); d = ((tag >> 5) << 8) | x; }
                    else { len = (tag >> 2) + 1u; d = x; }
                    if (d == 0u || d > o || len > n - o) { bad = true; break; }
                    ring.copy(o, d, len);
                    o += len;
                    __builtin_amdgcn_wave_barrier();
                    ring.advance(o);
                }
            }
            if (bad || o != n) st = MI_ERR_CORRUPT;
            else { size = n; ring.finish(n); }
        }
    }
    if (lane == 0) {
        b.status[item] = st;
        b.out_bytes[item] = size;
        if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
    }
}

__global__ __launch_bounds__(256)
void k_snappy_batch_size(SnapBatch b, uint32_t count)
{
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= count) return;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(b.in[item]);
    const uint64_t nb = b.in_bytes[item];
    uint32_t st, n = 0, hb = 0;
    if ((nb && !in) || nb > INFB_MAX_BYTES) st = MI_ERR_ARG;
    else if (nb == 0) st = MI_ERR_CORRUPT;
    else st = snappy_preamble(nb, [&](uint32_t k) -> uint32_t { return in[k]; }, &n, &hb);
    b.status[item] = st;
    b.out_bytes[item] = st == MI_OK ? n : 0u;
    if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
}

// ---------------------------------------------------------------------------------------------------------------------
// The encoder: LZ_SNAPPY, a form of the one pipeline (lz_emit.hip).  Finder and parse are mode Z's (k_lz_parse_emit leaves one
// u32 record per token); this is the last stage in place of k_defz_plan / k_defz_encode.  Records are whole bytes, and the
// batch's placement (deflate_batch.hip) puts them behind each item's preamble.
//
// The emission rule, over a block's tokens after mode Z's clip of a last match that runs past the block (defz.hip):
//   a literal, or a match shorter than 4, joins the pending literal run;
//   a match (L >= 4, d) flushes the run as ONE literal element in its shortest form (tag len - 1 < 60, or 60 and one length
//   byte, or 61 and two: a run is at most a block), then becomes copies by stock Snappy's split — 64 while L >= 68, then 60
//   if L > 64, then the rest, so that every piece is >= 4 — each a copy-1 when 4 <= len <= 11 and d < 2048, else a copy-2
//   (d <= 32 768 always fits; copy-4 is never written);
//   the run pending at the block's end is flushed.
//
//   k_snappy_emit   one workgroup per block; thread t owns the tokens [t C, (t + 1) C), C = ceil(ntok / 256), and walks them
//                   four times, a workgroup scan between two walks:
//                     1. input bytes covered -> where the thread's tokens start
//                     2. the end of its last copy -> (max scan) where the run pending at its first token began
//                     3. bytes of the elements it owns — a literal element belongs to the copy that flushes it, the block's
//                        last run to thread 255 -> (sum scan) where they go, and the record's size
//                     4. the stores: tags, copies, and the bytes of runs up to SNE_INLINE; a longer run goes on a list in
//                        LDS that the whole workgroup copies afterwards, a wave per run
//                   block_bits[lb] = 8 x the record's bytes.  A PAD block (one zero byte) comes out as 00 00 and is placed nowhere.
// ---------------------------------------------------------------------------------------------------------------------
#define SNE_THREADS 256
#define SNE_INLINE  16u                        // a run up to this long is copied by the thread that writes its tag
// longer runs per block: each but the last is followed by a copy, so together they cover more than SNE_INLINE + 4 bytes
#define SNE_RUNS    (LZ_MAX_BLOCK / (SNE_INLINE + 1u + 4u) + 2u)

struct OpMaxU32 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };

// bytes of the tag and length bytes of a literal element of r bytes (r <= 65 536)
__device__ __forceinline__ uint32_t sn_lit_head(uint32_t r) { return r == 0u ? 0u : r <= 60u ? 1u : r <= 256u ? 2u : 3u; }
// bytes of the copies of a match (L >= 4, d)
__device__ __forceinline__ uint32_t sn_copy_bytes(uint32_t L, uint32_t d)
{
    uint32_t b = 0;
    while (L >= 68u) { b += 3u; L -= 64u; }
    if (L > 64u) { b += 3u; L -= 60u; }
    return b + ((L <= 11u && d < 2048u) ? 2u : 3u);
}
__device__ __forceinline__ uint32_t sn_put_copy(uint8_t *o, uint32_t len, uint32_t d)
{
    if (len <= 11u && d < 2048u) { o[0] = (uint8_t)(1u | ((len - 4u) << 2) | ((d >> 8) << 5)); o[1] = (uint8_t)d; return 2u; }
    o[0] = (uint8_t)(2u | ((len - 1u) << 2)); o[1] = (uint8_t)d; o[2] = (uint8_t)(d >> 8);
    return 3u;
}
__device__ __forceinline__ uint32_t sn_put_match(uint8_t *o, uint32_t L, uint32_t d)
{
    uint32_t b = 0;
    while (L >= 68u) { b += sn_put_copy(o + b, 64u, d); L -= 64u; }
    if (L > 64u) { b += sn_put_copy(o + b, 60u, d); L -= 60u; }
    return b + sn_put_copy(o + b, L, d);
}
__device__ __forceinline__ uint32_t sn_put_lit_head(uint8_t *o, uint32_t r)
{
    const uint32_t v = r - 1u;
    if (r <= 60u) { o[0] = (uint8_t)(v << 2); return 1u; }
    if (r <= 256u) { o[0] = (uint8_t)(60u << 2); o[1] = (uint8_t)v; return 2u; }
    o[0] = (uint8_t)(61u << 2); o[1] = (uint8_t)v; o[2] = (uint8_t)(v >> 8);
    return 3u;
}

__global__ __launch_bounds__(SNE_THREADS)
void k_snappy_emit(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, uint64_t *__restrict__ block_bits,
                   const uint8_t *__restrict__ in, uint32_t block, uint64_t block0)
{
    __shared__ uint32_t s_tmp[SNE_THREADS / 64 + 2];
    __shared__ uint32_t s_run[SNE_RUNS], s_dst[SNE_RUNS];              // run: first byte | (length - 1) << 16
    __shared__ uint32_t s_nrun;
    const uint32_t tid = threadIdx.x, lb = blockIdx.x;
    const uint8_t *src; uint32_t n;
    lz_block_src<true>(in, 0, block, block0, lb, src, n);
    const uint32_t ntok = (uint32_t)block_bits[lb];                    // k_lz_parse_emit left the token count here (>= 1)
    const uint32_t *trec = trec_all + (size_t)lb * LZ_MAX_BLOCK;
    uint8_t *out = reinterpret_cast<uint8_t *>(slots + (size_t)lb * LZ_SLOT_WORDS);
    const uint32_t per = (ntok + SNE_THREADS - 1u) / SNE_THREADS;
    const uint32_t t0 = tid * per < ntok ? tid * per : ntok, t1 = t0 + per < ntok ? t0 + per : ntok;
    if (tid == 0) s_nrun = 0;
    // ---- 1: where the thread's tokens start (only the block's last token may cover bytes past n: nothing starts behind it)
    uint32_t cov = 0;
    for (uint32_t t = t0; t < t1; ++t) { const uint32_t r = trec[t]; cov += (r >> 31) ? (r >> 16) & 0x7FFFu : 1u; }
    uint32_t total;
    const uint32_t p0 = block_exclusive_scan<uint32_t>(cov, OpAddU32(), 0u, s_tmp, &total);
    // token r at position p -> the bytes it covers after the clip; *d != 0: it is a copy
    auto token = [&](uint32_t r, uint32_t p, uint32_t *d) -> uint32_t {
        *d = 0;
        if (!(r >> 31)) return 1u;
        const uint32_t L = (r >> 16) & 0x7FFFu, Lc = L < n - p ? L : n - p;
        if (Lc >= 4u) *d = r & 0xFFFFu;
        return Lc;
    };
    // ---- 2: where the run pending at the thread's first token began: behind the last copy in front of it
    uint32_t last_end = 0;
    for (uint32_t t = t0, p = p0; t < t1; ++t) { uint32_t d; const uint32_t c = token(trec[t], p, &d); p += c; if (d) last_end = p; }
    uint32_t tail_from;                                                // where the block's last run begins
    const uint32_t rs0 = block_exclusive_scan<uint32_t>(last_end, OpMaxU32(), 0u, s_tmp, &tail_from);
    // ---- 3: the bytes of the elements the thread owns
    uint32_t bytes = 0;
    for (uint32_t t = t0, p = p0, rs = rs0; t < t1; ++t) {
        uint32_t d;
        const uint32_t c = token(trec[t], p, &d);
        if (d) { bytes += sn_lit_head(p - rs) + (p - rs) + sn_copy_bytes(c, d); rs = p + c; }
        p += c;
    }
    if (tid == SNE_THREADS - 1u) bytes += sn_lit_head(n - tail_from) + (n - tail_from);
    uint32_t rec;
    uint32_t o = block_exclusive_scan<uint32_t>(bytes, OpAddU32(), 0u, s_tmp, &rec);
    // ---- 4: the stores.  A run's bytes are contiguous input: [rs, rs + r) -> out[at, at + r)
    auto literal = [&](uint32_t rs, uint32_t r) {
        if (r == 0u) return;
        o += sn_put_lit_head(out + o, r);
        uint32_t k = SNE_RUNS;
        if (r > SNE_INLINE) k = atomicAdd(&s_nrun, 1u);
        if (k < SNE_RUNS) { s_run[k] = rs | ((r - 1u) << 16); s_dst[k] = o; }
        else for (uint32_t j = 0; j < r; ++j) out[o + j] = src[rs + j];
        o += r;
    };
    {
        uint32_t rs = rs0;
        for (uint32_t t = t0, p = p0; t < t1; ++t) {
            uint32_t d;
            const uint32_t c = token(trec[t], p, &d);
            if (d) { literal(rs, p - rs); o += sn_put_match(out + o, c, d); rs = p + c; }
            p += c;
        }
        if (tid == SNE_THREADS - 1u) literal(tail_from, n - tail_from);
    }
    __syncthreads();
    const uint32_t nrun = s_nrun < SNE_RUNS ? s_nrun : SNE_RUNS;
    for (uint32_t k = tid >> 6; k < nrun; k += SNE_THREADS / 64u) {
        const uint32_t rs = s_run[k] & 0xFFFFu, r = (s_run[k] >> 16) + 1u, at = s_dst[k];
        for (uint32_t j = tid & 63u; j < r; j += 64u) out[at + j] = src[rs + j];
    }
    if (tid == 0) block_bits[lb] = 8ull * rec;
}

void snappy_launch_emit(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, const uint8_t *d_desc, uint32_t block,
                        uint64_t b0, uint32_t nb, hipStream_t s)
{
    hipLaunchKernelGGL(k_snappy_emit, dim3(nb), dim3(SNE_THREADS), 0, s, trec, slots, block_bits, d_desc, block, b0);
}

// An item of n bytes in blocks of b: a run of r literals in front of a copy costs sn_lit_head(r) - 1 bytes more than the input
// bytes the two cover (the copy itself at most 3 for at least 4), and sn_lit_head(r) - 1 <= r / 61 (1 from 61 on, 2 from 257);
// the last run of a block, which no copy follows, costs at most 3; the preamble at most 5.
extern "C" uint64_t mi_snappy_batch_bound_bytes(uint64_t n_item, const mi_lz_params *p)
{
    const uint64_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK;
    return 5u + n_item + n_item / 61u + 3u * ((n_item + block - 1u) / block);
}

extern "C" uint64_t mi_snappy_batch_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p)
{
    return mi_deflate_batch_max_blocks(total_in_bytes, count, p);
}

extern "C" mi_status mi_snappy_encode_batch_dev(mi_ctx *ctx, const mi_lz_params *p, uint64_t count, const void *const *d_in,
                                                const uint64_t *d_in_bytes, uint64_t max_blocks, void *const *d_out,
                                                const uint64_t *d_out_cap, uint64_t *d_out_bytes, uint32_t *d_status,
                                                uint32_t *d_failed, void *stream)
{
    if (!ctx) return MI_ERR_ARG;
    mi_status st = defz_check(p, MI_CONTAINER_RAW);
    if (st) return st;
    if (count > DFB_MAX_BYTES || max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out || !d_out_cap || !d_out_bytes || !d_status) return MI_ERR_ARG;
    const DfbCall b{DFB_SNAPPY, count, max_blocks, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed};
    return lz_encode_impl(ctx, p, nullptr, 0, nullptr, 0, nullptr, stream, LzCall{LZ_SNAPPY, DFB_SNAPPY, nullptr, &b});
}

extern "C" mi_status mi_snappy_decode_batch_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                                void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                                uint32_t *d_status, uint32_t *d_failed, uint32_t flags, void *stream)
{
    if (!ctx || flags || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out || !d_out_cap || !d_out_bytes || !d_status) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cnt = (uint32_t)count;
    if (d_failed) MI_HIP(ctx, hipMemsetAsync(d_failed, 0, 4, s));
    const SnapBatch b{d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed};
    {
        mi_prof_scope pr(ctx, "k_snappy_batch", s, 0);
        // the ring: as the batched inflate — few items cannot fill the CUs anyway and get a 32 KiB ring
        if (lz_decode_ring_want(cnt, 32768u, 4096u) <= 4096u) hipLaunchKernelGGL((k_snappy_batch<4096u>), dim3(cnt), dim3(64), 0, s, b);
        else hipLaunchKernelGGL((k_snappy_batch<32768u>), dim3(cnt), dim3(64), 0, s, b);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

extern "C" mi_status mi_snappy_batch_size_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                              uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, void *stream)
{
    if (!ctx || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out_bytes || !d_status) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cnt = (uint32_t)count;
    if (d_failed) MI_HIP(ctx, hipMemsetAsync(d_failed, 0, 4, s));
    const SnapBatch b{d_in, d_in_bytes, nullptr, nullptr, d_out_bytes, d_status, d_failed};
    {
        mi_prof_scope pr(ctx, "k_snappy_batch_size", s, 0);
        hipLaunchKernelGGL(k_snappy_batch_size, dim3((cnt + 255u) / 256u), dim3(256), 0, s, b, cnt);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}
