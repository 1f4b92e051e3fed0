// deflate_batch.hip — many independent buffers compressed in one call: every item from its own address, of its own size, into
// its own buffer of a given CAPACITY as a complete raw / zlib / gzip stream, with its own verdict and length written on the
// device.  Item i's bytes are exactly what mi_deflate_z_encode_dev writes for item i alone: the blocks of all items run through
// the one encoder pipeline (lz_encode_impl, lz_emit.hip) — finder, parse, entropy stage see a BLOCK, and nothing in them looks
// across a block boundary.  include/mi_codec.h has the contract.  What a batch adds:
//
//   k_dfb_scan     one workgroup over the size array: blocks per item, exclusive scan, the MI_ERR_ARG verdicts (a NULL pointer
//                  with a size, a size or capacity above 2^31 - 1, blocks that do not fit the caller's bound), the real block count
//   k_dfb_fill     one thread per block of the bound: {address, length, item, number in the item, last} (LzBlkDesc, lz_common.h),
//                  the item found by a binary search over the scan; behind the real blocks PAD blocks of one zero byte
//   k_dfb_cksum    one workgroup per block: the pure CRC-32 (gzip) or the raw Adler-32 sums (zlib) of the block's INPUT bytes
//                  (crc32.h / adler32.h); combined per item at the end, so that one 100 MB item is not one workgroup's tail
//   (the pipeline: the six kernels that read input bytes take the block from the table — lz_block_src, template parameter DESC)
//   k_dfb_place    per pipeline batch, one workgroup per block, in place of scan / concatenate: records are whole bytes, so the
//                  record goes to d_out[item] + header + (bytes of the item's earlier records) — dword stores where the
//                  destination is aligned, bytes at the edges, every store checked against the item's capacity
//   k_dfb_finish   one wave per item: the checksum from its blocks' parts, container header, 03 00, trailer, size, verdict
// The batched Snappy encoder (snappy_batch.hip) runs the same frame with its own records: DFB_SNAPPY in DfbCall.container makes the
// bytes in front of an item's records a function of the item (its preamble) and the finish write that preamble and nothing else.
// The batched LZ4 encoder (lz4_batch.hip) likewise: DFB_LZ4_BLOCK has no header and refuses an item of more than one block in the
// scan; DFB_LZ4_FRAME has a uniform 7-byte header and the finish writes it and the EndMark.
//
// The grid of every pipeline kernel is sized by the caller's bound (no device-to-host read), so blocks between the real count
// and the bound exist as PAD blocks: one zero byte each, encoded like any one-byte block and placed nowhere.  They do not
// "return at once": the stages behind the six kernels (find, replay, the fallback chain) index per-block records that an early
// exit would leave as the previous batch wrote them; a one-byte block is a case every stage already handles.  A tight bound
// (mi_deflate_batch_max_blocks of the exact total) has fewer than total / block + 1 of them.
//
// A preset dictionary (mi_deflate_batch_dict_dev; zlib's deflateSetDictionary): one per call, read-only.  U, its last
// min(dict_bytes, 32 768, block / 2) bytes, lies in front of every item's first block, which holds block - |U| bytes of the item
// so that U and the head are one block to the finder (internal.h: dfb_first, dfb_nblk); the later blocks are today's.
//   k_dfb_stage    per pipeline batch, one workgroup per block: for an item's first block, U and the item's head into the block
//                  slot's CELL of the batch's scratch set — the finder wants contiguous bytes.  The descriptor points at the cell
//                  with n = |U| + head and skip = |U|; the parse starts at skip (k_lz_parse_emit<DESC, DICT>), the entropy stage
//                  and the checksums work on the item's bytes behind it.  Cells: one block-sized cell per block slot of a set,
//                  whatever the count of items.
//   the zlib header is then 78 BB and the Adler-32 of the WHOLE dictionary (DICTID), computed on the stream
#include "lz_common.h"
#include "crc32.h"
#include "adler32.h"
#include "internal.h"

#define DFB_HEAD      256u                     // workspace head: u32 nreal, u64 carry[2] at byte 8, a zero byte at byte 64 (the PAD block),
                                               // u32 DICTID at byte 128
#define DFB_DICTID_AT 128u

struct DfbWs {
    uint8_t   *head;
    uint32_t  *item_first;                     // [count] first block of the item (clamped to the bound): ascending
    uint32_t  *item_st;                        // [count] MI_OK or MI_ERR_ARG
    uint64_t  *item_total;                     // [count] bytes of the item's records (written with its last block)
    uint32_t  *ck;                             // [2 * max_blocks] per block: pure CRC-32, or the raw Adler sums a, s
    LzBlkDesc *desc;                           // [max_blocks]
    uint8_t   *zck;                            // the partials of the dictionary's Adler-32 (zlib with a dictionary)
    size_t     bytes;
};

static DfbWs dfb_carve(void *ws, const DfbCall &b)
{
    mi_carver cv(ws);
    DfbWs w;
    w.head = cv.take<uint8_t>(DFB_HEAD);
    w.item_first = cv.take<uint32_t>(b.count);
    w.item_st = cv.take<uint32_t>(b.count);
    w.item_total = cv.take<uint64_t>(b.count);
    w.ck = cv.take<uint32_t>(2 * b.max_blocks);
    w.desc = cv.take<LzBlkDesc>(b.max_blocks);
    w.zck = b.ulen && b.container == MI_CONTAINER_ZLIB ? cv.take<uint8_t>(defz_ws_bytes()) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

size_t dfb_ws_bytes(const DfbCall &b) { return dfb_carve(nullptr, b).bytes; }

// one cell per block slot of a scratch set, and room for the 16-byte words the block loaders round their reads out to
size_t dfb_stage_bytes(const DfbCall &b, uint32_t nbmax, uint32_t block) { return b.ulen ? (size_t)nbmax * block + 64u : 0; }

// the bytes in front of an item's first record.  The three DEFLATE containers: the container header, the same for every item of a
// call (`uniform`, from the host: with a dictionary the zlib header carries DICTID).  Snappy: the item's preamble, varint32(in_bytes).
// LZ4: uniform too — nothing in front of a raw block, the frame header's seven bytes.
static uint32_t dfb_header_uniform(const DfbCall &b)
{
    if (b.container == DFB_LZ4_BLOCK || b.container == DFB_LZ4_FRAME) return b.container == DFB_LZ4_FRAME ? 7u : 0u;
    return b.container == DFB_SNAPPY ? 0u : defz_header_bytes(b.container) + (b.ulen && b.container == MI_CONTAINER_ZLIB ? 4u : 0u);
}
__device__ __forceinline__ uint32_t dfb_header_bytes(const DfbCall &b, uint32_t item, uint32_t uniform)
{
    return b.container == DFB_SNAPPY ? dfb_varint_bytes(b.in_bytes[item]) : uniform;
}

struct OpAddU64 { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; } };

__global__ __launch_bounds__(1024)
void k_dfb_scan(DfbCall b, uint32_t block, uint32_t *__restrict__ item_first, uint32_t *__restrict__ item_st, uint32_t *__restrict__ nreal)
{
    __shared__ uint64_t s_tmp[18];
    __shared__ uint32_t s_real;
    const uint32_t tid = threadIdx.x, count = (uint32_t)b.count;
    if (tid == 0) s_real = 0;
    __syncthreads();
    uint64_t run = 0;                                                  // blocks of the items before this round (uniform)
    for (uint32_t base = 0; base < count; base += 1024u) {
        const uint32_t i = base + tid;
        uint64_t nblk = 0;
        uint32_t st = MI_OK;
        if (i < count) {
            const uint64_t nb = b.in_bytes[i], cap = b.out_cap[i];
            if ((nb && !b.in[i]) || (cap && !b.out[i]) || nb > DFB_MAX_BYTES || cap > DFB_MAX_BYTES) st = MI_ERR_ARG;
            else if (b.container == DFB_LZ4_BLOCK && nb > block) st = MI_ERR_ARG;      // a raw LZ4 item is one block: refused alone, with 0 blocks
            else nblk = dfb_nblk(nb, block, b.ulen);
        }
        uint64_t tot;
        const uint64_t first = run + block_exclusive_scan<uint64_t>(nblk, OpAddU64(), 0ull, s_tmp, &tot);
        if (i < count) {
            // an item whose blocks do not fit the bound is refused, and with it every item behind it (their first block lies
            // past the bound too); the items before it are untouched
            if (st == MI_OK && first + nblk > b.max_blocks) st = MI_ERR_ARG;
            if (st == MI_OK && nblk) atomicMax(&s_real, (uint32_t)(first + nblk));
            item_first[i] = (uint32_t)(first < b.max_blocks ? first : b.max_blocks);
            item_st[i] = st;
        }
        run += tot;
    }
    __syncthreads();
    if (tid == 0) *nreal = s_real;
}

__global__ __launch_bounds__(256)
void k_dfb_fill(DfbCall b, uint32_t block, const uint32_t *__restrict__ item_first, const uint32_t *__restrict__ nreal,
                const uint8_t *pad_byte, LzBlkDesc *__restrict__ desc)
{
    const uint64_t g64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g64 >= b.max_blocks) return;
    const uint32_t g = (uint32_t)g64;
    LzBlkDesc d;
    d.skip = 0;
    if (g >= *nreal) { d.src = pad_byte; d.n = 1u; d.item = LZ_DESC_PAD; d.blk = 0u; d.last = 0u; }
    else {
        // the last item whose first block is <= g: items without blocks share their first block with the next item that has
        // some, which comes last among them; refused items start at or behind the real count
        uint32_t lo = 0, hi = (uint32_t)b.count - 1u;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (item_first[mid] <= g) lo = mid; else hi = mid - 1u; }
        const uint32_t blk = g - item_first[lo];
        const uint64_t nb = b.in_bytes[lo], off = dfb_begin_of(blk, block, b.ulen), room = blk ? block : block - b.ulen;
        d.src = reinterpret_cast<const uint8_t *>(b.in[lo]) + off;
        d.n = (uint32_t)((nb - off) < room ? (nb - off) : room);
        d.item = lo; d.blk = blk; d.last = off + room >= nb ? 1u : 0u;
        if (b.ulen && blk == 0u) {
            // the item's first block is read from its cell, behind U (k_dfb_stage fills it when the block's pipeline batch comes up)
            d.src = b.stage[(g / b.nbmax) % b.nsets] + (size_t)(g % b.nbmax) * block;
            d.n += b.ulen; d.skip = (uint16_t)b.ulen;
        }
    }
    desc[g] = d;
}

// the cells of one pipeline batch: U, then the head of the item whose first block this is
__global__ __launch_bounds__(256)
void k_dfb_stage(DfbCall b, const LzBlkDesc *__restrict__ desc, uint64_t b0)
{
    const LzBlkDesc d = desc[b0 + blockIdx.x];
    if (d.item == LZ_DESC_PAD || d.skip == 0u) return;                 // (the whole workgroup)
    uint8_t *cell = const_cast<uint8_t *>(d.src);                      // (inside this set's staging area: k_dfb_fill placed it)
    const uint8_t *u = b.dict + (b.dict_bytes - d.skip), *head = reinterpret_cast<const uint8_t *>(b.in[d.item]);
    for (uint32_t i = threadIdx.x; i < d.n; i += 256u) cell[i] = i < d.skip ? u[i] : head[i - d.skip];
}

// (a staged block's own bytes are read where the item has them: its cell is not filled before its pipeline batch comes up)
template <bool CRC>
__global__ __launch_bounds__(ZCK_THREADS)
void k_dfb_cksum(const LzBlkDesc *__restrict__ desc, uint32_t *__restrict__ ck, const void *const *__restrict__ in)
{
    __shared__ typename std::conditional<CRC, CrcLds, AdlerLds>::type s_lds;
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    LzBlkDesc d = desc[g];
    if (d.item == LZ_DESC_PAD) return;                                 // (the whole workgroup)
    if (d.skip) { d.src = reinterpret_cast<const uint8_t *>(in[d.item]); d.n -= d.skip; }
    if constexpr (CRC) {
        crc_lds_init(s_lds, tid);
        __syncthreads();
        const uint32_t pure = crc_range(d.src, d.n, s_lds, tid);
        if (tid == 0) ck[2u * g] = pure;
    } else {
        uint32_t ra, rs;
        adler_range(d.src, 0, d.n, (((uintptr_t)d.src) & 15u) == 0, s_lds, tid, ra, rs);
        if (tid == 0) { ck[2u * g] = ra; ck[2u * g + 1u] = rs; }
    }
}

// The records of one pipeline batch (blocks [b0, b0 + nb), slot lb holds block b0 + lb's record, block_bits[lb] its bits) to
// their items.  An item's blocks are consecutive, so the bytes of its earlier records are: the sum over its blocks of THIS batch
// in front of this one, plus — for the one item that began in an earlier batch — what that batch's last workgroup left in
// carry[seq & 1].  Batches reach the stream in order; the carry alternates between two words so that nobody reads the word
// the last workgroup writes.
__global__ __launch_bounds__(256)
void k_dfb_place(DfbCall b, const LzBlkDesc *__restrict__ desc, const uint32_t *__restrict__ item_first, uint64_t *__restrict__ item_total,
                 uint64_t *carry, uint32_t seq, uint32_t hb, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ block_bits,
                 uint64_t b0, uint32_t nb)
{
    __shared__ uint64_t s_red[4];
    const uint32_t tid = threadIdx.x, lb = blockIdx.x;
    const LzBlkDesc d = desc[b0 + lb];
    const bool lastwg = lb == nb - 1u;
    if (d.item == LZ_DESC_PAD) {                                       // (the whole workgroup; PAD blocks follow every real one)
        if (lastwg && tid == 0) carry[(seq + 1u) & 1u] = 0;
        return;
    }
    const uint64_t first = item_first[d.item];
    const uint32_t fl = first > b0 ? (uint32_t)(first - b0) : 0u;      // the item's first block in this batch
    uint64_t sum = 0;
    for (uint32_t j = fl + tid; j < lb; j += 256u) sum += block_bits[j] >> 3;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((tid & 63u) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    const uint64_t before = (first < b0 ? carry[seq & 1u] : 0ull) + s_red[0] + s_red[1] + s_red[2] + s_red[3];
    const uint32_t rec = (uint32_t)(block_bits[lb] >> 3);
    if (tid == 0) {
        if (d.last) item_total[d.item] = before + rec;
        if (lastwg) carry[(seq + 1u) & 1u] = d.last ? 0ull : before + rec;
    }
    // ---- the copy: slot bytes [0, rec) -> out[at, at + rec), nothing at or past the capacity
    uint8_t *out = reinterpret_cast<uint8_t *>(b.out[d.item]);
    const uint64_t cap = b.out_cap[d.item], at = (uint64_t)dfb_header_bytes(b, d.item, hb) + before;
    if (at >= cap) return;                                             // (the needed size goes on accumulating above)
    const uint32_t *S = slots + (size_t)lb * LZ_SLOT_WORDS;
    const uint8_t *Sb = reinterpret_cast<const uint8_t *>(S);
    uint32_t head = (4u - (uint32_t)((uintptr_t)(out + at) & 3u)) & 3u;           // bytes in front of the first aligned dword
    if (head > rec) head = rec;
    if (tid < head && at + tid < cap) out[at + tid] = Sb[tid];
    const uint32_t nd = (rec - head) >> 2;
    for (uint32_t j = tid; j < nd; j += 256u) {
        // destination dword j holds slot bytes [head + 4 j, head + 4 j + 4): two slot words, shifted (S[j + 1] is inside the slot)
        const uint32_t w = head ? (uint32_t)((((uint64_t)S[j + 1] << 32) | S[j]) >> (8u * head)) : S[j];
        const uint64_t p = at + head + 4ull * j;
        if (p + 4u <= cap) *reinterpret_cast<uint32_t *>(out + p) = w;
        else for (uint32_t k = 0; k < 4u; ++k) if (p + k < cap) out[p + k] = (uint8_t)(w >> (8u * k));
    }
    const uint32_t t0 = head + 4u * nd;
    if (t0 + tid < rec && at + t0 + tid < cap) out[at + t0 + tid] = Sb[t0 + tid];     // (at most three bytes)
}

__constant__ uint8_t kDfbLz4Frame[7] = {0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82};   // version 1, independent blocks, no checksums, no content
                                                                                     // size, 64 KiB maximum; HC = byte 1 of XXH32(60 40)
__constant__ uint8_t kDfbGzip[10] = {0x1F, 0x8B, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0xFF};    // as k_defz_finish writes it

__global__ __launch_bounds__(64)
void k_dfb_finish(DfbCall b, uint32_t block, const uint32_t *__restrict__ item_first, const uint32_t *__restrict__ item_st,
                  const uint64_t *__restrict__ item_total, const uint32_t *__restrict__ ck, const uint32_t *__restrict__ dictid)
{
    const uint32_t lane = threadIdx.x, i = blockIdx.x;
    const uint32_t st0 = item_st[i];
    if (st0 != MI_OK) {
        if (lane == 0) { b.status[i] = st0; b.out_bytes[i] = 0; if (b.failed) atomicAdd(b.failed, 1u); }
        return;
    }
    const uint64_t nb = b.in_bytes[i];
    const uint32_t nblk = (uint32_t)dfb_nblk(nb, block, b.ulen), first = item_first[i];
    auto end_of = [&](uint32_t k) -> uint64_t { const uint64_t e = dfb_begin_of(k + 1u, block, b.ulen); return e < nb ? e : nb; };
    // ---- the item's checksum from its blocks' parts: a part moves to the end of the item by the bytes behind its block
    uint32_t check = 0;
    if (b.container == MI_CONTAINER_GZIP) {
        uint32_t c = 0;
        for (uint32_t k = lane; k < nblk; k += 64u) {
            const uint64_t end = end_of(k);
            c ^= crc_mulmod(ck[2u * (first + k)], crc_xpow8(nb - end));
        }
        for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o);
        check = crc_standard(c, nb);
    } else if (b.container == MI_CONTAINER_ZLIB) {
        uint64_t A = 0, S = 0;
        for (uint32_t k = lane; k < nblk; k += 64u) {
            const uint64_t end = end_of(k);
            const uint64_t a = ck[2u * (first + k)], s = ck[2u * (first + k) + 1u];
            A += a;
            S += (s + a * ((nb - end) % ADLER_MOD)) % ADLER_MOD;
        }
        for (int o = 32; o > 0; o >>= 1) { A += __shfl_xor(A, o); S += __shfl_xor(S, o); }
        check = adler_standard((uint32_t)(A % ADLER_MOD), (uint32_t)(S % ADLER_MOD), nb);
    }
    if (lane != 0) return;
    uint8_t *out = reinterpret_cast<uint8_t *>(b.out[i]);
    const uint64_t cap = b.out_cap[i];
    auto put = [&](uint64_t at, uint32_t v) { if (at < cap) out[at] = (uint8_t)v; };
    uint64_t r = 0;
    if (b.container == DFB_SNAPPY) {
        // the preamble and the records: no closing block, no trailer; an empty item is the single byte 00
        for (uint64_t v = nb;; v >>= 7) { put(r++, (uint32_t)(v & 0x7Fu) | (v > 0x7Fu ? 0x80u : 0u)); if (v <= 0x7Fu) break; }
        r += nblk ? item_total[i] : 0ull;
        const uint32_t st = r <= cap ? MI_OK : MI_ERR_CAPACITY;
        b.status[i] = st;
        b.out_bytes[i] = r;
        if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
        return;
    }
    if (b.container == DFB_LZ4_BLOCK || b.container == DFB_LZ4_FRAME) {
        // a raw block: its one record, or the closing token 00 alone for an empty item; a frame: header, the blocks' slots, EndMark
        const bool fr = b.container == DFB_LZ4_FRAME;
        if (fr) for (uint32_t k = 0; k < 7u; ++k) put(r++, kDfbLz4Frame[k]);
        r += nblk ? item_total[i] : 0ull;
        if (fr) for (uint32_t k = 0; k < 4u; ++k) put(r++, 0u);
        else if (!nblk) put(r++, 0u);
        const uint32_t st = r <= cap ? MI_OK : MI_ERR_CAPACITY;
        b.status[i] = st;
        b.out_bytes[i] = r;
        if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
        return;
    }
    if (b.container == MI_CONTAINER_ZLIB && b.ulen) {                 // FDICT, and DICTID: the Adler-32 of the whole dictionary
        const uint32_t id = *dictid;
        put(0, 0x78); put(1, 0xBB); r = 2;
        for (int k = 0; k < 4; ++k) put(r++, id >> (24 - 8 * k));
    } else if (b.container == MI_CONTAINER_ZLIB) { put(0, 0x78); put(1, 0x9C); r = 2; }
    else if (b.container == MI_CONTAINER_GZIP) { for (uint32_t k = 0; k < 10u; ++k) put(k, kDfbGzip[k]); r = 10; }
    r += nblk ? item_total[i] : 0ull;
    put(r++, 0x03); put(r++, 0x00);                                    // BFINAL = 1, fixed, end-of-block; padding
    if (b.container == MI_CONTAINER_ZLIB) {
        for (int k = 0; k < 4; ++k) put(r++, check >> (24 - 8 * k));
    } else if (b.container == MI_CONTAINER_GZIP) {
        for (int k = 0; k < 4; ++k) put(r++, check >> (8 * k));
        for (int k = 0; k < 4; ++k) put(r++, (uint32_t)nb >> (8 * k));
    }
    const uint32_t st = r <= cap ? MI_OK : MI_ERR_CAPACITY;
    b.status[i] = st;
    b.out_bytes[i] = r;
    if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
}

// in front of the pipeline, on `s`: the scan, the table, the per-block checksums.  *desc: what the pipeline takes as its input.
mi_status dfb_begin(mi_ctx *ctx, const DfbCall &b, uint32_t block, void *ws, hipStream_t s, const uint8_t **desc)
{
    const DfbWs w = dfb_carve(ws, b);
    MI_HIP(ctx, hipMemsetAsync(w.head, 0, DFB_HEAD, s));
    if (b.failed) MI_HIP(ctx, hipMemsetAsync(b.failed, 0, 4, s));
    uint32_t *nreal = reinterpret_cast<uint32_t *>(w.head);
    if (w.zck) {                                                        // DICTID, on the stream: k_dfb_finish writes it into every header
        const mi_status st = defz_checksum(ctx, false, b.dict, b.dict_bytes, w.zck, reinterpret_cast<uint32_t *>(w.head + DFB_DICTID_AT), s);
        if (st) return st;
    }
    mi_prof_scope pr(ctx, "k_dfb_table", s, 0);
    hipLaunchKernelGGL(k_dfb_scan, dim3(1), dim3(1024), 0, s, b, block, w.item_first, w.item_st, nreal);
    if (b.max_blocks) {
        hipLaunchKernelGGL(k_dfb_fill, dim3((unsigned)((b.max_blocks + 255u) / 256u)), dim3(256), 0, s, b, block, w.item_first, nreal,
                           w.head + 64, w.desc);
        if (b.container == MI_CONTAINER_GZIP) hipLaunchKernelGGL(k_dfb_cksum<true>, dim3((unsigned)b.max_blocks), dim3(ZCK_THREADS), 0, s, w.desc, w.ck, b.in);
        else if (b.container == MI_CONTAINER_ZLIB) hipLaunchKernelGGL(k_dfb_cksum<false>, dim3((unsigned)b.max_blocks), dim3(ZCK_THREADS), 0, s, w.desc, w.ck, b.in);
    }
    MI_HIP(ctx, hipGetLastError());
    *desc = reinterpret_cast<const uint8_t *>(w.desc);
    return MI_OK;
}

void dfb_launch_place(const DfbCall &b, void *ws, const uint32_t *slots, const uint64_t *block_bits, uint64_t b0, uint32_t nb,
                      uint64_t seq, hipStream_t s)
{
    const DfbWs w = dfb_carve(ws, b);
    hipLaunchKernelGGL(k_dfb_place, dim3(nb), dim3(256), 0, s, b, w.desc, w.item_first, w.item_total,
                       reinterpret_cast<uint64_t *>(w.head + 8), (uint32_t)(seq & 1u), dfb_header_uniform(b), slots, block_bits, b0, nb);
}

void dfb_launch_stage(const DfbCall &b, uint32_t block, void *ws, uint64_t b0, uint32_t nb, hipStream_t s)
{
    const DfbWs w = dfb_carve(ws, b);
    hipLaunchKernelGGL(k_dfb_stage, dim3(nb), dim3(256), 0, s, b, w.desc, b0);
}

mi_status dfb_end(mi_ctx *ctx, const DfbCall &b, uint32_t block, void *ws, hipStream_t s)
{
    const DfbWs w = dfb_carve(ws, b);
    mi_prof_scope pr(ctx, "k_dfb_finish", s, 0);
    hipLaunchKernelGGL(k_dfb_finish, dim3((unsigned)b.count), dim3(64), 0, s, b, block, w.item_first, w.item_st, w.item_total, w.ck,
                       reinterpret_cast<const uint32_t *>(w.head + DFB_DICTID_AT));
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

extern "C" uint64_t mi_deflate_batch_bound_bytes(uint64_t n_item, const mi_lz_params *p, uint32_t container)
{
    return mi_deflate_z_bound_bytes(n_item, p, container);
}

extern "C" uint64_t mi_deflate_batch_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p)
{
    const uint64_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK;
    return total_in_bytes / block + count;                             // sum of ceil(n_i / block) <= floor(sum n_i / block) + count
}

// with a dictionary of dict_bytes: the first block of an item is shorter by |U|, so an item has at most one block more, and its
// zlib header four bytes more
uint32_t dfb_ulen(uint64_t dict_bytes, uint32_t block)
{
    const uint64_t u = dict_bytes < 32768u ? dict_bytes : 32768u;
    return (uint32_t)(u < block / 2u ? u : block / 2u);
}

extern "C" uint64_t mi_deflate_batch_dict_bound_bytes(uint64_t n_item, const mi_lz_params *p, uint32_t container, uint64_t dict_bytes)
{
    const uint32_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK, ulen = dfb_ulen(dict_bytes, block);
    if (!ulen) return mi_deflate_z_bound_bytes(n_item, p, container);
    // the first block's record at its stored bound, the rest as one stream of whole blocks (which counts container and 03 00)
    const uint64_t h = dfb_first(n_item, block, ulen);
    return (h ? h + 5u * ((h + 65534u) / 65535u) + 5u : 0u) + mi_deflate_z_bound_bytes(n_item - h, p, container) +
           (container == MI_CONTAINER_ZLIB ? 4u : 0u);
}

extern "C" uint64_t mi_deflate_batch_dict_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p, uint64_t dict_bytes)
{
    const uint32_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK;
    return total_in_bytes / block + (dfb_ulen(dict_bytes, block) ? 2u : 1u) * count;
}

extern "C" mi_status mi_deflate_batch_dict_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                                               const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                                               void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                               uint32_t *d_status, uint32_t *d_failed, const uint8_t *d_dict, uint64_t dict_bytes, void *stream)
{
    if (!ctx) return MI_ERR_ARG;
    mi_status st = defz_check(p, container);
    if (st) return st;
    if (dict_bytes && (!d_dict || container == MI_CONTAINER_GZIP || dict_bytes > DFB_MAX_BYTES)) return MI_ERR_ARG;     // gzip has no FDICT
    if (count > DFB_MAX_BYTES || max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out || !d_out_cap || !d_out_bytes || !d_status) return MI_ERR_ARG;
    DfbCall b{container, count, max_blocks, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed};
    b.ulen = dfb_ulen(dict_bytes, p->block);
    if (b.ulen) { b.dict = d_dict; b.dict_bytes = dict_bytes; }
    return lz_encode_impl(ctx, p, nullptr, 0, nullptr, 0, nullptr, stream, LzCall{LZ_BATCH, container, nullptr, &b});
}

extern "C" mi_status mi_deflate_batch_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                                          const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                                          void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                          uint32_t *d_status, uint32_t *d_failed, void *stream)
{
    if (!ctx) return MI_ERR_ARG;
    mi_status st = defz_check(p, container);
    if (st) return st;
    if (count > DFB_MAX_BYTES || max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out || !d_out_cap || !d_out_bytes || !d_status) return MI_ERR_ARG;
    const DfbCall b{container, count, max_blocks, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed};
    return lz_encode_impl(ctx, p, nullptr, 0, nullptr, 0, nullptr, stream, LzCall{LZ_BATCH, container, nullptr, &b});
}
