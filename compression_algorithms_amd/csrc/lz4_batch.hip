// lz4_batch.hip — many independent LZ4 buffers decoded or encoded in one call, as raw blocks (lz4_Block_format.md: what
// LZ4_compress_default writes; Parquet LZ4_RAW, ORC, blosc, ClickHouse, RocksDB) or as frames (lz4_Frame_format.md: the `lz4`
// tool, Arrow IPC): every item at its own address, of its own size, into its own buffer of a given CAPACITY, with its own verdict
// and length written on the device.  The frame is snappy_batch.hip's — one wave per item, parallel across items only.
// include/mi_codec.h has the contract.
//
//   k_lz4_batch<RING, FRAME>  one wave per item.  Tokens, length chains, offsets and the frame's words come wave-uniform out of the
//                     register window (BitsLsb over WaveWords, lz_decode.h: an item may start at any byte address, and no dword
//                     outside those that cover [in, in + nb) is loaded); literals go from the input into the ring lane-parallel
//                     and matches through OutRing::copy, both at most L4_PIECE bytes per step so that OutRing::advance keeps its
//                     contract (an LZ4 match has no longest length).  Every bound is checked before the element stores: a
//                     malformed item is MI_ERR_CORRUPT, never a fault.  Neither format has to name its size, so a capacity works
//                     as in the batched inflate: the first element that does not fit flips the wave into COUNTING — nothing is
//                     stored from there on, the walk goes on with every check, and the item is MI_ERR_CAPACITY with the size it
//                     needs.  FRAME: the header (its HC byte checked: XXH32 of a descriptor of under 16 bytes, the short-input
//                     path alone), then blocks behind their size words — stored ones are literals — up to the EndMark; block and
//                     content checksums are skipped over, not verified.  One ring per item: linked blocks (B.Indep = 0) reach
//                     whatever the item has written; with B.Indep = 1 a match may not reach in front of its block.
//   k_lz4_batch_size<FRAME>   one thread per item: the same walk (lz4_sequences, lz4_frame_body) over plain loads with a sink that
//                     stores nothing; a frame that carries a content size answers from its header alone.
//
// LDS per wave: the ring only — 4 096 bytes, or 32 768 in a call of fewer than 1 024 items (lz_decode_ring_want).
#include "lz_common.h"
#include "lz_decode.h"
#include "internal.h"

#define L4_PIECE 512u                          // bytes per literal or match step: < OutRing<4096>::CH

struct Lz4Batch {
    const void *const *in; const uint64_t *in_bytes;
    void *const *out; const uint64_t *out_cap;
    uint64_t *out_bytes; uint32_t *status, *failed;
};

enum Lz4Walk : uint32_t { L4W_OK, L4W_BAD, L4W_BIG };   // well-formed; malformed; well-formed, but past the per-item limit

// ---- the two readers: byte(), u16(), u32() take the next bytes (the caller has checked that they exist); skip(ip_new, k) moves
// k >= 1 bytes on to position ip_new of the item
struct Lz4WaveReader {
    BitsLsb br; const uint8_t *in; uint64_t nb; uint32_t lane;
    __device__ __forceinline__ uint32_t byte() { br.refill(); const uint32_t c = br.peek(8); br.skip(8); return c; }
    __device__ __forceinline__ uint32_t u16() { br.refill(); const uint32_t c = br.peek(16); br.skip(16); return c; }
    __device__ __forceinline__ uint32_t u32() { br.refill(); const uint32_t c = (uint32_t)br.buf; br.skip(32); return c; }   // (more than 32 bits held)
    __device__ __forceinline__ void skip(uint32_t ip_new, uint32_t k) { if (ip_new < nb) bits_seek_bytes(br, in, nb, ip_new, k, lane); }
    // byte k of the item's first 24 (a frame header), before anything is consumed: its dwords are in the first register window
    __device__ __forceinline__ uint32_t head(uint32_t k)
    {
        const uint32_t a = (uint32_t)((uintptr_t)in & 3u) + k;
        return (br.w.get(a >> 2) >> (8u * (a & 3u))) & 0xFFu;
    }
};
struct Lz4ByteReader {
    const uint8_t *in; uint32_t p;
    __device__ __forceinline__ uint32_t byte() { return in[p++]; }
    __device__ __forceinline__ uint32_t u16() { const uint32_t c = in[p] | ((uint32_t)in[p + 1] << 8); p += 2; return c; }
    __device__ __forceinline__ uint32_t u32() { const uint32_t c = u16(); return c | (u16() << 16); }
    __device__ __forceinline__ void skip(uint32_t ip_new, uint32_t) { p = ip_new; }
};

// ---- the two sinks: an element is stored whole or not at all
struct Lz4Count {
    __device__ __forceinline__ void literals(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void match(uint32_t, uint32_t, uint32_t) {}
};
template <uint32_t RING>
struct Lz4Store {
    OutRing<RING> ring; uint8_t *s_ring; const uint8_t *in; uint64_t cap; uint32_t lane; bool counting;
    // item bytes [ip, ip + len) -> positions [o, o + len)
    __device__ __forceinline__ void literals(uint32_t ip, uint32_t len, uint32_t o)
    {
        if (!counting && len > cap - o) counting = true;               // (o <= cap while storing)
        if (counting) return;
        const uint8_t *src = in + ip;
        for (uint32_t done = 0; done < len;) {
            const uint32_t piece = len - done < L4_PIECE ? len - done : L4_PIECE;
            uint8_t v[L4_PIECE / 64u];
#pragma unroll
            for (uint32_t q = 0; q < L4_PIECE / 64u; ++q) { const uint32_t j = q * 64u + lane; v[q] = j < piece ? src[done + j] : (uint8_t)0; }
#pragma unroll
            for (uint32_t q = 0; q < L4_PIECE / 64u; ++q) { const uint32_t j = q * 64u + lane; if (j < piece) s_ring[(o + j) & OutRing<RING>::RM] = v[q]; }
            done += piece; o += piece;
            __builtin_amdgcn_wave_barrier();
            ring.advance(o);
        }
    }
    // 1 <= d <= o: a piece of a match is a match of the same distance
    __device__ __forceinline__ void match(uint32_t d, uint32_t len, uint32_t o)
    {
        if (!counting && len > cap - o) counting = true;
        if (counting) return;
        while (len) {
            const uint32_t piece = len < L4_PIECE ? len : L4_PIECE;
            ring.copy(o, d, piece);
            o += piece; len -= piece;
            __builtin_amdgcn_wave_barrier();
            ring.advance(o);
        }
    }
};

// a length nibble of 15 goes on in bytes of 255 and one below 255, all inside [ip, bend); 64 bits hold any chain an item has room for
template <class R>
__device__ __forceinline__ bool lz4_chain(R &r, uint32_t &ip, uint32_t bend, uint64_t &v)
{
    uint32_t c;
    do {
        if (ip >= bend) return false;
        c = r.byte(); ++ip;
        v += c;
    } while (c == 255u);
    return true;
}

// The sequences of one block, item bytes [ip, bend) (bend > ip is the caller's rule: a block of 0 bytes has no last sequence): token,
// literal-length chain, literals, and — unless the literals end the block — offset, match-length chain.  o: the output position, moved
// on; floor: the first position a match may reach; limit >= o: where the output must end at the latest, `over` the verdict past it.
template <class R, class S>
__device__ __forceinline__ Lz4Walk lz4_sequences(R &r, S &sink, uint32_t &ip, uint32_t bend, uint32_t &o, uint32_t floor, uint32_t limit, Lz4Walk over)
{
    for (;;) {
        if (ip >= bend) return L4W_BAD;                                // the block ends behind a match: no closing literals
        const uint32_t tok = r.byte(); ++ip;
        uint64_t ll = tok >> 4;
        if (ll == 15u && !lz4_chain(r, ip, bend, ll)) return L4W_BAD;
        if (ll > bend - ip) return L4W_BAD;
        if (ll > limit - o) return over;
        if (ll) {
            sink.literals(ip, (uint32_t)ll, o);
            o += (uint32_t)ll; ip += (uint32_t)ll;
            r.skip(ip, (uint32_t)ll);
        }
        if (ip == bend) return L4W_OK;                                 // the closing sequence: literals only (its match nibble is not looked at)
        if (bend - ip < 2u) return L4W_BAD;
        const uint32_t d = r.u16(); ip += 2u;
        uint64_t ml = tok & 15u;
        if (ml == 15u && !lz4_chain(r, ip, bend, ml)) return L4W_BAD;
        ml += 4u;
        if (d == 0u || d > o - floor) return L4W_BAD;
        if (ml > limit - o) return over;
        sink.match(d, (uint32_t)ml, o);
        o += (uint32_t)ml;
    }
}

// ---- the frame
#define L4F_MAGIC     0x184D2204u
#define L4F_SKIPPABLE 0x184D2A50u              // .. 0x184D2A5F
#define L4F_LEGACY    0x184C2102u
#define XXH_P1 2654435761u
#define XXH_P2 2246822519u
#define XXH_P3 3266489917u
#define XXH_P4 668265263u
#define XXH_P5 374761393u
__device__ __forceinline__ uint32_t xxh_rotl(uint32_t v, uint32_t k) { return (v << k) | (v >> (32u - k)); }

struct Lz4Frame { uint32_t hb, bmax; uint64_t csize; bool indep, bcheck, ccheck, has_csize; };

// The header of an item of nb >= 1 bytes, byte(k) its byte k < nb: magic, FLG, BD, the optional content size and DictID, HC.  HC is
// byte 1 of XXH32(descriptor, seed 0); a descriptor is 2, 6, 10 or 14 bytes, so the hash is XXH32's path for inputs below 16 bytes:
// whole little-endian words, then single bytes, then the avalanche.  -> MI_OK with *f, MI_ERR_CORRUPT (cut short, a wrong magic,
// version, reserved bit, block maximum or HC), MI_ERR_ARG (well-formed, unsupported: a skippable or legacy frame, a DictID, a content
// size above the per-item limit).
template <class Byte>
__device__ __forceinline__ uint32_t lz4_frame_header(uint64_t nb, Byte byte, Lz4Frame *f)
{
    if (nb < 4u) return MI_ERR_CORRUPT;
    const uint32_t magic = byte(0) | (byte(1) << 8) | (byte(2) << 16) | (byte(3) << 24);
    if (magic != L4F_MAGIC) return ((magic & 0xFFFFFFF0u) == L4F_SKIPPABLE || magic == L4F_LEGACY) ? MI_ERR_ARG : MI_ERR_CORRUPT;
    if (nb < 7u) return MI_ERR_CORRUPT;
    const uint32_t flg = byte(4), bd = byte(5);
    if ((flg >> 6) != 1u || (flg & 2u) || (bd & 0x8Fu) || (bd >> 4) < 4u) return MI_ERR_CORRUPT;
    const bool has_csize = (flg & 8u) != 0, dict = (flg & 1u) != 0;
    const uint32_t dl = 2u + (has_csize ? 8u : 0u) + (dict ? 4u : 0u);
    if (4u + dl + 1u > nb) return MI_ERR_CORRUPT;
    uint32_t h = XXH_P5 + dl, acc = 0;
    uint64_t cs = 0;
    for (uint32_t j = 0; j < dl; ++j) {
        const uint32_t c = byte(4u + j);
        if (has_csize && j >= 2u && j < 10u) cs |= (uint64_t)c << (8u * (j - 2u));
        if (j < (dl & ~3u)) {
            acc |= c << (8u * (j & 3u));
            if ((j & 3u) == 3u) { h += acc * XXH_P3; h = xxh_rotl(h, 17) * XXH_P4; acc = 0; }
        } else { h += c * XXH_P5; h = xxh_rotl(h, 11) * XXH_P1; }
    }
    h ^= h >> 15; h *= XXH_P2; h ^= h >> 13; h *= XXH_P3; h ^= h >> 16;
    if (((h >> 8) & 0xFFu) != byte(4u + dl)) return MI_ERR_CORRUPT;
    if (dict || cs > INFB_MAX_BYTES) return MI_ERR_ARG;
    f->hb = 4u + dl + 1u; f->bmax = 1u << (8u + 2u * (bd >> 4));       // 64 KiB, 256 KiB, 1 MiB, 4 MiB
    f->csize = cs; f->has_csize = has_csize;
    f->indep = (flg & 32u) != 0; f->bcheck = (flg & 16u) != 0; f->ccheck = (flg & 4u) != 0;
    return MI_OK;
}

// The blocks behind the header, item bytes [ip, end): a size word each (top bit: stored; 0: the EndMark), 1 to bmax
// bytes of data giving at most bmax bytes of output; a block checksum and the content checksum are stepped over; nothing may
// follow; a content size must be what came out.
template <class R, class S>
__device__ __forceinline__ Lz4Walk lz4_frame_body(R &r, S &sink, const Lz4Frame &f, uint32_t ip, uint32_t end, uint32_t &o)
{
    for (;;) {
        if (end - ip < 4u) return L4W_BAD;
        const uint32_t w = r.u32(); ip += 4u;
        if (w == 0u) break;
        const uint32_t bs = w & 0x7FFFFFFFu;
        if (bs == 0u || bs > f.bmax || bs > end - ip) return L4W_BAD;  // (80 00 00 00 is neither the EndMark nor a block)
        const uint64_t room = (uint64_t)o + f.bmax;
        const uint32_t limit = room > INFB_MAX_BYTES ? (uint32_t)INFB_MAX_BYTES : (uint32_t)room;
        const Lz4Walk over = room > INFB_MAX_BYTES ? L4W_BIG : L4W_BAD;
        if (w >> 31) {
            if (bs > limit - o) return over;
            sink.literals(ip, bs, o);
            o += bs; ip += bs;
            r.skip(ip, bs);
        } else {
            const Lz4Walk st = lz4_sequences(r, sink, ip, ip + bs, o, f.indep ? o : 0u, limit, over);
            if (st != L4W_OK) return st;
        }
        if (f.bcheck) { if (end - ip < 4u) return L4W_BAD; ip += 4u; r.skip(ip, 4u); }
    }
    if (f.ccheck) { if (end - ip < 4u) return L4W_BAD; ip += 4u; }
    if (ip != end) return L4W_BAD;
    if (f.has_csize && f.csize != o) return L4W_BAD;
    return L4W_OK;
}

template <uint32_t RING, bool FRAME>
__global__ __launch_bounds__(64)
void k_lz4_batch(Lz4Batch b)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[RING];
    static_assert(L4_PIECE <= OutRing<RING>::CH, "a step adds at most one quarter of the ring");
    const uint32_t lane = threadIdx.x, item = blockIdx.x;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(b.in[item]);
    const uint64_t nb = b.in_bytes[item];
    uint8_t *out = reinterpret_cast<uint8_t *>(b.out[item]);
    const uint64_t cap = b.out_cap[item];
    uint32_t st = MI_OK;
    uint64_t size = 0;
    if ((nb && !in) || (cap && !out) || nb > INFB_MAX_BYTES || cap > INFB_MAX_BYTES) st = MI_ERR_ARG;
    else if (nb == 0) st = MI_ERR_CORRUPT;                             // (a block has its closing token at least, a frame its header)
    else {
        Lz4WaveReader r;
        r.in = in; r.nb = nb; r.lane = lane;
        r.br.init(in, 0, 8ull * nb, lane);
        Lz4Frame f;
        if constexpr (FRAME) st = lz4_frame_header(nb, [&](uint32_t k) -> uint32_t { return r.head(k); }, &f);
        if (st == MI_OK) {
            Lz4Store<RING> sink;
            sink.ring.init(s_ring, out, lane);
            sink.s_ring = s_ring; sink.in = in; sink.cap = cap; sink.lane = lane; sink.counting = false;
            const uint32_t end = (uint32_t)nb;
            uint32_t o = 0, ip = 0;
            Lz4Walk w;
            if constexpr (FRAME) { r.skip(f.hb, f.hb); w = lz4_frame_body(r, sink, f, f.hb, end, o); }   // (hb < nb, or the body is cut short at once)
            else w = lz4_sequences(r, sink, ip, end, o, 0u, (uint32_t)INFB_MAX_BYTES, L4W_BIG);
            if (w != L4W_OK) st = w == L4W_BIG ? MI_ERR_ARG : MI_ERR_CORRUPT;
            else if (sink.counting) { st = MI_ERR_CAPACITY; size = o; }
            else { size = o; sink.ring.finish(o); }
        }
    }
    if (lane == 0) {
        b.status[item] = st;
        b.out_bytes[item] = size;
        if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
    }
}

template <bool FRAME>
__global__ __launch_bounds__(256)
void k_lz4_batch_size(Lz4Batch b, uint32_t count)
{
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= count) return;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(b.in[item]);
    const uint64_t nb = b.in_bytes[item];
    uint32_t st = MI_OK;
    uint64_t size = 0;
    if ((nb && !in) || nb > INFB_MAX_BYTES) st = MI_ERR_ARG;
    else if (nb == 0) st = MI_ERR_CORRUPT;
    else {
        Lz4Frame f;
        if constexpr (FRAME) st = lz4_frame_header(nb, [&](uint32_t k) -> uint32_t { return in[k]; }, &f);
        if (st == MI_OK && FRAME && f.has_csize) size = f.csize;       // the header alone: the body is not looked at
        else if (st == MI_OK) {
            Lz4ByteReader r{in, FRAME ? f.hb : 0u};
            Lz4Count sink;
            uint32_t o = 0, ip = 0;
            Lz4Walk w;
            if constexpr (FRAME) w = lz4_frame_body(r, sink, f, f.hb, (uint32_t)nb, o);
            else w = lz4_sequences(r, sink, ip, (uint32_t)nb, o, 0u, (uint32_t)INFB_MAX_BYTES, L4W_BIG);
            if (w != L4W_OK) st = w == L4W_BIG ? MI_ERR_ARG : MI_ERR_CORRUPT;
            else size = o;
        }
    }
    b.status[item] = st;
    b.out_bytes[item] = size;
    if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
}

// ---------------------------------------------------------------------------------------------------------------------
// The encoder: LZ_LZ4, a form of the one pipeline (lz_emit.hip), as LZ_SNAPPY is.  Finder and parse are mode Z's (k_lz_parse_emit
// leaves one u32 record per token: bit 31 match, L in bits 16..30, d in the low 16); this is the last stage.  Records are whole
// bytes, and the batch's placement (deflate_batch.hip) puts them behind each item's header (none, or the frame's seven bytes).
//
// The emission rule, over a block of n bytes and its tokens after mode Z's clip of a last match that runs past the block:
//   a literal joins the pending run;
//   a match (L, d) at position p joins it too when p + 12 > n, or when L = min(L, n - 5 - p) leaves L < 4 — the format's end rules
//   (the last match starts at least 12 bytes before the end, the last 5 bytes are literals), which stock decoders enforce; what a
//   shortened match no longer covers begins the next run;
//   any other match flushes the run and itself as ONE sequence: token, literal-length chain, literals, offset, match-length chain;
//   the run pending at the block's end is the closing sequence, literals only (a block below 13 bytes is nothing else).
//
//   k_lz4_emit<FRAME>  k_snappy_emit's shape: one workgroup per block; thread t owns the tokens [t C, (t + 1) C), C = ceil(ntok / 256),
//                   and walks them four times, a workgroup scan between two walks:
//                     1. input bytes covered -> where the thread's tokens start
//                     2. the end of its last match written -> (max scan) where the run pending at its first token began
//                     3. bytes of the sequences it owns — a sequence belongs to its match, the closing one to thread 255 ->
//                        (sum scan) where they go, and the record's size
//                     4. the stores: tokens, chains, offsets, and the bytes of runs up to L4E_INLINE; a longer run goes on a list
//                        in LDS that the whole workgroup copies afterwards, a wave per run
//                   FRAME: the record lies behind its 4-byte size word in the slot; a record that would not be shorter than the
//                   block is not written — the block goes in stored (n | 0x80000000, then its bytes).
//                   block_bits[lb] = 8 x the slot's bytes.  A record is at most n + n / 255 + 2 bytes (mi_lz4_batch_bound_bytes), a
//                   frame's slot 4 + n: both far inside the 4 LZ_SLOT_WORDS bytes of a slot (131 136 for n <= 65 536).  A PAD block
//                   (one zero byte) comes out as 10 00 (FRAME: stored) and is placed nowhere.
// ---------------------------------------------------------------------------------------------------------------------
#define L4E_THREADS 256
#define L4E_INLINE  16u                        // a run up to this long is copied by the thread that writes its token
// longer runs per block: each but the last is followed by a match of 4 or more, so together they cover more than L4E_INLINE + 4 bytes
#define L4E_RUNS    (LZ_MAX_BLOCK / (L4E_INLINE + 1u + 4u) + 2u)
static_assert(4u + LZ_MAX_BLOCK + LZ_MAX_BLOCK / 255u + 16u <= 4u * LZ_SLOT_WORDS, "an LZ4 record fits its slot");

struct OpMaxU32L4 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };

// bytes of the chain behind a length nibble of value v (a literal count, or a match length - 4)
__device__ __forceinline__ uint32_t l4_chain_bytes(uint32_t v) { return v < 15u ? 0u : (v - 15u) / 255u + 1u; }
__device__ __forceinline__ uint32_t l4_put_chain(uint8_t *o, uint32_t v)
{
    if (v < 15u) return 0u;
    uint32_t k = 0;
    for (v -= 15u; v >= 255u; v -= 255u) o[k++] = 255u;
    o[k++] = (uint8_t)v;
    return k;
}

template <bool FRAME>
__global__ __launch_bounds__(L4E_THREADS)
void k_lz4_emit(const uint32_t *__restrict__ trec_all, uint32_t *__restrict__ slots, uint64_t *__restrict__ block_bits,
                const uint8_t *__restrict__ in, uint32_t block, uint64_t block0)
{
    __shared__ uint32_t s_tmp[L4E_THREADS / 64 + 2];
    __shared__ uint32_t s_run[L4E_RUNS], s_dst[L4E_RUNS];              // run: first byte | (length - 1) << 16
    __shared__ uint32_t s_nrun;
    const uint32_t tid = threadIdx.x, lb = blockIdx.x;
    const uint8_t *src; uint32_t n;
    lz_block_src<true>(in, 0, block, block0, lb, src, n);
    const uint32_t ntok = (uint32_t)block_bits[lb];                    // k_lz_parse_emit left the token count here (>= 1)
    const uint32_t *trec = trec_all + (size_t)lb * LZ_MAX_BLOCK;
    uint8_t *slot = reinterpret_cast<uint8_t *>(slots + (size_t)lb * LZ_SLOT_WORDS), *out = slot + (FRAME ? 4u : 0u);
    const uint32_t per = (ntok + L4E_THREADS - 1u) / L4E_THREADS;
    const uint32_t t0 = tid * per < ntok ? tid * per : ntok, t1 = t0 + per < ntok ? t0 + per : ntok;
    if (tid == 0) s_nrun = 0;
    // ---- 1: where the thread's tokens start (only the block's last token may cover bytes past n: nothing starts behind it)
    uint32_t cov = 0;
    for (uint32_t t = t0; t < t1; ++t) { const uint32_t r = trec[t]; cov += (r >> 31) ? (r >> 16) & 0x7FFFu : 1u; }
    uint32_t total;
    const uint32_t p0 = block_exclusive_scan<uint32_t>(cov, OpAddU32(), 0u, s_tmp, &total);
    // token r at position p -> the bytes it covers after the clip; *m != 0: it is written as a match of *m bytes at distance *d
    auto token = [&](uint32_t r, uint32_t p, uint32_t *m, uint32_t *d) -> uint32_t {
        *m = 0; *d = 0;
        if (!(r >> 31)) return 1u;
        const uint32_t L = (r >> 16) & 0x7FFFu, Lc = L < n - p ? L : n - p;
        if (p + 12u <= n) {
            const uint32_t Lm = Lc < n - 5u - p ? Lc : n - 5u - p;
            if (Lm >= 4u) { *m = Lm; *d = r & 0xFFFFu; }
        }
        return Lc;
    };
    // ---- 2: where the run pending at the thread's first token began: behind the last match written in front of it
    uint32_t last_end = 0;
    for (uint32_t t = t0, p = p0; t < t1; ++t) { uint32_t m, d; const uint32_t c = token(trec[t], p, &m, &d); if (m) last_end = p + m; p += c; }
    uint32_t tail_from;                                                // where the block's closing run begins
    const uint32_t rs0 = block_exclusive_scan<uint32_t>(last_end, OpMaxU32L4(), 0u, s_tmp, &tail_from);
    // ---- 3: the bytes of the sequences the thread owns
    uint32_t bytes = 0;
    for (uint32_t t = t0, p = p0, rs = rs0; t < t1; ++t) {
        uint32_t m, d;
        const uint32_t c = token(trec[t], p, &m, &d);
        if (m) { bytes += 1u + l4_chain_bytes(p - rs) + (p - rs) + 2u + l4_chain_bytes(m - 4u); rs = p + m; }
        p += c;
    }
    if (tid == L4E_THREADS - 1u) bytes += 1u + l4_chain_bytes(n - tail_from) + (n - tail_from);
    uint32_t rec;
    uint32_t o = block_exclusive_scan<uint32_t>(bytes, OpAddU32(), 0u, s_tmp, &rec);
    if (FRAME && rec >= n) {                                           // (the whole workgroup) stored
        for (uint32_t j = tid; j < n; j += L4E_THREADS) out[j] = src[j];
        if (tid == 0) { *reinterpret_cast<uint32_t *>(slot) = n | 0x80000000u; block_bits[lb] = 8ull * (4u + n); }
        return;
    }
    // ---- 4: the stores.  A run's bytes are contiguous input: [rs, rs + r) -> out[at, at + r)
    auto sequence = [&](uint32_t rs, uint32_t r, uint32_t m, uint32_t d) {
        const uint32_t mv = m ? m - 4u : 0u;
        out[o++] = (uint8_t)(((r < 15u ? r : 15u) << 4) | (mv < 15u ? mv : 15u));
        o += l4_put_chain(out + o, r);
        uint32_t k = L4E_RUNS;
        if (r > L4E_INLINE) k = atomicAdd(&s_nrun, 1u);
        if (k < L4E_RUNS) { s_run[k] = rs | ((r - 1u) << 16); s_dst[k] = o; }
        else for (uint32_t j = 0; j < r; ++j) out[o + j] = src[rs + j];
        o += r;
        if (m) { out[o++] = (uint8_t)d; out[o++] = (uint8_t)(d >> 8); o += l4_put_chain(out + o, mv); }
    };
    {
        uint32_t rs = rs0;
        for (uint32_t t = t0, p = p0; t < t1; ++t) {
            uint32_t m, d;
            const uint32_t c = token(trec[t], p, &m, &d);
            if (m) { sequence(rs, p - rs, m, d); rs = p + m; }
            p += c;
        }
        if (tid == L4E_THREADS - 1u) sequence(tail_from, n - tail_from, 0u, 0u);
    }
    __syncthreads();
    const uint32_t nrun = s_nrun < L4E_RUNS ? s_nrun : L4E_RUNS;
    for (uint32_t k = tid >> 6; k < nrun; k += L4E_THREADS / 64u) {
        const uint32_t rs = s_run[k] & 0xFFFFu, r = (s_run[k] >> 16) + 1u, at = s_dst[k];
        for (uint32_t j = tid & 63u; j < r; j += 64u) out[at + j] = src[rs + j];
    }
    if (tid == 0) {
        if (FRAME) *reinterpret_cast<uint32_t *>(slot) = rec;
        block_bits[lb] = 8ull * (rec + (FRAME ? 4u : 0u));
    }
}

void lz4_launch_emit(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, const uint8_t *d_desc, uint32_t block,
                     uint64_t b0, uint32_t nb, bool frame, hipStream_t s)
{
    if (frame) hipLaunchKernelGGL(k_lz4_emit<true>, dim3(nb), dim3(L4E_THREADS), 0, s, trec, slots, block_bits, d_desc, block, b0);
    else hipLaunchKernelGGL(k_lz4_emit<false>, dim3(nb), dim3(L4E_THREADS), 0, s, trec, slots, block_bits, d_desc, block, b0);
}

// A block of n bytes.  A sequence with a match — token, chain, r literals, offset, chain — takes 3 bytes for a match of 4 to 18 and
// 4 for a longer one (a match here is at most 258 bytes: one chain byte), so at least one byte less than the match covers; its
// literal chain is 0 bytes below 15 literals and (r - 15) / 255 + 1 from there on, so the sequence is at most r / 255 bytes longer
// than the input it covers.  The closing sequence has no match to save on: 1 + 1 + r / 255 more than its r literals.  Together
// n + n / 255 + 2; the bound is LZ4_compressBound's n + n / 255 + 16.  An item in block format is one block (an empty one the
// byte 00).  A frame: the 7-byte header, the 4-byte EndMark, and per block a 4-byte size word and at most the block's own bytes,
// since a record that is not shorter goes in stored.
extern "C" uint64_t mi_lz4_batch_bound_bytes(uint64_t n_item, const mi_lz_params *p, uint32_t format)
{
    const uint64_t block = (p && p->block) ? p->block : LZ_MAX_BLOCK;
    if (format == MI_LZ4_FRAME) return 11u + n_item + 4u * ((n_item + block - 1u) / block);
    return n_item + n_item / 255u + 16u;
}

extern "C" uint64_t mi_lz4_batch_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p)
{
    return mi_deflate_batch_max_blocks(total_in_bytes, count, p);
}

extern "C" mi_status mi_lz4_encode_batch_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t format, uint64_t count,
                                             const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                                             void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                             uint32_t *d_status, uint32_t *d_failed, void *stream)
{
    if (!ctx || format > MI_LZ4_FRAME) return MI_ERR_ARG;
    mi_status st = defz_check(p, MI_CONTAINER_RAW);
    if (st) return st;
    if (count > DFB_MAX_BYTES || max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out || !d_out_cap || !d_out_bytes || !d_status) return MI_ERR_ARG;
    const uint32_t container = format == MI_LZ4_FRAME ? DFB_LZ4_FRAME : DFB_LZ4_BLOCK;
    const DfbCall b{container, count, max_blocks, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed};
    return lz_encode_impl(ctx, p, nullptr, 0, nullptr, 0, nullptr, stream, LzCall{LZ_LZ4, container, nullptr, &b});
}

extern "C" mi_status mi_lz4_decode_batch_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                             void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                             uint32_t *d_status, uint32_t *d_failed, uint32_t format, uint32_t flags, void *stream)
{
    if (!ctx || format > MI_LZ4_FRAME || flags || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out || !d_out_cap || !d_out_bytes || !d_status) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cnt = (uint32_t)count;
    if (d_failed) MI_HIP(ctx, hipMemsetAsync(d_failed, 0, 4, s));
    const Lz4Batch b{d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed};
    {
        mi_prof_scope pr(ctx, "k_lz4_batch", s, 0);
        // the ring: as the batched inflate — few items cannot fill the CUs anyway and get a 32 KiB ring
        const bool small = lz_decode_ring_want(cnt, 32768u, 4096u) <= 4096u, frame = format == MI_LZ4_FRAME;
        if (small && frame) hipLaunchKernelGGL((k_lz4_batch<4096u, true>), dim3(cnt), dim3(64), 0, s, b);
        else if (small) hipLaunchKernelGGL((k_lz4_batch<4096u, false>), dim3(cnt), dim3(64), 0, s, b);
        else if (frame) hipLaunchKernelGGL((k_lz4_batch<32768u, true>), dim3(cnt), dim3(64), 0, s, b);
        else hipLaunchKernelGGL((k_lz4_batch<32768u, false>), dim3(cnt), dim3(64), 0, s, b);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

extern "C" mi_status mi_lz4_batch_size_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                           uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, uint32_t format, void *stream)
{
    if (!ctx || format > MI_LZ4_FRAME || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out_bytes || !d_status) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cnt = (uint32_t)count;
    if (d_failed) MI_HIP(ctx, hipMemsetAsync(d_failed, 0, 4, s));
    const Lz4Batch b{d_in, d_in_bytes, nullptr, nullptr, d_out_bytes, d_status, d_failed};
    {
        mi_prof_scope pr(ctx, "k_lz4_batch_size", s, 0);
        if (format == MI_LZ4_FRAME) hipLaunchKernelGGL(k_lz4_batch_size<true>, dim3((cnt + 255u) / 256u), dim3(256), 0, s, b, cnt);
        else hipLaunchKernelGGL(k_lz4_batch_size<false>, dim3((cnt + 255u) / 256u), dim3(256), 0, s, b, cnt);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}
