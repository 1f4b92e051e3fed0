// bgzf.hip — BGZF (the blocked gzip of bgzip / htslib, SAM specification 4.1) in both directions: mode Z's records framed
// as independent gzip members of at most 64 KiB, and any BGZF stream indexed and inflated from nothing but its bytes.
// include/mi_codec.h has the contract.
//
// Write (inside the mode-Z pipeline of lz_emit.hip, between k_defz_encode and k_lz_scan_blocks):
//   k_bgzf_frame     one workgroup per block: the CRC-32 of the block's input bytes (crc_range, crc32.h), the record moved
//                    up by the 18 header bytes inside its slot, header with BSIZE, 03 00, CRC-32 and ISIZE around it; the
//                    slot then holds the whole member and the block's size is the member's, so k_lz_scan_blocks and
//                    k_lz_concat place members as they place records
//   k_bgzf_finish    one thread: the 28-byte EOF member and the total
// Read:
//   k_bgzf_spec      one wave per 128 KiB chunk of the stream: the first position in the chunk that looks like a member
//                    header and from which a walk of BSIZE hops reaches the chunk's end is the chunk's guessed entry
//                    (chunk 0 enters at 0); the walk leaves the chunk's exit, member count and sum of ISIZE
//   k_bgzf_verify    one wave: chunk c's true entry is chunk c - 1's exit.  64 guesses are compared per step; a chunk whose
//                    guess is wrong (a decoy header inside a stored block, say) is walked again from its true entry.  Then
//                    the exclusive scan of counts and ISIZE sums.  Exactly the serial walk from offset 0, whatever the bytes.
//   k_bgzf_list      one wave per chunk: the walk again from the verified entry, writing (stream offset, output offset)
//   k_bgzf_segments  one thread per member of the requested range: the header read again and checked against the
//                    (untrusted) table -> an InfSeg descriptor for k_inflate<.., DESC> (inflate.hip)
//   k_bgzf_check     one workgroup per member: CRC-32 of the decoded bytes against the member's trailer
#include "lz_common.h"
#include "crc32.h"
#include "internal.h"
#include "bgzf_core.h"                 // the member header and its check against a table, shared with bgzf_ranges.hip

// a member of the largest block in its stored form: header 18, record b + 5 ceil(b / 65535) + 5, 03 00, trailer 8
static_assert(MI_BGZF_MAX_BLOCK + 5u * ((MI_BGZF_MAX_BLOCK + 65534u) / 65535u) + 5u + 2u + 26u <= 65536u, "BSIZE fits 16 bits");
static_assert(MI_BGZF_MAX_BLOCK + 1u + 5u * ((MI_BGZF_MAX_BLOCK + 1u + 65534u) / 65535u) + 5u + 2u + 26u > 65536u, "and no larger block does");
static_assert(MI_BGZF_BLOCK <= MI_BGZF_MAX_BLOCK && 65536u / 4u + 8u < LZ_SLOT_WORDS, "a member fits its slot");

#define BGZF_HDR       18u                     // 1F 8B 08 04 MTIME(4) XFL OS XLEN(2) 'B' 'C' 02 00 BSIZE(2)
#define BGZF_FRAME     28u                     // header + 03 00 + CRC-32 + ISIZE
#define BGZF_CHUNK     131072ull               // index: stream bytes per wave; > 65 536, so every chunk but the last holds a member start
#define BGZF_TRIES     8u                      // guessed entries tried per chunk before it is left to the verify pass
#define BGZF_NONE      (~0ull)
#define BGZF_MAGIC     0x04088B1Fu             // 1F 8B 08 04 as a little-endian word: gzip, CM = 8, FLG = FEXTRA alone

__constant__ uint8_t kBgzfHead[16] = {0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xFF, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00};
__constant__ uint8_t kBgzfEof[28] = {0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xFF, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00,
                                     0x1B, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0};

// ---------------------------------------------------------------------------------------------
// write
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ZCK_THREADS)
void k_bgzf_frame(uint32_t *slots, uint64_t *__restrict__ block_bits, const uint8_t *__restrict__ in, uint64_t n_total,
                  uint32_t block, uint64_t block0)
{
    __shared__ CrcLds s_crc;
    const uint32_t tid = threadIdx.x, lb = blockIdx.x;
    const uint64_t off = (block0 + lb) * (uint64_t)block;
    const uint32_t n = (uint32_t)((n_total - off) < block ? (n_total - off) : block);
    crc_lds_init(s_crc, tid);
    __syncthreads();
    const uint32_t pure = crc_range(in + off, n, s_crc, tid);          // (thread 0)
    uint32_t *out = slots + (size_t)lb * LZ_SLOT_WORDS;
    const uint32_t R = (uint32_t)(block_bits[lb] >> 3);                 // the record's bytes (k_defz_encode)
    // the record moves up by 18 bytes = 4 words and 16 bits, the highest words first: a chunk is read whole, then written
    constexpr uint32_t PER = 4u, CH = PER * ZCK_THREADS;
    const uint32_t W = (BGZF_HDR + R + 3u) / 4u;                        // words [4, W) take record bytes
    for (int32_t c = (int32_t)((W - 4u + CH - 1u) / CH) - 1; c >= 0; --c) {
        const uint32_t base = 4u + (uint32_t)c * CH;
        uint32_t v[PER];
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            const uint32_t j = base + q * ZCK_THREADS + tid;
            v[q] = j < W ? (out[j - 4u] << 16) | (j >= 5u ? out[j - 5u] >> 16 : 0u) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            const uint32_t j = base + q * ZCK_THREADS + tid;
            if (j < W) out[j] = v[q];
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint8_t *m = reinterpret_cast<uint8_t *>(out);
        const uint32_t bsize = R + BGZF_FRAME - 1u;                     // (<= 65 535: the static_assert above)
        for (uint32_t i = 0; i < 16u; ++i) m[i] = kBgzfHead[i];
        m[16] = (uint8_t)bsize; m[17] = (uint8_t)(bsize >> 8);
        uint32_t t = BGZF_HDR + R;
        m[t++] = 0x03; m[t++] = 0x00;                                   // BFINAL = 1, fixed, end-of-block; padding
        const uint32_t crc = crc_standard(pure, n);
        for (uint32_t i = 0; i < 4u; ++i) m[t++] = (uint8_t)(crc >> (8u * i));
        for (uint32_t i = 0; i < 4u; ++i) m[t++] = (uint8_t)(n >> (8u * i));
        block_bits[lb] = 8ull * (R + BGZF_FRAME);
    }
}

void bgzf_launch_frame(uint32_t *slots, uint64_t *block_bits, const uint8_t *d_in, uint64_t n, uint32_t block, uint64_t b0,
                       uint32_t nb, hipStream_t s)
{
    hipLaunchKernelGGL(k_bgzf_frame, dim3(nb), dim3(ZCK_THREADS), 0, s, slots, block_bits, d_in, n, block, b0);
}

__global__ void k_bgzf_finish(uint8_t *__restrict__ out, const uint64_t *__restrict__ member_bits, uint64_t nblocks,
                              uint64_t *__restrict__ out_bytes)
{
    // (the bound leaves these 28 bytes behind the members: k_lz_concat, which writes whole words, has written all of theirs)
    uint64_t r = member_bits[nblocks] >> 3;
    for (uint32_t i = 0; i < 28u; ++i) out[r++] = kBgzfEof[i];
    *out_bytes = r;
}

mi_status bgzf_end(mi_ctx *ctx, uint8_t *d_out, const uint64_t *d_member_bits, uint64_t nblocks, uint64_t *d_out_bytes, hipStream_t s)
{
    hipLaunchKernelGGL(k_bgzf_finish, dim3(1), dim3(1), 0, s, d_out, d_member_bits, nblocks, d_out_bytes);
    return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_HIP;
}

extern "C" uint64_t mi_bgzf_bound_bytes(uint64_t n, const mi_lz_params *p)
{
    if (!p || p->block == 0u || p->block > MI_BGZF_MAX_BLOCK) return 0;
    const uint64_t block = p->block, nblocks = (n + block - 1) / block;
    const uint64_t last = n - (nblocks ? (nblocks - 1) * block : 0);
    auto member = [](uint64_t b) -> uint64_t { return b + 5 * ((b + 65534) / 65535) + 5 + 2 + 26; };
    return (nblocks ? (nblocks - 1) * member(block) + member(last) : 0) + 28;
}

// ---------------------------------------------------------------------------------------------
// read: the member header
// ---------------------------------------------------------------------------------------------
// (bgzf_parse, the member header as include/mi_codec.h reads it: bgzf_core.h)

// Members from `pos` while they start before `lim` (<= nbytes); false where one does not parse.  Every lane of the wave
// runs it with the same arguments.  put(k, stream offset, output bytes before it) sees every member.
template <typename F>
__device__ bool bgzf_walk(const uint8_t *__restrict__ s, uint64_t nbytes, uint64_t pos, uint64_t lim, uint64_t &exit_at,
                          uint64_t &count, uint64_t &isz, F &&put)
{
    count = 0; isz = 0;
    while (pos < lim) {                                                 // every round moves on by at least 28 bytes
        uint32_t msize, isize, xlen;
        if (!bgzf_parse(s, pos, nbytes, msize, isize, xlen)) return false;
        put(count, pos, isz);
        pos += msize; count += 1u; isz += isize;
    }
    exit_at = pos;
    return true;
}

// per chunk in the workspace
struct BgzfChunks { uint64_t *entry, *exit_at, *count, *isz, *idx0, *out0; };

__device__ __forceinline__ uint32_t bgzf_word(const uint8_t *__restrict__ s, uint64_t nbytes, uint64_t p)   // p 4-byte aligned
{
    if (p + 4u <= nbytes) return *reinterpret_cast<const uint32_t *>(s + p);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; ++k) if (p + k < nbytes) v |= (uint32_t)s[p + k] << (8u * k);
    return v;
}

__global__ __launch_bounds__(64)
void k_bgzf_spec(const uint8_t *__restrict__ s, uint64_t nbytes, BgzfChunks ck)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t c = blockIdx.x;
    const uint64_t lo = c * BGZF_CHUNK, hi = lo + BGZF_CHUNK < nbytes ? lo + BGZF_CHUNK : nbytes;
    uint64_t entry = BGZF_NONE, exit_at = BGZF_NONE, count = 0, isz = 0;
    auto none = [](uint64_t, uint64_t, uint64_t) {};
    if (c == 0) {
        if (bgzf_walk(s, nbytes, 0, hi, exit_at, count, isz, none)) entry = 0;
        else exit_at = BGZF_NONE;
    } else {
        uint32_t tries = 0;
        for (uint64_t base = lo; base < hi && entry == BGZF_NONE && tries < BGZF_TRIES; base += 256u) {
            const uint64_t p = base + 4u * lane;
            const uint32_t w = bgzf_word(s, nbytes, p);
            uint32_t nx = (uint32_t)__shfl_down((int)w, 1);
            if (lane == 63u) nx = bgzf_word(s, nbytes, p + 4u);
            const uint64_t v = (uint64_t)w | ((uint64_t)nx << 32);
            uint32_t m = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) if ((uint32_t)(v >> (8u * k)) == BGZF_MAGIC && p + k < hi) m |= 1u << k;
            uint64_t any = __ballot(m != 0u);
            while (any && entry == BGZF_NONE && tries < BGZF_TRIES) {
                const uint32_t L = (uint32_t)__ffsll((long long)any) - 1u;
                any &= any - 1u;
                const uint32_t mm = (uint32_t)__shfl((int)m, (int)L);
                for (uint32_t k = 0; k < 4u && entry == BGZF_NONE && tries < BGZF_TRIES; ++k) {
                    if (!((mm >> k) & 1u)) continue;
                    const uint64_t cand = base + 4u * L + k;
                    ++tries;
                    if (bgzf_walk(s, nbytes, cand, hi, exit_at, count, isz, none)) entry = cand;
                }
            }
        }
        if (entry == BGZF_NONE) { exit_at = BGZF_NONE; count = 0; isz = 0; }
    }
    if (lane == 0) { ck.entry[c] = entry; ck.exit_at[c] = exit_at; ck.count[c] = count; ck.isz[c] = isz; }
}

// (k_bgzf_verify reads what its own lane 0 wrote a moment ago: past the CU's L1, as OutRing::fetch does)
__device__ __forceinline__ uint64_t bgzf_ld(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64)
void k_bgzf_verify(const uint8_t *__restrict__ s, uint64_t nbytes, uint64_t nchunks, BgzfChunks ck, uint64_t *__restrict__ members,
                   uint64_t cap_members, uint64_t *__restrict__ d_count, uint32_t *__restrict__ err)
{
    const uint32_t lane = threadIdx.x;
    auto none = [](uint64_t, uint64_t, uint64_t) {};
    uint64_t cur = 0;                                                   // the true entry of chunk c0
    bool bad = false;
    for (uint64_t c0 = 0; c0 < nchunks && !bad;) {                      // every round settles at least one chunk
        const uint64_t c = c0 + lane;
        const bool in = c < nchunks;
        const uint64_t prev = lane == 0u ? cur : (in ? bgzf_ld(ck.exit_at + c - 1u) : BGZF_NONE);
        const uint64_t guess = in ? bgzf_ld(ck.entry + c) : BGZF_NONE;
        const bool ok = in && guess != BGZF_NONE && guess == prev;
        const uint64_t wrong = __ballot(in && !ok);
        const uint32_t b = wrong ? (uint32_t)__ffsll((long long)wrong) - 1u : 64u;
        const uint64_t left = nchunks - c0, upto = b < left ? b : (left < 64u ? left : 64u);   // chunks [c0, c0 + upto) hold
        if (upto) cur = bgzf_ld(ck.exit_at + c0 + upto - 1u);
        c0 += upto;
        if (!wrong) continue;
        // chunk c0 again, from its true entry (the last chunk may start behind the last member: nothing to walk)
        const uint64_t hi = (c0 + 1u) * BGZF_CHUNK < nbytes ? (c0 + 1u) * BGZF_CHUNK : nbytes;
        uint64_t exit_at = cur, count = 0, isz = 0;
        if (!bgzf_walk(s, nbytes, cur, hi, exit_at, count, isz, none)) { bad = true; break; }
        if (lane == 0u) { ck.entry[c0] = cur; ck.exit_at[c0] = exit_at; ck.count[c0] = count; ck.isz[c0] = isz; }
        __threadfence();
        cur = exit_at;
        c0 += 1u;
    }
    // the stream ends exactly where a member ends.  (An invariant, not a reachable refusal: the last chunk's walk goes on while
    // pos < nbytes and a member that parses ends at or before nbytes, so a walk that returns true there stops at nbytes;
    // trailing bytes and a cut member fail to parse and end in `bad` above.)
    if (!bad && cur != nbytes) bad = true;
    if (bad) { if (lane == 0u) { atomicOr(err, 1u); d_count[0] = 0; d_count[1] = 0; } return; }
    // exclusive scan of the member counts and the ISIZE sums, 64 chunks a round
    uint64_t n_run = 0, o_run = 0;
    for (uint64_t c0 = 0; c0 < nchunks; c0 += 64u) {
        const uint64_t c = c0 + lane;
        const uint64_t cn = c < nchunks ? bgzf_ld(ck.count + c) : 0u, co = c < nchunks ? bgzf_ld(ck.isz + c) : 0u;
        uint64_t in_n = cn, in_o = co;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t tn = __shfl_up(in_n, o), to = __shfl_up(in_o, o);
            if ((int)lane >= o) { in_n += tn; in_o += to; }
        }
        if (c < nchunks) { ck.idx0[c] = n_run + in_n - cn; ck.out0[c] = o_run + in_o - co; }
        n_run += __shfl(in_n, 63); o_run += __shfl(in_o, 63);
    }
    if (lane == 0u) {
        d_count[0] = n_run; d_count[1] = o_run;
        if (members && n_run <= cap_members) { members[2u * n_run] = nbytes; members[2u * n_run + 1u] = o_run; }
    }
}

__global__ __launch_bounds__(64)
void k_bgzf_list(const uint8_t *__restrict__ s, uint64_t nbytes, BgzfChunks ck, uint64_t *__restrict__ members, uint64_t cap_members,
                 const uint32_t *__restrict__ err)
{
    if (*err) return;                                                   // (k_bgzf_verify: the table below is whole only without it)
    const uint32_t lane = threadIdx.x;
    const uint64_t c = blockIdx.x;
    const uint64_t hi = (c + 1u) * BGZF_CHUNK < nbytes ? (c + 1u) * BGZF_CHUNK : nbytes;
    const uint64_t idx0 = ck.idx0[c], out0 = ck.out0[c];
    uint64_t exit_at, count, isz;
    bgzf_walk(s, nbytes, ck.entry[c], hi, exit_at, count, isz, [&](uint64_t k, uint64_t at, uint64_t before) {
        if (lane == 0u && idx0 + k < cap_members) { members[2u * (idx0 + k)] = at; members[2u * (idx0 + k) + 1u] = out0 + before; }
    });
}

extern "C" mi_status mi_bgzf_index_dev(mi_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, uint64_t *d_members,
                                       uint64_t cap_members, uint64_t *d_count, void *stream)
{
    if (!ctx || !d_count || (stream_bytes && !d_stream)) return MI_ERR_ARG;
    if (((uintptr_t)d_stream & 3u) || stream_bytes > (UINT64_MAX >> 4)) return MI_ERR_ARG;
    const uint64_t nchunks = (stream_bytes + BGZF_CHUNK - 1) / BGZF_CHUNK;
    if (nchunks > 0x7FFFFFFFull) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    BgzfChunks ck;
    const mi_status st = mi_ws_carve(ctx, [&](mi_carver &cv) {
        cv.take(ck.entry, nchunks); cv.take(ck.exit_at, nchunks); cv.take(ck.count, nchunks);
        cv.take(ck.isz, nchunks); cv.take(ck.idx0, nchunks); cv.take(ck.out0, nchunks);
    });
    if (st) return st;
    uint32_t *err = mi_err_slot(ctx, s);
    if (!err) return MI_ERR_HIP;
    {
        mi_prof_scope pr(ctx, "k_bgzf_index", s, stream_bytes);
        if (nchunks) hipLaunchKernelGGL(k_bgzf_spec, dim3((unsigned)nchunks), dim3(64), 0, s, d_stream, stream_bytes, ck);
        hipLaunchKernelGGL(k_bgzf_verify, dim3(1), dim3(64), 0, s, d_stream, stream_bytes, nchunks, ck, d_members, cap_members, d_count, err);
        if (nchunks && d_members) hipLaunchKernelGGL(k_bgzf_list, dim3((unsigned)nchunks), dim3(64), 0, s, d_stream, stream_bytes, ck, d_members, cap_members, err);
    }
    if (hipGetLastError() != hipSuccess) return MI_ERR_HIP;
    uint32_t h_err = 0; uint64_t h_count[2] = {0, 0};
    MI_HIP(ctx, hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipMemcpyAsync(h_count, d_count, 16, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    if (h_err) return MI_ERR_CORRUPT;
    return (d_members && h_count[0] > cap_members) ? MI_ERR_CAPACITY : MI_OK;
}

// ---------------------------------------------------------------------------------------------
// read: members -> segment descriptors -> k_inflate -> CRC-32 against the trailers
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_bgzf_segments(const uint8_t *__restrict__ s, uint64_t nbytes, const uint64_t *__restrict__ members, uint64_t first,
                     uint32_t nmem, uint64_t out_bytes, InfSeg *__restrict__ seg, uint32_t *__restrict__ err)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nmem) return;
    const uint64_t m = first + i;
    const uint64_t s0 = members[2u * m], o0 = members[2u * m + 1u], s1 = members[2u * m + 2u], o1 = members[2u * m + 3u];
    const uint64_t obase = members[2u * first + 1u];
    InfSeg d = {0, 0, 0, 0, 0};
    bool ok = o0 >= obase && o1 >= o0 && o1 - obase <= out_bytes;
    if (ok && i + 1u == nmem) ok = o1 - obase == out_bytes;            // the range fills the output exactly
    ok = ok && bgzf_member_seg(s, nbytes, s0, o0, s1, o1, d);          // (bgzf_core.h: the table's pairs and the header read again)
    if (ok) d.out_off = o0 - obase;
    else atomicOr(err, 1u);                                            // (d is still all zero)
    seg[i] = d;
}

// seg_status (bgzf_ranges.hip; NULL: the one `err` word): a segment whose word is not zero is not read at all, and a
// mismatch sets the segment's own word
__global__ __launch_bounds__(ZCK_THREADS)
void k_bgzf_check(const uint8_t *__restrict__ out, const InfSeg *__restrict__ seg, uint32_t *__restrict__ err, uint32_t *__restrict__ seg_status)
{
    __shared__ CrcLds s_crc;
    const uint32_t tid = threadIdx.x;
    if (seg_status && seg_status[blockIdx.x] != 0u) return;            // (the whole workgroup)
    const InfSeg d = seg[blockIdx.x];
    crc_lds_init(s_crc, tid);
    __syncthreads();
    const uint32_t pure = crc_range(out + d.out_off, d.out_len, s_crc, tid);
    if (tid == 0 && crc_standard(pure, d.out_len) != d.crc) {
        if (seg_status) seg_status[blockIdx.x] = 1u;
        else atomicOr(err, 1u);
    }
}

void bgzf_launch_check(const uint8_t *d_out, const InfSeg *d_seg, uint32_t nseg, uint32_t *err, hipStream_t s, uint32_t *seg_status)
{
    hipLaunchKernelGGL(k_bgzf_check, dim3(nseg), dim3(ZCK_THREADS), 0, s, d_out, d_seg, err, seg_status);
}

extern "C" mi_status mi_bgzf_inflate_dev(mi_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_members,
                                         uint64_t first_member, uint64_t n_members, uint8_t *d_out, uint64_t out_bytes,
                                         uint32_t flags, void *stream)
{
    if (!ctx || (stream_bytes && !d_stream) || !d_members || (out_bytes && !d_out)) return MI_ERR_ARG;
    if ((flags & ~MI_INFLATE_NO_CHECKSUM) || ((uintptr_t)d_stream & 3u) || stream_bytes > (UINT64_MAX >> 4)) return MI_ERR_ARG;
    if (n_members > 0x7FFFFFFFull || first_member > (UINT64_MAX >> 8)) return MI_ERR_ARG;
    if (n_members == 0) return out_bytes ? MI_ERR_ARG : MI_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nmem = (uint32_t)n_members;
    InfSeg *seg;
    const mi_status st = mi_ws_carve(ctx, [&](mi_carver &cv) { cv.take(seg, nmem); });
    if (st) return st;
    uint32_t *err = mi_err_slot(ctx, s);
    if (!err) return MI_ERR_HIP;
    hipLaunchKernelGGL(k_bgzf_segments, dim3((nmem + 255u) / 256u), dim3(256), 0, s, d_stream, stream_bytes, d_members, first_member,
                       nmem, out_bytes, seg, err);
    {
        mi_prof_scope pr(ctx, "k_inflate", s, out_bytes);
        inflate_launch_segments(d_stream, stream_bytes, seg, nmem, d_out, err, s);
    }
    if (!(flags & MI_INFLATE_NO_CHECKSUM)) {
        mi_prof_scope pr(ctx, "k_bgzf_check", s, out_bytes);
        bgzf_launch_check(d_out, seg, nmem, err, s);
    }
    if (hipGetLastError() != hipSuccess) return MI_ERR_HIP;
    uint32_t h_err = 0;
    MI_HIP(ctx, hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return h_err ? MI_ERR_CORRUPT : MI_OK;
}
