// inflate_batch.hip — many independent DEFLATE streams (raw, zlib or gzip, one container per call) inflated in one launch:
// every item at its own address, of its own size, into its own buffer of a given CAPACITY, with its own verdict and length
// written on the device.  Parallel across items only: inside an item one wave decodes serially.  include/mi_codec.h has the
// contract.
//
//   k_batch_hist / k_batch_scan / k_batch_scatter   an opt-in dispatch order (MI_INFLATE_BATCH_ORDER=1): items by size class
//                     (the position of the leading one of their compressed size), the largest class first, since workgroups
//                     start in blockIdx order; unmeasured, hence off by default
//   k_inflate_batch<RING, COUNT_ONLY>   one wave per item: header and trailer read by the wave itself (the rules of
//                     k_inflate_frame), then inf_blocks (inflate_core.h), k_inflate's block and token loop, with the output
//                     limit a capacity: past it the wave goes on COUNTING without storing.  COUNT_ONLY (the size pass) counts
//                     from the first byte and has no ring.
//   k_inflate_batch_check   one workgroup per item that came out MI_OK: CRC-32 (crc32.h) or Adler-32 (adler32.h) of the
//                     decoded bytes against the item's trailer
//
//   DICT (mi_inflate_batch_dict_*)   one preset dictionary for the call, zlib's FDICT: its last min(dict_bytes, 32 768) bytes E
//                     lie in front of every item that uses it (raw: every item; zlib: an item whose header has FDICT and whose
//                     DICTID is the Adler-32 of the whole dictionary, computed on the stream by the kernels of mi_adler32_dev).
//                     The wave preloads the last min(RING, |E|) bytes of E into the ring cells of positions -1, -2, ...; what
//                     lies farther back is read from the dictionary itself, as far matches read the output (lz_decode.h).
//                     A third template parameter: the instantiations without it are the code they were.
//
// LDS per wave: the tables of k_inflate (4 324 bytes) + the ring: 8 420 with the 4 KiB ring, 37 092 with the 32 KiB ring
// (fewer than 1 024 items), 4 324 without one.  DESIGN.md 3.5 has the resource lines.
#include "lz_common.h"
#include "lz_decode.h"
#include "inflate_core.h"
#include "crc32.h"
#include "adler32.h"
#include "internal.h"
#include <stdlib.h>

#define INFB_CLASSES   33u                     // size classes: 0 (empty), then 1 + the position of the leading one, capped
#define INFB_WS_HEAD   512u                    // bytes in front of `order`: u32 hist[64], cursor[64]

struct InfBatch {
    const void *const *in; const uint64_t *in_bytes;
    void *const *out; const uint64_t *out_cap;
    uint64_t *out_bytes; uint32_t *status, *failed;
    const uint32_t *order;                     // workgroup j takes item order[j]; NULL: item j
    uint32_t container;
};

// the call's preset dictionary as the DICT kernels see it; nothing where there is none
template <bool DICT> struct InfDict {};
template <> struct InfDict<true> {
    const uint8_t *end;                        // behind the dictionary's last byte
    uint32_t n;                                // |E| = min(dict_bytes, 32 768)
    const uint32_t *adler;                     // Adler-32 of the whole dictionary (zlib container; NULL for raw)
};

__device__ __forceinline__ uint32_t infb_class(uint64_t bytes)
{
    const uint32_t c = bytes ? 64u - (uint32_t)__clzll((long long)bytes) : 0u;
    return c < INFB_CLASSES ? c : INFB_CLASSES - 1u;
}

__global__ __launch_bounds__(256)
void k_batch_hist(const uint64_t *__restrict__ in_bytes, uint32_t count, uint32_t *__restrict__ hist)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) atomicAdd(&hist[infb_class(in_bytes[i])], 1u);
}

__global__ void k_batch_scan(const uint32_t *__restrict__ hist, uint32_t *__restrict__ cursor)
{
    uint32_t run = 0;
    for (int c = (int)INFB_CLASSES - 1; c >= 0; --c) { cursor[c] = run; run += hist[c]; }     // the largest class first
}

__global__ __launch_bounds__(256)
void k_batch_scatter(const uint64_t *__restrict__ in_bytes, uint32_t count, uint32_t *__restrict__ cursor, uint32_t *__restrict__ order)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) order[atomicAdd(&cursor[infb_class(in_bytes[i])], 1u)] = i;       // (< count: the cursors partition [0, count))
}

template <uint32_t RING, bool COUNT_ONLY, bool DICT = false>
__global__ __launch_bounds__(64)
void k_inflate_batch(InfBatch b, InfDict<DICT> dd)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[COUNT_ONLY ? 16u : RING];
    __shared__ uint16_t s_llut[1 << INF_LL_BITS], s_dlut[1 << INF_D_BITS];
    __shared__ InfCode<288> s_ll;
    __shared__ InfCode<32> s_dc;
    __shared__ __attribute__((aligned(4))) uint8_t s_len[288 + 32 + 4], s_cl[20];
    const uint32_t lane = threadIdx.x;
    const uint32_t item = b.order ? b.order[blockIdx.x] : blockIdx.x;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(b.in[item]);
    const uint64_t nb = b.in_bytes[item];
    uint8_t *out = COUNT_ONLY ? nullptr : reinterpret_cast<uint8_t *>(b.out[item]);
    const uint64_t cap = COUNT_ONLY ? 0ull : b.out_cap[item];
    uint32_t st = MI_OK;
    uint64_t size = 0;
    if ((nb && !in) || (cap && !out) || nb > INFB_MAX_BYTES || cap > INFB_MAX_BYTES) st = MI_ERR_ARG;
    else {
        // ---- header and trailer: every lane reads the same few bytes, all inside [in, in + nb)
        bool bad = false;
        auto byte = [&](uint64_t i) -> uint32_t { if (i >= nb) { bad = true; return 0u; } return in[i]; };
        bool fdict = false;
        uint32_t dictid = 0, dn = 0;                                    // dn: |E| for an item that uses the dictionary
        const uint64_t hb = inf_header_bytes<DICT>(b.container, byte, bad, &fdict, &dictid);
        const uint8_t *dend = nullptr;
        if constexpr (DICT) {
            dend = dd.end;
            if (b.container == MI_CONTAINER_RAW) dn = dd.n;
            else if (fdict && !bad) { if (dictid == *dd.adler) dn = dd.n; else bad = true; }    // another dictionary's stream
        }
        const uint64_t tl = b.container == MI_CONTAINER_GZIP ? 8u : b.container == MI_CONTAINER_ZLIB ? 4u : 0u;
        if (bad || hb + tl >= nb) st = MI_ERR_CORRUPT;                  // (no room for one byte of DEFLATE data)
        else {
            // the DEFLATE data lies between header and trailer and ends, padded, exactly where the trailer starts
            const uint64_t nbits = 8ull * (nb - hb - tl);
            OutRing<RING> ring;
            const InfWalk w = inf_blocks<RING, true, COUNT_ONLY, DICT>(in, 8ull * hb, nbits, out, (uint32_t)cap, true, ring, s_ring, s_llut,
                                                                       s_dlut, s_ll, s_dc, s_len, s_cl, lane, dend, dn);
            if (w.big) st = MI_ERR_ARG;                                 // more than 2^31 - 1 bytes: not a batch item
            else if (w.bad || !w.final_seen || ((w.pos + 7u) & ~7ull) != nbits) st = MI_ERR_CORRUPT;
            else {
                if (b.container == MI_CONTAINER_GZIP) {
                    const uint64_t t = nb - 4u;
                    const uint32_t isz = (uint32_t)in[t] | ((uint32_t)in[t + 1] << 8) | ((uint32_t)in[t + 2] << 16) | ((uint32_t)in[t + 3] << 24);
                    if (isz != w.o) st = MI_ERR_CORRUPT;
                }
                if (st == MI_OK) {
                    size = w.o;
                    if constexpr (!COUNT_ONLY) {
                        if (w.counting) st = MI_ERR_CAPACITY;
                        else ring.finish(w.o);
                    }
                }
            }
        }
    }
    if (lane == 0) {
        b.status[item] = st;
        b.out_bytes[item] = size;
        if (st != MI_OK && b.failed) atomicAdd(b.failed, 1u);
    }
}

// The checksum of every item that came out MI_OK against its trailer (zlib: Adler-32 big-endian in the last four bytes; gzip:
// CRC-32 little-endian in front of ISIZE).  One workgroup per item: an item of hundreds of megabytes belongs to mi_inflate_dev.
__global__ __launch_bounds__(ZCK_THREADS)
void k_inflate_batch_check(InfBatch b)
{
    __shared__ CrcLds s_crc;
    __shared__ AdlerLds s_adl;
    __shared__ uint32_t s_st;
    const uint32_t tid = threadIdx.x, item = blockIdx.x;
    if (tid == 0) s_st = b.status[item];
    __syncthreads();
    if (s_st != MI_OK) return;                                         // (the whole workgroup)
    const uint8_t *in = reinterpret_cast<const uint8_t *>(b.in[item]);
    const uint8_t *out = reinterpret_cast<const uint8_t *>(b.out[item]);
    const uint64_t nb = b.in_bytes[item], n = b.out_bytes[item];
    uint32_t have = 0, want = 0;
    if (b.container == MI_CONTAINER_GZIP) {
        crc_lds_init(s_crc, tid);
        __syncthreads();
        const uint32_t pure = crc_range(out, n, s_crc, tid);
        if (tid == 0) {
            const uint64_t t = nb - 8u;
            have = crc_standard(pure, n);
            want = (uint32_t)in[t] | ((uint32_t)in[t + 1] << 8) | ((uint32_t)in[t + 2] << 16) | ((uint32_t)in[t + 3] << 24);
        }
    } else {
        uint32_t ra, rs;
        adler_range(out, 0, n, (((uintptr_t)out) & 15u) == 0, s_adl, tid, ra, rs);
        if (tid == 0) {
            const uint64_t t = nb - 4u;
            have = adler_standard(ra, rs, n);
            want = ((uint32_t)in[t] << 24) | ((uint32_t)in[t + 1] << 16) | ((uint32_t)in[t + 2] << 8) | (uint32_t)in[t + 3];
        }
    }
    if (tid == 0 && have != want) {
        b.status[item] = MI_ERR_CORRUPT;
        b.out_bytes[item] = 0;
        if (b.failed) atomicAdd(b.failed, 1u);
    }
}

static mi_status batch_launch(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                              void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes, uint32_t *d_status,
                              uint32_t *d_failed, uint32_t flags, hipStream_t s, bool count_only, const uint8_t *d_dict = nullptr,
                              uint64_t dict_bytes = 0)
{
    if (!ctx || container > MI_CONTAINER_GZIP || (flags & ~MI_INFLATE_NO_CHECKSUM) || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (dict_bytes && (!d_dict || container == MI_CONTAINER_GZIP || dict_bytes > INFB_MAX_BYTES)) return MI_ERR_ARG;   // gzip has no FDICT
    if (count == 0) return MI_OK;
    if (!d_in || !d_in_bytes || !d_out_bytes || !d_status || (!count_only && (!d_out || !d_out_cap))) return MI_ERR_ARG;
    const uint32_t cnt = (uint32_t)count;
    // The size-class dispatch order is opt-in (MI_INFLATE_BATCH_ORDER=1, read at call time) until it is measured to pay for
    // its memset and three launches (DESIGN_HISTORY.md): by default workgroup j takes item j and no workspace is touched.
    const char *e = getenv("MI_INFLATE_BATCH_ORDER");
    const bool ordered = e && atoi(e) != 0;
    uint32_t *head = nullptr, *order = nullptr;              // head: hist[64], cursor[64]
    // DICTID: the Adler-32 of the whole dictionary, on the stream, its partials and its result in the workspace
    const bool dict = dict_bytes != 0, dsum = dict && container == MI_CONTAINER_ZLIB;
    uint8_t *zws = nullptr;
    uint32_t *d_adler = nullptr;
    const mi_status st = ordered || dsum ? mi_ws_carve(ctx, [&](mi_carver &cv) {
                                               if (ordered) { cv.take(head, INFB_WS_HEAD / 4); cv.take(order, cnt); }
                                               if (dsum) { cv.take(zws, defz_ws_bytes()); cv.take(d_adler, 1); }
                                           })
                                         : MI_OK;            // (allocates and synchronises only while it grows)
    if (st) return st;
    if (dsum) { const mi_status sd = defz_checksum(ctx, false, d_dict, dict_bytes, zws, d_adler, s); if (sd) return sd; }
    if (d_failed) MI_HIP(ctx, hipMemsetAsync(d_failed, 0, 4, s));
    if (ordered) {
        uint32_t *hist = head, *cursor = hist + 64;
        MI_HIP(ctx, hipMemsetAsync(hist, 0, INFB_WS_HEAD, s));
        mi_prof_scope pr(ctx, "k_batch_order", s, 0);
        hipLaunchKernelGGL(k_batch_hist, dim3((cnt + 255u) / 256u), dim3(256), 0, s, d_in_bytes, cnt, hist);
        hipLaunchKernelGGL(k_batch_scan, dim3(1), dim3(1), 0, s, hist, cursor);
        hipLaunchKernelGGL(k_batch_scatter, dim3((cnt + 255u) / 256u), dim3(256), 0, s, d_in_bytes, cnt, cursor, order);
    }
    InfBatch b{d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed, order, container};
    {
        mi_prof_scope pr(ctx, count_only ? "k_inflate_batch_size" : "k_inflate_batch", s, 0);
        // the ring: as mi_inflate_dev — few items cannot fill the CUs anyway and get the whole 32 KiB window in LDS
        const uint32_t want = lz_decode_ring_want(cnt, 32768u, 4096u);
        if (dict) {
            const InfDict<true> dd{d_dict + dict_bytes, (uint32_t)(dict_bytes < 32768u ? dict_bytes : 32768u), d_adler};
            if (count_only) hipLaunchKernelGGL((k_inflate_batch<4096u, true, true>), dim3(cnt), dim3(64), 0, s, b, dd);
            else if (want <= 4096u) hipLaunchKernelGGL((k_inflate_batch<4096u, false, true>), dim3(cnt), dim3(64), 0, s, b, dd);
            else hipLaunchKernelGGL((k_inflate_batch<32768u, false, true>), dim3(cnt), dim3(64), 0, s, b, dd);
        } else if (count_only) hipLaunchKernelGGL((k_inflate_batch<4096u, true>), dim3(cnt), dim3(64), 0, s, b, InfDict<false>{});
        else if (want <= 4096u) hipLaunchKernelGGL((k_inflate_batch<4096u, false>), dim3(cnt), dim3(64), 0, s, b, InfDict<false>{});
        else hipLaunchKernelGGL((k_inflate_batch<32768u, false>), dim3(cnt), dim3(64), 0, s, b, InfDict<false>{});
    }
    if (!count_only && container != MI_CONTAINER_RAW && !(flags & MI_INFLATE_NO_CHECKSUM)) {
        mi_prof_scope pr(ctx, "k_inflate_batch_check", s, 0);
        hipLaunchKernelGGL(k_inflate_batch_check, dim3(cnt), dim3(ZCK_THREADS), 0, s, b);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}

extern "C" mi_status mi_inflate_batch_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                          const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap,
                                          uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, uint32_t flags, void *stream)
{
    return batch_launch(ctx, container, count, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed, flags,
                        (hipStream_t)stream, false);
}

extern "C" mi_status mi_inflate_batch_size_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                               const uint64_t *d_in_bytes, uint64_t *d_out_bytes, uint32_t *d_status,
                                               uint32_t *d_failed, uint32_t flags, void *stream)
{
    return batch_launch(ctx, container, count, d_in, d_in_bytes, nullptr, nullptr, d_out_bytes, d_status, d_failed, flags,
                        (hipStream_t)stream, true);
}

// One preset dictionary for the call (include/mi_codec.h).  dict_bytes == 0 is the call without one.
extern "C" mi_status mi_inflate_batch_dict_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                               const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap,
                                               uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, const uint8_t *d_dict,
                                               uint64_t dict_bytes, uint32_t flags, void *stream)
{
    return batch_launch(ctx, container, count, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, d_failed, flags,
                        (hipStream_t)stream, false, d_dict, dict_bytes);
}

extern "C" mi_status mi_inflate_batch_dict_size_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                                    const uint64_t *d_in_bytes, uint64_t *d_out_bytes, uint32_t *d_status,
                                                    uint32_t *d_failed, const uint8_t *d_dict, uint64_t dict_bytes, uint32_t flags,
                                                    void *stream)
{
    return batch_launch(ctx, container, count, d_in, d_in_bytes, nullptr, nullptr, d_out_bytes, d_status, d_failed, flags,
                        (hipStream_t)stream, true, d_dict, dict_bytes);
}
