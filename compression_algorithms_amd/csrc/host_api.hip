// host_api.hip — every host-buffer convenience entry point of the library: copy in, run the public *_dev path on the
// context's private stream, copy out, synchronise.  The PCIe-inclusive path of the drop-in libraries (dropin_*.c);
// throughput numbers are quoted on the *_dev entry points.  No kernel lives here and nothing here is on the hot path.
//
//   the owners of the buffers, the one-more-try rule of the encoders
//   the chunked (pipelined) paths of the byte-aligned block formats, both directions
//   Huffman, the block formats (tokens, mode H, mode Z, BGZF, FSE), inflate, the whole-buffer lz77 forms
//   the batches (inflate, deflate) and their one staging routine; BGZF read from host bytes (inflate, ranges)
//
// One error convention: a HIP call that fails stores its own code in ctx->last_hip and the entry point returns MI_ERR_HIP
// (MI_HIP, common.h); an allocation that fails is MI_ERR_NOMEM.
#include "common.h"
#include "internal.h"
#include <stdlib.h>
#include <string.h>

namespace {
// The owners of an entry point's buffers.  Nothing may outlive the buffers: a DevBuf's hipFree waits for the device, so no
// kernel or copy still touches device memory when it goes; host staging (HostBuf) is DECLARED BEFORE the DevBufs of its
// function, hence destroyed after them — after that wait — so no copy on the stream still reads or writes it.
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess; }
    template <typename T> T *as() { return reinterpret_cast<T *>(p); }
};
struct HostBuf {
    void *p = nullptr;
    ~HostBuf() { free(p); }
    bool alloc(size_t n) { return (p = malloc(n)) != nullptr; }
    bool zalloc(size_t n) { return (p = calloc(1, n)) != nullptr; }
    template <typename T> T *as() { return reinterpret_cast<T *>(p); }
};
}

// A synchronous entry point has its result in hand when it returns, so an order violation reported while it ran (lz_common.h
// lz_order_violation) is repaired here: the context has switched to ballot ranking, the call encodes once more.
template <class Once> static mi_status host_encode_with_retry(mi_ctx *ctx, Once once)
{
    mi_order_poll(ctx);
    const uint32_t seen_before = ctx->order_violations;
    mi_status st = once();
    mi_order_poll(ctx);                                                     // (chunked paths poll between their chunks too)
    if (st != MI_OK || ctx->order_violations == seen_before) return st;
    const uint32_t seen = ctx->order_violations;
    st = once();
    mi_order_poll(ctx);
    if (st == MI_OK && ctx->order_violations != seen) st = MI_ERR_UNSTABLE; // ballots cannot mis-rank: this does not happen
    ctx->order_reported = ctx->order_violations;                            // handled here: mi_sync need not repeat it
    return st;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host buffers larger than one chunk, byte-aligned formats (deflate tokens, mode H): the input goes up and the stream comes
// down in chunks while the GPU encodes the chunk between them.  One-shot (copy everything, encode, copy everything) was
// 93-98 ms per 10^9 bytes of which only 61 are the encoder (scripts/time_host_api.py).  Chunks are whole blocks, their
// streams are whole bytes, so they are laid end to end on the host and the per-chunk block tables shifted by the running
// total.  Two device buffers of each kind, two short-lived copy streams (created per call: an idle extra stream costs the
// *_dev pipeline 4-7 %, ctx.hip), events only — the host blocks once per chunk to learn the chunk's size.
// MI_HOST_CHUNK_BLOCKS sets the chunk (default 1024 blocks = one batch of the encoder: 14.7 GB/s against 11.6 at 2048 and 11.4 at 4000; tests use small ones).
// ---------------------------------------------------------------------------------------------------------------------
static uint64_t host_chunk_blocks()
{
    const char *e = getenv("MI_HOST_CHUNK_BLOCKS");
    long v = e ? atol(e) : 1024;
    if (v < 1) v = 1;
    if (v > 4000) v = 4000;                               // one chunk's block table must fit half of the pinned staging area
    return (uint64_t)v;
}

static mi_status mi_encode_host_pipelined(mi_ctx *ctx, const mi_lz_params *p, int mode_h, const uint8_t *h_in, uint64_t n,
                                          uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits, bool *done)
{
    *done = false;
    const uint64_t cb = host_chunk_blocks(), C = cb * (uint64_t)p->block;
    if (!p->deflate || n <= C || !ctx->h_pinned || ctx->h_pinned_bytes < 2 * (cb + 1) * 8) return MI_OK;      // the caller's one-shot path
    const uint64_t nchunks = (n + C - 1) / C;
    const uint64_t cbound = (mode_h ? mi_deflate_h_bound_bytes(C, p) : mi_lz_bound_bytes(C, p)) + 64;
    hipStream_t s = mi_host_stream(ctx), cin = nullptr, cout = nullptr;
    hipEvent_t ev_in[2] = {}, ev_enc[2] = {}, ev_out[2] = {};
    DevBuf in[2], out[2], bits[2];
    mi_status st = MI_OK;
    bool ok = hipStreamCreateWithFlags(&cin, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&cout, hipStreamNonBlocking) == hipSuccess;
    for (int b = 0; b < 2 && ok; ++b)
        ok = in[b].alloc(C + 64) && out[b].alloc(cbound) && bits[b].alloc((cb + 1) * 8) &&
             hipEventCreateWithFlags(&ev_in[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ev_enc[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ev_out[b], hipEventDisableTiming) == hipSuccess;
    auto chunk_len = [&](uint64_t c) -> uint64_t { return (c + 1 < nchunks) ? C : n - c * C; };
    auto issue_h2d = [&](uint64_t c) -> bool {
        const int b = (int)(c & 1);
        if (c >= 2 && hipStreamWaitEvent(cin, ev_enc[b], 0) != hipSuccess) return false;          // encode(c - 2) has read in[b]
        if (hipMemcpyAsync(in[b].p, h_in + c * C, chunk_len(c), hipMemcpyHostToDevice, cin) != hipSuccess) return false;
        return hipEventRecord(ev_in[b], cin) == hipSuccess;
    };
    uint64_t *pinned = reinterpret_cast<uint64_t *>(ctx->h_pinned);
    auto issue_encode = [&](uint64_t c) -> mi_status {
        const int b = (int)(c & 1);
        if (hipStreamWaitEvent(s, ev_in[b], 0) != hipSuccess) return MI_ERR_HIP;
        if (c >= 2 && hipStreamWaitEvent(s, ev_out[b], 0) != hipSuccess) return MI_ERR_HIP;       // the stream of chunk c - 2 has left out[b]
        const mi_status e = mode_h ? mi_deflate_h_encode_dev(ctx, p, in[b].as<uint8_t>(), chunk_len(c), out[b].as<uint8_t>(), cbound, bits[b].as<uint64_t>(), s)
                                   : mi_lz_encode_dev(ctx, p, in[b].as<uint8_t>(), chunk_len(c), out[b].as<uint8_t>(), cbound, bits[b].as<uint64_t>(), s);
        if (e) return e;
        const uint64_t nb = (chunk_len(c) + p->block - 1) / p->block;
        if (hipMemcpyAsync(pinned + (size_t)b * (cb + 1), bits[b].p, (nb + 1) * 8, hipMemcpyDeviceToHost, s) != hipSuccess) return MI_ERR_HIP;
        return hipEventRecord(ev_enc[b], s) == hipSuccess ? MI_OK : MI_ERR_HIP;
    };
    uint64_t base_bits = 0;
    if (!ok) st = MI_ERR_NOMEM;
    if (st == MI_OK && !issue_h2d(0)) st = MI_ERR_HIP;
    if (st == MI_OK) st = issue_encode(0);
    for (uint64_t c = 0; c < nchunks && st == MI_OK; ++c) {
        const int b = (int)(c & 1);
        if (c + 1 < nchunks) {
            if (!issue_h2d(c + 1)) { st = MI_ERR_HIP; break; }                                     // (may block the host: the GPU is encoding chunk c)
            st = issue_encode(c + 1);                                                              // queued behind chunk c: no idle GPU while the host reads c's sizes
            if (st) break;
        }
        if (hipEventSynchronize(ev_enc[b]) != hipSuccess) { st = MI_ERR_HIP; break; }
        const uint64_t nb = (chunk_len(c) + p->block - 1) / p->block, blk0 = c * cb;
        const uint64_t *cbits = pinned + (size_t)b * (cb + 1);
        for (uint64_t k = 0; k <= nb; ++k) h_block_bits[blk0 + k] = base_bits + cbits[k];
        const uint64_t cbytes = cbits[nb] / 8;                                                     // whole bytes: byte tokens / word-aligned records
        if (base_bits / 8 + cbytes > cap_bytes) { st = MI_ERR_CAPACITY; break; }
        if (cbytes && hipMemcpyAsync(h_out + base_bits / 8, out[b].p, cbytes, hipMemcpyDeviceToHost, cout) != hipSuccess) { st = MI_ERR_HIP; break; }
        if (hipEventRecord(ev_out[b], cout) != hipSuccess) { st = MI_ERR_HIP; break; }
        base_bits += cbits[nb];
    }
    // the owners' rule (above), and the copy streams and events are destroyed next: drain all three streams whatever happened
    if (cin) (void)hipStreamSynchronize(cin);
    (void)hipStreamSynchronize(s);
    if (cout) (void)hipStreamSynchronize(cout);
    for (int b = 0; b < 2; ++b) { if (ev_in[b]) (void)hipEventDestroy(ev_in[b]); if (ev_enc[b]) (void)hipEventDestroy(ev_enc[b]); if (ev_out[b]) (void)hipEventDestroy(ev_out[b]); }
    if (cin) (void)hipStreamDestroy(cin);
    if (cout) (void)hipStreamDestroy(cout);
    if (st == MI_OK) *done = true;
    return st;
}

// ---------------------------------------------------------------------------------------------------------------------
// The way back, every block format: the stream goes up and the bytes come down in chunks of whole blocks while the GPU decodes
// the chunks between them.  The device buffers are whole (stream, table, output) — a chunk's kernel gets the table from its own
// first block on and the output from its own first byte on; the table's bit offsets stay absolute — so there is nothing to
// recycle.  A decoder wave is one block and the chip wants ~8 000 of them in flight, so chunks are launched AHEAD chunks before
// their bytes are fetched, on AHEAD streams (kernels of neighbouring chunks overlap: one stream alone ran them one after the
// other and mode H gained nothing).  Host order per chunk c: upload(c + AHEAD), launch(c + AHEAD), download(c) — pageable
// copies block the calling thread, and the GPU has AHEAD chunks to decode while they do.
// MI_HOST_DECODE_CHUNK_BLOCKS sets the chunk, MI_HOST_DECODE_AHEAD the look-ahead (1..4); tests use small chunks.  10^9 bytes of
// output, ms one shot -> chunks of 4096 ahead 2: lz77 tokens 65 -> 52, deflate tokens 64 -> 41 (2 GB over the link: it is the
// copies now), mode H 85 -> 78 (2048 x 3: 57 / 44 / 80; 1024 x 4: 71 / 56 / 100; scripts/ab_hostdec.sh).
// ---------------------------------------------------------------------------------------------------------------------
static uint64_t host_decode_chunk_blocks()
{
    const char *e = getenv("MI_HOST_DECODE_CHUNK_BLOCKS");
    long v = e ? atol(e) : 4096;
    if (v < 1) v = 1;
    return (uint64_t)v;
}
static uint32_t host_decode_ahead()
{
    const char *e = getenv("MI_HOST_DECODE_AHEAD");
    long v = e ? atol(e) : 2;
    return (uint32_t)(v < 1 ? 1 : v > 4 ? 4 : v);
}

static mi_status mi_decode_host_pipelined(mi_ctx *ctx, const mi_lz_params *p, int mode_h, const uint8_t *h_stream, uint64_t stream_bytes,
                                          const uint64_t *h_block_bits, uint8_t *h_out, uint64_t n, bool *done)
{
    *done = false;
    constexpr uint32_t NE = 8;                                                                    // events in rotation (> AHEAD)
    const uint64_t cb = host_decode_chunk_blocks(), C = cb * (uint64_t)p->block;
    const uint32_t AHEAD = host_decode_ahead();
    const uint64_t nblocks = (n + p->block - 1) / p->block;
    if (nblocks <= cb) return MI_OK;                                                              // the caller's one-shot path
    const uint64_t nchunks = (nblocks + cb - 1) / cb;
    hipStream_t s = mi_host_stream(ctx), cin = nullptr, cout = nullptr, sx[4] = {s, nullptr, nullptr, nullptr};
    hipEvent_t ev_in[NE] = {}, ev_dec[NE] = {}, ev_setup = nullptr;
    DevBuf st_, bits, out;
    if (!st_.alloc(stream_bytes + 64) || !bits.alloc((nblocks + 1) * 8) || !out.alloc(n + 16)) return MI_ERR_NOMEM;
    bool ok = hipStreamCreateWithFlags(&cin, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&cout, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&ev_setup, hipEventDisableTiming) == hipSuccess;
    for (uint32_t k = 1; k < AHEAD && ok; ++k) ok = hipStreamCreateWithFlags(&sx[k], hipStreamNonBlocking) == hipSuccess;
    for (uint32_t b = 0; b < NE && ok; ++b)
        ok = hipEventCreateWithFlags(&ev_in[b], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&ev_dec[b], hipEventDisableTiming) == hipSuccess;
    mi_status st = ok ? MI_OK : MI_ERR_HIP;
    uint32_t *err = nullptr;
    if (st == MI_OK) {
        ok = hipMemsetAsync(st_.as<uint8_t>() + stream_bytes, 0, 64, s) == hipSuccess &&
             hipMemcpyAsync(bits.p, h_block_bits, (nblocks + 1) * 8, hipMemcpyHostToDevice, s) == hipSuccess;
        err = ok ? mi_err_slot(ctx, s) : nullptr;
        if (!err || hipEventRecord(ev_setup, s) != hipSuccess) st = MI_ERR_HIP;
        for (uint32_t k = 1; k < AHEAD && st == MI_OK; ++k)                                       // table and status word first
            if (hipStreamWaitEvent(sx[k], ev_setup, 0) != hipSuccess) st = MI_ERR_HIP;
    }
    // stream bytes [lo, hi) of chunk c: from where the chunk before stopped to the dword that holds the chunk's last bit
    // (the readers fetch aligned dwords, lz_decode.h)
    auto stream_end = [&](uint64_t c) -> uint64_t {
        if (c + 1 >= nchunks) return stream_bytes;
        const uint64_t e = (((h_block_bits[(c + 1) * cb] + 7) >> 3) + 3) & ~3ull;
        return e < stream_bytes ? e : stream_bytes;
    };
    auto chunk_len = [&](uint64_t c) -> uint64_t { return (c + 1 < nchunks) ? C : n - c * C; };
    auto upload_launch = [&](uint64_t c) -> mi_status {
        const uint64_t lo = c ? stream_end(c - 1) : 0, hi = stream_end(c);
        hipStream_t sc = sx[c % AHEAD];
        if (hi > lo && hipMemcpyAsync(st_.as<uint8_t>() + lo, h_stream + lo, hi - lo, hipMemcpyHostToDevice, cin) != hipSuccess) return MI_ERR_HIP;
        if (hipEventRecord(ev_in[c % NE], cin) != hipSuccess || hipStreamWaitEvent(sc, ev_in[c % NE], 0) != hipSuccess) return MI_ERR_HIP;
        const mi_status e = mode_h ? mi_deflate_h_decode_launch(ctx, p, st_.as<uint8_t>(), stream_bytes, bits.as<uint64_t>() + c * cb, out.as<uint8_t>() + c * C, chunk_len(c), err, sc)
                                   : mi_lz_decode_launch(ctx, p, st_.as<uint8_t>(), stream_bytes, bits.as<uint64_t>() + c * cb, out.as<uint8_t>() + c * C, chunk_len(c), err, sc);
        if (e) return e;
        return hipEventRecord(ev_dec[c % NE], sc) == hipSuccess ? MI_OK : MI_ERR_HIP;
    };
    for (uint64_t c = 0; c < AHEAD && c < nchunks && st == MI_OK; ++c) st = upload_launch(c);
    for (uint64_t c = 0; c < nchunks && st == MI_OK; ++c) {
        if (c + AHEAD < nchunks) { st = upload_launch(c + AHEAD); if (st) break; }
        if (hipStreamWaitEvent(cout, ev_dec[c % NE], 0) != hipSuccess ||
            hipMemcpyAsync(h_out + c * C, out.as<uint8_t>() + c * C, chunk_len(c), hipMemcpyDeviceToHost, cout) != hipSuccess) { st = MI_ERR_HIP; break; }
    }
    // the owners' rule (above), and the streams and events are destroyed next: drain every stream whatever happened
    if (cin) (void)hipStreamSynchronize(cin);
    for (uint32_t k = 0; k < 4; ++k) if (k == 0 || sx[k]) (void)hipStreamSynchronize(sx[k]);
    if (cout) (void)hipStreamSynchronize(cout);
    uint32_t h_err = 0;
    if (st == MI_OK && hipMemcpy(&h_err, err, 4, hipMemcpyDeviceToHost) != hipSuccess) st = MI_ERR_HIP;
    for (uint32_t b = 0; b < NE; ++b) { if (ev_in[b]) (void)hipEventDestroy(ev_in[b]); if (ev_dec[b]) (void)hipEventDestroy(ev_dec[b]); }
    if (ev_setup) (void)hipEventDestroy(ev_setup);
    if (cin) (void)hipStreamDestroy(cin);
    if (cout) (void)hipStreamDestroy(cout);
    for (uint32_t k = 1; k < 4; ++k) if (sx[k]) (void)hipStreamDestroy(sx[k]);
    if (st == MI_OK && h_err) st = MI_ERR_CORRUPT;       // (the caller's buffer may hold the chunks that came down before the bad one)
    if (st == MI_OK) *done = true;
    return st;
}

extern "C" mi_status mi_huffman_encode(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, uint32_t *h_words,
                                       uint64_t cap_words, mi_huffman_info *h_info, mi_huffman_tree *h_tree)
{
    if (!ctx || !h_words || !h_info || (n && !h_in)) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    // reserve the kernels' workspace first: growing it later would synchronise mid-sequence
    mi_status st = mi_ws_reserve(ctx, huff_ws_bytes(n));
    if (st) return st;
    DevBuf in, words, info, tree;
    if (!in.alloc(n + 16) || !words.alloc(cap_words * 4) || !info.alloc(sizeof(mi_huffman_info)) ||
        !tree.alloc(sizeof(mi_huffman_tree))) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpyAsync(in.p, h_in, n, hipMemcpyHostToDevice, s));
    st = mi_huffman_encode_dev(ctx, in.as<uint8_t>(), n, words.as<uint32_t>(), cap_words, info.as<mi_huffman_info>(),
                               tree.as<mi_huffman_tree>(), nullptr, s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(h_info, info.p, sizeof(*h_info), hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    if (h_tree) MI_HIP(ctx, hipMemcpy(h_tree, tree.p, sizeof(*h_tree), hipMemcpyDeviceToHost));
    if (h_info->status != MI_OK) return (mi_status)h_info->status;
    const uint64_t nw = (h_info->total_bits + 31) >> 5;
    if (nw > cap_words) return MI_ERR_CAPACITY;
    if (nw) MI_HIP(ctx, hipMemcpy(h_words, words.p, nw * 4, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" mi_status mi_huffman_encode2(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, uint32_t *h_words, uint64_t cap_words,
                                        mi_huffman_info *h_info, mi_huffman_tree *h_tree, uint64_t *h_tile_off)
{
    if (!ctx || !h_words || !h_info || (n && !h_in)) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t ntiles = (n + MI_HUFFMAN_TILE - 1) / MI_HUFFMAN_TILE;
    DevBuf in, words, info, tree, toff;
    if (!in.alloc(n + 16) || !words.alloc(cap_words * 4) || !info.alloc(sizeof(mi_huffman_info)) ||
        !tree.alloc(sizeof(mi_huffman_tree)) || !toff.alloc((ntiles + 1) * 8)) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpyAsync(in.p, h_in, n, hipMemcpyHostToDevice, s));
    mi_status st = mi_huffman_encode_dev(ctx, in.as<uint8_t>(), n, words.as<uint32_t>(), cap_words, info.as<mi_huffman_info>(),
                                         tree.as<mi_huffman_tree>(), toff.as<uint64_t>(), s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(h_info, info.p, sizeof(*h_info), hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    if (h_tree) MI_HIP(ctx, hipMemcpy(h_tree, tree.p, sizeof(*h_tree), hipMemcpyDeviceToHost));
    if (h_info->status != MI_OK) return (mi_status)h_info->status;
    const uint64_t nw = (h_info->total_bits + 31) >> 5;
    if (nw > cap_words) return MI_ERR_CAPACITY;
    if (nw) MI_HIP(ctx, hipMemcpy(h_words, words.p, nw * 4, hipMemcpyDeviceToHost));
    if (h_tile_off) MI_HIP(ctx, hipMemcpy(h_tile_off, toff.p, (ntiles + 1) * 8, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" mi_status mi_huffman_decode(mi_ctx *ctx, const uint32_t *h_words, uint64_t total_bits, const mi_huffman_tree *h_tree,
                                       uint32_t n_nodes, const uint64_t *h_tile_off, uint8_t *h_out, uint64_t n)
{
    if (!ctx || !h_words || !h_tree || (n && !h_out)) return MI_ERR_ARG;
    if (n == 0) return MI_OK;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t nw = (total_bits + 31) >> 5, ntiles = (n + MI_HUFFMAN_TILE - 1) / MI_HUFFMAN_TILE;
    if (h_tile_off) {                                   // tile offsets index the words: monotonic and inside the stream
        mi_status vt = mi_validate_block_table(h_tile_off, ntiles, nw * 4, 1u);
        if (vt) return vt;
        if (h_tile_off[ntiles] > total_bits) return MI_ERR_CORRUPT;
    }
    DevBuf words, tree, toff, out;
    if (!words.alloc((nw + 2) * 4) || !tree.alloc(sizeof(mi_huffman_tree)) || !toff.alloc((ntiles + 1) * 8) || !out.alloc(n + 16))
        return MI_ERR_NOMEM;
    MI_HIP(ctx, hipMemsetAsync(words.as<uint32_t>() + nw, 0, 8, s));
    if (nw) MI_HIP(ctx, hipMemcpyAsync(words.p, h_words, nw * 4, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(tree.p, h_tree, sizeof(*h_tree), hipMemcpyHostToDevice, s));
    if (h_tile_off) MI_HIP(ctx, hipMemcpyAsync(toff.p, h_tile_off, (ntiles + 1) * 8, hipMemcpyHostToDevice, s));
    mi_status st = mi_huffman_decode_dev(ctx, words.as<uint32_t>(), total_bits, tree.as<mi_huffman_tree>(), n_nodes,
                                         h_tile_off ? toff.as<uint64_t>() : nullptr, out.as<uint8_t>(), n, s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    return MI_OK;
}

// histogram + tree build alone, host buffer in (the drop-in's build_huffman_tree, huffman.c:179-215)
extern "C" mi_status mi_huffman_build(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, mi_huffman_info *h_info, mi_huffman_tree *h_tree)
{
    if (!ctx || !h_info || !h_tree || (n && !h_in)) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t ntiles = mi_huffman_num_tiles(n);
    DevBuf in, hist, thist, info, tree;
    if (!in.alloc(n + 16) || !hist.alloc(256 * 8) || !thist.alloc((ntiles + 1) * 1024) || !info.alloc(sizeof(mi_huffman_info)) ||
        !tree.alloc(sizeof(mi_huffman_tree))) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpyAsync(in.p, h_in, n, hipMemcpyHostToDevice, s));
    mi_status st = mi_huffman_hist_dev(ctx, in.as<uint8_t>(), n, hist.as<uint64_t>(), thist.as<uint32_t>(), s);
    if (st) return st;
    st = mi_huffman_build_dev(ctx, hist.as<uint64_t>(), info.as<mi_huffman_info>(), tree.as<mi_huffman_tree>(), s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(h_info, info.p, sizeof(*h_info), hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipMemcpyAsync(h_tree, tree.p, sizeof(*h_tree), hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return (mi_status)h_info->status;
}

// pack with GIVEN codes from a bit offset (the drop-in's _huffman_compress, huffman.c:267-285, which appends to a
// BitWriter wherever it stands).  h_words[0] holds the stream from bit `bit_offset` on (its first bit_offset bits are 0).
extern "C" mi_status mi_huffman_encode_with_codes(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, const uint32_t *h_codes,
                                                  const uint8_t *h_lengths, uint32_t bit_offset, uint32_t *h_words,
                                                  uint64_t cap_words, mi_huffman_info *h_info)
{
    if (!ctx || !h_codes || !h_lengths || !h_words || !h_info || (n && !h_in) || bit_offset > 31 || cap_words < 2) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t ntiles = mi_huffman_num_tiles(n);
    mi_huffman_tree t;
    memset(&t, 0, sizeof t);
    memcpy(t.code, h_codes, sizeof t.code); memcpy(t.length, h_lengths, sizeof t.length);
    DevBuf in, hist, thist, info, tree, words;
    if (!in.alloc(n + 16) || !hist.alloc(256 * 8) || !thist.alloc((ntiles + 1) * 1024) || !info.alloc(sizeof(mi_huffman_info)) ||
        !tree.alloc(sizeof(mi_huffman_tree)) || !words.alloc(cap_words * 4)) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpyAsync(in.p, h_in, n, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(tree.p, &t, sizeof t, hipMemcpyHostToDevice, s));
    mi_status st = mi_huffman_hist_dev(ctx, in.as<uint8_t>(), n, hist.as<uint64_t>(), thist.as<uint32_t>(), s);
    if (st) return st;
    st = mi_huffman_encode_with_tree_dev(ctx, in.as<uint8_t>(), n, tree.as<mi_huffman_tree>(), thist.as<uint32_t>(), bit_offset,
                                         words.as<uint32_t>(), cap_words, info.as<mi_huffman_info>(), nullptr, s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(h_info, info.p, sizeof(*h_info), hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    if (h_info->status != MI_OK) return (mi_status)h_info->status;
    const uint64_t nw = (h_info->total_bits + 31) >> 5;
    if (nw > cap_words) return MI_ERR_CAPACITY;
    if (nw) MI_HIP(ctx, hipMemcpy(h_words, words.p, nw * 4, hipMemcpyDeviceToHost));
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The block formats, one shot: everything up, the *_dev call, everything down.
// ---------------------------------------------------------------------------------------------------------------------
// How an encoder's stream length is learned once its table is down: the table's last entry rounded up to bytes (tokens: the
// lz77 flavour ends inside a byte), the same in whole bytes (mode H), or the out_bytes word the encoder writes behind the
// table (mode Z, BGZF: containers and the EOF member are not in the table).
enum BytesFrom { TABLE_BITS_ROUNDED_UP, TABLE_BITS_WHOLE, OUT_BYTES_WORD };

// enc(d_in, d_out, cap, d_block_bits, d_out_bytes, s): the *_dev call; d_out_bytes is there with OUT_BYTES_WORD only
template <class Enc>
static mi_status block_encode_once(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, uint64_t nblocks, uint64_t bound, BytesFrom from,
                                   uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits, uint64_t *h_out_bytes, Enc enc)
{
    hipStream_t s = mi_host_stream(ctx);
    const bool word = from == OUT_BYTES_WORD;
    DevBuf in, out, bits;
    if (!in.alloc(n + 64) || !out.alloc(bound + 64) || !bits.alloc((nblocks + 1 + word) * 8)) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpyAsync(in.p, h_in, n, hipMemcpyHostToDevice, s));
    mi_status st = enc(in.as<uint8_t>(), out.as<uint8_t>(), bound + 64, bits.as<uint64_t>(), bits.as<uint64_t>() + nblocks + 1, s);
    if (st) return st;
    uint64_t bytes = 0;
    MI_HIP(ctx, hipMemcpyAsync(h_block_bits, bits.p, (nblocks + 1) * 8, hipMemcpyDeviceToHost, s));
    if (word) MI_HIP(ctx, hipMemcpyAsync(&bytes, bits.as<uint64_t>() + nblocks + 1, 8, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    if (!word) bytes = (h_block_bits[nblocks] + (from == TABLE_BITS_ROUNDED_UP ? 7 : 0)) / 8;
    if (bytes > cap_bytes) return MI_ERR_CAPACITY;       // (tokens, Z, BGZF: the caller's capacity is at least the bound already)
    if (bytes) MI_HIP(ctx, hipMemcpy(h_out, out.p, bytes, hipMemcpyDeviceToHost));
    if (h_out_bytes) *h_out_bytes = bytes;
    return MI_OK;
}

extern "C" mi_status mi_lz_encode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_in, uint64_t n,
                                  uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits)
{
    if (!ctx || !h_out || !h_block_bits || (n && !h_in) || !p || p->parse) return MI_ERR_ARG;
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        const uint64_t nblocks = p->block ? (n + p->block - 1) / p->block : 0;
        const uint64_t bound = mi_lz_bound_bytes(n, p);
        if (cap_bytes < bound) return MI_ERR_CAPACITY;
        if (lz_check_params(p) == MI_OK && p->deflate) {       // byte tokens: chunks overlap their transfers with the encoder
            bool done = false;
            const mi_status ps = mi_encode_host_pipelined(ctx, p, 0, h_in, n, h_out, cap_bytes, h_block_bits, &done);
            if (ps || done) return ps;
        }
        return block_encode_once(ctx, h_in, n, nblocks, bound, TABLE_BITS_ROUNDED_UP, h_out, cap_bytes, h_block_bits, nullptr,
            [&](uint8_t *d_in, uint8_t *d_out, uint64_t cap, uint64_t *d_bits, uint64_t *, hipStream_t s) {
                return mi_lz_encode_dev(ctx, p, d_in, n, d_out, cap, d_bits, s); });
    });
}

extern "C" mi_status mi_deflate_h_encode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_in, uint64_t n,
                                         uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits)
{
    if (!ctx || !p || !h_out || !h_block_bits || (n && !h_in) || !p->block || p->parse) return MI_ERR_ARG;
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        bool done = false;
        const mi_status ps = mi_encode_host_pipelined(ctx, p, 1, h_in, n, h_out, cap_bytes, h_block_bits, &done);
        if (ps || done) return ps;
        const uint64_t nblocks = (n + p->block - 1) / p->block, bound = mi_deflate_h_bound_bytes(n, p);
        return block_encode_once(ctx, h_in, n, nblocks, bound, TABLE_BITS_WHOLE, h_out, cap_bytes, h_block_bits, nullptr,
            [&](uint8_t *d_in, uint8_t *d_out, uint64_t cap, uint64_t *d_bits, uint64_t *, hipStream_t s) {
                return mi_deflate_h_encode_dev(ctx, p, d_in, n, d_out, cap, d_bits, s); });
    });
}

extern "C" mi_status mi_deflate_z_encode(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, const uint8_t *h_in, uint64_t n,
                                         uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits, uint64_t *h_out_bytes)
{
    if (!ctx || !p || !h_out || !h_block_bits || (n && !h_in)) return MI_ERR_ARG;
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        mi_status st = defz_check(p, container);
        if (st) return st;
        const uint64_t bound = mi_deflate_z_bound_bytes(n, p, container);
        if (cap_bytes < bound) return MI_ERR_CAPACITY;
        return block_encode_once(ctx, h_in, n, (n + p->block - 1) / p->block, bound, OUT_BYTES_WORD, h_out, cap_bytes, h_block_bits, h_out_bytes,
            [&](uint8_t *d_in, uint8_t *d_out, uint64_t cap, uint64_t *d_bits, uint64_t *d_out_bytes, hipStream_t s) {
                return mi_deflate_z_encode_dev(ctx, p, container, d_in, n, d_out, cap, d_bits, d_out_bytes, s); });
    });
}

extern "C" mi_status mi_bgzf_encode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_in, uint64_t n, uint8_t *h_out,
                                    uint64_t cap_bytes, uint64_t *h_member_bits, uint64_t *h_out_bytes)
{
    if (!ctx || !p || !h_out || !h_member_bits || (n && !h_in)) return MI_ERR_ARG;
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        mi_status st = defz_check(p, MI_CONTAINER_RAW);
        if (st) return st;
        if (p->block > MI_BGZF_MAX_BLOCK) return MI_ERR_ARG;
        const uint64_t bound = mi_bgzf_bound_bytes(n, p);
        if (cap_bytes < bound) return MI_ERR_CAPACITY;
        return block_encode_once(ctx, h_in, n, (n + p->block - 1) / p->block, bound, OUT_BYTES_WORD, h_out, cap_bytes, h_member_bits, h_out_bytes,
            [&](uint8_t *d_in, uint8_t *d_out, uint64_t cap, uint64_t *d_bits, uint64_t *d_out_bytes, hipStream_t s) {
                return mi_bgzf_encode_dev(ctx, p, d_in, n, d_out, cap, d_bits, d_out_bytes, s); });
    });
}

// tokens (mode_h 0) and mode H (1): the table indexes the stream, so it is checked before anything is copied or launched
static mi_status block_decode_host(mi_ctx *ctx, const mi_lz_params *p, int mode_h, const uint8_t *h_stream, uint64_t stream_bytes,
                                   const uint64_t *h_block_bits, uint8_t *h_out, uint64_t n)
{
    if (!ctx || !p || !h_stream || !h_block_bits || (n && !h_out) || !p->block) return MI_ERR_ARG;
    if (n == 0) return MI_OK;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t nblocks = (n + p->block - 1) / p->block;
    mi_status st = mi_validate_block_table(h_block_bits, nblocks, stream_bytes, mode_h ? 32u : p->deflate ? 8u : 1u);
    if (st) return st;
    {
        bool done = false;
        st = mi_decode_host_pipelined(ctx, p, mode_h, h_stream, stream_bytes, h_block_bits, h_out, n, &done);
        if (st || done) return st;
    }
    DevBuf st_, bits, out;
    if (!st_.alloc(stream_bytes + 64) || !bits.alloc((nblocks + 1) * 8) || !out.alloc(n + 16)) return MI_ERR_NOMEM;
    MI_HIP(ctx, hipMemsetAsync(st_.as<uint8_t>() + stream_bytes, 0, 64, s));
    MI_HIP(ctx, hipMemcpyAsync(st_.p, h_stream, stream_bytes, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(bits.p, h_block_bits, (nblocks + 1) * 8, hipMemcpyHostToDevice, s));
    st = mode_h ? mi_deflate_h_decode_dev(ctx, p, st_.as<uint8_t>(), stream_bytes, bits.as<uint64_t>(), out.as<uint8_t>(), n, s)
                : mi_lz_decode_dev(ctx, p, st_.as<uint8_t>(), stream_bytes, bits.as<uint64_t>(), out.as<uint8_t>(), n, s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" mi_status mi_lz_decode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_stream, uint64_t stream_bytes,
                                  const uint64_t *h_block_bits, uint8_t *h_out, uint64_t n)
{
    return block_decode_host(ctx, p, 0, h_stream, stream_bytes, h_block_bits, h_out, n);
}

extern "C" mi_status mi_deflate_h_decode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_stream, uint64_t stream_bytes,
                                         const uint64_t *h_block_bits, uint8_t *h_out, uint64_t n)
{
    return block_decode_host(ctx, p, 1, h_stream, stream_bytes, h_block_bits, h_out, n);
}

// standard DEFLATE from a table of restart points (no tail memset, an empty output is a valid call: not block_decode_host)
extern "C" mi_status mi_inflate(mi_ctx *ctx, uint32_t container, uint32_t block, const uint8_t *h_stream, uint64_t stream_bytes,
                                const uint64_t *h_seg_bits, uint8_t *h_out, uint64_t n, uint32_t flags)
{
    if (!ctx || !h_stream || !h_seg_bits || (n && !h_out) || block == 0u) return MI_ERR_ARG;
    const uint64_t nseg = (n + block - 1) / block;
    mi_status st = mi_validate_block_table(h_seg_bits, nseg, stream_bytes, 8u);
    if (st) return st;
    hipStream_t s = mi_host_stream(ctx);
    DevBuf st_, bits, out;
    if (!st_.alloc(stream_bytes + 64) || !bits.alloc((nseg + 1) * 8) || !out.alloc(n + 16)) return MI_ERR_NOMEM;
    if (stream_bytes) MI_HIP(ctx, hipMemcpyAsync(st_.p, h_stream, stream_bytes, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(bits.p, h_seg_bits, (nseg + 1) * 8, hipMemcpyHostToDevice, s));
    st = mi_inflate_dev(ctx, container, block, st_.as<uint8_t>(), stream_bytes, bits.as<uint64_t>(), out.as<uint8_t>(), n, flags, s);
    if (st) return st;
    if (n) MI_HIP(ctx, hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" mi_status mi_fse_encode(mi_ctx *ctx, const mi_fse_params *p, const uint8_t *h_in, uint64_t n, uint8_t *h_packed,
                                   uint64_t cap_bytes, uint64_t *h_offsets)
{
    if (!ctx || !p || !h_packed || !h_offsets || (n && !h_in) || !p->block) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t nblocks = (n + p->block - 1) / p->block, need = nblocks * mi_fse_block_bound(p);
    if (cap_bytes < need) return MI_ERR_CAPACITY;
    DevBuf in, out, offs;
    if (!in.alloc(n + 16) || !out.alloc(need + 16) || !offs.alloc((nblocks + 1) * 8)) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpyAsync(in.p, h_in, n, hipMemcpyHostToDevice, s));
    mi_status st = mi_fse_encode_dev(ctx, p, in.as<uint8_t>(), n, out.as<uint8_t>(), need + 16, offs.as<uint64_t>(), s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(h_offsets, offs.p, (nblocks + 1) * 8, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t bytes = h_offsets[nblocks] / 8;
    if (bytes) MI_HIP(ctx, hipMemcpy(h_packed, out.p, bytes, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" mi_status mi_fse_decode(mi_ctx *ctx, const mi_fse_params *p, const uint8_t *h_packed, uint64_t packed_bytes,
                                   const uint64_t *h_offsets, uint8_t *h_out, uint64_t n)
{
    if (!ctx || !p || !h_packed || !h_offsets || (n && !h_out) || !p->block) return MI_ERR_ARG;
    if (n == 0) return MI_OK;
    hipStream_t s = mi_host_stream(ctx);
    const uint64_t nblocks = (n + p->block - 1) / p->block;
    mi_status st = mi_validate_block_table(h_offsets, nblocks, packed_bytes, 32u);
    if (st) return st;
    const uint64_t bytes = h_offsets[nblocks] / 8;
    DevBuf in, offs, out;
    if (!in.alloc(bytes + 16) || !offs.alloc((nblocks + 1) * 8) || !out.alloc(n + 16)) return MI_ERR_NOMEM;
    MI_HIP(ctx, hipMemcpyAsync(in.p, h_packed, bytes, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(offs.p, h_offsets, (nblocks + 1) * 8, hipMemcpyHostToDevice, s));
    st = mi_fse_decode_dev(ctx, p, in.as<uint8_t>(), bytes, offs.as<uint64_t>(), out.as<uint8_t>(), n, s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The whole-buffer lz77 forms of the drop-in (lz77_compress_old and the decoder of what it writes): on the NULL stream, with
// blocking copies and a device-wide synchronise, as they always were.
// ---------------------------------------------------------------------------------------------------------------------
// h_out holds mi_lz77_old_bound_bytes(n) bytes
extern "C" mi_status mi_lz77_old_encode(mi_ctx *ctx, uint32_t wbits, uint32_t lbits, const uint8_t *h_in, uint64_t n,
                                        uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_total_bits)
{
    if (!ctx || !h_out || !h_total_bits || (n && !h_in)) return MI_ERR_ARG;
    if (cap_bytes < mi_lz77_old_bound_bytes(n)) return MI_ERR_CAPACITY;
    const uint64_t cap = mi_lz77_old_bound_bytes(n);
    DevBuf in, out, bits;
    if (!in.alloc(n ? n : 1) || !out.alloc(cap) || !bits.alloc(8)) return MI_ERR_NOMEM;
    if (n) MI_HIP(ctx, hipMemcpy(in.p, h_in, n, hipMemcpyHostToDevice));
    mi_status st = mi_lz77_old_encode_dev(ctx, wbits, lbits, in.as<uint8_t>(), n, out.as<uint8_t>(), cap, bits.as<uint64_t>(), nullptr);
    if (st) return st;
    MI_HIP(ctx, hipDeviceSynchronize());
    MI_HIP(ctx, hipMemcpy(h_total_bits, bits.p, 8, hipMemcpyDeviceToHost));
    MI_HIP(ctx, hipMemcpy(h_out, out.p, (size_t)(*h_total_bits / 8 + 1), hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" mi_status mi_lz77_whole_decode(mi_ctx *ctx, uint32_t wbits, uint32_t lbits, const uint8_t *h_stream, uint64_t stream_bytes,
                                          uint64_t total_bits, uint8_t *h_out, uint64_t n)
{
    if (!ctx || !h_stream || (n && !h_out)) return MI_ERR_ARG;
    if (n == 0) return MI_OK;
    const uint64_t sb = (stream_bytes + 3) & ~3ull;
    DevBuf st_, out;
    if (!st_.alloc(sb + 8) || !out.alloc(n)) return MI_ERR_NOMEM;
    MI_HIP(ctx, hipMemset(st_.p, 0, sb + 8));
    MI_HIP(ctx, hipMemcpy(st_.p, h_stream, stream_bytes, hipMemcpyHostToDevice));
    mi_status st = mi_lz77_whole_decode_dev(ctx, wbits, lbits, st_.as<uint8_t>(), sb, total_bits, out.as<uint8_t>(), n, nullptr);
    if (st) return st;
    MI_HIP(ctx, hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The batches: arrays of host pointers.  The items are packed into one device buffer (each at a 16-byte boundary), the
// outputs likewise by their capacities; copy up, run the batch, copy down what came out MI_OK.
// ---------------------------------------------------------------------------------------------------------------------
// The caller's arrays and the per-item limit of the device form.  An item the device answers with MI_ERR_ARG takes no room
// in the packed buffers: its (bad) pointer and size go up as they are.
struct BatchItems {
    uint64_t count; const void *const *in; const uint64_t *in_bytes; void *const *out; const uint64_t *out_cap; uint64_t limit;
    bool in_ok(uint64_t i) const { return in_bytes[i] <= limit && (in[i] || !in_bytes[i]); }
    bool out_ok(uint64_t i) const { return out_cap[i] <= limit && (out[i] || !out_cap[i]); }
};

// call(d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, s): the *_dev call.  Without b.out or b.out_cap nothing is
// staged for the outputs and d_out, d_out_cap are NULL (the size-only mode of the inflater).
template <class Call>
static mi_status batch_host_once(mi_ctx *ctx, const BatchItems &b, uint64_t *h_out_bytes, uint32_t *h_status, Call call)
{
    const uint64_t count = b.count;
    const bool size_only = !b.out || !b.out_cap;
    uint64_t in_total = 0, out_total = 0;
    for (uint64_t i = 0; i < count; ++i) {
        if (b.in_ok(i)) in_total += mi_align_up(b.in_bytes[i], 16);
        if (!size_only && b.out_ok(i)) out_total += mi_align_up(b.out_cap[i], 16);
    }
    hipStream_t s = mi_host_stream(ctx);
    const size_t arr = mi_align_up((size_t)count * 8u, 256);
    // host staging: [in ptrs | in bytes | out ptrs | out caps | out bytes | status], the packed inputs, the packed outputs
    HostBuf h_arr, h_pack, h_res;
    DevBuf d_arr, d_pack, d_res;
    if (!h_arr.zalloc(6 * arr) || !h_pack.alloc(in_total + 16) || !h_res.alloc(out_total + 16)) return MI_ERR_NOMEM;
    if (!d_arr.alloc(6 * arr) || !d_pack.alloc(in_total + 64) || !d_res.alloc(out_total + 64)) return MI_ERR_NOMEM;
    uint8_t *ha = h_arr.as<uint8_t>(), *da = d_arr.as<uint8_t>();
    uint64_t *p_in = (uint64_t *)ha, *p_nb = (uint64_t *)(ha + arr), *p_out = (uint64_t *)(ha + 2 * arr), *p_cap = (uint64_t *)(ha + 3 * arr);
    uint64_t at = 0, ot = 0;
    for (uint64_t i = 0; i < count; ++i) {
        p_nb[i] = b.in_bytes[i];
        if (b.in_ok(i)) {
            p_in[i] = (uint64_t)(uintptr_t)(d_pack.as<uint8_t>() + at);
            if (b.in_bytes[i]) memcpy(h_pack.as<uint8_t>() + at, b.in[i], b.in_bytes[i]);
            at += mi_align_up(b.in_bytes[i], 16);
        } else p_in[i] = b.in[i] ? (uint64_t)(uintptr_t)d_pack.p : 0u;
        if (size_only) continue;
        p_cap[i] = b.out_cap[i];
        if (b.out_ok(i)) { p_out[i] = (uint64_t)(uintptr_t)(d_res.as<uint8_t>() + ot); ot += mi_align_up(b.out_cap[i], 16); }
        else p_out[i] = b.out[i] ? (uint64_t)(uintptr_t)d_res.p : 0u;
    }
    MI_HIP(ctx, hipMemcpyAsync(da, ha, 4 * arr, hipMemcpyHostToDevice, s));
    if (in_total) MI_HIP(ctx, hipMemcpyAsync(d_pack.p, h_pack.p, in_total, hipMemcpyHostToDevice, s));
    mi_status st = call((const void *const *)da, (const uint64_t *)(da + arr), size_only ? nullptr : (void *const *)(da + 2 * arr),
                        size_only ? nullptr : (const uint64_t *)(da + 3 * arr), (uint64_t *)(da + 4 * arr), (uint32_t *)(da + 5 * arr), s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(ha + 4 * arr, da + 4 * arr, 2 * arr, hipMemcpyDeviceToHost, s));
    if (out_total) MI_HIP(ctx, hipMemcpyAsync(h_res.p, d_res.p, out_total, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t *r_nb = (const uint64_t *)(ha + 4 * arr);
    const uint32_t *r_st = (const uint32_t *)(ha + 5 * arr);
    ot = 0;
    for (uint64_t i = 0; i < count; ++i) {
        h_out_bytes[i] = r_nb[i];
        h_status[i] = r_st[i];
        if (size_only || !b.out_ok(i)) continue;
        if (r_st[i] == MI_OK && r_nb[i]) memcpy(b.out[i], h_res.as<uint8_t>() + ot, r_nb[i]);
        ot += mi_align_up(b.out_cap[i], 16);
    }
    return MI_OK;
}

// inflate, or only size (without h_out / h_out_cap)
extern "C" mi_status mi_inflate_batch(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *h_in,
                                      const uint64_t *h_in_bytes, void *const *h_out, const uint64_t *h_out_cap,
                                      uint64_t *h_out_bytes, uint32_t *h_status, uint32_t flags)
{
    if (!ctx || container > MI_CONTAINER_GZIP || (flags & ~MI_INFLATE_NO_CHECKSUM) || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out_bytes || !h_status) return MI_ERR_ARG;
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, INFB_MAX_BYTES};
    return batch_host_once(ctx, b, h_out_bytes, h_status,
        [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
            uint32_t *d_status, hipStream_t s) {
            return d_out ? mi_inflate_batch_dev(ctx, container, count, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, nullptr, flags, s)
                         : mi_inflate_batch_size_dev(ctx, container, count, d_in, d_in_bytes, d_out_bytes, d_status, nullptr, flags, s); });
}

// ... with one preset dictionary for the call, copied up in front of the items
extern "C" mi_status mi_inflate_batch_dict(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *h_in,
                                           const uint64_t *h_in_bytes, void *const *h_out, const uint64_t *h_out_cap,
                                           uint64_t *h_out_bytes, uint32_t *h_status, const uint8_t *h_dict, uint64_t dict_bytes,
                                           uint32_t flags)
{
    if (!ctx || container > MI_CONTAINER_GZIP || (flags & ~MI_INFLATE_NO_CHECKSUM) || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (dict_bytes && (!h_dict || container == MI_CONTAINER_GZIP || dict_bytes > INFB_MAX_BYTES)) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out_bytes || !h_status) return MI_ERR_ARG;
    DevBuf dict;
    if (!dict.alloc(dict_bytes + 16)) return MI_ERR_NOMEM;
    if (dict_bytes) MI_HIP(ctx, hipMemcpyAsync(dict.p, h_dict, dict_bytes, hipMemcpyHostToDevice, mi_host_stream(ctx)));
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, INFB_MAX_BYTES};
    return batch_host_once(ctx, b, h_out_bytes, h_status,
        [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
            uint32_t *d_status, hipStream_t s) {
            return d_out ? mi_inflate_batch_dict_dev(ctx, container, count, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, nullptr,
                                                     dict.as<uint8_t>(), dict_bytes, flags, s)
                         : mi_inflate_batch_dict_size_dev(ctx, container, count, d_in, d_in_bytes, d_out_bytes, d_status, nullptr,
                                                          dict.as<uint8_t>(), dict_bytes, flags, s); });
}

extern "C" mi_status mi_deflate_batch(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                                      const void *const *h_in, const uint64_t *h_in_bytes,
                                      void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status)
{
    if (!ctx) return MI_ERR_ARG;
    mi_status st = defz_check(p, container);
    if (st) return st;
    if (count > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out || !h_out_cap || !h_out_bytes || !h_status) return MI_ERR_ARG;
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, DFB_MAX_BYTES};
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        uint64_t max_blocks = 0;                                           // the launch bound: the blocks of the items that go up
        for (uint64_t i = 0; i < count; ++i)
            if (b.in_ok(i)) max_blocks += (h_in_bytes[i] + p->block - 1) / p->block;
        if (max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
        return batch_host_once(ctx, b, h_out_bytes, h_status,
            [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                uint32_t *d_status, hipStream_t s) {
                return mi_deflate_batch_dev(ctx, p, container, count, d_in, d_in_bytes, max_blocks, d_out, d_out_cap, d_out_bytes, d_status, nullptr, s); });
    });
}

// ... with one preset dictionary for the call, copied up in front of the items
extern "C" mi_status mi_deflate_batch_dict(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                                           const void *const *h_in, const uint64_t *h_in_bytes, void *const *h_out,
                                           const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status, const uint8_t *h_dict,
                                           uint64_t dict_bytes)
{
    if (!ctx) return MI_ERR_ARG;
    mi_status st = defz_check(p, container);
    if (st) return st;
    if (dict_bytes && (!h_dict || container == MI_CONTAINER_GZIP || dict_bytes > DFB_MAX_BYTES)) return MI_ERR_ARG;
    if (count > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out || !h_out_cap || !h_out_bytes || !h_status) return MI_ERR_ARG;
    DevBuf dict;
    if (!dict.alloc(dict_bytes + 16)) return MI_ERR_NOMEM;
    if (dict_bytes) MI_HIP(ctx, hipMemcpyAsync(dict.p, h_dict, dict_bytes, hipMemcpyHostToDevice, mi_host_stream(ctx)));
    const uint32_t ulen = dfb_ulen(dict_bytes, p->block);
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, DFB_MAX_BYTES};
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        uint64_t max_blocks = 0;                                           // the launch bound: the blocks of the items that go up
        for (uint64_t i = 0; i < count; ++i)
            if (b.in_ok(i)) max_blocks += dfb_nblk(h_in_bytes[i], p->block, ulen);
        if (max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
        return batch_host_once(ctx, b, h_out_bytes, h_status,
            [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                uint32_t *d_status, hipStream_t s) {
                return mi_deflate_batch_dict_dev(ctx, p, container, count, d_in, d_in_bytes, max_blocks, d_out, d_out_cap, d_out_bytes, d_status,
                                                 nullptr, dict.as<uint8_t>(), dict_bytes, s); });
    });
}

// raw Snappy: encode (as mi_deflate_batch), and decode or only size (without h_out / h_out_cap, as mi_inflate_batch)
extern "C" mi_status mi_snappy_encode_batch(mi_ctx *ctx, const mi_lz_params *p, uint64_t count, const void *const *h_in,
                                            const uint64_t *h_in_bytes, void *const *h_out, const uint64_t *h_out_cap,
                                            uint64_t *h_out_bytes, uint32_t *h_status)
{
    if (!ctx) return MI_ERR_ARG;
    mi_status st = defz_check(p, MI_CONTAINER_RAW);
    if (st) return st;
    if (count > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out || !h_out_cap || !h_out_bytes || !h_status) return MI_ERR_ARG;
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, DFB_MAX_BYTES};
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        uint64_t max_blocks = 0;                                           // the launch bound: the blocks of the items that go up
        for (uint64_t i = 0; i < count; ++i)
            if (b.in_ok(i)) max_blocks += (h_in_bytes[i] + p->block - 1) / p->block;
        if (max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
        return batch_host_once(ctx, b, h_out_bytes, h_status,
            [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                uint32_t *d_status, hipStream_t s) {
                return mi_snappy_encode_batch_dev(ctx, p, count, d_in, d_in_bytes, max_blocks, d_out, d_out_cap, d_out_bytes, d_status, nullptr, s); });
    });
}

extern "C" mi_status mi_snappy_decode_batch(mi_ctx *ctx, uint64_t count, const void *const *h_in, const uint64_t *h_in_bytes,
                                            void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status,
                                            uint32_t flags)
{
    if (!ctx || flags || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out_bytes || !h_status) return MI_ERR_ARG;
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, INFB_MAX_BYTES};
    return batch_host_once(ctx, b, h_out_bytes, h_status,
        [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
            uint32_t *d_status, hipStream_t s) {
            return d_out ? mi_snappy_decode_batch_dev(ctx, count, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, nullptr, flags, s)
                         : mi_snappy_batch_size_dev(ctx, count, d_in, d_in_bytes, d_out_bytes, d_status, nullptr, s); });
}

// LZ4, raw blocks or frames: as the two Snappy forms (a raw-block item above the block size is refused on the device and has no blocks)
extern "C" mi_status mi_lz4_encode_batch(mi_ctx *ctx, const mi_lz_params *p, uint32_t format, uint64_t count, const void *const *h_in,
                                         const uint64_t *h_in_bytes, void *const *h_out, const uint64_t *h_out_cap,
                                         uint64_t *h_out_bytes, uint32_t *h_status)
{
    if (!ctx || format > MI_LZ4_FRAME) return MI_ERR_ARG;
    mi_status st = defz_check(p, MI_CONTAINER_RAW);
    if (st) return st;
    if (count > DFB_MAX_BYTES) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out || !h_out_cap || !h_out_bytes || !h_status) return MI_ERR_ARG;
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, DFB_MAX_BYTES};
    return host_encode_with_retry(ctx, [&]() -> mi_status {
        uint64_t max_blocks = 0;
        for (uint64_t i = 0; i < count; ++i)
            if (b.in_ok(i) && (format == MI_LZ4_FRAME || h_in_bytes[i] <= p->block)) max_blocks += (h_in_bytes[i] + p->block - 1) / p->block;
        if (max_blocks > DFB_MAX_BYTES) return MI_ERR_ARG;
        return batch_host_once(ctx, b, h_out_bytes, h_status,
            [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                uint32_t *d_status, hipStream_t s) {
                return mi_lz4_encode_batch_dev(ctx, p, format, count, d_in, d_in_bytes, max_blocks, d_out, d_out_cap, d_out_bytes, d_status, nullptr, s); });
    });
}

extern "C" mi_status mi_lz4_decode_batch(mi_ctx *ctx, uint64_t count, const void *const *h_in, const uint64_t *h_in_bytes,
                                         void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status,
                                         uint32_t format, uint32_t flags)
{
    if (!ctx || format > MI_LZ4_FRAME || flags || count > 0x7FFFFFFFull) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_in || !h_in_bytes || !h_out_bytes || !h_status) return MI_ERR_ARG;
    const BatchItems b{count, h_in, h_in_bytes, h_out, h_out_cap, INFB_MAX_BYTES};
    return batch_host_once(ctx, b, h_out_bytes, h_status,
        [&](const void *const *d_in, const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
            uint32_t *d_status, hipStream_t s) {
            return d_out ? mi_lz4_decode_batch_dev(ctx, count, d_in, d_in_bytes, d_out, d_out_cap, d_out_bytes, d_status, nullptr, format, flags, s)
                         : mi_lz4_batch_size_dev(ctx, count, d_in, d_in_bytes, d_out_bytes, d_status, nullptr, format, s); });
}

// ---------------------------------------------------------------------------------------------------------------------
// BGZF read from host bytes: the stream goes up and is indexed on the device in two steps — count the members (and the bytes
// they inflate to), then, with a table of that size, list them.
// ---------------------------------------------------------------------------------------------------------------------
struct BgzfIndexed { DevBuf stream, count, members; uint64_t cnt[2] = {0, 0}; };   // cnt: members, inflated bytes (count on the device)

// between(): the caller's look at ix.cnt before the table is allocated (its limits, its own buffers of that size)
template <class Between>
static mi_status bgzf_index_host(mi_ctx *ctx, const uint8_t *h_stream, uint64_t stream_bytes, BgzfIndexed &ix, Between between)
{
    hipStream_t s = mi_host_stream(ctx);
    if (!ix.stream.alloc(stream_bytes + 64) || !ix.count.alloc(16)) return MI_ERR_NOMEM;
    if (stream_bytes) MI_HIP(ctx, hipMemcpyAsync(ix.stream.p, h_stream, stream_bytes, hipMemcpyHostToDevice, s));
    mi_status st = mi_bgzf_index_dev(ctx, ix.stream.as<uint8_t>(), stream_bytes, nullptr, 0, ix.count.as<uint64_t>(), s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpy(ix.cnt, ix.count.p, 16, hipMemcpyDeviceToHost));
    st = between();
    if (st) return st;
    if (!ix.members.alloc((ix.cnt[0] + 1) * 16)) return MI_ERR_NOMEM;
    return mi_bgzf_index_dev(ctx, ix.stream.as<uint8_t>(), stream_bytes, ix.members.as<uint64_t>(), ix.cnt[0], ix.count.as<uint64_t>(), s);
}

// copy in, index, inflate everything, copy out
extern "C" mi_status mi_bgzf_inflate(mi_ctx *ctx, const uint8_t *h_stream, uint64_t stream_bytes, uint8_t *h_out, uint64_t out_cap,
                                     uint64_t *h_out_bytes, uint32_t flags)
{
    if (!ctx || (stream_bytes && !h_stream) || (out_cap && !h_out)) return MI_ERR_ARG;
    if (flags & ~MI_INFLATE_NO_CHECKSUM) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    BgzfIndexed ix;
    DevBuf out;
    mi_status st = bgzf_index_host(ctx, h_stream, stream_bytes, ix, [&]() -> mi_status {
        if (ix.cnt[1] > out_cap) return MI_ERR_CAPACITY;
        return out.alloc(ix.cnt[1] + 16) ? MI_OK : MI_ERR_NOMEM;
    });
    if (st) return st;
    st = mi_bgzf_inflate_dev(ctx, ix.stream.as<uint8_t>(), stream_bytes, ix.members.as<uint64_t>(), 0, ix.cnt[0], out.as<uint8_t>(),
                             ix.cnt[1], flags, s);
    if (st) return st;
    if (ix.cnt[1]) MI_HIP(ctx, hipMemcpy(h_out, out.p, ix.cnt[1], hipMemcpyDeviceToHost));
    if (h_out_bytes) *h_out_bytes = ix.cnt[1];
    return MI_OK;
}

// copy up, index, read, copy down.  The bound on the pieces comes from the table itself: the members, empty ones included,
// between the first one that holds a byte of the range and the last.
extern "C" mi_status mi_bgzf_read_ranges(mi_ctx *ctx, const uint8_t *h_stream, uint64_t stream_bytes, uint64_t count,
                                         const uint64_t *h_off, const uint64_t *h_len, uint8_t *h_out, const uint64_t *h_out_off,
                                         uint64_t out_bytes, uint64_t *h_got, uint32_t *h_status, uint32_t flags)
{
    if (!ctx || (stream_bytes && !h_stream) || (out_bytes && !h_out)) return MI_ERR_ARG;
    if ((flags & ~MI_INFLATE_NO_CHECKSUM) || count > BGZR_MAX / 2u) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!h_off || !h_len || !h_out_off || !h_got || !h_status) return MI_ERR_ARG;
    hipStream_t s = mi_host_stream(ctx);
    const size_t arr = mi_align_up((size_t)count * 8u, 256);           // [off | len | out off | got | status]
    HostBuf h_members;
    DevBuf d_arr, d_out;
    BgzfIndexed ix;
    if (!d_arr.alloc(5 * arr) || !d_out.alloc(out_bytes + 16)) return MI_ERR_NOMEM;
    mi_status st = bgzf_index_host(ctx, h_stream, stream_bytes, ix, [&]() -> mi_status {
        if (ix.cnt[0] > BGZR_MAX) return MI_ERR_ARG;
        return h_members.alloc((ix.cnt[0] + 1) * 16) ? MI_OK : MI_ERR_NOMEM;
    });
    if (st) return st;
    MI_HIP(ctx, hipMemcpy(h_members.p, ix.members.p, (ix.cnt[0] + 1) * 16, hipMemcpyDeviceToHost));
    uint64_t max_pieces = 0;
    {
        // (the index's own table: its output offsets do not decrease)
        const uint64_t nm = ix.cnt[0], total = ix.cnt[1];
        auto o = [&](uint64_t m) { return h_members.as<uint64_t>()[2 * m + 1]; };
        for (uint64_t i = 0; i < count; ++i) {
            const uint64_t a = h_off[i], len = h_len[i];
            if (!len || a >= total) continue;
            const uint64_t b = len < total - a ? a + len : total;
            uint64_t lo = 0, hi = nm;                                   // the first member that ends behind a
            while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (o(mid + 1) > a) hi = mid; else lo = mid + 1; }
            const uint64_t m0 = lo;
            hi = nm;                                                    // the first member at or behind m0 that starts at or behind b
            while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (o(mid) >= b) hi = mid; else lo = mid + 1; }
            max_pieces += lo - m0;
        }
        if (max_pieces > BGZR_MAX) return MI_ERR_ARG;
    }
    uint8_t *da = d_arr.as<uint8_t>();
    MI_HIP(ctx, hipMemcpyAsync(da, h_off, count * 8, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(da + arr, h_len, count * 8, hipMemcpyHostToDevice, s));
    MI_HIP(ctx, hipMemcpyAsync(da + 2 * arr, h_out_off, count * 8, hipMemcpyHostToDevice, s));
    if (out_bytes) MI_HIP(ctx, hipMemcpyAsync(d_out.p, h_out, out_bytes, hipMemcpyHostToDevice, s));   // what lies between the slots stays
    st = mi_bgzf_read_ranges_dev(ctx, ix.stream.as<uint8_t>(), stream_bytes, ix.members.as<uint64_t>(), ix.cnt[0], count, (const uint64_t *)da,
                                 (const uint64_t *)(da + arr), d_out.as<uint8_t>(), (const uint64_t *)(da + 2 * arr), out_bytes, max_pieces,
                                 (uint64_t *)(da + 3 * arr), (uint32_t *)(da + 4 * arr), nullptr, flags, s);
    if (st) return st;
    MI_HIP(ctx, hipMemcpyAsync(h_got, da + 3 * arr, count * 8, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipMemcpyAsync(h_status, da + 4 * arr, count * 4, hipMemcpyDeviceToHost, s));
    if (out_bytes) MI_HIP(ctx, hipMemcpyAsync(h_out, d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    MI_HIP(ctx, hipStreamSynchronize(s));
    return MI_OK;
}
