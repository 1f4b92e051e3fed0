// internal.h — every function and limit one .hip file of libmi_codec.so defines and another uses, declared ONCE, by defining file
// (ctx.hip's are in common.h beside mi_ctx, the public extern "C" ones in include/mi_codec.h).  Users and definers include it.
// host_api.hip, the home of every host-buffer entry point, has no section: nothing it defines is called from another file.  The
// library links -shared, which accepts undefined symbols, and a definition that differs from its declaration is an overload to
// C++: a declaration that drifts shows as ONE undefined symbol the first time the library is loaded, whichever caller runs.
#pragma once
#include "lz_common.h"               // LzP, LzScratch, LzwScratch
#include "lz2.h"                     // Lz2Scratch

// ---- huffman.hip: the workspace of mi_huffman_encode_dev over n bytes (the measure of its carve)
size_t    huff_ws_bytes(uint64_t n);

// ---- lz_find.hip: parameters, workspace and the stages of the match finder
mi_status lz_check_params(const mi_lz_params *p);                      // parse 0 only
mi_status lz_check_fields(const mi_lz_params *p);                      // every field but `parse` (for defz_check, which takes parse 1 too)
// (what a call decides before it queues anything — LzSwitches, LzHint, LzPlan — is lz_plan.h: read once per call at the entry point)
void      lz_carve(mi_carver &cv, uint32_t nb, bool debug, LzScratch *sc, Lz2Scratch *sc2);   // one scratch set; sets are multiples of 4096
LzHint    lz_hint_read(const mi_ctx *ctx);
mi_status lz_find_stage_a(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                          const LzScratch &sc, const Lz2Scratch &sc2, hipStream_t s, hipStream_t sf, hipEvent_t ev_part, hipEvent_t ev_fb,
                          hipEvent_t ev_wide, const LzPlan &plan);
mi_status lz_find_stage_b(mi_ctx *ctx, const LzP &P, uint32_t nb, const Lz2Scratch &sc2, hipStream_t s, int which, const LzPlan &plan);

// ---- lz2_partition.hip, lz2_find.hip: the LDS-resident finder
void      lz2_launch_partition(const uint8_t *d_in, uint64_t n, const LzP &P, const Lz2Scratch &sc, uint64_t block0, uint32_t nb, hipStream_t s);
void      lz2_carve(mi_carver &cv, uint32_t nb, bool debug, Lz2Scratch *sc);                  // debug: the phase counters are carved
void      lz2_set_switches(Lz2Scratch *sc, const LzSwitches &sw);                             // wave_min, prefix, stop_phase of a carved set
mi_status lz2_stage_partition(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                              const Lz2Scratch &sc, hipStream_t s);
mi_status lz2_stage_find(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                         const Lz2Scratch &sc, hipStream_t s);
mi_status lz2_stage_find_wide(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                              const Lz2Scratch &sc, hipStream_t s, bool aside, const LzPlan &plan);
mi_status lz2_stage_b(mi_ctx *ctx, const LzP &P, uint32_t nb, const Lz2Scratch &sc, hipStream_t s, int which, const LzPlan &plan);
void      lz2_launch_scatter(const Lz2Scratch &sc, uint16_t *cand_by_pos, uint32_t nb, hipStream_t s);

// ---- lzw.hip: the lz77 flavour on blocks above 64 KiB
mi_status lzw_reserve(mi_ctx *ctx, uint32_t *nb, uint32_t block, LzwScratch *sc, uint64_t **base_bits);   // measures, halves *nb on MI_ERR_NOMEM, places
uint32_t  lzw_batch_blocks(mi_ctx *ctx, uint64_t nblocks, uint32_t block);
mi_status lzw_or_lzs_find(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb, const LzwScratch &sc, hipStream_t s,
                          const LzSwitches &sw);
void      lzw_launch_parse_emit(const uint8_t *d_in, uint64_t n, const LzP &P, const LzwScratch &sc, uint64_t block0, uint32_t nb, hipStream_t s);

// ---- lzs.hip: the time-sliced LDS-resident finder for those blocks
bool      lzs_applicable(const LzP &P, bool sliced);                       // sliced: MI_LZW_SLICED
mi_status lzs_find(mi_ctx *ctx, const LzP &P, const uint8_t *d_in, uint64_t n, uint64_t block0, uint32_t nb,
                   const LzwScratch &ws, hipStream_t s, uint32_t *flagged, const uint32_t **flag_list, const LzSwitches &sw);

// ---- lz_decode.hip; lz_emit.hip: block sizes -> offsets in place and the published table, the block decoder without its closing
// status read (host_api.hip launches one per chunk)
void      lz_launch_decode(const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_block_bits, const LzP &P, uint8_t *d_out,
                           uint64_t n, uint64_t nblocks, uint32_t *err, hipStream_t s);
void      lz_launch_scan_blocks(uint64_t *block_bits, uint32_t nb, const uint64_t *base_bits, uint64_t *excl_global, hipStream_t s);
mi_status mi_lz_decode_launch(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                              const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, uint32_t *err, hipStream_t s);

// ---- defh.hip: mode H — the entropy stage of one batch; the decoder without its closing status read
void      defh_launch_encode(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, uint32_t nb, const uint64_t *base_bits,
                             uint64_t *excl_global, uint8_t *d_out, uint64_t cap_bytes, hipStream_t s);
mi_status mi_deflate_h_decode_launch(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                                     const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, uint32_t *err, hipStream_t s);

// ---- defz.hip: mode Z (standard DEFLATE) — the entropy stage, the container's prologue (checksum) and epilogue
void      defz_launch_encode(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, const uint8_t *d_in, uint64_t n,
                             uint32_t block, uint64_t b0, uint32_t nb, bool desc, hipStream_t s, bool dict = false);
                             // desc: d_in is a descriptor table; dict: whose blocks may begin with bytes that are not the item's (LzBlkDesc.skip)
uint32_t  defz_header_bytes(uint32_t container);
uint32_t  defz_trailer_bytes(uint32_t container);
size_t    defz_ws_bytes();                                             // the checksum partials
mi_status defz_checksum(mi_ctx *ctx, bool crc, const uint8_t *d_in, uint64_t n, void *zws, uint32_t *d_res, hipStream_t s);   // zws: those
mi_status defz_check(const mi_lz_params *p, uint32_t container);
mi_status defz_begin(mi_ctx *ctx, uint32_t container, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t *base_bits,
                     void *zws, hipStream_t s);
mi_status defz_end(mi_ctx *ctx, uint32_t container, uint8_t *d_out, uint64_t *d_block_bits, uint64_t nblocks, uint64_t n,
                   void *zws, uint64_t *d_out_bytes, hipStream_t s);

// ---- lz_emit.hip: the encoder pipeline and the form of its output (lz_emit.hip describes the seven); deflate_batch.hip: what a batch
// adds to it — the descriptor table and per-block checksums in front, the placement of one pipeline batch's records, the per-item finish
enum LzForm { LZ_TOKENS, LZ_H, LZ_Z, LZ_BGZF, LZ_BATCH, LZ_SNAPPY, LZ_LZ4 };
struct DfbCall;
struct LzCall { LzForm form; uint32_t container; uint64_t *d_out_bytes; const DfbCall *batch; };   // container, d_out_bytes: LZ_Z, LZ_BGZF; batch: LZ_BATCH, LZ_SNAPPY, LZ_LZ4
mi_status lz_encode_impl(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap_bytes,
                         uint64_t *d_block_bits, void *stream, const LzCall &c);
struct DfbCall {
    uint32_t container; uint64_t count, max_blocks;
    const void *const *in; const uint64_t *in_bytes; void *const *out; const uint64_t *out_cap;
    uint64_t *out_bytes; uint32_t *status, *failed;
    // a preset dictionary (mi_deflate_batch_dict_dev; all zero without one).  ulen = |U|, the bytes of its tail an item's first block
    // is staged behind: that block holds block - ulen bytes of the item, the later ones `block` each (dfb_first / dfb_nblk below)
    const uint8_t *dict; uint64_t dict_bytes; uint32_t ulen;
    // the staging cells, filled in by lz_encode_impl once the pipeline's batches are known: block g of the table is block g % nbmax of
    // pipeline batch g / nbmax, which runs on scratch set (g / nbmax) % nsets — its cell is stage[that set] + (g % nbmax) * block
    uint32_t nbmax, nsets; uint8_t *stage[MI_SETS];
};
// the block layout of an item of nb bytes: bytes in its first block, its blocks, where block k starts and ends
__host__ __device__ static inline uint64_t dfb_first(uint64_t nb, uint32_t block, uint32_t ulen) { return nb < block - ulen ? nb : block - ulen; }
__host__ __device__ static inline uint64_t dfb_nblk(uint64_t nb, uint32_t block, uint32_t ulen)
{
    return nb == 0 ? 0 : 1u + (nb - dfb_first(nb, block, ulen) + block - 1u) / block;
}
__host__ __device__ static inline uint64_t dfb_begin_of(uint64_t k, uint32_t block, uint32_t ulen) { return k ? (uint64_t)(block - ulen) + (k - 1u) * block : 0; }
#define DFB_MAX_BYTES 0x7FFFFFFFull            // per item and per count: block numbers and positions inside an item are 32-bit
// DfbCall.container of LZ_SNAPPY (snappy_batch.hip): not a public container — every public entry point refuses a value above
// MI_CONTAINER_GZIP.  An item is its preamble, varint32(in_bytes), then its blocks' records: no 03 00, no trailer, no checksum.
#define DFB_SNAPPY    0x100u
__host__ __device__ static inline uint32_t dfb_varint_bytes(uint64_t v) { uint32_t k = 1; while (v >>= 7) ++k; return k; }
// DfbCall.container of LZ_LZ4 (lz4_batch.hip), as little public.  DFB_LZ4_BLOCK: an item is ONE block's record and nothing else (an
// item above the block size is MI_ERR_ARG, an empty one the byte 00).  DFB_LZ4_FRAME: the seven bytes of kDfbLz4Frame, every block's
// slot (size word and record, or size word and the block stored), the EndMark 00 00 00 00.
#define DFB_LZ4_BLOCK 0x101u
#define DFB_LZ4_FRAME 0x102u
size_t    dfb_ws_bytes(const DfbCall &b);
mi_status dfb_begin(mi_ctx *ctx, const DfbCall &b, uint32_t block, void *ws, hipStream_t s, const uint8_t **desc);
void      dfb_launch_place(const DfbCall &b, void *ws, const uint32_t *slots, const uint64_t *block_bits, uint64_t b0, uint32_t nb,
                           uint64_t seq, hipStream_t s);
mi_status dfb_end(mi_ctx *ctx, const DfbCall &b, uint32_t block, void *ws, hipStream_t s);
void      dfb_launch_stage(const DfbCall &b, uint32_t block, void *ws, uint64_t b0, uint32_t nb, hipStream_t s);   // U and the items' heads -> the cells
uint32_t  dfb_ulen(uint64_t dict_bytes, uint32_t block);                                                           // |U| = min(dict_bytes, 32 768, block / 2)
size_t    dfb_stage_bytes(const DfbCall &b, uint32_t nbmax, uint32_t block);                                       // per scratch set; 0 without a dictionary

// ---- snappy_batch.hip: the last stage of LZ_SNAPPY — one raw Snappy record per block in its slot, block_bits[lb] = 8 x its bytes
void      snappy_launch_emit(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, const uint8_t *d_desc, uint32_t block,
                             uint64_t b0, uint32_t nb, hipStream_t s);

// ---- lz4_batch.hip: the last stage of LZ_LZ4 — one LZ4 block record per block in its slot (frame: behind its size word, or the
// block stored), block_bits[lb] = 8 x the slot's bytes
void      lz4_launch_emit(const uint32_t *trec, uint32_t *slots, uint64_t *block_bits, const uint8_t *d_desc, uint32_t block,
                          uint64_t b0, uint32_t nb, bool frame, hipStream_t s);

// ---- inflate_batch.hip: the per-item limit
#define INFB_MAX_BYTES 0x7FFFFFFFull           // per item, compressed and inflated: positions inside an item are 32-bit

// ---- inflate.hip: k_inflate over segment descriptors (BGZF members) instead of a table of restart points
struct InfSeg { uint64_t first_bit, last_bit, out_off; uint32_t out_len, crc; };   // crc: the member's trailer, for bgzf.hip
void      inflate_launch_segments(const uint8_t *d_stream, uint64_t stream_bytes, const InfSeg *d_seg, uint32_t nseg, uint8_t *d_out,
                                  uint32_t *err, hipStream_t s, uint32_t *seg_status = nullptr);
// seg_status: one word per segment instead of `err` (which may then be NULL) — a segment whose word is not zero is skipped, one
// that fails sets its word to 1

// ---- bgzf.hip: the member framing of one batch of mode-Z records in their slots; the EOF member and the total; the CRC-32 of
// decoded members against their trailers, one workgroup per descriptor (seg_status as for inflate_launch_segments)
void      bgzf_launch_check(const uint8_t *d_out, const InfSeg *d_seg, uint32_t nseg, uint32_t *err, hipStream_t s,
                            uint32_t *seg_status = nullptr);
void      bgzf_launch_frame(uint32_t *slots, uint64_t *block_bits, const uint8_t *d_in, uint64_t n, uint32_t block, uint64_t b0,
                            uint32_t nb, hipStream_t s);
mi_status bgzf_end(mi_ctx *ctx, uint8_t *d_out, const uint64_t *d_member_bits, uint64_t nblocks, uint64_t *d_out_bytes, hipStream_t s);

// ---- bgzf_ranges.hip: the per-call limit
#define BGZR_MAX     0x7FFFFFFFull             // ranges, members and pieces per call: their numbers are 32-bit
