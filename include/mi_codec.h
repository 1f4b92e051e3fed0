/*
 * mi_codec.h — C ABI of the MI355X-native block-parallel compressor core
 * (libmi_codec.so: hand-written HIP kernels for gfx950 + this thin C layer).
 *
 * This is the drop-in boundary for the hot path of jdm365/Compression_Algorithms
 * (SURVEY.md section 8b).  Plain pointers and sizes only; no torch / C++ types.
 * Every entry point returns an mi_status instead of the reference's printf+exit(1).
 * The reference-NAMED wrappers (lz77_compress, huffman_compress, compress, ...) that a
 * maintainer links instead of the sources under algorithms/<dir>/ are declared in mi_lz77.h,
 * mi_huffman.h, mi_deflate.h and mi_fse.h; each is a few lines over the functions here.
 *
 * Pointer conventions
 *   d_*   device (HBM) pointers, caller-owned (hipMalloc / torch tensor.data_ptr()).
 *   h_*   host pointers.
 *   stream: a hipStream_t passed as void* (NULL = HIP's default stream, as everywhere in HIP).
 *           The host-buffer convenience calls use a private stream of the context.
 * Encoders (*_encode_dev, mi_huffman_hist/build/encode_with_tree_dev, mi_fse_normalise_dev) are asynchronous on `stream`.
 * Their scratch is the context workspace: it grows — hipDeviceSynchronize + hipFree + hipMalloc — only when a call needs
 * more than any earlier call of the context did; after a first call of the largest size a context will see, the encoders
 * neither allocate nor synchronise.  One encode per context may be in flight at a time (the workspace is shared; use one
 * context per concurrent stream).  The LZ encoders fork onto three internal streams of the context and join back into
 * `stream` with events before they return control of it.  One exception: the lz77 flavour on blocks above 64 KiB
 * synchronises `stream` once per batch of <= 256 MiB (it reads back whether a block needs the whole-block finder).
 * Decoders (*_decode_dev) synchronise `stream` before returning: MI_ERR_CORRUPT is decided on the device.  They take the
 * readable length of the stream and never read outside it, whatever an (untrusted) offset table says; every decode call
 * uses its own device status word, so decodes on different streams of one context do not interfere.
 * One exception: the batched inflate (mi_inflate_batch_dev, mi_inflate_batch_size_dev, their _dict twins) and the BGZF range read
 * (mi_bgzf_read_ranges_dev) are asynchronous on `stream` under the encoders' contract above — their verdicts are per item and stay on the device, so nothing needs a host round trip: scratch is
 * the context workspace, the calls allocate or synchronise only while it grows, one call per context in flight at a time.
 */
#ifndef MI_CODEC_H
#define MI_CODEC_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MI_OK = 0,
    MI_ERR_ARG = 1,            /* bad argument (NULL, size, params out of range)           */
    MI_ERR_HIP = 2,            /* a HIP call failed; mi_last_hip_error() has the code        */
    MI_ERR_NOMEM = 3,
    MI_ERR_CAPACITY = 4,       /* output buffer too small                                   */
    MI_ERR_EMPTY_INPUT = 5,    /* reference: "ERROR: Queue is empty" exit(1)  huffman.c:149-152 */
    MI_ERR_SINGLE_SYMBOL = 6,  /* reference: "ERROR: No code for character" exit(1) huffman.c:278-281 */
    MI_ERR_CODE_TOO_LONG = 7,  /* a Huffman code > 32 bits: the reference silently emits garbage (u32 code) */
    MI_ERR_CORRUPT = 8,        /* decoder: malformed stream                                  */
    MI_ERR_NO_DEVICE = 9,      /* no gfx950 device / HIP runtime: there is NO CPU fallback   */
    MI_ERR_UNSTABLE = 10,      /* a kernel found one of its sorts out of (key, time) order: see mi_order_violations */
    MI_ERR_TRANSPORT = 11      /* multi-device gather: RCCL missing or an RCCL call failed (mi_multi_last_transport_error) */
} mi_status;

typedef struct mi_ctx mi_ctx;

/* One context per process-and-GPU (one process per GPU is the deployment model). */
mi_status   mi_ctx_create(mi_ctx **out, int device_ordinal);
void        mi_ctx_destroy(mi_ctx *ctx);
const char *mi_status_str(mi_status s);
int         mi_last_hip_error(const mi_ctx *ctx);
const char *mi_version(void);
/* blocks until everything queued on `stream` has finished.  Returns MI_ERR_UNSTABLE once if an encoder kernel reported a
 * sort out of order since the last call (below): the stream it was building is valid but may not be the reference's. */
mi_status   mi_sync(mi_ctx *ctx, void *stream);
/* The match finders sort positions by bucket with LDS radix passes whose ranks come from returning LDS atomics — stable
 * only if the hardware serves the lanes of one such instruction in lane order.  gfx950 does (probed when the context is
 * created; MI_LZ_NO_ARANK=1 forces the ballot ranking), the ISA does not promise it, and an unstable sort would still
 * round-trip.  So every consumer of a sort checks its order, and a violation is never silent: it is counted here, the
 * context ranks with ballots from its next call on, mi_sync() returns MI_ERR_UNSTABLE once, and the host-buffer entry points
 * (mi_lz_encode, mi_deflate_h_encode — what the drop-ins call) encode again before they return.  A caller of the
 * asynchronous *_dev encoders re-encodes when mi_sync says so.  Returns the number of violations seen by this context. */
uint32_t    mi_order_violations(mi_ctx *ctx);
/* Host-side check of a block table (exclusive prefix of per-block stream lengths in BITS, nblocks+1 entries) that came
 * from a file or a peer: non-decreasing, every entry a multiple of align_bits (1: bit-packed lz77; 8: deflate tokens;
 * 32: mode-H and FSE records), last entry <= 8 * stream_bytes.  MI_OK or MI_ERR_CORRUPT.  The host-buffer decoders call
 * it themselves; callers of the *_dev decoders that hold the table on the host should. */
mi_status   mi_validate_block_table(const uint64_t *h_block_bits, uint64_t nblocks, uint64_t stream_bytes, uint32_t align_bits);

/* ------------------------------------------------------------------------------------
 * Huffman, whole buffer, one tree        replaces algorithms/huffman/huffman.c:288-328
 *   histogram (huffman.c:184-187) -> heap-exact tree (:189-211) -> tree-path codes
 *   (:217-250) -> MSB-first u32 words (:18-48)
 * ------------------------------------------------------------------------------------ */
typedef struct {
    uint64_t total_bits;
    uint64_t word_idx;          /* BitWriter.word_idx  = total_bits / 32                    */
    uint64_t bit_idx;           /* BitWriter.bit_idx   = total_bits % 32                    */
    uint64_t buffer_size;       /* BitWriter.buffer_size per huffman.c:318-320              */
    uint32_t n_symbols;
    uint32_t max_code_len;
    uint32_t status;            /* mi_status decided on the device (empty / single / too long) */
    uint32_t n_nodes;           /* tree nodes written to the tree arrays (<= 511)           */
} mi_huffman_info;

/* the tree in array form, node ids in creation order (leaves in symbol order, then merges);
 * root = n_nodes-1.  Mirrors the reference's Node{value,frequency,left,right}. */
typedef struct {
    uint32_t frequency[511];
    int16_t  left[511];         /* -1 for a leaf */
    int16_t  right[511];
    uint8_t  value[511];
    uint8_t  pad;
    uint32_t code[256];
    uint8_t  length[256];
} mi_huffman_tree;

/* words needed for n input bytes in the worst case the ABI accepts (codes <= 32 bits) */
static inline uint64_t mi_huffman_bound_words(uint64_t n) { return n + 2; }

/* d_words must hold cap_words u32 (>= ceil(bits/32)+1).  Words [0, ceil(bits/32)) are fully defined
 * (unused low bits of the last one are 0, as after init_bitwriter's memset); words past that are not touched.
 * d_info / d_tree are device buffers of sizeof(mi_huffman_info) / sizeof(mi_huffman_tree). */
#define MI_HUFFMAN_TILE 32768u   /* input bytes per encoder tile (one sync point each) */
/* d_tile_off (optional, may be NULL): u64[ceil(n/MI_HUFFMAN_TILE)+1], bit offset at which each
 * tile's codes start — the only sync points a variable-length code has; the parallel decoder
 * needs them, the reference format has no place for them. */
mi_status mi_huffman_encode_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n,
                                uint32_t *d_words, uint64_t cap_words,
                                mi_huffman_info *d_info, mi_huffman_tree *d_tree,
                                uint64_t *d_tile_off, void *stream);
/* host-buffer convenience: copies in, encodes, copies out, synchronises. h_words: cap_words u32. */
mi_status mi_huffman_encode(mi_ctx *ctx, const uint8_t *h_in, uint64_t n,
                            uint32_t *h_words, uint64_t cap_words,
                            mi_huffman_info *h_info, mi_huffman_tree *h_tree);
/* decode exactly n symbols with the tree arrays; replaces huffman.c:330-364.  With d_tile_off
 * (from the encoder) one lane per tile; with NULL a single lane walks the whole stream.
 * d_words needs one readable word past the stream.  Synchronises (returns MI_ERR_CORRUPT). */
mi_status mi_huffman_decode_dev(mi_ctx *ctx, const uint32_t *d_words, uint64_t total_bits,
                                const mi_huffman_tree *d_tree, uint32_t n_nodes,
                                const uint64_t *d_tile_off, uint8_t *d_out, uint64_t n, void *stream);

/* host-buffer decode (copies in/out, synchronises).  h_tile_off may be NULL (single-lane decode). */
mi_status mi_huffman_decode(mi_ctx *ctx, const uint32_t *h_words, uint64_t total_bits,
                            const mi_huffman_tree *h_tree, uint32_t n_nodes,
                            const uint64_t *h_tile_off, uint8_t *h_out, uint64_t n);
/* like mi_huffman_encode, also returning the tile offsets (h_tile_off: u64[ceil(n/MI_HUFFMAN_TILE)+1] or NULL) */
mi_status mi_huffman_encode2(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, uint32_t *h_words, uint64_t cap_words,
                             mi_huffman_info *h_info, mi_huffman_tree *h_tree, uint64_t *h_tile_off);

/* The same encoder in three steps, for ONE tree over a buffer spread over several GPUs (whole-buffer parity across
 * ranks: huffman.c:179-215 builds one tree over the whole buffer, :267-328 packs with it).  Per rank:
 *   mi_huffman_hist_dev   shard -> d_hist u64[256] (+ d_tile_hist u32[mi_huffman_num_tiles(n)][256], kept by the caller)
 *   -- all-reduce (sum) of d_hist over the ranks: 2 KiB --
 *   mi_huffman_build_dev  summed histogram (taken modulo 2^32 like the reference's u32 counters) -> tree, codes, status
 *   -- bits of a shard = sum(hist[s] * length[s]); an all-gather of those gives every shard its global bit offset --
 *   mi_huffman_encode_with_tree_dev  shard -> words; the stream starts bit_offset (= global offset mod 32) bits into
 *                         d_words[0]; d_info->total_bits = bit_offset + the shard's bits; d_tile_off (optional)
 *                         are offsets relative to d_words[0].  MI_ERR_ARG in d_info->status if the shard holds a
 *                         byte the tree has no code for.
 * Shard word ranges overlap by one word at a seam; OR-ing them there yields the single-GPU stream bit for bit
 * (compression_algorithms_amd/sharded.py does the exchange over torch.distributed / RCCL). */
uint64_t  mi_huffman_num_tiles(uint64_t n);
mi_status mi_huffman_hist_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t *d_hist, uint32_t *d_tile_hist, void *stream);
mi_status mi_huffman_build_dev(mi_ctx *ctx, const uint64_t *d_hist, mi_huffman_info *d_info, mi_huffman_tree *d_tree, void *stream);
mi_status mi_huffman_encode_with_tree_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n, const mi_huffman_tree *d_tree,
                                          const uint32_t *d_tile_hist, uint32_t bit_offset, uint32_t *d_words, uint64_t cap_words,
                                          mi_huffman_info *d_info, uint64_t *d_tile_off, void *stream);

/* host-buffer forms of the steps (the drop-in's build_huffman_tree and _huffman_compress, huffman.c:179-215, :267-285) */
mi_status mi_huffman_build(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, mi_huffman_info *h_info, mi_huffman_tree *h_tree);
mi_status mi_huffman_encode_with_codes(mi_ctx *ctx, const uint8_t *h_in, uint64_t n, const uint32_t *h_codes,
                                       const uint8_t *h_lengths, uint32_t bit_offset, uint32_t *h_words, uint64_t cap_words,
                                       mi_huffman_info *h_info);

/* ------------------------------------------------------------------------------------
 * LZ77 greedy tokenisers, block-parallel.
 *   deflate flavour: algorithms/deflate/lz77.c:199-280 per block of `block` bytes with a
 *     FRESH table per block (the sharded parity definition); byte tokens
 *     {0,c} / {1,dlo,dhi,len} (lz77.c:176-197).
 *   lz77 flavour: algorithms/lz77/lz77.c:264-345 per block; LSB-first bit tokens
 *     1+8 / 1+wbits+lbits (lz77.c:290-330).
 * A block is encoded as if followed by zero bytes (the reference reads past `size`).
 * ------------------------------------------------------------------------------------ */
typedef struct {
    uint32_t wbits;       /* window bits: lz77 14 (shipped) or 16; deflate 15             */
    uint32_t lbits;       /* length bits: lz77 4; deflate 5                               */
    uint32_t tbits;       /* log2 table size: lz77 wbits+6; deflate 20                    */
    uint32_t deflate;     /* 1: deflate rules (insert probe wraps, literal iff p-m >= W-1, byte tokens) */
    uint32_t block;       /* block size in bytes: 1..65536; lz77 flavour also 65792..1048576 in steps of 256 —
                           * the HBM-resident finder of lzw.hip, where a 64 KiB window really slides (exact, slower) */
    uint32_t parse;       /* MI_PARSE_REFERENCE (0, what every initialiser below leaves): the reference's greedy parse.
                           * MI_PARSE_LAZY (1): mode Z's lazy parse with matches up to 255 bytes — the standard-DEFLATE
                           * writers only (mode Z, BGZF, the batched deflate); MI_ERR_ARG everywhere else */
} mi_lz_params;
#define MI_PARSE_REFERENCE 0
#define MI_PARSE_LAZY      1

static inline mi_lz_params mi_lz_params_deflate(void) { mi_lz_params p = {15, 5, 20, 1, 65536, MI_PARSE_REFERENCE}; return p; }
static inline mi_lz_params mi_lz_params_lz77(uint32_t wbits) { mi_lz_params p = {wbits, 4, wbits + 6, 0, 65536, MI_PARSE_REFERENCE}; return p; }
/* the deflate flavour with the parse chosen: mi_lz_params_deflate_parse(MI_PARSE_LAZY) for mode Z, BGZF and the batched deflate */
static inline mi_lz_params mi_lz_params_deflate_parse(uint32_t parse) { mi_lz_params p = {15, 5, 20, 1, 65536, parse}; return p; }

static inline uint64_t mi_lz_num_blocks(uint64_t n, const mi_lz_params *p) { return (n + p->block - 1) / p->block; }
/* bound on the concatenated stream, in bytes.  Per block: every byte a literal (2 bytes / 9 bits), except that the
 * block's LAST token may be a match that covers a single real byte and runs on into the zero tail the reference
 * reads past `size`: that match costs 4 bytes (deflate) or 1+wbits+lbits bits (lz77) instead of
 * one literal — +2 bytes / +(wbits+lbits-8) bits per block. */
static inline uint64_t mi_lz_bound_bytes(uint64_t n, const mi_lz_params *p)
{
    const uint64_t nblocks = p->block ? (n + p->block - 1) / p->block : 0;
    if (p->deflate) return 2 * n + 2 * nblocks + 8;
    return (9 * n + nblocks * (uint64_t)(p->wbits + p->lbits - 8) + 7) / 8 + 16;
}

/*
 * Encode n bytes at d_in as ceil(n/block) independent blocks.
 *   d_out        concatenated stream: deflate flavour = byte tokens of block 0,1,2,...;
 *                lz77 flavour = the blocks' bit streams concatenated bit-contiguously
 *                (block b starts at bit d_block_bits_excl[b]); zero-filled by the call.
 *   d_block_bits u64[nblocks+1]: EXCLUSIVE prefix sum of per-block stream lengths in BITS
 *                (deflate: 8 * bytes); entry nblocks = total.
 */
mi_status mi_lz_encode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                           uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, void *stream);
mi_status mi_lz_encode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_in, uint64_t n,
                       uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits);
/* decode; every block is truncated at its original length (an overshooting last match, A.3.4).
 * stream_bytes = readable bytes at d_stream: the kernel never reads outside [d_stream, d_stream + stream_bytes) and
 * never outside a block's own bit range, whatever the table says.  Like every decoder of this ABI it synchronises
 * `stream` before returning (MI_ERR_CORRUPT is decided on the device). */
mi_status mi_lz_decode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                           const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, void *stream);

/* host buffers: the table is validated (mi_validate_block_table) before anything is copied; above one chunk (4 096
 * blocks) the stream goes up and the bytes come down chunk by chunk around the decoder.  On MI_ERR_CORRUPT h_out may hold
 * the chunks decoded before the bad block. */
mi_status mi_lz_decode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_stream, uint64_t stream_bytes,
                       const uint64_t *h_block_bits, uint8_t *h_out, uint64_t n);

/* debugging / parity hooks used by the tests: find() at every position of every block
 * (0xFFFF = none), i.e. the output of the match-finder stage alone. */
mi_status mi_lz_find_all_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                             uint16_t *d_cand, void *stream);
/* the same for blocks above 64 KiB (lz77 flavour only): 32-bit positions, 0xFFFFFFFF = none */
mi_status mi_lz_find_all32_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                               uint32_t *d_cand, void *stream);

/* The reference's first, brute-force parser — lz77_compress_old, algorithms/lz77/lz77.h:51-54, lz77.c:185-262 (its call is
 * commented out at lz77/main.c:26): the whole window of 2^wbits - 1 bytes is searched at every token start, first-longest
 * match wins, ONE stream over the whole buffer in lz77_compress's token format.  O(n * 2^wbits) by definition; on the GPU
 * the best match of every position is found independently (lz_old.hip).  d_out: mi_lz77_old_bound_bytes(n) bytes, 4-byte
 * aligned, zeroed by the call; *total_bits = the reference's bit_index (the stream is total_bits / 8 + 1 bytes, lz77.c:258).
 * wbits 8..16, lbits 3..5 (the reference: 14, 4).  mi_lz77_whole_decode* decodes a whole-buffer stream (this parser's, or
 * lz77_compress's for a buffer of one block): lz77.c:347-377 on one wave; n < 2^32. */
uint64_t  mi_lz77_old_bound_bytes(uint64_t n);
mi_status mi_lz77_old_encode_dev(mi_ctx *ctx, uint32_t wbits, uint32_t lbits, const uint8_t *d_in, uint64_t n,
                                 uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_total_bits, void *stream);
mi_status mi_lz77_old_encode(mi_ctx *ctx, uint32_t wbits, uint32_t lbits, const uint8_t *h_in, uint64_t n,
                             uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_total_bits);
mi_status mi_lz77_whole_decode_dev(mi_ctx *ctx, uint32_t wbits, uint32_t lbits, const uint8_t *d_stream, uint64_t stream_bytes,
                                   uint64_t total_bits, uint8_t *d_out, uint64_t n, void *stream);
mi_status mi_lz77_whole_decode(mi_ctx *ctx, uint32_t wbits, uint32_t lbits, const uint8_t *h_stream, uint64_t stream_bytes,
                               uint64_t total_bits, uint8_t *h_out, uint64_t n);

/* ------------------------------------------------------------------------------------
 * Deflate "mode H": the entropy stage algorithms/deflate/lz77.c:279 leaves as a TODO
 * ("Build huffman tree and encode compressed buffer").  The token sequence is the
 * reference's (same finder and parse as mi_lz_encode_dev with deflate = 1); each block's
 * tokens are then coded with a dynamic Huffman code over the reference's 286-symbol
 * alphabet (deflate/huffman.h:6, huffman.c:49-62), lengths from the reference's heap
 * procedure (algorithms/huffman/huffman.c:100-163), canonical code assignment, MSB-first
 * u32 packing (deflate/huffman.c:16-46).  The reference has no such encoder: the bit
 * stream is defined by this build (oracle/orc_defh.c restates it).
 *
 * Block record (4-byte aligned): u32 n_tokens | u8 len[286] + 2 pad | u32 words[]
 *   literal b -> code[b];  match (d, l) -> code[256 + clz16(d)], the 15 - clz16(d) offset
 *   bits below d's leading one, the 5-bit length.
 * d_block_bits u64[nblocks+1]: exclusive prefix of record lengths in BITS (multiples of 32).
 * p must be a deflate-flavour parameter set with lbits <= 5 and wbits <= 16.
 * ------------------------------------------------------------------------------------ */
/* worst case of the concatenated records: per block the 292-byte header plus 9 bits per byte (a Huffman code is never
 * longer than the fixed 9-bit code over 286 symbols) plus one overshooting last match (<= 20 extra bits), word aligned */
uint64_t  mi_deflate_h_bound_bytes(uint64_t n, const mi_lz_params *p);
mi_status mi_deflate_h_encode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n,
                                  uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, void *stream);
mi_status mi_deflate_h_decode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_stream, uint64_t stream_bytes,
                                  const uint64_t *d_block_bits, uint8_t *d_out, uint64_t n, void *stream);
mi_status mi_deflate_h_encode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_in, uint64_t n,
                              uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits);
mi_status mi_deflate_h_decode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_stream, uint64_t stream_bytes,
                              const uint64_t *h_block_bits, uint8_t *h_out, uint64_t n);

/* ------------------------------------------------------------------------------------
 * Deflate "mode Z": standard DEFLATE (RFC 1951), raw or in a zlib (RFC 1950) / gzip (RFC 1952)
 * container — what zlib's inflate, gzip -d and HTTP stacks read.
 *
 * Tokens: per input block of p->block bytes exactly the token sequence of mi_lz_encode_dev
 * (deflate flavour: same finder, same parse, fresh table per block), with one change: a last
 * match that runs past the block end (A.3.4) is clipped to L' = block_end - pos, a match of L'
 * if L' >= 3, else L' literals read from the input.  Lengths -> codes 257..285, distances ->
 * codes 0..29, with their extra bits.
 * One RECORD per input block: DEFLATE blocks with BFINAL = 0 coding exactly that block, then an
 * empty stored block (3 header bits, padding to a byte, 00 00 FF FF: a sync flush), so a record is
 * whole bytes, starts on a byte boundary and never refers to an earlier block.  The block type is
 * the shortest in bits of dynamic Huffman (BTYPE 10), fixed Huffman (01) and stored (00), ties in
 * that order, all three sized exactly from the histograms; a stored block of 65 536 bytes is two
 * stored blocks (LEN <= 65 535).  Sizes in bits (end-of-block counted in both Huffman forms):
 *   dynamic  3 + 14 + 3 HCLEN + code-length symbols with their extra bits + tokens with extra bits
 *   fixed    3 + tokens with extra bits in the fixed code
 *   stored   40 ceil(n / 65535) + 8 n
 * Codes: literal/length and distance lengths <= 15, code-length lengths <= 7, every code complete.
 * The lengths are the mode-H heap's (leaves in symbol order) over the block's tally, end-of-block
 * always counted.  A code with fewer than two used symbols gets two codes of length 1 as zlib's
 * build_tree pads: none used -> symbols 0 and 1; one used, s -> s and s + 1 if s < 2, else s and 0.
 * Where a length exceeds the limit L (15; 7 for the code-length code): every length above L is
 * clamped to L; while the Kraft sum exceeds 1, one code moves a level down, from the deepest level
 * l < L that has one (l >= 1); while it is below 1, one code moves a level up, from the deepest
 * level l <= L (l >= 2) that has one and whose step 2^-l still fits; the level counts are then dealt
 * out to the used symbols in (unlimited length, symbol) order, the shortest level first.
 * Header: HLIT is trimmed while > 257 and the last literal/length length is 0, HDIST while > 1 and
 * the last distance length is 0, HCLEN while > 4 and the last code-length length in RFC order is 0.
 * The HLIT + HDIST lengths are run-length coded as ONE sequence: a run of r zeros as 18s of
 * min(r, 138) while r >= 11, then one 17 if r >= 3; a run of r copies of v != 0 as v, then 16s of
 * min(rest, 6) while rest >= 3; whatever is left of a run is written as plain lengths.  The stream
 * ends with 03 00 (a final fixed block with only end-of-block); for n = 0 the raw stream is just
 * 03 00.  oracle/orc_defz.c restates all of this on the CPU; the encoder gives its bytes.
 * Parse 1 (p->parse == MI_PARSE_LAZY; wbits 15, lbits 5): other tokens, everything behind them as above.  Per block of n
 * bytes, skip = the bytes of a preset dictionary's tail in front of an item's first block (else 0), cand[p] the finder's
 * answer at p as for parse 0:
 *   len0(p) = 0 if there is no candidate or p - cand[p] >= 32767 (the literal rule, unchanged); else the length l of the
 *             common prefix of in[cand[p]..] and in[p..], at most min(255, n - p) — no byte at or past n is compared, no
 *             match runs past the block, so nothing is ever clipped; 0 if l < 3.  len0(n) = 0.
 *   eff(p)  = 0 if len0(p) == 0 or len0(p + 1) > len0(p) (a one-step lazy rule: the longer match one byte on wins),
 *             else len0(p).
 *   walk:     p = skip; while p < n: eff(p) ? match (eff(p), p - cand[p]), p += eff(p) : literal in[p], p += 1.
 * The streams are standard DEFLATE as before and smaller (text about 2 %, zero pages and runs several times); they
 * are no longer the reference's tokens.  The bounds do not change: stored is still the ceiling.
 * Containers: MI_CONTAINER_RAW the above; MI_CONTAINER_ZLIB 78 9C, the raw stream, Adler-32
 * big-endian; MI_CONTAINER_GZIP 1F 8B 08 00 00 00 00 00 00 FF (no flags, MTIME 0, OS 255: the
 * output is reproducible), the raw stream, CRC-32 little-endian, ISIZE = n mod 2^32 little-endian.
 * d_block_bits u64[nblocks+1]: entry b is the bit offset in d_out where record b starts (the
 * container header included, so entry 0 is 0, 16 or 80; all multiples of 8); entry nblocks is where
 * the final 03 00 starts.  Every record can be inflated on its own from there: restart points.
 * *d_out_bytes: the total length in bytes (on the device, like the table).
 * p: deflate flavour with wbits <= 15, lbits <= 8, block <= 65 536, parse 0 or 1 (1: wbits 15 and
 * lbits 5); anything else, or an unknown container, is MI_ERR_ARG.  d_out 4-byte aligned; cap_bytes below mi_deflate_z_bound_bytes is
 * MI_ERR_CAPACITY.
 * ------------------------------------------------------------------------------------ */
#define MI_CONTAINER_RAW  0u
#define MI_CONTAINER_ZLIB 1u
#define MI_CONTAINER_GZIP 2u
/* per block of b bytes b + 5 ceil(b / 65535) + 5 (the stored form and its sync flush), plus the container's header and
 * trailer (raw 0, zlib 2 + 4, gzip 10 + 8) and the closing 03 00 */
uint64_t  mi_deflate_z_bound_bytes(uint64_t n, const mi_lz_params *p, uint32_t container);
mi_status mi_deflate_z_encode_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, const uint8_t *d_in, uint64_t n,
                                  uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_block_bits, uint64_t *d_out_bytes, void *stream);
/* host buffers: copy in, encode, copy out; h_block_bits u64[nblocks+1]; *h_out_bytes (may be NULL) = bytes written */
mi_status mi_deflate_z_encode(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, const uint8_t *h_in, uint64_t n,
                              uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits, uint64_t *h_out_bytes);
/* the checksums of the containers on their own (zlib's crc32 / adler32 of the whole buffer), asynchronous on `stream`:
 * per-workgroup partials, then one combine step; the result is one u32 on the device.  The partials live in the context
 * workspace like every encoder's scratch (8 KiB): one call of a context in flight at a time, as for the encoders.
 * Inside mi_deflate_z_encode_dev the checksum runs on `stream` ahead of the LZ pipeline (~0.5 ms for 10^9 bytes). */
mi_status mi_crc32_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t *d_crc, void *stream);
mi_status mi_adler32_dev(mi_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t *d_adler, void *stream);

/* ------------------------------------------------------------------------------------
 * Inflate: standard DEFLATE read back on the GPU from a table of restart points — a mode-Z
 * stream with the table its encoder wrote, or any stream cut the same way (stock zlib with
 * Z_FULL_FLUSH every `block` input bytes: INTEGRATION.md has the recipe).
 *
 * d_seg_bits u64[nseg+1], nseg = ceil(n / block): entry s is the bit offset in d_stream where
 * SEGMENT s starts (entry 0 = the end of the container header: 0 for raw, 16 for zlib, 8 * the
 * header length for gzip), entry nseg where the closing part starts; all multiples of 8.  It is
 * exactly the d_block_bits of mi_deflate_z_encode_dev, so a mode-Z stream decodes with the
 * arguments it was encoded with.  `block` is a plain number, 1 .. 2^31 - 1 (positions inside a
 * segment are 32-bit); n = 0 is legal (no segment: only the frame is checked).
 * Segment s: whole DEFLATE blocks with BFINAL = 0, of any type (stored, fixed, dynamic; the full
 * RFC 1951 alphabet: lengths to 258, distances to 32 768, codes to 15 bits), that use the bits
 * [entry s, entry s+1) exactly and inflate to exactly the bytes [s * block, min((s+1) * block, n))
 * without referring to anything before them.  One wave decodes it.
 * Closing part, from entry nseg: blocks that produce no bytes (stored with LEN = 0, or fixed with
 * end-of-block alone; an empty dynamic block is not accepted there), the last with BFINAL = 1 —
 * mode Z and zlib write 03 00 — then at the next byte boundary the trailer: none (raw), Adler-32
 * big-endian (zlib), CRC-32 and ISIZE = n mod 2^32 little-endian (gzip); the stream ends exactly
 * there (stream_bytes).
 * One relaxation: in a one-segment call (nseg == 1) the BFINAL = 1 block may be the segment's
 * last block; entry 1 is then the end of the DEFLATE data (the byte after its last bit) and the
 * closing part is empty.  zlib.compress(x) writes that.  A stream without a table is one segment
 * (block >= n): correct, and slow — one wave.
 * Header: raw none; zlib CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0, FDICT = 0; gzip 1F 8B,
 * CM = 8, reserved flag bits zero, FEXTRA / FNAME / FCOMMENT / FHCRC skipped by their lengths
 * (FHCRC not verified).
 * MI_ERR_CORRUPT: a table entry that is not a multiple of 8, decreasing or past the stream; a
 * segment that uses more or fewer bits than it has or produces more or fewer bytes than its range;
 * BTYPE 11; a stored block whose NLEN is not ~LEN; HLIT > 286 or HDIST > 30; an over-subscribed
 * code; an incomplete code (except a distance code with a single code of length 1, or with no
 * code at all in a block of literals); no end-of-block code; a repeat (16) with no previous
 * length or a run past HLIT + HDIST; symbols 286, 287, distance codes 30, 31; a distance reaching
 * before the segment's first byte; BFINAL = 1 inside a segment (but see above); a header, closing
 * part or trailer other than described; ISIZE != n mod 2^32; a checksum that differs from that of
 * the decoded bytes (mi_crc32_dev / mi_adler32_dev run after the inflate kernel and are compared
 * on the device) unless MI_INFLATE_NO_CHECKSUM is set.
 * MI_ERR_ARG: NULL pointers, an unknown container, block 0 or above 2^31 - 1, d_stream not 4-byte
 * aligned, unknown flag bits.
 * Reads stay inside [d_stream, d_stream + stream_bytes) rounded out to whole aligned 4-byte words
 * and inside the segment's own bits whatever the (untrusted) table says; writes inside the
 * segment's own output range; every loop is bounded by the segment's bit or byte count.
 * mi_inflate_dev synchronises `stream` before returning; it uses the context workspace (8 KiB of
 * checksum partials): one call of a context in flight at a time.
 * Out of scope here: finding restart points in a stream that comes without a table and
 * multi-member gzip — BGZF (below) is the answer to both: members that carry their own sizes;
 * generic multi-member gzip without 'BC' subfields stays out of scope — preset dictionaries,
 * MI_FRAME_* packing of mode Z, the multi-GPU path.
 * ------------------------------------------------------------------------------------ */
#define MI_INFLATE_NO_CHECKSUM 1u   /* skip the Adler-32 / CRC-32 comparison (ISIZE and the frame are still checked) */
mi_status mi_inflate_dev(mi_ctx *ctx, uint32_t container, uint32_t block, const uint8_t *d_stream, uint64_t stream_bytes,
                         const uint64_t *d_seg_bits, uint8_t *d_out, uint64_t n, uint32_t flags, void *stream);
/* host buffers: the table is validated (mi_validate_block_table, 8-bit alignment) before anything is copied; copy in,
 * decode, copy out, in one piece */
mi_status mi_inflate(mi_ctx *ctx, uint32_t container, uint32_t block, const uint8_t *h_stream, uint64_t stream_bytes,
                     const uint64_t *h_seg_bits, uint8_t *h_out, uint64_t n, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * BGZF: the blocked gzip of bgzip / htslib / samtools / tabix (SAM specification, 4.1) — a
 * sequence of complete, independent gzip members of at most 65 536 bytes, compressed and
 * uncompressed, each carrying its own size.  gzip -d, zcat, Python's gzip module and HTTP
 * stacks read it as plain multi-member gzip; the GPU reads it back with no side table.
 *
 * Written: member b holds input block b of p->block bytes —
 *   1F 8B 08 04 00 00 00 00 00 FF 06 00 42 43 02 00   gzip, CM 8, FLG = FEXTRA, MTIME 0, XFL 0, OS 255
 *                                                     (reproducible, like mode Z's gzip), XLEN 6, 'B' 'C', SLEN 2
 *   BSIZE u16 little-endian                            the member's total bytes - 1
 *   mode Z's RECORD of block b, unchanged              same tokens, clip, limiter, header rules, block-type choice
 *   03 00                                              the final fixed block with end-of-block alone
 *   CRC-32 of the block's input bytes, ISIZE = the block's length, both u32 little-endian
 * then the 28-byte EOF member 1F 8B 08 04 00 00 00 00 00 FF 06 00 42 43 02 00 1B 00 03 00 and eight
 * zero bytes.  For n = 0 the stream is that member alone.  A member is its record + 28 bytes.
 * p: mode Z's constraints and block <= MI_BGZF_MAX_BLOCK, anything else MI_ERR_ARG: the stored form
 * of such a block, the longest a record gets, makes a member of at most 65 536 bytes, so BSIZE
 * always fits (no run-time check).  d_member_bits u64[nblocks+1]: entry b is the bit offset of
 * member b's first byte (entry 0 is 0), entry nblocks that of the EOF member.  *d_out_bytes: the
 * total length.  d_out 4-byte aligned; cap_bytes below mi_bgzf_bound_bytes is MI_ERR_CAPACITY.
 * Asynchronous, no allocation once the workspace has grown: the encoders' contract (top of file).
 *
 * Index (mi_bgzf_index_dev): from offset 0 every member is read as
 *   1F 8B, CM = 8, FLG = 4 exactly (any other flag bit is MI_ERR_CORRUPT); MTIME, XFL, OS ignored;
 *   any XLEN; its subfields (SI1 SI2 SLEN data) in turn — the first 'B' 'C' with SLEN = 2 that lies
 *   inside the XLEN bytes gives BSIZE; a subfield that runs past XLEN ends the search; none found
 *   is MI_ERR_CORRUPT;
 *   BSIZE + 1 >= XLEN + 12 + 2 + 8, and the member lies inside the stream;
 *   ISIZE = its last four bytes, at most 65 536.
 * The next member starts BSIZE + 1 bytes on; the stream must end exactly at a member's end (an
 * empty stream has no members).  An EOF member is not required; empty members may stand anywhere.
 * d_stream 4-byte aligned (the chunk scan reads aligned words), else MI_ERR_ARG, as for inflate.
 * d_members u64[2 * (cap_members + 1)]: members + 1 pairs (stream byte offset, output byte offset),
 * the last one (stream_bytes, total) — the content of htslib's .gzi.  d_members = NULL only counts.
 * d_count u64[2]: members, total output bytes (both 0 on MI_ERR_CORRUPT).  More members than
 * cap_members is MI_ERR_CAPACITY (d_count is valid, the pairs below cap_members are written).
 * The result is that of the serial walk from offset 0 for every input — also where stored blocks
 * hold byte-exact member headers (a BGZF file compressed again): the kernels guess a way into
 * every 128 KiB of the stream in parallel, and a guess stands only once the walk from the chunk
 * before it arrives exactly there; otherwise that chunk is walked again from where it did arrive.
 *
 * Inflate (mi_bgzf_inflate_dev): members [first_member, first_member + n_members) of the table
 * (which holds at least first_member + n_members + 1 pairs) are written to d_out, member m at
 * its output offset less that of first_member; out_bytes must be the range's size (an empty range:
 * out_bytes = 0, else MI_ERR_ARG).  Random access by member.  Per member the header is read again
 * as above and must agree with the table (BSIZE + 1 = the distance to the next pair, ISIZE = the
 * output distance); the DEFLATE data must occupy exactly the bytes between header and trailer, end
 * in a BFINAL = 1 block (its only one), inflate to exactly ISIZE bytes and refer to nothing before
 * the member; all block types and the whole RFC 1951 alphabet, as mi_inflate_dev; the CRC-32 of the
 * decoded bytes is compared with the trailer's on the device unless MI_INFLATE_NO_CHECKSUM is set.
 * MI_ERR_CORRUPT: any of that failing, a table that is decreasing, leaves the stream or the output
 * range or does not fill out_bytes exactly, and every condition of the mi_inflate_dev list, per
 * member.  MI_ERR_ARG: NULL pointers, d_stream not 4-byte aligned, unknown flag bits.
 * The table is untrusted: reads stay inside [d_stream, d_stream + stream_bytes) rounded out to whole
 * aligned 4-byte words and inside the member's own bytes, writes inside the member's own output
 * range, every loop is bounded.  Index and inflate synchronise `stream` before returning and use
 * the context workspace: one call of a context in flight at a time.
 * mi_bgzf_inflate: host buffers — copy in, index, inflate every member, copy out; out_cap below
 * the stream's total is MI_ERR_CAPACITY; *h_out_bytes (may be NULL) = the total.
 * ------------------------------------------------------------------------------------ */
#define MI_BGZF_BLOCK     65280u   /* htslib's block size */
#define MI_BGZF_MAX_BLOCK 65498u   /* largest b with b + 5 ceil(b/65535) + 5 + 2 + 26 <= 65536 */
/* per block of b bytes b + 5 ceil(b / 65535) + 5 (mode Z's per-block bound: the stored form and its sync flush) + 2 (03 00)
 * + 26 (header and trailer), plus the 28 bytes of the EOF member; 0 if p is not a BGZF parameter set */
uint64_t  mi_bgzf_bound_bytes(uint64_t n, const mi_lz_params *p);
mi_status mi_bgzf_encode_dev(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap_bytes,
                             uint64_t *d_member_bits, uint64_t *d_out_bytes, void *stream);
/* host buffers: copy in, encode, copy out; h_member_bits u64[nblocks+1]; *h_out_bytes (may be NULL) = bytes written */
mi_status mi_bgzf_encode(mi_ctx *ctx, const mi_lz_params *p, const uint8_t *h_in, uint64_t n, uint8_t *h_out, uint64_t cap_bytes,
                         uint64_t *h_member_bits, uint64_t *h_out_bytes);
mi_status mi_bgzf_index_dev(mi_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, uint64_t *d_members, uint64_t cap_members,
                            uint64_t *d_count, void *stream);
mi_status mi_bgzf_inflate_dev(mi_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_members,
                              uint64_t first_member, uint64_t n_members, uint8_t *d_out, uint64_t out_bytes, uint32_t flags, void *stream);
mi_status mi_bgzf_inflate(mi_ctx *ctx, const uint8_t *h_stream, uint64_t stream_bytes, uint8_t *h_out, uint64_t out_cap,
                          uint64_t *h_out_bytes, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * BGZF byte ranges: many (offset, length) slices of the UNCOMPRESSED data in one call — what
 * tabix / BAI region queries and bgzf_seek + bgzf_read ask for, thousands at a time, each inside
 * one to three members.  The pattern of the batch entry points below: device arrays in, one
 * verdict per range on the device, one launch set; a bad range does not spoil the rest.
 *
 * d_members, n_members: the table mi_bgzf_index_dev wrote, n_members + 1 pairs.  Every other array
 * is a DEVICE array of `count` entries.  Let total be the output offset of the last pair.  Range i
 * is the bytes [d_off[i], min(d_off[i] + d_len[i], total)) of the inflated stream and is written at
 * d_out + d_out_off[i]; its SLOT is [d_out_off[i], d_out_off[i] + d_len[i]).  out_bytes is the size
 * of d_out: nothing is stored at or past it.  Ranges may overlap in the source, repeat and come in
 * any order; their slots must not overlap — the library does NOT check that.  No alignment is
 * required of d_out or the offsets; d_stream is 4-byte aligned, as for mi_bgzf_inflate_dev.
 * Members with ISIZE 0 (empty members, the EOF member) contribute nothing and are skipped unread.
 *
 * Per range, on the device: d_status[i] (an mi_status) and d_got[i] —
 *   MI_OK            d_got[i] = the bytes delivered: d_len[i], or fewer where the range ends past
 *                    the end of the data (a short read, as bgzf_read gives); 0 for d_len[i] = 0 and
 *                    for d_off[i] >= total.  The slot's bytes behind d_got[i] are left as they were.
 *   MI_ERR_CORRUPT   d_got[i] = 0: a member the range touches fails the header re-check against
 *                    the table, the decode (every condition of mi_bgzf_inflate_dev, per member) or,
 *                    unless MI_INFLATE_NO_CHECKSUM is set, its CRC-32; a table that decreases where
 *                    the range meets it, or holds no member for bytes below its total.  The slot's
 *                    content is unspecified; nothing outside the slot is written.
 *   MI_ERR_ARG       d_got[i] = 0: a slot (of d_len[i] > 0) that leaves [0, out_bytes) — nothing is
 *                    written for it; pieces beyond max_pieces (below).
 * *d_failed (may be NULL) = the number of ranges whose status is not MI_OK.
 * max_pieces: a HOST-side upper bound on the number of PIECES, a piece being one (range, non-empty
 * member) pair, so that grids and workspace are sized without reading the device — the max_blocks
 * of mi_deflate_batch_dev.  mi_bgzf_read_max_pieces gives count + total_len / min_member_bytes +
 * count from the sum of the lengths and the smallest non-empty member's uncompressed size (at most
 * two cut members per range plus the whole ones that fit between them): MI_BGZF_BLOCK for the
 * output of one bgzip run (only its last member is shorter, and the last member never lies
 * between two others); for concatenated files, or foreign writers, the smallest member there is,
 * or the exact count from the index.  Every piece of the bound costs a wave per stage whether a range fills it or
 * not: keep it tight.  A range whose pieces do not fit the bound — the first such range and every
 * range behind it — is MI_ERR_ARG; the ranges before it are unaffected.
 * A piece whose member lies wholly inside the range is decoded straight into the slot; a member cut
 * by the range's start or end is decoded whole into a 64 KiB cell of the context workspace (at most
 * 4 096 cells, 256 MiB, used again group after group) and the slice copied out, so every member
 * read is CRC-checked whole.
 * The table is untrusted, exactly as for mi_bgzf_inflate_dev: the same bounds on stream reads, every
 * loop bounded, writes inside the range's own slot.
 * The call itself returns only MI_OK, MI_ERR_ARG (NULL arrays, d_stream not 4-byte aligned, unknown
 * flag bits, count above 2^30 - 1, n_members or max_pieces above 2^31 - 1), MI_ERR_HIP or
 * MI_ERR_NOMEM; count == 0 is MI_OK and launches nothing.  Asynchronous on `stream`: no host
 * synchronisation and no device-to-host read once the workspace has grown; read the verdicts after
 * mi_sync or in stream order.  It uses the context workspace: one call of a context in flight at a
 * time.
 * mi_bgzf_read_ranges: host buffers and host arrays — copy up (h_out too: what lies between the
 * slots comes back as it was), index, read, copy down; it finds its own bound from the index.
 * ------------------------------------------------------------------------------------ */
uint64_t  mi_bgzf_read_max_pieces(uint64_t count, uint64_t total_len, uint64_t min_member_bytes);
mi_status mi_bgzf_read_ranges_dev(mi_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_members,
                                  uint64_t n_members, uint64_t count, const uint64_t *d_off, const uint64_t *d_len,
                                  uint8_t *d_out, const uint64_t *d_out_off, uint64_t out_bytes, uint64_t max_pieces,
                                  uint64_t *d_got, uint32_t *d_status, uint32_t *d_failed, uint32_t flags, void *stream);
mi_status mi_bgzf_read_ranges(mi_ctx *ctx, const uint8_t *h_stream, uint64_t stream_bytes, uint64_t count,
                              const uint64_t *h_off, const uint64_t *h_len, uint8_t *h_out, const uint64_t *h_out_off,
                              uint64_t out_bytes, uint64_t *h_got, uint32_t *h_status, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * Batched inflate: many independent DEFLATE streams in one launch — Parquet / ORC pages, zarr /
 * HDF5 chunks, PNG IDAT payloads, HTTP bodies, per-record blobs.  Parallel across items only: one
 * wave decodes an item serially, so an item of hundreds of megabytes belongs to mi_inflate_dev
 * with a table (its checksum, too, is computed by ONE workgroup here).
 *
 * Every array lives on the device and has `count` entries; d_in[i] / d_out[i] are device pointers.
 * Item i is ONE complete stream of the call's `container` (one container per call) in the bytes
 * [d_in[i], d_in[i] + d_in_bytes[i]): the header (the rules of mi_inflate_dev: raw none; zlib CM = 8,
 * CINFO <= 7, FCHECK, FDICT = 0; gzip 1F 8B, CM = 8, reserved flag bits zero, FEXTRA / FNAME /
 * FCOMMENT / FHCRC skipped by their lengths, FHCRC not verified); DEFLATE blocks of any type, the
 * last one — and only that one — with BFINAL = 1; matches may reach back across block boundaries
 * inside the item, up to 32 768 bytes, never before the item's first byte; the padding to a byte
 * boundary; the trailer — none (raw), Adler-32 big-endian (zlib), CRC-32 and ISIZE little-endian
 * (gzip).  The item ends exactly at d_in_bytes[i]: a second gzip member behind the first is trailing
 * data, MI_ERR_CORRUPT.  Multi-member items are out of scope (BGZF above reads members in parallel).
 * No alignment is required of d_in[i] or d_out[i].  Reads stay inside the item's own bytes, rounded
 * out to whole aligned 4-byte words; writes inside [d_out[i], d_out[i] + d_out_cap[i]); every loop
 * is bounded by the item's bit or byte count.  Items may overlap in their inputs (pointers into one
 * stream) but not in their outputs.  An item never influences another item's bytes or verdict.
 *
 * Per item, on the device: d_status[i] (an mi_status) and d_out_bytes[i] —
 *   MI_OK            d_out_bytes[i] = the inflated size, <= d_out_cap[i]; zlib / gzip: the checksum of
 *                    the decoded bytes matched the trailer unless MI_INFLATE_NO_CHECKSUM is set; ISIZE
 *                    (= the size mod 2^32) is always checked.
 *   MI_ERR_CAPACITY  the stream is well-formed but longer than d_out_cap[i]: d_out_bytes[i] = the size
 *                    the caller must provide.  Nothing is written at or past the capacity (a token
 *                    that does not fit is not written at all; from there the wave only counts, with
 *                    every bound still checked); the bytes below it are unspecified; the checksum of
 *                    such an item is not compared.
 *   MI_ERR_CORRUPT   d_out_bytes[i] = 0: every condition of the mi_inflate_dev list, no BFINAL = 1
 *                    block, data behind it other than padding and trailer, a bad header, ISIZE that
 *                    differs, a checksum mismatch.
 *   MI_ERR_ARG       d_out_bytes[i] = 0: a NULL pointer with a non-zero size; d_in_bytes[i] or
 *                    d_out_cap[i] above 2^31 - 1 (positions inside an item are 32-bit); an item that
 *                    inflates to more than 2^31 - 1 bytes.
 * *d_failed (may be NULL) = the number of items whose status is not MI_OK.
 * The call itself returns only MI_OK, MI_ERR_ARG (NULL arrays, an unknown container, unknown flag
 * bits, count > 2^31 - 1), MI_ERR_HIP or MI_ERR_NOMEM; count == 0 is MI_OK and launches nothing.
 * Asynchronous on `stream` (top of file): read the verdicts after mi_sync or in stream order.
 * mi_inflate_batch_size_dev: the same walk without writing a byte — d_out_bytes[i] = what item i
 * inflates to, d_status[i] as above except that MI_ERR_CAPACITY does not occur and that a checksum
 * mismatch cannot be seen (such an item is MI_OK here); gzip's ISIZE is compared.
 * Workgroup j takes item j.  MI_INFLATE_BATCH_ORDER=1 (environment, read at call time) hands the
 * items out by size class instead (the position of the leading one of d_in_bytes[i]), the largest
 * first, so that one large item among thousands of small ones does not start last; it costs a
 * memset and three small launches per call and is off until measured.  No output depends
 * on it.  The ring is chosen as in mi_inflate_dev (32 KiB below 1 024 items, else 4 KiB) and
 * MI_LZ_DECODE_RING overrides it here as there.
 * mi_inflate_batch: host buffers, arrays of host pointers — copy up, inflate, copy down the items
 * that came out MI_OK; h_out = NULL or h_out_cap = NULL runs the size pass alone (h_out_bytes and
 * h_status are filled, nothing is inflated), which is how a caller without sizes gets them — at the
 * price of the inputs travelling to the device twice, once per call.
 * ------------------------------------------------------------------------------------ */
mi_status mi_inflate_batch_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                               void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes, uint32_t *d_status,
                               uint32_t *d_failed, uint32_t flags, void *stream);
mi_status mi_inflate_batch_size_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                    const uint64_t *d_in_bytes, uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed,
                                    uint32_t flags, void *stream);
mi_status mi_inflate_batch(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *h_in, const uint64_t *h_in_bytes,
                           void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * Batched inflate with a preset dictionary (zlib's FDICT: what inflateSetDictionary, or Python's
 * zlib.decompressobj(wbits, zdict=...), reads): ONE dictionary per call, shared by all items, for
 * the small unrelated buffers that have no history of their own to match against.
 * d_dict: dict_bytes bytes on the device, read-only, no alignment required; it must stay as it is
 * until the call has run.  Let E be its last min(dict_bytes, 32 768) bytes.  Everything above holds,
 * with these differences:
 *   raw    every item uses the dictionary.
 *   zlib   an item whose header has FDICT = 1 has a 6-byte header — CMF, FLG and DICTID, four bytes
 *          big-endian — and uses the dictionary if and only if DICTID is the Adler-32 of the WHOLE
 *          dictionary (all dict_bytes); another DICTID is MI_ERR_CORRUPT for that item.  An item
 *          with FDICT = 0 is decoded as without a dictionary.  The Adler-32 of the dictionary is
 *          computed on the device, on `stream`, by the kernels of mi_adler32_dev: no host read.
 *   gzip   has no dictionary field: with dict_bytes > 0 the call is MI_ERR_ARG.
 * For an item that uses the dictionary a match may reach back to |E| bytes before the item's first
 * byte — distance <= position + |E| and <= 32 768 — in the inflate, behind the capacity and in the
 * size pass alike; it may start in E and run into the item's own output, and overlap itself across
 * that seam.  One byte farther is MI_ERR_CORRUPT, as it is for an item that does not use the
 * dictionary (FDICT = 0) one byte before its own first.  The trailer's Adler-32 covers the item's
 * bytes only.  The items' waves read E alone; the Adler-32 reads all of the dictionary.
 * dict_bytes == 0 (d_dict may then be NULL) is the call without a dictionary, verdict for verdict
 * and byte for byte; a zlib item with FDICT is then MI_ERR_CORRUPT.  dict_bytes > 2^31 - 1, or
 * d_dict == NULL with dict_bytes > 0, is MI_ERR_ARG.  The zlib form takes its checksum partials
 * from the context's workspace (which grows, and synchronises, on first use only).
 * mi_inflate_batch_dict: the host form; h_dict is host memory and travels up with the items.
 * ------------------------------------------------------------------------------------ */
mi_status mi_inflate_batch_dict_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                    const uint64_t *d_in_bytes, void *const *d_out, const uint64_t *d_out_cap,
                                    uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, const uint8_t *d_dict,
                                    uint64_t dict_bytes, uint32_t flags, void *stream);
mi_status mi_inflate_batch_dict_size_dev(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *d_in,
                                         const uint64_t *d_in_bytes, uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed,
                                         const uint8_t *d_dict, uint64_t dict_bytes, uint32_t flags, void *stream);
mi_status mi_inflate_batch_dict(mi_ctx *ctx, uint32_t container, uint64_t count, const void *const *h_in, const uint64_t *h_in_bytes,
                                void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status,
                                const uint8_t *h_dict, uint64_t dict_bytes, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * Batched deflate: many independent buffers compressed in ONE call, each from its own address
 * and of its own size into its own buffer as a complete raw, zlib or gzip stream (one container
 * per call) — the twin of the batched inflate above, for Parquet / ORC pages, zarr / HDF5 chunks,
 * PNG IDAT, HTTP bodies.  The blocks of all items run through the one mode-Z pipeline, and item
 * i's output is byte for byte what mi_deflate_z_encode_dev writes for item i alone (same p, same
 * container): one record per p->block input bytes, then 03 00 and the trailer.
 * All arrays are DEVICE arrays of `count` entries.  p: as mode Z (the deflate flavour, wbits <= 15,
 * lbits <= 8, block <= 65536).  No alignment is required of d_in[i] or d_out[i].  Reads stay
 * inside the item's own bytes, rounded out to whole aligned 16-byte words; writes inside
 * [d_out[i], d_out[i] + d_out_cap[i]).  Items may overlap in their inputs but not in their
 * outputs.  An item never influences another item's bytes or verdict.
 * max_blocks: a HOST-side upper bound on the sum of ceil(d_in_bytes[i] / p->block), so that grids
 * and workspace are sized without reading the device; the batch max_blocks helper below gives it
 * from a bound on the total bytes (total / block + count).  Every block of the bound costs a
 * workgroup per stage whether an item fills it or not: keep it tight.  If the device finds more
 * blocks than the bound, the items whose blocks do not fit — the first such item and every item
 * behind it — are MI_ERR_ARG; the items before them are unaffected.
 *
 * Per item, on the device: d_status[i] (an mi_status) and d_out_bytes[i] —
 *   MI_OK            d_out_bytes[i] = the stream's size, <= d_out_cap[i].  An empty item is MI_OK:
 *                    the container header, 03 00 and the trailer, as mode Z writes for n = 0.
 *   MI_ERR_CAPACITY  d_out_bytes[i] = the exact size the caller must provide (at most the batch
 *                    bound of the item's size).  Nothing is written at or past the capacity; the
 *                    bytes below it are unspecified.
 *   MI_ERR_ARG       d_out_bytes[i] = 0: a NULL pointer with a non-zero size or capacity;
 *                    d_in_bytes[i] or d_out_cap[i] above 2^31 - 1; blocks beyond max_blocks.
 * *d_failed (may be NULL) = the number of items whose status is not MI_OK.
 * The call itself returns only MI_OK, MI_ERR_ARG (NULL arrays, p or a container mode Z refuses,
 * count or max_blocks above 2^31 - 1), MI_ERR_HIP or MI_ERR_NOMEM; count == 0 is MI_OK and
 * launches nothing.  Asynchronous on `stream` under the encoders' contract (top of file): no host
 * synchronisation and no device-to-host read; read the verdicts after mi_sync or in stream order.
 * MI_LZ_BATCH (blocks per pipeline batch) works as in every encoder; an item's blocks may
 * straddle pipeline batches.
 * The host form: arrays of host pointers — copy up, encode, copy down the items that came out MI_OK.
 * ------------------------------------------------------------------------------------ */
uint64_t  mi_deflate_batch_bound_bytes(uint64_t n_item, const mi_lz_params *p, uint32_t container);   /* = mi_deflate_z_bound_bytes */
uint64_t  mi_deflate_batch_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p); /* total / block + count */
mi_status mi_deflate_batch_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                               const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                               void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                               uint32_t *d_status, uint32_t *d_failed, void *stream);
mi_status mi_deflate_batch(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                           const void *const *h_in, const uint64_t *h_in_bytes,
                           void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status);

/* ------------------------------------------------------------------------------------
 * Batched deflate with a preset dictionary (zlib's FDICT: what deflateSetDictionary, or Python's
 * zlib.compressobj(..., zdict=...), writes): ONE dictionary per call, shared by all items — the
 * history a 700-byte item does not have.  The streams are standard: stock zlib inflates them with
 * inflateSetDictionary / zlib.decompressobj(wbits, zdict=...), and so does
 * mi_inflate_batch_dict_dev above.
 * d_dict: dict_bytes bytes on the device, read-only, no alignment required.  An encoder may use
 * any suffix of a dictionary; this one uses U, its last min(dict_bytes, 32 768, p->block / 2)
 * bytes.  Everything of mi_deflate_batch_dev holds, with these differences:
 *   blocks  item i's first record covers its first min(n_i, p->block - |U|) bytes — U and that head
 *           are one block to the match finder, and the matches of the head may reach into U — and
 *           its later records p->block bytes each, exactly the records of mi_deflate_batch_dev
 *           for those bytes.  An item has at most one block more than without a dictionary:
 *           mi_deflate_batch_dict_max_blocks (total / block + 2 count) bounds max_blocks, and
 *           mi_deflate_batch_dict_bound_bytes an item's stream.
 *   raw     no header: the caller tells the reader which dictionary it was.
 *   zlib    the header is 78 BB and DICTID, the Adler-32 of the WHOLE dictionary (all dict_bytes)
 *           big-endian: 6 bytes; then the records, 03 00 and the Adler-32 of the item's bytes.  An
 *           empty item: header, 03 00, trailer.  DICTID is computed on the device, on `stream`.
 *   gzip    has no dictionary field: with dict_bytes > 0 the call is MI_ERR_ARG, as zlib refuses it.
 * dict_bytes == 0 (d_dict may then be NULL) is mi_deflate_batch_dev byte for byte; so is a block
 * size below 2, which leaves no room for U.  dict_bytes > 2^31 - 1, or d_dict == NULL with
 * dict_bytes > 0, is MI_ERR_ARG.  Verdicts, capacities (nothing written at or past one, the exact
 * size needed reported), blocks beyond max_blocks and asynchrony are those of
 * mi_deflate_batch_dev.  Workspace: one p->block-byte staging cell per block of a pipeline batch
 * (MI_LZ_BATCH) and scratch set, whatever `count` is.
 * mi_deflate_batch_dict: the host form; h_dict is host memory and travels up with the items.
 * ------------------------------------------------------------------------------------ */
uint64_t  mi_deflate_batch_dict_bound_bytes(uint64_t n_item, const mi_lz_params *p, uint32_t container, uint64_t dict_bytes);
uint64_t  mi_deflate_batch_dict_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p, uint64_t dict_bytes);
mi_status mi_deflate_batch_dict_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                                    const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                                    void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                    uint32_t *d_status, uint32_t *d_failed, const uint8_t *d_dict, uint64_t dict_bytes, void *stream);
mi_status mi_deflate_batch_dict(mi_ctx *ctx, const mi_lz_params *p, uint32_t container, uint64_t count,
                                const void *const *h_in, const uint64_t *h_in_bytes,
                                void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status,
                                const uint8_t *h_dict, uint64_t dict_bytes);

/* ------------------------------------------------------------------------------------
 * Batched Snappy: many independent RAW Snappy buffers encoded or decoded in one call — the
 * default codec of Parquet pages, offered by ORC, Arrow IPC, Kafka and LevelDB too.  An item is
 * what snappy::Compress writes and snappy::Uncompress reads (format_description.txt of
 * google/snappy): varint32(uncompressed length), then literal elements (tag 00) and copies with
 * a 1-, 2- or 4-byte offset (tags 01, 10, 11).  OUT OF SCOPE: the framing format (.sz files, with
 * CRC-32C), Hadoop's block wrapper, and reading Parquet page headers (thrift) — the caller hands
 * over the compressed bytes of each page.
 * All arrays are DEVICE arrays of `count` entries, as for the batched inflate and deflate above:
 * items and outputs at any byte address, every item with its own verdict and size, *d_failed (may
 * be NULL) = the items that are not MI_OK, count == 0 is MI_OK and launches nothing, no item
 * influences another.  All three device calls are asynchronous on `stream`: no host
 * synchronisation, no device-to-host read.
 *
 * mi_snappy_decode_batch_dev — one wave per item.  flags must be 0.  Loads stay inside the aligned
 * dwords that cover the item; no byte at or past min(d_out_cap[i], preamble) is stored.
 *   MI_OK            d_out_bytes[i] = the preamble = the bytes written.
 *   MI_ERR_CAPACITY  the preamble is larger than d_out_cap[i]: d_out_bytes[i] = the preamble, and
 *                    NOTHING is written (it is decided before the first store; the body is not
 *                    validated).
 *   MI_ERR_CORRUPT   d_out_bytes[i] = 0, bytes below min(capacity, preamble) unspecified: an item
 *                    of 0 bytes; a preamble that is cut off, longer than five bytes or above
 *                    2^32 - 1; a copy with offset 0 or an offset larger than the bytes produced so
 *                    far; an element that would pass the preamble length; input that ends inside
 *                    an element, or with fewer bytes produced than the preamble says; input left
 *                    over once the preamble length is reached.
 *   MI_ERR_ARG       d_out_bytes[i] = 0: a NULL pointer with a non-zero size or capacity; a size,
 *                    capacity or preamble above 2^31 - 1.
 * mi_snappy_batch_size_dev — the preamble alone (snappy::GetUncompressedLength), one thread per
 * item: d_out_bytes[i] and the header verdicts above.  It does NOT validate the body: an item
 * that is MI_OK here may be MI_ERR_CORRUPT when decoded.
 *
 * mi_snappy_encode_batch_dev — the batched deflate's pipeline (same finder, same parse, the same
 * blocks: stock Snappy also compresses in independent blocks of at most 64 KiB) with Snappy
 * elements as its last stage.  p and max_blocks: exactly as for mi_deflate_batch_dev (the deflate
 * flavour, wbits <= 15, block <= 65536, parse 0 or 1; mi_snappy_batch_max_blocks is that call's
 * rule).  The bytes are deterministic.  Per block, over the token sequence: literals and matches
 * shorter than 4 gather in a run; a match (L >= 4, d) first flushes the run as ONE literal
 * element in its shortest form, then becomes copies of 64 while L >= 68, one of 60 if L > 64, and
 * the rest (so every piece is >= 4), each with a 1-byte offset form when 4 <= len <= 11 and
 * d < 2048, else the 2-byte form; the run pending at the block's end is flushed.  The 4-byte
 * offset form is never written.  An empty item is the single byte 00.
 *   MI_OK / MI_ERR_CAPACITY (d_out_bytes[i] = the exact size needed, nothing written at or past the
 *   capacity) / MI_ERR_ARG (also: blocks beyond max_blocks) as for mi_deflate_batch_dev.
 * mi_snappy_batch_bound_bytes(n, p) = 5 + n + n / 61 + 3 ceil(n / block): the preamble; a run of r
 * literals in front of a copy costs at most r / 61 bytes more than the input it covers together
 * with that copy; a block's last run at most 3.
 * The host forms: arrays of host pointers — copy up, run, copy down the items that came out MI_OK;
 * mi_snappy_decode_batch with h_out = NULL or h_out_cap = NULL answers the sizes alone.
 * ------------------------------------------------------------------------------------ */
uint64_t  mi_snappy_batch_bound_bytes(uint64_t n_item, const mi_lz_params *p);
uint64_t  mi_snappy_batch_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p);   /* total / block + count */
mi_status mi_snappy_encode_batch_dev(mi_ctx *ctx, const mi_lz_params *p, uint64_t count,
                                     const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                                     void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                     uint32_t *d_status, uint32_t *d_failed, void *stream);
mi_status mi_snappy_decode_batch_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                     void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                     uint32_t *d_status, uint32_t *d_failed, uint32_t flags, void *stream);
mi_status mi_snappy_batch_size_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                   uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, void *stream);
mi_status mi_snappy_encode_batch(mi_ctx *ctx, const mi_lz_params *p, uint64_t count,
                                 const void *const *h_in, const uint64_t *h_in_bytes,
                                 void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status);
mi_status mi_snappy_decode_batch(mi_ctx *ctx, uint64_t count, const void *const *h_in, const uint64_t *h_in_bytes,
                                 void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status,
                                 uint32_t flags);

/* ------------------------------------------------------------------------------------
 * Batched LZ4: many independent LZ4 buffers encoded or decoded in one call, in one of two
 * formats chosen per call:
 *   MI_LZ4_BLOCK  a RAW block (lz4_Block_format.md; what LZ4_compress_default writes and
 *                 LZ4_decompress_safe reads): Parquet LZ4_RAW, ORC, zarr / blosc, ClickHouse, RocksDB.
 *                 Sequences of token (literal-length nibble high, match-length nibble low), a chain
 *                 of 255-valued bytes behind a nibble of 15, the literals, a 2-byte little-endian
 *                 offset, the match-length chain (match length = nibble + chain + 4); the last
 *                 sequence is literals only and ends exactly at the item's end.  A block does not
 *                 name its size.
 *   MI_LZ4_FRAME  a frame (lz4_Frame_format.md; the `lz4` tool, Arrow IPC / Feather buffers):
 *                 magic 04 22 4D 18, FLG, BD, optional content size, HC, then blocks behind 4-byte
 *                 size words (top bit: stored) up to the EndMark 00 00 00 00.
 * OUT OF SCOPE: dictionaries, skippable and concatenated frames, the legacy frame, Hadoop's LZ4
 * wrapper, LZ4-HC parsing, and XXH32 beyond the header's HC byte — the encoder writes no block or
 * content checksum, and the decoder SKIPS OVER both without verifying them (`flags` must be 0 and
 * is reserved for a later verify).
 * Arrays, addresses, verdicts, *d_failed, count == 0 and asynchrony: exactly as for the batched
 * Snappy above.
 *
 * mi_lz4_decode_batch_dev — one wave per item.  Loads stay inside the aligned dwords that cover
 * the item; every bound is checked before an element stores; no byte at or past d_out_cap[i] is
 * stored.  Neither format has to name its size, so a capacity works as in mi_inflate_batch_dev:
 * past it the walk goes on without stores.
 *   MI_OK            d_out_bytes[i] = the bytes written.  The single byte 00 is a block of 0 bytes.
 *   MI_ERR_CAPACITY  well-formed to its end, but larger than d_out_cap[i]: d_out_bytes[i] = the
 *                    size it needs; bytes below the capacity unspecified.
 *   MI_ERR_CORRUPT   d_out_bytes[i] = 0, bytes below the capacity unspecified: an item of 0 bytes;
 *                    offset 0 or an offset above the bytes written (with B.Indep = 1: above the bytes
 *                    written by its block); input that ends inside a sequence, or a block that does
 *                    not end with a literals-only sequence.  Frame: a wrong magic, version, reserved
 *                    bit, BD, or HC (which IS checked); block data or block output above the BD
 *                    maximum; a missing EndMark or checksum field; a content size that is not the
 *                    decoded length; bytes behind the frame.
 *                    The decoder does NOT enforce the encoder-side end rules (last 5 bytes literal,
 *                    last match starting >= 12 bytes before the end): the specification leaves
 *                    those to encoders.
 *   MI_ERR_ARG       d_out_bytes[i] = 0: a NULL pointer with a non-zero size or capacity; a size,
 *                    capacity, content size or decoded length above 2^31 - 1; well-formed but
 *                    unsupported — a frame with a DictID, a skippable-frame or the legacy magic.
 * mi_lz4_batch_size_dev — one thread per item, the same walk without stores and the same
 * verdicts, EXCEPT that a frame which carries a content size answers from its header alone (its
 * body is not looked at, as for mi_snappy_batch_size_dev).
 *
 * mi_lz4_encode_batch_dev — the batched deflate's pipeline (finder, parse 0 or 1, blocks) with LZ4
 * sequences as its last stage.  p and max_blocks: exactly as for mi_snappy_encode_batch_dev.  The
 * bytes are deterministic.  Per block of n bytes, over the token sequence: a literal joins the
 * pending run; a match (L, d) at position p joins it too when p + 12 > n, or when
 * L = min(L, n - 5 - p) leaves L < 4 (the format's end rules, which stock decoders enforce; the
 * bytes a shortened match no longer covers begin the next run); any other match flushes the run
 * and itself as one sequence; the run pending at the block's end is the closing literals-only
 * sequence, so a block below 13 bytes is all literals.
 *   MI_LZ4_BLOCK: an item is ONE block — no header, no trailer, an empty item the byte 00.  An item
 *   with in_bytes > p->block is MI_ERR_ARG for that item alone (it takes none of max_blocks).
 *   Items of several pipeline blocks are not written: a block's closing run would have to merge
 *   into the next block's first sequence, a dependency along the item the pipeline has no place for.
 *   MI_LZ4_FRAME: an item of any size up to 2^31 - 1 is 04 22 4D 18 60 40 82 (version 1,
 *   independent blocks, no checksums, no content size, 64 KiB maximum), one frame block per
 *   pipeline block — the size word and the record, or, where the record would not be shorter than
 *   the block, n | 0x80000000 and the block's bytes — and 00 00 00 00.  An empty item is those 11 bytes.
 *   MI_OK / MI_ERR_CAPACITY (d_out_bytes[i] = the exact size needed, nothing written at or past the
 *   capacity) / MI_ERR_ARG (also: blocks beyond max_blocks) as for mi_deflate_batch_dev.
 * mi_lz4_batch_bound_bytes(n, p, format): block n + n / 255 + 16 (LZ4_compressBound; a sequence
 * is at most r / 255 bytes longer than the r literals and the match it covers, the closing one
 * 2 + r / 255); frame 11 + n + 4 ceil(n / block).
 * The host forms: as mi_snappy_encode_batch / mi_snappy_decode_batch.
 * ------------------------------------------------------------------------------------ */
#define MI_LZ4_BLOCK 0u
#define MI_LZ4_FRAME 1u
uint64_t  mi_lz4_batch_bound_bytes(uint64_t n_item, const mi_lz_params *p, uint32_t format);
uint64_t  mi_lz4_batch_max_blocks(uint64_t total_in_bytes, uint64_t count, const mi_lz_params *p);   /* total / block + count */
mi_status mi_lz4_encode_batch_dev(mi_ctx *ctx, const mi_lz_params *p, uint32_t format, uint64_t count,
                                  const void *const *d_in, const uint64_t *d_in_bytes, uint64_t max_blocks,
                                  void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                  uint32_t *d_status, uint32_t *d_failed, void *stream);
mi_status mi_lz4_decode_batch_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                  void *const *d_out, const uint64_t *d_out_cap, uint64_t *d_out_bytes,
                                  uint32_t *d_status, uint32_t *d_failed, uint32_t format, uint32_t flags, void *stream);
mi_status mi_lz4_batch_size_dev(mi_ctx *ctx, uint64_t count, const void *const *d_in, const uint64_t *d_in_bytes,
                                uint64_t *d_out_bytes, uint32_t *d_status, uint32_t *d_failed, uint32_t format, void *stream);
mi_status mi_lz4_encode_batch(mi_ctx *ctx, const mi_lz_params *p, uint32_t format, uint64_t count,
                              const void *const *h_in, const uint64_t *h_in_bytes,
                              void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status);
mi_status mi_lz4_decode_batch(mi_ctx *ctx, uint64_t count, const void *const *h_in, const uint64_t *h_in_bytes,
                              void *const *h_out, const uint64_t *h_out_cap, uint64_t *h_out_bytes, uint32_t *h_status,
                              uint32_t format, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * FSE / tANS, block-parallel (fse/src/main.zig — an unfinished sketch; the stream format is
 * defined by this build).  Record layout in include/mi_fse.h.
 * ------------------------------------------------------------------------------------ */
typedef struct {
    uint32_t table_log;   /* 8 (reference TABLE_LOG) .. 12                                 */
    uint32_t streams;     /* sub-streams per block, 1..64 (one GPU lane each)               */
    uint32_t spread;      /* 0: contiguous symbol ranges (main.zig:159-177), 1: stride spread */
    uint32_t block;       /* block size in bytes, 4..65536                                  */
} mi_fse_params;

static inline mi_fse_params mi_fse_params_default(void) { mi_fse_params p = {8, 64, 1, 65536}; return p; }
uint64_t  mi_fse_block_bound(const mi_fse_params *p);        /* bytes per block record, worst case */
/* d_out: nblocks records at stride mi_fse_block_bound(); d_sizes u32[nblocks] = used bytes.
 * d_packed (optional, may be NULL): the records concatenated; d_offsets u64[nblocks+1]. */
mi_status mi_fse_encode_dev(mi_ctx *ctx, const mi_fse_params *p, const uint8_t *d_in, uint64_t n,
                            uint8_t *d_packed, uint64_t cap_bytes, uint64_t *d_offsets, void *stream);
mi_status mi_fse_decode_dev(mi_ctx *ctx, const mi_fse_params *p, const uint8_t *d_packed, uint64_t packed_bytes,
                            const uint64_t *d_offsets, uint8_t *d_out, uint64_t n, void *stream);
/* host-buffer versions.  h_packed needs mi_fse_block_bound() * nblocks bytes; h_offsets u64[nblocks+1] (bits). */
mi_status mi_fse_encode(mi_ctx *ctx, const mi_fse_params *p, const uint8_t *h_in, uint64_t n,
                        uint8_t *h_packed, uint64_t cap_bytes, uint64_t *h_offsets);
mi_status mi_fse_decode(mi_ctx *ctx, const mi_fse_params *p, const uint8_t *h_packed, uint64_t packed_bytes,
                        const uint64_t *h_offsets, uint8_t *h_out, uint64_t n);
/* the normalisation step alone (main.zig:106-149), for parity tests: d_freq u64[256] -> d_cnt u32[256] */
mi_status mi_fse_normalise_dev(mi_ctx *ctx, const uint64_t *d_freq, uint32_t table_log, uint32_t *d_cnt, void *stream);

/* ------------------------------------------------------------------------------------
 * Several GPUs of one node from ONE process (BASELINE config 5 behind the reference's own API).
 *   The reference's block loop (algorithms/deflate/deflate.c:47-63) walks the file block by block; blocks are independent
 *   here (fresh table per block), so device g of `ndev` encodes the contiguous block range
 *   mi_multi_shard(nblocks, g, ndev) with its own context and the single-GPU pipeline, concurrently, with no data-path
 *   collective.  The only exchange is the assembly of ONE stream + ONE block table on device 0 ("RCCL gather of per-block
 *   compressed streams over xGMI"): the per-device sizes meet on the host (8 bytes each), then ONE group of point-to-point
 *   transfers — ncclGroupStart .. ncclSend / ncclRecv x (ndev - 1) .. ncclGroupEnd — moves streams and tables into device 0,
 *   every peer over its own xGMI link.  A shard that starts on a 32-bit boundary of the final stream (mode H always) is
 *   received in place; otherwise it lands in a staging area and one kernel shifts it in (the bit-packed lz77 flavour:
 *   result bit-contiguous, exactly what one GPU writes for the whole buffer).
 *   Transport: RCCL (librccl.so, loaded on first use — libmi_codec.so does not link it) when the listed devices are
 *   distinct; hipMemcpyPeerAsync when a device is listed more than once (two contexts on one GPU: how the path is tested
 *   on a one-GPU box) or when MI_MULTI_TRANSPORT=peer.  MI_MULTI_TRANSPORT=rccl insists on RCCL (MI_ERR_TRANSPORT if the
 *   device list has a duplicate or the library is missing).
 *   The result is byte-identical to the single-context entry points' (tests/test_multi_gpu.py).
 *   The drop-in compress() takes this path when MI_CODEC_DEVICES=0,1,... is set (include/mi_deflate.h).
 * ------------------------------------------------------------------------------------ */
typedef struct mi_multi mi_multi;
mi_status   mi_multi_create(mi_multi **out, const int *devices, int ndev);       /* 1 <= ndev <= 64 */
void        mi_multi_destroy(mi_multi *m);
int         mi_multi_ndev(const mi_multi *m);
mi_ctx     *mi_multi_ctx(mi_multi *m, int g);                                    /* device g's context (owned by m) */
const char *mi_multi_transport(const mi_multi *m);                               /* "rccl" | "peer-copy" */
const char *mi_multi_last_transport_error(const mi_multi *m);                    /* text of the last MI_ERR_TRANSPORT, or "" */
/* contiguous block range [*lo, *hi) of device g: ceil(nblocks / ndev) blocks each, the last ones possibly fewer or none
 * (the rule of compression_algorithms_amd/sharded.py shard_blocks) */
void        mi_multi_shard(uint64_t nblocks, int g, int ndev, uint64_t *lo, uint64_t *hi);
/* Shards resident: d_in[g] points at device g's shard (its block range of the n input bytes, on device g; NULL for an
 * empty range).  mode_h = 0: mi_lz_encode_dev's stream (either flavour, any block size it takes), 1: mi_deflate_h_encode_dev's.
 * d_out0 (cap_bytes >= the single-device bound for n, 4-byte aligned) and d_block_bits0 (u64[nblocks + 1]) live on
 * devices[0].  Returns when the assembled stream is complete (it synchronises every device's stream). */
mi_status   mi_lz_encode_multi_dev(mi_multi *m, const mi_lz_params *p, int mode_h, const uint8_t *const *d_in, uint64_t n,
                                   uint8_t *d_out0, uint64_t cap_bytes, uint64_t *d_block_bits0);
/* host buffers: shards go up to their devices side by side, the assembled stream comes down from device 0 */
mi_status   mi_lz_encode_multi(mi_multi *m, const mi_lz_params *p, const uint8_t *h_in, uint64_t n,
                               uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits);
mi_status   mi_deflate_h_encode_multi(mi_multi *m, const mi_lz_params *p, const uint8_t *h_in, uint64_t n,
                                      uint8_t *h_out, uint64_t cap_bytes, uint64_t *h_block_bits);
/* moves `bytes` pattern bytes from the LAST device to device 0 through the gather's transport and checks them there:
 * the one way to drive the RCCL entry points on a one-GPU box (ndev = 1: a send to self inside the group). */
mi_status   mi_multi_selftest_transport(mi_multi *m, uint64_t bytes);
/* what the LZ encoders of a context met since it was created: blocks the LDS-resident finder handed to the fallback
 * pipeline (a giant cluster), parts above 2 560 entries (k_lz2_find_wide).  Both 0 on text; a corpus that lives there
 * runs at the fallback's rate and would otherwise only show as a slow number.  Synchronises the device. */
mi_status   mi_lz_path_stats(mi_ctx *ctx, uint64_t *fallback_blocks, uint64_t *wide_parts);

/* ------------------------------------------------------------------------------------
 * timing of the last *_dev call's dominant kernel, measured with hipEvents on the stream
 * the kernels ran on (bench.py's roofline leg).  Enabled by mi_set_profiling(ctx, 1).
 * ------------------------------------------------------------------------------------ */
typedef struct {
    const char *name;
    double      ms;       /* average duration per launch                                   */
    uint64_t    launches;
    uint64_t    bytes;    /* algorithmic bytes the launches moved               */
} mi_kernel_time;
mi_status mi_set_profiling(mi_ctx *ctx, int on);
/* returns the number of entries written (<= cap); resets the accumulators */
int       mi_get_kernel_times(mi_ctx *ctx, mi_kernel_time *out, int cap);

#ifdef __cplusplus
}
#endif
#endif
