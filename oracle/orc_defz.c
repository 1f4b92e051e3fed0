/*
 * ORACLE — TEST INFRASTRUCTURE ONLY (see orc_table.h).
 *
 * orc_defz.c — "mode Z": standard DEFLATE (RFC 1951) over the reference's deflate tokens, in a raw,
 * zlib (RFC 1950) or gzip (RFC 1952) container.  A plain sequential restatement of the contract in
 * include/mi_codec.h ("mode Z") and DESIGN.md section 3.5; the GPU encoder must give these bytes.
 *
 * What is taken from the reference: the token sequence (algorithms/deflate/lz77.c:199-280 with a
 * fresh table per block, restated in orc_lz.c) and the heap procedure that gives the unlimited code
 * lengths (algorithms/huffman/huffman.c:100-163,189-211, restated in orc_defh.c).  Everything else is
 * this build's format, written out in the contract:
 *   the clip          a block's last match running past the block end is cut to L' = n - pos: a match
 *                     of L' if L' >= 3, else L' literals read from the input
 *   padding           a code with fewer than two used symbols gets two codes of length 1, as zlib's
 *                     build_tree pads: none used -> symbols 0 and 1; one used, s -> s and s + 1 if
 *                     s < 2, else s and 0
 *   the limiter       lengths above `limit` (15; 7 for the code-length code) are clamped; while the
 *                     Kraft sum exceeds 1 one code moves a level down from the deepest level l <
 *                     limit that has one (l >= 1); while it is below 1 one code moves a level up from
 *                     the deepest level l <= limit (l >= 2) that has one and whose step 2^-l still
 *                     fits; the level counts are then dealt out to the used symbols in (unlimited
 *                     length, symbol) order, shortest first
 *   the header        HLIT trimmed while > 257 and the last literal/length length is 0, HDIST while
 *                     > 1 and the last distance length is 0, HCLEN while > 4 and the last length in
 *                     RFC order is 0; one run-length sequence over the HLIT + HDIST lengths: a run of
 *                     zeros as 18s of min(run, 138) while run >= 11, then one 17 if run >= 3; a run of
 *                     v != 0 as v, then 16s of min(rest, 6) while rest >= 3; what is left as literals
 *   the block type    the shortest in bits of dynamic, fixed and stored, ties dynamic > fixed > stored:
 *                       dynamic 3 + 14 + 3 HCLEN + code-length symbols and extras + tokens + extras
 *                       fixed   3 + tokens and extras in the fixed code
 *                       stored  40 ceil(n / 65535) + 8 n       (end-of-block counts in both Huffman sizes)
 *   the record        that block (BFINAL = 0), then 000 + padding + 00 00 FF FF; bits LSB first
 *   the stream        container header, the records, 03 00, the container trailer
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int orc_heap_lengths(const uint32_t *freq, int nsym, uint8_t *len);     /* orc_defh.c */

#define DZ_LL 286
#define DZ_DC 30
#define DZ_CL 19

static const uint8_t dz_order[DZ_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
static const uint16_t dz_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83,
                                         99, 115, 131, 163, 195, 227, 258};
static const uint8_t dz_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t dz_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769,
                                          1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t dz_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11,
                                          12, 12, 13, 13};

/* the RFC 1951 3.2.5 tables, searched */
static int dz_len_code(uint32_t L) { int i = 28; while (dz_len_base[i] > L) --i; return i; }       /* 0..28 -> 257 + i */
static int dz_dist_code(uint32_t d) { int i = 29; while (dz_dist_base[i] > d) --i; return i; }
static uint32_t dz_fixed_len(int s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

/* Length-limited code lengths over freq[0, nsym), nsym <= 288: the unlimited heap lengths, zlib's padding, then the
 * limiter.  Returns 1 when the limiter changed the lengths (some unlimited length was above `limit`), else 0. */
int orc_defz_lengths(const uint32_t *freq, int nsym, int limit, uint8_t *len)
{
    const int used = orc_heap_lengths(freq, nsym, len);
    if (used < 2) {
        int first = -1;
        for (int s = 0; s < nsym; ++s) if (freq[s]) { first = s; break; }
        memset(len, 0, (size_t)nsym);
        if (first < 0) { len[0] = 1; len[1] = 1; }
        else { len[first] = 1; len[first < 2 ? first + 1 : 0] = 1; }
        return 0;
    }
    int maxlen = 0;
    for (int s = 0; s < nsym; ++s) if (len[s] > maxlen) maxlen = len[s];
    if (maxlen <= limit) return 0;
    /* clamp */
    uint64_t cnt[64] = {0};
    for (int s = 0; s < nsym; ++s) if (len[s]) ++cnt[len[s] > limit ? limit : len[s]];
    const uint64_t full = 1ull << limit;
    uint64_t K = 0;
    for (int l = 1; l <= limit; ++l) K += cnt[l] << (limit - l);
    /* down: one code one level deeper, from the deepest level below the limit that has one */
    while (K > full) {
        int l = limit - 1;
        while (l > 1 && cnt[l] == 0) --l;
        if (cnt[l] == 0) abort();                                   /* (cannot happen: nsym <= 2^limit) */
        cnt[l]--; cnt[l + 1]++; K -= 1ull << (limit - l - 1);
    }
    /* up: one code one level shallower, from the deepest level whose step still fits */
    while (K < full) {
        int l = limit;
        while (l > 2 && (cnt[l] == 0 || (1ull << (limit - l)) > full - K)) --l;
        if (cnt[l] == 0) abort();
        cnt[l]--; cnt[l - 1]++; K += 1ull << (limit - l);
    }
    /* deal the levels out in (unlimited length, symbol) order, shortest level first */
    int q = 1;
    for (int l = 1; l <= maxlen; ++l)
        for (int s = 0; s < nsym; ++s) {
            if (len[s] != l) continue;
            while (cnt[q] == 0) ++q;
            cnt[q]--;
            len[s] = (uint8_t)(64 + q);                             /* (marked: dealt; 64 + q > any unlimited length) */
        }
    for (int s = 0; s < nsym; ++s) if (len[s]) len[s] -= 64;
    return 1;
}

/* RFC 1951 3.2.2 canonical codes */
static void dz_codes(const uint8_t *len, int nsym, uint32_t *code)
{
    uint32_t count[17] = {0}, next[17] = {0};
    for (int s = 0; s < nsym; ++s) if (len[s]) ++count[len[s]];
    uint32_t c = 0;
    for (int l = 1; l <= 16; ++l) { c = (c + count[l - 1]) << 1; next[l] = c; }
    for (int s = 0; s < nsym; ++s) code[s] = len[s] ? next[len[s]]++ : 0;
}

/* LSB-first bit writer (RFC 1951 3.1.1) */
typedef struct { uint8_t *p; uint64_t bit; } dz_bits;
static void dz_put(dz_bits *b, uint32_t v, uint32_t k)                 /* a field: value LSB first */
{
    for (uint32_t i = 0; i < k; ++i, ++b->bit)
        if ((v >> i) & 1u) b->p[b->bit >> 3] |= (uint8_t)(1u << (b->bit & 7));
}
static void dz_put_code(dz_bits *b, uint32_t code, uint32_t k)         /* a Huffman code: its MSB first */
{
    for (uint32_t i = 0; i < k; ++i, ++b->bit)
        if ((code >> (k - 1 - i)) & 1u) b->p[b->bit >> 3] |= (uint8_t)(1u << (b->bit & 7));
}

/* one token after the clip: a literal (L = 0, value c) or a match (L >= 3, d) */
typedef struct { uint16_t L, d; uint8_t c; } dz_tok;

/* byte tokens of one block ({0,c} / {1,dlo,dhi,len}) -> the clipped token list; returns the count, *clip = L' or 0 */
static uint32_t dz_clip(const uint8_t *tok, uint64_t ntok_bytes, const uint8_t *in, uint32_t n, dz_tok *t, uint32_t *clip)
{
    uint32_t k = 0, pos = 0;
    *clip = 0;
    for (uint64_t i = 0; i < ntok_bytes;) {
        if (tok[i] == 0) { t[k].L = 0; t[k].d = 0; t[k].c = tok[i + 1]; ++k; ++pos; i += 2; continue; }
        uint32_t d = tok[i + 1] | ((uint32_t)tok[i + 2] << 8), L = tok[i + 3];
        i += 4;
        if (i >= ntok_bytes && pos + L > n) {                      /* the last token runs past the block end */
            L = n - pos;
            *clip = L;
            if (L < 3) {
                for (uint32_t j = 0; j < L; ++j) { t[k].L = 0; t[k].d = 0; t[k].c = in[n - L + j]; ++k; }
                pos += L;
                continue;
            }
        }
        t[k].L = (uint16_t)L; t[k].d = (uint16_t)d; t[k].c = 0; ++k; pos += L;
    }
    return k;
}

/* info[] of orc_defz_record */
enum { DZI_TYPE, DZI_DYN, DZI_FIX, DZI_STO, DZI_LIM_LL, DZI_LIM_DC, DZI_LIM_CL, DZI_CLIP, DZI_HLIT, DZI_HDIST, DZI_HCLEN, DZI_N };

/* Bytes a record of an n-byte block can take at most, in any of the three forms. */
uint64_t orc_defz_record_cap(uint32_t n) { return 2ull * n + 5ull * ((n + 65534u) / 65535u) + 1024u; }

/*
 * One record: tok = the oracle's byte tokens of one block, in = that block's n >= 1 bytes.  force < 0 chooses the
 * block type; 0 / 1 / 2 writes that BTYPE whatever it costs.  out must hold orc_defz_record_cap(n) bytes.
 * info (may be NULL) gets DZI_N values: the chosen type, the three sizes in bits, the three limiter flags (literal /
 * length, distance, code-length code), the clip, HLIT, HDIST, HCLEN.  Returns the record's length in bytes.
 */
uint64_t orc_defz_record(const uint8_t *tok, uint64_t ntok_bytes, const uint8_t *in, uint32_t n, int force, uint8_t *out,
                         uint64_t *info)
{
    dz_tok *t = (dz_tok *)malloc(sizeof(dz_tok) * ((size_t)n + 2));
    if (!t) return 0;
    uint32_t clip;
    const uint32_t ntok = dz_clip(tok, ntok_bytes, in, n, t, &clip);

    /* the tally */
    uint32_t f_ll[DZ_LL] = {0}, f_dc[DZ_DC] = {0}, f_cl[DZ_CL] = {0};
    uint64_t ext = 0;
    for (uint32_t k = 0; k < ntok; ++k) {
        if (!t[k].L) { ++f_ll[t[k].c]; continue; }
        const int lc = dz_len_code(t[k].L), dc = dz_dist_code(t[k].d);
        ++f_ll[257 + lc]; ++f_dc[dc];
        ext += dz_len_extra[lc] + dz_dist_extra[dc];
    }
    ++f_ll[256];

    /* the two token codes */
    uint8_t l_ll[DZ_LL], l_dc[DZ_DC], l_cl[DZ_CL];
    const int lim_ll = orc_defz_lengths(f_ll, DZ_LL, 15, l_ll);
    const int lim_dc = orc_defz_lengths(f_dc, DZ_DC, 15, l_dc);

    /* the run-length sequence over HLIT + HDIST lengths */
    uint32_t hlit = DZ_LL, hdist = DZ_DC;
    while (hlit > 257 && !l_ll[hlit - 1]) --hlit;
    while (hdist > 1 && !l_dc[hdist - 1]) --hdist;
    uint8_t seq[DZ_LL + DZ_DC];
    const uint32_t N = hlit + hdist;
    for (uint32_t i = 0; i < N; ++i) seq[i] = i < hlit ? l_ll[i] : l_dc[i - hlit];
    uint8_t rsym[DZ_LL + DZ_DC], rext[DZ_LL + DZ_DC];
    uint32_t nr = 0;
    for (uint32_t i = 0; i < N;) {
        const uint32_t v = seq[i];
        uint32_t run = 1;
        while (i + run < N && seq[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const uint32_t q = run < 138 ? run : 138; rsym[nr] = 18; rext[nr++] = (uint8_t)(q - 11); run -= q; }
            if (run >= 3) { rsym[nr] = 17; rext[nr++] = (uint8_t)(run - 3); run = 0; }
        } else {
            rsym[nr] = (uint8_t)v; rext[nr++] = 0; --run;
            while (run >= 3) { const uint32_t q = run < 6 ? run : 6; rsym[nr] = 16; rext[nr++] = (uint8_t)(q - 3); run -= q; }
        }
        while (run) { rsym[nr] = (uint8_t)v; rext[nr++] = 0; --run; }
    }
    for (uint32_t j = 0; j < nr; ++j) ++f_cl[rsym[j]];
    const int lim_cl = orc_defz_lengths(f_cl, DZ_CL, 7, l_cl);
    uint32_t hclen = DZ_CL;
    while (hclen > 4 && !l_cl[dz_order[hclen - 1]]) --hclen;

    /* the three sizes, the type */
    uint64_t dyn = 3 + 14 + 3ull * hclen + ext, fix = 3 + ext;
    for (int s = 0; s < DZ_CL; ++s) dyn += (uint64_t)f_cl[s] * (l_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
    for (int s = 0; s < DZ_LL; ++s) { dyn += (uint64_t)f_ll[s] * l_ll[s]; fix += (uint64_t)f_ll[s] * dz_fixed_len(s); }
    for (int s = 0; s < DZ_DC; ++s) { dyn += (uint64_t)f_dc[s] * l_dc[s]; fix += (uint64_t)f_dc[s] * 5u; }
    const uint32_t npieces = (n + 65534u) / 65535u;
    const uint64_t sto = 40ull * npieces + 8ull * n;
    const int chosen = (dyn <= fix && dyn <= sto) ? 2 : fix <= sto ? 1 : 0;
    const int type = force >= 0 ? force : chosen;
    if (info) {
        const uint64_t v[DZI_N] = {(uint64_t)chosen, dyn, fix, sto, (uint64_t)lim_ll, (uint64_t)lim_dc, (uint64_t)lim_cl, clip,
                                   hlit, hdist, hclen};
        memcpy(info, v, sizeof v);
    }

    const uint64_t cap = orc_defz_record_cap(n);
    memset(out, 0, cap);
    uint64_t bytes;
    if (type == 0) {
        uint64_t o = 0;
        for (uint32_t p = 0; p < npieces; ++p) {
            const uint32_t len = n - 65535u * p < 65535u ? n - 65535u * p : 65535u;
            out[o++] = 0;                                          /* BFINAL 0, BTYPE 00, padding */
            out[o++] = (uint8_t)len; out[o++] = (uint8_t)(len >> 8);
            out[o++] = (uint8_t)~len; out[o++] = (uint8_t)(~len >> 8);
            memcpy(out + o, in + 65535u * p, len);
            o += len;
        }
        out[o++] = 0; out[o++] = 0; out[o++] = 0; out[o++] = 0xFF; out[o++] = 0xFF;
        bytes = o;
    } else {
        uint32_t c_ll[288], c_dc[32], c_cl[DZ_CL];
        uint8_t L_ll[288], L_dc[32];
        if (type == 1) {
            for (int s = 0; s < 288; ++s) L_ll[s] = (uint8_t)dz_fixed_len(s);
            for (int s = 0; s < 32; ++s) L_dc[s] = 5;
        } else {
            memcpy(L_ll, l_ll, DZ_LL); L_ll[286] = L_ll[287] = 0;
            memcpy(L_dc, l_dc, DZ_DC); L_dc[30] = L_dc[31] = 0;
        }
        dz_codes(L_ll, 288, c_ll);
        dz_codes(L_dc, 32, c_dc);
        dz_bits b = {out, 0};
        dz_put(&b, 0, 1);                                          /* BFINAL 0 */
        dz_put(&b, (uint32_t)type, 2);
        if (type == 2) {
            dz_codes(l_cl, DZ_CL, c_cl);
            dz_put(&b, hlit - 257, 5); dz_put(&b, hdist - 1, 5); dz_put(&b, hclen - 4, 4);
            for (uint32_t i = 0; i < hclen; ++i) dz_put(&b, l_cl[dz_order[i]], 3);
            for (uint32_t j = 0; j < nr; ++j) {
                const int s = rsym[j];
                dz_put_code(&b, c_cl[s], l_cl[s]);
                if (s == 16) dz_put(&b, rext[j], 2);
                else if (s == 17) dz_put(&b, rext[j], 3);
                else if (s == 18) dz_put(&b, rext[j], 7);
            }
        }
        for (uint32_t k = 0; k < ntok; ++k) {
            if (!t[k].L) { dz_put_code(&b, c_ll[t[k].c], L_ll[t[k].c]); continue; }
            const int lc = dz_len_code(t[k].L), dc = dz_dist_code(t[k].d);
            dz_put_code(&b, c_ll[257 + lc], L_ll[257 + lc]);
            dz_put(&b, t[k].L - dz_len_base[lc], dz_len_extra[lc]);
            dz_put_code(&b, c_dc[dc], L_dc[dc]);
            dz_put(&b, t[k].d - dz_dist_base[dc], dz_dist_extra[dc]);
        }
        dz_put_code(&b, c_ll[256], L_ll[256]);                     /* end-of-block */
        dz_put(&b, 0, 3);                                          /* the sync flush: an empty stored block */
        uint64_t o = (b.bit + 7) >> 3;
        out[o++] = 0; out[o++] = 0; out[o++] = 0xFF; out[o++] = 0xFF;
        bytes = o;
    }
    free(t);
    return bytes;
}

/* CRC-32 (zlib's crc32) and Adler-32 (zlib's adler32) of a whole buffer, bit by bit and byte by byte */
uint32_t orc_crc32(const uint8_t *p, uint64_t n)
{
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
        tab[i] = c;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint32_t orc_adler32(const uint8_t *p, uint64_t n)
{
    uint64_t a = 1, s = 0;
    for (uint64_t i = 0; i < n; ++i) { a = (a + p[i]) % 65521u; s = (s + a) % 65521u; }
    return (uint32_t)(s << 16 | a);
}

/* Bytes orc_defz_stream may write for n input bytes in blocks of `block`. */
uint64_t orc_defz_stream_cap(uint64_t n, uint32_t block)
{
    const uint64_t nb = (n + block - 1) / block;
    return nb * orc_defz_record_cap(block) + 32;
}

/*
 * The whole stream: in[0, n), its byte tokens tok (all blocks, the oracle's deflate_stream with a fresh table per
 * block) with tok_sizes[b] bytes for block b; container 0 raw, 1 zlib, 2 gzip.  out must hold orc_defz_stream_cap
 * bytes; block_bits gets nblocks + 1 entries (record b starts at bit block_bits[b], the last entry is where 03 00
 * starts).  Returns the stream's length in bytes, 0 on a bad argument or no memory.
 */
uint64_t orc_defz_stream(const uint8_t *in, uint64_t n, uint32_t block, uint32_t container, const uint8_t *tok,
                         const uint64_t *tok_sizes, uint8_t *out, uint64_t *block_bits)
{
    static const uint8_t gz[10] = {0x1F, 0x8B, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0xFF};
    if (container > 2 || block == 0 || block > 65536) return 0;
    uint64_t o = 0;
    if (container == 1) { out[o++] = 0x78; out[o++] = 0x9C; }
    if (container == 2) { memcpy(out, gz, 10); o = 10; }
    const uint64_t nb = (n + block - 1) / block;
    uint64_t at = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        const uint32_t len = (uint32_t)(n - b * block < block ? n - b * block : block);
        block_bits[b] = 8 * o;
        const uint64_t w = orc_defz_record(tok + at, tok_sizes[b], in + b * block, len, -1, out + o, NULL);
        if (!w) return 0;
        o += w;
        at += tok_sizes[b];
    }
    block_bits[nb] = 8 * o;
    out[o++] = 0x03; out[o++] = 0x00;
    if (container == 1) {
        const uint32_t a = orc_adler32(in, n);
        for (int i = 0; i < 4; ++i) out[o++] = (uint8_t)(a >> (24 - 8 * i));
    } else if (container == 2) {
        const uint32_t c = orc_crc32(in, n), isz = (uint32_t)n;
        for (int i = 0; i < 4; ++i) out[o++] = (uint8_t)(c >> (8 * i));
        for (int i = 0; i < 4; ++i) out[o++] = (uint8_t)(isz >> (8 * i));
    }
    return o;
}
