// bgzf_ranges.hip — many (offset, length) slices of a BGZF stream's UNCOMPRESSED bytes in one call: what tabix / BAI region
// queries and bgzf_seek + bgzf_read ask for.  Device arrays in, one verdict per range on the device, one launch set, nothing
// read back.  include/mi_codec.h has the contract.
//
// A PIECE is one (range, non-empty member) pair.  A piece whose member lies wholly inside the range is INTERIOR and is decoded
// straight to its place in the range's slot; a piece whose member is cut by the range's start or end is an EDGE piece: the
// whole member is decoded into a 64 KiB cell of a scratch area in the context workspace and the slice copied from there.  So
// every member that is read is decoded whole by k_inflate<.., DESC> as it is (no second token loop) and its CRC-32 stays
// checkable.  A range has at most two edge pieces: edge slot 2 i (its first piece) and 2 i + 1 (any later one).
//
//   k_bgzr_members  one workgroup over the table: the members whose output offsets differ (ISIZE > 0), compacted, so that
//                   nobody walks empty members
//   k_bgzr_plan     one thread per range: the slot against out_bytes (MI_ERR_ARG), the clip against the total, two binary
//                   searches over the compacted members for the first and last piece
//   k_bgzr_scan     one workgroup: the exclusive scan of the piece counts, MI_ERR_ARG where the caller's bound is passed,
//                   the real piece count
//   k_bgzr_fill     one thread per piece of the bound: its range (binary search over the scan), the member's pairs and its
//                   header checked against the stream (bgzf_member_seg, bgzf_core.h), interior or edge -> an InfSeg, a status
//                   word and, for an edge piece, what k_bgzr_place copies; pieces beyond the real count are inert
//   (k_inflate over the interior descriptors with base d_out; then per group of BGZR_GROUP edge slots: k_inflate with base
//    scratch, k_bgzf_check, k_bgzr_place — the scratch area is one group's cells and is used again by the next group)
//   k_bgzr_place    one workgroup per edge slot: scratch[lo, hi) -> its place in the slot
//   k_bgzr_finish   one thread per range: the pieces' status words folded into d_status[i], d_got[i] and *d_failed
//
// Status word of a piece or an edge slot: 0 decode it / it decoded, 1 refused or failed, 2 nothing here (an interior word
// of 2 inside a range means: this piece is an edge piece, look at the range's edge slot).  k_inflate and k_bgzf_check skip
// every word that is not 0 and set 1.
#include "lz_common.h"
#include "internal.h"
#include "bgzf_core.h"

#define BGZR_CELL    65536u                    // a member inflates to at most this
#define BGZR_GROUP   4096u                     // edge slots decoded per launch set: 256 MiB of scratch at most
#define BGZR_HEAD    256u                      // workspace head: u32 nnz (non-empty members), u32 nreal (pieces)
#define BGZR_SKIP    2u

struct BgzrPlace { uint64_t dst, slot_lo, slot_hi; uint32_t lo, hi; };     // cell bytes [lo, hi) -> d_out[dst ...), inside the slot

struct BgzrCall {
    const uint8_t *stream; uint64_t nbytes;
    const uint64_t *members; uint64_t n_members;
    uint64_t count; const uint64_t *off, *len;
    uint8_t *out; const uint64_t *out_off; uint64_t out_bytes, max_pieces;
    uint64_t *got; uint32_t *status, *failed;
};

struct BgzrWs {
    uint8_t   *head;
    uint32_t  *nz;                             // [n_members] the non-empty members, ascending
    uint32_t  *r_k0, *r_np, *r_st, *r_first;   // [count] first compacted member, pieces, verdict so far, first piece (clamped)
    InfSeg    *seg_i; uint32_t *st_i;          // [max_pieces] interior descriptors and status words
    InfSeg    *seg_e; uint32_t *st_e;          // [2 count] edge slots
    BgzrPlace *place;                          // [2 count]
    uint8_t   *cells;                          // [min(2 count, BGZR_GROUP)] x 64 KiB
    size_t     bytes;
};

static BgzrWs bgzr_carve(void *ws, const BgzrCall &c)
{
    mi_carver cv(ws);
    BgzrWs w;
    const size_t ne = 2 * (size_t)c.count;
    w.head = cv.take<uint8_t>(BGZR_HEAD);
    w.nz = cv.take<uint32_t>(c.n_members);
    w.r_k0 = cv.take<uint32_t>(c.count); w.r_np = cv.take<uint32_t>(c.count);
    w.r_st = cv.take<uint32_t>(c.count); w.r_first = cv.take<uint32_t>(c.count);
    w.seg_i = cv.take<InfSeg>(c.max_pieces); w.st_i = cv.take<uint32_t>(c.max_pieces);
    w.seg_e = cv.take<InfSeg>(ne); w.st_e = cv.take<uint32_t>(ne);
    w.place = cv.take<BgzrPlace>(ne);
    w.cells = cv.take<uint8_t>((ne < BGZR_GROUP ? ne : (size_t)BGZR_GROUP) * BGZR_CELL);
    w.bytes = cv.bytes();
    return w;
}

struct OpAddU64r { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; } };

// output offset of pair m of the table
__device__ __forceinline__ uint64_t bgzr_o(const uint64_t *__restrict__ members, uint64_t m) { return members[2u * m + 1u]; }

__global__ __launch_bounds__(1024)
void k_bgzr_members(const uint64_t *__restrict__ members, uint32_t n_members, uint32_t *__restrict__ nz, uint32_t *__restrict__ nnz)
{
    __shared__ uint32_t s_tmp[18];
    const uint32_t tid = threadIdx.x;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n_members; base += 1024u) {         // (uniform: every thread takes every round)
        const uint32_t m = base + tid;
        // "not empty" is "the offsets differ": a member of a decreasing table is a piece too, and is refused as one
        const uint32_t f = (m < n_members && bgzr_o(members, m) != bgzr_o(members, m + 1ull)) ? 1u : 0u;
        uint32_t tot;
        const uint32_t at = run + block_exclusive_scan<uint32_t>(f, OpAddU32(), 0u, s_tmp, &tot);
        if (f) nz[at] = m;
        run += tot;
    }
    if (tid == 0) *nnz = run;
}

__global__ __launch_bounds__(256)
void k_bgzr_plan(BgzrCall c, const uint32_t *__restrict__ nz, const uint32_t *__restrict__ nnz_p, uint32_t *__restrict__ r_k0,
                 uint32_t *__restrict__ r_np, uint32_t *__restrict__ r_st)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.count) return;
    const uint64_t a = c.off[i], len = c.len[i], at = c.out_off[i];
    const uint64_t total = bgzr_o(c.members, c.n_members);
    const uint32_t nnz = *nnz_p;
    uint32_t st = MI_OK, k0 = 0, np = 0;
    if (len && (at > c.out_bytes || len > c.out_bytes - at)) st = MI_ERR_ARG;          // the slot leaves [0, out_bytes)
    else if (len && a < total) {
        const uint64_t b = len < total - a ? a + len : total;
        // the first member that ends behind a, the last one that starts before b.  The table is untrusted: the searches end
        // whatever it holds, and k_bgzr_fill checks that the pieces found cover [a, b) exactly
        uint32_t lo = 0, hi = nnz;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (bgzr_o(c.members, nz[mid] + 1ull) > a) hi = mid; else lo = mid + 1u; }
        k0 = lo;
        lo = k0; hi = nnz;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (bgzr_o(c.members, nz[mid]) >= b) hi = mid; else lo = mid + 1u; }
        if (lo <= k0) st = MI_ERR_CORRUPT;                              // bytes in [a, b) and no member that holds them
        else np = lo - k0;
    }
    r_k0[i] = k0; r_np[i] = np; r_st[i] = st;
}

__global__ __launch_bounds__(1024)
void k_bgzr_scan(uint32_t count, uint64_t max_pieces, const uint32_t *__restrict__ r_np, uint32_t *__restrict__ r_st,
                 uint32_t *__restrict__ r_first, uint32_t *__restrict__ nreal)
{
    __shared__ uint64_t s_tmp[18];
    __shared__ uint32_t s_real;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_real = 0;
    __syncthreads();
    uint64_t run = 0;                                                  // pieces of the ranges before this round (uniform)
    for (uint32_t base = 0; base < count; base += 1024u) {
        const uint32_t i = base + tid;
        const uint64_t np = i < count ? r_np[i] : 0u;
        uint64_t tot;
        const uint64_t first = run + block_exclusive_scan<uint64_t>(np, OpAddU64r(), 0ull, s_tmp, &tot);
        if (i < count) {
            // a range whose pieces do not fit the bound is refused, and with it every range behind it (their first piece lies
            // past the bound too); the ranges before it are untouched
            uint32_t st = r_st[i];
            if (st == MI_OK && first + np > max_pieces) { st = MI_ERR_ARG; r_st[i] = st; }
            if (st == MI_OK && np) atomicMax(&s_real, (uint32_t)(first + np));
            r_first[i] = (uint32_t)(first < max_pieces ? first : max_pieces);
        }
        run += tot;
    }
    __syncthreads();
    if (tid == 0) *nreal = s_real;
}

__global__ __launch_bounds__(256)
void k_bgzr_fill(BgzrCall c, const uint32_t *__restrict__ nz, const uint32_t *__restrict__ r_k0, const uint32_t *__restrict__ r_np,
                 const uint32_t *__restrict__ r_st, const uint32_t *__restrict__ r_first, const uint32_t *__restrict__ nreal,
                 InfSeg *__restrict__ seg_i, uint32_t *__restrict__ st_i, InfSeg *__restrict__ seg_e, uint32_t *__restrict__ st_e,
                 BgzrPlace *__restrict__ place)
{
    const uint64_t g64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g64 >= c.max_pieces) return;
    const uint32_t g = (uint32_t)g64;
    InfSeg d = {0, 0, 0, 0, 0};
    if (g >= *nreal) { seg_i[g] = d; st_i[g] = BGZR_SKIP; return; }    // inert: nobody decodes it
    // the last range whose first piece is <= g: ranges without pieces share their first piece with the next range that has
    // some, which comes last among them; refused ranges start at or behind the real count (k_dfb_fill, deflate_batch.hip)
    uint32_t lo = 0, hi = (uint32_t)c.count - 1u;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (r_first[mid] <= g) lo = mid; else hi = mid - 1u; }
    const uint32_t i = lo, j = g - r_first[i], np = r_np[i];
    if (r_st[i] != MI_OK || j >= np) { seg_i[g] = d; st_i[g] = BGZR_SKIP; return; }
    const uint64_t a = c.off[i], len = c.len[i], total = bgzr_o(c.members, c.n_members);
    const uint64_t b = len < total - a ? a + len : total;              // (a < total: the range has pieces)
    const uint64_t m = nz[r_k0[i] + j];
    const uint64_t s0 = c.members[2u * m], o0 = c.members[2u * m + 1u], s1 = c.members[2u * m + 2u], o1 = c.members[2u * m + 3u];
    // the member as the table and its own header give it; it holds bytes of [a, b); the first piece starts at or before a and
    // the last one ends at or behind b.  Neighbouring pieces touch by construction (only members whose two offsets are equal
    // lie between them), so pieces that all pass cover [a, b) exactly once.
    bool ok = bgzf_member_seg(c.stream, c.nbytes, s0, o0, s1, o1, d);
    ok = ok && o0 < b && o1 > a && (j != 0u || o0 <= a) && (j + 1u != np || o1 >= b);
    if (!ok) { seg_i[g] = InfSeg{0, 0, 0, 0, 0}; st_i[g] = 1u; return; }
    const uint64_t slot = c.out_off[i];
    if (o0 >= a && o1 <= b) {                                           // interior: straight to its place in the slot
        d.out_off = slot + (o0 - a);
        seg_i[g] = d; st_i[g] = 0u;
        return;
    }
    const uint64_t from = o0 > a ? o0 : a, to = o1 < b ? o1 : b;
    const uint32_t e = 2u * i + (j != 0u ? 1u : 0u);
    seg_i[g] = InfSeg{0, 0, 0, 0, 0}; st_i[g] = BGZR_SKIP;
    d.out_off = (uint64_t)(e % BGZR_GROUP) * BGZR_CELL;
    seg_e[e] = d;
    place[e] = BgzrPlace{slot + (from - a), slot, slot + len, (uint32_t)(from - o0), (uint32_t)(to - o0)};
    st_e[e] = 0u;
}

// cell bytes [lo, hi) of edge slot e0 + blockIdx.x to their place: bytes up to the destination's first 16-byte boundary,
// 16-byte stores (the source dwords shifted where source and destination differ modulo 4, read as they lie where they agree
// modulo 16), bytes behind the last one.  Every store is checked against the slot.
__global__ __launch_bounds__(256)
void k_bgzr_place(const uint8_t *__restrict__ cells, const BgzrPlace *__restrict__ place, const uint32_t *__restrict__ st_e,
                  const uint32_t *__restrict__ r_st, uint8_t *__restrict__ out, uint32_t e0)
{
    const uint32_t tid = threadIdx.x, e = e0 + blockIdx.x;
    if (st_e[e] != 0u || r_st[e >> 1] != MI_OK) return;                 // (the whole workgroup) nothing here, or failed already
    const BgzrPlace p = place[e];
    const uint8_t *cell = cells + (size_t)blockIdx.x * BGZR_CELL;
    if (p.hi > BGZR_CELL || p.lo > p.hi) return;
    const uint32_t n = p.hi - p.lo;
    auto inside = [&](uint64_t at, uint32_t w) { return at >= p.slot_lo && at + w <= p.slot_hi; };
    uint32_t head = (16u - (uint32_t)((uintptr_t)(out + p.dst) & 15u)) & 15u;
    if (head > n) head = n;
    if (tid < head && inside(p.dst + tid, 1u)) out[p.dst + tid] = cell[p.lo + tid];
    const uint32_t nv = (n - head) >> 4, src0 = p.lo + head;
    const uint32_t *C = reinterpret_cast<const uint32_t *>(cell);      // (the cell is 256-byte aligned and 16 384 dwords long)
    if ((src0 & 15u) == 0u) {
        for (uint32_t v = tid; v < nv; v += 256u) {
            const uint4 q = *reinterpret_cast<const uint4 *>(cell + src0 + 16u * v);
            const uint64_t at = p.dst + head + 16ull * v;
            if (inside(at, 16u)) *reinterpret_cast<uint4 *>(out + at) = q;
        }
    } else {
        const uint32_t w0 = src0 >> 2, sh = 8u * (src0 & 3u);
        for (uint32_t v = tid; v < nv; v += 256u) {
            uint32_t w[5];
#pragma unroll
            for (uint32_t k = 0; k < 5u; ++k) { const uint32_t x = w0 + 4u * v + k; w[k] = x < BGZR_CELL / 4u ? C[x] : 0u; }
            uint4 q;
            q.x = sh ? (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> sh) : w[0];
            q.y = sh ? (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> sh) : w[1];
            q.z = sh ? (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> sh) : w[2];
            q.w = sh ? (uint32_t)((((uint64_t)w[4] << 32) | w[3]) >> sh) : w[3];
            const uint64_t at = p.dst + head + 16ull * v;
            if (inside(at, 16u)) *reinterpret_cast<uint4 *>(out + at) = q;
        }
    }
    const uint32_t t0 = head + 16u * nv;                                // (at most fifteen bytes)
    if (t0 + tid < n && inside(p.dst + t0 + tid, 1u)) out[p.dst + t0 + tid] = cell[p.lo + t0 + tid];
}

__global__ __launch_bounds__(256)
void k_bgzr_finish(BgzrCall c, const uint32_t *__restrict__ r_np, const uint32_t *__restrict__ r_st, const uint32_t *__restrict__ r_first,
                   const uint32_t *__restrict__ st_i, const uint32_t *__restrict__ st_e)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.count) return;
    uint32_t st = r_st[i];
    uint64_t got = 0;
    if (st == MI_OK) {
        const uint32_t np = r_np[i], first = r_first[i];
        for (uint32_t j = 0; j < np && st == MI_OK; ++j) {
            uint32_t v = st_i[first + j];
            if (v == BGZR_SKIP) v = st_e[2u * i + (j != 0u ? 1u : 0u)];    // an edge piece: the range's own slot
            if (v != 0u) st = MI_ERR_CORRUPT;
        }
        if (st == MI_OK && np) {
            const uint64_t a = c.off[i], len = c.len[i], total = bgzr_o(c.members, c.n_members);
            got = len < total - a ? len : total - a;
        }
    }
    c.status[i] = st;
    c.got[i] = got;
    if (st != MI_OK && c.failed) atomicAdd(c.failed, 1u);
}

extern "C" uint64_t mi_bgzf_read_max_pieces(uint64_t count, uint64_t total_len, uint64_t min_member_bytes)
{
    // a range of len bytes over members of at least m bytes holds at most (len - 2) / m whole ones between its two cut ones
    return count + total_len / (min_member_bytes ? min_member_bytes : 1u) + count;
}

extern "C" mi_status mi_bgzf_read_ranges_dev(mi_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_members,
                                             uint64_t n_members, uint64_t count, const uint64_t *d_off, const uint64_t *d_len,
                                             uint8_t *d_out, const uint64_t *d_out_off, uint64_t out_bytes, uint64_t max_pieces,
                                             uint64_t *d_got, uint32_t *d_status, uint32_t *d_failed, uint32_t flags, void *stream)
{
    if (!ctx || (stream_bytes && !d_stream) || !d_members || (out_bytes && !d_out)) return MI_ERR_ARG;
    if ((flags & ~MI_INFLATE_NO_CHECKSUM) || ((uintptr_t)d_stream & 3u) || stream_bytes > (UINT64_MAX >> 4)) return MI_ERR_ARG;
    if (count > BGZR_MAX / 2u || n_members > BGZR_MAX || max_pieces > BGZR_MAX) return MI_ERR_ARG;
    if (count == 0) return MI_OK;
    if (!d_off || !d_len || !d_out_off || !d_got || !d_status) return MI_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const BgzrCall c{d_stream, stream_bytes, d_members, n_members, count, d_off, d_len, d_out, d_out_off, out_bytes, max_pieces,
                     d_got, d_status, d_failed};
    mi_status st = mi_ws_reserve(ctx, bgzr_carve(nullptr, c).bytes);
    if (st) return st;
    const BgzrWs w = bgzr_carve(ctx->ws, c);
    const uint32_t ne = 2u * (uint32_t)count, np = (uint32_t)max_pieces;
    uint32_t *nnz = reinterpret_cast<uint32_t *>(w.head), *nreal = nnz + 1;
    MI_HIP(ctx, hipMemsetAsync(w.head, 0, BGZR_HEAD, s));
    MI_HIP(ctx, hipMemsetAsync(w.st_e, (int)BGZR_SKIP, (size_t)ne * 4u, s));    // (any word that is not 0 is skipped)
    if (d_failed) MI_HIP(ctx, hipMemsetAsync(d_failed, 0, 4, s));
    const unsigned rgrid = (unsigned)((count + 255u) / 256u);
    {
        mi_prof_scope pr(ctx, "k_bgzr_plan", s, 0);
        hipLaunchKernelGGL(k_bgzr_members, dim3(1), dim3(1024), 0, s, d_members, (uint32_t)n_members, w.nz, nnz);
        hipLaunchKernelGGL(k_bgzr_plan, dim3(rgrid), dim3(256), 0, s, c, w.nz, nnz, w.r_k0, w.r_np, w.r_st);
        hipLaunchKernelGGL(k_bgzr_scan, dim3(1), dim3(1024), 0, s, (uint32_t)count, max_pieces, w.r_np, w.r_st, w.r_first, nreal);
        if (np) hipLaunchKernelGGL(k_bgzr_fill, dim3((np + 255u) / 256u), dim3(256), 0, s, c, w.nz, w.r_k0, w.r_np, w.r_st, w.r_first, nreal,
                                   w.seg_i, w.st_i, w.seg_e, w.st_e, w.place);
    }
    const bool check = !(flags & MI_INFLATE_NO_CHECKSUM);
    if (np) {
        {
            mi_prof_scope pr(ctx, "k_inflate", s, 0);
            inflate_launch_segments(d_stream, stream_bytes, w.seg_i, np, d_out, nullptr, s, w.st_i);
        }
        if (check) { mi_prof_scope pr(ctx, "k_bgzf_check", s, 0); bgzf_launch_check(d_out, w.seg_i, np, nullptr, s, w.st_i); }
        // the edge slots, one group of cells at a time: every launch behind the first waits for the one before it on `s`, so a
        // group's cells are read (k_bgzr_place) before the next group decodes into them
        for (uint32_t e0 = 0; e0 < ne; e0 += BGZR_GROUP) {
            const uint32_t n = ne - e0 < BGZR_GROUP ? ne - e0 : BGZR_GROUP;
            {
                mi_prof_scope pr(ctx, "k_inflate", s, 0);
                inflate_launch_segments(d_stream, stream_bytes, w.seg_e + e0, n, w.cells, nullptr, s, w.st_e + e0);
            }
            if (check) { mi_prof_scope pr(ctx, "k_bgzf_check", s, 0); bgzf_launch_check(w.cells, w.seg_e + e0, n, nullptr, s, w.st_e + e0); }
            mi_prof_scope pr(ctx, "k_bgzr_place", s, 0);
            hipLaunchKernelGGL(k_bgzr_place, dim3(n), dim3(256), 0, s, w.cells, w.place, w.st_e, w.r_st, d_out, e0);
        }
    }
    {
        mi_prof_scope pr(ctx, "k_bgzr_finish", s, 0);
        hipLaunchKernelGGL(k_bgzr_finish, dim3(rgrid), dim3(256), 0, s, c, w.r_np, w.r_st, w.r_first, w.st_i, w.st_e);
    }
    MI_HIP(ctx, hipGetLastError());
    return MI_OK;
}
