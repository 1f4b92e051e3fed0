"""A small pure-Python RFC 1951 reader for the tests (a helper module, not a conftest).

read(buf, pos=0) walks DEFLATE blocks from byte `pos` until a block with BFINAL = 1 (or, with stop_at_end=False, until the
input runs out on a block boundary) and returns a Stream: the blocks with their type, their code lengths (dynamic blocks)
and their tokens, and the inflated bytes.  Tokens are (byte,) for a literal and (length, distance) for a match.
"""
from dataclasses import dataclass, field

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class DeflateError(ValueError):
    pass


@dataclass
class Block:
    btype: int
    final: int
    lit_lengths: list = None
    dist_lengths: list = None
    cl_lengths: list = None
    tokens: list = field(default_factory=list)
    start_bit: int = 0


@dataclass
class Stream:
    blocks: list
    data: bytes
    end_bit: int                     # bit position after the last block read

    @property
    def tokens(self):
        return [t for b in self.blocks for t in b.tokens]


class _Bits:
    def __init__(self, buf, pos):
        self.buf, self.pos = buf, pos * 8

    def get(self, k):
        v = 0
        for i in range(k):
            byte = self.pos >> 3
            if byte >= len(self.buf):
                raise DeflateError("read past the end")
            v |= ((self.buf[byte] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7


def kraft(lengths):
    """Kraft sum of a set of code lengths as a fraction numerator over 2^max (0 lengths ignored): (num, 2^max)"""
    used = [l for l in lengths if l]
    if not used:
        return 0, 1
    m = max(used)
    return sum(1 << (m - l) for l in used), 1 << m


class _Decoder:
    def __init__(self, lengths):
        self.table = {}
        code, nxt = 0, {}
        mx = max(lengths) if lengths else 0
        cnt = [0] * (mx + 2)
        for l in lengths:
            if l:
                cnt[l] += 1
        for l in range(1, mx + 1):
            code = (code + cnt[l - 1]) << 1 if l > 1 else 0
            nxt[l] = code
        for s, l in enumerate(lengths):
            if l:
                self.table[(l, nxt[l])] = s
                nxt[l] += 1
        self.max = mx

    def read(self, br):
        code = 0
        for l in range(1, self.max + 1):
            code = (code << 1) | br.get(1)
            s = self.table.get((l, code))
            if s is not None:
                return s
        raise DeflateError("no such code")


def read(buf, pos=0, stop_at_end=True, out=None):
    buf = bytes(buf)
    br = _Bits(buf, pos)
    out = bytearray() if out is None else bytearray(out)
    base = len(out)
    blocks = []
    while True:
        if not stop_at_end and br.pos >= len(buf) * 8:
            break
        b = Block(btype=-1, final=0, start_bit=br.pos)
        b.final = br.get(1)
        b.btype = br.get(2)
        if b.btype == 0:
            br.align()
            ln, nln = br.get(16), br.get(16)
            if ln != (~nln & 0xFFFF):
                raise DeflateError("stored LEN / NLEN")
            for _ in range(ln):
                c = br.get(8)
                out.append(c)
                b.tokens.append((c,))
        elif b.btype in (1, 2):
            if b.btype == 1:
                ll, dl = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = br.get(3)
                b.cl_lengths = cl
                cdec = _Decoder(cl)
                seq = []
                while len(seq) < hlit + hdist:
                    s = cdec.read(br)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        if not seq:
                            raise DeflateError("repeat with no previous length")
                        seq += [seq[-1]] * (3 + br.get(2))
                    elif s == 17:
                        seq += [0] * (3 + br.get(3))
                    else:
                        seq += [0] * (11 + br.get(7))
                if len(seq) != hlit + hdist:
                    raise DeflateError("code lengths overrun")
                ll, dl = seq[:hlit], seq[hlit:]
                b.lit_lengths, b.dist_lengths = ll, dl
            ldec, ddec = _Decoder(ll), _Decoder(dl)
            while True:
                s = ldec.read(br)
                if s < 256:
                    out.append(s)
                    b.tokens.append((s,))
                elif s == 256:
                    break
                else:
                    i = s - 257
                    if i >= 29:
                        raise DeflateError("bad length code")
                    L = LEN_BASE[i] + br.get(LEN_EXTRA[i])
                    dc = ddec.read(br)
                    if dc >= 30:
                        raise DeflateError("bad distance code")
                    d = DIST_BASE[dc] + br.get(DIST_EXTRA[dc])
                    if d > len(out):
                        raise DeflateError("distance too far back")
                    for _ in range(L):
                        out.append(out[-d])
                    b.tokens.append((L, d))
        else:
            raise DeflateError("BTYPE 11")
        blocks.append(b)
        if b.final and stop_at_end:
            break
    return Stream(blocks=blocks, data=bytes(out[base:]), end_bit=br.pos)
