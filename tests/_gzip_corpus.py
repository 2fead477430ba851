"""Gzip streams for the inflate tests (test_inflate_model.py, test_gpu_inflate.py,
tools/inflate_asan_check.py): what zlib writes at every level and strategy,
hand-built DEFLATE blocks (a small bit writer) for what zlib never writes, and
invalid streams with the status they must end in.  Python's zlib is the oracle
for the valid ones; an invalid one's status follows from how it is built.

corpus() -> {name: Case}; Case.status is the TSG_INFLATE_* value, Case.payload
the inflated bytes of a valid stream, Case.group the group the GPU test runs
it in.  pack() lays streams and slots out as tsg_inflate_gzip_device takes
them; run_model() calls the CPU model on such a batch between guard bytes."""
import collections
import functools
import struct
import zlib

import numpy as np

OK, HEADER, CORRUPT, EOF, CHECKSUM, DST_FULL = range(6)
TEXT = {OK: "", HEADER: "gzip: invalid header", CORRUPT: "flate: corrupt input", EOF: "unexpected EOF",
        CHECKSUM: "gzip: invalid checksum", DST_FULL: ""}

Case = collections.namedtuple("Case", "name gz status payload group")


# ---- a DEFLATE bit writer ----
class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):                        # n bits of v, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                        # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.bits((c >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


def canon(lens):
    """canonical codes of the code lengths `lens` (RFC 1951 3.2.2): {sym: (code, len)}"""
    out, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def len_sym(length):
    s = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_sym(dist):
    s = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def tokens(w, toks, lit, dist):
    """toks: ints (literal / raw symbol) and (length, distance) pairs, coded with {sym: (code, len)} maps;
    dist None: the fixed 5-bit distance codes"""
    for t in toks:
        if isinstance(t, tuple):
            s, eb, ev = len_sym(t[0])
            w.code(*lit[s])
            w.bits(ev, eb)
            d, eb, ev = dist_sym(t[1])
            if dist is None:
                w.code(d, 5)
            elif d in dist:                      # (a table without codes: the decoder fails here)
                w.code(*dist[d])
            w.bits(ev, eb)
        else:
            w.code(*lit[t])


def fixed_block(w, toks, final=True, end=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    tokens(w, toks, FIXED_LIT, None)
    if end:
        w.code(*FIXED_LIT[256])


def stored_block(w, data, final=True, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen))
    w.raw(data)


LITS = [9] * 256 + [1]                           # every literal and the end of block: Kraft sum 1
PLAIN_CL = [4] * 16 + [0, 0, 0]                  # every length 0..15 as a 4-bit code, no repeat codes


def dyn_header(w, final, lit_lens, dist_lens, cl_lens=None, cl_seq=None, hclen=None, hlit=None, hdist=None):
    """a dynamic block's header: the code lengths lit_lens + dist_lens written with the code-length code cl_lens
    (by symbol 0..18) as the sequence cl_seq of (symbol, extra value) -- default: every length on its own"""
    cl_lens = PLAIN_CL if cl_lens is None else cl_lens
    if cl_seq is None:
        cl_seq = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    if hclen is None:
        hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
    w.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cl = canon(cl_lens)
    for s, ev in cl_seq:
        w.code(*cl[s])
        w.bits(ev, {16: 2, 17: 3, 18: 7}.get(s, 0))


def dyn_block(w, toks, lit_lens, dist_lens, final=True, **kw):
    dyn_header(w, final, lit_lens, dist_lens, **kw)
    tokens(w, list(toks) + [256], canon(lit_lens), canon(dist_lens))


def expand(toks):
    """the bytes a token list inflates to"""
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def member(deflate, payload, flg=0, extra=b"", name=b"name.tar", comment=b"a comment", crc=None, isize=None, hcrc=None,
           head=None):
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\x03") if head is None else bytearray(head)
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) if hcrc is None else hcrc)
    return bytes(h) + deflate + struct.pack("<II", zlib.crc32(payload) if crc is None else crc,
                                            (len(payload) & 0xFFFFFFFF) if isize is None else isize)


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=7):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    if flush is None:
        return c.compress(data) + c.flush()
    out = b""
    for k in range(0, len(data), every):
        out += c.compress(data[k:k + every]) + c.flush(flush)
    return out + c.flush()


def py_inflate(stream):
    """zlib.decompressobj(31) chained over the members; raises where it fails"""
    out = b""
    if not stream:
        raise zlib.error("empty")
    while stream:
        d = zlib.decompressobj(31)
        out += d.decompress(stream)
        if not d.eof:
            raise zlib.error("truncated")
        stream = d.unused_data
    return out


def text(n, seed=5):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 11, 3000)]
    words += [b"\n", b"=", b"/usr/lib/", b"AKIA", b"0x%04x" % 77, b"  "]
    idx = rng.zipf(1.3, n // 4 + 16) % len(words)
    return b" ".join(words[i] for i in idx)[:n]


FIB_LITS = [ord("a") + k for k in range(14)]     # code lengths 1..14, then 256 and 257 with 15: Kraft sum 1


def fib_tables():
    lit = [0] * 258
    for k, s in enumerate(FIB_LITS):
        lit[s] = k + 1
    lit[256] = lit[257] = 15
    return lit


@functools.lru_cache(maxsize=None)
def corpus():
    cases = {}

    def add(name, stream, status=OK, payload=None, group="blocks"):
        assert name not in cases
        cases[name] = Case(name, bytes(stream), status, payload if status == OK else None, group)

    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    txt = text(150000)

    # -- what zlib writes --
    add("stored_l0", gz(rnd, 0), payload=rnd)                                     # 65535-byte stored blocks
    add("stored_65535", gz(rnd[:65535], 0), payload=rnd[:65535])
    w = Bits()
    stored_block(w, b"", final=False)
    stored_block(w, b"xyz", final=False)
    stored_block(w, b"")
    add("stored_empty", member(w.done(), b"xyz"), payload=b"xyz")
    for name, lvl, st in (("fixed", 6, zlib.Z_FIXED), ("l1", 1, 0), ("l6", 6, 0), ("l9", 9, 0),
                          ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)):
        add(name, gz(txt, lvl, st), payload=txt)
    add("l6_random", gz(rnd, 6), payload=rnd)
    add("empty", gz(b""), payload=b"")
    add("one_byte", gz(b"Q"), payload=b"Q")
    add("sync_flush", gz(txt[:3000], 6, flush=zlib.Z_SYNC_FLUSH), payload=txt[:3000], group="flush")
    add("full_flush", gz(txt[:3000], 6, flush=zlib.Z_FULL_FLUSH, every=5), payload=txt[:3000], group="flush")
    add("sync_flush_fixed", gz(txt[:2000], 6, zlib.Z_FIXED, flush=zlib.Z_SYNC_FLUSH, every=3), payload=txt[:2000],
        group="flush")
    for j in range(8):                           # the final block ends at bit 2 + j of a byte
        w = Bits()
        toks = [0xC8] * j                        # 9-bit literals
        fixed_block(w, toks)
        assert (10 + 9 * j) % 8 == (2 + j) % 8
        add("end_phase_%d" % ((2 + j) % 8), member(w.done(), expand(toks)), payload=expand(toks), group="flush")

    # -- matches and the window --
    add("run_a", gz(b"a" * 100000, 9), payload=b"a" * 100000, group="matches")    # dist 1, len 258
    add("period_2", gz(b"xy" * 30000, 9), payload=b"xy" * 30000, group="matches")
    add("period_3", gz(b"pqr" * 20000, 9), payload=b"pqr" * 20000, group="matches")
    for d in (1, 2, 3, 5, 63, 64, 65, 257):      # hand-built: every length against a short distance
        toks = list(rnd[:d]) + [(l, d) for l in (3, 4, 63, 64, 65, 130, 257, 258)]
        w = Bits()
        fixed_block(w, toks)
        add("overlap_d%d" % d, member(w.done(), expand(toks)), payload=expand(toks), group="matches")
    far = rnd[:32768]
    w = Bits()
    stored_block(w, far, final=False)
    fixed_block(w, [(258, 32768), (100, 32768)])
    add("dist_32768", member(w.done(), far + far[:358]), payload=far + far[:358], group="matches")
    w = Bits()
    stored_block(w, far[:32767], final=False)
    fixed_block(w, [(258, 32768)])
    add("dist_32768_before_start", member(w.done(), b"") + bytes(16), CORRUPT, group="invalid")
    w = Bits()                                   # a match reaching over a block boundary, of every block type
    fixed_block(w, list(b"abcdefgh"), final=False)
    fixed_block(w, [(20, 8)], final=False)
    stored_block(w, b"-stored-", final=False)
    lit = [9] * 256 + [2] + [0] * 17             # lengths 9 (symbol 263) and 30 (271), distances 8 (5) and 37 (10)
    lit[263] = lit[271] = 3
    dyn_block(w, [ord("a"), (9, 8), (30, 37)], lit, [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    toks = list(b"abcdefgh") + [(20, 8)] + list(b"-stored-") + [ord("a"), (9, 8), (30, 37)]
    add("match_over_blocks", member(w.done(), expand(toks)), payload=expand(toks), group="matches")
    toks = list(rnd[:60]) + [(10, 7), (258, 61)] + list(rnd[60:120]) + [(11, 130)]
    w = Bits()
    fixed_block(w, toks)
    add("match_over_line", member(w.done(), expand(toks)), payload=expand(toks), group="matches")

    # -- hand-built code tables --
    toks = FIB_LITS + [(3, 2), ord("n"), ord("m")] + FIB_LITS[::-1] + [(3, 2)]
    w = Bits()
    dyn_block(w, toks, fib_tables(), [0, 1])     # 15-bit codes; the one distance code of length 1 is distance 2
    add("fib_15bit", member(w.done(), expand(toks)), payload=expand(toks), group="tables")
    assert max(PLAIN_CL[CL_ORDER[k]] and k + 1 for k in range(19)) == 19          # HCLEN = 19
    toks = list(b"only literals")
    w = Bits()
    dyn_block(w, toks, LITS, [0])     # HLIT = 257, HDIST = 1, no distance code at all
    add("hlit_257_no_dist", member(w.done(), bytes(toks)), payload=bytes(toks), group="tables")
    w = Bits()
    dyn_block(w, toks, LITS, [1])     # the single distance code, unused
    add("hdist_1_unused", member(w.done(), bytes(toks)), payload=bytes(toks), group="tables")
    toks2 = [ord("z"), (258, 1), (5, 1)]
    w = Bits()
    lit = [9] * 256 + [2] + [0] * 29             # lengths 5 (symbol 259) and 258 (285): HLIT = 286
    lit[259] = lit[285] = 3
    dyn_block(w, toks2, lit, [1])                # ... used: distance 1
    add("hdist_1_used", member(w.done(), expand(toks2)), payload=expand(toks2), group="tables")
    # the same lengths written with repeat codes: 16, 17 and 18, HCLEN < 19
    cl = [0] * 19
    cl[9] = cl[16] = cl[17] = 2
    cl[18] = cl[1] = 3
    w = Bits()
    seq = [(9, 0)] + [(16, 3)] * 42 + [(16, 0)] + [(1, 0), (17, 0), (18, 0), (1, 0)]   # 9 x 256, 1, 0 x 3, 0 x 11, 1
    lit = LITS + [0] * 14
    dyn_header(w, True, lit, [1], cl_lens=cl, cl_seq=seq)
    tokens(w, toks + [256], canon(lit), canon([1]))
    assert 1 + 42 * 6 + 3 + 1 + 3 + 11 + 1 == len(lit) + 1
    add("repeat_codes", member(w.done(), bytes(toks)), payload=bytes(toks), group="tables")

    # -- headers and members --
    small = gz(b"header payload\n" * 3)[10:-8]
    for flg in range(0, 32, 2):
        add("flags_%02x" % flg, member(small, b"header payload\n" * 3, flg, extra=b"ex\0tra"),
            payload=b"header payload\n" * 3, group="headers")
    add("fextra_0", member(small, b"header payload\n" * 3, 4, extra=b""), payload=b"header payload\n" * 3, group="headers")
    add("fextra_65535", member(small, b"header payload\n" * 3, 6, extra=rnd[:65535]), payload=b"header payload\n" * 3,
        group="headers")
    add("fname_511", member(small, b"header payload\n" * 3, 8, name=b"n" * 511), payload=b"header payload\n" * 3,
        group="headers")
    add("fname_512", member(small, b"header payload\n" * 3, 8, name=b"n" * 512), HEADER, group="invalid")
    add("members_2", gz(txt[:5000]) + gz(rnd[:3000], 0), payload=txt[:5000] + rnd[:3000], group="headers")
    parts = [txt[k * 311:k * 311 + (k * 37) % 700] for k in range(50)]
    add("members_50", b"".join(gz(p, 1 + k % 9) for k, p in enumerate(parts)), payload=b"".join(parts), group="headers")
    add("members_empty", gz(b"") + gz(b"mid") + gz(b"") + gz(b""), payload=b"mid", group="headers")

    # -- one large stream --
    big = text(8 << 20, seed=9)
    add("big_8mib", gz(big, 6), payload=big, group="big")

    # -- invalid streams --
    good = gz(txt[:4000])
    tail = bytes(16)                             # so that the intended error comes before the end of the stream

    def inv(name, stream, status):
        add(name, stream, status, group="invalid")

    inv("bad_magic", b"\x1f\x8c" + good[2:], HEADER)
    inv("bad_cm", good[:2] + b"\x07" + good[3:], HEADER)
    inv("reserved_flag", good[:3] + b"\x20" + good[4:], HEADER)
    inv("bad_fhcrc", member(small, b"header payload\n" * 3, 2, hcrc=0x1234), HEADER)
    w = Bits()
    w.bits(1, 1)
    w.bits(3, 2)
    inv("btype_3", member(w.done() + tail, b""), CORRUPT)
    w = Bits()
    stored_block(w, b"hello", nlen=5)
    inv("len_nlen", member(w.done() + tail, b"hello"), CORRUPT)

    def dyn_invalid(name, status=CORRUPT, **kw):
        w = Bits()
        kw.setdefault("lit_lens", LITS)
        kw.setdefault("dist_lens", [1])
        dyn_header(w, True, **kw)
        w.bits(0, 7)
        inv(name, member(w.done() + tail, b""), status)

    dyn_invalid("over_lit", lit_lens=[1, 1, 1] + [0] * 253 + [2])
    dyn_invalid("over_dist", dist_lens=[1, 1, 1])
    dyn_invalid("over_cl", cl_lens=[1, 1, 1] + [0] * 16, cl_seq=[])
    dyn_invalid("incomplete_lit", lit_lens=[2] + [0] * 255 + [2])
    dyn_invalid("incomplete_dist", dist_lens=[2])
    dyn_invalid("hlit_287", hlit=30, cl_seq=[])
    dyn_invalid("hlit_288", hlit=31, cl_seq=[])
    dyn_invalid("hdist_31", hdist=30, cl_seq=[])
    dyn_invalid("hdist_32", hdist=31, cl_seq=[])
    cl16 = [1] + [0] * 15 + [1, 0, 0]
    dyn_invalid("repeat_16_first", cl_lens=cl16, cl_seq=[(16, 0)])
    cl18 = [1] + [0] * 17 + [1]
    dyn_invalid("repeat_overrun", cl_lens=cl18, cl_seq=[(18, 127), (18, 127)])     # 138 + 138 > 257 + 1
    # HCLEN = 4 can only name the lengths of 16, 17, 18 and 0: every code length is 0 and the first symbol fails
    dyn_invalid("hclen_4_empty_lit", lit_lens=[0] * 257, dist_lens=[0], cl_lens=[1] + [0] * 17 + [1],
                cl_seq=[(18, 127), (18, 109)], hclen=4)
    for s in (286, 287):
        w = Bits()
        fixed_block(w, [ord("a"), s], end=False)
        inv("lit_sym_%d" % s, member(w.done() + tail, b""), CORRUPT)
    for d in (30, 31):
        w = Bits()
        fixed_block(w, [ord("a")], end=False)
        w.code(*FIXED_LIT[257])
        w.code(d, 5)
        inv("dist_sym_%d" % d, member(w.done() + tail, b""), CORRUPT)
    w = Bits()
    fixed_block(w, [ord("a"), (3, 2)])
    inv("dist_before_start", member(w.done() + tail, b""), CORRUPT)
    inv("dist_into_first_member", good + member(w.done() + tail, b""), CORRUPT)
    w = Bits()
    dyn_block(w, [ord("a"), (3, 1)], [9] * 256 + [2, 2], [0])
    inv("dist_from_empty_table", member(w.done() + tail, b""), CORRUPT)
    inv("bad_crc", good[:-8] + struct.pack("<I", zlib.crc32(txt[:4000]) ^ 1) + good[-4:], CHECKSUM)
    inv("bad_isize", good[:-4] + struct.pack("<I", 3999), CHECKSUM)
    inv("bad_crc_then_corrupt", good[:-8] + b"\0\0\0\0" + good[-4:] + cases["btype_3"].gz, CHECKSUM)
    inv("trailing_zero", good + b"\0", EOF)       # Go reads ten header bytes first; Python's gzip module accepts it
    inv("trailing_zeros_16", good + bytes(16), HEADER)
    inv("trailing_garbage", good + b"garbage behind the stream", HEADER)
    inv("no_bytes", b"", EOF)
    w = Bits()
    stored_block(w, b"stored payload, a few bytes of it")
    trunc_src = {"stored": member(w.done(), b"stored payload, a few bytes of it"),
                 "fixed": gz(b"fixed block payload payload", 6, zlib.Z_FIXED),
                 "dynamic": gz(txt[:160], 9)}
    assert trunc_src["dynamic"][10] & 6 == 4     # a dynamic block
    for kind, s in trunc_src.items():
        add("small_" + kind, s, payload=py_inflate(s), group="small")
        for k in range(len(s)):
            add("trunc_%s_%03d" % (kind, k), s[:k], EOF, group="truncated")
    return cases


def remainder(case):
    """what follows a truncated stream in the buffer: the rest of the stream it was cut from"""
    kind, k = case.name.split("_")[1], int(case.name.split("_")[2])
    return corpus()["small_" + kind].gz[k:]


@functools.lru_cache(maxsize=None)
def batch_300():
    """300 streams whose lengths spread over three orders of magnitude, valid and invalid mixed"""
    c = corpus()
    rng = np.random.default_rng(3)
    out = [c[n] for n in c if c[n].group in ("tables", "flush", "invalid")][:110]
    out += [c[n] for n in list(c) if c[n].group == "truncated"][::9][:30]
    src = text(400000, seed=21)
    k = 0
    while len(out) < 300:
        n = int(10 ** rng.uniform(1.5, 5.0))
        at = int(rng.integers(0, len(src) - n))
        p = src[at:at + n]
        out.append(Case("gen_%03d" % k, gz(p, int(rng.integers(0, 10))), OK, p, "batch"))
        k += 1
    lens = [len(x.gz) for x in out]
    assert max(lens) > 1000 * max(1, min(l for l in lens if l))
    return out


def align16(n):
    return (n + 15) & ~15


def pack(streams, caps, gaps=None):
    """(gz bytes + 16 of padding, gz_offsets, dst_offsets) for streams in slots of caps[i] bytes; gaps[i]: bytes
    laid behind stream i as a stream of its own (returned offsets then count 2 n streams, the odd ones the gaps)"""
    items, slot = [], []
    for i, s in enumerate(streams):
        items.append(s)
        slot.append(caps[i])
        if gaps is not None:
            items.append(gaps[i])
            slot.append(0)
    go = np.zeros(len(items) + 1, np.uint64)
    go[1:] = np.cumsum([len(s) for s in items])
    do = np.zeros(len(items) + 1, np.uint64)
    sizes = [align16(c) for c in slot]
    sizes[-1] = slot[-1]                         # the last slot may have any size
    do[1:] = np.cumsum(sizes)
    buf = np.frombuffer(b"".join(items) + b"\xEE" * 16, np.uint8).copy()
    return buf, go, do


def default_cap(case):
    return len(case.payload) if case.status == OK else 40000 if case.group == "invalid" else 4096


GUARD = 256
FILL = 0xA5


def run_model(streams, caps, gaps=None):
    """tsg_test_inflate_model over pack(streams, caps, gaps) into a 0xA5-filled buffer with GUARD bytes on both
    sides: (rc, message, status, out_lens, dst without the guards, dst_offsets); checks the guards"""
    from trivy_amd import _lib
    L = _lib.lib()
    buf, go, do = pack(streams, caps, gaps)
    n = len(go) - 1
    dst = np.full(int(do[-1]) + 2 * GUARD, FILL, np.uint8)
    out_lens, status = np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    rc = L.tsg_test_inflate_model(None, buf.ctypes.data, go.ctypes.data, n, dst.ctypes.data + GUARD, do.ctypes.data,
                                  out_lens.ctypes.data, status.ctypes.data, None)
    msg = L.tsg_last_error().decode() if rc else ""
    assert (dst[:GUARD] == FILL).all() and (dst[len(dst) - GUARD:] == FILL).all()
    return rc, msg, status.tolist(), out_lens.tolist(), dst[GUARD:len(dst) - GUARD], do.tolist()


def check_slots(streams_status, out_lens, dst, do, only_good=True):
    """outside every good stream's [begin, begin + out_len) the fill is intact (a failed stream may dirty its slot)"""
    for i, st in enumerate(streams_status):
        b, e = int(do[i]), int(do[i + 1])
        if st == OK or not only_good:
            assert (dst[b + int(out_lens[i]):e] == FILL).all(), i
