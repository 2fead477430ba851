"""Host side of the split block mode of the 6-bit wire codec
(trivy_amd/csrc/wirepack.cpp, wirepack.h) through tsg_test_wire_pack3.

model() below extends test_wirepack2.model by the fourth mode: per block the
sizes of all four modes from the size formulas in wirepack.h, the smallest
(of equal sizes raw, then 7-bit, then 6-bit, then split), and the exact bytes
of a split block: mask, hot nibbles, 5-bit values, escaped bytes, one zero pad
to 16.  The model, the scalar path and every SIMD path the CPU has must agree
byte for byte, and the host unpack must give the source back.

tools/wirepack_tool.cpp (check3) runs such cases under AddressSanitizer without
Python.
"""
import ctypes

import numpy as np
import pytest

import test_wirepack2 as W2
from test_wirepack2 import BLOCK, REGION, SAMPLE, RAW, SIX, PUNCT, alpha_bytes, alphabet, noise, pad, words
from trivy_amd import _lib

SPLIT = RAW | SIX
HOT, WARM, ESC5 = 16, 47, 31
PATHS = {1: "scalar", 2: "avx2", 3: "avx512"}


def split_bytes(ln, h, e):
    """wire2_split_bytes of wirepack.h"""
    return pad(-(-ln // 8) + (h + 1) // 2 + (5 * (ln - h) + 7) // 8 + e, 16)


def pack3(buf, path=0, offset=0):
    """as test_wirepack2.pack2, split blocks allowed; counts has a fifth value, the split blocks"""
    a = np.frombuffer(bytes(offset) + bytes(buf), dtype=np.uint8).copy()
    n = len(a) - offset
    packed = np.zeros(n + 16, np.uint8)
    table = np.zeros(max(1, -(-n // BLOCK)), np.uint32)
    alpha = np.full(max(1, alpha_bytes(n)), 0xEE, np.uint8)
    back = np.full(max(1, n), 0xEE, np.uint8)
    counts = np.zeros(5, np.uint64)
    plen, used, vbmi2 = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().tsg_test_wire_pack3(a.ctypes.data + offset, n, path, packed.ctypes.data, len(packed),
                                              table.ctypes.data, alpha.ctypes.data, ctypes.byref(plen),
                                              ctypes.byref(used), ctypes.byref(vbmi2), counts.ctypes.data,
                                              back.ctypes.data))
    VBMI2[0] = bool(vbmi2.value)
    return (packed[:plen.value].tobytes(), table[:-(-n // BLOCK)].tolist(), alpha[:alpha_bytes(n)].tobytes(), used.value,
            [int(c) for c in counts], back[:n].tobytes())


VBMI2 = [None]      # whether path 3 packs split blocks with AVX-512 VBMI2 here (else: the AVX2 lookup), by the last pack3()


def packer_of(used):
    """the split packer that ran for the path pack3() reports"""
    return {1: "scalar", 2: "avx2 lookup"}.get(used, "avx512 vbmi2" if VBMI2[0] else "avx2 lookup, avx512 emit")


def bits_le(vals, width):
    """the values, `width` bits each, as a little-endian bit string (whole bytes, zero pad bits)"""
    v = np.asarray(vals, np.uint8)
    bits = ((v[:, None] >> np.arange(width, dtype=np.uint8)) & 1).astype(np.uint8).ravel()
    return np.packbits(bits, bitorder="little").tobytes()


def model(buf, split=True):
    """(packed, table, alphabets, [6-bit, 7-bit, raw blocks, escaped bytes, split blocks]) of the strip buf"""
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = len(a)
    alpha = bytearray(alpha_bytes(n))
    out, table, counts = bytearray(), [], [0, 0, 0, 0, 0]
    code = None
    for b in range(0, n, BLOCK):
        if b % REGION == 0:
            al = alphabet(a[b:b + REGION])
            alpha[b // REGION * 64:b // REGION * 64 + 63] = bytes(al)
            code = np.full(256, 63, np.uint32)
            code[al] = np.arange(63, dtype=np.uint32)
        blk = a[b:b + BLOCK]
        ln = len(blk)
        c = code[blk]
        esc6 = blk[c == 63]
        cb = pad(-(-ln // 4) * 3, 16)
        hot = c < HOT
        h = int(hot.sum())
        esc = blk[c >= WARM]
        sizes = {"raw": ln, "6": cb + pad(len(esc6), 16)}
        if blk.max() < 0x80:
            sizes["7"] = -(-ln // 8) * 7
        if split:
            sizes["split"] = split_bytes(ln, h, len(esc))
        mode = min(sizes, key=lambda m: (sizes[m], ("raw", "7", "6", "split").index(m)))
        if mode == "raw":
            table.append(len(out) | RAW)
            out += blk.tobytes()
            counts[2] += 1
        elif mode == "7":
            table.append(len(out))
            g = np.zeros(pad(ln, 8), np.uint64)
            g[:ln] = blk
            g = g.reshape(-1, 8)
            v = sum(g[:, i] << np.uint64(7 * i) for i in range(8))
            out += b"".join(int(x).to_bytes(8, "little")[:7] for x in v)
            counts[1] += 1
        elif mode == "6":
            table.append(len(out) | SIX)
            codes = bits_le(c, 6)
            codes = codes[:-(-ln // 4) * 3] + bytes(-(-ln // 4) * 3 - len(codes))
            out += codes + bytes(cb - len(codes)) + esc6.tobytes() + bytes(pad(len(esc6), 16) - len(esc6))
            counts[0] += 1
            counts[3] += len(esc6)
        else:
            table.append(len(out) | SPLIT)
            five = np.where(c[~hot] < WARM, c[~hot] - HOT, ESC5)
            body = (np.packbits(hot, bitorder="little").tobytes() + bits_le(c[hot], 4) + bits_le(five, 5) +
                    esc.tobytes())
            assert len(body) + 15 & ~15 == sizes["split"]
            out += body + bytes(sizes["split"] - len(body))
            counts[4] += 1
            counts[3] += len(esc)
    return bytes(out), table, bytes(alpha), counts


def check(buf, offset=0):
    """every path against the model; returns (packed, table, alphabets, counts)"""
    buf = bytes(buf)
    want = model(buf)
    for path in (1, 2, 3, 0):
        packed, table, alpha, used, counts, back = pack3(buf, path, offset)
        assert back == buf, PATHS.get(used)
        assert table == want[1] and counts == want[3], PATHS.get(used)
        assert alpha == want[2], PATHS.get(used)
        assert packed == want[0], PATHS.get(used)
    return want


def modes(table):
    return ["split" if t & SPLIT == SPLIT else "raw" if t & RAW else "6" if t & SIX else "7" for t in table]


# 47 values: sampled text of them (from 47 samples on) has them as codes 0..46 and no sampled byte that escapes
V47 = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTU", dtype=np.uint8)
TILDE = ord("~")                                # never sampled below, and no alphabet is filled up as far as 126


def crafted(classes, xval=TILDE, seed=5):
    """A strip of len(classes) bytes whose bytes are of the given classes: 'h' a hot value, 'w' a warm one, 'c' one
    with a code past 46, 'x' xval (outside the alphabet), '.' as words() drew it.  The sampled bytes (every 64th)
    stay as words(n, seed, V47) drew them whatever their class says, so each region's alphabet is that text's and
    each block's sampled bytes are V47[0], V47[1], ... in turn.
    Returns (bytes, per block: (hot count, split escapes, 6-bit escapes))."""
    n = len(classes)
    buf = np.frombuffer(bytes(words(n, seed, V47)), dtype=np.uint8).copy()
    cls = np.frombuffer(classes.encode(), np.uint8)
    free = (np.arange(n) % SAMPLE != 0) & (cls != ord("."))
    per_block = []
    for r in range(0, n, REGION):
        al = alphabet(buf[r:r + REGION])
        assert xval not in al
        val = np.zeros(256, np.uint8)
        val[[ord("h"), ord("w"), ord("c"), ord("x")]] = [al[1], al[20], al[50], xval]
        sl = slice(r, min(n, r + REGION))
        buf[sl][free[sl]] = val[cls[sl][free[sl]]]
        code = np.full(256, 63)
        code[al] = np.arange(63)
        for b in range(r, min(n, r + REGION), BLOCK):
            c = code[buf[b:b + BLOCK]]
            per_block.append((int((c < HOT).sum()), int((c >= WARM).sum()), int((c == 63).sum())))
    return bytearray(buf.tobytes()), per_block


def block(h, e, ln=BLOCK, e6=None, xval=TILDE, seed=5):
    """one block (a strip of its own) with exactly h hot bytes and e bytes that escape in split mode, e6 of
    them (default: all) outside the alphabet; the rest warm"""
    e6 = e if e6 is None else e6
    hs, es, _ = crafted("w" * ln, xval, seed)[1][0]           # what the sampled bytes are
    nfree = ln - -(-ln // SAMPLE)
    assert es == 0 and hs <= h and h - hs + e <= nfree, (h, e, hs, es)
    cl = ["h"] * (h - hs) + ["x"] * e6 + ["c"] * (e - e6) + ["w"] * (nfree - (h - hs) - e)
    np.random.default_rng(seed).shuffle(cl)
    it = iter(cl)
    buf, got = crafted("".join("." if k % SAMPLE == 0 else next(it) for k in range(ln)), xval, seed)
    assert got == [(h, e, e6)]
    return buf


def test_switch_off_is_v2():
    buf = block(2000, 40) + words(BLOCK + 9, 3) + noise(BLOCK, 4)
    want = W2.model(bytes(buf))
    got = model(buf, split=False)
    assert got[:3] == want[:3] and got[3][:4] == want[3] and got[3][4] == 0
    for path in (1, 2, 3, 0):
        p = W2.pack2(bytes(buf), path)
        assert (p[0], p[1], p[2], p[4]) == want
    assert model(buf)[3][4] >= 1


@pytest.mark.parametrize("n", [0, 1, 5, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1, REGION + 5])
def test_round_trip_lengths(n):
    rng = np.random.default_rng(n)
    cl = "".join(rng.choice(list("h" * 20 + "w" * 11 + "c"), n)) if n else ""
    _, table, _, counts = check(crafted(cl, seed=n + 1)[0])
    assert counts[4] == (n // BLOCK if n % BLOCK < 1000 else -(-n // BLOCK)) and sum(counts[:3]) + counts[4] == len(table)
    check(words(n, n + 3))
    check(noise(n, n + 4))


@pytest.mark.parametrize("offset", [1, 3, 13])
def test_misaligned_source(offset):
    buf = crafted("hhw" * BLOCK)[0][:2 * BLOCK + 45]
    buf[77] = 0xC3
    _, table, _, _ = check(buf, offset)
    assert modes(table) == ["split", "split", "split"]       # (45 bytes: 6 + 15 + 10 -> 32)


def test_bit_layout_of_one_block():
    # bytes 1..23 by hand: w h h c x w w | h h h h h h h h | w w w w w w w w; byte 0 is a sampled one, 'a', hot
    ln = BLOCK
    buf, [(h, e, e6)] = crafted("hwhhcxww" + "h" * 8 + "w" * 8 + "h" * (ln - 24))
    packed, table, alpha, counts = check(buf)
    al = list(alpha[:63])
    code = {v: c for c, v in enumerate(al)}
    assert modes(table) == ["split"] and counts == [0, 0, 0, e, 1]
    assert al[0] == ord("a") and packed[0] == 0b00001101 and packed[1] == 0xFF and packed[2] == 0x00
    M = ln // 8
    mask = int.from_bytes(packed[:M], "little")
    hot = [code.get(x, 63) < HOT for x in buf]
    assert all((mask >> k) & 1 == hot[k] for k in range(ln))
    # hot codes: 4 bits each in block order, the first in the low nibble
    N = (h + 1) // 2
    nib = int.from_bytes(packed[M:M + N], "little")
    hc = [code[x] for x, t in zip(buf, hot) if t]
    assert hc[:3] == [0, 1, 1] and packed[M] == 0x10 and packed[M + 1] & 15 == 1
    assert all((nib >> (4 * j)) & 15 == hc[j] for j in range(h)) and nib >> (4 * h) == 0
    # the others: 5 bits each; code - 16, or 31 and the byte itself in the tail
    F = (5 * (ln - h) + 7) // 8
    five = int.from_bytes(packed[M + N:M + N + F], "little")
    fc = [code.get(x, 63) for x, t in zip(buf, hot) if not t]
    assert fc[:5] == [20, 50, 63, 20, 20]
    assert five & 0x1FFFFFF == 4 | 31 << 5 | 31 << 10 | 4 << 15 | 4 << 20
    assert all((five >> (5 * j)) & 31 == (c - 16 if c < WARM else 31) for j, c in enumerate(fc))
    assert five >> (5 * len(fc)) == 0
    body = M + N + F
    assert packed[body:body + 2] == bytes([al[50], TILDE])
    assert packed[body:body + e] == bytes(x for x in buf if code.get(x, 63) >= WARM)
    assert len(packed) == split_bytes(ln, h, e) and not any(packed[body + e:])


@pytest.mark.parametrize("h,ln", [(BLOCK, BLOCK), (1501, BLOCK), (1500, BLOCK - 3), (900, 2999), (1000, 2000 - 4),
                                  (701, 1501), (3001, 3001)])
def test_block_contents(h, ln):
    # h = len; h odd; (len - h) no multiple of 8; len no multiple of 8 or 16
    if h == ln:
        buf = bytearray(b"e" * ln)                      # one value, hot, sampled bytes included
        packed, table, _, counts = check(buf)
        assert modes(table) == ["split"] and len(packed) == split_bytes(ln, ln, 0) == pad(-(-ln // 8) + (ln + 1) // 2, 16)
        return
    buf = block(h, 7, ln=ln)
    packed, table, _, counts = check(buf)
    assert modes(table) == ["split"] and counts == [0, 0, 0, 7, 1] and len(packed) == split_bytes(ln, h, 7)


def test_no_hot_byte():
    # with h = 0 a split block is never below the 6-bit one (3072 + e against 3072 + pad16(e6), e >= e6): the packer
    # must not choose it; as few hot bytes as the sampled ones allow
    assert split_bytes(BLOCK, 0, 0) == 3072
    buf, [(h, e, e6)] = crafted("w" * BLOCK)
    _, table, _, _ = check(buf)
    assert h < 128 and modes(table) == ["6"]
    buf, [(h, e, e6)] = crafted("wx" * (BLOCK // 2), xval=0x80)
    _, table, _, _ = check(buf)
    assert modes(table) == ["raw"]


@pytest.mark.parametrize("where", ["first", "last", "lane", "both"])
@pytest.mark.parametrize("xval", [0x00, 0x7F, 0x80, 0xFF])
def test_escapes_and_edge_values(where, xval):
    ln = BLOCK
    at = {"first": [0], "last": [ln - 1], "lane": range(16 * 77, 16 * 78), "both": [0, ln - 1]}[where]
    buf = crafted("hhhw" * (ln // 4))[0]
    for k in at:
        buf[k] = xval                   # (byte 0 is a sampled one: 0x00 and 0x7F are then seen once and get a code)
    packed, table, alpha, counts = check(buf)
    assert modes(table) == ["split"]
    if xval >= 0x80:
        assert counts[3] == len(at)
    elif 0 not in at:
        assert counts[3] == (len(at) if xval == 0x7F or alpha.index(xval) >= WARM else 0)


def test_hot_and_warm_alternating():
    for cl in ("hw" * (BLOCK // 2), ("h" * 1024 + "w" * 1024) * 2, "w" * 1023 + "h" * 1025 + "w" * 1024 + "h" * 1024):
        _, table, _, _ = check(crafted(cl)[0])
        assert modes(table) == ["split"]


def _first(pred, rng):
    return next(v for v in rng if pred(v))


def test_mode_boundaries_from_the_size_formula():
    ln = BLOCK
    size6, size7 = 3072, 3584
    # against 6-bit, no escape anywhere: split wins from the first hot count whose size is below 3072
    h0 = _first(lambda h: split_bytes(ln, h, 0) < size6, range(ln + 1))
    assert h0 == 128 and split_bytes(ln, h0 - 1, 0) == size6          # 3072 - 128 / 8 = 3056; one less ties
    for h, mode in ((h0 - 1, "6"), (h0, "split")):
        packed, table, _, counts = check(block(h, 0))
        assert modes(table) == [mode] and len(packed) == (split_bytes(ln, h, 0) if mode == "split" else size6)
    # against 6-bit with escapes that only split has (codes 47..62): at h = 1024 split is 2944 + e
    h = 1024
    e0 = _first(lambda e: split_bytes(ln, h, e) >= size6, range(ln))
    assert e0 == 113 and split_bytes(ln, h, e0) == size6               # 2944 + 113 -> 3072: the tie goes to 6-bit
    for e, mode in ((e0 - 1, "split"), (e0, "6")):
        _, table, _, counts = check(block(h, e, e6=0))
        assert modes(table) == [mode] and counts[3] == (e if mode == "split" else 0)
    # against 7-bit: bytes outside the alphabet cost 6-bit as much as split, which stays 128 ahead of it
    e0 = _first(lambda e: split_bytes(ln, h, e) >= size7, range(ln))
    assert e0 == 625 and split_bytes(ln, h, e0) == size7               # 2944 + 625 -> 3584: the tie goes to 7-bit
    for e, mode in ((e0 - 1, "split"), (e0, "7")):
        _, table, _, _ = check(block(h, e))
        assert modes(table) == [mode]
    # against raw: the same with bytes >= 0x80, which rule 7-bit out
    e0 = _first(lambda e: split_bytes(ln, h, e) >= ln, range(ln))
    assert e0 == 1137 and split_bytes(ln, h, e0) == ln                 # 2944 + 1137 -> 4096: the tie goes to raw
    for e, mode in ((e0 - 1, "split"), (e0, "raw")):
        packed, table, _, _ = check(block(h, e, xval=0x80))
        assert modes(table) == [mode] and len(packed) == (ln if mode == "raw" else ln - 16)


def test_tie_order_in_a_short_block():
    # 2048 bytes, 300 of them outside the alphabet: 7-bit is 1792, 6-bit 1536 + 304; split ties with 7-bit over a
    # range of hot counts and is kept only below it
    ln, x = 2048, 300
    h_tie = _first(lambda h: split_bytes(ln, h, x) == 1792, range(ln))
    h_win = _first(lambda h: split_bytes(ln, h, x) < 1792, range(ln))
    assert 32 < h_tie < h_win
    for h, mode in ((h_tie, "7"), (h_win - 1, "7"), (h_win, "split")):
        _, table, _, _ = check(block(h, x, ln=ln))
        assert modes(table) == [mode]


def test_two_regions_two_alphabets():
    a = crafted("hhw" * (REGION // 3) + "h")[0]
    b = np.frombuffer(bytes(words(REGION // 2 + 7, 22, PUNCT)), np.uint8).copy()
    al = alphabet(b)
    b[np.arange(len(b)) % SAMPLE != 0] = al[0]
    b[1::5] = al[30]
    packed, table, alpha, counts = check(a + bytearray(b.tobytes()))
    assert set(V47.tolist()) == set(alpha[:47]) and set(PUNCT.tolist()) == set(alpha[64:64 + 32])
    assert modes(table) == ["split"] * 24 + ["raw"] and counts[3] == 0


def test_all_four_modes_in_one_strip():
    buf = block(2000, 10) + block(100, 0) + noise(BLOCK, 12) + bytearray(b"\xc3\xa9" * (BLOCK // 2)) + \
        block(1500, 3, ln=1000 + 555)
    # (one alphabet for the region, that of all its samples: the noise moves some codes, not the modes)
    packed, table, _, counts = check(buf)
    assert modes(table) == ["split", "6", "7", "raw", "split"] and counts[:3] == [1, 1, 1] and counts[4] == 2


def test_paths_agree():
    buf = block(2222, 50) + words(2 * BLOCK + 77, 17) + noise(BLOCK, 18) + block(2900, 5, ln=3001)
    buf[BLOCK + 5] = 0x90
    scalar = pack3(bytes(buf), 1)
    assert scalar[3] == 1 and scalar[4][4] >= 1
    ran = 0
    for path in (2, 3):
        simd = pack3(bytes(buf), path)
        if simd[3] != path:
            continue
        ran += 1
        assert scalar[:3] == simd[:3] and scalar[4:] == simd[4:], PATHS[path]
        print("path", path, "ran; its split packer:", packer_of(simd[3]))
    print("paths present:", ran, "; AVX-512 VBMI2:", VBMI2[0], "; the CPU's best packs split blocks with:",
          packer_of(pack3(b"x")[3]))


