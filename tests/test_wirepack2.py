"""Host side of the 6-bit wire codec with escapes (trivy_amd/csrc/wirepack.cpp,
"v2" in wirepack.h) through tsg_test_wire_pack2.

model() below predicts a packed strip from its bytes alone: the alphabet of
each 64 KiB region (the 63 most frequent values < 0x80 among every 64th byte,
equal counts by lower value), the mode of each 4096-byte block (the smallest of
raw, 7-bit and 6-bit; of equal sizes raw, then 7-bit) and the exact bytes.  The
model, the scalar path and every SIMD path the CPU has must agree byte for
byte, and the host unpack must give the source back.

tools/wirepack_tool.cpp (check2) runs the same cases under AddressSanitizer without
Python.
"""
import ctypes

import numpy as np
import pytest

from trivy_amd import _lib

BLOCK = 4096
REGION = 65536
SAMPLE = 64
RAW = 1 << 31
SIX = 1 << 30
PATHS = {1: "scalar", 2: "avx2", 3: "vbmi"}


def pad(n, m):
    return -(-n // m) * m


def alpha_bytes(n):
    return pad(-(-n // REGION) * 64, 256)


def pack2(buf, path=0, offset=0):
    """(packed, table, alphabets, path used, counts, host unpack) of buf as one strip read from a source at `offset`"""
    a = np.frombuffer(bytes(offset) + bytes(buf), dtype=np.uint8).copy()
    n = len(a) - offset
    packed = np.zeros(n + 16, np.uint8)
    table = np.zeros(max(1, -(-n // BLOCK)), np.uint32)
    alpha = np.full(max(1, alpha_bytes(n)), 0xEE, np.uint8)
    back = np.full(max(1, n), 0xEE, np.uint8)
    counts = np.zeros(4, np.uint64)
    plen, used = ctypes.c_size_t(), ctypes.c_int()
    _lib.check(_lib.lib().tsg_test_wire_pack2(a.ctypes.data + offset, n, path, packed.ctypes.data, len(packed),
                                              table.ctypes.data, alpha.ctypes.data, ctypes.byref(plen),
                                              ctypes.byref(used), counts.ctypes.data, back.ctypes.data))
    return (packed[:plen.value].tobytes(), table[:-(-n // BLOCK)].tolist(), alpha[:alpha_bytes(n)].tobytes(), used.value,
            [int(c) for c in counts], back[:n].tobytes())


def alphabet(region):
    s = region[::SAMPLE]
    cnt = np.bincount(s[s < 0x80], minlength=128)
    return sorted(range(128), key=lambda v: (-int(cnt[v]), v))[:63]


def model(buf):
    """(packed, table, alphabets, [6-bit blocks, 7-bit blocks, raw blocks, escaped bytes]) of the strip buf"""
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = len(a)
    alpha = bytearray(alpha_bytes(n))
    out, table, counts = bytearray(), [], [0, 0, 0, 0]
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
        esc = blk[c == 63]
        cb = pad(-(-ln // 4) * 3, 16)
        size6 = cb + pad(len(esc), 16)
        size7 = -(-ln // 8) * 7 if blk.max() < 0x80 else None
        if ln <= size6 and (size7 is None or ln <= size7):
            table.append(len(out) | RAW)
            out += blk.tobytes()
            counts[2] += 1
        elif size7 is not None and size7 <= size6:
            table.append(len(out))
            g = np.zeros(pad(ln, 8), np.uint64)
            g[:ln] = blk
            g = g.reshape(-1, 8)
            v = sum(g[:, i] << np.uint64(7 * i) for i in range(8))
            out += b"".join(int(x).to_bytes(8, "little")[:7] for x in v)
            counts[1] += 1
        else:
            table.append(len(out) | SIX)
            g = np.zeros(pad(ln, 4), np.uint32)
            g[:ln] = c
            g = g.reshape(-1, 4)
            v = g[:, 0] | g[:, 1] << 6 | g[:, 2] << 12 | g[:, 3] << 18
            codes = np.stack([v & 255, v >> 8 & 255, v >> 16], axis=1).astype(np.uint8).tobytes()
            out += codes + bytes(cb - len(codes)) + esc.tobytes() + bytes(pad(len(esc), 16) - len(esc))
            counts[0] += 1
            counts[3] += len(esc)
    return bytes(out), table, bytes(alpha), counts


def check(buf, offset=0):
    """every path against the model; returns (packed, table, alphabets, counts)"""
    buf = bytes(buf)
    want = model(buf)
    for path in (1, 2, 3, 0):
        packed, table, alpha, used, counts, back = pack2(buf, path, offset)
        assert back == buf, PATHS.get(used)
        assert table == want[1] and counts == want[3], PATHS.get(used)
        assert alpha == want[2], PATHS.get(used)
        assert packed == want[0], PATHS.get(used)
    return want


# 63 values: text of them fills the alphabet, so any other byte escapes
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ", dtype=np.uint8)
PUNCT = np.frombuffer(b"!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~", dtype=np.uint8)             # 32 others


def words(n, seed, vals=LETTERS):
    """n bytes drawn from at most 63 values, which take turns at the sampled offsets (each is seen
    about len / 4096 times per region): blocks of it pack to 6 bits without an escape"""
    a = vals[np.random.default_rng(seed).integers(0, len(vals), n)]
    a[::SAMPLE] = np.resize(vals, len(a[::SAMPLE]))
    return bytearray(a.tobytes())


def noise(n, seed):
    """all 128 ASCII values alike: half of the bytes would escape, so blocks of it go 7-bit"""
    return bytearray(np.random.default_rng(seed).integers(0, 128, n, dtype=np.uint8).tobytes())


def modes(table):
    return ["raw" if t & RAW else "6" if t & SIX else "7" for t in table]


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 5])
def test_round_trip_lengths(n):
    check(words(n, n + 3))
    check(noise(n, n + 4))


@pytest.mark.parametrize("offset", [1, 3, 13])
def test_misaligned_source(offset):
    buf = words(2 * BLOCK + 45, offset)
    buf[77] = 0xC3
    check(buf, offset)
    check(noise(2 * BLOCK + 45, offset), offset)


def test_no_escape_and_bit_layout():
    buf = words(2 * BLOCK, 1)
    packed, table, alpha, counts = check(buf)
    assert modes(table) == ["6", "6"] and counts == [2, 0, 0, 0]
    assert len(packed) == 2 * 3072 and table[1] == 3072 | SIX
    # byte k of a block is the 6-bit code in bits 6k .. 6k+5 of a little-endian bit string
    code = {v: c for c, v in enumerate(alpha[:63])}
    bits = int.from_bytes(packed[:3072], "little")
    assert all((bits >> (6 * k)) & 63 == code[buf[k]] for k in range(BLOCK))
    assert alpha[63] == 0 and len(alpha) == 256 and not any(alpha[64:])


@pytest.mark.parametrize("pos", [0, BLOCK - 1, BLOCK, 4 * BLOCK - 1])
@pytest.mark.parametrize("value", [ord("#"), 0xE2])
def test_one_escape_at_a_block_edge(pos, value):
    buf = words(4 * BLOCK, 2)
    buf[pos] = value                    # (a block's first byte is a sampled one: seen once, '#' stays out)
    packed, table, _, counts = check(buf)
    assert modes(table) == ["6"] * 4 and counts == [4, 0, 0, 1]
    b = pos // BLOCK
    assert len(packed) == 4 * 3072 + 16
    tail = packed[(table[b] & ~SIX) + 3072:][:16]
    assert tail == bytes([value]) + bytes(15)


@pytest.mark.parametrize("n", [3 * BLOCK + 1029, 3 * BLOCK + 1030, 3 * BLOCK + 1031])
def test_escapes_in_the_last_partial_group(n):
    buf = words(n, 3)
    for i in range(n - n % 4, n):
        buf[i] = ord("@")
    buf[BLOCK + 7] = 0xFF
    _, table, _, counts = check(buf)
    assert modes(table) == ["6"] * 4 and counts[3] == n % 4 + 1


def _with_escapes(k, value):
    buf = words(BLOCK, 5)
    step = BLOCK // k
    assert step >= 2 and step % 2 == 0
    for i in range(k):
        buf[i * step + 1] = value               # odd offsets: never a sampled byte
    assert sum(1 for x in buf if x == value) == k
    return buf


@pytest.mark.parametrize("k,value,mode", [(496, ord("#"), "6"), (497, ord("#"), "7"),
                                          (1008, 0x80, "6"), (1009, 0x80, "raw")])
def test_escape_count_thresholds(k, value, mode):
    # 3072 + pad16(496) = 3568 < 3584, 3072 + pad16(497) = 3584: the tie goes to 7-bit;
    # a non-ASCII block: 3072 + pad16(1008) = 4080 < 4096, 3072 + pad16(1009) = 4096: the tie goes to raw
    buf = _with_escapes(k, value)
    packed, table, _, counts = check(buf)
    assert modes(table) == [mode]
    assert len(packed) == {"6": 3072 + pad(k, 16), "7": 3584, "raw": 4096}[mode]
    assert counts[3] == (k if mode == "6" else 0)


def test_more_than_63_values():
    # 96 values, 60 of them far ahead: of the other 36 all but three escape
    rng = np.random.default_rng(7)
    common = rng.integers(32, 92, REGION).astype(np.uint8)
    rare = rng.integers(92, 128, REGION).astype(np.uint8)
    buf = np.where(rng.random(REGION) < 0.03, rare, common).tobytes()
    assert len(set(buf)) > 63
    _, table, alpha, counts = check(buf)
    assert modes(table) == ["6"] * 16 and 0 < counts[3] < 16 * 300
    assert set(range(32, 92)) <= set(alpha[:63])
    # all 128 values alike: 7-bit
    _, table, _, _ = check(noise(3 * BLOCK, 8))
    assert modes(table) == ["7"] * 3


@pytest.mark.parametrize("value", [0x00, 0x7F, 0x80, 0xFF])
@pytest.mark.parametrize("pos", [0, BLOCK - 1, BLOCK, REGION - 1, REGION, REGION + 4 * BLOCK - 1])
def test_edge_values(value, pos):
    buf = words(REGION + 4 * BLOCK, 9)
    buf[pos] = value
    packed, table, _, counts = check(buf)
    assert modes(table) == ["6"] * 20
    # one escaped byte costs its block 16 bytes, and only its block (a sampled 0x00 / 0x7F does not reach the alphabet)
    assert counts[3] == 1 and len(packed) == 20 * 3072 + 16


def test_non_ascii_goes_raw():
    buf = b"\xc3\xa9" * (3 * BLOCK // 2 + 9)
    packed, table, _, counts = check(buf)
    assert packed == buf and modes(table) == ["raw"] * 4 and counts == [0, 0, 4, 0]


def test_three_modes_in_one_strip():
    buf = words(10 * BLOCK, 11) + noise(BLOCK, 12) + bytearray(b"\xc3\xa9" * (BLOCK // 2)) + words(BLOCK + 100, 13)
    buf[12 * BLOCK + 50] = 0xC3                     # a UTF-8 character does not cost the block its packing
    buf[12 * BLOCK + 51] = 0xA9
    packed, table, _, counts = check(buf)
    assert modes(table) == ["6"] * 10 + ["7", "raw", "6", "6"] and counts == [12, 1, 1, 2]
    o = 10 * 3072
    assert [t & ~(RAW | SIX) for t in table[9:]] == [o - 3072, o, o + 3584, o + 3584 + 4096, o + 3584 + 4096 + 3072 + 16]
    assert len(packed) == o + 3584 + 4096 + 3072 + 16 + 80


def test_two_regions_two_alphabets():
    buf = words(REGION, 21) + words(REGION // 2 + 7, 22, PUNCT)
    packed, table, alpha, counts = check(buf)
    assert set(LETTERS.tolist()) == set(alpha[:63]) and set(PUNCT.tolist()) <= set(alpha[64:127])
    # the blocks on both sides of the region edge pack without an escape, each with its own alphabet
    assert modes(table) == ["6"] * 24 + ["raw"] and counts[3] == 0      # (the 7-byte last block gains nothing)
    # a block of the second kind inside the first region: every byte escapes, it goes 7-bit
    buf[5 * BLOCK:6 * BLOCK] = words(BLOCK, 23, PUNCT)
    _, table, _, _ = check(buf)
    assert modes(table)[4:7] == ["6", "7", "6"]


def test_alphabet_tie_goes_to_the_lower_value():
    # 64 values sampled 16 times each: the highest of them stays out
    vals = np.arange(40, 104, dtype=np.uint8)
    buf = bytearray(np.repeat(vals, REGION // 64).tobytes())
    samples = bytes(buf[::SAMPLE])
    assert all(samples.count(int(v)) == 16 for v in vals)
    _, table, alpha, counts = check(buf)
    assert list(alpha[:63]) == list(range(40, 103))
    assert modes(table) == ["6"] * 15 + ["7"] and counts[3] == 0
    # a value seen more often moves to the front; the rest keep value order
    for i in range(0, 17 * SAMPLE, SAMPLE):         # 16 samples of 40 and one of 41
        buf[i] = 103
    _, _, alpha, _ = check(buf)
    assert list(alpha[:63]) == [103] + list(range(42, 103)) + [41]
    # nothing sampled at all (values >= 0x80 are skipped): the 63 lowest values
    _, _, alpha, _ = check(b"\xff" * 100)
    assert list(alpha[:63]) == list(range(63))


def test_paths_agree():
    buf = words(5 * BLOCK + 77, 17) + noise(BLOCK, 18)
    buf[BLOCK + 5] = 0x90
    buf[2 * BLOCK:2 * BLOCK + 64] = bytes(range(0xC0, 0x100))
    scalar = pack2(bytes(buf), 1)
    assert scalar[3] == 1
    ran = 0
    for path in (2, 3):
        simd = pack2(bytes(buf), path)
        if simd[3] != path:
            continue
        ran += 1
        assert scalar[:3] == simd[:3] and scalar[4:] == simd[4:], PATHS[path]
    print("paths present:", ran, "best:", PATHS[pack2(b"x")[3]])
    if not ran:
        pytest.skip("this CPU has neither AVX2 nor AVX-512 VBMI")
