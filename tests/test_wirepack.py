"""Host side of the wire packing (trivy_amd/csrc/wirepack.cpp) through
tsg_test_wire_pack: ASCII blocks of a strip are written as 7 bytes per 8, any
other block unchanged, with a table of block offsets and modes.

* pack then host unpack gives the source back at lengths around the group,
  vector and block sizes, with 0x00 / 0x7F / 0x80 / 0xFF on block and strip
  edges, for all-non-ASCII and alternating buffers, and from misaligned
  sources;
* the packed size and the table are exactly what the format says (so a scan's
  wire_bytes can be predicted), and the scalar and AVX2 paths agree byte for
  byte.

tools/wirepack_tool.cpp runs the same cases under AddressSanitizer without Python.
"""
import ctypes

import numpy as np
import pytest

from trivy_amd import _lib

BLOCK = 4096
RAW = 1 << 31
STRIP = 4 * BLOCK          # the strip these tests cut: four blocks


def pack(buf, path=0, offset=0):
    """(packed bytes, table, path used, host unpack) of buf[offset:] as one strip"""
    a = np.frombuffer(bytes(offset) + bytes(buf), dtype=np.uint8).copy()
    n = len(a) - offset
    packed = np.zeros(n + 8, np.uint8)
    table = np.zeros(max(1, -(-n // BLOCK)), np.uint32)
    back = np.full(max(1, n), 0xEE, np.uint8)
    plen, used = ctypes.c_size_t(), ctypes.c_int()
    _lib.check(_lib.lib().tsg_test_wire_pack(a.ctypes.data + offset, n, path, packed.ctypes.data, len(packed),
                                             table.ctypes.data, ctypes.byref(plen), ctypes.byref(used),
                                             back.ctypes.data))
    return packed[:plen.value].tobytes(), table[:-(-n // BLOCK)].tolist(), used.value, back[:n].tobytes()


def predict(buf):
    """the format's packed size and table, from the bytes alone"""
    o, table = 0, []
    for b in range(0, len(buf), BLOCK):
        blk = buf[b:b + BLOCK]
        if max(blk) < 0x80:
            table.append(o)
            o += -(-len(blk) // 8) * 7
        else:
            table.append(o | RAW)
            o += len(blk)
    return o, table


def text(n, seed=1):
    return bytes(np.random.default_rng(seed).integers(0, 128, n, dtype=np.uint8))


def check(buf, offset=0):
    want_len, want_table = predict(buf)
    outs = []
    for path in (1, 2, 0):
        packed, table, used, back = pack(buf, path, offset)
        assert back == buf
        assert len(packed) == want_len and table == want_table
        outs.append((packed, table))
    assert outs[0] == outs[1] == outs[2]
    return outs[0][0]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 31, 32, 33, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 5])
def test_round_trip_lengths(n):
    check(text(n, n + 3))


@pytest.mark.parametrize("value", [0x00, 0x7F, 0x80, 0xFF])
@pytest.mark.parametrize("pos", [0, BLOCK - 1, BLOCK, 2 * BLOCK - 1, STRIP - 1])
def test_edge_values(value, pos):
    buf = bytearray(text(STRIP, 9))
    buf[pos] = value
    packed = check(bytes(buf))
    # a byte >= 0x80 sends its block, and only its block, unchanged
    assert len(packed) == STRIP // 8 * 7 + (BLOCK // 8 if value >= 0x80 else 0)


def test_bit_layout():
    # byte i of a group lands in bits 7i .. 7i+6 of a little-endian 56-bit value
    packed = check(bytes(range(1, 9)))
    assert int.from_bytes(packed, "little") == sum((i + 1) << (7 * i) for i in range(8))
    assert check(b"\x7f") == b"\x7f" + bytes(6)


def test_non_ascii_and_alternating():
    buf = b"\xc3\xa9" * (3 * BLOCK // 2 + 9)
    assert check(buf) == buf
    alt = bytearray(text(6 * BLOCK + 3, 5))
    for b in (0, 2, 4):
        alt[b * BLOCK + 100] = 0xE2
    _, table, _, _ = pack(bytes(alt))
    assert [bool(t & RAW) for t in table] == [True, False, True, False, True, False, False]
    check(bytes(alt))


@pytest.mark.parametrize("offset", [1, 3, 13])
def test_misaligned_source(offset):
    check(text(2 * BLOCK + 45, offset), offset)


def test_scalar_and_avx2_agree():
    buf = bytearray(text(5 * BLOCK + 77, 17))
    buf[BLOCK + 5] = 0x90
    scalar = pack(bytes(buf), 1)
    avx2 = pack(bytes(buf), 2)
    assert scalar[2] == 1
    if avx2[2] != 2:
        pytest.skip("this CPU has no AVX2")
    assert scalar[0] == avx2[0] and scalar[1] == avx2[1]
