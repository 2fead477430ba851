"""The CPU model of the GPU zstd decode (zstdec.h; tsg_test_zstd_model): every
valid stream of tests/_zstd_corpus.py decodes to the bytes its seed gives, and
to what libzstd gives where libzstd loads; every invalid one ends in the status
its construction implies; over every single-byte corruption of the small
checksummed frames the model says OK only where libzstd says OK, and then with
the same bytes; tsg_zstd_size_bound is exact where it claims to be and never
below the true size; tsg_layer_compression tells the three kinds apart; a slot
exactly as large as needed succeeds, one byte less and none at all end
TSG_ZSTD_DST_FULL, and nothing outside a slot is written."""
import ctypes
import gzip

import numpy as np
import pytest

import _zstd_corpus as Z
from trivy_amd import _lib
from trivy_amd import secret as S

CORPUS = Z.corpus()
VALID = [n for n, c in CORPUS.items() if c.status == Z.OK]
INVALID = [n for n, c in CORPUS.items() if c.status != Z.OK]
GROUPS = ["levels", "windows", "literals", "sequences", "frames", "small"]

# Streams the model accepts and libzstd 1.4.8 rejects, with the clause of RFC 8878 that makes them valid: none.
# (The other way round is allowed and happens: the model holds Huffman codes to 11 bits and blocks to
# Block_Maximum_Size as the RFC does, libzstd's one-shot decoder is laxer on both.)
MODEL_ONLY_OK = {}


def libzstd():
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError:
        return None
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return z


def zstd_decompress(z, blob, cap):
    out = ctypes.create_string_buffer(max(cap, 1))
    n = z.ZSTD_decompress(out, cap, bytes(blob), len(blob))
    return None if z.ZSTD_isError(n) else out.raw[:n]


@pytest.mark.parametrize("group", GROUPS)
def test_valid_streams_decode_to_their_payload(group):
    cases = [c for c in CORPUS.values() if c.group == group]
    assert cases and all(c.status == Z.OK for c in cases)
    caps = [Z.default_cap(c) for c in cases]
    rc, msg, status, out_lens, dst, do = Z.run_model([c.z for c in cases], caps)
    assert rc == 0 and status == [Z.OK] * len(cases), msg
    for i, c in enumerate(cases):
        assert out_lens[i] == len(c.payload), c.name
        assert dst[do[i]:do[i] + out_lens[i]].tobytes() == c.payload, c.name
    Z.check_slots(out_lens, dst, do)


def test_corpus_is_what_it_claims():
    assert len(VALID) > 120 and len(INVALID) > 250
    assert {c.group for c in CORPUS.values()} == set(GROUPS) | {"invalid"}
    ev, st = Z.trace(CORPUS["w17_far"].z, len(CORPUS["w17_far"].payload))
    assert st == Z.OK and all(ev[e] for e in ("off32768", "off32769", "straddle", "far_same_line", "off_ring_edge", "off_ring_edge1"))
    assert Z.trace(CORPUS["zeros_long"].z, 131072)[0]["long_overlap"] == 1
    assert Z.trace(CORPUS["tiny_300"].z, 4096)[0]["frame"] == 300
    assert Z.trace(CORPUS["seq_rle_long"].z, 200000)[0]["seq_long"] == 1
    assert Z.trace(CORPUS["seq127"].z, 20000)[0]["seq127"] and Z.trace(CORPUS["seq128"].z, 20000)[0]["seq128"]
    assert Z.trace(CORPUS["lit_bits11"].z, 40000)[0]["huf_bits11"]
    assert len(CORPUS["w10_text"].payload) > 8 * 1024 and len(CORPUS["w17_far"].payload) > 128 * 1024


def test_valid_streams_equal_libzstd():
    z = libzstd()
    if z is None:
        pytest.skip("no libzstd on this machine")
    for name in VALID:
        c = CORPUS[name]
        assert zstd_decompress(z, c.z, len(c.payload)) == c.payload, name


def test_invalid_streams_end_in_their_status():
    L = _lib.lib()
    seen = set()
    for name in INVALID:
        c = CORPUS[name]
        rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [Z.default_cap(c)])
        assert status == [c.status], (name, status, c.status)
        assert rc != 0 and msg == "zstd stream 0: " + Z.TEXT[c.status], (name, msg)
        assert L.tsg_zstd_status_text(c.status).decode() == Z.TEXT[c.status]
        Z.check_slots(out_lens, dst, do)
        seen.add(c.status)
    assert seen == {Z.HEADER, Z.CORRUPT, Z.EOF, Z.CHECKSUM, Z.DICT}
    assert L.tsg_zstd_status_text(Z.OK) == b"" and L.tsg_zstd_status_text(Z.DST_FULL) == b""


def test_first_error_in_stream_order_wins():
    good, bad = CORPUS["fcs2_single"], CORPUS["wrong_checksum"]
    rc, msg, status, out_lens, dst, do = Z.run_model([good.z, bad.z, good.z + CORPUS["block_type_3"].z], [400, 400, 400])
    assert status == [Z.OK, Z.CHECKSUM, Z.CORRUPT] and msg == "zstd stream 1: zstd: invalid checksum"
    assert dst[do[0]:do[0] + out_lens[0]].tobytes() == good.payload                  # valid beside a failed neighbour
    assert dst[do[2]:do[2] + out_lens[2]].tobytes() == good.payload                  # what preceded the corrupt frame


def test_single_byte_corruptions_against_libzstd():
    z = libzstd()
    if z is None:
        pytest.skip("no libzstd on this machine")
    exceptions = {}
    for name in ("small_text", "small_few", "small_records"):
        c = CORPUS[name]
        n, cap = len(c.z), len(c.payload) + 64
        base = np.frombuffer(c.z, dtype=np.uint8)
        for pos in range(n):
            streams = np.tile(base, (255, 1))
            streams[:, pos] = [v for v in range(256) if v != base[pos]]
            blobs = [s.tobytes() for s in streams]
            rc, msg, status, out_lens, dst, do = Z.run_model(blobs, [cap] * 255)
            for k in np.flatnonzero(np.array(status) == Z.OK):
                want = zstd_decompress(z, blobs[k], cap)
                got = dst[do[k]:do[k] + out_lens[k]].tobytes()
                if want != got:
                    exceptions.setdefault(name, []).append((pos, int(streams[k, pos]), want is None))
    assert exceptions == MODEL_ONLY_OK


def test_size_bound_is_exact_where_claimed_and_never_below():
    nexact = 0
    for name in VALID:
        c = CORPUS[name]
        bound, exact, clean = S.Scanner.ZstdSizeBound(c.z)
        assert clean and bound >= len(c.payload), name
        if exact:
            assert bound == len(c.payload), name
            nexact += 1
    assert 40 < nexact < len(VALID)
    assert S.Scanner.ZstdSizeBound(CORPUS["rle_128k"].z)[0] == 131072                # 131072 bytes from a frame of 17
    assert S.Scanner.ZstdSizeBound(CORPUS["skip_only"].z) == (0, True, True)
    # without a Frame_Content_Size a compressed block counts Block_Maximum_Size, a raw or RLE block its size
    c = CORPUS["lv_text_3_c0_s0"]                # one compressed block under a 16 KiB window
    assert S.Scanner.ZstdSizeBound(c.z) == (16384, False, True)
    assert S.Scanner.ZstdSizeBound(CORPUS["window_mantissa"].z) == (2500, False, True)
    # the bound holds for whatever the model accepts: a compressed block that would regenerate more than
    # Block_Maximum_Size (97551 bytes under a 1 KiB window) is corrupt, inside a slot of the bound + 64 as in a large one
    c = CORPUS["block_output_above_max"]
    bound, exact, clean = S.Scanner.ZstdSizeBound(c.z)
    assert (bound, exact, clean) == (8 + 1024, False, True)
    for cap in (bound + 64, 200000):
        rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [cap])
        assert status == [Z.CORRUPT] and out_lens[0] <= bound, cap
    for name in ("truncated_005", "truncated_100", "bad_magic", "block_type_3"):
        bound, exact, clean = S.Scanner.ZstdSizeBound(CORPUS[name].z)
        assert not clean and not exact, name


def test_layer_compression_by_the_first_bytes():
    kind = S.Scanner.LayerCompression
    assert kind(CORPUS["small_text"].z) == _lib.LAYER_ZSTD and kind(b"\x28\xb5\x2f\xfd") == _lib.LAYER_ZSTD
    assert kind(gzip.compress(b"x")) == _lib.LAYER_GZIP and kind(b"\x1f\x8b") == _lib.LAYER_GZIP
    tar = Z.layer_tars()["smoke"]
    assert kind(tar) == _lib.LAYER_NONE and kind(b"") == _lib.LAYER_NONE and kind(b"\x28\xb5\x2f") == _lib.LAYER_NONE
    assert kind(Z.skippable(0, b"x")) == _lib.LAYER_NONE                              # the peek knows the frame magic alone


@pytest.mark.parametrize("name", ["lv_text_19_c1_s1", "lv_zeros_3_c1_s0", "w10_text", "rle_blocks", "tiny_300", "lit_raw_fmt3",
                                  "seq_rle_long", "lv_rnd_1_c0_s1"])
def test_slot_exact_one_byte_short_and_none(name):
    c = CORPUS[name]
    n = len(c.payload)
    rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [n])
    assert (rc, status, out_lens) == (0, [Z.OK], [n]) and dst.tobytes() == c.payload
    for cap in (n - 1, 0):
        rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [cap])
        assert rc != 0 and status == [Z.DST_FULL] and msg == "zstd stream 0: the output does not fit its slot"
        assert out_lens[0] <= cap and dst[:out_lens[0]].tobytes() == c.payload[:out_lens[0]]
        Z.check_slots(out_lens, dst, do)


def test_output_before_an_error_stays():
    c = CORPUS["corrupt_after_36000"]
    rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [Z.default_cap(c)])
    assert status == [Z.CORRUPT] and out_lens == [50 + 8 + 36000]                   # what was written when the bitstream ran dry
    assert dst[:50].tobytes() == CORPUS["good_then_corrupt"].z[9:59]                # the good frame's raw block
    assert dst[50:58].tobytes() == b"abcdefgh" and dst[58:61].tobytes() == b"abc"   # offsets 8, 4, 1, 8 ...


def test_slot_comes_before_an_error_further_on():
    c = CORPUS["good_then_corrupt"]
    rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [49])
    assert status == [Z.DST_FULL]
    rc, msg, status, out_lens, dst, do = Z.run_model([c.z], [50])
    assert status == [Z.CORRUPT] and out_lens == [50]


def test_xxh64_known_values():
    assert Z.xxh64(b"") == 0xef46db3751d8e999
    assert Z.xxh64(b"a") == 0xd24ec4f1a98c6e5b
    assert Z.xxh64(b"abc") == 0x44bc2cf5ad770999
