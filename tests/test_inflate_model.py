"""The CPU model of the GPU gzip inflate (inflate.h; tsg_test_inflate_model):
every valid stream of tests/_gzip_corpus.py inflates to what Python's zlib
gives, member after member; every invalid one ends in the status its
construction implies, with Go's text; a slot exactly as large as needed
succeeds, one byte less ends TSG_INFLATE_DST_FULL, and nothing outside a slot
is written; the checksum pass -- CRC32 in slices folded with the shift
operator -- equals zlib.crc32; and the corpus is what it claims to be."""
import ctypes
import gzip
import zlib

import numpy as np
import pytest

import _gzip_corpus as G
from trivy_amd import _lib

CORPUS = G.corpus()
VALID = [n for n, c in CORPUS.items() if c.status == G.OK]
INVALID = [n for n, c in CORPUS.items() if c.status != G.OK]
# Go and Python differ on these two: Python's gzip module skips zero padding behind the last member, Go's
# multistream reader takes it for a header; Go's readString gives up on a name of more than 511 bytes
PYTHON_ACCEPTS = {"trailing_zero": gzip.decompress, "trailing_zeros_16": gzip.decompress, "fname_512": G.py_inflate}


def test_valid_streams_equal_zlib():
    assert len(VALID) > 60
    for name in VALID:
        c = CORPUS[name]
        want = G.py_inflate(c.gz)
        rc, msg, status, out_lens, dst, _ = G.run_model([c.gz], [len(want)])
        assert (rc, status, out_lens) == (0, [G.OK], [len(want)]), (name, msg)
        assert dst.tobytes() == want == c.payload, name


def test_valid_streams_in_one_batch():
    cases = [CORPUS[n] for n in VALID if n != "big_8mib"]
    rc, msg, status, out_lens, dst, do = G.run_model([c.gz for c in cases], [len(c.payload) for c in cases])
    assert rc == 0 and status == [G.OK] * len(cases), msg
    for i, c in enumerate(cases):
        assert dst[do[i]:do[i] + out_lens[i]].tobytes() == c.payload, c.name
    G.check_slots(status, out_lens, dst, do)


def test_invalid_streams_end_in_their_status():
    L = _lib.lib()
    assert len(INVALID) > 200
    seen = set()
    for name in INVALID:
        c = CORPUS[name]
        rc, msg, status, out_lens, dst, do = G.run_model([c.gz], [G.default_cap(c)])
        assert status == [c.status], (name, status, c.status)
        assert rc != 0 and msg == "gzip stream 0: " + G.TEXT[c.status], (name, msg)
        assert L.tsg_inflate_status_text(c.status).decode() == G.TEXT[c.status]
        assert out_lens[0] <= G.default_cap(c)
        seen.add(c.status)
    assert seen == {G.HEADER, G.CORRUPT, G.EOF, G.CHECKSUM}


def test_truncated_stream_followed_by_its_remainder():
    # a decoder that reads past its stream's end finds the rest of the stream there and wrongly succeeds
    cases = [CORPUS[n] for n in INVALID if CORPUS[n].group == "truncated"]
    rc, msg, status, out_lens, dst, do = G.run_model([c.gz for c in cases], [4096] * len(cases),
                                                     gaps=[G.remainder(c) for c in cases])
    assert rc != 0 and status[0::2] == [G.EOF] * len(cases)
    assert msg == "gzip stream 0: unexpected EOF"
    assert all(o == 0 for o in out_lens[1::2])               # the remainders have slots of no bytes


def test_first_failing_stream_is_named_and_neighbours_stay_valid():
    good, bad = CORPUS["l6"], CORPUS["btype_3"]
    rc, msg, status, out_lens, dst, do = G.run_model([good.gz, bad.gz, good.gz, CORPUS["bad_crc"].gz],
                                                     [len(good.payload), 64, len(good.payload), 4000])
    assert rc != 0 and msg == "gzip stream 1: flate: corrupt input"
    assert status == [G.OK, G.CORRUPT, G.OK, G.CHECKSUM]
    for i in (0, 2):
        assert dst[do[i]:do[i] + out_lens[i]].tobytes() == good.payload
    G.check_slots(status, out_lens, dst, do)


@pytest.mark.parametrize("name", ["l6", "stored_l0", "fixed", "run_a", "overlap_d3", "members_50", "one_byte", "dist_32768"])
def test_slot_exact_and_one_byte_short(name):
    c = CORPUS[name]
    n = len(c.payload)
    rc, msg, status, out_lens, dst, do = G.run_model([c.gz], [n])
    assert (rc, status, out_lens) == (0, [G.OK], [n]) and dst.tobytes() == c.payload
    rc, msg, status, out_lens, dst, do = G.run_model([c.gz], [n - 1])
    assert rc != 0 and status == [G.DST_FULL] and out_lens[0] <= n - 1
    assert msg == "gzip stream 0: the output does not fit its slot"
    assert dst[:out_lens[0]].tobytes() == c.payload[:out_lens[0]]
    assert (dst[out_lens[0]:] == G.FILL).all()


def test_empty_payload_needs_no_slot():
    rc, msg, status, out_lens, dst, do = G.run_model([CORPUS["empty"].gz, CORPUS["members_empty"].gz], [0, 3])
    assert (rc, status, out_lens) == (0, [G.OK, G.OK], [0, 3])


def _crc(data):
    L = _lib.lib()
    a = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
    crc, sl, ns = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    _lib.check(L.tsg_test_crc32_slices(a.ctypes.data, len(data), ctypes.byref(crc), ctypes.byref(sl), ctypes.byref(ns)))
    return crc.value, sl.value, ns.value


def test_crc32_slices_and_combine_equal_zlib():
    _, sl, _ = _crc(b"")
    assert sl == 4096
    rng = np.random.default_rng(2)
    blob = rng.integers(0, 256, 20 * sl + 5, dtype=np.uint8).tobytes()
    lens = [0, 1, sl - 1, sl, sl + 1, 2 * sl - 1, 2 * sl, 2 * sl + 1, len(blob)] + rng.integers(0, len(blob), 3000).tolist()
    for n in lens:
        at = int(rng.integers(0, len(blob) - n + 1))
        crc, _, ns = _crc(blob[at:at + n])
        assert crc == zlib.crc32(blob[at:at + n]) and ns == (n + sl - 1) // sl, n
    assert _crc(bytes(3 * sl))[0] == zlib.crc32(bytes(3 * sl))


def test_size_hint():
    L = _lib.lib()
    v = ctypes.c_uint64()
    s = CORPUS["members_2"].gz
    assert L.tsg_gzip_size_hint(s, len(s), ctypes.byref(v)) == 0 and v.value == 3000     # the last member's alone
    assert L.tsg_gzip_size_hint(b"\0" * 40, 40, ctypes.byref(v)) != 0
    assert L.tsg_gzip_size_hint(s, 17, ctypes.byref(v)) != 0


def test_corpus_is_what_it_claims():
    for name, c in CORPUS.items():
        if c.status == G.OK:
            assert G.py_inflate(c.gz) == c.payload, name
        elif name in PYTHON_ACCEPTS:
            PYTHON_ACCEPTS[name](c.gz)                       # no error: where Python and Go differ
        else:
            with pytest.raises((zlib.error, EOFError, OSError)):
                G.py_inflate(c.gz)
    groups = {c.group for c in CORPUS.values()}
    assert groups == {"blocks", "flush", "matches", "tables", "headers", "big", "invalid", "small", "truncated"}
    assert len(CORPUS["dist_32768"].payload) == 32768 + 358
    assert max(len(c.payload) for c in CORPUS.values() if c.status == G.OK and c.group != "big") <= 256 << 10
    lens = [len(c.gz) for c in G.batch_300()]
    assert len(lens) == 300 and max(lens) > 1000 * min(l for l in lens if l)
