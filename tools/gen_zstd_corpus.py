#!/usr/bin/env python3
"""Write tests/golden/zstd/*.zst: the compressed fixtures of tests/_zstd_corpus.py.

    python tools/gen_zstd_corpus.py [--check]

Every frame is compressed by the system libzstd (ctypes; ZSTD_compress2 with
the parameters of its Spec) from the seeded input of its Spec, decoded again by
libzstd, decoded by the CPU model (tsg_test_zstd_trace), and the model's trace
must show every condition the fixture was built for: a fixture that does not
hold what its name says is an error here, not a silent gap in the tests.
--check writes nothing and fails when a committed file differs."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _zstd_corpus as Z  # noqa: E402

# ZSTD_cParameter (zstd.h)
C_LEVEL, C_WINDOW_LOG, C_CONTENT_SIZE, C_CHECKSUM = 100, 101, 200, 201
MAX_FILE, MAX_TOTAL = 256 * 1024, 1000 * 1000


def libzstd():
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    z.ZSTD_compress2.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return z


def compress(z, data, level=3, window_log=0, checksum=0, content_size=1):
    c = z.ZSTD_createCCtx()
    try:
        for p, v in ((C_LEVEL, level), (C_WINDOW_LOG, window_log), (C_CHECKSUM, checksum), (C_CONTENT_SIZE, content_size)):
            if z.ZSTD_isError(z.ZSTD_CCtx_setParameter(c, p, v)):
                raise RuntimeError("ZSTD_CCtx_setParameter(%d, %d)" % (p, v))
        out = ctypes.create_string_buffer(z.ZSTD_compressBound(len(data)))
        n = z.ZSTD_compress2(c, out, len(out), data, len(data))
        if z.ZSTD_isError(n):
            raise RuntimeError("ZSTD_compress2")
        return out.raw[:n]
    finally:
        z.ZSTD_freeCCtx(c)


def decompress(z, blob, cap):
    """bytes, or None where libzstd reports an error"""
    out = ctypes.create_string_buffer(max(cap, 1))
    n = z.ZSTD_decompress(out, cap, blob, len(blob))
    return None if z.ZSTD_isError(n) else out.raw[:n]


def checked(z, name, data, params, need):
    blob = compress(z, data, **params)
    assert decompress(z, blob, len(data)) == data, name
    ev, st = Z.trace(blob, len(data))
    assert st == Z.OK, (name, st)
    missing = [e for e in need if not ev[e]]
    return blob, ev, missing


def main():
    check = "--check" in sys.argv
    z = libzstd()
    files, group_events = {}, {}
    for s in Z.SPECS:
        blob, ev, missing = checked(z, s.name, Z.payload_of(s), s.params, s.need)
        assert not missing, "%s lacks %s" % (s.name, missing)
        files[s.name + ".zst"] = blob
        for e, n in ev.items():
            if n:
                group_events.setdefault(s.group, set()).add(e)
    for key, (group, gen, seed, params, event) in Z.SEARCHED.items():
        for n in range(600, 6000):              # the first input length whose only block holds that many sequences
            blob, ev, missing = checked(z, key, Z.GEN[gen](n, seed), params, [event])
            if not missing:
                files["%s_n%d.zst" % (key, n)] = blob
                group_events.setdefault(group, set()).update(e for e, k in ev.items() if k)
                break
        else:
            raise AssertionError("no input length gives " + event)
    tars = Z.layer_tars()
    for name, level in Z.LAYER_LEVELS.items():
        files["layer_%s.zst" % name], _, _ = checked(z, name, tars[name], dict(level=level, checksum=1), [])
    for name, (group, blob, payload) in Z.hand_blocks().items():
        assert decompress(z, blob, len(payload)) == payload, name
        ev, st = Z.trace(blob, len(payload))
        assert st == Z.OK, (name, st)
        group_events.setdefault(group, set()).update(e for e, k in ev.items() if k)
    lacking = [e for e in Z.SEQUENCE_EVENTS if e not in group_events["sequences"]]
    assert not lacking, "the sequences group lacks %s" % lacking
    for e in ("lit_raw", "lit_rle", "lit_fmt0", "lit_fmt1", "lit_fmt3", "lit_huf1", "lit_huf4", "lit_treeless", "weights_direct",
              "weights_fse", "huf_bits11"):
        assert e in group_events["literals"], e
    total = sum(len(b) for b in files.values())
    assert total < MAX_TOTAL and all(len(b) < MAX_FILE for b in files.values()), total
    os.makedirs(Z.GOLDEN, exist_ok=True)
    stale = [f for f in os.listdir(Z.GOLDEN) if f.endswith(".zst") and f not in files]
    for fn, blob in sorted(files.items()):
        path = os.path.join(Z.GOLDEN, fn)
        if check:
            assert open(path, "rb").read() == blob, fn + " differs"
        else:
            with open(path, "wb") as f:
                f.write(blob)
    if check:
        assert not stale, stale
    else:
        for fn in stale:
            os.remove(os.path.join(Z.GOLDEN, fn))
    # the hand-built streams: what they claim, and libzstd's verdict on them
    Z._CORPUS = None
    c = Z.corpus()
    need = {"fcs0": "fcs0", "fcs2": "fcs2", "fcs4": "fcs4", "fcs8": "fcs8", "fcs1_single": "fcs1", "fcs2_single": "single_segment",
            "skip_before": "skippable", "skip_between": "skippable", "skip_after": "skippable", "empty_frame": "empty_frame",
            "rle_blocks": "block_rle", "rle_128k": "block_rle"}
    for name, case in c.items():
        if case.group == "frames" or name in Z.hand_blocks():
            ev, st = Z.trace(case.z, len(case.payload))
            assert st == Z.OK and (name not in need or ev[need[name]]), (name, st)
            assert decompress(z, case.z, len(case.payload)) == case.payload, name
        elif case.group == "invalid":
            ev, st = Z.trace(case.z, Z.default_cap(case))
            assert st == case.status, (name, st, case.status)
    assert Z.trace(c["tiny_300"].z, 4096)[0]["frame"] == 300
    print("%d files, %d bytes; %d cases" % (len(files), total, len(c)))


if __name__ == "__main__":
    main()
