"""The device tar walk on the CPU (tsg_prepare_layer_tar_device_model;
csrc/tarscan.h): marks -> SparseTarInput -> walk_layer -> gate -> interleaved
entries -> plan_prep equals the host call tsg_prepare_layer_tar_opts on every
tar of tests/_tar_corpus.py, with the marks and without them; a walk over the
marked blocks needs at most two reads they do not serve; the walk equals the
oracle's; and the block test tar_block_is_header agrees with the walker's
acceptance of a header on 100k+ blocks."""
import numpy as np
import pytest

import _tar_corpus as TC
from oracle import walker_oracle as wo
from trivy_amd import _lib
from trivy_amd import secret as S

CORPUS = TC.corpus()
_sc = []


def scanner():
    if not _sc:
        _sc.append(S.Scanner(None))
    return _sc[0]


def test_corpus_conditions():
    for t in CORPUS.values():
        if t.check:
            t.check(t.data, TC.py_marks(t.data))
    names = set(CORPUS)
    assert {"ustar", "gnu", "pax", "golden", "names", "sizes", "content", "nested", "prefilter_edge", "special_1mib",
            "special_too_long", "kernel_edges", "flip_name", "flip_size", "flip_checksum", "flip_typeflag", "len_0",
            "len_511", "zero_1", "zero_3", "zero_then_data"} <= names
    assert sum(1 for n in names if n.startswith("trunc_")) > 60


def test_marks_equal_python_restatement():
    # plan_tar_marks against the header test restated in Python, payload rule included
    for t in CORPUS.values():
        tar, nb = t.data, len(t.data) // 512
        want = np.zeros(nb, np.uint8)
        for b in range(nb):
            h = tar[b * 512:(b + 1) * 512]
            if not TC.is_header_py(h):
                continue
            want[b] = 1
            if h[156:157] in (b"x", b"g", b"L", b"K"):
                f = h[124:136]
                size = int.from_bytes(f[1:], "big") if f[0] & 0x80 else int(f.strip(b" \0") or b"0", 8)
                if 0 <= size <= TC.MIB:
                    want[b + 1:b + 1 + (size + 511) // 512] = 1
        assert np.array_equal(TC.py_marks(tar), want), t.name


@pytest.mark.parametrize("opt", range(len(TC.OPTIONS)))
def test_model_equals_host_call(opt):
    opts = TC.OPTIONS[opt]
    sc = scanner()
    nerr = 0
    for t in CORPUS.values():
        kind, want = TC.host_view(sc, t.data, **opts)
        for use_marks in (True, False):
            k, got, fb = TC.model_view(sc, t.data, use_marks, **opts)
            assert (k, got) == (kind, want), (t.name, use_marks)
            if use_marks:
                assert fb <= 2, (t.name, fb)                 # the design's bound
            elif t.data:
                assert fb >= 1, t.name                       # nothing gathered: every read is a fallback
        if kind == "error":
            assert want.startswith("failed to extract the archive: "), (t.name, want)
            nerr += 1
        else:
            assert want["pinned"] is False
            assert t.wellformed or t.name.startswith(("trunc_", "zero_", "len_0", "no_end"))
    assert nerr > 50


def test_error_texts_cover_every_kind():
    sc = scanner()
    seen = {TC.host_view(sc, t.data)[1] for t in CORPUS.values() if TC.host_view(sc, t.data)[0] == "error"}
    pre = "failed to extract the archive: archive/tar: "
    assert {pre + "invalid tar header", pre + "unexpected EOF", pre + "header field too long"} <= seen


def test_gate_and_walk_options_take_effect():
    sc = scanner()
    tar = CORPUS["content"].data
    base = TC.model_view(sc, tar)[1]
    assert base["opq_dirs"] == ["etc/"] and base["wh_files"] == ["var/gone.db", "var/secret.env"]
    assert b"/tiny.txt" not in base["paths"] and b"/bin/tool" not in base["paths"]
    assert dict(zip(base["paths"], base["binary"]))[b"/lib/mod.pyc"] == 1
    assert dict(zip(base["paths"], base["binary"]))[b"/lib/clean.pyc"] == 0
    assert b"\r" not in base["data"]
    skipped = TC.model_view(sc, tar, **TC.OPTIONS[1])[1]
    assert "skipme/inner/key.env" in base["files"] and "skipme/inner/key.env" not in skipped["files"]
    assert "skipped_file.env" not in skipped["files"]
    pats = TC.model_view(sc, tar, **TC.OPTIONS[2])[1]
    assert b"/tiny.txt" in pats["paths"]
    cfg = TC.model_view(sc, tar, **TC.OPTIONS[3])[1]
    assert b"/kept.env" in base["paths"] and b"/kept.env" not in cfg["paths"]


def test_model_walk_equals_oracle():
    sc = scanner()
    n = 0
    for t in CORPUS.values():
        if not t.oracle:
            continue
        for opts in TC.OPTIONS[:2]:
            k, got, _ = TC.model_view(sc, t.data, **opts)
            files, opq, wh = wo.walk(t.data, opts.get("skip_files", ()), opts.get("skip_dirs", ()))
            assert k == "ok", (t.name, got)
            assert got["files"] == [p for p, _ in files], t.name
            assert (got["opq_dirs"], got["wh_files"]) == (opq, wh), t.name
            n += 1
    assert n >= 20


def _blocks_for_predicate():
    rng = np.random.default_rng(5)
    out = [rng.integers(0, 256, (40000, 512), dtype=np.uint8)]
    hi = rng.integers(0x80, 0x100, (10000, 512), dtype=np.uint8)           # all bytes 0x80..0xff
    out += [hi, np.zeros((8, 512), np.uint8)]
    # real headers and mutations of them: one byte changed, one bit changed, the checksum field rewritten
    heads = []
    for t in TC.corpus().values():
        a = np.frombuffer(t.data[:len(t.data) // 512 * 512], np.uint8).reshape(-1, 512)
        m = TC.py_marks(t.data).astype(bool)
        heads.append(a[m][:60])
    heads = np.concatenate(heads)
    heads = heads[[TC.is_header_py(h.tobytes()) for h in heads]]
    assert len(heads) > 300
    out.append(heads)
    for rep in range(70):
        mut = heads.copy()
        k = np.arange(len(mut))
        pos = rng.integers(0, 512, len(mut)) if rep % 2 else rng.integers(148, 156, len(mut))
        if rep % 3 == 0:
            mut[k, pos] ^= (1 << rng.integers(0, 8, len(mut))).astype(np.uint8)
        else:
            mut[k, pos] = rng.choice(np.frombuffer(b" \0" b"01234567" b"89\x80\xff", np.uint8), len(mut))
        out.append(mut)
    # random content under a checksum field that parses: octal, padded, base-256, empty.  The size
    # field and type flag say "directory, no data", so that only the checksum can fail such a block.
    def plain(a):
        a[:, 124:136] = np.frombuffer(b"00000000000\0", np.uint8)
        a[:, 156] = ord("5")
        return a
    fields = [b"0000000\0", b"       \0", b"\0" * 8, b"0177777 ", b" 12345\0 ", b"1 2\0\0\0\0\0", b"\x80\0\0\0\0\0\x7f\x80",
              b"\xff\xff\xff\xff\xff\xff\xff\x00", b"00077400", b"7777777\0"]
    for f in fields:
        a = rng.integers(0, 256, (1500, 512), dtype=np.uint8)
        a[:700] = rng.integers(0, 2, (700, 512), dtype=np.uint8)          # small sums
        plain(a)[:, 148:156] = np.frombuffer(f, np.uint8)
        out.append(a)
    # blocks whose field is set to their own sum, unsigned or signed (negative ones in base-256)
    a = rng.integers(0, 256, (6000, 512), dtype=np.uint8)
    a[3000:, :] |= 0x80
    plain(a)[:, 148:156] = 32
    u = a.astype(np.int64).sum(1)
    s = a.view(np.int8).astype(np.int64).sum(1)
    for i in range(len(a)):
        v = int(u[i]) if i % 2 == 0 else int(s[i])
        if v >= 0:
            a[i, 148:156] = np.frombuffer(b"%07o\0" % v, np.uint8)
        else:
            a[i, 148:156] = np.frombuffer((v & ((1 << 64) - 1)).to_bytes(8, "big"), np.uint8)
    out.append(a)
    return np.ascontiguousarray(np.concatenate(out))


def test_block_test_agrees_with_the_walkers_acceptance():
    """tar_block_is_header(block) <=> walk_layer does not fail at block 0 with
    "invalid tar header" for the one-header tar [block]: the walker's own
    checksum test decides there, before anything else of the header is read.
    (A block that is all NUL is the end marker, which never reaches the test.)"""
    import ctypes
    blocks = _blocks_for_predicate()
    n = len(blocks)
    assert n >= 100_000
    is_h = np.zeros(n, np.uint8)
    L = _lib.lib()
    _lib.check(L.tsg_test_tar_is_header(blocks.ctypes.data, n, is_h.ctypes.data))
    assert 2000 < int(is_h.sum()) < n - 2000
    sc = scanner()
    bad = b"failed to extract the archive: archive/tar: invalid tar header"
    o, keep = _lib.feed_opts(threads=1)
    nonzero = blocks.any(axis=1)
    base = blocks.ctypes.data
    for i in range(n):
        if not nonzero[i]:
            assert not is_h[i]
            continue
        h = ctypes.c_void_p()
        rc = L.tsg_prepare_layer_tar_opts(sc._rs, base + 512 * i, 512, ctypes.byref(o), ctypes.byref(h))
        if rc == 0:
            L.tsg_prepared_free(h)
        accepted = rc == 0 or L.tsg_last_error() != bad
        assert accepted == bool(is_h[i]), (i, rc, L.tsg_last_error())
    del keep
