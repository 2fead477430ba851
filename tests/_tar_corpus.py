"""Layer tars for the device tar walk (tsg_prepare_layer_tar_device; csrc/tarscan.h,
tarscan.hip): every tar format, size-field and name case the walk knows,
tars stored inside the layer (blocks that pass the header test without being
headers), the prefilter's and the kernels' edges, and malformed archives.

corpus() -> {name: Tar}.  A Tar carries the conditions it is meant to meet
(`check(tar bytes, marks)`, marks = plan_tar_marks as a uint8 array); the CPU
test asserts them, so that a tar cannot silently lose its edge.  The kernels'
units (tarscan.hip): a wave step of 64 blocks, a region of 128 blocks per
wave, a workgroup of 4 regions.

views: host_view / model_view run tsg_prepare_layer_tar_opts and
tsg_prepare_layer_tar_device_model and return either ("ok", dict) or
("error", message)."""
import ctypes
import io
import json
import tarfile

import numpy as np

from test_layer_tar import AWS, GHP, _fixture, _make_layer, _pax_layer, _raw_header
from trivy_amd import _lib
from trivy_amd import secret as S

STEP, REGION, GROUP = 64, 128, 512          # blocks
GNU_MAGIC = b"ustar  \0"
MIB = 1 << 20


def pad(b):
    return b + bytes(-len(b) % 512)


def hdr(name, size, typ, prefix=b"", magic=b"ustar\x0000", size_field=None, signed=False, linkname=b""):
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108] = b"0000644\0"
    h[108:116] = h[116:124] = b"0000000\0"
    h[124:136] = size_field if size_field is not None else b"%011o\0" % size
    h[136:148] = b"00000000000\0"
    h[156] = typ if isinstance(typ, int) else ord(typ)
    h[157:157 + len(linkname)] = linkname
    h[257:257 + len(magic)] = magic
    h[345:345 + len(prefix)] = prefix
    h[148:156] = b" " * 8
    s = sum(b - 256 if b >= 128 else b for b in h) if signed else sum(h)
    h[148:156] = b"%06o\0 " % s
    return bytes(h)


def entry(name, data, typ="0", **kw):
    return hdr(name, len(data), typ, **kw) + pad(data)


def pax_rec(key, val):
    rec = key + b"=" + val + b"\n"
    n = len(rec) + 2
    while len(b"%d " % n) + len(rec) != n:
        n += 1
    return b"%d " % n + rec


def pax_rec_of(total, key=b"comment"):
    """one record of exactly `total` bytes"""
    head = b"%d " % total + key + b"="
    return head + b"v" * (total - len(head) - 1) + b"\n"


END = bytes(1024)
TEXT = b"".join(b"line %04d of some text\n" % i for i in range(400))


def is_header_py(b):
    """the header test, restated: archive/tar parseNumeric of bytes 148..155, both sums"""
    f = b[148:156]
    if f[0] & 0x80:
        inv = 0xff if f[0] & 0x40 else 0
        x = 0
        for i, c in enumerate(f):
            c ^= inv
            if i == 0:
                c &= 0x7f
            x = (x << 8) | c
        want = ~x if inv else x
    else:
        t = f.strip(b" \0")
        if any(c not in b"01234567" for c in t):
            return False
        want = int(t, 8) if t else 0
    body = b[:148] + b" " * 8 + b[156:]
    return want in (sum(body), sum(c - 256 if c >= 128 else c for c in body))


class Tar:
    def __init__(self, name, data, check=None, oracle=True, wellformed=True):
        self.name, self.data, self.check = name, bytes(data), check
        self.wellformed = wellformed
        self.oracle = oracle and wellformed          # compared with oracle.walker_oracle too


def _types_in(tar):
    return {tar[b + 156:b + 157] for b in range(0, len(tar) - 511, 512) if is_header_py(tar[b:b + 512])}


def _fill_to(parts, block, k):
    """a filler entry so that the next entry's header is block `block`"""
    cur = sum(len(p) for p in parts) // 512
    gap = block - cur
    assert gap >= 1, (block, cur)
    parts.append(entry(b"fill/%03d.txt" % k, (TEXT * 200)[:(gap - 1) * 512 - 7 if gap > 1 else 0]))
    assert sum(len(p) for p in parts) // 512 == block


def _names():
    long1 = b"deep/" + b"/".join(b"gnu_long_directory_%02d" % i for i in range(6)) + b"/secret.env"
    long2 = b"deep/" + b"/".join(b"pax_long_directory_%02d" % i for i in range(6)) + b"/token.txt"
    longlink = b"target/" + b"x" * 120
    assert len(long1) > 100 and len(long2) > 100
    parts = [
        entry(b"pax_global_header", pax_rec(b"comment", b"a global header"), "g"),
        entry(b"././@LongLink", long1 + b"\0", "L", magic=GNU_MAGIC), entry(long1[:100], AWS * 2, "0", magic=GNU_MAGIC),
        entry(b"PaxHeaders/token", pax_rec(b"path", long2) + pax_rec(b"mtime", b"1700000000.5"), "x"),
        entry(b"short", GHP * 2),
        entry(b"././@LongLink", longlink + b"\0", "K", magic=GNU_MAGIC),
        hdr(b"app/lnk", 0, "2", linkname=longlink[:100], magic=GNU_MAGIC),
        entry(b"file_with_prefix.txt", AWS + TEXT[:900], prefix=b"usr/share/" + b"p" * 100),
        END]

    def check(tar, marks):
        assert {b"g", b"L", b"K", b"x"} <= _types_in(tar)
        assert any(tar[b + 345] for b in range(0, len(tar), 512) if is_header_py(tar[b:b + 512]))
    return Tar("names", b"".join(parts), check)


def _sizes():
    body = GHP + b"y" * 659
    parts = [
        # PAX size= larger and smaller than the header's size field
        entry(b"PaxHeaders/a", pax_rec(b"size", b"700"), "x"), hdr(b"pax_larger.txt", 100, "0") + pad(body),
        entry(b"PaxHeaders/b", pax_rec(b"size", b"700"), "x"), hdr(b"pax_smaller.txt", 5000, "0") + pad(body),
        # a base-256 size field
        hdr(b"base256.txt", 0, "0", size_field=b"\x80" + (700).to_bytes(11, "big")) + pad(body),
        # header-only types with a size field: no data follows
        hdr(b"hard", 4096, "1", linkname=b"base256.txt"), hdr(b"sym", 4096, "2", linkname=b"x"),
        hdr(b"chr", 512, "3"), hdr(b"blk", 512, "4"), hdr(b"dir_with_size", 8192, "5"), hdr(b"fifo", 1024, "6"),
        # type flag NUL: a directory with a trailing '/', else a regular file
        hdr(b"olddir/", 1024, 0), entry(b"olddir/oldfile.txt", AWS + TEXT[:300], 0),
        # V7: no magic
        entry(b"v7file.txt", GHP + TEXT[:200], "0", magic=b""),
        # a checksum that verifies only as the signed sum
        entry("café_signed.txt".encode(), AWS + TEXT[:100], "0", signed=True),
        END]
    tar = b"".join(parts)

    def check(tar, marks):
        signed = [b for b in range(0, len(tar), 512) if tar[b:b + 3] == b"caf"][0]
        blk = tar[signed:signed + 512]
        bodyb = blk[:148] + b" " * 8 + blk[156:]
        assert int(blk[148:154], 8) == sum(c - 256 if c >= 128 else c for c in bodyb) != sum(bodyb)
        assert any(tar[b + 124] & 0x80 for b in range(0, len(tar), 512) if is_header_py(tar[b:b + 512]))
        assert {b"1", b"2", b"3", b"4", b"5", b"6", b"\0"} <= _types_in(tar)
    return Tar("sizes", tar, check)


def _content():
    pyc_bin = b"\x00\x01\x02head\x00" + AWS.strip() + b"\x00\x03tail of the binary" + b"\x00" * 40
    parts = [
        hdr(b"etc/", 0, "5"), hdr(b"skipme/", 0, "5"),
        entry(b"etc/crlf.conf", (AWS + TEXT[:2000]).replace(b"\n", b"\r\n")),
        entry(b"bin/tool", b"\x7fELF\x01\x01" + AWS + b"\x00" * 1000),
        entry(b"lib/mod.pyc", pyc_bin), entry(b"lib/clean.pyc", b"x = 1\r\n" + GHP),
        entry(b"tiny.txt", b"tiny"), entry(b"nine.txt", b"123456789"),
        entry(b"empty1", b""), entry(b"empty2", b""), entry(b"empty3.txt", b""),
        entry(b"etc/.wh..wh..opq", b""), entry(b"var/.wh.gone.db", b""), entry(b"var/.wh.secret.env", AWS),
        entry(b"skipme/inner/key.env", AWS), entry(b"skipped_file.env", GHP), entry(b"kept.env", GHP),
        END]

    def check(tar, marks):
        hd = [b // 512 for b in range(0, len(tar), 512) if is_header_py(tar[b:b + 512])]
        assert any(b + 1 in hd and b + 2 in hd for b in hd)        # empty files: adjacent headers
    return Tar("content", b"".join(parts), check)


def _inner_tar():
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.PAX_FORMAT) as tf:
        for i in range(5):
            data = AWS + b"inner %d\n" % i * 50
            ti = tarfile.TarInfo("inner/" + "n" * (120 if i == 2 else 5) + "%d.txt" % i)
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
    return buf.getvalue()


def _nested():
    inner = _inner_tar()
    spill = hdr(b"PaxHeaders/spill", 20 * 512, "x") + bytes(512)      # its claimed payload: 20 blocks
    parts = [entry(b"backup/inner.tar", inner), entry(b"backup/spill.tar", spill),
             entry(b"after_spill.txt", (TEXT * 2)[:30 * 512 - 100]), entry(b"last.env", AWS),
             entry(b"backup/past_end.tar", hdr(b"PaxHeaders/huge", MIB, "x")), END]
    tar = b"".join(parts)
    o_inner, o_spill = 512, 512 + len(pad(inner)) + 512

    def check(tar, marks):
        nb = len(tar) // 512
        assert marks[o_inner // 512:(o_inner + len(inner)) // 512].sum() >= 6     # false positives
        assert marks[o_spill // 512 + 1:o_spill // 512 + 21].all()                # past the enclosing file's 2 blocks
        assert not marks[o_spill // 512 + 21:o_spill // 512 + 30].any()           # the next file's data
        assert marks[nb - 2:].all()                                               # clipped at the tar's end
    return Tar("nested", tar, check)


def _prefilter_edge():
    blk = bytearray((TEXT * 2)[:512])
    blk[148:156] = b"0012345\0"
    data = TEXT[:1024] + bytes(blk) + TEXT[:700]
    tar = entry(b"data/edge.txt", data) + entry(b"zeros.bin", bytes(4096)) + END

    def check(tar, marks):
        b = 512 + 1024
        assert tar[b + 148:b + 156] == b"0012345\0" and not is_header_py(tar[b:b + 512]) and not marks[b // 512]
        assert marks.sum() == 2
    return Tar("prefilter_edge", tar, check)


def _special_1mib():
    tar = (entry(b"PaxHeaders/big", pax_rec_of(MIB), "x") + entry(b"after_big.env", AWS) + END)

    def check(tar, marks):
        assert int(tar[124:135], 8) == MIB and marks[:1 + MIB // 512 + 1].all()
    return Tar("special_1mib", tar, check)


def _special_too_long():
    tar = entry(b"././@LongLink", b"n" * (MIB + 1), "L", magic=GNU_MAGIC) + entry(b"f.txt", AWS) + END

    def check(tar, marks):
        assert int(tar[124:135], 8) == MIB + 1 and marks[0] and not marks[1:MIB // 512].any()
    return Tar("special_too_long", tar, check, wellformed=False)


def _kernel_edges():
    parts = [entry(b"first.env", AWS)]
    at = []
    for k, block in enumerate((STEP - 1, REGION - 1, GROUP - 1, GROUP + 2 * REGION - 1)):
        _fill_to(parts, block, k)
        at.append(block)
        parts.append(entry(b"PaxHeaders/e%d" % k, pax_rec(b"path", b"edge/file_%d.env" % k), "x"))
        parts.append(entry(b"e%d" % k, GHP + b"%d\n" % k))
    # a payload that spans a whole region
    _fill_to(parts, GROUP + 4 * REGION - 3, 9)
    parts.append(entry(b"PaxHeaders/wide", pax_rec_of(300 * 512 - 11), "x"))
    parts.append(entry(b"wide.env", AWS))
    parts.append(END)
    tar = b"".join(parts)

    def check(tar, marks):
        nb = len(tar) // 512
        assert nb > 2 * GROUP
        for b in at:
            assert tar[b * 512 + 156:b * 512 + 157] == b"x" and marks[b] and marks[b + 1]
        assert any(marks[r * REGION:(r + 1) * REGION].all() and not is_header_py(tar[r * REGION * 512:][:512])
                   for r in range(nb // REGION))
    return Tar("kernel_edges", tar, check)


def _small_pax():
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.PAX_FORMAT) as tf:
        for name, data in (("etc/app.env", AWS), ("deep/" + "d" * 110 + "/long.txt", GHP + TEXT[:600]),
                           ("empty", b""), ("src/main.py", TEXT[:1500])):
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
    tar = buf.getvalue()
    end = max(b for b in range(0, len(tar), 512) if any(tar[b:b + 512])) + 512
    return tar[:end + 1024]


def _malformed(out):
    base = _small_pax()
    assert len(base) // 512 <= 40
    cuts = sorted({c + d for c in range(0, len(base) + 1, 512) for d in (0, 1, -1, 255, -255) if 0 <= c + d <= len(base)})
    for c in cuts:
        out.append(Tar("trunc_%05d" % c, base[:c], wellformed=False))
    first = 0
    second = [b for b in range(512, len(base), 512) if is_header_py(base[b:b + 512]) and base[b + 156:b + 157] == b"0"][0]
    for field, off in (("name", first + 3), ("size", second + 133), ("checksum", first + 150), ("typeflag", first + 156)):
        t = bytearray(base)
        t[off] ^= 0x01
        out.append(Tar("flip_" + field, t, wellformed=False))
    out.append(Tar("len_0", b"", wellformed=False))
    out.append(Tar("len_511", base[:511], wellformed=False))
    out.append(Tar("zero_1", bytes(512), wellformed=False))
    out.append(Tar("zero_3", bytes(1536), wellformed=False))
    out.append(Tar("zero_then_data", bytes(512) + TEXT[:512] + TEXT[:512], wellformed=False))
    out.append(Tar("zero_then_header", bytes(512) + entry(b"late.env", AWS) + END, wellformed=False))
    out.append(Tar("zero_then_tail", entry(b"ok.env", AWS) + bytes(512) + b"\0" * 100, wellformed=False))
    out.append(Tar("no_end_marker", entry(b"ok.env", AWS), wellformed=False))


_corpus = None


def corpus():
    global _corpus
    if _corpus is None:
        tars = []
        for fmt, name in ((tarfile.USTAR_FORMAT, "ustar"), (tarfile.GNU_FORMAT, "gnu"), (tarfile.PAX_FORMAT, "pax")):
            want = {tarfile.USTAR_FORMAT: None, tarfile.GNU_FORMAT: b"L", tarfile.PAX_FORMAT: b"x"}[fmt]

            def check(tar, marks, want=want):
                if want:
                    assert want in _types_in(tar)
                else:
                    assert any(tar[b + 345] for b in range(0, len(tar), 512) if is_header_py(tar[b:b + 512]))
            tars.append(Tar(name, _make_layer(10 + fmt, fmt), check))
        tars.append(Tar("golden", _fixture()))
        tars.append(Tar("pax_size", _pax_layer(b"700")))
        tars += [_names(), _sizes(), _content(), _nested(), _prefilter_edge(), _special_1mib(), _special_too_long(),
                 _kernel_edges()]
        _malformed(tars)
        _corpus = {t.name: t for t in tars}
        assert len(_corpus) == len(tars)
    return _corpus


OPTIONS = [
    dict(),
    dict(skip_files=("**/*.md", "skipped_file.env", "app/src/*.{py,js}"), skip_dirs=("node_modules", "skipme", "/var/cache")),
    dict(file_patterns=("secret:\\.(png|lock)$", "secret:^tiny\\.txt$")),
    dict(config_path="conf/kept.env", skip_dirs=("usr/**",)),
]


def py_marks(tar):
    n = len(tar) // 512
    m = np.zeros(max(n, 1), np.uint8)
    _lib.check(_lib.lib().tsg_test_tar_marks(tar, len(tar), m.ctypes.data))
    return m[:n]


def _view_of(L, h):
    try:
        offs, idx, binf, data = S._prepared_view(L, h)
        pp, pl = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_uint32)()
        _lib.check(L.tsg_prepared_paths(h, ctypes.byref(pp), ctypes.byref(pl)))
        paths = [ctypes.string_at(pp[k], pl[k]) for k in range(len(idx))]
        walk = json.loads(L.tsg_prepared_walk_json(h).decode("utf-8", "surrogateescape"))
        return dict(offsets=offs.tolist(), index=idx, binary=binf, data=data, paths=paths, files=walk["files"],
                    opq_dirs=walk["opq_dirs"], wh_files=walk["wh_files"], pinned=walk["pinned"])
    finally:
        L.tsg_prepared_free(h)


def host_view(sc, tar, **opts):
    L = _lib.lib()
    o, keep = _lib.feed_opts(opts.get("config_path", ""), opts.get("file_patterns", ()), opts.get("skip_files", ()),
                             opts.get("skip_dirs", ()), threads=2)
    h = ctypes.c_void_p()
    rc = L.tsg_prepare_layer_tar_opts(sc._rs, tar, len(tar), ctypes.byref(o), ctypes.byref(h))
    del keep
    if rc:
        return "error", L.tsg_last_error().decode("utf-8", "replace")
    return "ok", _view_of(L, h)


def model_view(sc, tar, use_marks=True, **opts):
    """(kind, view or message, fallback reads)"""
    L = _lib.lib()
    o, keep = _lib.feed_opts(opts.get("config_path", ""), opts.get("file_patterns", ()), opts.get("skip_files", ()),
                             opts.get("skip_dirs", ()), threads=2)
    h, fb = ctypes.c_void_p(), ctypes.c_uint32()
    rc = L.tsg_prepare_layer_tar_device_model(sc._rs, tar, len(tar), ctypes.byref(o), 1 if use_marks else 0,
                                              ctypes.byref(fb), ctypes.byref(h))
    del keep
    if rc:
        return "error", L.tsg_last_error().decode("utf-8", "replace"), fb.value
    return "ok", _view_of(L, h), fb.value
