"""Raw batches for the device-side content preparation (tsg_prepare_batch_device,
its CPU model tsg_prepare_device_model), shared by tests/test_prepare_model.py
and tests/test_gpu_prepare_device.py.

Every file names its expected fate: "text" (kept, CR stripped), "printable"
(a binary .pyc: ExtractPrintableBytes) or "dropped" (the gate, or a binary
that is not a .pyc).  The shapes are the smallest at which the kernels can go
wrong: their grid is 16-byte words, 1 KiB sub-tiles and 64 KiB regions, and
IsBinary reads the first 300 bytes of a file.

corpora() -> {name: Corpus}; a Corpus has files [(path, bytes, fate)],
config_path and file_patterns (the feed options of the case)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALLOW_PATH_CONFIG = os.path.join(GOLDEN, "scanner", "testdata", "global-allow-path.yaml")   # allow path .*\.txt

WORD, SUB, REGION = 16, 1024, 64 * 1024
# IsBinary's trigger bytes below 0x20 (utils.go:74-80): all but 7 8 9 10 12 13 27
TRIGGERS = frozenset(set(range(0, 32)) - {7, 8, 9, 10, 12, 13, 27}) | {0x7F}
ANY = ("secret:.*",)          # a file pattern that passes every path through the gate


class Corpus:
    def __init__(self, name, config_path="", file_patterns=()):
        self.name = name
        self.config_path = config_path
        self.file_patterns = tuple(file_patterns)
        self.files = []
        self.pos = 0
        self._fill = 0

    def add(self, path, data, fate):
        assert fate in ("text", "printable", "dropped")
        self.files.append((path, bytes(data), fate))
        self.pos += len(data)
        return self

    def pad_to(self, pos):
        """A text filler file that ends at raw position pos."""
        n = pos - self.pos
        assert n >= 0, (self.name, pos, self.pos)
        if n:
            self._fill += 1
            body = (b"filler line %d\n" % self._fill) * (n // 10 + 1)
            self.add("fill/f%d.c" % self._fill, body[:n], "text" if n >= 10 or self.file_patterns == ANY else "dropped")
        return self

    @property
    def raw_files(self):
        return [(p, c) for p, c, _ in self.files]

    @property
    def total(self):
        return self.pos


def _text(n, ch=b"t"):
    return (ch * 39 + b"\n") * (n // 40) + ch * (n % 40)


def _head_edges():
    c = Corpus("head_edges")
    for at in (0, 298, 299):                      # inside the sniffed 300 bytes: binary
        body = bytearray(_text(400))
        body[at] = 0
        c.add("head/in%d.txt" % at, body, "dropped")
        c.add("head/in%d.pyc" % at, body, "printable")
    for at in (300, 301):                         # past them: text, and the byte stays
        body = bytearray(_text(400))
        body[at] = 0
        c.add("head/past%d.txt" % at, body, "text")
        c.add("head/past%d.pyc" % at, body, "text")
    for v in list(range(32)) + [0x7F]:            # every control byte at index 5
        c.add("head/byte%02x.txt" % v, b"hello" + bytes([v]) + b"world, more text\r\n",
              "dropped" if v in TRIGGERS else "text")
    c.add("head/high.txt", b"caf\xe9 \x80\x9f\xa0\xad\xff and on\r\n", "text")   # bytes >= 0x80 never trigger
    for n in (10, 11, 150, 299):                  # shorter than 300, the trigger is the last byte
        c.add("head/last%d.txt" % n, b"a" * (n - 1) + b"\x01", "dropped")
    c.add("head/len10.txt", b"0123456789", "text")
    c.add("head/len299.txt", _text(299), "text")
    # the byte right after a short file's end is a trigger byte of the next file
    c.add("head/short.txt", b"short text file\r\n", "text")
    c.add("head/next.txt", b"\x00" + _text(30), "dropped")
    # a head that straddles a sub-tile edge and a region edge: the file starts
    # 150 bytes before it and its only trigger byte lies behind the edge
    for unit in (SUB, REGION, SUB, REGION):
        for at, ext, fate in ((160, "txt", "dropped"), (299, "pyc", "printable"), (300, "txt", "text")):
            edge = -(-(c.pos + 150) // unit) * unit
            if unit == SUB and edge % REGION == 0:                   # a sub-tile edge that is no region edge
                edge += SUB
            c.pad_to(edge - 150)
            body = bytearray(_text(400, b"h"))
            body[at] = 0
            c.add("head/straddle_%d_%d.%s" % (edge, at, ext), body, fate)
    return c


def head_straddles(c, unit):
    """Files of c whose sniffed head (first 300 bytes) crosses a `unit`-byte edge."""
    out, pos = [], 0
    for p, data, _ in c.files:
        n = min(len(data), 300)
        if n and pos // unit != (pos + n - 1) // unit:
            out.append(p)
        pos += len(data)
    return out


def _drop():
    c = Corpus("drop")
    junk = b"\x01" + b"long printable run in a dropped binary\r\n" * 30 + b"\x00\r\r" + b"k" * 700
    c.add("d/a.txt", _text(700) + b"\r\n", "text")
    c.add("d/junk.bin2", junk, "dropped")
    c.add("d/b.txt", b"begins right after the dropped file\r\n" * 20, "text")
    c.add("d/a.pyc", b"\x00first binary pyc\x01" + b"p" * 900 + b"\x02", "printable")
    c.add("d/junk.exe", junk, "dropped")
    c.add("d/b.pyc", b"second\x00binary pyc\x03tail", "printable")
    return c


RUN_DELIMS = (0x00, 0x0A, 0x0D, 0x7F, 0x80, 0x9F, 0xA0, 0xAD)
EDGE_PRINTABLES = (0x20, 0x7E, 0xA1, 0xAC, 0xAE, 0xFF)


def _runs():
    c = Corpus("runs")
    for d in RUN_DELIMS:                          # runs of 0..9 bytes: 4 goes, 5 stays
        body = b"\x00"
        for n in range(10):
            body += bytes([ord("a") + n]) * n + bytes([d])
        c.add("r/delim%02x.pyc" % d, body, "printable")
    for v in EDGE_PRINTABLES:
        c.add("r/edge%02x.pyc" % v, b"\x00" + bytes([v]) * 4 + b"\x00" + bytes([v]) * 5 + b"\x01" + bytes([v]) * 7,
              "printable")
    # two adjacent .pyc files that end and begin with 3 printable bytes: neither run is kept
    c.add("r/end3.pyc", b"\x00abcdefg\x00xyz", "printable")
    c.add("r/begin3.pyc", b"uvw\x00hijklmn\x00", "printable")
    # a file ending inside a run: the '\n' is appended, the file grows by one
    c.add("r/grows.pyc", b"abcde\x00fghij", "printable")
    c.add("r/after_grows.txt", b"its start shifts by one\r\n", "text")
    # a clean head: the text path for a .pyc -- CR stripped, short runs and NULs kept
    c.add("r/clean_head.pyc", b"A" * 300 + b"\r\nab\x00cd\r\x01e", "text")
    # a binary .pyc directly before a text file that starts with printable bytes
    c.add("r/before_text.pyc", b"\x00printable\x00abc", "printable")
    c.add("r/text_after.txt", b"defghij starts printable\r\n", "text")
    return c


def _runs_at_edges(name, unit, nedges_from):
    """One binary .pyc of NULs with a 5-run and a 4-run starting at every
    offset -8..+8 around `unit`-byte edges, each run at an edge of its own."""
    c = Corpus(name)
    c.add("e/lead.txt", _text(100), "text")
    spans = [(n, d) for d in range(-8, 9) for n in (5, 4)]
    start = c.pos
    step = unit if unit >= 64 else 64             # 16-byte edges: one run per 64 bytes
    first_edge = ((start + 16) // step + nedges_from) * step
    body = bytearray(first_edge - start + step * len(spans) + 16)
    for k, (n, d) in enumerate(spans):
        at = first_edge + k * step + d - start
        body[at:at + n] = bytes([ord("A") + k % 26]) * n
    c.add("e/edges.pyc", body, "printable")
    c.add("e/tail.txt", _text(50), "text")
    return c


def _long_run():
    c = Corpus("long_run")
    c.add("l/lead.txt", _text(1000), "text")
    c.add("l/run.pyc", b"\x00" + b"x" * 200_000 + b"\x00", "printable")      # kept whole, one '\n'
    c.add("l/run_to_end.pyc", b"\x01" + b"y" * 70_000, "printable")           # ends inside the run
    c.add("l/tail.txt", _text(64), "text")
    return c


def _all_grow():
    """Every file an allowed binary that grows by one: prepared = total + files."""
    c = Corpus("all_grow")
    for k in range(5):
        c.add("g/%d.pyc" % k, b"abcde" * (k + 1) + b"\x00" + b"fghij" * (3 * k + 1), "printable")
    return c


def _cr(kind):
    """The shapes of tests/test_cr_strip.py, every file passed through the gate."""
    rng = np.random.default_rng(sum(kind.encode()))
    c = Corpus("cr_" + kind, file_patterns=ANY)
    files = []
    if kind == "ragged":
        files = [b"", b"\r", b"\r\r\r\r", b"a\r", b"\rb", b"abc", b"x" * 15, b"\r" * 17]
        for _ in range(300):                       # tiny files, many per sub-tile
            files.append(bytes(rng.choice(np.frombuffer(b"ab\r\n", np.uint8), int(rng.integers(0, 24)))))
        for n in (65535, 65536, 65537, 131072 + 7, 300_001):   # across 64 KiB regions
            a = rng.integers(32, 127, n, dtype=np.uint8)
            a[rng.random(n) < 0.03] = 13
            files.append(a.tobytes())
        files += [b"", b""]                        # trailing empty files end at the batch end
    elif kind == "no_cr":
        files = [rng.integers(32, 127, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 100_000, 24)]
    elif kind == "dense":
        for n in rng.integers(0, 70_000, 16):
            a = np.full(int(n), 13, np.uint8)
            a[rng.random(int(n)) < 0.01] = ord("k")
            files.append(a.tobytes())
    elif kind == "crlf":
        for n in rng.integers(1, 40_000, 60):
            lines = [bytes(rng.integers(97, 123, int(m), dtype=np.uint8)) for m in rng.integers(0, 80, int(n) // 40 + 1)]
            files.append(b"\r\n".join(lines) + (b"\r\n" if n % 2 else b""))
    elif kind == "all_empty":
        files = [b"", b"", b""]
    for k, f in enumerate(files):
        c.add("cr/%s_%d.txt" % (kind, k), f, "text")
    return c


def _gate(patterns):
    c = Corpus("gate_patterns" if patterns else "gate", config_path=ALLOW_PATH_CONFIG, file_patterns=patterns)
    body = b"secret text that the gate decides about\r\n"
    c.add("src/main.py", body, "text")
    c.add("node_modules/pkg/index.js", body, "dropped")
    c.add("img.png", body, "text" if patterns else "dropped")
    c.add("tiny.cfg", b"nine byte", "text" if patterns else "dropped")
    c.add("global-allow-path.yaml", body, "dropped")          # the config file's base name
    c.add("docs/notes.txt", body, "dropped")                  # the global allow path
    c.add("lib/mod.pyc", b"\x00binary pyc content\x01", "printable")
    c.add("src/last.go", body, "text")
    return c


def _sizes(rem):
    """Empty files anywhere, trailing dropped and empty files, total = rem (mod 16)."""
    c = Corpus("sizes_mod%d" % rem)
    c.add("s/e0.txt", b"", "dropped")
    c.add("s/a.txt", _text(100) + b"\r\n", "text")
    c.add("s/e1.txt", b"", "dropped")
    c.add("s/e2.pyc", b"", "dropped")
    c.add("s/b.pyc", b"\x00" + b"q" * 50 + b"\x00\x00", "printable")
    c.add("s/e3.txt", b"", "dropped")
    c.add("s/c.txt", _text(2000), "text")
    c.pad_to(c.pos + 40 + (rem - (c.pos + 40 + 30)) % 16)
    c.add("s/trail.bin", b"\x00" * 30, "dropped")
    c.add("s/e4.txt", b"", "dropped")
    c.add("s/e5.txt", b"", "dropped")
    assert c.total % 16 == rem
    return c


def _all_dropped():
    c = Corpus("all_dropped")
    c.add("x/a.png", _text(500), "dropped")
    c.add("x/b.txt", b"\x00" + _text(3000), "dropped")
    c.add("x/c.txt", b"short", "dropped")
    c.add("x/e.txt", b"", "dropped")
    return c


def _tiny_mixed():
    """300 tiny files of mixed kinds inside one sub-tile."""
    c = Corpus("tiny_mixed", file_patterns=ANY)
    c.add("t/lead.txt", _text(SUB + 8), "text")
    shapes = ((b"ab\r", "txt", "text"), (b"\x00abcde", "pyc", "printable"), (b"\x01\r", "txt", "dropped"),
              (b"", "txt", "text"), (b"abcdef\x00", "pyc", "printable"), (b"q", "txt", "text"),
              (b"\x00ab", "pyc", "printable"), (b"abc", "pyc", "text"))
    for k in range(300):
        body, ext, fate = shapes[k % len(shapes)]
        c.add("t/%d.%s" % (k, ext), body, fate)
    assert c.pos < 2 * SUB
    c.add("t/tail.txt", _text(300), "text")
    return c


def corpora():
    out = [_head_edges(), _drop(), _runs(), _runs_at_edges("runs_word_edges", WORD, 4),
           _runs_at_edges("runs_subtile_edges", SUB, 1), _runs_at_edges("runs_region_edges", REGION, 1),
           _long_run(), _all_grow()]
    out += [_cr(k) for k in ("ragged", "dense", "crlf", "no_cr", "all_empty")]
    out += [_gate(()), _gate(("secret:tiny\\.cfg$", "secret:\\.png$", "dockerfile:Dockerfile.*"))]
    out += [_sizes(0), _sizes(1), _sizes(15), _all_dropped(), _tiny_mixed()]
    return {c.name: c for c in out}


NAMES = ["head_edges", "drop", "runs", "runs_word_edges", "runs_subtile_edges", "runs_region_edges", "long_run",
         "all_grow", "cr_ragged", "cr_dense", "cr_crlf", "cr_no_cr", "cr_all_empty", "gate", "gate_patterns",
         "sizes_mod0", "sizes_mod1", "sizes_mod15", "all_dropped", "tiny_mixed"]
