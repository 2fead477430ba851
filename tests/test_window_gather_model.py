"""The device-only scan with windows, without a GPU: the layout
(csrc/gather.h plan_gather_windows) against a numpy restatement, the anchored
regex runs' examined position (goregexp match_*_examined), and the windowed
CPU model (tsg_scan_device_model_opts: table-model candidates, the layout, a
memcpy gather with every run in an allocation of its own, scan_file_windows,
the fallback round) against the table model and the oracle on every corpus of
tests/_window_corpus.py -- findings equal, the insufficient files equal to the
set each corpus names.
"""
import json
import tempfile

import numpy as np
import pytest

import _window_corpus as WC
from _oracle_pool import oracle_scan_many
from oracle import secret_oracle as so
from trivy_amd import secret as S

NONE, WHOLE, WINDOW = WC.NONE, WC.WHOLE, WC.WINDOW
NO_RUN = 0xFFFFFFFF
_SC = {}


def scanner(cfg):
    key = repr(cfg)
    if key not in _SC:
        _SC[key] = S.Scanner(cfg)
    return _SC[key]


# ------------------------------------------------------------------ layout
def numpy_layout(off, cands, fflags, all_rules, windowable, chunk, window, lead):
    """gather.h plan_gather_windows restated with sets and numpy."""
    before, after, min_file = window
    off = np.asarray(off, np.int64)
    nfiles = len(off) - 1
    total = int(off[-1])
    nchunks = -(-total // chunk)
    lens = np.diff(off)
    has = np.zeros(nfiles, bool)
    whole = np.zeros(nfiles, bool)
    for f, r, s in cands:
        if lead <= f < nfiles:
            has[f] = True
            if r >= len(windowable) or not windowable[r] or s >= lens[f]:
                whole[f] = True
    cls = np.zeros(nfiles, np.uint8)
    marks = np.zeros(nchunks, bool)
    for f in range(lead, nfiles):
        if all_rules or fflags[f] or has[f]:
            w = all_rules or fflags[f] or whole[f] or lens[f] < min_file or lens[f] == 0
            cls[f] = WHOLE if w else WINDOW
            if not w:
                marks[off[f] // chunk] = True
    for f, r, s in cands:
        if lead <= f < nfiles and cls[f] == WINDOW:
            lo, hi = WC.window_chunks(int(off[f]), int(lens[f]), s, before, after, chunk)
            nfc = (off[f + 1] - 1) // chunk - off[f] // chunk + 1
            if 2 * (hi - lo + 1) > nfc:
                whole[f] = True
            else:
                marks[lo:hi + 1] = True
    window_marks = marks.copy()
    for f in range(lead, nfiles):
        if cls[f] == WINDOW:
            c0, c1 = off[f] // chunk, (off[f + 1] - 1) // chunk
            if whole[f] or 2 * int(window_marks[c0:c1 + 1].sum()) > c1 - c0 + 1:
                cls[f] = WHOLE
    for f in range(lead, nfiles):
        if cls[f] == WHOLE:
            if lens[f] == 0:
                if off[f] // chunk < nchunks:
                    marks[off[f] // chunk] = True
            else:
                marks[off[f] // chunk:(off[f + 1] - 1) // chunk + 1] = True
    m = np.concatenate([[False], marks, [False]]).astype(np.int8)
    starts = np.nonzero(np.diff(m) == 1)[0]
    ends = np.nonzero(np.diff(m) == -1)[0]
    before_marks = np.concatenate([[0], np.cumsum(marks)])
    runs = np.array([(a * chunk, before_marks[a] * chunk, min(b * chunk, total) - a * chunk) for a, b in zip(starts, ends)],
                    np.uint64).reshape(-1, 3)
    gathered = int(runs[-1][1] + runs[-1][2]) if len(runs) else 0
    return cls, marks, runs, -(-gathered // 64) * 64


def check_layout(off, cands, fflags, all_rules, windowable, chunk, window, lead=0):
    got = S.plan_gather_windows(off, cands, fflags, all_rules, windowable, chunk, window, lead=lead)
    cls, marks, runs, total = numpy_layout(off, cands, fflags, all_rules, windowable, chunk, window, lead)
    assert np.array_equal(got["cls"], cls), (got["cls"], cls)
    assert np.array_equal(got["marks"].astype(bool), marks)
    assert np.array_equal(got["runs"], runs) and got["total"] == total
    off = np.asarray(off, np.int64)
    r = got["runs"].astype(np.int64)
    # alignment, order, disjointness (sources and destinations), the buffer's size
    assert (r[:, 1] % 64 == 0).all() and (r[:, 0] % chunk == 0).all() and (r[:, 2] > 0).all()
    assert (r[1:, 0] > r[:-1, 0] + r[:-1, 2]).all()             # a gap of at least a chunk between runs
    assert (r[1:, 1] >= r[:-1, 1] + r[:-1, 2]).all()
    assert total % 64 == 0 and (len(r) == 0 or total >= r[-1, 1] + r[-1, 2])

    def run_of(byte):
        k = np.searchsorted(r[:, 0], byte, side="right") - 1
        return int(k) if k >= 0 and byte < r[k, 0] + r[k, 2] else NO_RUN
    before, after, _ = window
    for f in range(lead, len(off) - 1):
        n = int(off[f + 1] - off[f])
        head = int(off[f]) // chunk * chunk
        if got["cls"][f] == NONE:
            assert got["first_run"][f] == NO_RUN
            continue
        if head < int(off[-1]):
            assert got["first_run"][f] == run_of(head) != NO_RUN     # the head is present
        if got["cls"][f] == WHOLE and n:
            k = run_of(head)
            assert off[f + 1] <= r[k, 0] + r[k, 2]
    for f, _r, s in cands:
        if lead <= f < len(off) - 1 and got["cls"][f] == WINDOW:    # every candidate's span inside one run
            n = int(off[f + 1] - off[f])
            a, b = int(off[f]) + max(s - before, 0), int(off[f]) + max(min(s + after, n), s + 1)
            k = run_of(a)
            assert k != NO_RUN and b <= r[k, 0] + r[k, 2]
    return got


def test_layout_against_numpy_random():
    rng = np.random.RandomState(7)
    for trial in range(60):
        chunk = int(rng.choice([128, 256, 1024]))
        nfiles = int(rng.randint(1, 24))
        lens = rng.choice([0, 1, 57, chunk - 1, chunk, chunk + 1, 5 * chunk + 3, 40 * chunk, 200 * chunk + 77], nfiles)
        off = np.concatenate([[0], np.cumsum(lens)])
        lead = int(rng.randint(0, 2)) if nfiles > 1 else 0
        nrows = 6
        windowable = np.array([1, 1, 0, 1, 1, 0], np.uint8)
        cands = []
        for _ in range(int(rng.randint(0, 30))):
            f = int(rng.randint(0, nfiles + 1))                       # (one past the files: skipped)
            n = int(lens[f]) if f < nfiles else 10
            s = int(rng.randint(0, n + 2)) if rng.rand() < 0.9 else 0xFFFFFFFFFFFFFFFF
            r = int(rng.choice([0, 1, 3, 4, 4, 4, 2, 5, 6, 99]))
            cands.append((f, r, s))
        cands += cands[:3]                                            # duplicates, as K2 emits them
        fflags = (rng.rand(nfiles) < 0.08).astype(np.uint32)
        window = (int(rng.choice([0, 5, 100, 700])), int(rng.choice([1, 64, 300, 5000])), int(rng.choice([0, 1000, 50000])))
        check_layout(off, cands, fflags, trial % 17 == 0, windowable, chunk, window, lead)


def test_layout_of_every_corpus():
    for name in WC.NAMES:
        c = WC.corpus(name)
        sc = scanner(c.cfg)
        cands, info = S.prefilter_table_model(sc, c.args, with_info=True)
        rows, nrules = S.windowable_rows(sc)
        flat = [(f, r, int(s)) for (f, r), v in cands.items() for s in v]
        all_rules = c.name == "whole_mode1"
        got = check_layout(c.offsets, flat, info["special"].astype(np.uint32), all_rules, rows, c.chunk, c.window)
        for f, want in c.classes.items():
            assert got["cls"][f] == want, (name, f, got["cls"])


def test_windowable_rows():
    c = WC.corpus("whole_rules")
    sc = scanner(c.cfg)
    rows, nrules = S.windowable_rows(sc)
    ids = sc.rule_ids
    assert len(rows) == nrules + 1 and nrules == len(ids)             # one exclude-block pseudo-rule
    by = dict(zip(ids, rows[:nrules]))
    assert by["github-pat"] and by["private-key"] and by["w-fixed"] and by["w-az"] and by["w-bound"] and by["jwt-token"]
    assert not by["w-hostgate"] and not by["w-presence"] and not by["aws-secret-access-key"] and not rows[nrules]
    rows1, n1 = S.windowable_rows(scanner(WC.corpus("whole_mode1").cfg))
    assert not rows1[list(scanner(WC.corpus("whole_mode1").cfg).rule_ids).index("w-hex40")]


# --------------------------------------------------- the examined position
def test_examined_position_decides_not_the_match_end():
    text = b"A" + b"x" * 20 + b"Z tail"
    for sub in (False, True):
        # the cut text gives a shorter match, well inside it: only the examined position shows the cut
        end, ex = S.regex_examined("A(.*Z)?", text, 0, submatch=sub, cut=10)
        assert end == 1 and ex >= 10
        end, ex = S.regex_examined("A(.*Z)?", text, 0, submatch=sub)
        assert end == 22 and ex >= len(text)                          # greedy: it looked for a later Z
        end, ex = S.regex_examined("A(.*?Z)?", text + b"\n", 0, submatch=sub)
        assert end == 22
    tok = b"ghp_" + b"a" * 36
    for sub in (False, True):
        assert S.regex_examined("ghp_[0-9a-zA-Z]{36}", tok + b"zz", 0, submatch=sub, cut=40) == (40, 39)
        assert S.regex_examined("ghp_[0-9a-zA-Z]{36}", tok + b"zz", 0, submatch=sub, cut=39) == (-1, 39)
        # the lookahead of \b, of $ and of a rune decode counts
        assert S.regex_examined("ghp_[0-9a-zA-Z]{36}\\b", tok + b" z", 0, submatch=sub, cut=40) == (40, 40)
        assert S.regex_examined("ghp_[0-9a-zA-Z]{36}$", tok + b" z", 0, submatch=sub, cut=40) == (40, 40)
        assert S.regex_examined("ab.", "abé".encode() + b"z", 0, submatch=sub, cut=3)[1] == 3   # half a rune
        end, ex = S.regex_examined("ab.", "abé".encode() + b"z", 0, submatch=sub, cut=4)
        assert end == 4 and ex == 3
    # the lazy DFA (an unbounded pattern without captures) stops at a state that can only match
    assert S.regex_examined("x[0-9]+q", b"x123q...", 0, cut=5) == (5, 4)
    assert S.regex_examined("x[a-z]+q", b"xabcq...", 0, cut=5) == (5, 5)    # [a-z]+ may still take the q and go on
    assert S.regex_examined("x[a-z]+", b"xabc def", 0, cut=6) == (4, 4)
    assert S.regex_examined("x[a-z]+", b"xabcdef", 0, cut=4) == (4, 4)     # 4 = the cut: it asked for more


def test_examined_agrees_with_the_uncut_run():
    rng = np.random.RandomState(3)
    pats = ["ghp_[0-9a-zA-Z]{36}", "a+b*c?", "(ab|a)(bc|c)?", "x.*y", "x.*?y", "\\bfoo\\b", "(?m)^foo$", "fo+\\s+bar",
            "[^a]+a", "é+z", "a{2,5}b"]
    alphabet = [b"a", b"b", b"c", b"x", b"y", b"f", b"o", b" ", b"\n", b"r", "é".encode(), b"z", b"\xa9"]
    for _ in range(300):
        text = b"".join(alphabet[i] for i in rng.randint(0, len(alphabet), 24))
        pos = int(rng.randint(0, len(text)))
        pat = pats[int(rng.randint(0, len(pats)))]
        for sub in (False, True):
            full = S.regex_examined(pat, text, pos, submatch=sub)
            for cut in range(pos, len(text)):
                end, ex = S.regex_examined(pat, text, pos, submatch=sub, cut=cut)
                if ex < cut:                                          # sufficient: the same on the longer text
                    assert end == full[0], (pat, text, pos, cut, sub, end, ex, full)


# ------------------------------------------------------------ the model
_ORACLE = {}


def oracle(c):
    """The oracle's findings for corpus c (its config goes through a YAML file, as parse_config reads one)."""
    if c.name not in _ORACLE:
        cfg = None
        if c.cfg is not None:
            with tempfile.NamedTemporaryFile("w", suffix=".yaml") as fp:
                json.dump(c.cfg, fp)
                fp.flush()
                cfg = so.parse_config(fp.name)
        _ORACLE[c.name] = oracle_scan_many([(a.FilePath, a.Content, a.Binary) for a in c.args], procs=4, cfg=cfg)
    return _ORACLE[c.name]


@pytest.mark.parametrize("name", WC.NAMES)
def test_corpus_holds_what_it_was_built_for(name):
    c = WC.corpus(name)
    WC.holds(c, S.prefilter_table_model(scanner(c.cfg), c.args))


@pytest.mark.parametrize("name", WC.NAMES)
def test_windowed_model(name):
    c = WC.corpus(name)
    sc = scanner(c.cfg)
    want = S.scan_table_model(sc, c.args)
    assert want == oracle(c)
    got, rec, fb, st = S.scan_device_model_windows(sc, c.args, c.chunk, c.window)
    assert got == want
    assert rec["insufficient"] == c.insufficient
    for f, cls in c.classes.items():
        assert rec["cls"][f] == cls, (f, rec["cls"])
    # the record against the layout hook, the stats against the record
    cands, info = S.prefilter_table_model(sc, c.args, with_info=True)
    flat = [(f, r, int(s)) for (f, r), v in cands.items() for s in v]
    rows, _ = S.windowable_rows(sc)
    lay = S.plan_gather_windows(c.offsets, flat, info["special"].astype(np.uint32), name == "whole_mode1", rows, c.chunk,
                                c.window)
    assert np.array_equal(rec["cls"], lay["cls"]) and np.array_equal(rec["runs"], lay["runs"]) and rec["total"] == lay["total"]
    data, _off = S.pack(c.args)
    for src, dst, n in rec["runs"].astype(np.int64):
        assert np.array_equal(rec["bytes"][dst:dst + n], data[src:src + n])
    need = np.zeros(len(c.args), np.uint8)
    need[c.insufficient] = 1
    goff, runs, total = S.plan_gather(c.offsets, need, c.chunk)
    assert np.array_equal(fb["goff"], goff) and np.array_equal(fb["runs"], runs) and fb["total"] == total
    for src, dst, n in runs.astype(np.int64):
        assert np.array_equal(fb["bytes"][dst:dst + n], data[src:src + n])
    nwin = int((rec["cls"] == WINDOW).sum())
    assert st["window_files"] == nwin - len(c.insufficient) and st["window_runs"] == len(rec["runs"])
    assert st["window_bytes"] == rec["total"] and st["fallback_files"] == len(c.insufficient)
    assert st["fallback_bytes"] == total and st["gather_bytes"] == rec["total"] + total
    assert st["gather_runs"] == len(rec["runs"]) + len(runs)
    assert st["gather_files"] == int((rec["cls"] != NONE).sum())
    assert sum(len(s["Findings"]) for s in got) > 0 or name == "match_ends"


def test_windowed_model_other_chunks_and_windows():
    # the same findings whatever the chunk and the window; the fallback set may only change with them
    for name in ("positions", "censoring", "head_newlines", "runes", "fallbacks"):
        c = WC.corpus(name)
        sc = scanner(c.cfg)
        want = S.scan_table_model(sc, c.args)
        for chunk, window in ((256, (8, 40, 0)), (512, (700, 700, 0)), (1024, (3, 3, 100000)), (128, (4000, 4000, 0))):
            got, rec, fb, st = S.scan_device_model_windows(sc, c.args, chunk, window)
            assert got == want, (name, chunk, window)


def test_large_sparse_gathers_little():
    c = WC.corpus("large_sparse")
    got, rec, fb, st = S.scan_device_model_windows(scanner(c.cfg), c.args, c.chunk, c.window)
    total = int(c.offsets[-1])
    assert st["fallback_files"] == 0 and st["window_files"] == len(c.args)
    assert st["window_bytes"] == st["gather_bytes"] < total // 100          # two windows and a head per file


def test_options_off_is_the_whole_file_gather():
    c = WC.corpus("whole_builtin")
    sc = scanner(c.cfg)
    base = S.scan_device_model(sc, c.args, c.chunk, with_gather=True)
    for window in (None, (0, 0, 0), (0, 0, 4096)):
        if window is None:
            got = S.scan_device_model(sc, c.args, c.chunk, with_gather=True)
        else:
            out, rec, fb, st = S.scan_device_model_windows(sc, c.args, c.chunk, window)
            got = (out, rec, st)
            assert not rec["cls"].size and not rec["insufficient"] and not any(
                st[k] for k in ("window_files", "window_runs", "window_bytes", "fallback_files", "fallback_bytes"))
        assert got[0] == base[0]
        for k in ("need", "goff", "runs", "bytes"):
            assert np.array_equal(got[1][k], base[1][k]), k
        assert got[1]["total"] == base[1]["total"]
        for k in ("gather_files", "gather_bytes", "gather_runs"):
            assert got[2][k] == base[2][k]
