"""The comparison of raw GPU outputs with the CPU table model that
tests/test_gpu_candidates.py (one resident segment: check) and
tests/test_gpu_paths.py (every segmented path of Engine::scan: check_scan)
share."""
import numpy as np
import pytest

import _edge_corpus as EC
from trivy_amd import secret as S


def where(c, f, start, chunk):
    """Names the edges next to a candidate start, for a failure message."""
    if start == int(S.FULL_SCAN_START):
        return "start kFullScanStart"
    b = int(c.offsets[f]) + start
    return ("start %d = batch offset %d (mod chunk %d: %d, mod 64: %d, mod 4 chunks: %d, mod 8 chunks: %d, "
            "mod 64 KiB: %d; %d bytes before the file's end; batch of %d bytes)%s"
            % (start, b, chunk, b % chunk, b % 64, b % (4 * chunk), b % (8 * chunk), b % EC.BLOCK,
               int(c.offsets[f + 1]) - b, c.nbytes, located(c, b)))


def located(c, b):
    """The wave item, level and lane of a batch offset where the corpus knows
    K1's schedule (tests/_schedule_corpus.py: note["locate"])."""
    return "; " + c.note["locate"](b) if "locate" in c.note else ""


def check(c, rule_ids, got, info, want, winfo, expect_chunk=None):
    chunk = info["chunk_bytes"]
    # ---- candidates: the same keys, the same sorted starts
    for key in sorted(set(got) | set(want)):
        g = got.get(key, np.zeros(0, np.uint64))
        w = want.get(key, np.zeros(0, np.uint64))
        if np.array_equal(g, w):
            continue
        f, r = key
        missing, extra = np.setdiff1d(w, g), np.setdiff1d(g, w)
        kind, start = ("the GPU lacks", int(missing[0])) if len(missing) else ("the GPU adds", int(extra[0]))
        rid = rule_ids[r] if r < len(rule_ids) else "exclude-block #%d" % (r - len(rule_ids))
        pytest.fail("%s: %s a candidate (%d missing, %d extra in this list): file %d %s (%d bytes), rule %d %s, %s"
                    % (c.name, kind, len(missing), len(extra), f, c.args[f].FilePath, len(c.args[f].Content), r, rid,
                       where(c, f, start, chunk)))
    assert info["stats"]["hits"] == winfo["hits"], (c.name, "anchor hits", info["stats"]["hits"], winfo["hits"])
    # ---- newline counts: one per chunk of the packed batch
    assert chunk == info["stats"]["chunk_bytes"] and chunk > 0
    if expect_chunk:
        assert chunk == expect_chunk
    data, offsets = S.pack(c.args)
    total = int(offsets[-1])
    nl = info["chunk_newlines"]
    assert len(nl) == -(-total // chunk), (c.name, len(nl), total, chunk)
    # (summed as int64 without an int64 copy of the batch: the schedule corpora are hundreds of MB)
    ref = np.add.reduceat(data[:total] == 10, np.arange(0, total, chunk), dtype=np.int64) if total else np.zeros(0)
    bad = np.nonzero(nl.astype(np.int64) != ref)[0]
    assert len(bad) == 0, ("%s: newline count of chunk %d (batch offset %d, chunk %d): GPU %d, batch %d; %d chunks differ%s"
                           % (c.name, bad[0], bad[0] * chunk, chunk, nl[bad[0]], ref[bad[0]], len(bad),
                              located(c, int(bad[0]) * chunk)))
    # ---- file flags: bit 0 (engine.h kFileFoldSpecial) is the only bit K1 sets
    flags = info["flags"]
    assert len(flags) == len(c.args)
    assert not (flags & ~np.uint32(S.FILE_FOLD_SPECIAL)).any()
    gs = (flags & S.FILE_FOLD_SPECIAL) != 0
    bad = gs != winfo["special"]
    if c.note.get("flags") == "word16":
        # The one exception, by K1's design (engine.hip k1_special): a 16-byte
        # word that holds a file boundary is checked as one piece and every
        # file overlapping it is flagged -- a superset, safe because a flagged
        # file is only scanned more carefully.  So a file the model does not
        # call special may be flagged iff it shares a 16-byte word of the
        # batch with the end of a sequence; a special file is always flagged.
        words = EC.fold_special_words(data, total)
        for f in np.nonzero(bad)[0]:
            lo, hi = int(offsets[f]), int(offsets[f + 1])
            near = hi > lo and ((words * 16 < hi) & (words * 16 + 16 > lo)).any()
            if gs[f] and not winfo["special"][f] and near:
                bad[f] = False
    bad = np.nonzero(bad)[0]
    if len(bad):
        f = int(bad[0])
        pytest.fail("%s: fold-special flag of file %d %s (%d bytes at batch offset %d, mod 16: %d): GPU %d, model %d; "
                    "%d files differ" % (c.name, f, c.args[f].FilePath, len(c.args[f].Content), int(c.offsets[f]),
                                          int(c.offsets[f]) % 16, gs[f], winfo["special"][f], len(bad)))


# ------------------------------------------------- a whole Engine::scan, by segment
def seg_where(c, segs, f, start):
    """Names the segment next to a candidate of batch file f, its ring slot
    parity and the distances to the cuts, for a failure message."""
    k = max(i for i, s in enumerate(segs) if s["f0"] <= f)
    s = segs[k]
    if start == int(S.FULL_SCAN_START):
        b = int(c.offsets[f])
    else:
        b = int(c.offsets[f]) + start
    return ("segment %d of %d (ring slot %d; files %d..%d, file %d of the segment; lead of %d bytes), %d bytes after "
            "the segment's cut at batch offset %d, %d before the next at %d; mod 64 KiB of the segment: %d, mod 4096: %d"
            % (k, len(segs), k & 1, s["f0"], s["f0"] + s["nfiles"] - 1, f - s["f0"] + s["lead"], s["lead_bytes"],
               b - s["b0"], s["b0"], s["b0"] + s["bytes"] - b, s["b0"] + s["bytes"],
               (b - s["b0"] + s["lead_bytes"]) % EC.BLOCK, (b - s["b0"] + s["lead_bytes"]) % 4096))


_SEG_MODEL = {}


def segment_model(key, msc, c, data, seg):
    """The CPU model on one segment's files as a batch of their own, the lead
    (the bytes between the piece's start and its first file) as file 0:
    (candidates, info).  Cached by key + the segment's cut."""
    k = (key, c.name, seg["f0"], seg["nfiles"], seg["lead_bytes"])
    if k not in _SEG_MODEL:
        own = seg["nfiles"] - seg["lead"]
        args = list(c.args[seg["f0"]:seg["f0"] + own])
        if seg["lead"]:
            args.insert(0, S.ScanArgs("", data[seg["b0"] - seg["lead_bytes"]:seg["b0"]].tobytes()))
        _SEG_MODEL[k] = S.prefilter_table_model(msc, args, with_info=True)
    return _SEG_MODEL[k]


def check_scan(key, c, msc, rule_ids, want, winfo, want_findings, plan, findings, got, info):
    """One tsg_scan_batch / tsg_scan_batch_resident with the raw-output hook on
    (S.scan_raw) against the CPU model: want, winfo = the model of the whole
    batch (it is per file: the cuts do not enter), want_findings =
    S.scan_table_model's, plan = S.plan_segments under the engine's policy.
    Everything is exact."""
    segs = info["segments"]
    data, offsets = S.pack(c.args)
    # ---- the segment records are the planner's
    for s in plan:
        s.setdefault("own", s["nfiles"] - s["lead"])
    assert [(s["f0"], s["nfiles"], s["lead"], s["b0"], s["bytes"], s["lead_bytes"]) for s in segs] == \
           [(s["f0"], s["own"], s["lead"], s["b0"], s["bytes"], s["lead_bytes"]) for s in plan], c.name
    assert info["stats"]["pieces"] == len(plan)
    # ---- candidates of the real files: the same keys, the same sorted starts
    for key2 in sorted(set(got) | set(want)):
        g = got.get(key2, np.zeros(0, np.uint64))
        w = want.get(key2, np.zeros(0, np.uint64))
        if np.array_equal(g, w):
            continue
        f, r = key2
        missing, extra = np.setdiff1d(w, g), np.setdiff1d(g, w)
        kind, start = ("the GPU lacks", int(missing[0])) if len(missing) else ("the GPU adds", int(extra[0]))
        rid = rule_ids[r] if r < len(rule_ids) else "exclude-block #%d" % (r - len(rule_ids))
        chunk = [s for s in segs if s["f0"] <= f][-1]["chunk_bytes"]
        pytest.fail("%s: %s a candidate (%d missing, %d extra in this list): file %d %s (%d bytes), rule %d %s, %s; %s"
                    % (c.name, kind, len(missing), len(extra), f, c.args[f].FilePath, len(c.args[f].Content), r, rid,
                       where(c, f, start, chunk), seg_where(c, plan, f, start)))
    flags = info["flags"]
    assert len(flags) == len(c.args)
    assert not (flags & ~np.uint32(S.FILE_FOLD_SPECIAL)).any()
    gs = (flags & S.FILE_FOLD_SPECIAL) != 0
    noted = set(range(len(c.args))) if c.note.get("flags") == "word16" else c.note.get("word16", set())
    for k, (s, p) in enumerate(zip(segs, plan)):
        mc, mi = segment_model(key, msc, c, data, p)
        lo, hi = s["b0"] - s["lead_bytes"], s["b0"] + s["bytes"]
        tag = "%s segment %d (ring slot %d, files %d..%d, lead %d bytes)" % (c.name, k, k & 1, s["f0"],
                                                                               s["f0"] + s["nfiles"] - 1, s["lead_bytes"])
        # ---- anchor hits, the lead a file of its own
        assert s["hits"] == mi["hits"], (tag, "anchor hits: GPU, model", s["hits"], mi["hits"])
        # ---- newline counts: one per chunk, the grid from the lead's first byte
        chunk = s["chunk_bytes"]
        assert chunk > 0 and chunk % 128 == 0, tag
        nl = s["chunk_newlines"]
        assert len(nl) == -(-(hi - lo) // chunk), (tag, len(nl), hi - lo, chunk)
        ref = np.add.reduceat((data[lo:hi] == 10).astype(np.int64), np.arange(0, hi - lo, chunk))
        bad = np.nonzero(nl.astype(np.int64) != ref)[0]
        assert len(bad) == 0, ("%s: newline count of chunk %d (segment offset %d, chunk %d): GPU %d, batch %d; %d chunks "
                               "differ" % (tag, bad[0], bad[0] * chunk, chunk, nl[bad[0]], ref[bad[0]], len(bad)))
        # ---- flags: the model's; a file noted word16 may be flagged beyond it
        # iff it shares a 16-byte word -- counted from the segment's first
        # byte, inside the segment's bytes alone -- with the end of a sequence
        words = EC.fold_special_words(data[lo:hi], hi - lo)

        def near(a, b):
            return b > a and bool(((words * 16 < b - lo) & (words * 16 + 16 > a - lo)).any())
        for j in range(s["nfiles"]):
            f = s["f0"] + j
            a, b = int(offsets[f]), int(offsets[f + 1])
            ok = gs[f] == winfo["special"][f] or (f in noted and gs[f] and near(a, b))
            assert ok, ("%s: fold-special flag of file %d %s (%d bytes, %d after the cut, segment offset mod 16: %d): "
                        "GPU %d, model %d" % (tag, f, c.args[f].FilePath, b - a, a - s["b0"], (a - lo) % 16, gs[f],
                                              winfo["special"][f]))
        # ---- the lead: its flag and its candidates are the model's on its
        # bytes, recorded under the lead and (the comparison above) under no file
        if s["lead"]:
            assert not (s["lead_flags"] & ~S.FILE_FOLD_SPECIAL), tag
            lf = bool(s["lead_flags"] & S.FILE_FOLD_SPECIAL)
            assert lf == bool(mi["special"][0]) or (s["f0"] - 1 in noted and lf and near(lo, s["b0"])), \
                (tag, "lead flag: GPU, model", lf, mi["special"][0])
            wl = sorted((r, int(x)) for (f, r), v in mc.items() if f == 0 for x in v)
            assert s["lead_cands"] == wl, (tag, "lead candidates: GPU, model", s["lead_cands"][:6], wl[:6])
            assert s["lead_emitted"] >= len(wl)
        else:
            assert s["lead_bytes"] == 0 and s["lead_emitted"] == 0 and not s["lead_cands"], tag
    assert sum(s["hits"] for s in segs) == info["stats"]["hits"]
    # ---- the findings: the hook changes nothing
    assert len(findings) == len(want_findings)
    for f, (g, w) in enumerate(zip(findings, want_findings)):
        assert g == w, (c.name, "findings of file %d %s" % (f, c.args[f].FilePath))
