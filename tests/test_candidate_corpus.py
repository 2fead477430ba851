"""The edge corpora of tests/_edge_corpus.py against the CPU model of K1 + K2
(tsg_prefilter_table_model), without a GPU: the conditions that make the GPU
comparison of tests/test_gpu_candidates.py mean something.

* every probe fires its rule's anchor and (secrets, accepted decoys) yields a
  candidate; rejected decoys and probes cut by a file end yield none;
* every prefilter mode of the rule set has candidates somewhere;
* kFullScanStart appears for the long reverse prefixes and nowhere else;
* the tempting tails of the file-start corpora would produce a candidate in
  the previous file if the two files were one;
* only the keyword + anchor files of the gate corpus have candidates;
* the overflow inputs exceed a fresh lane's capacities;
* the model's fold-special flag is "the file holds one of the sequences";
* for files without them the model's candidates are tsg_scan_table_model's;
* every true match start (the oracle's regexp on the probe's surroundings) is
  in the model's set: the superset property, at the edges.
"""
import numpy as np
import pytest

import _edge_corpus as EC
from oracle import secret_oracle as so
from oracle.goregex import GoRegexp
from trivy_amd import secret as S

_STATE = {}


def _setup(ruleset, monkeypatch):
    """(scanner, rule table, probes) of a rule set; TSG_K1C is set for the
    caller's test through monkeypatch (the model reads it when it compiles)."""
    cfg, env = EC.ruleset_config(ruleset)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if ruleset not in _STATE:
        sc = S.Scanner(cfg)
        rules = EC.rule_table(sc)
        _STATE[ruleset] = (sc, rules, EC.probes(ruleset, rules))
    return _STATE[ruleset]


_MODEL = {}


def _model(ruleset, sc, corpus):
    key = (ruleset, corpus.name)
    if key not in _MODEL:
        _MODEL[key] = S.prefilter_table_model(sc, corpus.args, with_info=True)
    return _MODEL[key]


def _starts(cands, f, rule):
    return cands.get((f, rule), np.zeros(0, np.uint64))


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_rule_set_shape(ruleset, monkeypatch):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    rep = S.prefilter_report(sc)
    ngroups = int(rep.splitlines()[1].split()[0])
    if ruleset == "builtin":
        assert ngroups == 1 and "K1c one-pass table" not in rep
        assert {r["mode"] for r in rules.values()} == {0, 4}
    else:
        assert ngroups > 1
        assert ("K1c one-pass table: not used" in rep) == (ruleset == "groups"), rep[:600]
        assert rules["edge-presence"]["mode"] == 3 and rules["edge-presence"]["gate"] == "g"
        assert rules["edge-gated"]["mode"] == 0 and rules["edge-gated"]["gate"] == "g"
        assert {r["mode"] for r in rules.values()} == {0, 3, 4}
    assert {p.mode for p in pr} == {r["mode"] for r in rules.values()}
    # the filler alone: no anchor hit, no candidate, in any rule set
    cands, info = S.prefilter_table_model(sc, [S.ScanArgs("filler.txt", EC.filler(3 << 20))], with_info=True)
    assert info["hits"] == 0 and not cands


@pytest.mark.parametrize("cut", [False, True], ids=["span", "cut"])
@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_edge_sweep_model(ruleset, cut, monkeypatch):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    for p in pr:
        c = EC.edge_sweep(p, cut)
        cands, info = _model(ruleset, sc, c)
        assert len(c.placements) == 4 * EC.SWEEP_BLOCKS
        # every offset -40 .. +40 at every kind of edge
        for j, o in enumerate(EC.EDGE_OFFSETS):
            deltas = sorted(pl.anchor_at % EC.BLOCK - o for pl in c.placements[j::4])
            deltas = [d - EC.BLOCK if d > EC.BLOCK // 2 else d for d in deltas]
            assert sorted(deltas) == list(range(-40, 41)), (p.name, o)
        assert info["hits"] >= len(c.placements) or cut
        # files that may hold a candidate: a whole probe, or a head long
        # enough for the rule (Probe.min_head)
        may, cut_files = set(), set()
        for pl in c.placements:
            if pl.start is None:
                cut_files.update((pl.file, pl.file + 1))
            if pl.head >= p.min_head:
                may.add(pl.file)
        assert bool(cut_files) == cut and (cut or len(c.args) < 40)
        nwhole = 0
        for pl in c.placements:
            got = _starts(cands, pl.file, p.index)
            if pl.start is None:
                continue
            if p.kind == "reject":
                assert len(got) == 0, (p.name, pl.file)
            elif p.mode == 3:
                assert len(got) > 0, (p.name, pl.file)
            else:
                # a candidate at the probe (its match starts at most dmax bytes before the text)
                near = (got.astype(np.int64) >= pl.start - 8) & (got.astype(np.int64) <= pl.start + len(p.text))
                assert near.any(), (p.name, pl.file, pl.start, got[:8])
            nwhole += 1
        assert nwhole > 0
        # a probe cut by a file end: no candidate for its rule in the file that
        # holds its head nor in the one its rest opens
        quiet = sorted(cut_files - may)
        assert not cut or len(quiet) >= 20, (p.name, len(quiet))
        for f in quiet:
            assert len(_starts(cands, f, p.index)) == 0, (p.name, c.args[f].FilePath, _starts(cands, f, p.index)[:4])
        assert not any((v == S.FULL_SCAN_START).any() for v in cands.values()), p.name
        assert not info["special"].any()


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_small_corpora_model(ruleset, monkeypatch):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    seen_modes = set()
    by_index = {r["index"]: r for r in rules.values()}
    for c in EC.small_corpora(ruleset, rules, pr):
        cands, info = _model(ruleset, sc, c)
        assert list(info["special"]) == [EC.fold_special(a.Content) for a in c.args], c.name
        seen_modes.update(by_index[r]["mode"] for (_, r) in cands)
        full = {f for (f, r), v in cands.items() if (v == S.FULL_SCAN_START).any()}
        assert full == c.note.get("full", set()), c.name
        for p, f, start, _, _ in c.placements:
            got = _starts(cands, f, p.index)
            if start is None:                       # batch end, the walk alive at the last byte
                assert len(got) == 0, c.name
            elif p.kind == "reject":
                assert len(got) == 0, c.name
            else:
                assert len(got) > 0, (c.name, f)
                if p.mode != 3:
                    assert got.astype(np.int64).min() >= 0 and got.max() < len(c.args[f].Content), c.name
        if c.name.startswith("gate-"):
            for rule, want in c.note["both"].items():
                assert {f for (f, r) in cands if r == rule} == want, (c.name, rule)
            assert any(len(a.Content) == 0 for a in c.args)
            sizes = [len(a.Content) for a in c.args if a.Content]
            assert min(sizes) >= 8 and max(sizes) <= (160 if ruleset == "builtin" else 60)
        if c.name in ("nlflags", "nlnear"):
            assert not cands and info["special"].sum() >= (8 if c.name == "nlflags" else 100)
    assert seen_modes == {r["mode"] for r in rules.values()}
    # the tempting tails work: as one file, a candidate starts in the tail
    for p in pr:
        if p.mode == 3 or (p.mode == 0 and p.dmax == 0) or p.kind == "reject":
            continue
        j = EC.joined_file_start(p)
        cands, _ = _model(ruleset, sc, j)
        got = _starts(cands, 0, p.index).astype(np.int64)
        assert ((got >= j.note["tail_at"]) & (got < j.note["probe_at"])).any(), (p.name, got)


def test_overflow_inputs_model(monkeypatch):
    sc, rules, pr = _setup("builtin", monkeypatch)
    a = EC.overflow_hits()
    cands, info = _model("builtin", sc, a)
    assert info["hits"] > EC.HIT_CAP0 + EC.OVER_CAP0
    assert a.nbytes < 18_000_000
    assert {r for (_, r) in cands} >= {rules[k]["index"] for k in ("aws-access-key-id", "github-pat", "jwt-token")}
    b = EC.overflow_candidates()
    cands, info = _model("builtin", sc, b)
    assert info["candidates"] > EC.CAND_CAP0 and b.nbytes < 7_000_000
    assert EC.HIT_CAP0 + EC.OVER_CAP0 > info["hits"] > EC.CAND_CAP0    # (b) regrows the candidate buffer alone


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_model_equals_scan_table_model(ruleset, monkeypatch):
    # tsg_scan_table_model plans its confirmation from the same candidates,
    # except in fold-special files (the variant tables' there)
    sc, rules, pr = _setup(ruleset, monkeypatch)
    corpora = [EC.newline_flags(), EC.fold_special_neighbours(), EC.keyword_gate(ruleset, rules), EC.reverse_limit(),
               EC.file_start(pr[0])]
    for c in corpora:
        cands, info = _model(ruleset, sc, c)
        other = S.table_model_candidates(sc, c.args)
        plain = {f for f in range(len(c.args)) if not info["special"][f]}
        assert len(plain) > 3
        a = {k: v.tolist() for k, v in cands.items() if k[0] in plain}
        b = {k: v.tolist() for k, v in other.items() if k[0] in plain}
        assert a == b, c.name


def _oracle_match_starts(ref, rule_id, content):
    """Start offsets of the oracle's matches of one rule in content (the
    rule's regexp where the oracle reports a finding of the rule)."""
    found = ref.scan("probe.txt", content)
    if not any(f["RuleID"] == rule_id for f in found["Findings"]):
        return []
    rule = [r for r in ref.rules if r.id == rule_id][0]
    return [m[0] for m in rule.regex.find_all(content, GoRegexp.prepare(content))]


@pytest.mark.parametrize("ruleset", ["builtin", "k1c"])
def test_true_matches_are_candidates(ruleset, monkeypatch, tmp_path):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    path = EC.write_config(ruleset, tmp_path)
    ref = so.Scanner(so.parse_config(path) if path else None)
    checked = 0
    for p in pr:
        matched = 0
        for cut in (False, True):
            c = EC.edge_sweep(p, cut)
            cands, _ = _model(ruleset, sc, c)
            for _, f, start, _, _ in c.placements[::3]:
                if start is None:
                    continue
                content = c.args[f].Content
                lo = max(0, start - 300)
                excerpt = content[lo:start + len(p.text) + 300]
                got = _starts(cands, f, p.index)
                for s in _oracle_match_starts(ref, p.rule, excerpt):
                    matched += 1
                    if p.mode == 3:
                        assert len(got) > 0
                    else:
                        assert np.uint64(lo + s) in got, (p.name, c.args[f].FilePath, lo + s, got[:6])
        assert (matched > 0) == (p.kind == "secret"), (p.name, matched)
        checked += matched
    assert checked > 200


# ------------------------------------------------- corpora whose edges are cuts
def _cut_files(segs):
    return [s["f0"] for s in segs[1:]]


def _true_match_starts_in_model(ref, p, c, cands, placements):
    """Every match the oracle finds around a whole probe starts at a model
    candidate; returns the matches seen."""
    matched = 0
    for pl in placements:
        if pl.start is None or pl.probe is not p:
            continue
        content = c.args[pl.file].Content
        lo = max(0, pl.start - 300)
        got = _starts(cands, pl.file, p.index)
        for s in _oracle_match_starts(ref, p.rule, content[lo:pl.start + len(p.text) + 300]):
            matched += 1
            if p.mode == 3:
                assert len(got) > 0
            else:
                assert np.uint64(lo + s) in got, (c.name, p.name, c.args[pl.file].FilePath, lo + s, got[:6])
    return matched


def _check_placements(ruleset, sc, c, tmp_path):
    """What the sweeps' tests assert, for a cut corpus: whole probes fire, a
    probe cut by a file end is silent on both sides of it, true matches are
    candidates, the model's flags are the files that hold a sequence."""
    cands, info = _model(ruleset, sc, c)
    assert set(np.nonzero(info["special"])[0].tolist()) == c.note["special"], c.name
    nwhole = ncut = 0
    for pl in c.placements:
        p = pl.probe
        got = _starts(cands, pl.file, p.index).astype(np.int64)
        if pl.start is not None:
            assert p.kind == "secret"
            near = (got >= pl.start - 8) & (got <= pl.start + len(p.text))
            assert near.any() if p.mode != 3 else len(got) > 0, (c.name, p.name, pl.file, pl.start, got[:8])
            nwhole += 1
        else:
            # the head ends the file, the rest opens the next one: no candidate of the rule in either piece
            assert pl.head < p.min_head
            n = len(c.args[pl.file].Content)
            assert not ((got >= n - pl.head - 8) & (got < n)).any(), (c.name, p.name, pl.file, got[-4:])
            nxt = _starts(cands, pl.file + 1, p.index).astype(np.int64)
            assert not ((nxt >= 0) & (nxt < len(p.text) - pl.head + 8)).any(), (c.name, p.name, pl.file + 1, nxt[:4])
            ncut += 1
    assert nwhole >= 6 and ncut >= 4, (c.name, nwhole, ncut)
    assert not any((v == S.FULL_SCAN_START).any() for v in cands.values()), c.name
    if ruleset != "groups":
        path = EC.write_config(ruleset, tmp_path)
        ref = so.Scanner(so.parse_config(path) if path else None)
        for p in {pl.probe for pl in c.placements}:
            assert _true_match_starts_in_model(ref, p, c, cands, c.placements) > 0, (c.name, p.name)
    return cands, info


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_cuts_sparse_corpus(ruleset, monkeypatch, tmp_path):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    c = EC.cuts_sparse(pr)
    kinds = [k[0] for k in EC.cut_kinds(pr)]
    n = len(c.args)
    # at most 8 files per MB: not dense, so balanced cuts and wire packing
    assert n * 1e9 <= 8000.0 * c.nbytes and n * 1e6 <= 8 * c.nbytes and c.nbytes >= 4 * EC.WIRE_STRIP
    # SPARSE_UPLOAD: every file boundary is a cut, and every kind lies on one
    up = EC.plan(c, **EC.SPARSE_UPLOAD)
    assert _cut_files(up) == list(range(1, n))
    assert sorted(c.note["kind_at"][f] for f in _cut_files(up)) == sorted(kinds)
    assert len(set(kinds)) == 16
    # both anchor directions across cuts, whole and cut
    fwd, rev = pr[0], [p for p in pr if p.name == "jwt"][0]
    assert fwd.mode == 0 and rev.mode == 4
    for p in (fwd, rev):
        assert {"whole-%s" % p.name, "alive-%s" % p.name, "inside-anchor-%s" % p.name} <= {k.split("+")[0] for k in kinds}
    # SPARSE_WIRE: every other boundary; the builder's strip grid is the plan's
    wire = EC.plan(c, **EC.SPARSE_WIRE)
    assert [s["b0"] for s in wire] == c.note["wire_starts"] and _cut_files(wire) == list(range(2, n, 2))
    assert wire[-1]["bytes"] % EC.WIRE_STRIP == 5 and wire[-1]["bytes"] > EC.WIRE_STRIP
    data, offsets = S.pack(c.args)
    bounds = set(int(o) for o in offsets)
    seen = {"strip": set(), "block": set()}
    anchors = {}
    for pl in c.placements:
        if pl.start is not None:
            anchors.setdefault(pl.anchor_at, pl.probe.name)
    for s in wire:
        for e in range(s["b0"] + EC.WIRE_BLOCK, s["b0"] + s["bytes"] - 64, EC.WIRE_BLOCK):
            edge = "strip" if (e - s["b0"]) % EC.WIRE_STRIP == 0 else "block"
            assert e not in bounds
            if data[e - 1] == 10 and data[e] == 10:
                seen[edge].add("nl")
            if data[e - 1:e + 2].tobytes() == EC.FOLD_SPECIAL[2]:
                seen[edge].add("seq")
            for d in range(-20, 21):
                if e + d in anchors:
                    seen[edge].add(anchors[e + d])
    assert seen["strip"] >= {"nl", "seq", fwd.name, rev.name}, seen
    assert seen["block"] >= {"nl", "seq", fwd.name, rev.name}, seen
    # one byte >= 0x80 alone in its 4096-byte block of the segment, ASCII blocks around it
    h = c.note["high"]
    s = [s for s in wire if s["b0"] <= h < s["b0"] + s["bytes"]][0]
    b = s["b0"] + (h - s["b0"]) // EC.WIRE_BLOCK * EC.WIRE_BLOCK
    assert (data[b:b + EC.WIRE_BLOCK] >= 0x80).sum() == 1 and data[h] >= 0x80
    assert not (data[b - EC.WIRE_BLOCK:b] >= 0x80).any() and not (data[b + EC.WIRE_BLOCK:b + 2 * EC.WIRE_BLOCK] >= 0x80).any()
    # a split sequence makes neither file special; the word16 files are its neighbours and the near ones'
    cands, info = _check_placements(ruleset, sc, c, tmp_path)
    plain_split = 0
    for f, k in c.note["kind_at"].items():
        if k.startswith("split"):
            # (the model's flags are "the file holds a whole sequence": _check_placements)
            seq, n = EC.FOLD_SPECIAL[int(k[5])], int(k[7])
            assert c.args[f - 1].Content.endswith(seq[:n]) and c.args[f].Content.startswith(seq[n:])
            assert {f - 1, f} <= c.note["word16"]
            plain_split += not info["special"][f - 1] and not info["special"][f]
        if "near" in k:
            assert info["special"][f - 1] or info["special"][f]
            assert {f - 1, f} <= c.note["word16"]
    assert plain_split >= 3


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_cuts_resident_corpus(ruleset, monkeypatch, tmp_path):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    c = EC.cuts_resident(pr)
    cands, info = _check_placements(ruleset, sc, c, tmp_path)
    whole_in_lead = head_in_lead = 0
    for pieces in EC.RESIDENT_PIECES:
        leads = set()
        for base in EC.RESIDENT_BASES:
            assert base % 16 == 0
            segs = EC.plan(c, resident=True, base=base, pieces=pieces, min_piece=1)
            assert len(segs) == pieces and set(_cut_files(segs)) <= set(EC.RESIDENT_CUTS)
            for s in segs[1:]:
                assert c.note["kind_at"][s["f0"]] == EC.RESIDENT_CUTS[s["f0"]][0]
                assert s["lead_bytes"] == (base + s["b0"]) % 256 and s["lead"] == (s["lead_bytes"] > 0)
                leads.add(s["lead_bytes"])
                prev = c.args[s["f0"] - 1].Content
                lead = prev[len(prev) - s["lead_bytes"]:] if s["lead_bytes"] else b""
                for pl in c.placements:
                    if pl.file != s["f0"] - 1:
                        continue
                    if pl.start is not None and pl.start >= len(prev) - s["lead_bytes"]:
                        # a whole probe in the lead: the lead alone yields its candidate (the
                        # engine must drop it), and the previous file holds it once
                        lc = S.prefilter_table_model(sc, [S.ScanArgs("", lead)])
                        assert len(lc.get((0, pl.probe.index), ())) > 0
                        got = _starts(cands, pl.file, pl.probe.index).astype(np.int64)
                        assert ((got >= pl.start - 8) & (got <= pl.start + len(pl.probe.text))).sum() >= 1
                        whole_in_lead += 1
                    if pl.start is None and pl.head <= s["lead_bytes"]:
                        head_in_lead += 1
        assert leads >= {0, 1, 15, 16, 17, 255}, (pieces, sorted(leads))
    assert whole_in_lead >= 2 and head_in_lead >= 2


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_cuts_dense_corpus(ruleset, monkeypatch):
    sc, rules, pr = _setup(ruleset, monkeypatch)
    c = EC.cuts_dense(ruleset, rules)
    sizes = [len(a.Content) for a in c.args]
    assert len(c.args) * 1e9 > 8000.0 * c.nbytes                      # dense: the geometric tail
    segs = EC.plan(c, **EC.DENSE_UPLOAD)
    assert [s["bytes"] for s in segs] == [131072] * 4 + [65536, 32768, 16384, 16384]
    kinds = c.note["kinds"]
    for s in segs:
        last = s["f0"] + s["nfiles"] - 1
        # a run of empty files opens every segment but the first, one lies before every segment's last file
        assert s["f0"] == 0 or (sizes[s["f0"]] == 0 and sizes[s["f0"] - 1] > 0)
        assert sizes[last] > 0 and sizes[last - 1] == 0 and sizes[last - 2] == 0
    # file j of segment k holds a keyword or a sequence => file j of segments
    # k + 1 and k + 2 holds neither (k + 2: the same ring slot, the same lane)
    pairs = {}
    for k, s in enumerate(segs):
        for j in range(s["nfiles"]):
            kind = kinds[s["f0"] + j]
            if kind not in ("keyword", "both", "special"):
                continue
            for later in segs[k + 1:k + 3]:
                if j < later["nfiles"]:
                    other = kinds[later["f0"] + j]
                    assert other in ("anchor", "plain", "empty"), (k, j, kind, other)
                    key = (kind, other, later is not segs[k + 1])
                    pairs[key] = pairs.get(key, 0) + 1
    for kind, other in (("keyword", "anchor"), ("both", "anchor"), ("special", "plain")):
        assert pairs.get((kind, other, False), 0) >= 20 and pairs.get((kind, other, True), 0) >= 20, pairs
    cands, info = _model(ruleset, sc, c)
    for rule, want in c.note["both"].items():
        assert {f for (f, r) in cands if r == rule} == want and len(want) > 50, (c.name, rule)
    assert set(np.nonzero(info["special"])[0].tolist()) == c.note["special"] and len(c.note["special"]) > 50


def test_cuts_lane_state_corpus(monkeypatch):
    sc, rules, pr = _setup("builtin", monkeypatch)
    c = EC.cuts_lane_state()
    up = EC.plan(c, **EC.LANE_UPLOAD)
    res = EC.plan(c, resident=True, **EC.LANE_RESIDENT)
    assert 8_000_000 < c.nbytes < 9_000_000
    for segs in (up, res):
        assert [(s["f0"], s["nfiles"], s["bytes"]) for s in segs] == [(i, 1, EC.LANE_FILE) for i in range(4)]
    hits = []
    want = {rules[k]["index"] for k in ("aws-access-key-id", "github-pat", "jwt-token")}
    for a in c.args:
        cands, info = S.prefilter_table_model(sc, [a], with_info=True)
        hits.append(info["hits"])
        assert {r for (_, r) in cands} >= want          # the probes fire in every segment
    # K2's grid (engine.hip): seg_hand_off leaves k2_maxr_per_byte = 1.25 *
    # maxr / total, maxr the fullest hit region of the segment; seg_launch_k2
    # sizes the next segment's grid as nsub = ceil(maxr_est / 256) workgroups
    # of 256 threads per region (one hit per thread), maxr_est =
    # k2_maxr_per_byte * total + 1.  A sparse segment's fullest region holds at
    # most all its hits and the segments are of one size, so a dense one after
    # it gets nsub <= ceil((1.25 * sparse + 1) / 256), a grid that covers
    # 256 * nsub hits of a region in one pass.  Its fullest region holds at
    # least dense / regions hits, regions <= 256 (one K1 workgroup per CU, one
    # scan-DFA group for the builtin rules): the grid sized from the
    # predecessor is too small by a factor of at least 2.
    for i in c.note["dense"]:
        nsub = -(-int(1.25 * hits[i - 1] + 1) // 256)
        assert nsub == 1 and hits[i] / 256 > 2 * 256 * nsub, (hits, nsub)
        assert hits[i] > 256 * 256 * nsub                    # (the issue's form: 256 hits per region times the estimate)
