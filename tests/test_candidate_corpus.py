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
