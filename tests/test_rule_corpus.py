"""The per-rule corpora of tests/_rule_corpus.py against the CPU model of
K1 + K2 (tsg_prefilter_table_model) and the oracle, without a GPU: the
conditions that make the GPU comparison of tests/test_gpu_rule_candidates.py
mean something.

* every row of the rule table of mode 0, 3 or 4 -- the exclude-block
  pseudo-rules included -- has a probe that yields a candidate of that row;
* every anchor literal of the prefilter report occurs in a probe of its rule;
* every (mode, gate, dmin, dmax) class and every verify limit of the table is
  reached by a firing probe;
* every true match (the oracle's regexp, in every file of every corpus in which
  the oracle reports the rule; the exclude-block regexes in every file) starts
  at a model candidate;
* the file end of rule_file_ends() matters: for (nearly) every probe of mode 0
  or 4 some cut removes a candidate the joined file has.

Measured (MEASURED below holds the figures asserted, rounded down):

  builtin  87 rows, 191 probes (2 per rule; 9 each for the two aws rules of 9
           literals, 3 or 4 for three more rules of several literals, 1 where
           the samples are one string)
           rule-ends    23 982 files, 3 015 937 bytes; 4 103 true matches of 87 rules
           rule-phases  22 files, 2 134 386 bytes (1 041 edge + 3 056 phase
                        placements); 4 096 true matches of 87 rules
           rule-gates   180 files, 4 977 bytes; 30 true matches of 5 rules
           every one of the 191 probes is tempted by a cut behind its anchor
           (the verify walk has to stop at the file's end), 58 also by a cut
           before it (the window or reverse walk has to stop at the file's start)
  k1c      197 rows (192 mode 0, 4 mode 4, 1 mode 3; gates 172 g, 18 a, 7 h), 411 probes
           rule-ends    45 986 files, 5 442 289 bytes; 8 328 true matches of
                        187 rules + 347 of exclude-block regexes
           rule-phases  49 files, 4 809 072 bytes (2 347 edge + 6 576 phase
                        placements); 8 482 true matches of 187 rules + 311
           rule-gates   252 files, 6 195 bytes; 42 true matches of 7 rules
           409 of 409 probes of mode 0 / 4 tempted behind the anchor, 99 before it

The rules per class are asserted in test_every_k2_class_is_reached.  The whole
module takes about 25 s.
"""
import collections

import numpy as np
import pytest

import _edge_corpus as EC
import _rule_corpus as RC
from oracle import secret_oracle as so
from oracle.goregex import GoRegexp
from trivy_amd import secret as S

RULESETS = ("builtin", "k1c")

# exclude-block rows the sampler cannot serve: {row id: reason}.  (None: every
# configured block regex yields validated samples whose anchor fires.)
EXCUSED = {}

# what the soundness test found, rounded down: true matches of real rules,
# rules among them, matches of exclude-block regexes, per corpus
MEASURED = {
    "builtin": {"rule-ends": (4000, 87, 0), "rule-phases": (4000, 87, 0), "rule-gates": (30, 5, 0)},
    "k1c": {"rule-ends": (8000, 187, 300), "rule-phases": (8000, 187, 300), "rule-gates": (40, 7, 0)},
}

_STATE = {}
_MODEL = {}


def _setup(ruleset):
    if ruleset not in _STATE:
        sc = S.Scanner(EC.ruleset_config(ruleset)[0])
        rules = RC.rule_table(sc)
        pr = RC.rule_probes(ruleset, rules)
        _STATE[ruleset] = (sc, rules, pr, RC.corpora(ruleset, pr, rules))
    return _STATE[ruleset]


def _model(ruleset, sc, corpus):
    key = (ruleset, corpus.name)
    if key not in _MODEL:
        _MODEL[key] = S.prefilter_table_model(sc, corpus.args, with_info=True)
    return _MODEL[key]


def _starts(cands, f, rule):
    return cands.get((f, rule), np.zeros(0, np.uint64))


def _rows(rules):
    return {rid: r for rid, r in rules.items() if r["mode"] in RC.MODES}


def _firing(ruleset):
    """{row id: probes placed whole in rule_phases() with a candidate of the
    row at them (mode 3: in their file)}."""
    sc, rules, pr, corpora = _setup(ruleset)
    c = corpora[1]
    cands, info = _model(ruleset, sc, c)
    assert info["hits"] >= len(c.placements)          # every placement's anchor fires
    out = collections.defaultdict(set)
    for pl in c.placements:
        p = pl.probe
        assert pl.start is not None, (c.name, p.name)
        got = _starts(cands, pl.file, p.index).astype(np.int64)
        lo = pl.start - (0 if p.mode == 0 else 8)
        if len(got) and (p.mode == 3 or ((got >= lo) & (got <= pl.start + len(p.text))).any()):
            out[p.rule].add(p.name)
    return out


@pytest.mark.parametrize("ruleset", RULESETS)
def test_rule_table_shape(ruleset):
    sc, rules, pr, corpora = _setup(ruleset)
    rows = _rows(rules)
    modes = collections.Counter(r["mode"] for r in rows.values())
    gates = collections.Counter(r["gate"] for r in rows.values())
    if ruleset == "builtin":
        assert len(rules) == len(rows) == 87 and modes == {0: 84, 4: 3}
        assert [c.name.rsplit("-", 1)[0] for c in corpora] == ["rule-ends", "rule-phases", "rule-gates"]
    else:
        assert len(rules) == len(rows) == 197 and modes == {0: 192, 4: 4, 3: 1}
        assert gates == {"g": 172, "a": 18, "h": 7}
        blocks = [rid for rid in rules if rid.startswith("exclude-block #")]
        assert len(blocks) == 8 == len(RC.exclude_patterns(EC.ruleset_config(ruleset)[0]))
        assert all(rules[b]["gate"] == "a" for b in blocks)
    # deterministic: a second build gives the same probes
    again = RC.rule_probes(ruleset, rules)
    assert [(p.name, p.text) for p in again] == [(p.name, p.text) for p in pr]
    # every probe is what the oracle's regexp of its rule (or block) matches
    rx = {}
    for p in pr:
        if p.pattern not in rx:
            rx[p.pattern] = GoRegexp(p.pattern)
        assert rx[p.pattern].find_all(p.text), p.name
        assert b"\n" not in p.text and (p.keyword is None or p.text == p.base + b" " + p.keyword.encode())
    for c in corpora:
        assert c.nbytes < 6_000_000, c.name


@pytest.mark.parametrize("ruleset", RULESETS)
def test_every_rule_fires(ruleset):
    sc, rules, pr, corpora = _setup(ruleset)
    firing = _firing(ruleset)
    silent = sorted(set(_rows(rules)) - set(firing))
    # no real rule may be left out; at most two exclude-block rows, each named in EXCUSED
    assert silent == sorted(EXCUSED), silent
    assert len(EXCUSED) <= 2 and all(rid.startswith("exclude-block #") for rid in EXCUSED)
    # ... and in rule_file_ends(): the whole probe (h = len) has its candidate in file A
    c = corpora[0]
    cands, info = _model(ruleset, sc, c)
    whole = {pl.probe.rule for pl in c.placements
             if pl.start is not None and len(_starts(cands, pl.file, pl.probe.index))}
    assert sorted(set(_rows(rules)) - whole) == sorted(EXCUSED)


@pytest.mark.parametrize("ruleset", RULESETS)
def test_every_literal_fires(ruleset):
    sc, rules, pr, corpora = _setup(ruleset)
    nlit = 0
    for rid, r in _rows(rules).items():
        assert r["variants"], rid
        held = set().union(*[p.literals for p in pr if p.rule == rid])
        assert held == set(range(len(r["variants"]))), (rid, [sorted(v) for k, v in enumerate(r["variants"])
                                                                if k not in held])
        nlit += len(r["variants"])
    assert nlit == (112 if ruleset == "builtin" else 222)          # the report's "anchor literals"
    if ruleset == "builtin":
        # the three literals of aws-secret-access-key that no stored sample holds
        extra = [p for p in pr if p.text in RC.AWS_SECRET_EXTRA]
        assert len(extra) == 3 and all(p.rule == "aws-secret-access-key" for p in extra)


@pytest.mark.parametrize("ruleset", RULESETS)
def test_every_k2_class_is_reached(ruleset):
    sc, rules, pr, corpora = _setup(ruleset)
    firing = _firing(ruleset)
    rows = {rid: r for rid, r in _rows(rules).items() if rid not in EXCUSED}
    want = collections.Counter(RC.k2_class(r) for r in rows.values())
    got = collections.Counter(RC.k2_class(rules[rid]) for rid in firing)
    assert got == want
    assert {rules[rid]["limit"] for rid in firing} == {r["limit"] for r in rows.values()}
    if ruleset == "builtin":
        windows = collections.Counter((r["dmin"], r["dmax"]) for r in rows.values() if r["mode"] == 0)
        assert windows == {(0, 0): 52, (0, 4): 13, (1, 1): 5, (2, 2): 3, (3, 3): 2, (4, 4): 1, (10, 10): 1, (14, 14): 1,
                           (17, 17): 1, (0, 1): 2, (5, 11): 2, (18, 60): 1}
        assert sum(1 for r in rows.values() if r["limit"] < 64) == 17
        assert min(r["limit"] for r in rows.values()) == 25
        # seven host-gated rules: five of mode 0, the two lob rules of mode 4
        assert collections.Counter(r["mode"] for r in rows.values() if r["gate"] == "h") == {0: 5, 4: 2}
    else:
        blocks = [r for rid, r in rows.items() if rid.startswith("exclude-block #")]
        assert sorted((r["mode"], r["dmin"], r["dmax"]) for r in blocks) == \
            [(0, 0, 0)] * 5 + [(0, 4, 4), (0, 10, 10), (4, 5, None)]


@pytest.mark.parametrize("ruleset", RULESETS)
def test_gate_corpus(ruleset):
    sc, rules, pr, corpora = _setup(ruleset)
    gated = RC.gate_rules(pr, rules)
    assert len(gated) == (5 if ruleset == "builtin" else 7)
    c = corpora[2]
    cands, info = _model(ruleset, sc, c)
    assert any(len(a.Content) == 0 for a in c.args)
    for p in gated:
        # the anchor fires without the keyword (a hit in the model of the sample alone), the gate holds it back
        alone, ainfo = S.prefilter_table_model(sc, [S.ScanArgs("a.txt", b"\n" + p.base + b"\n")], with_info=True)
        assert ainfo["hits"] > 0 and not any(r == p.index for (_, r) in alone), p.name
        assert {f for (f, r) in cands if r == p.index} == c.note["both"][p.index], p.name


def _check_true_matches(ruleset, sc, ref, rules, c, cands):
    """Every match the oracle's regexps find in a file of c starts at a model
    candidate: (matches of real rules, the rules, matches of block regexes)."""
    index = {rid: r["index"] for rid, r in rules.items()}
    by_id = {r.id: r for r in ref.rules}
    full = int(S.FULL_SCAN_START)
    nmatch, seen, nblock = 0, set(), 0
    blocks = [(len(sc.rule_ids) + k, GoRegexp(pat), rules["exclude-block #%d" % k])
              for k, pat in enumerate(RC.exclude_patterns(EC.ruleset_config(ruleset)[0]))]

    def covered(f, row, info, start):
        got = set(_starts(cands, f, row).tolist())
        return bool(got) if info["mode"] == 3 else (start in got or full in got)
    for f, a in enumerate(c.args):
        if not a.Content:
            continue
        found = ref.scan(a.FilePath, a.Content)
        prepared = None
        for rid in sorted({x["RuleID"] for x in found["Findings"]}):
            prepared = prepared or GoRegexp.prepare(a.Content)
            for m in by_id[rid].regex.find_all(a.Content, prepared):
                assert covered(f, index[rid], rules[rid], m[0]), (c.name, a.FilePath, rid, m[0])
                nmatch += 1
                seen.add(rid)
        for row, rx, info in blocks:
            if info["mode"] not in RC.MODES:
                continue
            for m in rx.find_all(a.Content):
                assert covered(f, row, info, m[0]), (c.name, a.FilePath, "exclude-block", row, m[0])
                nblock += 1
    return nmatch, seen, nblock


@pytest.mark.parametrize("ruleset", RULESETS)
def test_true_matches_are_candidates(ruleset, tmp_path):
    sc, rules, pr, corpora = _setup(ruleset)
    path = EC.write_config(ruleset, tmp_path)
    ref = so.Scanner(so.parse_config(path) if path else None)
    for c in corpora:
        cands, _ = _model(ruleset, sc, c)
        nmatch, seen, nblock = _check_true_matches(ruleset, sc, ref, rules, c, cands)
        print("%s: %d files, %d bytes: %d true matches of %d rules, %d of exclude-block regexes"
              % (c.name, len(c.args), c.nbytes, nmatch, len(seen), nblock))
        want = MEASURED[ruleset][c.name.rsplit("-", 1)[0]]
        assert nmatch >= want[0] and len(seen) >= want[1] and nblock >= want[2], (c.name, want)


@pytest.mark.parametrize("ruleset", RULESETS)
def test_the_cut_matters(ruleset):
    # The joined file A + B holds the whole probe, so the model has its
    # candidate there, starting in A's part.  The cut tempts a kernel only if
    # it takes that candidate away: file A must not hold it (a verify walk
    # that ran past A's end would), and no candidate of B may lie before B's
    # start or of A past A's end (a window or reverse walk not clipped would
    # put one there).  For every probe of mode 0 or 4 some h must do so.
    sc, rules, pr, corpora = _setup(ruleset)
    c = corpora[0]
    j = RC.rule_file_ends(pr, "rule-ends-%s" % ruleset, joined=True)
    cands, _ = _model(ruleset, sc, c)
    jc, _ = _model(ruleset, sc, j)
    full = int(S.FULL_SCAN_START)
    assert len(j.args) == len(c.note["pairs"]) and len(c.args) == 2 * len(j.args) + RC.CLIPPED_STARTS * len(pr)
    fwd, back, probes = set(), set(), [k for k, p in enumerate(pr) if p.mode in (0, 4)]
    for n, (k, h, fa) in enumerate(c.note["pairs"]):
        p = pr[k]
        if p.mode not in (0, 4) or h == len(p.text):
            continue
        na, nb = len(c.args[fa].Content), len(c.args[fa + 1].Content)
        assert j.args[n].Content == c.args[fa].Content + c.args[fa + 1].Content
        in_a = {s for s in _starts(jc, n, p.index).tolist() if s < na}
        a = set(_starts(cands, fa, p.index).tolist())
        b = set(_starts(cands, fa + 1, p.index).tolist())
        assert all(s < na or s == full for s in a) and all(s < nb or s == full for s in b), (p.name, h)
        if full in a or not in_a - a:
            continue
        if h > p.anchor_end:
            fwd.add(k)             # the anchor fires in A: the verify walk has to stop at A's end
        if h <= p.anchor_end + 1 - p.lit_len:
            back.add(k)            # the anchor lies in B: the window / reverse walk has to stop at B's start
    failed = [pr[k].name for k in probes if k not in fwd | back]
    print("%s: %d of %d probes of mode 0 / 4 are not tempted by any cut: %s; %d by a walk past A's end, %d by a "
          "start before B's" % (c.name, len(failed), len(probes), failed, len(fwd), len(back)))
    assert len(failed) * 20 <= len(probes), failed
    assert len(fwd) * 2 >= len(probes) and len(back) >= (30 if ruleset == "builtin" else 40)
