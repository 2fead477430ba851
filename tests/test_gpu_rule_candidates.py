"""K1 + K2 on the GPU against the CPU model of the same tables for EVERY rule:
the corpora of tests/_rule_corpus.py -- a file end at every byte of two or
more probes of every rule-table row (the exclude-block pseudo-rules included),
every probe's anchor at every phase of a 16-byte word and every byte of its
literal behind a 2 KiB edge, the keyword-gate triples -- through
tsg_prefilter_resident for every rule set and the default, 2 KiB-chunk and
kU = 8 settings of tests/test_gpu_candidates.py.  Candidates, anchor hits,
newline counts and file flags equal tsg_prefilter_table_model's exactly
(tests/_candidate_check.py check), not as a superset.

tests/test_gpu_candidates.py pins the same outputs at many more edges, but for
six rules (four in the custom sets), all of mode 0 with the offset window
[0,4], or of mode 3 / 4.  Which lines of tsg_k2_verify a hit runs is decided by
its own K2Anchor record; here every record has hits, whole and cut by a file
end or start at every byte.

test_upload_rule_file_ends_gpu runs the builtin set's file-end corpus through a
whole Engine::scan (tsg_scan_batch, the engine's default policy, the raw-output
hook on) and compares per segment and the findings
(tests/_candidate_check.py check_scan, as tests/test_gpu_paths.py does): tens
of thousands of tiny files, a dense batch.

The conditions that make the comparison mean something are asserted on the CPU
in tests/test_rule_corpus.py.  Measured there:

  builtin  87 rows, 191 probes: mode 0 x 84, mode 4 x 3; offset windows of the
           mode-0 rows [0,0] x 52, [0,4] x 13, [1,1] x 5, [2,2] x 3, [3,3] x 2,
           [0,1] x 2, [5,11] x 2, [4,4], [10,10], [14,14], [17,17], [18,60];
           17 rows with a verify limit of 25 .. 57, the others 64; gates g x 80,
           h x 7
           rule-ends    23 982 files, 3 015 937 bytes, 4 103 true matches
           rule-phases  22 files, 2 134 386 bytes, 4 096 true matches
           rule-gates   180 files, 4 977 bytes, 30 true matches (5 rules)
  k1c      197 rows, 411 probes: mode 0 x 192, mode 4 x 4, mode 3 x 1; gates
           g x 172, a x 18, h x 7; 8 exclude-block rows ([0,0] x 5, [4,4],
           [10,10], reverse [5,inf])
           rule-ends    45 986 files, 5 442 289 bytes, 8 328 true matches + 347 of block regexes
           rule-phases  49 files, 4 809 072 bytes, 8 482 true matches + 311 of block regexes
           rule-gates   252 files, 6 195 bytes, 42 true matches (7 rules)
  groups   the k1c rules and corpora, one K1 launch per scan-DFA group
"""
import pytest

import _edge_corpus as EC
import _rule_corpus as RC
import test_gpu_candidates as GC
from _candidate_check import check, check_scan
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

SETTINGS = ("default", "chunk2048", "top8")

_RULESETS = {}      # ruleset -> (model scanner, rule table, probes, corpora)


def _ruleset(name, monkeypatch):
    cfg, env = EC.ruleset_config(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _RULESETS:
        sc = S.Scanner(cfg)
        rules = RC.rule_table(sc)
        pr = RC.rule_probes(name, rules)
        _RULESETS[name] = (sc, rules, pr, RC.corpora(name, pr, rules))
    return _RULESETS[name]


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_rule_corpora_candidates_gpu(ruleset, setting, monkeypatch):
    msc, rules, pr, corpora = _ruleset(ruleset, monkeypatch)
    assert [c.name for c in corpora] == ["rule-%s-%s" % (k, ruleset) for k in ("ends", "phases", "gates")]
    assert {p.rule for p in pr} == {rid for rid, r in rules.items() if r["mode"] in RC.MODES}
    sc = GC._gpu_scanner(ruleset, setting, monkeypatch)
    expect = int(GC.SETTINGS[setting].get("TSG_K1_CHUNK", 0))
    pad = ((b"\n" + pr[0].text) * 4)[:64]            # behind every batch: nothing there is the batch's
    for c in corpora:
        want, winfo = GC._model(ruleset, msc, c)     # once per (rule set, corpus), shared by the settings
        got, info = S.prefilter_resident(sc, c.args, pad=pad)
        check(c, sc.rule_ids, got, info, want, winfo, expect)
        assert info["stats"]["hits"] >= len(c.placements)


def test_upload_rule_file_ends_gpu(monkeypatch):
    msc, rules, pr, corpora = _ruleset("builtin", monkeypatch)
    c = corpora[0]
    assert len(c.args) * 1e9 > 8000.0 * c.nbytes                      # dense
    want, winfo = GC._model("builtin", msc, c)
    want_findings = S.scan_table_model(msc, c.args)
    sc = S.Scanner(None)
    sc.engine()
    plan = EC.plan(c)
    findings, got, info = S.scan_raw(sc, c.args)
    check_scan("builtin", c, msc, sc.rule_ids, want, winfo, want_findings, plan, findings, got, info)
    assert sum(1 for f in findings if f["Findings"]) > 3000
