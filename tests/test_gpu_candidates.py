"""K1 + K2 on the GPU against the CPU model of the same tables, directly:
for every edge corpus of tests/_edge_corpus.py, every rule set and K1 chunk
setting,

* the candidates tsg_prefilter_resident returns equal
  tsg_prefilter_table_model's exactly -- the same (file, rule) keys, the same
  sorted starts; not a superset, nothing sampled.  (The findings tests see a
  kernel error only where a planted secret lies on it: the host confirmer is
  exact and hides every spurious candidate, and a lost one shows only under a
  secret.)
* K1's anchor-hit count equals the model's;
* K1's per-chunk newline counts equal a numpy count over the packed batch, at
  the chunk size the stats report, one entry per chunk;
* K1's per-file fold-special flag equals the model's -- but for the files of
  one corpus that share a 16-byte word with a neighbour's sequence, where K1
  flags a superset by design (see _candidate_check.check).

The conditions that make these comparisons meaningful (every probe fires,
cut probes are silent, the overflow inputs overflow, ...) are asserted on the
CPU in tests/test_candidate_corpus.py.
"""
import pytest

import _edge_corpus as EC
from _candidate_check import check as _check          # (shared with tests/test_gpu_paths.py)
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

# the default chunk policy (128-byte chunks for batches this small, a grid
# round of 1-chunk ranges), forced chunk sizes, and the kU = 8 bulk level with
# no tail rounds (every wave item 64 lanes x 8 chunks)
SETTINGS = {
    "default": {},
    "chunk128": {"TSG_K1_CHUNK": "128"},
    "chunk512": {"TSG_K1_CHUNK": "512"},
    "chunk2048": {"TSG_K1_CHUNK": "2048"},
    "top8": {"TSG_K1_TOP8": "2", "TSG_K1_TAIL_ROUNDS": "0"},
    # ... at the chunk the product runs that level with (launches of >= 2 GiB),
    # and at 4096 B: a 2 MiB wave item, the hit record's offset limit
    "top8_1024": {"TSG_K1_TOP8": "2", "TSG_K1_TAIL_ROUNDS": "0", "TSG_K1_CHUNK": "1024"},
    "top8_4096": {"TSG_K1_TOP8": "2", "TSG_K1_TAIL_ROUNDS": "0", "TSG_K1_CHUNK": "4096"},
}

_RULESETS = {}      # ruleset -> (model scanner, rule table, probes)
_CORPORA = {}       # (ruleset, group) -> corpora
_MODEL = {}         # (ruleset, corpus name) -> model result


def _ruleset(name, monkeypatch):
    cfg, env = EC.ruleset_config(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _RULESETS:
        sc = S.Scanner(cfg)
        rules = EC.rule_table(sc)
        _RULESETS[name] = (sc, rules, EC.probes(name, rules))
    return _RULESETS[name]


def _corpora(name, group, rules, pr):
    if (name, group) not in _CORPORA:
        if group == "sweep":
            _CORPORA[(name, group)] = [EC.edge_sweep(p, cut) for p in pr for cut in (False, True)]
        else:
            _CORPORA[(name, group)] = EC.small_corpora(name, rules, pr)
    return _CORPORA[(name, group)]


def _model(name, sc, corpus):
    """The CPU model's candidates of a corpus, computed once for all settings."""
    if (name, corpus.name) not in _MODEL:
        _MODEL[(name, corpus.name)] = S.prefilter_table_model(sc, corpus.args, with_info=True)
    return _MODEL[(name, corpus.name)]


def _gpu_scanner(name, setting, monkeypatch):
    """A scanner whose engine is created under the setting's environment."""
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    sc = S.Scanner(EC.ruleset_config(name)[0])
    sc.engine()
    return sc


def _run(name, setting, group, monkeypatch):
    msc, rules, pr = _ruleset(name, monkeypatch)
    corpora = _corpora(name, group, rules, pr)
    sc = _gpu_scanner(name, setting, monkeypatch)
    expect = int(SETTINGS[setting].get("TSG_K1_CHUNK", 0))
    default_pad = ((b"\n" + pr[0].text) * 4)[:64]        # behind every batch: nothing there is the batch's
    for c in corpora:
        want, winfo = _model(name, msc, c)
        got, info = S.prefilter_resident(sc, c.args, pad=c.pad or default_pad)
        _check(c, sc.rule_ids, got, info, want, winfo, expect)
    return corpora


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_edge_sweep_candidates_gpu(ruleset, setting, monkeypatch):
    corpora = _run(ruleset, setting, "sweep", monkeypatch)
    assert len(corpora) >= 8 and all(len(c.placements) == 4 * EC.SWEEP_BLOCKS for c in corpora)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_small_corpora_candidates_gpu(ruleset, setting, monkeypatch):
    # file-start clipping, batch ends, keyword-gate separation, newline and
    # fold-special edges, the reverse walk's give-up
    corpora = _run(ruleset, setting, "small", monkeypatch)
    names = {c.name.split("-")[0] for c in corpora}
    assert names == {"gate", "nlflags", "nlnear", "clip", "end", "revlimit"}


def test_overflow_regrow_candidates_gpu(monkeypatch):
    # a fresh scanner: lane capacities persist on its pooled lanes
    msc, rules, pr = _ruleset("builtin", monkeypatch)
    sc = S.Scanner(None)
    a, b = EC.overflow_hits(), EC.overflow_candidates()
    want_a, winfo_a = _model("builtin", msc, a)
    got, info = S.prefilter_resident(sc, a.args)
    # more hits than the hit regions and the overflow pool held: K1 ran again with a grown pool
    assert info["stats"]["hits"] > EC.HIT_CAP0 + EC.OVER_CAP0, info["stats"]
    _check(a, sc.rule_ids, got, info, want_a, winfo_a)
    want_b, winfo_b = _model("builtin", msc, b)
    got, info = S.prefilter_resident(sc, b.args)
    # more candidates than the candidate buffer held: K2 ran again with a grown buffer
    assert info["stats"]["candidates"] > EC.CAND_CAP0, info["stats"]
    _check(b, sc.rule_ids, got, info, want_b, winfo_b)
    # (a) again: the capacities are grown, no retry, the same sets
    got, info = S.prefilter_resident(sc, a.args)
    _check(a, sc.rule_ids, got, info, want_a, winfo_a)
