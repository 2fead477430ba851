"""The raw GPU outputs of a real Engine::scan -- tsg_scan_batch and
tsg_scan_batch_resident with the raw-output hook on (tsg_test_keep_raw,
S.scan_raw) -- against the CPU table model, on every path that feeds K1:

* the two-slot upload ring under balanced cuts and on the geometric tail, with
  one and with two drivers pulling the segments;
* strips restored by the wire unpack (forced, racing the link, no packers);
* a small pinned batch the segment prologue copies itself (direct stage), the
  data 0, 8 and 1 bytes into its allocation, and the same batch from pageable
  memory through the copy engine;
* resident pieces behind leads of 0 .. 255 bytes, one and two drivers, every
  K1 chain mode;
* a lane whose capacities and K2 grid estimate a dense or a sparse predecessor
  left;
* two scans at once on one engine.

tests/test_gpu_candidates.py compares the same outputs of one device-resident
segment on a fresh lane; the product never runs that way.  Here the corpora's
edges are the cuts (tests/_edge_corpus.py cuts_*; their conditions are asserted
on the CPU in tests/test_candidate_corpus.py) and the comparison is per segment
(tests/_candidate_check.py check_scan): candidates per (file, rule), anchor
hits, newline counts per chunk, file flags, what K2 emitted for a lead, the
segment records against the planner, the findings.  Everything is exact.
"""
import threading

import pytest

import _edge_corpus as EC
from _candidate_check import check_scan
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

_RULESETS = {}      # ruleset -> (model scanner, rule table, probes)
_CORPORA = {}       # (ruleset, builder) -> corpus / corpora
_EXPECT = {}        # (ruleset, corpus name) -> (model candidates, model info, model findings)


def _ruleset(name, monkeypatch):
    cfg, env = EC.ruleset_config(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _RULESETS:
        sc = S.Scanner(cfg)
        rules = EC.rule_table(sc)
        _RULESETS[name] = (sc, rules, EC.probes(name, rules))
    return _RULESETS[name]


def _corpus(name, what, monkeypatch):
    """A corpus (or the list of the small ones / the sweeps), built once."""
    msc, rules, pr = _ruleset(name, monkeypatch)
    if (name, what) not in _CORPORA:
        if what == "small":
            c = EC.small_corpora(name, rules, pr)
        elif what == "sweep":
            c = [EC.edge_sweep(p, cut) for p in pr if p.name in ("aws", "jwt") for cut in (False, True)]
        elif what == "dense":
            c = EC.cuts_dense(name, rules)
        elif what == "lane":
            c = EC.cuts_lane_state()
        else:
            c = {"sparse": EC.cuts_sparse, "resident": EC.cuts_resident}[what](pr)
        _CORPORA[(name, what)] = c
    return _CORPORA[(name, what)]


def _scanner(name, env, monkeypatch):
    """A scanner whose engine is created under env (and the rule set's)."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    sc = S.Scanner(EC.ruleset_config(name)[0])
    sc.engine()
    return sc


def _expect(name, msc, c):
    if (name, c.name) not in _EXPECT:
        want, winfo = S.prefilter_table_model(msc, c.args, with_info=True)
        _EXPECT[(name, c.name)] = (want, winfo, S.scan_table_model(msc, c.args))
    return _EXPECT[(name, c.name)]


def _scan(name, monkeypatch, sc, c, pol, resident=False, base=0, **kw):
    """One scan of c on sc, compared with the model; pol: the policy the
    engine was created with, as EC.plan takes it."""
    msc = _ruleset(name, monkeypatch)[0]
    want, winfo, want_findings = _expect(name, msc, c)
    plan = EC.plan(c, resident=resident, base=base, **pol)
    findings, got, info = S.scan_raw(sc, c.args, resident=resident, base=base, **kw)
    check_scan(name, c, msc, sc.rule_ids, want, winfo, want_findings, plan, findings, got, info)
    return got, info


# ---------------------------------------------------------------- 1. upload, balanced
@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_upload_balanced_sparse_gpu(ruleset, monkeypatch):
    # every file boundary of cuts_sparse is a cut: 17 segments through the two ring slots
    sc = _scanner(ruleset, dict(EC.policy_env(**EC.SPARSE_UPLOAD), TSG_WIRE_PACK="0"), monkeypatch)
    _, info = _scan(ruleset, monkeypatch, sc, _corpus(ruleset, "sparse", monkeypatch), EC.SPARSE_UPLOAD)
    assert info["stats"]["pieces"] == 17 and info["stats"]["packed_strips"] == 0


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_upload_balanced_sweeps_gpu(ruleset, monkeypatch):
    # the aws (forward) and jwt (reverse) sweeps in 256 KiB segments: the cuts fall on the file
    # boundaries of the sweep, the chunk, line and 64 KiB edges lie at every offset of a segment
    sc = _scanner(ruleset, dict(EC.policy_env(**EC.SPARSE_UPLOAD), TSG_WIRE_PACK="0"), monkeypatch)
    corpora = _corpus(ruleset, "sweep", monkeypatch)
    assert len(corpora) == 4
    for c in corpora:
        _, info = _scan(ruleset, monkeypatch, sc, c, EC.SPARSE_UPLOAD)
        assert info["stats"]["pieces"] >= 3


SMALL_CUT = dict(segment=1024, segment_min=512)


@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_upload_small_corpora_cut_gpu(ruleset, monkeypatch):
    # the small corpora of test_gpu_candidates.py in segments of 1 KiB (512 bytes on the tail): at
    # least three each, but for the two-file batch-end corpora, which cuts at file boundaries make two
    sc = _scanner(ruleset, dict(EC.policy_env(**SMALL_CUT), TSG_WIRE_PACK="0"), monkeypatch)
    for c in _corpus(ruleset, "small", monkeypatch):
        _, info = _scan(ruleset, monkeypatch, sc, c, SMALL_CUT)
        assert info["stats"]["pieces"] >= min(3, sum(1 for a in c.args if a.Content)), c.name


# ---------------------------------------------------------------- 2. upload, geometric tail
@pytest.mark.parametrize("replicas", [1, 2])
@pytest.mark.parametrize("ruleset", EC.RULESETS)
def test_upload_geometric_tail_gpu(ruleset, replicas, monkeypatch):
    # replicas 2: two drivers pull the segments, each on a lane and a ring of its own
    sc = _scanner(ruleset, dict(EC.policy_env(**EC.DENSE_UPLOAD), TSG_ENGINE_REPLICAS=replicas), monkeypatch)
    dense = _corpus(ruleset, "dense", monkeypatch)
    _, info = _scan(ruleset, monkeypatch, sc, dense, EC.DENSE_UPLOAD)
    assert info["stats"]["pieces"] == 8 and info["stats"]["devices"] == replicas
    names = set()
    for c in _corpus(ruleset, "small", monkeypatch):
        if c.name.split("-")[0] in ("clip", "gate", "nlflags", "nlnear"):
            _scan(ruleset, monkeypatch, sc, c, EC.DENSE_UPLOAD)
            names.add(c.name.split("-")[0])
    assert names == {"clip", "gate", "nlflags", "nlnear"}
    # the dense corpus again, behind the others on the same lanes
    _scan(ruleset, monkeypatch, sc, dense, EC.DENSE_UPLOAD)


# ---------------------------------------------------------------- 3. wire packing
WIRE_MODES = {"force": {"TSG_WIRE_PACK": "force"}, "race": {"TSG_WIRE_PACK": "1"},
              "nopackers": {"TSG_WIRE_PACK": "1", "TSG_WIRE_PACK_THREADS": "0"}}


@pytest.mark.parametrize("mode", list(WIRE_MODES))
@pytest.mark.parametrize("ruleset", ["builtin", "k1c"])
def test_wire_packed_strips_gpu(ruleset, mode, monkeypatch):
    env = dict(EC.policy_env(**EC.SPARSE_WIRE), TSG_WIRE_STRIP_BYTES=EC.WIRE_STRIP, **WIRE_MODES[mode])
    sc = _scanner(ruleset, env, monkeypatch)
    c = _corpus(ruleset, "sparse", monkeypatch)
    _, info = _scan(ruleset, monkeypatch, sc, c, EC.SPARSE_WIRE)
    st = info["stats"]
    nstrips = sum(-(-s["bytes"] // EC.WIRE_STRIP) for s in info["segments"])
    assert st["pieces"] == 9 and st["packed_strips"] + st["raw_strips"] == nstrips
    if mode == "force":
        # every strip waits for a packer; the 5-byte one gains nothing and goes as it is
        assert st["packed_strips"] > 0 and st["raw_strips"] >= 1
    if mode == "nopackers":
        assert st["packed_strips"] == 0


# ---------------------------------------------------------------- 4. direct stage
FEEDS = {"pinned+0": dict(pinned=True, data_shift=0), "pinned+8": dict(pinned=True, data_shift=8),
         "pinned+1": dict(pinned=True, data_shift=1), "pageable": dict(pinned=False, data_shift=0)}


@pytest.mark.parametrize("feed", list(FEEDS))
@pytest.mark.parametrize("ruleset", ["builtin", "k1c"])
def test_direct_stage_gpu(ruleset, feed, monkeypatch):
    # the default policy: one segment.  A pinned batch of at most 1 MiB is copied by the prologue
    # kernel (16-byte words from an aligned source, bytes from the others); a pageable one is uploaded
    sc = _scanner(ruleset, {}, monkeypatch)
    corpora = _corpus(ruleset, "small", monkeypatch) + [_corpus(ruleset, "dense", monkeypatch)]
    assert all(c.nbytes <= 1 << 20 for c in corpora)
    for c in corpora:
        _, info = _scan(ruleset, monkeypatch, sc, c, {}, **FEEDS[feed])
        st = info["stats"]
        assert st["pieces"] == 1, c.name
        # (the copy engine's time is measured only where it is used)
        assert (st["h2d_ms"] > 0) == (feed == "pageable"), (c.name, st["h2d_ms"])


# ---------------------------------------------------------------- 5. resident pieces
@pytest.mark.parametrize("drivers", [1, 2])
@pytest.mark.parametrize("pieces", EC.RESIDENT_PIECES)
@pytest.mark.parametrize("ruleset", ["builtin", "k1c"])
def test_resident_pieces_gpu(ruleset, pieces, drivers, monkeypatch):
    pol = dict(pieces=pieces, min_piece=1)
    sc = _scanner(ruleset, dict(EC.policy_env(**pol), TSG_RESIDENT_DRIVERS=drivers), monkeypatch)
    c = _corpus(ruleset, "resident", monkeypatch)
    leads, lead_cands = set(), 0
    for base in EC.RESIDENT_BASES:
        _, info = _scan(ruleset, monkeypatch, sc, c, pol, resident=True, base=base)
        assert info["stats"]["pieces"] == pieces
        leads.update(s["lead_bytes"] for s in info["segments"][1:])
        lead_cands += sum(len(s["lead_cands"]) for s in info["segments"])
    assert leads >= {0, 1, 15, 16, 17, 255}
    # the leads that hold a whole probe: K2 emitted its candidate for the lead (dropped), and the
    # comparison found it once under the previous file, from the previous piece
    assert lead_cands >= 2


@pytest.mark.parametrize("chain", [0, 1, 2])
def test_resident_chain_modes_gpu(chain, monkeypatch):
    pol = dict(pieces=9, min_piece=1)
    sc = _scanner("builtin", dict(EC.policy_env(**pol), TSG_RESIDENT_DRIVERS=2, TSG_CHAIN_K1=chain), monkeypatch)
    c = _corpus("builtin", "resident", monkeypatch)
    _, info = _scan("builtin", monkeypatch, sc, c, pol, resident=True, base=240)
    # base 240: the leads of 255 and 241 bytes hold a whole probe and a probe's head
    assert sum(len(s["lead_cands"]) for s in info["segments"]) >= 1


# ---------------------------------------------------------------- 6. lane state
LANE_DENSE_UPLOAD = dict(EC.LANE_UPLOAD, segment_min=16384)      # cuts_dense under it: six halving segments


@pytest.mark.parametrize("resident", [False, True], ids=["upload", "resident"])
def test_lane_state_gpu(resident, monkeypatch):
    pol = EC.LANE_RESIDENT if resident else LANE_DENSE_UPLOAD
    sc = _scanner("builtin", dict(EC.policy_env(**pol), TSG_WIRE_PACK="0"), monkeypatch)
    dense, lane = _corpus("builtin", "dense", monkeypatch), _corpus("builtin", "lane", monkeypatch)
    first, info1 = _scan("builtin", monkeypatch, sc, dense, pol, resident=resident)
    assert info1["stats"]["pieces"] >= 4
    # sparse, dense, sparse, dense: each dense segment's K2 grid is sized from a sparse one's
    _, info = _scan("builtin", monkeypatch, sc, lane, pol, resident=resident)
    hits = [s["hits"] for s in info["segments"]]
    assert len(hits) == 4 and min(hits[1], hits[3]) > 256 * 256 > 256 > max(hits[0], hits[2])
    # grown capacities and a dense predecessor change nothing for a later batch
    again, info2 = _scan("builtin", monkeypatch, sc, dense, pol, resident=resident)
    assert sorted(again) == sorted(first) and all((again[k] == first[k]).all() for k in first)
    assert [(s["hits"], s["chunk_newlines"].tolist()) for s in info2["segments"]] == \
           [(s["hits"], s["chunk_newlines"].tolist()) for s in info1["segments"]]
    assert (info2["flags"] == info1["flags"]).all()


# ---------------------------------------------------------------- 7. concurrent scans
def test_concurrent_scans_gpu(monkeypatch):
    # two threads, two corpora, one engine with the hook on: each result is its own
    sc = _scanner("builtin", dict(EC.policy_env(**EC.DENSE_UPLOAD), TSG_WIRE_PACK="0"), monkeypatch)
    msc = _ruleset("builtin", monkeypatch)[0]
    corpora = [_corpus("builtin", "dense", monkeypatch), _corpus("builtin", "resident", monkeypatch)]
    expect = [_expect("builtin", msc, c) for c in corpora]
    out, errs = [[], []], []

    def run(i):
        try:
            for _ in range(3):
                out[i].append(S.scan_raw(sc, corpora[i].args))
        except Exception as e:               # noqa: BLE001 -- reported by the main thread
            errs.append(e)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i, c in enumerate(corpora):
        plan = EC.plan(c, **EC.DENSE_UPLOAD)
        assert len(out[i]) == 3
        for findings, got, info in out[i]:
            check_scan("builtin", c, msc, sc.rule_ids, *expect[i], [dict(s) for s in plan], findings, got, info)
