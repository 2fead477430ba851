"""K1's guided work schedule on the GPU against the CPU table model, item by
item: the schedule corpora of tests/_schedule_corpus.py, built for this
device's grid (W = 16 x its CUs), run through tsg_prefilter_resident with
128-byte chunks so that one launch has

* two, three or four levels of lane ranges (8 | 4 | 2 | 1 chunks), or one
  level dealt wholly by the counters;
* a partial last item of the top level with a clipped lane;
* dozens of items from each of the eight per-XCD counters (and, in the
  `groups` cases, from every scan-DFA group's own counter set);
* a probe in every wave item, so a skipped item loses a candidate and a
  repeated one adds anchor hits, and probes swept over item, lane-range and
  level edges, whose hits take their item_base from a level offset.

Everything is exact (_candidate_check.check): the same (file, rule) keys with
the same sorted starts, the same anchor-hit count, one newline count per chunk
equal to numpy's, the same file flags.  Before each corpus an all-'\\n' batch
of the same length runs on the same scanner: K1's per-chunk count buffer is
reused, so a chunk the real run skipped would otherwise keep a count of an
earlier run that may already be right; after the poison it keeps 128.

What makes the comparison meaningful (every item holds a model candidate,
every counter hands out items, the poison differs in every chunk, ...) is
asserted on the CPU in tests/test_schedule_corpus.py, as is the host's
restatement of the schedule (csrc/k1_schedule.h) that shapes the corpora.
"""
import time

import numpy as np
import pytest

import _edge_corpus as EC
import _schedule_corpus as SC
from _candidate_check import check as _check
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

CASES = [(shape, "builtin") for shape in SC.SHAPES] + \
        [(shape, ruleset) for ruleset in ("k1c", "groups") for shape in ("l421", "l8421")]

_RULESETS = {}      # ruleset -> (model scanner, probes, scan-DFA groups)


def _ruleset(name, monkeypatch):
    cfg, env = EC.ruleset_config(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _RULESETS:
        sc = S.Scanner(cfg)
        ngroups = int(S.prefilter_report(sc).splitlines()[1].split()[0])
        _RULESETS[name] = (sc, EC.probes(name, EC.rule_table(sc)), ngroups)
    return (cfg,) + _RULESETS[name]


def _resident(sc, args, pad=None):
    """One upload and one run of K1 + K2; the device copy of the batch is
    freed before the next upload, so the peak device use is one batch."""
    import torch
    out = S.prefilter_resident(sc, args, pad=pad)
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("shape,ruleset", CASES, ids=["%s-%s" % c for c in CASES])
def test_k1_schedule_gpu(shape, ruleset, monkeypatch):
    import torch
    t0 = time.perf_counter()
    sms = torch.cuda.get_device_properties(0).multi_processor_count
    W = 16 * sms
    cfg, msc, pr, ngroups = _ruleset(ruleset, monkeypatch)
    for k, v in SC.shape_env(shape).items():
        monkeypatch.setenv(k, v)
    c = SC.build(shape, W, pr, tag=ruleset)
    sched = c.note["sched"]
    assert sched.nitems > W and sched.levels() == list(SC.SHAPES[shape][3])
    sc = S.Scanner(cfg)
    sc.engine()
    # ---- the poison: every chunk's count becomes 128 (the last chunk's: its bytes)
    got, info = _resident(sc, SC.poison(c))
    assert info["stats"]["k1_blocks"] == sms and info["stats"]["chunk_bytes"] == SC.CHUNK == info["chunk_bytes"]
    want_poison = np.full(sched.nchunks, SC.CHUNK, np.int64)
    want_poison[-1] = SC.CHUNK - SC.END_SHORT
    nl = info["chunk_newlines"].astype(np.int64)
    assert len(nl) == sched.nchunks
    bad = np.nonzero(nl != want_poison)[0]
    assert len(bad) == 0, ("poison: newline count of chunk %d: GPU %d, batch %d; %d chunks differ; %s"
                           % (bad[0], nl[bad[0]], want_poison[bad[0]], len(bad), sched.locate(int(bad[0]) * SC.CHUNK)))
    assert info["stats"]["hits"] == 0 and info["stats"]["candidates"] == 0 and not got
    # ---- the corpus against the model
    want, winfo = S.prefilter_table_model(msc, c.args, with_info=True)
    assert winfo["hits"] >= sched.nitems
    got, info = _resident(sc, c.args, pad=((b"\n" + pr[0].text) * 4)[:64])
    assert info["stats"]["k1_blocks"] == sms and info["stats"]["chunk_bytes"] == SC.CHUNK
    _check(c, sc.rule_ids, got, info, want, winfo, SC.CHUNK)
    if ruleset == "groups":
        # one launch per scan-DFA group, each on its own counter set
        assert ngroups > 1 and info["stats"]["k1_launches"] == ngroups
    else:
        assert info["stats"]["k1_launches"] == 1
    print("%s: %d bytes (%.1f MiB), %d wave items on W = %d waves, %d anchor hits, K1 %.3f ms, test %.2f s"
          % (c.name, c.nbytes, c.nbytes / 2 ** 20, sched.nitems, W, winfo["hits"], info["stats"]["k1_ms"],
             time.perf_counter() - t0))
