"""K1's item schedule without a GPU: the host's restatement of it
(csrc/k1_schedule.h through tsg_test_k1_schedule) and the schedule corpora of
tests/_schedule_corpus.py -- the conditions that make the GPU comparison of
tests/test_gpu_k1_schedule.py mean something.

The restatement, over grids of 1 .. 304 workgroups, 0 .. 16 tail rounds, with
and without the 8-chunk level, at and around every level boundary:
* the lanes' ranges of items 0 .. nitems - 1 partition [0, nchunks) exactly;
* every lane range lies inside its item's 64 * kU chunks (the hit record's
  offset bound);
* the static round plus the eight counters reach every item whenever
  k1_grid_ok holds, and where it does not some item has no taker -- but for
  the at most `blocks` items right behind the static round, which the
  counters of a grid of fewer than 8 workgroups do reach (the guard is
  conservative by that much);
* for the grid the host picks, k1_grid_ok holds on every device of 8 or more
  CUs and fails on smaller ones.

The corpora: the levels the shape names and no others, more items than waves,
at least two draws from each counter, a clipped lane in the top level's last
item, a model candidate starting in every item, and an all-'\\n' poison batch
whose newline counts differ from the corpus's in every chunk.
"""
import numpy as np
import pytest

import _edge_corpus as EC
import _schedule_corpus as SC
from trivy_amd import secret as S

BLOCKS = list(range(1, 10)) + [15, 16, 32, 255, 256, 304]
ROUNDS = (0, 1, 2, 16)
FULL_LANES_LIMIT = 1 << 19           # lanes expanded one by one below this many; item by item above


def _boundaries(W, rounds, top8):
    """nchunks at which a level fills up, and the offsets around them."""
    out = {1, 63, 64, 65}
    at = 0
    for k in (1, 2, 4) + ((8,) if top8 else ()):
        at += 64 * k * W * rounds
        for d in (0, 1, -1, 64 * k, -64 * k):
            out.add(at + d)
        if rounds == 0:
            break
    top = 8 if top8 else 4
    for d in (1, top - 1, top, 64 * top - 1, 64 * top, 64 * top + 1, 64 * top * (W + 3) + 5):
        out.add(at + d)
    out.update(SC.nchunks_of(n, W) for n in SC.SHAPES)
    return sorted(n for n in out if n > 0)


def _reachable(nitems, W, blocks):
    """Items some wave takes: wave w item w, then W + xc + 8 k from counter xc
    of the workgroups with blockIdx.x % 8 == xc (tsg_k1_scan_v3's take())."""
    got = np.zeros(nitems, bool)
    got[:W] = True
    for xc in {b % 8 for b in range(min(blocks, 8))}:
        got[W + xc::8] = True
    return got


def _check_schedule(nchunks, blocks, rounds, top8):
    W = 16 * blocks
    sc = S.k1_schedule(nchunks, blocks, rounds, top8)
    tag = (nchunks, blocks, rounds, top8)
    kU, c0, rend, n = sc["kU"], sc["c0"], sc["rend"], sc["nitems"]
    assert sc["n8"] + sc["n4"] + sc["n2"] + sc["n1"] == nchunks, tag
    assert top8 or sc["n8"] == 0, tag
    # the levels as tsg_k1_scan_v3 states them
    n1 = min(nchunks, W * 64 * rounds)
    n2 = min(nchunks - n1, W * 128 * rounds)
    n4 = min(nchunks - n1 - n2, W * 256 * rounds) if top8 else nchunks - n1 - n2
    assert (sc["n8"], sc["n4"], sc["n2"], sc["n1"]) == (nchunks - n1 - n2 - n4, n4, n2, n1), tag
    assert n == len(kU) == sum(-(-sc[k] // (64 * u)) for k, u in (("n8", 8), ("n4", 4), ("n2", 2), ("n1", 1))), tag
    assert n > 0 and set(np.unique(kU)) <= {1, 2, 4, 8}, tag
    assert (np.diff(kU) <= 0).all(), tag                       # 8 | 4 | 2 | 1 through the batch
    # ---- the items tile [0, nchunks): each begins where the one before ends
    cend = np.minimum(c0 + 64 * kU, rend)
    assert c0[0] == 0 and cend[-1] == nchunks and (c0[1:] == cend[:-1]).all() and (cend > c0).all(), tag
    # ---- the lanes: lane j of an item walks [c0 + j kU, min(c0 + (j + 1) kU, rend))
    if n * 64 <= FULL_LANES_LIMIT:
        items = np.arange(n)
    else:                                                      # every level's first and last items, and a sample
        edge = np.nonzero(np.diff(kU))[0]
        items = np.unique(np.concatenate([[0, 1, n - 2, n - 1], edge, edge + 1, edge + 2, edge - 1,
                                          np.arange(0, n, max(1, n // 997))]).clip(0, n - 1))
    lane = np.arange(64)[None, :]
    lo = c0[items, None] + lane * kU[items, None]
    hi = np.minimum(lo + kU[items, None], rend[items, None])
    live = lo < rend[items, None]
    # inside the item's 64 * kU chunks; the live lanes, in order, tile the item
    assert (hi[live] <= (c0[items, None] + 64 * kU[items, None]).repeat(64, 1)[live]).all(), tag
    assert (hi[live] > lo[live]).all() and live[:, 0].all(), tag
    assert (live[:, 1:] <= live[:, :-1]).all(), tag            # idle lanes only behind the clipped one
    assert (lo[:, 1:][live[:, 1:]] == hi[:, :-1][live[:, 1:]]).all(), tag
    last = live.sum(1) - 1
    assert (hi[np.arange(len(items)), last] == cend[items]).all() and (lo[:, 0] == c0[items]).all(), tag
    if len(items) == n:
        covered = np.zeros(nchunks + 1, np.int64)
        np.add.at(covered, lo[live], 1)
        np.add.at(covered, hi[live], -1)
        assert (np.cumsum(covered)[:nchunks] == 1).all(), tag
    # ---- takers
    reach = _reachable(n, W, blocks)
    assert sc["grid_ok"] == (blocks >= 8 or n <= W), tag
    if sc["grid_ok"]:
        assert reach.all(), tag
    else:
        assert blocks < 8 and n > W, tag
        assert reach.all() == (n <= W + blocks), tag
    return sc


@pytest.mark.parametrize("top8", [False, True], ids=["top4", "top8"])
@pytest.mark.parametrize("rounds", ROUNDS)
def test_restatement_partitions_and_takers(rounds, top8):
    lost = 0
    for blocks in BLOCKS:
        for nchunks in _boundaries(16 * blocks, rounds, top8):
            sc = _check_schedule(nchunks, blocks, rounds, top8)
            lost += not sc["grid_ok"]
    assert lost > 0                    # the guard's failing side is among the cases


def test_host_grid_is_ok_from_8_cus_on():
    # the grid Engine::seg_prologue picks: min(ceil(nchunks / 1024), CUs)
    bad_small = 0
    for sms in list(range(1, 41)) + [64, 104, 128, 228, 255, 256, 304]:
        for rounds in ROUNDS:
            for top8 in (False, True):
                for nchunks in _boundaries(16 * sms, rounds, top8) + [1024 * sms - 1, 1024 * sms, 1024 * sms + 1,
                                                                      1024 * (sms - 1) + 1, 1 << 24]:
                    if nchunks <= 0:
                        continue
                    blocks = max(1, min(-(-nchunks // 1024), sms))
                    sc = S.k1_schedule(nchunks, blocks, rounds, top8, with_items=False)
                    if sms >= 8:
                        assert sc["grid_ok"], (sms, nchunks, rounds, top8)
                        # a grid below the device's CUs holds all its items in the static round
                        assert blocks == sms or sc["nitems"] <= 16 * blocks, (sms, nchunks, rounds, top8)
                    else:
                        bad_small += not sc["grid_ok"]
    assert bad_small > 0               # only a device of fewer than 8 CUs can fail the guard


def test_hook_rejects_bad_arguments():
    from trivy_amd import _lib
    lv = np.zeros(6, np.uint64)
    L = _lib.lib()
    assert L.tsg_test_k1_schedule(100, 0, 1, 0, lv.ctypes.data, None, 0) != 0
    assert L.tsg_test_k1_schedule(100, 1, 1, 0, None, None, 0) != 0
    items = np.zeros(3, np.uint64)
    assert L.tsg_test_k1_schedule(1000, 1, 1, 0, lv.ctypes.data, items.ctypes.data, 1) != 0      # 16 items
    assert L.tsg_test_k1_schedule(0, 1, 1, 0, lv.ctypes.data, None, 0) == 0 and lv[4] == 0


# ------------------------------------------------------------------ corpora
_STATE = {}


def _builtin():
    if "builtin" not in _STATE:
        sc = S.Scanner(None)
        rules = EC.rule_table(sc)
        _STATE["builtin"] = (sc, EC.probes("builtin", rules))
    return _STATE["builtin"]


CASES = [(name, 4096) for name in SC.SHAPES] + [("l21", 512)]


@pytest.mark.parametrize("name,W", CASES, ids=["%s-W%d" % c for c in CASES])
def test_schedule_corpus(name, W):
    msc, pr = _builtin()
    c = SC.build(name, W, pr)
    sc = c.note["sched"]
    rounds, top8, _, levels = SC.SHAPES[name]
    # ---- the shape: these levels, more items than waves, every counter drawn from
    assert sc.levels() == list(levels) and (sc.rounds, sc.top8) == (rounds, top8)
    assert sc.nchunks >= 64 * W                                # the host's grid is the whole device
    assert sc.nitems > W and sc.grid_ok
    draws = np.bincount((np.arange(W, sc.nitems) - W) % 8, minlength=8)
    assert draws.min() >= 2 and draws.min() >= 30 and draws.sum() == sc.nitems - W
    for xc in range(8):
        assert [sc.counter_of(W + xc + 8 * k) for k in range(2)] == [xc, xc]
    # ---- the top level's last item is partial, one of its lanes clipped
    top = levels[0]
    first, last = sc.level_items(top)
    assert first == 0 and not sc.full(last) and sc.full(last - 1)
    left = int(sc.cend[last] - sc.c0[last])
    assert left % top != 0 and 0 < left // top < 63            # a clipped lane, idle lanes behind it
    assert c.nbytes == sc.nchunks * SC.CHUNK - SC.END_SHORT and int(sc.end[-1]) == c.nbytes
    # ---- the edges: a sweep of every offset per level (where it has that many items), the unique ones
    for k in levels:
        f, l = sc.level_items(k)
        sw = c.note["swept"][k]
        assert len(sw) == min(SC.SWEEP, l - max(f, W if l >= W else f) + 1) - (1 if f == 0 and l < W else 0)
        if len(sw) >= SC.SWEEP - 1:
            assert len({d for _, d, _ in sw}) >= SC.SWEEP - 8, k   # (a delta moves where a probe met a neighbour)
        assert {cut for _, _, cut in sw} == {False, True}
        assert all(sc.item_of(e) >= W for e, _, _ in sw) == (l >= W)
        assert int(sc.start[l]) in c.note["edges"] and (f == 0 or int(sc.start[f]) in c.note["edges"])
        for i in (f, l if sc.full(l) else l - 1):
            for lane in (1, 31, 63):
                assert int(sc.start[i]) + lane * k * SC.CHUNK in c.note["edges"], (k, i, lane)
    for i in range(W - 1, W + 9):
        assert int(sc.start[i]) in c.note["edges"], i
    assert all(-40 <= d <= 40 for _, d, _ in c.note["edges"].values())
    offs = set(c.offsets.tolist())
    cuts = [e for sw in c.note["swept"].values() for e, _, cut in sw if cut]
    assert cuts and all(e in offs for e in cuts)
    assert len(offs - set(cuts) - {0, c.nbytes}) >= 3          # file boundaries away from any edge
    assert any(pl.start is None for pl in c.placements) and len(c.args) > len(cuts)
    # ---- every probe kind lies in items; every item has a probe of its own
    assert len(c.note["item_probes"]) == sc.nitems
    assert {n for names in c.note["item_probes"] for n in names} == {p.name for p in pr}
    # ---- the model: a candidate starts in every item, an anchor hit per item at least
    cands, info = S.prefilter_table_model(msc, c.args, with_info=True)
    assert info["hits"] >= sc.nitems
    per_item = np.zeros(sc.nitems, np.int64)
    for (f, r), starts in cands.items():
        st = starts[starts != S.FULL_SCAN_START].astype(np.int64) + int(c.offsets[f])
        np.add.at(per_item, np.searchsorted(sc.start, st, side="right") - 1, 1)
    none = np.nonzero(per_item == 0)[0]
    assert len(none) == 0, ("items without a model candidate", none[:8], sc.locate(int(sc.start[none[0]])))
    # ---- the poison batch: its count differs from the corpus's in every chunk
    data, offsets = S.pack(c.args)
    ref = SC.chunk_newlines(data, c.nbytes, SC.CHUNK)
    want_poison = np.full(sc.nchunks, SC.CHUNK, np.int64)
    want_poison[-1] = SC.CHUNK - SC.END_SHORT
    assert len(ref) == sc.nchunks and (ref != want_poison).all() and ref.max() < SC.CHUNK - SC.END_SHORT
    pz = SC.poison(c)
    assert len(pz) == 1 and len(pz[0].Content) == c.nbytes and set(pz[0].Content[:4096]) == {10}


def test_tiled_filler_is_the_filler():
    n = (3 << 20) + 1234
    assert SC.tiled_filler(n).tobytes() == EC.filler(n)
