"""Schedule corpora: batches shaped so that one K1 launch runs every part of
the guided work schedule of tsg_k1_scan_v3 (engine.hip) -- several levels of
8-, 4-, 2- and 1-chunk lane ranges, a partial last item of the top level, and
dozens of items from each of the eight per-XCD counters -- with a probe in
every wave item and around every kind of item edge.  tests/
test_schedule_corpus.py checks them on the CPU, tests/test_gpu_k1_schedule.py
compares K1 + K2 on them with the CPU table model.

The geometry comes from the host's restatement of the schedule
(csrc/k1_schedule.h through S.k1_schedule), never from the kernel: the GPU
tests tie the two together.  Everything is deterministic.

Shapes, in chunks of CHUNK bytes on W waves (16 x the workgroups of a full
grid) with q = Q:

  l21     rounds 1            64 W + 128 q + 39    levels 2 (partial), 1
  l421    rounds 1           192 W + 256 q + 87    levels 4 (partial), 2, 1
  l8421   rounds 1, top8     448 W + 512 q + 299   levels 8 (partial), 4, 2, 1
  r2      rounds 2           128 W + 128 q + 39    levels 2 (partial), 1 (two rounds)
  all4    rounds 0           256 (W + q) + 87      level 4 only
  all8    rounds 0, top8     512 (W + q) + 299     level 8 only

The remainders are no multiples of the level's range length, so one lane of
the top level's last item is clipped by the level's end and the lanes behind
it idle; the batch ends END_SHORT bytes before the end of its last chunk.
"""
import bisect

import numpy as np

import _edge_corpus as EC
from trivy_amd import secret as S

CHUNK = 128
Q = 300
END_SHORT = 77
SWEEP = 81                              # swept item edges per level: one per offset -40 .. +40
MARGIN = 64                             # an item's own probe keeps this far from the item's ends

# name: (TSG_K1_TAIL_ROUNDS, top8, nchunks(W, q), the levels (kU) present)
SHAPES = {
    "l21": (1, False, lambda W, q: 64 * W + 128 * q + 39, (2, 1)),
    "l421": (1, False, lambda W, q: 192 * W + 256 * q + 87, (4, 2, 1)),
    "l8421": (1, True, lambda W, q: 448 * W + 512 * q + 299, (8, 4, 2, 1)),
    "r2": (2, False, lambda W, q: 128 * W + 128 * q + 39, (2, 1)),
    "all4": (0, False, lambda W, q: 256 * (W + q) + 87, (4,)),
    "all8": (0, True, lambda W, q: 512 * (W + q) + 299, (8,)),
}


def shape_env(name, chunk=CHUNK):
    """The environment an engine needs to run the shape's schedule on a
    resident batch (TSG_K1_TOP8=2 forces the 8-chunk level onto one)."""
    rounds, top8, _, _ = SHAPES[name]
    env = {"TSG_K1_CHUNK": str(chunk), "TSG_K1_TAIL_ROUNDS": str(rounds)}
    if top8:
        env["TSG_K1_TOP8"] = "2"
    return env


def nchunks_of(name, W, q=Q):
    return SHAPES[name][2](W, q)


class Schedule:
    """The items of one launch (S.k1_schedule) in bytes of the batch."""

    def __init__(self, nchunks, W, rounds, top8, chunk, total):
        assert W % 16 == 0
        sc = S.k1_schedule(nchunks, W // 16, rounds, top8)
        self.nchunks, self.W, self.rounds, self.top8, self.chunk, self.total = nchunks, W, rounds, top8, chunk, total
        self.sizes = {8: sc["n8"], 4: sc["n4"], 2: sc["n2"], 1: sc["n1"]}
        self.nitems, self.grid_ok = sc["nitems"], sc["grid_ok"]
        self.kU, self.c0, self.rend = sc["kU"], sc["c0"], sc["rend"]
        self.cend = np.minimum(self.c0 + 64 * self.kU, self.rend)           # the item's chunks: [c0, cend)
        self.start = self.c0 * chunk                                        # ... and bytes: [start, end)
        self.end = np.minimum(self.cend * chunk, total)

    def levels(self):
        """kU of the non-empty levels, in batch order."""
        return [k for k in (8, 4, 2, 1) if self.sizes[k]]

    def level_items(self, k):
        """(first, last) item of level kU = k."""
        idx = np.nonzero(self.kU == k)[0]
        return int(idx[0]), int(idx[-1])

    def full(self, i):
        return int(self.cend[i] - self.c0[i]) == 64 * int(self.kU[i])

    def item_of(self, b):
        return int(np.searchsorted(self.start, b, side="right")) - 1

    def counter_of(self, i):
        """The counter (blockIdx.x % 8 of its readers) that hands out item i; None: the static round."""
        return None if i < self.W else (i - self.W) % 8

    def locate(self, b):
        """Names the item, level, lane and counter of a batch offset, for a failure message."""
        i = self.item_of(b)
        k = int(self.kU[i])
        first, last = self.level_items(k)
        lane, within = divmod(b - int(self.start[i]), k * self.chunk)
        xc = self.counter_of(i)
        return ("wave item %d of %d (W = %d: %s), level kU = %d (items %d..%d, %s item), lane %d, chunk %d of its %d, "
                "byte %d of the item's %d"
                % (i, self.nitems, self.W, "static round" if xc is None else "draw %d of counter %d" % ((i - self.W) // 8, xc),
                   k, first, last, "a full" if self.full(i) else "the partial", lane, within // self.chunk, k,
                   b - int(self.start[i]), int(self.end[i] - self.start[i])))


class _Occupied:
    """Disjoint byte intervals of the buffer that hold a probe or lie next to a file boundary."""

    def __init__(self):
        self.s, self.e = [], []

    def free(self, a, b):
        i = bisect.bisect_right(self.s, a)
        return (i == 0 or self.e[i - 1] <= a) and (i == len(self.s) or self.s[i] >= b)

    def add(self, a, b):
        i = bisect.bisect_right(self.s, a)
        self.s.insert(i, a)
        self.e.insert(i, b)


def tiled_filler(n):
    """EC.filler(n) by tiling: the same bytes without an index array of n entries."""
    base = np.frombuffer(EC.filler((1 << 20) + 37), dtype=np.uint8)
    return np.resize(base, n)


def build(name, W, pr, tag="builtin", chunk=CHUNK, q=Q):
    """The shape's corpus for a grid of W waves and the probes pr (EC.probes).
    note: "sched" (Schedule), "edges" {batch offset of an item / lane / level
    edge: (what, delta, probe name)}, "swept" {kU: [(edge, delta, is a file
    boundary)]}, "item_probes" (one list of probe names per item), "locate"."""
    rounds, top8, fn, _ = SHAPES[name]
    nchunks = fn(W, q)
    total = nchunks * chunk - END_SHORT
    sc = Schedule(nchunks, W, rounds, top8, chunk, total)
    buf = bytearray(tiled_filler(total))
    occ = _Occupied()
    placed, bounds, edges, swept = [], [], {}, {}
    loud = [p for p in pr if p.kind != "reject" and p.mode != 3]     # probes that yield a candidate at their text

    def fits(p, anchor_end_at):
        at = anchor_end_at - p.anchor_end
        return at - 1 >= 0 and at + len(p.text) + 1 <= total and occ.free(at - 1, at + len(p.text) + 1)

    def put(p, anchor_end_at):
        at = EC._place(buf, p, anchor_end_at)
        occ.add(at - 1, at + len(p.text) + 1)
        placed.append((p, at))
        return at

    def edge(e, what, k, j, boundary=False):
        """A probe whose anchor ends at e + delta, delta cycling as EC.edge_sweep's;
        the next probe (then the next delta) where one does not fit.  The batch's
        first byte has no room in front of it and gets none."""
        if e in edges or e <= 0 or e >= total:
            return None
        for t in range(len(pr) * SWEEP):
            delta = (k + 20 * j + 17 * (t // len(pr))) % SWEEP - 40
            p = pr[(k + j + t) % len(pr)]
            if fits(p, e + delta):
                put(p, e + delta)
                edges[e] = (what, delta, p.name)
                if boundary:
                    bounds.append(e)
                return delta
        raise AssertionError("no probe fits the edge at %d (%s)" % (e, what))

    # ---- the sweep: SWEEP consecutive item starts per level, from item W on
    # where the level has items the counters hand out (else its static items)
    for j, k in enumerate(sc.levels()):
        first, last = sc.level_items(k)
        i0 = max(first, W) if last >= W else first
        swept[k] = []
        for n, i in enumerate(range(i0, min(i0 + SWEEP, last + 1))):
            e = int(sc.start[i])
            cut = n % 2 == 1
            d = edge(e, "sweep kU=%d item %d" % (k, i), n, j, boundary=cut)
            if d is not None:
                swept[k].append((e, d, cut))
    # ---- the unique edges
    u = [0]

    def unique(e, what):
        edge(int(e), what, u[0], 5)
        u[0] += 1
    for k in sc.levels():
        first, last = sc.level_items(k)
        unique(sc.start[first], "level kU=%d begins" % k)
        unique(sc.start[last], "last item of level kU=%d" % k)
        lane_items = [first if sc.full(first) else None, last if sc.full(last) else last - 1]
        for i in lane_items:
            if i is None or i < first or not sc.full(i):
                continue
            for lane in (1, 31, 63):
                unique(sc.start[i] + lane * k * chunk, "lane %d of item %d (kU=%d)" % (lane, i, k))
    for i in range(W - 1, min(W + 9, sc.nitems)):
        unique(sc.start[i], "item W%+d" % (i - W))
    # ---- a few file boundaries inside items, away from every edge
    for n in range(1, 6):
        i = sc.nitems * n // 6
        b = int(sc.start[i] + (sc.end[i] - sc.start[i]) // 2) + 13
        if occ.free(b - 2, b + 2):
            bounds.append(b)
            occ.add(b - 2, b + 2)
    # ---- one probe in every item, all probes in turn; where that one yields
    # no candidate at its place (a rejected decoy, a presence rule), a second
    # one that does: a lost item always loses a candidate
    rng = np.random.RandomState(0x5CED + W)
    item_probes = []
    for i in range(sc.nitems):
        a, b = int(sc.start[i]) + MARGIN, int(sc.end[i]) - MARGIN
        mine = [pr[i % len(pr)]]
        if mine[0] not in loud:
            mine.append(loud[i % len(loud)])
        for p in mine:
            for _ in range(200):
                at = int(rng.randint(a + 1, b - len(p.text) - 1))
                if occ.free(at - 1, at + len(p.text) + 1):
                    put(p, at + p.anchor_end)
                    break
            else:
                raise AssertionError("no room for a probe in item %d" % i)
        item_probes.append([p.name for p in mine])
    note = {"sched": sc, "edges": edges, "swept": swept, "item_probes": item_probes, "locate": sc.locate, "shape": name}
    c = EC._from_buffer("sched-%s-W%d-%s" % (name, W, tag), buf, bounds, placed, note=note)
    assert c.nbytes == total
    return c


def poison(c):
    """A batch of the corpus's length that is all '\\n', in one file."""
    return [S.ScanArgs("poison.txt", b"\n" * c.nbytes)]


def chunk_newlines(data, total, chunk):
    """The '\\n' count of every chunk of a packed batch."""
    return np.add.reduceat(data[:total] == 10, np.arange(0, total, chunk), dtype=np.int64)
