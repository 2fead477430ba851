"""Probes of EVERY rule of a rule set, and the corpora that put a file end at
every byte of them (tests/test_rule_corpus.py on the CPU,
tests/test_gpu_rule_candidates.py on the GPU).

tests/_edge_corpus.py probes six builtin rules (four in the custom sets); which
lines of K2 a hit runs is decided by the hit's own anchor record -- offset
window, literal lengths, verify limit, gate, reverse DFA -- so here every row
of the rule table whose mode is 0, 3 or 4 gets probes of its own, the
exclude-block pseudo-rules included:

  builtin rules   the shortest and the longest distinct sample of
                  workload/rule_samples.json (strings the oracle's regexp
                  matches), plus the shortest sample of every anchor literal
                  the two do not hold, plus hand-written `aws-secret-access-key`
                  probes for the three literals no sample holds
  custom rules    strings drawn from the rule's regex (workload.synth._Sampler,
                  a fixed seed), kept when the oracle's GoRegexp matches them;
                  " " + keyword is appended where a sample holds no keyword
  exclude blocks  the configured exclude-block regexes, the global ones, then
                  the rules' in rule order (the report's order), sampled alike

Corpora (Corpus objects of tests/_edge_corpus.py, all deterministic):

  rule_file_ends  for every byte h of every probe a file that ends with the
                  probe's first h bytes, directly followed by a file that
                  begins with the rest; then the whole probe 0 .. 19 bytes
                  behind a file's start
  rule_phases     spanning files: every probe's anchor ends at every phase of
                  a 16-byte word, and every byte of its anchor literal lies
                  once just behind a multiple of 2048 (an edge of every K1
                  chunk size and of a 128-byte line)
  rule_gates      rules whose keyword gate is K1's bits ("g") and whose sample
                  holds no keyword of its own: the sample alone, the keyword
                  alone, and both, as adjacent tiny files with 0 - 2 empty
                  files between.  Rules of this kind among the probes: 5 of
                  the builtin set; the same 5 in the custom sets, whose own
                  rules all hold their keyword, plus `edge-presence` and
                  `edge-gated` of tests/_edge_corpus.py: 7.
"""
import itertools
import random
import re

import numpy as np

import _edge_corpus as EC
from oracle.goregex import GoRegexp
from trivy_amd import secret as S
from workload import synth

SEED = 0x52C0
CUSTOM_SAMPLES = 4                   # validated strings drawn per custom rule / exclude-block regex
MODES = (0, 3, 4)
CLIPPED_STARTS = 20                  # rule_file_ends: the whole probe 0 .. 19 bytes behind a file's start
EDGE = 2048                          # rule_phases: a multiple of every K1 chunk size up to 2 KiB

_KEY40 = b"q8Zr/2Lm+Vx0TgY7dKc3HnBw5PjS9fUeA1oRiX6="
assert len(_KEY40) == 40
# the literals of aws-secret-access-key that none of its 24 samples holds
AWS_SECRET_EXTRA = (b'awsaccesskey = "' + _KEY40 + b'"',            # awsacc
                    b"awskey: " + _KEY40,                          # awskey
                    b"aws__access_key=" + _KEY40 + b",")            # aws__a


# ------------------------------------------------------------- rule table
def _units(tok):
    """One literal of the report as a list of units, each the list of its
    alternatives (bytes)."""
    def unescape(s):
        return re.sub(rb"\\x([0-9a-f]{2})", lambda m: bytes([int(m.group(1), 16)]), s.encode("latin-1"))
    out, i = [], 0
    while i < len(tok):
        if tok[i] == "(":
            j = tok.index(")", i)
            out.append([unescape(a) for a in tok[i + 1:j].split("|")])
            i = j + 1
        elif tok[i] == "\\":
            out.append([unescape(tok[i:i + 4])])
            i += 4
        else:
            out.append([tok[i].encode("latin-1")])
            i += 1
    return out


def _variants(tok):
    """Every lower-cased byte string the literal stands for."""
    return frozenset(b"".join(c).lower() for c in itertools.product(*_units(tok)))


def rule_table(scanner):
    """EC.rule_table plus, per row, "limit" (the verify limit, None for mode 3)
    and "variants": one frozenset of lower-cased byte strings per anchor
    literal.  (A literal may hold blanks, which also separate the literals of
    the report's list: the list is split only where the row has several.)"""
    rules = EC.rule_table(scanner)
    lines = S.prefilter_report(scanner).splitlines()
    for rid, info in rules.items():
        info["limit"], info["variants"] = None, []
        for ln in lines:
            if ln.startswith(rid + ": ") and ln.endswith("}"):
                n = int(re.search(r"(\d+) literal\(s\)", ln).group(1))
                m = re.search(r"limit (\d+)", ln[:ln.rindex("{")])
                info["limit"] = int(m.group(1)) if m else None
                body = ln[ln.rindex(" {") + 2:-1]
                toks = [body] if n == 1 else body.split(" ")
                assert len(toks) == n, ln
                info["variants"] = [_variants(t) for t in toks]
                break
    return rules


def k2_class(info):
    return (info["mode"], info["gate"], info["dmin"], info["dmax"])


# ------------------------------------------------------------------ probes
class RuleProbe(EC.Probe):
    """base: the text without the keyword appended to it; keyword: that
    keyword, or None where the sample holds one itself; pattern: the regex the
    oracle validated the text with."""

    def __init__(self, name, rule, text, pattern, base=None, keyword=None):
        EC.Probe.__init__(self, name, rule, text)
        self.pattern, self.base, self.keyword = pattern, text if base is None else base, keyword

    def bind(self, rules):
        r = rules[self.rule]
        self.index, self.mode, self.gate, self.dmin, self.dmax = r["index"], r["mode"], r["gate"], r["dmin"], r["dmax"]
        self.limit = r["limit"]
        low = self.text.lower()
        found = [(low.find(v), v) for vs in r["variants"] for v in vs if low.find(v) >= 0]
        assert found, (self.name, r["variants"])
        at, lit = min(found)
        self.anchor_end = at + len(lit) - 1         # index of the anchor literal's last byte in text
        self.lit_len = len(lit)
        self.literals = {k for k, vs in enumerate(r["variants"]) if any(v in low for v in vs)}
        return self


def _with_keyword(text, keywords):
    """(text, base, keyword): " " + keyword appended where text holds none."""
    low = text.lower()
    if keywords and not any(k.lower().encode() in low for k in keywords):
        return text + b" " + keywords[0].encode(), text, keywords[0]
    return text, text, None


def _split_keyword(text, keywords):
    """A stored sample as (text, base, keyword): workload.synth.rule_samples
    appended " " + keywords[0] where the string held no keyword."""
    if keywords:
        tail = b" " + keywords[0].encode()
        base = text[:-len(tail)]
        if text.endswith(tail) and not any(k.lower().encode() in base.lower() for k in keywords):
            return text, base, keywords[0]
    return text, text, None


def _sampled(pattern, rng, want=CUSTOM_SAMPLES):
    """Distinct strings of `pattern` that the oracle's regexp matches."""
    rx = GoRegexp(pattern)
    got = []
    for _ in range(want * 40):
        if len(got) == want:
            break
        s = synth._Sampler(pattern, rng).sample()
        if "example" in s.lower() or "\n" in s or "\r" in s:
            continue
        b = s.encode("utf-8", "surrogateescape")
        if b not in got and rx.find_all(b):
            got.append(b)
    return got


def _pick(texts, variants):
    """The shortest and the longest of texts, then the shortest that holds
    each anchor literal those two lack."""
    texts = sorted(set(texts), key=lambda t: (len(t), t))
    out = [texts[0]] + ([texts[-1]] if len(texts) > 1 else [])
    for vs in variants:
        if not any(v in t.lower() for t in out for v in vs):
            more = [t for t in texts if any(v in t.lower() for v in vs)]
            out += more[:1]
    return out


def exclude_patterns(cfg):
    """The exclude-block regexes in the order of the table's pseudo-rules."""
    if cfg is None:
        return []
    out = list((cfg.get("exclude-block") or {}).get("regexes") or [])
    for r in cfg["rules"]:
        out += (r.get("exclude-block") or {}).get("regexes") or []
    return out


def rule_probes(ruleset, rules):
    """Bound probes of every row of rules (rule_table()) of mode 0, 3 or 4."""
    cfg, _ = EC.ruleset_config(ruleset)
    rng = random.Random(SEED)
    samples = synth.load_samples()
    sources = []                                   # (row id, pattern, [(text, base, keyword)])
    for r in S.GetBuiltinRules():
        kws = r.get("keywords") or []
        texts = [s.encode("utf-8", "surrogateescape") for s in samples[r["id"]]]
        if r["id"] == "aws-secret-access-key":
            texts += list(AWS_SECRET_EXTRA)
        sources.append((r["id"], r["regex"], [_split_keyword(t, kws) for t in texts]))
    if cfg is not None:
        for r in cfg["rules"]:
            kws = r.get("keywords") or []
            sources.append((r["id"], r["regex"], [_with_keyword(t, kws) for t in _sampled(r["regex"], rng)]))
        for k, pat in enumerate(exclude_patterns(cfg)):
            sources.append(("exclude-block #%d" % k, pat, [(t, t, None) for t in _sampled(pat, rng)]))
    out = []
    for rid, pattern, triples in sources:
        if rid not in rules or rules[rid]["mode"] not in MODES or not triples:
            continue
        by_text = {t[0]: t for t in triples}
        for k, text in enumerate(_pick(list(by_text), rules[rid]["variants"])):
            _, base, kw = by_text[text]
            out.append(RuleProbe("%s/%d" % (rid, k), rid, text, pattern, base, kw).bind(rules))
    return out


# ----------------------------------------------------------------- corpora
def file_end_pair(probe, h):
    """File A ends with the probe's first h bytes, file B begins with the
    rest."""
    return (EC.filler(100 + h, at=h) + b"\n" + probe.text[:h],
            probe.text[h:] + b"\n" + EC.filler(60, at=3 * h))


def rule_file_ends(probes, name="rule-ends", joined=False):
    """(a) For every probe and every h in 1 .. len(text): file_end_pair().  A
    verify walk that does not stop at A's end accepts; a window or reverse
    walk that is not clipped at B's start emits a start inside A; A's end and
    B's start pass through every phase of a 16-byte word.  note["pairs"]:
    (probe number, h, file A's number).  Behind the pairs of a probe come
    CLIPPED_STARTS files in which the whole probe begins 0 .. 19 bytes after
    the file's start: an offset window clipped there, with a true match
    behind it.  joined: every pair as ONE file (what
    an unclipped kernel would see), for the CPU test."""
    files, pairs, placed = [], [], []
    at = 0
    for k, p in enumerate(probes):
        for h in range(1, len(p.text) + 1):
            a, b = file_end_pair(p, h)
            pairs.append((k, h, len(files)))
            whole = h == len(p.text)
            placed.append(EC.Placement(p, len(files), len(a) - h if whole or joined else None,
                                       at + len(a) - h + p.anchor_end, len(p.text) if joined else h))
            files += [a + b] if joined else [a, b]
            at += len(a) + len(b)
        for d in range(0 if joined else CLIPPED_STARTS):
            head = EC.filler(d - 1, at=d) + b"\n" if d else b""
            placed.append(EC.Placement(p, len(files), d, at + d + p.anchor_end, len(p.text)))
            files.append(head + p.text + b"\n" + EC.filler(40 + d, at=7 * d))
            at += len(files[-1])
    return EC.Corpus(name + ("-joined" if joined else ""), files, placed, note={"pairs": pairs})


def rule_phases(probes, name="rule-phases"):
    """(b) Spanning files, no cut at a probe.  Every probe is placed 16 times,
    the batch offset of its anchor's last byte congruent to 0 .. 15 mod 16, and
    once for every s in 0 .. lit_len - 1 with that byte at E + s, E a multiple
    of 2048: every byte of the literal lies once just behind an edge of every
    chunk size up to 2 KiB and of a 128-byte line."""
    edge, busy, end = [], [], EDGE
    for p in probes:                               # the edge placements, one multiple of EDGE each
        for s in range(p.lit_len):
            e = -(-(end + p.anchor_end + 2 - s) // EDGE) * EDGE
            lo = e + s - p.anchor_end
            edge.append((p, e + s))
            busy.append((lo - 1, lo + len(p.text) + 1))
            end = busy[-1][1]
    gaps = [(a[1], b[0]) for a, b in zip([(0, 64)] + busy, busy + [(1 << 40, 1 << 40)])]
    phase, g = [], 0
    lo, hi = gaps[0]
    for p in probes:                               # the phase placements, first fit into the gaps between
        for k in range(16):
            while True:
                x = lo + 1 + p.anchor_end
                x += (k - x) % 16
                if x - p.anchor_end + len(p.text) + 1 <= hi:
                    break
                g += 1
                lo, hi = gaps[g]
            phase.append((p, x))
            lo = x - p.anchor_end + len(p.text) + 1
    total = max(lo, end) + 333
    buf = bytearray(EC.filler(total))
    placed = [(p, EC._place(buf, p, x)) for p, x in edge + phase]
    spans = sorted((at - 1, at + len(p.text) + 1) for p, at in placed)
    starts = [s[0] for s in spans]
    bounds = []
    for b in range(EC.BLOCK + 30011, total - 4096, 3 * EC.BLOCK // 2):
        while True:                                # no file boundary inside a probe or next to one
            i = int(np.searchsorted(starts, b, side="right")) - 1
            if i < 0 or b > spans[i][1] + 1:
                break
            b = spans[i][1] + 2
        bounds.append(b)
    c = EC._from_buffer(name, buf, bounds, placed)
    c.note = {"edge": len(edge), "phase": len(phase)}
    return c


def gate_rules(probes, rules):
    """One probe per rule with gate "g" whose sample holds no keyword of its
    own (the keyword was appended): the anchor fires without the keyword."""
    out = {}
    for p in probes:
        if p.keyword is not None and rules[p.rule]["gate"] == "g" and p.rule not in out:
            out[p.rule] = p
    return list(out.values())


def rule_gates(probes, rules, name="rule-gates"):
    """(c) For every gate_rules() probe, six times over: the sample without
    its keyword, the keyword alone, both -- adjacent tiny files, 0 to 2 empty
    files between them.  Only `both` may hold a candidate of the rule.
    note["both"]: {rule index: files}; None where the rule set has no such
    rule."""
    files, both = [], {}
    for p in gate_rules(probes, rules):
        want = both.setdefault(p.index, set())
        for t in range(6):
            for part, empties in ((p.base, t % 3), (p.keyword.encode(), (t + 1) % 3), (p.text, (t + 2) % 3)):
                if part is p.text:
                    want.add(len(files))
                files.append(b"\n" + part + b"\n" + EC.filler(t * 3, at=t))
                files.extend([b""] * empties)
    return EC.Corpus(name, files, note={"both": both}) if files else None


def corpora(ruleset, probes, rules):
    """The corpora of a rule set, named by it."""
    out = [rule_file_ends(probes, "rule-ends-%s" % ruleset), rule_phases(probes, "rule-phases-%s" % ruleset)]
    gates = rule_gates(probes, rules, "rule-gates-%s" % ruleset)
    return out + ([gates] if gates is not None else [])
