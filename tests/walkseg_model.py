"""enc_walkseg_kernel's schedule (pcodec_amd/csrc/encode_walkseg.hip) as a PLAIN MODEL: which batches of a long page are walked with both ends
of the arc of states, where each chain of each segment meets, what is walked again and in which round, and the words and final states that
come out.  Python and numpy; no code shared with oracle/.  pack_layout_model parses the chunk, tans_model spreads the symbols.

  * Table: a chunk's bins (weights, ans_size_log) -> per symbol next[state], bits[state], row_index[state] (ans/spec.rs:37-59 spread with
    stride (3 T / 5) | 1; ans/encoding.rs:65-87 one step: bits bring state >> bits into [weight, 2 weight), the row of next states ascends).
    States are kept as state - T.
  * The symbols of a page come from DECODING the oracle's chunk (decoder_nodes: the decoder's side of the table); the true walk ENCODES them
    again, four interleaved chains in reverse from T, and must arrive at the four states in the page's head with the batches' bit totals the
    layout model measured -- the pin to the oracle.
  * PageWalk.run(mutant) is the kernel's schedule, literally; run(None) must give the true walk.  MUTANTS are the kernel changed in one place.
    What a schedule gives is (words, final states, whether the chunk was failed): a row REVEALS an edge when a mutant's differs from the true one.

Under weights (T - 1, 1) a step of the heavy symbol emits no bit for all but the top two states: a wrong state shows in the words only at the
next rare symbol below it in its chain (weight 1: the word carries the whole state) or in the page's final states.  That is why rows are
judged by `reveals` and not by what they intend.

Every constant is read from the .hip sources: a moved constant fails this module."""
import collections
import functools
import os
import re

import numpy as np

import pack_layout_model as P
from tans_model import BATCH_N, decoder_nodes, spread_state_symbols

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcodec_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (what, found)
    return int(found.pop())


_F, _W, _K, _D = _read("encode_fast.hip"), _read("encode_walkseg.hip"), _read("encode_kernels.hip"), _read("pco_dev.h")
kWsSegs = _one(r"\bkWsSegs\s*=\s*(\d+)\s*,", _F, "kWsSegs")
kWsMinBatches = _one(r"\bkWsMinBatches\s*=\s*(\d+)\s*,", _F, "kWsMinBatches")
kWsMaxItems = _one(r"\bkWsMaxItems\s*=\s*(\d+)\s*;", _F, "kWsMaxItems")
kWsSkew = _one(r"\bkWsSkew\s*=\s*(\d+)\s*;", _W, "kWsSkew")
kWsSymBase = _one(r"\bkWsSymBase\s*=\s*(\d+)\s*,", _W, "kWsSymBase")
kBatchN = _one(r"\bkBatchN\s*=\s*(\d+)\s*;", _D, "kBatchN")
kDirectHistRange = _one(r"\bkDirectHistRange\s*=\s*(\d+)\s*;", _K, "kDirectHistRange")
kFastEncMaxAsl = _one(r"\bkFastEncMaxAsl\s*=\s*(\d+)\s*;", _K, "kFastEncMaxAsl")
kRunBatches = _one(r"\bkRunBatches\s*=\s*(\d+)\s*;", _F, "kRunBatches")   # enc_scan_kernel keeps the batches' prefix sums at every run start only
# the expressions the model restates, as the kernel writes them
assert re.search(r"nbs\s*=\s*\(\(\(nb \+ kWsSegs - 1\) / kWsSegs\) \| 1u\) \+ \(kWsSkew - 1\), n_seg = \(nb \+ nbs - 1\) / nbs;", _W), "the segment geometry moved"
assert re.search(r"ew_info_off\(uint32_t asl\) \{ return \(\(2u << asl\) \+ 7u\) & ~7u; \}", _F), "ew_info_off moved"
assert re.search(r"all_lds = finds && pv\.n_bins <= 256 && pv\.range < 4096 && vt_off \+ \(uint32_t\)pv\.range \+ 1u <= kWsSymBase;", _W), "all_lds moved"
assert kBatchN == BATCH_N

MUTANTS = ("a", "b", "c", "d", "e", "f", "g", "h")
MUTANT_TEXT = {"a": "fix_n >= my_nb becomes >", "b": "the quad-OR of open ORs pairs", "c": "no `all` reset", "d": "at most 4 rounds",
               "e": "the top segment starts with B = 2T - 1", "f": "up_ok per lane", "g": "nbs not made odd", "h": "no redo"}

Table = collections.namedtuple("Table", "asl T weights nxt bts ridx")


@functools.lru_cache(maxsize=64)
def table_of(asl, weights):
    """Per symbol three lists over state - T: next state - T, bits emitted, index into the symbol's row."""
    T = 1 << asl
    assert sum(weights) == T
    owner = np.array(spread_state_symbols(asl, list(weights)))
    stride = ((3 * T) // 5) | 1
    assert all(owner[(stride * k) % T] == 0 for k in range(weights[0])), "the spread's stride is not (3 T / 5) | 1"
    x = np.arange(T, 2 * T, dtype=np.int64)
    nxt, bts, ridx = [], [], []
    for s, w in enumerate(weights):
        row = np.flatnonzero(owner == s)                       # ascending: encoding.rs pushes table_size + state_idx in table order
        assert row.size == w
        bits = np.zeros(T, np.int64)
        for b in range(asl + 1):
            bits[((x >> b) >= w) & ((x >> b) < 2 * w)] = b
        idx = (x >> bits) - w
        assert (idx >= 0).all() and (idx < w).all()
        nxt.append(row[idx].tolist()); bts.append(bits.tolist()); ridx.append(idx.tolist())
    return Table(asl, T, tuple(weights), nxt, bts, ridx)


# ------------------------------------------------------------------------------------------------ a chunk's symbols, from its bytes
Decoded = collections.namedtuple("Decoded", "layout syms states")


def decode_symbols(chunk):
    """One standalone chunk -> (layout, per variable the symbols in page order or None, per variable the four states of the page's head)."""
    lay = P.parse_chunk(chunk)
    r = P.Reader(chunk); r.pos = lay.meta_end
    states = [None, None, None]
    for v in range(3):
        if not lay.present[v]: continue
        if v == 1: r.skip(lay.latent_bits * lay.state_n)
        states[v] = [r.read(lay.asl[v]) for _ in range(4)]
    data = bytes(chunk); syms = [None, None, None]
    for v in range(3):
        if not lay.present[v] or len(lay.bins[v]) < 2: continue
        nd = decoder_nodes(lay.asl[v], [b[0] for b in lay.bins[v]])
        sym_of = [n[0] for n in nd]; bits_of = [n[1] for n in nd]; base_of = [n[2] for n in nd]
        st = list(states[v]); out = []
        for row in lay.batches:
            if v not in row: continue
            pos = row[v].pos
            for i in range(len(row[v].widths)):
                j = i & 3; k = st[j]; b = bits_of[k]; q = pos >> 3
                out.append(sym_of[k])
                st[j] = base_of[k] + ((int.from_bytes(data[q:q + 4], "little") >> (pos & 7)) & ((1 << b) - 1))
                pos += b
            assert pos - row[v].pos == row[v].ans_bits
        assert len(out) == lay.n_lat[v]
        syms[v] = np.array(out, np.int32)
    return Decoded(lay, syms, states)


def wrapped_as_standalone(dtype_byte, n, meta, page):
    """A page of a wrapped chunk behind its ChunkMeta, in the shape of a standalone chunk (type byte, 24 bits of n - 1, meta, page)."""
    return bytes([dtype_byte]) + int(n - 1).to_bytes(3, "little") + bytes(meta) + bytes(page)


# ------------------------------------------------------------------------------------------------ geometry and sources
Geometry = collections.namedtuple("Geometry", "nb nbs n_seg segs")   # segs: [(first latent, latents, batches)]


def geometry(n_lat, odd=True):
    nb = (n_lat + kBatchN - 1) // kBatchN
    share = (nb + kWsSegs - 1) // kWsSegs
    nbs = (share | 1 if odd else share) + (kWsSkew - 1)
    n_seg = (nb + nbs - 1) // nbs
    segs = []
    for q in range(n_seg):
        first = q * nbs * kBatchN; nl = min(n_lat - first, nbs * kBatchN)
        segs.append((first, nl, (nl + kBatchN - 1) // kBatchN))
    assert n_seg <= kWsSegs and sum(s[1] for s in segs) == n_lat
    return Geometry(nb, nbs, n_seg, segs)


def is_long(n_lat, n_bins):
    """ws_walks: the variable has something to walk and at least kWsMinBatches batches."""
    return n_bins > 1 and n_lat >= kWsMinBatches * kBatchN


def info_off(asl): return ((2 << asl) + 7) & ~7


def vt_off(asl, n_bins): return info_off(asl) + 8 * n_bins + ((n_bins + 3) & ~3)


def source(compact, rng, asl, n_bins):
    """Where the walker's symbols come from: "finds" (the gathering wave looks 16-bit latents up by value), "all_lds" (finds, with the value
    table in the block's LDS), "stages" (the walker stages what enc_dissect_kernel wrote)."""
    if not (compact and rng < kDirectHistRange): return "stages"
    if n_bins <= 256 and rng < 4096 and vt_off(asl, n_bins) + rng + 1 <= kWsSymBase: return "all_lds"
    return "finds"


# ------------------------------------------------------------------------------------------------ the walks
SegEvent = collections.namedtuple("SegEvent", "fix_n my_nb whole_open met_in_last last_chain round resets_before resets_after met")
Outcome = collections.namedtuple("Outcome", "words finals error segs rounds longest_pending geom bat")


class PageWalk:
    """One (page, variable): its table and its symbols in page order."""

    def __init__(self, tab, syms):
        self.tab = tab; self.S = [int(s) for s in syms]; self.n = len(self.S)
        self._p1 = {}; self._true = None; self._runs = {}

    # ---- the reference's walk
    def true(self):
        """(words per latent, the four final states - T, tANS bits per batch)"""
        if self._true is None:
            t = self.tab; S = self.S; N, B = t.nxt, t.bts
            words = np.zeros(self.n, np.uint16); finals = []
            bb = np.zeros((self.n + kBatchN - 1) // kBatchN, np.int64)
            for j in range(4):
                a = 0; idx = range(j + ((self.n - 1 - j) // 4) * 4, j - 1, -4) if self.n > j else range(0)
                w = []
                for i in idx:
                    s = S[i]; bits = B[s][a]
                    w.append((bits << 12) | (a & ((1 << bits) - 1))); a = N[s][a]
                if w:
                    words[j::4] = w[::-1]
                finals.append(a)
            np.add.at(bb, np.arange(self.n) // kBatchN, words >> 12)
            self._true = (words, tuple(finals), bb)
        return self._true

    # ---- the first pass of one walker lane: both ends of the arc, batch after batch in walk order
    def _pass1(self, lo, nl, j, a, b, reset_on):
        key = (lo, nl, j, a, b, reset_on)
        if key in self._p1: return self._p1[key]
        t = self.tab; S = self.S; N, Bt, R = t.nxt, t.bts, t.ridx; top_state = t.T - 1
        my_nb = (nl + kBatchN - 1) // kBatchN
        A, Bs, res, words, meet, pb = [], [], [], [], None, []
        for it in range(my_nb):
            hb = my_nb - 1 - it
            start = hb * kBatchN; end = min(start + kBatchN, nl)
            A.append(a); Bs.append(b); r = 0; n0 = len(words)
            first = start + j
            idx = range(lo + first + ((end - 1 - first) // 4) * 4, lo + first - 1, -4) if first < end else range(0)
            if a != b and end - start == kBatchN:       # walk_batch2 (any lane open, and this one is; a full batch)
                for i in idx:
                    s = S[i]
                    if a != b:
                        rr = R[s]
                        if reset_on and b < a and rr[a] == rr[b]:
                            a = 0; b = top_state; r += 1
                        bits = Bt[s][a]; words.append((bits << 12) | (a & ((1 << bits) - 1)))
                        nn = N[s]; a = nn[a]; b = nn[b]
                        if a == b: meet = i
                    else:
                        bits = Bt[s][a]; words.append((bits << 12) | (a & ((1 << bits) - 1)))
                        a = N[s][a]; b = a
            else:                                       # walk_batch from st_a, then st_b = st_a
                for i in idx:
                    s = S[i]; bits = Bt[s][a]
                    words.append((bits << 12) | (a & ((1 << bits) - 1))); a = N[s][a]
                b = a
            res.append(r); pb.append(sum(w >> 12 for w in words[n0:]))
        A.append(a); Bs.append(b)
        out = (A, Bs, res, np.array(words[::-1], np.uint16), meet, pb)
        self._p1[key] = out
        return out

    def _walk_batch_from(self, buf, cnt, j, state):
        """walk_batch of chain j over the `cnt` symbols in a segment's LDS buffer (indexed by the latent's place in its batch): (state, words
        in page order, bits)."""
        N, Bt = self.tab.nxt, self.tab.bts
        a = state; w = []
        if j < cnt:
            for i in range(j + ((cnt - 1 - j) // 4) * 4, j - 1, -4):
                s = buf[i]; bits = Bt[s][a]
                w.append((bits << 12) | (a & ((1 << bits) - 1))); a = N[s][a]
        return a, w[::-1], sum(x >> 12 for x in w)

    # ---- the kernel's schedule
    def run(self, mutant=None):
        if mutant in self._runs: return self._runs[mutant]
        assert mutant is None or mutant in MUTANTS
        t = self.tab; T = t.T
        g = geometry(self.n, odd=mutant != "g")
        reset_on = mutant != "c"
        words = np.zeros(self.n, np.uint16); bat = np.zeros(g.nb, np.int64)
        fix = [[0] * 4 for _ in range(kWsSegs)]; st_met = [[0] * 4 for _ in range(kWsSegs)]
        st_a = [[0] * 4 for _ in range(kWsSegs)]; exact = [[1] * 4 for _ in range(kWsSegs)]
        info = []
        for q, (lo, nl, nbq) in enumerate(g.segs):
            top = q + 1 == g.n_seg
            b0 = 0 if top and mutant != "e" else T - 1
            lanes = [self._pass1(lo, nl, j, 0, b0, reset_on) for j in range(4)]
            met_seen = [False] * 4
            for j in range(4):
                words[lo + j: lo + nl: 4] = lanes[j][3]
            for it in range(nbq):                        # (the quad's sum, written by lane 0)
                bat[lo // kBatchN + nbq - 1 - it] = sum(lanes[j][5][it] for j in range(4))
            for it in range(nbq):
                op = [lanes[j][0][it] != lanes[j][1][it] for j in range(4)]
                for j in range(4):
                    qo = (op[j] or op[j ^ 1]) if mutant == "b" else any(op)
                    fix[q][j] += 1 if qo else 0
                    if not qo and not met_seen[j]:
                        st_met[q][j] = lanes[j][0][it]; met_seen[j] = True
            for j in range(4):
                st_a[q][j] = lanes[j][0][-1]; exact[q][j] = 1 if lanes[j][0][-1] == lanes[j][1][-1] else 0
            meets = [lanes[j][4] for j in range(4)]
            open_at = [[lanes[j][0][it] != lanes[j][1][it] for j in range(4)] for it in range(nbq)]
            quad_fix = sum(any(o) for o in open_at)
            info.append(dict(fix_n=quad_fix, my_nb=nbq, meets=meets, met=all(exact[q]), open0=open_at[0] if open_at else [False] * 4,
                             before=sum(sum(lanes[j][2][:quad_fix]) for j in range(4)), after=sum(sum(lanes[j][2][quad_fix:]) for j in range(4))))
        ex_state = [list(r) for r in st_a]; ex_exact = [list(r) for r in exact]
        lds = []                                         # per segment the two symbol buffers as the first pass leaves them: its batches 0 and 1
        for lo, nl, nbq in g.segs:
            lds.append([(self.S[lo + p * kBatchN: min(lo + (p + 1) * kBatchN, lo + nl)] + [0] * kBatchN)[:kBatchN] if p < nbq else [0] * kBatchN for p in range(2)])
        pending = [[fix[q][j] != 0 for j in range(4)] for q in range(kWsSegs)]
        first_pending = [any(p) for p in pending]
        redone = [None] * kWsSegs
        error = False; rounds = 0
        limit = 0 if mutant == "h" else 4 if mutant == "d" else kWsSegs
        for rnd in range(limit):
            if not any(any(p) for p in pending): break
            rounds += 1
            plan = []
            for q in range(kWsSegs):
                up = q + 1 if q + 1 < kWsSegs else q
                ok = [ex_exact[up][j] if pending[q][j] else 1 for j in range(4)]
                for j in range(4):
                    up_ok = ok[j] if mutant == "f" else min(ok)
                    if pending[q][j] and up_ok:
                        plan.append((q, j, ex_state[up][j]))
            # One wave in lockstep: every lane has read the exits above before any is written.  The symbols of a batch walked again come from
            # the segment's two LDS buffers, which the lanes that are ON refill from the scratch, a quarter (64 latents) each: a quad whose
            # lanes disagree walks whatever the other quarters still hold.
            state_of = {(q, j): st for q, j, st in plan}
            for it in range(max((fix[q][j] for q, j, _ in plan), default=0)):
                for q in sorted({q for q, _, _ in plan}):
                    lo, nl, nbq = g.segs[q]
                    on = [j for j in range(4) if (q, j) in state_of and it < fix[q][j]]
                    if not on: continue
                    hb = nbq - 1 - it; base = lo + hb * kBatchN; cnt = min(kBatchN, nl - hb * kBatchN)
                    buf = lds[q][hb & 1]
                    for j in on:
                        buf[64 * j: 64 * j + 64] = (self.S[base + 64 * j: base + 64 * j + 64] + [0] * 64)[:64]
                    total = {}
                    for j in on:
                        state_of[(q, j)], w, total[j] = self._walk_batch_from(buf, cnt, j, state_of[(q, j)])
                        words[base + j: base + cnt: 4] = w
                    if 0 in total: bat[lo // kBatchN + hb] = sum(total.values())   # (lane 0 writes the quad's sum; a lane that is off adds nothing)
            for q, j, _ in plan:
                nbq = g.segs[q][2]; state = state_of[(q, j)]
                if (fix[q][j] > nbq) if mutant == "a" else (fix[q][j] >= nbq): st_a[q][j] = state
                elif state != st_met[q][j]: error = True
                ex_state[q][j] = st_a[q][j]; ex_exact[q][j] = 1; pending[q][j] = False
                if redone[q] is None: redone[q] = rnd
        segs = []
        for q, d in enumerate(info):
            ms = d["meets"]
            never = [j for j in range(4) if ms[j] is None and d["open0"][j]]
            order = sorted((m, j) for j, m in enumerate(ms) if m is not None)
            last = None if d["fix_n"] == 0 or len(never) > 1 else never[0] if never else order[0][1] if order else None   # (the walk runs downwards: the smallest index met last)
            segs.append(SegEvent(d["fix_n"], d["my_nb"], d["fix_n"] == d["my_nb"], d["fix_n"] == d["my_nb"] and d["met"], last, redone[q],
                                 d["before"], d["after"], d["met"]))
        run_len = longest = 0
        for q in range(g.n_seg):
            run_len = run_len + 1 if first_pending[q] else 0
            longest = max(longest, run_len)
        out = Outcome(words, tuple(st_a[0]), error, tuple(segs), rounds, longest, g, bat)
        self._runs[mutant] = out
        return out

    def reveals(self, mutant):
        """Whether the mutant's output differs from the true one in what the page shows: a word, a final state, a chunk failed, or the
        batches' bit totals where enc_scan_kernel keeps them -- as the prefix sum at every run of kRunBatches batches and the page's total
        (inside a run the packer places the fields by the words' own bit counts: two wrong totals that cancel within a run change no byte)."""
        w, f, bb = self.true(); o = self.run(mutant)
        return o.error or o.finals != f or not np.array_equal(o.words, w) or shown_totals(o.bat) != shown_totals(bb)


def shown_totals(bat):
    c = np.concatenate([[0], np.cumsum(bat)])
    return c[::kRunBatches].tolist() + [int(c[-1])]


def page_walks(chunk):
    """{variable: PageWalk} for the variables of a standalone chunk that enc_walkseg_kernel walks, and what decode_symbols found."""
    d = decode_symbols(chunk)
    out = {}
    for v in range(3):
        if d.syms[v] is not None and is_long(d.layout.n_lat[v], len(d.layout.bins[v])) and d.layout.asl[v] <= kFastEncMaxAsl and len(d.layout.bins[v]) <= 256:
            out[v] = PageWalk(table_of(d.layout.asl[v], tuple(b[0] for b in d.layout.bins[v])), d.syms[v])
    return out, d


def pinned_to_oracle(walk, decoded, v):
    """The true walk against the oracle's chunk: the page's four states, and every batch's tANS bit total.  Returns a list of complaints."""
    w, finals, bb = walk.true(); bad = []
    if list(finals) != list(decoded.states[v]): bad.append(f"final states {finals}, the page's head holds {decoded.states[v]}")
    want = [row[v].ans_bits for row in decoded.layout.batches if v in row]
    if bb.tolist() != want:
        k = next(i for i, (x, y) in enumerate(zip(bb.tolist(), want)) if x != y) if len(want) == bb.size else -1
        bad.append(f"tANS bits of batch {k}: differ from the chunk's")
    return bad


# ------------------------------------------------------------------------------------------------ brute force (small tables)
def brute_arc_check(tab, syms_desc, a=0, b=None, reset_on=True):
    """The model's arc over `syms_desc` (symbols in walk order) beside ALL T trajectories: every reachable state lies on the arc, and when the
    ends are equal every start has reached that state.  Returns (step at which they met or None, resets)."""
    T = tab.T; b = T - 1 if b is None else b
    states = np.arange(T); resets = 0
    for k, s in enumerate(syms_desc):
        nn = np.array(tab.nxt[s]); rr = tab.ridx[s]
        states = np.unique(nn[states])
        if a != b:
            if reset_on and b < a and rr[a] == rr[b]: a, b = 0, T - 1; resets += 1
            a, b = tab.nxt[s][a], tab.nxt[s][b]
        else:
            a = b = tab.nxt[s][a]
        on = (states >= a) & (states <= b) if a <= b else (states >= a) | (states <= b)
        assert on.all(), ("a trajectory left the arc", k, a, b)
        if a == b:
            assert states.size == 1 and int(states[0]) == a, ("the ends met before every trajectory had", k)
            return k, resets
    return None, resets
