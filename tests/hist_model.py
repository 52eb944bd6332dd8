"""A plain model of the encoder's unoptimized histogram (histograms.rs), written from the reference's text and from the header comment of K2
in pcodec_amd/csrc/encode_kernels.hip, on the SORTED MULTISET of a variable's latents.  Python integers and bisect; it shares no code with
the library.

The builder is the reference's: n_applied, next_avail (next_avail_bin_idx), the incomplete bin, bin_idx(c) = floor(c * B / n) and
c_count(b) = ceil((b + 1) * n / B).  The rule is what apply_quicksort_recurse comes to once every partition has been made: standing at rank
pos = n_applied, with target = bin_idx(pos) and c = c_count(target), take the run [st, en) of the value at rank c - 1.

  * en <= c: every run in [pos, c) ends by c.  Absorb the ranks up to c into the incomplete bin and complete the target bin.
  * otherwise the run straddles c: apply the prefix [pos, st) to the incomplete bin, then apply_constant_run on [st, en): the bin of the
    run's middle, the spare-bin rule (if that bin is beyond next_avail, either complete what is pending in the bin before it -- "spare
    completed" -- or, with nothing pending, move the run into it -- "spare taken"), and completion iff en >= c_count(bin).

apply_sorted, which the reference reaches only behind its heapsort branch, differs in ONE point: it treats the run at rank c - 1 as a constant
run whether or not it straddles c (unless c is the end of the data).  That is the variant `sorted_rule`.

Besides the bins, histogram() returns a Report: how often each branch of the rule was taken (REPORT), the largest number of bins a run
skipped, whether the one-thread-per-bin shortcut of hist_emit applies (n >= B and no run straddles any c_count(b)), and -- for a variable of
more than `window` (256) bins, which the device walks a window at a time -- per window its kind ("simple": entered clean and nothing
straddles, one thread per bin; "walked"; "skipped": never entered, a run carried the walk past it) and whether a pending bin or a straddling
run crossed its start.

`variants` (names from VARIANTS) switches one comparison to a plausible wrong one.  The tests use them ONLY to prove that a case stands on
the comparison it names: a case whose bins do not change under its variant tests nothing.

One of the issue's variants cannot change a bin, and tests/test_hist_model.py proves it by exhaustion on small inputs rather than naming a
case for it: `window_clean_ignores_pending`.  A window is clean when nothing is pending AND the walk stands exactly on c_count(wb - 1) AND
n >= B.  A bin is left pending only by a run with en < c_count(b), where b <= bin_idx(middle) <= bin_idx(en - 1); with en == c_count(wb - 1)
that gives b <= wb - 1, so c_count(b) <= en and the run completes.  Pending and "on the window's first rank" exclude one another, so the
position check alone already refuses every window that is entered with a pending bin.  The variant that does matter is the other half,
`window_clean_ignores_pos`."""
import bisect
import collections

import numpy as np

VARIANTS = ("absorb_strict", "sorted_rule", "mid_rounds_up", "bin_of_start", "spare_never", "spare_always", "complete_strict", "c_count_floor",
            "shortcut_below_B", "window_clean_ignores_pending",
            # beyond the issue's list: the half of the window's `clean` that can change a bin (see above)
            "window_clean_ignores_pos")
EQUIVALENT_VARIANTS = ("window_clean_ignores_pending",)
REPORT = ("absorb", "absorb_run_ends_at_c", "prefix", "spare_completed", "spare_taken", "no_spare", "joins_pending", "completes_beyond",
          "completes_at_equality", "left_pending")
WINDOW_KINDS = ("simple", "walked", "skipped")
WINDOW = 256

Window = collections.namedtuple("Window", "kind pending_crossed run_crossed")


class Report:
    def __init__(self):
        self.counts = collections.Counter()
        self.steps = []            # (branch names, run start, run end, bin) of every step, in order
        self.max_skipped = 0
        self.shortcut = False
        self.windows = []          # [Window] when B > window, else []

    def hit(self, names, st, en, b):
        for nm in names:
            assert nm in REPORT, nm
            self.counts[nm] += 1
        self.steps.append((tuple(names), st, en, b))

    def step_of(self, st):
        """The step whose run begins at rank st: (branch names, st, en, the bin the run was put in or the target bin of an absorb)."""
        found = [x for x in self.steps if x[1] == st]
        return found[0] if found else None


def _variants(variants):
    v = frozenset(variants or ())
    assert v <= set(VARIANTS), v - set(VARIANTS)
    return v


def bin_idx(c, n, bins_log):
    return (int(c) << bins_log) // int(n)


def c_count(b, n, bins_log, floor=False):
    """ceiling of (b + 1) * n / B"""
    B = 1 << bins_log
    return ((int(b) + 1) * int(n) + (0 if floor else B - 1)) >> bins_log


class Builder:
    """HistogramBuilder: apply_incomplete with tight bounds, complete_bin."""

    def __init__(self, n, bins_log):
        self.n, self.bins_log = n, bins_log
        self.n_applied, self.next_avail, self.incomplete, self.dst = 0, 0, None, []

    def apply_incomplete(self, count, lower, upper):
        if count == 0:
            return
        if self.incomplete is not None:
            self.incomplete[0] += count; self.incomplete[2] = upper
        else:
            self.incomplete = [count, lower, upper]
        self.n_applied += count

    def complete_bin(self, b):
        if self.incomplete is None:
            return False
        self.next_avail = b + 1
        self.dst.append(tuple(self.incomplete)); self.incomplete = None
        return True


def shortcut_applies(s, bins_log):
    """hist_emit's `simple`: n >= B and ren[b] <= c_count(b) for every bin b."""
    n = len(s); B = 1 << bins_log
    if n < B:
        return False
    return all(bisect.bisect_right(s, s[c_count(b, n, bins_log) - 1]) <= c_count(b, n, bins_log) for b in range(B))


def histogram(latents, bins_log, variants=(), window=WINDOW):
    """(bins [(count, lower, upper)], Report) of the multiset `latents` at 2^bins_log bins."""
    return histogram_sorted(sorted(int(x) for x in np.asarray(latents).ravel().tolist()), bins_log, variants, window)


def histogram_sorted(s, bins_log, variants=(), window=WINDOW):
    """The same from the sorted list of Python integers."""
    V = _variants(variants)
    n = len(s); B = 1 << bins_log
    rep = Report()
    if n == 0:
        return [], rep
    floor = "c_count_floor" in V

    def cc(b):
        return c_count(b, n, bins_log, floor)

    def bi(c):
        return bin_idx(c, n, bins_log)

    rep.shortcut = shortcut_applies(s, bins_log)
    st8 = Builder(n, bins_log)

    def fits(b):                      # the run at the last rank of bin b ends by c_count(b)
        c = min(max(cc(b), 1), n)
        return bisect.bisect_right(s, s[c - 1]) <= c

    def step():
        pos = st8.n_applied
        target = bi(pos); c = cc(target)
        if c <= pos: c = pos + 1      # (only under c_count_floor, whose bin ends can fall on pos itself: keep the walk moving)
        c = min(c, n)
        v = s[c - 1]
        st = max(bisect.bisect_left(s, v), pos); en = bisect.bisect_right(s, v)
        if "sorted_rule" in V: absorb = c >= n
        elif "absorb_strict" in V: absorb = en < c
        else: absorb = en <= c
        if absorb:
            st8.apply_incomplete(c - pos, s[pos], v)
            st8.complete_bin(target)
            rep.hit(("absorb", "absorb_run_ends_at_c") if en == c and en - st >= 2 else ("absorb",), st, en, target)
            return
        names = []
        if st > pos:
            st8.apply_incomplete(st - pos, s[pos], s[st - 1]); names.append("prefix")
        length = en - st
        mid = st + ((length + 1) // 2 if "mid_rounds_up" in V else length // 2)
        b = bi(st) if "bin_of_start" in V else bi(min(mid, n - 1) if "mid_rounds_up" in V else mid)
        spare = b >= 1 if "spare_always" in V else (False if "spare_never" in V else b > st8.next_avail)
        if spare:
            if st8.complete_bin(b - 1): names.append("spare_completed")
            else: b -= 1; names.append("spare_taken")
        else:
            names.append("no_spare")
        if st8.incomplete is not None: names.append("joins_pending")
        st8.apply_incomplete(length, v, v)
        done = en > cc(b) if "complete_strict" in V else en >= cc(b)
        if done:
            st8.complete_bin(b)
            names.append("completes_at_equality" if en == cc(b) else "completes_beyond")
            rep.max_skipped = max(rep.max_skipped, (bi(en) if en < n else B) - (b + 1))
        else:
            names.append("left_pending")
        rep.hit(names, st, en, b)

    if B <= window:
        if "shortcut_below_B" in V and n < B and all(fits(b) for b in range(B)):
            # the one-thread-per-bin shortcut taken with fewer latents than bins: bin b = ranks [c_count(b - 1), c_count(b)), empty ones included
            for b in range(B):
                c0, c1 = (0 if b == 0 else cc(b - 1)), cc(b)
                st8.dst.append((c1 - c0, s[0] if b == 0 else s[min(c0, n - 1)], s[c1 - 1]))
            return st8.dst, rep
        while st8.n_applied < n:
            step()
        assert st8.incomplete is None, "the last run always completes: c_count(B - 1) == n"
        return st8.dst, rep

    for wb in range(0, B, window):
        wn = min(window, B - wb)
        pos = st8.n_applied
        first = 0 if wb == 0 else cc(wb - 1)
        pending = st8.incomplete is not None
        all_fit = all(fits(b) for b in range(wb, wb + wn))
        truly_clean = not pending and n >= B and pos == first
        clean = ((not pending) or "window_clean_ignores_pending" in V) and (n >= B or "shortcut_below_B" in V) and (pos == first or "window_clean_ignores_pos" in V)
        entered = pos < n and bi(pos) < wb + wn
        kind = "simple" if truly_clean and all_fit else ("walked" if entered else "skipped")
        rep.windows.append(Window(kind, pending, pos > first))
        if clean and all_fit and not (truly_clean and all_fit):
            # a window taken for simple that is not: one thread per bin writes bin b = ranks [c_count(b - 1), c_count(b)) behind what was
            # emitted so far, and the walk is put on c_count(wb + wn - 1) with whatever was pending still pending
            for b in range(wb, wb + wn):
                c0, c1 = (0 if b == 0 else cc(b - 1)), cc(b)
                st8.dst.append((c1 - c0, s[min(pos, n - 1)] if b == wb else s[min(c0, n - 1)], s[c1 - 1]))
            st8.n_applied = cc(wb + wn - 1); st8.next_avail = wb + wn
            continue
        while st8.n_applied < n and bi(st8.n_applied) < wb + wn:
            step()
    if st8.incomplete is not None:    # (only a wrong variant leaves one)
        st8.dst.append(tuple(st8.incomplete))
    return st8.dst, rep


def known_answers():
    """histograms.rs test_histogram_quicksort, as (latents, bins_log, bins); the shuffles are the caller's."""
    out = [([], 2, []), ([8], 0, [(1, 8, 8)]),
           (list(range(100)), 2, [(25, 0, 24), (25, 25, 49), (25, 50, 74), (25, 75, 99)]),
           ([1] + [0] * 99, 2, [(99, 0, 0), (1, 1, 1)]),
           ([0] + [1] * 99, 2, [(1, 0, 0), (99, 1, 1)]),
           ([3, 7, 7] + [5] * 97, 2, [(1, 3, 3), (97, 5, 5), (2, 7, 7)]),
           ([3, 7, 7] + [5] * 97, 1, [(98, 3, 5), (2, 7, 7)]),
           ([3, 3, 7] + [5] * 97, 1, [(2, 3, 3), (98, 5, 7)])]
    return out
