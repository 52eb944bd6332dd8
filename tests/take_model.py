"""A plain Python model of what pco_gfx_take_rows (include/pco_gfx.h section 4n) plans from a list of row ids: which segments of the page are walked,
the read task {first, count} of each, and the task's result (n_out, aux, consumed).  It restates pcodec_amd/csrc/pco_take.h line by line, and
MUTANTS are that arithmetic changed in one place: plan(..., mutant=m) must differ from plan(...) on the cases of tests/test_take_rows_abi.py, which is
how those cases are known to look at every line.

The shapes and id lists here are the ones the GPU tests use as well (tests/test_gpu_take_rows.py)."""
from collections import namedtuple

PAGE_NS = (1, 255, 256, 257, 1000, 2049, 70000)
EVERY_ROWS = (0, 256, 512, 4096)
ROW_BASES = (0, 1000003)

MUTANTS = ("boundary", "no_plus_one", "batch_floor", "row_base_ignored")
MUTANT_TEXT = {"boundary": "segment of a local row: (row - 1) / every_rows, so that row s * every_rows falls into segment s - 1",
               "no_plus_one": "a mark holds the largest wanted row, not the row + 1: count is one short (and row 0 leaves its segment unmarked)",
               "batch_floor": "batches = count / 256, not its ceiling",
               "row_base_ignored": "the local row is the id itself"}

Plan = namedtuple("Plan", "n_seg marks tasks n_out aux consumed local")   # marks / tasks per segment; local: per id its page row or None


def n_segments(page_n, every_rows):
    return 1 if every_rows == 0 else (page_n - 1) // every_rows + 1


def plan(page_n, every_rows, row_base, ids, mutant=None):
    assert mutant is None or mutant in MUTANTS
    n_seg = n_segments(page_n, every_rows)
    marks = [0] * n_seg
    local = []
    n_out = 0
    for rid in ids:
        base = 0 if mutant == "row_base_ignored" else row_base
        if rid < base or rid - base >= page_n:
            local.append(None)
            continue
        row = rid - base
        local.append(row)
        n_out += 1
        if every_rows == 0:
            s = 0
        elif mutant == "boundary":
            s = max(row - 1, 0) // every_rows
        else:
            s = row // every_rows
        marks[s] = max(marks[s], row if mutant == "no_plus_one" else row + 1)
    tasks = []
    aux = consumed = 0
    for s, m in enumerate(marks):
        first = s * every_rows
        count = 0 if m == 0 else m - first
        tasks.append((first, count))
        if m:
            aux += 1
            consumed += count // 256 if mutant == "batch_floor" else (count + 255) // 256
    return Plan(n_seg, marks, tasks, n_out, aux, consumed, local)


def id_lists(page_n, every_rows, row_base):
    """{name: [row ids]} for one page: the edges of the plan's arithmetic.  Ids are in the caller's numbering (row_base + the page's row)."""
    last = page_n - 1
    out = {"empty": [], "row0": [row_base], "last": [row_base + last], "first_and_last": [row_base, row_base + last]}
    edges = []
    if every_rows:
        for s in range(1, n_segments(page_n, every_rows)):
            edges += [s * every_rows - 1, s * every_rows]
    else:
        edges = [r for r in (254, 255, 256, 257, 511, 512) if r <= last]
    out["boundaries"] = [row_base + r for r in edges if r <= last]
    outside = [row_base + page_n, row_base + page_n + 255, (1 << 64) - 1]
    if row_base:
        outside += [row_base - 1, 0]
    out["outside"] = outside
    out["outside_and_inside"] = outside[:2] + [row_base + last] + outside[2:] + [row_base + min(256, last)]
    out["duplicates"] = [row_base + min(3, last)] * 5 + [row_base + last] * 3 + [row_base + min(3, last)]
    asc = sorted({0, min(1, last), last // 3, last // 2, min(255, last), min(256, last), last})
    out["reversed"] = [row_base + r for r in reversed(asc)]
    out["batch_edge"] = [row_base + r for r in (255, 256, 511) if r <= last] or [row_base]
    return out


def cases():
    """Every (page_n, every_rows, row_base, name, ids) of the model."""
    for page_n in PAGE_NS:
        for every_rows in EVERY_ROWS:
            for row_base in ROW_BASES:
                for name, ids in id_lists(page_n, every_rows, row_base).items():
                    yield page_n, every_rows, row_base, name, ids
