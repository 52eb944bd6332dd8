"""The text of every refusal the partial-decode entry points make on the host, against tests/golden/partial_messages.json.

The *_abi.py tests pin the status codes of the host checks and the order they fire in; the text pco_gfx_last_error() returns is pinned here.  Every
refused call those tests enumerate -- their case lists are imported, not restated -- runs through their own `call` helpers, and (return code, status,
message) must be the recorded triple.  The checks run before a device is asked for, so nothing here needs one.

Covered: pco_gfx_decompress_page_ranges[_dir], pco_gfx_decompress_page_reads[_ex, _hist, _dir], pco_gfx_index_pages[_ex, _hist, _dir],
pco_gfx_decompress_chunk_reads_dir, pco_gfx_index_chunks_dir and pco_gfx_scan_chunks: the entry points of the pco_gfx_ranges.hip translation unit.

The golden file is a recording: `python tests/test_partial_messages.py` rewrites it (do that only with a library whose messages are known to be the
intended ones, and say in the commit why they changed)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import test_chunk_directory_abi as CDA  # noqa: E402
import test_general_cursors_abi as GA  # noqa: E402
import test_lookback_history_abi as HA  # noqa: E402
import test_lookback_index_abi as LIA  # noqa: E402
import test_page_directory_abi as DA  # noqa: E402
import test_page_index_abi as IA  # noqa: E402
import test_page_ranges_abi as RA  # noqa: E402
import test_page_reads_abi as A  # noqa: E402
import test_page_reads_dir_abi as RDA  # noqa: E402
import test_scan_abi as SA  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "partial_messages.json")
FORMS = ("sync", "async")
FLAGS = (0, 1)
UNKNOWN_FLAGS = (2, 0xFFFFFFFF)
NO_RESULTS_NO_TASKS = dict(n_tasks=0, no_results=True)   # (section 4e: the _dir forms refuse it, the pointer forms do not)


def _range_cases():
    """test_page_ranges_abi keeps its rows in the parametrize mark and its good task in the test's body: the read task's, without the cursors"""
    mark = next(m for m in RA.test_argument_checks_come_before_anything_else.pytestmark if m.name == "parametrize")
    good = {k: v for k, v in A.GOOD_TASK.items() if k not in ("from_", "to")}
    return [(kw, lambda kw=kw: RA.call(G.PageRangeTask(**dict(good, **kw)))) for kw, _ in mark.args[1]]


def cases():
    """{id: a function that makes the refused call}; the id names the entry point, the flags, the form and the case's keywords"""
    out = {}

    def add(entry, flags, form, kw, fn):
        key = f"{entry} flags={flags} {form} {json.dumps(kw, sort_keys=True)}"
        assert key not in out, key
        out[key] = fn

    for kw, fn in _range_cases():
        add("page_ranges", "-", "sync", kw, fn)
    for kw, _ in DA.COMMON + DA.RANGES_ONLY:
        add("page_ranges_dir", "-", "sync", kw, lambda kw=kw: DA.call(True, **kw))
    for kw, _ in A.CHECKS:
        add("page_reads", "-", "sync", kw, lambda kw=kw: A.call(**kw))
    for kw, _ in IA.CHECKS:
        add("index_pages", "-", "sync", kw, lambda kw=kw: IA.call(**kw))
    for flags in FLAGS + UNKNOWN_FLAGS:
        for kw, _ in (A.CHECKS if flags in FLAGS else [({}, 0)]):
            add("page_reads_ex", flags, "sync", kw, lambda kw=kw, flags=flags: GA.call_reads(flags, **kw))
        for kw, _ in (GA.INDEX_CHECKS if flags in FLAGS else [({}, 0)]):
            add("index_pages_ex", flags, "sync", kw, lambda kw=kw, flags=flags: GA.call_index(flags, **kw))
        for form in FORMS:
            for kw, _ in (A.CHECKS + HA.HISTORY_CHECKS if flags in FLAGS else [({}, 0)]):
                add("page_reads_hist", flags, form, kw, lambda kw=kw, flags=flags, form=form: HA.call_hist(flags, form=form, **kw))
            for kw, _ in (IA.CHECKS + LIA.HISTORY_CHECKS if flags in FLAGS else [({}, 0)]):
                add("index_pages_hist", flags, form, kw, lambda kw=kw, flags=flags, form=form: LIA.call_hist(flags, form=form, **kw))
            for mod, word, rows in ((RDA, "page", RDA.CASES), (CDA, "chunk", [c for c in CDA.CASES if c[0] != "page"])):
                if flags in FLAGS:
                    rows = [(kind, kw) for kind, kw, _ in rows] + [(kind, NO_RESULTS_NO_TASKS) for kind in ("read", "index")]
                else:   # (an unknown flag is refused in front of a missing directory and a null task array)
                    rows = [(kind, kw) for kind in ("read", "index") for kw in ({}, dict(no_dir=True), dict(no_tasks=True))]
                for kind, kw in rows:
                    add(f"{word}_{kind}_dir", flags, form, kw, lambda mod=mod, kind=kind, kw=kw, flags=flags, form=form: mod.call(kind, flags, form, **kw))
    for form in FORMS:
        for _, kw, _ in SA.CHECKS:
            add("scan_chunks", "-", form, kw, lambda kw=kw, form=form: SA.call(G.lib(), form, kw))
            add("scan_chunks second task", "-", form, kw, lambda kw=kw, form=form: SA.call(G.lib(), form, None, n_tasks=2, second=kw))
        for kw in (dict(no_tasks=True, no_results=True), dict(no_results=True), dict(n_tasks=0, no_results=True)):
            add("scan_chunks", "-", form, kw, lambda kw=kw, form=form: SA.call(G.lib(), form, dict(src=None), **kw))
    return out


CASES = cases()


def triple(fn):
    """(return code, status, message) of one refused call"""
    code, status = fn()[:2]
    return [int(code), int(status), (G.lib().pco_gfx_last_error() or b"").decode()]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones(golden):
    assert set(CASES) == set(golden)
    assert len({k.split(" ")[0] for k in CASES}) == 13 and len(CASES) > 500


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_refusal_is_the_recorded_one(golden, key):
    got = triple(CASES[key])
    assert got[0] == G.PcoDecompressionError and got[2], got   # (every case IS a refusal with a message)
    assert got == golden[key]


def test_the_recording_names_every_entry_point_s_words(golden):
    """each entry point words its refusals its own way; a recording in which one took another's words would pin nothing"""
    words = {"page_ranges": "page range", "page_ranges_dir": "page range", "page_reads": "page read", "page_reads_ex": "page read", "page_reads_hist": "page read",
             "index_pages": "page index", "index_pages_ex": "page index", "index_pages_hist": "page index", "page_read_dir": "page read", "page_index_dir": "page index",
             "chunk_read_dir": "chunk read", "chunk_index_dir": "chunk index", "scan_chunks": "scan"}
    for key, (_, _, msg) in golden.items():
        assert words[key.split(" ")[0]] in msg, (key, msg)
    assert any("with histories: unknown flags" in m for _, _, m in golden.values()) and any("directory: results and d_results are both null" in m for _, _, m in golden.values())


if __name__ == "__main__":   # the recorder
    rec = {key: triple(fn) for key, fn in CASES.items()}
    bad = {k: v for k, v in rec.items() if v[0] != G.PcoDecompressionError or not v[2]}
    assert not bad, bad
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} refusals into {out}")
