"""The task lists pcodec_amd.paged hands to the library, call by call and field by field, against tests/golden/paged_plans.json: the record of
paged.py as it was before its functions were built from one page source, one output allocation and one launch (tests/paged_plan_util.py says
how the record is made and what the stand-ins for torch and the library are).  Addresses follow allocation order, so the order of a call's
allocations is pinned with them."""
import json
import os

import pytest

import paged_plan_util as U
from pcodec_amd import build as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paged_plans.json")


@pytest.fixture(scope="module")
def plans():
    if B.needs_build():
        B.build()
    from pcodec_amd import paged
    return json.loads(json.dumps(U.record(paged))), json.load(open(GOLDEN))


def test_no_case_is_left_out(plans):
    got, want = plans
    assert sorted(got) == sorted(want) and len(want) >= 60
    assert os.path.getsize(GOLDEN) < 64 << 10
    assert {c["fn"] for case in want.values() for c in case["calls"]} == {
        "pco_gfx_compress_wrapped_chunks_ex", "pco_gfx_compact_wrapped_chunks", "pco_gfx_decompress_pages", "pco_gfx_decompress_page_ranges",
        "pco_gfx_decompress_pages_dir", "pco_gfx_decompress_page_ranges_dir", "pco_gfx_decompress_page_reads", "pco_gfx_index_pages"}


@pytest.mark.parametrize("case", sorted(json.load(open(GOLDEN))))
def test_calls_and_returned_tensors_match_the_record(plans, case):
    got, want = plans[0][case], plans[1][case]
    assert [c["fn"] for c in got["calls"]] == [c["fn"] for c in want["calls"]]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i} ({w['fn']}) of {case}"
    assert got["returned"] == want["returned"]


def test_the_stand_ins_leave_nothing_behind():
    import sys
    from pcodec_amd import paged
    before = sys.modules.get("torch"), paged._require_device
    U.record(paged)
    assert (sys.modules.get("torch"), paged._require_device) == before
