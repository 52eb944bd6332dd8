"""Build libpco_gfx.so (HIP, gfx950 only) in-tree.  `python -m pcodec_amd.build`."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpco_gfx.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
         "-Wno-unused-result",
         "-Wno-pass-failed"]   # (hipcc refuses a few `#pragma unroll` requests inside the lookback and select kernels' data-dependent loops: measured kernels, the warnings say nothing new)


def sources():
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [os.path.join(HERE, "..", "include", "pco_gfx.h")]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(s) > t for s in sources())


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    # two translation units: the library, and the entry points that decode part of a page -- pco_gfx_decompress_page_ranges[_dir],
    # pco_gfx_decompress_page_reads[_hist, _dir], pco_gfx_index_pages[_hist, _dir] and their standalone-chunk forms -- with the range, resume and index forms of the decode kernels (pco_gfx_ranges.hip, which
    # includes decode_range.hip, decode_resume.hip, decode_index.hip and decode_general.hip, scan.hip for pco_gfx_scan_chunks and take.hip for pco_gfx_take_rows, and whose host code is in pco_partial_driver.inc,
    # pco_partial_entry.inc, pco_scan_host.inc and pco_take_entry.inc); dir_resolve.hip is included by both.  sources() lists every file of csrc/
    cmd = [HIPCC] + FLAGS + [os.path.join(CSRC, "pco_gfx.hip"), os.path.join(CSRC, "pco_gfx_ranges.hip"), "-o", LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
