// pco_gfx_ranges.hip -- the entry points that decode PART of a wrapped page: pco_gfx_decompress_page_ranges (include/pco_gfx.h section 4d), its
// device-directory form pco_gfx_decompress_page_ranges_dir (4e), pco_gfx_decompress_page_reads (4f) and pco_gfx_index_pages (4g), which walks a
// prefix for its cursors alone; their _ex forms under PCO_GFX_CURSOR_GENERAL; pco_gfx_decompress_page_reads_hist (4i) and pco_gfx_index_pages_hist
// (4j) with a history reference per task; pco_gfx_decompress_page_reads_dir / pco_gfx_index_pages_dir (4k), those two behind 4e's device directory,
// and their standalone-chunk forms (4l); pco_gfx_scan_chunks (4m), which finds a standalone file's chunk directory; and pco_gfx_take_rows (4n), rows by device-resident row ids.
// A translation unit of its own, so that the kernels the whole-page entry points launch (pco_gfx.hip) are compiled exactly as before.  The kernels
// are in decode_range.hip, decode_resume.hip, decode_index.hip, decode_general.hip, dir_resolve.hip, scan.hip and take.hip.  The host side, as on the encode
// side, is in four includes: pco_partial_driver.inc (ONE driver for all the partial decodes: the request an entry point fills, the plan derived
// from it, the named steps), pco_partial_entry.inc (the extern "C" entry points and the one set of argument checks they share) and
// pco_scan_host.inc (pco_gfx_scan_chunks and its small driver); pco_take_entry.inc is pco_gfx_take_rows, which runs the driver over its segments.
#include "pco_host.h"
#include "pco_half.h"

#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "decode_resume.hip"   // (and, through it, decode_range.hip)
#include "decode_index.hip"
#include "decode_general.hip"
#include "dir_resolve.hip"
#include "scan.hip"
#include "take.hip"
#include "pco_launch.h"   // the timed launch, the LDS reservation, width_group / launch_width / flatten_groups, Layout, the scratch budget

static_assert(sizeof(PcoGfxPageCursor) == 8 * pcogfx::kCursorWords, "PcoGfxPageCursor");
static_assert(sizeof(PcoGfxPageRangeTask) == 72 && sizeof(PcoGfxPageReadTask) == 88, "PcoGfxPageReadTask: PcoGfxPageRangeTask, then the two cursors");
static_assert(sizeof(PcoGfxPageIndexTask) == 64, "PcoGfxPageIndexTask");
static_assert(sizeof(PcoGfxPageIndexHistTask) == 80, "PcoGfxPageIndexHistTask: PcoGfxPageIndexTask, then the histories");
static_assert(sizeof(PcoGfxPageReadHistTask) == 104 && PCO_GFX_HISTORY_HEADER_BYTES == pcogfx::kHistoryHeaderBytes, "PcoGfxPageReadHistTask: PcoGfxPageReadTask, then the history");
static_assert(sizeof(PcoGfxDirPageReadTask) == 80 && sizeof(PcoGfxDirPageIndexTask) == 56, "PcoGfxDirPageReadTask, PcoGfxDirPageIndexTask");
static_assert(sizeof(pcogfx::DirCursorPair) == sizeof(pcogfx::ReadRef) && offsetof(pcogfx::DirCursorPair, to) == offsetof(pcogfx::ReadRef, to), "dir_resolve_reads_kernel writes ReadRef's two words");
static_assert(sizeof(PcoGfxScanTask) == 48, "PcoGfxScanTask");
static_assert(sizeof(PcoGfxTakeTask) == 96 && offsetof(PcoGfxTakeTask, d_rows) == 64 && offsetof(PcoGfxTakeTask, dtype) == 88, "PcoGfxTakeTask");

#include "pco_partial_driver.inc"
#include "pco_partial_entry.inc"
#include "pco_scan_host.inc"
#include "pco_take_entry.inc"
