"""pcodec_amd.paged without a GPU: what each of its functions would hand to libpco_gfx.so, as data.

Building a page-task list is arithmetic over the directory and the addresses torch hands out, so it runs under two stand-ins: a `torch` module
whose tensors carry an address, a shape and a dtype name (addresses are handed out in allocation order), and a library that records every call
-- the entry point, n_tasks, the task array field by field, the PcoGfxDirectory of the _dir forms, the scalar arguments -- and launches nothing.
The three host-only size functions compress_chunks needs go to the real library.  record() runs the case list and returns the calls and the
tensors each case returned; tests/golden/paged_plans.json is that record, made with pcodec_amd/paged.py as it was before its functions were
built from shared pieces (python tests/paged_plan_util.py <out.json>, with that paged.py on the path), and tests/test_paged_plans.py compares."""
import contextlib
import ctypes as C
import json
import sys
import types

BASE, GRAIN, STREAM_HANDLE = 1 << 40, 512, 0x5151   # (addresses beyond 32 bits: a pointer cut to an int shows)
WIDTHS = {"uint8": 1, "int8": 1, "uint16": 2, "int16": 2, "float16": 2, "uint32": 4, "int32": 4, "float32": 4, "uint64": 8, "int64": 8, "float64": 8}


class FakeDtype:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "torch." + self.name


class FakeTensor:
    is_cuda = True

    def __init__(self, addr, shape, dtype):
        self._addr, self.shape, self.dtype = addr, tuple(shape), dtype

    def data_ptr(self):
        return self._addr

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def __getitem__(self, key):   # t[a:b] of a 1-D tensor
        assert isinstance(key, slice) and key.step is None and len(self.shape) == 1
        a, b, _ = key.indices(self.shape[0])
        return FakeTensor(self._addr + a * WIDTHS[self.dtype.name], (max(b - a, 0),), self.dtype)

    def view(self, dtype):
        n_bytes = self.numel() * WIDTHS[self.dtype.name]
        assert len(self.shape) == 1 and n_bytes % WIDTHS[dtype.name] == 0
        return FakeTensor(self._addr, (n_bytes // WIDTHS[dtype.name],), dtype)

    def describe(self):
        return [self._addr - BASE, list(self.shape), self.dtype.name]


class FakeStream:
    cuda_stream = STREAM_HANDLE

    def synchronize(self):
        pass


class FakeTorch(types.ModuleType):
    """The part of torch that pcodec_amd.paged touches.  Every allocation gets the next address, GRAIN-aligned, so that addresses are a function
    of the order and the sizes of a call's allocations."""

    def __init__(self):
        super().__init__("torch")
        self._next = BASE
        for name in WIDTHS:
            setattr(self, name, FakeDtype(name))
        self.cuda = types.SimpleNamespace(current_stream=FakeStream, stream=lambda s: contextlib.nullcontext())

    def _alloc(self, shape, dtype=None, device=None):
        assert device == "cuda"
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        t = FakeTensor(self._next, shape, dtype)
        self._next += (t.numel() * WIDTHS[dtype.name] + GRAIN) // GRAIN * GRAIN
        return t

    empty = zeros = _alloc

    def tensor_of(self, n, name):
        """A caller's 1-D device tensor of n numbers."""
        return self._alloc(n, dtype=getattr(self, name), device="cuda")


def _int(x):
    return getattr(x, "value", x)


def _fields(struct):
    """A task or a directory field by field, pointers as integers or None.  The structs are scalars without padding, so this is their bytes."""
    assert sum(C.sizeof(t) for _, t in struct._fields_) == C.sizeof(struct)
    return [getattr(struct, name) for name, _ in struct._fields_]


class FakeLib:
    """Records what the library is called with.  `calls` is the record."""
    FORWARDED = ("pco_gfx_wrapped_chunk_cap", "pco_gfx_wrapped_chunk_cap_exact", "pco_gfx_wrapped_n_pages")
    DIR_FORMS = ("pco_gfx_decompress_pages_dir", "pco_gfx_decompress_page_ranges_dir")

    def __init__(self, G):
        self._G, self.calls = G, []

    def __getattr__(self, name):
        if name in self.FORWARDED:
            return getattr(self._G.lib(), name)

        def call(n_tasks, tasks, *rest):
            G = self._G
            rec = {"fn": name, "n_tasks": n_tasks}
            if isinstance(tasks, C.Array) and tasks._type_ is G.WrappedTask:   # page_sizes points into host memory: record what it points to
                copy = type(tasks).from_buffer_copy(tasks)
                rec["page_sizes"] = []
                for t in copy:
                    sizes = C.cast(t.page_sizes, C.POINTER(C.c_uint64))
                    rec["page_sizes"].append([int(sizes[i]) for i in range(t.n_pages)] if t.page_sizes else None)
                    t.page_sizes = None
                tasks = copy
                rest = rest[1:]   # the config's host address
            rec["tasks"] = [_fields(t) for t in tasks]
            if name in self.DIR_FORMS:
                rec["dir"] = _fields(G.Directory.from_address(_int(rest[0])))
                rest = rest[1:]
            rec["args"] = ["host" if isinstance(a, C.Array) else _int(a) for a in rest]   # results (a host array, or None), d_results, ..., stream
            self.calls.append(rec)
            return G.PcoSuccess
        return call


# ------------------------------------------------------------------------------------------------------------------------------ the cases
DTYPES = ["uint32", "float64", "int16"]
PAGE_NS = [[1000, 999, 257], [300], [1]]   # three pages; one page; a single page of one row
META_LENS, PAGE_LENS = [37, 21, 9], [[1234, 1201, 333], [2400], [2]]
ROWS = {"empty_skipped_whole": [(5, 5), None, (0, 1)], "inside_a_batch": [(300, 310), (256, 300), None],
        "across_pages": [(990, 2100), None, (0, 0)], "whole_chunks": [(0, 2256), (0, 300), (0, 1)]}
ROWS_FROM = {"in_front_of_the_first_cursor": [(10, 20), (0, 5), None], "behind_the_last_cursor": [(900, 1000), (280, 300), (0, 1)],
             "across_pages": [(990, 2100), None, None]}


def directory(gap):
    """The page directory of DTYPES' three chunks with `gap` bytes in front of every piece: (chunk, piece, n, offset, length) tuples."""
    out = []; at = 0
    for c, (meta_len, lens) in enumerate(zip(META_LENS, PAGE_LENS)):
        for piece, (n, length) in enumerate(zip([0] + PAGE_NS[c], [meta_len] + lens)):
            out.append((c, piece, n, at + gap, length)); at += gap + length
    return out, at


def _returned(x):
    """What a function returned, as JSON: tensors by address, shape and dtype; a PageIndex with its results tensor behind its cursors."""
    if isinstance(x, FakeTensor):
        return x.describe()
    if isinstance(x, (list, tuple)):
        out = [_returned(y) for y in x]
        return out + [{"results": x.results.describe()}] if getattr(x, "results", None) is not None else out
    return x


def record(paged):
    """{case: {"calls": [...], "returned": ...}} of `paged` (a pcodec_amd.paged module) under the stand-ins, every case on fresh addresses."""
    from pcodec_amd import ChunkConfig, PagingSpec
    from pcodec_amd import _lib as G
    G.lib()   # (loads the real torch first where there is one: the stand-in is for paged's functions only)
    out = {}
    real_torch, real_require = sys.modules.get("torch"), paged._require_device

    def case(name, fn):
        torch = sys.modules["torch"] = FakeTorch()
        lib = FakeLib(G)
        paged._require_device = lambda: lib
        assert name not in out
        out[name] = {"returned": _returned(fn(torch)), "calls": lib.calls}

    def blob_case(name, gap, fn):
        def run(torch):
            pieces, total = directory(gap)
            return fn(torch.empty(total + 64, dtype=torch.uint8, device="cuda"), pieces)
        case(f"{name}/gap{gap}", run)

    def read_in_slices(blob, pieces, chunk, sizes):
        reader = paged.ChunkReader(blob, pieces, DTYPES, chunk)
        return [reader.cursors] + [reader.read(reader.n - reader.pos if n is None else n) for n in sizes]

    def compress(torch, gap, page_sizes):
        tensors = [torch.tensor_of(sum(ns), name) for ns, name in zip(PAGE_NS, DTYPES)]
        return paged.compress_chunks(tensors, ChunkConfig(paging_spec=PagingSpec.equal_pages_up_to(1000)), page_sizes=page_sizes, gap=gap)

    def compressed_case(name, gap, page_sizes, fn):
        def run(torch):
            cc = compress(torch, gap, page_sizes)
            return [cc.page_ns, fn(cc)]
        case(f"{name}/gap{gap}", run)

    try:
        for gap in (0, 4):
            blob_case("decompress_chunks", gap, lambda blob, pieces: paged.decompress_chunks(blob, pieces, DTYPES))
            for label, rows in ROWS.items():
                blob_case(f"decompress_rows/{label}", gap, lambda blob, pieces, rows=rows: paged.decompress_rows(blob, pieces, DTYPES, rows))
            blob_case("chunk_reader/three_pages", gap, lambda blob, pieces: read_in_slices(blob, pieces, 0, (256, 512, None)))
            blob_case("chunk_reader/off_the_batch_grid", gap, lambda blob, pieces: read_in_slices(blob, pieces, 0, (1024, 256, None)))
            blob_case("chunk_reader/one_page", gap, lambda blob, pieces: read_in_slices(blob, pieces, 1, (256, None)))
            blob_case("chunk_reader/one_row", gap, lambda blob, pieces: read_in_slices(blob, pieces, 2, (0, None)))
            for every_rows in (256, 512):
                blob_case(f"save_cursors/every{every_rows}", gap, lambda blob, pieces, e=every_rows: paged.save_cursors(blob, pieces, DTYPES, e))
                blob_case(f"index_pages/every{every_rows}", gap, lambda blob, pieces, e=every_rows: paged.index_pages(blob, pieces, DTYPES, e))

                def rows_from(blob, pieces, rows, e=every_rows, keep=lambda pc: True):
                    cursors = [pc for pc in paged.index_pages(blob, pieces, DTYPES, e) if keep(pc)]
                    return paged.decompress_rows_from(blob, pieces, DTYPES, cursors, rows)
                for label, rows in ROWS_FROM.items():
                    blob_case(f"decompress_rows_from/every{every_rows}/{label}", gap, lambda blob, pieces, rows=rows, f=rows_from: f(blob, pieces, rows))
                blob_case(f"decompress_rows_from/every{every_rows}/first_page_without_cursors", gap,
                          lambda blob, pieces, f=rows_from: f(blob, pieces, ROWS_FROM["across_pages"], keep=lambda pc: (pc.chunk, pc.piece) != (0, 1)))
                blob_case(f"decompress_chunks_from/every{every_rows}", gap, lambda blob, pieces, e=every_rows:
                          paged.decompress_chunks_from(blob, pieces, DTYPES, paged.save_cursors(blob, pieces, DTYPES, e)))
            for label, page_sizes in (("equal_pages", None), ("exact_for_one_chunk_of_three", [PAGE_NS[0], None, None])):
                compressed_case(f"compress_chunks/{label}", gap, page_sizes, lambda cc: [cc.blob, cc.offsets, cc.dtypes, cc.gap])
                compressed_case(f"decompress_chunks_async/{label}", gap, page_sizes, lambda cc: paged.decompress_chunks_async(cc))
                for rows_label, rows in ROWS.items():
                    if label == "equal_pages" and rows_label != "across_pages":
                        continue
                    compressed_case(f"decompress_rows_async/{label}/{rows_label}", gap, page_sizes, lambda cc, rows=rows: paged.decompress_rows_async(cc, rows))

        def written(cc):
            return [cc.page_ns, cc.blob, cc.offsets]
        case("compress_chunks/exact_for_one_chunk_of_two", lambda torch: written(paged.compress_chunks(
            [torch.tensor_of(2256, "uint32"), torch.tensor_of(300, "float64")], ChunkConfig(), page_sizes=[None, [44, 256]])))
        case("compress_chunks/the_config_is_exact", lambda torch: written(paged.compress_chunks(
            [torch.tensor_of(300, "float64")], ChunkConfig(paging_spec=PagingSpec.exact_page_sizes([256, 44])))))
    finally:
        paged._require_device = real_require
        if real_torch is None:
            sys.modules.pop("torch", None)
        else:
            sys.modules["torch"] = real_torch
    return out


if __name__ == "__main__":
    import os
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (behind PYTHONPATH: the package under record may be another)
    from pcodec_amd import paged
    cases = record(paged)
    print(f"{len(cases)} cases of {paged.__file__}")
    with open(sys.argv[1], "w") as f:   # one call per line
        f.write("{\n" + ",\n".join(
            f'{json.dumps(name)}: {{"returned": {json.dumps(c["returned"])}, "calls": [\n  ' + ",\n  ".join(json.dumps(x) for x in c["calls"]) + "]}"
            for name, c in sorted(cases.items())) + "\n}\n")
