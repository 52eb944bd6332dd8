"""-m gpu: the encoder's bit packers at their width, staging and join edges (the rows of pack_edges_util.py).

One synchronous pco_gfx_compress_chunks call per family and config (pack_edges_util.CALLS), into destinations filled with 0xff -- the packers
OR shared dwords into what enc_scan_kernel zeroed, and must not count on anything else being zero.  Per row:

  * pco_gfx_debug_pack_routes shows the packer pack_layout_model predicted for the row in this call, and pco_gfx_debug_histogram the 16-bit /
    full-width latents the row was built on (a row that reaches another packer fails: it would be testing something else);
    the hook reports the shifted copy and the general kernel's other pages alike (0: one kernel, one nibble), so that a "copy" row took the
    copy branch rests on pack_layout_model.is_copy and the hist_path read back, not on the device's word;
  * the chunk equals the oracle's byte for byte -- a difference is reported with the row's name, the first differing bit and what the model
    says lies there (variable, batch, tANS or offset section);
  * the chunk decodes to the input bit for bit, with a guard byte behind every chunk's numbers.

The run-join and tail families and the shifted copy run at destinations 0 and 8 modulo 16; the walk-and-pack family runs at 8, and once more in
a fresh process with PCO_GFX_WALKP=0, where its rows take the lean kernel and must give the same bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _imports():
    global torch, G, E, P, decode_call
    import torch
    from pcodec_amd import _lib as G
    import pack_edges_util as E
    import pack_layout_model as P
    from test_gpu_width_paths import decode_call


@pytest.fixture(scope="module")
def L():
    _imports()
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def encode(L, arrays, kw, shift, fill=0xFF):
    """One synchronous pco_gfx_compress_chunks call over `arrays`, every destination `shift` bytes past a 16-byte boundary in a buffer of
    `fill` bytes.  Returns (chunk bytes, the pack route byte per page, hist_path per chunk and variable)."""
    k = len(arrays)
    s_offs = np.concatenate([[0], np.cumsum([(a.nbytes + 15) // 16 * 16 for a in arrays])]).astype(np.int64)
    host_src = np.zeros(int(s_offs[-1]) + 16, np.uint8)
    for o, a in zip(s_offs, arrays):
        host_src[o:o + a.nbytes] = a.view(np.uint8)
    src = torch.from_numpy(host_src).cuda()
    caps = [L.pco_gfx_guarantee_chunk_size(a.size, G.DTYPE_BYTE[a.dtype.name]) + 64 for a in arrays]
    d_offs = np.concatenate([[0], np.cumsum([(c + 32 + 15) // 16 * 16 for c in caps])]).astype(np.int64)
    comp = torch.full((int(d_offs[-1]) + 64,), fill, dtype=torch.uint8, device="cuda")
    assert comp.data_ptr() % 16 == 0
    tasks = (G.EncodeTask * k)(*[G.EncodeTask(src.data_ptr() + int(s_offs[i]), arrays[i].size, comp.data_ptr() + int(d_offs[i]) + shift, caps[i],
                                              G.DTYPE_BYTE[arrays[i].dtype.name], 0) for i in range(k)])
    assert all(t.dst % 16 == shift for t in tasks)
    res = (G.TaskResult * k)()
    cfg = G.make_config(enable_8_bit=True, **kw)
    G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(cfg), res, None, None))
    routes = np.full(k, 0xEE, np.uint8)
    assert L.pco_gfx_debug_pack_routes(routes.ctypes.data_as(C.c_void_p), k) == k
    paths = []
    for i in range(k):
        row = []
        for v in range(3):
            info = (C.c_uint32 * 4)()
            assert L.pco_gfx_debug_histogram(i, v, None, None, None, 0, info) >= 0
            row.append(int(info[2]))
        paths.append(row)
    host = comp.cpu().numpy()
    chunks = []
    for i in range(k):
        assert res[i].status == 0 and 0 < res[i].n_out <= caps[i], (i, res[i].status, res[i].n_out)
        chunks.append(host[int(d_offs[i]) + shift: int(d_offs[i]) + shift + res[i].n_out].tobytes())
    return chunks, routes, paths


def first_difference(got, want, layout):
    """"bit N (byte, bit): what the model says lies there", for two chunks that differ."""
    n = min(len(got), len(want))
    a = np.frombuffer(got[:n], np.uint8); b = np.frombuffer(want[:n], np.uint8)
    d = np.flatnonzero(a != b)
    if d.size == 0:
        return f"lengths {len(got)} / {len(want)} bytes, equal up to the shorter"
    x = int(a[d[0]]) ^ int(b[d[0]]); bit = 8 * int(d[0]) + (x & -x).bit_length() - 1
    return f"first differing bit {bit} (byte {int(d[0])}: {int(a[d[0]]):02x} for {int(b[d[0]]):02x}, {d.size} bytes differ, lengths {len(got)} / {len(want)}): {P.what_lies_at(layout, bit)}"


def check_rows(L, names, kw, shift, routes_want):
    """Encode `names` in one call at one destination offset; returns (failures by row name, chunks, arrays)."""
    arrays = [E.numbers(n) for n in names]
    chunks, routes, paths = encode(L, arrays, kw, shift)
    bad = []
    for i, name in enumerate(names):
        row = E.BY_NAME()[name]; lay = E.layout(name)
        for v in range(3):
            if lay.present[v] and not P.trivial(lay, v) and (paths[i][v] == 0) != row.compact[v]:
                bad.append(f"{name} @{shift}: variable {v} has hist_path {paths[i][v]}, the row was built for {'16-bit' if row.compact[v] else 'full-width'} latents")
        if int(routes[i]) != P.ROUTE_BYTE[routes_want[name]]:
            bad.append(f"{name} @{shift}: pack route byte {int(routes[i]):#x}, predicted {routes_want[name]} ({P.ROUTE_BYTE[routes_want[name]]:#x})")
        if chunks[i] != E.oracle_chunk(name):
            bad.append(f"{name} @{shift} [{routes_want[name]}]: {first_difference(chunks[i], E.oracle_chunk(name), lay)}")
    return bad, chunks, arrays


def _calls():
    import pack_edges_util as E_
    return E_.CALLS()


@pytest.mark.parametrize("call", _calls(), ids=[c.name for c in _calls()])
def test_rows_take_their_packer_and_give_the_oracles_bytes(L, call):
    want = E.predicted_routes(call)
    assert all(want[n] == E.BY_NAME()[n].route for n in call.rows)   # (what the CPU suite checks)
    bad = []
    for shift in call.shifts:
        b, chunks, arrays = check_rows(L, list(call.rows), call.kw, shift, want)
        bad += b
    assert not bad, "\n" + "\n".join(bad[:40]) + f"\n({len(bad)} in all)"
    decode_call([E.oracle_chunk(n) for n in call.rows], arrays)   # (the chunks equal the oracle's: these are the device's bytes)


def test_walk_and_pack_rows_give_the_same_bytes_from_the_lean_kernel(L):
    """Family P once more with PCO_GFX_WALKP=0, which is read once per process: a fresh child.  Its rows then take enc_pack1_kernel."""
    env = dict(os.environ, PCO_GFX_WALKP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--walkp-off"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "walkp-off ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_4112_copies_of_three_long_pages(L):
    """More than 4096 items: no segmented walk, enc_walkp_kernel takes every block, and enc_place_kernel moves each body in two pieces.
    Every copy's bytes are compared (the oracle runs for the three distinct pages only), in one call with every destination 8 bytes past a
    16-byte boundary and one with every destination on one."""
    names = [f"P-u8-long-{i % 3}" for i in range(4112)]
    call = E.Call("P8", E.CLASSIC, tuple(names), (0, 8))
    want = E.predicted_routes(call)
    assert set(want.values()) == {"walkp"} and P.kWsMaxItems < len(names)
    arrays = [E.numbers(n) for n in names]
    for shift in (8, 0):
        chunks, routes, paths = encode(L, arrays, call.kw, shift)
        assert (routes == P.ROUTE_BYTE["walkp"]).all(), np.flatnonzero(routes != 15)[:10]
        bad = [f"copy {i} of {n} @{shift}: {first_difference(c, E.oracle_chunk(n), E.layout(n))}" for i, (n, c) in enumerate(zip(names, chunks)) if c != E.oracle_chunk(n)]
        assert not bad, "\n" + "\n".join(bad[:20]) + f"\n({len(bad)} in all)"
    decode_call(chunks[:96], arrays[:96])


def test_the_hook_counts_without_writing_and_reports_a_page_that_did_not_fit(L):
    """pco_gfx_debug_pack_routes' contract beside the routes: 0xfe for a page whose destination is too small (its neighbour is packed as
    predicted), the page count with no room to write, a negative status for room without a buffer."""
    names = ["T-lean2-5", "T-wide64-5"]
    arrays = [E.numbers(n) for n in names]
    src = [torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in arrays]
    caps = [L.pco_gfx_guarantee_chunk_size(arrays[0].size, G.DTYPE_BYTE[arrays[0].dtype.name]) + 64, 64]   # (the second chunk is 1385 bytes long)
    assert len(E.oracle_chunk(names[1])) > caps[1]
    dst = [torch.full((4096,), 0xFF, dtype=torch.uint8, device="cuda") for _ in arrays]
    tasks = (G.EncodeTask * 2)(*[G.EncodeTask(src[i].data_ptr(), arrays[i].size, dst[i].data_ptr(), caps[i], G.DTYPE_BYTE[arrays[i].dtype.name], 0) for i in range(2)])
    res = (G.TaskResult * 2)()
    cfg = G.make_config(enable_8_bit=True, **E.CLASSIC)
    L.pco_gfx_compress_chunks(2, tasks, C.byref(cfg), res, None, None)
    assert res[0].status == 0 and res[1].status != 0 and res[1].n_out == 0
    assert bytes(dst[0][:res[0].n_out].cpu().numpy()) == E.oracle_chunk(names[0])
    assert (dst[1].cpu().numpy()[64:] == 0xFF).all(), "written past a destination that was too small"
    routes = np.full(4, 0xEE, np.uint8)
    assert L.pco_gfx_debug_pack_routes(routes.ctypes.data_as(C.c_void_p), 4) == 2
    want = E.predicted_routes(E.Call("x", E.CLASSIC, tuple(names), (0,)))
    assert routes.tolist() == [P.ROUTE_BYTE[want[names[0]]], 0xFE, 0xEE, 0xEE], routes
    assert L.pco_gfx_debug_pack_routes(None, 0) == 2
    routes[:] = 0xEE
    assert L.pco_gfx_debug_pack_routes(routes.ctypes.data_as(C.c_void_p), 1) == 2 and routes.tolist()[1:] == [0xEE] * 3
    assert L.pco_gfx_debug_pack_routes(None, 2) < 0


def walkp_off_child():
    """The child of test_walk_and_pack_rows_give_the_same_bytes_from_the_lean_kernel."""
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
    _imports()
    lib = G.lib()
    call = next(c for c in E.CALLS() if c.name == "P")
    lean = {n: P.route(E.layout(n), E.BY_NAME()[n].compact, False) for n in call.rows}
    assert set(lean.values()) == {"lean<2>", "general"}, lean
    bad, _, _ = check_rows(lib, list(call.rows), call.kw, 8, lean)
    if bad:
        print("\n".join(bad)); sys.exit(1)
    print("walkp-off ok")


if __name__ == "__main__":
    if "--walkp-off" in sys.argv:
        walkp_off_child()
