"""CPU checks of the mesh component filter (include/rgbid_mesh.h, rgbid.mesh): the numpy restatement the GPU tests compare the kernels
against (tests/mesh_mirror.py) against the sequential union-find of the same contract on hand-built meshes, on shapes that are hard for
hooking and on TSDF meshes with measured figures; the Python argument checks one by one; the header as C99; the library's exports; the
command line's option errors; a filtered mesh through the PLY writer."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rgbid import _lib
from rgbid import mesh as MS
from rgbid import tsdf as TS
from tests import mesh_mirror as MM
from tests import tsdf_mirror as TM
from tests.test_cpu_tsdf import SPHERE, sphere_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
SMALL = dict(centre=(0.12, 0.12, 0.12), radius=0.08)


def tris(*rows):
    return np.array(rows, U32).reshape(-1, 3)


# ---- the meshes: name -> (triangles uint32 [n_t, 3], n_v) ----------------------------------------------------------------------------
def hand_meshes():
    return {
        "one_shared_vertex": (tris((0, 1, 2), (2, 3, 4)), 5),
        "two_apart": (tris((0, 1, 2), (3, 4, 5)), 6),
        "degenerate": (tris((3, 3, 3), (1, 1, 4), (5, 0, 0)), 7),
        "duplicate": (tris((4, 2, 6), (4, 2, 6), (1, 3, 5)), 7),
        "unreferenced": (tris((2, 3, 4), (6, 7, 8), (8, 7, 4)), 11),        # 0, 1 first, 5 between, 9, 10 last
        "no_triangles": (tris(), 4),
        "no_vertices": (tris(), 0),
        "sizes": (tris((0, 1, 2), (1, 2, 3), (2, 3, 4), (5, 6, 7), (6, 7, 8), (9, 10, 11)), 13),   # 3, 2, 1 triangles and vertex 12 alone
    }


@functools.lru_cache(maxsize=None)
def hard_meshes():
    p = np.random.default_rng(1).permutation(5002).astype(U32)
    strip = p[np.arange(5000)[:, None] + np.arange(3)[None, :]]
    fan = np.stack([np.full(4096, 8192), 2 * np.arange(4096), 2 * np.arange(4096) + 1], 1).astype(U32)
    many = np.random.default_rng(2).permutation(600000).astype(U32).reshape(-1, 3)
    return {"strip": (strip, 5002), "strip_reversed": (np.ascontiguousarray(strip[::-1]), 5002), "fan": (fan, 8193), "many": (many, 600000)}


def two_sphere_volume(cut=False):
    vol = TM.Volume(24, 20, 16, (0.0, 0.0, 0.0), 0.05, 0.2)
    big, W = TM.sphere_state(vol, **SPHERE)
    small, _ = TM.sphere_state(vol, **SMALL)
    if cut:
        W = W.copy()
        W[:, :, 12] = 0
    vol.set_state(np.minimum(big, small), W)
    return vol


def noise_volume():
    vol = TM.Volume(24, 20, 16, (0.0, 0.0, 0.0), 0.05, 0.2)
    rng = np.random.default_rng(5)
    D = rng.uniform(-0.2, 0.2, vol.shape).astype(F)
    W = (rng.random(vol.shape) < 0.7).astype(U32)
    vol.set_state(D, W)
    return vol


@functools.lru_cache(maxsize=None)
def tsdf_meshes():
    """name -> (vertices, colours, triangles) of the mirror's extraction"""
    return {"two_spheres": TM.extract(two_sphere_volume(), 1), "cut": TM.extract(two_sphere_volume(cut=True), 1), "noise": TM.extract(noise_volume(), 1),
            "sphere": TM.extract(sphere_volume(), 1)}


def all_meshes():
    out = dict(hand_meshes())
    out.update(hard_meshes())
    out.update({k: (v[2], len(v[0])) for k, v in tsdf_meshes().items() if k != "sphere"})
    return out


@functools.lru_cache(maxsize=None)
def labelled(name):
    """the mirror's (table, labels) of a mesh of all_meshes, computed once"""
    tri, n_v = all_meshes()[name]
    return MM.label(tri, n_v)


def attributes(n_v, seed=0):
    """positions and normals float32 [n_v, 3] with NaNs of distinct payloads among them, colours uint8 [n_v, 3]"""
    rng = np.random.default_rng(100 + seed)
    pos = rng.integers(0, 1 << 32, (n_v, 3), dtype=np.uint64).astype(U32)
    nrm = rng.integers(0, 1 << 32, (n_v, 3), dtype=np.uint64).astype(U32)
    if n_v:
        pos[::7, 1] = U32(0x7FC00000) + (np.arange(len(pos[::7])) % 1000 + 1).astype(U32)     # quiet NaNs, payload = a counter
        nrm[::5, 2] = U32(0xFF800001) + (np.arange(len(nrm[::5])) % 1000).astype(U32)         # signalling NaNs
    return pos.view(F), rng.integers(0, 256, (n_v, 3), dtype=np.uint8), nrm.view(F)


# ---- mirror against loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(set(all_meshes()) - {"many"}))
def test_mirror_equals_the_sequential_union_find(name):
    tri, n_v = all_meshes()[name]
    table, labels = labelled(name)
    lt, ll = MM.label_loop(tri, n_v)
    assert table.dtype == U32 and labels.dtype == U32 and table.shape == (len(lt), 3) and labels.shape == (n_v,)
    assert table.tolist() == lt and labels.tolist() == ll
    pos, col, nrm = attributes(n_v)
    most = int(table[:, 2].max()) if len(table) else 0
    mask = (np.arange(len(table)) % 3 != 1).astype(np.uint8)
    for mt, m in ((0, None), (1, None), (most, None), (most + 1, None), (0, mask), (1, mask), (0, np.zeros(len(table), np.uint8))):
        out = MM.emit(tri, labels, MM.select(table, mt, m), pos, col, nrm)
        old, lt_, kc = MM.filter_loop(tri, n_v, mt, m)
        assert out["old_index"].tolist() == old and out["triangles"].tolist() == lt_ and out["components"] == kc
        assert out["vertices"].view(U32).tolist() == pos.view(U32)[old].tolist() and out["colours"].tolist() == col[old].tolist()
        assert out["normals"].view(U32).tolist() == nrm.view(U32)[old].tolist()


def test_many_components_mirror_against_loop():
    tri, n_v = all_meshes()["many"]
    table, labels = labelled("many")
    lt, ll = MM.label_loop(tri, n_v)
    assert table.shape == (200000, 3) and (table[:, 1] == 3).all() and (table[:, 2] == 1).all()
    assert table.tolist() == lt and labels.tolist() == ll


# ---- hand-built meshes --------------------------------------------------------------------------------------------------------------------
def test_hand_built_meshes():
    H = hand_meshes()
    t, l = MM.label(*H["one_shared_vertex"]); assert t.tolist() == [[0, 5, 2]] and l.tolist() == [0] * 5
    t, l = MM.label(*H["two_apart"]); assert t.tolist() == [[0, 3, 1], [3, 3, 1]] and l.tolist() == [0, 0, 0, 1, 1, 1]
    t, l = MM.label(*H["degenerate"])
    assert t.tolist() == [[0, 2, 1], [1, 2, 1], [2, 1, 0], [3, 1, 1], [6, 1, 0]] and l.tolist() == [0, 1, 2, 3, 1, 0, 4]
    t, l = MM.label(*H["duplicate"]); assert t.tolist() == [[0, 1, 0], [1, 3, 1], [2, 3, 2]] and l.tolist() == [0, 1, 2, 1, 2, 1, 2]
    t, l = MM.label(*H["unreferenced"])
    assert t.tolist() == [[0, 1, 0], [1, 1, 0], [2, 6, 3], [5, 1, 0], [9, 1, 0], [10, 1, 0]] and l.tolist() == [0, 1, 2, 2, 2, 3, 2, 2, 2, 4, 5]
    t, l = MM.label(*H["no_triangles"]); assert t.tolist() == [[v, 1, 0] for v in range(4)] and l.tolist() == [0, 1, 2, 3]
    t, l = MM.label(*H["no_vertices"]); assert t.shape == (0, 3) and l.shape == (0,)
    out = MM.filter_mesh(*H["no_vertices"], np.zeros((0, 3), F))
    assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["components"] == 0
    for bad in (tris((0, 1, 5)), tris((0, 1, 2), (0xFFFFFFFF, 1, 2))):
        with pytest.raises(ValueError):
            MM.label(bad, 5)
        with pytest.raises(ValueError):
            MM.label_loop(bad, 5)


def test_selection_by_size_and_mask():
    tri, n_v = hand_meshes()["sizes"]
    table, labels = MM.label(tri, n_v)
    assert table.tolist() == [[0, 5, 3], [5, 4, 2], [9, 3, 1], [12, 1, 0]]
    pos, col, nrm = attributes(n_v)
    kept = lambda mt, m=None: MM.emit(tri, labels, MM.select(table, mt, m), pos, col, nrm)
    o = kept(0)                                                      # everything: the input's bytes
    assert o["vertices"].tobytes() == pos.tobytes() and o["colours"].tobytes() == col.tobytes() and o["normals"].tobytes() == nrm.tobytes()
    assert o["triangles"].tobytes() == tri.tobytes() and o["old_index"].tolist() == list(range(13)) and o["components"] == 4
    o = kept(1)                                                      # exactly the unreferenced vertex goes
    assert o["old_index"].tolist() == list(range(12)) and o["triangles"].tobytes() == tri.tobytes() and o["components"] == 3
    o = kept(2); assert o["old_index"].tolist() == list(range(9)) and len(o["triangles"]) == 5          # on the count of component 1
    o = kept(3); assert o["old_index"].tolist() == list(range(5)) and len(o["triangles"]) == 3          # one above it
    o = kept(4); assert o["components"] == 0 and o["vertices"].shape == (0, 3) and o["triangles"].shape == (0, 3)
    o = kept(0, [0, 1, 0, 1])                                        # the mask alone
    assert o["old_index"].tolist() == [5, 6, 7, 8, 12] and o["triangles"].tolist() == [[0, 1, 2], [1, 2, 3]] and o["components"] == 2
    o = kept(1, [0, 1, 0, 1]); assert o["old_index"].tolist() == [5, 6, 7, 8] and o["components"] == 1   # with a threshold
    o = kept(2, [5, 0, 255, 0]); assert o["old_index"].tolist() == [0, 1, 2, 3, 4]
    o = kept(0, [0, 0, 0, 0]); assert o["components"] == 0 and len(o["old_index"]) == 0 and len(o["triangles"]) == 0


def test_largest_mask_breaks_a_tie_by_root():
    table = np.array([[0, 3, 2], [3, 9, 5], [12, 3, 2], [15, 4, 5], [19, 1, 0]], U32)
    for f in (MM.largest_mask, MS.largest_mask):
        assert f(table, 1).tolist() == [0, 1, 0, 0, 0] and f(table, 2).tolist() == [0, 1, 0, 1, 0]
        assert f(table, 3).tolist() == [1, 1, 0, 1, 0] and f(table, 4).tolist() == [1, 1, 1, 1, 0] and f(table, 9).tolist() == [1] * 5
        assert f(table[:0], 2).tolist() == []
    import torch
    m = MS.largest_mask(torch.from_numpy(table.view(np.int32)), 2)
    assert isinstance(m, torch.Tensor) and m.dtype == torch.uint8 and m.tolist() == [0, 1, 0, 1, 0]


# ---- shapes that are hard for hooking -------------------------------------------------------------------------------------------------
def test_hard_shapes():
    for name, n_v, n_t in (("strip", 5002, 5000), ("strip_reversed", 5002, 5000), ("fan", 8193, 4096)):
        table, labels = labelled(name)
        assert table.tolist() == [[0, n_v, n_t]] and not labels.any(), name
    table, labels = labelled("many")
    tri, _ = all_meshes()["many"]
    assert len(table) == 200000 and np.array_equal(table[:, 0], np.sort(tri.min(1))) and (labels[tri] == labels[tri[:, :1]]).all()


# ---- TSDF meshes: figures measured on the mirrors ------------------------------------------------------------------------------------------
def closed(tri):
    edges, two, _ = TM.mesh_topology(tri)
    return edges, two == edges


def test_two_spheres():
    v, c, tri = tsdf_meshes()["two_spheres"]
    sv, sc, st = tsdf_meshes()["sphere"]
    table, labels = labelled("two_spheres")
    assert (len(v), len(tri)) == (2142, 4276) and table.tolist() == [[0, 140, 276], [98, 2002, 4000]]
    for comp, edges in ((0, 414), (1, 6000)):
        assert closed(tri[labels[tri[:, 0]] == comp]) == (edges, True)
    big = MM.filter_mesh(tri, len(v), v, c, min_triangles=277)
    assert big["vertices"].tobytes() == sv.tobytes() and big["triangles"].tobytes() == st.tobytes() and big["colours"].tobytes() == sc.tobytes()
    assert big["components"] == 1 and (len(sv), len(st)) == (2002, 4000)
    both = MM.filter_mesh(tri, len(v), v, c, min_triangles=276)
    assert both["components"] == 2 and both["vertices"].tobytes() == v.tobytes() and both["triangles"].tobytes() == tri.tobytes()
    one = MM.filter_mesh(tri, len(v), v, c, largest=1)
    assert one["vertices"].tobytes() == sv.tobytes() and one["triangles"].tobytes() == st.tobytes()


def test_cut_spheres():
    v, c, tri = tsdf_meshes()["cut"]
    table, _ = labelled("cut")
    assert (len(v), len(tri), len(table)) == (1902, 3640, 3) and sorted(table[:, 2].tolist()) == [276, 1676, 1688]


def test_noise_volume():
    v, c, tri = tsdf_meshes()["noise"]
    table, labels = labelled("noise")
    nt = table[:, 2]
    assert (len(v), len(tri), len(table)) == (11968, 2788, 9306)
    assert int((nt == 0).sum()) == 9090 and (table[nt == 0, 1] == 1).all() and int((nt >= 1).sum()) == 216
    assert [int((nt >= k).sum()) for k in (4, 8, 16, 64)] == [153, 118, 47, 5] and int(nt.max()) == 122
    referenced = np.zeros(len(v), bool)
    referenced[tri.reshape(-1)] = True
    for mt, comps in ((1, 216), (8, 118), (64, 5)):
        out = MM.filter_mesh(tri, len(v), v, c, min_triangles=mt)
        assert out["components"] == comps and len(out["triangles"]) == int(nt[nt >= mt].sum()) and len(out["vertices"]) == int(table[nt >= mt, 1].sum())
        assert (out["triangles"] < len(out["vertices"])).all()
        used = np.zeros(len(out["vertices"]), bool)
        used[out["triangles"].reshape(-1)] = True
        assert used.all()                                            # every kept vertex is referenced
        if mt == 1:
            assert np.array_equal(out["old_index"], np.nonzero(referenced)[0])


# ---- the Python checkers, one by one --------------------------------------------------------------------------------------------------
def test_capacity_checker():
    assert MS.capacity_arg(1, 1) == (1, 1) and MS.capacity_arg(1 << 31, np.int64(1 << 31)) == (1 << 31, 1 << 31)
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, (1 << 31) + 1), (-1, 1), (1.0, 1), (1, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            MS.capacity_arg(v, t)


def test_min_triangles_and_largest_checkers():
    assert [MS.min_triangles_arg(n) for n in (0, 1, (1 << 32) - 1, np.int32(7))] == [0, 1, (1 << 32) - 1, 7]
    for n in (-1, 1 << 32, 1.0, "1", None, True):
        with pytest.raises(ValueError):
            MS.min_triangles_arg(n)
    assert MS.largest_arg(None) is None and MS.largest_arg(1) == 1 and MS.largest_arg(np.int64(5)) == 5
    for k in (0, -1, 1.0, "1", False):
        with pytest.raises(ValueError):
            MS.largest_arg(k)
    assert TS.component_filter_arg(None, None) is None and TS.component_filter_arg(8, None) == (8, None)
    assert TS.component_filter_arg(None, 2) == (1, 2) and TS.component_filter_arg(0, 3) == (0, 3)
    for a, b in ((-1, None), (None, 0), (1.5, None), (None, "2")):
        with pytest.raises(ValueError):
            TS.component_filter_arg(a, b)


def test_mesh_and_keep_checkers_need_cuda_tensors():
    import torch
    host = torch.zeros((4, 3), dtype=torch.int32)
    for tri, n_v in ((host, 5),                                     # a host tensor
                     (host.numpy(), 5), (None, 5), ([[0, 1, 2]], 5)):
        with pytest.raises(ValueError):
            MS.mesh_arg(tri, n_v)
    for n_v in (-1, 2.0, None, "5", True):
        with pytest.raises(ValueError):
            MS.mesh_arg(host, n_v)
    assert MS.keep_arg(None, 3) is None
    for keep in (torch.zeros(3, dtype=torch.uint8),                 # a host tensor
                 np.zeros(3, np.uint8), [1, 0, 1], 1):
        with pytest.raises(ValueError):
            MS.keep_arg(keep, 3)


def test_checks_come_before_the_library():
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 4)):
        with pytest.raises(ValueError):
            MS.Components(None, v, t)

    class Ctx:
        device = 0
    cc = MS.Components.__new__(MS.Components)
    cc.ctx, cc.max_vertices, cc.max_triangles, cc._triangles, cc.kept, cc.components, cc.n_vertices = Ctx(), 10, 10, None, None, 0, 0
    with pytest.raises(ValueError):
        cc.label(np.zeros((1, 3), np.int32), 3)
    for mt in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError):
            cc.select(mt)
    with pytest.raises(ValueError):
        cc.select(1)                                                # nothing is labelled
    with pytest.raises(ValueError):
        cc.emit(None)                                               # nothing is selected
    cc._h = None
    for kw in (dict(min_triangles=-1), dict(largest=0), dict(min_triangles="8")):
        with pytest.raises(ValueError):
            MS.filter_components(None, None, None, None, **kw)
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for kw in (dict(min_component=-1), dict(largest_components=0), dict(min_component=1.5)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), **kw)
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    for kw in (dict(min_component=-1), dict(largest_components=0)):
        with pytest.raises(ValueError):
            vol.extract(1, **kw)
    vol._h = None


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_mesh.c"
    src.write_text('#include "rgbid_mesh.h"\n'
                   "int use(rgbid_mesh* m, rgbid_ctx* ctx, const uint32_t* tris, const float* v, const uint8_t* c, const float* n, float* vo, uint8_t* co,\n"
                   "        float* no, uint32_t* old, uint32_t* to, uint32_t* table, uint32_t* labels, const uint8_t* mask) {\n"
                   "  unsigned long long nc, kc, kv, kt; float ms[3];\n"
                   "  return rgbid_mesh_create(&m, ctx, RGBID_MESH_MAX_VERTICES, RGBID_MESH_MAX_TRIANGLES) + rgbid_mesh_label(m, 10, 5, tris, &nc)\n"
                   "       + rgbid_mesh_components(m, table, labels) + rgbid_mesh_select(m, 4294967295u, mask, &kc, &kv, &kt)\n"
                   "       + rgbid_mesh_emit(m, v, c, n, vo, co, no, old, to, kv, kt) + rgbid_mesh_timing(m, 1, ms) + rgbid_mesh_destroy(m); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_mesh.h")).read()
    assert int(re.search(r"RGBID_MESH_MAX_VERTICES\s+(\d+)ull", txt).group(1)) == MS.MAX_VERTICES == 1 << 31
    assert int(re.search(r"RGBID_MESH_MAX_TRIANGLES\s+(\d+)ull", txt).group(1)) == MS.MAX_TRIANGLES == 1 << 31


def test_library_exports_mesh_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_mesh.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_mesh_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(MS.EXPORTS) and len(declared) == 7, set(declared) ^ set(MS.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_mesh_create.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_ulonglong]
    L.rgbid_mesh_label.argtypes = [c.c_void_p, c.c_ulonglong, c.c_ulonglong, c.c_void_p, c.c_void_p]
    L.rgbid_mesh_components.argtypes = [c.c_void_p] * 3
    L.rgbid_mesh_select.argtypes = [c.c_void_p, c.c_uint32] + [c.c_void_p] * 4
    L.rgbid_mesh_emit.argtypes = [c.c_void_p] * 9 + [c.c_ulonglong] * 2
    L.rgbid_mesh_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_mesh_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_mesh_create(c.byref(h), None, 10, 10) == -1 and not h.value and L.rgbid_mesh_create(None, None, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 31) + 1)):
        assert L.rgbid_mesh_create(c.byref(h), fake, v, t) == -1 and not h.value
    n = c.c_ulonglong()
    assert L.rgbid_mesh_label(None, 1, 0, None, c.byref(n)) == -1 and L.rgbid_mesh_components(None, None, None) == -1
    assert L.rgbid_mesh_select(None, 1, None, None, None, None) == -1 and L.rgbid_mesh_emit(None, *([None] * 8), 0, 0) == -1
    assert L.rgbid_mesh_timing(None, 0, None) == -1 and L.rgbid_mesh_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-min-component", "8"], "need --mesh"), (["--mesh-largest-components", "1"], "need --mesh"),
                      (mesh + ["--mesh-min-component", "-1"], "min_triangles must lie in"),
                      (mesh + ["--mesh-min-component", "4294967296"], "min_triangles must lie in"),
                      (mesh + ["--mesh-largest-components", "0"], "largest must be at least 1"),
                      (mesh + ["--mesh-min-component", "x"], "invalid int value")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()


def test_filtered_mesh_through_the_ply_writer(tmp_path):
    v, c, tri = tsdf_meshes()["noise"]
    c = np.random.default_rng(3).integers(0, 256, c.shape, dtype=np.uint8)
    nrm = attributes(len(v))[2]
    out = MM.filter_mesh(tri, len(v), v, c, nrm, min_triangles=8)
    path = tmp_path / "filtered.ply"
    TS.write_mesh_ply(str(path), out["vertices"], out["colours"], out["triangles"], out["normals"])
    pv, pc, pt, pn = TS.read_mesh_ply(path.read_bytes())
    assert pv.tobytes() == out["vertices"].tobytes() and pc.tobytes() == out["colours"].tobytes() and pt.tobytes() == out["triangles"].tobytes()
    assert pn.tobytes() == out["normals"].tobytes() and len(pt) == int(labelled("noise")[0][:, 2][labelled("noise")[0][:, 2] >= 8].sum())
