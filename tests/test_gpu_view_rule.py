"""GPU tests that hold the three statements of the visibility rule (steps 3 - 4 of include/rgbid_recolour.h) to one table and to each other:
k_recolour_add and k_texture_add, which keep it written out, and view_device.h's view_sample, which colour alignment walks.  The cases are
tests/test_cpu_recolour.py's -- BOUNDARIES, every class boundary exact in float32, and two random cases that hold all six classes -- put in
front of the texturer as degenerate triangles and in front of the colour aligner's target pass by tests/view_rule_cases.py (the CPU file
tests/test_cpu_view_rule_cases.py shows on the mirrors that the builders do what they say).  Every output is compared byte for byte, with a
canary element behind it: each operator with its own mirror, so that a failure names the copy that moved, and the device texturer and
colour aligner with the device recolourer, so that a drift between the kernels fails whatever the mirrors say."""
import numpy as np
import pytest

from rgbid import colouralign as CA, recolour as RC, texture as TX
from tests import colouralign_mirror as AM
from tests import recolour_mirror as CM
from tests import test_gpu_colouralign as GC
from tests import test_gpu_recolour as GR
from tests import test_gpu_texture as GT
from tests import view_rule_cases as VC
from tests.test_cpu_recolour import BOUNDARIES, OPTIONAL, mirror as recolour_mirror, random_case
from tests.test_cpu_texture import mirror as texture_mirror

pytestmark = pytest.mark.gpu
U32 = np.uint32
MODES = ("mean", "best")
CAP_N, CAP_VIEWS = 257, 33                                       # the largest case below: 257 vertices, 33 views
CAP_SLOTS = max(TX.layout(CAP_N, patch, 3)["slots"] for patch in (2, 5, 6))


@pytest.fixture(scope="module")
def rc(ctx):
    h = RC.Recolourer(ctx, CAP_N)
    yield h
    h.close()


@pytest.fixture(scope="module")
def tx(ctx):
    h = TX.Texturer(ctx, CAP_N, CAP_SLOTS)
    yield h
    h.close()


@pytest.fixture(scope="module")
def ca(ctx):
    h = CA.ColourAligner(ctx, CAP_N, CAP_VIEWS)
    yield h
    h.close()


def host(t):
    a = t.cpu().numpy()
    return a.view(U32) if a.dtype == np.int32 else a


def counts_of(h):
    return np.array([[k[x] for x in CM.COUNTS] for k in h.counts()], np.int64)


def recolour_device(rc, c, mode, drop=()):
    """the device recolourer's outputs of a case, a canary element behind each -> dict(colours, views_used, best_view, counts) as numpy"""
    n = len(c["vertices"])
    names = [o for o in GR.OUTPUTS if o != "best_view" or mode == "best"]
    rc.begin(n, mode)
    held = GR.add_views(rc, c, None, drop)
    out = GR.outputs_with_canary(n, names)
    rc.ctx.wait_torch_stream()
    rc.finish_into(None, **{("colours_out" if o == "colours" else o): out[o][:n] for o in names})
    rc.ctx.sync()
    del held
    assert all((out[o][n] == GR.CANARY[o]).all() for o in names)
    return dict({o: host(out[o][:n]) for o in names}, counts=counts_of(rc))


def texture_device(tx, t, mode, drop=()):
    """the device texturer's outputs of a texture case, a canary element behind each -> dict(atlas, views_used, best_view, counts) as numpy"""
    names = [o for o in VC.PLANES if o != "best_view" or mode == "best"]
    lay = tx.begin(len(t["triangles"]), t["patch"], t["tiles_x"], mode)
    held = GT.add_views(tx, t, None, drop)
    out = GT.outputs_with_canary(lay, names)
    tx.ctx.wait_torch_stream()
    tx.finish_into(None, None, **{o: out[o][1] for o in names})
    tx.ctx.sync()
    del held
    assert all((out[o][0][out[o][1].numel():] == GT.CANARY[o]).all() for o in names)
    return dict({o: host(out[o][1]) for o in names}, counts=counts_of(tx))


def colouralign_device(ca, a, **rule):
    """the device colour aligner on view_rule_cases.as_colouralign's arguments -> (records, S, W, used), the canaries checked"""
    return GC.run_device(ca, a, fixed=a["fixed"], rows=a["rows"], cols=a["cols"], K_=a["K"], prm=a["params"], **rule)


def assert_bytes(got, exp, what):
    """every output of `got` has the bytes of the mirror's"""
    for o in got:
        assert got[o].shape == exp[o].shape and got[o].tobytes() == np.asarray(exp[o]).astype(got[o].dtype).tobytes(), \
            (what, o, np.argwhere(got[o] != exp[o])[:5].tolist())


def assert_texture_repeats(tex, vert, n, patch, tiles_x, what):
    """the device texturer on the triangles (v, v, v) against the device recolourer on the vertices: every texel of triangle v holds what
    vertex v holds, and a view counts each class once per texel"""
    P = VC.texels(patch)
    assert (tex["counts"] == P * vert["counts"]).all(), (what, tex["counts"], vert["counts"])
    for plane in tex:
        if plane != "counts":
            got, want = VC.texel_view(tex[plane], n, patch, tiles_x), vert[VC.VERTEX_OUTPUT[plane]]
            assert got.shape[:2] == (n, P) and (got == want[:, None]).all(), (what, plane, np.argwhere((got != want[:, None]).reshape(n, -1).any(1))[:5].tolist())


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_texture_at_the_class_boundaries(rc, tx, name):
    """tiles_x 3 leaves the last row of tiles partly empty and puts used and unused slots in one wave: view_tally's class -1 beside each
    boundary class"""
    c, _ = BOUNDARIES[name]
    n = len(c["vertices"])
    for mode in MODES:
        vert = recolour_device(rc, c, mode)
        assert_bytes(vert, recolour_mirror(c, mode), (name, mode, "recolour"))
        for patch in (2, 3, 6):
            for tiles_x in (1, 3):
                t = VC.as_texture(c, patch, tiles_x)
                tex = texture_device(tx, t, mode)
                assert_bytes(tex, texture_mirror(t, mode), (name, mode, patch, tiles_x))
                assert_texture_repeats(tex, vert, n, patch, tiles_x, (name, mode, patch, tiles_x))


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_colouralign_at_the_class_boundaries(ca, name):
    """the case's view twice, the first held, one target pass at the given poses: a vertex the view takes is used twice, and the first
    system of the second view uses exactly the taken vertices of its lattice; images of 3 x 5, 1 x 5 and 1 x 1"""
    c, want = BOUNDARIES[name]
    taken = VC.taken_table(want)[0]
    a = VC.as_colouralign(c, twice=True)
    try:
        for form in ("walk", "chunks"):
            ca.target_form(form)
            for stride in (1, 2):
                rule = dict(VC.ONCE, stride=stride)
                got = colouralign_device(ca, a, **rule)
                GC.assert_same(got, AM.run(**a, **rule), (name, form, stride))
                rec, _, _, used = got
                assert (used == 2 * taken[::stride]).all(), (name, form, stride, used)
                assert rec["used"][1, 0] == taken[::stride].sum() and rec["iterations"].tolist() == [0, 1], (name, form, stride)
    finally:
        ca.target_form("auto")


@pytest.mark.parametrize("which", sorted(VC.RANDOM))
def test_three_operators_agree_on_random_views(rc, tx, ca, which):
    """the three device operators on the same vertices, normals, views and planes; 257 x 17 also with each optional input dropped in turn"""
    n, V, seed = VC.RANDOM[which]
    c = random_case(n, V, seed=seed)
    assert all(c[k] is not None for k in OPTIONAL)
    for drop in [()] + ([(k,) for k in OPTIONAL] if which == "257 x 17" else []):
        vert = {}
        for mode in MODES:
            exp = recolour_mirror(c, mode, drop=drop)
            vert[mode] = recolour_device(rc, c, mode, drop)
            assert_bytes(vert[mode], exp, (which, drop, mode, "recolour"))
            if not drop:
                assert (exp["counts"].sum(0) > 0).all()              # every class: no copy of the rule skips a branch
            for patch in (2, 5):
                t = VC.as_texture(c, patch, 3)
                tex = texture_device(tx, t, mode, drop)
                assert_bytes(tex, texture_mirror(t, mode, drop=drop), (which, drop, mode, patch))
                assert_texture_repeats(tex, vert[mode], n, patch, 3, (which, drop, mode, patch))
        a = VC.as_colouralign(VC.without(c, drop))
        exp = AM.run(**a, **VC.ONCE)
        try:
            for form in ("walk", "chunks"):
                ca.target_form(form)
                got = colouralign_device(ca, a, **VC.ONCE)
                GC.assert_same(got, exp, (which, drop, form))
                assert got[3].tobytes() == vert["mean"]["views_used"].tobytes() == vert["best"]["views_used"].tobytes(), (which, drop, form)
        finally:
            ca.target_form("auto")
