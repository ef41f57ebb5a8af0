"""CPU checks of tests/view_rule_cases.py: that its builders put every boundary case of tests/test_cpu_recolour.py (BOUNDARIES) and its random
cases in front of the texture and the colour-alignment mirrors exactly as the recolour mirror sees them -- the three mirrors are related as
that file's docstring says, for both modes and patches 2, 3, 6 and 30; that the scalar restatements (texture_mirror.texture_loop,
colouralign_mirror.pair_loop and terms_loop) give the vectorised mirrors' bytes on these cases too; and that the random cases hold every
one of the six classes, so that none of the three copies of the rule can skip a branch unnoticed on them."""
import numpy as np
import pytest

from tests import colouralign_mirror as AM
from tests import recolour_mirror as CM
from tests import view_rule_cases as VC
from tests.render_mirror import pose_cw
from tests.test_cpu_recolour import BOUNDARIES, OPTIONAL, mirror as recolour, random_case
from tests.test_cpu_texture import loops as texture_loops, mirror as texture, same

D = np.float64
PATCHES = (2, 3, 6, 30)
FACING_WEIGHTS = [1024, 819, 0, 1024, 1024, 1024, 0, 1024, 1024]        # test_boundary_weights' hand-derived values


def assert_texture_repeats_recolour(c, patch, tiles_x, mode, rc=None, drop=()):
    """the texture mirror on the degenerate triangles against the recolour mirror on the vertices"""
    c = VC.without(c, drop)
    n, P = len(c["vertices"]), VC.texels(patch)
    rc = recolour(c, mode) if rc is None else rc
    tx = texture(VC.as_texture(c, patch, tiles_x), mode)
    assert (tx["counts"] == P * rc["counts"]).all(), (tx["counts"], rc["counts"])
    for plane in VC.PLANES[:3 if mode == "best" else 2]:
        got, want = VC.texel_view(tx[plane], n, patch, tiles_x), rc[VC.VERTEX_OUTPUT[plane]]
        assert got.shape[:2] == (n, P) and (got == want[:, None]).all(), (plane, patch, tiles_x)
    return tx


def colouralign(c, twice=False, **rule):
    return AM.run(**VC.as_colouralign(c, twice), **dict(VC.ONCE, **rule))


def assert_colouralign_repeats_recolour(c, rc, drop=()):
    """the colour-alignment mirror's target pass at the given poses against the recolour mirror's MEAN result"""
    out = colouralign(VC.without(c, drop))
    assert out["used"].tobytes() == rc["views_used"].tobytes() and out["W"].tobytes() == VC.mean_weights(rc).tobytes()
    return out


# ---- the builders --------------------------------------------------------------------------------------------------------------------------
def test_the_builders():
    c, want = BOUNDARIES["facing"]
    t = VC.as_texture(c, 3, 2)
    assert t["triangles"].tolist() == [[v] * 3 for v in range(9)] and t["triangles"].dtype == np.uint32 and (t["patch"], t["tiles_x"]) == (3, 2)
    assert t["vertices"] is c["vertices"] and VC.texels(2) == 4 and VC.texels(3) == 8 and VC.texels(30) == 494
    a, b = VC.as_colouralign(c), VC.as_colouralign(c, twice=True)
    assert len(a["R"]) == 1 and len(b["R"]) == len(b["t"]) == len(b["colours"]) == 2 and b["surface"] is None and a["fixed"] == (0,)
    assert b["colours"][0].tobytes() == b["colours"][1].tobytes() == c["colours"][0].tobytes()
    assert VC.taken_table(want).tolist() == [[True, True, False, True, True, True, False, True, True]]
    plane = np.arange(4 * 8).reshape(4, 8)                       # patch 2 (T = 4), three triangles, two tiles beside each other: H = 4, W = 8
    view = VC.texel_view(plane, 3, 2, 2)                         # the lower half row by row; the upper half is the tile turned by 180 degrees
    assert view.shape == (3, 4) and view[0].tolist() == [0, 1, 8, 9] and view[1].tolist() == [27, 26, 19, 18] and view[2].tolist() == [4, 5, 12, 13]
    assert VC.without(c, ("normals",))["normals"] is None and c["normals"] is not None


# ---- every boundary case through the texture mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_texture_mirror_at_the_class_boundaries(name):
    c, _ = BOUNDARIES[name]
    for mode in ("mean", "best"):
        rc = recolour(c, mode)
        for k, patch in enumerate(PATCHES):
            assert_texture_repeats_recolour(c, patch, (1, 3)[k & 1], mode, rc)


# ---- every boundary case through the colour-alignment mirror ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_colouralign_mirror_at_the_class_boundaries(name):
    c, want = BOUNDARIES[name]
    rc = recolour(c)
    taken, w = VC.taken_table(want), VC.mean_weights(rc)
    assert (rc["views_used"] == taken.sum(0)).all() and ((w > 0) == taken[0]).all()
    once = assert_colouralign_repeats_recolour(c, rc)
    assert once["records"]["status"].tolist() == [AM.FIXED]
    two = colouralign(c, twice=True)
    assert (two["used"] == 2 * taken[0]).all() and (two["W"] == 2 * w).all()
    assert two["records"]["used"][1, 0] == two["records"]["used"][1, 1] == taken.sum() and two["records"]["iterations"].tolist() == [0, 1]
    if name == "facing":
        assert two["W"].tolist() == [2 * x for x in FACING_WEIGHTS]
    lattice = colouralign(c, twice=True, stride=2)
    assert (lattice["used"] == 2 * taken[0, ::2]).all() and (lattice["W"] == 2 * w[::2]).all() and lattice["records"]["used"][1, 0] == taken[0, ::2].sum()


# ---- the scalar restatements on these cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_scalar_restatements_at_the_class_boundaries(name):
    c, want = BOUNDARIES[name]
    for mode in ("mean", "best"):
        for patch, tiles_x in ((2, 3), (3, 1)):
            t = VC.as_texture(c, patch, tiles_x)
            assert same(texture(t, mode), texture_loops(t, mode)), (mode, patch)
    a = VC.as_colouralign(c, twice=True)
    n, V, prm = len(a["vertices"]), len(a["R"]), a["params"]
    ms = [pose_cw(a["R"][v], a["t"][v]) for v in range(V)]
    plane = lambda key, v: None if a[key] is None else a[key][v]
    pairs = [[AM.pair_loop(a["vertices"][i], None if a["normals"] is None else a["normals"][i], ms[v], a["K"], a["rows"], a["cols"], a["colours"][v],
                           plane("surface", v), plane("depthinv", v), prm) for i in range(n)] for v in range(V)]
    assert [[p is not None for p in per_view] for per_view in pairs] == VC.taken_table(want).tolist() * 2
    S, W, used = AM.targets(a["vertices"], a["normals"], ms, a["K"], a["rows"], a["cols"], a["colours"], a["surface"], a["depthinv"], prm)
    for i in range(n):
        got = [p[i] for p in pairs if p[i] is not None]
        assert int(used[i]) == len(got) and int(W[i]) == sum(g["w"] for g in got) and int(S[i]) == sum(g["w"] * g["s"] for g in got)
    has, C = AM.target_values(S, W, used, 2)
    for huber in (16.0, 0.5):
        for v in range(V):
            u, t = AM.terms(a["vertices"], a["normals"], ms[v], a["K"], a["rows"], a["cols"], a["colours"][v], plane("surface", v), plane("depthinv", v),
                            prm, has, C, huber)
            for i in range(n):
                assert bool(u[i]) == (pairs[v][i] is not None)          # a vertex one view took has its two views
                one = AM.terms_loop(pairs[v][i], a["vertices"][i], ms[v], a["K"], C[i], huber) if u[i] else [0.0] * 28
                assert np.array(one, D).tobytes() == t[:, i].tobytes(), (v, i)


# ---- the random cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(VC.RANDOM))
def test_three_mirrors_agree_on_random_views(which):
    n, V, seed = VC.RANDOM[which]
    c = random_case(n, V, seed=seed)
    rc = {mode: recolour(c, mode) for mode in ("mean", "best")}
    total = rc["mean"]["counts"].sum(0)
    print("classes:", dict(zip(CM.COUNTS, total.tolist())))
    assert (total > 0).all() and total.tolist() == VC.RANDOM_COUNTS[which]        # a condition on the inputs: every branch of the rule is met
    assert (rc["mean"]["views_used"] == 0).any() and (rc["mean"]["views_used"] >= 2).any()
    for mode in ("mean", "best"):
        for patch in (2, 5):
            assert_texture_repeats_recolour(c, patch, 3, mode, rc[mode])
    out = assert_colouralign_repeats_recolour(c, rc["mean"])
    assert (out["records"]["used"][1:, 0] <= (out["used"] >= 2).sum()).all() and out["records"]["used"][1:, 0].any()
    if which == "257 x 17":
        for drop in OPTIONAL:
            part = recolour(c, "mean", drop=(drop,))
            assert_texture_repeats_recolour(c, 2, 3, "mean", part, drop=(drop,))
            assert_colouralign_repeats_recolour(c, part, drop=(drop,))
