"""What puts one (point, view) pair of the visibility rule -- steps 3 - 4 of include/rgbid_recolour.h -- in front of all three places that
state it: k_recolour_add, k_texture_add and view_device.h's view_sample (colour alignment).  Builders only, plain numpy and the mirrors; the
cases themselves are tests/test_cpu_recolour.py's: BOUNDARIES, every class boundary exact in float32, and random_case.

 texture           as_texture: a triangle (v, v, v) per vertex.  Step 4 of include/rgbid_texture.h gives a texel ((wa A + wb A) + wc A) / D with
                   wa + wb + wc = D = n - 1; for a finite float32 A and |weights| <= 30 every product and sum is exact in double and D A / D is A,
                   so all P texels of the triangle, the gutter's wa = -1 ones included, are the vertex, and its normal mixes the same way.  A
                   component that is not finite stays so.  Hence per view counts == P x recolour's, and atlas, views_used and best_view at the
                   triangle's texels (texel_view) are recolour's outputs of the vertex.
 colour alignment  as_colouralign: the same views with rounds = iterations = 1, so that the target pass runs at the given poses: `used` is
                   recolour's views_used and W plane 3 of its MEAN state (mean_weights).  With the views doubled and the first one held,
                   used == 2 x the views that took the vertex, W == 2 w, and records["used"][1, 0], the pairs the first system of view 1 used, is
                   the number of vertices view 0 took (taken_table): two views meet min_views."""
import numpy as np

from tests import texture_mirror as TM

U32, U64 = np.uint32, np.uint64
ONCE = dict(rounds=1, iterations=1)            # the schedule whose only target pass runs at the poses given
PLANES = ("atlas", "views_used", "best_view")  # texture's outputs, and the recolour output each one repeats
VERTEX_OUTPUT = dict(atlas="colours", views_used="views_used", best_view="best_view")
# random_case(vertices, views, seed=seed) with all six classes (their counts over the views, asserted on the CPU): 17 views are a chunk of
# the add kernels and one, 33 are three launches of them and three blockIdx.y of k_ca_target<true>
RANDOM = {"257 x 17": (257, 17, 41), "65 x 33": (65, 33, 7)}
RANDOM_COUNTS = {"257 x 17": [1351, 1743, 762, 274, 43, 196], "65 x 33": [503, 925, 377, 156, 31, 153]}


def texels(patch):
    """P of include/rgbid_texture.h: the used texels of a triangle"""
    return patch * (patch + 1) // 2 + (patch - 1)


def as_texture(c, patch, tiles_x):
    """a recolour case -> the texture case whose triangle v is (v, v, v)"""
    n = len(c["vertices"])
    return dict(c, triangles=np.repeat(np.arange(n, dtype=U32)[:, None], 3, 1), patch=patch, tiles_x=tiles_x)


def as_colouralign(c, twice=False):
    """a recolour case -> the arguments of colouralign_mirror.run (ColourAligner.run_into takes `params` spread out), the first view held;
    twice: every view a second time behind the first ones"""
    rep = (lambda x: None if x is None else np.concatenate([x, x])) if twice else (lambda x: x)
    return dict(vertices=c["vertices"], normals=c["normals"], R=rep(c["R"]), t=rep(c["t"]), K=c["K"], rows=c["rows"], cols=c["cols"],
                colours=rep(c["colours"]), surface=rep(c["surface"]), depthinv=rep(c["depthinv"]), fixed=(0,), params=dict(c["params"]))


def without(c, drop):
    """the case without the optional inputs named in `drop`"""
    return dict(c, **{k: None for k in drop})


def texel_view(arr, n_t, patch, tiles_x):
    """an atlas-shaped array [H, W, ...] -> [n_t, P, ...]: the used texels of every triangle, in patch_texels' order"""
    col, row = TM.atlas_pixels(n_t, patch, tiles_x)
    return np.asarray(arr)[row, col]


def taken_table(want):
    """BOUNDARIES' class names [view][vertex] -> bool [V, n]: the pair is TAKEN"""
    return np.array(want) == "taken"


def mean_weights(out):
    """W per vertex of a recolour mirror result in MEAN mode: plane 3 of its state"""
    n = len(out["views_used"])
    return np.frombuffer(out["state"][:32 * n], U64).reshape(4, n)[3]
