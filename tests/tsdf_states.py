"""States of the TSDF volume that no integration of clean data produces, for the CPU and GPU tests of include/rgbid_tsdf.h: counts at and
next to the cap of 65 535 with colour sums that wrap modulo 2^32, a designed walk of W and Cn onto the cap at every view index either side
of the view chunk, and D planes that hold NaN, infinities, signed zeros, denormals and values next to the largest float32.  Everything is
built on the mixed volume (24 x 20 x 16 voxels) and the 48 x 64 views of tests/test_cpu_tsdf.py, deterministic and seeded; every call
returns a fresh copy.  tests/test_cpu_tsdf_states.py asserts, on the mirror alone, that the states reach what they are meant to reach."""
import functools

import numpy as np

from tests import tsdf_mirror as TM
from tests.test_cpu_tsdf import GATE, mixed_scene, mixed_volume
from tests.test_cpu_consist import K

F = np.float32
CAP = TM.MAX_W
VIEWS = 17                              # RGBID_TSDF_VIEW_CHUNK + 1: one full launch and the first view of a second one
WALK = 19                               # bands k = 0 .. 18 of the cap walk: 17 views reach the cap for k <= 17 at the most
# the bits of the kinds of D: a quiet NaN, a negative signalling NaN with a payload (whatever is propagated from it shows its sign and
# payload), infinities, signed zeros, the smallest and a larger denormal, values next to the largest float32
POISON = {name: np.array([v], F).view(np.uint32)[0] for name, v in
          (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("-0", -0.0), ("+0", 0.0), ("+1e-45", 1e-45), ("-1e-45", -1e-45),
           ("+1e-39", 1e-39), ("-1e-39", -1e-39), ("+3e38", 3e38), ("-3e38", -3e38))}
POISON["-snan"] = np.uint32(0xFFA00001)
# (inside end, +x neighbour): inf / inf, D_b = +0 and -0 (t = 1), a denormal difference, a difference that overflows, a NaN that is
# propagated instead of generated
PAIRS = (("-inf", "+inf"), ("-inf", "+0"), ("-1e-45", "+0"), ("-1e-45", "-0"), ("-1e-39", "+1e-39"), ("-3e38", "+3e38"), ("-inf", "nan"),
         ("-3e38", "+inf"))
ALIGN_OFFSET = np.array([0.01, -0.005, 0.008])
ALIGN_LEVELS = ((2, 3), (1, 3))


def views(a=0, b=VIEWS, without_colour=()):
    """views a .. b - 1 of the 19-view mixed scene as integrate's arguments: dict(R, t, planes, colours), colours a list (None at the
    indices, counted from view 0, in `without_colour`)"""
    sc = mixed_scene(19)
    cols = [None if i in without_colour else sc["colours"][i] for i in range(a, b)]
    return dict(R=sc["R"][a:b], t=sc["t"][a:b], planes=sc["planes"][a:b], colours=cols)


def integrate(vol, sc):
    return TM.integrate(vol, sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)


def clone(vol):
    out = TM.Volume(vol.nx, vol.ny, vol.nz, vol.origin, vol.voxel, vol.trunc, colour=vol.colour)
    out.set_state(vol.D, vol.counts(), vol.rgb)
    return out


@functools.lru_cache(maxsize=None)
def _clean():
    sc = mixed_scene(3)
    return TM.integrate(mixed_volume(), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)


def clean_state():
    """the mixed volume after the three views of mixed_scene(3)"""
    return clone(_clean())


def saturate(vol, rng):
    """every touched voxel: W and, independently, Cn in 65 530 .. 65 535, each colour sum in [2^32 - 3000, 2^32)"""
    touched = vol.W > 0
    n = int(touched.sum())
    vol.W[touched] = rng.integers(CAP - 5, CAP + 1, n).astype(np.uint32)
    vol.Cn[touched] = rng.integers(CAP - 5, CAP + 1, n).astype(np.uint32)
    # a uniform draw from the 3 000 values would wrap one sum in fifteen (a voxel takes min(65 535 - W, 65 535 - Cn), 1.5 on average,
    # more colours of 127 on average): half of the sums lie within 256 of 2^32 instead, so that wrapped and unwrapped sums are both many
    gap = np.where(rng.random((3, n)) < 0.5, rng.integers(1, 257, (3, n)), rng.integers(1, 3001, (3, n)))
    vol.rgb[:, touched] = ((1 << 32) - gap).astype(np.uint32)
    return vol


def saturated_state(seed=11):
    return saturate(clean_state(), np.random.default_rng(seed))


def cap_walk_state():
    """designed: voxel (i, j, k) has W = 65 535 - i mod 19 and Cn = 65 535 - j mod 19 (the volume is 24 x 20 voxels across, so every band
    and every crossing exists, Cn above, at and below W), D of the clean state and the sums of a mean colour"""
    vol = clean_state()
    i, j = np.arange(vol.nx) % WALK, np.arange(vol.ny) % WALK
    # contiguous planes: the mirror's integrate works on flat views of them
    vol.W = np.ascontiguousarray(np.broadcast_to((CAP - i)[None, None, :], vol.shape), np.uint32)
    vol.Cn = np.ascontiguousarray(np.broadcast_to((CAP - j)[None, :, None], vol.shape), np.uint32)
    mean = np.random.default_rng(3).integers(0, 256, (3,) + vol.shape).astype(np.uint32)
    vol.rgb = mean * vol.Cn[None]
    return vol


def poison(vol, rng, n, pairs_each):
    """n touched voxels get a random kind of POISON, then `pairs_each` x-neighbours of touched voxels get each pair of PAIRS; vol.poison
    maps a kind to the linear indices that hold it"""
    D, W = vol.D.reshape(-1).view(np.uint32), vol.W.reshape(-1)           # the bits: no conversion touches a signalling NaN
    assert np.shares_memory(D, vol.D)
    names = list(POISON)
    touched = np.nonzero(W > 0)[0]
    pick = rng.choice(touched, n, replace=False)
    D[pick] = np.array([POISON[names[k]] for k in rng.integers(0, len(names), n)], np.uint32)
    cand = touched[touched % vol.nx + 1 < vol.nx]
    cand = rng.permutation(cand[W[cand + 1] > 0])
    written, taken, it = set(pick.tolist()), set(), iter(cand.tolist())
    for a, b in PAIRS * pairs_each:
        p = next(x for x in it if not {x, x + 1} & taken)
        taken |= {p, p + 1}
        D[p], D[p + 1] = POISON[a], POISON[b]
    written = np.array(sorted(written | taken), np.int64)
    vol.poison = {name: written[D[written] == v] for name, v in POISON.items()}
    assert sum(len(x) for x in vol.poison.values()) == len(written)
    return vol


def poisoned_state(seed=9, n=600, pairs_each=6):
    return poison(clean_state(), np.random.default_rng(seed), n, pairs_each)


def align_nan_case(alternate=False):
    """the one way a D that is not finite reaches the alignment's sums: a pixel is used only with |f| < trunc, which NaN and infinity
    fail, but a fraction of exactly 0 hides a corner from f and not from the gradient.  View 0 of the threshold scene's case "edges"
    (tests/test_cpu_align.py) has fx_ = 0 in pixel column 0; with D = 3e38 in the voxel column i = 1 those pixels have f = 0, an infinite
    J_0 and the products inf 0 = NaN.  With `alternate` the column holds 3e38 (-1)^(j + k): Gx is inf - inf, so J_0 is a float32 NaN and
    the second operand of the difference J_5 = px J_1 - py J_0, where the device's subtraction turns a NaN's sign and x86's does not:
    -> (volume, planes, R, t, the arguments of align after cols)"""
    from tests.test_cpu_align import th_align
    vol, planes, R, t, a = th_align("edges", [0])
    vol = clone(vol)
    sign = (-1.0) ** (np.arange(vol.ny)[None, :] + np.arange(vol.nz)[:, None]) if alternate else 1.0
    vol.D[:, :, 1] = (F(3e38) * sign).astype(F)
    return vol, planes, R, t, a


def cast_views():
    """the poses of mixed_scene(3), all of which see the surface: -> (R, t)"""
    sc = mixed_scene(3)
    return sc["R"], sc["t"]


def align_views():
    """the three views of mixed_scene(3) from poses moved by ALIGN_OFFSET: -> (planes, R, t)"""
    sc = mixed_scene(3)
    return sc["planes"], sc["R"], sc["t"] + ALIGN_OFFSET
