"""The odometry-keyframe switch chain builds the bilateral-filtered keyframe maps and their Sobel pairs only as far as something reads them, which
may not change a single bit of what the engine computes:

1. the trimmed chain against RGBID_ENGINE_FULL_FILTERED_PYRAMID=1 (the reference's whole chain, all maps allocated), each in a fresh engine;
2. RGBID_FILTER_GRADS reads every level: the switch changes neither its results nor its allocation;
3. rgbid_engine_bytes shrinks by exactly the maps that are no longer allocated.

Geometries: the step ledger's own -- 120 x 160 with 3 levels (every vectorised path) and 122 x 166 with 2 levels (cols % 4 != 0: the fallbacks).  8 frames with
max_odoKF_count = 2 and max_integrKF_count = 3 (the covisibility thresholds at their defaults, which these slow sequences do not reach): every lane switches its
odometry keyframe at least twice after the first frame (asserted on the status bits), and integration keyframes are switched and exported."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from rgbid import engine as E

pytestmark = pytest.mark.gpu

T = 8
GEOM = {"vec": (120, 160, 3, 3), "odd": (122, 166, 2, 2)}   # rows, cols, levels, lanes
ENV_KEYS = ("RGBID_ENGINE_FULL_FILTERED_PYRAMID", "RGBID_ENGINE_MAP_SKEW", "RGBID_ENGINE_LANE_PAD")
MAP_SKEW = 0x1100   # the engine's default skew between the maps of one allocation order


def intrinsics(rows, cols):
    s = cols / 640.0
    return (525.0 * s, 525.0 * s, (319.5 + 0.5) * s - 0.5, (239.5 + 0.5) * rows / 480.0 - 0.5)


@pytest.fixture(scope="module")
def frames():
    """per geometry: K, depth [T, B, rows, cols] (int16 bits of the u16 frame), rgb.  The corner pixels of every frame hold depth 0 (invalid), 65 535, 12 000
    and 10 001 (all three above the 10 m clamp)"""
    from tests.test_gpu_engine import make_lanes
    out = {}
    for name, (rows, cols, levels, lanes) in GEOM.items():
        K = intrinsics(rows, cols)
        _, depth, rgb = make_lanes(lanes, T, rows, cols, K, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
        depth[:, :, 0, 0] = 0
        depth[:, :, 0, -1] = -1        # 65 535
        depth[:, :, -1, 0] = 12000
        depth[:, :, -1, -1] = 10001
        out[name] = (K, depth, rgb)
    return out


class env:
    """the engine's environment switches for the engines created inside the block; every other switch of ENV_KEYS is unset there"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ENV_KEYS}
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        for k, v in self.kv.items():
            assert k in ENV_KEYS
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def config(geom, K, **cfg_kw):
    rows, cols, levels, lanes = GEOM[geom]
    kw = dict(rows=rows, cols=cols, levels=levels, lanes=lanes, K=K, record_capacity=T, keyframe_capacity=4, max_odoKF_count=2, max_integrKF_count=3, use_graph=0)
    if levels == 2:
        kw["iters"] = [6, 4]
    kw.update(cfg_kw)
    return E.default_config(**kw)


def run(ctx, geom, frames, environment, **cfg_kw):
    """records, keyframe maps of every lane, keyframe counts, exported keyframes and rgbid_engine_bytes of a fresh engine over the T frames"""
    K, depth, rgb = frames[geom]
    B = GEOM[geom][3]
    with env(**environment):
        eng = E.Engine(ctx, config(geom, K, **cfg_kw))
        for k in range(T):
            eng.step(depth[k], rgb[k])
        rec = eng.records().copy()
        maps = [np.concatenate([m.reshape(-1).view(np.uint8) for m in eng.keyframe_maps(l)]) for l in range(B)]
        counts = [int(v) for v in eng.keyframe_counts()]
        kfs = []
        for l in range(B):
            for i in range(max(0, counts[l] - 4), counts[l]):
                a = eng.read_keyframe(l, i)
                kfs.append(b"".join(np.ascontiguousarray(a[k]).tobytes() for k in sorted(a) if isinstance(a[k], np.ndarray)) + repr((a["id"], a["end_id"], a["lane"], a["seq"])).encode())
        nbytes = eng.bytes()
        eng.close()
    return rec, maps, counts, kfs, nbytes


def assert_same_run(a, b):
    assert a[0].tobytes() == b[0].tobytes(), "pose records (every field, the covariances included)"
    assert a[2] == b[2], "keyframe counts"
    assert a[3] == b[3], "exported keyframes"
    assert len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])), "keyframe maps"


def assert_switched(rec):
    """every lane tracked and switched its odometry keyframe at least twice after the first frame"""
    st = rec["status"]
    assert np.all(st[0] & E.ST_FIRST)
    for l in range(st.shape[1]):
        assert all(st[k, l] & E.ST_TRACKED for k in range(1, T)), (l, st[:, l])
        assert sum(1 for k in range(1, T) if st[k, l] & E.ST_ODO_KF) >= 2, (l, st[:, l])


def pitched(rows, cols, lanes):
    return ((cols * 4 + 255) & ~255) * rows * lanes


# the maps of one level in allocation order (two frame buffers come first): position in the order decides the map's skew slot
PER_LEVEL = ("iD_curr", "I_curr", "iD_kf", "I_kf", "iD_kf_f", "I_kf_f", "gxI", "gyI", "gxD", "gyD", "gxI_c", "gyI_c", "gxD_c", "gyD_c", "wiD", "wI")


def dropped_bytes(rows, cols, levels, lanes, finest_level, skew):
    """what the default configuration does not allocate: iD_kf_f / I_kf_f below finest_level, the four g*_c maps of every level but finest_level"""
    total = 0
    for l in range(levels):
        names = (["iD_kf_f", "I_kf_f"] if l > finest_level else []) + (["gxI_c", "gyI_c", "gxD_c", "gyD_c"] if l != finest_level else [])
        for n in names:
            slot = (2 + 16 * l + PER_LEVEL.index(n)) % 16
            total += pitched(rows >> l, cols >> l, lanes) + skew * slot
    return total


# ---- 1. the trimmed chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,geom,cfg_kw", [
    ("default", "vec", {}),
    ("exact class", "vec", dict(fast_numerics=0)),
    ("unfused Gauss-Newton", "vec", dict(fused_gn=0)),
    ("finest level 1", "vec", dict(finest_level=1, iters=[0, 6, 4])),    # the filtered pyrDown to level 1 still runs, the Sobel pair at level 1 only
    ("a level without iterations", "vec", dict(iters=[10, 0, 3])),
    ("graph replay", "vec", dict(use_graph=1)),
    ("odd size, 2 levels", "odd", {}),
])
def test_trimmed_chain_is_bit_identical_to_the_full_chain(ctx, frames, name, geom, cfg_kw):
    new = run(ctx, geom, frames, {}, **cfg_kw)
    full = run(ctx, geom, frames, {"RGBID_ENGINE_FULL_FILTERED_PYRAMID": "1"}, **cfg_kw)
    assert_switched(new[0])
    assert sum(new[2]) > 0   # keyframes were exported
    assert_same_run(new, full)
    assert new[4] < full[4]


# ---- 2. RGBID_FILTER_GRADS reads every level -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["vec", "odd"])
def test_filtered_gradients_are_untouched(ctx, frames, geom):
    a = run(ctx, geom, frames, {}, image_filtering=O.FILTER_GRADS)
    b = run(ctx, geom, frames, {"RGBID_ENGINE_FULL_FILTERED_PYRAMID": "1"}, image_filtering=O.FILTER_GRADS)
    assert_switched(a[0])
    assert_same_run(a, b)
    assert a[4] == b[4]   # all levels still allocated


# ---- 3. allocation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,finest_level", [("vec", 0), ("vec", 1), ("vec", 2), ("odd", 0), ("odd", 1)])
@pytest.mark.parametrize("skew", [0, MAP_SKEW])
def test_engine_bytes_shrink_by_the_dropped_maps(ctx, geom, finest_level, skew):
    """rgbid_engine_bytes of the default configuration against the full allocation: the difference is the pitched size of every dropped map (rows x the row
    pitch of 256-byte multiples x lanes) -- plus, with the default placement, the skew of the slot the map would have taken (the slot stays reserved, so every other
    map keeps its place).  No step is run."""
    rows, cols, levels, lanes = GEOM[geom]
    K = intrinsics(rows, cols)
    sizes = []
    for full in ("0", "1"):
        with env(RGBID_ENGINE_FULL_FILTERED_PYRAMID=full, RGBID_ENGINE_MAP_SKEW=str(skew)):
            eng = E.Engine(ctx, config(geom, K, finest_level=finest_level, iters=[0 if l < finest_level else 4 for l in range(levels)]))
            sizes.append(eng.bytes())
            eng.close()
    want = dropped_bytes(rows, cols, levels, lanes, finest_level, skew)
    assert want > 0 and sizes[1] - sizes[0] == want, (sizes, want)
