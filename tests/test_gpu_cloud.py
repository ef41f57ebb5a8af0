"""GPU tests of the keyframe point cloud (include/rgbid_cloud.h, csrc/kernels_cloud.hip, rgbid.cloud): the kernels against the float64
restatement of the reference's computeAlignedPointCloud (tests/test_cpu_cloud.py cloud_numpy) byte for byte, on synthetic blocks and on
the engine's own exports; the chunked run's cloud against its trajectory and the synthetic scene; the --cloud option of
tools/track_dataset.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import cloud as CL
from rgbid import engine as E
from rgbid import sequence, synth, tum
from tests.test_cpu_cloud import cloud_numpy, make_block, records_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SMALL = (synth.TUM_K[0] / 4, synth.TUM_K[1] / 4, (synth.TUM_K[2] + 0.5) / 4 - 0.5, (synth.TUM_K[3] + 0.5) / 4 - 0.5)


def make_lanes(n_lanes, n_frames, rows, cols, K, **kw):
    seqs = [synth.make_sequence(n_frames, seed=synth.SEED + 17 * l, K=K, rows=rows, cols=cols, device="cuda", **kw) for l in range(n_lanes)]
    depth = torch.stack([s["depth"] for s in seqs], 1).to(torch.int16).contiguous()   # [T, B, rows, cols]
    rgb = torch.stack([s["rgb"] for s in seqs], 1).contiguous()                       # [T, B, rows, cols, 3]
    return seqs, depth, rgb


def random_pose(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.normal(scale=2.0, size=3)


def synth_block(rng, rows, cols, kind="mixed"):
    """a packed export block with ~70 % valid pixels: NaN holes of mixed sizes, scattered NaN pixels, NaN normals (x only / y only), the
    special inverse depths 0, -0, negative, inf and denormal, overlap masks 0 / 1 in patches"""
    N = rows * cols
    iD = rng.uniform(0.1, 3.0, (rows, cols)).astype(np.float32)
    nrm = rng.normal(size=(3, rows, cols)).astype(np.float32)
    mask = (rng.random((rows // 4 + 1, cols // 4 + 1)) < 0.5).repeat(4, 0).repeat(4, 1)[:rows, :cols].astype(np.uint8)
    col = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    if kind == "empty":
        iD[:] = np.nan
    elif kind == "mixed":
        for _ in range(6):                                           # holes from one pixel to a quarter of the image
            h, w = rng.integers(1, rows // 2 + 2), rng.integers(1, cols // 2 + 2)
            y, x = rng.integers(0, rows), rng.integers(0, cols)
            iD[y:y + h, x:x + w] = np.nan
        iD[rng.random((rows, cols)) < 0.08] = np.nan
        nrm[0][rng.random((rows, cols)) < 0.05] = np.nan
        nrm[1][rng.random((rows, cols)) < 0.05] = np.nan
        flat = iD.reshape(-1)
        for v in (0.0, -0.0, -1.5, np.inf, -np.inf, float(np.ldexp(np.float32(1), -127)), float(np.ldexp(np.float32(1), -140))):
            flat[rng.integers(0, N, 3)] = v
    else:                                                            # "full": every pixel valid and novel
        mask[:] = 0
    return make_block(mask, col, iD, nrm)


def upload_blocks(blocks, misalign=0):
    """blocks -> one device buffer holding them in reverse order with gaps (and a byte offset) + their device addresses"""
    nb = blocks[0].size
    stride = nb + 256
    buf = torch.zeros(len(blocks) * stride + 256, dtype=torch.uint8, device="cuda")
    addr = []
    for i, b in enumerate(blocks):
        o = (len(blocks) - 1 - i) * stride + misalign
        buf[o:o + nb] = torch.from_numpy(b).cuda()
        addr.append(buf.data_ptr() + o)
    torch.cuda.synchronize()
    return buf, addr


def check_batch(ctx, rows, cols, blocks, poses, K, mode, misalign=0):
    buf, addr = upload_blocks(blocks, misalign)
    srcs = [CL.source(a, R, t) for a, (R, t) in zip(addr, poses)]
    cl = CL.Cloud(ctx, rows, cols, len(blocks))
    pts, off = cl.build(srcs, K, mode)
    cl.close()
    exp = [cloud_numpy(b, rows, cols, K, R, t, mode) for b, (R, t) in zip(blocks, poses)]
    eoff = np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64)
    assert np.array_equal(off, eoff), (off[:8], eoff[:8])
    got = CL.as_numpy(pts)
    ok, first = records_equal(got, np.concatenate(exp))
    assert ok, (first, got[first] if first is not None else None, np.concatenate(exp)[first] if first is not None else None)
    return got, off


@pytest.mark.parametrize("rows,cols", [(120, 160), (480, 640), (97, 131)])
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("mode", ["all", "novel"])
def test_cloud_synthetic_blocks(ctx, rows, cols, n, mode):
    rng = np.random.default_rng(rows * 1000 + cols + 7 * n + (mode == "novel"))
    blocks = [synth_block(rng, rows, cols) for _ in range(n)]
    poses = [random_pose(rng) for _ in range(n)]
    K = (rng.uniform(100, 600), rng.uniform(100, 600), cols / 2 - 0.5, rows / 2 - 0.5)
    got, off = check_batch(ctx, rows, cols, blocks, poses, K, mode)
    assert 0 < len(got) < n * rows * cols
    if n == 7 and rows == 120:                                        # the same keyframes from 4-byte aligned blocks: the scalar path
        check_batch(ctx, rows, cols, blocks, poses, K, mode, misalign=4)


@pytest.mark.parametrize("mode", ["all", "novel"])
def test_cloud_300_keyframes(ctx, mode):
    rows, cols, n = 120, 160, 300
    rng = np.random.default_rng(300 + (mode == "novel"))
    kinds = ["mixed"] * n
    kinds[17], kinds[200] = "empty", "full"
    blocks = [synth_block(rng, rows, cols, k) for k in kinds]
    poses = [random_pose(rng) for _ in range(n)]
    got, off = check_batch(ctx, rows, cols, blocks, poses, K_SMALL, mode)
    assert off[18] == off[17] and off[201] - off[200] == rows * cols


@pytest.mark.parametrize("fast", [0, 1])
def test_cloud_from_engine_exports(ctx, fast):
    """the engine's export ring -> keyframe_sources -> Cloud: byte-identical to the restatement of the same keyframes read back through
    read_keyframe, both modes; 3 lanes with several exports each"""
    rows, cols, n, B = 120, 160, 9, 3
    seqs, depth, rgb = make_lanes(B, n, rows, cols, K_SMALL, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    eng = E.Engine(ctx, E.default_config(rows=rows, cols=cols, lanes=B, K=K_SMALL, record_capacity=n, keyframe_capacity=8, fast_numerics=fast,
                                         visratio_odo=0.985, visratio_integr=0.97))
    for k in range(n):
        eng.step(depth[k], rgb[k])
    counts = eng.keyframe_counts()
    assert (counts >= 2).all(), counts
    pairs = [(l, s) for l in range(B) for s in range(int(counts[l]))][::-1]     # any order of lanes and slots
    srcs, hdrs = eng.keyframe_sources(pairs)
    kfs = [eng.read_keyframe(l, s) for l, s in pairs]
    for h, a in zip(hdrs, kfs):
        assert (h["lane"], h["seq"], h["id"]) == (a["lane"], a["seq"], a["id"]) and np.array_equal(h["R"], a["R"]) and np.array_equal(h["t"], a["t"])
    cl = CL.Cloud(ctx, rows, cols, len(pairs))
    for mode in ("all", "novel"):
        pts, off = cl.build(srcs, K_SMALL, mode)
        exp = [cloud_numpy(make_block(a["overlap_mask"], a["colors"], a["depthinv"], a["normals"]), rows, cols, K_SMALL, a["R"], a["t"], mode)
               for a in kfs]
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64))
        ok, first = records_equal(CL.as_numpy(pts), np.concatenate(exp))
        assert ok, (mode, first)
        assert len(pts) > 0
    cl.close()
    for bad in [(0, int(counts[0])), (B, 0), (1, -1)]:
        with pytest.raises(Exception):
            eng.keyframe_sources([bad])
    eng.close()


def test_keyframe_sources_refuses_lapped_exports(ctx):
    rows, cols, n = 120, 160, 7
    seqs, depth, rgb = make_lanes(1, n, rows, cols, K_SMALL, trans_step=(0.003, 0.012), rot_step_deg=(0.1, 0.8))
    eng = E.Engine(ctx, E.default_config(rows=rows, cols=cols, lanes=1, K=K_SMALL, record_capacity=n, keyframe_capacity=2, max_integrKF_count=1))
    for k in range(n):
        eng.step(depth[k], rgb[k])
    cnt = int(eng.keyframe_counts()[0])
    assert cnt == n - 1
    srcs, hdrs = eng.keyframe_sources([(0, cnt - 1), (0, cnt - 2)])
    assert [h["seq"] for h in hdrs] == [cnt - 1, cnt - 2]
    with pytest.raises(Exception):
        eng.keyframe_sources([(0, cnt - 3)])                           # overwritten by a later export
    eng.close()


def _height_residuals(pc, scene):
    p = pc.numpy()
    xyz = torch.from_numpy(np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64))
    return np.abs((xyz[:, 2] - scene.depth(xyz[:, 0], xyz[:, 1])).numpy())


def test_chunked_cloud_one_chunk_matches_headers(ctx):
    """one chunk: each keyframe's trajectory pose equals its header pose (composition rounding only) and the points equal those placed
    with the header poses"""
    rows, cols, n = 120, 160, 16
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    cfg = dict(visratio_odo=0.985, visratio_integr=0.97)
    R, t, ranges = sequence.track_chunked(ctx, depth, rgb, 1, K_SMALL, **cfg)
    R2, t2, ranges2, pc = sequence.track_chunked(ctx, depth, rgb, 1, K_SMALL, cloud="all", **cfg)
    assert np.array_equal(R, R2) and np.array_equal(t, t2)            # the cloud does not change the trajectory
    assert len(pc.keyframes) >= 2 and len(pc) > 0
    for kf in pc.keyframes:
        assert np.abs(kf["R"] - kf["header_R"]).max() < 1e-9 and np.abs(kf["t"] - kf["header_t"]).max() < 1e-9, kf["frame"]
    # the same keyframes placed with the header poses
    eng = E.Engine(ctx, E.default_config(rows=rows, cols=cols, lanes=1, K=K_SMALL, record_capacity=n, keyframe_capacity=n, **cfg))
    for k in range(n):
        eng.step(depth[k:k + 1], rgb[k:k + 1])
    srcs, _ = eng.keyframe_sources([(0, s) for s in range(len(pc.keyframes))])
    cl = CL.Cloud(ctx, rows, cols, len(srcs))
    pts, off = cl.build(srcs, K_SMALL, "all")
    cl.close(); eng.close()
    assert np.array_equal(off, pc.offsets)
    a, b = CL.as_numpy(pts), pc.numpy()
    assert np.array_equal(a["pixel"], b["pixel"]) and np.array_equal(a["flags"], b["flags"])
    for f in ("x", "y", "z"):
        assert np.nanmax(np.abs(a[f] - b[f])) <= 1e-5, f


def test_chunked_cloud_against_the_scene(ctx):
    """noise-free synthetic sequence in 2 chunks: the world novel cloud lies on the scene's height field z = f(x, y).  Measured on the
    MI355X: median 0.48 mm, no point beyond 2 cm (45 609 points); the bounds keep a margin of about 3x on the median"""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    R, t, ranges, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97)
    assert {kf["chunk"] for kf in pc.keyframes} == {0, 1}
    res = _height_residuals(pc, synth.Scene(seed=synth.SEED))
    res = res[np.isfinite(res)]
    med, far = float(np.median(res)), float((res > 0.02).mean())
    print(f"cloud vs scene: {len(res)} points, median |z - f(x, y)| {med * 1e3:.3f} mm, {100 * far:.3f} % beyond 2 cm")
    assert len(res) > 0.3 * rows * cols
    assert med <= 1.5e-3 and far <= 0.002, (med, far)


def write_tum_folder(root, seq):
    """TUM layout: 16-bit PNG depth = millimetres x 5 (tum.Dataset.grab applies x0.2), 8-bit RGB PNG, association files"""
    d = seq["depth"].cpu().numpy().astype(np.uint32); c = seq["rgb"].cpu().numpy()
    os.makedirs(root / "depth"); os.makedirs(root / "rgb")
    hdr = "# line 1\n# line 2\n# timestamp filename\n"
    dl, cl = [], []
    for k in range(d.shape[0]):
        st = 1305031102.175304 + k / 30.0
        tum.write_png(str(root / "depth" / f"{st:.6f}.png"), (d[k] * 5).astype(np.uint16))
        tum.write_png(str(root / "rgb" / f"{st:.6f}.png"), c[k])
        dl.append(f"{st:.6f} depth/{st:.6f}.png"); cl.append(f"{st:.6f} rgb/{st:.6f}.png")
    (root / "depth_associated.txt").write_text(hdr + "\n".join(dl) + "\n")
    (root / "rgb_associated.txt").write_text(hdr + "\n".join(cl) + "\n")


def test_track_dataset_cloud_option(ctx, tmp_path):
    rows, cols, n = 120, 160, 30
    # enough motion for the default visibility thresholds (0.9 / 0.7) to switch the integration keyframe in each 15-frame chunk
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    ds = tum.Dataset(str(root))
    g = ds.grab(5, rows, cols)
    assert np.array_equal(g[0], seq["depth"][5].cpu().numpy().astype(np.uint16)) and np.array_equal(g[1], seq["rgb"][5].cpu().numpy())
    ds.close()
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    outs = {}
    for name, extra in (("plain", []), ("cloud", ["--cloud", str(tmp_path / "map.ply")])):
        out = tmp_path / f"traj_{name}.txt"
        r = subprocess.run(base + ["--out", str(out)] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out.read_bytes()
    assert outs["plain"] == outs["cloud"]
    data = (tmp_path / "map.ply").read_bytes()
    head, body = data.split(b"end_header\n", 1)
    nv = int([l for l in head.split(b"\n") if l.startswith(b"element vertex")][0].split()[-1])
    assert nv > 0 and len(body) == 27 * nv
    # the same run in process
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    R, t, ranges, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0)
    assert {kf["chunk"] for kf in pc.keyframes} == {0, 1}                # every chunk exported
    assert len(pc) == nv
    assert CL.ply_bytes(pc.points) == data
