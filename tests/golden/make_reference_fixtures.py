"""Records what tests/test_cpu_host.py and tests/test_cpu_surface.py hold the product to from a checkout of the reference, so that those
tests run from this repository alone:

  * reference_config_data/*.ini   the nine configuration / calibration files the reference ships (config_data/; settings only)
  * reference_settings_answers.json   the reference's own INI parser (oracle/_ref/libref_settings.so, built by `make -C oracle REF=<dir>`)
                                  on tests/golden/visodo_test.ini, on every (section, key) of those nine files and on seeded random files that
                                  mix every production of the grammar (the file texts are stored with the answers)
  * reference_surface.json        names: the members the reference application reaches through `visodo_->`, and the `RGBID_SLAM::device::`
                                  functions its tracker and KeyframeAlign call

    python tests/golden/make_reference_fixtures.py <reference checkout>     (run from the repo root, after `make -C oracle REF=<same dir>`)
"""
import ctypes
import glob
import json
import os
import re
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "rgbid-slam_amd"))


def ref_parser():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_settings.so"))

    def get(path, sec, key):
        buf = ctypes.create_string_buffer(8192)
        n = lib.ref_settings_get(path.encode(), sec.encode(), key.encode(), buf, 8192)
        return None if n < 0 else buf.value.decode()
    return get


def random_grammar_cases(n_cases=40, seed=20260929):
    """headers with and without ']', repeated headers, keys before any header, repeated keys, empty keys, empty values, continuation lines
    after accepted, refused and dropped assignments, comments, blank and blank-padded lines"""
    rs = np.random.default_rng(seed)
    secs, keys = ["A", "B", "", "A B"], ["k", "x", "kd", "long key", ""]
    pad = lambda: " " * int(rs.integers(0, 3)) + "\t" * int(rs.integers(0, 2))
    cases = []
    for _ in range(n_cases):
        lines = []
        for _ in range(int(rs.integers(5, 40))):
            kind = int(rs.integers(0, 9))
            s, k = secs[int(rs.integers(0, len(secs)))], keys[int(rs.integers(0, len(keys)))]
            v = " ".join(str(int(q)) for q in rs.integers(0, 99, int(rs.integers(0, 4))))
            if kind == 0: body = ""
            elif kind == 1: body = ("#" if rs.random() < 0.5 else ";") + " note = 1"
            elif kind == 2: body = "[" + pad() + s + pad() + ("]" if rs.random() < 0.8 else "") + (" trailing" if rs.random() < 0.2 else "")
            elif kind in (3, 4, 5): body = k + pad() + "=" + pad() + v + ("= 7" if rs.random() < 0.1 else "")
            elif kind == 6: body = "=" + v
            else: body = v if v else "word"
            lines.append(pad() + body + pad() + ("\r" if rs.random() < 0.1 else ""))
        cases.append(("\n".join(lines) + ("\n" if rs.random() < 0.5 else ""), [(s, k) for s in secs + ["missing"] for k in keys + ["missing"]]))
    return cases


def settings_answers(ref_dir, get):
    from tests.test_cpu_host import QUERIES
    out = {"visodo_test": [[s, k, get(os.path.join(GOLDEN, "visodo_test.ini"), s, k)] for s, k in QUERIES], "config_data": {}, "random_grammar": []}
    dst = os.path.join(GOLDEN, "reference_config_data")
    os.makedirs(dst, exist_ok=True)
    for f in sorted(glob.glob(os.path.join(ref_dir, "config_data", "*.ini"))):
        shutil.copyfile(f, os.path.join(dst, os.path.basename(f)))
        text = open(f).read()
        sections = set(m.strip() for m in re.findall(r"^\s*\[([^\]]*)\]", text, re.M)) | {"VISODO", "CALIBRATION"}
        keys = set(m.strip() for m in re.findall(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s*=", text, re.M)) | {"fx", "kd", "dRc", "t_dc", "q0", "missing"}
        out["config_data"][os.path.basename(f)] = [[s, k, get(f, s, k)] for s in sorted(sections) for k in sorted(keys)]
    tmp = os.path.join(GOLDEN, "_case.ini")
    try:
        for text, queries in random_grammar_cases():
            with open(tmp, "w") as fh:
                fh.write(text)
            out["random_grammar"].append({"text": text, "answers": [[s, k, get(tmp, s, k)] for s, k in queries]})
    finally:
        os.remove(tmp)
    return out


def _strip_comments(txt):
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def surface(ref_dir):
    used = set()
    for f in ("tools/RGBID_SLAMapp.cpp", "src/visualization_manager.cpp", "src/keyframe_manager.cpp"):
        p = os.path.join(ref_dir, f)
        if os.path.exists(p):
            used |= set(re.findall(r"visodo_(?:ptr_)?->\s*([A-Za-z_][A-Za-z_0-9]*)", _strip_comments(open(p).read())))
    called = set()
    for f in ("src/visodo.cpp", "src/keyframe_align.cpp"):
        txt = _strip_comments(open(os.path.join(ref_dir, f)).read())
        called |= set(re.findall(r"\bdevice::([a-z][A-Za-z0-9_]*)\s*(?:<[^>]*>)?\s*\(", txt))
        called |= set(re.findall(r"(?<![A-Za-z_:>.])((?:pyrDown|convert|compute|decompose|copyImage|initialise|buildSystem|warp|integrate|getVisibility|create[VN]Map|generateImage|bilateralFilter|undistort|registerDepthinv)[A-Za-z0-9_]*)\s*(?:<[^>]*>)?\s*\(", txt))
    called -= {"computeInterframeTime", "computeCovisibility", "computeOverlapping", "integrateImagesIntoKeyframes", "integrateCurrentRGBIntoKeyframe", "warpAtLevel",
               "computeErrorGridStride_", "convertTransforms"}      # host-side methods of the tracker itself
    proto = open(os.path.join(ref_dir, "src", "internal.h")).read()
    called = {c for c in called if re.search(r"\b%s\b" % re.escape(c), proto)}   # prototypes of src/internal.h only
    return {"visodo_members": sorted(used), "bridge_functions": sorted(called)}


if __name__ == "__main__":
    ref_dir = sys.argv[1]
    answers = settings_answers(ref_dir, ref_parser())
    with open(os.path.join(GOLDEN, "reference_settings_answers.json"), "w") as fh:
        json.dump(answers, fh, indent=0)
    with open(os.path.join(GOLDEN, "reference_surface.json"), "w") as fh:
        json.dump(surface(ref_dir), fh, indent=1)
    print("config files", len(answers["config_data"]), "random cases", len(answers["random_grammar"]))
