"""The drop-in surface, checked against the reference's own callers (the names they use are recorded in tests/golden/reference_surface.json by
tests/golden/make_reference_fixtures.py): every member / method the reference application and its visualisation thread reach through `visodo_->`
must exist in include/rgbid/visodo.h, every `RGBID_SLAM::device::` function the reference tracker and KeyframeAlign call must be declared in
include/rgbid/internal.h, and INTEGRATION.md must list every caller-side type change (lock type, Eigen getters, keyframe manager, dev_prop)."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_surface.json")))


def _strip_comments(txt):
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def test_every_member_the_reference_application_touches_exists():
    ours = _strip_comments(open(os.path.join(ROOT, "include", "rgbid", "visodo.h")).read())
    used = set(SURFACE["visodo_members"])
    assert len(used) >= 12, used
    missing = sorted(m for m in used if not re.search(r"\b%s\b" % re.escape(m), ours))
    assert not missing, missing


def test_every_bridge_function_the_reference_host_code_calls_is_declared():
    ours = _strip_comments(open(os.path.join(ROOT, "include", "rgbid", "internal.h")).read())
    called = set(SURFACE["bridge_functions"])
    assert len(called) >= 20, called
    missing = sorted(c for c in called if not re.search(r"\b%s\b" % re.escape(c), ours))
    assert not missing, missing


def test_integration_document_lists_every_caller_side_change():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for needle in ("dev_prop", "scoped_try_lock", "std::mutex", "getCameraPose", "Eigen::Affine3f", "keyframe_manager_ptr_", "TrackerSink", "rmatsKF_",
                   "visodo_reference_types.h"):
        assert needle in doc, needle
    assert "the one unavoidable source change" not in doc and "the only edits" not in doc


def test_reference_types_header_compiles_without_eigen_and_boost(tmp_path):
    """the opt-in adapter header is valid C++ in the default configuration (its Eigen / Boost branches need those headers, which this image lacks)"""
    import subprocess
    src = tmp_path / "t.cpp"
    src.write_text('#include "rgbid/visodo_reference_types.h"\nint main() { RGBID_SLAM::compat::mutex m; RGBID_SLAM::compat::mutex::scoped_try_lock l(m); return l ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
