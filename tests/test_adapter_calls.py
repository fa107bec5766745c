"""include/ndt_matcher_hip.hpp against a recording stand-in for the library (tests/cpp/adapter_stub.cpp): which C functions
every public member of the adapter calls, in which order, with which arguments - the poses, tables and clouds it packs by
their contents - and every field of what it returns, for ndt2d_* and for ndt3d_*, with every call succeeding and with
every call failing.  The expectation, tests/golden/adapter_calls.txt, was recorded from the header in which the 2D and
the 3D classes were two texts (tests/golden/make_adapter_calls_golden.py), not from the header under test.  The program
runs under AddressSanitizer and UndefinedBehaviorSanitizer.  Needs neither a device nor the built library.

A pose packed in the wrong field order, a `where` string that names another entry point, a destroy after a failed create,
a k that is clamped before it is passed on: each changes a line of the record."""
import difflib

import adapter_calls as AC

MATCHER = ["defaultParams", "setTarget", "reserveTarget", "addTargetPoints", "addTargetPointsDev", "removeTargetPoints",
           "removeTargetPointsDev", "gridInfo", "saveMap", "loadMap", "coarsenInto", "align", "alignDev", "alignMultiStartDev",
           "alignMultiScanDev", "searchDev", "searchAlignDev", "scorePosesDev", "stream", "sweepMotion", "deskewPointsDev",
           "scoreParticlesDev", "scoreParticlesAsync", "scoreParticles", "bestPosesDev", "bestPosesAlignDev", "fitPointsDev",
           "selectPointsDev", "voxelFilterDev", "mergeMap", "unmergeMap", "alignMap", "alignMapMulti", "evaluateMap", "searchMap",
           "searchMapScores", "searchAlignMap", "scoreMapPosesDev", "bestMapPosesDev", "bestMapPosesAlignDev", "raw"]
ONLY_2D = ["polarToPointsDev", "to_search_hit", "evaluate"]
ONLY_3D = ["setTuning", "setNeighbourhood", "neighbourhood", "rangeImageToPointsDev", "toSearchHit", "toMatchResult"]
OTHERS = {
    "NdtPyramidHip": ["NdtPyramidHip", "setTarget", "align"],
    "NdtBatchHip": ["NdtBatchHip", "standardPyramid", "setTuning", "align"],
    "NdtMultiHip": ["NdtMultiHip", "deviceCount", "align", "alignDev"],
    "NdtBatchHip3": ["NdtBatchHip3", "setTuning", "align", "alignDev", "stream"],
    "NdtMultiHip3": ["NdtMultiHip3", "deviceCount", "raw"],
}
FREE = ["invert3", "invert6", "to_match_result", "covarianceInLocalFrame", "rotationOf", "covarianceInLocalFrame3"]


def test_the_record_equals_the_one_of_the_two_class_header():
    got, want = AC.record(), open(AC.GOLDEN).read()
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "golden", "record", lineterm="", n=1))
        raise AssertionError("\n".join(line[:300] for line in diff[:60]))


def test_every_public_member_has_a_section_in_both_dimensions():
    parsed, calls = AC.parse(AC.record()), AC.calls()
    want = list(FREE)
    want += [f"{cls}.{m}" for cls, only in (("NdtMatcherHip", ONLY_2D), ("NdtMatcherHip3", ONLY_3D))
             for m in [cls, *MATCHER, *only]]
    want += [f"{cls}.{m}" for cls, ms in OTHERS.items() for m in ms]
    for name in want:
        assert name in calls, f"{name} has no section"
    # ... and nothing pure among them but the free functions and the conversions: every other member reaches the library
    pure = set(FREE) - {"to_match_result"} | {"NdtMatcherHip.to_search_hit", "NdtMatcherHip3.toSearchHit",
                                              "NdtMatcherHip3.toMatchResult", "NdtMatcherHip.raw", "NdtMatcherHip3.raw", "NdtMultiHip3.raw"}
    for name in want:
        assert bool(calls[name]) == (name not in pure), (name, calls[name])
    # the 2D and the 3D member of a name call the same entry points of their own prefix
    for m in MATCHER:
        if m == "alignMultiStartDev":                       # 3D builds it on alignMultiScanDev
            continue
        # the 2D results carry the calibrated covariance; 3D alignDev and alignMultiScanDev take no producer stream
        aside = {"calibrated_covariance"} | ({"wait_stream"} if m in ("alignDev", "alignMultiScanDev") else set())
        c2, c3 = AC.called_by(m)
        assert all(f.startswith("ndt2d_") for f in c2) and all(f.startswith("ndt3d_") for f in c3), m
        # (once each: a 2D member with a std::vector overload is called more often)
        assert list(dict.fromkeys(f[6:] for f in c2 if f[6:] not in aside)) == list(dict.fromkeys(f[6:] for f in c3)), m
    # every section that reaches the library ran in the two failing modes too (a destructor has no status to report)
    for (name, mode), fns in parsed.items():
        if mode == "ok" and fns and ".~" not in name:
            assert (name, "fail") in parsed and (name, "fail-after-wait") in parsed, name


def test_every_status_the_adapter_checks_was_seen_failing():
    """A section ends at its first throw, so a later call of the same body never runs in the failing modes: every entry
    point that returned a status while all succeeded must also have returned the error somewhere, or the `where` string
    and the check behind it are not pinned.  The destroy functions are the exception: a destructor reports nothing."""
    seen = AC.statuses(AC.record())
    assert len(seen) > 100
    for fn, by_mode in seen.items():
        if fn.endswith("_destroy"):
            continue
        assert 0 in by_mode.get("ok", ()), fn
        # (behind a wait for the producer stream, a call is reached only where that wait succeeds)
        assert -1 in by_mode.get("fail", set()) | by_mode.get("fail-after-wait", set()), f"{fn} is never seen failing"


def test_a_failed_create_is_not_followed_by_a_destroy():
    parsed = AC.parse(AC.record())
    seen = 0
    for (name, mode), fns in parsed.items():
        if mode != "ok" and any("create" in f for f in fns):
            assert not any("destroy" in f for f in fns), (name, mode, fns)
            seen += 1
    assert seen >= 2 * 9                                       # the constructors of the nine classes, both failing modes
