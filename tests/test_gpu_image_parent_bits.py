"""The image passes (skh_denoise, skh_temporal, skh_moments, skh_denoise_variance, skh_rectify, skh_rewind_guides) written in shared words (csrc/skh_image.h, DESIGN.md
section 2 "Image passes"): nothing of it may change a bit of an output plane.

The reference is the library of the commit before skh_image.h existed, where every kernel spelled out its own tile decode, taps, footprint and pack pass.
tests/golden/image_passes_parent.json holds what THAT library wrote for every case below -- the SHA-256 of every output plane's bytes, recorded with
`python tests/test_gpu_image_parent_bits.py --record <the parent's hash>` under SKH_LIB=<the parent's library> on an MI355X -- and a case passes when the digests of
this tree's planes equal the recorded ones.  (Byte equality: -0.0 != 0.0 and every NaN payload counts.)  The two level filters and the estimate pass are otherwise
held only inside a float64 bar; here they are held to the parent's bits.  A mismatch is a failure of the code, never a reason to record again.

The inputs are the seeded synthetic planes of the suites of the passes (tests/denoiseref.py, temporalref.py, varianceref.py, rectifyref.py, motionref.py) at
65 x 63 -- a partial tile on both axes, dilated taps that leave the image on every side (a stride of 16 pixels is the widest that still lands inside from both
sides), reprojection footprints that straddle the border -- and at 1 x 1, where every neighbour is clamped."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import denoiseref as D  # noqa: E402
from tests import motionref as M  # noqa: E402
from tests import rectifyref as R  # noqa: E402
from tests import temporalref as T  # noqa: E402
from tests import varianceref as V  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "image_passes_parent.json")
SHAPES = ((65, 63), (1, 1))
INF = float("inf")


@functools.lru_cache(maxsize=None)
def planes(w, h):
    """the suites' synthetic inputs at w x h, made once and never written"""
    return {"denoise": D.synthetic(w, h, seed=w + h), "temporal": T.synthetic(w, h, seed=w + h), "moments": V.synthetic_moments(w, h, seed=w + h),
            "variance": V.synthetic(w, h, seed=w + h), "rectify": R.synthetic(w, h, seed=w + h), "motion": M.synthetic(w, h, seed=w + h)}


def with_flags(p, flags):
    q = np.array(p)
    q["flags"] = flags
    return q


def _denoise(w, h, first, levels, flags):
    def run(ctx):
        s = planes(w, h)["denoise"]
        return [ctx.denoise(s["color"], s, D.params(w, h, first_level=first, levels=levels, flags=flags))]
    return run


def _temporal(w, h, prev, flags):
    def run(ctx):
        s = planes(w, h)["temporal"]
        got = ctx.temporal(s["color"], s, s["prev"] if prev else None, with_flags(s["params"], flags))
        return [got["image"], got["history"], got["motion"]]
    return run


def _moments(w, h, prev):
    def run(ctx):
        s = planes(w, h)["moments"]
        return [ctx.moments(s["color"], s, s["motion"] if prev else None, s["prev_moments"] if prev else None, s["params"])]
    return run


def _variance(w, h, first, levels, sigma, estimate):
    def run(ctx):
        s = planes(w, h)["variance"]
        p = V.vparams(w, h, first_level=first, levels=levels, sigma_luminance=sigma, flags=V.DEMODULATE | V.REMODULATE | (V.ESTIMATE if estimate else 0))
        got = ctx.denoise_variance(s["color"], s, s["moments"], p)
        return [got["image"], got["moments"]]
    return run


def _rectify(w, h, radius, k, info):
    def run(ctx):
        s = planes(w, h)["rectify"]
        got = ctx.rectify(s["image"], s, s["history"], s["fast"], R.params(w, h, radius=radius, k=k), info=info)
        return [got["image"], got["history"]] + ([got["info"]] if info else [])
    return run


def _rewind(w, h):
    def run(ctx):
        s = planes(w, h)["motion"]
        flags = [int(f) for f in s["table"]["flags"]]
        assert 0 in flags and M.MOVED in flags and (M.MOVED | M.DROP) in flags  # an unmoved, a moved and a dropped entry
        ctx.set_instance_motion(s["table"])
        try:
            got = ctx.rewind_guides(s)
        finally:
            ctx.set_instance_motion(None)
        return [got["position"], got["normal"]]
    return run


CASES = {}
for _w, _h in SHAPES:
    _at = "%dx%d" % (_w, _h)
    for _first, _levels in ((0, 1), (0, 5), (4, 1)):
        for _flags in (0, D.DEMODULATE | D.REMODULATE):
            CASES["denoise_%s_first%d_levels%d_flags%d" % (_at, _first, _levels, _flags)] = _denoise(_w, _h, _first, _levels, _flags)
    for _prev in (True, False):
        for _flags in (T.DEMODULATE, 0):
            CASES["temporal_%s_prev%d_flags%d" % (_at, _prev, _flags)] = _temporal(_w, _h, _prev, _flags)
        CASES["moments_%s_prev%d" % (_at, _prev)] = _moments(_w, _h, _prev)
    for _estimate in (True, False):
        for _sigma in (4.0, INF):
            CASES["variance_%s_estimate%d_sigma%g" % (_at, _estimate, _sigma)] = _variance(_w, _h, 0, 3, _sigma, _estimate)
    CASES["variance_%s_first4" % _at] = _variance(_w, _h, 4, 1, 4.0, True)
    for _radius in (1, 2, 3):
        for _info in (True, False):
            CASES["rectify_%s_radius%d_info%d" % (_at, _radius, _info)] = _rectify(_w, _h, _radius, 2.0, _info)
    CASES["rectify_%s_k_inf" % _at] = _rectify(_w, _h, 1, INF, True)
    CASES["rewind_%s" % _at] = _rewind(_w, _h)


def digests(arrays):
    return [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in arrays]


def record(parent):
    """-> the fixture: the digests of every case from whatever library SKH_LIB names (none: this tree's), and the commit it was built from"""
    from strelka_amd import capi

    ctx = capi.Context(0)
    try:
        cases = {}
        for name, run in CASES.items():
            got = run(ctx)
            assert any(np.ascontiguousarray(a).view(np.uint8).any() for a in got) or "1x1" in name, name  # (empty planes would equal empty planes)
            cases[name] = digests(got)
        return {"parent": parent, "cases": cases}
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def ctx():
    from strelka_amd import build, capi

    build.build()
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_fixture_names_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_output_planes_equal_the_parent_librarys(ctx, golden, name):
    got = digests(CASES[name](ctx))
    print(name, got, "recorded", golden[name])
    assert got == golden[name]


if __name__ == "__main__":
    # --record <the parent's hash> [<out.json>, in place of the fixture's path]
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--record", __doc__
    fixture = record(sys.argv[2])
    with open(sys.argv[3] if len(sys.argv) == 4 else GOLDEN, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(fixture["cases"]), "cases from", os.environ.get("SKH_LIB") or "this tree's library")
