"""k_shade's builds by bounce position (FIRST / MIDDLE / LAST; the last bounce without a continuation and without its path-state stores):
nothing of it may change a bit of an image.

The reference is the library of the commit before these builds existed: one k_shade for every bounce.  tests/golden/shade_positions_parent.json holds what THAT library rendered for every case below -- the SHA-256 of the image, the diffuse and the
specular accumulator, recorded with `python tests/test_gpu_shade_positions.py record <file>` under SKH_LIB=<the parent's library> on an MI355X -- and a case
passes when the three digests of this tree's render equal the recorded ones: array_equal through a digest.  (Byte equality, so -0.0 != 0.0 and every NaN
payload counts: stricter than array_equal, never weaker.)

The cases: the Cornell box at 64 x 64, 4 sub-frames in one pass, max_depth 1 (bounce 0 alone: the FIRST build ends the paths), 2 (FIRST + LAST), 3, 4, and 6
(the roulette at depth > 3 runs in a MIDDLE build and is gone from the LAST one); a 64 x 64 view of the kitchen stand-in at depth 4 (glass and metal: `inside`
and `specularBounce` carried across bounces); one small scene for each of the ENV, EMIT, MTEX, LSHAPE and HAIR builds at depth 2 and 4; one sample per call
through render_subframe (the path that reads the event word where k_shade left it); and debug 1."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from strelka_amd import scene as S  # noqa: E402
from strelka_amd import scenes  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "shade_positions_parent.json")
W = H = 64
SPP = 4


def _cornell():
    return scenes.cornell_box(), None


def _kitchen():
    return scenes.kitchen_standin(seed=3, n_meshes=12, n_instances=200, tri_lo=50, tri_hi=2000), None


def _env():
    from tests import envref
    from tests.test_gpu_env import QUARTER

    sc = scenes.cornell_box()
    sc.setEnvironment(envref.sky_map(64, 32, seed=8), (0.5, 0.5, 0.5), QUARTER)
    return sc, None


def _emit():
    sc = scenes.cornell_box()

    def after(ctx, arr):
        em = np.zeros((len(arr["materials"]), 3), np.float32)
        em[0] = (2.0, 2.0, 2.0)
        ctx.set_emission(em)
        assert ctx.emitter_info()["triangles"] > 0

    return sc, after


def _mtex():
    from tests.test_gpu_mtex import two_quads

    tex = np.random.RandomState(9).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    uv = (0.0, 2.0, 0.0, 1.0)
    mapped = [dict(type=S.MAT_PBR, base_color=(0.8, 0.5, 0.3), metallic=0.5, roughness=0.5, roughness_texture=1, roughness_channel=1, roughness_scale=0.8,
                   roughness_bias=0.1)]
    sc, arr = two_quads(0, 0, [tex], uv, uv, materials=mapped, distant=True)
    return (sc, arr), None


def _lshape():
    return scenes.spot_room(), None


def _hair():
    return scenes.hair_standin(seed=5, n_strands=400, n_cp=8), None


SCENES = {"cornell": _cornell, "kitchen": _kitchen, "env": _env, "emit": _emit, "mtex": _mtex, "lshape": _lshape, "hair": _hair}

# name -> (scene, max_depth, how).  how: "pass" = the 4 sub-frames in one pass (render_subframes, subframe_batch 4); "single" = one sample per call through
# render_subframe; "debug" = debug 1, one call, whose output image stands in the image's place
CASES = {"cornell_d%d" % d: ("cornell", d, "pass") for d in (1, 2, 3, 4, 6)}
CASES["kitchen_d4"] = ("kitchen", 4, "pass")
for _s in ("env", "emit", "mtex", "lshape", "hair"):
    for _d in (2, 4):
        CASES["%s_d%d" % (_s, _d)] = (_s, _d, "pass")
CASES["cornell_single_d4"] = ("cornell", 4, "single")
CASES["kitchen_single_d3"] = ("kitchen", 3, "single")
CASES["cornell_debug"] = ("cornell", 4, "debug")


def render_case(name):
    """-> (image, diffuse, specular), float32 (H, W, 4) each, from a context of its own"""
    from strelka_amd import capi

    which, depth, how = CASES[name]
    made, after = SCENES[which]()
    sc, arr = made if isinstance(made, tuple) else (made, made.arrays())
    ctx = capi.Context(0)
    try:
        ctx.set_scene(arr)
        if after:
            after(ctx, arr)
        ctx.resize(W, H)
        kw = dict(spp_total=SPP, max_depth=depth, debug=1 if how == "debug" else 0)
        if how == "debug":
            # (a debug view goes to the call's output image, not to the accumulator)
            import torch

            img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            ctx.render_subframe(S.frame_params(sc.getCamera(), W, H, subframe_index=0, **kw), img.data_ptr())
            return img.cpu().numpy(), ctx.read_aov(0).copy(), ctx.read_aov(1).copy()
        if how == "single":
            for i in range(SPP):
                ctx.render_subframe(S.frame_params(sc.getCamera(), W, H, subframe_index=i, **kw))
        else:
            ctx.set_option("subframe_batch", SPP)
            ctx.render_subframes(S.frame_params(sc.getCamera(), W, H, subframe_index=0, **kw), SPP)
        return ctx.read_accum().copy(), ctx.read_aov(0).copy(), ctx.read_aov(1).copy()
    finally:
        ctx.close()


def digests(planes):
    return [hashlib.sha256(np.ascontiguousarray(p, np.float32).tobytes()).hexdigest() for p in planes]


@pytest.fixture(scope="module")
def golden():
    from strelka_amd import build

    build.build()
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_image_and_accumulators_equal_the_parent_librarys(golden, name):
    planes = render_case(name)
    image = planes[0][..., :3]
    assert np.isfinite(image).all() and image.max() > 0  # (a black image would equal a black image)
    got = digests(planes)
    print(name, "image / diffuse / specular", got, "recorded", golden[name])
    assert got == golden[name]


if __name__ == "__main__":
    # python tests/test_gpu_shade_positions.py record <out.json>: the digests of whatever library SKH_LIB names (none: this tree's)
    assert len(sys.argv) == 3 and sys.argv[1] == "record", __doc__
    out = {}
    for case in CASES:
        p = render_case(case)
        assert np.isfinite(p[0][..., :3]).all() and p[0][..., :3].max() > 0, case
        out[case] = digests(p)
        print(case, out[case][0][:16], flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
