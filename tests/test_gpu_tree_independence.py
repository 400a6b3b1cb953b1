"""The device's hit records do not depend on the tree ("Determinism rules"; tests/treeref.py; docs/LOG.md "A hit record that depended on the tree").

Every scene of tests/treeref.py -- flat_room, coplanar_panels, slats, mechanism_scene -- is built under every tree of TREES by the shipped library (the last one the SPLIT build of the world-only kernel), and under two other
libraries that cluster differently (PLOC pairing ties from its first round, SKH_PLOC_PAIRED_FIRST=1; PLOC's cost search stopped after one round, SKH_PLOC_MAX_ROUNDS=1;
each compiled once per module and run in a child process through SKH_LIB).  Of every tree, with no ray left out: the closest-hit records of the scene's rays and of
its any-hit twins are byte-equal to the checker's BRUTE-FORCE loop, the any-hit answers of the twins equal the checker's.  On the rays treeref's float64 reference
decides: the float64 primitive exactly (a miss where it says so) and t, u, v inside its bars; the worst measured fraction of each bar is in every assertion message.

Before the node test culled against the best t by the ray's dominant axis alone, mechanism_scene failed here as the architectural kitchen's record 865 did (docs/LOG.md
has the run): a sliver facet's computed t in front of its own box, a neighbouring facet's t in between, the winner decided by the visit order."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import treeref as R

pytestmark = pytest.mark.gpu

NAMES = sorted(R.SCENES)
REFIT = "refit"
TREES = [{}, {"build_quality": 0}, {"leaf_max_tris": 4}, {"leaf_max_tris": 7, "leaf_lines": 1}, {"reinsert_rounds": 0}, {"reinsert_rounds": 13, "reinsert_min_size": 1},
         {"morton_bits": 5}, {"morton_bits": 18}, {"world_kernel": 0}, {"bake_world": 0, "tlas_build": 0}, {"bake_world": 0, "tlas_build": 1}, {REFIT: 1},
         {"tail_split": 2}]  # (the world-only SPLIT build, which scenes this small do not get by themselves: idle lanes take over stack entries of the last rays)
VARIANT_TREES = [{}, {"leaf_max_tris": 4}, {"bake_world": 0, "tlas_build": 1}]  # what a variant library is asked for: its clustering is the difference


def ids(x):
    return "_".join("%s%s" % kv for kv in x.items()) or "defaults"


@functools.lru_cache(maxsize=None)
def arbiter(name, bake):
    """the checker's brute-force loop over a scene's rays and twins, once per bake mode: closest hits of both sets, any-hit answers of the twins"""
    from tests import orklib

    scene, arr, tri, rays, ref, shadow = R.cached(name)
    o = orklib.new_context()
    o.set_bake(bake)
    o.set_scene(arr)
    return o.trace(rays, 0, brute=True), o.trace(shadow, 0, brute=True), o.trace(shadow, 1, brute=True)


def hold(ctx, name, options, label=""):
    """build the scene in ctx under `options` (already set on it) and ask everything the module docstring lists; -> the worst fractions of the t and u / v bars"""
    scene, arr, tri, rays, ref, shadow = R.cached(name)
    ctx.set_scene(arr)
    if options.get(REFIT):
        ctx.set_geometry(arr)
        ctx.refit_accel()
        assert ctx.build_info()["refit"] == 1
    want, want_twin, want_any = arbiter(name, options.get("bake_world", 4))
    got = ctx.trace(rays, 0)
    wrong, ft, fb = R.check_decided(name, got)
    diff = np.nonzero(got != want)[0]
    what = "%s%s under %s: t at %.3f of its bar, u / v at %.3f of theirs" % (label, name, ids(options), ft, fb)
    print(what)
    assert got.tobytes() == want.tobytes(), "%s; %d of %d closest-hit records differ from the checker's brute force: rays %s (families %s, aimed at instances %s), got %s, brute force %s" % (
        what, len(diff), len(rays), diff[:4], ref["family"][diff[:4]], tri[0][ref["aim"][diff[:8]]], got[diff[:4]], want[diff[:4]])
    assert len(wrong) == 0, "%s; %d decided rays name another primitive than float64 (first %s)" % (what, len(wrong), wrong[:4])
    assert ft <= 1.0 and fb <= 1.0, what
    assert ctx.trace(shadow, 0).tobytes() == want_twin.tobytes(), what + "; the twins' closest hits differ from the checker's brute force"
    got_any = ctx.trace(shadow, 1)
    assert np.array_equal(got_any, want_any), "%s; %d any-hit answers differ from the checker's" % (what, int((got_any != want_any).sum()))
    return ft, fb


@pytest.fixture(scope="module")
def contexts():
    """one context per set of options, reused by every scene built under it"""
    from strelka_amd import build, capi

    build.build()
    made = {}

    def get(options):
        key = ids(options)
        if key not in made:
            made[key] = capi.Context(0)
            for k, v in options.items():
                if k != REFIT:
                    made[key].set_option(k, v)
        return made[key]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("options", TREES, ids=ids)
def test_records_do_not_depend_on_the_tree(contexts, options, name):
    hold(contexts(options), name, options)


CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["SKH_ROOT"])
from strelka_amd import capi
from tests.test_gpu_tree_independence import NAMES, VARIANT_TREES, REFIT, hold
for options in VARIANT_TREES:
    ctx = capi.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    for name in NAMES:
        hold(ctx, name, options, label=os.environ["SKH_LABEL"] + ": ")
    ctx.close()
print("TREE-INDEPENDENT-OK")
'''


@pytest.fixture(scope="module")
def variant_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("variants")


@pytest.mark.parametrize("define", ["SKH_PLOC_PAIRED_FIRST=1", "SKH_PLOC_MAX_ROUNDS=1"])
def test_records_do_not_depend_on_the_clustering(variant_dir, define):
    """the same source with another clustering compiled in (one compile per define), every scene under it in a child process that loads it through SKH_LIB"""
    from strelka_amd import build

    for name in NAMES:
        R.export(name, variant_dir)  # (the child reads the reference this process has computed)
    lib = build.build_variant(str(variant_dir / ("libstrelka_hip_%s.so" % define.split("=")[0].lower())), [define])
    env = dict(os.environ, SKH_LIB=lib, SKH_LABEL=define, TREEREF_CACHE=str(variant_dir), SKH_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and "TREE-INDEPENDENT-OK" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
