"""The one place where the dependency matrix of derived state is asserted (strelka_amd/csrc/skh_stale.h): which change of an input
invalidates which derived state of a context, and the value the flag takes.  tests/cpp/stale_table.cpp includes nothing but that header, runs its apply() over
every row and prints what it did; the matrix below is typed out by hand from the setters as they were before the table existed."""
import os
import re
import subprocess

from strelka_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "strelka_amd", "csrc")

# "ready" flags fall (=0), "edited" / "stale" flags rise (=1)
MATRIX = """\
set_geometry: accel_built=0 verts_edited=1 emit_stale=1
set_curves: accel_built=0 curve_points_edited=1
set_instances: accel_built=0 emit_stale=1 cut_stale=1
set_lights: lshape_stale=1
set_textures: cut_stale=1
set_materials: emit_stale=1 cut_stale=1
set_emission: emit_stale=1 cut_stale=1
set_material_textures:
set_material_cutouts: cut_stale=1
set_material_blend: cut_stale=1
set_light_shapes: lshape_stale=1
rebuild_option: accel_built=0 refit_ready=0
update_accel_instances: emit_stale=1 cut_stale=1
failed_update: accel_built=0 refit_ready=0 update_ready=0
"""


def test_the_table_is_the_matrix(tmp_path):
    exe = str(tmp_path / "stale_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror=switch", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "stale_table.cpp")])
    out = subprocess.run([exe], capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode() == MATRIX


def test_the_header_has_no_hip_in_it_and_is_a_dependency_of_the_build():
    text = open(os.path.join(CSRC, "skh_stale.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["cstdint"]
    assert "skh_stale.h" in [os.path.basename(d) for d in build.DEPS]


def test_no_setter_sets_the_flags_by_hand():
    """Outside the builders and *_ensure functions, which CLEAR what they have just derived, no host file raises a stale / edited flag or drops a ready flag."""
    pat = re.compile(r"\b(stale|vertsEdited|curvePointsEdited) = true|\b(built|refitReady) = false")
    for fn in ("strelka_hip.hip", "skh_accel.inc", "skh_probes.inc", "skh_image.inc", "skh_host.h"):
        text = open(os.path.join(CSRC, fn)).read()
        assert [m.group(0) for m in pat.finditer(text) if not text[:m.start()].endswith("bool ")] == [], fn
