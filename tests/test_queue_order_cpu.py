"""The first queue's order on the host (strelka_amd/csrc/skh_order.h; DESIGN.md section 3 "Queue order"): tests/cpp/queue_order_main.cpp includes nothing but that
header, builds both orders' tables for a tile list and holds them to their properties --

  * (block or chunk, sub-frame, rank) -> queue position is a bijection onto [0, total): k_raygen writes every position once and none outside;
  * every (cell, sub-frame) run is contiguous and a cell's sub-frames are adjacent;
  * the cells with a valid slot are numbered along a Morton curve over their first pixel, and run g of the eight holds curve positions g, g + 8, ... back to back;
  * no shard -- positions [g * per, (g + 1) * per), the cut k_raygen makes whatever the order -- outgrows a queue region; the order's own runs differ from the
    shards by the difference between cells only (and are the shards where all cells are alike and their number is a multiple of eight);
  * queue_order 0 is blockBase / validPerSub exactly.

A list of fewer than eight cells has runs longer than an eighth of the queue: the region bound is the shards', which is what a region holds."""
import os
import re
import subprocess

import pytest

from strelka_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "strelka_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queue_order") / "queue_order_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "cpp", "queue_order_main.cpp")])
    return out


def grid_tiles(n, across=8, tile=32):
    """n tiles of a grid `across` wide, in an order that is NOT the curve's (odd columns first)"""
    cells = [(i % across, i // across) for i in range(n)]
    cells.sort(key=lambda c: (1 - c[0] % 2, c[1], c[0]))
    return ";".join("%d,%d" % (x * tile, y * tile) for x, y in cells)


# name: (W, H, T, tiles, frozen)
LISTS = {
    "1_tile": (256, 256, 32, grid_tiles(1), 0),
    "7_tiles": (256, 256, 32, grid_tiles(7), 0),
    "8_tiles": (256, 256, 32, grid_tiles(8), 0),
    "9_tiles": (256, 256, 32, grid_tiles(9), 0),
    "61_tiles": (256, 256, 32, grid_tiles(61), 0),
    "200x120": (200, 120, 32, "all", 0),  # partial tiles on two sides
    # a subset of the 200 x 120 image's tiles, off the grid, one listed twice, one whose lower half lies below the image (a block without a valid slot)
    "200x120_custom": (200, 120, 32, "160,64;0,0;192,104;32,32;0,0;96,96;192,0", 0),
    "200x120_frozen": (200, 120, 32, "all", 3),
    "61_tiles_frozen": (256, 256, 32, grid_tiles(61), 2),
    "tile_8": (100, 60, 8, "all", 0),  # a block spans eight tiles, the last block is short of 512 slots
    "tile_64": (200, 120, 64, "all", 5),
}
BATCHES = (1, 2, 5, 8, 64)
CELLS = (-1, 1, 2)


def run(exe, name, batch, cell):
    W, H, T, tiles, frozen = LISTS[name]
    out = subprocess.run([exe, str(W), str(H), str(T), str(batch), str(cell), tiles, str(frozen)], capture_output=True, timeout=120)
    text = out.stdout.decode().strip()
    assert out.returncode == 0 and text.startswith("OK "), (name, batch, cell, text, out.stderr.decode())
    return {k: v for k, v in re.findall(r"(\w+)=(\S+)", text)}


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_both_orders_hold_their_properties(exe, name, cell):
    for batch in BATCHES:
        got = run(exe, name, batch, cell)
        assert int(got["total"]) % batch == 0


def test_the_cases_are_the_ones_they_claim_to_be(exe):
    """partial blocks, a block with no valid slot, and a list whose runs are the shards are all among the cases"""
    a = run(exe, "200x120", 5, 1)
    assert int(a["partial"]) > 0 and int(a["total"]) == 200 * 120 * 5
    b = run(exe, "200x120_custom", 5, 1)
    assert int(b["partial"]) > 0 and int(b["empty"]) >= 1
    c = run(exe, "8_tiles", 8, 2)
    assert c["uniform"] == "1" and len(set(c["runs"].split(","))) == 1
    d = run(exe, "200x120_frozen", 8, 1)
    assert int(d["total"]) < 200 * 120 * 8 and int(d["empty"]) > 0


def test_the_header_has_no_hip_in_it_and_is_a_dependency_of_the_build():
    text = open(os.path.join(CSRC, "skh_order.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstdint", "vector"]
    assert "skh_order.h" in [os.path.basename(d) for d in build.DEPS]
