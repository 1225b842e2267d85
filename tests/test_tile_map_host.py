"""pgslam_amd/csrc/tile_map.hpp without a device: the map from a block of the fast matcher to the tile it runs
(tests/cpp/tile_map_host.cpp, a stand-alone program; once more under the address and undefined-behaviour sanitizers).

For nb in {1 ... 70, 128, 512, 1568, 1569, 4093} and G in {-1, 0, 1, 2, 3, 4, 16, 32, 196, 1000} the program checks that
  * the map is a bijection onto [0, nb);
  * every class b & 7 (an XCD) receives at most ceil(nb / 8) tiles -- what the queue segments are sized by;
  * tiles ascend with j = b >> 3 inside a class;
  * G <= 0 and G >= nb / 8 give the contiguous spans of kernels.hip's xcd_tile, restated in the program.
One case is then read back and checked by hand on this side."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_map_host.cpp")
N_CASES = 75 * 10


def build_exe(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "pgslam_amd", "csrc"), SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("tile_map") / "tile_map_host"))


def test_every_table_entry(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"tile map ok: {N_CASES} cases" in out.stdout


def test_every_table_entry_under_sanitizers(tmp_path):
    san = build_exe(str(tmp_path / "tile_map_host_san"), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([san], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"tile map ok: {N_CASES} cases" in out.stdout


def dump(exe, nb, G):
    out = subprocess.run([exe, "dump", str(nb), str(G)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return [int(x) for x in out.stdout.split()]


def test_groups_of_three_among_sixteen_tiles_per_class(exe):
    """nb = 128, G = 3: five whole groups (tiles 0 ... 119), then one tile per class"""
    got = dump(exe, 128, 3)
    assert sorted(got) == list(range(128))
    for b, t in enumerate(got):
        x, j = b & 7, b >> 3
        want = ((j // 3) * 8 + x) * 3 + j % 3 if j < 15 else 120 + x
        assert t == want, (b, t, want)
    # class 0 runs tiles 0 1 2, 24 25 26, ...: G consecutive tiles, then a stride of 8 G
    assert [got[8 * j] for j in range(7)] == [0, 1, 2, 24, 25, 26, 48]


def test_whole_groups_cover_everything_when_they_divide(exe):
    """nb = 1568 (a 100 000-point scan at 64 queries a wave), G = 4: 196 tiles per class = 49 whole groups, no remainder"""
    got = dump(exe, 1568, 4)
    assert all(t == ((b >> 3) // 4 * 8 + (b & 7)) * 4 + (b >> 3) % 4 for b, t in enumerate(got))
    assert dump(exe, 1568, 196) == dump(exe, 1568, 0) == [(b & 7) * 196 + (b >> 3) for b in range(1568)]
