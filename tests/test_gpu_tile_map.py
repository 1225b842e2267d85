"""The fast matcher's tile map (pgslam_amd/csrc/tile_map.hpp, PGICP_TILE_GROUP) moves no arithmetic: a tile holds the same 64
queries whichever block runs it, so every group size must leave every byte of every result where the contiguous spans
(PGICP_TILE_GROUP=0, the map before the groups) leave it -- and those must equal the oracle bit for bit, as
tests/test_gpu_bit_exact.py compares.

The knob is read once, so every setting is one process (tests/tile_map_worker.py): a ragged batch of nine problems of
1 ... 8191 points and one single-problem call, float and double, point-to-plane.  With max_n = 8191 there are 128 tiles, 16 per
XCD: 1 and 4 divide them, 3 leaves a tail of one tile per XCD, 16 and 32 fall back to the spans; with PGICP_FAST_LANES=16 there
are 512 tiles.  No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tile_map_worker as worker

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = {"PGICP_TILE_GROUP": "0"}
SETTINGS = [{"PGICP_TILE_GROUP": g} for g in ("1", "3", "4", "16", "32")] + [{"PGICP_TILE_GROUP": "3", "PGICP_FAST_LANES": "16"}]

_runs = {}


def run_setting(setting, tmp_path_factory):
    key = tuple(sorted(setting.items()))
    if key not in _runs:
        out = str(tmp_path_factory.mktemp("tile_map") / "out.npz")
        env = {k: v for k, v in os.environ.items() if k not in ("PGICP_TILE_GROUP", "PGICP_FAST_LANES")}
        env.update(setting)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tile_map_worker.py"), out], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        with np.load(out) as z:
            _runs[key] = {k: z[k] for k in z.files}
    return _runs[key]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_spans_equal_the_oracle_bit_for_bit(tmp_path_factory, oracle32, oracle64):
    got = run_setting(BASE, tmp_path_factory)
    map_xyz, map_nrm, readings, T_inits = worker.scene()
    rd1, T1 = worker.single(readings, T_inits)
    for dtype, orc in ((np.float32, oracle32), (np.float64, oracle64)):
        name = np.dtype(dtype).name
        ref, nrm = map_xyz.astype(dtype), map_nrm.astype(dtype)
        for tag, rds, T0s in (("batch", readings, T_inits), ("single", [rd1], [T1])):
            pre = f"{name}__{tag}__"
            for p, (rd, T0) in enumerate(zip(rds, T0s)):
                what = (name, tag, p)
                order = got[pre + f"order__{p}"]
                assert sorted(order.tolist()) == list(range(len(rd))), what
                o = orc.icp(rd.astype(dtype), ref, nrm, T0, pair_order=order, **worker.CHAIN)
                st = {k: got[pre + "stats__" + k][p] for k in ("status", "iterations", "converged", "overlap", "residual", "trim_limit", "n_kept", "cov")}
                assert st["status"] == o["status"], what
                if o["status"] != 0:
                    continue
                assert st["iterations"] == o["iterations"] and bool(st["converged"]) == o["converged"], what
                assert same_bits(got[pre + "T"][p], o["T"]), (what, np.abs(got[pre + "T"][p] - o["T"]).max())
                assert same_bits(st["cov"].reshape(6, 6), o["cov"]), (what, "cov")
                assert same_bits(st["residual"], o["residual"]) and same_bits(st["overlap"], o["overlap"]), what
                assert st["n_kept"] == o["n_kept"] and same_bits(st["trim_limit"], o["trim_limit"]), what
    # the scene does what it is for: the large problems align, and their last pass matched most of their points
    assert got["float32__batch__stats__status"][-1] == 0 and got["float64__single__stats__status"][0] == 0
    assert (got[f"float32__batch__ids__{len(readings) - 1}"] >= 0).mean() > 0.5


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k[6:]}={v}" for k, v in s.items()))
def test_every_group_size_leaves_every_byte_in_place(setting, tmp_path_factory):
    want = run_setting(BASE, tmp_path_factory)
    got = run_setting(setting, tmp_path_factory)
    assert sorted(got) == sorted(want)
    assert any(k.endswith("__ids__8") for k in want) and any(k.endswith("__counters") for k in want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (setting, k)
