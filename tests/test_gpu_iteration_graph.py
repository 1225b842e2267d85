"""An iteration replayed from a captured graph (PGICP_GRAPH_MAX_P) computes what the same iteration launched kernel by kernel
computes, in every configuration of the driver and across buffers that grow: the graph's key covers every address and every
switch its launches were captured with (api_icp.inc: IterBufs, IterPlan).

tests/iteration_graph_worker.py runs, on one context, every configuration at 257 points, at 5 000 and at 257 again; a key that
misses a buffer replays, in the third run, a graph that names the block the buffer had in the first.  One child runs it with
nothing set, one with every iteration captured or replayed; the two leave the same bytes.  No tolerance anywhere."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("PGICP_GRAPH_MAX_P", "PGICP_GRAPH_DEBUG")


def run_child(setting, out):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(setting)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "iteration_graph_worker.py"), out], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_replayed_iterations_leave_the_bytes_of_launched_ones(tmp_path):
    plain_npz, graph_npz = str(tmp_path / "plain.npz"), str(tmp_path / "graph.npz")
    r = run_child({}, plain_npz)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]          # (the second child is not started behind a failed first)
    g = run_child({"PGICP_GRAPH_MAX_P": "4096", "PGICP_GRAPH_DEBUG": "1"}, graph_npz)
    assert g.returncode == 0, g.stdout[-2000:] + g.stderr[-3000:]
    m = re.search(r"(\d+) iteration graphs captured, (\d+) replayed, (\d+) failures", g.stderr)
    assert m, g.stderr[-2000:]
    captured, replayed, failures = (int(x) for x in m.groups())
    print("iteration graphs: captured", captured, "replayed", replayed, "failures", failures)
    assert captured > 8 and replayed > 0 and failures == 0               # (more than eight: the eight-entry cache evicts)
    want, got = load(plain_npz), load(graph_npz)
    assert sorted(got) == sorted(want)
    # the worker did what it is for: every configuration ran at every size, and the large runs aligned
    for name in ("p2plane_f32", "p2plane_f64", "p2point", "var_trim", "robust", "desc_soft", "reading_normals", "radii_trimmed", "radii_var_trim",
                 "radii_robust", "knn3", "knn3_radii", "brute", "align_batch", "align_residual_batch"):
        for tag in ("0_257", "1_5000", "2_257"):
            assert f"{name}__{tag}__T" in want, (name, tag)
        assert (want[f"{name}__1_5000__stats__status"] == 0).all(), name
    assert "partial_chain_batch__2_257__ratio" in want and "match__2_257__ids" in want
    differ = [k for k in sorted(want)
              if not (got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes())]
    assert not differ, differ
