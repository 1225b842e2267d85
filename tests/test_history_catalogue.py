"""The catalogue of tests/history_cases.py reaches every entry point include/pgicp.h and include/pgicp_density.h declare, or names it in an exclusion list
with a reason.  The exclusion list holds administrative entry points only -- nothing that computes on a cloud.  (No GPU needed:
the header is parsed the way tests/test_abi.py parses it; tests/test_gpu_history.py runs the cases.)"""
import re

import history_cases as hc


def test_every_declared_entry_point_is_reached_or_excluded_with_a_reason():
    declared = set(hc.declared())
    reached, excluded = set(hc.reached()), set(hc.EXCLUDED)
    assert not declared - reached - excluded, sorted(declared - reached - excluded)
    assert not (reached | excluded) - declared, sorted((reached | excluded) - declared)           # no stale names
    assert not reached & excluded, sorted(reached & excluded)
    assert all(isinstance(r, str) and r for r in hc.EXCLUDED.values())


def test_nothing_that_computes_on_a_cloud_is_excluded():
    compute = re.compile(r"align|icp_pair|match|outlier|error_stats|partial_chain|transform|build_local_map|normal|voxel|densit|filter|upload|"
                         r"map_create|map_set_values|map_transfer|map_destroy|map_size|var_trim|set_params|reading_order|last_matches")
    assert not [n for n in hc.EXCLUDED if compute.search(n)]


def test_the_catalogue_covers_both_sides_of_the_selection_limits():
    small_n, band_p = hc.library_limits()
    assert any(p < band_p for p in hc.BATCH_P) and any(p >= band_p for p in hc.BATCH_P)
    assert len(hc.s2m().scans_xyz[0]) <= small_n < hc.BIG_N
    for P in hc.BATCH_P:
        for sfx in ("_f32", "_f64"):
            assert f"align_batch_{P}{sfx}" in hc.CASES and f"partial_chain_batch_{P}{sfx}" in hc.CASES
        assert f"align_batch_{P}big_f32" in hc.CASES
    assert len(hc.ERROR_CASES) >= 3
