"""The escape cull's exactness on oracle-traced rays of random bench tiles (scripts/escape_census.py): no ray
that hits the disc meets the cull test before its event, no accepted step after the test comes back inside R_cull, and the
E/L speed bound holds along every culled ray.  CPU only."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

import escape_census  # noqa: E402


def test_escape_cull_exact_on_oracle_rays_of_bench_tiles():
    c = escape_census.census(tiles=24, seed=7)
    assert c["rays"] == 24 * 64
    assert 0.15 < c["hit_fraction"] < 0.5
    assert c["hits_meeting_test_before_event"] == 0
    assert c["steps_inside_r_cull_after_test"] == 0
    assert c["steps_beyond_speed_bound"] == 0
    # the cull removes about a third of the steps (0.674 on 1000 tiles)
    assert 0.5 < c["wave_steps_ratio"] < 0.8
