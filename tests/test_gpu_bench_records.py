"""The candidate records a plain bench.py run scores: built on the device (bench.paired_candidates_device) or packed and uploaded, they are
bit for bit what EdgeScorer.pack_cands makes of the host's records of the same workload — the records every --full run and test scores.
Config 3 itself: tests/test_gpu_c3.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("workload,rank", [("c2", 0), ("c2", 1), ("c2q35r", 0), ("c4", 0)])
def test_device_records_are_the_host_records_packed(workload, rank):
    import bench
    import haploconduct_amd as hc

    _, cand, cfg, _ = bench.build_workload(workload, rank)
    _, d_cand, d_cfg, _ = bench.build_workload(workload, rank, on_device=True)
    assert d_cand.is_cuda and tuple(d_cand.shape) == (cand.size, 4) and d_cfg == cfg
    assert d_cand.cpu().numpy().tobytes() == hc.EdgeScorer.pack_cands(cand).tobytes()
