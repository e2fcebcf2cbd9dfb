"""Dev tool (times build): how often does the cross-wave hand-over repair the winner's position of a query that has no candidate at all
(every squared distance overflows; dev_bvh.hpp, the XW fold repair with bi < 0 -- g_dev_counts[13])?  The clouds of
tests/test_gpu_seeded.py::test_seeded_search_queries_without_candidate_vs_oracle (both variants), the longest chain that test runs, in
both forms of the loop.  A zero count means the test does not reach the line it guards.
usage: ICP_HIP_LIB=.../libicp_hip_times.so python tools/dev_no_candidate_counts.py"""
import sys, os, ctypes as C
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from icp_amd import binding
from test_gpu_seeded import no_candidate_cloud
def counters(c, reset=1):
    buf = np.zeros(16, np.uint32)
    assert c.lib.icp_debug_dev_counters(c.h, buf.ctypes.data_as(C.c_void_p), C.c_int32(reset)) == 0
    return buf.astype(np.int64)
for huge_targets in (False, True):
    tgt, tn, src, sn, is_huge, poses = no_candidate_cloud(0, huge_targets)
    for form in ("merged", "separate"):
        os.environ["ICP_HIP_MERGE"] = "0" if form == "separate" else "1"
        c = binding.Context(0)
        c.params.max_distance = 100.0; c.params.metric = 1; c.params.rejection = 0; c.params.knn_backend = 1; c.push_params()
        c.set_target(tgt, tn); c.set_source(src, sn)
        counters(c)
        m, _ = c.match_seeded(poses)
        k = counters(c)
        print("huge targets %d, %-8s: %d queries (%d without candidate), chain of %d launches: fold repairs with no candidate %d, "
              "lone searches %d / %d" % (huge_targets, form, len(src), int(is_huge.sum()), len(poses), k[13], k[11], k[12]))
        c.close()
