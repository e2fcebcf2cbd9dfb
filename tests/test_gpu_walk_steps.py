"""The two steps of the shared BVH walk as the device runs them (leaf_eval<3> and quad_lb<3> of icp-variants_amd/csrc/dev_bvh.hpp, through
the debug entry point icp_debug_walk_steps) against their NumPy float32 restatements (tests/walk_restatement.py), bitwise.  The leaf
update is compared with the SEQUENTIAL scan -- the definition -- and the flag "this leaf took the scan" with the restatement's tie
predicate, so the closed form is what ran wherever there was no tie."""
import ctypes as C
import numpy as np
import pytest
import walk_restatement as wr
from support import raw_bits as bits

pytestmark = pytest.mark.gpu
N = 4096


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def call(c, leaves=None, nodes=None):
    """leaves: a dict of wr.leaf_cases; nodes: (LO, HI, P) -> (state out or None, flags, bounds or None, empty box (lo, hi))."""
    fn = c.lib.icp_debug_walk_steps
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p] * 4
    nl = len(leaves["leaf"]) if leaves else 0
    nn = len(nodes[0]) if nodes else 0
    rec = np.zeros((nl, 32), np.uint32)                  # BvhLeafT<3>: c[3][8], idx[8]
    lq = sf = of = np.zeros((nl, 3), np.float32); si = np.zeros((nl, 3), np.int32); no = np.zeros(nl, np.int32); oi = np.zeros((nl, 4), np.int32)
    if nl:
        rec[:, :24] = leaves["C"].reshape(nl, 24).view(np.uint32); rec[:, 24:] = leaves["IDX"].view(np.uint32)
        lq = np.ascontiguousarray(leaves["P"]); no = np.ascontiguousarray(leaves["leaf"])
        sf = np.stack([leaves["best"], leaves["b2"], leaves["b3"]], axis=1).astype(np.float32)
        si = np.stack([leaves["bi"], leaves["bpos"], leaves["l2"]], axis=1).astype(np.int32)
        of = np.zeros((nl, 3), np.float32)
    nrec = np.zeros((nn, 32), np.float32)                # BvhQuadT<3>: lo[3][4], hi[3][4], pad[8]
    nq = np.zeros((nn, 3), np.float32); bounds = np.zeros((nn, 4), np.float32)
    if nn:
        nrec[:, :12] = nodes[0].reshape(nn, 12); nrec[:, 12:24] = nodes[1].reshape(nn, 12); nq = np.ascontiguousarray(nodes[2])
    empty = np.zeros(2, np.float32)
    rc = fn(c.h, nl, ptr(rec), ptr(lq), ptr(no), ptr(sf), ptr(si), ptr(of), ptr(oi), nn, ptr(nrec), ptr(nq), ptr(bounds), ptr(empty))
    assert rc == 0, rc
    out = (of[:, 0].copy(), oi[:, 0].copy(), oi[:, 1].copy(), of[:, 1].copy(), oi[:, 2].copy(), of[:, 2].copy()) if nl else None
    return out, oi[:, 3].copy(), bounds if nn else None, (float(empty[0]), float(empty[1]))


@pytest.mark.parametrize("category", wr.CATEGORIES)
def test_device_leaf_update_equals_the_sequential_scan_bitwise(gpu_ctx_factory, category):
    c = gpu_ctx_factory()
    case = wr.leaf_cases(category, N, seed=2)
    seq = wr.leaf_update_sequential(**case)
    rare = wr.leaf_update_closed(**case)[6]
    out, flags, _, _ = call(c, leaves=case)
    for name, a, b in zip(("best", "bi", "bpos", "b2", "l2", "b3"), seq, out):
        assert np.array_equal(bits(a), bits(b)), (category, name, int((bits(a) != bits(b)).sum()))
    dd = wr.leaf_distances(case["C"], case["P"])
    heavy = np.minimum(dd.min(axis=1), wr.FLT_MAX) <= case["best"]
    assert np.array_equal((flags & 1) != 0, heavy)
    assert np.array_equal((flags & 2) != 0, rare), (category, int(((flags & 2) != 0).sum()), int(rare.sum()))
    if category == "continuous":
        assert not (flags & 2).any() and heavy.any()       # no tie, no scan: the closed form did every update


def test_device_node_bounds_equal_the_formula_bitwise(gpu_ctx_factory):
    c = gpu_ctx_factory()
    _, _, _, (elo, ehi) = call(c)
    LO, HI, P = wr.node_cases(N, elo, ehi, seed=3)
    want = wr.quad_bounds(LO, HI, P)
    _, _, got, _ = call(c, nodes=(LO, HI, P))
    assert np.array_equal(bits(want), bits(got)), int((bits(want) != bits(got)).sum())
    empty = (LO[:, 0, :] == np.float32(elo)) & (HI[:, 0, :] == np.float32(ehi)) & np.isinf(LO[:, 0, :])
    assert empty.sum() > 100 and np.isposinf(got[empty]).all()          # an empty child is never entered
    assert (got == 0).sum() > 100 and not np.signbit(got).any()         # queries inside a box: +0
    assert np.isinf(want[~empty]).any()                                 # squares that overflow


def test_builder_marks_empty_children_the_same_way(gpu_ctx_factory):
    """A tree whose last 4-wide node has empty children (9 leaves: 16 slots under two levels) finds the exact neighbours: queries far
    outside the cloud, whose walks test every box of the top node."""
    rng = np.random.default_rng(4)
    tp = rng.uniform(-1, 1, (70, 3)).astype(np.float32); tn = np.tile(np.float32([0, 0, 1]), (70, 1))
    sp = (rng.uniform(-1, 1, (200, 3)) * 3).astype(np.float32); sn = np.tile(np.float32([0, 0, 1]), (200, 1))
    c = gpu_ctx_factory()
    c.params.knn_backend = 1; c.params.metric = 1; c.params.max_distance = 100.0; c.push_params()
    c.set_target(tp, tn); c.set_source(sp, sn)
    m, d2 = c.match(np.eye(4))
    d = ((sp[:, None, :] - tp[None, :, :]) ** 2).astype(np.float32)
    ref = ((d[:, :, 0] + d[:, :, 1]).astype(np.float32) + d[:, :, 2]).astype(np.float32)
    assert np.array_equal(m["idx"], ref.argmin(axis=1)) and np.array_equal(d2.view(np.uint32), ref.min(axis=1).view(np.uint32))
