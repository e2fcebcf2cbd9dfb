"""k_gicp_normals<K> and k_color_gradients<K> on the crafted clouds of tests/neighbourhood_cases.py against the fp64 restatements, on
EVERY point: exact distance ties decided by the lowest index, sizes around K, the block and the tree levels, repeats, lines, non-finite
holes, bad normals, scale extremes and neighbourhoods placed at the determinant threshold.  Each kernel carries its own copy of the
K-nearest tree walk; this file is to them what tests/test_gpu_normals.py is to k_normals_knn.

Per case and K in {5, 10, 20}: the GICP normals of the target through both knn_backend values (its own tree / a scratch tree) and of the
source, the colour gradients through both backends.  The rules are support.check_gicp_normals and support.check_color_gradients
(crafted form: no point left out).  The paths must agree bit for bit: the neighbour list is ordered by (d2, index), so the fp64 sums do
not depend on the tree that found it.  Two clouds then go through icp_correspond with metric GICP and metric colored, so that the crafted
normals and gradients reach k_post_gicp / k_post_colored by original index."""
import json
import numpy as np
import pytest

import colored_restatement as CR
import gicp_restatement as G
import neighbourhood_cases as NC
import support as S

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = S.GICP_EPS
LAM = 0.968


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


@pytest.mark.parametrize("k", NC.KS)
@pytest.mark.parametrize("name", NC.NAMES)
def test_case_every_point(ctx, name, k):
    pts, nrm, rgba = NC.CASES[name]
    ref = NC.reference(name, k)
    gref, cref = (ref["nrm"], ref["ev"], ref["cov"]), (ref["grad"], ref["margin"], ref["solved"])
    ctx.set_gicp_options(EPS, k)
    ctx.set_colored_options(LAM, k)
    normals, grads = [], []
    for knn_backend in (1, 0):                                # the target's own tree / a scratch tree
        S.configure(ctx, metric=3, knn_backend=knn_backend)
        ctx.set_target(pts, nrm, rgba)
        normals.append(ctx.gicp_normals("target"))
        grads.append(ctx.color_gradients())
    ctx.set_source(pts, nrm, rgba)
    normals.append(ctx.gicp_normals("source"))
    sn = sg = None
    for what, dev in zip(("target, own tree", "target, scratch tree", "source"), normals):
        sn = S.check_gicp_normals(dev, pts, k, "%s %s" % (name, what), gref)
    for what, dev in zip(("own tree", "scratch tree"), grads):
        sg = S.check_color_gradients(dev, pts, nrm, rgba, k, "%s %s" % (name, what), cref, crafted=True)
    # across paths, bit for bit (NaN payloads included)
    assert np.array_equal(S.u32(normals[0]), S.u32(normals[1])), "%s k=%d: GICP normals differ between the backends" % (name, k)
    assert np.array_equal(S.u32(normals[0]), S.u32(normals[2])), "%s k=%d: GICP normals differ between target and source" % (name, k)
    assert np.array_equal(S.u32(grads[0]), S.u32(grads[1])), "%s k=%d: colour gradients differ between the backends" % (name, k)
    if name == "one colour":                                  # every gradient is zero, either sign of zero
        assert (grads[0] == 0).all()
    if name == "linear intensity":                            # the closed form, to fp32 rounding and the solve's error
        assert np.abs(grads[0] - NC.linear_gradient(nrm)).max() <= 1e-5
    if name == "mixed scales":                                # the contract as written: no gradient on a neighbourhood 1e-4 across
        assert (grads[0][NC.MARKS["tight"]] == 0).all() and (grads[0][~NC.MARKS["tight"]] != 0).any(1).all()
    print("NBHD " + json.dumps(dict(case=name, family=NC.FAMILY[name], k=k, n=len(pts), fin=sn["fin"], gapped=sn["gapped"], ungapped=sn["ungapped"],
                                    worst_cov=sn["worst_cov"], worst_rayleigh=sn["worst_rayleigh"], worst_len=sn["worst_len"],
                                    band=sg["band"], near=sg["near"], worst_grad=sg["worst"], worst_band=sg["worst_band"])))


@pytest.mark.parametrize("name", ["block shuffled", "holes"])
def test_through_the_metrics(gpu_ctx_factory, name):
    """icp_correspond with source = target = the crafted cloud, at the identity and a small motion: the sums of metric GICP (k = 5) and of
    metric colored (k = 5) against the restatements on the device's own records, at the tolerances of the teacher-forced tests."""
    from icp_amd import synth
    pts, nrm, rgba = NC.CASES[name]
    c = gpu_ctx_factory()
    poses = (np.eye(4, dtype=f32), synth.make_pose((0.001, -0.002, 0.0015), (0.004, -0.003, 0.002)).astype(f32))
    S.configure(c, metric=3, max_distance=1.0)
    c.set_gicp_options(EPS, 5)
    c.set_target(pts, nrm, rgba); c.set_source(pts, nrm, rgba)
    tg, sg = c.gicp_normals("target"), c.gicp_normals("source")
    S.check_gicp_normals(tg, pts, 5, name, (lambda r: (r["nrm"], r["ev"], r["cov"]))(NC.reference(name, 5)))
    for pose in poses:
        recs, sums, nv = c.correspond(pose)
        p = c.transform_points(pts, pose)
        idx = recs["idx"]; j = np.maximum(idx, 0)
        valid = (idx >= 0) & np.isfinite(p).all(1) & np.isfinite(pts[j]).all(1)
        s_ref, sa = G.sums(p, pts[j], tg[j], c.transform_normals(sg, pose), recs["weight"], EPS, valid)
        assert nv == int(s_ref[0]) and sums[0] == s_ref[0] and nv > 0.5 * np.isfinite(pts).all(1).sum()
        err = np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)
        assert err.max() <= 1e-9, ("gicp", name, int(np.argmax(err)) + 1, sums[1:34], s_ref[1:34])
    S.configure(c, metric=4, max_distance=1.0)
    c.set_colored_options(LAM, 5)
    grad = c.color_gradients()
    r = NC.reference(name, 5)
    S.check_color_gradients(grad, pts, nrm, rgba, 5, name, (r["grad"], r["margin"], r["solved"]), crafted=True)
    for pose in poses:
        recs, sums, nv = c.correspond(pose)
        s_ref, sa = CR.record_sums(recs, pose, pts, pts, nrm, grad, rgba, rgba, LAM)
        assert nv == int(s_ref[0]) and sums[0] == s_ref[0] and nv > 0.5 * np.isfinite(pts).all(1).sum()
        err = np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)
        assert err.max() <= 1e-9, ("colored", name, int(np.argmax(err)) + 1, sums[1:34], s_ref[1:34])
