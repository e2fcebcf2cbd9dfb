"""Helpers that are about testing, shared by the test modules (`import support as S`): bit views, the params / cloud plumbing of a
context, and the checks one test module used to import from another.  Data generators live in icp_amd/synth.py, CPU specifications in
the *_restatement.py modules; fixtures stay with the module that uses them."""
import ctypes as C
import os
import numpy as np

f32 = np.float32
LBVH = 1
POSE_TOL = 1e-5        # north_star: 1e-5 rad / 1e-5 m
FORMS = ("merged", "separate")
NRM_TOL = 2e-6
CURV_TOL = 2e-6
GAP_REL = 1e-9


def bits(a):
    """The contiguous fp32 cast of `a`, viewed as uint32."""
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def u32(a):
    """`a` as it is (no cast), contiguous, viewed as uint32."""
    return np.ascontiguousarray(a).view(np.uint32)


def raw_bits(a):
    """A float32 array viewed as uint32; an array of any other type as it is."""
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def pose_of(angles, t):
    from icp_amd import synth
    return synth.make_pose(angles, t).astype(f32)


def rand_pose(seed, ang=0.1, tr=0.2):
    r = np.random.default_rng(seed)
    return pose_of(r.uniform(-ang, ang, 3), r.uniform(-tr, tr, 3))


def configure(ctx, metric=1, weighting=0, rejection=1, color_icp=0, knn_backend=1, n_iterations=10, multires=0, selection=0, proba=1.0,
              max_distance=0.0003, matching=0, seed=7, K=None, width=0, height=0, **kw):
    """Sets these fields of ctx.params, then any other field given by name, then the camera fields where projective matching comes with a
    K (a caller that leaves K out sets them itself), and pushes them."""
    p = ctx.params
    p.metric, p.weighting, p.rejection, p.color_icp, p.knn_backend, p.n_iterations = metric, weighting, rejection, color_icp, knn_backend, n_iterations
    p.multires, p.selection, p.selection_proba, p.selection_seed, p.max_distance, p.matching = multires, selection, proba, seed, max_distance, matching
    for k, v in kw.items():
        setattr(p, k, v)
    if matching == 1 and K is not None:
        p.fx, p.fy, p.cx, p.cy, p.width, p.height = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), width, height
    ctx.push_params()


def load(ctx, d, colors=True):
    ctx.set_target(d["tgt_pts"], d["tgt_nrm"], d.get("tgt_rgba") if colors else None)
    ctx.set_source(d["src_pts"], d["src_nrm"], d.get("src_rgba") if colors else None)


def upload(ctx, vol, color=False):
    """A restatement's volume (tsdf_restatement.Volume, with tsdf_color_restatement's arrays when color) into the context's."""
    ctx.tsdf_create(color=color, dims=(vol.nx, vol.ny, vol.nz), origin=tuple(float(x) for x in vol.o), voxel_size=float(vol.s))
    ctx.tsdf_upload(vol.tsdf, vol.weight)
    if color:
        ctx.tsdf_color_upload(vol.rgb, vol.wc)


def tsdf_blocks_equal_restatement(ctx, hv, what):
    """The context's hashed TSDF volume against an htsdf_restatement.HVolume: coordinates, tsdf and weight bit for bit, nothing unplaced."""
    info, coords, t, w = ctx.tsdf_blocks()
    rc, rt, rw = hv.sorted_blocks()
    assert info["n_blocks"] == len(rc) and info["n_unplaced"] == 0 and info["n_out_of_range"] == hv.n_out_of_range, (what, info, len(rc))
    assert np.array_equal(coords, rc), what
    assert same_bits(t, rt) and same_bits(w, rw), what
    return info


def fuse_cloud(ctx, vol, pts, pose, origin=None):
    """The cloud as the source, fused on the device and by tsdf_cloud_restatement into `vol`; every field of the info equal."""
    import tsdf_cloud_restatement as CR
    ctx.set_source(pts)
    info = ctx.tsdf_integrate_cloud("source", pose=pose, sensor_origin=origin)
    want = CR.integrate(vol, pts, pose, origin)
    print("cloud of %d: %s" % (len(pts), info))
    assert info == want, (info, want)
    return info


def loaded_ctx(factory, tgt, src, **params):
    """A context with `params` set by name and the (points, normals, colours) triples resident; src may be None."""
    c = factory()
    for k, v in params.items():
        setattr(c.params, k, v)
    c.push_params()
    c.set_target(*tgt)
    if src is not None:
        c.set_source(*src)
    return c


def make_ctx(factory, form, **params):
    """A context whose point-to-plane loop takes `form` ("merged" / True, "separate" / False), on the LBVH backend."""
    if form is True:
        form = "merged"
    elif form is False:
        form = "separate"
    env = {"ICP_HIP_MERGE": "0" if form == "separate" else "1"}                                              # read once, at icp_ctx_create
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = factory()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    c.params.knn_backend = LBVH; c.params.metric = 1
    for k, v in params.items():
        setattr(c.params, k, v)
    c.push_params()
    return c


def counters(c):
    a, b = C.c_int32(0), C.c_int32(0)
    assert c.lib.icp_debug_counters(c.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def assert_same_run(ra, rb):
    assert len(ra) == len(rb)
    for k, (a, b) in enumerate(zip(ra, rb)):
        assert a["n_valid"] == b["n_valid"] and a["status"] == b["status"] and a["n_src"] == b["n_src"], k
        assert np.array_equal(a["pose"], b["pose"]), k


def check_stats(dev, ref, label):
    """One iteration's robust stats of the device against the restatement's: counts equal, trim_d2 and sigma bit-equal."""
    assert dev["n_entering"] == ref["n_entering"] and dev["n_kept"] == ref["n_kept"], (label, dev, ref)
    assert u32(f32(dev["trim_d2"])) == u32(f32(ref["trim_d2"])) and u32(f32(dev["sigma"])) == u32(f32(ref["sigma"])), (label, dev, ref)


def restated_step(c, pair, metric, pose, opts=None):
    """The non-linear restatement's Solve on the device's records at `pose` -> (x, summary, decisions, new pose)."""
    import lm_restatement as lm
    recs, _, _ = c.correspond(pose)
    st = c.transform_points(pair["src_pts"], pose)
    nt = c.transform_normals(pair["src_nrm"], pose)
    b = lm.blocks(metric, st, nt, pair["tgt_pts"], pair["tgt_nrm"], recs)
    x, summ, dec = lm.solve_blocks(b, opts)
    newpose = pose if summ["termination"] == lm.NO_RESIDUALS else lm.compose(x, pose)
    return x, summ, dec, newpose


def check_normals(orc, pts, k, vp, nrm, curv, label=""):
    """Asserts the device's (nrm, curv) against orc.estimate_normals on every point; returns the statistics."""
    pts = np.ascontiguousarray(pts, f32); vp = np.asarray(vp, f32)
    on, oc, nb = orc.estimate_normals(pts, k, vp, return_neighbours=True)
    assert nrm.shape == on.shape and curv.shape == oc.shape
    nan_n, nan_c = np.isnan(nrm), np.isnan(curv)
    bad_nan = np.nonzero((nan_n != np.isnan(on)).any(1) | (nan_c != np.isnan(oc)))[0]
    assert len(bad_nan) == 0, "%s: NaN pattern differs at %s: dev %s orc %s" % (label, bad_nan[:5], nrm[bad_nan[:5]], on[bad_nan[:5]])
    fin = np.nonzero(~np.isnan(on).any(1))[0]
    stats = dict(label=label, n=len(pts), n_normals=len(fin), worst_nrm=0.0, worst_curv=0.0, bit_identical=1.0, n_ambiguous=0)
    if len(fin) == 0:
        return stats
    assert np.isfinite(nrm[fin]).all() and np.isfinite(curv[fin]).all()
    # covariance of the oracle's neighbour sets (fp64; eigenvalues by LAPACK, independent of both Jacobis)
    ids = nb[fin]; m = ids >= 0; cnt = m.sum(1)
    X = np.where(m[..., None], pts[np.where(m, ids, 0)].astype(np.float64), 0.0)
    D = (X - (X.sum(1) / cnt[:, None])[:, None, :]) * m[..., None]
    C = np.einsum("nki,nkj->nij", D, D) / cnt[:, None, None]
    w = np.linalg.eigvalsh(C)
    lmax = w[:, 2]
    amb = (lmax > 0) & (w[:, 1] - w[:, 0] <= GAP_REL * lmax)
    nd, no = nrm[fin].astype(np.float64), on[fin].astype(np.float64)
    dn = np.abs(nd - no).max(1)
    dn[amb] = 0.0
    dc = np.abs(curv[fin].astype(np.float64) - oc[fin])
    stats.update(worst_nrm=float(dn.max()), worst_curv=float(dc.max()), n_ambiguous=int(amb.sum()),
                 bit_identical=float((nrm[fin].view(np.uint32) == on[fin].view(np.uint32)).all(1).mean()))

    def where(r, what):
        i = fin[r]
        return "%s: %s at point %d %s (%d-NN %s): dev n %s curv %r, oracle n %s curv %r, eig %s; %.6f of normals bit-identical" % (
            label, what, i, pts[i], k, nb[i].tolist(), nrm[i], float(curv[i]), on[i], float(oc[i]), w[r], stats["bit_identical"])
    r = int(np.argmax(dn))
    assert dn[r] <= NRM_TOL, where(r, "|n_dev - n_orc| = %.3g" % dn[r])
    r = int(np.argmax(dc))
    assert dc[r] <= CURV_TOL, where(r, "|curv_dev - curv_orc| = %.3g" % dc[r])
    if amb.any():
        a = np.nonzero(amb)[0]
        q = np.einsum("ni,nij,nj->n", nd[a], C[a], nd[a])
        over = q - (w[a, 0] + GAP_REL * lmax[a])
        r = int(np.argmax(over))
        assert over[r] <= 0, where(a[r], "n^T C n above the near-null space by %.3g" % over[r])
        ln = np.abs(np.linalg.norm(nd[a], axis=1) - 1)
        r = int(np.argmax(ln))
        assert ln[r] <= 1e-6, where(a[r], "| |n| - 1 | = %.3g" % ln[r])
        e = (vp[None, :] - pts[fin[a]]).astype(np.float64)
        flip = (e * nd[a]).sum(1) + 1e-6 * np.linalg.norm(e, axis=1)
        r = int(np.argmin(flip))
        assert flip[r] >= 0, where(a[r], "normal points away from the viewpoint")
    return stats


GICP_EPS = 1e-3        # the epsilon the GICP tests run with, and the one the sign-free measure plane_cov is taken at
GICP_GAP = 1e-3        # (l1 - l0) / l2 below which a neighbourhood's normal is not unique enough to compare directions
GRAD_NEAR = (0.5, 2.0)                 # det / threshold: within 2x of the threshold either side is right
GRAD_BAND = (1e-2, 1e4)                # det / threshold: the fp64 adjugate's determinant differs from numpy's by up to 2.2e-4 / (det / threshold)
GRAD_SHARE_CAP = 0.02


def check_gicp_normals(dev, pts, k, label, ref=None):
    """Asserts the device's GICP normals against gicp_restatement on EVERY finite point; returns the statistics.
      * the NaN patterns are identical, and | |n| - 1 | <= 1e-6 on every finite point;
      * where the reference neighbourhood has a usable eigen-gap ((l1 - l0) / l2 >= GICP_GAP) or no extent at all:
        |plane_cov(dev) - plane_cov(ref)| <= 1e-5 (sign-free); coincident neighbours give exactly (1, 0, 0);
      * where it has none (collinear or isotropic neighbours, the direction is not unique): the Rayleigh quotient
        n_dev^T C n_dev / |n_dev|^2 <= l0 + 1e-9 lmax with C the fp64 covariance of the restatement's neighbour set.
    ref: (normals, eigenvalues, covariances) of gicp_restatement.normals(pts, k, cov=True) when the caller has them."""
    import gicp_restatement as G
    rn, ev, cov = G.normals(pts, k, cov=True) if ref is None else ref
    assert dev.shape == rn.shape
    assert np.array_equal(np.isnan(dev), np.isnan(rn)), "%s k=%d: NaN pattern" % (label, k)
    fin = np.nonzero(~np.isnan(rn).any(1))[0]
    n_finite = int(np.isfinite(np.asarray(pts, f32)).all(1).sum())
    assert len(fin) == (n_finite if n_finite >= 3 else 0), "%s k=%d: %d normals for %d finite points" % (label, k, len(fin), n_finite)
    st = dict(label=label, k=k, n=len(rn), fin=len(fin), gapped=0, ungapped=0, coincident=0, worst_cov=0.0, worst_rayleigh=0.0, worst_len=0.0)
    if len(fin) == 0:
        return st
    nd = dev[fin].astype(np.float64)
    ln = np.abs(np.linalg.norm(nd, axis=1) - 1)
    st["worst_len"] = float(ln.max())
    assert ln.max() <= 1e-6, "%s k=%d: | |n| - 1 | = %.3g at point %d" % (label, k, ln.max(), fin[int(np.argmax(ln))])
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (ev[fin, 1] - ev[fin, 0]) / ev[fin, 2]
    flat = ~(np.abs(cov[fin]).reshape(len(fin), 9) > 0).any(1)
    gapped = (gap >= GICP_GAP) | (ev[fin, 2] == 0) | flat
    use = fin[gapped]
    if len(use):
        err = np.abs(G.plane_cov(dev[use], GICP_EPS) - G.plane_cov(rn[use], GICP_EPS)).reshape(len(use), 9).max(1)
        r = int(np.argmax(err))
        st["worst_cov"] = float(err[r])
        assert err[r] <= 1e-5, "%s k=%d: point %d dev %s ref %s eig %s" % (label, k, use[r], dev[use[r]], rn[use[r]], ev[use[r]])
    co = fin[flat]
    assert np.array_equal(dev[co], np.tile(f32([1, 0, 0]), (len(co), 1))), "%s k=%d: coincident neighbours" % (label, k)
    rest = fin[~gapped]
    if len(rest):
        n = dev[rest].astype(np.float64)
        n /= np.linalg.norm(n, axis=1, keepdims=True)         # the Rayleigh quotient: an fp32 normal's |n|^2 is off 1 by up to 1.2e-7, more than
        q = np.einsum("ni,nij,nj->n", n, cov[rest], n)        # the 1e-9 allows once l0 is of lmax's size (an isotropic neighbourhood); |n| is checked above
        over = (q - ev[rest, 0]) / ev[rest, 2]
        r = int(np.argmax(over))
        st["worst_rayleigh"] = float(over[r])
        assert over[r] <= 1e-9, "%s k=%d: n^T C n above l0 by %.3g lmax at point %d, dev %s eig %s" % (label, k, over[r], rest[r], dev[rest[r]], ev[rest[r]])
    st.update(gapped=len(use), ungapped=len(rest), coincident=len(co))
    assert st["gapped"] + st["ungapped"] == st["fin"], st                     # every finite point was checked by one rule or the other
    return st


def check_color_gradients(dev, pts, nrm, rgba, k, label, ref=None, crafted=False):
    """Asserts the device's colour gradients against colored_restatement on every point; returns the statistics.
    On a natural cloud (crafted=False): the points with det / threshold inside GRAD_NEAR are left out, at most GRAD_SHARE_CAP of the
    cloud; on all others the NaN and zero patterns are identical and |dev - ref| <= 1e-5 max(1, |ref|).
    On a crafted cloud: no point is left out.  The NaN pattern is identical everywhere; the zero pattern wherever det / threshold is
    outside GRAD_NEAR; |dev - ref| <= 1e-5 max(1, |ref|) wherever det / threshold >= 1e4; a point inside GRAD_BAND is allowed
    1e-5 max(1, 1e4 / (det / threshold)) max(1, |ref|) and, inside GRAD_NEAR, either exactly zero or that far from the gradient solved
    without the threshold; the points inside GRAD_BAND are at most GRAD_SHARE_CAP of the cloud.
    ref: (gradients, det / threshold, gradients solved without the threshold) of colored_restatement.gradients(..., full=True)."""
    import colored_restatement as CR
    rg, margin, solved = CR.gradients(pts, nrm, rgba, k, full=True) if ref is None else ref
    assert dev.shape == rg.shape
    n = len(rg)
    with np.errstate(invalid="ignore"):
        near = (margin > GRAD_NEAR[0]) & (margin < GRAD_NEAR[1])
        band = (margin > GRAD_BAND[0]) & (margin < GRAD_BAND[1])
    far = ~near
    st = dict(label=label, k=k, n=n, near=int(near.sum()), band=int(band.sum()), checked=0, worst=0.0, worst_band=0.0)
    if crafted:
        assert np.array_equal(np.isnan(dev), np.isnan(rg)), "%s k=%d: NaN pattern" % (label, k)
        assert band.sum() <= GRAD_SHARE_CAP * n, "%s k=%d: %d of %d points in the threshold band" % (label, k, band.sum(), n)
    else:
        assert np.array_equal(np.isnan(dev[far]), np.isnan(rg[far])), "%s k=%d: NaN pattern" % (label, k)
        assert near.sum() <= GRAD_SHARE_CAP * n, "%s k=%d: %d of %d points within 2x of the threshold" % (label, k, near.sum(), n)
    live = ~np.isnan(rg).any(1)
    fin = far & live
    # the zero of the threshold is (0, 0, 0).  A crafted cloud can make ONE component of a solved gradient vanish exactly in one arithmetic and
    # not in the other (a lattice whose gradient is perpendicular to an axis), so there the pattern is taken per point; the natural clouds
    # keep the per-component comparison they always had.
    zd, zr = ((dev[fin] == 0).all(1), (rg[fin] == 0).all(1)) if crafted else ((dev[fin] == 0), (rg[fin] == 0))
    assert np.array_equal(zd, zr), "%s k=%d: zero pattern at %s" % (label, k, np.nonzero(fin)[0][(zd != zr).reshape(len(zd), -1).any(1)][:5])
    err = np.abs(dev.astype(np.float64) - rg) / np.maximum(1.0, np.abs(rg.astype(np.float64)))
    tight = fin & ~band if crafted else fin
    st["checked"] = int(tight.sum())
    if tight.any():
        st["worst"] = float(err[tight].max())
        assert st["worst"] <= 1e-5, (label, k, st["worst"], int(np.nonzero(tight)[0][np.argmax(err[tight].max(1))]))
    if crafted and band.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            tol = 1e-5 * np.maximum(1.0, 1e4 / margin)
        b = band & far & live
        if b.any():
            rel = err[b].max(1) / tol[b]
            st["worst_band"] = float(rel.max())
            assert rel.max() <= 1.0, "%s k=%d: band point %d off by %.3g of its tolerance" % (label, k, np.nonzero(b)[0][int(np.argmax(rel))], rel.max())
        for i in np.nonzero(near & live)[0]:
            if (dev[i] == 0).all():
                continue
            e = np.abs(dev[i].astype(np.float64) - solved[i]) / np.maximum(1.0, np.abs(solved[i].astype(np.float64)))
            assert e.max() <= tol[i], "%s k=%d: point %d at det / threshold %.3g is neither zero nor the solved gradient: %s, %s" % (label, k, i, margin[i], dev[i], solved[i])
        st["checked"] += int((band & live).sum())
    return st


def assert_matches_icp_run(c, starts, max_stats=512):
    """Every start of ONE multistart call against icp_run from that start on the same context: records and pose, bit for bit."""
    res, stats, best = c.run_multistart(starts, max_stats=max_stats)
    assert len(res) == len(starts)
    for k, s in enumerate(starts):
        pose, recs, rc = c.run(s, max_stats=max_stats, check=False)
        assert res[k]["status"] == rc, k
        assert np.array_equal(res[k]["pose"], pose), k
        assert len(stats[k]) == len(recs), k
        for i, (a, b) in enumerate(zip(stats[k], recs)):
            assert (a["n_src"], a["n_valid"], a["status"]) == (b["n_src"], b["n_valid"], b["status"]), (k, i)
            assert np.array_equal(a["pose"], b["pose"]), (k, i)
            assert a["rmse"] == -1.0 and a["benchmark_error"] == -1.0
    return res, stats, best


def expected_best(res):
    best = 0
    for k, r in enumerate(res):
        b = res[best]
        if r["n_inliers"] > b["n_inliers"] or (r["n_inliers"] == b["n_inliers"] and r["inlier_rmse"] < b["inlier_rmse"]):
            best = k
    return best
