"""A call on a context that has been used for anything else returns the bits that the same call returns on a fresh context.

The recipes of tests/context_reuse_cases.py -- one per call family, size and layout of the buffers a context shares between its families
(icp-variants_amd/csrc/host_ctx.hpp) -- are run
  * each on a fresh context, against the reference that family already has in the suite, with that reference's bound
    (test_fresh_equals_reference): the rest is then not a comparison of the code with itself;
  * in one hand-written order on one context (test_fixed_sequence), chosen so that on every shared resource a large use is followed by
    a small one, a small by a large and one layout by another (the comments of FIXED_ORDER name the pairs);
  * in three seeded random orders (test_seeded_orders);
  * with one refused call per family between them (test_refused_call_in_between);
and every step must give the fresh context's result bit for bit, with nothing left out but context_reuse_cases.HISTORY_FIELDS.  A context
on the caller's stream (icp_ctx_create_on_stream) is driven from C++ (tests/cpp/caller_stream.cpp) and compared with a default context.

The loop form (merged / separate launches) is fixed when a context is made, so the sequences run once per form.

Measured (MI355X): no step of any order differed from its fresh result on this commit; no defect was found in the host layer.  The one
field that did differ is no function of the call's inputs and moved to HISTORY_FIELDS: n_moved of icp_tsdf_evict_blocks counts the kept
blocks that sat at or above n_keep, and where a block sits in the pool is a race by contract (dev_tsdf_hash_evict.hpp).

Measured (MI355X), a defect of the kind the orders are meant to catch, put into the library by hand for one run and not committed: the
re-zeroing of tc_acc after a cloud fuse skipped (tc_fold_voxel leaves S and N as they are).  test_fixed_sequence fails in both forms at
step 29, "cloud_fuse_evict_insert_fuse" behind "cloud_fuse_hashed_colored", first differing field info_1[n_updated], and the seeded
orders fail at the same recipe and field.  That is the second fuse into a volume whose pool an evict and an insert have re-ordered: the
stale sums meet other voxels than on the fresh context only because pool placement is a race, so the orders see this defect by
accident.  What sees it by construction is test_fresh_equals_reference, which fails for that recipe and for "cloud_fuse_dense_plain",
the recipes that fuse twice into one volume.  Between two recipes the defect cannot show: icp_tsdf_create, icp_tsdf_create_hashed and
icp_tsdf_release drop the accumulators, so they never outlive a volume (see REQUIRED_PAIRS["volume"]).
The two other defects of that kind -- the clear of the triangle table in mc_run dropped, the +2048 pointer taken before ensure_pinned in
one driver -- were not run: the first makes k_mc_tri_insert read canon[] through whatever words the table's place held before (indices
of no bound), the second makes the host read, and a copy write, a page-locked block that has been freed.  From the code alone: the
first can show at "mesh_cluster_63" behind "mesh_cluster_262145" (the small call's table lies where the large call's canonical triples
lay; fields "triangles" and "info"), the second at a step whose driver asks for more than the block holds: "hmap_4099" behind
"run_m1_65" (field "insert_0"), "run_m1_long" behind "mesh_cluster_no_triangles" and "multistart_256" behind "cloud_fuse_hashed_plain".
"""
import os
import subprocess
import time

import numpy as np
import pytest

import context_reuse_cases as R
import support as S

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_FRESH = {}


def fresh(name, form, factory):
    """The recipe's result on a fresh context of the given loop form, computed once and left unchanged."""
    key = (name, form if R.RECIPES[name].per_form else None)
    if key not in _FRESH:
        ctx = S.make_ctx(factory, form)
        _FRESH[key] = R.run(name, ctx, fresh=True)
        ctx.close()
    return _FRESH[key]


FRESH_PARAMS = [(n, "merged") for n in R.RECIPES] + [(n, "separate") for n, r in R.RECIPES.items() if r.per_form]


def test_neutral_puts_every_option_back(gpu_ctx_factory):
    """After neutral every public option getter returns what it returns on a fresh context, whatever was set before."""
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    want = R.option_state(a)
    R.unsettle(b)
    moved = R.option_state(b)
    assert all(moved[k] != want[k] for k in want), [k for k in want if moved[k] == want[k]]
    R.neutral(b)
    got = R.option_state(b)
    assert got == want, [k for k in want if got[k] != want[k]]
    R.neutral(a)
    assert R.option_state(a) == want


@pytest.mark.parametrize("name,form", FRESH_PARAMS, ids=["%s-%s" % p for p in FRESH_PARAMS])
def test_fresh_equals_reference(gpu_ctx_factory, name, form):
    t = time.time()
    got = fresh(name, form, gpu_ctx_factory)
    R.check(name, got, lambda: S.make_ctx(gpu_ctx_factory, form))
    print("%s (%s): %s; %.2f s" % (name, form, R.RECIPES[name].reference, time.time() - t))


def run_order(order, form, factory, label, between=None):
    """The recipes of `order` on ONE context of the given form; every step against the fresh result, bit for bit."""
    want = [fresh(name, form, factory) for name in order]
    ctx = S.make_ctx(factory, form)
    prev = "a fresh context"
    t = time.time()
    for i, name in enumerate(order):
        if between is not None and i > 0:
            prev = "%s, then %s" % (prev, between(i, ctx))
        got = R.run(name, ctx)
        d = R.first_difference(got, want[i])
        assert d is None, "%s, %s form, step %d: %s behind %s: first differing field %s" % (label, form, i, name, prev, d)
        prev = name
    print("%s, %s form: %d steps, every one the fresh context's bits; %.2f s" % (label, form, len(order), time.time() - t))
    ctx.close()


@pytest.mark.parametrize("form", S.FORMS)
def test_fixed_sequence(gpu_ctx_factory, form):
    run_order(R.FIXED_ORDER, form, gpu_ctx_factory, "the fixed order")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_orders(gpu_ctx_factory, seed):
    names = list(R.RECIPES)
    order = [names[i] for i in np.random.default_rng(seed).permutation(len(names))]
    run_order(order, S.FORMS[seed % 2], gpu_ctx_factory, "seed %d" % seed)


# ---- one refused call per family, between two recipes
def refusals():
    """[(label, the call icp_last_error must name, the refused call: ctx -> the message it left, the recipe to run behind it)]."""
    from icp_amd import binding as B

    def raises(call):
        def go(ctx):
            with pytest.raises(B.IcpError) as e:
                call(ctx)
            assert e.value.code == B.ICP_OK + 1, e.value
            return ctx.lib.icp_last_error(ctx.h).decode()
        return go

    def cluster_one_short(ctx):
        import test_gpu_mesh_cluster as TMC
        case, want = TMC.reference("random_mesh", (257,))
        rc, arrays, info, msg = TMC._raw(ctx, case, want[4]["n_vertices"] - 1, want[4]["n_triangles"])
        assert rc == 1 and all((a == 7).all() for a in arrays)
        return msg

    def multistart_with_reciprocal(ctx):
        ctx.set_reciprocal_options(True)
        with pytest.raises(B.IcpError) as e:
            ctx.run_multistart([np.eye(4, dtype=f32)])
        assert e.value.code == B.ICP_OK + 1, e.value
        return ctx.lib.icp_last_error(ctx.h).decode()

    def no_volume(call):
        def go(ctx):
            R.release_volume(ctx)
            return raises(call)(ctx)
        return go
    return [
        ("a capacity one short", "icp_mesh_cluster", cluster_one_short, "mesh_cluster_63"),
        ("robust options out of range", "icp_set_robust_options", raises(lambda c: c.set_robust_options("huber", overlap=1.5)), "run_robust"),
        ("GICP options out of range", "icp_set_gicp_options", raises(lambda c: c.set_gicp_options(1e-3, 7)), "run_gicp"),
        ("NSS options out of range", "icp_set_nss_options", raises(lambda c: c.set_nss_options(4, True)), "run_m1_nss"),
        ("global options out of range", "icp_set_global_options", raises(lambda c: c.set_global_options(k=7)), "global_k5"),
        ("depth filter out of range", "icp_set_depth_filter_options", raises(lambda c: c.set_depth_filter(9)), "depth_clouds_33x17_filtered"),
        ("carve options out of range", "icp_set_tsdf_carve_options", raises(lambda c: c.set_tsdf_carve(-1.0)), "cloud_fuse_hashed_carved"),
        ("a cloud fuse without a volume", "icp_tsdf_integrate_cloud", no_volume(lambda c: c.tsdf_integrate_cloud("source")), "cloud_fuse_dense_plain"),
        ("a clustered mesh without a volume", "icp_tsdf_mesh_clustered", no_volume(lambda c: c.tsdf_mesh(cluster=0.2)), "tsdf_mesh_clustered_dense"),
        ("an SDF sample without a volume", "icp_tsdf_sample", no_volume(lambda c: c.tsdf_sample(np.zeros((3, 3), f32))), "sdf_6"),
        ("a scan aligned without a volume", "icp_tsdf_align_cloud", no_volume(lambda c: c.tsdf_align_cloud("source")), "align_cloud_1"),
        ("an evict without a hashed volume", "icp_tsdf_evict_blocks", no_volume(lambda c: c.tsdf_evict_blocks((0.0, 0.0, 0.0), 1.0)), "htsdf_evict_insert"),
        ("an insert without a voxel map", "icp_voxel_map_insert", raises(lambda c: (c.voxel_map_destroy(), c.voxel_map_insert(1, np.eye(4, dtype=f32)))), "hmap_1"),
        ("multi-start with reciprocal rejection on", "icp_run_multistart", multistart_with_reciprocal, "multistart_1"),
        ("convergence options out of range", "icp_set_convergence_options", raises(lambda c: c.set_convergence_options(1e-6, 1e-6, 1, 9)), "run_m1"),
    ]


def test_refused_call_in_between(gpu_ctx_factory):
    table = refusals()
    order = ["vgicp_6"] + [t[3] for t in table]

    def between(i, ctx):
        label, who, call, _ = table[i - 1]
        msg = call(ctx)
        assert who in msg, (label, msg)
        return "the refused call (%s: %s)" % (label, who)
    run_order(order, "merged", gpu_ctx_factory, "refused calls in between", between)


# ---- a context on the caller's stream
SRC = os.path.join(ROOT, "tests", "cpp", "caller_stream.cpp")
LIBDIR = os.path.join(ROOT, "icp-variants_amd", "lib")
STEP = ["timeout", "-k", "10"]


def build_driver(tmp):
    """The driver linked against libicp_hip.so and the HIP runtime that library is bound to."""
    exe = os.path.join(tmp, "caller_stream")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call(STEP + ["300", hipcc, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                                  "-L", LIBDIR, "-licp_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + rocm_lib])
    return exe


def stream_inputs():
    import mesh_cluster_cases as K
    from icp_amd.synth import tum_K, wavy_depth
    b = R.bunny()
    W, H = 33, 17
    Kc = tum_K(W)
    cam = f32([Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2], W, H])
    vol = f32([9, 9, 9, -0.2, -0.2, 0.8, 0.05])
    depth = np.ascontiguousarray(wavy_depth(W, H, 1.0), f32)
    mesh = K.random_mesh(63)
    grid = f32([mesh["cell_size"]] + list(mesh["origin"]))
    return dict(b=b, W=W, H=H, K=Kc, cam=cam, vol=vol, depth=depth, mesh=mesh, grid=grid)


def write_inputs(path, d):
    b = d["b"]
    with open(path, "wb") as f:
        for a in (b["src_pts"], b["src_nrm"], b["tgt_pts"], b["tgt_nrm"], d["depth"], d["cam"], d["vol"], d["mesh"]["vertices"]):
            a = np.ascontiguousarray(a, f32)
            f.write(np.int32(a.size).tobytes()); f.write(a.tobytes())
        t = np.ascontiguousarray(d["mesh"]["triangles"], np.uint32)
        f.write(np.int32(t.size).tobytes()); f.write(t.tobytes())
        f.write(np.int32(d["grid"].size).tobytes()); f.write(d["grid"].tobytes())


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(-1).tolist() if a.dtype.itemsize == 4 else np.ascontiguousarray(a, np.int32).view(np.uint32).reshape(-1).tolist()


def default_context_results(factory, d):
    """The driver's calls on a default context, as the driver prints them: {label: words}."""
    from icp_amd import binding as B
    out = {}
    b = d["b"]

    def bunny_run(ctx, metric, label):
        S.configure(ctx, metric=metric, knn_backend=S.LBVH, n_iterations=5, max_distance=0.0003, seed=ctx.params.selection_seed)
        ctx.set_target(b["tgt_pts"], b["tgt_nrm"]); ctx.set_source(b["src_pts"], b["src_nrm"])
        pose, recs, rc = ctx.run(np.eye(4, dtype=f32))
        out[label + "_pose"] = words(B.pose_to_c(pose))
        rec = []
        for r in recs:
            rec += [r["n_src"], r["n_valid"], r["status"]] + words(B.pose_to_c(r["pose"]))
        out[label + "_records"] = rec
    ctx = factory()
    bunny_run(ctx, 1, "run")
    v = d["vol"]
    ctx.tsdf_create(dims=(int(v[0]), int(v[1]), int(v[2])), origin=(float(v[3]), float(v[4]), float(v[5])), voxel_size=float(v[6]))
    out["volume_updated"] = [ctx.tsdf_integrate(d["depth"], B.depth_camera(d["K"], d["W"], d["H"]), np.eye(4, dtype=f32))]
    vert, nrm, tris = ctx.tsdf_mesh(0.0)
    out["volume_vertices"], out["volume_normals"], out["volume_triangles"] = words(vert), words(nrm), words(tris)
    assert out["volume_updated"][0] > 0 and len(tris) > 0
    ctx.tsdf_release()
    m = d["mesh"]
    cv, _, _, ct, info = ctx.mesh_cluster(m["vertices"], m["triangles"], m["cell_size"], origin=m["origin"])
    out["cluster_info"] = [info[k] for k, _ in B.IcpMeshClusterInfo._fields_]
    out["cluster_vertices"], out["cluster_triangles"] = words(cv), words(ct)
    other = factory()
    bunny_run(other, 0, "metric0")
    return out


def test_caller_stream(gpu_ctx_factory, tmp_path):
    """Two contexts made on the caller's streams, a blocking and a non-blocking one, with the caller's own 64 MB memset enqueued in front of
    every library call: every result is the default context's, bit for bit; two contexts on one stream, their runs in turn, likewise; the
    streams are idle, usable and the caller's to destroy once the contexts are gone."""
    d = stream_inputs()
    want = default_context_results(gpu_ctx_factory, d)
    exe = build_driver(str(tmp_path))
    path = os.path.join(str(tmp_path), "inputs.bin")
    write_inputs(path, d)
    p = subprocess.run(STEP + ["120", exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, "the driver ended with %d:\n%s" % (p.returncode, p.stderr.decode()[-4000:])
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "streams ok", lines[-3:]
    got = {ln.split()[0]: [int(w, 16) for w in ln.split()[1:]] for ln in lines[:-1]}
    for s in ("blocking", "nonblocking"):
        for label, w in want.items():
            if label.startswith("metric0"):
                continue
            assert got["%s_%s" % (s, label)] == w, (s, label)
    for rnd in (0, 1):
        for part in ("pose", "records"):
            assert got["shared_a%d_%s" % (rnd, part)] == want["run_" + part], (rnd, part)
            assert got["shared_b%d_%s" % (rnd, part)] == want["metric0_" + part], (rnd, part)
    assert want["run_pose"] != want["metric0_pose"]
    print("caller's stream: %d results, every word the default context's; the streams outlived the contexts" % (len(got)))
