"""Recipes for tests/test_gpu_context_reuse.py (the device) and tests/test_context_reuse_host.py (the table itself, without a device).
Test infrastructure only.

A recipe is one public call family run to the end on a context: `run(name, ctx)` puts the context back to neutral, loads what the call
needs, sets every option it depends on, makes the call and returns a list of (field, value) pairs that can be compared bit for bit --
fp32 arrays through support.bits, fp64 and integer arrays by their bytes, records and info dicts field by field.  The property under
test is that `run(name, ctx)` on a context that has been used for anything else returns what it returns on a fresh one.  `check(name,
fresh, factory)` ties the fresh result to the reference that family already has in the suite, with that test's own bound, so that the
sequences are not a comparison of the code with itself.

The shared resources of a context (icp-variants_amd/csrc/host_ctx.hpp) and the demand a recipe puts on them (RECIPES[name].uses):

  pinned     the page-locked block: pose at 0, prune counters at 2016, hashed-map words at 2032, count slot / SDF state and record at
             2048, the loop's lay_out from 256, the multi-start's records and results.  "large": more than its first 4096 bytes.
  staging    cloud uploads, level builds, normals, back-projection, depth mesh, depth filter, ray-casts
  tm         tm_bits / tm_mask / tm_base / tm_blk / tm_out (+ tm_nbr / tm_ord): layouts "dense", "hashed", "clustered"
  sdf        sdf_partials / sdf_state: layouts "28+2" and "29+3", by block count
  loop       partials / partials2 / ring / totals / sums / stats / block_t1 and the multi-start's slices
  select     d_count / sel_temp / depth_blocks / sel_blocks / nss_table
  volume     tc_acc / tcc_acc (zero between calls), te_work and the outboxes
  events     the event list, indexed by position
  mc         the mesh-cluster scratch mc_*

HISTORY_FIELDS below lists what is history by contract and therefore left out of a recipe's fields.

Findings while writing the table (no defect, but worth knowing):
  * the non-linear optimiser's options and the stage-timing mode have no getter, so `option_state` cannot show that `neutral` puts
    them back; `neutral` sets both unconditionally and every loop recipe runs behind it.
  * the loop form (merged / separate) is read once, at icp_ctx_create; it is a property of the context, not an option.  The sequences
    therefore run once per form, and the loop recipes' fresh results are cached per form.
"""
import ctypes as C
import functools
import os

import numpy as np

import support as S

f32, f64 = np.float32, np.float64
EYE = np.eye(4, dtype=f32)
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
RESOURCES = ("pinned", "staging", "tm", "sdf", "loop", "select", "volume", "events", "mc")

# History by contract: these fields of an info record depend on what the context did before the call, and are left out of a recipe's
# fields.  Nothing else is left out.  (Timings -- icp_get_timing, icp_get_iteration_times, the pass times of icp_debug_*_time -- and the
# icp_debug_* counters are never asked for by a recipe; they are listed so that the table says so in one place.)
HISTORY_FIELDS = {
    "timing": ("match_ms", "weight_reject_build_ms", "solve_ms", "total_ms", "iterations", "sampled_iterations"),
    "tsdf_hashed_info": ("n_grown",),                       # growths of the pool so far
    "tsdf_stream_info": ("n_grown", "n_moved"),             # n_moved: the kept blocks that sat at or above n_keep; where a block sits in the pool is a race by contract (dev_tsdf_hash_evict.hpp)
    "voxel_hash_map_info": ("n_grown",),                    # rehashes so far
    "voxel_map_prune_info": ("n_compacted",),               # compactions so far
    "tsdf_carve_stats": ("n_carved_total",),                # since the options were last set
    "tsdf_cloud_info": (), "voxel_map_insert_info": (), "mesh_cluster_info": (), "iter_stats": (), "sdf_frame": (), "sdf_iter": (),
    "sdf_color_frame": (), "sdf_color_iter": (), "start_result": (), "convergence_result": (), "lm_summary": (), "robust_stats": (),
    "reciprocal_stats": (), "track_frame": (),
}


def info_struct(kind):
    """The ctypes record a kind of info dict is read from (the host test derives the keys from it)."""
    from icp_amd import binding as B
    return dict(timing=B.IcpTiming, tsdf_hashed_info=B.IcpTsdfHashedInfo, tsdf_stream_info=B.IcpTsdfStreamInfo, voxel_hash_map_info=B.IcpVoxelHashMapInfo,
                voxel_map_prune_info=B.IcpVoxelMapPruneInfo, tsdf_carve_stats=B.IcpTsdfCarveInfo, tsdf_cloud_info=B.IcpTsdfCloudInfo,
                voxel_map_insert_info=B.IcpVoxelMapInsertInfo, mesh_cluster_info=B.IcpMeshClusterInfo, iter_stats=B.IcpIterStats, sdf_frame=B.IcpSdfFrame,
                sdf_iter=B.IcpSdfIter, sdf_color_frame=B.IcpSdfColorFrame, sdf_color_iter=B.IcpSdfColorIter, start_result=B.IcpStartResult,
                convergence_result=B.IcpConvergenceResult, lm_summary=B.IcpLmSummary, robust_stats=B.IcpRobustStats, reciprocal_stats=B.IcpReciprocalStats,
                track_frame=B.IcpTrackFrame)[kind]


RESERVED = ("reserved", "pad")                                    # padding words of a record; the binding drops them from some dicts itself


def shaped(kind, d):
    """An info dict of `kind` as a recipe compares it: every key but HISTORY_FIELDS[kind] (and padding)."""
    drop = HISTORY_FIELDS[kind] + RESERVED
    return {k: v for k, v in d.items() if k not in drop}


def shaped_list(kind, records):
    return [shaped(kind, r) for r in records]


# ---------------------------------------------------------------------------------------------------- comparing
def canon(x):
    """A value as something `==` compares bit for bit."""
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        if a.dtype == np.float32:
            return ("f32", a.shape, S.bits(a).tobytes())
        return (str(a.dtype), a.shape, a.tobytes())
    if isinstance(x, dict):
        return {k: canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return ("f64", np.float64(x).tobytes())
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, C.Structure):
        return bytes(x)
    return x


def first_difference(got, want):
    """The name of the first field of two recipe results that differs, or None."""
    if [k for k, _ in got] != [k for k, _ in want]:
        return "the field names: %s / %s" % ([k for k, _ in got], [k for k, _ in want])
    for (k, a), (_, b) in zip(got, want):
        ca, cb = canon(a), canon(b)
        if ca != cb:
            if isinstance(ca, dict) and isinstance(cb, dict):
                return "%s[%s]" % (k, next((q for q in ca if q not in cb or ca[q] != cb[q]), "keys"))
            if isinstance(ca, list) and isinstance(cb, list) and len(ca) == len(cb):
                i = next(i for i in range(len(ca)) if ca[i] != cb[i])
                if isinstance(ca[i], dict) and isinstance(cb[i], dict):
                    return "%s[%d][%s]" % (k, i, next((q for q in ca[i] if q not in cb[i] or ca[i][q] != cb[i][q]), "keys"))
                return "%s[%d]" % (k, i)
            return k
    return None


def field(result, name):
    return dict(result)[name]


# ---------------------------------------------------------------------------------------------------- neutral
def neutral(ctx):
    """Every option family back to what a fresh context has; volume and map released."""
    from icp_amd import binding as B
    ctx.params = B.default_params()
    ctx.push_params()
    ctx.set_gicp_options(); ctx.set_colored_options(); ctx.set_robust_options(); ctx.set_reciprocal_options(False)
    ctx.set_convergence_options(None); ctx.set_nss_options(); ctx.set_global_options(); ctx.set_optimizer(None)
    ctx.set_depth_filter(radius=0); ctx.set_tsdf_carve(0.0, 0.0); ctx.set_stage_timing(1)
    release_volume(ctx); ctx.voxel_map_destroy()


def release_volume(ctx):
    """icp_tsdf_release where the context holds a volume (the call is refused where it holds none)."""
    rc = ctx.lib.icp_tsdf_release(ctx.h)
    assert rc in (0, 1), ctx.lib.icp_last_error(ctx.h).decode()
    ctx._tsdf_dims = None


def option_state(ctx):
    """What every public option getter returns, as bytes by family."""
    from icp_amd import binding as B
    p = B.IcpParams()
    ctx._ck(ctx.lib.icp_get_params(ctx.h, C.byref(p)))
    return dict(params=bytes(p), gicp=bytes(ctx.gicp_options()), colored=bytes(ctx.colored_options()), robust=bytes(ctx.robust_options()),
                reciprocal=bytes(ctx.reciprocal_options()), convergence=bytes(ctx.convergence_options()), nss=bytes(ctx.nss_options()),
                global_registration=bytes(ctx.global_options()), depth_filter=bytes(ctx.depth_filter_options()), carve=bytes(ctx.tsdf_carve_options()))


def unsettle(ctx):
    """Every option family away from its default (what `neutral` has to undo); needs no cloud."""
    p = ctx.params
    p.metric, p.weighting, p.rejection, p.n_iterations, p.multires, p.selection, p.selection_proba, p.selection_seed, p.max_distance = 2, 1, 0, 7, 1, 2, 0.25, 99, 0.5
    p.knn_backend, p.knn_incremental, p.record_rmse = 1, 1, 1
    ctx.push_params()
    ctx.set_gicp_options(1e-2, 10); ctx.set_colored_options(0.5, 10); ctx.set_robust_options("tukey", 2.0, 0.1, 0.6); ctx.set_reciprocal_options(True)
    ctx.set_convergence_options(1e-4, 1e-4, 2, 2); ctx.set_nss_options(7, False); ctx.set_global_options(k=5, feature_stride=3, mutual=0, n_hypotheses=64, seed=5, n_best=2)
    ctx.set_optimizer(True, max_num_iterations=3); ctx.set_depth_filter(2, 3.0, 0.05); ctx.set_tsdf_carve(1.0, 0.25); ctx.set_stage_timing(0)


# ---------------------------------------------------------------------------------------------------- the table
class Recipe:
    """name; setup(ctx) -> state (loads and options, behind neutral); call(ctx, state) -> [(field, value)]; check(fresh, factory): the
    fresh result against `reference` (a sentence naming it and its bound); uses: resource -> demand ("large" / "small" / a layout);
    pin: bytes asked of the page-locked block; iters: iterations of its loop (0: none); per_form: the result depends on the loop form."""

    def __init__(self, name, setup, call, check, reference, uses, pin=4096, iters=0, per_form=False):
        self.name, self.setup, self.call, self.check, self.reference, self.uses, self.pin, self.iters, self.per_form = name, setup, call, check, reference, dict(uses), pin, iters, per_form


RECIPES = {}


def add(name, setup, call, check, reference, uses, **kw):
    assert name not in RECIPES, name
    RECIPES[name] = Recipe(name, setup, call, check, reference, uses, **kw)


def run(name, ctx, fresh=False):
    """The recipe on `ctx`.  fresh: this is the run on a fresh context whose result is cached; a stateful recipe's state is kept from it."""
    r = RECIPES[name]
    neutral(ctx)
    out = r.call(ctx, r.setup(ctx))
    if getattr(r.call, "stateful", False):
        out, state = out
        if fresh:
            _STATE[name] = state
    return out


def prepared(name, factory):
    """A fresh context behind the recipe's neutral + setup: where a reference needs the device (a teacher-forced restatement)."""
    ctx = factory()
    neutral(ctx)
    return ctx, RECIPES[name].setup(ctx)


def check(name, fresh, factory):
    RECIPES[name].check(fresh, factory)


def assert_equal(got, want, what):
    d = first_difference(got, want)
    assert d is None, "%s: first differing field %s" % (what, d)


# ---- the page-locked block's demand, from host_loop.hpp (LoopRun::lay_out), host_multi.hpp and the fixed slots
SIZEOF = dict(pose_state=128, iter_stats=84, run_tail=512, convergence_step=16, lm_summary=104, start_result=80, sdf_frame=104)
PIN_MIN = 4096


def _pad(b):
    return (b + 255) & ~255


def pin_loop(iters, lm=False, cvg=False):
    """LoopRun::lay_out: pose state | records | tail | trace | stamps | LM records."""
    tail = 256 + _pad(iters * SIZEOF["iter_stats"])
    stamps = tail + SIZEOF["run_tail"] + (_pad(iters * SIZEOF["convergence_step"]) if cvg else 0)
    lm_at = stamps + _pad(2 * (iters + 1) * 8)
    return lm_at + (iters * SIZEOF["lm_summary"] if lm else 0)


def pin_multi(starts, iters):
    """icp_run_multistart: pose states up | records down | results down."""
    rec = _pad(starts * SIZEOF["pose_state"])
    return rec + _pad(starts * max(iters, 1) * SIZEOF["iter_stats"]) + starts * SIZEOF["start_result"]


PIN_SLOT = 4096                                             # count_slot / read_count, the SDF driver's state and record at 2048
PIN_MAP = 4096 + SIZEOF["sdf_frame"]                        # host_hmap.hpp and host_vmap_prune.hpp: the words in front of the record's place


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def bunny():
    d = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pair.npz"))
    out = {k: d[k] for k in d.files}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bunny65():
    """The bunny pair with the first 65 source points: one wave and one point."""
    b = dict(bunny())
    for k in ("src_pts", "src_nrm", "src_rgba"):
        b[k] = np.ascontiguousarray(b[k][:65])
    return b


@functools.lru_cache(maxsize=None)
def rgbd():
    from icp_amd import synth
    d = synth.compact_rgbd_pair()
    return {k: d[k] for k in ("src_pts", "src_nrm", "src_rgba", "tgt_pts", "tgt_nrm", "tgt_rgba")}


def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def clouds_of(d):
    return tuple(d.get(k) for k in ("src_pts", "src_nrm", "src_rgba", "tgt_pts", "tgt_nrm", "tgt_rgba"))


# ---------------------------------------------------------------------------------------------------- icp_run
SEED = 1234
ITERS = 5
LONG_ITERS = 40                                             # the loop recipe with the largest iteration count: its lay_out passes 4096 bytes


def run_fields(ctx, pose, recs, rc):
    return [("pose", pose), ("status", rc), ("records", shaped_list("iter_stats", recs)), ("convergence", shaped("convergence_result", ctx.convergence()))]


def add_run(name, data, reference, check_fn, iters=ITERS, colors=True, options=None, extra=None, lm=False, uses=None, **params):
    """An icp_run recipe: support.configure(**params), the option setter `options(ctx)`, the clouds of `data()`; fields: the pose, the
    status, the records, icp_get_convergence, the query sets of a run with a selection and extra(ctx)."""
    params = dict(dict(metric=1, knn_backend=S.LBVH, max_distance=0.0003, seed=SEED, proba=0.5), n_iterations=iters, **params)

    def setup(ctx):
        S.configure(ctx, **params)
        if options:
            options(ctx)
        S.load(ctx, data(), colors=colors)
        return data()

    def call(ctx, d):
        pose, recs, rc = ctx.run(EYE, check=False)
        out = run_fields(ctx, pose, recs, rc)
        if params.get("selection"):
            out.append(("selection", [ctx.selection(i) for i in range(len(recs))]))
        return out + (extra(ctx) if extra else [])
    u = dict(pinned="large" if pin_loop(iters, lm) > PIN_MIN else "small", loop="large" if iters > ITERS or len(data()["src_pts"]) > 1000 else "small", staging="small")
    if params.get("selection") or params.get("multires"):
        u["select"] = "large" if len(data()["src_pts"]) > 1000 else "small"
    if params.get("knn_backend") == 0 or params.get("metric") != 1:
        u["events"] = "small" if iters <= ITERS else "large"          # the separate launches bracket their stages with 4 events an iteration
    u.update(uses or {})
    add(name, setup, call, lambda fresh, factory: check_fn(name, fresh, factory, data(), params), reference, u, pin=pin_loop(iters, lm), iters=iters, per_form=True)


def check_oracle_pose(name, fresh, factory, d, params):
    """The linear metrics: the oracle's estimatePose within support.POSE_TOL, as smoke() and tests/test_gpu_multistart.py hold it."""
    orc = oracle()
    prm = orc.make_params(metric=params["metric"], n_iterations=params["n_iterations"], max_distance=params["max_distance"], solver_mode=1, multires=params.get("multires", 0),
                          selection=params.get("selection", 0), selection_proba=params["proba"] if params.get("selection") else 1.0, selection_seed=params["seed"])
    po, _ = orc.estimate_pose(prm, *clouds_of(d), EYE)
    err = float(np.abs(field(fresh, "pose") - po).max())
    print("%s: max |pose - oracle| = %.3g" % (name, err))
    assert field(fresh, "status") == 0 and len(field(fresh, "records")) == params["n_iterations"] and err < S.POSE_TOL, (name, err)


def check_nss(name, fresh, factory, d, params):
    """Normal-space sampling: the lists are nss_restatement's, and every iteration is the oracle's on the device's own list, within 1e-5
    (tests/test_gpu_nss.py::test_teacher_forced_parity)."""
    import nss_restatement as nss
    from icp_amd import binding as B
    orc = oracle()
    prm0 = B.default_params(); prm0.n_iterations, prm0.multires = params["n_iterations"], 0
    lists = nss.run_lists(d["src_pts"], d["src_nrm"], B.schedule(prm0, len(d["src_pts"])), params["proba"], params["seed"], grid=5, resample=True)
    prm = orc.make_params(metric=params["metric"], n_iterations=1, max_distance=params["max_distance"], solver_mode=1)
    before = EYE
    for i, (L, r, dev) in enumerate(zip(lists, field(fresh, "records"), field(fresh, "selection"))):
        assert np.array_equal(dev, L), (name, i)
        po, _, nv, _, _ = orc.iterate(prm, d["src_pts"][L], d["src_nrm"][L], d["src_rgba"][L], d["tgt_pts"], d["tgt_nrm"], d["tgt_rgba"], before)
        assert r["status"] == 0 and r["n_src"] == len(L) and r["n_valid"] == nv and np.abs(r["pose"] - po).max() < 1e-5, (name, i)
        before = r["pose"]


def check_gicp(name, fresh, factory, d, params):
    """GICP: tests/test_gpu_gicp.py::free_running on a context of its own -- every iteration within 1e-5 of gicp_restatement's step from the
    device's previous pose -- and the fresh result is that run, bit for bit."""
    import test_gpu_gicp as TG
    ctx, _ = prepared(name, factory)
    pose, recs = TG.free_running(ctx, d, params["n_iterations"])
    assert_equal(fresh[:3], run_fields(ctx, pose, recs, 0)[:3], name + " against the checked run")


def check_colored(name, fresh, factory, d, params):
    """Colored ICP: every iteration within 1e-5 of colored_restatement's step from the device's previous pose, n_valid exactly
    (tests/test_gpu_colored.py::test_free_running_against_restatement)."""
    import colored_restatement as CR
    ctx, _ = prepared(name, factory)
    grad = ctx.color_gradients()
    prev = EYE
    assert field(fresh, "status") == 0
    for i, r in enumerate(field(fresh, "records")):
        recs_i, _, _ = ctx.correspond(prev)
        s_ref, _ = CR.record_sums(recs_i, prev, d["src_pts"], d["tgt_pts"], d["tgt_nrm"], grad, d["src_rgba"], d["tgt_rgba"], 0.968)
        assert r["n_valid"] == int(s_ref[0]), (name, i)
        assert np.abs(r["pose"] - CR.compose(CR.solve(s_ref), prev)).max() <= 1e-5, (name, i)
        prev = r["pose"]


def check_lm(name, fresh, factory, d, params):
    """The non-linear optimiser: every iteration's summary is lm_restatement's (tests/test_gpu_lm.py::same_solve) and its pose within 1e-5,
    teacher-forced on the device's poses."""
    import lm_restatement as lm
    import test_gpu_lm as TL
    ctx, _ = prepared(name, factory)
    prev = EYE
    for i, (r, summ) in enumerate(zip(field(fresh, "records"), field(fresh, "lm"))):
        _, want, _, ref_pose = S.restated_step(ctx, d, params["metric"], prev)
        TL.same_solve(summ, want)
        assert r["status"] == (8 if want["termination"] == lm.NO_RESIDUALS else 0) and np.abs(r["pose"] - ref_pose).max() <= 1e-5, (name, i)
        prev = r["pose"]


ROBUST = dict(kernel="huber", overlap=0.7)


def check_robust(name, fresh, factory, d, params):
    """Trimmed + Huber: every iteration's stats are robust_restatement's on the option-off records at the incoming pose, counts equal and
    trim_d2 / sigma bit-equal (support.check_stats, tests/test_gpu_robust.py::test_free_running)."""
    import robust_restatement as R
    ctx, _ = prepared(name, factory)
    ctx.set_robust_options()
    prev = EYE
    st = field(fresh, "robust")
    assert len(st) == len(field(fresh, "records")) == params["n_iterations"]
    for i, r in enumerate(field(fresh, "records")):
        base, _, _ = ctx.correspond(prev)
        ref = R.robust(base, ctx.transform_points(d["src_pts"], prev), d["tgt_pts"], dict(ROBUST, kernel=1), 1)
        S.check_stats(st[i], ref["stats"], "%s iteration %d" % (name, i))
        assert r["n_valid"] == st[i]["n_kept"], (name, i)
        prev = r["pose"]


def check_reciprocal(name, fresh, factory, d, params):
    """Reciprocal rejection: every iteration's stats, n_valid and pose (1e-5) from the option-off records at the previous pose through
    reciprocal_restatement (tests/test_gpu_reciprocal.py::test_free_running_full_resolution)."""
    import gicp_restatement as G
    import robust_restatement as R
    import test_gpu_reciprocal as TR
    ctx, _ = prepared(name, factory)
    ctx.set_reciprocal_options(False)
    prev = EYE
    st = field(fresh, "reciprocal")
    for i, r in enumerate(field(fresh, "records")):
        raw, _ = ctx.match(prev)
        base, _, _ = ctx.correspond(prev)
        exp, stats, _ = TR.expected(base, raw, prev, d["src_pts"], d["tgt_pts"])
        assert st[i] == stats, (name, i)
        s, _ = R.sums(1, ctx.transform_points(d["src_pts"], prev), d["tgt_pts"], exp, tgt_nrm=d["tgt_nrm"])
        assert r["n_valid"] == int(s[0]) and np.abs(G.compose(G.solve(s), prev).astype(f64) - r["pose"]).max() <= 1e-5, (name, i)
        prev = r["pose"]


@functools.lru_cache(maxsize=None)
def shuffled_bunny():
    import test_gpu_reciprocal as TR
    return TR.shuffled(dict(bunny()))


ORACLE = "the CPU oracle's estimatePose, pose within support.POSE_TOL (1e-5)"
for _m in (0, 1, 2):
    add_run("run_m%d" % _m, bunny, ORACLE, check_oracle_pose, metric=_m)
add_run("run_m1_brute", bunny, ORACLE, check_oracle_pose, knn_backend=0)
add_run("run_m1_multires", bunny, ORACLE, check_oracle_pose, multires=1, max_distance=0.001)
add_run("run_m1_random", bunny, ORACLE, check_oracle_pose, selection=1)
add_run("run_m1_nss", bunny, "nss_restatement's lists exactly; the oracle's iterate on them, 1e-5", check_nss, selection=2, options=lambda c: c.set_nss_options(5, True))
add_run("run_m1_65", bunny65, ORACLE, check_oracle_pose)
add_run("run_m1_long", bunny, ORACLE, check_oracle_pose, iters=LONG_ITERS)
add_run("run_m1_timed", bunny, ORACLE, check_oracle_pose, knn_backend=0, metric=2, options=lambda c: c.set_stage_timing(1), uses=dict(events="small"))
add_run("run_gicp", bunny, "gicp_restatement's step from the device's previous pose, 1e-5; n_valid exactly", check_gicp, metric=3, colors=False,
        options=lambda c: c.set_gicp_options(S.GICP_EPS, 20))
add_run("run_colored", rgbd, "colored_restatement's step from the device's previous pose, 1e-5; n_valid exactly", check_colored, metric=4, max_distance=0.01,
        options=lambda c: c.set_colored_options(0.968, 20))
add_run("run_lm", bunny, "lm_restatement's Solve per iteration: same decisions, x to 1e-9, pose 1e-5", check_lm, lm=True, colors=False,
        options=lambda c: c.set_optimizer(True), extra=lambda c: [("lm", shaped_list("lm_summary", c.lm_summaries()))])
add_run("run_robust", bunny, "robust_restatement's stats per iteration: counts equal, trim_d2 and sigma bit-equal", check_robust,
        options=lambda c: c.set_robust_options(**ROBUST), extra=lambda c: [("robust", shaped_list("robust_stats", c.robust_stats()))])
add_run("run_reciprocal", shuffled_bunny, "reciprocal_restatement's stats exactly; the point-to-plane restatement's pose, 1e-5", check_reciprocal, colors=False,
        options=lambda c: c.set_reciprocal_options(True), extra=lambda c: [("reciprocal", shaped_list("reciprocal_stats", c.reciprocal_stats()))])
LOOP_RECIPES = [n for n, r in RECIPES.items() if r.iters and n != "run_m1_long"]


# ---------------------------------------------------------------------------------------------------- multi-start, global registration
def multistart_poses(k):
    from icp_amd.multistart import start_poses
    yaw = [0.0] if k == 1 else list(np.linspace(-8.0, 8.0, k))
    return start_poses(np.eye(4), yaw_deg=yaw, axis=(0, 1, 0), points=bunny()["src_pts"])


def add_multistart(k):
    name = "multistart_%d" % k

    def setup(ctx):
        S.configure(ctx, metric=1, knn_backend=S.LBVH, n_iterations=ITERS)
        S.load(ctx, bunny())
        return multistart_poses(k)

    def fields(res, stats, best):
        return [("results", shaped_list("start_result", res)), ("records", [shaped_list("iter_stats", s) for s in stats]), ("best", best)]

    def call(ctx, starts):
        return fields(*ctx.run_multistart(starts))

    def chk(fresh, factory):
        ctx, starts = prepared(name, factory)
        res, stats, best = S.assert_matches_icp_run(ctx, starts)
        assert best == S.expected_best(res)
        assert_equal(fresh, fields(res, stats, best), name + " against the starts checked one by one")
    add(name, setup, call, chk, "icp_run from every start on the same context, records and pose bit for bit (support.assert_matches_icp_run)",
        dict(pinned="large" if pin_multi(k, ITERS) > PIN_MIN else "small", loop="large" if k > 1 else "small", staging="small"), pin=pin_multi(k, ITERS), iters=ITERS, per_form=True)


add_multistart(256)
add_multistart(1)
LOOP_RECIPES += ["multistart_256", "multistart_1"]

GLOBAL_N, GLOBAL_H = 257, 512


def _global_setup(ctx):
    import global_cases as gc
    import test_gpu_global as TGL
    sp, sn, tp, tn = gc.sub_clouds(bunny(), GLOBAL_N, 0)
    TGL.configure(ctx)
    ctx.set_target(tp, tn); ctx.set_source(sp, sn)
    ctx.set_global_options(k=5, mutual=0, n_hypotheses=GLOBAL_H, edge_similarity=0.0, seed=gc.edge_seed(GLOBAL_N, 0, GLOBAL_H), n_best=16)
    return sp, tp


def _global_fields(ctx, poses, recs, rc):
    return [("poses", list(poses)), ("records", recs), ("status", rc), ("hypotheses", ctx.global_hypotheses())]


def _global_check(fresh, factory):
    import global_cases as gc
    import test_gpu_global as TGL
    ctx, (sp, tp) = prepared("global_k5", factory)
    hyp, _, _, poses, recs, rc = TGL.teacher_forced_ransac(ctx, sp, tp, gc.edge_seed(GLOBAL_N, 0, GLOBAL_H), GLOBAL_H, 16, edge_similarity=0.0, label="global_k5")
    assert_equal(fresh, [("poses", list(poses)), ("records", recs), ("status", rc), ("hypotheses", hyp)], "global_k5 against the checked run")


add("global_k5", _global_setup, lambda ctx, st: _global_fields(ctx, *ctx.register_global(check=False)), _global_check,
    "global_restatement: draws, statuses, counts exactly, poses 1e-5, sum_d2 to 1e-12 (tests/test_gpu_global.py::teacher_forced_ransac)",
    dict(pinned="small", staging="small", select="small"))


# ---------------------------------------------------------------------------------------------------- measures and normals
def measure_poses():
    from icp_amd import synth
    return EYE, synth.eth_like_pair(0, n_tilt=43, n_beam=135)["gt"].astype(f32), S.rand_pose(4)


@functools.lru_cache(maxsize=None)
def measure_pairs(n):
    import test_gpu_parity as TP
    from icp_amd import synth
    return TP.measure_pairs(synth.eth_like_pair(0, n_tilt=43, n_beam=135), n)


def add_measures(n):
    name = "measures_%d" % n

    def setup(ctx):
        src, ref = measure_pairs(n)
        ctx.set_convergence_reference(src, ref)
        return src, ref

    def call(ctx, st):
        return [("rmse", [ctx.rmse(T) for T in measure_poses()]), ("benchmark_error", [ctx.benchmark_error(T) for T in measure_poses()])]

    def chk(fresh, factory):
        import test_gpu_parity as TP
        orc = oracle()
        src, ref = measure_pairs(n)
        poses = measure_poses()
        for k, T in enumerate(poses):
            a, b = field(fresh, "benchmark_error")[k], orc.benchmark_error(src, ref, T)
            if n == 1:
                assert not np.isfinite(b) and (a == b or (np.isnan(a) and np.isnan(b))), (a, b)
            else:
                assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (a, b)
            a, b, b64 = field(fresh, "rmse")[k], orc.rmse(src, ref, T), TP.rmse_fp64_fold(orc, src, ref, T)
            assert abs(a - b64) < 1e-6 and (abs(a - b) < 1e-6 or (n == 65537 and k == 2)), (a, b, b64)
    add(name, setup, call, chk, "the oracle's rmse and benchmark error, 1e-6 and 2e-6 (tests/test_gpu_parity.py::test_measures_at_grid_edges)",
        dict(pinned="small", staging="large" if n > 1000 else "small"))


add_measures(65537)
add_measures(1)


def add_normals(n):
    name = "normals_%d" % n
    pts = lambda: bunny()["tgt_pts"][:n]

    def call(ctx, st):
        nrm, curv = ctx.estimate_normals(pts(), 5, (0.0, 0.0, 0.0))
        return [("normals", nrm), ("curvature", curv)]
    add(name, lambda ctx: None, call, lambda fresh, factory: S.check_normals(oracle(), pts(), 5, (0, 0, 0), field(fresh, "normals"), field(fresh, "curvature"), name),
        "the oracle's k-NN PCA normals on every point, 2e-6 (support.check_normals)", dict(staging="large" if n > 1000 else "small", select="small"))


add_normals(1359)
add_normals(65)


@functools.lru_cache(maxsize=None)
def frames(n, w, h):
    from icp_amd import synth
    K, depth, rgbx, gt = synth.camera_sequence(n, w, h)
    for a in (K, depth, rgbx):
        a.setflags(write=False)
    return K, depth, rgbx, gt


def _backproject_call(ctx, st):
    K, depth, rgbx, _ = frames(2, 160, 120)
    xyz, nrm, rgba, valid = ctx.backproject_depth(depth[0], rgbx[0], K)
    return [("xyz", xyz), ("normals", nrm), ("rgba", rgba), ("valid", valid)]


def _backproject_check(fresh, factory):
    K, depth, rgbx, _ = frames(2, 160, 120)
    o = oracle().backproject(depth[0], rgbx[0], K)
    assert_equal(fresh, [("xyz", o[0]), ("normals", o[1]), ("rgba", o[2]), ("valid", o[3].astype(bool))], "backproject against the oracle")


add("backproject_160x120", lambda ctx: None, _backproject_call, _backproject_check, "the oracle's backproject, bit for bit (tests/test_gpu_parity.py)", dict(staging="small"))


# ---------------------------------------------------------------------------------------------------- depth frames
FILTER_ON = dict(radius=3, sigma_space=4.5, sigma_range=0.03)


def add_depth_clouds(w, h, filt):
    name = "depth_clouds_%dx%d%s" % (w, h, "_filtered" if filt else "")
    pose = lambda: frames(2, w, h)[3][0].astype(f64)

    def setup(ctx):
        from icp_amd import binding as B
        S.configure(ctx, metric=1, knn_backend=S.LBVH, n_iterations=ITERS, max_distance=0.1, seed=0)
        if filt:
            ctx.set_depth_filter(**FILTER_ON)
        K, depth, rgbx, _ = frames(2, w, h)
        return B.depth_camera(K, w, h), B.depth_options(False, 3, 0.1, False)

    def call(ctx, st):
        cam, opt = st
        K, depth, rgbx, _ = frames(2, w, h)
        n_s = ctx.set_source_depth(depth[1], rgbx[1], cam, opt)
        n_t = ctx.set_target_depth(depth[0], rgbx[0], cam, opt)
        m, d2 = ctx.match(pose())
        return [("n_source", n_s), ("n_target", n_t), ("match_idx", m["idx"]), ("match_weight", m["weight"]), ("d2", d2)]

    def chk(fresh, factory):
        import test_gpu_depth_tracking as TD
        ctx, (cam, opt) = prepared(name, factory)
        orc = oracle()
        K, depth, rgbx, _ = frames(2, w, h)
        d = [ctx.filter_depth(depth[k], **FILTER_ON) if filt else depth[k] for k in (0, 1)]      # the filter itself: tests/test_gpu_depth_filter.py, bit for bit
        sp, sn, sc = TD.oracle_cloud(orc, d[1], rgbx[1], K, None, opt)
        tp, tn, tc = TD.oracle_cloud(orc, d[0], rgbx[0], K, None, opt)
        assert (field(fresh, "n_source"), field(fresh, "n_target")) == (len(sp), len(tp))
        ctx.set_depth_filter(radius=0)
        ctx.set_target(tp, tn, tc); ctx.set_source(sp, sn, sc)
        m, d2 = ctx.match(pose())
        assert_equal(fresh[2:], [("match_idx", m["idx"]), ("match_weight", m["weight"]), ("d2", d2)], name + " against the host-built clouds")
    add(name, setup, call, chk, "the oracle's PointCloud(depthMap) of the (host-filtered) frames: counts equal, the matcher's records bit for bit "
        "(tests/test_gpu_depth_tracking.py::_cloud_case, tests/test_gpu_depth_filter.py::test_resident_clouds_equal_host_filtered_frames)",
        dict(pinned="small", staging="large" if w > 100 else "small", select="large" if w > 100 else "small"))


for _w, _h in ((320, 240), (33, 17)):
    for _f in (False, True):
        add_depth_clouds(_w, _h, _f)


def _track_setup(ctx):
    from icp_amd import binding as B, tum
    S.configure(ctx, metric=1, knn_backend=S.LBVH, n_iterations=ITERS, max_distance=0.1, seed=0)
    K, depth, rgbx, gt = frames(3, 64, 48)
    to, so = tum.reconstruct_room_options(ctx.params)
    return B.depth_camera(K, 64, 48), to, so


def _track_call(ctx, st):
    cam, to, so = st
    K, depth, rgbx, gt = frames(3, 64, 48)
    pose, recs, rc = ctx.track_depth_frames(depth, rgbx, cam, to, so, gt=gt)
    return [("pose", pose), ("status", rc), ("frames", shaped_list("track_frame", recs))]


def _track_check(fresh, factory):
    import test_gpu_depth_tracking as TD
    ctx, (cam, to, so) = prepared("track_depth_frames_64x48", factory)
    K, depth, rgbx, gt = frames(3, 64, 48)
    _, _, ref = TD._host_loop(ctx, oracle(), K, depth, rgbx, gt, to, so)
    for k, (r, h) in enumerate(zip(field(fresh, "frames"), ref)):
        assert (r["n_src"], r["iterations"], r["status"]) == (h["n_src"], h["iterations"], h["status"]) and S.same_bits(r["pose"], h["pose"]), k
    assert len(ref) == 2 and S.same_bits(field(fresh, "pose"), ref[-1]["pose"])


add("track_depth_frames_64x48", _track_setup, _track_call, _track_check,
    "set_target once, then set_source + icp_run per frame with host-built clouds: records and poses bit for bit (tests/test_gpu_depth_tracking.py::_host_loop)",
    dict(pinned="small", staging="small", select="small", loop="small"), pin=pin_loop(ITERS), iters=ITERS, per_form=True)
LOOP_RECIPES.append("track_depth_frames_64x48")


def add_depth_mesh(w, h, flat):
    name = "depth_mesh_%dx%d" % (w, h)

    def inputs():
        from icp_amd.synth import tum_K
        if flat:
            return tum_K(w), np.full((h, w), 1.5, f32), None, np.inf
        K, depth, rgbx, _ = frames(2, w, h)
        return K, depth[0], rgbx[0], np.inf

    def call(ctx, st):
        from icp_amd import binding as B
        K, depth, rgbx, thr = inputs()
        v, c, t = ctx.depth_mesh(depth, rgbx, B.depth_camera(K, w, h), EYE, thr)
        return [("vertices", v), ("colors", c), ("triangles", t)]

    def chk(fresh, factory):
        from depth_mesh_restatement import mesh_spec
        K, depth, rgbx, thr = inputs()
        sv, sc, st = mesh_spec(depth, rgbx, K, EYE, thr)[:3]
        assert_equal(fresh, [("vertices", sv), ("colors", None if rgbx is None else sc), ("triangles", st.astype(np.uint32).reshape(-1, 3))], name + " against mesh_spec")
    add(name, lambda ctx: None, call, chk, "depth_mesh_restatement.mesh_spec, bit for bit (tests/test_gpu_depth_mesh.py)",
        dict(pinned="small", staging="large" if flat else "small", select="large" if flat else "small"))


add_depth_mesh(640, 480, True)                              # 1196 blocks: the scan's carry between chunks
add_depth_mesh(33, 17, False)


# ---------------------------------------------------------------------------------------------------- the dense TSDF volume
def mesh_fields(mesh, prefix="mesh_"):
    names = ("vertices", "normals", "triangles", "colors")
    return [(prefix + n, a) for n, a in zip(names, mesh)]


RAY_FROM = S.pose_of((0.0, 0.0, 0.0), (0.0, 0.0, -0.9))        # a camera in front of the analytic volumes, looking along +z


@functools.lru_cache(maxsize=None)
def sphere37():
    import test_gpu_tsdf_mesh as TM
    import tsdf_mesh_restatement as TMR
    return TMR.analytic_volume(TMR.sphere(TM.CENTRE, 0.4), **TM.SMALL)


def ray_fields(cast):
    return list(zip(("ray_depth", "ray_vertices", "ray_normals", "ray_hits"), cast))


def _dense_large_call(ctx, st):
    import test_gpu_tsdf_mesh as TM
    from icp_amd import binding as B
    from icp_amd.synth import tum_K
    vol = TM.fused_volume(ctx)                              # 37 x 21 x 29: four frames fused, every count against tsdf_restatement inside
    t, w = ctx.tsdf_volume()
    out = [("tsdf", t), ("weight", w)] + mesh_fields(ctx.tsdf_mesh(0.0))
    S.upload(ctx, sphere37())                               # the same shape with an analytic sphere: the ray-cast (the fused one holds NaNs with payloads)
    return out + ray_fields(ctx.tsdf_raycast(B.depth_camera(tum_K(40), 40, 30), RAY_FROM)), vol


def _dense_large_check(fresh, factory):
    import tsdf_mesh_restatement as TMR
    import tsdf_restatement as TS
    from icp_amd.synth import tum_K
    vol = fresh_state("tsdf_dense_37x21x29")
    cast = TS.raycast(sphere37(), TS.Camera(tum_K(40), 40, 30), RAY_FROM)
    assert cast[3] > 100
    want = [("tsdf", vol.tsdf), ("weight", vol.weight)] + mesh_fields(TMR.mesh(vol, 0.0)) + ray_fields(cast)
    assert_equal(fresh, want, "dense 37 x 21 x 29 against the restatements")


_STATE = {}


def fresh_state(name):
    """What a stateful recipe's call left beside its fields on its FRESH run (a restatement's volume): the reference needs it.  `run` keeps
    it only when it is told that the run is the fresh one, so a run in a sequence never replaces it."""
    return _STATE[name]


def with_state(call):
    """Marks a call that returns (fields, state)."""
    call.stateful = True
    return call


add("tsdf_dense_37x21x29", lambda ctx: None, with_state(_dense_large_call), _dense_large_check,
    "tsdf_restatement's integrate and raycast, tsdf_mesh_restatement's mesh: bit for bit (tests/test_gpu_tsdf_mesh.py::fused_volume)",
    dict(pinned="small", staging="small", tm="dense large", select="small"))

SMALL9 = dict(dims=(9, 9, 9), origin=(-0.4, -0.4, 0.6), voxel_size=0.1)      # 0.8 m across, around the surface a 33 x 17 frame sees 1 m away
SMALL_FRAME = (33, 17)
SMALL_POSES = (EYE, S.pose_of((0.02, -0.03, 0.01), (0.03, -0.02, 0.01)))


@functools.lru_cache(maxsize=None)
def small_frame():
    """(K, depth (17, 33), rgbx (561, 4)): a wavy surface around 1 m with a hole, a NaN and a step, and a seeded colour frame."""
    from icp_amd.synth import tum_K, wavy_depth
    w, h = SMALL_FRAME
    depth = wavy_depth(w, h, base=0.9)
    depth[3, 4] = -np.inf; depth[9, 20] = np.nan
    rgbx = np.random.default_rng(9).integers(0, 256, (w * h, 4), dtype=np.uint8)
    for a in (depth, rgbx):
        a.setflags(write=False)
    return tum_K(w), depth, rgbx


def add_dense_small(color):
    """9 x 9 x 9: the frame integrated from two poses, the volume, its mesh and its ray-cast (color: with the colour array)."""
    name = "tsdf_dense_9x9x9" + ("_color" if color else "")

    def call(ctx, st):
        from icp_amd import binding as B
        K, depth, rgbx = small_frame()
        cam = B.depth_camera(K, *SMALL_FRAME)
        ctx.tsdf_create(color=color, **SMALL9)
        out = [("counts_%d" % k, ctx.tsdf_integrate(depth, cam, P, rgbx=rgbx if color else None)) for k, P in enumerate(SMALL_POSES)]
        out += volume_fields(ctx, False, color=color) + mesh_fields(ctx.tsdf_mesh(0.0, colors=color))
        if color:
            d, v, n, rgba, hits, ncol = ctx.tsdf_raycast_color(cam, EYE)
            return out + ray_fields((d, v, n, hits)) + [("ray_rgba", rgba), ("ray_colored", ncol)]
        return out + ray_fields(ctx.tsdf_raycast(cam, EYE))

    def chk(fresh, factory):
        import tsdf_color_restatement as TCR
        import tsdf_mesh_restatement as TMR
        import tsdf_restatement as TS
        K, depth, rgbx = small_frame()
        rcam = TS.Camera(K, *SMALL_FRAME)
        vol = TS.Volume(**SMALL9)
        if color:
            vol = TCR.add_color(vol)
            want = [("counts_%d" % k, TCR.integrate_color(vol, depth, rgbx, rcam, P)) for k, P in enumerate(SMALL_POSES)]
            want += [("tsdf", vol.tsdf), ("weight", vol.weight), ("rgb", vol.rgb), ("cweight", vol.wc)]
            want += mesh_fields(tuple(TMR.mesh(vol, 0.0)) + (TCR.mesh_colors(vol, 0.0),))
            rd, rv, rn, rrgba, rhits, rncol, _ = TCR.raycast_color(vol, rcam, EYE)
            want += ray_fields((rd, rv, rn, rhits)) + [("ray_rgba", rrgba), ("ray_colored", rncol)]
            assert rncol > 20 and all(c[1] > 0 for _, c in want[:2])
        else:
            want = [("counts_%d" % k, TS.integrate(vol, depth, rcam, P)) for k, P in enumerate(SMALL_POSES)]
            want += [("tsdf", vol.tsdf), ("weight", vol.weight)] + mesh_fields(TMR.mesh(vol, 0.0))
            cast = TS.raycast(vol, rcam, EYE)
            want += ray_fields(cast)
            assert cast[3] > 20 and all(c > 0 for _, c in want[:2])
        assert len(dict(want)["mesh_triangles"]) > 20 and vol.weight.max() == 2
        assert_equal(fresh, want, name + " against the restatements")
    add(name, lambda ctx: None, call, chk, "tsdf_restatement's integrate and raycast, tsdf_mesh_restatement's mesh (tsdf_color_restatement's integrate_color, mesh_colors and "
        "raycast_color): counts, arrays and mesh bit for bit", dict(pinned="small", staging="small", tm="dense small", select="small"))


add_dense_small(False)
add_dense_small(True)


def _dense_color_integrate_call(ctx, st):
    """tests/test_gpu_tsdf_color.py::integrate_case: 37 x 21 x 29 with a crafted start, four coloured integrations, max_weight 2."""
    import test_gpu_tsdf_color as TC
    from icp_amd import binding as B
    K, W, H, (t0, w0, c0, wc0), _, steps = TC.integrate_case()
    ctx.tsdf_create(color=True, **TC.INT_OPTS)
    ctx.tsdf_upload(t0, w0); ctx.tsdf_color_upload(c0, wc0)
    cam = B.depth_camera(K, W, H)
    out = [("counts_%d" % k, ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx)) for k, (depth, rgbx, pose) in enumerate(steps)]
    return out + volume_fields(ctx, False, color=True)


def _dense_color_integrate_check(fresh, factory):
    import test_gpu_tsdf_color as TC
    import tsdf_color_restatement as TCR
    import tsdf_restatement as TS
    K, W, H, (t0, w0, c0, wc0), _, steps = TC.integrate_case()
    vol = TCR.add_color(TS.Volume(**TC.INT_OPTS))
    vol.tsdf, vol.weight, vol.rgb, vol.wc = t0.copy(), w0.copy(), c0.copy(), wc0.copy()
    want = [("counts_%d" % k, TCR.integrate_color(vol, depth, rgbx, TS.Camera(K, W, H), pose)) for k, (depth, rgbx, pose) in enumerate(steps)]
    assert_equal(fresh, want + [("tsdf", vol.tsdf), ("weight", vol.weight), ("rgb", vol.rgb), ("cweight", vol.wc)], "coloured integrate against tsdf_color_restatement")


add("tsdf_dense_color_integrate", lambda ctx: None, _dense_color_integrate_call, _dense_color_integrate_check,
    "tsdf_color_restatement.integrate_color: both counts and the four arrays bit for bit (tests/test_gpu_tsdf_color.py)", dict(pinned="small", staging="small"))


def _dense_color_raycast_call(ctx, st):
    import test_gpu_tsdf_color as TC
    from icp_amd import binding as B
    from icp_amd.synth import tum_K
    cam = B.depth_camera(tum_K(40), 40, 30)
    ctx.tsdf_create(color=True, **TC.RAY_OPTS)
    vol = TC.raycast_case(ctx, cam, 40, 30)                 # (fused on the device; the restatement's volume holds the device's arrays)
    d, v, n, rgba, hits, ncol = ctx.tsdf_raycast_color(cam, TC.RAY_POSES[1])
    return ray_fields((d, v, n, hits)) + [("ray_rgba", rgba), ("ray_colored", ncol)], vol


def _dense_color_raycast_check(fresh, factory):
    import test_gpu_tsdf_color as TC
    import tsdf_color_restatement as TCR
    import tsdf_restatement as TS
    from icp_amd.synth import tum_K
    rd, rv, rn, rrgba, rhits, rncol, _ = TCR.raycast_color(fresh_state("tsdf_dense_color_raycast"), TS.Camera(tum_K(40), 40, 30), TC.RAY_POSES[1])
    assert rncol > 50
    assert_equal(fresh, ray_fields((rd, rv, rn, rhits)) + [("ray_rgba", rrgba), ("ray_colored", rncol)], "coloured ray-cast against tsdf_color_restatement")


add("tsdf_dense_color_raycast", lambda ctx: None, with_state(_dense_color_raycast_call), _dense_color_raycast_check,
    "tsdf_color_restatement.raycast_color of the volume the device fused: the four arrays and both counts bit for bit (tests/test_gpu_tsdf_color.py)",
    dict(pinned="small", staging="small"))


# ---------------------------------------------------------------------------------------------------- direct SDF, VGICP (tests/fold_cases.py)
def vg_prefix(blocks):
    """The first `blocks` blocks of fold_cases' smallest VGICP source: a block count below fold_cases.VG_CASES, no new scene."""
    import fold_cases as F
    pts, nrm = F.vg_source(min(F.VG_CASES))
    return pts[:blocks * F.VG_BLOCK], nrm[:blocks * F.VG_BLOCK]


@functools.lru_cache(maxsize=None)
def vg_prefix_reference(blocks):
    import fold_cases as F
    import vgicp_restatement as VR
    return VR.system(F.vg_target()[2], *vg_prefix(blocks), F.vg_pose(), F.VG_EPS, 1)


def add_fold(name, kind, blocks, layout):
    import fold_cases as F

    def setup(ctx):
        if kind == "vgicp":
            ctx.set_gicp_options(F.VG_EPS, 0)
            ctx.set_target(*F.vg_target()[:2], None)
        else:
            vol = F.sdf_volume(kind == "color")
            ctx.tsdf_create(color=kind == "color", **F.VOLUME)
            ctx.tsdf_upload(vol.tsdf, vol.weight)
            if kind == "color":
                ctx.tsdf_color_upload(vol.rgb, vol.wc)

    def call(ctx, st):
        import test_gpu_fold_sizes as TF
        if kind == "vgicp" and blocks not in F.VG_CASES:
            ctx.set_source(*vg_prefix(blocks), None)
            sums, counts = ctx.vgicp_system(F.vg_pose(), voxel_size=F.VG_VOXEL, min_points=1)
        else:
            sums, counts = dict(sdf=TF.sdf_call, color=TF.color_call, vgicp=TF.vg_call)[kind](ctx, blocks)
        return [("sums", sums), ("counts", tuple(counts))]

    def chk(fresh, factory):
        import sdf_color_restatement as SCR
        import test_gpu_fold_sizes as TF
        if kind == "sdf":
            ref = TF.sdf_reference(blocks, 0.0); terms = ref[0][1]
        elif kind == "vgicp":
            ref = TF.vg_reference(blocks, 1) if blocks in F.VG_CASES else vg_prefix_reference(blocks)
            terms = ref[0][1]
            assert ref[0][0] > ref[0][1] > 0
        else:
            c = F.sdf_case(blocks)
            ref = SCR.system(F.sdf_volume(True), c["depth"], c["rgbx"], F.rcam_of(c), F.sdf_pose(), stride=c["stride"], weight=F.COLOR_WEIGHT); terms = ref[0][1] + ref[0][2]
        got = (field(fresh, "sums"), field(fresh, "counts"))
        TF.compare(name, blocks, got, got, ref, terms)
    add(name, setup, call, chk, "the restatement's system: counts exactly, every sum within n 2^-52 sum |term| (tests/test_gpu_fold_sizes.py::compare)",
        dict(pinned="small", sdf=layout, staging="large" if blocks > 100 else "small"))


add_fold("sdf_1200", "sdf", 1200, "28+2 large")
add_fold("sdf_6", "sdf", 6, "28+2 small")
add_fold("sdf_color_257", "color", 257, "29+3")
add_fold("vgicp_513", "vgicp", 513, "28+2 large")
add_fold("vgicp_6", "vgicp", 6, "28+2 small")


def _align_depth_setup(ctx):
    import fold_cases as F
    vol = F.sdf_volume()
    ctx.tsdf_create(**F.VOLUME)
    ctx.tsdf_upload(vol.tsdf, vol.weight)


def _align_depth_call(ctx, st):
    import fold_cases as F
    import test_gpu_fold_sizes as TF
    c = F.sdf_case(257)
    pose, rec, rc, trace = ctx.tsdf_align_depth(c["depth"], TF.camera(c), F.sdf_pose(), trace=True, stride=c["stride"], n_iterations=3, stop_rotation=0.0, stop_translation=0.0)
    return [("pose", pose), ("status", rc), ("record", shaped("sdf_frame", rec)), ("trace", shaped_list("sdf_iter", trace))]


def _align_depth_check(fresh, factory):
    import fold_cases as F
    import sdf_restatement as SR
    import test_gpu_fold_sizes as TF
    c = F.sdf_case(257)
    TF.follow("align_depth_257", 257, F.sdf_pose(), field(fresh, "record"), field(fresh, "status"), field(fresh, "trace"),
              lambda p: SR.system(F.sdf_volume(), c["depth"], F.rcam_of(c), p, stride=c["stride"]))
    assert S.same_bits(field(fresh, "pose"), field(fresh, "record")["pose"])


add("align_depth_257", _align_depth_setup, _align_depth_call, _align_depth_check,
    "sdf_restatement's step from the device's previous pose, support.POSE_TOL; n_valid exactly (tests/test_gpu_fold_sizes.py::follow)",
    dict(pinned="small", sdf="28+2 large", staging="small"), iters=3)


# ---------------------------------------------------------------------------------------------------- the hashed TSDF volume
def blocks_fields(ctx, colors=False):
    info, *arrays = ctx.tsdf_blocks(colors=colors)
    return [("blocks_info", shaped("tsdf_hashed_info", info))] + list(zip(("coords", "tsdf", "weight", "rgb", "cweight"), arrays))


def _htsdf_grow_call(ctx, st):
    import htsdf_cases as HC
    cam, _ = HC.camera()
    ctx.tsdf_create_hashed(block_capacity=1, **HC.STRADDLE)
    n = ctx.tsdf_integrate(HC.crafted_frame(), cam, HC.TILTED)
    return [("n_updated", n)] + blocks_fields(ctx)


def _htsdf_grow_check(fresh, factory):
    import htsdf_cases as HC
    import htsdf_restatement as HR
    _, rcam = HC.camera()
    hv = HR.HVolume(**HC.STRADDLE)
    assert field(fresh, "n_updated") == HR.integrate(hv, HC.crafted_frame(), rcam, HC.TILTED)
    rc, rt, rw = hv.sorted_blocks()
    info = field(fresh, "blocks_info")
    assert info["n_blocks"] == len(rc) and info["n_unplaced"] == 0 and info["n_out_of_range"] == hv.n_out_of_range and info["capacity"] >= len(rc) > 1
    assert_equal(fresh[2:], [("coords", rc), ("tsdf", rt), ("weight", rw)], "hashed integrate from one block against htsdf_restatement")


add("htsdf_integrate_growth", lambda ctx: None, _htsdf_grow_call, _htsdf_grow_check, "htsdf_restatement: coordinates, tsdf and weight bit for bit (tests/test_gpu_htsdf.py)",
    dict(pinned="small", staging="small", volume="hashed small"))

RAYCAST_CASE, RAYCAST_SIZE, RAYCAST_POSE = 4, 4, 0             # htsdf_raycast_cases: case B (2 x 2 x 2 blocks), 64 x 48, the first pose


def _hraycast_setup(ctx):
    import htsdf_raycast_cases as RC
    name, opts, c, t, w, _ = RC.all_cases()[RAYCAST_CASE]
    assert name == "B"
    ctx.tsdf_create_hashed(block_capacity=1 << 12, **{k: v for k, v in opts.items() if k != "dims"})
    ctx.tsdf_upload_blocks(c, t, w)


def _hraycast_call(ctx, st):
    import htsdf_raycast_cases as RC
    d, v, n, hits = ctx.tsdf_raycast_hashed(RC.camera(*RC.SIZES[RAYCAST_SIZE])[0], RC.all_cases()[RAYCAST_CASE][5][RAYCAST_POSE])
    return [("depth", d), ("vertices", v), ("normals", n), ("hits", hits)]


def _hraycast_check(fresh, factory):
    import htsdf_raycast_cases as RC
    d, v, n, hits, _ = RC.restated(RAYCAST_CASE, RAYCAST_SIZE, RAYCAST_POSE)
    assert hits > 100
    assert_equal(fresh, [("depth", d), ("vertices", v), ("normals", n), ("hits", hits)], "hashed ray-cast against htsdf_raycast_restatement")


add("htsdf_raycast_B", _hraycast_setup, _hraycast_call, _hraycast_check, "htsdf_raycast_restatement, bit for bit (tests/test_gpu_htsdf_raycast.py)",
    dict(pinned="small", staging="small"))


def _hraycast_color_setup(ctx):
    import htsdf_color_view_cases as VC
    name, opts, c, t, w, rgb, wc, _ = VC.all_cases()[RAYCAST_CASE]
    assert name == "B"
    ctx.tsdf_create_hashed(block_capacity=1 << 12, color=True, **{k: v for k, v in opts.items() if k != "dims"})
    ctx.tsdf_upload_blocks(c, t, w, rgb, wc)


def _hraycast_color_call(ctx, st):
    import htsdf_color_view_cases as VC
    import htsdf_raycast_cases as RC
    d, v, n, rgba, hits, ncol = ctx.tsdf_raycast_color_hashed(RC.camera(*VC.SIZES[RAYCAST_SIZE])[0], VC.all_cases()[RAYCAST_CASE][7][RAYCAST_POSE])
    return ray_fields((d, v, n, hits)) + [("ray_rgba", rgba), ("ray_colored", ncol)]


def _hraycast_color_check(fresh, factory):
    import htsdf_color_view_cases as VC
    d, v, n, rgba, hits, ncol = VC.restated(RAYCAST_CASE, RAYCAST_SIZE, RAYCAST_POSE)[:6]
    assert hits >= ncol > 100
    assert_equal(fresh, ray_fields((d, v, n, hits)) + [("ray_rgba", rgba), ("ray_colored", ncol)], "coloured hashed ray-cast against htsdf_color_view_restatement")


add("htsdf_raycast_color_B", _hraycast_color_setup, _hraycast_color_call, _hraycast_color_check,
    "htsdf_color_view_restatement.raycast_color: the four arrays and both counts bit for bit (tests/test_gpu_htsdf_color_view.py)", dict(pinned="small", staging="small"))


def add_hashed_mesh(name, make_blocks, demand):
    import htsdf_mesh_cases as MC

    def setup(ctx):
        ctx.tsdf_create_hashed(**MC.OPTS)
        ctx.tsdf_upload_blocks(*make_blocks())

    def chk(fresh, factory):
        import htsdf_mesh_restatement as HM
        c, t, w = make_blocks()
        order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
        want = HM.mesh(c[order], t[order], w[order], MC.OPTS["origin"], MC.OPTS["voxel_size"], 0.0)
        assert len(want[2]) > 0
        assert_equal(fresh, mesh_fields(want[:3]), name + " against htsdf_mesh_restatement")
    add(name, setup, lambda ctx, st: mesh_fields(ctx.tsdf_mesh_hashed(0.0)), chk, "htsdf_mesh_restatement, bit for bit (tests/test_gpu_htsdf_mesh.py)",
        dict(pinned="small", tm="hashed " + demand, events="large"))


def _case_b():
    import htsdf_mesh_cases as MC
    return MC.case_b()


def _case_a():
    import htsdf_mesh_cases as MC
    return MC.case_a()


add_hashed_mesh("htsdf_mesh_B", _case_b, "large")
add_hashed_mesh("htsdf_mesh_one_block", _case_a, "small")


def _evict_setup(ctx):
    import test_htsdf_evict_host as EH
    hv, _ = EH.lattice_volume()
    ctx.tsdf_create_hashed(block_capacity=1024, **EH.LATTICE)
    ctx.tsdf_upload_blocks(*hv.sorted_blocks())


def _evict_call(ctx, st):
    import test_htsdf_evict_host as EH
    info, ec, et, ew = ctx.tsdf_evict_blocks(EH.LATTICE_CENTRE, 1.5, hold=True)
    assert 0 <= info["n_moved"] <= min(info["n_blocks"], info["n_evicted"]), info          # (what tests/test_gpu_htsdf_evict.py holds it to)
    out = [("evict_info", shaped("tsdf_stream_info", info)), ("evicted_coords", ec), ("evicted_tsdf", et), ("evicted_weight", ew)] + blocks_fields(ctx)
    back = ctx.tsdf_insert_blocks(ec[:100], et[:100], ew[:100])
    return out + [("insert_info", shaped("tsdf_stream_info", back))] + [("after_" + k, v) for k, v in blocks_fields(ctx)]


def _evict_check(fresh, factory):
    import htsdf_evict_restatement as ER
    import test_gpu_htsdf_evict as TE
    import test_htsdf_evict_host as EH
    hv, _ = EH.lattice_volume()
    before = hv.sorted_blocks()
    n_ev, out = ER.evict(hv, EH.LATTICE_CENTRE, 1.5)
    info = field(fresh, "evict_info")
    assert info["n_evicted"] == n_ev == 729 - 123 and info["n_blocks"] == 123 and info["n_held"] == n_ev and info["capacity"] == 1024
    gone = tuple(field(fresh, k) for k in ("evicted_coords", "evicted_tsdf", "evicted_weight"))
    kept = tuple(field(fresh, k) for k in ("coords", "tsdf", "weight"))
    assert TE.same_blocks(kept, hv.sorted_blocks()) and TE.same_blocks(gone, TE.hv_blocks(out))
    ins = field(fresh, "insert_info")
    assert ins["n_inserted"] == 100 and ins["n_present"] == 0 and ins["n_blocks"] == 223
    after = tuple(field(fresh, "after_" + k) for k in ("coords", "tsdf", "weight"))
    want = TE.sort_blocks(np.concatenate([kept[0], gone[0][:100]]), np.concatenate([kept[1], gone[1][:100]]), np.concatenate([kept[2], gone[2][:100]]))
    assert TE.same_blocks(after, want) and len(before[0]) == 729


add("htsdf_evict_insert", _evict_setup, _evict_call, _evict_check,
    "htsdf_evict_restatement on the 9 x 9 x 9 lattice: resident and evicted sets bit for bit; the inserted blocks come back as they left (tests/test_gpu_htsdf_evict.py)",
    dict(pinned="small", volume="hashed large"))


# ---------------------------------------------------------------------------------------------------- cloud fuses
def volume_fields(ctx, hashed, color=False):
    if hashed:
        return blocks_fields(ctx, colors=color)
    t, w = ctx.tsdf_volume()
    out = [("tsdf", t), ("weight", w)]
    if color:
        rgb, wc = ctx.tsdf_color_volume()
        out += [("rgb", rgb), ("cweight", wc)]
    return out


def add_carved_fuse(name, case_name, demand):
    """A case of tests/tsdf_carve_cases.py on the device, as tests/test_gpu_tsdf_carve.py::run makes it."""
    import tsdf_carve_cases as K

    def call(ctx, st):
        import test_gpu_tsdf_carve as TCV
        c = K.CASES[case_name]
        TCV.create(ctx, c)
        ctx.set_tsdf_carve(**c["carve"])
        out = []
        for k, (pts, pose, origin, which) in enumerate(c["steps"]):
            (ctx.set_source if which == "source" else ctx.set_target)(K.device_cloud(c, pts))
            info = ctx.tsdf_integrate_cloud(which, pose=pose, sensor_origin=origin)
            out += [("info_%d" % k, shaped("tsdf_cloud_info", info)), ("carve_%d" % k, shaped("tsdf_carve_stats", ctx.tsdf_carve_stats()))]
        return out + volume_fields(ctx, c["dims"] is None)

    def chk(fresh, factory):
        import htsdf_restatement as HR
        c = K.CASES[case_name]
        winfos, wstats, vol = K.reference(case_name)
        for k in range(len(c["steps"])):
            assert field(fresh, "info_%d" % k) == winfos[k] and field(fresh, "carve_%d" % k) == wstats[k], (name, k)
        if isinstance(vol, HR.HVolume):
            rc, rt, rw = vol.sorted_blocks()
            assert np.array_equal(field(fresh, "coords"), rc) and S.same_bits(field(fresh, "tsdf"), rt) and S.same_bits(field(fresh, "weight"), rw), name
        else:
            assert S.same_bits(field(fresh, "tsdf"), vol.tsdf) and S.same_bits(field(fresh, "weight"), vol.weight), name
    add(name, lambda ctx: None, call, chk, "tsdf_carve_restatement: infos, carve stats and the volume bit for bit (tests/test_gpu_tsdf_carve.py)",
        dict(pinned="small", volume=demand, staging="small"))


add_carved_fuse("cloud_fuse_dense_carved", "n3000/dense", "dense large")
add_carved_fuse("cloud_fuse_hashed_carved", "n65/hashed", "hashed small")


def add_plain_fuse(name, table, case_name, demand):
    import tsdf_cloud_cases as CC

    def call(ctx, st):
        steps = CC.TABLES[table][case_name][1]
        opts, dims = steps[0][0], steps[0][1]
        if dims is None:
            ctx.tsdf_create_hashed(block_capacity=max(steps[0][5], 1), **opts)
        else:
            ctx.tsdf_create(dims=dims, **opts)
        out = []
        for k, (_, _, pts, pose, origin, _) in enumerate(steps):
            ctx.set_source(pts)
            out.append(("info_%d" % k, shaped("tsdf_cloud_info", ctx.tsdf_integrate_cloud("source", pose=pose, sensor_origin=origin))))
        return out + volume_fields(ctx, dims is None)

    def chk(fresh, factory):
        import htsdf_restatement as HR
        infos, vol = CC.reference(table, case_name)
        for k, w in enumerate(infos):
            assert field(fresh, "info_%d" % k) == w, (name, k, field(fresh, "info_%d" % k), w)
        if isinstance(vol, HR.HVolume):
            rc, rt, rw = vol.sorted_blocks()
            assert np.array_equal(field(fresh, "coords"), rc) and S.same_bits(field(fresh, "tsdf"), rt) and S.same_bits(field(fresh, "weight"), rw), name
        else:
            assert S.same_bits(field(fresh, "tsdf"), vol.tsdf) and S.same_bits(field(fresh, "weight"), vol.weight), name
    add(name, lambda ctx: None, call, chk, "tsdf_cloud_restatement: every info field and the volume bit for bit (tests/test_gpu_tsdf_cloud.py)",
        dict(pinned="small", volume=demand, staging="small"))


add_plain_fuse("cloud_fuse_dense_plain", "DENSE_SHAPES", "65x5x17", "dense small")
add_plain_fuse("cloud_fuse_hashed_plain", "LANES", "same_256/capacity_1", "hashed large")


def add_colored_fuse(name, case_name, demand):
    import tsdf_cloud_color_cases as KC

    def call(ctx, st):
        import test_gpu_tsdf_cloud_color as TCC
        c = KC.CASES[case_name]
        got = TCC.run(ctx, c)
        out = []
        for k, (info, st_, nc) in enumerate(got):
            out += [("info_%d" % k, shaped("tsdf_cloud_info", info)), ("carve_%d" % k, st_), ("n_colored_%d" % k, nc)]
        return out + volume_fields(ctx, c["dims"] is None, color=True)

    def chk(fresh, factory):
        import htsdf_restatement as HR
        import tsdf_cloud_color_restatement as KR
        c = KC.CASES[case_name]
        want, vol = KC.reference(case_name)
        for k, (info, st_, nc) in enumerate(want):
            assert (field(fresh, "info_%d" % k), field(fresh, "carve_%d" % k), field(fresh, "n_colored_%d" % k)) == (info, st_, nc), (name, k)
        rgb, wc = KR.colors_of(vol)
        assert S.same_bits(field(fresh, "rgb"), rgb) and S.same_bits(field(fresh, "cweight"), wc), name
        if isinstance(vol, HR.HVolume):
            rc, rt, rw = vol.sorted_blocks()
            assert np.array_equal(field(fresh, "coords"), rc) and S.same_bits(field(fresh, "tsdf"), rt) and S.same_bits(field(fresh, "weight"), rw), name
        else:
            assert S.same_bits(field(fresh, "tsdf"), vol.tsdf) and S.same_bits(field(fresh, "weight"), vol.weight), name
    add(name, lambda ctx: None, call, chk, "tsdf_cloud_color_restatement: colours, colour weights, n_colored and the geometry bit for bit (tests/test_gpu_tsdf_cloud_color.py)",
        dict(pinned="small", volume=demand, staging="small"))


add_colored_fuse("cloud_fuse_hashed_colored", "n257/hashed", "hashed colour small")
add_colored_fuse("cloud_fuse_dense_colored", "n257/dense", "dense colour small")


SECOND_POSE = S.pose_of((-0.05, 0.1, 0.0), (-0.08, 0.04, 0.05))
EVICT_ABOUT, EVICT_RADIUS = (0.0, 0.0, 2.0), 1.5


def _fuse_evict_fuse_call(ctx, st):
    """tests/test_gpu_tsdf_cloud.py::test_after_evict_and_insert on ONE volume: a fuse, an evict with hold (the pool compacted under the
    accumulators), the evicted blocks inserted again, a second fuse."""
    import tsdf_cloud_cases as CC
    ctx.tsdf_create_hashed(block_capacity=16, **CC.OPTS)
    ctx.set_source(CC.cloud(2000, seed=41))
    out = [("info_0", shaped("tsdf_cloud_info", ctx.tsdf_integrate_cloud("source", pose=CC.TILTED)))]
    einfo, ec, et, ew = ctx.tsdf_evict_blocks(EVICT_ABOUT, EVICT_RADIUS, hold=True)
    out += [("evict_info", shaped("tsdf_stream_info", einfo)), ("evicted_coords", ec)]
    out.append(("insert_info", shaped("tsdf_stream_info", ctx.tsdf_insert_blocks(ec, et, ew))))
    ctx.set_source(CC.cloud(2000, seed=42))
    out.append(("info_1", shaped("tsdf_cloud_info", ctx.tsdf_integrate_cloud("source", pose=SECOND_POSE))))
    return out + blocks_fields(ctx)


def _fuse_evict_fuse_check(fresh, factory):
    import htsdf_restatement as HR
    import tsdf_cloud_cases as CC
    import tsdf_cloud_restatement as CR
    hv = HR.HVolume(**CC.OPTS)
    assert field(fresh, "info_0") == CR.integrate(hv, CC.cloud(2000, seed=41), CC.TILTED)
    e = field(fresh, "evict_info")
    assert 0 < e["n_evicted"] == e["n_held"] == len(field(fresh, "evicted_coords")) < len(hv.blocks) and e["n_blocks"] == len(hv.blocks) - e["n_evicted"]
    assert field(fresh, "insert_info")["n_inserted"] == e["n_evicted"] and field(fresh, "insert_info")["n_blocks"] == len(hv.blocks)
    assert field(fresh, "info_1") == CR.integrate(hv, CC.cloud(2000, seed=42), SECOND_POSE)      # (evict + insert of the same blocks leaves the restatement's volume as it was)
    rc, rt, rw = hv.sorted_blocks()
    assert np.array_equal(field(fresh, "coords"), rc) and S.same_bits(field(fresh, "tsdf"), rt) and S.same_bits(field(fresh, "weight"), rw) and rw.max() == 2


add("cloud_fuse_evict_insert_fuse", lambda ctx: None, _fuse_evict_fuse_call, _fuse_evict_fuse_check,
    "tsdf_cloud_restatement on a volume that never lost a block: both infos and the blocks bit for bit (tests/test_gpu_tsdf_cloud.py::test_after_evict_and_insert)",
    dict(pinned="small", volume="hashed large", staging="small"))


# ---------------------------------------------------------------------------------------------------- scan-to-TSDF alignment
def add_align_cloud(name, blocks, color):
    """icp_tsdf_align_cloud (color: with the photometric term) of sdf_cloud_cases' fold cloud, `blocks` blocks of points, 3 traced steps."""
    import sdf_cloud_cases as K
    opt = dict(n_iterations=3, stop_rotation=0.0, stop_translation=0.0)

    def n_points():
        import sdf_cloud_color_cases as KC
        return blocks * (KC.PER_BLOCK if color else K.PER_BLOCK)      # the coloured kernels have a constant of their own

    def cloud():
        return K.fold_cloud()[:n_points()]

    def colors():
        import sdf_cloud_color_cases as KC
        return KC.fold_colors()[:n_points()]

    def setup(ctx):
        if color:
            import sdf_cloud_color_cases as KC
            import test_gpu_sdf_cloud_color as TSC
            TSC.upload(ctx, KC.colored_model(False))
            ctx.set_source(cloud(), None, colors())
        else:
            import test_gpu_sdf_cloud as TS
            TS.upload(ctx, K.model(False))
            ctx.set_source(cloud())

    def call(ctx, st):
        import sdf_cloud_color_cases as KC
        kw = dict(color_weight=KC.WEIGHT) if color else {}
        pose, rec, rc, trace = ctx.tsdf_align_cloud("source", K.START, trace=True, **opt, **kw)
        kind = "sdf_color" if color else "sdf"
        return [("pose", pose), ("status", rc), ("record", shaped(kind + "_frame", rec)), ("trace", shaped_list(kind + "_iter", trace))]

    def chk(fresh, factory):
        if color:
            import sdf_cloud_color_cases as KC
            import test_gpu_sdf_cloud_color as TSC
            TSC.follow(name, KC.colored_model(False), cloud(), colors(), K.START, field(fresh, "record"), field(fresh, "status"), field(fresh, "trace"), **opt)
        else:
            import test_gpu_sdf_cloud as TS
            TS.follow(name, K.model(False), cloud(), K.START, field(fresh, "record"), field(fresh, "status"), field(fresh, "trace"), **opt)
        assert S.same_bits(field(fresh, "pose"), field(fresh, "record")["pose"])
    add(name, setup, call, chk, "sdf_cloud_restatement's step from the device's previous pose, support.POSE_TOL; n_valid exactly; the cost within its summation bound "
        "(tests/test_gpu_sdf_cloud.py::follow, tests/test_gpu_sdf_cloud_color.py::follow)",
        dict(pinned="small", sdf=("29+3" if color else "28+2") + (" large" if blocks > 1 else " small"), staging="large" if blocks > 1 else "small"), iters=3)


add_align_cloud("align_cloud_1", 1, False)
add_align_cloud("align_cloud_65", 65, False)
add_align_cloud("align_cloud_color_1", 1, True)
add_align_cloud("align_cloud_color_65", 65, True)


# ---------------------------------------------------------------------------------------------------- mesh clustering
def cluster_fields(got):
    v, n, c, t, info = got
    return [("vertices", v), ("normals", n), ("colors", c), ("triangles", t), ("info", shaped("mesh_cluster_info", info))]


def add_cluster(name, kind, key, normals, colors, demand):
    def call(ctx, st):
        import mesh_cluster_cases as K
        import test_gpu_mesh_cluster as TMC
        case, _ = TMC.reference(kind, key, normals, colors)
        a, kw = K.args(case, normals, colors)
        return cluster_fields(ctx.mesh_cluster(*a, **kw))

    def chk(fresh, factory):
        import test_gpu_mesh_cluster as TMC
        _, want = TMC.reference(kind, key, normals, colors)
        assert_equal(fresh, cluster_fields(want), name + " against mesh_cluster_restatement")
    add(name, lambda ctx: None, call, chk, "mesh_cluster_restatement, bit for bit (tests/test_gpu_mesh_cluster.py::reference)", dict(pinned="small", mc=demand))


BIG_MESH = 1024 * 256 + 1
add_cluster("mesh_cluster_262145", "random_mesh", (BIG_MESH,), True, True, "large, normals and colours")
add_cluster("mesh_cluster_63", "random_mesh", (63,), False, False, "small, neither")
add_cluster("mesh_cluster_63_attributes", "random_mesh", (63,), True, True, "small, normals and colours")
add_cluster("mesh_cluster_no_triangles", "crafted", "vertices without triangles", True, True, "T = 0")


def add_clustered_volume_mesh(name, hashed):
    def setup(ctx):
        import test_gpu_mesh_cluster as TMC
        if hashed:
            import htsdf_mesh_cases as MC
            ctx.tsdf_create_hashed(**MC.OPTS)
            ctx.tsdf_upload_blocks(*MC.case_b())
            return 2 * MC.OPTS["voxel_size"], MC.OPTS["origin"]
        import tsdf_mesh_restatement as TMR
        S.upload(ctx, TMR.analytic_volume(TMR.sphere(TMC.CENTRE, 0.6)))
        return 0.2, (-0.95, -0.95, -0.95)

    def call(ctx, st):
        mesh = ctx.tsdf_mesh_hashed if hashed else ctx.tsdf_mesh
        got = mesh(cluster=st[0])
        return mesh_fields(got) + [("info", shaped("mesh_cluster_info", ctx.mesh_cluster_info()))]

    def chk(fresh, factory):
        import mesh_cluster_restatement as R
        ctx, st = prepared(name, factory)
        plain = (ctx.tsdf_mesh_hashed if hashed else ctx.tsdf_mesh)()          # the unclustered mesh: bit for bit its restatement's in tests/test_gpu_(h)tsdf_mesh.py
        v, n, c, t, info = R.cluster(plain[0], plain[2], st[0], normals=plain[1], colors=None, origin=st[1])
        assert 0 < len(t) < len(plain[2])
        assert_equal(fresh, mesh_fields((v, n, t)) + [("info", shaped("mesh_cluster_info", info))], name + " against mesh_cluster_restatement of the unclustered mesh")
    add(name, setup, call, chk, "mesh_cluster_restatement of the unclustered call's mesh, bit for bit (tests/test_gpu_mesh_cluster.py::test_clustered_volume_mesh_equals_cluster_of_the_mesh)",
        dict(pinned="small", tm="clustered " + ("hashed" if hashed else "dense") + " large", mc="staged " + ("hashed" if hashed else "dense")))


add_clustered_volume_mesh("tsdf_mesh_clustered_dense", False)
add_clustered_volume_mesh("tsdf_mesh_clustered_hashed", True)

MC_NPASS = 8


def _timed_cluster_setup(ctx):
    import htsdf_mesh_cases as MC
    ctx.tsdf_create_hashed(**MC.OPTS)
    ctx.tsdf_upload_blocks(*MC.case_b())


def _timed_cluster_call(ctx, st):
    """icp_debug_mesh_cluster_time (10 events): the pass times are history, the counts are compared."""
    import htsdf_mesh_cases as MC
    from icp_amd import binding as B
    ms = (C.c_float * MC_NPASS)(); info = B.IcpMeshClusterInfo()
    fn = ctx.lib.icp_debug_mesh_cluster_time
    fn.argtypes = [C.c_void_p, C.c_float, C.POINTER(B.IcpMeshClusterOptions), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(B.IcpMeshClusterInfo)]
    fn.restype = C.c_int32
    ctx._ck(fn(ctx.h, 0.0, C.byref(B.mesh_cluster_options(2 * MC.OPTS["voxel_size"], MC.OPTS["origin"])), 0, 1, ms, C.byref(info)))
    return [("info", shaped("mesh_cluster_info", B._record(info)))]


def _timed_cluster_check(fresh, factory):
    import mesh_cluster_restatement as R
    import htsdf_mesh_cases as MC
    ctx, _ = prepared("mesh_cluster_timed", factory)
    plain = ctx.tsdf_mesh_hashed()
    info = R.cluster(plain[0], plain[2], 2 * MC.OPTS["voxel_size"], normals=plain[1], colors=None, origin=MC.OPTS["origin"])[4]
    assert field(fresh, "info") == shaped("mesh_cluster_info", info)


add("mesh_cluster_timed", _timed_cluster_setup, _timed_cluster_call, _timed_cluster_check, "mesh_cluster_restatement's counts of the unclustered mesh, exactly",
    dict(pinned="small", tm="clustered hashed large", mc="staged hashed", events="large"))


# ---------------------------------------------------------------------------------------------------- voxel maps
VMAP_VS = 0.25


def map_entries(ctx, hashed):
    if hashed:
        info, coords, counts, sums, cells = ctx.voxel_map_hashed()
        return [("map_info", shaped("voxel_hash_map_info", info)), ("coords", coords), ("counts", counts), ("sums", sums), ("cells", cells)]
    info, counts, sums, cells = ctx.voxel_map()
    return [("map_info", info), ("counts", counts), ("sums", sums), ("cells", cells)]


def add_vmap(name, hashed, n_points, with_system):
    """The crafted cloud of tests/test_gpu_hmap.py: its first n_points at POSE_A then POSE_B (a hashed map grows from 256 slots), a prune
    about the median, a compaction (hashed), and the system of the cloud at the identity."""
    def setup(ctx):
        import test_gpu_hmap as TH
        ctx.set_gicp_options(TH.EPS, 0)
        if hashed:
            ctx.voxel_map_create_hashed(VMAP_VS, 256)
        else:
            ctx.voxel_map_create(VMAP_VS, *TH.COVER)
        pts, nrm = TH.crafted()
        return pts[:n_points], nrm[:n_points]

    def centre(pts):
        return np.median(pts[np.isfinite(pts).all(1)], axis=0).astype(f32)

    def call(ctx, st):
        import test_gpu_hmap as TH
        pts, nrm = st
        ctx.set_source(pts, nrm, None)
        out = []
        for k, pose in enumerate((S.pose_of(*TH.POSE_A), S.pose_of(*TH.POSE_B))):
            out.append(("insert_%d" % k, shaped("voxel_map_insert_info", ctx.voxel_map_insert(1, pose))))
        out.append(("prune", shaped("voxel_map_prune_info", ctx.voxel_map_prune(centre(pts), 0.9))))
        if hashed:
            ctx.voxel_map_compact()
        out += map_entries(ctx, hashed)
        if with_system:
            sums, counts = ctx.voxel_map_system(S.pose_of(*TH.POSE_A), voxel_size=VMAP_VS)
            out += [("system_sums", sums), ("system_counts", tuple(counts))]
        return out

    def chk(fresh, factory):
        import hmap_restatement as HR
        import test_gpu_hmap as TH
        import vmap_prune_restatement as PR
        import vmap_restatement as MR
        pts, nrm = TH.crafted()
        pts, nrm = pts[:n_points], nrm[:n_points]
        m = HR.create(VMAP_VS, 256) if hashed else MR.create(VMAP_VS, *TH.COVER)
        for k, pose in enumerate((S.pose_of(*TH.POSE_A), S.pose_of(*TH.POSE_B))):
            assert field(fresh, "insert_%d" % k) == PR.insert(m, pts, nrm, pose), (name, k)
        want = PR.prune(m, centre(pts), 0.9)
        assert field(fresh, "prune") == shaped("voxel_map_prune_info", want), (name, field(fresh, "prune"), want)
        e = PR.entries(m)
        if hashed:
            got = tuple(field(fresh, k) for k in ("coords", "counts", "sums", "cells"))
        else:
            info = field(fresh, "map_info")
            got = HR.dense_entries(dict(lo=info["lo"], dims=info["dims"], counts=field(fresh, "counts"), sums=field(fresh, "sums"), cells=field(fresh, "cells")))
        TH.same_entries(got, e, name)
        if with_system:                                     # tests/test_gpu_hmap.py::test_system_against_the_dense_map: counts exactly, every sum within the contract's bound
            rcounts, rsums, rabs = HR.system(m, pts, nrm, S.pose_of(*TH.POSE_A), TH.EPS, 1)
            bound = rcounts[1] * 2.0 ** -52 * rabs
            assert field(fresh, "system_counts") == tuple(rcounts) and rcounts[1] > 0, (name, field(fresh, "system_counts"), rcounts)
            assert (np.abs(field(fresh, "system_sums") - rsums) <= bound).all(), name
    add(name, setup, call, chk, "vmap_prune_restatement (over hmap_restatement / vmap_restatement): every info field and every entry bit for bit; the system's counts exactly, its "
        "sums within n_valid 2^-52 sum |term| of hmap_restatement's (tests/test_gpu_hmap.py, tests/test_gpu_vmap_prune.py)",
        dict(dict(pinned="large", staging="large" if n_points > 1000 else "small"), **(dict(sdf="28+2 small") if with_system else {})), pin=PIN_MAP)


add_vmap("hmap_4099", True, 4099, True)
add_vmap("hmap_1", True, 1, False)
add_vmap("vmap_4099", False, 4099, False)
add_vmap("vmap_1", False, 1, False)


def _vmap_track_setup(ctx):
    import test_gpu_vmap as TV
    import vmap_outcome_fixture as MF
    ctx.set_gicp_options(TV.EPS, 0)
    ctx.voxel_map_create(MF.VOXEL, *MF.extent())
    return TV.small_scans()[:3], MF.truth(0).astype(f32)


def _vmap_track_fields(ctx, pose, recs, rc):
    return [("pose", pose), ("status", rc), ("records", shaped_list("sdf_frame", recs))] + map_entries(ctx, False)


def _vmap_track_check(fresh, factory):
    import test_gpu_vmap as TV
    ctx, (scans, start) = prepared("vmap_track_two_scans", factory)
    pose, recs, rc = ctx.track_scans_vmap(scans, start, **TV.TRACK)
    assert rc == 0 and len(recs) == 2
    TV.check_tracked(ctx, scans, start, [start] + [r["pose"] for r in recs], recs, [0] * 2)
    assert_equal(fresh, _vmap_track_fields(ctx, pose, recs, rc), "two tracked scans against the checked run")


def _vmap_track_call(ctx, st):
    import test_gpu_vmap as TV
    return _vmap_track_fields(ctx, *ctx.track_scans_vmap(st[0], st[1], **TV.TRACK))


add("vmap_track_two_scans", _vmap_track_setup, _vmap_track_call, _vmap_track_check,
    "vmap_restatement's align from the device's previous pose: counts exactly, the first cost within its bound, the pose 1e-5 per step, the map bit for bit "
    "(tests/test_gpu_vmap.py::check_tracked)", dict(pinned="small", sdf="28+2 small", staging="large"), iters=6)


# ---------------------------------------------------------------------------------------------------- the fixed order
# One context, these steps in this order; every step must give the fresh context's bits.  "x -> y" in a comment: that adjacent pair is the
# one that covers the resource.  REQUIRED_PAIRS (below) is what tests/test_context_reuse_host.py looks for.
FIXED_ORDER = [
    # pinned, first regrow: run_m1_65 (the block's first 4096 bytes) -> hmap_4099 (4096 + 104: regrown, the words at +2016 and +2032) -> sdf_6 (+2048)
    "run_m1_65", "hmap_4099", "sdf_6",
    # select / staging: depth_mesh_640x480 (1196 blocks) -> depth_clouds_33x17 (compaction of one block) -> run_m1_random (sel_blocks)
    "depth_mesh_640x480", "depth_clouds_33x17", "run_m1_random",
    # tm: dense 37 x 21 x 29 -> hashed one block -> clustered dense -> mesh_cluster_63 -> hashed case_b
    "tsdf_dense_37x21x29", "htsdf_mesh_one_block", "tsdf_mesh_clustered_dense", "mesh_cluster_63", "htsdf_mesh_B",
    # mc: normals and colours at 262 145 -> neither at 63 -> T = 0 (the triangle table of the large call behind both)
    "mesh_cluster_262145", "mesh_cluster_63", "mesh_cluster_no_triangles",
    # loop, and pinned's second regrow: run_m1_long (40 iterations: 5120 bytes) -> a run of 5; every loop recipe stands directly behind the
    # one with the largest iteration count (ring, totals, stats and the page-locked records of 40 iterations behind every run of 5); the
    # other loop recipes follow at the end of the order
    "run_m1_long", "run_m1", "run_m1_long", "run_m0", "run_m1_long", "run_m2", "run_m1_long", "run_lm",
    # sdf: 1200 blocks, 28 + 2 -> 257 blocks, 29 + 3 -> VGICP 513 -> scan-to-TSDF, one block -> 6 blocks
    "sdf_1200", "sdf_color_257", "vgicp_513", "align_cloud_1", "sdf_6",
    # volume: dense carved -> (tsdf_create_hashed inside) hashed coloured -> fuse, evict with hold, insert, fuse again on one volume -> the
    # lattice's evict and insert -> a fuse that grows its pool from one block; tc_acc / tcc_acc are laid out for the box, then for pools of
    # other sizes, and have to be all zero at every start
    "cloud_fuse_dense_carved", "cloud_fuse_hashed_colored", "cloud_fuse_evict_insert_fuse", "htsdf_evict_insert", "cloud_fuse_hashed_plain",
    # pinned, third regrow, and its offsets 0, +256.., +2016, +2032, +2048 in every neighbouring order: multistart_256 (157 KiB: regrown) ->
    # run_m1_65 (lay_out from +256) -> measures_65537 (+2048 count slot's neighbours) -> hmap_4099 (insert at +2032, prune at +2016) -> sdf_6 (+2048)
    "multistart_256", "run_m1_65", "measures_65537", "hmap_4099", "sdf_6",
    # events: 10 events of the timed clustering -> a run whose separate launches take events by position, stage timing 1 -> the hashed mesh's 8
    "mesh_cluster_timed", "run_m1_timed", "htsdf_mesh_B",
    # the other layouts and sizes, each behind a different family
    "cloud_fuse_hashed_carved", "cloud_fuse_dense_plain", "cloud_fuse_dense_colored", "align_cloud_color_65", "align_cloud_65", "align_cloud_color_1", "vgicp_6",
    "align_depth_257", "hmap_1", "vmap_4099", "vmap_1", "tsdf_mesh_clustered_hashed", "tsdf_dense_9x9x9", "tsdf_dense_9x9x9_color", "htsdf_integrate_growth",
    "htsdf_raycast_B", "htsdf_raycast_color_B", "tsdf_dense_color_integrate", "tsdf_dense_color_raycast", "vmap_track_two_scans", "depth_clouds_320x240", "depth_clouds_320x240_filtered", "depth_clouds_33x17_filtered", "depth_mesh_33x17", "backproject_160x120",
    "normals_1359", "normals_65", "measures_1", "mesh_cluster_63_attributes", "global_k5",
    # loop, the rest: each of the other loop recipes directly behind the 40-iteration run -- the brute-force and the multires run, both
    # selections, the 65-point run, the event-bracketed run, GICP, colored, robust, reciprocal, both multi-starts (the second regrows
    # nothing: the block holds 157 KiB since step 32) and the tracked frames
    "run_m1_long", "run_m1_brute", "run_m1_long", "run_m1_multires", "run_m1_long", "run_m1_random", "run_m1_long", "run_m1_nss",
    "run_m1_long", "run_m1_65", "run_m1_long", "run_m1_timed", "run_m1_long", "run_gicp", "run_m1_long", "run_colored",
    "run_m1_long", "run_robust", "run_m1_long", "run_reciprocal", "run_m1_long", "multistart_256", "run_m1_long", "multistart_1",
    "run_m1_long", "track_depth_frames_64x48",
]
REQUIRED_PAIRS = {
    "pinned": [("multistart_256", "run_m1_65"), ("run_m1_65", "measures_65537"), ("measures_65537", "hmap_4099"), ("hmap_4099", "sdf_6"), ("run_m1_65", "hmap_4099")],
    "select": [("depth_mesh_640x480", "depth_clouds_33x17"), ("depth_clouds_33x17", "run_m1_random")],
    "tm": [("tsdf_dense_37x21x29", "htsdf_mesh_one_block"), ("htsdf_mesh_one_block", "tsdf_mesh_clustered_dense"), ("tsdf_mesh_clustered_dense", "mesh_cluster_63"),
           ("mesh_cluster_63", "htsdf_mesh_B")],
    "mc": [("mesh_cluster_262145", "mesh_cluster_63"), ("mesh_cluster_63", "mesh_cluster_no_triangles")],
    "sdf": [("sdf_1200", "sdf_color_257"), ("sdf_color_257", "vgicp_513"), ("vgicp_513", "align_cloud_1"), ("align_cloud_1", "sdf_6")],
    # volume: icp_tsdf_create, icp_tsdf_create_hashed and icp_tsdf_release drop tc_acc and tcc_acc, and every recipe starts behind neutral's
    # release, so no accumulator outlives a recipe: between two recipes these pairs exercise te_work and the outboxes (and the pool's and
    # the box's allocations coming and going), nothing else that is shared.  What a stale accumulator does is seen INSIDE the recipes that
    # fuse twice into one volume, against their restatement.
    "volume": [("cloud_fuse_dense_carved", "cloud_fuse_hashed_colored"), ("cloud_fuse_hashed_colored", "cloud_fuse_evict_insert_fuse"),
               ("cloud_fuse_evict_insert_fuse", "htsdf_evict_insert"), ("htsdf_evict_insert", "cloud_fuse_hashed_plain")],
    "events": [("mesh_cluster_timed", "run_m1_timed"), ("run_m1_timed", "htsdf_mesh_B")],
    "loop": [("run_m1_long", n) for n in LOOP_RECIPES],
}
