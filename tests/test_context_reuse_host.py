"""The table of tests/context_reuse_cases.py, checked without a device: every shared resource has recipes of different demand, the fixed
order contains the adjacent pairs it is there for, HISTORY_FIELDS is exactly what the recipes' result shaping leaves out, and the demand
on the page-locked block, from the formulas of host_loop.hpp and host_multi.hpp, really makes the block grow in the middle of the order."""
import os
import re

import numpy as np

import context_reuse_cases as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "icp-variants_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def test_every_resource_has_recipes_of_different_demand():
    doc = R.__doc__
    for res in R.RESOURCES:
        assert re.search(r"^  %s\s" % res, doc, re.M), "the module docstring does not list %s" % res
        users = {n: r.uses[res] for n, r in R.RECIPES.items() if res in r.uses}
        assert len(users) >= 2, (res, users)
        assert len(set(users.values())) >= 2, "%s: every recipe puts the same demand on it: %s" % (res, users)
    used = set().union(*[set(r.uses) for r in R.RECIPES.values()])
    assert used == set(R.RESOURCES), used ^ set(R.RESOURCES)
    # a resource with more than one layout has a recipe per layout
    layouts = dict(tm=("dense", "hashed", "clustered"), sdf=("28+2", "29+3"), volume=("dense", "hashed", "colour"), mc=("normals and colours", "neither", "T = 0", "staged"))
    for res, names in layouts.items():
        have = " | ".join(str(r.uses.get(res, "")) for r in R.RECIPES.values())
        for layout in names:
            assert layout in have, (res, layout)


def test_every_recipe_names_its_reference_and_runs_in_the_fixed_order():
    for name, r in R.RECIPES.items():
        assert len(r.reference) > 20 and callable(r.check), name
        assert name in R.FIXED_ORDER, name
    assert set(R.FIXED_ORDER) == set(R.RECIPES)


def test_fixed_order_contains_the_required_pairs():
    order = R.FIXED_ORDER
    pairs = set(zip(order, order[1:]))
    for res, want in R.REQUIRED_PAIRS.items():
        for p in want:
            assert p in pairs, "%s: %s -> %s is not adjacent in the fixed order" % ((res,) + p)
    # every loop recipe stands directly behind the one with the largest iteration count
    longest = max(R.RECIPES.values(), key=lambda r: r.iters)
    assert longest.name == "run_m1_long" and longest.iters == R.LONG_ITERS
    loops = [n for n, r in R.RECIPES.items() if r.per_form and n != longest.name]
    assert sorted(loops) == sorted(R.LOOP_RECIPES)
    for n in loops:
        assert (longest.name, n) in pairs, n
    # on every resource the order has a large use followed by a small one and a small one followed by a large one (where the demands are
    # sizes), and two different layouts next to each other
    for res in R.RESOURCES:
        seq = [R.RECIPES[n].uses[res] for n in order if res in R.RECIPES[n].uses]
        steps = set(zip(seq, seq[1:]))
        assert any(a != b for a, b in steps), res
        sizes = [("large" in str(a), "large" in str(b)) for a, b in steps if ("large" in str(a)) != ("large" in str(b)) and ("small" in str(a) + str(b))]
        if any("small" in str(u) for u in seq) and any("large" in str(u) for u in seq):
            assert (True, False) in sizes and (False, True) in sizes, (res, sorted(steps, key=str))


def test_history_fields_are_exactly_what_is_left_out():
    """Every key of every kind of info record is either compared (it survives `shaped`) or listed in HISTORY_FIELDS; nothing is listed that
    the record does not have; padding is the only other thing dropped."""
    from icp_amd import binding as B
    for kind, listed in R.HISTORY_FIELDS.items():
        struct = R.info_struct(kind)
        keys = [k for k, _ in struct._fields_]
        recorded = B._record(struct())                       # a recorded dict of that kind, as the binding hands it to a recipe
        assert list(recorded) == keys
        kept = R.shaped(kind, recorded)
        assert set(listed) <= set(keys), (kind, set(listed) - set(keys))
        assert set(kept) | set(listed) | set(R.RESERVED) >= set(keys), kind
        assert not (set(kept) & set(listed)), kind
        assert set(keys) - set(kept) - set(listed) <= set(R.RESERVED), (kind, set(keys) - set(kept) - set(listed))
    # the kinds a recipe shapes are the kinds of the table: every shaped(...) call in the module names a listed kind
    text = open(R.__file__.replace(".pyc", ".py")).read()
    named = set(re.findall(r"shaped(?:_list)?\(\"(\w+)\"", text)) | {"sdf_frame", "sdf_iter", "sdf_color_frame", "sdf_color_iter"}
    assert named <= set(R.HISTORY_FIELDS), named - set(R.HISTORY_FIELDS)
    # what the header calls history: growth, rehash and compaction counts, the carve total
    assert R.HISTORY_FIELDS["tsdf_hashed_info"] == ("n_grown",) and R.HISTORY_FIELDS["tsdf_stream_info"] == ("n_grown", "n_moved") and R.HISTORY_FIELDS["voxel_map_prune_info"] == ("n_compacted",)
    assert R.HISTORY_FIELDS["tsdf_carve_stats"] == ("n_carved_total",)


def test_record_sizes_are_the_librarys():
    """The sizes the demand formulas use are the sizes of the records in the sources."""
    from icp_amd import binding as B
    import ctypes as C
    assert C.sizeof(B.IcpIterStats) == R.SIZEOF["iter_stats"] and C.sizeof(B.IcpStartResult) == R.SIZEOF["start_result"]
    assert C.sizeof(B.IcpLmSummary) == R.SIZEOF["lm_summary"] and C.sizeof(B.IcpSdfFrame) == R.SIZEOF["sdf_frame"]
    assert C.sizeof(B.IcpConvergenceStep) == R.SIZEOF["convergence_step"]
    loop = source("host_loop.hpp")
    assert "static_assert(sizeof(PoseState) == 128" in loop and "sizeof(RunTail) == 512" in loop
    # lay_out, as restated in pin_loop
    assert "pin_stats = 256" in loop and "pin_tail = pin_stats + pad((size_t)iters * sizeof(icp_iter_stats))" in loop
    assert "pin_stamps = pin_tail + sizeof(RunTail) + trace_pad" in loop and "pin_lm = pin_stamps + pad(RunStamps::bytes(iters))" in loop
    assert "return (size_t)2 * (iters + 1) * 8" in loop
    multi = source("host_multi.hpp")
    assert "pin_rec = (Kz * sizeof(PoseState) + 255) & ~(size_t)255" in multi and "ensure_pinned(c, pin_res + Kz * sizeof(icp_start_result))" in multi
    ctx = source("host_ctx.hpp")
    assert "return ensure_pin(c, c->pinned, bytes, 4096, 0)" in ctx and "c->pinned.as<char>() + 2048" in ctx
    assert "ensure_pinned(c, 4096 + sizeof(icp_sdf_frame))" in source("host_hmap.hpp") and "c->pinned.as<char>() + 2032" in source("host_hmap.hpp")
    assert "ensure_pinned(c, 4096 + sizeof(icp_sdf_frame))" in source("host_vmap_prune.hpp") and "c->pinned.as<char>() + 2016" in source("host_vmap_prune.hpp")


def test_the_page_locked_block_is_regrown_in_the_middle_of_the_order():
    """The block starts at 4096 bytes and only grows (ensure_pin): a step whose demand exceeds what the block holds frees it and moves it.
    Along the fixed order the demand rises above 4096 and falls below it again more than once, and the block is regrown at steps that
    have steps of every pinned offset before and behind them."""
    assert R.pin_loop(R.ITERS) < R.PIN_MIN < R.pin_loop(R.LONG_ITERS) < R.PIN_MAP + 4096 and R.pin_multi(256, R.ITERS) > 100000
    assert R.pin_loop(5) == 256 + 512 + 512 + 256 and R.pin_loop(5, lm=True) == 1536 + 5 * 104 and R.pin_loop(5, cvg=True) == 1536 + 256
    assert R.pin_multi(1, 5) == 256 + 512 + 80
    demand = [R.RECIPES[n].pin for n in R.FIXED_ORDER]
    cap, regrown = R.PIN_MIN, []
    for i, d in enumerate(demand):
        if d > cap:
            regrown.append(i)
            cap = d
    above = [d > R.PIN_MIN for d in demand]
    crossings = sum(1 for a, b in zip(above, above[1:]) if a != b)
    print("demand on the page-locked block along the fixed order: regrown at steps %s (%s); %d crossings of 4096" % (regrown, [R.FIXED_ORDER[i] for i in regrown], crossings))
    assert [R.FIXED_ORDER[i] for i in regrown] == ["hmap_4099", "run_m1_long", "multistart_256"]
    assert regrown[0] > 0 and regrown[1] > 10 and regrown[2] > regrown[1] + 10 and regrown[-1] < len(demand) - 30
    assert crossings >= 6
    # behind the last regrow every kind of user of the block comes again: the loop's lay_out, the count slot, the map's words, the SDF state
    rest = R.FIXED_ORDER[regrown[-1] + 1:]
    for name in ("run_m1_65", "measures_65537", "hmap_4099", "sdf_6", "mesh_cluster_63_attributes", "run_m1_long"):
        assert name in rest, name


def test_comparison_is_bit_for_bit():
    a = [("x", np.array([0.0, 1.0], np.float32)), ("info", dict(n=1, cost=0.5)), ("recs", [dict(pose=np.eye(4, dtype=np.float32))])]
    b = [("x", np.array([-0.0, 1.0], np.float32)), ("info", dict(n=1, cost=0.5)), ("recs", [dict(pose=np.eye(4, dtype=np.float32))])]
    assert R.first_difference(a, a) is None and R.first_difference(a, b) == "x"
    b[0] = a[0]; b[1] = ("info", dict(n=1, cost=np.nextafter(0.5, 1)))
    assert R.first_difference(a, b) == "info[cost]"
    b[1] = a[1]; q = np.eye(4, dtype=np.float32); q[0, 3] = np.nan
    b[2] = ("recs", [dict(pose=q)])
    assert R.first_difference(a, b) == "recs[0][pose]"
    nan = [("x", np.array([np.nan], np.float32))]
    assert R.first_difference(nan, nan) is None
    assert R.first_difference(a, a[:2]) is not None


def test_seeded_orders_are_permutations_of_the_table():
    names = list(R.RECIPES)
    for seed in (0, 1, 2):
        order = [names[i] for i in np.random.default_rng(seed).permutation(len(names))]
        assert sorted(order) == sorted(names) and order != names
