"""What stopping on a converged pose (icp_set_convergence_options) costs and saves, on the bench pair synth.eth_like_pair(0): 50
iterations, k-NN (LBVH), max distance 10, from the identity, stage timing 0.  Times are the run's device time (icp_get_timing total_ms:
events around the whole run, drained launches included).

Every library under test (the product, and any `--lib name=path`: the parent commit's build, the chunk-size variants of
tools/dev_build_variant.py <name> ICP_CONVERGE_CHUNK=<K>) is measured in child processes of its own, `--rounds` times, the libraries
alternating within a round; a child warms every configuration up once and then repeats them `--reps` times, interleaved.  Reported per
library and configuration: the median over all repeats of all rounds, the 10th and 90th percentile and the extremes.
  p2plane_off          point-to-plane, the option off (the merged loop)
  p2plane_on           the option on, eps (1e-6, 1e-6): where it stops, and the whole run with its drained launches
  p2plane_off_to_stop  the option off with n_iterations = that stop: the time up to the stop
                       -> drained_launch_us = (p2plane_on - p2plane_off_to_stop) / launches left
  p2plane_on_unmet     the option on with bounds nothing meets: all 50 iterations with the criterion on the reducer -> matcher path
                       -> criterion_us_per_iteration = (p2plane_on_unmet - p2plane_off) / 50
  gicp_off / gicp_on   GICP (the separate form, chunked enqueue), eps (1e-6, 1e-6)
A library without the entry points (the parent) is measured with the option off only.
usage: python tools/time_converge.py [--rounds 3] [--reps 7] [--lib name=path ...] [--json profiles/converge.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "icp-variants_amd", "python"))
import numpy as np

EPS = dict(rotation=1e-6, translation=1e-6)
UNMET = dict(rotation=1e-30, translation=1e-30)
N_ITER = 50


def child(pair_path, reps):
    from icp_amd import binding
    d = np.load(pair_path)
    has = hasattr(binding.load_library(), "icp_set_convergence_options")
    eye = binding.pose_to_c(np.eye(4))

    def context(metric):
        c = binding.Context(0)
        c.params.metric = metric; c.params.knn_backend = 1; c.params.max_distance = 10.0; c.params.n_iterations = N_ITER
        c.push_params(); c.set_stage_timing(0)
        c.set_target(d["tgt_pts"], d["tgt_nrm"]); c.set_source(d["src_pts"], d["src_nrm"])
        return c

    def run(c, n_iterations, opts):
        if c.params.n_iterations != n_iterations:
            c.params.n_iterations = n_iterations; c.push_params()
        if has:
            c.set_convergence_options(**opts) if opts else c.set_convergence_options(None)
        n = c.run_raw(eye.copy())
        return c.timing()["total_ms"], n

    out = {}
    for metric, name in ((1, "p2plane"), (3, "gicp")):
        c = context(metric)
        configs = [(name + "_off", N_ITER, None)]
        if has:
            _, n_stop = run(c, N_ITER, EPS)
            configs.append((name + "_on", N_ITER, EPS))
            if metric == 1:
                configs += [(name + "_off_to_stop", n_stop, None), (name + "_on_unmet", N_ITER, UNMET)]
            out[name + "_stop"] = n_stop
        for label, n_it, opts in configs:                      # warm-up: every shape the timed window uses
            run(c, n_it, opts)
        times = {label: [] for label, _, _ in configs}
        for _ in range(reps):
            for label, n_it, opts in configs:
                times[label].append(run(c, n_it, opts)[0])
        out.update(times)
        c.close()
    print("RESULT " + json.dumps(out), flush=True)


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)), min_ms=float(v[0]), max_ms=float(v[-1]), n=int(len(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", action="append", default=[], help="name=path of another build of the library to measure beside the product")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "converge.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    from icp_amd import synth
    libs = [("product", None)] + [tuple(s.split("=", 1)) for s in a.lib]
    p = synth.eth_like_pair(0)
    raw = {name: {} for name, _ in libs}
    with tempfile.TemporaryDirectory() as tmp:
        pair = os.path.join(tmp, "pair.npz")
        np.savez(pair, **{k: p[k] for k in ("src_pts", "src_nrm", "tgt_pts", "tgt_nrm")})
        for _ in range(a.rounds):
            for name, path in libs:
                env = dict(os.environ)
                env.pop("ICP_HIP_LIB", None)
                if path:
                    env["ICP_HIP_LIB"] = os.path.abspath(path)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pair, "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return 1
                res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                for k, v in res.items():
                    if isinstance(v, list):
                        raw[name].setdefault(k, []).extend(v)
                    else:
                        assert raw[name].setdefault(k, v) == v, (name, k, v)      # the stop iteration never varies
    out = dict(pair="synth.eth_like_pair(0)", n_src=int(len(p["src_pts"])), n_tgt=int(len(p["tgt_pts"])), iterations=N_ITER, eps=EPS, rounds=a.rounds, reps=a.reps, libs={})
    for name, _ in libs:
        row = {k: (spread(v) if isinstance(v, list) else v) for k, v in raw[name].items()}
        if "p2plane_on" in row:
            stop, left = row["p2plane_stop"], N_ITER - row["p2plane_stop"]
            row["drained_launch_us"] = 1e3 * (row["p2plane_on"]["median_ms"] - row["p2plane_off_to_stop"]["median_ms"]) / left if left > 0 else None
            row["criterion_us_per_iteration"] = 1e3 * (row["p2plane_on_unmet"]["median_ms"] - row["p2plane_off"]["median_ms"]) / N_ITER
            row["p2plane_on_over_off"] = row["p2plane_on"]["median_ms"] / row["p2plane_off"]["median_ms"]
            row["gicp_on_over_off"] = row["gicp_on"]["median_ms"] / row["gicp_off"]["median_ms"]
        out["libs"][name] = row
        print(json.dumps({name: row}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
