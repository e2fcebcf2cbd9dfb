"""Global registration: initial poses for ICP from the two clouds alone (Context.register_global), refined by multi-start ICP.

ICP is local; `multistart.start_poses` guesses initial poses on a one-parameter grid.  This module needs no guess: FPFH descriptors
(Rusu, Blodow, Beetz 2009) of both resident clouds, nearest-neighbour matching in feature space and RANSAC over three-point hypotheses
give the `n_best` best-supported rigid poses, and `Context.run_multistart` refines all of them in one call and scores the results.
Both clouds need normals; the refinement needs what multi-start ICP needs (k-NN matching on the LBVH backend, a linear metric).
"""
import numpy as np


def align(ctx, max_stats=512, **options):
    """register_global with **options (Context.set_global_options' keywords; none given: the context's current options), then
    run_multistart from the returned poses with the context's params.  Returns (pose, results, records, best): the refined pose of the
    best start (4 x 4 float32), run_multistart's per-start results, the RANSAC records of the starts (binding.GLOBAL_HYPOTHESIS_DTYPE,
    best first) and the index of the best start.  Raises binding.IcpError(ERR_NO_CORRESPONDENCES) when the clouds give fewer than three
    feature correspondences or no valid hypothesis."""
    if options:
        ctx.set_global_options(**options)
    ctx.push_params()
    poses, records, _ = ctx.register_global()
    results, _, best = ctx.run_multistart(poses, max_stats=max_stats)
    return np.asarray(results[best]["pose"], np.float32), results, records, best
