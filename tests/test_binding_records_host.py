"""binding's record marshalling and its count-then-fill getters, on the host: no GPU, no library call.

Every record struct is filled with distinct values and turned into a dict; the expected dict is written out from the expressions the
getters used before they shared one function (key order, the Python type of every value, dtype and shape of arrays, values).  All values
are exact in fp32.  The count-then-fill helper runs against a fake C function that reports a count, then fills."""
import ctypes as C
import numpy as np
import pytest
from icp_amd import binding as B

POSE_C = [float(k) + 0.5 for k in range(16)]                                    # column-major, as the library writes it
POSE = np.array(POSE_C, np.float32).reshape(4, 4).T                             # pose_from_c: (row, col)


def filled(cls, **values):
    s = cls()
    for k, v in values.items():
        if isinstance(v, list):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def same_record(got, want):
    assert list(got) == list(want)                                              # keys and their order
    for k, w in want.items():
        g = got[k]
        assert type(g) is type(w), k
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k
            assert g.flags["C_CONTIGUOUS"] and g.flags["OWNDATA"], k
        else:
            assert g == w, k


CASES = [
    (B.IcpIterStats, dict(n_src=1000, n_valid=900, pose=POSE_C, rmse=0.25, benchmark_error=0.125, status=8),
     dict(n_src=1000, n_valid=900, pose=POSE, rmse=0.25, benchmark_error=0.125, status=8)),
    (B.IcpStartResult, dict(pose=POSE_C, status=3, n_inliers=77, fitness=0.75, inlier_rmse=0.0625),
     dict(pose=POSE, status=3, n_inliers=77, fitness=0.75, inlier_rmse=0.0625)),
    (B.IcpTrackFrame, dict(n_src=4800, iterations=35, status=4, initial_rmse=0.5, final_rmse=0.03125, pose=POSE_C),
     dict(n_src=4800, iterations=35, status=4, initial_rmse=0.5, final_rmse=0.03125, pose=POSE)),
    (B.IcpLmSummary, dict(iterations=10, successful_steps=7, unsuccessful_steps=2, invalid_steps=1, termination=1, n_residual_blocks=1234,
                          accepted_steps_mask=0xFFFFFF7F, invalid_steps_mask=0x80000000, initial_cost=1.5e300, final_cost=2.5e-300,
                          trust_region_radius=1e4, x=[0.1, -0.2, 0.3, -0.4, 0.5, -0.6]),
     dict(iterations=10, successful_steps=7, unsuccessful_steps=2, invalid_steps=1, termination=1, n_residual_blocks=1234,
          accepted_steps_mask=0xFFFFFF7F, invalid_steps_mask=0x80000000, initial_cost=1.5e300, final_cost=2.5e-300,
          trust_region_radius=1e4, x=np.array([0.1, -0.2, 0.3, -0.4, 0.5, -0.6], np.float64))),
    (B.IcpRobustStats, dict(n_entering=500, n_kept=400, trim_d2=0.015625, sigma=0.0078125),
     dict(n_entering=500, n_kept=400, trim_d2=0.015625, sigma=0.0078125)),
    (B.IcpReciprocalStats, dict(n_matched=321, n_mutual=123), dict(n_matched=321, n_mutual=123)),
    (B.IcpTiming, dict(match_ms=1.1, weight_reject_build_ms=2.2, solve_ms=3.3, total_ms=6.6, iterations=20, sampled_iterations=5),
     dict(match_ms=1.1, weight_reject_build_ms=2.2, solve_ms=3.3, total_ms=6.6, iterations=20, sampled_iterations=5)),
    (B.IcpConvergenceResult, dict(converged=1, iterations_run=6, iterations_planned=20, rotation=0.0009765625, translation=0.001953125),
     dict(converged=True, iterations_run=6, iterations_planned=20, rotation=0.0009765625, translation=0.001953125)),
    (B.IcpConvergenceResult, dict(converged=0, iterations_run=20, iterations_planned=20, rotation=-1.0, translation=-1.0),
     dict(converged=False, iterations_run=20, iterations_planned=20, rotation=-1.0, translation=-1.0)),
]


@pytest.mark.parametrize("cls,values,want", CASES, ids=[c[0].__name__ + ("_off" if i == 8 else "") for i, c in enumerate(CASES)])
def test_record_dict(cls, values, want):
    same_record(B._record(filled(cls, **values)), want)
    arr = (cls * 3)()                                                           # as an element of a ctypes array, which is how run reads them
    arr[1] = filled(cls, **values)
    same_record(B._record(arr[1]), want)


class FakeGetter:
    """A C getter in Python: (h, *lead, out..., capacity, &n).  With capacity 0 it reports `count`; else it fills `count` entries."""

    def __init__(self, count, n_lead, n_out):
        self.count, self.n_lead, self.n_out, self.calls = count, n_lead, n_out, []

    def __call__(self, h, *args):
        lead, outs, cap, n = args[:self.n_lead], args[self.n_lead:self.n_lead + self.n_out], args[-2], args[-1]
        assert len(args) == self.n_lead + self.n_out + 2
        self.calls.append((h, tuple(a.value for a in lead), tuple(o is not None for o in outs), cap.value))
        n._obj.value = self.count
        for j, o in enumerate(outs):
            if o is not None and cap.value:
                if isinstance(o, C.Array):                                      # record structs
                    for i in range(cap.value):
                        o[i].n_matched, o[i].n_mutual = 10 * i + j, i
                else:                                                           # a c_void_p onto 4-byte entries
                    for i in range(cap.value * self.width[j]):
                        C.cast(o, C.POINTER(C.c_int32))[i] = 100 * j + i
        return B.ICP_OK


def bare_context():
    ctx = B.Context.__new__(B.Context)                                          # no icp_ctx_create: the helper only passes the handle on
    ctx.h = None
    return ctx


@pytest.mark.parametrize("count", [0, 1, 5])
def test_counted_one_array(count):
    ctx = bare_context()
    fake = FakeGetter(count, n_lead=1, n_out=1); fake.width = [3]
    out = ctx._counted(fake, (C.c_int32(7),), lambda n: np.full((n, 3), -1, np.int32))
    assert fake.calls == [(None, (7,), (False,), 0), (None, (7,), (True,), count)]
    assert out.shape == (count, 3) and out.dtype == np.int32
    assert np.array_equal(out.ravel(), np.arange(3 * count))


@pytest.mark.parametrize("count", [0, 4])
def test_counted_two_arrays(count):
    ctx = bare_context()
    fake = FakeGetter(count, n_lead=1, n_out=2); fake.width = [2, 1]
    a, b = ctx._counted(fake, (C.c_int32(1),), lambda n: (np.full((n, 2), -1, np.int32), np.full(n, -1, np.int32)), n_out=2)
    assert fake.calls == [(None, (1,), (False, False), 0), (None, (1,), (True, True), count)]
    assert a.shape == (count, 2) and b.shape == (count,)
    assert np.array_equal(a.ravel(), np.arange(2 * count)) and np.array_equal(b, 100 + np.arange(count))


@pytest.mark.parametrize("count", [0, 3])
def test_counted_records(count):
    ctx = bare_context()
    fake = FakeGetter(count, n_lead=0, n_out=1)
    recs = ctx._records(fake, B.IcpReciprocalStats)
    assert fake.calls == [(None, (), (False,), 0), (None, (), (True,), count)]
    assert recs == [dict(n_matched=10 * i, n_mutual=i) for i in range(count)]
    assert all(list(r) == ["n_matched", "n_mutual"] for r in recs)


def test_counted_raises_on_the_counting_call():
    ctx = bare_context()
    made = []

    class Lib:
        @staticmethod
        def icp_last_error(h):
            return b"nothing resident"
    ctx.lib = Lib

    with pytest.raises(B.IcpError, match="nothing resident") as e:
        ctx._counted(lambda h, *a: 3, (), lambda n: made.append(n))
    assert e.value.code == 3 and made == []                                     # no allocation, no filling call after a failed count
