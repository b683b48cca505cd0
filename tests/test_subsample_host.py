"""CPU-only: the ``subsample=`` keyword of SparseVICoreset / BatchPSVICoreset (constructor validation, the default objects
unchanged), when the sub-sampled enqueued loop is offered and how it draws its index table -- with NumPy stand-ins for the
device projector and sampler in the style of tests/test_sparsevi_host_logic.py."""
import numpy as np
import pytest

import bayesiancoresets_amd as bc
from bayesiancoresets_amd.projector import DeviceProjector
from models import linreg_log_likelihood, make_linreg_data
from test_sparsevi_host_logic import NumpyFusedProjector


class RowsProjector(NumpyFusedProjector):
    """The stand-in with the ``rows=`` forms: positions into the standing data set, NumPy inside."""
    _world, group, family = 1, None, "linreg"

    def colsum_and_core(self, pts, core, persistent=True, rows=None):
        return super().colsum_and_core(pts if rows is None else pts[rows], core)

    def project_select(self, pts, resid, row_ids=None, rows=None):
        return super().project_select(pts if rows is None else pts[rows], resid)


class Sampler(object):
    def __init__(self, answer="plan"):
        self.answer, self.calls = answer, []

    def __call__(self, n, wts, pts):
        return np.zeros((n, 4))

    def enqueue_plan(self, n, pts, steps):
        self.calls.append(("fixed", n, steps))
        return self.answer

    def enqueue_plan_moving(self, n, k, d, steps):
        self.calls.append(("moving", n, k, d, steps))
        return self.answer


Z = make_linreg_data(3, 500, 4)


def svi(sampler, k=2, **kw):
    a = bc.SparseVICoreset(Z, RowsProjector(sampler, 8, 1.0), **kw)
    a.wts, a.idcs, a.pts = np.ones(k), np.arange(k), Z[:k]
    return a


def psvi(sampler, k=2, **kw):
    a = bc.BatchPSVICoreset(Z, RowsProjector(sampler, 8, 1.0), **kw)
    a.wts, a.pts = np.ones(k), Z[:k].copy()
    return a


def test_constructor_validation():
    prj = RowsProjector(Sampler(), 8, 1.0)
    bbp = bc.BlackBoxProjector(Sampler(), 8, lambda z, th: linreg_log_likelihood(z, th, 1.0))
    for cls, kw in ((bc.SparseVICoreset, {}), (bc.BatchPSVICoreset, {"opt_itrs": 3})):
        assert cls(Z, prj, **kw).subsample == "host"                          # the default
        assert cls(Z, prj, subsample="device", **kw).subsample == "device"
        with pytest.raises(ValueError):
            cls(Z, prj, subsample="gpu", **kw)
        with pytest.raises(TypeError):
            cls(Z, prj, *([None] * 6), "device")                             # keyword-only
    with pytest.raises(ValueError):
        bc.SparseVICoreset(Z, bbp, subsample="device")                        # needs a DeviceProjector
    assert bc.SparseVICoreset(Z, bbp).subsample == "host"
    with pytest.raises(ValueError):
        bc.SparseVICoreset(Z, prj, subsample="device", group=object())       # one rank only
    grouped = RowsProjector(Sampler(), 8, 1.0)
    grouped.group = object()
    with pytest.raises(ValueError):
        bc.BatchPSVICoreset(Z, grouped, 3, subsample="device")


def test_default_objects_keep_their_enqueue_plan():
    """``_enqueue_plan()`` as before: offered on the full data set, None with ``n_subsample_opt`` -- whatever ``subsample`` says;
    and the new method offers nothing to a default object."""
    for make in (svi, psvi):
        assert make(Sampler(), opt_itrs=5)._enqueue_plan() == "plan"
        assert make(Sampler(), opt_itrs=5, n_subsample_opt=100)._enqueue_plan() is None
        assert make(Sampler(), opt_itrs=5, n_subsample_opt=100, subsample="device")._enqueue_plan() is None
        assert make(Sampler(), opt_itrs=5, subsample="device")._enqueue_plan() == "plan"
        s = Sampler()
        assert make(s, opt_itrs=5, n_subsample_opt=100)._enqueue_plan_subsampled() is None and s.calls == []


def test_subsampled_plan_is_offered_only_under_its_conditions():
    for make, kind in ((svi, "fixed"), (psvi, "moving")):
        s = Sampler()
        a = make(s, opt_itrs=5, n_subsample_opt=100, subsample="device")
        assert a._enqueue_plan_subsampled() == "plan" and [c[0] for c in s.calls] == [kind] and s.calls[0][-1] == 5
        n = len(s.calls)
        assert make(Sampler(None), opt_itrs=5, n_subsample_opt=100, subsample="device")._enqueue_plan_subsampled() is None
        assert make(lambda n_, w, p: np.zeros((n_, 4)), opt_itrs=5, n_subsample_opt=100,
                    subsample="device")._enqueue_plan_subsampled() is None                     # callback sampler: host loop
        for kw in ({"opt_itrs": 5, "subsample": "device"},                                     # the full data set: _enqueue_plan's case
                   {"opt_itrs": 0, "n_subsample_opt": 100, "subsample": "device"},
                   {"opt_itrs": 5, "n_subsample_opt": 100, "subsample": "device", "k": 0},
                   {"opt_itrs": 5, "n_subsample_opt": 100, "subsample": "device", "k": 4097}):
            assert make(s, **kw)._enqueue_plan_subsampled() is None
        off = make(s, opt_itrs=5, n_subsample_opt=100, subsample="device")
        off.ENQUEUE = False
        assert off._enqueue_plan_subsampled() is None
        small = make(s, opt_itrs=5, n_subsample_opt=100, subsample="device")
        small.INDEX_BUDGET = 8 * 5 * 100 - 1                                                   # the table is 8 * 5 * 100 bytes
        assert small._enqueue_plan_subsampled() is None
        small.INDEX_BUDGET = 8 * 5 * 100
        assert small._enqueue_plan_subsampled() == "plan"
        assert len(s.calls) == n + 1                                                           # only the last one asked the sampler


class FakeTorchTensor(object):
    def __init__(self, a):
        self.a = np.array(a, dtype=np.float64)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_enqueued_loop_draws_one_index_array_per_step(monkeypatch):
    """The sub-sampled enqueued SparseVI loop makes ``opt_itrs`` separate ``randint(n, size=n_sub)`` calls before its first step and
    hands the projector the table they make, the steps are ``run(0) .. run(T - 1)`` and the ADAM entry gets scaling = N / n_sub."""
    T, n_sub, k = 4, 50, 2
    rec = {"randint": [], "run": [], "adam": [], "order": []}
    real = np.random.randint

    def randint(*a, **kw):
        rec["randint"].append((a, kw))
        rec["order"].append("randint")
        return real(*a, **kw)
    monkeypatch.setattr(np.random, "randint", randint)

    class Lib(object):
        def bcx_sparsevi_adam_scratch_bytes(self, k_, S):
            return 0

        def bcx_sparsevi_adam_step_ws(self, *args):
            rec["adam"].append((args[4], args[11]))
            return 0

    class Torch(object):
        float64 = "f64"

        @staticmethod
        def from_numpy(a):
            class T_(object):
                def to(self, dev):
                    return Buf(a)
            return T_()

        @staticmethod
        def empty(n, dtype=None, device=None):
            return Buf(np.zeros(n))

    class Buf(object):
        def __init__(self, a):
            self.a = a

        def __getitem__(self, s):
            return Buf(self.a[s])

        def data_ptr(self):
            return 0

        def numel(self):
            return self.a.size

        def cpu(self):
            return FakeTorchTensor(self.a)

    class Prj(RowsProjector):
        _torch, _lib, device = Torch, Lib(), "dev"

        def _stream(self):
            return 0

        def _check(self, rc):
            assert rc == 0

        def enqueue_step_plan(self, pts, core, persistent, draws, mean, rows=None):
            rec["table"], rec["persistent"] = np.array(rows), persistent

            def run(i):
                rec["run"].append(i)
                rec["order"].append("run")
            return run, Buf(np.zeros(8 * (k + 1))), k

    class Plan(object):
        def buffers(self):
            return None, None

        def draw(self, w, i):
            rec["order"].append("draw")

    a = bc.SparseVICoreset(Z, Prj(Sampler(), 8, 1.0), opt_itrs=T, n_subsample_opt=n_sub, subsample="device")
    a.wts, a.idcs, a.pts = np.ones(k), np.arange(k), Z[:k]
    np.random.seed(5)
    out = a._optimize_enqueued(Plan(), n_sub=n_sub)
    assert out.shape == (k,)
    assert rec["randint"] == [((Z.shape[0],), {"size": n_sub})] * T                 # T separate calls, the host loop's own
    np.random.seed(5)
    want = np.stack([real(Z.shape[0], size=n_sub) for _ in range(T)])
    assert np.array_equal(rec["table"], want) and rec["persistent"] is False
    assert rec["run"] == list(range(T)) and rec["adam"] == [(Z.shape[0] / n_sub, i) for i in range(T)]
    assert rec["order"][:T] == ["randint"] * T and "randint" not in rec["order"][T:]


def test_host_loop_device_mode_is_the_default_path_with_rows(monkeypatch):
    """SparseVI's host loop with ``subsample="device"``: the same randint calls in the same places as the default path, the
    same coreset (the stand-in's ``rows=`` IS ``data[rows]``), NumPy's stream left in the same state."""
    from models import linreg_sampler
    res = {}
    for mode in ("host", "device"):
        np.random.seed(11)
        prj = RowsProjector(linreg_sampler(np.zeros(4), np.eye(4), 1.0), 16, 1.0)
        alg = bc.SparseVICoreset(Z, prj, n_subsample_select=60, n_subsample_opt=40, opt_itrs=5, subsample=mode)
        alg.build(3)
        res[mode] = (alg.idcs.copy(), alg.wts.copy(), alg.pts.copy(), np.random.get_state())
    for a, b in zip(res["host"][:3], res["device"][:3]):
        assert np.array_equal(a, b)
    sa, sb = res["host"][3], res["device"][3]
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert res["host"][0].size >= 1


def test_device_projector_is_the_base_of_the_stand_in():
    assert issubclass(RowsProjector, DeviceProjector)
