"""CPU-only: the host side of tests/test_gpu_front4_exact.py (tests/front4_restatement.py) on the model's own shadows.  Every
precondition of every case holds at every shape of the GPU test, the undecided band between the two tightness predicates stays
within its cap, and the list predicate rejects the three lists a wrong front pass would give."""
import numpy as np
import pytest

from tests import front4_restatement as fr
from tools import screen4_model as m4


@pytest.mark.parametrize("storage", fr.STORAGES)
@pytest.mark.parametrize("d", fr.D_LIST)
def test_preconditions_and_band_at_every_shape(d, storage):
    for k, n in enumerate(fr.row_counts(d)):
        X, info = fr.list_rows(d, n, 100 * d + k)
        model = fr.Model.from_host(X, storage)
        probes = dict(fr.build_probes(model, info))            # asserts the preconditions and the band cap
        lists = {}
        for name, o in probes.items():
            counts, lst = fr.model_list(model, o)
            listed = fr.check_list(model, o, counts, lst)       # the model's own list passes
            fr.check_duplicates(info, listed)
            lists[name] = (counts, lst)
            if o.same_as:
                assert np.array_equal(counts, lists[o.same_as][0]) and np.array_equal(lst, lists[o.same_as][1])
        tights = [o.tight for o in probes.values() if hasattr(o, "tight")]
        assert len(tights) >= 4 and min(tights) >= 0.95


def test_preconditions_and_band_at_the_multi_trip_shape():
    """d = 4096, three trips per workgroup.  (The d = 16 shape, 2 099 201 rows, costs as much host time again; its preconditions
    are asserted by the GPU test before it probes.)"""
    d = 4096
    X, info = fr.list_rows(d, fr.multi_trip_rows(d), 3 * d)
    model = fr.Model.from_host(X, "float32")
    for name, o in fr.multi_trip_probes(model):
        fr.check_list(model, o, *fr.model_list(model, o))


def test_err_coef_is_the_models_at_the_flagship_length():
    assert fr.err_coef(512, "float32") == float(np.float32(m4.err_coef_f32(512)))


def test_pack_and_unpack_are_inverse():
    rs = np.random.RandomState(0)
    for d in (1, 31, 33, 100):
        codes = rs.randint(-7, 8, size=(6, d)).astype(np.int8)
        back, pad = fr.unpack4(m4.pack4(codes), d)
        assert np.array_equal(back, codes) and (pad == 8).all() and pad.shape[1] == (d + 31) // 32 * 32 - d


@pytest.mark.parametrize("d", (40, 512))
def test_the_list_predicate_rejects_wrong_lists(d):
    n = fr.row_counts(d)[2]
    X, info = fr.list_rows(d, n, 7)
    model = fr.Model.from_host(X, "float32")
    probes = dict(fr.build_probes(model, info))
    o = probes["aligned_randn/0"]
    counts, lst = fr.model_list(model, o)
    lst = np.concatenate([lst, np.full((lst.shape[0], 2), -1, dtype=np.int32)], axis=1)
    fr.check_list(model, o, counts, lst)
    # the adversarial row removed: soundness
    b = int(model.bins[0])
    c2, l2 = counts.copy(), lst.copy()
    assert l2[b, 0] == 0
    l2[b, :-1] = l2[b, 1:]
    c2[b] -= 1
    with pytest.raises(AssertionError, match="soundness"):
        fr.check_list(model, o, c2, l2)
    # one clamped copy of row n - 1 appended to its segment: structure
    b = int(model.bins[n - 1])
    c2, l2 = counts.copy(), lst.copy()
    assert l2[b, c2[b] - 1] == n - 1
    l2[b, c2[b]] = n - 1
    c2[b] += 1
    with pytest.raises(AssertionError, match="order|count"):
        fr.check_list(model, o, c2, l2)
    # one segment out of order
    b = int(np.flatnonzero(counts >= 2)[0])
    l2 = lst.copy()
    l2[b, [0, 1]] = l2[b, [1, 0]]
    with pytest.raises(AssertionError, match="order"):
        fr.check_list(model, o, counts, l2)
    # a front pass whose eA is 10 % short does not list the target; one whose eA is twice too wide lists rows the formula excludes
    short = fr.score(model, o.q, o.sentinels, eA_factor=0.9)
    with pytest.raises(AssertionError, match="soundness"):
        fr.check_list(model, o, *fr.model_list(model, short))
    r = probes["random0/random64"]
    wide = fr.score(model, r.q, r.sentinels, eA_factor=2.0)
    with pytest.raises(AssertionError, match="tightness"):
        fr.check_list(model, r, *fr.model_list(model, wide))
