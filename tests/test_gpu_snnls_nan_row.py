"""GPU: the solver classes refuse rows that hold a NaN.  Such a row has no norm, and finalize rejects the rows as it rejects a
zero row, before any shadow of them is built: no stored NaN row can reach the screening tiers (csrc/screen8.hip,
csrc/screen4.hip) through these classes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("alg", ("FrankWolfe", "OrthoPursuit", "GIGA"))
def test_a_row_with_a_nan_is_refused_by_the_constructor(alg):
    import bayesiancoresets_amd as bc
    X = np.random.RandomState(46).randn(6001, 100)
    X[1234, 7] = np.nan
    with pytest.raises(ValueError):
        getattr(bc.snnls, alg)(X.T, np.nansum(X, axis=0), dtype="float32")
