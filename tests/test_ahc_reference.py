"""CPU: the float64 restatement of the clustering contract (tests/ahc_reference.py) against SciPy: on tie-free metric
data the clusters formed step by step -- and with them the partition at every height -- are
scipy.cluster.hierarchy.linkage's, the heights within 1e-12."""
import numpy as np
import pytest

import ahc_reference as R


@pytest.mark.parametrize("method", ("average", "complete", "single"))
@pytest.mark.parametrize("n,dim,seed", ((2, 3, 0), (17, 5, 1), (120, 8, 2), (250, 16, 3)))
def test_float64_restatement_is_scipys_linkage(method, n, dim, seed):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist, squareform
    x = np.random.RandomState(50 + seed).randn(n, dim)
    y = pdist(x)
    assert len(np.unique(y)) == len(y)                             # tie-free
    d = squareform(y)
    np.fill_diagonal(d, np.inf)
    ref = R.linkage_f64(d, method)
    Z = linkage(y, method)
    assert (np.diff(ref["height"]) >= 0).all()                     # monotone: the step order is the height order
    assert R.merged_sets(ref["pair"], n) == R.merged_sets_scipy(Z, n)
    np.testing.assert_array_equal(ref["size"], Z[:, 3].astype(np.int32))
    assert np.abs(ref["height"] - Z[:, 2]).max() <= 1e-12
    # slots: a cluster lives in its lowest member
    for (a, b), members in zip(ref["pair"].tolist(), R.merged_sets(ref["pair"], n)):
        assert a < b and a == min(members)


def test_cut_restatement_matches_fcluster():
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import pdist, squareform
    x = np.random.RandomState(60).randn(80, 6)
    y = pdist(x)
    d = squareform(y)
    np.fill_diagonal(d, np.inf)
    ref = R.linkage_f64(d, "average")
    Z = linkage(y, "average")
    for t in (0.5, 1.5, 2.5, 10.0):
        labels, found = R.cut(ref, 80, threshold=t)
        want = R.first_appearance(fcluster(Z, np.float32(t), criterion="distance"))
        assert labels.tolist() == want.tolist() and found == want.max() + 1
    for c in (1, 2, 7, 80):
        labels, found = R.cut(ref, 80, n_clusters=c)
        assert found == c and labels.tolist() == R.first_appearance(fcluster(Z, c, criterion="maxclust")).tolist()
