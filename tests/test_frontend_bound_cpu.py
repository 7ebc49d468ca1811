"""The reference of the PCA tests, checked before the kernel is held to it: oracle.pca_project (separate multiply and add, index
order) meets the derived bound of tests/frontend_cases.py at the five shapes of tests/test_gpu_frontend_shapes.py.  With whitening the
bound is taken on the projection itself (the whitened matrix, no normalisation): the division by the norm is not part of the sum."""
import numpy as np
import pytest

import frontend_cases as fc


@pytest.mark.parametrize("nc,ss,n,whiten", fc.PCA_SHAPES)
def test_oracle_projection_meets_the_derived_bound(oracle, nc, ss, n, whiten):
    Vt, mu, eig, X = fc.pca_case(nc, ss, n, whiten)
    Vw = oracle.pca_whiten(Vt, eig) if whiten else Vt
    yhat, bound = fc.pca_exact_and_bound(Vw, mu, X)
    Y = np.stack([oracle.pca_project(Vw, mu, x, False) for x in X])
    err = np.abs(Y.astype(np.longdouble) - yhat)
    print(f"oracle PCA nc={nc} ss={ss}: max err / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
    assert np.all(err <= bound), float(np.max(err - bound))
    assert np.all(Y[1] == 0.0) and np.all(bound[1] == 0.0)  # x = mu: every term is an exact zero


def test_bound_is_not_vacuous():
    """a result that is off by one part in 2^42 of the sum of magnitudes -- far inside the flat 1e-12 -- fails the bound"""
    nc, ss, n, whiten = fc.PCA_SHAPES[0]
    Vt, mu, eig, X = fc.pca_case(nc, ss, n, whiten)
    yhat, bound = fc.pca_exact_and_bound(Vt, mu, X)
    S = bound / (np.longdouble(ss + 2) * np.longdouble(2.0) ** -53)
    off = (yhat + S * np.longdouble(2.0) ** -42).astype(np.float64)
    assert float(np.max(np.abs(off - yhat.astype(np.float64)))) < 1e-12
    assert not np.all(np.abs(off.astype(np.longdouble) - yhat) <= bound)
    assert np.finfo(np.longdouble).nmant >= 63  # (the bound's own arithmetic needs the 64-bit significand)
