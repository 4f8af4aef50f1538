"""Host side of the graphical-lasso calls (elfi_amd/synlik.py): bad arguments are refused before the device is touched,
and the keyword shrinkage='glasso' of the older calls still raises (routing it is a follow-up)."""
import numpy as np
import pytest

import elfi_amd

S3 = np.eye(3)
X, Y = np.zeros((8, 3)), np.zeros(3)


@pytest.mark.parametrize('call', [
    lambda: elfi_amd.graphical_lasso(np.eye(65), 0.1),                       # m = 65
    lambda: elfi_amd.graphical_lasso(S3, -0.1),                              # negative alpha
    lambda: elfi_amd.graphical_lasso(S3, [0.1, -0.1]),
    lambda: elfi_amd.graphical_lasso(np.zeros((3, 4)), 0.1),                 # not square
    lambda: elfi_amd.graphical_lasso(S3, 0.1, tol=0.0),
    lambda: elfi_amd.graphical_lasso(S3, 0.1, max_iter=0),
    lambda: elfi_amd.glasso_loglik(X, Y, penalty=0.1, penalties=[0.1]),      # both
    lambda: elfi_amd.glasso_loglik(X, Y),                                    # neither
    lambda: elfi_amd.glasso_loglik(np.zeros((8, 65)), np.zeros(65), penalty=0.1),
    lambda: elfi_amd.glasso_loglik(X, Y, penalty=-1.0),
    lambda: elfi_amd.glasso_loglik(X, Y, penalty=0.1, tol=-1e-9),
    lambda: elfi_amd.glasso_loglik(X, Y, penalty=0.1, max_iter=0),
    lambda: elfi_amd.glasso_likelihood(-0.5),
])
def test_bad_arguments_raise_value_error(call):
    with pytest.raises(ValueError):
        call()


def test_the_shrinkage_keyword_still_raises():
    with pytest.raises(NotImplementedError):
        elfi_amd.syn_loglik(X, Y, shrinkage='glasso', penalty=0.1)
