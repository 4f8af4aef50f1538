"""No GPU: the widths the wide whitened semiparametric likelihood and the narrow one refuse in Python, and the missing
whitening matrix, before a context exists."""
import numpy as np
import pytest

import elfi_amd


@pytest.mark.parametrize('m', [64, 257])
def test_wide_call_names_its_range(m):
    with pytest.raises(ValueError, match=r'^%d summaries: the wide whitened semiparametric device kernel takes 65 to 256$' % m):
        elfi_amd.wide_wsemi_loglik(np.zeros((4, m)), np.zeros(m), np.eye(m))


def test_a_missing_whitening_matrix_is_named():
    X, y = np.zeros((4, 65)), np.zeros(65)
    with pytest.raises(ValueError, match='needs a whitening matrix'):
        elfi_amd.wide_wsemi_loglik(X, y, None)
    with pytest.raises(ValueError, match='needs a whitening matrix'):
        elfi_amd.wide_whitened_semiparametric_likelihood(None)
    with pytest.raises(ValueError, match='needs whitening='):
        elfi_amd.wide_wsemi_param_kernel_estimate(X, y)


def test_narrow_call_keeps_its_message():
    with pytest.raises(ValueError, match=r'^65 summaries: the device kernel takes 1 to 64$'):
        elfi_amd.wsemi_loglik(np.zeros((4, 65)), np.zeros(65), np.eye(65))
