"""No GPU: the widths the wide semiparametric likelihood and the narrow one refuse in Python, before a context exists."""
import numpy as np
import pytest

import elfi_amd


@pytest.mark.parametrize('m', [64, 257])
def test_wide_call_names_its_range(m):
    with pytest.raises(ValueError, match=r'^%d summaries: the wide semiparametric device kernel takes 65 to 256$' % m):
        elfi_amd.wide_semi_loglik(np.zeros((4, m)), np.zeros(m))


def test_narrow_call_keeps_its_message():
    with pytest.raises(ValueError, match=r'^65 summaries: the device kernel takes 1 to 64$'):
        elfi_amd.semi_loglik(np.zeros((4, 65)), np.zeros(65))
